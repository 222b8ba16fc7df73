"""-m gpu: the PEM form of the ingestion pipeline (ctmr_submit_pem / ctmr_wait_pem, include/ctmr.h).  PEM
files submitted as text without waiting coalesce into super-batches; every file is judged alone, its issuer index expanded
to its certificates on the device, and each ticket answers as one synchronous pem_decode_each + map_batch over its good
files would, in submission order.  The corpus is synth.host_batch written as files with pem_text.write; the yardstick is a
second engine that runs the two synchronous calls once per submit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import get_entries as ge, pem_text as pt, synth, _native as N  # noqa: E402
from ct_mapreduce_amd.engine import Batch, RECORD_DTYPE  # noqa: E402
from tests import pem_each_corpus as ec  # noqa: E402

NOW = synth.BASE_TIME
NONE = 2**64 - 1
NO_ISSUER = 0xFFFFFFFF


def make(issuers, profile="reference", **kw):
    kw.setdefault("table_slots", 1 << 16)
    kw.setdefault("pair_slots", 1 << 12)
    e = ctmr.Engine(device=0, **kw)
    e.set_profile(profile)
    e.add_issuers(issuers)
    e.set_filter(b"", False, NOW)
    return e


def sync(ref, files, iss):
    """one synchronous pem_decode_each + map_batch → (BatchResult, file_first, bad)"""
    pay, off, first, info, bad = ref.pem_decode_each(files)
    idx = np.repeat(np.asarray(iss, np.uint32), np.diff(first.astype(np.int64)))
    n = len(off) - 1
    return ref.map_batch(Batch(pay, off, idx, np.zeros(n, np.uint8))), first, bad, info


def same(got, want, where=""):
    res, first, bad, info = want
    assert got.records.tobytes() == res.records.tobytes(), where
    assert (got.new_idx == res.new_idx).all(), where
    for f in ("n", "n_new", "n_dup", "n_host_set", "payload_bytes"):
        assert getattr(got.stats, f) == getattr(res.stats, f), (where, f)
    assert list(got.stats.by_status) == list(res.stats.by_status), where
    assert (got.file_first == first).all() and [b is None for b in got.bad] == [b is None for b in bad], where
    for f in ("files", "certificates", "text_bytes", "payload_bytes", "regular", "irregular", "bad_file"):
        assert getattr(got.info, f) == getattr(info, f), (where, f)


def same_sets(eng, ref):
    assert (eng.issuer_counts() == ref.issuer_counts()).all()
    assert sorted(eng.keys(b"serials::*")) == sorted(ref.keys(b"serials::*"))
    assert eng.total_count() == ref.total_count()


def files_of(batch, cuts, line=64, eol=b"\n"):
    """the certificates of the batch cut into files at `cuts` → (files, one issuer per file: that of its first certificate)"""
    files, iss = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        files.append(pt.write([batch.cert(i) for i in range(a, b)], line, eol))
        iss.append(int(batch.issuer_idx[a]) if b > a else NO_ISSUER)
    return files, iss


def submit(eng, files, iss, pinned, keep):
    if not pinned:
        return eng.submit_pem(files, iss)
    text, fb = pt.join(files)
    buf = eng.pinned_array(len(text) + 5)
    buf[5:] = np.frombuffer(text, np.uint8)
    keep.append(buf)
    return eng.submit_pem((buf, fb + np.uint64(5)), iss)


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("profile", ["reference", "fast"])
def test_tickets_answer_like_synchronous_calls(profile, pinned):
    """one file, many files, one file of many blocks, no file, empty files, only bad files; the generator's duplicates span
    files and submits, so WasUnknown depends on the order"""
    cfg = synth.config(seed=131, n_issuers=6, zipf=1, dup_permille=150, ca_permille=20, expired_permille=20)
    issuers = synth.issuers(cfg)
    eng, ref = make(issuers, profile), make(issuers, profile)
    b = synth.host_batch(cfg, 0, 60)
    groups = [files_of(b, [0, 1]), files_of(b, list(range(1, 21))), files_of(b, [20, 50], 76, b"\r\n"), ([], []), ([b"", b" \n"], [0, 1]),
              ([ec.BAD_MARK, ec.BAD_CHECK], [2, 3]), files_of(b, [50, 55, 55, 60])]
    groups[1][0].insert(4, ec.GOOD_IRREGULAR)      # (no certificate: the map calls it a parse error, in both runs)
    groups[1][1].insert(4, NO_ISSUER)
    keep = []
    tickets = [submit(eng, f, i, pinned, keep) for f, i in groups]
    assert len({t >> 20 for t in tickets}) == 1
    for k, ((f, i), t) in enumerate(zip(groups, tickets)):
        res = eng.wait_pem(t)
        same(res, sync(ref, f, i), k)
        if k == 5:
            assert res.stats.n == 0 and all(x is not None and 0 <= x - (5 if pinned else 0) < len(f[0]) + len(f[1]) for x in res.bad)
    same_sets(eng, ref)
    assert eng.total_count() > 0
    eng.close()
    ref.close()


def test_the_issuer_of_a_file_is_that_of_all_its_certificates():
    cfg = synth.config(seed=132, n_issuers=5, zipf=1, ca_permille=0, expired_permille=0)
    issuers = synth.issuers(cfg)
    eng, ref = make(issuers), make(issuers)
    b = synth.host_batch(cfg, 0, 68)
    files = [b"", pt.write([b.cert(0)]), pt.write([b.cert(1), b.cert(2)]), pt.write([b.cert(i) for i in range(3, 68)]), pt.write([b.cert(0)])]
    iss = [4, 3, NO_ISSUER, 1, 2]                  # the last file: the first one's certificate under another issuer
    res = eng.wait_pem(eng.submit_pem(files, iss))
    assert (res.file_first == [0, 0, 1, 3, 68, 69]).all()
    assert (res.records["issuer_idx"] == np.repeat(np.asarray(iss, np.uint32), [0, 1, 2, 65, 1])).all()
    same(res, sync(ref, files, iss))
    assert res.records["status"][0] == res.records["status"][68] == N.ST_PASS and {0, 68} <= set(res.new_idx.tolist())
    same_sets(eng, ref)
    eng.close()
    ref.close()


def test_a_bad_file_between_good_ones_costs_no_other_ticket_anything():
    cfg = synth.config(seed=133, n_issuers=4, zipf=1, dup_permille=100)
    issuers = synth.issuers(cfg)
    b = synth.host_batch(cfg, 0, 30)
    groups = [files_of(b, [0, 5, 10]), files_of(b, [10, 15, 20]), files_of(b, [20, 25, 30])]
    bad1 = ([groups[1][0][0], ec.BAD_FILES, groups[1][0][1]], [groups[1][1][0], 0, groups[1][1][1]])
    eng, ref, eng2 = make(issuers), make(issuers), make(issuers)
    front = b"#" * 37                              # text that is not part of the submit: offsets count from the pointer given
    text, fb = pt.join(bad1[0])
    buf = np.frombuffer(front + text, np.uint8).copy()
    t = [eng.submit_pem(*groups[0]), eng.submit_pem((buf, fb + np.uint64(37)), bad1[1]), eng.submit_pem(*groups[2])]
    assert len({x >> 20 for x in t}) == 1
    t2 = [eng2.submit_pem(*g) for g in groups]
    got = {k: eng.wait_pem(t[k]) for k in (2, 1, 0)}
    want = [sync(ref, *g) for g in groups]
    for k in (0, 2):
        same(got[k], want[k], k)
        same(eng2.wait_pem(t2[k]), want[k], k)
    w1 = eng2.wait_pem(t2[1])
    assert got[1].records.tobytes() == w1.records.tobytes() and (got[1].new_idx == w1.new_idx).all()
    assert (got[1].file_first == [0, 5, 5, 10]).all() and got[1].bad[0] is None and got[1].bad[2] is None
    assert 37 + int(fb[1]) <= got[1].bad[1] < 37 + int(fb[2]) and got[1].info.bad_file == 1 and got[1].info.bad_offset == got[1].bad[1]
    same_sets(eng, ref)
    same_sets(eng2, ref)
    for e in (eng, eng2, ref):
        e.close()


def test_pem_json_raw_and_packed_submits_interleaved():
    """Every change of form closes the open super-batch and the order of the stream is kept across forms."""
    cfg = synth.config(seed=134, n_issuers=8, zipf=1, dup_permille=300)
    issuers = synth.issuers(cfg)
    eng, ref = make(issuers), make(issuers)
    size, pending, keep, seqs = 40, [], [], []

    def pairs_of(raw):
        return [(raw.leaf_input(i), raw.extra_data(i)) for i in range(raw.n)]

    def collect(form, x, t):
        if form == "packed":
            got, want = eng.wait(t, x.n), ref.map_batch(x)
            assert got.records.tobytes() == want.records.tobytes() and (got.new_idx == want.new_idx).all()
        elif form == "pem":
            same(eng.wait_pem(t), sync(ref, *x), form)
        else:
            got = eng.wait_entries(t, x.n) if form == "raw" else eng.wait_entries_json(t)
            want = ref.map_entries(x)
            assert got.records.tobytes() == want.records.tobytes() and (got.new_idx == want.new_idx).all()

    for k in range(12):
        form = ("pem", "raw", "pem", "packed", "pem", "json")[k % 6]
        a = None
        if form == "packed":
            x = synth.host_batch(cfg, k * size, size)
            a = (np.concatenate([x.payload, np.zeros(32, np.uint8)]), x.offsets.astype(np.uint64), x.issuer_idx.astype(np.uint32),
                 x.entry_type.astype(np.uint8))
            t = eng.submit_batch(a[0], a[1], a[2], a[3], x.n)
        elif form == "raw":
            x = synth.host_entries(cfg, k * size, size)
            a = (np.concatenate([x.blob, np.zeros(32, np.uint8)]), np.ascontiguousarray(x.bounds, np.uint64))
            t = eng.submit_entries(a[0], a[1], x.n)
        elif form == "json":
            x = synth.host_entries(cfg, k * size, size)
            t = eng.submit_entries_json(ge.write(pairs_of(x), 16))
        else:
            x = files_of(synth.host_batch(cfg, k * size, size), list(range(0, size + 1, 8)))
            t = eng.submit_pem(*x)
        keep.append(a)
        seqs.append(t >> 20)
        pending.append((form, x, t))
        if len(pending) == 3:          # at most four super-batches may be unfinished or uncollected
            collect(*pending.pop(0))
    while pending:
        collect(*pending.pop(0))
    assert len(set(seqs)) == 12         # a super-batch each: the forms closed each other's
    same_sets(eng, ref)
    eng.close()
    ref.close()


def test_the_size_query_double_collection_and_the_other_wait_calls():
    cfg = synth.config(seed=135, n_issuers=4)
    issuers = synth.issuers(cfg)
    eng, ref = make(issuers), make(issuers)
    files, iss = files_of(synth.host_batch(cfg, 0, 50), [0, 20, 40, 50])
    t = eng.submit_pem(files, iss)
    lib, h = eng._lib, eng._h
    rec = np.zeros(50, RECORD_DTYPE)
    st = N.BatchStats()
    assert lib.ctmr_wait(h, t, rec.ctypes.data, None, C.byref(st)) == N.E_INVAL           # refused,
    assert lib.ctmr_wait_entries(h, t, rec.ctypes.data, None, None, None, C.byref(st)) == N.E_INVAL
    assert lib.ctmr_wait_entries_json(h, t, 50, rec.ctypes.data, None, None, None, None, None, None, C.byref(st)) == N.E_INVAL
    assert not rec.tobytes().strip(b"\0")
    info = N.PemDecodeInfo()
    want = sync(ref, files, iss)
    for cap in (0, 49):                                                                    # … and still collectable
        rc = lib.ctmr_wait_pem(h, t, cap, rec.ctypes.data, None, None, None, C.byref(info), None)
        assert rc == N.E_RANGE and (info.certificates, info.files, info.bad_file) == (50, 3, NONE)
        assert info.payload_bytes == want[3].payload_bytes and not rec.tobytes().strip(b"\0")
    same(eng.wait_pem(t), want)
    with pytest.raises(ctmr.CtmrError) as ei:
        eng.wait_pem(t)
    assert ei.value.code == N.E_NOTFOUND
    assert lib.ctmr_wait_pem(h, t, 50, None, None, None, None, C.byref(info), None) == N.E_NOTFOUND
    # a JSON ticket is not for ctmr_wait_pem, and stays collectable too; nor is a packed one
    tj = eng.submit_entries_json([b'{"entries":[]}'])
    assert lib.ctmr_wait_pem(h, tj, 50, None, None, None, None, C.byref(info), None) == N.E_INVAL
    assert eng.wait_entries_json(tj).stats.n == 0
    x = synth.host_batch(cfg, 0, 5)
    a = (np.concatenate([x.payload, np.zeros(32, np.uint8)]), x.offsets.astype(np.uint64), x.issuer_idx.astype(np.uint32))
    tp = eng.submit_batch(a[0], a[1], a[2], None, 5)
    assert lib.ctmr_wait_pem(h, tp, 50, None, None, None, None, C.byref(info), None) == N.E_INVAL
    assert eng.wait(tp, 5).stats.n == 5
    # all outputs NULL; arguments
    t = eng.submit_pem([b""], [0])
    assert lib.ctmr_wait_pem(h, t, 0, None, None, None, None, None, None) == 0
    tk = C.c_uint64(0)
    fb = np.asarray([0, 5, 3], np.uint64)
    idx = np.zeros(2, np.uint32)
    assert lib.ctmr_submit_pem(h, fb.ctypes.data, fb.ctypes.data, 2, idx.ctypes.data, C.byref(tk)) == N.E_INVAL      # not monotone
    fb = np.asarray([0, 5], np.uint64)
    assert lib.ctmr_submit_pem(h, None, fb.ctypes.data, 1, idx.ctypes.data, C.byref(tk)) == N.E_INVAL                # bytes, no text
    assert lib.ctmr_submit_pem(h, fb.ctypes.data, fb.ctypes.data, 1, None, C.byref(tk)) == N.E_INVAL                 # no issuers
    eng.close()
    ref.close()


def test_flush_closes_and_super_batches_close_by_file_count():
    cfg = synth.config(seed=136, n_issuers=2)
    issuers = synth.issuers(cfg)
    eng = make(issuers)
    files, iss = files_of(synth.host_batch(cfg, 0, 4), [0, 2, 4])
    t0 = eng.submit_pem(files, iss)
    eng.flush()
    t1 = eng.submit_pem(files, iss)
    assert t0 >> 20 != t1 >> 20
    assert eng.wait_pem(t1).stats.n_new == 0 and eng.wait_pem(t0).stats.n_new == 4      # t0's super-batch ran first
    # 65 536 files close a super-batch: 66 submits of 1 000 empty files, the 67th opens the next
    empty = (np.zeros(1, np.uint8), np.zeros(1001, np.uint64))
    zeros = np.zeros(1000, np.uint32)
    tickets = [eng.submit_pem(empty, zeros) for _ in range(70)]
    seq = [t >> 20 for t in tickets]
    assert len(set(seq[:66])) == 1 and seq[66] != seq[65] and len(set(seq[66:])) == 1
    for t in tickets:
        res = eng.wait_pem(t)
        assert res.stats.n == 0 and res.bad == [None] * 1000 and not res.file_first.any()
    assert eng.total_count() == 4
    eng.close()


def test_a_submit_larger_than_a_slot_gets_its_own():
    cfg = synth.config(seed=137, n_issuers=1)
    issuers = synth.issuers(cfg)
    eng = make(issuers)
    b = synth.host_batch(cfg, 0, 2)
    small = pt.write([b.cert(0)])
    t0 = eng.submit_pem([small], [0])
    unit = np.frombuffer(pt.write([b.cert(1)]), np.uint8)
    reps = (386 << 20) // len(unit) + 1             # over the 384 MB a slot starts with
    big = np.tile(unit, reps)
    fb = np.asarray([0, len(unit) * (reps // 2), len(big)], np.uint64)
    t1 = eng.submit_pem((big, fb), [0, 0])
    assert t0 >> 20 != t1 >> 20
    res = eng.wait_pem(t1)
    assert (res.file_first == [0, reps // 2, reps]).all() and res.bad == [None, None]
    assert (res.stats.n, res.stats.n_new, res.info.irregular) == (reps, 1, 0) and res.new_idx.tolist() == [0]
    assert eng.wait_pem(t0).stats.n_new == 1 and eng.total_count() == 2
    eng.close()
