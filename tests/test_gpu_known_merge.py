"""-m gpu: set algebra on known-certificate images (include/ctmr.h ctmr_known_merge*; kernels/merge.h).

Expected bytes come from the CPU twins known_image.union / minus / intersect (tests/test_known_merge_cpu.py holds them to
Python sets), never from the code under test.  Which path an operand took — used where it lies, or copied and sorted — is
read from the line the library prints under CTMR_KNOWN_MERGE_INFO.  Engines are made the way
tests/test_gpu_known_image.py makes them, the corpora come from tests/known_corpus.py.
"""
import base64
import ctypes as C
import functools
import re
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr
from ct_mapreduce_amd import known_image as KI, synth, _native as N
from ct_mapreduce_amd.distributed import Group, shard_range
from tests import known_corpus as KC
from ct_mapreduce_amd.engine import Batch
from tests.test_gpu_exchange import DEV, dev_shard, to_dev
from tests.test_gpu_known_image import engine, state, add_point_members
from tests.test_gpu_known_sort import shuffled, one_set_image, table
from tests.test_known_merge_cpu import with_host_pairs

CFG = synth.config(seed=97, n_issuers=6, dup_permille=150, ca_permille=20, expired_permille=20)
HOURS = [491000 + k for k in range(11)]
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1025]
OPS = (N.KNOWN_UNION, N.KNOWN_MINUS, N.KNOWN_INTERSECT)
# (a twin's result is computed once per pair of operands, however many variants and buffer sizes are held against it)
TWIN = {N.KNOWN_UNION: functools.lru_cache(64)(KI.union), N.KNOWN_MINUS: functools.lru_cache(64)(KI.minus),
        N.KNOWN_INTERSECT: functools.lru_cache(64)(KI.intersect)}
GUARD = 4 * 48
EMPTY = KI.build({})
INFO = re.compile(rb"ctmr known merge: op=(\d) a=(\w+) b=(\w+)")


@pytest.fixture(scope="module")
def digests():
    issuers = synth.issuers(CFG)
    e = engine(issuers)
    out = [base64.urlsafe_b64decode(e.issuer_id(k)) for k in range(len(issuers))]
    e.close()
    return out


@pytest.fixture(scope="module")
def eng():
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)   # no issuer registered: the merge needs none
    yield e
    e.close()


def make_pairs(mix, digests, seed=7):
    """(A, B) as {key: members}: per set, in turn, one of — in A only, in B only, identical, disjoint, A ⊂ B, B ⊂ A,
    interleaved; set sizes cycle through SIZES, so every size meets partners of one member and of all the others."""
    c = KC.make(mix, digests, HOURS, SIZES, seed=seed)
    a, b = {}, {}
    for k, key in enumerate(sorted(c.sets)):
        ms = [m for m in c.sets[key] if len(m) <= 40]
        case, one = k % 7, (k // 7) % 2 == 0
        if case == 0:
            a[key] = ms
        elif case == 1:
            b[key] = ms
        elif case == 2:
            a[key], b[key] = ms, list(ms)
        elif case == 3:
            cut = 1 if one else len(ms) // 2
            a[key], b[key] = ms[:cut], ms[cut:]
        elif case == 4:
            a[key], b[key] = (ms[len(ms) // 2:][:1] if one else ms[::3]), ms
        elif case == 5:
            a[key], b[key] = ms, (ms[-1:] if one else ms[1::2])
        else:
            a[key], b[key] = ms[::2], ms[1::2]
    return {k: v for k, v in a.items() if v}, {k: v for k, v in b.items() if v}


def with_repeats(img, seed=2):
    """The image with some records of every set written twice or three times (the set entries and counts follow)."""
    meta, rec = KC.split(img)
    _, _, _, n_iss, _, n_sets, n_mem, host_bytes, n_host, _ = KI._HEADER.unpack_from(meta, 0)
    so = 64 + 32 * n_iss
    rng = np.random.default_rng(seed)
    parts, entries, first = [], [], 0
    for s in range(n_sets):
        eh, ordinal, f, cnt = KI._SET.unpack_from(meta, so + 24 * s)
        r = rec[f:f + cnt]
        extra = r[rng.integers(0, cnt, size=min(cnt, 3))]
        both = np.concatenate([r, extra, extra[:1]])
        both = both[rng.permutation(len(both))]
        parts.append(both)
        entries.append(KI._SET.pack(eh, ordinal, first, len(both)))
        first += len(both)
    head = KI._HEADER.pack(KI.MAGIC, KI.VERSION, 64, n_iss, 0, n_sets, first, host_bytes, n_host, 0)
    m2 = head + meta[64:so] + b"".join(entries) + meta[so + 24 * n_sets:]
    return m2 + (np.concatenate(parts).tobytes() if parts else b"")


def merge_host(e, op, a, b, cap=None):
    """ctmr_known_merge with guard bytes round `out` → (rc, info, image or None)."""
    info = N.KnownImageInfo()
    want = len(TWIN[op](a, b)) if cap is None else cap
    buf = np.full(want + 128, 0xEE, np.uint8)
    rc = e._lib.ctmr_known_merge(e._h, op, a, len(a), b, len(b) if b is not None else 0, buf.ctypes.data + 64, want,
                                 C.byref(info))
    assert (buf[:64] == 0xEE).all() and (buf[64 + want:] == 0xEE).all()
    if rc:
        assert (buf == 0xEE).all()
        return rc, info, None
    return rc, info, buf[64:64 + info.image_bytes].tobytes()


def merge_device(e, op, a, b, caps=None):
    """ctmr_known_merge_device with guard records round d_out and guard bytes round out_meta; the operands on the device
    must stay as they were → (rc, info, image or None)."""
    info = N.KnownImageInfo()
    want = TWIN[op](a, b)
    n_want = KI._HEADER.unpack_from(want, 0)[6]
    meta_cap, rec_cap = caps if caps is not None else (len(want) - 48 * n_want, n_want)
    ops = []
    for img in (a, b):
        if img is None:
            ops.append((None, 0, None, 0, None))
            continue
        meta, rec = KC.split(img)
        raw = rec.view(np.uint8).reshape(-1)
        t = torch.from_numpy(np.concatenate([raw, np.zeros(16, np.uint8)])).to(DEV)
        ops.append((meta, len(meta), t, len(rec), raw))
    out = torch.full((rec_cap * 48 + 2 * GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
    mbuf = np.full(meta_cap + 128, 0xEE, np.uint8)
    (am, al, at, an, araw), (bm, bl, bt, bn, braw) = ops
    rc = e._lib.ctmr_known_merge_device(e._h, op, am, al, C.c_void_p(at.data_ptr()) if an else None, an, bm, bl,
                                        C.c_void_p(bt.data_ptr()) if bn else None, bn, mbuf.ctypes.data + 64, meta_cap,
                                        C.c_void_p(out.data_ptr() + GUARD), rec_cap, C.byref(info))
    h = out.cpu().numpy()
    assert (h[:GUARD] == 0xEE).all() and (h[GUARD + rec_cap * 48:] == 0xEE).all()
    assert (mbuf[:64] == 0xEE).all() and (mbuf[64 + meta_cap:] == 0xEE).all()
    for t, n, raw in ((at, an, araw), (bt, bn, braw)):
        if n:
            assert (t.cpu().numpy()[:len(raw)] == raw).all()
    if rc:
        assert (h == 0xEE).all() and (mbuf == 0xEE).all()
        return rc, info, None
    return rc, info, mbuf[64:64 + info.meta_bytes].tobytes() + h[GUARD:GUARD + info.members * 48].tobytes()


def fields(info):
    return tuple(getattr(info, f) for f, _ in N.KnownImageInfo._fields_)


def check(e, op, a, b):
    """Both variants at exact-size buffers against the twin → the image."""
    want = TWIN[op](a, b)
    rc, info, got = merge_host(e, op, a, b)
    assert rc == 0, rc
    if got != want:
        assert len(got) == len(want), (len(got), len(want))
        bad = np.nonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[0]
        raise AssertionError("op %d: %d bytes differ, first at %d of %d" % (op, len(bad), bad[0], len(want)))
    rc, dinfo, dgot = merge_device(e, op, a, b)
    assert rc == 0 and dgot == want and fields(dinfo) == fields(info)
    im = KI.parse(want)
    assert (info.members, info.sets, info.host_members, info.issuers) == (im.n_members, im.n_sets, im.n_host_members,
                                                                         len(im.issuers))
    assert info.image_bytes == len(want) and info.meta_bytes == len(want) - 48 * im.n_members
    return got


def paths_of(capfd, call):
    capfd.readouterr()
    out = call()
    found = INFO.findall(capfd.readouterr().err.encode())
    assert found, "no CTMR_KNOWN_MERGE_INFO line"
    return out, [(int(o), a.decode(), b.decode()) for o, a, b in found]


# ---- 1. every mix, every case of make_pairs, all three ops, both variants

@pytest.mark.parametrize("mix", KC.MIXES)
def test_every_mix_every_case_all_ops(mix, eng, digests):
    a, b = make_pairs(mix, digests)
    ia, ib = KC.image(a), KC.image(b)
    if mix == "uniform":
        assert set(KC.record_lens(ia).tolist()) == set(range(41))
        assert set(SIZES) <= set(np.bincount(KC.record_sets(ia)).tolist()) | set(np.bincount(KC.record_sets(ib)).tolist())
    for op in OPS:
        check(eng, op, ia, ib)
        check(eng, op, ib, ia)
    assert eng.known_merge(N.KNOWN_UNION, ia, ib) == KI.union(ia, ib)
    meta, d = eng.known_merge_device(N.KNOWN_MINUS, *split_dev(ia), *split_dev(ib))
    assert meta + d.cpu().numpy().tobytes() == KI.minus(ia, ib)


def split_dev(img):
    meta, rec = KC.split(img)
    return meta, torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(DEV)


def test_images_of_zero_one_and_two_records_and_no_b(eng, digests):
    key = KI.set_key(HOURS[0], digests[0])
    one, two = KI.build({key: [b"\x01\x02\x03"]}), KI.build({key: [b"\x01\x02\x03", b"\x09"]})
    other = KI.build({KI.set_key(HOURS[1], digests[1]): [b"\x01\x02\x03"]})
    imgs = [EMPTY, one, two, other]
    for op in OPS:
        for a in imgs:
            for b in imgs + [None]:
                check(eng, op, a, b)
    big = KC.make("uniform", digests[:2], HOURS[:2], [300, 7], seed=3).image
    for op in OPS:
        check(eng, op, big, None)
        check(eng, op, EMPTY, big)
    assert check(eng, N.KNOWN_UNION, shuffled(big), None) == big              # UNION with nothing normalises


# ---- 2. operand forms: canonical, shuffled, with repeats — nine combinations, one result; the fast path is taken

def test_operand_forms_and_the_fast_path(eng, digests, capfd, monkeypatch):
    monkeypatch.setenv("CTMR_KNOWN_MERGE_INFO", "1")
    a, b = make_pairs("uniform", digests, seed=9)
    ia, ib = KC.image(a), KC.image(b)
    fa = {"in_place": ia, "shuffled": shuffled(ia, 4), "repeats": with_repeats(ia, 5)}
    fb = {"in_place": ib, "shuffled": shuffled(ib, 6), "repeats": with_repeats(ib, 7)}
    assert KI.parse(fa["repeats"]).sets == KI.parse(ia).sets and len(fa["repeats"]) > len(ia)
    for op in OPS:
        want = TWIN[op](ia, ib)
        for na, xa in fa.items():
            for nb, xb in fb.items():
                got, paths = paths_of(capfd, lambda: eng.known_merge(op, xa, xb))
                assert got == want, (op, na, nb)
                assert paths[-1] == (op, "in_place" if na == "in_place" else "sorted", "in_place" if nb == "in_place" else "sorted")
        _, paths = paths_of(capfd, lambda: check(eng, op, fa["repeats"], fb["shuffled"]))
        assert all(p == (op, "sorted", "sorted") for p in paths)


@pytest.mark.parametrize("chunk", [300, 257])
def test_unsorted_operands_in_forced_small_sort_runs(chunk, eng, digests, monkeypatch):
    a, b = make_pairs("runs", digests, seed=11)
    ia, ib = KC.image(a), KC.image(b)
    monkeypatch.setenv("CTMR_KNOWN_SORT_CHUNK", str(chunk))
    for op in OPS:
        assert eng.known_merge(op, with_repeats(ia), shuffled(ib)) == TWIN[op](ia, ib)


# ---- 3. ties the search must look past its first word for

def test_members_that_agree_in_their_first_octets(eng):
    rng = np.random.default_rng(13)
    for shared in (8, 16, 24, 32, 39):
        head = bytes(rng.integers(0, 256, size=shared, dtype=np.uint8).tolist())
        tails = sorted({bytes(rng.integers(0, 256, size=40 - shared, dtype=np.uint8).tolist()) for _ in range(400)})
        if shared == 39:
            tails = [bytes([v]) for v in range(256)]
        ms = [head + t for t in tails]
        a, b = one_set_image(sorted(ms[::2] + ms[1::5])), one_set_image(sorted(ms[1::2] + ms[::7]))
        for op in OPS:
            check(eng, op, a, b)
        # present in A, absent in B by its last octet only
        m = ms[len(ms) // 2]
        near = m[:-1] + bytes([m[-1] ^ 1])
        rest = [x for x in ms if x not in (m, near)]
        a, b = one_set_image(sorted(rest + [m])), one_set_image(sorted(rest + [near]))
        assert KI.records(check(eng, N.KNOWN_MINUS, a, b))[0] == [(KI.set_key(491000, bytes([7]) * 32), m)]
        assert m not in [x for _, x in KI.records(check(eng, N.KNOWN_INTERSECT, a, b))[0]]
        assert KI.parse(check(eng, N.KNOWN_UNION, a, b)).n_members == len(rest) + 2


def test_members_that_differ_in_length_alone(eng):
    zeros = [b"", b"\x00", b"\x00\x00"]
    for mask_a in range(8):
        for mask_b in range(8):
            a = one_set_image([z for k, z in enumerate(zeros) if mask_a >> k & 1] + [b"\x00\x01", b"\x01"])
            b = one_set_image([z for k, z in enumerate(zeros) if mask_b >> k & 1] + [b"\x00\x01"])
            for op in OPS:
                check(eng, op, a, b)
    ms = [b"\x00" * L for L in range(41)] + [b"\x05" * 9 + b"\x00" * L for L in range(32)]
    a, b = one_set_image(sorted(ms[::2])), one_set_image(sorted(ms[::3]))
    for op in OPS:
        check(eng, op, a, b)


def test_twins_corpus_against_itself_and_its_halves(eng, digests):
    c = KC.make("twins", digests[:3], HOURS[:2], 0, seed=15)
    dev = {k: [m for m in v if len(m) <= 40] for k, v in c.sets.items()}
    a = KC.image({k: v[::2] for k, v in dev.items()})
    b = KC.image({k: v[1::2] + v[::4] for k, v in dev.items()})
    for op in OPS:
        check(eng, op, a, b)
        check(eng, op, c.image, a)                                            # (host-section members above 40 octets too)


# ---- 4. issuers and sets that vanish

def test_sets_and_issuers_that_vanish(eng, digests):
    d = sorted(digests)
    a = {KI.set_key(HOURS[0], d[0]): [b"\x01"], KI.set_key(HOURS[0], d[1]): [b"\x02", b"\x03"],
         KI.set_key(HOURS[1], d[1]): [b"\x04"], KI.set_key(HOURS[0], d[3]): [b"\x05"], KI.set_key(HOURS[2], d[3]): [b"\x06", b"\x07"]}
    b = {KI.set_key(HOURS[0], d[1]): [b"\x03", b"\x02"], KI.set_key(HOURS[1], d[1]): [b"\x04", b"\x09"],
         KI.set_key(HOURS[2], d[3]): [b"\x07", b"\x06"], KI.set_key(HOURS[2], d[5]): [b"\x08"]}
    ia, ib = KI.build(a), KI.build(b)
    out = check(eng, N.KNOWN_MINUS, ia, ib)
    assert KI.parse(out).issuers == [d[0], d[3]] and KI.parse(out).n_sets == 2
    assert KI.parse(ia).issuers != KI.parse(ib).issuers                       # different lists, different ordinals
    for op in OPS:
        check(eng, op, ia, ib)
        check(eng, op, ib, ia)
    dis_a = KC.make("uniform", d[:3], HOURS[:3], [70, 300], seed=17).image
    dis_b = KC.make("uniform", d[3:], HOURS[1:4], [65, 2], seed=18).image
    assert check(eng, N.KNOWN_INTERSECT, dis_a, dis_b) == EMPTY
    assert check(eng, N.KNOWN_MINUS, dis_a, dis_a) == EMPTY


# ---- 5. the host section

def test_host_section_pairs(eng, digests):
    d = sorted(digests)
    key, other = KI.set_key(HOURS[1], d[2]), KI.set_key(HOURS[0], d[4])
    odd = b"serials::2026-01-05::" + KI.issuer_id(d[2])
    sets = {key: [b"\x01\x02", b"\x05" * 20], KI.set_key(HOURS[3], d[0]): [bytes([v]) for v in range(70)]}
    pairs = [(key, b"\x03" * 40), (key, b"\x04" * 41), (key, b"\x05" * 20), (other, b""), (odd, b"\x07\x08")]
    img = with_host_pairs(sets, pairs)
    norm = check(eng, N.KNOWN_UNION, img, None)
    dev, host = KI.records(norm)
    assert (key, b"\x03" * 40) in dev and (other, b"") in dev and dev.count((key, b"\x05" * 20)) == 1
    assert host == sorted([(odd, b"\x07\x08"), (key, b"\x04" * 41)])
    b = with_host_pairs({key: [b"\x03" * 40, b"\x09"]}, [(odd, b"\x07\x08"), (odd, b"\x01"), (key, b"\x04" * 42)])
    got = {}
    for op in OPS:
        got[op] = KI.records(check(eng, op, img, b))
        check(eng, op, b, img)
        check(eng, op, shuffled(img), b)
    assert got[N.KNOWN_UNION][0].count((key, b"\x03" * 40)) == 1              # A's host pair = B's member record: once,
    assert (key, b"\x03" * 40) not in got[N.KNOWN_MINUS][0]                   # dropped,
    assert got[N.KNOWN_INTERSECT] == ([(key, b"\x03" * 40)], [(odd, b"\x07\x08")])   # kept


# ---- 6. sizing and rejections

def test_buffers_one_short_give_range_with_the_same_info(eng, digests):
    a, b = make_pairs("uniform", digests, seed=19)
    ia, ib = KC.image(a), shuffled(KC.image(b))
    for op in OPS:
        want = TWIN[op](ia, ib)
        n = KI._HEADER.unpack_from(want, 0)[6]
        meta_bytes = len(want) - 48 * n
        rc, info, got = merge_host(eng, op, ia, ib)
        assert rc == 0 and got == want
        rc, short, got = merge_host(eng, op, ia, ib, cap=len(want) - 1)
        assert rc == N.E_RANGE and got is None and fields(short) == fields(info)
        rc, dinfo, got = merge_device(eng, op, ia, ib)
        assert rc == 0 and got == want
        for caps in ((meta_bytes - 1, n), (meta_bytes, n - 1)):
            rc, short, got = merge_device(eng, op, ia, ib, caps=caps)
            assert rc == N.E_RANGE and got is None and fields(short) == fields(dinfo) == fields(info)
        # the bounds size without a first call
        assert n <= (KI.parse(ia).n_members + KI.parse(ib).n_members if op == N.KNOWN_UNION else KI.parse(ia).n_members)
        assert meta_bytes <= len(KC.split(ia)[0]) + len(KC.split(ib)[0])


def test_rejected_operands_write_nothing(eng, digests):
    c = KC.make("uniform", digests, HOURS[:2], [300, 301, 299], seed=21)
    img = shuffled(c.image)
    good = KC.make("uniform", digests, HOURS[:2], [200, 3], seed=22).image
    n = c.members
    lens = KC.record_lens(img)
    n_iss = KI._HEADER.unpack_from(img, 0)[3]
    so = 64 + 32 * n_iss

    def damaged(edit):
        meta, rec = KC.split(img)
        edit(rec)
        return meta + rec.tobytes()

    bad = []
    for i in (0, n - 1):
        bad.append(damaged(lambda rec: rec["len"].__setitem__(i, 41)))
        for edge in (8, 16, 24, 32, 39):
            if lens[i] <= edge:
                bad.append(damaged(lambda rec: rec["serial"].__setitem__((i, edge), 1)))
    gap = bytearray(img)
    struct.pack_into("<Q", gap, so + 24 + 8, struct.unpack_from("<Q", img, so + 24 + 8)[0] + 1)
    ordinal = bytearray(img)
    struct.pack_into("<I", ordinal, so + 4, n_iss)
    order = bytearray(img)
    order[so:so + 24], order[so + 24:so + 48] = img[so + 24:so + 48], img[so:so + 24]
    magic = bytearray(img)
    magic[0] ^= 1
    bad += [bytes(gap), bytes(ordinal), bytes(order), bytes(magic)]
    assert len(bad) >= 8
    before = table(eng)
    cap = len(img) + len(good)
    for x in bad:
        with pytest.raises(KI.ImageError):
            KI.parse(x)
        for a, b in ((x, good), (good, x)):
            for op in (N.KNOWN_UNION, N.KNOWN_MINUS):
                rc, _, got = merge_host(eng, op, a, b, cap=cap)
                assert rc == N.E_INVAL and got is None
                rc, _, got = merge_device_raw(eng, op, a, b, cap)
                assert rc == N.E_INVAL and got is None
    for op in (3, -1):
        rc, _, got = merge_host(eng, op, good, good, cap=cap)
        assert rc == N.E_INVAL and got is None
        rc, _, got = merge_device_raw(eng, op, good, good, cap)
        assert rc == N.E_INVAL and got is None
    assert table(eng) == before


def merge_device_raw(e, op, a, b, cap):
    """merge_device for operands no twin accepts: the buffers sized by `cap` bytes."""
    info = N.KnownImageInfo()
    ts = []
    for img in (a, b):
        n_mem = min(KI._HEADER.unpack_from(img, 0)[6], len(img) // 48)
        at = len(img) - 48 * n_mem
        raw = np.frombuffer(img[at:], np.uint8)
        ts.append((bytes(img[:at]), torch.from_numpy(np.concatenate([raw, np.zeros(16, np.uint8)])).to(DEV), n_mem, raw))
    out = torch.full((cap,), 0xEE, dtype=torch.uint8, device=DEV)
    mbuf = np.full(cap, 0xEE, np.uint8)
    rc = e._lib.ctmr_known_merge_device(e._h, op, ts[0][0], len(ts[0][0]), C.c_void_p(ts[0][1].data_ptr()), ts[0][2],
                                        ts[1][0], len(ts[1][0]), C.c_void_p(ts[1][1].data_ptr()), ts[1][2],
                                        mbuf.ctypes.data, cap, C.c_void_p(out.data_ptr()), cap // 48, C.byref(info))
    for _, t, _, raw in ts:
        assert (t.cpu().numpy()[:len(raw)] == raw).all()
    if rc:
        assert (out.cpu().numpy() == 0xEE).all() and (mbuf == 0xEE).all()
    return rc, info, None


# ---- 7. the engine the call borrows, and the table route

def export_sorted(e):
    e.set_known_order(N.KNOWN_ORDER_SORTED)
    out = e.known_export()
    e.set_known_order(N.KNOWN_ORDER_ANY)
    return out


def test_merge_changes_nothing_of_the_engine(digests):
    issuers = synth.issuers(CFG)
    e = engine(issuers, table_slots=1 << 13)
    e.map_batch(synth.host_batch(CFG, 0, 1500))
    add_point_members(e, [e.issuer_id(k) for k in range(len(issuers))])
    before = (state(e), table(e), export_sorted(e), e.issuer_counts().tobytes())
    a, b = make_pairs("uniform", digests + [bytes(range(32))], seed=23)
    ia, ib = KC.image(a), KC.image(b)
    for op in OPS:
        check(e, op, shuffled(ia), ib)
    assert (state(e), table(e), export_sorted(e), e.issuer_counts().tobytes()) == before
    e.close()


def test_against_the_table_route(eng, digests):
    issuers = synth.issuers(CFG)
    a, b = make_pairs("interleaved", digests, seed=25)
    ia, ib = KC.image(a), KC.image(b)
    x = engine(issuers)
    x.known_import(ia)
    x.known_import(ib)
    assert export_sorted(x) == check(eng, N.KNOWN_UNION, ia, ib)
    y = engine(issuers, order=[5, 3, 1, 0, 2, 4])
    y.known_import(ia)
    y.known_remove(ib)
    assert export_sorted(y) == check(eng, N.KNOWN_MINUS, ia, ib)
    z = engine(issuers)
    z.known_import(ib)
    flags, _, _ = z.known_query(ia)
    meta, rec = KC.split(ia)
    hit = KI.records(ia)[0]
    held = {}
    for (k, m), f in zip(hit, flags):
        if f == 1:
            held.setdefault(k, []).append(m)
    assert KI.build(held) == check(eng, N.KNOWN_INTERSECT, ia, ib)
    for e in (x, y, z):
        e.close()


def test_incremental_snapshot(eng):
    issuers = synth.issuers(CFG)
    e = engine(issuers)
    e.map_batch(synth.host_batch(CFG, 0, 3000))
    old = export_sorted(e)
    res = e.map_batch(synth.host_batch(CFG, 2000, 3000))                      # the first third again, then new entries
    new = export_sorted(e)
    delta = check(eng, N.KNOWN_MINUS, new, old)
    assert check(eng, N.KNOWN_UNION, old, delta) == new
    assert KI.parse(delta).n_members == int(res.stats.n_new) > 0
    assert check(eng, N.KNOWN_MINUS, old, new) == EMPTY
    e.close()


# ---- 8. a group's image

@pytest.mark.parametrize("mode", ["owner", "bloom"])
@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_a_group_s_export_is_the_single_engine_s(mode, world):
    issuers = synth.issuers(CFG)
    single = engine(issuers)
    batches = [synth.host_batch(CFG, lo, 2400) for lo in (0, 1800)]           # the second repeats a quarter of the first
    for b in batches:
        single.map_batch(b)
    want = export_sorted(single)
    engines = [engine(issuers) for _ in range(world)]
    g = Group.local(engines)
    if mode == "bloom":
        g.bloom_config(1 << 16)
    base = 0
    for b in batches:
        shards, keep = [], []
        for r in range(world):
            lo, hi = shard_range(b.n, r, world)
            sub = Batch.from_certs([b.cert(i) for i in range(lo, hi)], b.issuer_idx[lo:hi], b.entry_type[lo:hi])
            t = to_dev(sub)
            keep.append(t)
            shards.append(dev_shard(t, sub.n, order_base=base + lo))
        g.map_batch(mode, shards)
        torch.cuda.synchronize()
        base += b.n
    assert g.total_count() == single.total_count()
    assert g.known_export() == want
    g.close()
    for e in engines + [single]:
        e.close()
