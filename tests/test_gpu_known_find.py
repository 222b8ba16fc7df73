"""-m gpu: serials looked up in a known image whatever their expiration date (include/ctmr.h ctmr_known_image_find*;
kernels/find.h k_find_build / k_find_scan / k_find_finish).

The device is held to the CPU twin known_image.find — which tests/test_find_corpus_cpu.py holds to the plain-list
expectation of tests/find_corpus.py — exactly, with no tolerance, through both variants and with guard bytes round both hit
buffers.  The shapes are the smallest at which the code can go wrong (tests/find_corpus.py lists them), not the workload's.
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr
from ct_mapreduce_amd import known_image as KI, synth, _native as N
from ct_mapreduce_amd.distributed import Group, shard_range
from ct_mapreduce_amd.engine import Batch
from tests import find_corpus as FC, xchg_corpus as XC
from tests.test_find_corpus_cpu import DAMAGED, GOOD
from tests.test_gpu_exchange import DEV, dev_shard, to_dev
from tests.test_gpu_known_image import engine, state, add_point_members
from tests.test_gpu_known_sort import table

CASES = {c.name: c for c in FC.all_cases()}
GUARD = 8          # hits in front of and behind each hit buffer
FILL = 0xEE
TWIN = functools.lru_cache(512)(KI.find)
CFG = synth.config(seed=131, n_issuers=6, dup_permille=150, ca_permille=20, expired_permille=20)


@pytest.fixture(scope="module")
def eng():
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)   # no issuer registered: the call needs none
    yield e
    e.close()


def fields(info):
    return {f: getattr(info, f) for f, _ in N.KnownFindInfo._fields_}


def parts(img):
    n_mem = min(KI._HEADER.unpack_from(img, 0)[6], len(img) // 48) if len(img) >= 64 else 0
    at = len(img) - 48 * n_mem
    return img[:at], np.frombuffer(img[at:], np.uint8), n_mem


def call(e, known, probes, now, device, hits_cap=None, host_cap=None):
    """One raw call with guard hits round both buffers → (rc, info, hits or None, host_hits or None).  The operands must
    stay as they were; a call that fails must leave both buffers as they were."""
    info = N.KnownFindInfo()
    n, n_host = e._header_counts(probes)
    hits_cap = n if hits_cap is None else hits_cap
    host_cap = n_host if host_cap is None else host_cap
    hh = np.full((host_cap + 2 * GUARD) * 16, FILL, np.uint8)
    if device:
        (k_meta, k_raw, nk), (p_meta, p_raw, npr) = parts(known), parts(probes)
        d_k = torch.from_numpy(np.concatenate([k_raw, np.zeros(16, np.uint8)])).to(DEV)
        d_p = torch.from_numpy(np.concatenate([p_raw, np.zeros(16, np.uint8)])).to(DEV)
        t = torch.full(((hits_cap + 2 * GUARD) * 16,), FILL, dtype=torch.uint8, device=DEV)
        assert t.data_ptr() % 16 == 0 and d_k.data_ptr() % 16 == 0 and d_p.data_ptr() % 16 == 0
        rc = e._lib.ctmr_known_image_find_device(
            e._h, k_meta, len(k_meta), C.c_void_p(d_k.data_ptr()) if nk else None, nk, p_meta, len(p_meta),
            C.c_void_p(d_p.data_ptr()) if npr else None, npr, int(now), C.c_void_p(t.data_ptr() + GUARD * 16), hits_cap,
            hh.ctypes.data + GUARD * 16, host_cap, C.byref(info))
        assert (d_k.cpu().numpy()[:len(k_raw)] == k_raw).all() and (d_p.cpu().numpy()[:len(p_raw)] == p_raw).all()
        hb = t.cpu().numpy()
    else:
        hb = np.full((hits_cap + 2 * GUARD) * 16, FILL, np.uint8)
        rc = e._lib.ctmr_known_image_find(e._h, known, len(known), probes, len(probes), int(now), hb.ctypes.data + GUARD * 16,
                                          hits_cap, hh.ctypes.data + GUARD * 16, host_cap, C.byref(info))
    for b, cap, what in ((hb, hits_cap, "hits"), (hh, host_cap, "host hits")):
        assert (b[:GUARD * 16] == FILL).all() and (b[(GUARD + cap) * 16:] == FILL).all(), what + " guards"
    if rc:
        assert (hb == FILL).all() and (hh == FILL).all(), "written on failure"
        return rc, info, None, None
    assert (hb[(GUARD + n) * 16:] == FILL).all() and (hh[(GUARD + n_host) * 16:] == FILL).all(), "written behind the last hit"
    return rc, info, hb[GUARD * 16:(GUARD + n) * 16].view(KI.HIT_DTYPE).copy(), hh[GUARD * 16:(GUARD + n_host) * 16].view(KI.HIT_DTYPE).copy()


def members_read(known, now):
    """The member records of the sets of `known` kept at `now`, from the set records."""
    _, _, _, n_iss, _, n_sets, _, _, _, _ = KI._HEADER.unpack_from(known, 0)
    total = 0
    for s in range(n_sets):
        eh, _, _, count = KI._SET.unpack_from(known, 64 + 32 * n_iss + 24 * s)
        if FC.HOUR_LO <= eh < FC.HOUR_HI and now < (eh + 1) * 3600:
            total += count
    return total


def differ(got, want, what):
    assert len(got) == len(want), what
    bad = np.flatnonzero(got != want)
    if len(bad):
        raise AssertionError("%s: %d of %d differ, first %d: got %r, want %r" % (what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]]))


def check(e, known, probes, now, variants=(False, True)):
    """Both variants against the twin, the info against what the twin and the headers say."""
    want, want_host = TWIN(known, probes, now)
    for device in variants:
        rc, info, hits, host_hits = call(e, known, probes, now, device)
        assert rc == 0, e._lib.ctmr_last_error(e._h)
        differ(hits, want, "hits (device=%s)" % device)
        differ(host_hits, want_host, "host hits (device=%s)" % device)
        f = fields(info)
        assert (f["probes"], f["host_probes"]) == (len(want), len(want_host))
        assert (f["found"], f["host_found"]) == (int((want["records"] > 0).sum()), int((want_host["records"] > 0).sum()))
        assert f["members_read"] == members_read(known, now)
    return want, want_host


# ---- 1. the corpus: counts, hours, near misses, serial lengths, now, repeats, host sections

@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_of_the_corpus(name, eng):
    c = CASES[name]
    want, want_host = check(eng, c.known, c.probes, c.now)
    assert np.array_equal(want, FC.as_array(c.hits)) and np.array_equal(want_host, FC.as_array(c.host_hits))


def test_the_python_entry_points(eng):
    c = CASES["host"]
    want, want_host = TWIN(c.known, c.probes, c.now)
    hits, host_hits, info = eng.known_image_find(c.known, c.probes, c.now)
    assert np.array_equal(hits, want) and np.array_equal(host_hits, want_host)
    assert info["probes"] == len(want) and info["found"] == int((want["records"] > 0).sum())
    (k_meta, k_raw, _), (p_meta, p_raw, _) = parts(c.known), parts(c.probes)
    d_hits, host_hits, info2 = eng.known_image_find_device(k_meta, torch.from_numpy(k_raw.copy()).to(DEV), p_meta,
                                                           torch.from_numpy(p_raw.copy()).to(DEV), c.now)
    assert d_hits.is_cuda and d_hits.dtype == torch.int32 and tuple(d_hits.shape) == (len(want), 4)   # left on the device
    assert np.array_equal(d_hits.cpu().numpy().view(KI.HIT_DTYPE).reshape(-1), want) and np.array_equal(host_hits, want_host)
    assert info2 == info


# ---- 2. the forced table: the smallest power of two above the probes, chains that wrap its end

@pytest.mark.parametrize("name", ["counts-63-257", "counts-64-257", "counts-255-257", "counts-256-257", "counts-1025-1025", "hours-300",
                                  "lengths-twins", "repeats", "host"])
def test_the_smallest_table(name, eng, monkeypatch):
    monkeypatch.setenv("CTMR_KNOWN_FIND_SLOTS", "1")
    c = CASES[name]
    check(eng, c.known, c.probes, c.now)


@functools.lru_cache(1)
def shared_tags():
    """8-octet serials of K ordinal 0 that share the 24-bit tag AND the home slot of a 64-word table under the find's
    hash — key_hash over (8 << 56 | ordinal) — found as tests/reduce_corpus.py finds them for the table's hash:
    → (pairs, pairs whose home slot is the last one, serials by home slot)."""
    U = XC.U
    s = XC.np_serials8(977, 1 << 22)
    with np.errstate(over="ignore"):
        h = XC.np_mixk(np.full(1, 8 << 56, U) + U(0x9e3779b97f4a7c15))
        h = XC.np_mixk(XC.np_mixk(h ^ s ^ U(0x3c6ef372fe94f82b)))
    assert int(h[0]) == XC.key_hash(8 << 56, XC.serial_words(XC.s8(s[0])))
    sig = (XC.np_key_tag(h) << U(8)) | (h & U(63))
    order = np.argsort(sig, kind="stable")
    ss = sig[order]
    change = np.flatnonzero(np.concatenate(([True], ss[1:] != ss[:-1], [True])))
    starts, lens = change[:-1], np.diff(change)
    p_at = starts[lens == 2]
    pair = lambda k: (XC.s8(s[order[k]]), XC.s8(s[order[k + 1]]))
    last = p_at[(ss[p_at] & U(0xff)) == U(63)]
    by_home = {}
    for k in range(2048):
        by_home.setdefault(int(h[k]) & 63, []).append(XC.s8(s[k]))
    return [pair(k) for k in p_at[:6]], [pair(k) for k in last[:2]], by_home


def test_probes_that_share_a_tag_and_a_home_slot(eng, monkeypatch):
    """With 40..63 probes the forced table has 64 words.  Of two probes with one tag and one home slot K holds the
    second only, or both: the walk must compare in full and go on behind a tag match that is no match; a pair at home
    slot 63 continues at word 0, and fillers at 58..63 and 0..3 push it further round."""
    monkeypatch.setenv("CTMR_KNOWN_FIND_SLOTS", "1")
    pairs, wrap, by_home = shared_tags()
    assert len(pairs) >= 4 and len(wrap) >= 1
    d = FC.digest(0)
    fill = [m for home in (58, 59, 60, 61, 62, 63, 0, 1, 2, 3) for m in by_home.get(home, [])[:3]]
    probes = [m for p in pairs[:4] + wrap[:1] for m in p] + fill
    assert 40 <= len(probes) <= 63 and len(set(probes)) == len(probes)
    held = [pairs[0][1], pairs[1][0], pairs[2][0], pairs[2][1], wrap[0][1]] + fill[::2]
    for order in (probes, probes[::-1]):
        for k_members in (held, held[::-1] + held[:3]):
            known = FC.raw_image([(FC.H0, d, k_members), (FC.H0 + 2, d, [pairs[3][0], pairs[3][1], wrap[0][0]])])[0]
            p_img = FC.raw_image([(0, d, order)])[0]
            want, _ = check(eng, known, p_img, FC.INT64_MIN)
            got = dict(zip(order, (tuple(h)[:3] for h in want)))
            assert got[pairs[0][0]] == (0, 0, 0) and got[pairs[0][1]][0] >= 1 and got[wrap[0][0]] == (1, FC.H0 + 2, FC.H0 + 2)


# 8-octet serials whose 24-bit tag stays the same when the hashed length goes from 8 to 9 (the serial followed by 00
# has the same five words) and when the hashed K ordinal goes from 0 to 1: found once by a search over 2^27 serials with
# the numpy port of the hash, held here and checked against the port below.  tests/reduce_corpus.py's way of finding
# keys that share a tag carries over; what does not is finding them at test time — a hit takes 2^24 tries.
SAME_TAG_NEXT_LENGTH = [bytes.fromhex(x) for x in ("11ae1e405dc2df6c", "11300a57b96c122c", "116071abd8277335")]
SAME_TAG_NEXT_ORDINAL = [bytes.fromhex(x) for x in ("1155e3ca8626e379", "11ef9d8500d0c723", "11d7847b1a49173b")]


def find_hash(kord, serial):
    return XC.key_hash((len(serial) << 56) | kord, XC.serial_words(serial))


@pytest.mark.parametrize("which", ["length", "ordinal"])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_a_tag_match_is_compared_in_full(which, k, eng, monkeypatch):
    """A record of K and a probe that differ ONLY in the serial's length (s and s 00) or ONLY in the issuer, and whose
    hashes still give the same tag: the hash covers length and ordinal, so nothing else brings such a pair to the full
    compare.  63 probes in the forced table of 64 words, 60 of them with the record's home slot: the one empty word lies
    right in front of that slot (which words end up occupied does not depend on the order of insertion), so the record
    walks all 63 and meets the probe wherever it went."""
    monkeypatch.setenv("CTMR_KNOWN_FIND_SLOTS", "1")
    a, b = FC.digest(0), FC.digest(1)       # K ordinals 0 and 1: K lists its issuers in digest order
    assert a < b
    s = (SAME_TAG_NEXT_LENGTH if which == "length" else SAME_TAG_NEXT_ORDINAL)[k]
    near = (a, s + b"\x00") if which == "length" else (b, s)
    kord = 0 if near[0] == a else 1
    assert XC.key_tag(find_hash(0, s)) == XC.key_tag(find_hash(kord, near[1])) and (near[0], near[1]) != (a, s)
    home = find_hash(0, s) & 63
    rng = np.random.default_rng(17)
    fill = []
    while len(fill) < 60:
        m = bytes(rng.integers(1, 256, size=8, dtype=np.uint8).tolist())
        if find_hash(0, m) & 63 == home and m != s and m not in fill:
            fill.append(m)
    third = next(m for m in (bytes([j]) + s[1:] for j in range(0x20, 0x40)) if find_hash(1, m) & 63 != (home - 1) & 63)
    specials = [(a, s), near, (b, third)]
    assert all(find_hash(0 if d == a else 1, m) & 63 != (home - 1) & 63 for d, m in specials)
    known = FC.raw_image([(FC.H0, a, [s, fill[0]]), (FC.H0 + 1, b, [third + b"\x01"])])[0]
    p_sets = [(0, a, [m for d, m in specials if d == a] + fill), (0, b, [m for d, m in specials if d == b])]
    probes, order, _ = FC.raw_image(p_sets)
    assert len(order) == 63
    want, _ = check(eng, known, probes, FC.INT64_MIN)
    got = dict(zip(order, (tuple(h)[:3] for h in want)))
    assert got[(a, s)] == (1, FC.H0, FC.H0) and got[near] == (0, 0, 0) and got[(a, fill[0])] == (1, FC.H0, FC.H0)


# ---- 3. forced runs

@pytest.mark.parametrize("chunk", [1, 100, 300])
def test_a_probe_matched_in_three_runs_accumulates(chunk, eng, monkeypatch):
    monkeypatch.setenv("CTMR_KNOWN_FIND_CHUNK", str(chunk))
    s = b"\x61\x62\x63\x64\x65"
    rng = np.random.default_rng(5)
    other = FC._serials(rng, 900, 6, 12)
    d = FC.digest(0)
    k_sets = [(FC.H0, d, other[:120] + [s]), (FC.H0 + 1, d, other[120:400]), (FC.H0 + 2, d, [s] + other[400:520]),
              (FC.H0 + 3, FC.digest(1), other[520:800] + [s]), (FC.H0 + 4, d, other[800:] + [s, s])]
    c = FC.case("runs", k_sets, [(0, d, [other[0], s, other[899], b"\x00"])], FC.INT64_MIN)
    assert c.hits[1] == (4, FC.H0, FC.H0 + 4)
    want, _ = check(eng, c.known, c.probes, c.now)
    assert np.array_equal(want, FC.as_array(c.hits))
    for name in ("counts-257-257", "hours-300", "host"):
        check(eng, CASES[name].known, CASES[name].probes, CASES[name].now)


# ---- 4. validation: every rejection leaves both buffers as they were

@pytest.mark.parametrize("name", [n for n, _ in DAMAGED])
def test_what_the_import_rejects_in_either_operand(name, eng):
    bad = dict(DAMAGED)[name]
    for device in (False, True):
        if device and name in ("short", "truncated", "trailing"):
            continue   # the device variant is given the member count apart: covered by test_a_member_count_that_disagrees
        for known, probes in ((bad, GOOD), (GOOD, bad)):
            rc, info, _, _ = call(eng, known, probes, 0, device)
            assert rc == N.E_INVAL, (name, device)
            if name in ("serial-len", "padding"):   # … found on the device: the message says which check
                assert b"member record" in eng._lib.ctmr_last_error(eng._h)


def test_a_member_count_that_disagrees(eng):
    (k_meta, k_raw, nk), (p_meta, p_raw, npr) = parts(GOOD), parts(GOOD)
    d = torch.from_numpy(np.concatenate([k_raw, np.zeros(48, np.uint8)])).to(DEV)
    hits = torch.full((16 * 16,), FILL, dtype=torch.uint8, device=DEV)
    hh = np.full(16 * 16, FILL, np.uint8)
    for a, b in ((nk + 1, npr), (nk, npr - 1)):
        rc = eng._lib.ctmr_known_image_find_device(eng._h, k_meta, len(k_meta), C.c_void_p(d.data_ptr()), a, p_meta, len(p_meta),
                                                   C.c_void_p(d.data_ptr()), b, 0, C.c_void_p(hits.data_ptr()), 16, hh.ctypes.data, 16,
                                                   C.byref(N.KnownFindInfo()))
        assert rc == N.E_INVAL
    assert (hits.cpu().numpy() == FILL).all() and (hh == FILL).all()


@pytest.mark.parametrize("key", [b"serials::2025-01-01-00", b"serials::a::b::c", b"serials::"])
def test_a_host_key_that_does_not_split_in_three(key, eng):
    bad = FC.raw_image([], [(key, b"\x01")])[0]
    for device in (False, True):
        for known, probes, now in ((bad, GOOD, 0), (GOOD, bad, 0), (bad, GOOD, 2 ** 62)):
            assert call(eng, known, probes, now, device)[0] == N.E_INVAL


def damaged_record(img, index, how):
    meta, raw, n = parts(img)
    rec = np.frombuffer(raw.tobytes(), KI.MEMBER_DTYPE).copy()
    if how == "len":
        rec["len"][index] = 41
    else:
        rec["serial"][index, int(rec["len"][index])] = 1
    return meta + rec.tobytes()


@pytest.mark.parametrize("how", ["len", "pad"])
def test_a_bad_record_in_the_last_run_and_in_a_set_that_is_not_kept(how, eng, monkeypatch):
    monkeypatch.setenv("CTMR_KNOWN_FIND_CHUNK", "200")
    c = CASES["counts-1025-1025"]
    n_k = KI.parse(c.known).n_members
    lens = np.frombuffer(parts(c.known)[1].tobytes(), KI.MEMBER_DTYPE)["len"]
    last = max(i for i in range(n_k) if lens[i] < 40)
    for device in (False, True):
        # K: the last record of all — the last run; P: its last record
        assert call(eng, damaged_record(c.known, last, how), c.probes, c.now, device)[0] == N.E_INVAL
        n_p = KI.parse(c.probes).n_members
        assert call(eng, c.known, damaged_record(c.probes, n_p - 1, how), c.now, device)[0] == N.E_INVAL
    # a set that is not kept is not read: its damage does not fail the call, and the answer is that of the image without it
    s = b"\x0a\x0b"
    k_sets = [(FC.H0, FC.digest(0), [s, b"\x0c"]), (FC.H0 + 5, FC.digest(0), [s, b"\x0d" * 7])]
    good = FC.raw_image(k_sets)[0]
    p = KI.probes({FC.digest(0): [s, b"\x0c"]})
    now = (FC.H0 + 1) * 3600
    bad = damaged_record(good, 1, how)
    for device in (False, True):
        rc, info, hits, _ = call(eng, bad, p, now, device)
        assert rc == 0 and np.array_equal(hits, TWIN(good, p, now)[0]) and info.members_read == 2 and info.sets_kept == 1
        assert call(eng, bad, p, now - 1, device)[0] == N.E_INVAL       # … one second earlier the set is kept and read


# ---- 5. sizing: the two-call convention

def test_short_hit_buffers(eng):
    c = CASES["host"]
    n, n_host = len(c.hits), len(c.host_hits)
    assert n > 1 and n_host > 1
    for device in (False, True):
        for hits_cap, host_cap in ((n - 1, n_host), (n, n_host - 1), (0, 0)):
            rc, info, _, _ = call(eng, c.known, c.probes, c.now, device, hits_cap, host_cap)
            assert rc == N.E_RANGE
            assert (info.probes, info.host_probes, info.members_read) == (n, n_host, members_read(c.known, c.now))
        rc, info, hits, host_hits = call(eng, c.known, c.probes, c.now, device, n + 3, n_host + 2)
        assert rc == 0 and np.array_equal(hits, FC.as_array(c.hits)) and np.array_equal(host_hits, FC.as_array(c.host_hits))
    # sized from P's header alone, null buffers
    info = N.KnownFindInfo()
    rc = eng._lib.ctmr_known_image_find(eng._h, c.known, len(c.known), c.probes, len(c.probes), int(c.now), None, 0, None, 0, C.byref(info))
    assert rc == N.E_RANGE and (info.probes, info.host_probes) == eng._header_counts(c.probes)


# ---- 6. read-only; the engine's own sets

@contextlib.contextmanager
def closing(*things):
    """The engines and groups of a test, closed in reverse order whether it passes or fails: a failed assertion must not
    leave a group and its engines behind for the tests that follow."""
    try:
        yield things
    finally:
        for x in reversed(things):
            x.close()


def built_engine(bloom=False):
    issuers = synth.issuers(CFG)
    e = engine(issuers, table_slots=1 << 13)
    if bloom:
        e.bloom_config(1 << 16)
    e.map_batch(synth.host_batch(CFG, 0, 2500))
    add_point_members(e, [e.issuer_id(k) for k in range(len(issuers))])
    return e


def probes_of(img, rng, extra=()):
    """A probe image of every third member of `img`, a shortened twin of each, every member above 40 octets, and
    `extra`."""
    by = {}
    for key, ms in KI.parse(img).sets.items():
        pk = KI.parse_key(key)
        if pk is None:
            continue
        for m in ms[::3] + [m for m in ms if len(m) > KI.MAX_SERIAL]:
            by.setdefault(pk[1], set()).update((m, m[:-1]))
    for dg, m in extra:
        by.setdefault(dg, set()).add(m)
    return KI.probes({d: sorted(ms) for d, ms in by.items()})


@pytest.mark.parametrize("bloom", [False, True])
def test_nothing_of_the_engine_is_read_or_changed(bloom):
    with closing(built_engine(bloom)) as (e,):
        nothing_read_or_changed(e)


def nothing_read_or_changed(e):
    e.set_known_order(N.KNOWN_ORDER_SORTED)
    img = e.known_export()
    p = probes_of(img, np.random.default_rng(1))
    before = (state(e), table(e), e.issuer_counts().tobytes(), bytes(e.table_info()))
    other = CASES["host"]
    check(e, other.known, other.probes, other.now)       # another image altogether: the engine's own sets play no part
    want, want_host = check(e, img, p, 0)
    assert (want["records"] > 0).any() and (want_host["records"] > 0).any()
    assert (state(e), table(e), e.issuer_counts().tobytes(), bytes(e.table_info())) == before and e.known_export() == img


def test_known_find_of_the_engine_s_own_sets():
    with closing(built_engine()) as (e,):
        own_sets(e)


def own_sets(e):
    e.set_known_order(N.KNOWN_ORDER_SORTED)
    img = e.known_export()
    p = probes_of(img, np.random.default_rng(2), [(FC.digest(9), b"\x01")])
    hours = sorted({KI.exp_date_span(k.split(b"::")[1])[0] // 3600 for k in KI.parse(img).sets})
    for now in (0, (hours[len(hours) // 2] + 1) * 3600):
        hits, host_hits, info = e.known_find(p, now)
        want, want_host = TWIN(img, p, now)
        differ(hits, want, "hits")
        differ(host_hits, want_host, "host hits")
        assert info["found"] == int((want["records"] > 0).sum()) > 0
    # after an expire_sweep the swept sets are gone from the export, and so from the answer at an earlier now
    cut = (hours[len(hours) // 2] + 1) * 3600
    assert e.expire_sweep(cut) > 0
    img2 = e.known_export()
    assert img2 != img
    hits, host_hits, _ = e.known_find(p, 0)
    want, want_host = TWIN(img2, p, 0)
    differ(hits, want, "hits after the sweep")
    differ(host_hits, want_host, "host hits after the sweep")
    assert not np.array_equal(want, TWIN(img, p, 0)[0])
    # after a known_remove of every third member of every set those are found no more
    e.known_remove(KI.build({k: ms[::3] for k, ms in KI.parse(img2).sets.items()}))
    hits, host_hits, info = e.known_find(p, 0)
    img3 = e.known_export()
    differ(hits, TWIN(img3, p, 0)[0], "hits after the remove")
    differ(host_hits, TWIN(img3, p, 0)[1], "host hits after the remove")
    assert info["found"] < int((want["records"] > 0).sum())


# ---- 7. groups

@pytest.mark.parametrize("mode", ["owner", "bloom"])
@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_a_group_answers_as_the_single_engine(mode, world):
    issuers = synth.issuers(CFG)
    single = engine(issuers)
    batches = [synth.host_batch(CFG, lo, 2400) for lo in (0, 1800)]
    for b in batches:
        single.map_batch(b)
    engines = [engine(issuers) for _ in range(world)]
    with closing(single, *engines, Group.local(engines)) as things:
        group_answers(things[-1], single, engines, batches, mode, world)


def group_answers(g, single, engines, batches, mode, world):
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
    single.set_known_order(N.KNOWN_ORDER_SORTED)
    img = single.known_export()
    p = probes_of(img, np.random.default_rng(3), [(FC.digest(9), b"\x01")])
    hours = sorted({KI.exp_date_span(k.split(b"::")[1])[0] // 3600 for k in KI.parse(img).sets})
    for now in (0, (hours[len(hours) // 2] + 1) * 3600):
        want, want_host, _ = single.known_find(p, now)
        differ(want, TWIN(img, p, now)[0], "the single engine")
        hits, host_hits = g.known_find(p, now)
        differ(hits, want, "the group's hits")
        differ(host_hits, want_host, "the group's host hits")
    assert (want["records"] > 0).any()
