"""-m gpu: a known image partitioned by a probe image, the hour as wildcard (include/ctmr.h ctmr_known_image_split*;
kernels/split.h k_split_mark / k_split_place / k_split_sets over kernels/find.h's table).

The device is held to the CPU twin known_image.split — which tests/test_split_corpus_cpu.py holds to the plain-list
expectation of tests/split_corpus.py — exactly, byte for byte, through both variants at exact-size buffers, with guard
bytes round all four output buffers (both metas, both member sections; the host variant's two images).  The operands
must stay as they were and a call that fails must leave every buffer as it was.  The shapes are the smallest at which
the code can go wrong (tests/split_corpus.py lists them), not the workload's.
"""
import base64
import ctypes as C
import functools
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr
from ct_mapreduce_amd import crl as CRL, known_image as KI, synth, _native as N
from ct_mapreduce_amd.engine import Batch
from tests import crl_corpus as CC, der as D, find_corpus as FC, split_corpus as SC, xchg_corpus as XC
from tests.test_find_corpus_cpu import DAMAGED, GOOD
from tests.test_gpu_exchange import DEV
from tests.test_gpu_known_find import (SAME_TAG_NEXT_LENGTH, SAME_TAG_NEXT_ORDINAL, built_engine, closing, damaged_record, find_hash, parts,
                                        probes_of, shared_tags)
from tests.test_gpu_known_image import state
from tests.test_gpu_known_sort import table

CASES = {c.name: c for c in SC.all_cases()}
GUARD = 64         # bytes in front of and behind each output buffer (a multiple of 16: the device pointers stay aligned)
FILL = 0xEE
TWIN = functools.lru_cache(512)(KI.split)
INFO_FIELDS = ("members", "sets", "host_members", "meta_bytes", "image_bytes", "issuers")


@pytest.fixture(scope="module")
def eng():
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)   # no issuer registered: the call needs none
    yield e
    e.close()


def image_info(img):
    h = KI._HEADER.unpack_from(img, 0)
    return dict(members=h[6], sets=h[5], host_members=h[8], meta_bytes=len(img) - 48 * h[6], image_bytes=len(img), issuers=h[3])


def info_of(part):
    return {f: getattr(part, f) for f in INFO_FIELDS}


def members_read(known, now):
    """The member records of the sets of `known` kept at `now`, from the set records."""
    h = KI._HEADER.unpack_from(known, 0)
    recs = [KI._SET.unpack_from(known, 64 + 32 * h[3] + 24 * s) for s in range(h[5])]
    return sum(r[3] for r in recs if FC.kept(r[0], now))


class Host:
    """One output buffer of the host variant between guards: cap bytes, or declined (cap None)."""

    def __init__(self, cap):
        self.cap = cap
        self.buf = np.full((cap or 0) + 2 * GUARD, FILL, np.uint8)

    def args(self):
        return (None, 0) if self.cap is None else (self.buf.ctypes.data + GUARD, self.cap)

    def untouched(self):
        return (self.buf == FILL).all()

    def image(self, info):
        assert (self.buf[:GUARD] == FILL).all() and (self.buf[GUARD + info.image_bytes:] == FILL).all(), "written outside the image"
        return self.buf[GUARD:GUARD + info.image_bytes].tobytes()


class Device:
    """One result of the device variant: a meta buffer on the host and a member buffer on the device, each between
    guards; caps = (meta bytes, member records), or declined (None)."""

    def __init__(self, caps, shift=0):
        self.caps = caps
        meta_cap, rec_cap = caps or (0, 0)
        self.meta = np.full(meta_cap + 2 * GUARD, FILL, np.uint8)
        self.rec = torch.full((48 * rec_cap + 2 * GUARD + 16,), FILL, dtype=torch.uint8, device=DEV)
        self.ptr = self.rec.data_ptr() + GUARD + shift
        assert (self.rec.data_ptr() + GUARD) % 16 == 0

    def args(self):
        if self.caps is None:
            return (None, 0, None, 0)
        return (self.meta.ctypes.data + GUARD, self.caps[0], C.c_void_p(self.ptr), self.caps[1])

    def untouched(self):
        return (self.meta == FILL).all() and (self.rec.cpu().numpy() == FILL).all()

    def image(self, info):
        rec = self.rec.cpu().numpy()
        assert (self.meta[:GUARD] == FILL).all() and (self.meta[GUARD + info.meta_bytes:] == FILL).all(), "written outside the meta"
        assert (rec[:GUARD] == FILL).all() and (rec[GUARD + 48 * info.members:] == FILL).all(), "written outside the member records"
        return self.meta[GUARD:GUARD + info.meta_bytes].tobytes() + rec[GUARD:GUARD + 48 * info.members].tobytes()


def call(e, known, probes, now, device, hit="exact", miss="exact", shift=(0, 0, 0, 0)):
    """One raw call → (rc, info, hit image or None, miss image or None).  hit / miss: "exact" — buffers of exactly the
    twin's sizes —, None — declined —, or the capacities: bytes (host variant), (meta bytes, member records) (device
    variant).  shift: bytes added to the device pointers of K, P, HIT and MISS.  The operands must stay as they were; a
    call that fails must leave every buffer as it was."""
    sizes = []
    for cap, want in zip((hit, miss), TWIN(known, probes, now) if "exact" in (hit, miss) else (None, None)):
        if cap == "exact":
            i = image_info(want)
            cap = (i["meta_bytes"], i["members"]) if device else i["image_bytes"]
        sizes.append(cap)
    info = N.KnownSplitInfo()
    keep = (bytes(bytearray(known)), bytes(bytearray(probes)))
    if device:
        (k_meta, k_raw, nk), (p_meta, p_raw, npr) = parts(known), parts(probes)
        d_k = torch.from_numpy(np.concatenate([k_raw, np.zeros(32, np.uint8)])).to(DEV)
        d_p = torch.from_numpy(np.concatenate([p_raw, np.zeros(32, np.uint8)])).to(DEV)
        assert d_k.data_ptr() % 16 == 0 and d_p.data_ptr() % 16 == 0
        outs = [Device(sizes[0], shift[2]), Device(sizes[1], shift[3])]
        rc = e._lib.ctmr_known_image_split_device(
            e._h, k_meta, len(k_meta), C.c_void_p(d_k.data_ptr() + shift[0]) if nk else None, nk, p_meta, len(p_meta),
            C.c_void_p(d_p.data_ptr() + shift[1]) if npr else None, npr, int(now), *outs[0].args(), *outs[1].args(), C.byref(info))
        assert (d_k.cpu().numpy()[:len(k_raw)] == k_raw).all() and (d_p.cpu().numpy()[:len(p_raw)] == p_raw).all()
    else:
        outs = [Host(sizes[0]), Host(sizes[1])]
        rc = e._lib.ctmr_known_image_split(e._h, known, len(known), probes, len(probes), int(now), *outs[0].args(), *outs[1].args(),
                                           C.byref(info))
    assert (known, probes) == keep, "an operand changed"
    if rc:
        assert outs[0].untouched() and outs[1].untouched(), "written on failure"
        return rc, info, None, None
    got = []
    for o, size, part in zip(outs, sizes, (info.hit, info.miss)):
        if size is None:
            assert o.untouched(), "a declined side was written"
            got.append(None)
        else:
            got.append(o.image(part))
    return rc, info, got[0], got[1]


def check(e, known, probes, now, variants=(False, True)):
    """Both variants against the twin, the info against what the twin's images and the headers say."""
    want = TWIN(known, probes, now)
    for device in variants:
        rc, info, hit, miss = call(e, known, probes, now, device)
        assert rc == 0, e._lib.ctmr_last_error(e._h)
        assert hit == want[0], "HIT (device=%s)" % device
        assert miss == want[1], "MISS (device=%s)" % device
        assert info_of(info.hit) == image_info(want[0]) and info_of(info.miss) == image_info(want[1])
        assert (info.probes, info.host_probes) == e._header_counts(probes)
        assert info.members_read == members_read(known, now) == info.hit.members + info.miss.members
    return want


# ---- 1. the corpus

@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_of_the_corpus(name, eng):
    c = CASES[name]
    want = check(eng, c.known, c.probes, c.now)
    assert want == (c.hit, c.miss)


def test_the_python_entry_points(eng):
    c = CASES["host-sides"]
    hit, miss, info = eng.known_image_split(c.known, c.probes, c.now)
    assert (hit, miss) == (c.hit, c.miss)
    assert info["hit"] == image_info(c.hit) and info["miss"] == image_info(c.miss) and info["members_read"] == 2
    only, none, info2 = eng.known_image_split(c.known, c.probes, c.now, want=("hit",))
    assert only == c.hit and none is None and info2 == info
    (k_meta, k_raw, _), (p_meta, p_raw, _) = parts(c.known), parts(c.probes)
    d_k, d_p = torch.from_numpy(k_raw.copy()).to(DEV), torch.from_numpy(p_raw.copy()).to(DEV)
    (hm, dh), (mm, dm), info3 = eng.known_image_split_device(k_meta, d_k, p_meta, d_p, c.now)
    assert dh.is_cuda and dm.is_cuda and dh.dtype == torch.uint8                                 # left on the device
    assert hm + dh.cpu().numpy().tobytes() == c.hit and mm + dm.cpu().numpy().tobytes() == c.miss and info3 == info
    none, (mm, dm), _ = eng.known_image_split_device(k_meta, d_k, p_meta, d_p, c.now, want=["miss"])
    assert none is None and mm + dm.cpu().numpy().tobytes() == c.miss
    with pytest.raises(ValueError):
        eng.known_image_split(c.known, c.probes, c.now, want=("both",))


# ---- 2. the forced table: the smallest power of two above the probes, chains that wrap its end

@pytest.mark.parametrize("name", ["counts-63", "counts-64", "counts-255", "counts-256", "counts-1025", "hours-300", "lengths-twins",
                                  "repeats", "host"])
def test_the_smallest_table(name, eng, monkeypatch):
    monkeypatch.setenv("CTMR_KNOWN_FIND_SLOTS", "1")
    c = CASES[name]
    assert check(eng, c.known, c.probes, c.now) == (c.hit, c.miss)


def test_probes_that_share_a_tag_and_a_home_slot(eng, monkeypatch):
    """The operands of the find's test of the same name: of two probes with one tag and one home slot K holds the second
    only, or both — the walk must compare in full and go on behind a tag match that is no match —; a pair at home slot
    63 continues at word 0."""
    monkeypatch.setenv("CTMR_KNOWN_FIND_SLOTS", "1")
    pairs, wrap, by_home = shared_tags()
    d = FC.digest(0)
    fill = [m for home in (58, 59, 60, 61, 62, 63, 0, 1, 2, 3) for m in by_home.get(home, [])[:3]]
    probes = [m for p in pairs[:4] + wrap[:1] for m in p] + fill
    assert 40 <= len(probes) <= 63 and len(set(probes)) == len(probes)
    lone = [b"\x00" + m[1:] for m in (pairs[0][0], wrap[0][0])]                # … held by K, no probe
    assert not set(lone) & set(probes)
    held = [pairs[0][1], pairs[1][0], lone[0], pairs[2][0], pairs[2][1], wrap[0][1], lone[1]] + fill[::2]
    for order in (probes, probes[::-1]):
        known = FC.raw_image([(FC.H0, d, held), (FC.H0 + 2, d, [pairs[3][0], lone[0], pairs[3][1], wrap[0][0]])])[0]
        hit, miss = check(eng, known, FC.raw_image([(0, d, order)])[0], FC.INT64_MIN)
        assert [m for _, m in KI.records(miss)[0]] == [lone[0], lone[1], lone[0]]


@pytest.mark.parametrize("which", ["length", "ordinal"])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_a_tag_match_is_compared_in_full(which, k, eng, monkeypatch):
    """A record of K and a probe that differ ONLY in the serial's length (s and s 00) or ONLY in the issuer, and whose
    hashes still give the same tag (the find's constants): the record must go to MISS.  63 probes in the forced table
    of 64 words, 61 of them with the record's home slot: the one empty word lies right in front of that slot, so the
    record walks all 63 and meets the probe wherever it went."""
    monkeypatch.setenv("CTMR_KNOWN_FIND_SLOTS", "1")
    a, b = FC.digest(0), FC.digest(1)       # K ordinals 0 and 1: K lists its issuers in digest order
    s = (SAME_TAG_NEXT_LENGTH if which == "length" else SAME_TAG_NEXT_ORDINAL)[k]
    near = (a, s + b"\x00") if which == "length" else (b, s)
    kord = 0 if near[0] == a else 1
    assert XC.key_tag(find_hash(0, s)) == XC.key_tag(find_hash(kord, near[1]))
    home = find_hash(0, s) & 63
    rng = np.random.default_rng(17)
    fill = []
    while len(fill) < 61:
        m = bytes(rng.integers(1, 256, size=8, dtype=np.uint8).tolist())
        if find_hash(0, m) & 63 == home and m != s and m not in fill:
            fill.append(m)
    third = next(m for m in (bytes([j]) + s[1:] for j in range(0x20, 0x40)) if find_hash(1, m) & 63 != (home - 1) & 63)
    specials = [near, (b, third)]
    assert all(find_hash(0 if d == a else 1, m) & 63 != (home - 1) & 63 for d, m in specials)
    known = FC.raw_image([(FC.H0, a, [s, fill[0]]), (FC.H0 + 1, b, [third + b"\x01", third])])[0]
    p_sets = [(0, a, [m for d, m in specials if d == a] + fill), (0, b, [m for d, m in specials if d == b])]
    probes, order, _ = FC.raw_image(p_sets)
    assert len(order) == 63
    hit, miss = check(eng, known, probes, FC.INT64_MIN)
    assert [m for _, m in KI.records(hit)[0]] == [fill[0], third] and [m for _, m in KI.records(miss)[0]] == [s, third + b"\x01"]
    assert by_the_bound(eng, SC.Case("", known, probes, FC.INT64_MIN, hit, miss)) == (hit, miss)


# ---- 3. forced runs: the hits in front of a block carry from run to run

@pytest.mark.parametrize("chunk", [1, 100, 300])
def test_runs_of_whole_sets(chunk, eng, monkeypatch):
    monkeypatch.setenv("CTMR_KNOWN_SPLIT_CHUNK", str(chunk))
    for name in ("boundary-257-sets", "boundary-768-and-257", "boundary-257-and-768", "boundary-whole-sets", "boundary-issuer-sides",
                 "boundary-digest-twice", "counts-1025", "hours-300", "host", "canonical"):
        c = CASES[name]
        assert check(eng, c.known, c.probes, c.now) == (c.hit, c.miss), name


def by_the_bound(e, c):
    """The device variant as Engine.known_image_split_device calls it — one call, each buffer as large as K — → the two
    images."""
    (k_meta, k_raw, _), (p_meta, p_raw, _) = parts(c.known), parts(c.probes)
    hit, miss, _ = e.known_image_split_device(k_meta, torch.from_numpy(k_raw.copy()).to(DEV), p_meta, torch.from_numpy(p_raw.copy()).to(DEV), c.now)
    return tuple(meta + d_rec.cpu().numpy().tobytes() for meta, d_rec in (hit, miss))


BOUND = sorted(n for n in CASES if n.startswith(("pattern-", "boundary-"))) + ["counts-1025", "misses"]


@pytest.mark.parametrize("name", BOUND)
def test_buffers_sized_by_the_bound(name, eng):
    assert by_the_bound(eng, CASES[name]) == (CASES[name].hit, CASES[name].miss)


@pytest.mark.parametrize("chunk", [1, 100, 300])
def test_buffers_sized_by_the_bound_in_runs(chunk, eng, monkeypatch):
    monkeypatch.setenv("CTMR_KNOWN_SPLIT_CHUNK", str(chunk))
    for name in ("boundary-257-sets", "boundary-768-and-257", "boundary-257-and-768", "boundary-issuer-sides"):
        assert by_the_bound(eng, CASES[name]) == (CASES[name].hit, CASES[name].miss), name


# ---- 4. declining and sizing

def test_each_side_declined_and_both(eng):
    c = CASES["boundary-issuer-sides"]
    for device in (False, True):
        rc, info, hit, miss = call(eng, c.known, c.probes, c.now, device, miss=None)
        assert rc == 0 and hit == c.hit and miss is None and info_of(info.miss) == image_info(c.miss)
        rc, info, hit, miss = call(eng, c.known, c.probes, c.now, device, hit=None)
        assert rc == 0 and hit is None and miss == c.miss and info_of(info.hit) == image_info(c.hit)
        rc, info, hit, miss = call(eng, c.known, c.probes, c.now, device, hit=None, miss=None)        # only sizes
        assert rc == 0 and info_of(info.hit) == image_info(c.hit) and info_of(info.miss) == image_info(c.miss)
        assert (info.probes, info.sets_kept, info.members_read) == (4, 5, 8)


def test_short_buffers_one_at_a_time(eng):
    c = CASES["host-sides"]
    hi, mi = image_info(c.hit), image_info(c.miss)
    for short in ((hi["image_bytes"] - 1, mi["image_bytes"]), (hi["image_bytes"], mi["image_bytes"] - 1), (0, mi["image_bytes"])):
        rc, info, _, _ = call(eng, c.known, c.probes, c.now, False, *short)
        assert rc == N.E_RANGE and info_of(info.hit) == hi and info_of(info.miss) == mi and info.members_read == 2
    full = ((hi["meta_bytes"], hi["members"]), (mi["meta_bytes"], mi["members"]))
    for side in (0, 1):
        for less in ((1, 0), (0, 1)):
            caps = [full[0], full[1]]
            caps[side] = (full[side][0] - less[0], full[side][1] - less[1])
            rc, info, _, _ = call(eng, c.known, c.probes, c.now, True, *caps)
            assert rc == N.E_RANGE and info_of(info.hit) == hi and info_of(info.miss) == mi and info.probes == 1
    # larger than needed: written at the front, the rest as it was; a caller can size by the bound without a first call
    k = image_info(c.known)
    rc, info, hit, miss = call(eng, c.known, c.probes, c.now, False, len(c.known), len(c.known))
    assert rc == 0 and (hit, miss) == (c.hit, c.miss)
    rc, info, hit, miss = call(eng, c.known, c.probes, c.now, True, (k["meta_bytes"], k["members"]), (k["meta_bytes"], k["members"]))
    assert rc == 0 and (hit, miss) == (c.hit, c.miss)
    assert all(image_info(x)["meta_bytes"] <= k["meta_bytes"] and image_info(x)["members"] <= k["members"]
               for cs in CASES.values() for x in (cs.hit, cs.miss) for k in [image_info(cs.known)])


def test_a_null_buffer_with_a_capacity(eng):
    c = CASES["repeats"]
    info = N.KnownSplitInfo()
    out = np.full(len(c.known), FILL, np.uint8)
    a = (eng._h, c.known, len(c.known), c.probes, len(c.probes), 0)
    assert eng._lib.ctmr_known_image_split(*a, None, 64, out.ctypes.data, out.nbytes, C.byref(info)) == N.E_INVAL
    assert eng._lib.ctmr_known_image_split(*a, out.ctypes.data, out.nbytes, None, 1, C.byref(info)) == N.E_INVAL
    (k_meta, k_raw, nk), (p_meta, p_raw, npr) = parts(c.known), parts(c.probes)
    d_k, d_p = torch.from_numpy(k_raw.copy()).to(DEV), torch.from_numpy(p_raw.copy()).to(DEV)
    d_out = torch.full((48 * nk,), FILL, dtype=torch.uint8, device=DEV)
    b = (eng._h, k_meta, len(k_meta), C.c_void_p(d_k.data_ptr()), nk, p_meta, len(p_meta), C.c_void_p(d_p.data_ptr()), npr, 0)
    assert eng._lib.ctmr_known_image_split_device(*b, None, 0, C.c_void_p(d_out.data_ptr()), nk, None, 0, None, 0, C.byref(info)) == N.E_INVAL
    assert eng._lib.ctmr_known_image_split_device(*b, None, 0, None, 0, None, 64, None, 0, C.byref(info)) == N.E_INVAL
    assert (out == FILL).all() and (d_out.cpu().numpy() == FILL).all()


# ---- 5. validation: every rejection leaves all four buffers as they were

def test_misaligned_device_pointers(eng):
    c = CASES["boundary-issuer-sides"]
    k = image_info(c.known)
    caps = (k["meta_bytes"], k["members"])
    for which in range(4):
        shift = [0, 0, 0, 0]
        shift[which] = 8
        assert call(eng, c.known, c.probes, c.now, True, caps, caps, shift=tuple(shift))[0] == N.E_INVAL, which


@pytest.mark.parametrize("name", [n for n, _ in DAMAGED])
def test_what_the_import_rejects_in_either_operand(name, eng):
    bad = dict(DAMAGED)[name]
    caps = {False: 4096, True: (4096, 64)}
    for device in (False, True):
        if device and name in ("short", "truncated", "trailing"):
            continue   # the device variant is given the member count apart: test_a_member_count_that_disagrees
        for known, probes in ((bad, GOOD), (GOOD, bad)):
            rc, info, _, _ = call(eng, known, probes, 0, device, caps[device], caps[device])
            assert rc == N.E_INVAL, (name, device)
            if name in ("serial-len", "padding"):   # … found on the device: the message says which check
                assert b"member record" in eng._lib.ctmr_last_error(eng._h)


def test_a_member_count_that_disagrees(eng):
    (k_meta, k_raw, nk), (p_meta, p_raw, npr) = parts(GOOD), parts(GOOD)
    d = torch.from_numpy(np.concatenate([k_raw, np.zeros(48, np.uint8)])).to(DEV)
    outs = [Device((4096, 64)), Device((4096, 64))]
    for a, b in ((nk + 1, npr), (nk, npr - 1)):
        rc = eng._lib.ctmr_known_image_split_device(eng._h, k_meta, len(k_meta), C.c_void_p(d.data_ptr()), a, p_meta, len(p_meta),
                                                    C.c_void_p(d.data_ptr()), b, 0, *outs[0].args(), *outs[1].args(),
                                                    C.byref(N.KnownSplitInfo()))
        assert rc == N.E_INVAL
    assert outs[0].untouched() and outs[1].untouched()


@pytest.mark.parametrize("key", [b"serials::2025-01-01-00", b"serials::a::b::c", b"serials::"])
def test_a_host_key_that_does_not_split_in_three(key, eng):
    bad = FC.raw_image([], [(key, b"\x01")])[0]
    for device, caps in ((False, 4096), (True, (4096, 64))):
        for known, probes, now in ((bad, GOOD, 0), (GOOD, bad, 0), (bad, GOOD, 2 ** 62)):
            assert call(eng, known, probes, now, device, caps, caps)[0] == N.E_INVAL


@pytest.mark.parametrize("how", ["len", "pad"])
def test_a_bad_record_in_p_in_the_last_run_of_k_and_in_a_set_that_is_not_kept(how, eng, monkeypatch):
    monkeypatch.setenv("CTMR_KNOWN_SPLIT_CHUNK", "200")
    c = CASES["counts-1025"]
    k = image_info(c.known)
    lens = np.frombuffer(parts(c.known)[1].tobytes(), KI.MEMBER_DTYPE)["len"]
    last = max(i for i in range(k["members"]) if lens[i] < 40)
    assert last >= k["members"] - 4                                 # … one of the last one-member sets: the last run
    n_p = image_info(c.probes)["members"]
    for device, caps in ((False, len(c.known)), (True, (k["meta_bytes"], k["members"]))):
        assert call(eng, damaged_record(c.known, last, how), c.probes, c.now, device, caps, caps)[0] == N.E_INVAL
        assert call(eng, c.known, damaged_record(c.probes, n_p - 1, how), c.now, device, caps, caps)[0] == N.E_INVAL
    # a set that is not kept is not read: its damage does not fail the call, and the results are those of the image without it
    s = b"\x0a\x0b"
    good = FC.raw_image([(FC.H0, FC.digest(0), [s, b"\x0c"]), (FC.H0 + 5, FC.digest(0), [s, b"\x0d" * 7])])[0]
    p = KI.probes({FC.digest(0): [s, b"\x0c"]})
    now = (FC.H0 + 1) * 3600
    bad = damaged_record(good, 1, how)
    want = TWIN(good, p, now)
    for device, caps in ((False, len(good)), (True, (256, 4))):
        rc, info, hit, miss = call(eng, bad, p, now, device, caps, caps)
        assert rc == 0 and (hit, miss) == want and info.members_read == 2 and info.sets_kept == 1
        assert call(eng, bad, p, now - 1, device, caps, caps)[0] == N.E_INVAL       # … one second earlier the set is kept and read


# ---- 6. more block counts than one tile of the scan

def test_4097_blocks():
    """1 048 577 records in two sets, every third one hit: the block counts cross one SCAN_TILE (4 096), and the second
    set begins inside the last full block.  Built and checked with numpy masks."""
    n, n2 = 4096 * 256 + 1, 1000
    rec = np.zeros(n, KI.MEMBER_DTYPE)
    rec["len"] = 8
    rec["serial"][:, :8] = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).astype(">u8").view(np.uint8).reshape(n, 8)
    mask = np.arange(n) % 3 == 0
    d = FC.digest(0)

    def image(counts, r):
        sets, first = b"", 0
        for hour, cnt in counts:
            if cnt:
                sets += struct.pack("<iIQQ", hour, 0, first, cnt)
                first += cnt
        n_sets = len(sets) // 24
        meta = KI._HEADER.pack(KI.MAGIC, 1, 64, 1 if n_sets else 0, 0, n_sets, first, 0, 0, 0) + (d if n_sets else b"") + sets
        return meta + b"\0" * (-len(meta) % 64), r
    cut = n - n2
    k_meta, k_rec = image([(FC.H0, cut), (FC.H0 + 1, n2)], rec)
    p_meta, p_rec = image([(0, int(mask.sum()))], rec[mask])
    want = [image([(FC.H0, int(m[:cut].sum())), (FC.H0 + 1, int(m[cut:].sum()))], rec[m]) for m in (mask, ~mask)]
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
    try:
        up = lambda r: torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).to(DEV)
        d_k, d_p = up(k_rec), up(p_rec)
        (hm, dh), (mm, dm), info = e.known_image_split_device(k_meta, d_k, p_meta, d_p, FC.INT64_MIN)
        assert info["members_read"] == n and info["hit"]["members"] == int(mask.sum())
        for (meta, d_rec), (w_meta, w_rec) in zip(((hm, dh), (mm, dm)), want):
            assert meta == w_meta
            assert np.array_equal(d_rec.cpu().numpy(), w_rec.view(np.uint8).reshape(-1))
        assert np.array_equal(d_k.cpu().numpy(), k_rec.view(np.uint8).reshape(-1))
    finally:
        e.close()


# ---- 7. read-only; the engine's own sets

def test_nothing_of_the_engine_is_read_or_changed():
    with closing(built_engine()) as (e,):
        e.set_known_order(N.KNOWN_ORDER_SORTED)
        img = e.known_export()
        p = probes_of(img, np.random.default_rng(1))
        before = (state(e), table(e), e.issuer_counts().tobytes(), bytes(e.table_info()))
        other = CASES["host"]
        check(e, other.known, other.probes, other.now)       # another image altogether: the engine's own sets play no part
        hit, miss = check(e, img, p, 0)
        assert image_info(hit)["members"] and image_info(miss)["members"] and image_info(hit)["host_members"]
        assert KI.union(hit, miss) == KI.union(img)
        if KI.union(img) == img:                             # a canonical K: both results are canonical byte for byte
            assert KI.union(hit) == hit and KI.union(miss) == miss
        assert (state(e), table(e), e.issuer_counts().tobytes(), bytes(e.table_info())) == before and e.known_export() == img


def test_known_split_of_the_engine_s_own_sets():
    with closing(built_engine()) as (e,):
        e.set_known_order(N.KNOWN_ORDER_SORTED)
        img = e.known_export()
        p = probes_of(img, np.random.default_rng(2), [(FC.digest(9), b"\x01")])
        hours = sorted({KI.exp_date_span(k.split(b"::")[1])[0] // 3600 for k in KI.parse(img).sets})
        cut = (hours[len(hours) // 2] + 1) * 3600
        for now in (0, cut):
            hit, miss, info = e.known_split(p, now)
            assert (hit, miss) == TWIN(img, p, now) and info["hit"]["members"] > 0
        only, none, _ = e.known_split(p, 0, want=("hit",))
        assert only == TWIN(img, p, 0)[0] and none is None
        # after an expire_sweep the swept sets are gone from the export, and so from both results at an earlier now
        assert e.expire_sweep(cut) > 0
        img2 = e.known_export()
        assert img2 != img
        hit, miss, _ = e.known_split(p, 0)
        assert (hit, miss) == TWIN(img2, p, 0) and hit != TWIN(img, p, 0)[0]
        # after a known_remove of every third member of every set those are in neither result
        e.known_remove(KI.build({k: ms[::3] for k, ms in KI.parse(img2).sets.items()}))
        hit3, miss3, info = e.known_split(p, 0)
        assert (hit3, miss3) == TWIN(e.known_export(), p, 0)
        assert info["hit"]["members"] < image_info(hit)["members"]


# ---- 8. from DER CRLs to both images

DG = CC.DIGESTS


def revoking_engine():
    """An engine that mapped 45 certificates of one issuer, serials of 1..45 octets, under two expiration hours, and
    CRLs of that issuer's that revoke every other one, two serials it does not hold, and one more under another issuer."""
    issuer = synth.issuer(synth.config(n_issuers=1), 0)
    name = D.name(D.rdn(3, b"Synth Issuer 000"))
    serials = [bytes([1 + L % 0x7e]) + bytes((L * 5 + j) % 256 for j in range(L - 1)) for L in range(1, 46)]
    certs = [D.cert(serial=s, issuer=name, not_after=D.utctime("270101000000Z" if k % 2 else "270301000000Z")) for k, s in enumerate(serials)]
    b = Batch.from_certs(certs, [0] * len(certs))
    b.payload = np.concatenate([b.payload, np.zeros(N.PAYLOAD_PAD, np.uint8)])
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
    e.add_issuers([issuer])
    e.set_filter(b"", True, 0)
    assert e.map_batch(b).stats.n_new == len(certs)
    digest = base64.urlsafe_b64decode(e.issuer_id(0))
    revoked = serials[::2] + [b"\x7f" * 9, b"\x7e" * 44] + serials[1::6]
    return e, digest, serials, revoked


def lists_of(e, side, now):
    ids, offs, text = e.known_image_lists_device(side[0], side[1], now)
    text = text.cpu().numpy().tobytes()
    return [(i, text[int(offs[k]):int(offs[k + 1])]) for k, i in enumerate(ids)]


def test_known_revoked_split():
    e, digest, serials, revoked = revoking_engine()
    with closing(e):
        e.set_known_order(N.KNOWN_ORDER_SORTED)
        crls = [CC.crl([CC.entry(s) for s in revoked[:10]]), CC.crl([CC.entry(s) for s in revoked[10:]]), CC.crl([CC.entry(serials[1])])]
        digests = [digest, digest, DG[5]]                        # the last: another issuer's CRL with a serial this one holds
        before = (state(e), table(e), e.issuer_counts().tobytes())
        p = CRL.probes_image(crls, digests)
        img = e.known_export()
        for now in (0, 1803859200):                              # everything kept; the January sets gone
            hit, miss, info = e.known_revoked_split(crls, digests, now)
            want = TWIN(img, p, now)
            assert hit[1].is_cuda and miss[1].is_cuda
            assert (hit[0] + hit[1].cpu().numpy().tobytes(), miss[0] + miss[1].cpu().numpy().tobytes()) == want
            assert info["hit"] == image_info(want[0]) and info["hit"]["members"] > 0 and info["hit"]["host_members"] > 0
            assert lists_of(e, hit, now) == KI.image_lists(want[0], now) and lists_of(e, miss, now) == KI.image_lists(want[1], now)
            lines = {}
            for side in (hit, miss):                             # revoked/<Issuer.ID> plus known/<Issuer.ID>: the lines of the engine's lists
                for i, text in lists_of(e, side, now):
                    lines.setdefault(i, []).extend(text.splitlines())
            assert {i: sorted(v) for i, v in lines.items()} == {i: sorted(t.splitlines()) for i, t in KI.image_lists(img, now)}
        assert (state(e), table(e), e.issuer_counts().tobytes()) == before           # read-only


def test_known_revoked_split_each_with_one_truncated_crl():
    e, digest, serials, revoked = revoking_engine()
    with closing(e):
        e.set_known_order(N.KNOWN_ORDER_SORTED)
        whole = CC.crl([CC.entry(s) for s in serials[1::2]])      # serials the engine holds, in a CRL it must not read
        crls = [CC.crl([CC.entry(s) for s in revoked[:10]]), whole[:-7], CC.crl([CC.entry(s) for s in revoked[10:]])]
        digests = [digest] * 3
        with pytest.raises(CRL.CrlError):
            e.known_revoked_split(crls, digests, 0)
        hit, miss, info, verdicts = e.known_revoked_split(crls, digests, 0, each=True)
        assert [k for k, v in enumerate(verdicts) if v[0] == CRL.NONE] == [0, 2] and verdicts == CRL.probes_each(crls, digests)[2]
        s_hit, s_miss, s_info = e.known_revoked_split([crls[0], crls[2]], [digest] * 2, 0)
        assert info == s_info and hit[0] == s_hit[0] and torch.equal(hit[1], s_hit[1]) and miss[0] == s_miss[0] and torch.equal(miss[1], s_miss[1])
        want = TWIN(e.known_export(), CRL.probes_image([crls[0], crls[2]], [digest] * 2), 0)
        assert (hit[0] + hit[1].cpu().numpy().tobytes(), miss[0] + miss[1].cpu().numpy().tobytes()) == want
        assert lists_of(e, hit, 0) == KI.image_lists(want[0], 0) and lists_of(e, miss, 0) == KI.image_lists(want[1], 0)
