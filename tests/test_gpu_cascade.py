"""-m gpu: the filter cascade of a revoked / not-revoked image pair (include/ctmr.h ctmr_cascade_build* /
ctmr_cascade_query*; kernels/cascade.h k_casc_insert / k_casc_test / k_casc_compact / k_casc_query).

The device is held to the CPU twin cascade.build / cascade.query — which tests/test_cascade_cpu.py holds to the
struct.pack-and-hashlib expectation of tests/cascade_corpus.py — exactly, byte for byte, through both variants at
exact-size buffers with guard bytes round every output buffer.  The operands must stay as they were and a call that
fails must leave its buffer as it was.  The shapes are the smallest at which the code can go wrong
(tests/cascade_corpus.py lists them), not the workload's.
"""
import base64
import ctypes as C
import functools
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr
from ct_mapreduce_amd import cascade as CA, crl as CRL, known_image as KI, _native as N
from tests import cascade_corpus as CC, crl_corpus as CRLC, find_corpus as FC
from tests.test_gpu_exchange import DEV
from tests.test_gpu_known_find import closing, parts
from tests.test_gpu_known_image import state
from tests.test_gpu_known_sort import table
from tests.test_gpu_known_split import revoking_engine

CASES = CC.all_cases()
GOOD = [c for c in CASES if c.cascade is not None]
REFUSED = [c for c in CASES if c.cascade is None]
GUARD = 64
FILL = 0xEE


@pytest.fixture(scope="module")
def eng():
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)   # no issuer registered: the calls need none
    yield e
    e.close()


def raw_params(p):
    k1, b1, k2, b2, max_layers, salt = p
    return N.CascadeParams(k1, b1, k2, b2, max_layers, len(salt), (C.c_uint8 * 16)(*salt[:16]))


def on_device(raw):
    d = torch.from_numpy(np.concatenate([raw, np.zeros(32, np.uint8)])).to(DEV)
    assert d.data_ptr() % 16 == 0
    return d


def layer_table(info):
    return [(l.level, l.k, l.m_bits, l.offset, l.n_held) for l in info.layer[:info.layers]]


def build(e, c, device, cap="exact", shift=(0, 0, 0), params=None):
    """One raw call → (rc, info, cascade bytes or None).  cap: "exact" — a buffer of exactly the expected size —, None —
    a null buffer —, or the capacity.  shift: bytes added to the device pointers of R, S and the output.  The operands
    must stay as they were; a call that fails must leave the buffer as it was."""
    if cap == "exact":
        cap = len(c.cascade)
    info = N.CascadeInfo()
    p = raw_params(params or c.params)
    keep = (bytes(bytearray(c.revoked)), bytes(bytearray(c.known)))
    size = (cap or 0) + 2 * GUARD + 16
    if device:
        (r_meta, r_raw, nr), (s_meta, s_raw, ns) = parts(c.revoked), parts(c.known)
        d_r, d_s = on_device(r_raw), on_device(s_raw)
        buf = torch.full((size,), FILL, dtype=torch.uint8, device=DEV)
        assert (buf.data_ptr() + GUARD) % 16 == 0
        rc = e._lib.ctmr_cascade_build_device(
            e._h, r_meta, len(r_meta), C.c_void_p(d_r.data_ptr() + shift[0]) if nr else None, nr, s_meta, len(s_meta),
            C.c_void_p(d_s.data_ptr() + shift[1]) if ns else None, ns, int(c.now), C.byref(p),
            None if cap is None else C.c_void_p(buf.data_ptr() + GUARD + shift[2]), cap or 0, C.byref(info))
        assert (d_r.cpu().numpy()[:len(r_raw)] == r_raw).all() and (d_s.cpu().numpy()[:len(s_raw)] == s_raw).all()
        buf = buf.cpu().numpy()
    else:
        buf = np.full(size, FILL, np.uint8)
        rc = e._lib.ctmr_cascade_build(e._h, c.revoked, len(c.revoked), c.known, len(c.known), int(c.now), C.byref(p),
                                       None if cap is None else buf.ctypes.data + GUARD, cap or 0, C.byref(info))
    assert (c.revoked, c.known) == keep, "an operand changed"
    if rc:
        assert (buf == FILL).all(), "written on failure"
        return rc, info, None
    assert (buf[:GUARD] == FILL).all() and (buf[GUARD + info.bytes:] == FILL).all(), "written outside the cascade"
    return rc, info, buf[GUARD:GUARD + info.bytes].tobytes()


def check_info(info, c):
    assert layer_table(info) == c.layers and info.layers == len(c.layers) and info.bytes == len(c.cascade)
    assert (info.r_records, info.s_records) == (len(c.r_keys), len(c.s_keys))
    assert (info.r_host_skipped, info.s_host_skipped) == (c.r_host, c.s_host) and info.left == 0
    tested = len(c.layers) - (1 if c.layers and c.layers[-1][0] == 1 and not c.s_keys else 0)
    assert info.syncs == 1 + (tested if c.r_keys else bool(c.s_keys))


# ---- 1. equality with the twin (and so with the corpus), both variants

@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("family", sorted(CC.FAMILIES))
def test_the_device_builds_the_twin_s_cascade_byte_for_byte(eng, family, device):
    for c in (c for c in GOOD if c.family == family):
        want, twin_info = CA.build_info(c.revoked, c.known, c.now, CA.Params(*c.params))
        assert want == c.cascade
        rc, info, got = build(eng, c, device)
        assert rc == 0, (c.name, eng._lib.ctmr_last_error(eng._h))
        assert got == want, c.name
        check_info(info, c)
        assert layer_table(info) == twin_info["layer"]


# ---- 2. sizing and buffer errors

@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_a_null_or_short_buffer_sizes_without_writing(eng, device):
    for c in (c for c in GOOD if c.name in ("sizes-257-257", "sizes-0-0", "sizes-65-0", "lengths-salt-7")):
        for cap in (None, 0, len(c.cascade) - 1, 63):
            rc, info, _ = build(eng, c, device, cap)
            assert rc == N.E_RANGE
            check_info(info, c)
        rc, info, got = build(eng, c, device, len(c.cascade) + 128)
        assert rc == 0 and got == c.cascade


def test_misaligned_device_pointers_are_refused(eng):
    c = next(c for c in GOOD if c.name == "sizes-65-65")
    for shift in ((8, 0, 0), (0, 4, 0), (0, 0, 8), (1, 0, 0)):
        assert build(eng, c, True, shift=shift)[0] == N.E_INVAL
    want = CA.query(c.cascade, c.known)
    for shift in ((8, 0, 0), (0, 8, 0), (0, 0, 4)):
        assert query(eng, c.cascade, c.known, True, shift=shift)[0] == N.E_INVAL
    assert query(eng, c.cascade, c.known, True)[2] == want


# ---- 3. refusals

@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_every_refusal_of_the_corpus_is_einval_and_writes_nothing(eng, device):
    assert len(REFUSED) >= 15
    for c in REFUSED:
        rc, info, _ = build(eng, c, device, 1 << 16)
        assert rc == N.E_INVAL, c.name
        assert info.left == c.left, c.name
        if c.notes.get("bad_record"):
            assert b"member record" in eng._lib.ctmr_last_error(eng._h)


def test_a_first_layer_of_2_32_bits_is_refused_before_anything_is_built(eng):
    """One kept set of 2^24 all-zero records (empty serials: valid, and repeats are allowed) at 65 536/256 bits each is
    a layer of 2^32 bits: CTMR_E_INVAL, the buffer untouched; the twin's size step refuses the same."""
    n = 1 << 24
    meta = KI._HEADER.pack(KI.MAGIC, KI.VERSION, KI.HEADER_BYTES, 1, 0, 1, n, 0, 0, 0) + FC.digest(0) + KI._SET.pack(FC.H0, 0, 0, n)
    meta += b"\0" * (-len(meta) % 64)
    s_meta = KI._HEADER.pack(KI.MAGIC, KI.VERSION, KI.HEADER_BYTES, 0, 0, 0, 0, 0, 0, 0)
    d_r = torch.zeros(48 * n, dtype=torch.uint8, device=DEV)
    buf = torch.full((4096,), FILL, dtype=torch.uint8, device=DEV)
    info = N.CascadeInfo()
    p = raw_params((1, 65536, 1, 370, 4, b""))
    rc = eng._lib.ctmr_cascade_build_device(eng._h, meta, len(meta), C.c_void_p(d_r.data_ptr()), n, s_meta, len(s_meta), None, 0,
                                            FC.INT64_MIN, C.byref(p), C.c_void_p(buf.data_ptr()), 4096, C.byref(info))
    assert rc == N.E_INVAL and b"bits" in eng._lib.ctmr_last_error(eng._h)
    assert info.r_records == n and info.layers == 0 and info.syncs == 0
    assert bool((buf == FILL).all())
    with pytest.raises(CA.CascadeError):
        CA.layer_shape(n, 1, CA.Params(1, 65536, 1, 370, 4, b""))
    # the same operand one step below the limit is sized, not refused: 2^32 - 2^16 bits in one layer, no test (S is empty)
    p = raw_params((1, 65535, 1, 370, 4, b""))
    rc = eng._lib.ctmr_cascade_build_device(eng._h, meta, len(meta), C.c_void_p(d_r.data_ptr()), n, s_meta, len(s_meta), None, 0,
                                            FC.INT64_MIN, C.byref(p), None, 0, C.byref(info))
    assert rc == N.E_RANGE and layer_table(info) == [(1, 1, 2 ** 32 - 2 ** 16, 128, n)] and info.bytes == 128 + (2 ** 32 - 2 ** 16) // 8
    assert bool((buf == FILL).all())


# ---- 4. small runs

@pytest.mark.parametrize("chunk", (1, 100, 300))
def test_small_runs_give_the_same_bytes(eng, chunk):
    os.environ["CTMR_CASCADE_CHUNK"] = str(chunk)
    try:
        for c in (c for c in GOOD if c.family == "sizes"):
            rc, info, got = build(eng, c, True)
            assert rc == 0 and got == c.cascade, c.name
            check_info(info, c)
            assert query(eng, c.cascade, c.known, True)[2] == CA.query(c.cascade, c.known), c.name
    finally:
        del os.environ["CTMR_CASCADE_CHUNK"]


# ---- 5. the query

def query(e, cascade, probes, device, cap=None, shift=(0, 0, 0)):
    """One raw call → (rc, info, answers or None), guard bytes round the answers."""
    n = e._header_counts(probes)[0]
    cap = n if cap is None else cap
    info = N.CascadeQueryInfo()
    size = cap + 2 * GUARD + 16
    if device:
        p_meta, p_raw, npr = parts(probes)
        d_p = on_device(p_raw)
        d_c = on_device(np.frombuffer(cascade, np.uint8))
        buf = torch.full((size,), FILL, dtype=torch.uint8, device=DEV)
        rc = e._lib.ctmr_cascade_query_device(e._h, C.c_void_p(d_c.data_ptr() + shift[0]), len(cascade), p_meta, len(p_meta),
                                              C.c_void_p(d_p.data_ptr() + shift[1]) if npr else None, npr,
                                              C.c_void_p(buf.data_ptr() + GUARD + shift[2]), cap, C.byref(info))
        assert d_c.cpu().numpy()[:len(cascade)].tobytes() == cascade and (d_p.cpu().numpy()[:len(p_raw)] == p_raw).all()
        buf = buf.cpu().numpy()
    else:
        buf = np.full(size, FILL, np.uint8)
        rc = e._lib.ctmr_cascade_query(e._h, cascade, len(cascade), probes, len(probes), buf.ctypes.data + GUARD, cap, C.byref(info))
    if rc:
        assert (buf == FILL).all(), "written on failure"
        return rc, info, None
    assert (buf[:GUARD] == FILL).all() and (buf[GUARD + n:] == FILL).all(), "written outside the answers"
    return rc, info, buf[GUARD:GUARD + n].tobytes()


def strangers(c):
    """A probe image of records in neither operand: every serial of R with one octet more, under R's issuers and a new one"""
    dev = KI._sections(c.revoked)[0]
    by = {}
    for k, (_, ident, m) in enumerate(dev[:200]):
        if len(m) < 40:
            by.setdefault(FC.digest(7) if k % 3 == 0 else base64.urlsafe_b64decode(ident), set()).add(m + b"\x99")
    return KI.probes({d: sorted(ms) for d, ms in by.items()}) if by else None


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("family", sorted(set(CC.FAMILIES) - {"refusals"}))
def test_the_query_equals_the_twin_s(eng, family, device):
    for c in (c for c in GOOD if c.family == family and not c.name.endswith("bad-record")):
        for image in (c.revoked, c.known, strangers(c)):
            if image is None:
                continue
            rc, info, got = query(eng, c.cascade, image, device)
            assert rc == 0, (c.name, eng._lib.ctmr_last_error(eng._h))
            assert got == CA.query(c.cascade, image), c.name
            assert info.probes == len(got) and info.layers == len(c.layers)
            assert info.host_probes == KI._HEADER.unpack_from(image, 0)[8]
        # all of R's kept records answer 1 and all of S's 0: here every set of these cases that is queried whole
        if c.now == FC.INT64_MIN:
            assert query(eng, c.cascade, c.revoked, device)[2] == b"\1" * len(c.r_keys)
            assert query(eng, c.cascade, c.known, device)[2] == b"\0" * len(c.s_keys)


def test_a_cascade_of_the_device_is_queried_by_the_twin_and_the_reverse(eng):
    c = next(c for c in GOOD if c.name == "sizes-1025-1025")
    _, _, built = build(eng, c, True)
    twin = CA.build(c.revoked, c.known, c.now, CA.Params(*c.params))
    assert CA.query(built, c.revoked) == b"\1" * 1025 and CA.query(built, c.known) == b"\0" * 1025
    for device in (False, True):
        assert query(eng, twin, c.revoked, device)[2] == b"\1" * 1025 and query(eng, twin, c.known, device)[2] == b"\0" * 1025


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_a_damaged_cascade_and_a_short_answer_buffer_are_refused(eng, device):
    damaged, good = CC.damaged()
    for name, b in damaged:
        if device and len(b) < 64:
            continue      # (the device variant is handed device memory of the length it is told)
        assert query(eng, b, good.revoked, device)[0] == N.E_INVAL, name
    rc, info, _ = query(eng, good.cascade, good.revoked, device, cap=len(good.r_keys) - 1)
    assert rc == N.E_RANGE and info.probes == len(good.r_keys)
    bad = bytearray(good.known)
    struct.pack_into("<Q", bad, len(bad) - 48, 41)
    assert query(eng, good.cascade, bytes(bad), device)[0] == N.E_INVAL


# ---- 6. a larger case: the block counts of one test pass cross a scan tile

@functools.lru_cache(1)
def larger():
    """262 145 / 1 048 577 records — 4 097 blocks on the S side — built with numpy: 8-octet serials that are distinct by
    their first four octets, R under two issuers and S under three."""
    n_r, n_s = 262_145, 1_048_577
    rng = np.random.default_rng(29)
    rec = np.zeros(n_r + n_s, KI.MEMBER_DTYPE)
    rec["len"] = 8
    rec["serial"][:, :4] = rng.permutation(n_r + n_s).astype("<u4").view(np.uint8).reshape(-1, 4)
    rec["serial"][:, 4:8] = rng.integers(0, 256, size=(n_r + n_s, 4), dtype=np.uint8)

    def image(r, cuts, digests):
        dg = sorted(digests)
        sets = [KI._SET.pack(FC.H0, k, cuts[k], cuts[k + 1] - cuts[k]) for k in range(len(dg))]
        meta = KI._HEADER.pack(KI.MAGIC, KI.VERSION, KI.HEADER_BYTES, len(dg), 0, len(dg), len(r), 0, 0, 0) + b"".join(dg) + b"".join(sets)
        return meta + b"\0" * (-len(meta) % 64) + r.tobytes()
    revoked = image(rec[:n_r], [0, 100_000, n_r], [FC.digest(0), FC.digest(1)])
    known = image(rec[n_r:], [0, 300_001, 700_000, n_s], [FC.digest(0), FC.digest(1), FC.digest(2)])
    return revoked, known


def test_a_larger_case_equals_the_twin_and_has_the_property(eng):
    revoked, known = larger()
    p = CA.crlite_params(262_145, 1_048_577, b"larger")
    want = CA.build(revoked, known, FC.INT64_MIN, p)
    d_c, info = eng.cascade_build_device(*[x for img in (revoked, known) for x in (parts(img)[0], on_device(parts(img)[1])[:-32])],
                                         FC.INT64_MIN, p)
    assert d_c.cpu().numpy().tobytes() == want
    assert info["layer"] == CA.parse(want)["layers"] and info["layers"] >= 3
    for img, bit in ((revoked, 1), (known, 0)):
        meta, raw, n = parts(img)
        got, _ = eng.cascade_query_device(d_c, meta, on_device(raw)[:-32])
        assert (got.cpu().numpy() == bit).all() and len(got) == n


# ---- 7. the engine is not touched

def test_the_engine_s_state_is_unchanged_by_a_build_and_a_query():
    e, digest, serials, revoked = revoking_engine()
    with closing(e):
        e.set_known_order(N.KNOWN_ORDER_SORTED)
        before = (state(e), table(e), e.issuer_counts().tobytes(), e.known_export())
        c = next(c for c in GOOD if c.name == "sizes-257-257")
        out, info = e.cascade_build(c.revoked, c.known, c.now, CA.Params(*c.params))
        assert out == c.cascade and info["layer"] == c.layers
        assert e.cascade_query(out, c.revoked)[0].tobytes() == b"\1" * 257
        assert (state(e), table(e), e.issuer_counts().tobytes(), e.known_export()) == before


# ---- 8. from DER CRLs to the cascade

def test_known_revoked_cascade_end_to_end():
    e, digest, serials, revoked = revoking_engine()
    with closing(e):
        e.set_known_order(N.KNOWN_ORDER_SORTED)
        whole = CRLC.crl([CRLC.entry(s) for s in serials[1::2]])
        crls = [CRLC.crl([CRLC.entry(s) for s in revoked[:10]]), whole[:-7], CRLC.crl([CRLC.entry(s) for s in revoked[10:]])]
        digests = [digest] * 3
        good = [crls[0], crls[2]]
        img = e.known_export()
        with pytest.raises(CRL.CrlError):
            e.known_revoked_cascade(crls, digests, 0)
        for now in (0, 1803859200):                              # everything kept; the January sets gone
            hit, miss = KI.split(img, CRL.probes_image(good, [digest] * 2), now)
            n_hit, n_miss = (KI._HEADER.unpack_from(x, 0)[6] for x in (hit, miss))
            p = CA.crlite_params(n_hit, n_miss)
            want = CA.build(hit, miss, now, p)
            d_c, info, verdicts = e.known_revoked_cascade(crls, digests, now, each=True)
            assert d_c.is_cuda and d_c.cpu().numpy().tobytes() == want
            assert [k for k, v in enumerate(verdicts) if v[0] == CRL.NONE] == [0, 2]
            twin = CA.build_info(hit, miss, now, p)[1]
            assert n_hit > 0 and (n_miss > 0) == (now == 0) and KI._HEADER.unpack_from(hit, 0)[8] > 0     # (later: all that is left is revoked)
            assert {f: info[f] for f in twin} == twin and info["r_host_skipped"] == KI._HEADER.unpack_from(hit, 0)[8]
            plain, _ = e.known_revoked_cascade(good, [digest] * 2, now, params=CA.Params(2, 1000, 1, 400, 40, b"other"))
            assert plain.cpu().numpy().tobytes() == CA.build(hit, miss, now, CA.Params(2, 1000, 1, 400, 40, b"other"))
            # the engine's export queried with the cascade: of the records of kept sets exactly the split's HIT says 1
            k_meta, k_raw, nk = parts(img)
            got = e.cascade_query_device(d_c, k_meta, on_device(k_raw)[:-32])[0].cpu().numpy()
            assert got.tobytes() == e.cascade_query(want, img)[0].tobytes() == CA.query(want, img)
            in_hit = {(ident, m) for _, ident, m in KI._sections(hit)[0]}
            dev = KI._sections(img)[0]
            kept = [FC.kept(h, now) for h, _, _ in dev]
            assert [bool(g) for g, k in zip(got, kept) if k] == [(ident, m) in in_hit for (_, ident, m), k in zip(dev, kept) if k]
            assert sum(g for g, k in zip(got, kept) if k) == n_hit
