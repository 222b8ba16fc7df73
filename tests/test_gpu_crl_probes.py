"""-m gpu: DER CRLs → a probe image (include/ctmr.h ctmr_crl_probes*; kernels/crl.h).

Expected bytes come from the CPU twin ct_mapreduce_amd/crl.py (tests/test_crl_corpus_cpu.py holds it to the corpus's plain
lists and offsets), never from the code under test; every comparison is exact bytes and runs through both variants at
exact-size buffers, with guard bytes round every buffer.  The device variant's blob lies at a chosen byte phase and is
followed by bytes that would parse — a read past len changes the result instead of faulting.  A call that fails must
leave every buffer as it was and name the CRL and the offset the corpus worked out."""
import base64
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr
from ct_mapreduce_amd import crl as CRL, known_image as KI, synth, _native as N
from ct_mapreduce_amd.engine import Batch
from tests import crl_corpus as CC, der as D
from tests.test_gpu_exchange import DEV
from tests.test_gpu_known_image import state
from tests.test_gpu_known_sort import table

GUARD = 64
TILE = 1024           # the bytes of a mark block (kernels/resp_parse.h RP_TILE); a turn of the block takes 256, a wave 64
DG = CC.DIGESTS
TEMPT = CC.small_crl() + b"".join(CC.entry(CC.serial_of(k, 7)) for k in range(4))
INFO = [f for f, _ in N.KnownImageInfo._fields_ if f != "reserved"]
CINFO = [f for f in CRL.INFO_FIELDS]


@pytest.fixture(scope="module")
def eng():
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)   # no issuer registered: the call needs none
    yield e
    e.close()


def fields(info, cinfo):
    return {f: getattr(info, f) for f in INFO}, {f: getattr(cinfo, f) for f in CINFO}


def expected(crls, digests):
    """→ (the twin's image, what ctmr_known_image_info and ctmr_crl_info shall say)"""
    want, winfo = CRL.probes_parts(crls, digests)
    im = KI._HEADER.unpack_from(want, 0)
    meta = len(want) - 48 * im[6]
    return want, ({"members": im[6], "sets": im[5], "host_members": im[8], "meta_bytes": meta, "image_bytes": len(want), "issuers": im[3]}, winfo)


def operands(crls, n=None):
    blob = b"".join(crls)
    offsets = np.zeros(len(crls) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(c) for c in crls], dtype=np.uint64)
    if n is not None:
        offsets[-1] = n
    return blob, offsets


def call_host(e, crls, digests, cap, n=None, offsets=None):
    """→ (rc, info, cinfo, image or None): the host variant with guards round the image buffer."""
    blob, offs = operands(crls, n)
    offs = offs if offsets is None else np.asarray(offsets, np.uint64)
    info, cinfo = N.KnownImageInfo(), N.CrlInfo()
    buf = np.full(cap + 2 * GUARD, 0xEE, np.uint8)
    rc = e._lib.ctmr_crl_probes(e._h, blob, len(blob) if n is None else n, offs.ctypes.data, len(offs) - 1, b"".join(digests),
                                buf.ctypes.data + GUARD, cap, C.byref(info), C.byref(cinfo))
    assert (buf[:GUARD] == 0xEE).all() and (buf[GUARD + cap:] == 0xEE).all(), "image guards"
    if rc:
        assert (buf == 0xEE).all(), "written on failure"
        return rc, info, cinfo, None
    assert (buf[GUARD + info.image_bytes:] == 0xEE).all()
    return rc, info, cinfo, buf[GUARD:GUARD + info.image_bytes].tobytes()


def call_device(e, crls, digests, meta_cap, members_cap, phase=0, n=None, offsets=None):
    """→ (rc, info, cinfo, image or None): the device variant.  The first n bytes of the CRLs (all by default) are the
    operand; the blob lies `phase` bytes behind a 16-byte boundary, and what follows its n bytes — the rest of the CRLs,
    then TEMPT — would parse."""
    blob, offs = operands(crls, n)
    offs = offs if offsets is None else np.asarray(offsets, np.uint64)
    info, cinfo = N.KnownImageInfo(), N.CrlInfo()
    n = len(blob) if n is None else n
    lead = b"\x30" * (16 + phase)
    raw = np.frombuffer(lead + blob + TEMPT, np.uint8)
    d_s = torch.from_numpy(raw.copy()).to(DEV)
    meta = np.full(meta_cap + 2 * GUARD, 0xEE, np.uint8)
    d_out = torch.full((48 * members_cap + 2 * GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
    assert d_s.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    rc = e._lib.ctmr_crl_probes_device(e._h, C.c_void_p(d_s.data_ptr() + len(lead)), n, offs.ctypes.data, len(offs) - 1, b"".join(digests),
                                       meta.ctypes.data + GUARD, meta_cap, C.c_void_p(d_out.data_ptr() + GUARD), members_cap,
                                       C.byref(info), C.byref(cinfo))
    assert (d_s.cpu().numpy() == raw).all(), "the blob changed"
    rec = d_out.cpu().numpy()
    assert (meta[:GUARD] == 0xEE).all() and (meta[GUARD + meta_cap:] == 0xEE).all(), "meta guards"
    assert (rec[:GUARD] == 0xEE).all() and (rec[GUARD + 48 * members_cap:] == 0xEE).all(), "record guards"
    if rc:
        assert (meta == 0xEE).all() and (rec == 0xEE).all(), "written on failure"
        return rc, info, cinfo, None
    assert (meta[GUARD + info.meta_bytes:] == 0xEE).all() and (rec[GUARD + 48 * info.members:] == 0xEE).all()
    return rc, info, cinfo, meta[GUARD:GUARD + info.meta_bytes].tobytes() + rec[GUARD:GUARD + 48 * info.members].tobytes()


def differ(got, want):
    if got != want:
        assert len(got) == len(want), (len(got), len(want))
        bad = np.nonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[0]
        raise AssertionError("%d bytes differ, first at %d of %d: %r, expected %r" % (
            len(bad), bad[0], len(want), got[max(bad[0] - 20, 0):bad[0] + 28], want[max(bad[0] - 20, 0):bad[0] + 28]))


def check(e, crls, digests, phases=(0,), host=True):
    """Both variants at exact-size buffers against the twin → (the twin's image, the last ctmr_crl_info)."""
    want, winfo = expected(crls, digests)
    cinfo = None
    if host:
        rc, info, cinfo, got = call_host(e, crls, digests, len(want))
        assert rc == 0, (rc, e._lib.ctmr_last_error(e._h), fields(info, cinfo), winfo)
        differ(got, want)
        assert fields(info, cinfo) == winfo
    for phase in phases:
        rc, info, cinfo, got = call_device(e, crls, digests, winfo[0]["meta_bytes"], winfo[0]["members"], phase)
        assert rc == 0, (rc, e._lib.ctmr_last_error(e._h), fields(info, cinfo), winfo)
        differ(got, want)
        assert fields(info, cinfo) == winfo
    return want, cinfo


def rejected(e, crls, digests, crl, offset, phases=(0,), n=None, offsets=None):
    total = sum(len(c) for c in crls)
    cap = 64 + 56 * len(crls) + 48 * (total // 6 + 1) + 64 * total
    rc, _, cinfo, got = call_host(e, crls, digests, cap, n, offsets)
    assert rc == N.E_INVAL and got is None and (cinfo.bad_crl, cinfo.bad_offset) == (crl, offset), (cinfo.bad_crl, cinfo.bad_offset, crl, offset)
    for phase in phases:
        rc, _, cinfo, got = call_device(e, crls, digests, cap, total // 6 + 1, phase, n, offsets)
        assert rc == N.E_INVAL and got is None and (cinfo.bad_crl, cinfo.bad_offset) == (crl, offset), (cinfo.bad_crl, cinfo.bad_offset, crl, offset)


def test_the_struct():
    assert C.sizeof(N.CrlInfo) == 64 and N.CrlInfo.bad_crl.offset == 48 and N.CrlInfo.candidates.offset == 40


# ---- 1. sizes and structure

def test_no_crls_and_no_entries(eng):
    want, _ = check(eng, [], [], phases=range(16))
    assert want == KI.build({})
    for nm, crls, digests, serials in CC.good_cases()[:4]:
        want, cinfo = check(eng, crls, digests, phases=range(16))
        assert want == KI.build({}) and cinfo.empty_crls == 1 and cinfo.entries == 0, nm
    assert eng.crl_probes([], [])[0] == KI.build({})


@pytest.mark.parametrize("case", CC.good_cases()[4:], ids=[c[0] for c in CC.good_cases()[4:]])
def test_the_corpus(case, eng):
    nm, crls, digests, serials = case
    want, cinfo = check(eng, crls, digests, phases=(len(nm) % 16, 0))
    assert cinfo.entries == sum(len(s) for s in serials) and cinfo.candidates >= cinfo.entries + 2 * len(crls)
    by = {}
    for d, ss in zip(digests, serials):
        by.setdefault(d, []).extend(ss)
    assert KI.union(want) == KI.probes({d: ss for d, ss in by.items() if ss})


def test_the_python_surface(eng):
    nm, crls, digests, serials = CC.good_cases()[-1]
    want = CRL.probes_image(crls, digests)
    img, info = eng.crl_probes(crls, digests)
    assert img == want and info["entries"] == sum(map(len, serials)) and info["bad_crl"] == CRL.NONE
    blob, offsets = operands(crls)
    d = torch.from_numpy(np.frombuffer(b"\0" * 5 + blob, np.uint8).copy()).to(DEV)[5:]
    meta, d_rec, info = eng.crl_probes_device(d, offsets, digests)
    assert meta + d_rec.cpu().numpy().tobytes() == want
    for exact in (True, False):                                                   # sized by a first call, and by the bound
        meta, d_rec, info = eng.crl_probes_device(d, offsets, digests, exact=exact)
        assert meta + d_rec.cpu().numpy().tobytes() == want and d_rec.numel() == 48 * info["records"]
    assert eng.crl_probes((blob, offsets), b"".join(digests))[0] == want
    with pytest.raises(CRL.CrlError) as x:
        eng.crl_probes(crls[:2] + [crls[2][:-1]] + crls[3:], digests)
    assert (x.value.crl, x.value.offset) == (2, len(crls[0]) + len(crls[1]))


def test_one_crl_of_70_000_entries(eng):
    """More than 2^16 tokens and more than 2 048 mark tiles: every level of the scans and of the prefix maximum."""
    rng = np.random.default_rng(41)
    ss = [bytes(x) for x in rng.integers(0, 256, size=(70000, 16), dtype=np.uint8)]
    c = CC.crl([CC.entry(s, ext=CC.REASON if k % 8 == 0 else None) for k, s in enumerate(ss)])
    assert len(c) > 2048 * TILE
    want, winfo = expected([c], [DG[0]])
    rc, info, cinfo, got = call_device(eng, [c], [DG[0]], winfo[0]["meta_bytes"], 70000, phase=7)
    assert rc == 0 and fields(info, cinfo) == winfo
    differ(got, want)
    rc, info, cinfo, got = call_host(eng, [c], [DG[0]], len(want))
    assert rc == 0 and fields(info, cinfo) == winfo
    differ(got, want)
    assert KI.records(got)[0] == [(KI.set_key(0, DG[0]), s) for s in ss]


def test_300_crls_of_0_to_3_entries(eng):
    crls, digests, by = [], [], {}
    for k in range(300):
        ss = [CC.serial_of(k * 3 + j, 10 + (k + j) % 35) for j in range(k % 4)]
        crls.append(CC.crl([CC.entry(s) for s in ss] if k % 7 else None if not ss else [CC.entry(s) for s in ss], next_update=k % 2 == 0))
        digests.append(DG[k % 5])
        by.setdefault(DG[k % 5], []).extend(ss)
    want, cinfo = check(eng, crls, digests, phases=(0, 11))
    dev, host = KI.records(want)
    for d in by:
        assert [m for k, m in dev if k == KI.set_key(0, d)] == [s for s in by[d] if len(s) <= 40]
    assert cinfo.empty_crls == sum(1 for k in range(300) if k % 4 == 0)


def test_shards_and_digests_whose_ids_sort_the_other_way(eng):
    a, b = CC.reversed_pair()
    assert a < b and KI.issuer_id(a) > KI.issuer_id(b)
    sa, sb = [CC.serial_of(k, 12) for k in range(5)], [CC.serial_of(40 + k, 13) for k in range(4)]
    crls = [CC.crl([CC.entry(s) for s in sa[:2]]), CC.crl([CC.entry(s) for s in sb[:1]]), CC.crl([CC.entry(s) for s in sa[2:3]]),
            CC.crl([CC.entry(s) for s in sb[1:]]), CC.crl([CC.entry(s) for s in sa[3:]])]
    want, _ = check(eng, crls, [a, b, a, b, a], phases=(0, 3))
    assert KI.parse(want).issuers == [a, b]
    assert KI.records(want)[0] == [(KI.set_key(0, b), s) for s in sb] + [(KI.set_key(0, a), s) for s in sa]
    # the same CRL twice under one digest: its records twice
    want, _ = check(eng, [crls[0], crls[0]], [a, a])
    assert [m for _, m in KI.records(want)[0]] == sa[:2] * 2


def test_known_revoked_on_an_engine_that_mapped_certificates(eng):
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
    crls = [CC.crl([CC.entry(s) for s in revoked[:10]]), CC.crl([CC.entry(s) for s in revoked[10:]]), CC.crl([CC.entry(serials[1])])]
    digests = [digest, digest, DG[5]]                                              # the last: another issuer's CRL with a serial this one holds
    before = (state(e), table(e), e.issuer_counts().tobytes())
    twin = CRL.probes_image(crls, digests)
    assert e.crl_probes(crls, digests)[0] == twin
    for now in (0, 1803859200):                                                    # everything kept; the January sets gone
        p_meta, hits, host_hits = e.known_revoked(crls, digests, now)
        want_hits, want_host = KI.find(e.known_export(), twin, now)
        assert p_meta == twin[:len(p_meta)] and len(p_meta) + 48 * len(hits) == len(twin)
        assert (hits == want_hits).all() and (host_hits == want_host).all()
        assert int((hits["records"] > 0).sum() + (host_hits["records"] > 0).sum()) > 0
    assert (state(e), table(e), e.issuer_counts().tobytes()) == before           # read-only
    e.close()


# ---- 2. tile, turn and wave edges

@pytest.mark.parametrize("which", ["30", "length", "02", "serial length", "17"])
def test_a_header_byte_as_the_last_of_a_tile_a_turn_and_a_wave(which, eng):
    j = ["30", "length", "02", "serial length", "17"].index(which)
    ss = [CC.serial_of(k, 16 + k % 2) for k in range(90)]
    es = [CC.entry(s, ext=CC.REASON if k % 8 == 0 else None) for k, s in enumerate(ss)]
    target = 40
    inside = (0, 1, 2, 3, 4 + len(ss[target]))[j] + sum(len(x) for x in es[:target])
    for edge, unit in ((TILE - 1, TILE), (2 * TILE - 1, TILE), (255, 256), (63, 64)):
        lo1 = CC.crl_at(es, tbs_pad=1)[1]                                         # a pad octet moves the value by one, or by two
        first = 1 + (edge - (lo1 + inside)) % unit                                 # where a length in front of it grows
        first += unit * max(0, -((lo1 + inside + first - 1 - edge) // unit))
        for pad in range(max(first - 16, 1), first + 4):
            c, lo = CC.crl_at(es, tbs_pad=pad)
            if (lo + inside) % unit == edge % unit and lo + inside >= edge:
                break
        else:
            raise AssertionError("no pad")
        assert c[lo + inside] == (0x30, len(es[target]) - 2, 0x02, len(ss[target]), 0x17)[j]
        check(eng, [c], [DG[0]], phases=(0, 15))


# ---- 3. fake entries

@pytest.mark.parametrize("case", CC.fake_cases(), ids=[c[0] for c in CC.fake_cases()])
def test_fake_entries(case, eng):
    nm, spec, start, end = case
    es = [CC.spec_entry(*x) for x in spec]
    c, lo = CC.crl_at(es)
    got = CRL.entry(c, lo + start, lo + sum(map(len, es)))
    assert (got[0] - lo if got else None) == end, nm
    want, cinfo = check(eng, [c], [DG[0]], phases=(0, 6))
    assert [m for _, m in KI.records(want)[0]] == [x[0] for x in spec if len(x[0]) <= 40]
    assert cinfo.candidates - cinfo.entries - 2 >= (end is not None)               # the fake was a candidate, and was thrown out
    check(eng, [c, c], [DG[0], DG[1]], phases=(3,))
    # … and with the value pushed across the tile by a longer issuer
    c2 = CC.crl(es, tbs_pad=1024 - (lo + start) % 1024 + 3)
    check(eng, [c2], [DG[2]], phases=(9,))


def test_a_fake_crl_where_nothing_is_read(eng):
    for nm, c, ss in CC.fake_crl_inside():
        want, cinfo = check(eng, [c], [DG[0]], phases=(0, 5))
        assert [m for _, m in KI.records(want)[0]] == ss and cinfo.candidates == len(ss) + 2, nm


# ---- 4. rejections and sizing

@pytest.mark.parametrize("case", CC.rejections(), ids=[c[0] for c in CC.rejections()])
def test_rejections(case, eng):
    nm, c, offset = case
    with pytest.raises(CRL.CrlError):
        CRL.entries(c)
    rejected(eng, [c], [DG[0]], 0, offset, phases=(0, 5))
    lead = [CC.crl([CC.entry(CC.serial_of(k, 16)) for k in range(30)]), CC.crl(None)]
    assert len(lead[0]) + len(lead[1]) > TILE
    rejected(eng, lead + [c], [DG[1], DG[2], DG[0]], 2, len(lead[0]) + len(lead[1]) + offset)


def test_the_lowest_crl_is_named(eng):
    rej = {nm: (c, off) for nm, c, off in CC.rejections()}
    head, ent = rej["tag 31 for signature"], rej["a fourth TLV in an entry"]
    good = CC.small_crl()
    rejected(eng, [good, ent[0], head[0]], DG[:3], 1, len(good) + ent[1])
    rejected(eng, [good, head[0], ent[0]], DG[:3], 1, len(good) + head[1])
    rejected(eng, [ent[0], good, ent[0]], DG[:3], 0, ent[1])


def test_every_prefix_and_a_slice_of_no_bytes(eng):
    c = CC.small_crl()
    good = CC.crl([CC.entry(b"\x09")])
    for n in range(len(c)):
        rejected(eng, [c], [DG[0]], 0, 0, phases=(n % 16,), n=n)                 # behind n: the rest of the CRL, then TEMPT
        if n % 16 == 1:
            rejected(eng, [good, c], DG[:2], 1, len(good), phases=(n % 16,), n=len(good) + n)
    at = len(good)
    rejected(eng, [good, b"", c], DG[:3], 1, at)
    rejected(eng, [b"", good], DG[:2], 0, 0)
    rejected(eng, [good, c, b""], DG[:3], 2, at + len(c))


def test_offsets_that_do_not_ascend_or_do_not_end_at_len(eng):
    a, b = CC.small_crl(), CC.crl([CC.entry(b"\x09")])
    A, B = len(a), len(b)
    for offsets, bad in (([1, A, A + B], (0, 0)), ([0, A + 1, A], (1, A + 1)), ([0, A, A + B - 1], (2, A + B)), ([0, A, A + B + 1], (2, A + B)),
                         ([0, A + B, A, A + B], (1, A + B))):
        assert CRL.check_offsets(offsets, len(offsets) - 1, A + B) == bad
        rejected(eng, [a, b], DG[:len(offsets) - 1], bad[0], bad[1], offsets=offsets)
    assert CRL.check_offsets([0, A, A + B], 2, A + B) is None


def test_short_buffers(eng):
    nm, crls, digests, serials = [c for c in CC.good_cases() if c[0].startswith("40 next to 41")][0]
    want, winfo = expected(crls, digests)
    assert winfo[0]["host_members"] == 2 and winfo[0]["members"] > 0
    for cap in (len(want) - 1, len(want) - 48, winfo[0]["meta_bytes"], 0):
        rc, info, cinfo, got = call_host(eng, crls, digests, cap)
        assert rc == N.E_RANGE and got is None and fields(info, cinfo) == winfo
    for mc, nc in ((winfo[0]["meta_bytes"] - 1, winfo[0]["members"]), (winfo[0]["meta_bytes"], winfo[0]["members"] - 1), (0, 0)):
        rc, info, cinfo, got = call_device(eng, crls, digests, mc, nc, phase=4)
        assert rc == N.E_RANGE and got is None and fields(info, cinfo) == winfo
    rc, info, cinfo, got = call_device(eng, crls, digests, winfo[0]["meta_bytes"] + 100, len(crls[0]) // 6, phase=4)     # sized by the bound
    assert rc == 0 and got == want


def test_a_length_of_4_gib_is_refused_without_a_read(eng):
    info, cinfo = N.KnownImageInfo(), N.CrlInfo()
    small = CC.small_crl()
    d = torch.from_numpy(np.frombuffer(small, np.uint8).copy()).to(DEV)
    out = np.full(4096, 0xEE, np.uint8)
    d_out = torch.full((4096,), 0xEE, dtype=torch.uint8, device=DEV)
    for n in (1 << 32, (1 << 32) - 64, 1 << 40):
        offsets = np.array([0, n], np.uint64)
        assert eng._lib.ctmr_crl_probes(eng._h, small, n, offsets.ctypes.data, 1, DG[0], out.ctypes.data, 4096, C.byref(info),
                                        C.byref(cinfo)) == N.E_INVAL
        assert eng._lib.ctmr_crl_probes_device(eng._h, C.c_void_p(d.data_ptr()), n, offsets.ctypes.data, 1, DG[0], out.ctypes.data, 4096,
                                               C.c_void_p(d_out.data_ptr()), 64, C.byref(info), C.byref(cinfo)) == N.E_INVAL
    assert (out == 0xEE).all() and (d_out.cpu().numpy() == 0xEE).all()
