"""-m gpu: DER CRLs → a probe image with a verdict per CRL (include/ctmr.h ctmr_crl_probes_each*; kernels/crl.h
k_crl_head<true>, k_crl_chain, k_crl_class<true>).

The harness is that of tests/test_gpu_crl_probes.py: expected bytes come from the CPU twin ct_mapreduce_amd/crl.py
probes_each (tests/test_crl_each_cpu.py holds it to the corpus's offsets), every comparison is exact and runs through both
variants at exact-size buffers, with guard bytes round the image or the meta and the records, and round `verdicts`.  The
device variant's blob lies at a chosen byte phase and is followed by bytes that would parse.  A call that fails must leave
every buffer, `verdicts` included, as it was."""
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
from tests import test_crl_each_cpu as EC
from tests import test_gpu_crl_probes as STRICT
from tests.test_gpu_exchange import DEV
from tests.test_gpu_known_image import state
from tests.test_gpu_known_sort import table

GUARD = STRICT.GUARD
TILE = STRICT.TILE
DG = CC.DIGESTS
NONE = CRL.NONE
REJ = EC.REJ
VERDICT = np.dtype([("bad_offset", "<u8"), ("records", "<u4"), ("long_entries", "<u4")])
fields, differ, operands = STRICT.fields, STRICT.differ, STRICT.operands


@pytest.fixture(scope="module")
def eng():
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)   # no issuer registered: the call needs none
    yield e
    e.close()


def expected(crls, digests):
    """→ (the twin's image, what ctmr_known_image_info and ctmr_crl_info shall say, the verdicts)"""
    want, winfo, verdicts = CRL.probes_each(crls, digests)
    im = KI._HEADER.unpack_from(want, 0)
    meta = len(want) - 48 * im[6]
    return want, ({"members": im[6], "sets": im[5], "host_members": im[8], "meta_bytes": meta, "image_bytes": len(want), "issuers": im[3]}, winfo), verdicts


class Verdicts:
    """A ctmr_crl_verdict[n] between guards."""

    def __init__(self, n, null=False):
        self.n, self.null = n, null
        self.buf = np.full(16 * n + 2 * GUARD, 0xEE, np.uint8)
        self.ptr = None if null else self.buf.ctypes.data + GUARD

    def read(self, rc):
        assert (self.buf[:GUARD] == 0xEE).all() and (self.buf[GUARD + 16 * self.n:] == 0xEE).all(), "verdict guards"
        if rc or self.null:
            assert (self.buf == 0xEE).all(), "verdicts written"
            return None
        return [tuple(int(x) for x in v) for v in self.buf[GUARD:GUARD + 16 * self.n].view(VERDICT)]


def call_host(e, crls, digests, cap, n=None, offsets=None, null=False):
    """→ (rc, info, cinfo, image or None, verdicts or None): the host variant with guards round the image and the verdicts."""
    blob, offs = operands(crls, n)
    offs = offs if offsets is None else np.asarray(offsets, np.uint64)
    info, cinfo, v = N.KnownImageInfo(), N.CrlInfo(), Verdicts(len(offs) - 1, null)
    buf = np.full(cap + 2 * GUARD, 0xEE, np.uint8)
    rc = e._lib.ctmr_crl_probes_each(e._h, blob, len(blob) if n is None else n, offs.ctypes.data, len(offs) - 1, b"".join(digests),
                                     buf.ctypes.data + GUARD, cap, C.byref(info), C.byref(cinfo), v.ptr)
    assert (buf[:GUARD] == 0xEE).all() and (buf[GUARD + cap:] == 0xEE).all(), "image guards"
    verdicts = v.read(rc)
    if rc:
        assert (buf == 0xEE).all(), "written on failure"
        return rc, info, cinfo, None, None
    assert (buf[GUARD + info.image_bytes:] == 0xEE).all()
    return rc, info, cinfo, buf[GUARD:GUARD + info.image_bytes].tobytes(), verdicts


def call_device(e, crls, digests, meta_cap, members_cap, phase=0, n=None, offsets=None, null=False):
    """→ (rc, info, cinfo, image or None, verdicts or None): the device variant.  The first n bytes of the CRLs (all by
    default) are the operand; the blob lies `phase` bytes behind a 16-byte boundary, and what follows its n bytes — the
    rest of the CRLs, then TEMPT — would parse."""
    blob, offs = operands(crls, n)
    offs = offs if offsets is None else np.asarray(offsets, np.uint64)
    info, cinfo, v = N.KnownImageInfo(), N.CrlInfo(), Verdicts(len(offs) - 1, null)
    n = len(blob) if n is None else n
    lead = b"\x30" * (16 + phase)
    raw = np.frombuffer(lead + blob + STRICT.TEMPT, np.uint8)
    d_s = torch.from_numpy(raw.copy()).to(DEV)
    meta = np.full(meta_cap + 2 * GUARD, 0xEE, np.uint8)
    d_out = torch.full((48 * members_cap + 2 * GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
    assert d_s.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    rc = e._lib.ctmr_crl_probes_each_device(e._h, C.c_void_p(d_s.data_ptr() + len(lead)), n, offs.ctypes.data, len(offs) - 1,
                                            b"".join(digests), meta.ctypes.data + GUARD, meta_cap, C.c_void_p(d_out.data_ptr() + GUARD),
                                            members_cap, C.byref(info), C.byref(cinfo), v.ptr)
    assert (d_s.cpu().numpy() == raw).all(), "the blob changed"
    rec = d_out.cpu().numpy()
    assert (meta[:GUARD] == 0xEE).all() and (meta[GUARD + meta_cap:] == 0xEE).all(), "meta guards"
    assert (rec[:GUARD] == 0xEE).all() and (rec[GUARD + 48 * members_cap:] == 0xEE).all(), "record guards"
    verdicts = v.read(rc)
    if rc:
        assert (meta == 0xEE).all() and (rec == 0xEE).all(), "written on failure"
        return rc, info, cinfo, None, None
    assert (meta[GUARD + info.meta_bytes:] == 0xEE).all() and (rec[GUARD + 48 * info.members:] == 0xEE).all()
    return rc, info, cinfo, meta[GUARD:GUARD + info.meta_bytes].tobytes() + rec[GUARD:GUARD + 48 * info.members].tobytes(), verdicts


def check(e, crls, digests, phases=(0,), host=True, bad=None):
    """Both variants at exact-size buffers against the twin → (the twin's image, its verdicts, the last ctmr_crl_info).
    bad: the CRLs the caller expects to be refused, held against the twin's verdicts first."""
    want, winfo, wverdicts = expected(crls, digests)
    if bad is not None:
        assert [k for k, v in enumerate(wverdicts) if v[0] != NONE] == sorted(bad)
    cinfo = None
    for phase in ([None] if host else []) + list(phases):
        if phase is None:
            rc, info, cinfo, got, verdicts = call_host(e, crls, digests, len(want))
        else:
            rc, info, cinfo, got, verdicts = call_device(e, crls, digests, winfo[0]["meta_bytes"], winfo[0]["members"], phase)
        assert rc == 0, (phase, rc, e._lib.ctmr_last_error(e._h), fields(info, cinfo), winfo)
        differ(got, want)
        assert fields(info, cinfo) == winfo, phase
        assert verdicts == wverdicts, (phase, [(k, a, b) for k, (a, b) in enumerate(zip(verdicts, wverdicts)) if a != b][:4])
    return want, wverdicts, cinfo


# ---- 1. with nothing bad: the strict call, bit for bit

def same_as_strict(e, crls, digests, phase, host):
    want, winfo, wverdicts = expected(crls, digests)
    assert all(v[0] == NONE for v in wverdicts)
    rc, info, cinfo, got, verdicts = call_device(e, crls, digests, winfo[0]["meta_bytes"], winfo[0]["members"], phase)
    src, sinfo, scinfo, sgot = STRICT.call_device(e, crls, digests, winfo[0]["meta_bytes"], winfo[0]["members"], phase)
    assert rc == src == 0 and got == sgot and verdicts == wverdicts
    assert bytes(info) == bytes(sinfo) and bytes(cinfo) == bytes(scinfo)          # every field, `candidates` included
    differ(got, want)
    assert fields(info, cinfo) == winfo
    if host:
        rc, info, cinfo, got, verdicts = call_host(e, crls, digests, len(want))
        src, sinfo, scinfo, sgot = STRICT.call_host(e, crls, digests, len(want))
        assert rc == src == 0 and got == sgot == want and verdicts == wverdicts
        assert bytes(info) == bytes(sinfo) and bytes(cinfo) == bytes(scinfo)


@pytest.mark.parametrize("case", CC.good_cases(), ids=[c[0] for c in CC.good_cases()])
def test_the_good_corpus_is_the_strict_call_bit_for_bit(case, eng):
    nm, crls, digests, serials = case
    same_as_strict(eng, crls, digests, len(nm) % 16, host=sum(map(len, crls)) < 1 << 20)


def test_the_fake_entry_corpus_is_the_strict_call_bit_for_bit(eng):
    for nm, spec, start, end in CC.fake_cases():
        c = CC.crl([CC.spec_entry(*x) for x in spec])
        same_as_strict(eng, [c, c], [DG[0], DG[1]], len(nm) % 16, host=True)
    assert eng.crl_probes_each([], []) == (KI.build({}), eng.crl_probes([], [])[1], [])


# ---- 2. bad CRLs among good ones

@pytest.mark.parametrize("case", CC.rejections(), ids=[c[0] for c in CC.rejections()])
def test_a_rejection_as_the_first_a_middle_and_the_last_of_five(case, eng):
    nm, c, offset = case
    four = CRL.probes_image(*EC.good_four())
    for k in (0, 2, 4):
        crls, digests = EC.five(c, k)
        want, verdicts, cinfo = check(eng, crls, digests, phases=((k + len(nm)) % 16,), bad=[k])
        assert want == four and verdicts[k] == (EC.starts(crls)[k] + offset, 0, 0)    # the offset the corpus worked out
        assert (cinfo.bad_crl, cinfo.bad_offset) == (k, verdicts[k][0])


def test_two_head_refused_crls_in_one_wave_of_the_head(eng):
    a, b = REJ["tag 31 for signature"], REJ["a TLV behind crlExtensions"]
    crls, digests = EC.good_four()
    crls, digests = [crls[0], a[0], crls[2], b[0], crls[3]], [DG[1], DG[1], DG[1], DG[5], DG[3]]
    at = EC.starts(crls)
    want, verdicts, cinfo = check(eng, crls, digests, phases=(0, 9), bad=[1, 3])
    assert (verdicts[1][0], verdicts[3][0]) == (at[1] + a[1], at[3] + b[1]) and cinfo.bad_crl == 1


def test_two_entry_refused_crls_in_one_tile_and_one_chain_wave(eng):
    """Three CRLs of three entries: 15 tokens, all in the first 1 024-byte tile of the mark pass and in the first wave of
    the chain check.  The first and the third are bad by an entry one byte short.  A chain check that reduced its
    findings over the wave to the lowest, as the strict call's does, would blame the first alone and let the third's
    records through."""
    short0, short1 = REJ["entry0 one byte short"], REJ["entry1 one byte short"]
    crls = [short1[0], CC.small_crl(), short0[0]]
    assert sum(map(len, crls)) <= TILE and 3 * (2 + 3) < 64
    at = EC.starts(crls)
    want, verdicts, _ = check(eng, crls, DG[:3], phases=(0,), bad=[0, 2])
    assert verdicts == [(at[0] + short1[1], 0, 0), (NONE, 3, 0), (at[2] + short0[1], 0, 0)]
    assert [m for _, m in KI.records(want)[0]] == CC.SMALL_SERIALS


def test_a_head_refused_and_an_entry_refused_crl_in_one_call(eng):
    head, ent = REJ["length of issuer in the form 80"], REJ["a fourth TLV in an entry"]
    good = CC.small_crl()
    for crls in ([good, head[0], ent[0]], [ent[0], good, head[0]], [head[0], ent[0], good]):
        want, verdicts, _ = check(eng, crls, DG[:3], phases=(5,), bad=[k for k, c in enumerate(crls) if c != good])
        assert [m for _, m in KI.records(want)[0]] == CC.SMALL_SERIALS


def test_all_crls_bad_is_ok_and_the_empty_image(eng):
    bad = [REJ["tag 31 for signature"], REJ["a fourth TLV in an entry"], REJ["entry2 one byte short"], (b"", 0),
           REJ["a byte behind the CertificateList"]]
    want, verdicts, cinfo = check(eng, [c for c, _ in bad], DG[:5], phases=(0, 3), bad=range(5))
    assert want == KI.build({}) and (cinfo.entries, cinfo.empty_crls, cinfo.bad_crl) == (0, 0, 0)
    assert [v[0] for v in verdicts] == [a + off for a, (_, off) in zip(EC.starts([c for c, _ in bad]), bad)]


@pytest.mark.parametrize("shape", list(EC.ZERO_SHAPES), ids=list(EC.ZERO_SHAPES))
def test_crls_of_0_bytes(shape, eng):
    """A CRL of 0 bytes has no byte and so no token: the records in front of it are those in front of the CRL behind it."""
    where = EC.ZERO_SHAPES[shape]
    if where is None:                                                            # n > 0 with len == 0: no launch at all
        for n in (1, 3):
            want, verdicts, cinfo = check(eng, [b""] * n, DG[:n], phases=(0, 7), bad=range(n))
            assert want == KI.build({}) and verdicts == [(0, 0, 0)] * n and (cinfo.bad_crl, cinfo.bad_offset, cinfo.candidates) == (0, 0, 0)
        return
    crls, digests = EC.good_four()
    for k in where:
        crls, digests = crls[:k] + [b""] + crls[k:], digests[:k] + [DG[1]] + digests[k:]
    want, verdicts, _ = check(eng, crls, digests, phases=(0, 13), bad=where)
    at = EC.starts(crls)
    assert want == CRL.probes_image(*EC.good_four()) and all(verdicts[k] == (at[k], 0, 0) for k in where)


def test_a_bad_crl_that_holds_a_41_octet_serial(eng):
    long, at = EC.long_then_broken()
    good = CC.crl([CC.entry(b"\x43" * 41), CC.entry(b"\x08")])
    want, verdicts, cinfo = check(eng, [good, long, good], [DG[0], DG[0], DG[1]], phases=(0, 2), bad=[1])
    assert verdicts == [(NONE, 1, 1), (len(good) + at, 0, 0), (NONE, 1, 1)]
    assert [m for _, m in KI.records(want)[1]] == [b"\x43" * 41] * 2 and cinfo.host_members == 2


def test_a_bad_shard_between_two_good_shards_and_a_bad_crl_alone_under_its_digest(eng):
    a, b = CC.reversed_pair()
    assert a < b and KI.issuer_id(a) > KI.issuer_id(b)
    ent = REJ["entry1 one byte long"]
    sa, sb = [CC.serial_of(k, 12) for k in range(5)], [CC.serial_of(40 + k, 13) for k in range(3)]
    shards = [CC.crl([CC.entry(s) for s in sa[:2]]), ent[0], CC.crl([CC.entry(s) for s in sa[2:]])]
    want, _, _ = check(eng, shards + [CC.crl([CC.entry(s) for s in sb])], [a, a, a, b], phases=(0, 3), bad=[1])
    assert KI.records(want)[0] == [(KI.set_key(0, b), s) for s in sb] + [(KI.set_key(0, a), s) for s in sa]
    # … and alone under a digest, on either side of the ID order: that digest is no issuer of the image
    for dg in ([a, b, a], [b, a, b]):
        want, _, _ = check(eng, [shards[0], ent[0], shards[2]], dg, phases=(6,), bad=[1])
        assert KI.parse(want).issuers == [dg[0]] and [m for _, m in KI.records(want)[0]] == sa


def test_a_crl_broken_behind_its_1025th_entry(eng):
    ss = [CC.serial_of(k, 16 + k % 2) for k in range(1025)]
    es = [CC.entry(s, ext=CC.REASON if k % 8 == 0 else None) for k, s in enumerate(ss)]
    c, lo = CC.crl_at(es + [b"\x30\x03\x02\x01"])
    good = CC.crl(es[:70])
    assert len(c) > 16 * TILE
    want, verdicts, cinfo = check(eng, [good, c, good], DG[:3], phases=(0, 11), bad=[1])
    assert verdicts[1] == (len(good) + lo + sum(map(len, es)), 0, 0) and cinfo.records == 140
    assert cinfo.candidates >= 1025 + 140 + 6                                    # the bad CRL's entries were candidates, and tokens


def test_a_fake_entry_region_inside_a_bad_crl(eng):
    for nm, spec, start, end in CC.fake_cases():
        es = [CC.spec_entry(*x) for x in spec]
        c, lo = CC.crl_at(es + [b"\x30\x03\x02\x01"])
        good = CC.crl(es)
        want, verdicts, _ = check(eng, [good, c, good], [DG[0], DG[0], DG[1]], phases=(len(nm) % 16,), host=False, bad=[1])
        assert verdicts[1][0] == len(good) + lo + sum(map(len, es)), nm
        assert want == CRL.probes_image([good, good], [DG[0], DG[1]])


def test_a_bad_crl_between_good_ones_at_every_blob_phase(eng):
    ent = REJ["entry2 one byte short"]
    good = CC.crl([CC.entry(CC.serial_of(k, 16)) for k in range(40)])
    crls = [good, ent[0], CC.small_crl()]
    want, verdicts, _ = check(eng, crls, DG[:3], phases=range(16), host=False, bad=[1])
    assert verdicts[1][0] == len(good) + ent[1]


def test_300_crls_of_0_to_3_entries_every_seventh_bad(eng):
    rej = CC.rejections()
    crls, digests, by, bad = [], [], {}, {}
    for k in range(300):
        ss = [CC.serial_of(k * 3 + j, 10 + (k + j) % 35) for j in range(k % 4)]
        if k % 7 == 3:
            _, c, off = rej[(k // 7 * 5) % len(rej)] if k % 28 != 10 else ("", b"", 0)    # (now and then one of 0 bytes)
            bad[k] = off
        else:
            c = CC.crl([CC.entry(s) for s in ss] if ss else None, next_update=k % 2 == 0)
            by.setdefault(DG[k % 5], []).extend(ss)
        crls.append(c)
        digests.append(DG[k % 5])
    at = EC.starts(crls)
    want, verdicts, cinfo = check(eng, crls, digests, phases=(0, 11), bad=sorted(bad))
    assert [verdicts[k][0] for k in sorted(bad)] == [at[k] + bad[k] for k in sorted(bad)]
    dev, _ = KI.records(want)
    for d in by:
        assert [m for k, m in dev if k == KI.set_key(0, d)] == [s for s in by[d] if len(s) <= 40]
    assert cinfo.empty_crls == sum(1 for k in range(300) if k % 4 == 0 and k not in bad)
    EC.identities(crls, want, {f: getattr(cinfo, f) for f in CRL.INFO_FIELDS}, verdicts)


# ---- 3. what still fails the whole call, and a NULL verdicts

def test_buffers_one_short_of_the_good_crls_need(eng):
    long, _ = EC.long_then_broken()
    crls, digests = EC.five(long, 2, DG[6])
    want, winfo, _ = expected(crls, digests)
    assert winfo[0]["host_members"] == 1 and winfo[0]["members"] > 0
    strict = len(CRL.probes_image(crls[:2] + crls[3:], digests[:2] + digests[3:]))
    assert strict == len(want)                                                   # sized by the good CRLs
    for cap in (len(want) - 1, len(want) - 48, winfo[0]["meta_bytes"], 0):
        rc, info, cinfo, got, verdicts = call_host(eng, crls, digests, cap)
        assert rc == N.E_RANGE and got is None and verdicts is None and fields(info, cinfo) == winfo
    for mc, nc in ((winfo[0]["meta_bytes"] - 1, winfo[0]["members"]), (winfo[0]["meta_bytes"], winfo[0]["members"] - 1), (0, 0)):
        rc, info, cinfo, got, verdicts = call_device(eng, crls, digests, mc, nc, phase=4)
        assert rc == N.E_RANGE and got is None and verdicts is None and fields(info, cinfo) == winfo
    rc, info, cinfo, got, verdicts = call_device(eng, crls, digests, winfo[0]["meta_bytes"] + 100, sum(map(len, crls)) // 6, phase=4)
    assert rc == 0 and got == want and verdicts[2][0] != NONE                     # sized by the bound


def test_null_verdicts(eng):
    crls, digests = EC.five(REJ["a fourth TLV in an entry"][0], 2)
    want, winfo, wverdicts = expected(crls, digests)
    rc, info, cinfo, got, _ = call_host(eng, crls, digests, len(want), null=True)
    assert rc == 0 and got == want and fields(info, cinfo) == winfo
    rc, info, cinfo, got, _ = call_device(eng, crls, digests, winfo[0]["meta_bytes"], winfo[0]["members"], phase=1, null=True)
    assert rc == 0 and got == want and fields(info, cinfo) == winfo and (cinfo.bad_crl, cinfo.bad_offset) == (2, wverdicts[2][0])


def test_the_three_offset_errors_still_fail_the_call(eng):
    a, b = CC.small_crl(), REJ["a fourth TLV in an entry"][0]
    A, B = len(a), len(b)
    cap = 64 + 56 * 3 + 48 * (A + B)
    for offsets, bad in (([1, A, A + B], (0, 0)), ([0, A + 1, A], (1, A + 1)), ([0, A, A + B - 1], (2, A + B)), ([0, A, A + B + 1], (2, A + B)),
                         ([0, A + B, A, A + B], (1, A + B))):
        assert CRL.check_offsets(offsets, len(offsets) - 1, A + B) == bad
        dg = DG[:len(offsets) - 1]
        rc, _, cinfo, got, verdicts = call_host(eng, [a, b], dg, cap, offsets=offsets)
        assert rc == N.E_INVAL and got is None and verdicts is None and (cinfo.bad_crl, cinfo.bad_offset) == bad
        rc, _, cinfo, got, verdicts = call_device(eng, [a, b], dg, cap, A + B, 3, offsets=offsets)
        assert rc == N.E_INVAL and got is None and verdicts is None and (cinfo.bad_crl, cinfo.bad_offset) == bad
    info, cinfo, v = N.KnownImageInfo(), N.CrlInfo(), Verdicts(1)
    offsets = np.array([0, 1 << 32], np.uint64)
    assert eng._lib.ctmr_crl_probes_each(eng._h, a, 1 << 32, offsets.ctypes.data, 1, DG[0], None, 0, C.byref(info), C.byref(cinfo), v.ptr) == N.E_INVAL
    assert v.read(N.E_INVAL) is None


# ---- 4. the Python surface

def test_the_python_surface(eng):
    crls, digests = EC.five(REJ["entry1 one byte short"][0], 2)
    want, winfo, wverdicts = CRL.probes_each(crls, digests)
    img, info, verdicts = eng.crl_probes_each(crls, digests)
    assert img == want and verdicts == wverdicts and {f: info[f] for f in CRL.INFO_FIELDS} == winfo
    blob, offsets = operands(crls)
    d = torch.from_numpy(np.frombuffer(b"\0" * 5 + blob, np.uint8).copy()).to(DEV)[5:]
    for exact in (None, True, False):
        meta, d_rec, info, verdicts = eng.crl_probes_each_device(d, offsets, digests, exact=exact)
        assert meta + d_rec.cpu().numpy().tobytes() == want and verdicts == wverdicts and d_rec.numel() == 48 * info["records"]
    assert eng.crl_probes_each((blob, offsets), b"".join(digests))[0] == want
    with pytest.raises(CRL.CrlError):                                             # the strict call is what it was
        eng.crl_probes(crls, digests)


def test_known_revoked_each_on_an_engine_that_mapped_certificates(eng):
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
    broken = CC.crl([CC.entry(s) for s in serials[1::2]] + [b"\x30\x03\x02\x01"])   # serials the engine holds, in a CRL it must not read
    crls = [CC.crl([CC.entry(s) for s in revoked[:10]]), broken, CC.crl([CC.entry(s) for s in revoked[10:]]), b"", CC.crl([CC.entry(serials[1])])]
    digests = [digest, digest, digest, digest, DG[5]]
    good = [0, 2, 4]
    before = (state(e), table(e), e.issuer_counts().tobytes())
    with pytest.raises(CRL.CrlError):
        e.known_revoked(crls, digests, 0)                                          # the default is what it was
    for now in (0, 1803859200):                                                    # everything kept; the January sets gone
        p_meta, hits, host_hits, verdicts = e.known_revoked(crls, digests, now, each=True)
        s_meta, s_hits, s_host = e.known_revoked([crls[k] for k in good], [digests[k] for k in good], now)
        assert p_meta == s_meta and (hits == s_hits).all() and (host_hits == s_host).all()
        assert [k for k, v in enumerate(verdicts) if v[0] == NONE] == good and verdicts == CRL.probes_each(crls, digests)[2]
        assert int((hits["records"] > 0).sum() + (host_hits["records"] > 0).sum()) > 0
    assert (state(e), table(e), e.issuer_counts().tobytes()) == before           # read-only
    e.close()
