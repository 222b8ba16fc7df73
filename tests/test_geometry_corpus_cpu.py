"""The geometry corpus of tests/geometry_corpus.py holds what it promises (no GPU; every assertion is on the corpus, never
on the device code): the oracle accepts what is meant to be accepted, twins are byte-identical except at the position
under test and differ in the oracle's record, the position under test reaches every residue and every offset around the
end of both windows, and the host simulation of the window walk decides nearly all of it without a miss — so that on the
device the WINDOW path is what answers, not the exact reader behind it.  This is what keeps tests/test_gpu_geometry.py
honest: a corpus whose fields never reach a window's end would let every case of it pass."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import geometry_corpus as G
from tests import harness
from tests.gpu_common import run_oracle, expected_records

W_STRICT, W_FAST, SKIP_FAST = 224, 216, 8
SWITCHES = {"reference": dict(strict_strings=True, strict_spki=True, strict_ext=True),
            "fast": dict(strict_strings=False, strict_spki=True, strict_ext=False)}
SWEPT = ("front", "front_rdn", "subject", "tail", "ext", "ext_unknown", "ext_crl", "san", "san_long", "small")
RSA_OID = bytes.fromhex("06092a864886f70d010101")
EC_OID = bytes.fromhex("06072a8648ce3d0201")


@functools.lru_cache(maxsize=None)
def oracle_records(name, profile):
    """(status, exp_hour as the record reports it) of a family in builder order; sequence families payload by payload."""
    fam = G.FAMILIES[name]()
    o = orc.Engine(G.FILT, False, G.NOW)
    o.set_profile(profile)
    cuts = fam.cuts or [0, len(fam.certs)]
    st, eh = [], []
    for lo, hi in zip(cuts, cuts[1:]):
        b = fam.batch(range(lo, hi))
        _, s, unk, e = run_oracle(b, G.registered_issuers(), engine=o)
        st.append(s)
        eh.append(expected_records(b, s, unk, e, **SWITCHES[profile])[2])
    return np.concatenate(st), np.concatenate(eh)


@functools.lru_cache(maxsize=None)
def parsed(name):
    return [orc.parse_cert(c[0]) for c in G.FAMILIES[name]().certs]


def hdr(der, p):
    """(content start, end) of the element at p."""
    ln = der[p + 1]
    if ln < 0x80:
        return p + 2, p + 2 + ln
    k = ln & 0x7f
    return p + 2 + k, p + 2 + k + int.from_bytes(der[p + 2:p + 2 + k], "big")


def diff_span(a, b):
    d = [k for k in range(len(a)) if a[k] != b[k]]
    return d[0], d[-1] + 1


@pytest.mark.parametrize("name", list(G.FAMILIES))
def test_twins_are_equal_except_at_one_place_and_the_oracle_tells_them_apart(name):
    fam = G.FAMILIES[name]()
    ps = parsed(name)
    assert len(fam.pairs) >= 3 and len(fam.certs) <= 2000
    for profile in ("reference", "fast"):
        st, eh = oracle_records(name, profile)
        for i, j, kind in fam.pairs:
            a, b = fam.certs[i][0], fam.certs[j][0]
            assert len(a) == len(b) and fam.certs[i][1:] == fam.certs[j][1:]
            lo, hi = diff_span(a, b)
            assert hi - lo <= 12, (name, kind, lo, hi)
            assert ps[i].ok and st[i] in (orc.ST_PASS, orc.ST_FILTERED_CA), (name, kind, i)     # the first twin is the well-formed one
            if kind == "ip" and profile == "fast":                               # (the subjectAltName is skipped by length)
                assert st[j] == orc.ST_PASS
                continue
            assert st[i] != st[j] or eh[i] != eh[j], (name, profile, kind, fam.marks[i])
        for i, kind in fam.singles:
            assert st[i] == orc.ST_PARSE_ERROR and not ps[i].ok, (name, kind)
    # the twins share a serial; from pair to pair serials differ, and the first octet names the family
    serials = [fam.certs[i][0][ps[i].serial_off:ps[i].serial_off + ps[i].serial_len] for i, _, _ in fam.pairs]
    if name != "waves":                                                          # (waves repeats certificates of front and subject)
        assert len(set(serials)) == len(serials) and all(s[0] == G.IDS[name] for s in serials)


def test_statuses_kinds_keys_serials_and_hours():
    want = {"front": (orc.ST_PASS, orc.ST_PARSE_ERROR, orc.ST_FILTERED_CN), "front_rdn": (orc.ST_PASS, orc.ST_PARSE_ERROR, orc.ST_FILTERED_CN),
            "subject": (orc.ST_PASS, orc.ST_PARSE_ERROR), "tail": (orc.ST_PASS, orc.ST_PARSE_ERROR),
            "tail_last": (orc.ST_PASS, orc.ST_PARSE_ERROR), "ext": (orc.ST_PASS, orc.ST_PARSE_ERROR, orc.ST_FILTERED_CA),
            "ext_unknown": (orc.ST_PASS, orc.ST_FILTERED_CA), "ext_crl": (orc.ST_PASS, orc.ST_FILTERED_CA),
            "san": (orc.ST_PASS, orc.ST_PARSE_ERROR, orc.ST_FILTERED_CA), "san_long": (orc.ST_PASS, orc.ST_FILTERED_CA),
            "small": (orc.ST_PASS, orc.ST_FILTERED_CN), "large": (orc.ST_PASS, orc.ST_FILTERED_CA),
            "waves": (orc.ST_PASS, orc.ST_PARSE_ERROR, orc.ST_FILTERED_CN)}
    kinds = {"front": {"cn", "hour", "tag"}, "subject": {"exp0", "neg", "shape", "hour"}, "tail": {"pad", "sigtag", "algover"},
             "tail_last": {"pad", "sigtag", "algover"}, "ext": {"ca", "critical"}, "san": {"ca", "ip"}}
    lengths = set()
    for name in G.FAMILIES:
        fam, ps = G.FAMILIES[name](), parsed(name)
        st, _ = oracle_records(name, "reference")
        for code in want[name]:
            assert (st == code).sum() > 0, (name, code)
        if name in kinds:
            assert {k for _, _, k in fam.pairs} == kinds[name]
        lengths |= {ps[i].serial_len for i, _, _ in fam.pairs}
        if name in SWEPT:
            # two thirds RSA keys, one third P-256 points (small: an unknown algorithm throughout)
            first = [i for i, _, _ in fam.pairs]
            ec = sum(EC_OID in fam.certs[i][0][ps[i].spki_off:ps[i].spki_off + 40] for i in first) / len(first)
            rsa = sum(RSA_OID in fam.certs[i][0][ps[i].spki_off:ps[i].spki_off + 40] for i in first) / len(first)
            assert (name == "small" and ec == rsa == 0) or (0.30 <= ec <= 0.36 and 0.64 <= rsa <= 0.70), (name, ec, rsa)
            hours = {ps[i].not_after // 3600 for i, _, _ in fam.pairs}
            assert len(hours) >= 40, (name, len(hours))
    assert lengths == set(range(1, 21))
    san = G.san()
    assert sum(c[2] for c in san.certs) * 2 in range(len(san.certs) - 30, len(san.certs) + 1)      # half are precertificate entries
    sub = G.subject()
    assert {m["m"] for m in sub.marks} == {0, 128, 250, 256, 384, 512}
    assert sorted(len(c[0]) for c in G.small().certs)[::2] == [t for t in G.SMALL_LENGTHS if t not in G.UNREACHABLE]
    assert {m["hints"] for m in G.front_rdn().marks} == {1, 2, 3, 4, 5}
    assert {m["count"] for m in G.ext_unknown().marks} == set(range(1, 25)) and {m["at"] for m in G.san_long().marks} == set(range(40))
    big = [(k, m["lane"]) for k, m in enumerate(G.large().marks) if m["big"]]
    assert [(k % 64, lane) for k, lane in big] == [(0, 0), (17, 17), (63, 63)] * 2
    assert all(len(G.large().certs[k][0]) == G.BIG == 70000 for k, _ in big)
    wv = G.waves()
    assert sorted({hi - lo for lo, hi in zip(wv.cuts, wv.cuts[1:])}) == sorted(G.WAVE_SIZES)
    tl = G.tail_last()
    for lo, hi in zip(tl.cuts, tl.cuts[1:]):
        assert tl.marks[hi - 1].get("last") and 1 <= hi - lo <= 4                 # the certificate under test ends its payload
    assert sorted(m["over"] for m in tl.marks if m.get("over")) == list(range(1, 41))
    for k, m in enumerate(tl.marks):                                              # … the TBSCertificate ends `over` octets behind it
        if m.get("over"):
            der = tl.certs[k][0]
            assert hdr(der, 0)[1] == len(der) and der[4] == 0x30 and hdr(der, 4)[1] == len(der) + m["over"]


def window_origins(base):
    """Payload addresses at which the first windows begin: the certificate (+ 8 for the fast kernels), down to a dword."""
    return {W_STRICT: base & ~3, W_FAST: (base + SKIP_FAST) & ~3}


def offsets_around_the_end(name, field_of, origin_of=None, kinds=None, by_kind=True):
    """{(W, kind): set of offsets of the field under test from the window's start}, and the address residues mod 16, over
    the two placements the GPU test maps: the family's packed batch (certificates back to back: natural phases) and its
    line view (certificate k at residue 37·k mod 128).  The window's start is rounded down to a dword of the PAYLOAD, so an
    offset is reached by a position and a phase together."""
    fam, ps = G.FAMILIES[name](), parsed(name)
    b = fam.batch()
    seen, residues = {}, {}
    for base in (b.offsets.astype(np.int64), G.line_view(b)[1].astype(np.int64)):
        for i, j, kind in fam.pairs:
            if kinds and kind not in kinds:
                continue
            kind = kind if by_kind else "any"
            for k in (i, j):
                at = int(base[k]) + field_of(fam, ps, k, i, j)
                residues.setdefault(kind, set()).add(at % 16)
                org = window_origins(int(base[k])) if origin_of is None else {W: origin_of(fam, ps, k, int(base[k])) for W in (W_STRICT, W_FAST)}
                for W, o in org.items():
                    seen.setdefault((W, kind), set()).add(at - o)
    return seen, residues


def first_difference(fam, ps, k, i, j):
    return diff_span(fam.certs[i][0], fam.certs[j][0])[0]


def check_window_end(seen, residues):
    for (W, kind), offs in seen.items():
        assert set(range(W - 24, W + 9)) <= offs, (W, kind, sorted(set(range(W - 24, W + 9)) - offs))
    for kind, r in residues.items():
        assert r == set(range(16)), (kind, r)


def test_front_fields_cross_the_end_of_the_first_window_octet_by_octet():
    """The issuer CN's first letter, the notAfter hour and the notAfter tag each lie at every offset W − 24 … W + 8 of the
    first window (W = 224 from the certificate's start, W = 216 from 8 octets in; both rounded down to a dword of the
    payload) and at every address residue mod 16; the SubjectPublicKeyInfo's head too."""
    check_window_end(*offsets_around_the_end("front", first_difference))
    check_window_end(*offsets_around_the_end("front", lambda fam, ps, k, i, j: ps[i].spki_off))
    seen, res = offsets_around_the_end("front_rdn", first_difference)
    assert all(r == set(range(16)) for r in res.values())


def test_subject_moves_the_key_head_and_the_key_end():
    check_window_end(*offsets_around_the_end("subject", lambda fam, ps, k, i, j: ps[i].spki_off, by_kind=False))
    fam, ps = G.subject(), parsed("subject")
    base = fam.batch().offsets.astype(np.int64)
    ends, address = {}, set()
    for i, _, _ in fam.pairs:                                # the key's end (what touch_tail gets as pos): kt = [pos − 12, pos + 4)
        ends.setdefault(fam.marks[i]["m"], set()).add((ps[i].spki_off + ps[i].spki_len) % 16)
        address.add((int(base[i]) + ps[i].spki_off + ps[i].spki_len) % 16)
    assert set(ends) == {0, 128, 250, 256, 384, 512} and all(r == set(range(16)) for r in ends.values()), ends
    assert address == set(range(16))
    assert len({m["filler"] for m in fam.marks}) == 301


def after_the_key(fam, ps, k, base):
    """The window touch_tail fills: it begins at the SubjectPublicKeyInfo's end, down to a dword of the payload."""
    return (base + ps[k].spki_off + ps[k].spki_len) & ~3


@pytest.mark.parametrize("name", ["ext", "ext_crl"])
def test_extension_headers_cross_the_end_of_the_window_behind_the_key(name):
    check_window_end(*offsets_around_the_end(name, first_difference, after_the_key, kinds={"ca"}))
    fam = G.FAMILIES[name]()
    assert {m["ski"] for m in fam.marks} == set(range(251))                       # 125..130: where the short form ends
    if name == "ext":
        assert {(m["critical"], m["first"]) for m in fam.marks} == {(True, False), (False, False), (True, True)}
        # the extension HEADER of basicConstraints (what the 12-octet fast form reads) as well
        seen, res = offsets_around_the_end(name, lambda fam, ps, k, i, j: fam.certs[k][0].rfind(bytes.fromhex("0603551d13")) - 2,
                                           after_the_key, kinds={"ca"})
        check_window_end(seen, res)


def test_tail_positions():
    fam, ps = G.tail(), parsed("tail")
    base = fam.batch().offsets.astype(np.int64)
    by_variant, offs, address = {}, set(), set()
    for i, _, _ in fam.pairs:
        k, m = i, fam.marks[i]
        tbs_end = ps[k].tbs_off + ps[k].tbs_len
        by_variant.setdefault(m["variant"], set()).add(tbs_end % 16)                 # (tail & 3 and tail & 15 take every value)
        address.add((int(base[k]) + tbs_end) % 16)
        der = fam.certs[k][0]
        assert der[tbs_end] == 0x30 and der[tbs_end + m["alg_len"]] in (0x03, 0x04)
        offs.add(m["alg_len"])                              # the signatureValue header's offset from tbs_end
    for v in range(4):
        assert by_variant[v] == set(range(16)), v
    assert address == set(range(16))
    assert set(range(10, 41)) <= offs and {12, 15, 30, len(G.PSS_SIGALG)} <= offs and len(G.PSS_SIGALG) > 27
    assert {m["filler"] for m in G.subject().marks} >= set(range(64))


def test_san_moves_basic_constraints_over_every_residue():
    fam = G.san()
    assert {m["san"] for m in fam.marks} == set(range(2, 701))
    _, res = offsets_around_the_end("san", first_difference)
    assert all(r == set(range(16)) for r in res.values())
    base = fam.batch().offsets.astype(np.int64)
    assert {(int(base[i]) + diff_span(fam.certs[i][0], fam.certs[j][0])[0]) % 32 for i, j, _ in fam.pairs} == set(range(32))


def test_the_line_view_takes_every_residue():
    b = G.front().batch()
    blob, start, end = G.line_view(b)
    assert ((start % 128) == (37 * np.arange(b.n)) % 128).all() and (np.diff(start.astype(np.int64)) > 0).all()
    assert set((start[:128] % 128).tolist()) == set(range(128))
    covered = np.zeros(len(blob), bool)
    for k in range(b.n):
        assert blob[int(start[k]):int(end[k])].tobytes() == b.cert(k)
        covered[int(start[k]):int(end[k])] = True
    assert (blob[~covered] != 0).all() and len(blob) == int(end[-1]) + G.N.PAYLOAD_PAD and (start[1:] >= end[:-1]).all()
    order = G.shuffled(G.front())
    assert sorted(order) == list(range(b.n)) and order != list(range(b.n)) and order == G.shuffled(G.front())
    wv = G.waves()
    sh = G.shuffled(wv)
    assert all(sorted(sh[lo:hi]) == list(range(lo, hi)) for lo, hi in zip(wv.cuts, wv.cuts[1:]))


@pytest.mark.parametrize("name", [n for n in G.FAMILIES if n not in ("small", "large")])
def test_the_window_path_decides(name):
    """A condition on the INPUTS: the host simulation of the window walk (per-lane refills; not the device) decides at least
    95 % of the family's accepted RSA-keyed certificates with no miss and no defer_exact, in both geometries — so at most
    5 % are certain to end on the exact reader, where a wrong window could not show.  (EC keys: the simulation evaluates
    the point through the window and misses on every one; the device defers the point to k_ec_resolve.)"""
    fam, ps = G.FAMILIES[name](), parsed(name)
    base = fam.batch().offsets.astype(np.int64)
    for args in ((W_STRICT, True, True, 0), (W_FAST, False, False, SKIP_FAST)):
        n = hit = 0
        for k, (der, _, _) in enumerate(fam.certs):
            if not ps[k].ok or RSA_OID not in der[ps[k].spki_off:ps[k].spki_off + 40]:
                continue
            ok, _, misses, _, _, _, defer = harness.walk_window(der, int(base[k]) % 128, args[0], args[1], args[2], skip=args[3])
            assert ok
            n += 1
            hit += misses == 0 and defer == 0
        assert n >= 20 and hit >= 0.95 * n, (name, args, hit, n)


def test_the_large_certificate_is_decided_70_kB_behind_its_first_window():
    """The 70 000-octet certificate's headers (30 83 …: five octets each) lie within the sixteen octets HeadView serves, so
    under skip = 8 the walk is NOT handed over for them: it is decided by a window the lane fetches for itself at the
    basicConstraints behind the 69 kB extension — one refill, 69 kB in, no miss — in both geometries."""
    fam = G.large()
    for k, m in enumerate(fam.marks):
        if m["big"]:
            der = fam.certs[k][0]
            assert der[:2] == der[5:7] == b"\x30\x83"
            for args in ((W_FAST, False, False, SKIP_FAST), (W_STRICT, True, True, 0)):
                ok, refills, misses, first_refill, _, _, defer = harness.walk_window(der, 37 * k % 128, *args[:3], skip=args[3])
                assert ok and refills >= 1 and first_refill > 69000 and misses == 0 and defer == 0


def test_small_certificates_are_the_hand_over_under_the_fast_geometry():
    """A certificate whose two outer headers take fewer than the 8 octets the fast window skips (30 7x 30 7x: four) has its
    version and serial IN FRONT of the window: every one of them misses under skip = 8 and goes to the exact reader, and
    none misses in the STRICT geometry, whose window begins at the certificate."""
    fam = G.small()
    short = [k for k, c in enumerate(fam.certs) if c[0][1] < 0x80]
    assert len(short) >= 60
    for k in short:
        der = fam.certs[k][0]
        assert harness.walk_window(der, 37 * k % 128, W_FAST, False, False, skip=SKIP_FAST)[2] > 0
        ok, _, misses, _, _, _, defer = harness.walk_window(der, 37 * k % 128, W_STRICT, True, True)
        assert ok and misses == 0 and defer == 0
