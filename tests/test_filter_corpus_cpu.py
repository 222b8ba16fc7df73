"""The filter corpus of tests/filter_corpus.py holds what it promises (no GPU): for every certificate under every setting the
oracle (orc_cert_is_filtered_out, Engine.batch under both profiles) and the host build of the product's walk
(harness.product_walk(..., cn_filter)) agree with the corpus's plain model; the oracle finds the recorded effective CN;
everything parses under both profiles but the `order` family's deliberate two; the `address` and `window` sweeps reach the
residues and the window edge they claim; and under simulated windows with contents of their own (walk_window_stale: reads
clamped into the window and counted, as WinReaderS does) and for lanes out of reach the verdict is the model's at every step.

WHAT THE WINDOW SWEEP CAN REACH.  walk_name asks for 32 octets from the start of each RDN; in the 12-octet fast form the CN
begins 11 octets in, and cn_prefix_match reads whole words: a piece of p octets reads 11 + 4·ceil(p / 4) octets from the
RDN's start.  For p <= 20 that is at most 31: the hint covers the compare wherever the CN lies — an RDN too close to the
window's end moves the window first — so NO step of such a piece can read outside, and the test asserts exactly that (a
hint that shrank would show here).  For p = 33, 40, 64 both kinds of step exist and both are asserted, in each of the three
configurations the map kernels run (GEOMETRIES).  The window family's values are T61Strings because a checked string type
changes this: value_strings_ok asks for the window every 64 octets of such a value."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import filter_corpus as F
from tests import harness
from tests.gpu_common import run_oracle

PROFILES = ("reference", "fast")
W_STRICT, W_FAST, SKIP_FAST = 224, 216, 8
HINTED = 20                                           # the longest piece walk_name's 32-octet hint covers: 11 + 4·ceil(p / 4) <= 32
# The windows as the map kernels run them: (name, octets, octets of the certificate in front of the first window, strict_strings
# in the walk, strict_extensions).  The 224-octet kernels are the reference profile's; the walk checks the Names' strings for
# precertificate entries only (kernels/map.h map_one), so both settings of `strings` occur there, lane by lane.
GEOMETRIES = (("strict, X509 entry", W_STRICT, 0, False, True), ("strict, precertificate", W_STRICT, 0, True, True),
              ("fast", W_FAST, SKIP_FAST, False, False))


@functools.lru_cache(maxsize=None)
def parsed(name):
    return [orc.parse_cert(c.der) for c in F.FAMILIES[name]().certs]


def filters_only(c, s):
    """certIsFilteredOut alone (the oracle's orc_cert_is_filtered_out answers for a certificate that parsed)."""
    st = F.status(F.Cert(c.der, 0, 0, c.cn, c.ca, c.not_after), s)
    assert st in (F.ST_PASS, F.ST_FILTERED_CA, F.ST_FILTERED_EXPIRED, F.ST_FILTERED_CN)
    return st


@pytest.mark.parametrize("name", list(F.FAMILIES))
def test_the_oracle_and_the_host_walk_agree_with_the_model(name):
    fam, ps = F.FAMILIES[name](), parsed(name)
    checked, walked = set(), set()                    # (case, certificate, profile) / (case, certificate): entered only BEHIND the assertions
    for k, (c, p) in enumerate(zip(fam.certs, ps)):
        assert bool(p.ok) == c.parses, (name, k, c.mark)
        if not c.parses:
            continue
        # under both profiles: no finding of any kind (a finding would drop a precertificate whatever the filter says)
        assert not (p.nonfatal or p.string_findings or p.ext_fatal or p.ext_findings or p.ext_string_findings or p.spki_fatal), (name, k)
        assert c.der[p.cn_off:p.cn_off + p.cn_len] == (c.cn or b""), (name, k, c.mark)
        assert p.not_after == c.not_after and bool(p.bc_valid and p.is_ca) == c.ca
    for k, (case, s) in enumerate(fam.in_force()):
        want = fam.expected(case, s)
        for i in case.idx:
            c = fam.certs[i]
            if not c.parses:
                continue
            assert orc.is_filtered_out(c.der, ps[i], s.filt, s.log_expired, s.now) == filters_only(c, s), (name, i, s.filt[:40])
            match = not F.cn_skips(s.filt, c.cn)
            w = harness.product_walk(c.der, cn_filter=s.filt if s.filt else None)     # (an empty filter: ctmr_set_filter leaves it inactive)
            assert w.ok and bool(w.cn_match) == match, (name, i, c.mark, s.filt[:40])
            assert c.der[w.cn_off:w.cn_off + w.cn_len] == (c.cn or b"")
            walked.add((k, i))
        b = fam.batch(case)
        et = b.entry_type.copy()
        for profile in PROFILES:
            o = orc.Engine(s.filt, s.log_expired, s.now)
            o.set_profile(profile)
            _, st, _, _ = run_oracle(b, F.registered_issuers(), engine=o)
            o.close()
            # (the oracle knows entry types 0 and 1: an entry the downloader dropped never reaches it)
            st = np.where(et == F.N.ENTRY_INVALID, F.ST_ENTRY_DECODE_ERROR, st)
            assert (st == want).all(), (name, profile, s.filt[:40], np.nonzero(st != want)[0][:10])
            checked |= {(k, i, profile) for i in case.idx}
    # What must have been checked, listed from the family alone: every certificate of every case under either profile, and by
    # the host walk every one but the deliberate certificate that does not parse (`order`, `switch`: it has no walk to ask).
    # A case or certificate a later change of the loops above leaves out is missing from the sets and counts as skipped.
    due = {(k, i) for k, case in enumerate(fam.cases) for i in case.idx}
    no_walk = {(k, i) for k, i in due if not fam.certs[i].parses}
    assert len(no_walk) == (len(fam.cases) if name in ("order", "switch") else 0)
    skipped = len({(k, i, p) for k, i in due for p in PROFILES} - checked) + len(due - no_walk - walked)
    assert skipped == 0


def test_prefix_lengths_octets_and_near_misses():
    fam = F.prefix()
    assert len(F.P) == 257 and b"," not in F.P and {0x00, 0xff, 0x80} <= set(F.P[:9]) and any(x >= 0x80 for x in F.P[60:])
    base = [c for c in fam.certs if c.mark["kind"] == "base"]
    assert [len(c.cn) for c in base] == list(F.CN_LENGTHS) and all(c.cn == F.P[:len(c.cn)] for c in base)
    # the string type: T61String — strict_strings accepts every octet there (tests/strings_corpus.py: "every other tag")
    for c, p in zip(fam.certs, parsed("prefix")):
        assert c.der[p.cn_off - (2 if p.cn_len < 128 else 3 if p.cn_len < 256 else 4)] == F.T61 and c.et == 0
    singles = [case for case in fam.cases if case.mark["kind"] == "piece"]
    assert [len(case.setting.filt) for case in singles] == list(F.PIECE_LENGTHS)
    near = {case.mark["p"]: case for case in fam.cases if case.mark["kind"] == "near"}
    assert sorted(near) == list(F.PIECE_LENGTHS[1:])
    for p, case in near.items():
        pieces = case.setting.filt.split(b",")
        assert len(pieces) == len(F.near_miss_positions(p)) and {0, p - 1, max(p - 2, 0), (p - 1) & ~3} == set(F.near_miss_positions(p))
        for piece, k in zip(pieces, F.near_miss_positions(p)):
            assert len(piece) == p and [j for j in range(p) if piece[j] != F.P[j]] == [k]
            hits = [c for c in fam.certs if (c.cn or b"").startswith(piece)]
            assert len(hits) == 1 and hits[0].mark == dict(kind="twin", p=p, k=k), (p, k)
    # a piece one octet longer than the CN, equal to it, one shorter: all in the grid
    assert all({c - 1, c, c + 1} & set(F.PIECE_LENGTHS) == {c - 1, c, c + 1} for c in range(1, 72))


def test_address_residues():
    fam, ps = F.address(), parsed("address")
    assert {c.mark["s"] for c in fam.certs} == set(range(1, 21)) and {c.mark["j"] for c in fam.certs} == set(range(-1, 23))
    assert {p.serial_len for p in ps} == set(range(1, 21))
    assert {p.cn_off % 4 for p in ps} == set(range(4)) and {p.cn_off % 16 for p in ps} == set(range(16))
    assert [len(case.setting.filt) for case in fam.cases] == list(range(1, 24)) and {case.lead for case in fam.cases} == set(range(16))
    off = fam.batch(fam.cases[0]).offsets.astype(np.int64)
    for j in (-1, 0, 11, 22):                          # … of one CN variant alone: the payload address of the CN takes every residue
        assert {(int(off[k]) + ps[k].cn_off) % 16 for k, c in enumerate(fam.certs) if c.mark["j"] == j} == set(range(16))
    for case in fam.cases:                             # each piece splits the variants: those changed inside it are filtered
        want = fam.expected(case, case.setting)
        p = case.mark["p"]
        assert [(w == F.ST_PASS) for w in want] == [not 0 <= fam.certs[i].mark["j"] < p for i in case.idx]


def phases(fam, case):
    off = fam.batch(case).offsets.astype(np.int64)
    return [(case.lead + int(o)) % 128 for o in off[:-1]]


def test_window_sweep_reaches_the_edge():
    fam, ps = F.window(), parsed("window")
    assert {case.mark["p"] for case in fam.cases} == set(F.WINDOW_PIECES) and {case.lead for case in fam.cases} == set(F.WINDOW_LEADS)
    for k, (c, p) in enumerate(zip(fam.certs, ps)):
        assert p.cn_off == c.mark["cn_off"] and len(c.cn) == c.mark["p"] + 2
    for i in range(0, len(fam.certs), 2):              # twins: equal length, one serial, ONE octet apart — at the marked offset
        a, b = fam.certs[i], fam.certs[i + 1]
        d = [j for j in range(len(a.der)) if a.der[j] != b.der[j]]
        assert len(a.der) == len(b.der) and d == [a.mark["at"]] and a.issuer_idx == b.issuer_idx
        q = F.Q[:a.mark["p"]]
        assert a.cn.startswith(q) and not b.cn.startswith(q)
    for p in F.WINDOW_PIECES:
        for kind in ("last", "first"):
            at = {c.mark["at"] for c in fam.certs if c.mark["p"] == p and c.mark["kind"] == kind}
            # 8 octets inside the end of the window (224, less up to 3: it begins on a dword of the payload) to 8 beyond
            assert at >= set(range(F.WINDOW_END - 11, F.WINDOW_END + 9)), (p, kind, sorted(at))
    for kind in ("last", "first"):                     # either kind as X509 and as precertificate entries
        assert {c.et for c in fam.certs if c.mark["kind"] == kind} == {0, 1}
    assert all(c.der[c.mark["cn_off"] - 2] == F.T61 for c in fam.certs)
    # the compare itself, through the simulated windows as the map kernels run them, per piece length
    for p in F.WINDOW_PIECES:
        seen = {(g, fl): [0, 0] for g, *_ in GEOMETRIES for fl in "SC"}        # steps [all reads inside, some read outside]
        for case in fam.cases:
            if case.mark["p"] != p:
                continue
            piece = case.setting.filt
            for i, ph in zip(case.idx, phases(fam, case)):
                der = fam.certs[i].der
                for g, W, skip, strings, ext in GEOMETRIES:
                    r = harness.walk_window(der, ph, W, strings, ext, skip=skip, cn_filter=piece)
                    assert r[0] and r[8] + r[9] >= 1          # the compare ran
                    seen[g, "S"][r[9] > 0] += 1
                    assert (r[9] > 0) <= (r[2] > 0)          # a compare outside the window IS a miss
                    # (a lane out of reach fills its own window, from the certificate's start down to 16 octets, in either geometry)
                    o, st = harness.walk_window_noreach(der, ph, W, "C", strings, ext, cn_filter=piece)
                    assert o.ok and st[6] + st[7] >= 1
                    seen[g, "C"][st[7] > 0] += 1
        for key, (inside, outside) in seen.items():
            assert inside > 0, (p, key)
            if p <= HINTED:
                assert outside == 0, (p, key, outside)      # walk_name's hint covers the compare: see the module docstring
            else:
                assert outside >= 20, (p, key, outside)
    assert [p for p in F.WINDOW_PIECES if p > HINTED] == [33, 40, 64]


@pytest.mark.parametrize("name", ["window", "address"])
def test_simulated_windows_give_the_models_verdict_at_every_step(name):
    """Windows with contents of their own (reads outside are served from the window's last octets and COUNTED: the exact
    reader then decides, as in k_map_fused), in the three configurations of GEOMETRIES, and lanes out of reach that read
    global memory outside their window (flavour C; flavour S begins without a window, so the exact reader always decides
    for it: no more than product_walk says): cn_match is the model's."""
    fam = F.FAMILIES[name]()
    missed = {g: 0 for g, *_ in GEOMETRIES}
    for case, s in fam.in_force():
        if name == "address" and case.mark["p"] % 4 != 3 and case.mark["p"] != 23:
            continue                                   # (the address family on the simulators: every fourth piece and the longest)
        for i, ph in zip(case.idx, phases(fam, case)):
            c = fam.certs[i]
            match = not F.cn_skips(s.filt, c.cn)
            for g, W, skip, strings, ext in GEOMETRIES:
                o, st = harness.walk_window_stale(c.der, ph, W, 4, strings, ext, cn_filter=s.filt, skip=skip)
                assert o.ok and bool(o.cn_match) == match, (name, i, c.mark, g, ph)
                assert st[5] == 0
                missed[g] += st[7] > 0
                o, st = harness.walk_window_noreach(c.der, ph, W, "C", strings, ext, cn_filter=s.filt)
                assert o.ok and bool(o.cn_match) == match, (name, i, c.mark, g, ph)
    # … and in every configuration some steps' verdicts did come from the exact reader behind a counted miss
    assert all((n >= 20) == (name == "window") and (n > 0) == (name == "window") for n in missed.values()), missed


def test_names_shapes():
    fam = F.names()
    shapes = {c.mark["shape"] for c in fam.certs}
    assert shapes == {"no_cn", "empty_cn", "two_rdns", "multi_valued", "non_string_behind", "non_string_in_front", "non_string_alone",
                      "subject_only", "other_oid", "string_tag", "long_cn", "long_set", "long_sequence"}
    assert {c.mark["tag"] for c in fam.certs if c.mark["shape"].startswith("non_string")} == {0x04, 0x1e, 0x1c, 0x02}
    assert {c.mark["tag"] for c in fam.certs if c.mark["shape"] == "string_tag"} == {0x0c, 0x12, 0x13, 0x14, 0x16}
    assert {c.mark["oid"] for c in fam.certs if c.mark["shape"] == "other_oid"} == {b"\x55\x04\x03\x01", b"\x55\x04\x2a", b"\x55\x04"}
    two = [c for c in fam.certs if c.mark["shape"] == "two_rdns"]
    for filt, want in ((b"Alpha", [False, True]), (b"Beta", [True, False])):         # matches only the last / only the first CN
        assert [not F.cn_skips(filt, c.cn) for c in two] == want
    assert [len(c.cn) for c in fam.certs if c.mark["shape"] == "long_cn"] == [127, 128]
    for c in fam.certs:                                # the long forms are long
        if c.mark["shape"] == "long_set":
            assert b"\x31\x81" in c.der
        if c.mark["shape"] == "long_sequence":
            at = c.der.index(b"\x06\x03\x55\x04\x03\x0c\x0aAlpha Root\x04\x81\xc8")
            assert c.der[at - 3:at - 1] == b"\x30\x81"
    assert {f for f in F.NAMES_FILTERS} == {case.setting.filt for case in fam.cases} and len(F.NAMES_FILTERS) >= 15
    # the inactive filter and the empty pieces pass all; "Gamma", the O= value, a BMPString's first octets and a piece one octet longer
    # than the longest CN none; the rest split the family
    nobody = (b"Gamma", b"Org", b"Gamma,\x00B", F.ALPHA + b"x" * 119)
    for case in fam.cases:
        st = set(fam.expected(case, case.setting).tolist())
        assert st == ({F.ST_PASS} if case.setting.filt in (b"", b",") else {F.ST_FILTERED_CN} if case.setting.filt in nobody
                      else {F.ST_PASS, F.ST_FILTERED_CN}), case.setting.filt


def test_lists_and_refused_settings():
    fam = F.lists()
    by = {case.setting.filt: fam.expected(case, s) for case, s in fam.in_force()}
    cns = [c.cn for c in fam.certs]
    assert (by[b""] == F.ST_PASS).all() and (by[b","] == F.ST_PASS).all() and (by[b",x"] == F.ST_PASS).all()      # an empty piece matches all
    assert (by[b"x,"] == F.ST_PASS).all() and (by[b"x,,y"] == F.ST_PASS).all() and cns[0] is None
    assert [cns[k] for k in np.nonzero(by[b" x"] == F.ST_PASS)[0]] == [b" x"]                                     # not trimmed
    assert [cns[k] for k in np.nonzero(by[b"x "] == F.ST_PASS)[0]] == [b"x "]
    assert [cns[k] for k in np.nonzero(by[b"xy"] == F.ST_PASS)[0]] == [b"xy"]                                     # the whole CN
    assert (by[b"x,x"] == fam.expected(fam.cases[0], F.Setting(b"x"))).all()
    p64 = F.pieces64(b"p%02d")
    for cn, at in ((b"p00-first", 0), (b"p31-middle", 31), (b"p63-last", 63)):
        assert [k for k, p in enumerate(p64) if cn.startswith(p)] == [at]
    assert [cns[k] for k in np.nonzero(by[b",".join(p64)] == F.ST_PASS)[0]] == [b"p00-first", b"p31-middle", b"p63-last"]
    assert (by[b",".join(F.pieces64(b"q%02d"))] == F.ST_FILTERED_CN).all()
    long_ = b",".join(F.LONG_PIECES)
    passed = [cns[k] for k in np.nonzero(by[long_] == F.ST_PASS)[0]]
    assert b"L" * 70 in passed and b"L" * 63 not in passed and b"x" not in passed
    assert [k for k, p in enumerate(F.LONG_PIECES) if (b"L" * 70).startswith(p)] == [63]
    assert [cns[k] for k in np.nonzero(by[b"a\x00\xff"] == F.ST_PASS)[0]] == [b"a\x00\xffb"]
    # the refused settings: what ctmr_set_filter counts (engine/map.inc: at most 64 pieces, 1024 words)
    refused = [case.setting.filt for case in fam.cases if case.setting.refused]
    assert refused == list(F.LISTS_REFUSED)
    words = [sum((len(p) + 3) // 4 for p in f.split(b",")) for f in refused]
    assert words[0] == 1025 and len(refused[0].split(b",")) == 64 and len(refused[1].split(b",")) == 65 and words[1] <= 1024
    force = fam.in_force()
    k = [n for n, (case, _) in enumerate(force) if case.setting.refused]
    assert force[k[0]][1].filt == long_ and force[k[1]][1].filt == b"x"                # the batch follows the filter set before


def test_order_and_switch_reach_every_status():
    fam = F.order()
    assert len(fam.certs) == 2 * 2 * 2 * 3 * 2 + 2 and [case.setting.log_expired for case in fam.cases] == [False, True]
    combos = {(c.ca, c.mark.get("gone"), c.mark.get("match"), c.issuer, c.et) for c in fam.certs[:-2]}
    assert len(combos) == 48
    for case in fam.cases:
        st = fam.expected(case, case.setting)
        assert set(st.tolist()) == set(range(8)) - ({F.ST_FILTERED_EXPIRED} if case.setting.log_expired else set())
    # the order of the filters: CA in front of expired in front of the CN; the issuer's trouble only behind all three
    s = fam.cases[0].setting
    for c, st in zip(fam.certs[:-2], fam.expected(fam.cases[0], s)):
        want = F.ST_FILTERED_CA if c.ca else F.ST_FILTERED_EXPIRED if c.mark["gone"] else F.ST_FILTERED_CN if not c.mark["match"] else \
            {"registered": F.ST_PASS, "range": F.ST_NO_ISSUER, "bad": F.ST_ISSUER_PARSE_ERROR}[c.issuer]
        assert st == want
    sw = F.switch()
    force = sw.in_force()
    assert sum(case.setting.refused for case in sw.cases) == 2 and sw.cases[0].setting == sw.cases[-1].setting
    assert all(s == force[k - 1][1] for k, (case, s) in enumerate(force) if case.setting.refused)
    assert len({tuple(sw.expected(case, s).tolist()) for case, s in force}) >= 6      # the settings tell the certificates apart
    assert not orc.parse_cert(F.registered_issuers()[F.BAD_ISSUER]).ok
