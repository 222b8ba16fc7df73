"""The strings corpus of tests/strings_corpus.py holds what it promises (no GPU; every assertion is on the corpus, the
oracle and the HOST build of der_walk.h, never on the device code): the rules stated in the corpus module, the oracle's
string_findings / ext_string_findings and the host build of the walk agree on every certificate; twins differ at the place
under test alone and in their verdict; every octet x byte lane, every listed length, every UTF-8 table entry at every
offset 0..19 and every bad-octet position of the swept ranges is there, counted by the marks the builder leaves; and the
window simulation decides the value families without a miss, refills inside the long values and finds the bad octet on both
sides of the first window's end.  This is what keeps tests/test_gpu_strings_corpus.py honest."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import der as D
from tests import harness
from tests import strings_corpus as S

W = 224                 # the window of both instantiations that carry the check (kernels/readers.h WIN_CH_STRICT)
NF_STRING = 4


@functools.lru_cache(maxsize=None)
def parsed(name):
    """Every certificate of a family, parsed by the oracle once."""
    return [orc.parse_cert(c[0]) for c in S.FAMILIES[name]().certs]


@pytest.fixture
def strict_host_walk():
    harness.product_set_strings(True)
    harness.product_set_ext(True)
    yield
    harness.product_set_strings(False)
    harness.product_set_ext(False)


@pytest.mark.parametrize("name", list(S.FAMILIES))
def test_the_rules_the_oracle_and_the_host_walk_agree_on_every_certificate(name, strict_host_walk):
    fam, ps = S.FAMILIES[name](), parsed(name)
    assert 100 <= len(fam.certs) <= S.MAX_CERTS and len(fam.certs) == len(fam.expect) == len(fam.marks)
    seen = {}
    for k, (der, _, et) in enumerate(fam.certs):
        o, want = ps[k], fam.expect[k]
        assert o.ok and not o.nonfatal and not o.ext_fatal and not o.ext_findings, (name, k, o.err_site)
        if name == "rel_name":
            assert (o.string_findings, o.ext_string_findings) == (0, want), (name, k, fam.marks[k])
        else:
            assert (o.string_findings, o.ext_string_findings) == (want, 0), (name, k, fam.marks[k])
        if der in seen:
            continue
        seen[der] = k
        p = harness.product_walk(der)                       # the same der_walk.h, compiled for the host
        assert p.ok and p.nonfatal == (NF_STRING if want else 0), (name, k, fam.marks[k], p.nonfatal)
        if name != "rel_name":
            for fill in (0xA5, 0x30, 0xBF):                 # what lies behind the certificate is nobody's business
                assert harness.product_name_strings(der, fill) == (0 if want else 1), (name, k, fam.marks[k])
    harness.product_set_strings(False)                      # the switch decides: without it the walk files nothing
    for der, k in list(seen.items())[::7]:
        p = harness.product_walk(der)
        assert p.ok and p.nonfatal == 0, (name, k)


def first_and_last_difference(a, b):
    d = np.nonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8))[0]
    return int(d[0]), int(d[-1]) + 1


@pytest.mark.parametrize("name", list(S.FAMILIES))
def test_twins_differ_at_the_place_under_test_and_in_their_verdict(name):
    fam, ps = S.FAMILIES[name](), parsed(name)
    assert len(fam.pairs) >= 90
    for i, j, kind in fam.pairs:
        a, b = fam.certs[i][0], fam.certs[j][0]
        assert len(a) == len(b) and fam.certs[i][1:] == fam.certs[j][1:], (name, kind, i, j)
        lo, hi = first_and_last_difference(a, b)
        assert hi - lo <= 3, (name, kind, fam.marks[j])
        assert fam.expect[i] == 0 and fam.expect[j] != 0, (name, kind, fam.marks[j])
        assert a[ps[i].serial_off:ps[i].serial_off + ps[i].serial_len] == b[ps[j].serial_off:ps[j].serial_off + ps[j].serial_len]
    # every case twice, interleaved: an X509 entry and a precertificate entry with a serial of its own
    for k in range(0, len(fam.certs), 2):
        (a, ia, ea), (b, ib, eb) = fam.certs[k], fam.certs[k + 1]
        assert (ea, eb) == (0, 1) and ia == ib and len(a) == len(b) and fam.expect[k] == fam.expect[k + 1]
        sa, sb = (c[p.serial_off:p.serial_off + p.serial_len] for c, p in ((a, ps[k]), (b, ps[k + 1])))
        assert len(sa) == len(sb) and (sa != sb or len(sa) < 5)
        lo, hi = first_and_last_difference(a, b) if a != b else (ps[k].serial_off, ps[k].serial_off)
        assert ps[k].serial_off <= lo and hi <= ps[k].serial_off + ps[k].serial_len


def by_kind(fam, kind):
    return [m for m in fam.marks if m["kind"] == kind and m["et"] == 0]


def test_alphabet_has_every_octet_in_every_lane_of_every_tag():
    fam = S.alphabet()
    cover = {}
    for k, m in enumerate(fam.marks):
        for c in m["cover"]:
            cover.setdefault(c, []).append(k)
    assert set(cover) == {(t, b, lane) for t in S.TAGS for b in range(256) for lane in range(4)}
    for (tag, b, lane), ks in cover.items():
        inside = S.finding(tag, bytes([b])) == 0 or (tag == 0x0c and b < 0x80)
        assert len(ks) == 2 and fam.certs[ks[0]][2] == 0 and fam.certs[ks[1]][2] == 1
        for k in ks:
            value = S.lane_value(tag, b, lane)
            assert value[lane] == b and len(value) == 8 and D.tlv(tag, value) in fam.certs[k][0]
            assert (fam.expect[k] == 0) == inside
            assert inside or len(fam.marks[k]["cover"]) == 1          # an octet outside the set answers alone
    assert sorted({tuple(m["cover"][0][:2]) for m in by_kind(fam, "masked")}) == \
        sorted([(0x13, b | 0x80) for b in S.PRINTABLE] + [(0x12, b | 0x80) for b in S.NUMERIC])
    assert (0x13, 0xc1) in {m["cover"][0][:2] for m in by_kind(fam, "masked")} and (0x12, 0xb1, 2) in cover
    # the boundary octets, the octets next to them outside the set, between 0x20 and between 0xff, in every lane
    want = {0x13: {0x1f, 0x20, 0x21, 0x25, 0x26, 0x3a, 0x3b, 0x3c, 0x3d, 0x3e, 0x3f, 0x40, 0x41, 0x5a, 0x5b, 0x60, 0x61, 0x7a, 0x7b},
            0x12: {0x1f, 0x20, 0x21, 0x2f, 0x30, 0x39, 0x3a}}
    for kind in ("edge_20", "edge_ff"):
        assert {m["edge"] for m in by_kind(fam, kind)} == {(t, b, lane) for t in want for b in want[t] for lane in range(4)}
    assert set(S.PRINTABLE_EDGES) <= want[0x13] and set(S.NUMERIC_EDGES) <= want[0x12]
    for k, m in enumerate(fam.marks):
        if m["kind"] in ("edge_20", "edge_ff"):
            tag, b, lane = m["edge"]
            nb = 0x20 if m["kind"] == "edge_20" else 0xff
            v = S.lane_value(tag, b, lane, nb, nb)
            assert D.tlv(tag, v) in fam.certs[k][0] and v[lane] == b and all(v[i] == nb for i in (lane - 1, lane + 1) if 0 <= i < 4)
            assert (fam.expect[k] == 0) == (nb == 0x20 and b in (S.PRINTABLE if tag == 0x13 else S.NUMERIC))
    assert {k for _, _, k in fam.pairs} == {"neighbour"} and len(fam.pairs) == 2 * 4 * (len(S.PRINTABLE_EDGES) + len(S.NUMERIC_EDGES))
    assert {m["where"] for m in fam.marks} == {"subject", "issuer"}


def fast_form(rdn):
    """walk_name's 12-octet fast form: SET, SEQUENCE, a three-octet OID and the value's header, every length short."""
    return rdn[0] == 0x31 and rdn[1] < 0x80 and rdn[2] == 0x30 and rdn[3] < 0x80 and rdn[4:6] == b"\x06\x03" and rdn[10] < 0x80


@pytest.mark.parametrize("name, table", [("lengths", S.LENGTHS), ("rel_name", S.REL_LENGTHS)])
def test_lengths_has_every_length_and_every_case_at_it(name, table):
    fam = S.FAMILIES[name]()
    assert set(range(81)) | {127, 128, 129, 255, 256, 257, 300} == set(S.LENGTHS) and set(S.REL_LENGTHS) == set(range(41))
    for tag in S.CHECKED:
        of = lambda kind: [m for m in by_kind(fam, kind) if m["tag"] == tag]
        assert sorted(m["n"] for m in of("clean")) == list(table)
        assert {(m["n"], m["at"]) for m in of("bad")} == {(n, i) for n in table for i in (0, n - 1, 15, 16, 63, 64) if 0 <= i < n}
        assert sorted((m["n"], m["long_oid"]) for m in of("trail")) == sorted((n, f) for n in table for f in (False, True))
        if tag == 0x0c:
            for kind in ("utf8_end", "utf8_cut"):
                assert sorted((m["n"], m["seq"]) for m in of(kind)) == sorted((n, q) for n in table for q in (2, 3, 4) if n >= q)
    for k, m in enumerate(fam.marks):
        der, tag, n = fam.certs[k][0], m["tag"], m["n"]
        f = S.filler(tag)
        if m["kind"] == "clean":
            assert D.tlv(tag, f * n) in der and fam.expect[k] == 0
        elif m["kind"] == "bad":
            assert D.tlv(tag, S.put(f * n, m["at"], [S.BAD[tag]])) in der and fam.expect[k] == S.SF_OF[tag]
        elif m["kind"] == "trail":                              # hostile octets behind the value, inside the SEQUENCE
            atv = S.Atv(tag, f * n, S.HOSTILE, m["long_oid"])
            assert atv.der() in der and atv.der().endswith(f * n + bytes.fromhex("ff5f80bf")) and fam.expect[k] == 0
            if name == "lengths":
                assert fast_form(S.rdn_of(atv)) == (n <= 80 and not m["long_oid"])
        elif m["kind"] == "utf8_end":
            assert D.tlv(tag, f * (n - m["seq"]) + S.END_SEQ[m["seq"]]) in der and fam.expect[k] == 0
        else:                                                   # … cut by one octet, which lies right behind the value
            whole = f * (n - m["seq"]) + S.END_SEQ[m["seq"]]
            assert D.tlv(tag, whole[:-1]) + whole[-1:] in der and fam.expect[k] == S.SF_UTF8
            assert S.finding(tag, whole) == 0 and m["kind"] == "utf8_cut"
    assert {m["where"] for m in fam.marks} == ({"subject", "issuer"} if name == "lengths" else {"rel"})
    if name == "rel_name":                                      # every value lies inside the extension block, not in a Name
        for k, p in enumerate(parsed(name)):
            der = fam.certs[k][0]
            assert bytes.fromhex("0603551d1f") in der[p.exts_off:p.exts_end] and b"\xa0" in der[p.exts_off:p.exts_end]


def test_utf8_edges_has_every_table_entry_at_every_offset_and_a_balanced_random_part():
    fam, table = S.utf8_edges(), S.utf8_table()
    octets = {s for _, s, _, _ in table}
    for h in ("c280", "dfbf", "e0a080", "ed9fbf", "ee8080", "efbfbf", "f0908080", "f48fbfbf"):
        assert bytes.fromhex(h) in S.UTF8_VALID and bytes.fromhex(h) in octets
    for h in ("e09fbf", "eda080", "f08fbfbf", "f4908080", "c0", "c1", "80", "bf") + tuple("%02x" % b for b in range(0xf5, 0x100)):
        assert bytes.fromhex(h) in octets
    for s in S.UTF8_VALID:
        for i in range(1, len(s)):
            assert S.put(s, i, [0x7f]) in octets and S.put(s, i, [0xc0]) in octets
    for name, s, valid, twin in table:
        assert (S.finding(0x0c, s) == 0) == valid == (name == "valid")
    placed = [m for m in fam.marks if m["kind"] != "random" and m["kind"] != "twin" and m["et"] == 0]
    assert {(m["entry"], m["pre"]) for m in placed} == {(e, pre) for e in range(len(table)) for pre in range(20)}
    for e in range(len(table)):
        assert {m["post"] for m in placed if m["entry"] == e} == set(range(5))
    for k, m in enumerate(fam.marks):
        if m["kind"] not in ("random", "twin"):
            s = table[m["entry"]][1]
            assert D.tlv(0x0c, b"a" * m["pre"] + s + b"a" * m["post"]) in fam.certs[k][0]
            assert (fam.expect[k] == 0) == table[m["entry"]][2]
    rnd = S.random_strings()
    assert len(rnd) >= 2000 and len(by_kind(fam, "random")) == len(rnd) and {len(v) for v in rnd} == set(range(41))
    assert all(set(v) <= set(S.RANDOM_ALPHABET) for v in rnd)
    bad = sum(S.finding(0x0c, v) != 0 for v in rnd)
    assert len(rnd) / 4 <= bad <= 3 * len(rnd) / 4, bad         # measured: see test_the_window_path_decides' docstring
    assert {k for _, _, k in fam.pairs} == {"continuation"}


def test_positions_has_the_bad_octet_at_every_index():
    fam = S.positions()
    for tag in S.CHECKED:
        for where in ("subject", "issuer"):
            at = lambda n, shape: {m["at"] for m in by_kind(fam, "bad") if (m.get("tag"), m["where"], m.get("n"), m["shape"]) == (tag, where, n, shape)}
            assert at(300, "plain") == set(range(300))
            assert at(700, "plain") == {m + d for m in range(0, 700, 64) for d in (-2, -1, 0, 1, 2) if 0 <= m + d < 700} | {699}
            for shape in ("multi", "long_oid"):
                assert at(300, shape) == set(range(0, 300, 11)) | {299}
    for where in ("subject", "issuer"):
        chain = [m for m in by_kind(fam, "bad") if m["shape"] == "fast_chain" and m["where"] == where]
        assert {(m["rdn"], m["at"]) for m in chain} == {(r, i) for r in range(S.FAST_CHAIN) for i in range(53)}
        assert {m["tag"] for m in chain} == set(S.CHECKED)
    ps = parsed("positions")
    for i, j, _ in fam.pairs:                                   # the twins differ where the mark says the bad octet is
        m, a, b = fam.marks[j], fam.certs[i][0], fam.certs[j][0]
        lo, _ = first_and_last_difference(a, b)
        if m["shape"] == "fast_chain":
            assert fast_form(a[lo - m["at"] - 11:]) and a[lo - m["at"] - 11:][10] == 53
        else:
            cv = S.value_start(a, m["tag"], m["n"])
            assert lo == cv + m["at"]
            if m["shape"] == "multi":                           # the SET holds two attributes; long_oid: nine octets of OID
                assert a[cv - 4 - 5 - 4 - 14 - 4] == 0x31 and b"multi" in a[cv - 4 - 5 - 4 - 14:cv]
            if m["shape"] == "long_oid":
                assert a[cv - 4 - 11:cv - 4] == D.tlv(0x06, S.LONG_OID)
    assert ps[0].ok


def test_positions_edge_puts_the_bad_octet_on_both_sides_of_the_first_windows_end():
    """Issuer: the bad octet at every certificate offset 180..280 for every serial length 1..20 — the first windows end at
    224 (minus the payload address mod 4).  Subject: at every offset 200..250 from the subject Name's contents, where the
    window refilled for the subject begins (rounded down to a dword or a 16-octet boundary of the payload: up to 15 in
    front), so its end lies at 209..224 from there."""
    fam, ps = S.positions_edge(), parsed("positions_edge")
    seen = {"issuer": {}, "subject": {}}
    for i, j, _ in fam.pairs:
        m, a, b = fam.marks[j], fam.certs[i][0], fam.certs[j][0]
        if m["et"]:
            continue
        lo, _ = first_and_last_difference(a, b)
        assert lo == m["cv"] + m["at"] and ps[j].serial_len == m["serial_len"] and m["n"] == S.EDGE_N == 260
        assert m["cv"] == S.value_start(a, m["tag"], 260) and 0 <= m["at"] < 260 - 2
        if m["where"] == "subject":
            assert m["cs"] - 4 == ps[j].issuer_off + ps[j].issuer_len + 32 and a[m["cs"] - 4] == 0x30   # behind the validity
            lo -= m["cs"]
        else:
            assert ps[j].issuer_off < m["cv"] < ps[j].issuer_off + ps[j].issuer_len
        seen[m["where"]].setdefault(m["serial_len"], {})[lo] = m["at"]
    for where, offsets in (("issuer", S.ISSUER_OFFSETS), ("subject", S.SUBJECT_OFFSETS)):
        assert set(seen[where]) == set(range(1, 21))
        for ln, at in seen[where].items():
            assert set(at) == set(offsets), (where, ln)
        assert min(offsets) <= W - 24 and max(offsets) >= W + 8
    assert list(S.ISSUER_OFFSETS) == list(range(180, 281)) and list(S.SUBJECT_OFFSETS) == list(range(200, 251))
    for off in S.ISSUER_OFFSETS:                               # from serial to serial: every residue of the value's 16-octet steps
        assert {seen["issuer"][ln][off] % 16 for ln in range(1, 21)} == set(range(16)), off
    assert {fam.marks[j]["tag"] for _, j, _ in fam.pairs if fam.marks[j]["where"] == "issuer"} == set(S.CHECKED)
    assert {fam.marks[j]["tag"] for _, j, _ in fam.pairs if fam.marks[j]["where"] == "subject"} == set(S.CHECKED)


def test_positions_end_puts_the_end_of_a_value_across_the_end_of_its_window():
    """The value's end at every certificate offset 216..232 (issuer) and every offset 200..228 from the subject Name's
    contents, for sixteen value lengths (every residue mod 16), the twins differing in the value's LAST octet alone.  And a
    condition on the inputs: in the window simulation the read of the value's last word reaches across the window's end —
    a miss whose position lies inside the value — for 176 of the 2944 certificates in the packed batch and 192 in the line
    view (measured), and nothing else in the family misses: these are the reads WinReaderS::ld4 clamps and must report."""
    fam, ps = S.positions_end(), parsed("positions_end")
    seen = {"issuer": set(), "subject": set()}
    for i, j, _ in fam.pairs:
        m, a, b = fam.marks[j], fam.certs[i][0], fam.certs[j][0]
        lo, hi = first_and_last_difference(a, b)
        cv = S.value_start(a, m["tag"], m["n"])
        assert hi - lo == 1 and lo == cv + m["n"] - 1 and 32 < m["n"] <= 64        # past touch(a, 32), within one hint
        if m["where"] == "subject":
            s0 = ps[j].issuer_off + ps[j].issuer_len + 32                        # the subject Name, behind the validity
            assert a[s0] == 0x30 and a[s0 + 1] == 0x81
            lo -= s0 + 3
        seen[m["where"]].add((m["n"], lo + 1))
        assert lo + 1 == m["end"]
    assert seen["issuer"] == {(n, e) for n in range(33, 49) for e in range(216, 233)}
    assert seen["subject"] == {(n, e) for n in range(33, 49) for e in range(200, 229)}
    assert {fam.marks[j]["tag"] for _, j, _ in fam.pairs} == set(S.CHECKED)
    b = fam.batch()
    for what, base in (("packed", b.offsets.astype(np.int64)), ("view", S.G.line_view(b)[1].astype(np.int64))):
        across = 0
        for k, (der, _, _) in enumerate(fam.certs):
            m = fam.marks[k]
            ok, _, misses, _, first_miss, _, defer = harness.walk_window(der, int(base[k]) % 128, W, strings=True, ext=True)
            assert ok and defer == 0
            if misses:
                end = der.index(D.tlv(m["tag"], S.filler(m["tag"]) * m["n"])[:-1]) + 2 + m["n"]
                assert end - m["n"] <= first_miss < end, (what, k, m)
                across += 1
        print("positions_end,", what, ": reads across the window's end:", across)
        assert across >= 150 and across <= len(fam.certs) // 8


def test_the_issuer_table():
    t = S.issuers()
    n = len(t.cas)
    assert 2000 <= n < 4096 and n == len(t.valid) == len(t.leaves) == len(t.marks)     # (one engine takes 6000 and more)
    assert sum(t.valid) >= 300 and n - sum(t.valid) >= 1500
    spkis = set()
    for k, ca in enumerate(t.cas):
        o = orc.parse_cert(ca)
        assert o.ok and not o.nonfatal and not o.spki_findings and o.is_ca and (o.string_findings == 0) == t.valid[k], (k, t.marks[k])
        assert harness.product_name_strings(ca) == int(t.valid[k])
        spkis.add(ca[o.spki_off:o.spki_off + o.spki_len])
        leaf = orc.parse_cert(t.leaves[k][0])
        assert leaf.ok and not leaf.nonfatal and not leaf.string_findings and t.leaves[k][1] == k % 2
    assert len(spkis) == n
    cover = {c for m in t.marks for c in m.get("cover", [])}
    assert cover == {(tag, b, lane) for tag in (0x13, 0x0c) for b in range(256) for lane in range(4)}
    assert {(m["entry"], m["pre"]) for m in t.marks if "entry" in m} == {(e, pre) for e in range(len(S.utf8_table())) for pre in range(20)}
    assert {m["where"] for m in t.marks} == {"subject", "issuer"}
    assert {(m["kind"], m["where"]) for m in t.marks} >= {(k, w) for k in ("outside", "inside", "valid", "invalid", "lone", "replaced")
                                                          for w in ("subject", "issuer")}


@functools.lru_cache(maxsize=None)
def windows(name):
    """harness.walk_window of every certificate at the phase the packed batch gives it."""
    fam = S.FAMILIES[name]()
    base = fam.batch().offsets.astype(np.int64)
    return [harness.walk_window(c[0], int(base[k]) % 128, W, strings=True, ext=True) for k, c in enumerate(fam.certs)]


@pytest.mark.parametrize("name", ["alphabet", "lengths", "utf8_edges"])
def test_the_window_path_decides(name):
    """A condition on the INPUTS: the host simulation of the window walk (224 octets, strings and extensions on) decides at
    least 95 % of the family with no miss and no defer_exact, so that on the device the WINDOW path is what answers.
    Measured: alphabet 7318 of 7318, lengths 6004 of 6004, utf8_edges 7640 of 7640 certificates without a miss or a
    deferral; 782 of the 2000 random strings are invalid by Python's decoder."""
    res = windows(name)
    hit = sum(r[0] and r[2] == 0 and r[6] == 0 for r in res)
    print(name, "decided by the window:", hit, "of", len(res))
    assert all(r[0] for r in res) and hit >= 0.95 * len(res), (name, hit, len(res))


def test_long_values_refill_their_window_as_often_as_their_hints_say():
    """positions: every certificate with a value of 300 or 700 octets shows at least one per-lane refill, none a miss.
    And no more refills than the hints of value_strings_ok ask for: a refill puts the window's start at most 15 octets in
    front of the hinted position, the hints come every 64 octets and ask for 64, so the next refill is due no sooner than
    three hints later (15 + 128 + 64 <= 224 < 192 + 64) — at most 1 + n // 192 inside a value of n octets, and a second
    walk through the automaton for a UTF8String that holds an octet >= 0x80.  Everything else in these certificates (the
    headers of both Names, the key, the tail) takes 3 refills at the most.  Measured: 2..4 refills with a value of 300
    octets, 4..8 with one of 700; with the value's hint enlarged from 64 to 256 the simulation refills at every hint and the
    clean 700-octet value takes 11."""
    fam, res = S.positions(), windows("positions")
    seen = {}
    for k, m in enumerate(fam.marks):
        if m.get("n") not in (300, 700):
            continue
        ok, refills, misses, _, _, _, defer = res[k]
        walks = 2 if m["tag"] == 0x0c and m["kind"] == "bad" else 1
        assert ok and misses == 0 and defer == 0, (k, m)
        assert 1 <= refills <= 3 + walks * (1 + m["n"] // 192), (k, m, refills)
        lo, hi = seen.get(m["n"], (99, 0))
        seen[m["n"]] = (min(lo, refills), max(hi, refills))
    print("refills:", seen)
    assert set(seen) == {300, 700}
    # the sweeps around the windows' ends: decided by the window as well
    edge = windows("positions_edge")
    assert all(r[0] and r[2] == 0 and r[6] == 0 for r in edge)
    assert min(r[1] for r in edge) >= 1
