"""The extension corpus of tests/ext_corpus.py holds what it promises (no GPU; every assertion is on the corpus, the oracle
and the HOST build of der_walk.h, never on the device code): the verdict every certificate carries is the oracle's and the
host walk's; twins differ, outside their serials, in the stated octets alone and in their verdict; the deciding octet of
every kind of `slide` lies at every offset of the extension block the encoding allows up to 255 and beyond; the special
element of `san_elements` begins at every offset 2..300 of the subjectAltName's value and, in the line view, at every residue
mod 128 of the payload; and the window simulation (harness.walk_window, 224 octets; harness.walk_window_noreach, flavour S)
agrees with the plain walk on every certificate while it reports, family by family, reads outside the window, defer_exact()
calls and cooperative subjectAltName refills — the paths tests/test_gpu_ext_corpus.py is there to drive.  And a window with
contents of its own (harness.walk_window_stale: stale rows behind a partial refill, clamped reads, poison where nobody
loaded) gives the same verdicts, whatever lies around the certificate."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import ext_corpus as E
from tests import geometry_corpus as G
from tests import harness

W = 224                 # kernels/readers.h WIN_CH_STRICT
NF_STRING, NF_EXT = 4, 16
PHASES = (0, 37)


@functools.lru_cache(maxsize=None)
def parsed(name):
    """Every certificate of a family, parsed by the oracle once."""
    return [orc.parse_cert(c[0]) for c in E.FAMILIES[name]().certs]


def oracle_verdict(o):
    assert o.ok and not o.nonfatal and not o.string_findings and not o.spki_findings, o.err_site
    return E.FATAL if o.ext_fatal else E.FINDING if o.ext_findings else E.STRING_FINDING if o.ext_string_findings else E.CLEAN


def host_verdict(p):
    return E.FATAL if not p.ok else E.FINDING if p.nonfatal & NF_EXT else E.STRING_FINDING if p.nonfatal & NF_STRING else E.CLEAN


def host_walks(der, verdict, where):
    """The host build of the walk with the switch off, on, and with strict_strings as well."""
    harness.product_set_ext(False)
    harness.product_set_strings(True)
    p = harness.product_walk(der)
    assert p.ok and p.nonfatal == 0, where                       # the switch decides: without it nothing is looked at
    harness.product_set_ext(True)
    assert host_verdict(harness.product_walk(der)) == verdict, where
    harness.product_set_strings(False)
    p = harness.product_walk(der)
    assert host_verdict(p) == (E.CLEAN if verdict == E.STRING_FINDING else verdict), where
    harness.product_set_ext(False)


@pytest.mark.parametrize("name", list(E.FAMILIES))
def test_the_corpus_the_oracle_and_the_host_walk_agree_on_every_certificate(name):
    fam, ps = E.FAMILIES[name](), parsed(name)
    assert len(fam.certs) == len(fam.verdict) == len(fam.marks) and len(fam.certs) % 64 != 0
    serials = set()
    for k, (der, issuer_idx, et) in enumerate(fam.certs):
        o = ps[k]
        assert oracle_verdict(o) == fam.verdict[k], (name, k, fam.marks[k])
        host_walks(der, fam.verdict[k], (name, k, fam.marks[k]))
        assert et == k % 2 == fam.marks[k]["et"] and 0 <= issuer_idx < E.N_ISSUERS and not o.is_ca
        serials.add(der[o.serial_off:o.serial_off + o.serial_len])
    assert len(serials) == len(fam.certs) and {len(s) for s in serials} == {8}
    assert set(fam.verdict) >= {E.CLEAN, E.FATAL, E.FINDING} and (name == "san_elements" or E.STRING_FINDING in fam.verdict)
    # the expected status, stated without the oracle: kernels/map.h map_one
    want = fam.expect()
    for k, (_, _, et) in enumerate(fam.certs):
        v = fam.verdict[k]
        assert want[k] == (orc.ST_PARSE_ERROR if v == E.FATAL or (v != E.CLEAN and et == 1) else orc.ST_PASS)
    assert (fam.expect(strict_ext=False) == orc.ST_PASS).all()


def test_rules_has_every_row_of_every_table_once_per_entry_type():
    fam = E.rules()
    assert set(E.TABLES) == {"key_usage", "subject_key_identifier", "ext_key_usage", "authority_key_identifier", "certificate_policies",
                             "authority_info_access", "subject_info_access", "subject_alt_name", "subject_alt_name_uri",
                             "crl_distribution_points", "name_constraints", "sct_list", "ip_addr_block", "as_identifiers"}
    seen = {}
    for k, m in enumerate(fam.marks):
        e, verdict = E.TABLES[m["kind"]][m["row"]]
        o = parsed("rules")[k]
        der = fam.certs[k][0]
        assert der[o.exts_off:o.exts_end] == e + G.bc(False) and verdict == fam.verdict[k] and verdict in E.VERDICTS
        seen.setdefault((m["kind"], m["row"]), []).append(m["et"])
    assert seen == {(t, r): [0, 1] for t, body in E.TABLES.items() for r in range(len(body))}
    assert sum(len(b) for b in E.TABLES.values()) >= 400


def differences(a, b, o):
    """The octets in which two certificates differ outside their serials: (first, last + 1)."""
    d = np.nonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8))[0]
    d = d[(d < o.serial_off) | (d >= o.serial_off + o.serial_len)]
    return int(d[0]), int(d[-1]) + 1


@pytest.mark.parametrize("name", ["slide", "san_elements"])
def test_twins_differ_in_the_stated_octets_and_in_their_verdict(name):
    fam, ps = E.FAMILIES[name](), parsed(name)
    assert len(fam.pairs) >= 48
    for i, j, kind in fam.pairs:
        a, b = fam.certs[i][0], fam.certs[j][0]
        assert len(a) == len(b) and fam.certs[i][1:] == fam.certs[j][1:] and ps[i].not_after == ps[j].not_after, (kind, i, j)
        lo, hi = differences(a, b, ps[i])
        assert hi - lo <= fam.marks[j]["span"] and ps[i].exts_off <= lo and hi <= ps[i].exts_end, (kind, fam.marks[j])
        assert fam.verdict[i] == E.CLEAN != fam.verdict[j]
        assert oracle_verdict(ps[i]) == E.CLEAN and oracle_verdict(ps[j]) == fam.verdict[j]
        assert (ps[i].serial_off, ps[i].serial_len) == (ps[j].serial_off, ps[j].serial_len)


def test_slide_puts_the_deciding_octet_at_every_offset_of_the_extension_block():
    """Per kind: the last octet in which the twins differ, counted from the first Extension (the oracle's exts_off), takes
    every value d0 + 7 .. d0 + 255 (d0: without a filler; an Extension has seven octets at the least, so d0 + 1 .. d0 + 6 do
    not exist, and no octet that decides lies inside its own Extension's headers: below 10) — every offset 64..255 among
    them: one window of 224 octets and two 16-octet refill steps."""
    fam, ps = E.slide(), parsed("slide")
    at = {}
    for i, j, kind in fam.pairs:
        lo, hi = differences(fam.certs[i][0], fam.certs[j][0], ps[i])
        at.setdefault((kind, fam.certs[i][2]), {})[fam.marks[j]["filler"]] = hi - 1 - ps[i].exts_off
        filler_len = sum(len(e) for e in E.filler(fam.marks[j]["filler"]))
        assert filler_len == fam.marks[j]["filler"] and fam.certs[i][0][ps[i].exts_off:].startswith(b"".join(E.filler(filler_len)))
    assert set(at) == {(kind, et) for kind in E.SLIDE_KINDS for et in (0, 1)} and len(E.SLIDE_KINDS) >= 20
    for want in ("key_usage", "subject_key_identifier", "ext_key_usage", "authority_key_identifier", "certificate_policies",
                 "authority_info_access", "san_ip", "san_uri", "dp_rel_name", "nc_dns", "nc_rfc822", "nc_uri", "nc_ip_mask", "sct_list",
                 "ip_addr_block", "as_identifiers"):
        assert want in E.SLIDE_KINDS
    assert E.FILLER_LENGTHS == (0,) + tuple(range(7, 256))
    for (kind, et), offs in at.items():
        d0 = offs[0]
        assert 10 <= d0 <= 57, (kind, d0)
        assert offs == {n: d0 + n for n in E.FILLER_LENGTHS}, kind
        assert set(offs.values()) >= set(range(d0 + 7, d0 + 256)) >= set(range(64, 256)), kind


def header(der, at):
    """(contents, end) of the DER element at `at`."""
    n = der[at + 1]
    if n < 0x80:
        return at + 2, at + 2 + n
    k = n & 0x7f
    return at + 2 + k, at + 2 + k + int.from_bytes(der[at + 2:at + 2 + k], "big")


def san_value(der, o):
    """Certificate offset of the (first) subjectAltName's extnValue contents."""
    at = der.index(bytes.fromhex("0603551d1104"), o.exts_off)
    return header(der, at + 5)[0]


def test_san_elements_puts_the_special_element_at_every_offset_and_every_residue():
    fam, ps = E.san_elements(), parsed("san_elements")
    _, start, _ = G.line_view(fam.batch())
    offsets, residues = {}, {}
    for k, m in enumerate(fam.marks):
        if m["kind"] not in E.SPECIALS:
            continue
        der = fam.certs[k][0]
        cv = san_value(der, ps[k])
        c, ce = header(der, cv)
        at = c + m["fill"]
        assert der[cv] == 0x30 and ce == ps[k].exts_end - len(G.bc(False)) and der[at:].startswith(m["special"]), (k, m)
        assert der[c:at] == b"".join(G.dns_names(m["fill"], m["fill"]))
        offsets.setdefault((m["kind"], m["et"]), set()).add(at - cv)
        residues.setdefault((m["kind"], m["et"]), set()).add((int(start[k]) + at) % 128)
        last = E.SPECIALS[m["kind"]][2]
        if last:                                    # its length runs one octet past the value
            assert at + len(m["special"]) == ce and header(der, at)[1] == ce + 1, (k, m)
        else:
            assert at + len(m["special"]) < ce or m["fill"] == 0, (k, m)
    assert set(offsets) == {(s, et) for s in E.SPECIALS for et in (0, 1)}
    for s in ("uri_good", "uri_bad", "ip4", "ip5", "ip16", "high_tag", "high_tag_illegal", "long_form", "other_name", "truncated"):
        assert s in E.SPECIALS
    assert E.SPECIALS["high_tag"][0] == b"\x9f\x21\x01\x00" and E.SPECIALS["high_tag_illegal"][0] == b"\x9f\x1e\x00"
    assert E.SPECIALS["long_form"][0][:3] == b"\x82\x81\x80" and E.SPECIALS["other_name"][0][0] == 0xa0
    assert [len(E.SPECIALS[s][0]) - 2 for s in ("ip4", "ip5", "ip16")] == [4, 5, 16]
    for key in offsets:                             # (0 and 1 are the SEQUENCE's own header; no element has one octet: 4 + 1 = 3 + 2)
        first = 3 if key[0] == "long_form" else 2   # (131 octets do not fit a SEQUENCE with a header of two)
        assert offsets[key] >= set(range(first, 301)), (key, sorted(set(range(first, 301)) - offsets[key]))
        assert residues[key] == set(range(128)), key
    # the subjectAltName's own headers across the end of the extension window; two of them; an empty one; fatal already
    at = set()
    for k, m in enumerate(fam.marks):
        if m["kind"] == "straddle":
            der = fam.certs[k][0]
            e = der.index(bytes.fromhex("0603551d1104"), ps[k].exts_off) - 4
            assert der[e:e + 2] == b"\x30\x82" and der[e + 9:e + 11] == b"\x04\x82"
            at.add(e - ps[k].exts_off)
    assert at == set(range(200, 224))
    kinds = [m["kind"] for m in fam.marks]
    assert min(kinds.count(k) for k in ("two", "empty", "fatal_before", "fatal_behind")) >= 12
    for k, m in enumerate(fam.marks):
        if m["kind"] == "two":
            assert fam.certs[k][0].count(bytes.fromhex("0603551d1104")) == 2


def window_walks(name):
    """Every certificate through the simulated window at two phases and as a lane out of reach: the same verdict as the
    plain walk.  Returns the sums (misses, defer_exact calls, cooperative refills) of the in-reach simulation."""
    fam = E.FAMILIES[name]()
    misses = defers = coops = decided = 0
    for k, (der, _, _) in enumerate(fam.certs):
        v = fam.verdict[k]
        for phase in PHASES:
            ok, _, miss, _, _, coop, defer = harness.walk_window(der, phase, W, strings=True, ext=True)
            # (a read outside the window or a deferral: the device repeats the certificate with the exact reader, whose
            # verdict is the plain walk's; the window alone must never refuse what the plain walk accepts)
            if miss == 0 and defer == 0:
                assert ok == (v != E.FATAL), (name, k, phase, fam.marks[k])
                decided += 1
            else:
                assert ok or v == E.FATAL, (name, k, phase, fam.marks[k])
            misses, defers, coops = misses + miss, defers + defer, coops + coop
            p, st = harness.walk_window_noreach(der, phase, W, "S", True, True)
            assert host_verdict(p) == v, (name, k, phase, fam.marks[k], st)
    return misses, defers, coops, decided


@pytest.mark.parametrize("name", list(E.FAMILIES))
def test_the_window_walk_agrees_and_the_corpus_drives_the_paths_it_is_meant_to(name):
    """Measured (sums over both phases; misses, defer_exact calls, cooperative refills, walks the window decides alone) —
    rules 48, 1 152, 46, 512 of 1 668; slide 764, 22 000, 696, 17 844 of 40 000; san_elements 24, 2 472, 27 152, 10 028 of 12 516."""
    misses, defers, coops, decided = window_walks(name)
    print(name, "window simulation: misses", misses, "defer_exact", defers, "cooperative refills", coops, "decided by the window alone", decided)
    assert misses >= 1 and defers >= 1 and coops >= 1 and decided >= 1


@pytest.mark.parametrize("name", list(E.FAMILIES))
def test_a_window_with_contents_of_its_own_gives_the_same_verdicts(name):
    """harness.walk_window_stale: the window is a buffer that holds what its refills copied — a partial cooperative refill
    leaves stale rows behind the subjectAltName's end, every read is served from the buffer (clamped and counted, or, for
    ld2, wherever it points), octets nobody loaded are poison, the certificate lies between hostile octets (0xff, 0x30).  A
    walk that used an octet it had not asked for, without a miss, would give another verdict for some certificate here; no
    unclamped read may leave the window at all.  With slack = 0 (coop_refill_lines_to without its `+ 4`) the verdicts are
    the same too: the four octets are a margin — a read that begins in front of the value's end reaches across it, but
    what it finds there never decides (every element must END at or in front of the value's end).  Measured (both phases,
    slack 4 | 0): rules 14 | 14 partial refills, slide 696 | 696, san_elements 9 034 | 9 254."""
    fam = E.FAMILIES[name]()
    partial = {4: 0, 0: 0}
    for k, (der, _, _) in enumerate(fam.certs):
        for phase, fill in zip(PHASES, (0xff, 0x30)):
            for slack in (4, 0):
                p, st = harness.walk_window_stale(der, phase, W, slack, True, True, fill)
                assert host_verdict(p) == fam.verdict[k] and st[5] == 0, (name, k, phase, slack, fam.marks[k], st)
                partial[slack] += st[4]
    print(name, "partial cooperative refills:", partial)
    assert partial[4] >= 1 and partial[0] >= partial[4]


def test_the_window_with_contents_notices_a_refill_that_stops_short():
    """The simulation can fail: a partial refill that stops sixteen octets short of the value's end (slack = -16) leaves the
    last elements of a subjectAltName stale, no read is clamped, and certificates of san_elements come out with another
    verdict than the rules give."""
    fam = E.san_elements()
    wrong = 0
    for k, (der, _, _) in enumerate(fam.certs):
        p, st = harness.walk_window_stale(der, 37, W, -16, True, True, 0xff)
        wrong += host_verdict(p) != fam.verdict[k]
    print("san_elements, a refill sixteen octets short: wrong verdicts", wrong, "of", len(fam.certs))
    assert wrong >= 100


def test_the_issuer_table():
    t = E.chain0()
    n = len(t.cas)
    assert 1000 <= n < 4096 and n == len(t.valid) == len(t.leaves) == len(t.marks) == len(t.verdict)
    spkis, places = set(), {}
    for k, ca in enumerate(t.cas):
        o = orc.parse_cert(ca)
        assert o.is_ca and oracle_verdict(o) == t.verdict[k] and t.valid[k] == (t.verdict[k] == E.CLEAN), (k, t.marks[k])
        harness.product_set_ext(True)
        harness.product_set_strings(True)
        assert host_verdict(harness.product_walk(ca)) == t.verdict[k], (k, t.marks[k])
        harness.product_set_strings(False)
        harness.product_set_ext(False)
        spkis.add(ca[o.spki_off:o.spki_off + o.spki_len])
        leaf = orc.parse_cert(t.leaves[k][0])
        assert oracle_verdict(leaf) == E.CLEAN and t.leaves[k][1] == k % 2
        if "filler" in t.marks[k]:
            places.setdefault(t.marks[k]["kind"], set()).add((t.marks[k]["filler"], t.marks[k]["twin"]))
    assert len(spkis) == n and sum(t.valid) >= 400 and n - sum(t.valid) >= 400
    assert places == {kind: {(f, tw) for f in E.CHAIN0_FILLERS for tw in (0, 1)} for kind in E.SLIDE_KINDS} and len(E.CHAIN0_FILLERS) == 16
    rows = {(m["kind"], m["row"]) for m in t.marks if "row" in m}
    assert rows == {(tb, r) for tb, body in E.TABLES.items() for r in range(len(body))}
