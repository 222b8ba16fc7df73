"""known_image.split — the CPU twin of Engine.known_image_split (include/ctmr.h ctmr_known_image_split) —
held byte for byte to the two images tests/split_corpus.py writes from plain lists, the corpus held to the coverage it
promises, and the results taken through parse, find and image_lists.  No GPU."""
import numpy as np
import pytest

from ct_mapreduce_amd import known_image as KI

import find_corpus as FC
import split_corpus as SC
from test_find_corpus_cpu import DAMAGED, GOOD

CASES = SC.all_cases()
BY_NAME = {c.name: c for c in CASES}


def header(img):
    return dict(zip(("issuers", "sets", "members", "host_members"), (lambda h: (h[3], h[5], h[6], h[8]))(KI._HEADER.unpack_from(img, 0))))


def test_case_names_are_unique():
    assert len(BY_NAME) == len(CASES)


@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_twin_matches_the_expectation(name):
    c = BY_NAME[name]
    hit, miss = KI.split(c.known, c.probes, c.now)
    assert hit == c.hit
    assert miss == c.miss


# ---- the corpus covers what it says

def test_every_family_is_present():
    assert {c.family for c in CASES} == set(SC.FAMILIES) == {"counts", "patterns", "boundaries", "hours", "misses", "lengths", "now",
                                                            "repeats", "host", "canonical"}
    assert {c.name for c in CASES} >= {c.name for c in FC.all_cases() if not c.name.startswith("counts-")}


def test_counts_family_has_every_count_on_both_operands():
    cs = {c.notes["n"]: c for c in SC.counts()}
    assert set(cs) == set(SC.COUNTS) == {0, 1, 63, 64, 65, 255, 256, 257, 1025}
    for n, c in cs.items():
        assert header(c.known)["members"] == n and header(c.probes)["members"] == n
        assert header(c.hit)["members"] == n // 2 and header(c.miss)["members"] == n - n // 2
    big = KI._SET.unpack_from(cs[1025].known, 64 + 64)
    assert big[3] >= 3 * 256 and header(cs[1025].known)["sets"] - 1 >= 4 * 64


def test_every_pattern_reaches_the_side_it_names():
    n = 1025
    for name, f in SC.PATTERNS.items():
        c = BY_NAME["pattern-" + name]
        hits = sum(f(i) for i in range(n))
        assert c.notes["hits"] == hits and header(c.known) == dict(issuers=1, sets=1, members=n, host_members=0)
        assert (header(c.hit)["members"], header(c.miss)["members"]) == (hits, n - hits)
        if name not in ("none", "all"):
            assert 0 < hits < n                       # both sides
    assert BY_NAME["pattern-none"].notes["hits"] == 0 and BY_NAME["pattern-all"].notes["hits"] == n
    assert header(BY_NAME["pattern-none"].hit)["sets"] == 0 and header(BY_NAME["pattern-all"].miss)["sets"] == 0


def test_boundaries_drop_sets_and_issuers():
    c = BY_NAME["boundary-257-sets"]
    assert (header(c.known)["sets"], header(c.hit)["sets"], header(c.miss)["sets"]) == (257, 129, 128)
    c = BY_NAME["boundary-768-and-257"]
    assert KI._SET.unpack_from(c.known, 64 + 32)[3] == 768 and header(c.hit)["sets"] == 1 + 128 and header(c.miss)["sets"] == 1 + 129
    c = BY_NAME["boundary-257-and-768"]
    assert KI._SET.unpack_from(c.known, 64 + 64 + 24 * 257)[3] == 768
    c = BY_NAME["boundary-whole-sets"]
    assert (header(c.known)["sets"], header(c.hit)["sets"], header(c.miss)["sets"]) == (3, 2, 2)
    c = BY_NAME["boundary-issuer-sides"]
    hit, miss = KI.parse(c.hit), KI.parse(c.miss)
    assert hit.issuers == [FC.digest(0), FC.digest(1)] and miss.issuers == [FC.digest(1), FC.digest(2)]
    assert KI.parse(c.known).issuers == [FC.digest(0), FC.digest(1), FC.digest(2)]
    # … renumbered: digest(1) is ordinal 1 in K and in HIT, ordinal 0 in MISS
    def named(img):
        h = header(img)
        recs = [KI._SET.unpack_from(img, 64 + 32 * h["issuers"] + 24 * s) for s in range(h["sets"])]
        return {(r[0], img[64 + 32 * r[1]:96 + 32 * r[1]]): r[1] for r in recs}
    assert named(c.hit) == {(FC.H0, FC.digest(0)): 0, (FC.H0, FC.digest(1)): 1, (FC.H0 + 3, FC.digest(0)): 0}
    assert named(c.miss) == {(FC.H0, FC.digest(1)): 0, (FC.H0 + 1, FC.digest(2)): 1, (FC.H0 + 2, FC.digest(2)): 1}
    c = BY_NAME["boundary-digest-twice"]
    assert KI.parse(c.known).issuers == [FC.digest(0), FC.digest(0), FC.digest(1)]
    assert KI.parse(c.hit).issuers == [FC.digest(0)] and KI.parse(c.miss).issuers == [FC.digest(0), FC.digest(1)]
    assert any(c.notes["hit_sets"] < c.notes["sets_kept"] and header(c.hit)["issuers"] < header(c.known)["issuers"] for c in CASES)


def test_hours_family_names_every_hour():
    for n in (1, 2, 300):
        c = BY_NAME["hours-%d" % n]
        s = b"\x01\x02\x03\x04\x05\x06\x07\x08"
        hours = [int(k[9:13]) for k, ms in KI.parse(c.hit).sets.items() if s in ms and k.endswith(FC.ident(FC.digest(0)))]
        assert len(hours) == n and (n < 2 or min(hours) < 1970)


def test_sets_that_are_not_kept_are_in_neither_result():
    for name in ("now-kept", "now-dropped", "now-all-gone", "now-early", "now-min-years", "now-years-late", "host-now", "host-day-gone"):
        c = BY_NAME[name]
        kept = sum(FC.kept(KI._SET.unpack_from(c.known, 64 + 32 * header(c.known)["issuers"] + 24 * s)[0], c.now)
                   for s in range(header(c.known)["sets"]))
        assert c.notes["sets_kept"] == kept
    assert header(BY_NAME["now-all-gone"].hit)["members"] == header(BY_NAME["now-all-gone"].miss)["members"] == 0
    assert BY_NAME["now-kept"].hit != BY_NAME["now-dropped"].hit
    wide = BY_NAME["now-min-years"]
    assert header(wide.hit)["members"] + header(wide.miss)["members"] == header(wide.known)["members"] - 4


def test_host_family_reaches_both_sides_in_both_sections():
    c = BY_NAME["host"]
    hit, miss = header(c.hit), header(c.miss)
    assert hit["host_members"] == 10 and miss["host_members"] == 0 and hit["members"] == 2 and miss["members"] == 0
    sides = BY_NAME["host-sides"]
    assert (header(sides.hit)["host_members"], header(sides.miss)["host_members"]) == (2, 2)
    assert sorted(len(m) for _, m in KI.records(sides.hit)[1]) == [40, 45] and sorted(len(m) for _, m in KI.records(sides.miss)[1]) == [2, 41]
    assert (header(sides.hit)["members"], header(sides.miss)["members"]) == (1, 1)
    pairs = KI.records(c.hit)[1]
    s = b"\x31\x32\x33"
    assert (FC.host_key(FC.H0 + 3, FC.digest(0)), s) in pairs                      # a pair the member section could carry: left there
    assert (FC.host_key(FC.H0 + 30, FC.digest(0), day=True), s) in pairs
    assert (b"serials::2025-01-01-07::not-a-digest", s) in pairs                   # met by P's host section only
    gone = KI.records(BY_NAME["host-day-gone"].hit)[1]
    assert (FC.host_key(FC.H0 + 30, FC.digest(0), day=True), s) not in gone
    assert (FC.host_key(FC.H0 + 30, FC.digest(0), day=True), s) in KI.records(BY_NAME["host-day-last"].hit)[1]
    everywhere = KI.records(c.hit)[1] + KI.records(c.miss)[1]
    assert not any(k.startswith(b"serials::soon::") or b"02-30" in k for k, _ in everywhere)   # a date that does not parse


def test_repeats_are_carried():
    c = BY_NAME["repeats"]
    s = b"\x21\x22\x23\x24"
    assert [m for _, m in KI.records(c.hit)[0]].count(s) == 3


def test_a_canonical_image_gives_canonical_results():
    c = BY_NAME["canonical"]
    assert KI.union(c.known) == c.known
    for img in (c.hit, c.miss):
        assert KI.build(KI.parse(img).sets) == img and header(img)["members"] and header(img)["host_members"]
    spans = {k: KI.exp_date_span(k.split(b"::")[1]) for k in KI.parse(c.known).sets}
    kept = KI.build({k: ms for k, ms in KI.parse(c.known).sets.items() if spans[k] is not None and spans[k][1] > c.now})
    assert kept != c.known and KI.union(c.hit, c.miss) == KI.union(kept) == kept


# ---- round trips through parse, find and image_lists

@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_round_trips(name):
    c = BY_NAME[name]
    hit, miss = KI.split(c.known, c.probes, c.now)
    KI.parse(hit)
    KI.parse(miss)
    # every record of HIT is found by some probe and no probe finds anything in MISS; the probes K answers are HIT's
    in_hit, in_hit_host = KI.find(hit, c.probes, FC.INT64_MIN)
    in_k, in_k_host = KI.find(c.known, c.probes, c.now)
    assert np.array_equal(in_hit, in_k) and np.array_equal(in_hit_host, in_k_host)
    none, none_host = KI.find(miss, c.probes, FC.INT64_MIN)
    assert not none["records"].any() and not none_host["records"].any()
    # … and no member of HIT is without a probe (P's sections read as find reads them: its dates are not looked at)
    probes = {(ident, m) for part in KI._sections(c.probes) for _, ident, m in part}
    assert all((ident, m) in probes for part in KI._sections(hit) for _, ident, m in part)
    assert not any((ident, m) in probes for part in KI._sections(miss) for _, ident, m in part)
    # the lists of HIT plus the lists of MISS hold, per issuer, the lines of the lists of K
    lines = {}
    for img in (hit, miss):
        for ident, text in KI.image_lists(img, c.now):
            lines.setdefault(ident, []).extend(text.splitlines())
    want = {ident: text.splitlines() for ident, text in KI.image_lists(c.known, c.now)}
    assert {i: sorted(v) for i, v in lines.items()} == {i: sorted(v) for i, v in want.items() if v}


# ---- rejections

@pytest.mark.parametrize("name", [n for n, _ in DAMAGED])
def test_twin_rejects_what_parse_rejects_in_either_operand(name):
    bad = dict(DAMAGED)[name]
    with pytest.raises(KI.ImageError):
        KI.split(bad, GOOD, 0)
    with pytest.raises(KI.ImageError):
        KI.split(GOOD, bad, 0)


@pytest.mark.parametrize("key", [b"serials::2025-01-01-00", b"serials::a::b::c", b"serials::"])
def test_twin_rejects_a_host_key_that_does_not_split_in_three(key):
    bad, _, _ = FC.raw_image([], [(key, b"\x01")])
    KI.parse(bad)
    for known, probes, now in ((bad, GOOD, 0), (GOOD, bad, 0), (bad, GOOD, 2 ** 62)):
        with pytest.raises(KI.ListsError):
            KI.split(known, probes, now)
