"""known_image.find — the CPU twin of Engine.known_image_find (include/ctmr.h ctmr_known_image_find) — held
to the expectation tests/find_corpus.py works out from plain lists, and the corpus held to the coverage it promises.
No GPU."""
import struct

import numpy as np
import pytest

from ct_mapreduce_amd import known_image as KI

import find_corpus as FC

CASES = FC.all_cases()
BY_NAME = {c.name: c for c in CASES}


def test_case_names_are_unique():
    assert len(BY_NAME) == len(CASES)


@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_twin_matches_the_expectation(name):
    c = BY_NAME[name]
    hits, host_hits = KI.find(c.known, c.probes, c.now)
    assert hits.dtype == KI.HIT_DTYPE and host_hits.dtype == KI.HIT_DTYPE
    assert np.array_equal(hits, FC.as_array(c.hits))
    assert np.array_equal(host_hits, FC.as_array(c.host_hits))


# ---- the corpus covers what it says

def test_counts_family_has_every_count_on_both_sides():
    cs = FC.counts()
    assert {c.notes["n_probes"] for c in cs if c.notes["n_known"] == 257} == set(FC.COUNTS)
    assert {c.notes["n_known"] for c in cs if c.notes["n_probes"] == 65} == set(FC.COUNTS)
    for c in cs:
        assert len(c.hits) == c.notes["n_probes"]
        assert KI.parse(c.known).n_members == c.notes["n_known"]
        if c.notes["n_probes"] > 1 and c.notes["n_known"] > 1:
            found = sum(h[0] > 0 for h in c.hits)
            assert 0 < found < len(c.hits)
    big = BY_NAME["counts-1025-1025"].notes
    assert big["largest_set"] >= 3 * 256 and big["one_member_sets"] >= 4 * 64


def test_hours_family():
    for n in (1, 2, 300):
        c = BY_NAME["hours-%d" % n]
        assert (n, ) == tuple({h[0] for h in c.hits[:1]})
        assert c.hits[0][1] <= c.hits[0][2] and (n < 2 or c.hits[0][1] < 0 < c.hits[0][2])
        assert c.notes["negative"] == n // 2


def test_misses_family():
    c = BY_NAME["misses"]
    n = len(c.hits) // 3
    d0, d1, d2 = c.hits[:n], c.hits[n:2 * n], c.hits[2 * n:]
    # (the members of a set of P are written as given: the order of near[])
    assert [h[0] for h in d0] == [1, 0, 0, 0, 0, 2, 0, 0]      # s; …; "" no; 00 under two hours; 00 00 no; s[:5] is issuer 1's
    assert [h[0] for h in d1] == [0, 0, 0, 0, 0, 0, 0, 1]
    assert all(h == (0, 0, 0) for h in d2)
    assert [h[0] for h in BY_NAME["misses-empty"].hits] == [1, 0, 0, 1]
    assert [h[0] for h in BY_NAME["misses-2p-1k"].hits] == [1, 0]
    assert BY_NAME["misses-1p-2k"].hits == [(2, FC.H0, FC.H0 + 9)]


def test_lengths_family_has_every_length_on_both_sides():
    k, p = set(), set()
    for c in FC.lengths():
        k |= set(c.notes["k_lengths"])
        p |= set(c.notes["p_lengths"])
        assert any(h[0] for h in c.hits) and not all(h[0] for h in c.hits)
    assert k == set(range(41)) and p == set(range(41))


def test_now_family():
    h = FC.H0 + 5
    assert BY_NAME["now-kept"].hits == [(1, h, h), (1, h + 1, h + 1)]
    assert BY_NAME["now-dropped"].hits == [(0, 0, 0), (1, h + 1, h + 1)]
    assert BY_NAME["now-all-gone"].hits == [(0, 0, 0), (0, 0, 0)]
    assert BY_NAME["now-early"].hits == [(2, h - 1, h), (2, h - 1, h + 1)]
    assert BY_NAME["now-min-years"].hits == [(3, FC.HOUR_LO, h), (3, h - 1, FC.HOUR_HI - 1)]
    assert BY_NAME["now-years-late"].hits == [(0, 0, 0), (1, FC.HOUR_HI - 1, FC.HOUR_HI - 1)]
    assert FC.HOUR_LO == KI._HOUR_LO and FC.HOUR_HI == KI._HOUR_HI


def test_repeats_family():
    c = BY_NAME["repeats"]
    # P in image order: issuer 0's probes, then issuer 1's, then issuer 3's (digest order is not ordinal order: by key)
    by = {}
    for (dg, m), h in zip(FC.raw_image([(0, FC.digest(0), [b"\x21\x22\x23\x24", b"\x21\x22\x23", b"\x21\x22\x23\x24", b"\x21\x22\x23\x24",
                                                          b"\x99", b"\x21\x22\x23"]),
                                        (0, FC.digest(3), [b"\x21\x22\x23\x24", b"\x21\x22\x23"]), (0, FC.digest(1), [b"\x99", b"\x99"])])[1], c.hits):
        by.setdefault((dg, m), []).append(h)
    assert by[(FC.digest(0), b"\x21\x22\x23\x24")] == [(3, FC.H0, FC.H0)] * 3
    assert by[(FC.digest(0), b"\x21\x22\x23")] == [(3, FC.H0, FC.H0 + 4)] * 2
    assert by[(FC.digest(1), b"\x99")] == [(1, FC.H0 + 4, FC.H0 + 4)] * 2
    assert by[(FC.digest(3), b"\x21\x22\x23")] == [(0, 0, 0)]


def test_host_family():
    c = BY_NAME["host"]
    _, p_host = KI.records(c.probes)
    got = {(k, m): h for (k, m), h in zip(p_host, c.host_hits)}
    day = (FC.H0 + 30) // 24 * 24
    longs = [bytes([40 + n]) * n for n in range(41, 46)]
    k0 = FC.host_key(0, FC.digest(0))
    assert got[(k0, longs[0])] == (2, FC.H0, FC.H0 + 2)          # the unparsable "soon" key is skipped
    assert got[(k0, longs[2])] == (1, FC.H0, FC.H0)
    assert got[(k0, longs[3])] == (0, 0, 0)
    assert got[(k0, longs[4])] == (1, day, day)
    s, t = b"\x31\x32\x33", b"\x34" * 40
    assert got[(FC.host_key(77, FC.digest(0)), s)] == (3, FC.H0, day)      # a member record, a host pair, the day key
    assert got[(FC.host_key(77, FC.digest(1)), t)] == (2, FC.H0 + 1, FC.H0 + 3)
    assert got[(b"serials::whenever::not-a-digest", s)] == (1, FC.H0 + 7, FC.H0 + 7)
    assert got[(b"serials::whenever::nobody", s)] == (0, 0, 0)
    dev, _ = KI.records(c.probes)
    hit = {(k, m): h for (k, m), h in zip(dev, c.hits)}
    assert hit[(KI.set_key(0, FC.digest(0)), s)] == (3, FC.H0, day)
    assert hit[(KI.set_key(0, FC.digest(1)), t)] == (2, FC.H0 + 1, FC.H0 + 3)
    assert hit[(KI.set_key(0, FC.digest(1)), s)] == (0, 0, 0)
    last, gone = BY_NAME["host-day-last"], BY_NAME["host-day-gone"]
    assert dict(zip(KI.records(last.probes)[0], last.hits))[(KI.set_key(0, FC.digest(0)), s)] == (1, day, day)
    assert dict(zip(KI.records(gone.probes)[0], gone.hits))[(KI.set_key(0, FC.digest(0)), s)] == (0, 0, 0)


# ---- known_image.probes

def test_probes_round_trip():
    longs = [b"\x07" * 41, b"\x08" * 60]
    want = {FC.digest(2): [b"\x01", b"", b"\x02" * 40] + longs, FC.digest(0): [b"\x05\x06", b"\x05\x06"]}
    img = KI.probes(want)
    p = KI.parse(img)
    assert p.sets == {KI.set_key(0, d): sorted(set(ms)) for d, ms in want.items()}
    assert p.n_members == 4 and p.n_host_members == 2 and p.issuers == sorted(want)
    assert KI.build(p.sets) == img
    dev, host = KI.records(img)
    assert [m for _, m in host] == longs and all(k == KI.set_key(0, FC.digest(2)) for k, _ in host)
    hits, host_hits = KI.find(KI.build({KI.set_key(FC.H0, FC.digest(2)): [b"\x01", longs[1]]}), img, 0)
    assert [tuple(h)[:3] for h in hits] == [(0, 0, 0), (0, 0, 0), (1, FC.H0, FC.H0), (0, 0, 0)]
    assert [tuple(h)[:3] for h in host_hits] == [(0, 0, 0), (1, FC.H0, FC.H0)]
    assert KI.parse(KI.probes({})).total == 0


# ---- rejections

def damaged_images():
    """(name, image) of what `parse` rejects, made from a small valid image."""
    good, _, _ = FC.raw_image([(FC.H0, FC.digest(0), [b"\x01\x02", b"\x03"]), (FC.H0 + 1, FC.digest(1), [b"\x04"])],
                              [(FC.host_key(FC.H0, FC.digest(0)), b"\x09" * 41)])
    KI.parse(good)
    b = bytearray(good)
    out = [("short", good[:40]), ("truncated", good[:-48]), ("trailing", good + b"\0" * 48)]

    def patched(name, at, data):
        x = bytearray(b)
        x[at:at + len(data)] = data
        out.append((name, bytes(x)))
    patched("magic", 0, b"X")
    patched("version", 8, struct.pack("<I", 2))
    patched("header-size", 12, struct.pack("<I", 128))
    patched("flags", 20, struct.pack("<I", 1))
    patched("reserved", 56, struct.pack("<Q", 1))
    so = KI.HEADER_BYTES + 64
    patched("ordinal", so + 4, struct.pack("<I", 2))
    patched("gap", so + 24 + 8, struct.pack("<Q", 3))
    patched("empty-set", so + 16, struct.pack("<Q", 0))
    patched("set-order", so, struct.pack("<i", FC.H0 + 2))
    patched("host-count", 48, struct.pack("<Q", 2))
    patched("host-prefix", so + 48 + 4, b"Serials")
    n_mem_at = len(good) - 3 * 48
    patched("serial-len", n_mem_at, struct.pack("<Q", 41))
    patched("padding", n_mem_at + 48 + 8 + 5, b"\x01")
    patched("meta-padding", n_mem_at - 1, b"\x01")
    return good, out


GOOD, DAMAGED = damaged_images()


@pytest.mark.parametrize("name", [n for n, _ in DAMAGED])
def test_twin_rejects_what_parse_rejects_in_either_operand(name):
    bad = dict(DAMAGED)[name]
    with pytest.raises(KI.ImageError):
        KI.parse(bad)
    with pytest.raises(KI.ImageError):
        KI.find(bad, GOOD, 0)
    with pytest.raises(KI.ImageError):
        KI.find(GOOD, bad, 0)


@pytest.mark.parametrize("key", [b"serials::2025-01-01-00", b"serials::a::b::c", b"serials::"])
def test_twin_rejects_a_host_key_that_does_not_split_in_three(key):
    bad, _, _ = FC.raw_image([], [(key, b"\x01")])
    KI.parse(bad)
    with pytest.raises(KI.ListsError):
        KI.find(bad, GOOD, 0)
    with pytest.raises(KI.ListsError):
        KI.find(GOOD, bad, 0)
    # … in K even when now has left the key behind: the key is split before its date is looked at
    with pytest.raises(KI.ListsError):
        KI.find(bad, GOOD, 2 ** 62)


# ---- the edges of now

@pytest.mark.parametrize("hour", [FC.H0, -1, 0, FC.HOUR_LO, FC.HOUR_HI - 1])
def test_the_expiry_edge_of_a_set_record(hour):
    k = FC.raw_image([(hour, FC.digest(0), [b"\x01"])])[0]
    p = KI.probes({FC.digest(0): [b"\x01"]})
    for now, want in (((hour + 1) * 3600 - 1, 1), ((hour + 1) * 3600, 0), (FC.INT64_MIN, 1), (2 ** 63 - 1, 0)):
        hits, _ = KI.find(k, p, now)
        assert tuple(hits[0]) == ((1, hour, hour, 0) if want else (0, 0, 0, 0))


def test_the_expiry_edge_of_a_host_key():
    day = (FC.H0 + 30) // 24 * 24
    long = b"\x02" * 41
    k = FC.raw_image([], [(FC.host_key(FC.H0 + 30, FC.digest(0), day=True), long), (FC.host_key(FC.H0, FC.digest(0)), long)])[0]
    p = KI.probes({FC.digest(0): [long]})
    for now, want in (((FC.H0 + 1) * 3600 - 1, (2, FC.H0, day)), ((FC.H0 + 1) * 3600, (1, day, day)),
                      ((day + 24) * 3600 - 1, (1, day, day)), ((day + 24) * 3600, (0, 0, 0)), (FC.INT64_MIN, (2, FC.H0, day))):
        _, host_hits = KI.find(k, p, now)
        assert tuple(host_hits[0])[:3] == want


def test_merge_hits():
    a = FC.as_array([(0, 0, 0), (2, 5, 9), (1, -7, -7), (0, 0, 0)])
    b = FC.as_array([(0, 0, 0), (1, 3, 3), (0, 0, 0), (4, -2, 8)])
    assert np.array_equal(KI.merge_hits([a, b]), FC.as_array([(0, 0, 0), (3, 3, 9), (1, -7, -7), (4, -2, 8)]))
    assert np.array_equal(KI.merge_hits([a]), a)
