"""Cases for the partition of a known image by a probe image (test helper, no test): a known image K, a probe image P, a
`now`, and the two images expected — include/ctmr.h ctmr_known_image_split, DESIGN.md §28.

The expectation is worked out here from the Python lists the images are written from, with sets and list
comprehensions only, and written with tests/find_corpus.py's `raw_image` (struct.pack, the order given): it never goes
through known_image.split (the twin under test in tests/test_split_corpus_cpu.py), known_image.build or the images'
bytes.  Host keys get their date strings from `datetime`.

Families (`FAMILIES`: name → function returning [Case]):
  counts      0, 1, 63, 64, 65, 255, 256, 257 and 1 025 records in K with as many probes, half of them held
  patterns    1 025 records in one set: no hit, all, every other record, lane 0 of each wave only, lane 63 only, a run
              of hits across a wave edge (60..70) and across a block edge (250..262), the last record only
  boundaries  257 one-member sets hit alternately (half the sets vanish from each side), a 768-record set next to
              them, a set entirely hit beside one entirely missed, an issuer whose every set goes to one side (the issuer
              tables differ, ordinals are renumbered), a digest K lists twice
  hours, misses, lengths, now, repeats, host
              the operands of the find's families of the same names (tests/find_corpus.py), taken as they are: one
              serial under 1, 2 and 300 hours with hours before 1970; the near misses; every serial length 0..40 on both
              sides; the edges of `now` and hours outside the years 0000..9999; repeated records and probes; members of
              41..45 octets, host pairs the member section could carry, a day key, a date that does not parse; and
              `host_sides`: kept host pairs of both kinds on both sides
  canonical   a K that known_image.build wrote, both sections used
"""
import contextlib
import struct
from dataclasses import dataclass, field

import numpy as np

from ct_mapreduce_amd import known_image as KI

import find_corpus as FC

INT64_MIN = FC.INT64_MIN
H0 = FC.H0
COUNTS = FC.COUNTS


@dataclass
class Case:
    name: str
    known: bytes
    probes: bytes
    now: int
    hit: bytes
    miss: bytes
    family: str = ""
    notes: dict = field(default_factory=dict)


def expected(k_sets, k_host, wanted, now):
    """(hit, miss, sets of K kept, sets in hit, sets in miss): K's kept sets in key order, each with the members on
    that side in the order given, a set left empty dropped; K's kept host pairs in (key, member) order."""
    sets, host = ([], []), ([], [])
    ordered = sorted(k_sets, key=lambda s: KI.set_key(s[0], s[1]))
    n_kept = 0
    for hour, dg, ms in ordered:
        if not FC.kept(hour, now):
            continue
        n_kept += 1
        on = [(FC.ident(dg), bytes(m)) in wanted for m in ms]
        for side in (0, 1):
            part = [bytes(m) for m, w in zip(ms, on) if w == (side == 0)]
            if part:
                sets[side].append((hour, dg, part))
    spans = {(k, m): (hour, span) for k, m, hour, span in k_host}
    for key, m in sorted(spans):
        hour, span = spans[(key, m)]
        if hour is not None and now < (hour + span) * 3600:
            host[(key.split(b"::")[2], bytes(m)) not in wanted].append((key, m))
    return FC.raw_image(sets[0], host[0])[0], FC.raw_image(sets[1], host[1])[0], n_kept, len(sets[0]), len(sets[1])


def case(name, k_sets, p_sets, now, k_host=(), p_host=(), **notes):
    """The arguments of find_corpus.case.  k_host: [(key, member, hour or None, hours the key lasts)]; p_host: [(key,
    member, Issuer.ID)]."""
    wanted = {(FC.ident(dg), bytes(m)) for _, dg, ms in p_sets for m in ms} | {(i, bytes(m)) for _, m, i in p_host}
    known = FC.raw_image(k_sets, [(k, m) for k, m, _, _ in k_host])[0]
    probes = FC.raw_image(p_sets, [(k, m) for k, m, _ in p_host])[0]
    hit, miss, n_kept, n_hit, n_miss = expected(k_sets, k_host, wanted, now)
    notes.update(sets_kept=n_kept, hit_sets=n_hit, miss_sets=n_miss)
    return Case(name, known, probes, now, hit, miss, notes=notes)


@contextlib.contextmanager
def _find_families_build_split_cases():
    """find_corpus's family functions hand their lists to find_corpus.case: while this is open they hand them to `case`
    above, so the two corpora share operands and differ in what is expected of them."""
    saved = FC.case
    FC.case = case
    try:
        yield
    finally:
        FC.case = saved


def _from_find(family):
    def make():
        with _find_families_build_split_cases():
            return [c for c in family() if isinstance(c, Case)]
    return make


def _counts_case(n, seed):
    """K: n records — issuer 0 holds three quarters in one set, issuer 1 the rest in one-member sets of consecutive
    hours, members in drawn order.  P: n probes, half of them members of K under the right issuer."""
    rng = np.random.default_rng(seed)
    ser = FC._serials(rng, 2 * n)
    rng.shuffle(ser)
    big = n * 3 // 4
    k_sets = ([(H0, FC.digest(0), ser[:big])] if big else []) + [(H0 + 1 + i, FC.digest(1), [ser[big + i]]) for i in range(n - big)]
    owner = {m: 0 for m in ser[:big]}
    owner.update({m: 1 for m in ser[big:n]})
    present = [ser[i] for i in rng.permutation(n)[:n // 2]] if n else []
    by = {0: [], 1: []}
    for m in present:
        by[owner[m]].append(m)
    for i, m in enumerate(ser[n:n + n - len(present)]):
        by[i & 1].append(m)
    p_sets = [(0, FC.digest(d), ms) for d, ms in by.items() if ms]
    return case("counts-%d" % n, k_sets, p_sets, INT64_MIN, n=n)


def counts():
    return [_counts_case(n, 400 + n) for n in COUNTS]


PATTERNS = {
    "none": lambda i: False,
    "all": lambda i: True,
    "every-other": lambda i: i % 2 == 1,
    "lane-0": lambda i: i % 64 == 0,
    "lane-63": lambda i: i % 64 == 63,
    "run-60-70": lambda i: 60 <= i <= 70,
    "run-250-262": lambda i: 250 <= i <= 262,
    "last": lambda i: i == 1024,
}


def patterns():
    rng = np.random.default_rng(77)
    ser = FC._serials(rng, 1025 + 40)
    rng.shuffle(ser)
    members, absent = ser[:1025], ser[1025:]
    out = []
    for name, f in PATTERNS.items():
        held = [m for i, m in enumerate(members) if f(i)]
        p_sets = [(0, FC.digest(0), held + absent)]
        out.append(case("pattern-" + name, [(H0, FC.digest(0), members)], p_sets, INT64_MIN, hits=len(held)))
    return out


def listed_twice():
    """A K whose issuer table names digest(0) twice: ordinal 0 under H0, ordinal 1 under H0 + 1, digest(1) as ordinal 2.
    Written here field by field; the results name every digest once."""
    a, b = FC.digest(0), FC.digest(1)
    assert a < b
    s, t, u = b"\x41\x42", b"\x43", b"\x44\x45\x46"
    table = [a, a, b]
    sets = [(H0, 0, [s, t]), (H0 + 1, 1, [t, s, u]), (H0 + 1, 2, [s])]
    members = [m for _, _, ms in sets for m in ms]
    set_part, first = [], 0
    for hour, ordinal, ms in sets:
        set_part.append(struct.pack("<iIQQ", hour, ordinal, first, len(ms)))
        first += len(ms)
    meta = struct.pack("<8sIIIIQQQQQ", b"CTMRKNWN", 1, 64, len(table), 0, len(sets), first, 0, 0, 0) + b"".join(table) + b"".join(set_part)
    meta += b"\0" * (-len(meta) % 64)
    known = meta + b"".join(struct.pack("<Q", len(m)) + m.ljust(40, b"\0") for m in members)
    probes = FC.raw_image([(0, a, [s]), (0, b, [u])])[0]
    hit = FC.raw_image([(H0, a, [s]), (H0 + 1, a, [s])])[0]
    miss = FC.raw_image([(H0, a, [t]), (H0 + 1, a, [t, u]), (H0 + 1, b, [s])])[0]
    return Case("boundary-digest-twice", known, probes, INT64_MIN, hit, miss, notes=dict(sets_kept=3, hit_sets=2, miss_sets=3))


def boundaries():
    rng = np.random.default_rng(91)
    ser = FC._serials(rng, 257 + 768 + 20)
    rng.shuffle(ser)
    ones, big, absent = ser[:257], ser[257:1025], ser[1025:]
    one_sets = [(H0 + 1 + i, FC.digest(1), [m]) for i, m in enumerate(ones)]
    out = [case("boundary-257-sets", one_sets, [(0, FC.digest(1), ones[::2] + absent)], INT64_MIN)]
    # the large set in front of the one-member sets (its key is lower), every third of its records hit
    out.append(case("boundary-768-and-257", [(H0, FC.digest(1), big)] + one_sets, [(0, FC.digest(1), big[::3] + ones[1::2])], INT64_MIN))
    # … and behind them, under another issuer of a later hour
    out.append(case("boundary-257-and-768", one_sets + [(H0 + 400, FC.digest(0), big)],
                    [(0, FC.digest(1), ones[::2]), (0, FC.digest(0), big[5::7])], INT64_MIN))
    s, t, u = ser[0], ser[1], ser[2]
    out.append(case("boundary-whole-sets", [(H0, FC.digest(0), [s, t]), (H0 + 1, FC.digest(0), [u, absent[0]]), (H0 + 2, FC.digest(0), [s, u])],
                    [(0, FC.digest(0), [s, t])], INT64_MIN))
    # issuer 0 is hit in every set, issuer 2 in none, issuer 1 in both ways: HIT names digests 0 and 1, MISS 1 and 2
    out.append(case("boundary-issuer-sides", [(H0, FC.digest(0), [s, t]), (H0 + 3, FC.digest(0), [u]), (H0, FC.digest(1), [s, t]),
                                              (H0 + 1, FC.digest(2), [s]), (H0 + 2, FC.digest(2), [t, u])],
                    [(0, FC.digest(0), [s, t, u]), (0, FC.digest(1), [t])], INT64_MIN))
    out.append(listed_twice())
    return out


def host_sides():
    """Kept host pairs on both sides: of two long members and two pairs the member section could carry, P holds one
    each — the long one in its host section, the short one as a member record —, and a pair under a key of no date."""
    a = FC.digest(0)
    longs = [bytes([90 + n]) * n for n in (41, 45)]
    s, t = b"\x51\x52", b"\x53" * 40
    key = FC.host_key(H0 + 3, a)
    k_host = [(key, longs[0], H0 + 3, 1), (key, longs[1], H0 + 3, 1), (key, s, H0 + 3, 1), (key, t, H0 + 3, 1),
              (b"serials::never::" + FC.ident(a), s, None, 0)]
    p_host = [(FC.host_key(0, a), longs[1], FC.ident(a))]
    return [case("host-sides", [(H0, a, [s, t])], [(0, a, [t])], INT64_MIN, k_host, p_host)]


def canonical():
    """A K known_image.build wrote — both sections, sorted, each member once — and probes of both sections."""
    rng = np.random.default_rng(5)
    ser = FC._serials(rng, 120, 1, 40)
    longs = [bytes([60 + n]) * n for n in range(41, 45)]
    k_sets = [(H0 + h, FC.digest(d), sorted(ser[20 * (2 * h + d):20 * (2 * h + d) + 20])) for h in range(3) for d in range(2)]
    k_host = [(FC.host_key(H0 + 1, FC.digest(0)), m, H0 + 1, 1) for m in longs] + [(b"serials::soon::" + FC.ident(FC.digest(0)), ser[0], None, 0)]
    as_dict = {KI.set_key(h, dg): list(ms) for h, dg, ms in k_sets}
    for k, m, _, _ in k_host:     # (the key of the long members is the key of a set record too: one key, both sections)
        as_dict.setdefault(k, []).append(m)
    known = KI.build(as_dict)
    p_sets = [(0, FC.digest(0), sorted(ser[::3])), (0, FC.digest(1), sorted(ser[1::3]))]
    p_host = [(FC.host_key(0, FC.digest(0)), m, FC.ident(FC.digest(0))) for m in longs[::2]]
    c = case("canonical", k_sets, p_sets, (H0 + 1) * 3600, k_host, p_host)
    assert c.known == known, "raw_image of sorted lists is the canonical image"
    return [c]


FAMILIES = {"counts": counts, "patterns": patterns, "boundaries": boundaries, "hours": _from_find(FC.hours),
            "misses": _from_find(FC.misses), "lengths": _from_find(FC.lengths), "now": _from_find(FC.now_edges),
            "repeats": _from_find(FC.repeats), "host": lambda: _from_find(FC.host)() + host_sides(), "canonical": canonical}


def all_cases():
    out = []
    for family, f in FAMILIES.items():
        for c in f():
            c.family = family
            out.append(c)
    return out
