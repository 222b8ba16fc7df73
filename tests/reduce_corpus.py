"""Constructed duplicate and tag patterns for the in-batch reduce of ONE engine (kernels/reduce.h: pass 1 of the insert —
insert_probe_h inside k_map_fused, or k_insert behind map variant 13 —, k_ec_resolve, pass 2 — k_insert2 → insert2_one →
settle_order / mark_dup_ord / index_upsert —, k_resolve, k_scan_blocks, k_compact).  No GPU, no torch.

The hash port and the dict model are tests/xchg_corpus.py's; certificates come from tests/der.py, EC points from
tests/ec_corpus.py.  A case is a list of batches, a batch a list of Entry(der, issuer index, key): key is what the entry
adds to the known set — (expiry hour, canonical issuer, serial octets) — or None when it does not reach the set.  Apart
from the named copies every entry is a filler with a key of its own, so positions can be chosen freely.  Unless a builder
says otherwise a case is the batch, the same batch again (all known: n_new = 0) and the batch reversed (all known, state
unchanged).  tests/test_reduce_corpus_cpu.py holds every builder to what it names and the model to the oracle;
tests/test_gpu_reduce_corpus.py runs the cases on the device under both map variants.

Groups: A multiplicity and placement in one batch · B known and new mixed · C keys that share the 24-bit tag (and the
home slot, or adjacent home slots) of a 64-slot index · D runs that wrap the end of the index · E what is and is not the
same key · F one key under different public keys (strict_spki: an EC key is inserted by k_ec_resolve, BEHIND the RSA keys
of the whole batch — the copy with the lower log index may be the one inserted later).

Capacity of the 64-slot engines (C, D): ensure_capacity leaves the index alone while (occupied + incoming) · 4 <= nslots
· 3, where incoming is the batch's entry count (every entry may claim a slot) and occupied the distinct keys stored so
far: occupied + n <= 48 before every batch (capacity_ok; asserted in the CPU test, and on the device by rebuilds == 0).

Branches and the cases that reach them ("race": which of two entries of one launch comes first is the scheduler's choice —
the case makes the branch likely, and either order must give the model's answer; "order": reached by construction)

  insert_probe_h (pass 1; k_map_fused / k_insert, and k_ec_resolve's insert of a good pending key)
    empty slot claimed                           every filler
    word of an earlier round, equal key          every case's second and third batch (the replay); B
    word of an earlier round, other key, same    C two_batches (C meets A and B), C adjacent_*_behind_filler's second
      tag: probe on                              batch (home slot held by P or Q of the first), D wrap_tag_pair's replay
    word of this round, same tag: DEFER          every in-batch copy (A); in k_ec_resolve: F (the RSA copy claimed inside the
                                                 map, order), A *_ec (all keys EC: copies meet each other in k_ec_resolve)
    other tag or tombstone: probe on             C, D (a 64-slot index at up to 3/4 load), D wrap_* through slot 63 → 0
    table full (ES_FULL)                         not reachable: ensure_capacity runs before every batch and keeps
                                                 occupied + n <= 3/4 · nslots, so every probe meets an empty slot; not forced
  insert2_one (pass 2)
    cell at the candidate slot is my key         every in-batch copy (A)
    cell differs → index_upsert created          C abab / baab / …: the first B defers at A's word and claims the next slot
    cell differs → found, word of this round     C abab, baab, abccba, a3_b_between: the second B (or the first, race)
    cell differs → found, word of an earlier     not reachable in the local reduce: the entry deferred at a word of THIS round
      round                                      that lies on its probe path; that slot was empty when the round began, and a
                                                 key of an earlier round never lies behind an empty slot of its own probe
                                                 path (linear probing; removals leave tombstones, which pass 1 never claims,
                                                 and a rebuild re-inserts every key).  The branch serves received key records
                                                 of the owner-computes exchange (kernels/exchange.h), out of scope here
    cell differs → full (SID_FULL)               not reachable: as ES_FULL above
  settle_order
    word points to my cell                       not reachable from k_insert2: a word points to an entry's cell only when
                                                 that entry claimed (then it is not DEFER) or created (insert2_one returns) or
                                                 moved it itself; reached by k_keys_insert2 (exchange)
    word of an earlier round                     not reachable from k_insert2 (the code says so): words move between
                                                 presenters of this round only
    holder's order lower: I lose                 every in-batch copy whose original claimed (A; F rsa_then_ec, order)
    holder's order higher: word moved,           F ec_then_rsa, F thread4_ec_first (order: k_ec_resolve inserts the lower
      holder marked (mark_dup_ord)               index behind the map); A same_4099, mult_4097, abab_2048 (race)
    compare-and-swap lost, look again            A wave_same, same_4099, mult_* (race between copies settling at once)
  k_ec_resolve
    point off the curve → PARSE_ERROR            F bad_ec_then_rsa, good_ec_then_bad_ec
    good, not ES_PENDING (filtered, host set)    E filtered_first_ec (a CA certificate with an EC key), E lengths_ec (41 octets)
    good, ES_PENDING → pass 1 as above           F, A *_ec
  k_insert2's todo loop                          A thread4_same (≥ 3 DEFER entries in one thread), thread4_distinct (4, race),
                                                 F thread4_rsa_first (4 DEFER entries in one thread, order)
  k_compact's prefix (counts 0..4 per thread)    every case with fillers: threads of four new entries (count 4, the m2 ballot)
                                                 next to threads with copies (counts 0..3)
"""
import calendar
import random
from collections import namedtuple

import numpy as np

from tests import der as D
from tests import xchg_corpus as XC

U = np.uint64
SEED = 20261019
NOW = 1767225600                                   # 2026-01-01: the filter's clock (log_expired off)
NOT_AFTER = XC.NOT_AFTER                           # 2027-01-01 00:00: the hour the port's EXP_HOUR stands for
SLOTS = 64                                         # the small index of groups C and D
BIG_SLOTS = 1 << 14                                # everything else: 3 batches of at most 4 099 entries, no rebuild needed

Entry = namedtuple("Entry", "der iss key")
Case = namedtuple("Case", "name group slots batches info")   # info: what the builder promises, for the CPU test


# ------------------------------------------------------------------------------------------------ issuers, certificates
def _issuer(cn, fill, serial):
    return D.cert(serial=serial, subject=D.name(D.rdn(3, cn)), spki=D.rsa_spki(n=b"\x00" + bytes([fill]) * 256), exts=[D.BC_CA])


# 0 and 1 carry one SubjectPublicKeyInfo: one canonical issuer (index 0); 2 is another issuer
ISSUERS = [_issuer(b"Reduce CA A", 0xc3, b"\x01"), _issuer(b"Reduce CA A bis", 0xc3, b"\x02"), _issuer(b"Reduce CA B", 0xc5, b"\x03")]
CANON = [0, 0, 2]
RSA = D.rsa_spki()
P256 = D.EC_SPKI
_certs = {}


def hour_of(not_after):
    t = (2000 + int(not_after[0:2]), int(not_after[2:4]), int(not_after[4:6]), int(not_after[6:8]), int(not_after[8:10]), int(not_after[10:12]))
    return calendar.timegm(t) // 3600


def entry(serial, iss=0, not_after=NOT_AFTER, spki=RSA, ca=False, reaches=True):
    """reaches: False for a certificate the builder knows not to reach the set (CA, expired, a point off the curve)."""
    k = (serial, not_after, spki, ca)
    der = _certs.get(k)
    if der is None:
        der = _certs[k] = D.cert(serial=serial, not_after=D.utctime(not_after), spki=spki, exts=[D.BC_CA if ca else D.BC_NOT_CA])
    return Entry(der, iss, (hour_of(not_after), CANON[iss], bytes(serial)) if reaches and not ca else None)


def broken(serial):
    """The certificate of `serial` with a TBSCertificate that is no SEQUENCE: a parse error, no key."""
    der = entry(serial).der
    assert der[0] == 0x30 and der[1] == 0x82 and der[4] == 0x30
    return Entry(der[:4] + b"\x31" + der[5:], 0, None)


def named(k, ln=7):
    """The k-th named serial of `ln` octets (fillers have 5, the searched serials of C and D 8)."""
    assert ln != 5 and ln != 8 and k < 1 << 16
    return (b"\x33" + k.to_bytes(2, "big") + b"\xa7" * 40)[:ln]


class Fillers:
    """Entries with a key of their own each; ec: every third one (or all, ec = "all") carries a P-256 key."""

    def __init__(self, base, ec=None):
        self.k, self.ec = base << 20, ec

    def __call__(self):
        self.k += 1
        ec = self.ec == "all" or (self.ec and self.k % 3 == 1)
        return entry(b"\x5a" + self.k.to_bytes(4, "big"), spki=P256 if ec else RSA)


def place(n, fixed, fill):
    """n entries: fixed[position] where given, fillers elsewhere."""
    assert all(0 <= p < n for p in fixed)
    return [fixed[i] if i in fixed else fill() for i in range(n)]


def thrice(batch):
    return [list(batch), list(batch), list(batch[::-1])]


def positions(batch):
    """key → ascending positions, for the keys of the batch."""
    out = {}
    for i, e in enumerate(batch):
        if e.key is not None:
            out.setdefault(e.key, []).append(i)
    return out


def capacity_ok(batches, slots):
    """ensure_capacity's bound before every batch: (distinct keys stored so far + entries of the batch) · 4 <= slots · 3."""
    seen = set()
    for b in batches:
        if (len(seen) + len(b)) * 4 > slots * 3:
            return False
        seen |= {e.key for e in b if e.key is not None}
    return True


# ------------------------------------------------------------------------------------------------ A: multiplicity, placement
MULTS = (2, 3, 4, 5, 64, 65, 256, 1025, 4097)
BLOCK_EDGES = (1023, 1024, 2047, 2048, 3071, 4096)
STRIDED = ((2, 2049), (3, 1366), (5, 819))         # (copies c, keys K): K · c = 4 098, 4 098, 4 095 ≈ 4 099


def group_a():
    out = []

    def case(name, n, fixed, info, ec=None):
        out.append(Case(name, "A", BIG_SLOTS, thrice(place(n, fixed, Fillers(1 + len(out), ec))), info))

    for m in MULTS:                                 # one key m times: a run from index 5 on, and every third index from 1 on
        e = entry(named(m))
        case("mult_%d_adjacent" % m, 5 + m + 6, {5 + r: e for r in range(m)}, {"copies": [list(range(5, 5 + m))]})
        if m <= 1025:
            case("mult_%d_strided" % m, 1 + 3 * m + 6, {1 + 3 * r: e for r in range(m)}, {"copies": [list(range(1, 1 + 3 * m, 3))]})
    for ec in (None, "all"):
        sfx, sp = ("_ec", P256) if ec else ("", RSA)
        e = entry(named(100), spki=sp)
        # the four entries 4t..4t+3 of k_insert2's thread t = 40, and one more copy two waves earlier: whichever of the five
        # claims, the thread has at least three DEFER entries
        case("thread4_same" + sfx, 200, {p: e for p in (2, 160, 161, 162, 163)}, {"copies": [[2, 160, 161, 162, 163]]}, ec)
        # four keys in one thread's four entries, each the copy of an entry of wave 0
        es = [entry(named(110 + q), spki=sp) for q in range(4)]
        fixed = {q: es[q] for q in range(4)}
        fixed.update({160 + q: es[q] for q in range(4)})
        case("thread4_distinct" + sfx, 200, fixed, {"copies": [[q, 160 + q] for q in range(4)]}, ec)
        e = entry(named(120), spki=sp)
        case("wave_same" + sfx, 200, {p: e for p in range(64, 128)}, {"copies": [list(range(64, 128))]}, ec)
        case("wave_straddle" + sfx, 230, {p: e for p in range(100, 165)}, {"copies": [list(range(100, 165))]}, ec)
        case("block_edges" + sfx, 4099, {p: e for p in BLOCK_EDGES}, {"copies": [list(BLOCK_EDGES)]}, ec)
    e = entry(named(130))
    case("same_4099", 4099, {p: e for p in range(4099)}, {"copies": [list(range(4099))]})
    a, b = entry(named(131)), entry(named(132))
    case("abab_2048", 2051, {p: (a, b)[p & 1] for p in range(2048)}, {"copies": [list(range(0, 2048, 2)), list(range(1, 2048, 2))]})
    for c, K in STRIDED:
        keys = [entry(named(1000 + k)) for k in range(K)]
        case("strided_%dx%d" % (K, c), 4099, {r * K + k: keys[k] for k in range(K) for r in range(c)},
             {"copies": [[r * K + k for r in range(c)] for k in range(K)]})
        case("adjacent_%dx%d" % (K, c), 4099, {k * c + r: keys[k] for k in range(K) for r in range(c)},
             {"copies": [[k * c + r for r in range(c)] for k in range(K)]})
    return out


# ------------------------------------------------------------------------------------------------ B: known and new mixed
def group_b(n_s=500, n_t=500):
    """Batch 1 inserts S; batch 2 interleaves 0..3 copies of every key of S ∪ T (seeded shuffle): only the first copies of
    T are unknown."""
    rng = random.Random(SEED + 2)
    S = [entry(named(3000 + k)) for k in range(n_s)]
    T = [entry(named(4000 + k)) for k in range(n_t)]
    b1 = list(S)
    rng.shuffle(b1)
    b2 = [e for k, e in enumerate(S + T) for _ in range((k + k // 4) % 4)]
    rng.shuffle(b2)
    info = {"S": {e.key for e in S}, "T": {e.key for e in T}}
    return [Case("known_and_new", "B", BIG_SLOTS, [b1, b2], info)]


# ------------------------------------------------------------------------------------------------ C, D: the search
SEARCH = 1 << 23
Found = namedtuple("Found", "pairs triples adjacent wrap_pairs n_pairs n_triples n_adjacent by_home")
_found = []


def home_of(serial, slots=SLOTS):
    return XC.serial_hash(serial) & (slots - 1)


def tag_of(serial):
    return XC.key_tag(XC.serial_hash(serial))


def search():
    """8-octet serials (issuer 0, the port's expiry hour) grouped by (24-bit tag, home slot of a 64-slot index) with the numpy
    port under a fixed seed: pairs and triples that share both, pairs with one tag and adjacent home slots, pairs whose
    shared home slot is the last one (63), and plain serials by home slot (fillers, the wrap runs)."""
    if _found:
        return _found[0]
    s = XC.np_serials8(SEED, SEARCH)
    h = XC.np_key_hash8(s)
    sig = (XC.np_key_tag(h) << U(8)) | (h & U(SLOTS - 1))
    order = np.argsort(sig, kind="stable")
    ss = sig[order]
    change = np.flatnonzero(np.concatenate(([True], ss[1:] != ss[:-1], [True])))
    starts, lens = change[:-1], np.diff(change)
    ser = lambda k: XC.s8(s[order[k]])
    p_at, t_at = starts[lens == 2], starts[lens >= 3]
    pairs = [(ser(k), ser(k + 1)) for k in p_at[:16]]
    triples = [(ser(k), ser(k + 1), ser(k + 2)) for k in t_at[:4]]
    last = p_at[(ss[p_at] & U(0xff)) == U(SLOTS - 1)]
    wrap_pairs = [(ser(k), ser(k + 1)) for k in last[:4]]
    rep = ss[starts]
    adj = np.flatnonzero((rep[1:] == rep[:-1] + U(1)) & ((rep[:-1] & U(0xff)) != U(SLOTS - 1)) & (lens[1:] == 1) & (lens[:-1] == 1))
    adjacent = [(ser(starts[k]), ser(starts[k + 1])) for k in adj[:4]]
    by_home = {}
    for k in range(4096):                           # singletons of the sorted order's far end: no constructed key among them
        x = XC.s8(s[k])
        by_home.setdefault(int(h[k]) & (SLOTS - 1), []).append(x)
    _found.append(Found(pairs, triples, adjacent, wrap_pairs, len(p_at), len(t_at), len(adj), by_home))
    return _found[0]


def far_fillers(home, count, taken):
    """`count` searched serials whose home slots lie 16, 21, 26, … slots behind `home`: out of reach of the runs that form
    there; none handed out twice (taken)."""
    f, out = search(), []
    for k in range(count):
        lst = f.by_home[(home + 16 + 5 * k) % SLOTS]
        x = next(x for x in lst if x not in taken)
        taken.add(x)
        out.append(entry(x))
    return out


def group_c():
    f = search()
    out, taken = [], set()
    for p in f.pairs + f.wrap_pairs:
        taken.update(p)
    for t in f.triples:
        taken.update(t)
    for p in f.adjacent:
        taken.update(p)

    def case(name, batches, info):
        assert capacity_ok(batches, SLOTS), name
        out.append(Case(name, "C", SLOTS, batches, info))

    def seq(name, pattern, keys):
        """One batch: the sequence (letters → keys) with far fillers in between, then again, then reversed."""
        home = home_of(keys["A"])
        fl = far_fillers(home, 4, taken)
        b = []
        for j, ch in enumerate(pattern):
            b.append(entry(keys[ch]))
            if j < len(fl):
                b.append(fl[j])
        case(name, thrice(b), {"same_slot": [tuple(keys[ch] for ch in sorted(set(pattern)))]})

    for k, pattern in enumerate(("abab", "baab", "a3_b_between")):
        a, b = f.pairs[k]
        seq(pattern, {"abab": "ABAB", "baab": "BAAB", "a3_b_between": "ABABA"}[pattern], {"A": a, "B": b})
    a, b, c = f.triples[0]
    seq("abccba", "ABCCBA", {"A": a, "B": b, "C": c})
    a, b, c = f.triples[1]
    fl = far_fillers(home_of(a), 4, taken)
    b1 = [entry(a), fl[0], entry(b), fl[1]]
    b2 = [entry(a), fl[2], entry(b), entry(c), fl[3]]
    case("two_batches", [b1, b2, b2[::-1]], {"same_slot": [(a, b, c)]})
    # known since an earlier batch and, under the same tag, new in this batch
    a, b = f.pairs[3]
    fl = far_fillers(home_of(a), 2, taken)
    case("known_then_twin", [[entry(a), fl[0]], [entry(b), entry(a), fl[1], entry(b)], [entry(b), entry(a)]], {"same_slot": [(a, b)]})
    for k, (p, q) in enumerate(f.adjacent[:2]):     # one tag, home slots j and j + 1
        for name, first, second in (("pq", p, q), ("qp", q, p)):
            fl = far_fillers(home_of(p), 2, taken)
            b = [entry(first), fl[0], entry(second), entry(first), fl[1], entry(second)]
            if k == 0:
                case("adjacent_" + name, thrice(b), {"adjacent": [(p, q)]})
            else:                                   # a key of another tag holds slot j since batch 1: P moves on to Q's home
                blocker = next(x for x in f.by_home[home_of(p)] if x not in taken)
                taken.add(blocker)
                case("adjacent_%s_behind_filler" % name, [[entry(blocker)], b, b, b[::-1]], {"adjacent": [(p, q)], "blocker": blocker})
    return out


def group_d():
    """Runs that continue from slot 63 through slot 0."""
    f = search()
    out = []
    run = [f.by_home[hm][k] for k in range(2) for hm in (61, 62, 63)]      # homes 61 62 63 61 62 63: slots 61 … 2
    ents = [entry(x) for x in run]
    info = {"homes": [home_of(x) for x in run]}
    out.append(Case("wrap_one_batch", "D", SLOTS, thrice(ents + ents), info))
    out.append(Case("wrap_two_batches", "D", SLOTS, [ents, ents[::-1], ents + ents], info))
    a, b = f.wrap_pairs[0]                          # one tag, home slot 63 both: the second lives in slot 0
    fl = [entry(f.by_home[hm][2]) for hm in (20, 30)]
    bt = [entry(a), fl[0], entry(b), entry(a), fl[1], entry(b)]
    out.append(Case("wrap_tag_pair", "D", SLOTS, thrice(bt), {"homes": [63, 63], "same_slot": [(a, b)]}))
    a, b = f.wrap_pairs[1]
    out.append(Case("wrap_tag_pair_two_batches", "D", SLOTS, [[entry(a)], [entry(b), entry(a), entry(b)], [entry(b), entry(a)]],
                    {"homes": [63, 63], "same_slot": [(a, b)]}))
    for c in out:
        assert capacity_ok(c.batches, SLOTS), c.name
    return out


# ------------------------------------------------------------------------------------------------ E: the same key, or not
DUP_LENGTHS = (1, 8, 20, 21, 24, 39, 40, 41)       # 41: the host-side set (ES_HOST)
TWIN_OCTETS = (20, 31, 39)


def group_e():
    out = []
    rng = random.Random(SEED + 5)

    def case(name, fixed_list, info, ec=None):
        """The listed entries at every third position from 2 on, fillers between; then again; then reversed."""
        fixed = {2 + 3 * k: e for k, e in enumerate(fixed_list)}
        out.append(Case(name, "E", BIG_SLOTS, thrice(place(2 + 3 * len(fixed_list) + 4, fixed, Fillers(64 + len(out), ec))), info))

    for ec in (None, "all"):
        sp = P256 if ec else RSA
        lst, keys = [], []
        for ln in DUP_LENGTHS:
            x = XC.rand_serial(rng, ln)
            keys.append(x)
            lst += [entry(x, spki=sp)] * 2
        case("lengths" + ("_ec" if ec else ""), lst, {"dups": keys}, ec)
    lst, twins = [], []
    for at in TWIN_OCTETS:                          # 40 octets, equal in octets 0..19, different at one octet behind
        x = XC.rand_serial(rng, 40)
        y = bytearray(x)
        y[at] ^= 0x10
        twins.append((x, bytes(y)))
        lst += [entry(x), entry(bytes(y)), entry(x)]
    for ln in (1, 8, 19, 20, 39, 40):               # X and X ‖ 00: equal zero-padded words, another length
        x = XC.rand_serial(rng, ln)
        twins.append((x, x + b"\x00"))
        lst += [entry(x), entry(x + b"\x00")]
    case("twins", lst, {"twins": twins})
    x = named(200)
    lst = [entry(x), entry(x, not_after="270101003000Z"), entry(x, not_after="270101010000Z"), entry(x, not_after="270101005959Z")]
    case("hours", lst, {"serial": x})
    x, y = named(201), named(202)
    lst = [entry(x, iss=0), entry(x, iss=1), entry(y, iss=1), entry(y, iss=2), entry(y, iss=0), entry(x, iss=2)]
    case("issuers", lst, {"serials": (x, y)})
    for ec in (None, "all"):
        sp = P256 if ec else RSA
        a, b, c = named(210), named(211), named(212)
        lst = [entry(a, spki=sp, ca=True), entry(a, spki=sp),
               entry(b, spki=sp, not_after="250601000000Z", reaches=False), entry(b, spki=sp),
               broken(c), entry(c, spki=sp)]
        case("filtered_first" + ("_ec" if ec else ""), lst, {"serials": (a, b, c)}, ec)
    return out


# ------------------------------------------------------------------------------------------------ F: one key, two public keys
F_PLACEMENTS = {"wave": (5, 41), "blocks": (200, 1024 + 30)}


def group_f():
    from tests import ec_corpus as E
    good = {"p256": E.case_spki(E.picks("P256", True, 1, skip=3)[0]), "p384": E.case_spki(E.picks("P384", True, 1, skip=3)[0])}
    bad = E.case_spki(next(c for c in E.cases("P256") if not c.ok and c.kind == "y+1"))
    out = []
    for pname, (lo, hi) in F_PLACEMENTS.items():
        fixed, pairs, k = {}, {}, 0

        def pair(name, first, second):
            nonlocal k
            fixed[lo + 2 * k], fixed[hi + 2 * k] = first, second
            pairs[name] = (lo + 2 * k, hi + 2 * k)
            k += 1

        for cv, sp in good.items():
            x = named(300 + k)
            pair("%s_then_rsa" % cv, entry(x, spki=sp), entry(x))
            x = named(300 + k)
            pair("rsa_then_%s" % cv, entry(x), entry(x, spki=sp))
        x = named(300 + k)
        pair("bad_ec_then_rsa", entry(x, spki=bad, reaches=False), entry(x))
        x = named(300 + k)
        pair("good_ec_then_bad_ec", entry(x, spki=good["p256"]), entry(x, spki=bad, reaches=False))
        x = named(300 + k)
        pair("rsa_then_bad_ec", entry(x), entry(x, spki=bad, reaches=False))
        # four keys in wave 0 and their copies in ONE k_insert2 thread (entries 4t..4t+3) behind everything else
        t0 = max(128, (hi + 2 * k + 8) & ~3)
        for q in range(4):
            x, y = named(320 + q), named(330 + q)
            fixed[60 + q], fixed[t0 + q] = entry(x), entry(x, spki=good["p256"])            # the EC copies defer, all four
            fixed[56 + q], fixed[t0 + 4 + q] = entry(y, spki=good["p256"]), entry(y)         # the RSA copies claim, the EC originals take over
        pairs["thread4_rsa_first"] = (60, t0)
        pairs["thread4_ec_first"] = (56, t0 + 4)
        n = t0 + 8 + 5
        out.append(Case("spki_pairs_" + pname, "F", BIG_SLOTS, thrice(place(n, fixed, Fillers(96 + len(out), ec=True))), {"pairs": pairs}))
    return out


# ------------------------------------------------------------------------------------------------ everything
_all = []


def cases():
    """Every case, built once (the tests share them and leave them unchanged)."""
    if not _all:
        _all.extend(group_a() + group_b() + group_c() + group_d() + group_e() + group_f())
        assert len({c.name for c in _all}) == len(_all)
    return _all


def model_verdicts(case):
    """Per batch, per entry: WasUnknown by the dict model (tests/xchg_corpus.py); → (verdicts, the model)."""
    m = XC.Model(key=lambda e: e.key)
    return [m.feed(b) for b in case.batches], m
