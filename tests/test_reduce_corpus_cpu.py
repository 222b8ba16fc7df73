"""tests/reduce_corpus.py held to what its builders name, without a GPU: positions, multiplicities, tags and home slots
by the hash port of tests/xchg_corpus.py, the capacity arithmetic of the 64-slot cases, and — entry by entry, on every
case — the dict model against the single-stream oracle, so that a disagreement on the device cannot be the corpus's own."""
from collections import Counter

import numpy as np
import pytest

from ct_mapreduce_amd.engine import Batch
from oracle import oracle as orc
from tests import reduce_corpus as R, xchg_corpus as XC
from tests.gpu_common import run_oracle


def by_name(group):
    return {c.name: c for c in R.cases() if c.group == group}


def copies_of(batch):
    """The position lists of the keys that occur more than once, sorted."""
    return sorted(p for p in R.positions(batch).values() if len(p) > 1)


def is_thrice(c):
    return len(c.batches) == 3 and c.batches[1] == c.batches[0] and c.batches[2] == c.batches[0][::-1]


# ------------------------------------------------------------------------------------------------ A
def test_group_a_places_its_copies_where_it_says():
    A = by_name("A")
    for c in A.values():
        assert is_thrice(c), c.name
        b = c.batches[0]
        assert all(e.key is not None for e in b) and len(b) <= 4099 + 11
        assert copies_of(b) == sorted(c.info["copies"]), c.name
        v, m = R.model_verdicts(c)
        first = {p[0] for p in R.positions(b).values()}
        assert [i for i, x in enumerate(v[0]) if x] == sorted(first), c.name
        assert not any(v[1]) and not any(v[2]), c.name
    got = Counter()
    for m in R.MULTS:
        (p,) = A["mult_%d_adjacent" % m].info["copies"]
        assert len(p) == m and p == list(range(p[0], p[0] + m))
        got[m] += 1
    assert set(got) == {2, 3, 4, 5, 64, 65, 256, 1025, 4097}
    for sfx in ("", "_ec"):
        (p,) = A["thread4_same" + sfx].info["copies"]
        assert len(p) == 5 and p[1] % 4 == 0 and p[1:] == [p[1] + k for k in range(4)] and p[0] // 64 != p[1] // 64
        ps = A["thread4_distinct" + sfx].info["copies"]
        t0 = ps[0][1]
        assert len(ps) == 4 and t0 % 4 == 0 and [q[1] for q in ps] == [t0 + k for k in range(4)] and all(q[0] < 64 <= t0 for q in ps)
        (p,) = A["wave_same" + sfx].info["copies"]
        assert len(p) == 64 and p[0] % 64 == 0 and p == list(range(p[0], p[0] + 64))
        (p,) = A["wave_straddle" + sfx].info["copies"]
        assert len(p) == 65 and p == list(range(p[0], p[0] + 65)) and {q // 64 for q in p} == {p[0] // 64, p[0] // 64 + 1}
        assert p[0] % 64 != 0 and (p[-1] + 1) % 64 != 0
        (p,) = A["block_edges" + sfx].info["copies"]
        assert p == [1023, 1024, 2047, 2048, 3071, 4096] and len(A["block_edges" + sfx].batches[0]) == 4099
        spki_ec = [R.P256 in e.der for e in A["wave_same" + sfx].batches[0]]
        assert all(spki_ec) if sfx else not any(spki_ec)
    c = A["same_4099"]
    assert len(c.batches[0]) == 4099 and len({e.der for e in c.batches[0]}) == 1
    assert R.model_verdicts(c)[0][0] == [True] + [False] * 4098
    a, b = A["abab_2048"].info["copies"]
    assert a == list(range(0, 2048, 2)) and b == list(range(1, 2048, 2))
    for cc, K in R.STRIDED:
        assert cc in (2, 3, 5) and 4099 - 5 < K * cc <= 4099
        s = A["strided_%dx%d" % (K, cc)].info["copies"]
        d = A["adjacent_%dx%d" % (K, cc)].info["copies"]
        assert len(s) == len(d) == K
        assert all(p == [r * K + k for r in range(cc)] for k, p in enumerate(s))
        assert all(p == [k * cc + r for r in range(cc)] for k, p in enumerate(d))
        assert len(A["strided_%dx%d" % (K, cc)].batches[0]) == 4099


# ------------------------------------------------------------------------------------------------ B
def test_group_b_mixes_known_and_new():
    (c,) = by_name("B").values()
    b1, b2 = c.batches
    S, T = c.info["S"], c.info["T"]
    assert {e.key for e in b1} == S and len(b1) == len(S) and not S & T
    pos = R.positions(b2)
    mult = lambda keys: Counter(len(pos.get(k, ())) for k in keys)
    assert set(mult(S)) == set(mult(T)) == {0, 1, 2, 3}, (mult(S), mult(T))
    v, _ = R.model_verdicts(c)
    assert all(v[0])
    assert [i for i, x in enumerate(v[1]) if x] == sorted(p[0] for k, p in pos.items() if k in T)
    assert len(b2) > 1024


# ------------------------------------------------------------------------------------------------ C, D
def test_the_search_finds_what_the_builders_need():
    f = R.search()
    print("pairs", f.n_pairs, "triples", f.n_triples, "adjacent pairs", f.n_adjacent, "pairs at slot 63", len(f.wrap_pairs))
    assert len(f.pairs) >= 4 and len(f.triples) >= 2 and len(f.adjacent) >= 2 and len(f.wrap_pairs) >= 2
    everything = [x for g in f.pairs + f.triples + f.adjacent + f.wrap_pairs for x in g]
    assert len(set(everything)) == len(everything) and all(len(x) == 8 and 1 <= x[0] < 0x7f for x in everything)
    for g in f.pairs + f.triples + f.wrap_pairs:                     # by the INTEGER port: one tag, one home slot
        assert len({R.tag_of(x) for x in g}) == 1 and len({R.home_of(x) for x in g}) == 1, g
    assert all(R.home_of(a) == R.SLOTS - 1 for a, _ in f.wrap_pairs)
    for p, q in f.adjacent:
        assert R.tag_of(p) == R.tag_of(q) and R.home_of(q) == R.home_of(p) + 1, (p, q)
    assert sorted(f.by_home) == list(range(R.SLOTS)) and all(len(v) >= 8 for v in f.by_home.values())
    assert all(R.home_of(x) == hm for hm, v in f.by_home.items() for x in v[:3])


def constructed(c):
    return [x for key in ("same_slot", "adjacent") for g in c.info.get(key, ()) for x in g]


@pytest.mark.parametrize("group", ["C", "D"])
def test_the_small_index_cases_keep_their_capacity_and_their_slots(group):
    """ensure_capacity leaves the 64-slot index alone while (occupied + incoming) · 4 <= 64 · 3: occupied = the distinct keys
    stored so far, incoming = the entries of the batch.  Recomputed here, batch by batch."""
    cs = by_name(group)
    if group == "C":
        assert set(cs) == {"abab", "baab", "a3_b_between", "abccba", "two_batches", "known_then_twin", "adjacent_pq", "adjacent_qp",
                           "adjacent_pq_behind_filler", "adjacent_qp_behind_filler"}
    for c in cs.values():
        assert c.slots == 64
        occupied = set()
        for b in c.batches:
            assert len(b) <= 48 and (len(occupied) + len(b)) * 4 <= 64 * 3, c.name
            occupied |= {e.key for e in b}
        assert R.capacity_ok(c.batches, 64) and not R.capacity_ok([c.batches[0][:1] * 49], 64)
        keys = {e.key[2] for b in c.batches for e in b}
        assert all(e.key[:2] == (XC.EXP_HOUR, 0) and e.iss == 0 for b in c.batches for e in b)      # the key the port hashed
        named = set(constructed(c))
        tags = {R.tag_of(x) for x in named}
        for x in keys - named:                                       # fillers: other tags
            assert R.tag_of(x) not in tags, (c.name, x)
        if group == "C":
            home = R.home_of(constructed(c)[0])
            for x in keys - named - {c.info.get("blocker")}:         # … and home slots out of the run's reach
                assert (R.home_of(x) - home) % 64 >= 16, (c.name, x)
            if "blocker" in c.info:
                p, q = c.info["adjacent"][0]
                assert R.home_of(c.info["blocker"]) == R.home_of(p) and R.tag_of(c.info["blocker"]) != R.tag_of(p)
                assert [e.key[2] for e in c.batches[0]] == [c.info["blocker"]]
    if group == "C":
        seqs = {n: "".join("ABC"[cs[n].info["same_slot"][0].index(e.key[2])] for e in cs[n].batches[0] if e.key[2] in constructed(cs[n]))
                for n in ("abab", "baab", "a3_b_between", "abccba")}
        assert seqs == {"abab": "ABAB", "baab": "BAAB", "a3_b_between": "ABABA", "abccba": "ABCCBA"}, seqs
        a, b, c3 = cs["two_batches"].info["same_slot"][0]
        strip = lambda batch: [e.key[2] for e in batch if e.key[2] in (a, b, c3)]
        assert [strip(x) for x in cs["two_batches"].batches[:2]] == [[a, b], [a, b, c3]]
        a, b = cs["known_then_twin"].info["same_slot"][0]
        assert [[e.key[2] for e in x if e.key[2] in (a, b)] for x in cs["known_then_twin"].batches[:2]] == [[a], [b, a, b]]
        for n in ("adjacent_pq", "adjacent_pq_behind_filler"):
            p, q = cs[n].info["adjacent"][0]
            strip = lambda batch: [e.key[2] for e in batch if e.key[2] in (p, q)]
            assert strip(cs[n].batches[-3]) == [p, q, p, q] and strip(cs[n.replace("pq", "qp")].batches[-3]) == [q, p, q, p]
    else:
        for n in ("wrap_one_batch", "wrap_two_batches"):
            assert sorted(cs[n].info["homes"]) == [61, 61, 62, 62, 63, 63]
            slots = {}
            for e in cs[n].batches[0]:                               # linear probing, in any order: the run fills 61 … 63, 0 … 2
                j = R.home_of(e.key[2])
                while j in slots and slots[j] != e.key:
                    j = (j + 1) % 64
                slots[j] = e.key
            assert sorted(slots) == [0, 1, 2, 61, 62, 63]
        assert all(len(p) == 2 for p in R.positions(cs["wrap_one_batch"].batches[0]).values())
        assert all(len(p) == 1 for b in cs["wrap_two_batches"].batches[:2] for p in R.positions(b).values())
        for n in ("wrap_tag_pair", "wrap_tag_pair_two_batches"):
            a, b = cs[n].info["same_slot"][0]
            assert R.home_of(a) == R.home_of(b) == 63 and R.tag_of(a) == R.tag_of(b)


# ------------------------------------------------------------------------------------------------ E, F
def verdict_at(c, serial_of_interest):
    """(issuer index, minute-resolution notAfter is not kept: position) → the model's verdicts of batch 0 for one serial."""
    v, _ = R.model_verdicts(c)
    return [x for e, x in zip(c.batches[0], v[0]) if e.key is not None and e.key[2] == serial_of_interest]


def test_group_e_names_what_is_the_same_key():
    E = by_name("E")
    assert set(E) == {"lengths", "lengths_ec", "twins", "hours", "issuers", "filtered_first", "filtered_first_ec"}
    assert all(is_thrice(c) for c in E.values())
    for n in ("lengths", "lengths_ec"):
        assert sorted(len(x) for x in E[n].info["dups"]) == [1, 8, 20, 21, 24, 39, 40, 41]
        assert all(verdict_at(E[n], x) == [True, False] for x in E[n].info["dups"])
    tw = E["twins"].info["twins"]
    diff = Counter()
    for x, y in tw:
        assert x != y and verdict_at(E["twins"], x)[0] and verdict_at(E["twins"], y)[0]
        if len(x) == len(y) == 40:
            assert x[:20] == y[:20]
            diff[next(k for k in range(40) if x[k] != y[k])] += 1
        else:
            assert y == x + b"\x00" and XC.serial_words(x) == XC.serial_words(y[:40])
            diff[("zero", len(x))] += 1
    assert set(diff) == {20, 31, 39, ("zero", 1), ("zero", 8), ("zero", 19), ("zero", 20), ("zero", 39), ("zero", 40)}
    h = [e for e in E["hours"].batches[0] if e.key[2] == E["hours"].info["serial"]]
    assert [e.key[0] - XC.EXP_HOUR for e in h] == [0, 0, 1, 0] and len({e.der for e in h}) == 4
    assert verdict_at(E["hours"], E["hours"].info["serial"]) == [True, False, True, False]
    x, y = E["issuers"].info["serials"]
    who = lambda s: [(e.iss, e.key[1]) for e in E["issuers"].batches[0] if e.key[2] == s]
    assert who(x) == [(0, 0), (1, 0), (2, 2)] and verdict_at(E["issuers"], x) == [True, False, True]
    assert who(y) == [(1, 0), (2, 2), (0, 0)] and verdict_at(E["issuers"], y) == [True, True, False]
    for n in ("filtered_first", "filtered_first_ec"):
        b = [e for e in E[n].batches[0] if e.key is None or e.key[2] in E[n].info["serials"]]
        assert [e.key is None for e in b] == [True, False] * 3
        v, _ = R.model_verdicts(E[n])
        assert [x for e, x in zip(E[n].batches[0], v[0]) if e in b] == [False, True] * 3


def test_group_f_pairs_one_key_with_two_public_keys():
    F = by_name("F")
    assert set(F) == {"spki_pairs_wave", "spki_pairs_blocks"}
    want = {"p256_then_rsa": (True, True, False), "rsa_then_p256": (True, True, False), "p384_then_rsa": (True, True, False),
            "rsa_then_p384": (True, True, False), "bad_ec_then_rsa": (False, False, True), "good_ec_then_bad_ec": (True, True, False),
            "rsa_then_bad_ec": (True, True, False)}      # (same key?, first unknown, second unknown)
    for c in F.values():
        assert is_thrice(c)
        b = c.batches[0]
        v, _ = R.model_verdicts(c)
        pairs = c.info["pairs"]
        for name, (same, u1, u2) in want.items():
            i, j = pairs[name]
            assert b[i].der != b[j].der and (v[0][i], v[0][j]) == (u1, u2), name
            assert (i // 64 == j // 64) if c.name.endswith("wave") else (i // 1024 != j // 1024), name
            if b[i].key is not None and b[j].key is not None:
                assert b[i].key == b[j].key
            ec = [R.RSA not in e.der for e in (b[i], b[j])]
            assert ec == [not name.startswith("rsa"), not name.endswith("rsa")], name
        for name, ec_first in (("thread4_rsa_first", False), ("thread4_ec_first", True)):
            i, j = pairs[name]
            assert j % 4 == 0 and i < 64 <= j
            for q in range(4):
                assert b[i + q].key == b[j + q].key and b[i + q].der != b[j + q].der
                assert (R.RSA not in b[i + q].der) == ec_first and (R.RSA in b[j + q].der) == ec_first
        assert any(R.P256 in e.der for e in b[:4] + b[-4:]) and any(R.RSA in e.der for e in b[:4] + b[-4:])     # fillers of both kinds


# ------------------------------------------------------------------------------------------------ the model is the oracle
def oracle_batches(case):
    o, out = None, []
    for b in case.batches:
        batch = Batch.from_certs([e.der for e in b], [e.iss for e in b])
        batch.payload = np.concatenate([batch.payload, np.zeros(64, np.uint8)])
        o, st, unk, _ = run_oracle(batch, R.ISSUERS, b"", False, R.NOW, engine=o)
        out.append((st, unk))
    return o, out


def test_the_model_equals_the_oracle_on_every_case():
    n = 0
    for c in R.cases():
        o, got = oracle_batches(c)
        want, m = R.model_verdicts(c)
        for k, (b, (st, unk)) in enumerate(zip(c.batches, got)):
            assert [s == orc.ST_PASS for s in st] == [e.key is not None for e in b], (c.name, k)
            assert [bool(u) for u in unk] == want[k], (c.name, k)
            n += len(b)
        assert o.total_count() == len(m.seen), c.name
    print("cases:", len(R.cases()), "entries compared:", n)
    assert {c.group for c in R.cases()} == set("ABCDEF")
