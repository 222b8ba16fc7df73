"""tests/ec_corpus.py against itself, the host build and the oracle.  CPU only.

The corpus is Python integers; this file (1) keeps it from degenerating quietly — floors per curve on what it must
contain, (2) holds the host build of k_ec_resolve's loader + ec_equation (harness.product_ec_point_bits) to the integer
verdict on EVERY case, byte-aligned and at a pad count of 3, and (3) holds the oracle and the product walk
(test_spki_cpu.verdict: both, key parse on and off) to it with the case wrapped in a certificate.  What passes here is what
tests/test_gpu_ec_corpus.py then asks of the device."""
import random

import numpy as np
import pytest

from ct_mapreduce_amd import synth
from ct_mapreduce_amd.engine import Batch, RawEntries
from oracle import oracle as orc
from tests import ec_corpus as E
from tests import harness
from tests.gpu_common import run_oracle
from tests.test_spki_cpu import CURVES, NF_SPKI, PRIMES, verdict

NOW = synth.BASE_TIME


@pytest.mark.parametrize("curve", list(CURVES))
def test_the_corpus_holds_what_it_promises(curve):
    cs = E.cases(curve)
    p = PRIMES[curve]
    acc = [c for c in cs if c.ok]
    ref = [c for c in cs if not c.ok]
    near_p = sum(c.x > p - 64 for c in acc)
    near_0 = sum(c.x < 64 for c in acc)
    unreduced = [c for c in ref if c.kind in ("x+mp", "y+mp")]
    print("%s: %d x values, %d accepted, %d refused; accepted with x > p - 64: %d, with x < 64: %d; x + m·p / y + m·p: %d"
          % (curve, len(E.x_values(curve)), len(acc), len(ref), near_p, near_0, len(unreduced)))
    assert len(acc) >= 400 and len(ref) >= 800
    assert near_p >= 20 and near_0 >= 20
    assert any(c.kind == "x+mp" for c in ref)
    if curve == "P521":
        assert sum(c.kind == "x+mp" and c.m == 127 for c in ref) >= 100
        assert sum(c.kind == "y+mp" and c.m == 127 for c in ref) >= 100
        assert {c.m for c in unreduced} == {1, 2, 64, 127}
    # every kind of case is there, the verdict is the integers', an unreduced coordinate is congruent to a point ON the curve
    assert {c.kind for c in cs} - {"top_bit"} == {"root", "y+1", "flip_y", "flip_x", "x+mp", "y+mp", "noroot", "edge"}
    # y ≥ p: on P-521 every y + m·p fits; on the other curves one y in 2^32 and more does — the corpus looks for such points
    assert sum(c.kind == "y+mp" and c.x < p <= c.y for c in ref) >= 8
    for c in cs:
        assert c.ok == E.on_curve(curve, c.x, c.y)
        if c.kind in ("x+mp", "y+mp"):
            assert not c.ok and c.m >= 1 and E.on_curve(curve, c.x % p, c.y % p) and max(c.x, c.y) >= p
        if c.kind == "root":
            assert c.ok
    # a limb boundary on either side at every limb, accepted
    for j in range(1, E.n_limbs(curve)):
        assert any(abs(c.x - (1 << 32 * j)) <= 8 for c in acc), j
        assert any(0 <= p - (1 << 32 * j) - c.x <= 7 for c in acc), j
    assert len({(c.x, c.y, c.kind) for c in cs}) >= len(cs) - 2           # (y = 0 is its own negative: at most a pair)
    assert E.cases(curve) is cs                                           # one corpus, shared


def test_p256_points_whose_squaring_carries_into_bit_32_of_the_ninth_limb():
    """ADVICE r05 as cases: with these coordinates a row of the P-256 product hands p256_redc_step a `top` of 2^32 — and
    with no other coordinate of the corpus, nor with any x = p − k the sweep of tests/test_spki_cpu.py takes."""
    p = PRIMES["P256"]
    for a in E.P256_CARRY33:
        assert a < p and max(E.p256_row_tops(a, a)) == 1 << 32
    cs = [c for c in E.cases("P256") if c.src == "carry33"]
    assert sum(c.ok for c in cs) == 16 and sum(not c.ok for c in cs) == 16
    assert {c.x for c in cs if c.ok} >= set(E.P256_CARRY33) - {E.P256_CARRY33[1]}         # x·x carries
    assert {c.y for c in cs if c.ok} >= set(E.P256_CARRY33) - {E.P256_CARRY33[0]}         # y·y carries
    for c in E.cases("P256"):
        if c.src != "carry33" and c.x < p and c.y < p:
            assert max(E.p256_row_tops(c.x, c.x) + E.p256_row_tops(c.y, c.y)) < 1 << 32
    assert all(max(E.p256_row_tops(p - k, p - k)) < 1 << 32 for k in range(1, 4000, 7))
    # (the host build's verdict on them: test_the_host_build_agrees_with_the_integers_on_every_case)


def test_p521_cases_with_a_bit_above_the_521st():
    cs = [c for c in E.cases("P521") if c.kind == "top_bit"]
    assert len(cs) == 8 * 7 * 2 and not any(c.ok for c in cs)
    for c in cs:          # masked to 521 bits the point is ON the curve: a loader that masks instead of checking accepts it
        assert E.on_curve("P521", c.x & (1 << 521) - 1, c.y & (1 << 521) - 1) and max(c.x, c.y) >> 521


def test_the_square_root_on_p224_is_tonelli_shanks_and_right():
    p = PRIMES["P224"]
    assert p % 4 == 1
    rng = random.Random(7)
    roots = 0
    for _ in range(200):
        a = rng.randrange(p)
        r = E.sqrt_mod(a, p)
        if r is None:
            assert pow(a, (p - 1) // 2, p) == p - 1
        else:
            assert r * r % p == a
            roots += 1
    assert 60 < roots < 140


@pytest.mark.parametrize("curve", list(CURVES))
def test_the_host_build_agrees_with_the_integers_on_every_case(curve):
    """k_ec_resolve's loader and equation, host build: X at a byte-aligned bit position, and the same point behind a BIT
    STRING with three pad bits (X starts three bits before an octet boundary; the bits around the point are other octets')."""
    cid = E.CURVE_ID[curve]
    rng = random.Random("host " + curve)
    bl = E.byte_len(curve)
    for k, c in enumerate(E.cases(curve)):
        pt = E.xy(c)
        pre = bytes(rng.randrange(256) for _ in range(5 + k % 4))
        buf = pre + pt + bytes(rng.randrange(256) for _ in range(8))
        assert harness.product_ec_point_bits(buf, 8 * len(pre), cid) == c.ok, c
        v = int.from_bytes(pt, "big") << 3
        body = v.to_bytes(2 * bl + 1, "big")
        buf = pre[:-1] + bytes([pre[-1] & 0xf8 | body[0]]) + body[1:-1] + bytes([body[-1] | rng.randrange(8)]) + pre
        assert harness.product_ec_point_bits(buf, 8 * len(pre) - 3, cid) == c.ok, c


@pytest.mark.parametrize("curve", list(CURVES))
def test_the_oracle_and_the_product_walk_agree_with_the_integers(curve):
    """Every case (the whole corpus takes a few seconds: no sampling), wrapped in a certificate: the oracle, the product
    walk — in-walk fe_load + ec_on_curve, host build — and both with the key parse off."""
    want_ok = (True, NF_SPKI if curve == "P192" else 0)
    n_ok = n_bad = 0
    for c in E.cases(curve):
        got = verdict(E.case_cert(c))
        assert got == (want_ok if c.ok else (False, None)), c
        n_ok += c.ok
        n_bad += not c.ok
    assert n_ok >= 400 and n_bad >= 800


def test_placement_cases_cover_every_pad_count_and_phase_and_match_the_oracle():
    pl = E.placement_cases()
    assert len(pl) == 5 * 6 * 8 * 4
    at = 0
    seen = set()
    for q in pl:
        assert (at + q.keypos) % 4 == q.phase
        at += len(q.der)
        seen.add((q.curve, q.pad, q.phase, q.ok))
        assert q.ok == E.unmarshal_ok(q.curve, q.der[q.keypos:q.keypos + 1 + 2 * E.byte_len(q.curve)], q.pad)
        assert verdict(q.der) == ((True, NF_SPKI if q.curve == "P192" else 0) if q.ok else (False, None)), q[:4]
    for curve in CURVES:
        for phase in range(4):
            for pad in range(8):
                assert (curve, pad, phase, False) in seen
                assert ((curve, pad, phase, True) in seen) == (pad < 6)       # 04 << 6 does not fit into the first octet
    assert len({q.der for q in pl}) == len(pl)
    # a second payload that starts elsewhere: the serial lengths follow
    assert [q.phase for q in E.placement_cases(start=3)] == [q.phase for q in pl]


def test_the_cases_closest_to_the_edges():
    for curve in CURVES:
        good, bad = E.closest_to_the_edges(curve)
        assert all(c.ok for c in good) and not any(c.ok for c in bad)
        assert max(E.edge_distance(c) for c in good) <= 16
        assert {c.kind for c in bad} >= {"y+1", "flip_y", "flip_x", "x+mp", "noroot", "edge"}
        assert len(set(good)) == 24 and len(set(bad)) == 24


# ------------------------------------------------------------------ the batches of tests/test_gpu_ec_corpus.py, oracle side
def oracle_map_twice(ent, issuers=None, iss=None):
    """What tests/test_gpu_ec_corpus.py expects of a batch independently of the oracle, asked of the oracle here: an X509
    entry is PARSE_ERROR exactly when the integer verdict on its key is False, the table then holds ent.stored
    certificates, and a second pass finds all of them known."""
    issuers = issuers or [E.RSA_ISSUER]
    batch = Batch.from_certs(ent.certs, iss or [0] * len(ent.certs), ent.ets)
    batch.payload = np.concatenate([batch.payload, np.zeros(64, np.uint8)])
    o, st, unk, _ = run_oracle(batch, issuers, b"", True, NOW)
    x509 = np.asarray(ent.ets) == 0
    bad = np.array([v is False for v in ent.ok])
    assert ((st == orc.ST_PARSE_ERROR)[x509] == bad[x509]).all()
    assert (st[x509 & ~bad] == orc.ST_PASS).all()
    assert o.total_count() == ent.stored == int(unk.sum())
    o, st2, unk2, _ = run_oracle(batch, issuers, b"", True, NOW, engine=o)
    assert (st2 == st).all() and not unk2.any() and o.total_count() == ent.stored
    return st


def test_the_leaf_batch_is_what_the_integers_say_in_the_oracle():
    ent, cs = E.leaf_entries()
    print("leaf batch: %d certificates, %d bytes, %d stored" % (len(cs), sum(map(len, ent.certs)), ent.stored))
    assert 8000 <= len(cs) < 65536 and len(set(ent.certs)) == len(cs)
    st = oracle_map_twice(ent)
    # both resolve kernels find their own in every 1 024-entry block
    for lo in range(0, len(cs) - 1023, 1024):
        curves = [c.curve for c in cs[lo:lo + 1024]]
        assert curves.count("P256") >= 100 and len(set(curves)) == 5
    for curve in CURVES:
        sel = np.array([c.curve == curve for c in cs])
        assert int((st[sel] == orc.ST_PASS).sum()) >= 200 and int((st[sel] == orc.ST_PARSE_ERROR).sum()) >= 800


@pytest.mark.parametrize("first_block", ["p256_and_p384", "p384_only"])
def test_the_block_batch_is_what_the_integers_say_in_the_oracle(first_block):
    ent = E.block_entries(first_block)
    assert len(ent.certs) == 2051 and ent.ok[2048:] == [None, None, False]
    assert all(v is not None for v in ent.ok[:1024]) and sum(v is not None for v in ent.ok[1024:2048]) == 257
    p256 = bytes.fromhex(CURVES["P256"][0])
    n256 = sum(p256 in c for c in ent.certs[:1024])
    assert n256 == (512 if first_block == "p256_and_p384" else 0)
    assert not any(p256 in c for c in ent.certs[1024:2048])
    for lo, hi in ((0, 1024), (1024, 2048)):                  # on and off the curve in both blocks, duplicates of accepted keys
        assert sum(v is True for v in ent.ok[lo:hi]) >= 100 and sum(v is False for v in ent.ok[lo:hi]) >= 100
        dup = [c for c, v in zip(ent.certs[lo:hi], ent.ok[lo:hi]) if v and ent.certs[lo:hi].count(c) == 2]
        assert len(dup) >= 8
    oracle_map_twice(ent)


def test_the_placement_batch_is_what_the_integers_say_in_the_oracle():
    pl = E.placement_cases()
    ets = [k & 1 for k in range(len(pl))]
    stored = sum(1 for k, q in enumerate(pl) if q.ok and not (ets[k] == 1 and q.curve == "P192"))
    oracle_map_twice(E.Entries([q.der for q in pl], ets, [q.ok for q in pl], stored))


def test_the_issuer_and_raw_entry_batches_are_what_the_integers_say_in_the_oracle():
    issuers, ent, cs = E.issuer_entries()
    assert len(cs) == 5 * 48 + 32 and len(set(issuers)) == len(cs)
    batch = Batch.from_certs(ent.certs, list(range(len(cs))), ent.ets)
    o, st, unk, _ = run_oracle(batch, issuers, b"", True, NOW)
    for k, c in enumerate(cs):
        assert st[k] == (orc.ST_PASS if c.ok and c.curve != "P192" else orc.ST_ISSUER_PARSE_ERROR), c
    assert o.total_count() == sum(c.ok and c.curve != "P192" for c in cs)
    pairs, cs2 = E.raw_precert_pairs()
    assert cs2 == cs
    raw = RawEntries.from_pairs(pairs)
    o = orc.Engine(b"", True, NOW)
    o.set_strict_leaf(True)
    st, unk, _, _ = o.raw_batch(raw.blob, raw.bounds)
    for k, c in enumerate(cs):
        assert st[k] == E.raw_precert_status(c), c
    off = orc.Engine(b"", True, NOW)                          # without strict_leaf the leaf's TBSCertificate is not walked
    off.set_strict_leaf(False)
    assert not (off.raw_batch(raw.blob, raw.bounds)[0] == orc.ST_ENTRY_DECODE_ERROR).any()
