"""tests/chain0_corpus.py held to its coverage, and its reference model to the oracle.  No GPU.

The corpus is only worth what it reaches: certificate lengths at every residue mod 16 and on both sides of the 1 KiB, 2 KiB
and 3 KiB steps of match_wave's comparison, twins that differ at every mandatory octet with the hash saying what the builder
claims, table certificates at the home slots they claim, batches that put every lane class at every lane.  The model (a dict
from Chain[0] bytes to index) must agree with the ORACLE's raw_batch on which entries reach an issuer; the GPU tests
(tests/test_gpu_chain0_corpus.py) then hold the product to both."""
import hashlib

import numpy as np
import pytest

from ct_mapreduce_amd.engine import RawEntries
from oracle import oracle as orc
from tests import chain0_corpus as K

NOW = 1_700_000_000


def test_the_hash_ports_are_the_products_hash():
    """quick_hash (Python integers, every length) and quick_hash_tails (numpy, the search) against the host build."""
    rng = K._rng("hash")
    for n in list(range(1, 70)) + [838, 1024, 5003]:
        c = rng.randbytes(n)
        assert K.quick_hash(c) == K.harness_quick_hash(c), n
    c = K.ca_cert(600, "hash")
    tails = np.random.default_rng(1).integers(0, 1 << 32, (64, 4), dtype=np.uint64)
    h = K.quick_hash_tails(len(c), c[:16], tails)
    for k in range(64):
        assert int(h[k]) == K.harness_quick_hash(c[:-16] + tails[k].astype("<u4").tobytes()), k


def test_the_builder_is_deterministic():
    a = K.lengths.__wrapped__()
    assert a.pairs == K.lengths().pairs and a.chain0 == K.lengths().chain0
    assert K.twins.__wrapped__().info["shuffled"] == K.twins().info["shuffled"]


def test_lengths_cover_every_residue_and_both_sides_of_each_step():
    fam = K.lengths()
    certs = fam.info["by_length"]
    assert all(len(c) == n for n, c in certs.items()) and len(set(certs.values())) == len(certs) == len(fam.chain0)
    run = [n for n in certs if n < 1000]
    assert len(run) >= 80 and run == list(range(run[0], run[0] + len(run)))
    assert {n % 16 for n in certs} == set(range(16))
    for lo, hi in ((1008, 1041), (2032, 2065), (3056, 3089)):
        assert set(range(lo, hi + 1)) <= set(certs)
    for step in (1024, 2048, 3072):
        assert {step - 1, step, step + 1} <= set(certs)
    assert max(certs) >= 5000
    # each: three entries at least — behind it 0xff of a second chain element, the next entry's leaf, a precertificate entry
    c0 = K.chain0_of(fam.pairs)
    at = 0
    behind = {}
    blob = b"".join(l + e for l, e in fam.pairs)
    view = K.expected_view(fam.pairs)
    for i, c in enumerate(c0):
        end = int(view["chain0_start"][i]) + len(c)
        assert blob[end - len(c):end] == c
        behind.setdefault(c, []).append(blob[end:end + 16])
    for c, b in behind.items():
        assert len(b) >= 3 and any(x[3:] == b"\xff" * 13 for x in b), len(c)   # (its three length octets, then 0xff)
        assert any(x[:2] == b"\xff\x00" for x in b), len(c)                   # the next leaf: version 0xff, leaf_type 0
    # … and as the last thing in a blob: every residue mod 16, both sides of every step
    last = [batch[-1] for batch in fam.info["last"]]
    ends = []
    for batch in fam.info["last"]:
        c = K.chain0_of(batch)[-1]
        assert (batch[-1][0] + batch[-1][1]).endswith(c) and c in certs.values()
        ends.append(len(c))
    assert {n % 16 for n in ends} == set(range(16)) and len(last) == len(K.LAST_IN_BLOB)
    for step in (1024, 2048, 3072):
        assert any(n < step for n in ends) and {step - 1, step, step + 1} & set(ends) and any(n > step for n in ends)


def test_short_covers_every_length_below_48_and_says_which_pairs_share_a_hash():
    fam = K.short()
    assert {len(c) for c in fam.chain0} == set(range(1, 48))
    assert len(set(fam.chain0)) == len(fam.chain0)
    for n in (31, 32, 33):
        same_len = [c for c in fam.chain0 if len(c) == n]
        assert any(sum(x != y for x, y in zip(a, b)) == 1 for a in same_len for b in same_len)
    assert set(fam.info["same_hash"]) == set(range(32, 48))
    for a, b in fam.info["pairs16"]:
        assert [k for k in range(len(a)) if a[k] != b[k]] == [16]
        same = K.harness_quick_hash(a) == K.harness_quick_hash(b)
        assert same == fam.info["same_hash"][len(a)] == (len(a) >= 33), len(a)
    for c in fam.chain0:
        assert not orc.parse_cert(c).ok


def test_twins_are_at_every_mandatory_position_and_hash_as_claimed():
    fam = K.twins()
    bases, tw = fam.info["bases"], fam.info["twins"]
    assert [len(b) for b in bases] == list(K.TWIN_BASES) and 2100 <= len(bases[0]) <= 2160 and 3150 <= len(bases[1]) <= 3250
    everything = bases + [c for *_, c in tw]
    assert len(set(everything)) == len(everything) == len(fam.chain0)          # pairwise distinct
    for bi, base in enumerate(bases):
        n = len(base)
        h = K.harness_quick_hash(base)
        mine = [(p, b, c) for i, p, b, c in tw if i == bi]
        pos = [p for p, _, _ in mine]
        assert len(set(pos)) == len(pos)
        want = set(range(64)) | set(range(n - 64, n)) | {p for p in range(n) if p % 16 in (0, 15)}
        want |= set(range(1008, 1041)) | set(range(2032, 2065)) | (set(range(3056, 3089)) if n > 3100 else set())
        assert want <= set(pos) and want == set(K.twin_positions(n)[0])
        rest = set(pos) - want
        # the stride: every residue mod 16 and every lane that is not mandatory throughout anyway (lanes 0 and 63: the
        # chunks on both sides of each KiB step)
        assert {p % 16 for p in rest} == set(range(1, 15)) and {(p // 16) % 64 for p in rest} >= set(range(1, 63))
        assert {p % 16 for p in pos} == set(range(16)) and {(p // 16) % 64 for p in pos} == set(range(64))
        assert any(p >= 1024 for p in rest) and (n < 3100 or (any(2048 <= p < 3072 for p in rest) and any(p >= 3072 for p in rest)))
        assert {b for _, b, _ in mine} == set(range(8))
        for p, b, c in mine:
            assert len(c) == n and [k for k in range(n) if c[k] != base[k]] == [p] and c[p] ^ base[p] == 1 << b
            assert (K.harness_quick_hash(c) == h) == (16 <= p < n - 16), p
            assert K.quick_hash(c) == K.harness_quick_hash(c)
    # carriers: two per twin, at different log indices AND lanes; the base before, between and after
    c0 = K.chain0_of(fam.pairs)
    where = {}
    for i, c in enumerate(c0):
        where.setdefault(c, []).append(i)
    for *_, c in tw:
        i, j = where[c]
        assert i != j and i % 64 != j % 64
    for bi, base in enumerate(bases):
        idx = where[base]
        carriers = [i for k, (b, *_r) in enumerate(tw) if b == bi for i in where[tw[k][3]]]
        assert idx[0] < min(carriers) and idx[-1] > max(carriers) and any(min(carriers) < i < max(carriers) for i in idx)
    assert sorted(fam.info["shuffled"]) == list(range(len(fam.pairs))) and fam.info["shuffled"] != list(range(len(fam.pairs)))
    # which twins are another issuer: those whose octet lies in the SubjectPublicKeyInfo
    assert fam.info["in_spki"]
    for k, (bi, p, b, c) in enumerate(tw):
        pc, pb = orc.parse_cert(c), orc.parse_cert(bases[bi])
        if pc.ok:
            same_spki = c[pc.spki_off:pc.spki_off + pc.spki_len] == bases[bi][pb.spki_off:pb.spki_off + pb.spki_len]
            assert same_spki == (k not in fam.info["in_spki"]) or pc.spki_off != pb.spki_off, (bi, p)


def test_edges_differ_in_the_last_octet_outside_the_hash_at_every_residue_in_every_row():
    fam = K.edges()
    rows = {}
    for base, hi, lo in fam.info["triples"]:
        n = len(base)
        assert len(hi) == len(lo) == n and len({base, hi, lo}) == 3
        assert [k for k in range(n) if hi[k] != base[k]] == [n - 17] and [k for k in range(n) if lo[k] != base[k]] == [16]
        assert K.harness_quick_hash(base) == K.harness_quick_hash(hi) == K.harness_quick_hash(lo)
        for c in (base, hi, lo):
            assert orc.parse_cert(c).ok
        rows.setdefault(min((n - 17) // 1024, 3), set()).add(n % 16)
    assert rows == {r: set(range(16)) for r in range(4)}          # first row, second row, first and second turn of the loop
    assert len(fam.chain0) == 3 * len(K.EDGE_LENGTHS)
    where = {}
    for i, c in enumerate(K.chain0_of(fam.pairs)):
        where.setdefault(c, []).append(i)
    assert all(len(v) == 3 and len({i % 64 for i in v}) == 3 for v in where.values())


def test_table_certificates_have_the_home_slots_they_claim():
    fam = K.table()
    reg, homes = fam.info["register"], fam.info["homes"]
    n = len(K.TABLE_HOMES)
    assert n >= 6 and len(set(reg)) == len(reg) <= K.TABLE_MAX_ISSUERS
    for c, home in zip(reg, homes):
        assert K.harness_quick_hash(c) & (K.TABLE_SLOTS - 1) == home
    assert tuple(homes[:n]) == K.TABLE_HOMES and set(K.TABLE_HOMES) == {1021, 1022, 1023}
    # registered in this order, linear probing puts them at 1021, 1022, 1023, 0, 1, … : the run wraps
    slots, used = [], set()
    for home in homes:
        j = home
        while j in used:
            j = (j + 1) % K.TABLE_SLOTS
        used.add(j)
        slots.append(j)
    assert slots[:n] == [1021, 1022, 1023, 0, 1, 2, 3]
    assert slots[n] == 4 and homes[n] == 1021                                 # the registered twin: the whole run in front of it
    a, b = fam.info["cross"]
    ha, hb = K.harness_quick_hash(a), K.harness_quick_hash(b)
    assert len(a) != len(b) and ha != hb and ha >> 32 == hb >> 32 and ha & 1023 == hb & 1023
    assert [ha, hb] == fam.info["hashes"]
    s = fam.info["stranger"]
    assert s not in reg and len(s) == len(reg[0]) and K.harness_quick_hash(s) == K.harness_quick_hash(reg[0])
    assert K.harness_quick_hash(reg[n]) == K.harness_quick_hash(reg[0]) and reg[n] != reg[0]
    for c in reg + [s]:
        assert orc.parse_cert(c).ok


def test_claims_are_distinct_in_content_and_hash_and_more_than_both_tables_hold():
    fam = K.claims()
    assert len(fam.chain0) == len(set(fam.chain0)) == K.N_CLAIMS > K.PEND_SLOTS + K.UNREG_CAP
    assert len(fam.pairs) == K.N_CLAIMS + K.N_CLAIM_REPEATS
    assert len({K.quick_hash(c) for c in fam.chain0}) == K.N_CLAIMS
    assert len({len(c) for c in fam.chain0}) == 1 and 540 <= len(fam.chain0[0]) <= 580
    order = fam.info["order"]
    seen, repeats = set(), 0
    for k in order:
        repeats += k in seen
        seen.add(k)
    assert repeats == K.N_CLAIM_REPEATS and len(seen) == K.N_CLAIMS
    for i in (0, 1, 12999, 13000, 13500, 27999):
        assert K.chain0_of([fam.pairs[i]]) == [fam.chain0[order[i]]]
    for c in fam.chain0[::2600]:
        assert orc.parse_cert(c).ok


def test_waves_put_every_class_at_every_lane():
    fam = K.waves()
    assert tuple(len(b) for b in fam.info["batches"]) == K.WAVE_SIZES
    assert {1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097} == set(K.WAVE_SIZES)
    at = {c: set() for c in K.CLASSES}
    uniform = set()
    for pairs, cls in zip(fam.info["batches"], fam.info["classes"]):
        c0 = K.chain0_of(pairs)
        view = K.expected_view(pairs)
        for i, c in enumerate(cls):
            at[c].add(i % 64)
            assert (c0[i] == K.UNDECODABLE) == (c == "undecodable")
            assert (c0[i] is None) == (c == "empty")
            assert (view["entry_type"][i] == 1) == (c == "precert" or (c == "empty" and pairs[i][0][10:12] == b"\x00\x01"))
            if c == "registered":
                assert c0[i] in fam.info["registered"]
            if c == "unregistered":
                assert c0[i] not in fam.info["registered"]
        for row in range(len(cls) // 64):
            if len(set(cls[64 * row:64 * row + 64])) == 1:
                uniform.add(cls[64 * row])
    for c in K.CLASSES:
        assert at[c] == set(range(64)), c
    assert uniform == set(K.CLASSES)                                          # whole waves of one class, each class
    assert {len(c) for c in fam.chain0} == set(K.WAVE_REGISTERED) | set(K.WAVE_UNREGISTERED)
    assert any(len(c) > 3056 for c in fam.chain0) and any(1024 < len(c) < 2048 for c in fam.chain0)


# ------------------------------------------------------------------ the model

@pytest.mark.parametrize("name", sorted(K.FAMILIES))
def test_the_models_framing_is_the_oracles(name):
    """decode_pair / expected_view against orc.decode_entry on every entry (claims: a sample)."""
    fam = K.FAMILIES[name]()
    pairs = fam.pairs if name != "claims" else fam.pairs[::97]
    view = K.expected_view(pairs)
    at = 0
    for i, (leaf, extra) in enumerate(pairs):
        o, d = orc.decode_entry(leaf, extra), K.decode_pair(leaf, extra)
        assert bool(o.ok) == (d is not None), i
        if d is not None:
            assert (d.entry_type, d.cert_in_extra, d.cert_off, d.cert_len, d.n_chain, d.chain0_len) == \
                (o.entry_type, bool(o.cert_in_extra), o.cert_off, o.cert_len, o.n_chain, o.chain0_len), i
            if d.n_chain:
                assert d.chain0_off == o.chain0_off and int(view["chain0_start"][i]) == at + len(leaf) + o.chain0_off
        else:
            assert view["entry_type"][i] == K.ENTRY_INVALID and view["cert_end"][i] == 0 and view["chain0_len"][i] == 0
        at += len(leaf) + len(extra)
    assert sum(view["counters"][:3]) == len(pairs)


def test_model_on_a_hand_made_batch():
    a, b, c = K.length_certs()[530], K.length_certs()[531], K.length_certs()[532]
    pairs = [K.entry(0, b, "x509"), K.undecodable(0), K.entry(1, None, "x509"), K.entry(2, a, "precert"), K.entry(3, b, "x509ff"),
             K.entry(4, c, "x509")]
    assert list(K.expected_issuer_idx(pairs, [a, b, c])) == [1, K.UNDECODABLE, K.NO_ISSUER, 0, 1, 2]
    with pytest.raises(KeyError):
        K.expected_issuer_idx(pairs, [a, b])
    assert K.expected_pending(pairs, [a]) == [b, c] and K.expected_pending(pairs, [a, b, c]) == []
    same = lambda x: 7                                                       # every certificate under one hash
    assert K.expected_pending(pairs, [], same) == [b] and K.expected_pending(pairs, [b], same) == [a]
    reg, rounds = K.expected_self_registration(pairs, [], same)
    assert reg == [b, a, c] and rounds == [[b], [a], [c]]
    reg, rounds = K.expected_self_registration(pairs)
    assert reg == [b, a, c] and rounds == [[b, a, c]]


def oracle_statuses(pairs, profile="reference"):
    raw = RawEntries.from_pairs(pairs)
    o = orc.Engine(b"", True, NOW)
    o.set_profile(profile)
    st, unk, eh, ts = o.raw_batch(np.concatenate([raw.blob, np.zeros(K.PAD, np.uint8)]), raw.bounds)
    return o, st


REACHED = (orc.ST_PASS, orc.ST_PARSE_ERROR, orc.ST_FILTERED_CA, orc.ST_FILTERED_EXPIRED, orc.ST_FILTERED_CN)


@pytest.mark.parametrize("name", ["lengths", "edges", "short", "twins", "waves"])
def test_the_oracle_agrees_with_the_model_on_which_entries_reach_an_issuer(name):
    """raw_batch's status per entry against the dict: undecodable ↔ ST_ENTRY_DECODE_ERROR, an empty chain ↔ ST_NO_ISSUER,
    a Chain[0] ↔ the issuer was parsed: ST_ISSUER_PARSE_ERROR exactly where parse_cert rejects those bytes, else a status
    behind the issuer; and the serials:: keys name exactly the issuer IDs of the Chain[0] certificates that parse."""
    fam = K.FAMILIES[name]()
    o, st = oracle_statuses(fam.pairs)
    idx = K.expected_issuer_idx(fam.pairs, fam.chain0)
    assert ((st == orc.ST_ENTRY_DECODE_ERROR) == (idx == K.UNDECODABLE)).all()
    assert ((st == orc.ST_NO_ISSUER) == (idx == K.NO_ISSUER)).all()
    has = (idx >= 0) & (idx != K.NO_ISSUER)
    assert np.isin(st[has], REACHED + (orc.ST_ISSUER_PARSE_ERROR,)).all()
    # one verdict per certificate, whichever entry carries it; what parse_cert rejects is no issuer (the engine's issuer
    # parse is the stricter one under the reference profile: extension bodies)
    ok_cert = {}
    for k, s1 in zip(idx[has], st[has]):
        assert ok_cert.setdefault(int(k), s1 != orc.ST_ISSUER_PARSE_ERROR) == (s1 != orc.ST_ISSUER_PARSE_ERROR), k
    ids = set()
    for k, c in enumerate(fam.chain0):
        pc = orc.parse_cert(c)
        assert pc.ok or not ok_cert[k], k
        if ok_cert[k]:
            ids.add(orc.issuer_id(c[pc.spki_off:pc.spki_off + pc.spki_len]))
    ok = np.asarray([h and ok_cert[int(k)] for k, h in zip(idx, has)])
    assert (st[ok] == orc.ST_PASS).all()
    seen = {k.split(b"::")[2].decode() for k in o.keys() if k.startswith(b"serials::")}
    assert seen == ids
    if name == "twins":
        assert ok.sum() >= 0.95 * len(fam.pairs), ok.mean()                 # a condition on the corpus
        assert len(ids) > 2                                                  # twins inside the modulus: issuers of their own
    if name == "short":
        assert not ok.any() and has.all()
    if name == "edges":
        assert ok.all() and len(ids) == len(K.EDGE_LENGTHS)
    if name == "lengths":
        assert ok.all() and len(ids) == len(fam.chain0)
        for batch in fam.info["last"]:
            assert (oracle_statuses(batch)[1] == orc.ST_PASS).all()
    o.close()


def test_issuer_ids_of_the_constructed_certificates():
    """The corpus knows the SubjectPublicKeyInfo it put into a certificate: the oracle finds the same octets."""
    for n in (530, 1024, 5003):
        c = K.length_certs()[n]
        off, ln = K.spki_of(c, K.modulus("len%d" % n))
        pc = orc.parse_cert(c)
        assert pc.ok and (pc.spki_off, pc.spki_len) == (off, ln)
        assert orc.sha256(c[off:off + ln]) == hashlib.sha256(c[off:off + ln]).digest()
