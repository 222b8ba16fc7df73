"""tests/xchg_corpus.py held to its conditions, without a GPU: every situation the builders promise occurs (counted with
the hash port, counts in the assertion messages), the model agrees with the single-stream oracle entry for entry, every
wrong model the corpus is meant to catch differs from the true one on at least one entry, and the port equals the host
build of the product's own hash functions."""
import ctypes as C
import random
from collections import Counter, defaultdict

import numpy as np
import pytest

from ct_mapreduce_amd import synth
from ct_mapreduce_amd.engine import Batch
from oracle import oracle as orc
from tests import harness, xchg_corpus as XC
from tests.gpu_common import run_oracle

ISSUER = synth.issuer(synth.config(n_issuers=1), 0)


def positive(counts):
    print(counts)
    assert counts and min(counts.values()) > 0, counts


# ------------------------------------------------------------------------------------------------ the port
def test_the_port_equals_the_host_build_of_the_product_headers():
    lib = harness.hash_lib()
    rng = random.Random(7)
    for ln in list(range(0, 41)) * 8:
        serial = bytes(rng.randrange(256) for _ in range(ln))
        exp_hour, canon = rng.randrange(-5, 1 << 20), rng.randrange(1 << 24)
        meta = XC.key_meta(exp_hour, canon, ln)
        assert meta == lib.harness_key_meta(exp_hour, canon, ln)
        s = XC.serial_words(serial)
        h = XC.key_hash(meta, s)
        assert h == lib.harness_key_hash(meta, (C.c_uint64 * 5)(*s))
        assert XC.mixk(h) == lib.harness_mixk(h)
        assert XC.key_tag(h) == lib.harness_key_tag(h)
        for world in (1, 2, 3, 5, 8, 15, 16):
            assert XC.key_owner_h(h, world) == lib.harness_key_owner_h(h, world)
        for wmask in (63, 1023, (1 << 20) - 1):
            w, b = C.c_uint64(), C.c_uint64()
            lib.harness_bloom_pos(h, wmask, C.byref(w), C.byref(b))
            assert XC.bloom_pos(h, wmask) == (w.value, b.value)
    for h in (0, 1 << 40, (1 << 64) - 1, 0xffffff << 40, (0xffffff << 40) - 1):      # the tags that are moved aside
        assert XC.key_tag(h) == lib.harness_key_tag(h)
    assert XC.key_tag(0) == 1 and XC.key_tag((1 << 64) - 1) == 0xfffffe


def test_the_numpy_forms_equal_the_integer_port():
    s = XC.np_serials8(5, 3000)
    h = XC.np_key_hash8(s)
    tag, word_bits = XC.np_key_tag(h), XC.np_bloom_pos(h, 1023)
    owners = {w: XC.np_key_owner_h(h, w) for w in (4, 5, 16)}
    for k in range(0, len(s), 7):
        serial = XC.s8(s[k])
        assert 1 <= serial[0] < 0x7f
        hh = XC.serial_hash(serial)
        assert hh == int(h[k]) and XC.key_tag(hh) == int(tag[k])
        assert XC.bloom_pos(hh, 1023) == (int(word_bits[0][k]), int(word_bits[1][k]))
        for w, o in owners.items():
            assert XC.key_owner_h(hh, w) == int(o[k])
    assert len(set(s.tolist())) == len(s)


def test_the_certificates_carry_the_key_the_port_assumes():
    c = orc.parse_cert(XC.cert(b"\x01\x02\x03"))
    assert c.ok and c.serial_len == 3 and orc.exp_hour(c.not_after) == XC.EXP_HOUR
    assert not orc.parse_cert(XC.bad_entry().der).ok


# ------------------------------------------------------------------------------------------------ coverage: holders
def holder_cells(world, rounds):
    fresh, known, triples, cells = set(), set(), set(), Counter()
    for name in XC.PLACEMENTS:
        cells[("non-owner's shard", name)] = cells[("owner's shard", name)] = 0
    cells["every rank"] = cells["a lower non-owner and the owner"] = cells["the owner and a higher non-owner"] = 0
    seen_by = {}
    for shards in rounds:
        assert [sh.order_base for sh in shards] == sorted(sh.order_base for sh in shards)
        pres = defaultdict(list)
        for r, sh in enumerate(shards):
            for i, e in enumerate(sh.entries):
                pres[e.serial].append((r, i))
        for k, pl in pres.items():
            o, ranks, before = XC.serial_owner(k, world), sorted({r for r, _ in pl}), seen_by.get(k)
            if before is None and len(pl) == 1:
                fresh.add((o, ranks[0]))
            if before is not None and len(pl) == 1 and ranks[0] not in before:
                known.add((o, ranks[0]))
            if before is None and len(pl) == 2 and len(ranks) == 2:
                triples.add((ranks[0], ranks[1], o))
                cells["a lower non-owner and the owner"] += ranks[1] == o
                cells["the owner and a higher non-owner"] += ranks[0] == o
            if before is None and len(ranks) == world:
                cells["every rank"] += 1
            if before is None and len(pl) == 2 and len(ranks) == 1:
                (_, i), (_, j) = pl
                where = "wave" if i // 64 == j // 64 else "block" if i // 1024 == j // 1024 else "blocks"
                cells[("owner's shard" if o == ranks[0] else "non-owner's shard", where)] += 1
        for k, pl in pres.items():
            seen_by.setdefault(k, set()).update(r for r, _ in pl)
    return fresh, known, triples, cells


@pytest.mark.parametrize("world", XC.HOLDER_WORLDS)
def test_holders_cover_every_situation(world):
    rounds = XC.holders(world)
    assert len(rounds) == 2 and all(len(shards) == world for shards in rounds)
    assert max(len(sh.entries) for shards in rounds for sh in shards) <= 2049
    fresh, known, triples, cells = holder_cells(world, rounds)
    every_pair = {(o, f) for o in range(world) for f in range(world)}
    assert fresh == every_pair, sorted(every_pair - fresh)
    assert known == every_pair, sorted(every_pair - known)
    pairs = {(a, b) for a in range(world) for b in range(a + 1, world)}
    assert {(a, b) for a, b, _ in triples} == pairs
    if world <= 5:
        assert triples == {(a, b, o) for a, b in pairs for o in range(world)}
    classes = Counter("f1" if o == a else "f2" if o == b else "third" for a, b, o in triples)
    cells.update({("two presenters, owner", c): classes[c] for c in (("f1", "f2", "third") if world > 2 else ("f1", "f2"))})
    cells["(owner, presenter) fresh"], cells["(owner, presenter) held by another rank"] = len(fresh), len(known)
    positive(cells)


# ------------------------------------------------------------------------------------------------ coverage: edges
def wave_counts(entries, world, rank):
    """Per wave of 64 entries: 32-byte records per owner, as the port partitions them."""
    n_waves = (len(entries) + 63) // 64
    cnt = np.zeros((n_waves, world), int)
    for i, e in enumerate(entries):
        if e.serial is not None and len(e.serial) <= 20:
            o = XC.serial_owner(e.serial, world)
            if o != rank:
                cnt[i // 64, o] += 1
    return cnt


@pytest.mark.parametrize("world", XC.EDGE_WORLDS)
def test_edges_cover_every_situation(world):
    for rank in XC.edge_ranks(world):
        ents = XC.edges(world, rank)
        assert len(ents) == 2049 == max(XC.EDGE_LENGTHS)
        cnt = wave_counts(ents, world, rank)
        remote = [o for o in range(world) if o != rank]
        tot = cnt.sum(axis=1)
        cells = Counter()
        cells["a wave of 64 for the lowest remote owner"] = int((cnt[:, remote[0]] == 64).sum())
        cells["a wave of 64 for the highest remote owner"] = int((cnt[:, remote[-1]] == 64).sum())
        for d in range((world + 3) // 4):
            if any(o != rank for o in range(4 * d, min(4 * d + 4, world))):
                cells[("a wave of 64 for an owner in count dword", d)] = int((cnt[:, 4 * d:4 * d + 4] == 64).any(axis=1).sum())
        for b in range(2):
            blk = cnt[16 * b:16 * b + 16]
            cells["a block of sixteen full waves for one owner"] += int((blk == 64).all(axis=0).any())
            cells["960 records ahead of a block's last wave"] += int((blk[:15].sum(axis=0) == 960).any())
        lane = lambda w, l: (lambda e: e.serial is not None and len(e.serial) <= 40 and XC.serial_owner(e.serial, world) != rank)(ents[64 * w + l])
        for w in range(32):
            only = tot[w] == 1
            cells["a wave whose only remote record is lane 0"] += bool(only and lane(w, 0))
            cells["a wave whose only remote record is lane 63"] += bool(only and lane(w, 63))
            cells["an empty wave between waves with records"] += bool(0 < w < 31 and tot[w] == 0 and tot[w - 1] and tot[w + 1])
            cells["a wave with a record for every remote owner"] += bool((cnt[w, remote] > 0).all())
            wave = ents[64 * w:64 * w + 64]
            cells["a parse error and a 41-octet serial in a wave of 62 records"] += bool(
                tot[w] == 62 and any(e.serial is None for e in wave) and any(e.serial and len(e.serial) == 41 for e in wave))
        p32, p64 = XC.partitions(ents, world, rank, 0)
        lens32 = Counter(r.meta >> 56 & 0x7f for p in p32 for r in p)
        lens64 = Counter(r.meta >> 56 & 0x7f for p in p64 for r in p)
        for ln in range(1, 21):
            cells[("32-byte records with a serial of", ln)] = lens32[ln]
        for ln in range(21, 41):
            cells[("64-byte records with a serial of", ln)] = lens64[ln]
        assert not p32[rank] and not p64[rank] and set(lens32) <= set(range(1, 21)) and set(lens64) <= set(range(21, 41))
        if remote[-1] > 3:                                               # (world 5 from rank 4: every remote owner is below 4)
            cells["owners above 3 with records"] = sum(1 for o in range(4, world) if p32[o])
        positive(cells)


# ------------------------------------------------------------------------------------------------ coverage: twins
@pytest.mark.parametrize("world", [4, 16])
def test_twins_cover_every_situation(world):
    rounds, pairs = XC.twins(world)
    where = defaultdict(list)
    for rnd, shards in enumerate(rounds[:2]):
        for r, sh in enumerate(shards):
            for e in sh.entries:
                where[e.serial].append((rnd, r))
    cells = Counter()
    for a, b in pairs:
        assert a != b and len(where[a]) == len(where[b]) == 1
        (ra, ka), (rb, kb) = where[a][0], where[b][0]
        assert ka != kb
        place = "one round, two ranks" if ra == rb else "two rounds, two ranks"
        if b == a + b"\x00":
            assert XC.serial_words(a) == XC.serial_words(b[:40]) and XC.serial_meta(a) != XC.serial_meta(b)
            cells[("X against X ‖ 00, length", len(a), place)] += 1
        else:
            assert len(a) == len(b)
            p = next(k for k in range(len(a)) if a[k] != b[k])
            cls = max(q for q in XC.TWIN_PREFIXES if q <= p)
            assert a[:cls] == b[:cls]
            cells[("equal in the first", cls, place)] += 1
    for place in ("one round, two ranks", "two rounds, two ranks"):
        for ln in XC.TWIN_LENGTHS:
            cells[("X against X ‖ 00, length", ln, place)] += 0
        for cls in XC.TWIN_PREFIXES:
            cells[("equal in the first", cls, place)] += 0
    positive(cells)
    verdicts = XC.model_verdicts(rounds)
    assert sum(sum(v) for v in verdicts[0]) + sum(sum(v) for v in verdicts[1]) == 2 * len(pairs)     # all of them are keys of their own
    assert not any(any(v) for v in verdicts[2])


# ------------------------------------------------------------------------------------------------ coverage: collisions
@pytest.mark.parametrize("world", XC.COLLISION_WORLDS)
def test_collisions_are_collisions(world):
    slots = 1024
    pairs, found = XC.collisions(world, slots)
    print(world, "pairs found:", found, "taken:", len(pairs))
    # expected: 2^44 / 2 pairs, each equal in 24 + 10 bits and the owner with probability 2^-34 / world: 512 / world
    assert len(pairs) == 12 <= found, (found, len(pairs))
    everything = [x for p in pairs for x in (p.a, p.b) + p.fillers]
    assert len(set(everything)) == len(everything)
    wmask = XC.COLLISION_BLOOM_BITS // 64 - 1
    for p in pairs:
        ha, hb = XC.serial_hash(p.a), XC.serial_hash(p.b)
        assert p.a != p.b and XC.key_tag(ha) == XC.key_tag(hb) and ha & (slots - 1) == hb & (slots - 1)
        assert XC.key_owner_h(ha, world) == XC.key_owner_h(hb, world) == p.owner
        word, bits = XC.bloom_pos(hb, wmask)
        have = 0
        for f in p.fillers:
            w, b = XC.bloom_pos(XC.serial_hash(f), wmask)
            assert w == word
            have |= b
        assert 1 <= len(p.fillers) <= 4 and have & bits == bits          # the holder's filter reports b
    cells = Counter()
    for placement in "abcd":
        rounds, holder = XC.collision_rounds(world, pairs, placement)
        assert 2 * len(XC.stream(rounds)) < slots * 3 // 4          # no rebuild, whatever a rank reserves: 3/4 of the slots is never near
        at = [{e.serial: r for r, sh in enumerate(shards) for e in sh.entries} for shards in rounds]
        for p in pairs:
            assert holder[p.a] == holder[p.b] == p.owner
            if placement == "a":
                cells["(a) both received from two senders"] += p.owner not in (at[0][p.a], at[0][p.b]) and at[0][p.a] != at[0][p.b]
            elif placement == "b":
                cells["(b) one in the owner's shard, one received"] += sorted((at[0][p.a] == p.owner, at[0][p.b] == p.owner)) == [False, True]
            else:
                cells["(%s) one held, one received" % placement] += at[0][p.a] != p.owner and at[1][p.b] not in (p.owner, at[0][p.a])
                if placement == "d":
                    cells["(d) duplicates of both from a third rank"] += at[2][p.a] == at[2][p.b] not in (p.owner, at[0][p.a], at[1][p.b])
    for placement in "cd":
        rounds, holder = XC.collision_rounds(world, pairs, placement, bloom=True)
        at0 = {e.serial: r for r, sh in enumerate(rounds[0]) for e in sh.entries}
        for p in pairs:
            cells["(%s) Bloom: the fillers sit with a's presenter, which holds a" % placement] += \
                all(at0[f] == at0[p.a] == holder[p.a] for f in p.fillers) and holder[p.b] != holder[p.a]
    assert all(v == len(pairs) for v in cells.values()), cells
    positive(cells)


# ------------------------------------------------------------------------------------------------ the saturated filter
def test_a_filter_of_64_words_is_saturated_by_3200_keys():
    """The threshold the device test relies on — more than 8 key records per new key in round 2 at 16 ranks — held against
    the port: every rank's 64-word filter holds the 3 200 keys that rank presented by the time round 2 is probed."""
    rounds = XC.saturating()
    sent = XC.bloom_traffic(rounds, XC.SATURATED_BITS)
    n2 = sum(len(sh.entries) for sh in rounds[1])
    keys = [e.serial for e in XC.stream(rounds)]
    assert len(set(keys)) == len(keys) == 2 * n2 and n2 == 16 * XC.SATURATED_PER_RANK
    assert max(len(sh.entries) for shards in rounds for sh in shards) <= 2049
    print("key records in round 1, round 2:", sent, "new keys in round 2:", n2)
    assert sent[1] > 8 * n2, (sent, n2)
    filt = defaultdict(int)
    for shards in rounds:
        for e in shards[0].entries:
            w, b = XC.bloom_pos(XC.serial_hash(e.serial), XC.SATURATED_BITS // 64 - 1)
            filt[w] |= b
    full = sum(bin(v).count("1") for v in filt.values()) / XC.SATURATED_BITS
    assert full > 0.93, full                                             # 1 − e^(−3200 · 4 / 4096) = 0.956
    owners = Counter(XC.serial_owner(k, 16) for k in keys)
    assert all(owners[o] > 0 for o in range(16))


# ------------------------------------------------------------------------------------------------ model against the oracle
def oracle_verdicts(entries):
    b = Batch.from_certs([e.der for e in entries], [0] * len(entries))
    b.payload = np.concatenate([b.payload, np.zeros(64, np.uint8)])
    _, st, unk, _ = run_oracle(b, [ISSUER], b"", True, 0)
    return st, unk


def assert_model_is_the_oracle(rounds):
    ents = XC.stream(rounds)
    st, unk = oracle_verdicts(ents)
    want = [v for shards in XC.model_verdicts(rounds) for sh in shards for v in sh]
    assert [s == 0 for s in st] == [e.serial is not None for e in ents]
    assert [bool(u) for u in unk] == want
    return len(ents)


def all_builders():
    for world in XC.HOLDER_WORLDS:
        yield ("holders", world), XC.holders(world)
    for world in XC.EDGE_WORLDS:
        for rank in XC.edge_ranks(world):
            yield ("edges", world, rank), XC.make_rounds([[XC.edges(world, rank)]])
    for world in (4, 16):
        yield ("twins", world), XC.twins(world)[0]
    for world in XC.COLLISION_WORLDS:
        pairs, _ = XC.collisions(world, 1024)
        for placement in "abcd":
            yield ("collisions", world, placement), XC.collision_rounds(world, pairs, placement)[0]
        for placement in "cd":
            yield ("collisions, Bloom", world, placement), XC.collision_rounds(world, pairs, placement, bloom=True)[0]
    yield ("saturating", 16), XC.saturating()


def test_the_model_equals_the_single_stream_oracle():
    n = 0
    for name, rounds in all_builders():
        try:
            n += assert_model_is_the_oracle(rounds)
        except AssertionError as ex:
            raise AssertionError(name) from ex
    print("entries compared:", n)


# ------------------------------------------------------------------------------------------------ sensitivity
def flat(verdicts):
    return [v for shards in verdicts for sh in shards for v in sh]


def wrong_winner(rounds, pick, per_rank_memory=False):
    """A model in which, of the presenters (rank, index) of a key that is new in a round, pick(presenters) keeps WasUnknown;
    per_rank_memory: a key counts as known only to the ranks that presented it in an earlier round."""
    seen, out = {}, []
    for shards in rounds:
        pres = defaultdict(list)
        for r, sh in enumerate(shards):
            for i, e in enumerate(sh.entries):
                if e.serial is not None:
                    pres[e.serial].append((r, i))
        v = [[False] * len(sh.entries) for sh in shards]
        for k, pl in pres.items():
            if per_rank_memory:
                pl = [(r, i) for r, i in pl if r not in seen.get(k, ())]
            elif k in seen:
                pl = []
            if pl:
                r, i = pick(pl)
                v[r][i] = True
        for k, pl in pres.items():
            seen.setdefault(k, set()).update(r for r, _ in pl)
        out.append(v)
    return out


def differs(rounds, wrong):
    return sum(a != b for a, b in zip(flat(XC.model_verdicts(rounds)), flat(wrong)))


@pytest.mark.parametrize("world", XC.HOLDER_WORLDS)
def test_holders_refuse_the_wrong_winners(world):
    rounds = XC.holders(world)
    assert differs(rounds, wrong_winner(rounds, min)) == 0                                   # the helper itself: the true rule
    got = {
        "the highest order of the round wins": differs(rounds, wrong_winner(rounds, max)),
        "inside one shard the later index wins": differs(rounds, wrong_winner(rounds, lambda pl: max(p for p in pl if p[0] == min(pl)[0]))),
        "held by another rank counts as new": differs(rounds, wrong_winner(rounds, min, per_rank_memory=True)),
    }
    positive(got)


def test_collisions_and_twins_refuse_the_wrong_identities():
    got = {}
    for world in XC.COLLISION_WORLDS:
        pairs, _ = XC.collisions(world, 1024)
        by_slot = lambda e: (lambda h: (XC.key_tag(h), h & 1023, XC.key_owner_h(h, world)))(XC.serial_hash(e.serial))
        for placement in "abcd":
            rounds, _ = XC.collision_rounds(world, pairs, placement)
            got[("keys are (tag, home slot, owner)", world, placement)] = \
                differs(rounds, XC.model_verdicts(rounds, XC.Model(key=by_slot)))
    for world in (4, 16):
        rounds, _ = XC.twins(world)
        got[("keys are their first 20 octets", world)] = \
            differs(rounds, XC.model_verdicts(rounds, XC.Model(key=lambda e: e.serial[:20])))
        got[("keys are their zero-padded words", world)] = \
            differs(rounds, XC.model_verdicts(rounds, XC.Model(key=lambda e: e.serial + bytes(48 - len(e.serial)))))
    positive(got)


@pytest.mark.parametrize("world", XC.EDGE_WORLDS)
def test_edges_refuse_the_wrong_owners(world):
    """(From the highest rank of world 5 every remote owner is below 4: the modulo shows from the other senders.)"""
    got = Counter()
    for rank in XC.edge_ranks(world):
        ents = XC.edges(world, rank)
        for n in XC.EDGE_LENGTHS:
            true = XC.partitions(ents[:n], world, rank, 0)
            got["the owner modulo 4"] += true != XC.partitions(ents[:n], world, rank, 0, lambda h, w: XC.key_owner_h(h, w) % 4)
            got["the owner under world − 1"] += true != XC.partitions(ents[:n], world, rank, 0, lambda h, w: XC.key_owner_h(h, w - 1))
        ents = ents[:64]
        assert XC.partitions(ents, world, rank, 5) != XC.partitions(ents, world, rank, 6)   # the order is part of the record
    positive(got)
