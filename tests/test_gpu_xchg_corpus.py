"""-m gpu: the cross-rank dedup at 2 to 16 ranks against constructed key patterns (tests/xchg_corpus.py; what each
builder promises is asserted without a GPU in tests/test_xchg_corpus_cpu.py).  Local groups of several engines on
device 0, as in tests/test_gpu_exchange.py.  Expectations come from the corpus's model — a dict fed the stream in log
order, which knows nothing of owners, tags or filters — and, for the partitions, from its port of the key hashing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr
from ct_mapreduce_amd import synth
from ct_mapreduce_amd.distributed import Group, shard_range
from ct_mapreduce_amd.engine import Batch, RECORD_DTYPE
from tests import xchg_corpus as XC
from tests.gpu_common import run_oracle
from tests.test_gpu_exchange import to_dev, dev_shard, make_engine, check_shards_against_oracle, FILT, NOW, DEV

ISSUER = synth.issuer(synth.config(n_issuers=1), 0)
REC32 = np.dtype([("meta", "<u8"), ("s0", "<u8"), ("s1", "<u8"), ("s2", "<u4"), ("ord", "<u4")])
REC64 = np.dtype([("meta", "<u8"), ("s", "<u8", (5,)), ("src", "<u4"), ("owner", "<u4"), ("ord", "<u8")])
GUARD = 0xA5


def engine(table_slots=1 << 12):
    e = ctmr.Engine(device=0, table_slots=table_slots, pair_slots=1 << 10)
    e.add_issuers([ISSUER])
    e.set_filter(b"", True, 0)
    return e


def group(world, mode, table_slots=1 << 12, bloom_bits=1 << 16):
    engines = [engine(table_slots) for _ in range(world)]
    g = Group.local(engines)
    if mode == "bloom":
        g.bloom_config(bloom_bits)
    return engines, g


def close(engines, g):
    g.close()
    for e in engines:
        e.close()


def batch_of(entries):
    return Batch.from_certs([e.der for e in entries], [0] * len(entries))


def load(shards):
    """One round of the corpus on the device → (tensors to keep, ctmr_shards, the shards' ranges in the round)."""
    keep, out, ranges, lo = [], [], [], 0
    for sh in shards:
        n = len(sh.entries)
        t = to_dev(batch_of(sh.entries))
        keep.append(t)
        out.append(dev_shard(t, n, order_base=sh.order_base))
        ranges.append((lo, lo + n))
        lo += n
    return keep, out, ranges


def run_rounds(g, mode, rounds, tag):
    """Every round through the group; after each, per rank: status, WasUnknown, n_new, the NEW list and by_status equal
    the model's (every entry of these builders parses: status PASS).  → what the last round left, for a replay."""
    verdicts = XC.model_verdicts(rounds)
    last = None
    for rnd, (shards, want) in enumerate(zip(rounds, verdicts)):
        keep, dsh, ranges = load(shards)
        stats = g.map_batch(mode, dsh)
        unk = np.array([v for sh in want for v in sh], np.uint8)
        st = np.zeros(len(unk), np.uint8)
        try:
            check_shards_against_oracle(keep, stats, ranges, st, unk)
        except AssertionError as ex:
            raise AssertionError((tag, mode, "round", rnd)) from ex
        last = (keep, dsh)
    return last


def distinct_keys(rounds):
    return {e.serial for e in XC.stream(rounds) if e.serial is not None}


def check_sets(engines, g, rounds):
    """The group holds every distinct key once: the total, and the members of the one set over all ranks."""
    keys = distinct_keys(rounds)
    assert g.total_count() == len(keys) == sum(e.total_count() for e in engines)
    names = sorted(set(sum((e.keys(b"serials::*") for e in engines), [])))
    assert len(names) == 1
    members = sum((e.set_list(names[0]) for e in engines), [])
    assert len(members) == len(set(members)) and set(members) == keys
    return names[0]


# ------------------------------------------------------------------------------------------------ partitions, exactly
def expected32(p32):
    flat = [r for p in p32 for r in p]
    a = np.zeros(len(flat), REC32)
    for k, r in enumerate(flat):
        a[k] = (r.meta, r.s0, r.s1, r.s2, r.ord)
    return a


def expected64(p64):
    flat = sorted((r for p in p64 for r in p), key=lambda r: (r.owner, r.ord))
    a = np.zeros(len(flat), REC64)
    for k, r in enumerate(flat):
        a[k] = (r.meta, r.s, r.src, r.owner, r.ord & 0xffffffff)
    return a


@pytest.mark.parametrize("world", XC.EDGE_WORLDS)
def test_partitions_equal_the_port_byte_for_byte(world):
    """Engine.xchg_map + Engine.xchg_keys on edges(world) from a low, a middle and the highest rank at every shard length:
    the per-owner counts and every 32-byte record (meta, s0, s1, s2, ord = ord_base + index; ascending log order inside a
    partition; nothing for the rank itself; the guard bytes behind the last record untouched) and every 64-byte record
    (21..40 octets; sorted by (owner, order)) equal what the port says.  Full waves for one owner (the count byte at 64),
    sixteen of them in a block (960 ahead of the last wave), owners in every dword of the count row, lone records in lane
    0 and lane 63: tests/test_xchg_corpus_cpu.py.  Also the device pin of the hash port at every serial length."""
    for rank in XC.edge_ranks(world):
        ents = XC.edges(world, rank)
        eng = engine()
        for n in XC.EDGE_LENGTHS:
            part = ents[:n]
            ord_base = 1000 * (rank + 1) if rank < world - 1 else 0xffffffff - n     # the highest order a round can hold
            p32, p64 = XC.partitions(part, world, rank, ord_base)
            want32, want64 = expected32(p32), expected64(p64)
            t = to_dev(batch_of(part))
            counts, n_long = eng.xchg_map(dev_shard(t, n), world, rank, ord_base)
            assert counts == [len(p) for p in p32], (world, rank, n)
            assert n_long == len(want64), (world, rank, n)
            d32 = torch.full((len(want32) * 32 + 64,), GUARD, dtype=torch.uint8, device=DEV)
            d64 = torch.full((len(want64) * 64 + 64,), GUARD, dtype=torch.uint8, device=DEV)
            counts64 = eng.xchg_keys(world, d32.data_ptr(), d64.data_ptr())
            assert counts64 == [len(p) for p in p64], (world, rank, n)
            got32, got64 = d32.cpu().numpy(), d64.cpu().numpy()
            assert (got32[len(want32) * 32:] == GUARD).all() and (got64[len(want64) * 64:] == GUARD).all(), (world, rank, n)
            g32 = got32[:len(want32) * 32].view(REC32)
            bad = np.nonzero(g32 != want32)[0]
            assert len(bad) == 0, (world, rank, n, bad[:8], g32[bad[:2]], want32[bad[:2]])
            g64 = got64[:len(want64) * 64].view(REC64)
            g64 = g64[np.lexsort((g64["ord"], g64["owner"]))]
            assert g64.tobytes() == want64.tobytes(), (world, rank, n)
        eng.close()


# ------------------------------------------------------------------------------------------------ holder patterns
@pytest.mark.parametrize("mode", ["owner", "bloom"])
@pytest.mark.parametrize("world", XC.HOLDER_WORLDS)
def test_holder_patterns(world, mode):
    """holders(world): every (owner, presenter) pair fresh and held by another rank, two presenters with the owner one of
    them or a third rank, a key from every rank, a key twice in one shard (one wave, two waves, two blocks; the owner's
    shard and another's), a received record that beats the owner's own entry."""
    rounds = XC.holders(world)
    engines, g = group(world, mode)
    keep, dsh = run_rounds(g, mode, rounds, ("holders", world))
    assert g.info().world == world
    check_sets(engines, g, rounds)
    again = g.map_batch(mode, dsh)                                   # a replay of the last round: nothing is new anywhere
    assert all(s.n_new == 0 for s in again)
    assert g.total_count() == len(distinct_keys(rounds))
    close(engines, g)


def test_a_saturated_filter_at_16_ranks():
    """A filter of 64 words per rank under the 3 200 keys that rank presents in two rounds: nearly every key of round 2 hits
    nearly every peer — partitions 4..15 fill and the high bits of the hit mask are set — and the results stay the
    model's.  The traffic threshold is the port's (tests/test_xchg_corpus_cpu.py); the device sends what the port says."""
    world = 16
    rounds = XC.saturating(world)
    engines, g = group(world, "bloom", bloom_bits=XC.SATURATED_BITS)
    verdicts = XC.model_verdicts(rounds)
    traffic = XC.bloom_traffic(rounds, XC.SATURATED_BITS)
    for rnd, shards in enumerate(rounds):
        keep, dsh, ranges = load(shards)
        stats = g.map_batch("bloom", dsh)
        unk = np.array([v for sh in verdicts[rnd] for v in sh], np.uint8)
        check_shards_against_oracle(keep, stats, ranges, np.zeros(len(unk), np.uint8), unk)
        info = g.info()
        print("round", rnd, "keys_sent", info.keys_sent, "port", traffic[rnd], "new keys", int(unk.sum()))
        assert info.keys_sent == info.keys_received == traffic[rnd]
    assert info.keys_sent > 8 * int(unk.sum())
    check_sets(engines, g, rounds)
    close(engines, g)


# ------------------------------------------------------------------------------------------------ twins
@pytest.mark.parametrize("mode", ["owner", "bloom"])
@pytest.mark.parametrize("world", [4, 16])
def test_twins_stay_two_keys(world, mode):
    """Serials equal in their first 8 / 16 / 20 octets, and X against X ‖ 00 at every word and record boundary (up to
    40 → 41, where the partner lives in the host-side set): partners on two ranks in one round and in two rounds are new
    both; presented again from other ranks they are known both."""
    rounds, pairs = XC.twins(world)
    engines, g = group(world, mode)
    run_rounds(g, mode, rounds, ("twins", world))
    name = check_sets(engines, g, rounds)
    for a, b in pairs:                                               # (Bloom mode: SetContains also answers for a SHADOW copy)
        held = [sum(e.set_contains(name, k) for e in engines) for k in (a, b)]
        assert held == [1, 1] if mode == "owner" else min(held) >= 1, (a, b, held)
    close(engines, g)


# ------------------------------------------------------------------------------------------------ tag collisions
@pytest.mark.parametrize("mode,placement", [("owner", "a"), ("owner", "b"), ("owner", "c"), ("owner", "d"),
                                            ("bloom", "c"), ("bloom", "d")])
@pytest.mark.parametrize("world", XC.COLLISION_WORLDS)
def test_tag_collisions_across_ranks(world, mode, placement):
    """Two keys with the same 24-bit tag, the same home slot of a 1 024-slot table and the same owner: (a) both received
    in one round (k_keys_insert defers the second, k_keys_insert2 finds another key under the tag and upserts), (b) one in
    the owner's own shard, (c) one held since an earlier round (k_keys_insert compares the cell and probes on), (d) then
    duplicates of both.  Bloom mode: the holder's filter reports the partner (filler keys cover its bits), so
    k_keys_lookup's table_find walks past the partner's cell, and in (d) k_bloom_apply's does on the asker.  No table may
    rebuild: the home slots would not be the ones searched for."""
    slots = 1024
    pairs, _ = XC.collisions(world, slots)
    rounds, holder = XC.collision_rounds(world, pairs, placement, bloom=mode == "bloom")
    engines, g = group(world, mode, table_slots=slots, bloom_bits=XC.COLLISION_BLOOM_BITS)
    run_rounds(g, mode, rounds, ("collisions", world, placement))
    name = check_sets(engines, g, rounds)
    for e in engines:
        info = e.table_info()
        assert info.rebuilds == 0 and info.slots == slots
    for p in pairs:
        for k in (p.a, p.b):
            at = [r for r, e in enumerate(engines) if e.set_contains(name, k)]
            # (Bloom mode: SetContains also answers for the SHADOW copy a later presenter keeps)
            assert at == [holder[k]] if mode == "owner" else holder[k] in at, (p, k, at)
    close(engines, g)


# ------------------------------------------------------------------------------------------------ a rebuild inside a round
@pytest.mark.parametrize("chunks", [1, 3])
def test_a_table_rebuild_inside_a_round(chunks):
    """World 4, owner mode, tables of 1 024 slots and no cap, three rounds of 3 000 mostly fresh entries per rank: the tables
    rebuild while rounds are open — also in ctmr_xchg_insert_device, after the shard's own entries have claimed their
    slots.  Records equal the single-stream oracle's after every round.

    table_info().occupied is ctmr_engine::occupied (ctmr_engine.hip): "slots claimed since the table was last (re)built:
    live members + tombstones" — index slots of the device table.  Nothing is removed here (no tombstones), owner mode has
    no SHADOW cells, and members of host-side sets (serials beyond 40 octets) claim no slot: occupied = total_count()
    less the rank's host-set members, of which this stream has none (asserted)."""
    world, rounds, per = 4, 3, 3000
    cfg = synth.config(seed=77, n_issuers=8, dup_permille=150, ca_permille=20, expired_permille=20)
    issuers = synth.issuers(cfg)
    engines = [make_engine(issuers, table_slots=1 << 10) for _ in range(world)]
    g = Group.local(engines)
    if chunks > 1:
        g.set_chunks(chunks)
    o = None
    rose = set()
    for rnd in range(rounds):
        base = rnd * per * world
        keep, shards, want = [], [], []
        for r in range(world):
            lo, hi = shard_range(per * world, r, world)
            b = synth.host_batch(cfg, base + lo, hi - lo)
            o, st, unk, _ = run_oracle(b, issuers, FILT, False, NOW, engine=o)
            want.append((st, unk))
            t = to_dev(b)
            keep.append(t)
            shards.append(dev_shard(t, hi - lo, order_base=base + lo))
        before = [e.table_info().rebuilds for e in engines]
        stats = g.map_batch("owner", shards)
        after = [e.table_info() for e in engines]
        rose |= {r for r in range(world) if after[r].rebuilds > before[r]}
        for r in range(world):
            st, unk = want[r]
            rec = keep[r][4].cpu().numpy().view(RECORD_DTYPE)[:len(st)]
            assert (rec["status"] == st).all(), (rnd, r)
            assert (((rec["flags"] & 2) != 0) == (unk != 0)).all(), (rnd, r)
            assert stats[r].n_new == int(unk.sum()) and stats[r].n_host_set == 0
            assert (keep[r][5][:stats[r].n_new].cpu().numpy() == np.nonzero(unk)[0]).all()
            print("round", rnd, "rank", r, "slots", after[r].slots, "occupied", after[r].occupied, "total_count", engines[r].total_count(),
                  "rebuilds", after[r].rebuilds)
        for r in range(world):
            assert after[r].occupied == engines[r].total_count(), (rnd, r, after[r].occupied, engines[r].total_count())
    assert len(rose) >= 2, rose
    assert g.total_count() == o.total_count() == sum(e.total_count() for e in engines)
    close(engines, g)
