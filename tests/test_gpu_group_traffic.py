"""-m gpu: what a group round MOVES between its ranks, pinned to recorded values.  The other group tests hold the results
to the oracle and the traffic counters only to `sent == received > 0`: count plumbing that moves every key correctly and
counts it wrongly would pass them.  Here a local group of three engines on one device runs three rounds per mode — owner,
owner mapped in three chunks, bloom — and after every round ctmr_group_info's keys_sent, keys_received,
filter_bytes_received and wire_bytes_sent must equal tests/golden/group_traffic.json: integers recorded once (the file
names the commit), none of them computed by the code under test at test time.

The shards are the smallest that take every branch of the count plumbing: 2 100 entries (with three chunks the chunk size
rounds to 1 024: [0, 1024), [1024, 2048) and a partial last block), 700 entries (chunks 1 and 2 empty) and an empty shard
that still owns keys.  Serials of 21..40 octets on the first two shards put records on the 64-byte side channel in both
directions, two serials beyond CTMR_MAX_SERIAL take round_finish past its first return, and rounds 2 and 3 repeat part of
round 1 so that owners answer "known"."""
import json
import os
import random

import pytest

pytestmark = pytest.mark.gpu

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import synth  # noqa: E402
from ct_mapreduce_amd.distributed import Group  # noqa: E402
from tests import der as D  # noqa: E402
from tests.test_gpu_exchange import to_dev, dev_shard  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "group_traffic.json")
MODES = ["owner", "owner_chunks3", "bloom"]
FIELDS = ("keys_sent", "keys_received", "filter_bytes_received", "wire_bytes_sent")
SIZES = (2100, 700, 0)                                            # shards A, B, C of every round
FIRST = ((0, 2100), (1050, 3150), (0, 3850))                      # where A and B begin in the synthetic stream, per round
# where the constructed certificates stand: (shard, entry) → octets of the serial; the same serials in every round
SPECIAL = {(0, 5): 21, (0, 700): 33, (0, 1030): 40, (0, 1500): 25, (0, 2070): 21, (0, 2099): 38,
           (1, 3): 22, (1, 300): 40, (1, 650): 29, (1, 699): 36,
           (0, 100): 41, (1, 200): 57}


def rounds():
    """Three rounds of three host batches, built once: the same bytes whatever ran before."""
    cfg = synth.config(seed=83, n_issuers=6, dup_permille=200, ca_permille=0, expired_permille=0)
    issuers = synth.issuers(cfg)
    rng = random.Random(8383)
    name = D.name(D.rdn(3, b"Synth Issuer 000"))
    special = {}
    for at, ln in sorted(SPECIAL.items()):
        s = bytes([rng.randrange(1, 0x7f)] + [rng.randrange(256) for _ in range(ln - 1)])
        special[at] = D.cert(serial=s, issuer=name, not_after=D.utctime("270101000000Z"))
    out = []
    for first in FIRST:
        batches = []
        for k, n in enumerate(SIZES):
            b = synth.host_batch(cfg, first[k] if n else 0, n)
            certs = [b.cert(i) for i in range(n)]
            idx = b.issuer_idx.copy()
            for (sk, i), c in special.items():
                if sk == k:
                    certs[i], idx[i] = c, 0
            batches.append(ctmr.Batch.from_certs(certs, idx, b.entry_type) if n else b)
        out.append(batches)
    return issuers, out


def measure(mode, issuers, rnds):
    """One group, kept over the three rounds: [[keys_sent, keys_received, filter_bytes_received, wire_bytes_sent]] per round."""
    engines = []
    for _ in SIZES:
        e = ctmr.Engine(device=0, table_slots=1 << 14, pair_slots=1 << 10)
        e.add_issuers(issuers)
        e.set_filter(b"", True, 0)
        engines.append(e)
    g = Group.local(engines)
    if mode == "bloom":
        g.bloom_config(1 << 14)
    if mode == "owner_chunks3":
        g.set_chunks(3)
    got, base = [], 0
    for batches in rnds:
        keep = [to_dev(b) for b in batches]
        shards = []
        for t, n in zip(keep, SIZES):
            shards.append(dev_shard(t, n, order_base=base))
            base += n
        stats = g.map_batch("bloom" if mode == "bloom" else "owner", shards)
        assert sum(int(s.n_host_set) for s in stats) > 0         # the serials beyond CTMR_MAX_SERIAL were there
        info = g.info()
        got.append([int(getattr(info, f)) for f in FIELDS])
    g.close()
    for e in engines:
        e.close()
    return got


@pytest.fixture(scope="module")
def traffic():
    issuers, rnds = rounds()
    return {mode: measure(mode, issuers, rnds) for mode in MODES}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("mode", MODES)
def test_traffic_counters_equal_the_recorded_values(mode, traffic, golden):
    assert golden["fields"] == list(FIELDS)
    for rnd, (got, want) in enumerate(zip(traffic[mode], golden[mode])):
        print(mode, rnd, got)
        assert got == want, (mode, rnd, dict(zip(FIELDS, got)), dict(zip(FIELDS, want)))
    assert len(traffic[mode]) == len(golden[mode]) == len(FIRST)


def test_chunked_owner_rounds_move_the_same_keys(traffic):
    for rnd, (a, b) in enumerate(zip(traffic["owner"], traffic["owner_chunks3"])):
        assert a[:2] == b[:2] and a[0] == a[1] > 0, (rnd, a, b)
