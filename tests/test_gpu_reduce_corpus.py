"""-m gpu: the in-batch reduce of one engine against constructed duplicate and tag patterns (tests/reduce_corpus.py; what
each builder promises, and that its dict model IS the oracle, is asserted without a GPU in tests/test_reduce_corpus_cpu.py).

Both map variants of tests/test_gpu_parity.py: 15 (k_map_fused: pass 1 of the insert inside the map) and 13 (k_map_winc +
k_insert).  Both support strict_spki — k_insert leaves an entry whose EC key owes the curve equation ES_PENDING exactly as
the fused kernel does, and k_ec_resolve inserts it — so group F runs under both.

After every batch: every record field, flags, new_idx, n_new and by_status against the oracle (assert_records_equal) and
stats.n_dup.  After every case: the state against the oracle (assert_state_equal), total_count() against the model's
distinct keys, and set_list of every set against the model's members, none twice.  The 64-slot cases (C, D) also ask
set_contains and a refused set_insert for every key, and that the index was never rebuilt (the home slots would not be the
ones searched for).  Nothing here reads anything outside the repository."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import _native as N  # noqa: E402
from ct_mapreduce_amd.engine import Batch  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import reduce_corpus as R  # noqa: E402
from tests.gpu_common import run_oracle, assert_records_equal, assert_state_equal  # noqa: E402

VARIANTS = {"winc_separate_insert": (13, 0, 0), "fused": (15, 0, 0)}
_reference = {}


def reference(c):
    """The oracle's verdicts on the case, batch by batch, its final state and the model's — computed once, shared by the
    variants, read only."""
    ref = _reference.get(c.name)
    if ref is None:
        o, batches = None, []
        for b in c.batches:
            batch = Batch.from_certs([e.der for e in b], [e.iss for e in b])
            batch.payload = np.concatenate([batch.payload, np.zeros(N.PAYLOAD_PAD, np.uint8)])
            o, st, unk, eh = run_oracle(batch, R.ISSUERS, b"", False, R.NOW, engine=o)
            batches.append((batch, st, unk, eh))
        want, model = R.model_verdicts(c)
        for (_, st, unk, _), w, b in zip(batches, want, c.batches):
            assert [bool(u) for u in unk] == w and [s == orc.ST_PASS for s in st] == [e.key is not None for e in b]
        ref = _reference[c.name] = (batches, o, model)
    return ref


def run_case(c, variant):
    batches, o, model = reference(c)
    v, tile, lds = variant
    eng = ctmr.Engine(device=0, map_variant=v, certs_per_tile=tile, lds_tile_bytes=lds, table_slots=c.slots, pair_slots=1 << 10)
    try:
        eng.add_issuers(R.ISSUERS)
        assert [eng.issuer_info(k).canonical_idx for k in range(len(R.ISSUERS))] == R.CANON
        eng.set_filter(b"", False, R.NOW)
        known = 0
        for k, (batch, st, unk, eh) in enumerate(batches):
            res = eng.map_batch(batch)
            known += int(unk.sum())
            try:
                assert_records_equal(res, batch, st, unk, eh)
                assert res.stats.n_dup == int(((st == orc.ST_PASS) & (unk == 0)).sum())
                assert eng.total_count() == known                    # (a replay, forward or reversed, leaves the state as it was)
            except AssertionError as ex:
                raise AssertionError("batch %d: %s" % (k, str(ex).splitlines()[0] if str(ex) else "")) from ex
        assert_state_equal(eng, o, len(R.ISSUERS))
        assert eng.total_count() == len(model.seen)
        members = {}
        for hour, canon, serial in model.seen:
            name = ("serials::%s::%s" % (orc.exp_date_id(hour), eng.issuer_id(canon))).encode()
            members.setdefault(name, []).append(serial)
        assert sorted(eng.keys(b"serials::*")) == sorted(members)
        for name, want in members.items():
            got = eng.set_list(name)
            assert len(got) == len(set(got)) == len(want) and set(got) == set(want), name
        if c.slots == R.SLOTS:
            for name, want in members.items():
                for m in want:
                    assert eng.set_contains(name, m) and not eng.set_insert(name, m), m
            info = eng.table_info()
            assert info.rebuilds == 0 and info.slots == R.SLOTS and info.occupied == len(model.seen)
            assert eng.total_count() == len(model.seen)
    finally:
        eng.close()


@pytest.mark.parametrize("group", ["A", "B", "C", "D", "E", "F"])
@pytest.mark.parametrize("variant", list(VARIANTS), ids=list(VARIANTS))
def test_the_reduce_on_constructed_patterns(variant, group):
    """Every case of the group; the failing cases are all named, not the first one only."""
    cases = [c for c in R.cases() if c.group == group]
    assert cases
    t0 = time.perf_counter()
    failed = []
    for c in cases:
        try:
            run_case(c, VARIANTS[variant])
        except AssertionError as ex:
            failed.append("%s: %s" % (c.name, str(ex).splitlines()[0] if str(ex) else "assertion"))
    print("group %s, %s: %d cases, %d entries, %.2f s" % (group, variant, len(cases), sum(len(b) for c in cases for b in c.batches),
                                                           time.perf_counter() - t0))
    assert not failed, "\n".join(failed)
