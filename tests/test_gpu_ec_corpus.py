"""-m gpu: the curve equation on the device, at the values where multi-limb arithmetic goes wrong (tests/ec_corpus.py:
coordinates next to 0 and p, around every limb boundary, patterned limbs, unreduced x + m·p, both roots of every x that has
one), at all three sites it runs at — k_ec_resolve<true> (P-256) and k_ec_resolve<false> (the other four curves) behind
the map, and the in-walk ec_on_curve of issuer registration and of the strict_leaf TBS check — every test bit for bit
against the oracle and, for the status, against the verdict of Python's integers.  Plus k_ec_resolve's block structure:
a block's pending list full between the two instantiations and in one, 257 pending entries in a block, a batch that ends
inside a group of four with a pending entry last, in-batch duplicates, a second pass over the same batch.

The device code is compiled apart from the host build tests/test_ec_corpus_cpu.py checks (rolled loop, 64-bit multiply-add
chains, 206 VGPRs for P-521): the same cases, no sampling."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import synth, _native as N  # noqa: E402
from ct_mapreduce_amd.engine import Batch, RawEntries  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import ec_corpus as E  # noqa: E402
from tests.gpu_common import run_oracle, assert_records_equal, assert_state_equal  # noqa: E402
from tests.test_gpu_entries import check_against_oracle  # noqa: E402
from tests.test_spki_cpu import CURVES  # noqa: E402

NOW = synth.BASE_TIME
RSA_ISSUER = E.RSA_ISSUER


def padded(batch):
    batch.payload = np.concatenate([batch.payload, np.zeros(N.PAYLOAD_PAD, np.uint8)])
    return batch


def map_twice_against_the_oracle(ent, table=1 << 16):
    """One engine and one good issuer, the batch (ec_corpus.Entries) mapped twice; records and state against the oracle
    after each pass.  Independently of the oracle: an X509 entry is PARSE_ERROR exactly when the integer verdict on its key
    is False; after the first pass the table holds exactly ent.stored certificates; the second pass finds every one of them
    known and stores nothing."""
    certs, ets, ok, stored_if_ok = ent
    issuers = [RSA_ISSUER]
    batch = padded(Batch.from_certs(certs, [0] * len(certs), ets))
    eng = ctmr.Engine(device=0, table_slots=table, pair_slots=1 << 10)
    eng.add_issuers(issuers)
    eng.set_filter(b"", True, NOW)
    res = eng.map_batch(batch)
    o, st, unk, eh = run_oracle(batch, issuers, b"", True, NOW)
    assert_records_equal(res, batch, st, unk, eh)
    assert_state_equal(eng, o, len(issuers))
    status = res.records["status"].copy()
    x509 = np.asarray(ets) == 0
    bad = np.array([v is False for v in ok])
    assert ((status == orc.ST_PARSE_ERROR)[x509] == bad[x509]).all(), np.nonzero(((status == orc.ST_PARSE_ERROR) != bad) & x509)[0][:10]
    assert (status[x509 & ~bad] == orc.ST_PASS).all()
    assert eng.total_count() == stored_if_ok
    assert res.stats.n_new == stored_if_ok
    res2 = eng.map_batch(batch)
    o, st2, unk2, eh2 = run_oracle(batch, issuers, b"", True, NOW, engine=o)
    assert_records_equal(res2, batch, st2, unk2, eh2)
    assert_state_equal(eng, o, len(issuers))
    assert (res2.records["status"] == status).all()
    assert res2.stats.n_new == 0 and not (res2.records["flags"] & 2).any() and len(res2.new_idx) == 0
    assert eng.total_count() == stored_if_ok
    eng.close()
    return status


def test_every_case_as_a_leaf_through_both_resolve_kernels():
    """The whole corpus, one certificate per case, X509 and precertificate entries in turn, shuffled: P-256 and the other
    curves share their 1 024-entry blocks, so both instantiations of k_ec_resolve pick their own out of every block."""
    ent, cs = E.leaf_entries()
    assert 8000 <= len(cs) < 65536
    status = map_twice_against_the_oracle(ent)
    for curve in CURVES:
        sel = np.array([c.curve == curve for c in cs])
        assert int((status[sel] == orc.ST_PASS).sum()) >= 200 and int((status[sel] == orc.ST_PARSE_ERROR).sum()) >= 800, curve


def test_every_curve_at_every_pad_count_and_byte_phase():
    """The placement cases in payload order (their serial lengths put the key at the byte phase wanted): fe_load_bits'
    funnel shifts at every bit offset 0 … 31 modulo a dword, on every curve."""
    pl = E.placement_cases(start=0)
    certs = [q.der for q in pl]
    ets = [k & 1 for k in range(len(pl))]
    offsets = Batch.from_certs(certs, [0] * len(pl), ets).offsets
    seen = set()
    for k, q in enumerate(pl):
        assert (int(offsets[k]) + q.keypos) % 4 == q.phase
        seen.add((q.curve, q.pad, q.phase))
    assert len(seen) == 5 * 8 * 4
    stored = sum(1 for k, q in enumerate(pl) if q.ok and not (ets[k] == 1 and q.curve == "P192"))
    map_twice_against_the_oracle(E.Entries(certs, ets, [q.ok for q in pl], stored), table=1 << 12)


def test_the_cases_closest_to_the_edges_as_issuers():
    """The in-walk equation (fe_load + ec_on_curve inside k_issuer_ids): each case registered as a Chain[0] issuer with one
    RSA leaf of its own.  A refused key is ISSUER_PARSE_ERROR, an accepted one PASS — but for secp192r1, whose finding costs
    an issuer its place either way (there the oracle comparison holds the device to "finding", not "fatal")."""
    issuers, ent, cs = E.issuer_entries()
    batch = padded(Batch.from_certs(ent.certs, list(range(len(cs))), ent.ets))
    eng = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
    eng.add_issuers(issuers)
    eng.set_filter(b"", True, NOW)
    res = eng.map_batch(batch)
    o, st, unk, eh = run_oracle(batch, issuers, b"", True, NOW)
    assert_records_equal(res, batch, st, unk, eh)
    assert_state_equal(eng, o, len(issuers))
    for k, c in enumerate(cs):
        want = orc.ST_PASS if c.ok and c.curve != "P192" else orc.ST_ISSUER_PARSE_ERROR
        assert res.records["status"][k] == want, (k, c)
    assert eng.total_count() == sum(c.ok and c.curve != "P192" for c in cs)
    eng.close()


def test_the_cases_closest_to_the_edges_as_raw_precertificate_entries_with_strict_leaf():
    """The in-walk equation of the strict_leaf TBS check: a precertificate entry whose leaf TBSCertificate carries a key
    that does not parse is dropped as the downloader drops it (ENTRY_DECODE_ERROR) — exactly the refused cases."""
    pairs, cs = E.raw_precert_pairs()
    raw = RawEntries.from_pairs(pairs)
    raw.blob = np.concatenate([raw.blob, np.zeros(N.PAYLOAD_PAD, np.uint8)])
    eng = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
    eng.set_filter(b"", True, NOW)
    eng.set_strict_leaf(True)
    res = eng.map_entries(raw)
    o = orc.Engine(b"", True, NOW)
    o.set_strict_leaf(True)
    check_against_oracle(eng, raw, o, res)
    for k, c in enumerate(cs):
        assert res.records["status"][k] == E.raw_precert_status(c), (k, c)
    eng.close()


@pytest.mark.parametrize("first_block", ["p256_and_p384", "p384_only"])
def test_the_block_structure_of_the_resolve_kernels(first_block):
    """ec_corpus.block_entries: a block's pending list full between the two instantiations / in one, 257 pending entries
    in a block, the batch ending inside a group of four with a pending entry last, in-batch duplicates; mapped twice."""
    map_twice_against_the_oracle(E.block_entries(first_block), table=1 << 13)
