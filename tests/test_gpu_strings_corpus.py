"""-m gpu: the Names' string rules (strict_strings) in the map kernels, at every octet, length and window position.

der_walk.h value_strings_ok / string_word_ok / utf8_exact_ok run inside walk_name and walk_rdns for every precertificate
(kernels/map.h passes `strings` for entry type 1 only: the lanes of a wave diverge on it) and, through the exact
GlobalReader of k_issuer_ids, for every issuer that is registered.  tests/strings_corpus.py builds the inputs and states
the rules once more, independently; tests/test_strings_corpus_cpu.py holds the builder, the oracle and the host build of
the walk to them.  Here the ENGINE is compared

  with the ORACLE engine over each family, bit for bit and without tolerances — status, flags, serial, exp_hour,
  issuer_idx, the NEW list, by_status (assert_records_equal) and the known sets (assert_state_equal);
  with the verdict the corpus carries for every certificate: a precertificate entry whose Names hold a finding is a
  PARSE_ERROR, every other entry — every X509 copy among them — is a PASS.

Matrix: family x map_variant {0 (k_map_fused), 13 (k_map_winc + k_insert)} x switches x placement {packed through
map_batch_device with exactly CTMR_PAYLOAD_PAD octets behind the last certificate, ascending line view through
map_view_device: certificate k at residue 37·k mod 128} x order {as built, seeded shuffle}.  The switches:
  reference      set_profile("reference"): k_map_fused<WIN_CH_STRICT, …, true> / k_map_winc<WIN_CH_STRICT, true>, the
                 224-octet window that begins at the certificate, strict_extensions on
  fast_strings   set_profile("fast"), then set_strict_strings(True) alone.  engine/map.inc launches by
                 `strict = strict_strings || strict_ext`: the SAME instantiation and the same 224-octet window geometry as
                 the reference profile (the fast profile's 216-octet window that begins 8 octets in belongs to the
                 instantiation without the check, which this setting never launches); strict_extensions is off at run
                 time, so the extension bodies — and with them rel_name's nameRelativeToCRLIssuer — are not walked.
rel_name therefore runs under the reference profile only.  A second map of the same input finds nothing new.  One oracle
reference per (family, order, switches), shared by the variants and placements and only read afterwards.

Beyond the matrix: the fast profile with the switch OFF keeps every certificate of alphabet, lengths and utf8_edges (the
switch decides, nothing else in the corpus does); lengths and utf8_edges wrapped as RFC 6962 entries through map_entries
under the reference profile (strict_leaf: k_leaf_tbs_check walks the bare TBSCertificate of every precertificate entry);
the issuer table registered through add_issuers (issuer_info(k).valid against the corpus' verdict, one leaf under each)
and as Chain[0] of raw entries that the engine registers itself.  Nothing of the corpus was cut for time: the families
are as tests/strings_corpus.py describes them."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import _native as N  # noqa: E402
from ct_mapreduce_amd.engine import Batch, RawEntries  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import strings_corpus as S  # noqa: E402
from tests.gpu_common import run_oracle, assert_records_equal, assert_state_equal  # noqa: E402
from tests.test_entry_decode_cpu import x509_leaf, precert_leaf, chain, asn1cert  # noqa: E402
from tests.test_gpu_entries import check_against_oracle  # noqa: E402
from tests.test_gpu_geometry import Packed, placed  # noqa: E402
from tests.test_gpu_view_order import STRICT  # noqa: E402
from tests.test_walk_cpu import tbs_of  # noqa: E402

VARIANTS = (0, 13)
ORDERS = ("sorted", "shuffled")
PLACEMENTS = ("packed", "view")
SWITCHES = {"reference": STRICT["reference"], "fast_strings": dict(strict_strings=True, strict_spki=True, strict_ext=False),
            "fast": STRICT["fast"]}
FILTER_STATUSES = (orc.ST_PASS, orc.ST_FILTERED_CA, orc.ST_FILTERED_EXPIRED, orc.ST_FILTERED_CN)


def switch(e, switches):
    """The product's engine and the oracle's take the same calls."""
    e.set_profile("reference" if switches == "reference" else "fast")
    if switches == "fast_strings":
        e.set_strict_strings(True)


def engine(variant, switches, issuers=None, max_issuers=0):
    e = ctmr.Engine(device=0, table_slots=1 << 15, pair_slots=1 << 12, map_variant=variant, max_issuers=max_issuers)
    switch(e, switches)                                          # before the issuers: they are judged when registered
    if issuers is not None:
        assert e.add_issuers(issuers) == 0
    e.set_filter(S.FILT, False, S.NOW)
    return e


def oracle_engine(switches):
    o = orc.Engine(S.FILT, False, S.NOW)
    switch(o, switches)
    return o


@functools.lru_cache(maxsize=None)
def ordered(name, order):
    """(batch, expected findings per entry, entry types) of a family in the given order: built once per module."""
    fam = S.FAMILIES[name]()
    idx = list(range(len(fam.certs))) if order == "sorted" else S.shuffled(fam)
    return fam.batch(idx), np.array([fam.expect[i] for i in idx]), np.array([fam.certs[i][2] for i in idx])


def wanted_status(expect, et, switches):
    """What the corpus' own rules say: a precertificate entry with a finding loses its place; everything else is kept."""
    drops = (expect != 0) & (et == 1) if SWITCHES[switches]["strict_strings"] else np.zeros(len(et), bool)
    return np.where(drops, orc.ST_PARSE_ERROR, orc.ST_PASS).astype(np.uint8)


_REFERENCES = {}


@pytest.fixture(scope="module", autouse=True)
def close_the_references():
    yield
    for o, *_ in _REFERENCES.values():
        o.close()
    _REFERENCES.clear()


def reference(name, order, switches):
    """(oracle engine after the family, status, unknown, exp_hour): computed once per (family, order, switches)."""
    key = (name, order, switches)
    if key not in _REFERENCES:
        o = oracle_engine(switches)
        _, st, unk, eh = run_oracle(ordered(name, order)[0], S.registered_issuers(), engine=o)
        _REFERENCES[key] = (o, st, unk, eh)
    return _REFERENCES[key]


def run_family(name, variant, switches, placement, order):
    b, expect, et = ordered(name, order)
    o, st, unk, eh = reference(name, order, switches)
    want = wanted_status(expect, et, switches)
    assert (st == want).all(), np.nonzero(st != want)[0][:10]    # (the oracle against the corpus: asserted on the CPU too)
    eng = engine(variant, switches, S.registered_issuers())
    dev = placed(b, placement)
    res = dev.map(eng)
    assert (res.records["status"] == want).all(), np.nonzero(res.records["status"] != want)[0][:10]
    assert_records_equal(res, b, st, unk, eh, **SWITCHES[switches])
    counts = eng.issuer_counts().copy()
    again = dev.map(eng)                                         # the same input once more: everything is known
    assert again.stats.n_new == 0 and len(again.new_idx) == 0
    assert (again.records["status"] == st).all() and ((again.records["flags"] & 2) == 0).all()
    assert (eng.issuer_counts() == counts).all()
    assert_state_equal(eng, o, S.N_ISSUERS)
    eng.close()
    return want


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("switches", ["reference", "fast_strings"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", [n for n in S.FAMILIES if n != "rel_name"])
def test_every_string_rule_at_every_octet_length_and_position(name, variant, switches, placement, order):
    want = run_family(name, variant, switches, placement, order)
    assert (want == orc.ST_PARSE_ERROR).sum() > 500 and (want == orc.ST_PASS).sum() > len(want) // 2


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_relative_names_of_distribution_points_under_the_reference_profile(variant, placement, order):
    want = run_family("rel_name", variant, "reference", placement, order)
    assert (want == orc.ST_PARSE_ERROR).sum() > 500


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["alphabet", "lengths", "utf8_edges"])
def test_without_the_switch_every_certificate_is_kept(name, variant):
    want = run_family(name, variant, "fast", "packed", "sorted")
    assert (want == orc.ST_PASS).all() and np.isin(reference(name, "sorted", "fast")[1], FILTER_STATUSES).all()


@functools.lru_cache(maxsize=None)
def raw_entries(name):
    """The family as RFC 6962 entries: the X509 copies as X509 entries, the precertificate copies as precertificate entries
    whose leaf TBSCertificate is the certificate's own; Chain[0] = the registered issuer."""
    fam, iss = S.FAMILIES[name](), S.registered_issuers()
    pairs = []
    for k, (der, issuer_idx, et) in enumerate(fam.certs):
        if et == 0:
            pairs.append((x509_leaf(der, ts=1000 + k), chain([iss[issuer_idx]])))
        else:
            pairs.append((precert_leaf(tbs_of(der), ts=1000 + k), asn1cert(der) + chain([iss[issuer_idx]])))
    raw = RawEntries.from_pairs(pairs)
    raw.blob = np.concatenate([raw.blob, np.zeros(N.PAYLOAD_PAD, np.uint8)])
    return raw


def raw_engine(variant, max_issuers=0):
    eng = ctmr.Engine(device=0, table_slots=1 << 15, pair_slots=1 << 14, map_variant=variant, max_issuers=max_issuers)
    eng.set_profile("reference")
    eng.set_filter(S.FILT, False, S.NOW)
    return eng


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["lengths", "utf8_edges"])
def test_the_raw_path_with_strict_leaf_over_the_same_values(name, variant):
    raw, fam = raw_entries(name), S.FAMILIES[name]()
    eng = raw_engine(variant)
    res = eng.map_entries(raw)
    o = oracle_engine("reference")
    st, unk = check_against_oracle(eng, raw, o, res)
    want = wanted_status(np.array(fam.expect), np.array([c[2] for c in fam.certs]), "reference")
    assert (st == want).all() and (res.records["status"] == want).all()
    assert res.decode.n_precert == res.decode.n_x509 == raw.n // 2 and eng.issuer_count() == S.N_ISSUERS
    o.close()
    eng.close()


def leaves_batch(t):
    return Batch.from_certs([leaf for leaf, _ in t.leaves], list(range(len(t.cas))), [et for _, et in t.leaves])


@pytest.mark.parametrize("switches", ["reference", "fast_strings", "fast"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_issuers_register_as_valid_exactly_when_their_names_keep_to_the_rules(variant, switches):
    t = S.issuers()
    n = len(t.cas)
    valid = np.array(t.valid) if SWITCHES[switches]["strict_strings"] else np.ones(n, bool)
    eng = engine(variant, switches, t.cas, max_issuers=4096)    # k_issuer_ids: the exact GlobalReader
    assert eng.issuer_count() == n
    got = np.array([bool(eng.issuer_info(k).valid) for k in range(n)])
    assert (got == valid).all(), np.nonzero(got != valid)[0][:10]
    b = leaves_batch(t)
    o = oracle_engine(switches)
    _, st, unk, eh = run_oracle(b, t.cas, engine=o)
    want = np.where(valid, orc.ST_PASS, orc.ST_ISSUER_PARSE_ERROR).astype(np.uint8)
    assert (st == want).all()
    dev = Packed(b)
    res = dev.map(eng)
    assert (res.records["status"] == want).all(), np.nonzero(res.records["status"] != want)[0][:10]
    assert_records_equal(res, b, st, unk, eh, **SWITCHES[switches])
    again = dev.map(eng)
    assert again.stats.n_new == 0 and (again.records["status"] == st).all()
    assert_state_equal(eng, o, n)
    o.close()
    eng.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_issuer_table_as_chain0_of_raw_entries(variant):
    """Auto-registration: the engine meets each CA as Chain[0] of one entry and judges it there."""
    t = S.issuers()
    pairs = []
    for k, (leaf, et) in enumerate(t.leaves):
        if et == 0:
            pairs.append((x509_leaf(leaf, ts=5000 + k), chain([t.cas[k]])))
        else:
            pairs.append((precert_leaf(tbs_of(leaf), ts=5000 + k), asn1cert(leaf) + chain([t.cas[k]])))
    raw = RawEntries.from_pairs(pairs)
    raw.blob = np.concatenate([raw.blob, np.zeros(N.PAYLOAD_PAD, np.uint8)])
    eng = raw_engine(variant, max_issuers=4096)
    res = eng.map_entries(raw)
    o = oracle_engine("reference")
    st, unk = check_against_oracle(eng, raw, o, res)
    want = np.where(np.array(t.valid), orc.ST_PASS, orc.ST_ISSUER_PARSE_ERROR).astype(np.uint8)
    assert (st == want).all() and (res.records["status"] == want).all()
    assert eng.issuer_count() == res.decode.n_issuers_added == len(t.cas)
    assert sum(bool(eng.issuer_info(k).valid) for k in range(len(t.cas))) == sum(t.valid)
    o.close()
    eng.close()
