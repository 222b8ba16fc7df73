"""-m gpu: the extension-body rules (strict_extensions) in the map kernels, at every window position.

der_walk.h ext_body_check, ext_san_check / ext_san_coop, san_uri_ok, crl_dps with rel_name, ext_nc_check, ext_sct_ok,
ext_ipaddr_ok and ext_asnum_ok are pinned rule by rule on the host build (tests/test_ext_cpu.py).  On the device they run
behind kernels/readers.h WinReaderS — a 224-octet LDS window whose reads outside are clamped and only remembered in `miss`,
defer_exact() as the only way to the content parsers (a URI, nameConstraints, the RFC 3779 extensions, the SCT list, a
nameRelativeToCRLIssuer), the wave-collective walk of the subjectAltName — and through the exact GlobalReader of the
repeats, of k_leaf_tbs_check and of k_issuer_ids.  tests/ext_corpus.py builds the inputs and states each certificate's
verdict from the rule tables; tests/test_ext_corpus_cpu.py holds the builder, the oracle and the host build to them and
shows that the simulated window misses, defers and refills cooperatively over each family.  Here the ENGINE is compared

  with the ORACLE engine over each family, bit for bit and without tolerances — status, flags, serial, exp_hour,
  issuer_idx, the NEW list, by_status (assert_records_equal) and the known sets (assert_state_equal);
  with the status the corpus states for every certificate: fatal — PARSE_ERROR; a finding — PARSE_ERROR for a
  precertificate entry, PASS for an X509 entry; clean — PASS.

Matrix: family x map_variant {0 (k_map_fused), 13 (k_map_winc + k_insert)} x switches x placement {packed through
map_batch_device with exactly CTMR_PAYLOAD_PAD octets behind the last certificate, ascending line view through
map_view_device: certificate k at residue 37·k mod 128} x order {as built, seeded shuffle}.  The switches:
  reference   set_profile("reference"): strict_strings and strict_extensions
  fast_ext    set_profile("fast"), then set_strict_extensions(True) alone: the same instantiation (engine/map.inc launches by
              `strict = strict_strings || strict_ext`), strict_strings off at run time — a string finding inside a
              nameRelativeToCRLIssuer costs nothing
`slide` (20 000 certificates) runs in four parts of five kinds each — nothing of it is left out; a part is a batch of its
own with an oracle reference of its own.  A second map of the same input finds nothing new.  One oracle reference per
(family part, order, switches), shared by the variants and placements and only read afterwards.

Beyond the matrix: the fast profile with the switch OFF keeps every certificate of `rules`; `slide` and `san_elements`
wrapped as RFC 6962 entries through map_entries under the reference profile (strict_leaf: k_leaf_tbs_check walks the bare
TBSCertificate of a precertificate entry and drops the ENTRY over a fatal body alone; the certificate in extra_data then
loses its place over a finding); the issuer table registered through add_issuers (issuer_info(k).valid against the corpus'
verdict, one leaf under each) and as Chain[0] of raw entries that the engine registers itself."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import _native as N  # noqa: E402
from ct_mapreduce_amd.engine import Batch, RawEntries  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import ext_corpus as E  # noqa: E402
from tests.gpu_common import run_oracle, assert_records_equal, assert_state_equal  # noqa: E402
from tests.test_entry_decode_cpu import x509_leaf, precert_leaf, chain, asn1cert  # noqa: E402
from tests.test_gpu_entries import check_against_oracle  # noqa: E402
from tests.test_gpu_geometry import Packed, placed  # noqa: E402
from tests.test_gpu_view_order import STRICT  # noqa: E402
from tests.test_walk_cpu import tbs_of  # noqa: E402

VARIANTS = (0, 13)
ORDERS = ("sorted", "shuffled")
PLACEMENTS = ("packed", "view")
SWITCHES = {"reference": STRICT["reference"], "fast_ext": dict(strict_strings=False, strict_spki=True, strict_ext=True),
            "fast": STRICT["fast"]}
PARTS = {"rules": 1, "slide": 4, "san_elements": 1}
FAMILY_PARTS = [(name, part) for name, n in PARTS.items() for part in range(n)]


def switch(e, switches):
    """The product's engine and the oracle's take the same calls."""
    e.set_profile("reference" if switches == "reference" else "fast")
    if switches == "fast_ext":
        e.set_strict_extensions(True)


def engine(variant, switches, issuers=None, max_issuers=0):
    e = ctmr.Engine(device=0, table_slots=1 << 15, pair_slots=1 << 12, map_variant=variant, max_issuers=max_issuers)
    switch(e, switches)                                          # before the issuers: they are judged when registered
    if issuers is not None:
        assert e.add_issuers(issuers) == 0
    e.set_filter(E.FILT, False, E.NOW)
    return e


def oracle_engine(switches):
    o = orc.Engine(E.FILT, False, E.NOW)
    switch(o, switches)
    return o


def part_of(name, part):
    """The certificates of a family's part: slide's kinds lie one behind the other, a part is five of them."""
    n = len(E.FAMILIES[name]().certs)
    cut = [n * k // PARTS[name] // 4 * 4 for k in range(PARTS[name])] + [n]
    return list(range(cut[part], cut[part + 1]))


@functools.lru_cache(maxsize=None)
def ordered(name, part, order):
    """(batch, indices into the family) of a family's part in the given order: built once per module."""
    fam = E.FAMILIES[name]()
    idx = part_of(name, part)
    if order == "shuffled":
        idx = [idx[i] for i in np.random.default_rng([20261021, E.IDS[name], part]).permutation(len(idx))]
    return fam.batch(idx), np.array(idx)


_REFERENCES = {}


@pytest.fixture(scope="module", autouse=True)
def close_the_references():
    yield
    for o, *_ in _REFERENCES.values():
        o.close()
    _REFERENCES.clear()


def reference(name, part, order, switches):
    """(oracle engine after the part, status, unknown, exp_hour): computed once per (family part, order, switches)."""
    key = (name, part, order, switches)
    if key not in _REFERENCES:
        o = oracle_engine(switches)
        _, st, unk, eh = run_oracle(ordered(name, part, order)[0], E.registered_issuers(), engine=o)
        _REFERENCES[key] = (o, st, unk, eh)
    return _REFERENCES[key]


def run_family(name, part, variant, switches, placement, order):
    b, idx = ordered(name, part, order)
    o, st, unk, eh = reference(name, part, order, switches)
    kw = SWITCHES[switches]
    want = E.FAMILIES[name]().expect(kw["strict_ext"], kw["strict_strings"])[idx]
    assert b.n % 64 != 0 and (st == want).all(), np.nonzero(st != want)[0][:10]      # (the oracle against the corpus: asserted on the CPU too)
    eng = engine(variant, switches, E.registered_issuers())
    dev = placed(b, placement)
    res = dev.map(eng)
    assert (res.records["status"] == want).all(), [(int(idx[i]), E.FAMILIES[name]().marks[idx[i]]) for i in np.nonzero(res.records["status"] != want)[0][:6]]
    assert_records_equal(res, b, st, unk, eh, **kw)
    counts = eng.issuer_counts().copy()
    again = dev.map(eng)                                         # the same input once more: everything is known
    assert again.stats.n_new == 0 and len(again.new_idx) == 0
    assert (again.records["status"] == st).all() and ((again.records["flags"] & 2) == 0).all()
    assert (eng.issuer_counts() == counts).all()
    assert_state_equal(eng, o, E.N_ISSUERS)
    eng.close()
    return want


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("switches", ["reference", "fast_ext"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name, part", FAMILY_PARTS)
def test_every_extension_rule_at_every_window_position(name, part, variant, switches, placement, order):
    want = run_family(name, part, variant, switches, placement, order)
    assert (want == orc.ST_PARSE_ERROR).sum() > 100 and (want == orc.ST_PASS).sum() > len(want) // 3


@pytest.mark.parametrize("variant", VARIANTS)
def test_without_the_switch_every_certificate_is_kept(variant):
    """The switch decides, nothing else in the corpus does."""
    want = run_family("rules", 0, variant, "fast", "packed", "sorted")
    assert (want == orc.ST_PASS).all() and (reference("rules", 0, "sorted", "fast")[1] == orc.ST_PASS).all()


@functools.lru_cache(maxsize=None)
def raw_entries(name, part):
    """A family's part as RFC 6962 entries: the X509 copies as X509 entries, the precertificate copies as precertificate
    entries whose leaf TBSCertificate is the certificate's own and whose extra_data carries the certificate; Chain[0] = the
    registered issuer."""
    fam, iss = E.FAMILIES[name](), E.registered_issuers()
    pairs = []
    for k in part_of(name, part):
        der, issuer_idx, et = fam.certs[k]
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
    eng.set_filter(E.FILT, False, E.NOW)
    return eng


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name, part", [fp for fp in FAMILY_PARTS if fp[0] != "rules"])
def test_the_raw_path_with_strict_leaf_over_the_same_bodies(name, part, variant):
    raw, fam, idx = raw_entries(name, part), E.FAMILIES[name](), part_of(name, part)
    eng = raw_engine(variant)
    res = eng.map_entries(raw)
    o = oracle_engine("reference")
    st, unk = check_against_oracle(eng, raw, o, res)
    # k_leaf_tbs_check: a fatal body in the leaf TBSCertificate of a precertificate entry fails the ENTRY; a finding does not
    want = fam.expect()[idx]
    fatal_precert = np.array([fam.verdict[k] == E.FATAL and fam.certs[k][2] == 1 for k in idx])
    want = np.where(fatal_precert, orc.ST_ENTRY_DECODE_ERROR, want).astype(np.uint8)
    assert (st == want).all() and (res.records["status"] == want).all(), np.nonzero(res.records["status"] != want)[0][:10]
    assert res.decode.n_x509 == raw.n // 2 and res.decode.n_precert + res.decode.n_decode_error == raw.n // 2
    assert res.decode.n_decode_error == int(fatal_precert.sum()) > 50 and eng.issuer_count() == E.N_ISSUERS
    o.close()
    eng.close()


def leaves_batch(t):
    return Batch.from_certs([leaf for leaf, _ in t.leaves], list(range(len(t.cas))), [et for _, et in t.leaves])


@pytest.mark.parametrize("switches", ["reference", "fast_ext", "fast"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_issuers_register_as_valid_exactly_when_their_extensions_keep_to_the_rules(variant, switches):
    """k_issuer_ids walks every registered certificate with the exact reader; ANY finding drops the issuer."""
    t = E.chain0()
    n = len(t.cas)
    kw = SWITCHES[switches]
    valid = np.array([not kw["strict_ext"] or v == E.CLEAN or (v == E.STRING_FINDING and not kw["strict_strings"]) for v in t.verdict])
    eng = engine(variant, switches, t.cas, max_issuers=4096)
    assert eng.issuer_count() == n
    got = np.array([bool(eng.issuer_info(k).valid) for k in range(n)])
    assert (got == valid).all(), [(int(k), t.marks[k]) for k in np.nonzero(got != valid)[0][:10]]
    b = leaves_batch(t)
    o = oracle_engine(switches)
    _, st, unk, eh = run_oracle(b, t.cas, engine=o)
    want = np.where(valid, orc.ST_PASS, orc.ST_ISSUER_PARSE_ERROR).astype(np.uint8)
    assert (st == want).all(), np.nonzero(st != want)[0][:10]
    dev = Packed(b)
    res = dev.map(eng)
    assert (res.records["status"] == want).all(), np.nonzero(res.records["status"] != want)[0][:10]
    assert_records_equal(res, b, st, unk, eh, **kw)
    again = dev.map(eng)
    assert again.stats.n_new == 0 and (again.records["status"] == st).all()
    assert_state_equal(eng, o, n)
    assert valid.sum() >= 400 and (switches == "fast" or (~valid).sum() >= 400)
    o.close()
    eng.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_issuer_table_as_chain0_of_raw_entries(variant):
    """Auto-registration: the engine meets each CA as Chain[0] of one entry and judges it there."""
    t = E.chain0()
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
