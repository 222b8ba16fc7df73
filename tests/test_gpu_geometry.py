"""-m gpu: the map kernels (k_map_fused, k_map_winc + k_insert, k_leaf_tbs_check on the raw path) with every verdict-bearing
field at every position of their windows.

Everything the kernels read of a certificate comes through kernels/readers.h: a per-lane LDS window filled sixteen lanes per
certificate, moved by the walk's hints, two register prefetches (the 32 octets behind the TBSCertificate, the 16 around the
key's end) and the subjectAltName's rounds.  A read served wrongly without raising `miss` is silent — the record still has a
serial, an hour and a verdict, of the wrong bytes.  tests/geometry_corpus.py builds twins for every such geometry (equal
but for a few octets at the position under test, different in the oracle's record); tests/test_geometry_corpus_cpu.py holds
the builder to its coverage and to the window path being what decides.

Reference: the ORACLE engine over each family in entry order (status, flags, serial, exp_hour, issuer_idx, the NEW list,
by_status, the known sets) — bit for bit, no tolerances.

Matrix: family x map_variant {0 (k_map_fused), 13 (k_map_winc + k_insert)} x profile {reference, fast} x placement {packed
through map_batch_device with exactly CTMR_PAYLOAD_PAD octets behind the last certificate, ascending line view through
map_view_device: certificate k at residue 37·k mod 128} x order {as built: neighbouring lanes nearly equal, seeded shuffle:
cooperative refills serve some lanes and leave the others}.  A second map of the same input finds nothing new.  The
sequence families (tail_last, waves) are small payloads mapped one after the other through ONE engine.  Beyond the matrix:
first sightings (collect_meta) over front and ext_crl, whose memo pre-check reads the issuer Name and the distribution point
out of the same windows; front, subject and san wrapped as RFC 6962 entries through map_entries under the reference profile
(strict_leaf: k_leaf_tbs_check walks the bare TBSCertificate, with no tail behind it, over the same sweep)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import _native as N  # noqa: E402
from ct_mapreduce_amd.engine import BatchResult, RawEntries, RECORD_DTYPE  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import geometry_corpus as G  # noqa: E402
from tests.gpu_common import run_oracle, assert_records_equal, assert_state_equal  # noqa: E402
from tests.test_entry_decode_cpu import x509_leaf, precert_leaf, chain, asn1cert  # noqa: E402
from tests.test_gpu_entries import check_against_oracle  # noqa: E402
from tests.test_gpu_meta import expected_first_sightings  # noqa: E402
from tests.test_gpu_view_order import DevView, STRICT, first_sightings, up  # noqa: E402
from tests.test_walk_cpu import tbs_of  # noqa: E402

DEV = torch.device("cuda:0")
VARIANTS = (0, 13)
PROFILES = ("reference", "fast")
ORDERS = ("sorted", "shuffled")
PLACEMENTS = ("packed", "view")


def engine(variant, profile, meta=False):
    e = ctmr.Engine(device=0, table_slots=1 << 15, pair_slots=1 << 12, map_variant=variant, collect_meta=meta)
    e.set_profile(profile)
    e.add_issuers(G.registered_issuers())
    e.set_filter(G.FILT, False, G.NOW)
    return e


@functools.lru_cache(maxsize=None)
def slices(name, order):
    """The family's payloads in the given order (one, or the sequence families' many): built once per module."""
    fam = G.FAMILIES[name]()
    idx = list(range(len(fam.certs))) if order == "sorted" else G.shuffled(fam)
    cuts = fam.cuts or [0, len(idx)]
    return [fam.batch(idx[lo:hi]) for lo, hi in zip(cuts, cuts[1:])]


_REFERENCES = {}


@pytest.fixture(scope="module", autouse=True)
def close_the_references():
    yield
    for o, _ in _REFERENCES.values():
        o.close()
    _REFERENCES.clear()


def reference(name, order, profile):
    """(oracle engine after all payloads, [(status, unknown, exp_hour) per payload]): computed once, shared by the variants
    and placements, and only read afterwards."""
    if (name, order, profile) not in _REFERENCES:
        _REFERENCES[name, order, profile] = make_reference(name, order, profile)
    return _REFERENCES[name, order, profile]


def make_reference(name, order, profile):
    o = orc.Engine(G.FILT, False, G.NOW)
    o.set_profile(profile)
    out = []
    for b in slices(name, order):
        _, st, unk, eh = run_oracle(b, G.registered_issuers(), engine=o)
        out.append((st, unk, eh))
    return o, out


class Packed:
    """A packed batch on the device with EXACTLY CTMR_PAYLOAD_PAD octets (non-zero noise) behind its last certificate."""

    def __init__(self, b):
        self.n = b.n
        pad = np.random.default_rng(b.n).integers(1, 256, size=N.PAYLOAD_PAD, dtype=np.uint8)
        self.pay = up(np.concatenate([b.payload, pad]))
        self.off, self.iss, self.et = up(b.offsets, np.int64), up(b.issuer_idx, np.int32), up(b.entry_type, np.uint8)
        self.rec = torch.zeros(b.n * 32, dtype=torch.uint8, device=DEV)
        self.new = torch.zeros(b.n, dtype=torch.int64, device=DEV)

    def map(self, eng):
        st = eng.map_batch_device(self.pay.data_ptr(), self.off.data_ptr(), self.iss.data_ptr(), self.et.data_ptr(), self.n,
                                  self.rec.data_ptr(), self.new.data_ptr())
        return BatchResult(self.rec.cpu().numpy().view(RECORD_DTYPE).copy(), self.new[:st.n_new].cpu().numpy().astype(np.uint64), st)


def placed(b, placement):
    if placement == "packed":
        return Packed(b)
    blob, start, end = G.line_view(b, fill=b.n)
    assert int(end[-1]) == len(blob) - N.PAYLOAD_PAD            # the last certificate ends the blob: the pad alone lies behind it
    return DevView(b, blob, start, end)


def run_family(name, variant, profile, placement, order, meta=False):
    o, ref = reference(name, order, profile)
    eng = engine(variant, profile, meta)
    canon = None
    for b, (st, unk, eh) in zip(slices(name, order), ref):
        dev = placed(b, placement)
        res = dev.map(eng)
        assert_records_equal(res, b, st, unk, eh, **STRICT[profile])
        if meta:
            certs = [b.cert(i) for i in range(b.n)]
            canon = canon or [eng.issuer_info(k).canonical_idx for k in range(G.N_ISSUERS)]
            want = expected_first_sightings(certs, [canon[int(k)] for k in b.issuer_idx], [int(i) for i in res.new_idx], res.records["exp_hour"])
            got = set()
            items = first_sightings(eng, dev, res)
            for it in items:
                c, der = canon[int(it["issuer_idx"])], certs[int(it["entry"])]
                if it["kind"] == N.MK_HOST:
                    got.add((N.MK_HOST, int(it["entry"])))
                elif it["kind"] == N.MK_EXPDATE:
                    got.add((N.MK_EXPDATE, c, int(it["exp_hour"]), b""))
                else:
                    got.add((int(it["kind"]), c, 0, der[int(it["off"]):int(it["off"]) + int(it["len"])]))
            assert len(items) == len(got) and got == want
            assert {k[0] for k in want} >= {N.MK_EXPDATE, N.MK_DN}
        counts = eng.issuer_counts().copy()
        again = dev.map(eng)                                     # the same input once more: everything is known
        assert again.stats.n_new == 0 and len(again.new_idx) == 0
        assert (again.records["status"] == st).all() and ((again.records["flags"] & 2) == 0).all()
        assert (eng.issuer_counts() == counts).all()
    assert_state_equal(eng, o, G.N_ISSUERS)
    eng.close()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(G.FAMILIES))
def test_every_field_at_every_window_position(name, variant, profile, placement, order):
    run_family(name, variant, profile, placement, order)


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["front", "ext_crl"])
def test_first_sightings_out_of_the_same_windows(name, variant, profile):
    run_family(name, variant, profile, "view", "sorted", meta=True)
    if name == "ext_crl":
        run_family(name, variant, profile, "view", "shuffled", meta=True)


@functools.lru_cache(maxsize=None)
def raw_entries(name):
    """The family as RFC 6962 entries, pair by pair X509 entries and precertificate entries whose leaf TBSCertificate is the
    certificate's own; Chain[0] = the registered issuer."""
    fam, iss = G.FAMILIES[name](), G.registered_issuers()
    pairs = []
    for k, (der, issuer_idx, _) in enumerate(fam.certs):
        if k // 2 % 2 == 0:
            pairs.append((x509_leaf(der, ts=1000 + k), chain([iss[issuer_idx]])))
        else:
            pairs.append((precert_leaf(tbs_of(der), ts=1000 + k), asn1cert(der) + chain([iss[issuer_idx]])))
    raw = RawEntries.from_pairs(pairs)
    raw.blob = np.concatenate([raw.blob, np.zeros(N.PAYLOAD_PAD, np.uint8)])
    return raw


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["front", "subject", "san"])
def test_the_raw_path_walks_the_leaf_tbs_over_the_same_sweep(name, variant):
    raw = raw_entries(name)
    eng = ctmr.Engine(device=0, table_slots=1 << 15, pair_slots=1 << 14, map_variant=variant)
    eng.set_profile("reference")
    eng.set_filter(G.FILT, False, G.NOW)
    res = eng.map_entries(raw)
    o = orc.Engine(G.FILT, False, G.NOW)
    o.set_profile("reference")
    st, unk = check_against_oracle(eng, raw, o, res)
    assert res.decode.n_precert > raw.n // 4 and res.decode.n_x509 > raw.n // 4
    assert (st == orc.ST_PASS).sum() > raw.n // 4
    assert name == "san" or (st == orc.ST_ENTRY_DECODE_ERROR).sum() > 40                             # strict_leaf drops leaves
    assert eng.issuer_count() == G.N_ISSUERS
    eng.close()
