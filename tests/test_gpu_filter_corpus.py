"""-m gpu: the issuer CN filter (certIsFilteredOut filter 3) through the map kernels, at every piece length, Name shape and
window edge.

ctmr_set_filter cuts the filter into pieces, walk_name<CN> picks the CommonName, cn_prefix_match compares word by word
through whichever reader the kernel uses — and asks for no window of its own: a piece longer than walk_name's 32-octet hint
reads past what the window is known to hold.  WinReaderS (k_map_fused) must count that read as a miss so that the exact
reader decides; WinReaderC (k_map_winc) must serve it from global memory; a lane out of its wave's reach (a reversed view)
takes yet another path.  A read served from the wrong bytes without a miss is silent: the record says PASS or FILTERED_CN.
tests/filter_corpus.py builds the certificates, the settings and the MODEL (a plain startswith over the recorded effective
CN, and the if-chain of the statuses); tests/test_filter_corpus_cpu.py holds the builder to its claims and the oracle and
the host walk to the model.

Reference: the corpus's model for the status vector; the oracle engine — whose statuses are asserted equal to the model's
first — for the NEW list, exp_hour and the known sets.  Bit for bit, no tolerances.

Matrix: family x map_variant {15 (k_map_fused), 13 (k_map_winc + k_insert)} x profile {reference, fast}, ONE engine per
(variant, profile) for the whole module: the filter changes with set_filter from batch to batch (the known sets are dropped
in between: every batch starts from nothing, as its oracle engine does).  Every family runs through map_batch; `window` and
`address` also through map_view_device with the case's lead padding, ascending and reversed (reversed: lanes 1..63 of every
wave are out of the wave descriptor's reach).  `window`'s pairs are X509 and precertificate entries in turn: under the
reference profile the walk checks a Name's strings in the precertificate lanes only, so both forms of the walk meet the
long pieces at the window's end.  A setting ctmr_set_filter must refuse answers CTMR_E_INVAL and the batch
mapped afterwards follows the setting in force before."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import _native as N  # noqa: E402
from ct_mapreduce_amd.engine import CtmrError  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import filter_corpus as F  # noqa: E402
from tests import view_corpus as V  # noqa: E402
from tests.gpu_common import run_oracle, assert_records_equal, assert_state_equal  # noqa: E402
from tests.test_gpu_view_order import DevView, STRICT  # noqa: E402

VARIANTS = (15, 13)
PROFILES = ("reference", "fast")
N_ISSUERS = len(F.registered_issuers())

_ENGINES, _REFERENCES = {}, {}


@pytest.fixture(scope="module", autouse=True)
def close_engines_and_references():
    yield
    for e in _ENGINES.values():
        e.close()
    for o, *_ in _REFERENCES.values():
        o.close()
    _ENGINES.clear()
    _REFERENCES.clear()


def engine(variant, profile):
    """The one engine of (variant, profile): every family's settings go through its ctmr_set_filter in turn."""
    if (variant, profile) not in _ENGINES:
        e = ctmr.Engine(device=0, table_slots=1 << 15, pair_slots=1 << 12, map_variant=variant)
        e.set_profile(profile)
        e.add_issuers(F.registered_issuers())
        assert [e.issuer_info(k).valid for k in range(N_ISSUERS)] == [True] * F.N_GOOD_ISSUERS + [False]
        _ENGINES[variant, profile] = e
    return _ENGINES[variant, profile]


def reference(name, k, profile):
    """(oracle engine after the batch, the MODEL's status vector, unknown, exp_hour, batch) of case k: computed once, shared
    by the variants and placements, only read afterwards.  The oracle's statuses must be the model's.  The tests run family
    by family: the references of the family before are closed when the next one asks."""
    for key in [key for key in _REFERENCES if key[0] != name]:
        _REFERENCES.pop(key)[0].close()
    if (name, k, profile) not in _REFERENCES:
        fam = F.FAMILIES[name]()
        case, s = fam.in_force()[k]
        b = fam.batch(case)
        o = orc.Engine(s.filt, s.log_expired, s.now)
        o.set_profile(profile)
        # an entry the downloader dropped (CTMR_ENTRY_INVALID) never reaches insertCTWorker: the oracle maps the others
        keep = np.nonzero(b.entry_type != N.ENTRY_INVALID)[0]
        _, st_k, unk_k, eh_k = run_oracle(fam.batch(F.Case(s, [case.idx[int(i)] for i in keep])), F.registered_issuers(), engine=o)
        st, unk, eh = np.full(b.n, F.ST_ENTRY_DECODE_ERROR, np.uint8), np.zeros(b.n, np.uint8), np.zeros(b.n, np.int32)
        st[keep], unk[keep], eh[keep] = st_k, unk_k, eh_k
        for i in np.nonzero(b.entry_type == N.ENTRY_INVALID)[0]:      # (its record still reports the fields of a certificate that parsed)
            eh[i] = orc.exp_hour(orc.parse_cert(b.cert(int(i))).not_after)
        want = fam.expected(case, s)
        assert (st == want).all(), (name, k, profile, np.nonzero(st != want)[0][:10])
        _REFERENCES[name, k, profile] = (o, want, unk, eh, b)
    return _REFERENCES[name, k, profile]


def apply(eng, setting):
    if setting.refused:
        with pytest.raises(CtmrError) as err:
            eng.set_filter(setting.filt, setting.log_expired, setting.now)
        assert err.value.code == N.E_INVAL
    else:
        eng.set_filter(setting.filt, setting.log_expired, setting.now)
    eng.reset_known()


def run_family(name, variant, profile, placement):
    fam = F.FAMILIES[name]()
    eng = engine(variant, profile)
    seen = set()
    for k, (case, s) in enumerate(fam.in_force()):
        o, st, unk, eh, b = reference(name, k, profile)
        apply(eng, case.setting)
        if placement == "packed":
            res = eng.map_batch(b)
        else:
            blob, start, end = V.make_view(b, placement, fill=1000 + k, lead=case.lead)
            assert int(start.min()) == case.lead and (placement == "ascending" or V.lanes_below_lane0(start).sum() >= min(b.n, 64) - 1)
            res = DevView(b, blob, start, end).map(eng)
        assert_records_equal(res, b, st, unk, eh, **STRICT[profile])
        assert_state_equal(eng, o, N_ISSUERS)           # nothing filtered is in a set
        seen |= set(st.tolist())
    return seen


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(F.FAMILIES))
def test_the_filter_through_map_batch(name, variant, profile):
    seen = run_family(name, variant, profile, "packed")
    assert {F.ST_PASS, F.ST_FILTERED_CN} <= seen
    if name in ("order", "switch"):
        assert seen == set(range(8))


@pytest.mark.parametrize("order", ["ascending", "reversed"])
@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", [n for n in F.FAMILIES if F.FAMILIES[n]().views])
def test_the_filter_through_entry_views(name, variant, profile, order):
    assert run_family(name, variant, profile, order) == {F.ST_PASS, F.ST_FILTERED_CN}
