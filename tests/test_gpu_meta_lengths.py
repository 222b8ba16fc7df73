"""-m gpu: the IssuerMetadata memo (kernels/meta.h k_meta_new, the map kernel's pre-check in kernels/meta_core.h,
engine/meta.inc) at every item length, address and path — the corpora of tests/meta_corpus.py through the C ABI.  What a
call must report is always the reference's memo semantics over the oracle's field extraction
(meta_corpus.expected_first_sightings); the comparisons are sets of byte strings, exact.

The memo keeps two items apart, and makes two sightings of one item equal, by a byte mask on the item's last 16-byte chunk
alone: every corpus shows an item twice with other bytes behind it (A, again) and once with another last byte (prime)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401

import ct_mapreduce_amd as ctmr
from ct_mapreduce_amd import _native as N
from ct_mapreduce_amd.engine import Batch
from tests import meta_corpus as MC

CORPORA = ("name_lengths", "uri_lengths", "addresses")
ITEM_DTYPE = np.dtype([("entry", "<u8"), ("kind", "<u4"), ("issuer_idx", "<u4"), ("exp_hour", "<i4"), ("off", "<u4"),
                       ("len", "<u4"), ("pad", "<u4")])


@functools.lru_cache(maxsize=None)
def corpus(which):
    return getattr(MC, which)()


def engine(c, profile, table_slots=1 << 14):
    eng = ctmr.Engine(device=0, table_slots=table_slots, pair_slots=1 << 12, collect_meta=True)
    eng.set_profile(profile)
    eng.add_issuers(c.issuers)
    eng.set_filter(b"", True, 0)
    return eng


class Memo:
    """An engine and what its memo has reported so far; run() maps a batch and compares its first sightings."""

    def __init__(self, c, profile, table_slots=1 << 14):
        self.eng = engine(c, profile, table_slots)
        self.seen = set()

    def check(self, ders, idx, new_idx, hours, items, cold=False):
        exp = MC.expected_first_sightings(ders, [int(k) for k in idx], [int(i) for i in new_idx], hours)
        if not cold:
            exp -= self.seen
        got = MC.got_first_sightings(self.eng, items)
        assert len(items) == len(got)                                # nothing reported twice
        assert got == exp, (sorted(got - exp)[:3], sorted(exp - got)[:3])
        if cold:
            self.seen = set()
        self.seen.update(k for k in exp if k[0] != N.MK_HOST)        # a host-routed certificate is handed over every time
        return exp

    def run(self, ders, idx, cold=False):
        res = self.eng.map_batch(Batch.from_certs(ders, idx))
        assert (res.records["status"] == N.ST_PASS).all() and res.stats.n_new == len(ders)
        return self.check(ders, idx, res.new_idx, res.records["exp_hour"], self.eng.meta_new(), cold)


class DeviceBatch:
    """A batch in device memory for ctmr_map_batch_device / ctmr_meta_new_device, and the item buffer of the test's own."""

    def __init__(self, ders, idx, items_cap):
        dev = torch.device("cuda:0")
        b = Batch.from_certs(ders, idx)
        self.n, self.ders, self.idx, self.items_cap = b.n, ders, idx, items_cap
        self.payload = np.concatenate([b.payload, np.zeros(N.PAYLOAD_PAD, np.uint8)])
        self.offsets = b.offsets
        self.d_pay = torch.from_numpy(self.payload).to(dev)
        self.d_off = torch.from_numpy(b.offsets.astype(np.int64)).to(dev)
        self.d_iss = torch.from_numpy(b.issuer_idx.astype(np.int32)).to(dev)
        self.d_et = torch.zeros(b.n, dtype=torch.uint8, device=dev)
        self.d_rec = torch.zeros(b.n * 32, dtype=torch.uint8, device=dev)
        self.d_new = torch.zeros(b.n, dtype=torch.int64, device=dev)
        self.d_items = torch.zeros(items_cap * 32, dtype=torch.uint8, device=dev)

    def map(self, eng):
        st = eng.map_batch_device(self.d_pay.data_ptr(), self.d_off.data_ptr(), self.d_iss.data_ptr(), self.d_et.data_ptr(),
                                  self.n, self.d_rec.data_ptr(), self.d_new.data_ptr())
        assert st.n_new == self.n and st.by_status[N.ST_PASS] == self.n
        self.n_new = st.n_new
        return st

    def meta(self, eng):
        """→ (new_idx, exp_hour per entry, items as Engine.meta_new gives them)."""
        got = eng.meta_new_device(self.d_pay.data_ptr(), self.d_off.data_ptr(), 0, self.d_rec.data_ptr(), self.d_new.data_ptr(),
                                  self.n_new, self.d_items.data_ptr(), self.items_cap)
        assert got <= self.items_cap
        items = np.frombuffer(self.d_items[:got * 32].cpu().numpy().tobytes(), ITEM_DTYPE)
        rec = np.frombuffer(self.d_rec.cpu().numpy().tobytes(), ctmr.engine.RECORD_DTYPE)
        raw, offs, out = self.payload.tobytes(), self.offsets, []
        for it in items.tolist():
            entry, kind, iss, hour, off, ln, _ = it
            at = int(offs[entry]) + off
            out.append((kind, entry, iss, hour, raw[at:at + ln] if kind in (N.MK_CRL, N.MK_DN) else b""))
        return self.d_new[:self.n_new].cpu().numpy(), rec["exp_hour"], out


@pytest.mark.parametrize("profile", ["reference", "fast"])
@pytest.mark.parametrize("which", CORPORA)
def test_cold_memo_one_batch(which, profile):
    """The whole corpus as ONE batch: A and again meet inside one launch, often inside one wave — the claim of a slot, the
    poll for its publication and the comparison with bytes another lane is writing.  A is reported once, prime once."""
    c = corpus(which)
    ders, idx, rows = c.part()
    m = Memo(c, profile)
    exp = m.run(ders, idx)
    items = {k[3] for k in exp if k[0] in (N.MK_CRL, N.MK_DN)}
    if which == "name_lengths":
        assert {len(b) for b in items} >= {n for n in range(15, 161) if n not in c.unreachable} | set(range(4090, 4097))
        assert sum(k[0] == N.MK_HOST for k in exp) == 3 * 4         # 4097..4100: three certificates each
    if which == "uri_lengths":
        assert {len(k[3]) for k in exp if k[0] == N.MK_CRL} >= set(range(0, 161)) | set(range(4090, 4097))
        assert sum(k[0] == N.MK_HOST for k in exp) == 4 * 3 * 4 + 2  # 4097..4100 in four forms; five URIs, twice
    m.eng.close()


@pytest.mark.parametrize("profile", ["reference", "fast"])
@pytest.mark.parametrize("which", CORPORA)
def test_warm_memo_and_steady_state(which, profile):
    """A and prime first, again in a second batch: the second batch reports nothing but host-routed certificates (its hours
    are the first batch's).  Then the table is cleared and the whole corpus runs again: every certificate is new, only the
    host-routed ones come back — the steady state, in which the map kernel's pre-check and meta_home_match decide alone."""
    c = corpus(which)
    m = Memo(c, profile)
    first, second = c.part("first"), c.part("second")
    exp1 = m.run(first[0], first[1])
    assert {k[0] for k in exp1} >= {N.MK_EXPDATE, N.MK_CRL, N.MK_DN}
    exp2 = m.run(second[0], second[1])
    assert {k[0] for k in exp2} <= {N.MK_HOST}
    m.eng.reset_known()
    ders, idx, _ = c.part()
    exp3 = m.run(ders, idx)
    assert {k[0] for k in exp3} <= {N.MK_HOST}
    m.eng.close()


@pytest.mark.parametrize("profile", ["reference", "fast"])
@pytest.mark.parametrize("which", CORPORA)
def test_second_batch_without_the_pre_check(which, profile):
    """The device variant.  The first part warms the memo; the second part is mapped against it (the pre-check marks what it
    finds seen), then ctmr_meta_reset(): the memo is cold and meta_precheck_n = 0, so k_meta_new gets no hint (a.ent null)
    and must look at every new certificate — the sightings are everything in the second batch, exactly."""
    c = corpus(which)
    m = Memo(c, profile)
    first, second = c.part("first"), c.part("second")
    b1 = DeviceBatch(first[0], first[1], 4 * len(first[0]) + 1024)
    b1.map(m.eng)
    m.check(first[0], first[1], *b1.meta(m.eng))
    b2 = DeviceBatch(second[0], second[1], 6 * len(second[0]) + 1024)
    b2.map(m.eng)
    m.eng.meta_reset()
    exp = m.check(second[0], second[1], *b2.meta(m.eng), cold=True)
    assert {k[0] for k in exp} >= {N.MK_EXPDATE, N.MK_CRL, N.MK_DN}
    m.eng.close()


def test_sixty_thousand_items_in_one_memo():
    """60 000 distinct URIs in the memo's 2^22 slots: a home index that spreads puts n(n − 1) / 2^23 ≈ 429 pairs on one home
    slot, and a probe step (meta_upsert's j = (j + 1) & mask) that fails loses or repeats one item of each pair.  Cold every
    URI is reported once; warm, after the table is cleared, none — the items off their home slot are ones the pre-check
    and meta_home_match must leave to meta_upsert; then 2 000 new URIs mixed into 2 000 old ones: exactly the new ones."""
    n = 60000
    c = MC.crowd(n)
    m = Memo(c, "reference", table_slots=1 << 17)
    ders, idx, _ = c.part()
    b = DeviceBatch(ders, idx, n + 4096)
    b.map(m.eng)
    exp = m.check(ders, idx, *b.meta(m.eng))
    assert sum(k[0] == N.MK_CRL for k in exp) == n and len(exp) == n + 2 * MC.CROWD_ISSUERS
    m.eng.reset_known()
    b.map(m.eng)
    assert b.meta(m.eng)[2] == []
    # an old URI keeps the issuer it was seen under (that of the even index of its pair)
    mixed = MC.crowd_certs([(2 * k, n + k, 2 * k) if k & 1 else (n + k, 2 * k, 2 * k) for k in range(2000)], tag=1)
    ders3, idx3 = [d for d, _ in mixed], [i for _, i in mixed]
    b3 = DeviceBatch(ders3, idx3, 8192)
    b3.map(m.eng)
    exp3 = m.check(ders3, idx3, *b3.meta(m.eng))
    assert exp3 == {(N.MK_CRL, 2 * k % MC.CROWD_ISSUERS, 0, MC.crowd_uri(n + k)) for k in range(2000)}
    m.eng.close()


@pytest.mark.parametrize("shared", ["some", "more_than_the_slack"])
@pytest.mark.parametrize("profile", ["reference", "fast"])
def test_more_first_sightings_than_the_item_buffer_holds(profile, shared):
    """ctmr_meta_new (engine/meta.inc) runs k_meta_new into a buffer of 3·n_new + 1024 items.  A batch that brings more makes
    ctmr_meta_new_device fail with CTMR_E_RANGE after it CLEARED the memo (what was appended is lost, so what "seen" meant is
    too); ctmr_meta_new then runs once more into got + 1024 items, without the map kernel's hint (meta_precheck_n = 0).  The
    contract: the call succeeds and reports the batch's first sightings as a COLD memo sees them — items an earlier batch
    reported come again (the host's sets dedup), nothing comes twice in the call; a second call returns the same list; and
    the memo afterwards holds the whole batch.  When the memo held more than 1024 of the batch's items, got + 1024 is too
    small for the cold run as well: that run's own count sizes a third one (before, the call failed with CTMR_E_RANGE
    and Engine.meta_new returned an empty list)."""
    c = MC.overflow() if shared == "some" else MC.overflow(n_big=1000, n_small=200, small_uris=4)
    m = Memo(c, profile)
    small, big = c.part("first"), c.part("second")
    exp_small = m.run(small[0], small[1])
    res = m.eng.map_batch(Batch.from_certs(big[0], big[1]))
    assert res.stats.n_new == len(big[0]) >= 400
    items = m.eng.meta_new()
    exp = m.check(big[0], big[1], res.new_idx, res.records["exp_hour"], items, cold=True)
    assert len(exp) > 3 * len(big[0]) + 1024 and exp & exp_small
    assert m.eng.meta_new() == items
    m.eng.reset_known()
    assert m.run(big[0], big[1]) == set()
    m.eng.close()
