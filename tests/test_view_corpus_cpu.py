"""The entry-view builder of tests/view_corpus.py holds what it promises (no GPU): every entry's bytes are the batch's, every
byte order has its stated per-wave property, ranges overlap only where the order says so, and nothing between the
certificates is a zero.  This is what keeps tests/test_gpu_view_order.py honest: a builder that quietly produced an ascending
view would let all of its cases pass."""
import numpy as np
import pytest

from ct_mapreduce_amd import synth, _native as N
from ct_mapreduce_amd.engine import Batch
from tests import view_corpus as V


def dup_batch(n, seed=5):
    """A synthetic batch in which every seventh entry repeats an EARLIER entry byte for byte (same issuer and entry type)."""
    cfg = synth.config(seed=seed, n_issuers=4, dup_permille=100)
    b = synth.host_batch(cfg, 0, n)
    certs, iss, et = [], [], []
    for i in range(n):
        j = i // 2 if i % 7 == 6 else i
        certs.append(b.cert(j)); iss.append(int(b.issuer_idx[j])); et.append(int(b.entry_type[j]))
    return Batch.from_certs(certs, iss, et)


SIZES = (64 * 5, 64 * 4 + 37, 5)


def covered(blob, start, end):
    m = np.zeros(len(blob), bool)
    for lo, hi in zip(start, end):
        m[int(lo):int(hi)] = True
    return m


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("order", V.ORDERS)
@pytest.mark.parametrize("lead,gap", [(0, 0), (301, 150)])
def test_every_entry_is_the_batch_certificate_and_the_order_has_its_property(order, n, lead, gap):
    b = dup_batch(n)
    if order == "with_empties":
        b = V.with_empty_entries(b, 5)
    blob, start, end = V.make_view(b, order, fill=3, lead=lead, gap=gap)
    total = len(blob) - N.PAYLOAD_PAD
    assert start.dtype == end.dtype == np.uint64 and len(start) == len(end) == n
    assert (end >= start).all() and int(end.max()) <= total
    for i in range(n):
        assert blob[int(start[i]):int(end[i])].tobytes() == b.cert(i), i
    # noise, never zeros, wherever no certificate lies — the pad behind the blob included
    free = ~covered(blob, start, end)
    assert free[total:].all() and (blob[free] != 0).all()
    if lead:
        assert free[:lead].all() and int(start[end > start].min()) == lead and free.sum() > lead + N.PAYLOAD_PAD
    # ranges do not overlap, except where entries alias one range
    live = np.nonzero(end > start)[0]
    ranges = sorted({(int(start[i]), int(end[i])) for i in live})
    assert all(a[1] <= c[0] for a, c in zip(ranges, ranges[1:]))
    if order == "aliased":
        assert len(ranges) < len(live) or n < 7                                  # cert_start repeats
        groups = {}
        for i in live:
            groups.setdefault(int(start[i]), set()).add(b.cert(i))
        assert all(len(g) == 1 for g in groups.values())
        assert len(ranges) == len({b.cert(i) for i in range(n)})                  # every byte-identical group shares ONE range
    else:
        assert len(ranges) == len(live)
    # the per-wave property
    below = V.lanes_below_lane0(start)
    sizes = np.array([min(64, n - w0) for w0 in range(0, n, 64)])
    if order == "ascending":
        assert (below == 0).all() and (np.diff(start.astype(np.int64)) > 0).all()
    elif order in ("reversed", "first_lane_highest"):
        assert (below == sizes - 1).all()
        if order == "first_lane_highest":                                         # … and otherwise ascending
            for w0 in range(0, n, 64):
                s = start[w0 + 1:w0 + 64].astype(np.int64)
                assert (np.diff(s) > 0).all()
            assert (np.diff(start[::64].astype(np.int64)) > 0).all()
    elif order == "one_lane_low":
        assert (below == np.minimum(sizes - 1, 1)).all()
        lows = [int(np.nonzero(start[w0:w0 + 64] < start[w0])[0][0]) for w0 in range(0, n, 64) if min(64, n - w0) > 1]
        assert all(1 <= j <= 63 for j in lows) and (len(lows) < 3 or len(set(lows)) > 1)      # the lane varies over the waves
    elif order in ("shuffled", "aliased"):
        assert n < 64 or (below.sum() > 0 and ((below > 0) & (below < sizes - 1)).any())      # neither sorted nor reversed
        assert not (np.diff(start.astype(np.int64)) > 0).all()
    elif order == "with_empties":
        empty = np.nonzero(end == start)[0]
        assert len(empty) == len(range(2, n, 5)) and (b.entry_type == dup_batch(n).entry_type).all()
        at = [int(start[i]) for i in empty]
        assert at[0] == 0 and (len(at) < 3 or at[2] == total) and (len(at) < 2 or 0 < at[1] < total)
        assert (np.diff(start[live].astype(np.int64)) > 0).all()


def test_the_orders_differ_and_are_reproducible():
    b = dup_batch(64 * 3 + 9)
    seen = {}
    for order in V.ORDERS:
        bb = V.with_empty_entries(b, 5) if order == "with_empties" else b
        v1, v2 = V.make_view(bb, order, fill=9, lead=17, gap=40), V.make_view(bb, order, fill=9, lead=17, gap=40)
        assert all((x == y).all() for x, y in zip(v1, v2))
        seen[order] = v1[1].tobytes()
    assert len(set(seen.values())) == len(V.ORDERS)
    other = V.make_view(b, "shuffled", fill=10, lead=17, gap=40)
    assert other[1].tobytes() != seen["shuffled"]
    with pytest.raises(KeyError):
        V.make_view(b, "sorted")
