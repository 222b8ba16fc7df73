"""Entry views in any byte order (pure numpy, no GPU): the certificates of a packed host Batch laid out in a blob in an order
of the caller's choosing, addressed as [cert_start[i], cert_end[i]) — what ctmr_map_view_device and every call that takes
`offsets` + `ends` accept.  Entry i of a view is always byte for byte batch.cert(i); only WHERE it lies changes.

The map kernels read through one buffer descriptor per wave of 64 entries whose base is the certificate of the wave's first
lane (kernels/readers.h wave_buf): a lane whose certificate lies BELOW that base is out of the descriptor's reach and takes the
exact readers.  Each order below is described by what it guarantees per wave of 64 entries (lanes_below_lane0 counts it;
tests/test_view_corpus_cpu.py holds the builder to it — a builder that quietly produced an ascending view would let every GPU
test of tests/test_gpu_view_order.py pass):

  ascending           control: no lane out of reach
  reversed            lanes 1..63 all below lane 0
  shuffled            a seeded permutation of the whole batch
  first_lane_highest  ascending, except that each wave's lane 0 lies behind the other lanes of its wave
  one_lane_low        ascending, except one lane per wave (the lane index varies 1..63 over the waves) lies below lane 0
  aliased             entries whose certificates are byte-identical share ONE byte range (cert_start repeats), shuffled
  with_empties        ascending; zero-length entries (with_empty_entries makes every k-th one) have start == end at offset 0,
                      at an arbitrary offset and at the blob's end in turn; entry_type stays the caller's

The space in front of, between and behind the certificates is NON-ZERO noise, never zeros: a stale or zeroed window must not be
able to pass for padding."""
import numpy as np

from ct_mapreduce_amd import _native as N
from ct_mapreduce_amd.engine import Batch

ORDERS = ("ascending", "reversed", "shuffled", "first_lane_highest", "one_lane_low", "aliased", "with_empties")
WAVE = 64


def with_empty_entries(batch, k, first=2):
    """The batch with entries first, first + k, … replaced by zero-length certificates (issuer_idx and entry_type kept)."""
    certs = [b"" if i >= first and (i - first) % k == 0 else batch.cert(i) for i in range(batch.n)]
    return Batch.from_certs(certs, batch.issuer_idx.copy(), batch.entry_type.copy())


def _placement(batch, order, rng):
    """Slots in blob order: a list of lists of entry indices; the entries of one slot share one byte range."""
    n = batch.n
    if order in ("ascending", "with_empties"):
        seq = list(range(n))
    elif order == "reversed":
        seq = list(range(n - 1, -1, -1))
    elif order == "shuffled":
        seq = [int(i) for i in rng.permutation(n)]
    elif order == "first_lane_highest":
        seq = []
        for w0 in range(0, n, WAVE):
            seq += list(range(w0 + 1, min(w0 + WAVE, n))) + [w0]
    elif order == "one_lane_low":
        seq = []
        for w, w0 in enumerate(range(0, n, WAVE)):
            m = min(WAVE, n - w0)
            lanes = list(range(m))
            if m > 1:
                j = 1 + w % min(WAVE - 1, m - 1)
                lanes = [j] + [x for x in lanes if x != j]
            seq += [w0 + x for x in lanes]
    elif order == "aliased":
        groups = {}
        for i in range(n):
            groups.setdefault(batch.cert(i), []).append(i)
        slots = list(groups.values())
        return [slots[int(k)] for k in rng.permutation(len(slots))]
    else:
        raise KeyError(order)
    return [[i] for i in seq]


def make_view(batch, order, fill=1, lead=0, gap=0):
    """(blob u8, cert_start u64[n], cert_end u64[n]) with blob[cert_start[i]:cert_end[i]] == batch.cert(i) for every entry,
    laid out in the byte order `order` (module docstring).  fill: the seed of the noise (integers 1..255) and of the order's
    own choices; lead: noise octets in front of the first certificate; gap: between two certificates lie 0..gap noise octets
    (seeded).  len(blob) = blob_bytes + CTMR_PAYLOAD_PAD: the view's blob_bytes is len(blob) - N.PAYLOAD_PAD, and the pad
    behind it is readable noise."""
    if order not in ORDERS:
        raise KeyError(order)
    rng = np.random.default_rng([int(fill), ORDERS.index(order)])
    slots = _placement(batch, order, rng)
    n = batch.n
    start = np.zeros(n, np.uint64)
    end = np.zeros(n, np.uint64)
    at, where, empties = int(lead), [], []
    for slot in slots:
        ln = len(batch.cert(slot[0]))
        if ln == 0 and order == "with_empties":
            empties.append((slot, at))
            continue
        where.append((slot, at, ln))
        at += ln + (int(rng.integers(0, gap + 1)) if gap else 0)
    total = at
    blob = rng.integers(1, 256, size=total + N.PAYLOAD_PAD, dtype=np.uint8)
    for slot, lo, ln in where:
        blob[lo:lo + ln] = np.frombuffer(batch.cert(slot[0]), np.uint8)
        for i in slot:
            start[i], end[i] = lo, lo + ln
    for k, (slot, here) in enumerate(empties):       # offset 0, where ascending order would put it, the blob's end
        lo = (0, here, total)[k % 3]
        for i in slot:
            start[i] = end[i] = lo
    return blob, start, end


def lanes_below_lane0(start):
    """Per wave of 64 entries: how many lanes' certificates begin below the one of the wave's lane 0 (out of reach)."""
    start = np.asarray(start, np.uint64)
    return np.array([int((start[w0:w0 + WAVE] < start[w0]).sum()) for w0 in range(0, len(start), WAVE)], np.int64)
