"""CPU twin of the ingestion pipeline's write-back (include/ctmr.h: ctmr_ticket_writeback; csrc/engine/pipeline_writeback.inc
and csrc/kernels/writeback.h): a super-batch's results cut into what each of its tickets gets.  No GPU, no library: the
model the GPU tests hold the device to.

The rules:
  * a super-batch's NEW list ascends and its tickets lie back to back, so a ticket's new entries are one contiguous range of
    the list — and with them its PEM blocks (rebased: pem_offsets[0] == 0), its items and their bytes;
  * an item belongs to the ticket that holds its entry; `entry` is counted from the ticket's first entry;
  * inside a ticket the items are ordered by (entry, kind, off);
  * an empty ticket gets nothing, wherever it lies.
"""
from dataclasses import dataclass

import numpy as np


@dataclass
class Slice:
    new_idx: np.ndarray       # u64: the ticket's new entries, relative to the ticket, ascending
    pem_at: int               # where the ticket's PEM starts in the super-batch's
    pem_offsets: np.ndarray   # u64[len(new_idx) + 1], [0] == 0
    items: list               # [(kind, entry, issuer_idx, exp_hour, bytes)], entry relative to the ticket

    def pem_blocks(self, pem):
        """The ticket's blocks out of the super-batch's PEM bytes."""
        pem = bytes(pem)
        return [pem[self.pem_at + int(self.pem_offsets[k]):self.pem_at + int(self.pem_offsets[k + 1])]
                for k in range(len(self.new_idx))]


def split(new_idx, ticket_first, pem_offsets, items):
    """new_idx: the super-batch's NEW list (ascending entry indices).  ticket_first: T + 1 ascending entry indices, ticket t
    holds the entries [ticket_first[t], ticket_first[t + 1]).  pem_offsets: len(new_idx) + 1 offsets of the super-batch's PEM
    blocks, or None.  items: (kind, entry, issuer_idx, exp_hour, bytes) or (…, bytes, off) with entry an index into the
    super-batch, in any order; off (the item's place in its certificate; 0 when left out) only orders.
    → [Slice] per ticket."""
    new_idx = np.asarray(new_idx, np.uint64)
    tf = [int(x) for x in ticket_first]
    if any(b < a for a, b in zip(tf, tf[1:])) or (len(new_idx) > 1 and (np.diff(new_idx.astype(np.int64)) <= 0).any()):
        raise ValueError("ticket bounds must ascend and the NEW list must ascend strictly")
    if len(new_idx) and (int(new_idx[0]) < tf[0] or int(new_idx[-1]) >= tf[-1]):
        raise ValueError("a new entry outside every ticket")
    po = np.zeros(len(new_idx) + 1, np.uint64) if pem_offsets is None else np.asarray(pem_offsets, np.uint64)
    if len(po) != len(new_idx) + 1:
        raise ValueError("pem_offsets: one more than the NEW list")
    new_set = set(int(i) for i in new_idx)
    keyed = []
    for it in items:
        kind, entry, idx, hour, b = it[:5]
        if int(entry) not in new_set:
            raise ValueError("an item of entry %d, which is not new" % entry)
        keyed.append((int(entry), int(kind), int(it[5]) if len(it) > 5 else 0, int(idx), int(hour), bytes(b)))
    keyed.sort(key=lambda x: x[:3])
    out, at = [], 0
    for t in range(len(tf) - 1):
        lo = int(np.searchsorted(new_idx, tf[t], "left"))
        hi = int(np.searchsorted(new_idx, tf[t + 1], "left"))
        mine = []
        while at < len(keyed) and keyed[at][0] < tf[t + 1]:
            e, kind, _, idx, hour, b = keyed[at]
            mine.append((kind, e - tf[t], idx, hour, b))
            at += 1
        out.append(Slice(new_idx[lo:hi] - np.uint64(tf[t]), int(po[lo]), po[lo:hi + 1] - po[lo], mine))
    return out
