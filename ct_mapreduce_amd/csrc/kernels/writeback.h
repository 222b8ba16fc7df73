// kernels/writeback.h — first sightings per ticket for the ingestion pipeline's write-back.
// gfx950 (CDNA4, wave64) only; part of kernels.h, which includes the pieces in dependency order.
#pragma once
#include "meta.h"

namespace ctmr {

// k_meta_new appends a super-batch's items in the order its atomics fall.  A ticket wants its own: grouped by entry,
// ordered by (entry, kind, off), `entry` counted from the ticket's first, the items' bytes back to back in item order.
// Four small passes over the items (rare once the memo is warm — written for every length and phase, not tuned):
//   k_wb_count   each item's position in the NEW list (the list ascends: a binary search) and its arrival rank there;
//   (scan_u64)   positions → where each new entry's items begin;
//   k_wb_place   items to their entry's range;
//   k_wb_order   one lane per new entry: its ≤ WB_MAX_ITEMS items ordered by (kind, off), rebased to their ticket, their
//                byte source and length written down;
//   (scan_u64)   lengths → where each item's bytes begin;
//   k_wb_gather  one wave per item: certificate → packed bytes.
// k_meta_new emits at most six items a certificate: one expDate, then either one host item or one Name and up to
// META_MAX_URIS URIs.  The bound is checked, not assumed: WB_E_* flags fail the super-batch.
constexpr uint32_t WB_MAX_ITEMS = 2u + META_MAX_URIS;
enum : uint32_t { WB_E_NOT_NEW = 1u, WB_E_TOO_MANY = 2u, WB_E_RANGE = 4u };

struct WbArgs {
  MetaItem* items;              // n_items: k_meta_new's, in arrival order; k_wb_order writes the ordered ones back here
  MetaItem* placed;             // n_items: grouped by new entry, arrival order inside
  uint64_t n_items;
  const uint64_t* new_idx;      // the super-batch's NEW list, ascending
  uint64_t n_new;
  unsigned long long* istart;   // n_new + 1: counts, then (scan) where each new entry's items begin
  uint2* where;                 // n_items: (position in the NEW list, arrival rank there)
  const uint64_t* offsets;      // the certificates, as k_meta_new read them
  const uint64_t* ends;
  const uint64_t* ticket_first; // n_tickets + 1, ascending; [n_tickets] = the super-batch's entries
  uint32_t n_tickets;
  unsigned long long* src;      // n_items: where the item's bytes start in the payload
  unsigned long long* boff;     // n_items + 1: lengths, then (scan) where each item's bytes begin
  uint32_t* err;                // WB_E_* flags
};

__global__ void __launch_bounds__(256) k_wb_count(WbArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= a.n_items) return;
  const uint64_t entry = a.items[k].entry;
  uint64_t lo = 0, hi = a.n_new;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (a.new_idx[mid] < entry) lo = mid + 1;
    else hi = mid;
  }
  if (lo >= a.n_new || a.new_idx[lo] != entry) {  // (cannot happen: k_meta_new walks this list)
    atomicOr(a.err, WB_E_NOT_NEW);
    a.where[k] = make_uint2(~0u, 0u);
    return;
  }
  const unsigned long long rank = atomicAdd(&a.istart[lo], 1ull);
  a.where[k] = make_uint2((uint32_t)lo, (uint32_t)(rank < 0xffffffffull ? rank : 0xffffffffull));
}

__global__ void __launch_bounds__(256) k_wb_place(WbArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= a.n_items) return;
  const uint2 w = a.where[k];
  if (w.x == ~0u) return;
  const unsigned long long at = a.istart[w.x] + w.y;
  if (at < a.istart[w.x + 1] && at < a.n_items) a.placed[at] = a.items[k];
}

__global__ void __launch_bounds__(256) k_wb_order(WbArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.n_new) return;
  const unsigned long long b = a.istart[r], e = a.istart[r + 1];
  if (e == b) return;
  if (e - b > WB_MAX_ITEMS || e > a.n_items) {
    atomicOr(a.err, WB_E_TOO_MANY);
    return;
  }
  const uint32_t c = (uint32_t)(e - b);
  MetaItem it[WB_MAX_ITEMS];
#pragma unroll
  for (uint32_t k = 0; k < WB_MAX_ITEMS; k++)
    if (k < c) it[k] = a.placed[b + k];
  // (kind, off) ascending: a selection over at most six
  uint32_t ord[WB_MAX_ITEMS];
#pragma unroll
  for (uint32_t k = 0; k < WB_MAX_ITEMS; k++) {
    uint32_t below = 0;
#pragma unroll
    for (uint32_t j = 0; j < WB_MAX_ITEMS; j++)
      if (k < c && j < c && j != k) {
        const unsigned long long kj = ((unsigned long long)it[j].kind << 32) | it[j].off, kk = ((unsigned long long)it[k].kind << 32) | it[k].off;
        below += (kj < kk || (kj == kk && j < k)) ? 1u : 0u;
      }
    ord[k] = below;
  }
  const uint64_t entry = a.new_idx[r];
  uint64_t lo, hi;
  cert_range(a.offsets, a.ends, entry, lo, hi);
  // the entry's ticket: the last one that starts at or before it (empty tickets in front share its start)
  uint32_t tl = 0, th = a.n_tickets;
  while (tl < th) {
    const uint32_t mid = tl + ((th - tl) >> 1);
    if (a.ticket_first[mid] <= entry) tl = mid + 1;
    else th = mid;
  }
  const uint64_t base = tl ? a.ticket_first[tl - 1] : 0;
#pragma unroll
  for (uint32_t k = 0; k < WB_MAX_ITEMS; k++) {
    if (k >= c) continue;
    MetaItem m = it[k];
    if (m.kind == MK_HOST || m.kind == MK_EXPDATE) m.len = 0;  // they carry no bytes (ctmr_meta_new)
    if ((uint64_t)m.off + m.len > hi - lo) {
      atomicOr(a.err, WB_E_RANGE);
      m.len = 0;
    }
    m.entry = entry - base;
    const unsigned long long at = b + ord[k];
    a.items[at] = m;
    a.src[at] = lo + m.off;
    a.boff[at] = m.len;
  }
}

// One wave per item.  The destination decides the phases: byte stores up to its first 16-byte boundary, whole 16-byte
// chunks (one unaligned dwordx4 load from the certificate, as GlobalSrc, one aligned store), byte stores for the rest.
// Every load lies inside the item.
__global__ void __launch_bounds__(256) k_wb_gather(const uint8_t* payload, const unsigned long long* src, const unsigned long long* boff,
                                                   uint64_t n_items, uint8_t* out, uint64_t out_cap) {
  const uint64_t k = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  if (k >= n_items) return;
  const unsigned long long at = boff[k], end = boff[k + 1];
  if (end <= at || end > out_cap) return;
  const uint64_t len = end - at;
  const uint8_t* s = payload + src[k];
  uint8_t* d = out + at;
  uint64_t head = (16u - (uint32_t)((uintptr_t)d & 15u)) & 15u;
  if (head > len) head = len;
  if (lane < head) d[lane] = s[lane];
  const uint64_t chunks = (len - head) >> 4;
  for (uint64_t q = lane; q < chunks; q += 64) {
    const U16 v = *(const U16*)(s + head + 16u * q);
    *(uint4*)(d + head + 16u * q) = make_uint4(v.a, v.b, v.c, v.d);
  }
  const uint64_t done = head + 16u * chunks;
  if (lane < len - done) d[done + lane] = s[done + lane];
}

}  // namespace ctmr
