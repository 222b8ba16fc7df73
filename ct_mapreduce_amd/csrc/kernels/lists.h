// kernels/lists.h — per-issuer known-serial lists (include/ctmr.h ctmr_known_lists*): the 48-byte member
// records k_known_export stages (image.h) turned into the text LocalDiskBackend.StoreKnownCertificateList writes, one
// line hex(serial) "\n" per record.  A count pass (per-block byte totals, then scan_u64) and a write pass that stages
// each block's text in LDS and stores it with 16-byte stores between two ragged ends.
// ctmr_known_image_lists*  runs the same two passes over the member records of an image where they lie:
// the kept sets are the segments of a virtual record sequence in list order (KnownSegs, kernels/image.h).  Its count pass (k_image_lists_count) also validates every record it reads.
// gfx950 (CDNA4, wave64) only; part of kernels.h, which includes the pieces in dependency order.
#pragma once
#include "image.h"

namespace ctmr {

constexpr uint32_t LIST_LINE_MAX = 2u * CTMR_MAX_SERIAL + 1u;  // 81: 40 octets as hex and the newline
constexpr uint32_t LIST_BLOCK = 256;

// the serial_len of a record (0..40; clamped so that count and write agree on every length whatever the record holds)
__device__ __forceinline__ uint32_t list_rec_len(const uint8_t* recs, uint64_t i) {
  const uint32_t l = *(const uint32_t*)(recs + i * KNOWN_REC_BYTES);
  return l < (uint32_t)CTMR_MAX_SERIAL ? l : (uint32_t)CTMR_MAX_SERIAL;
}

// Count pass: cnt[blk] = the text bytes of records [256 blk, 256 blk + 256).
__global__ void __launch_bounds__(LIST_BLOCK) k_lists_count(const uint8_t* recs, uint64_t n, unsigned long long* cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * LIST_BLOCK + threadIdx.x;
  uint32_t b = i < n ? 2u * list_rec_len(recs, i) + 1u : 0u;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) b += __shfl_xor(b, d);
  known_block_count(b, cnt, blockIdx.x);
}

__device__ __forceinline__ uint8_t list_hex(uint32_t v) { return (uint8_t)(v < 10u ? '0' + v : 'a' - 10u + v); }

// Write pass, behind the exclusive scan of cnt[] (base[blk]).  Record i's line goes to out + base[blk] + (the bytes of
// the lines before it in its block).  The block's text (at most 256 × 81 B) is laid out in LDS shifted by the 16-byte
// phase of its first global byte, so that every 16-byte aligned global chunk is one aligned 16-byte LDS word.
// pts[0..npts) (ascending record indices of the chunk): pt_off[k] = the text offset of record pts[k] — where the host
// needs the text position of a record (an issuer's first line, host-store lines that go in between).
// src.at(i, n): where record i of the n the launch covers lies (called with i < n by every such lane of a wave).
template <class Src>
__device__ __forceinline__ void lists_write_body(const Src& src, uint64_t n, const unsigned long long* base, uint8_t* out,
                                                 const uint64_t* pts, uint64_t npts, unsigned long long* pt_off) {
  __shared__ __attribute__((aligned(16))) uint8_t text[LIST_BLOCK * LIST_LINE_MAX + 16];
  __shared__ uint32_t ws[LIST_BLOCK / 64];
  const uint64_t i = (uint64_t)blockIdx.x * LIST_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint4 c0 = make_uint4(0u, 0u, 0u, 0u), c1 = c0, c2 = c0;
  if (i < n) {
    const uint4* rec = src.at(i, n);
    c0 = rec[0];
    c1 = rec[1];
    c2 = rec[2];
  }
  const uint32_t len = i < n ? (c0.x < (uint32_t)CTMR_MAX_SERIAL ? c0.x : (uint32_t)CTMR_MAX_SERIAL) : 0u;
  const uint32_t bytes = i < n ? 2u * len + 1u : 0u;
  // block-local exclusive scan: the wave's inclusive scan, then the totals of the waves before
  uint32_t inc = bytes;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t v = __shfl_up(inc, d);
    if ((int)lane >= d) inc += v;
  }
  if (lane == 63u) ws[wv] = inc;
  __syncthreads();
  uint32_t pre = 0u, total = 0u;
#pragma unroll
  for (uint32_t k = 0; k < LIST_BLOCK / 64; k++) {
    pre += k < wv ? ws[k] : 0u;
    total += ws[k];
  }
  const uint32_t local = pre + inc - bytes;
  const unsigned long long g0 = base[blockIdx.x];
  uint8_t* const gstart = out + g0;
  const uint32_t phase = (uint32_t)((uintptr_t)gstart & 15u);
  if (i < n) {
    uint8_t* t = text + phase + local;
    const uint32_t w[10] = {c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w};
#pragma unroll
    for (uint32_t q = 0; q < 10; q++) {
#pragma unroll
      for (uint32_t b = 0; b < 4; b++) {
        if (4u * q + b < len) {
          const uint32_t o = (w[q] >> (8u * b)) & 0xffu;
          t[2u * (4u * q + b)] = list_hex(o >> 4);
          t[2u * (4u * q + b) + 1u] = list_hex(o & 15u);
        }
      }
    }
    t[2u * len] = '\n';
  }
  // the positions the host asked for that fall in this wave
  if (npts) {
    const uint64_t wfirst = (uint64_t)blockIdx.x * LIST_BLOCK + wv * 64u;
    uint64_t lo = 0, hi = npts;  // first point >= wfirst (wave-uniform)
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (pts[mid] < wfirst) lo = mid + 1;
      else hi = mid;
    }
    for (uint64_t k = lo; k < npts && pts[k] < wfirst + 64u; k++)
      if (pts[k] == i && i < n) pt_off[k] = g0 + local;
  }
  __syncthreads();
  // out: [gstart, gstart + total); LDS byte x ↔ global byte gstart - phase + x
  const uint32_t head = (16u - phase) & 15u;                 // bytes before the first 16-byte aligned global address
  if (head >= total) {
    if (threadIdx.x < total) gstart[threadIdx.x] = text[phase + threadIdx.x];
    return;
  }
  const uint32_t nvec = (total - head) >> 4, tail = (total - head) & 15u;
  if (threadIdx.x < head) gstart[threadIdx.x] = text[phase + threadIdx.x];
  uint4* gv = (uint4*)(gstart + head);
  const uint4* lv = (const uint4*)(text + phase + head);    // phase + head is 0 or 16: aligned
  for (uint32_t k = threadIdx.x; k < nvec; k += LIST_BLOCK) gv[k] = lv[k];
  if (threadIdx.x < tail) {
    const uint32_t x = head + 16u * nvec + threadIdx.x;
    gstart[x] = text[phase + x];
  }
}

// the records where they were staged: record i is the i-th of recs
struct ListStaged {
  const uint8_t* recs;
  __device__ __forceinline__ const uint4* at(uint64_t i, uint64_t) const { return (const uint4*)(recs + i * KNOWN_REC_BYTES); }
};

__global__ void __launch_bounds__(LIST_BLOCK) k_lists_write(const uint8_t* recs, uint64_t n, const unsigned long long* base,
                                                           uint8_t* out, const uint64_t* pts, uint64_t npts,
                                                           unsigned long long* pt_off) {
  lists_write_body(ListStaged{recs}, n, base, out, pts, npts, pt_off);
}

// ---- the lists of an image (ctmr_known_image_lists*).  A launch covers n virtual records of k whole segments — the
// kept sets in list order — and reads record i where KnownSegs::at finds it (kernels/image.h).
using ListSegs = KnownSegs;

// Count pass over the segments: cnt[blk] = the text bytes of the launch's records [256 blk, 256 blk + 256), and every
// record read is validated (known_load) and a bad one reported in *err (known_report_bad).
__global__ void __launch_bounds__(LIST_BLOCK) k_image_lists_count(ListSegs g, uint64_t n, unsigned long long* cnt, uint32_t* err) {
  const uint64_t i = (uint64_t)blockIdx.x * LIST_BLOCK + threadIdx.x;
  uint32_t b = 0u, bad = 0u;
  if (i < n) {
    unsigned long long len, s[5];
    bad = known_load(g.at(i, n), len, s);
    b = 2u * (uint32_t)(len < (unsigned long long)CTMR_MAX_SERIAL ? len : (unsigned long long)CTMR_MAX_SERIAL) + 1u;
  }
  known_report_bad(bad, err);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) b += __shfl_xor(b, d);
  known_block_count(b, cnt, blockIdx.x);
}

// Write pass over the segments: k_lists_write with the indirect source (pts / pt_off in the launch's record indices).
__global__ void __launch_bounds__(LIST_BLOCK) k_image_lists_write(ListSegs g, uint64_t n, const unsigned long long* base,
                                                                 uint8_t* out, const uint64_t* pts, uint64_t npts,
                                                                 unsigned long long* pt_off) {
  lists_write_body(g, n, base, out, pts, npts, pt_off);
}

}  // namespace ctmr
