// kernels/text_scan.h — what the two text decoders share (kernels/entries_json.h: get-entries JSON bodies; kernels/
// pem_decode.h: PEM certificate files).  A text is bytes at any alignment, cut into segments by ascending bounds (a
// response there, a file here).  Both decoders run the same two kinds of pass over it:
//   mark      one wave per TX_TILE bytes: the aligned 16-byte chunks that cover the text are read, what lies outside the
//             bounds is masked (tx_chunk); per byte a class, per block counts, an exclusive scan, then the token list.
//   decode    the hot path: one tile of TX_DTILE base64 characters of one item per block → TX_DOUT bytes, staged in LDS at
//             the 16-byte phase of the first global byte and stored as k_lists_write stores.  k_ej_tiles and
//             k_ej_tile_list list the tiles: both decoders launch them, under the names their recorded statistics know.
// Non-temporal loads: the text is read and never needed again.  gfx950 (CDNA4, wave64) only; part of kernels.h.
#pragma once
#include "resp_parse.h"

namespace ctmr {

constexpr uint32_t TX_BLOCK = 64, TX_PER = 16, TX_TILE = TX_BLOCK * TX_PER;  // mark: one wave, 16 bytes a lane
constexpr uint32_t TX_DBLOCK = 256, TX_DTILE = 4 * TX_DBLOCK, TX_DOUT = 3 * TX_DBLOCK;  // decode: a quantum a lane
// A launch takes at most TX_GRID blocks (a grid of 2^32 threads and more is not launched whole): the host launches in
// turns, b0 = the first block of the turn.
constexpr uint64_t TX_GRID = 1ull << 22;

// the text: segment r is s[sb[r], sb[r + 1]); a0 = the address of s + sb[0] rounded down to 16
struct TxText {
  const uint8_t* s;
  const uint64_t* sb;  // S + 1, ascending (device)
  uint64_t S, lo, hi;  // lo = sb[0], hi = sb[S], lo < hi
  uint64_t a0;
};

// the segment of the byte at p (lo <= p < hi): the largest r < S with sb[r] <= p
__device__ __forceinline__ uint64_t tx_segment_of(const uint64_t* sb, uint64_t S, uint64_t p) {
  uint64_t l = 0, h = S - 1;
  while (l < h) {
    const uint64_t mid = (l + h + 1) >> 1;
    if (sb[mid] <= p) l = mid;
    else h = mid - 1;
  }
  return l;
}

// the mark block of the byte at p
__device__ __forceinline__ uint64_t tx_block_of(const TxText& T, uint64_t p) { return ((uint64_t)(uintptr_t)T.s + p - T.a0) / TX_TILE; }

// the lane's chunk of block blk: its 16 bytes (zero when none is of the text), *p0 = the offset of its first byte from
// s (below lo, even negative, when the chunk begins before the text), *valid = the bytes that lie in [lo, hi)
__device__ __forceinline__ uint4 tx_chunk(const TxText& T, uint64_t blk, uint32_t lane, int64_t* p0, uint32_t* valid) {
  const uint64_t a = T.a0 + blk * TX_TILE + lane * TX_PER;
  const int64_t p = (int64_t)(a - (uint64_t)(uintptr_t)T.s);
  const int64_t first = (int64_t)T.lo - p, end = (int64_t)T.hi - p;  // valid: first <= q < end
  uint32_t m = 0xffffu;
  if (first > 0) m &= first >= 16 ? 0u : (0xffffu << (uint32_t)first);
  if (end < 16) m &= end <= 0 ? 0u : (0xffffu >> (16u - (uint32_t)end));
  m &= 0xffffu;
  *p0 = p;
  *valid = m;
  return m ? ld_payload16((const uint4*)(uintptr_t)a) : make_uint4(0u, 0u, 0u, 0u);
}

__device__ __forceinline__ uint32_t tx_byte(const uint4& v, uint32_t q) {
  const uint32_t w = q < 8u ? (q < 4u ? v.x : v.y) : (q < 12u ? v.z : v.w);
  return (w >> (8u * (q & 3u))) & 0xffu;
}

// 1 when c is of the base64 alphabet A-Za-z0-9+/, else 0: a bit of the mask below, and what a mark kernel asks in the loop
// that classes its bytes.  A macro: behind a function's boundary the compiler orders the mark kernels' class loops
// otherwise, which costs k_ej_mark<false> four VGPRs and a wave per SIMD.
#define TX_ALPHABET_BIT(c) (((((c) | 0x20u) - 0x61u) < 26u || ((c) - 0x30u) < 10u || (c) == 0x2bu || (c) == 0x2fu) ? 1u : 0u)

// the bytes of a chunk that are of the alphabet — PAD: or '='
template <bool PAD>
__device__ __forceinline__ uint32_t tx_alphabet_mask(const uint4& v) {
  uint32_t m = 0u;
#pragma unroll
  for (uint32_t q = 0; q < TX_PER; q++) {
    const uint32_t c = tx_byte(v, q);
    m |= (TX_ALPHABET_BIT(c) | ((PAD && c == 0x3du) ? 1u : 0u)) << q;
  }
  return m;
}

// the bytes of the chunk at p0 that lie below at
__device__ __forceinline__ uint32_t tx_below(int64_t p0, uint64_t at) {
  const int64_t d = (int64_t)at - p0;
  return d >= 16 ? 0xffffu : d > 0 ? 0xffffu >> (16u - (uint32_t)d) : 0u;
}

// the exclusive prefix sum of v over the wave; *total = the wave's sum
__device__ __forceinline__ uint32_t tx_wave_scan(uint32_t v, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d);
    if ((int)lane >= d) inc += o;
  }
  *total = __shfl(inc, 63);
  return inc - v;
}

// the block's segment, when it has one only: that of its first byte of the text, whose end lies behind the block.
// → that segment; *uniform = no byte of the block lies in another
__device__ __forceinline__ uint64_t tx_block_segment(const TxText& T, uint64_t blk, bool* uniform) {
  const uint64_t s0 = (uint64_t)(uintptr_t)T.s;
  const uint64_t blk_lo = T.a0 + blk * TX_TILE - s0 + (blk == 0 ? T.lo - (T.a0 - s0) : 0ull);
  const uint64_t blk_end = T.a0 + (blk + 1ull) * TX_TILE - s0;
  const uint64_t r_lo = tx_segment_of(T.sb, T.S, blk_lo);
  *uniform = T.sb[r_lo + 1] >= (blk_end < T.hi ? blk_end : T.hi);
  return r_lo;
}

// What is counted of [lo, at), at in block blk: cnt[blk], the scanned block count, plus what MASK marks among the text's
// bytes of the block below at.  Every lane of the wave calls and gets the same.
template <uint32_t (*MASK)(const uint4&)>
__device__ __forceinline__ unsigned long long tx_boundary_prefix(const TxText& T, uint64_t blk, uint64_t at, const unsigned long long* cnt) {
  int64_t p0;
  uint32_t valid, total;
  const uint4 v = tx_chunk(T, blk, threadIdx.x & 63u, &p0, &valid);
  (void)tx_wave_scan((uint32_t)__popc(MASK(v) & valid & tx_below(p0, at)), &total);
  return cnt[blk] + total;
}

// first[k] = the tokens in front of sb[r + k], k = 0, 1 (r <= S; behind the last bound comes that bound again): the first
// token at or behind it.  tok[] ascends, a token's position is tok[] >> shift, its kind lies below.
__device__ __forceinline__ void tx_first_tokens(const TxText& T, uint64_t r, const unsigned long long* tok, uint64_t ntok, uint32_t shift,
                                                uint64_t (&first)[2]) {
#pragma unroll
  for (uint32_t k = 0; k < 2; k++) {
    const uint64_t at = T.sb[r + k < T.S ? r + k : T.S];
    uint64_t l = 0, h = ntok;
    while (l < h) {
      const uint64_t mid = (l + h) >> 1;
      if ((tok[mid] >> shift) < at) l = mid + 1;
      else h = mid;
    }
    first[k] = l;
  }
}

// the lowest segment outside the grammar and the lowest offset reported: every lane of the wave calls.  An offset lies
// inside its segment, segments ascend, so the lowest offset belongs to the lowest segment.
__device__ __forceinline__ void tx_report(unsigned long long* err, bool bad, uint64_t r, uint64_t off) {
  unsigned long long v = bad ? (unsigned long long)r : ~0ull, o = bad ? (unsigned long long)off : ~0ull;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long v2 = __shfl_xor(v, d), o2 = __shfl_xor(o, d);
    v = v2 < v ? v2 : v;
    o = o2 < o ? o2 : o;
  }
  if ((threadIdx.x & 63u) == 0 && v != ~0ull) {
    atomicMin(err, v);
    atomicMin(err + 1, o);
  }
}

// each (every segment judged on its own), behind check: the item count of a segment with a verdict, from whichever pass,
// goes to zero.  cnt[r] = the items of segment r when bad_at[r] says none, else 0; cnt[R] = 0 (the scan's total).  first0:
// the scan of the counts the check numbered its items by.  Both decoders launch it, as they do the two kernels below.
__global__ void __launch_bounds__(RP_BLOCK) k_ej_drop(uint64_t b0, uint64_t R, const unsigned long long* bad_at, const unsigned long long* first0,
                                                      unsigned long long* cnt) {
  const uint64_t r = (b0 + blockIdx.x) * RP_BLOCK + threadIdx.x;
  if (r > R) return;
  cnt[r] = (r < R && bad_at[r] == ~0ull) ? first0[r + 1] - first0[r] : 0ull;
}

// tiles[i] = the decode tiles of item i (bounds: the scanned decoded lengths)
__global__ void __launch_bounds__(RP_BLOCK) k_ej_tiles(uint64_t b0, const unsigned long long* bounds, uint64_t nstr, unsigned long long* tiles) {
  const uint64_t i = (b0 + blockIdx.x) * RP_BLOCK + threadIdx.x;
  if (i < nstr) tiles[i] = (bounds[i + 1] - bounds[i] + TX_DOUT - 1) / TX_DOUT;
}

// tile_str[t] = the item of tile t (tile_first: the scanned tiles[]).  A lane writes the first TX_OWN tiles of its
// item; what a long item has beyond them the whole wave writes, one such item after the other.
constexpr uint32_t TX_OWN = 8;
__global__ void __launch_bounds__(RP_BLOCK) k_ej_tile_list(uint64_t b0, const unsigned long long* tile_first, uint64_t nstr,
                                                           unsigned long long* tile_str) {
  const unsigned long long i = (b0 + blockIdx.x) * RP_BLOCK + threadIdx.x;
  const unsigned long long t0 = i < nstr ? tile_first[i] : 0ull, t1 = i < nstr ? tile_first[i + 1] : 0ull;
  for (unsigned long long t = t0; t < t1 && t < t0 + TX_OWN; t++) tile_str[t] = i;
  unsigned long long big = __ballot(t1 - t0 > TX_OWN);
  while (big) {  // (wave-uniform)
    const int l = __ffsll(big) - 1;
    big &= big - 1ull;
    const unsigned long long from = __shfl(t0, l) + TX_OWN, to = __shfl(t1, l), str = __shfl(i, l);
    for (unsigned long long t = from + (threadIdx.x & 63u); t < to; t += 64ull) tile_str[t] = str;
  }
}

// A-Z a-z 0-9 + / → 0..63; '=' → 0 (its bits are dropped).  Range arithmetic: nothing else reaches the decoder.
__device__ __forceinline__ uint32_t tx_sextet(uint32_t c) {
  uint32_t v = c - 65u;
  if (c >= 97u) v = c - 71u;
  if (c < 65u) v = c + 4u;
  if (c < 48u) v = c == 43u ? 62u : 63u;
  if (c == 61u) v = 0u;
  return v & 63u;
}

// A staged tile leaves: stage[phase, phase + total) → [gstart, gstart + total), LDS byte x ↔ global byte gstart - phase + x
// (k_lists_write): 16-byte non-temporal stores for the body, byte stores for the ragged ends, so that neighbouring tiles
// never share a store.  phase = the 16-byte phase of gstart; every thread of the block calls, behind the barrier.
__device__ __forceinline__ void tx_store_tile(const uint8_t* stage, uint32_t phase, uint32_t total, uint8_t* gstart) {
  const uint32_t head = (16u - phase) & 15u;
  if (head >= total) {
    if (threadIdx.x < total) gstart[threadIdx.x] = stage[phase + threadIdx.x];
    return;
  }
  const uint32_t nvec = (total - head) >> 4, tail = (total - head) & 15u;
  if (threadIdx.x < head) gstart[threadIdx.x] = stage[phase + threadIdx.x];
  if (threadIdx.x < nvec) st_stream16((uint4*)(gstart + head) + threadIdx.x, ((const uint4*)(stage + phase + head))[threadIdx.x]);
  if (threadIdx.x < tail) {
    const uint32_t x = head + 16u * nvec + threadIdx.x;
    gstart[x] = stage[phase + x];
  }
}

// the decode block of tile t: tile k of item i = tile_item[t], its characters [TX_DTILE k, …) → total (1 … TX_DOUT)
// bytes at dst = bounds[i] + TX_DOUT k of the output
struct TxTile { uint64_t i, k, dst; uint32_t total; };
__device__ __forceinline__ TxTile tx_tile(uint64_t t, const unsigned long long* tile_item, const unsigned long long* tile_first,
                                          const unsigned long long* bounds) {
  const uint64_t i = tile_item[t], k = t - tile_first[i];
  const uint64_t at0 = bounds[i], left = bounds[i + 1] - at0 - k * TX_DOUT;
  return TxTile{i, k, at0 + k * TX_DOUT, left < TX_DOUT ? (uint32_t)left : TX_DOUT};
}

// The decode of a tile (stage: TX_DOUT + 16 bytes of LDS, 16-byte aligned).  The lane has a quantum, four characters:
__device__ __forceinline__ bool tx_has_quantum(const TxTile& w) { return 3u * threadIdx.x < w.total; }
// that lane's quantum, at address a of any alignment — two non-temporal dword loads and a funnel shift — is staged
__device__ __forceinline__ void tx_stage_quantum(uint8_t* stage, const TxTile& w, uint64_t a) {
  const uint32_t sh = 8u * (uint32_t)(a & 3ull);
  const uint32_t* p = (const uint32_t*)(uintptr_t)(a & ~3ull);
  uint32_t ch = __builtin_nontemporal_load(p);
  if (sh) ch = (ch >> sh) | (__builtin_nontemporal_load(p + 1) << (32u - sh));  // (the quantum reaches into p[1])
  const uint32_t x = (tx_sextet(ch & 0xffu) << 18) | (tx_sextet((ch >> 8) & 0xffu) << 12) | (tx_sextet((ch >> 16) & 0xffu) << 6) |
                     tx_sextet(ch >> 24);
  uint8_t* o = stage + (uint32_t)(w.dst & 15ull) + 3u * threadIdx.x;
  o[0] = (uint8_t)(x >> 16);
  o[1] = (uint8_t)(x >> 8);
  o[2] = (uint8_t)x;
}
// every thread of the block: behind the barrier the staged tile leaves for out + w.dst
__device__ __forceinline__ void tx_tile_leaves(const uint8_t* stage, const TxTile& w, uint8_t* out) {
  __syncthreads();
  tx_store_tile(stage, (uint32_t)(w.dst & 15ull), w.total, out + w.dst);
}

}  // namespace ctmr
