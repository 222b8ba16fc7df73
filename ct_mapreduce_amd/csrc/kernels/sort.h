// kernels/sort.h — the order inside a known-certificate set (include/ctmr.h ctmr_known_sort*): a segmented
// sort of 48-byte member records, whole sets contiguous, by (set, the 40 padded serial octets big-endian, serial_len).
// The records do not move until the end: a 16-byte key per record {u64 word, u32 group, u32 perm} is sorted by
// (group, word) with a stable LSD radix sort of 8-bit digits, in at most SORT_ROUNDS rounds —
//   round 1      group = the record's set within the run, word = serial octets 0..7 as a big-endian number;
//   rounds 2..5  group = the rank of the record's tie group after the round before (records that agreed in set and in
//                every octet so far), word = octets 8..15, 16..23, 24..31, 32..39 fetched through perm;
//   round 6      word = serial_len (zero padding makes b"", 00, 00 00 agree in all 40 octets);
// and the rounds end as soon as no record shares its group with a neighbour — after ONE for CT serials (16..20 random
// octets).  Six rounds whatever the data holds: a common prefix costs one more round per 8 octets, never a quadratic
// tie-break.  k_sort_gather then writes record perm[i] to position i of a buffer aside.
// One radix pass = k_sort_hist (per-tile digit counts, digit-major) → scan_u64 → k_sort_scatter.
// gfx950 (CDNA4, wave64) only; plain vector loads and stores, LDS and LDS / global atomics.
#pragma once
#include "image.h"

namespace ctmr {

constexpr uint32_t SORT_THREADS = 256, SORT_ITEMS = 4, SORT_TILE = SORT_THREADS * SORT_ITEMS;  // keys per block of a pass
constexpr uint32_t SORT_SUBS = SORT_TILE / 64;  // wave-sized pieces of a tile, in key order
constexpr uint32_t SORT_ROUNDS = 6;

// digit d of a key, least significant first: 0..7 = the bytes of word, 8..11 = the bytes of group
__device__ __forceinline__ uint32_t sort_digit(const uint4& k, uint32_t d) {
  const uint32_t w = d < 4u ? k.x : (d < 8u ? k.y : k.z);
  return (w >> ((d & 3u) * 8u)) & 255u;
}

// the lanes of the wave whose digit equals this lane's (every lane of the wave calls; lanes with !valid match nobody):
// eight ballots, one per bit — no LDS, no atomics, and no cost that depends on how the digits repeat
__device__ __forceinline__ unsigned long long sort_peers(uint32_t d, bool valid) {
  unsigned long long m = __ballot(valid);
#pragma unroll
  for (uint32_t b = 0; b < 8u; b++) {
    const bool bit = (d >> b) & 1u;
    const unsigned long long v = __ballot(bit);
    m &= bit ? v : ~v;
  }
  return m;
}

// the word of round r (0-based) of record p: octets 8r..8r+7 as a big-endian number, the last round serial_len
__device__ __forceinline__ unsigned long long sort_word(const uint8_t* rec, uint64_t p, uint32_t r) {
  const unsigned long long* q = (const unsigned long long*)(rec + p * KNOWN_REC_BYTES);
  return r + 1u < SORT_ROUNDS ? __builtin_bswap64(q[1u + r]) : q[0];
}

// Keys of round 1 for records [lo, lo + n) of rec: first[0..ns] = the first record of each set of the run (first[0] = lo,
// first[ns] = lo + n); the set of a record comes from known_run_set (kernels/image.h).
__global__ void __launch_bounds__(256) k_sort_keys(const uint8_t* rec, uint64_t lo, uint64_t n, const uint64_t* first,
                                                   uint32_t ns, uint4* keys) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t set = known_run_set(first, ns, i, n);
  const unsigned long long w = sort_word(rec, lo + i, 0u);
  keys[i] = make_uint4((uint32_t)w, (uint32_t)(w >> 32), set, (uint32_t)i);
}

// A pass, step 1: how often each value of digit d occurs in tile b → hist[value × nb + b].  One LDS atomic per (wave,
// value): a digit on which every key agrees (the high bytes of group, a common prefix) costs what a random one does.
__global__ void __launch_bounds__(SORT_THREADS) k_sort_hist(const uint4* keys, uint64_t n, uint32_t d,
                                                            unsigned long long* hist, uint64_t nb) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t base = (uint64_t)blockIdx.x * SORT_TILE;
#pragma unroll
  for (uint32_t it = 0; it < SORT_ITEMS; it++) {
    const uint64_t i = base + it * SORT_THREADS + threadIdx.x;
    const bool valid = i < n;
    const uint32_t v = valid ? sort_digit(keys[i], d) : 0u;
    const unsigned long long m = sort_peers(v, valid);
    if (valid && (int)lane == __ffsll((long long)m) - 1) atomicAdd(&h[v], (uint32_t)__popcll(m));
  }
  __syncthreads();
  hist[(uint64_t)threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];
}

// A pass, step 2 (behind the exclusive scan of hist[]: offs[value × nb + b] = where tile b's keys of that value go).
// The tile is ranked in LDS — key j of the tile is the (keys of its value in earlier wave-sized pieces + peers in lower
// lanes)-th of its value, so the pass is stable —, put into value order there, and stored from there: lanes next to each
// other hold keys of one value and write next to each other.
__global__ void __launch_bounds__(SORT_THREADS) k_sort_scatter(const uint4* in, uint4* out, uint64_t n, uint32_t d,
                                                               const unsigned long long* offs, uint64_t nb) {
  __shared__ uint32_t cnt[SORT_SUBS][256];
  __shared__ uint32_t lstart[256], wsum[4];
  __shared__ unsigned long long gdelta[256];
  __shared__ uint4 stage[SORT_TILE];
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  const uint64_t base = (uint64_t)blockIdx.x * SORT_TILE;
  const uint32_t ntile = n - base < SORT_TILE ? (uint32_t)(n - base) : SORT_TILE;
#pragma unroll
  for (uint32_t s = 0; s < SORT_SUBS; s++) cnt[s][t] = 0u;
  uint4 k[SORT_ITEMS];
  uint32_t v[SORT_ITEMS], r[SORT_ITEMS];
#pragma unroll
  for (uint32_t it = 0; it < SORT_ITEMS; it++) {
    const uint32_t j = it * SORT_THREADS + t;
    k[it] = j < ntile ? in[base + j] : make_uint4(0u, 0u, 0u, 0u);
    v[it] = sort_digit(k[it], d);
  }
  __syncthreads();
#pragma unroll
  for (uint32_t it = 0; it < SORT_ITEMS; it++) {
    const bool valid = it * SORT_THREADS + t < ntile;
    const unsigned long long m = sort_peers(v[it], valid);
    r[it] = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (valid && (int)lane == __ffsll((long long)m) - 1) cnt[it * 4u + wv][v[it]] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  // thread t owns value t: its keys in the pieces before each piece, its total, and the tile's keys of lower values
  uint32_t tot = 0u;
#pragma unroll
  for (uint32_t s = 0; s < SORT_SUBS; s++) {
    const uint32_t c = cnt[s][t];
    cnt[s][t] = tot;
    tot += c;
  }
  uint32_t inc = tot;
#pragma unroll
  for (uint32_t o = 1; o < 64u; o <<= 1) {
    const uint32_t up = __shfl_up(inc, o);
    if (lane >= o) inc += up;
  }
  if (lane == 63u) wsum[wv] = inc;
  __syncthreads();
  uint32_t before = inc - tot;
  for (uint32_t w = 0; w < wv; w++) before += wsum[w];
  lstart[t] = before;
  gdelta[t] = offs[(uint64_t)t * nb + blockIdx.x] - before;  // + position in the tile's value order = position in out
  __syncthreads();
#pragma unroll
  for (uint32_t it = 0; it < SORT_ITEMS; it++)
    if (it * SORT_THREADS + t < ntile) stage[lstart[v[it]] + cnt[it * 4u + wv][v[it]] + r[it]] = k[it];
  __syncthreads();
#pragma unroll
  for (uint32_t it = 0; it < SORT_ITEMS; it++) {
    const uint32_t j = it * SORT_THREADS + t;
    if (j < ntile) {
      const uint4 q = stage[j];
      out[gdelta[sort_digit(q, d)] + j] = q;
    }
  }
}

// is key i the first of its tie group / does it share the group with a neighbour (keys sorted by (group, word))
__device__ __forceinline__ bool sort_differ(const uint4& a, const uint4& b) { return (a.x != b.x) | (a.y != b.y) | (a.z != b.z); }

// After a round, step 1: tie-group heads per 256 keys → cnt[blk]; keys that still share (group, word) with a neighbour
// → *tied, one atomic per block.
__global__ void __launch_bounds__(256) k_sort_heads(const uint4* keys, uint64_t n, unsigned long long* cnt,
                                                    unsigned long long* tied) {
  __shared__ uint32_t wc[2][4];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  bool head = false, tie = false;
  if (i < n) {
    const uint4 k = keys[i];
    head = i == 0 || sort_differ(keys[i - 1], k);
    tie = !head || (i + 1 < n && !sort_differ(k, keys[i + 1]));
  }
  const unsigned long long mh = __ballot(head), mt = __ballot(tie);
  if (lane == 0) {
    wc[0][wv] = (uint32_t)__popcll(mh);
    wc[1][wv] = (uint32_t)__popcll(mt);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    cnt[blockIdx.x] = (unsigned long long)(wc[0][0] + wc[0][1] + wc[0][2] + wc[0][3]);
    const uint32_t nt = wc[1][0] + wc[1][1] + wc[1][2] + wc[1][3];
    if (nt) atomicAdd(tied, (unsigned long long)nt);
  }
}

// After a round, step 2 (behind the exclusive scan of cnt[]): the keys of round r + 1 (r: 0-based, the round to come) —
// group = heads at or before the key − 1, the rank of its tie group; word = sort_word(perm, r) of a key that is still
// tied, 0 of one that is alone in its group (no read).  Written to `out`: the neighbours are read from `in`.
__global__ void __launch_bounds__(256) k_sort_regroup(const uint4* in, uint4* out, uint64_t n, const unsigned long long* base,
                                                      const uint8_t* rec, uint64_t lo, uint32_t r) {
  __shared__ uint32_t wc[4];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  bool head = false, tie = false;
  uint4 k = make_uint4(0u, 0u, 0u, 0u);
  if (i < n) {
    k = in[i];
    head = i == 0 || sort_differ(in[i - 1], k);
    tie = !head || (i + 1 < n && !sort_differ(k, in[i + 1]));
  }
  const unsigned long long mh = __ballot(head);
  if (lane == 0) wc[wv] = (uint32_t)__popcll(mh);
  __syncthreads();
  if (i >= n) return;
  uint64_t g = base[blockIdx.x] + (uint64_t)__popcll(mh & ((2ull << lane) - 1ull));
  for (uint32_t w = 0; w < wv; w++) g += wc[w];
  const unsigned long long word = tie ? sort_word(rec, lo + k.w, r) : 0ull;
  out[i] = make_uint4((uint32_t)word, (uint32_t)(word >> 32), (uint32_t)(g - 1u), k.w);
}

// The end: record lo + perm[i] to position i of `out` — three 16-byte loads at a random record, three 16-byte stores
// next to the neighbour lanes'.
__global__ void __launch_bounds__(256) k_sort_gather(const uint8_t* rec, uint64_t lo, const uint4* keys, uint64_t n,
                                                     uint8_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint4* src = (const uint4*)(rec + (lo + keys[i].w) * KNOWN_REC_BYTES);
  const uint4 a = src[0], b = src[1], c = src[2];
  uint4* o = (uint4*)(out + i * KNOWN_REC_BYTES);
  o[0] = a;
  o[1] = b;
  o[2] = c;
}

}  // namespace ctmr
