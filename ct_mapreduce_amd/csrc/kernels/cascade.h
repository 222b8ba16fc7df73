// kernels/cascade.h — the CRLite filter cascade of a revoked / not-revoked image pair (include/ctmr.h ctmr_cascade_*,
// DESIGN.md §29): Bloom filter layers whose hash functions are SHA-256 over salt ‖ u32le(i) ‖ u8(level) ‖ key, the key a
// member record's 32-byte issuer digest and its serial octets.  k_casc_insert sets the bits of the records a layer
// holds, k_casc_test leaves the flags of the pass (KnownFlags, kernels/image.h): one bit per record that passes the
// layer; after a scan of the counts k_casc_compact writes the survivors as (record index, issuer ordinal) pairs at
// their ranks (known_flags_before), the list the next layers read instead of the image.  k_casc_query walks a
// finished cascade for every member record of a probe image.
// One lane per record; the message is assembled in registers and hashed in one or two sha256_compress per hash function.
// No cross-workgroup publish, no spin-wait; the global atomics are the bits' atomicOr (no return value used) and the
// bad-record report (known_report_bad).
// gfx950 (CDNA4, wave64) only; part of kernels.h, which includes the pieces in dependency order.
#pragma once
#include "split.h"

namespace ctmr {

// Where the records of a launch lie.  list == null: the run of whole kept sets g (KnownSegs, kernels/image.h; g.kord:
// the issuer ordinal of each set in the image's own issuer table, g.hour: null).  Otherwise record i of the launch is member
// record list[i].x of g.recs under issuer ordinal list[i].y — a survivor list k_casc_compact wrote.
struct CascSrc {
  FindSegs g;
  const uint2* list;
  const uint32_t* dig;  // the image's issuer table: 8 words per ordinal
};

// What every message of a call begins with: salt ‖ four zero octets (i) ‖ one zero octet (level), as little-endian
// words, zeros behind; i and level are put in per hash.
struct CascHash {
  uint32_t pre[6];
  uint32_t salt_len;  // 0..16
};

// One layer: m bits in 32-bit words (bit b: word b >> 5, mask 1 << (b & 31) — byte b >> 3, mask 1 << (b & 7)).
struct CascLayer {
  uint32_t* bits;
  uint32_t m, k, level;
};

// Record i of a launch of n: its index in the image and its issuer ordinal — the list's pair, or the segment search.
__device__ __forceinline__ void casc_locate(const CascSrc& c, uint64_t i, uint64_t n, uint32_t& idx, uint32_t& ord) {
  if (c.list) {
    const uint2 e = c.list[i];
    idx = e.x;
    ord = e.y;
  } else {
    uint32_t set;
    idx = (uint32_t)c.g.index(i, n, &set);
    ord = c.g.kord[set];
  }
}

// … and the record itself, validated (known_load).
__device__ __forceinline__ uint32_t casc_fetch(const CascSrc& c, uint64_t i, uint64_t n, uint32_t& idx, uint32_t& ord,
                                               unsigned long long& len, unsigned long long s[5]) {
  casc_locate(c, i, n, idx, ord);
  return known_load((const uint4*)(c.g.recs + (uint64_t)idx * KNOWN_REC_BYTES), len, s);
}

// The padded message of a valid record as 32 big-endian words, i and level zero: the prefix, the digest of ordinal ord,
// the len serial octets (the record's own padding supplies the zeros behind them), 0x80, and the bit length at the end
// of the first block (→ false: 37..55 octets) or of the second (→ true: 56..93 octets).  Every index is static after
// unrolling: M[] stays in registers.
__device__ __forceinline__ bool casc_message(const CascHash& hp, const uint32_t* dig, unsigned long long len, const unsigned long long s[5],
                                             uint32_t M[32]) {
  uint32_t b[19];
#pragma unroll
  for (int j = 0; j < 8; j++) b[j] = dig[j];
#pragma unroll
  for (int j = 0; j < 5; j++) {
    b[8 + 2 * j] = (uint32_t)s[j];
    b[9 + 2 * j] = (uint32_t)(s[j] >> 32);
  }
  b[18] = 0u;
  // the body moved up by the prefix's length P = salt_len + 5 = 4 q + r octets: first by r octets …
  const uint32_t P = hp.salt_len + 5u, q = P >> 2, sh = 32u - 8u * (P & 3u);
  uint32_t c[19];
#pragma unroll
  for (int t = 0; t < 19; t++) {
    const unsigned long long two = ((unsigned long long)b[t] << 32) | (unsigned long long)(t ? b[t - 1] : 0u);
    c[t] = (uint32_t)(two >> sh);
  }
  // … then by q = 1..5 words (wave-uniform selects)
  const uint32_t L = P + 32u + (uint32_t)len;
#pragma unroll
  for (int j = 0; j < 24; j++) {
    uint32_t v = j < 6 ? hp.pre[j] : 0u;
#pragma unroll
    for (int qq = 1; qq <= 5; qq++)
      if (j - qq >= 0 && j - qq <= 18 && q == (uint32_t)qq) v |= c[j - qq];
    if ((L >> 2) == (uint32_t)j) v |= 0x80u << (8u * (L & 3u));
    M[j] = __builtin_bswap32(v);
  }
#pragma unroll
  for (int j = 24; j < 32; j++) M[j] = 0u;
  const bool two_blocks = L > 55u;
  if (two_blocks) M[31] = L * 8u;
  else M[15] = L * 8u;
  return two_blocks;
}

// u32le(SHA-256(message with i and level put in)[0:4])
__device__ __forceinline__ uint32_t casc_hash(const uint32_t M[32], bool two_blocks, uint32_t salt_len, uint32_t level, uint32_t i,
                                              const uint32_t* kc) {
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  uint32_t w[16];
  const uint32_t wi = salt_len >> 2, si = 24u - 8u * (salt_len & 3u);             // u32le(i): i < 256, one octet
  const uint32_t wl = (salt_len + 4u) >> 2, sl = 24u - 8u * ((salt_len + 4u) & 3u);  // u8(level)
#pragma unroll
  for (int j = 0; j < 16; j++) {
    uint32_t v = M[j];
    if (j < 6) {
      if (wi == (uint32_t)j) v |= i << si;
      if (wl == (uint32_t)j) v |= level << sl;
    }
    w[j] = v;
  }
  sha256_compress(h, w, kc);
  if (two_blocks) {
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = M[16 + j];
    sha256_compress(h, w, kc);
  }
  return __builtin_bswap32(h[0]);
}

// the round constants into LDS: every thread of a 256-thread block calls it
__device__ __forceinline__ void casc_constants(uint32_t* kc) {
  if (threadIdx.x < 64) kc[threadIdx.x] = K256[threadIdx.x];
  __syncthreads();
}

// One lane per record the layer holds: k hash functions, one relaxed atomicOr on a 32-bit word each.  A bad record is
// reported and sets nothing.
__global__ void __launch_bounds__(256) k_casc_insert(CascSrc c, uint64_t n, CascHash hp, CascLayer ly, uint32_t* err) {
  __shared__ uint32_t kc[64];
  casc_constants(kc);
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t bad = 0u;
  if (i < n) {
    uint32_t idx, ord;
    unsigned long long len, s[5];
    bad = casc_fetch(c, i, n, idx, ord, len, s);
    if (!bad) {
      uint32_t M[32];
      const bool two = casc_message(hp, c.dig + (uint64_t)ord * 8u, len, s, M);
      for (uint32_t f = 0; f < ly.k; f++) {
        const uint32_t bit = casc_hash(M, two, hp.salt_len, ly.level, f, kc) % ly.m;
        atomicOr(&ly.bits[bit >> 5], 1u << (bit & 31u));
      }
    }
  }
  known_report_bad(bad, err);
}

// One lane per record the layer is tested with: hash function f is computed only while all earlier bits were set; the
// record passes when all k are (k = 0: every valid record passes — the pass that only validates).  The flags go to
// block blk0 + blockIdx.x (known_flags_out).
__global__ void __launch_bounds__(256) k_casc_test(CascSrc c, uint64_t n, CascHash hp, CascLayer ly, KnownFlags fl, uint64_t blk0,
                                                   uint32_t* err) {
  __shared__ uint32_t kc[64];
  casc_constants(kc);
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t bad = 0u;
  bool pass = false;
  if (i < n) {
    uint32_t idx, ord;
    unsigned long long len, s[5];
    bad = casc_fetch(c, i, n, idx, ord, len, s);
    if (!bad) {
      uint32_t M[32];
      const bool two = casc_message(hp, c.dig + (uint64_t)ord * 8u, len, s, M);
      pass = true;
      for (uint32_t f = 0; f < ly.k && pass; f++) {
        const uint32_t bit = casc_hash(M, two, hp.salt_len, ly.level, f, kc) % ly.m;
        pass = (ly.bits[bit >> 5] >> (bit & 31u)) & 1u;
      }
    }
  }
  known_report_bad(bad, err);
  known_flags_out(pass, fl, blk0 + blockIdx.x);
}

// One lane per record of the run again, after the scan: a record whose flag is set goes to out[rank] as (record index,
// issuer ordinal).  No record is read.
__global__ void __launch_bounds__(256) k_casc_compact(CascSrc c, uint64_t n, KnownFlags fl, uint64_t blk0, uint2* out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  bool flag;
  const unsigned long long rank = known_flags_before(fl.ball, fl.cnt, (blk0 + blockIdx.x) * 256 + threadIdx.x, &flag);
  if (!flag) return;
  uint2 e;
  casc_locate(c, i, n, e.x, e.y);
  out[rank] = e;
}

// One lane per member record of the probe image's run (record dst[0] + i of the image answers in out[dst[0] + i]).  The
// layer table is walked by the whole wave, layer after layer (its loads are wave-uniform), while any lane is still
// passing; a lane stops hashing at its first unset bit.  A record that fails layer j + 1 after passing j layers is
// revoked iff j is odd; one that passes all of them iff their number is odd.
__global__ void __launch_bounds__(256) k_casc_query(CascSrc c, uint64_t n, CascHash hp, const CascLayer* layers, uint32_t n_layers,
                                                    uint8_t* out, uint32_t* err) {
  __shared__ uint32_t kc[64];
  casc_constants(kc);
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t bad = 0u, passed = 0u;
  uint32_t M[32];
  bool two = false, alive = false;
  if (i < n) {
    uint32_t idx, ord;
    unsigned long long len, s[5];
    bad = casc_fetch(c, i, n, idx, ord, len, s);
    if (!bad) {
      two = casc_message(hp, c.dig + (uint64_t)ord * 8u, len, s, M);
      alive = true;
    }
  }
  for (uint32_t l = 0; l < n_layers && __any(alive); l++) {
    const CascLayer ly = layers[l];
    if (alive) {
      for (uint32_t f = 0; f < ly.k && alive; f++) {
        const uint32_t bit = casc_hash(M, two, hp.salt_len, ly.level, f, kc) % ly.m;
        alive = (ly.bits[bit >> 5] >> (bit & 31u)) & 1u;
      }
      if (alive) passed++;
    }
  }
  if (i < n) out[c.g.dst[0] + i] = (uint8_t)(passed & 1u);
  known_report_bad(bad, err);
}

}  // namespace ctmr
