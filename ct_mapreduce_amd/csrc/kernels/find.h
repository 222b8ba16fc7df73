// kernels/find.h — serials looked up in a known image whatever their expiration date (include/ctmr.h
// ctmr_known_image_find*).  The probes (the small side) go into an open-addressed table of 8-byte words
// that stays in cache (k_find_build); the member records of the known image's kept sets (the large side) are streamed
// once where they lie and walked against it (k_find_scan); a finish pass turns the working hits into the caller's
// (k_find_finish).  No sort, no staging of the image, no table of the engine.
// gfx950 (CDNA4, wave64) only; part of kernels.h, which includes the pieces in dependency order.
#pragma once
#include "lists.h"

namespace ctmr {

constexpr uint32_t FIND_NO_ISSUER = 0xffffffffu;  // a probe whose Issuer.ID the known image does not name

// What is hashed and compared besides the serial words: the K ordinal of the Issuer.ID and the serial's length — a
// key_meta of hour 0, with all 32 bits of the ordinal.
__device__ __forceinline__ unsigned long long find_meta(uint32_t kord, unsigned long long len) {
  return (len << 56) | (unsigned long long)kord;
}

// The probes: P's member records where they lie, then n_extra records of the call's own — the members of P's host
// section that a member record of K can equal (at most 40 octets, an Issuer.ID K names).  Probe i < n_main belongs to
// the last set of P whose first member is <= i.
struct FindProbes {
  const uint8_t* recs;         // n_main records
  const uint8_t* extra;        // n_extra records
  const uint32_t* extra_kord;  // the K ordinal of each
  const uint64_t* set_first;   // n_sets + 1
  const uint32_t* set_kord;    // per set of P: the K ordinal of its issuer (P ordinal → K ordinal, looked up per set)
  uint64_t n_main, n_extra;
  uint32_t n_sets;
  __device__ __forceinline__ const uint4* rec(uint64_t i) const {
    return (const uint4*)(i < n_main ? recs + i * KNOWN_REC_BYTES : extra + (i - n_main) * KNOWN_REC_BYTES);
  }
};

// The probe table: words of tag (24 bits, key_tag) | probe index + 1 (40 bits); 0 = empty.  mask + 1 is a power of two
// above the number of probes, so every chain ends at an empty word.
struct FindTable {
  unsigned long long* words;
  uint64_t mask;
};

// One lane per probe.  The working hit of the probe is initialised — records 0, first_hour INT32_MAX, last_hour
// INT32_MIN, and in the reserved word the probe's K ordinal, which k_find_scan compares and k_find_finish clears — and
// the probe claims the first empty word from its home slot on (atomicCAS, linear).  Equal probes take one word each.
// A bad record (known_load; reported in *err) and a probe whose issuer K does not name are not inserted.
__global__ void __launch_bounds__(256) k_find_build(FindProbes p, FindTable t, uint4* hits, uint32_t* err) {
  const uint64_t n = p.n_main + p.n_extra;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t bad = 0u;
  if (i < n) {
    unsigned long long len, s[5];
    bad = known_load(p.rec(i), len, s);
    uint32_t kord = FIND_NO_ISSUER;
    if (i < p.n_main) {
      kord = p.set_kord[known_run_set(p.set_first, p.n_sets, i, p.n_main)];
    } else {
      kord = p.extra_kord[i - p.n_main];
    }
    if (bad) kord = FIND_NO_ISSUER;
    hits[i] = make_uint4(0u, 0x7fffffffu, 0x80000000u, kord);
    if (kord != FIND_NO_ISSUER) {
      const unsigned long long h = key_hash(find_meta(kord, len), s);
      const unsigned long long word = ((unsigned long long)key_tag(h) << 40) | (i + 1ull);
      uint64_t j = h & t.mask;
      for (uint64_t k = 0; k <= t.mask; k++) {
        if (atomicCAS(&t.words[j], 0ull, word) == 0ull) break;
        j = (j + 1ull) & t.mask;
      }
    }
  }
  known_report_bad(bad, err);
}

// A run of k whole kept sets of K: the segment table (KnownSegs, kernels/image.h) and per segment its set's hour and
// K ordinal.
struct FindSegs : KnownSegs {
  const int32_t* hour;   // k
  const uint32_t* kord;  // k
};

// One lane per member record of the run: three 16-byte loads (a wave reads 3 KiB in a row), the record validated
// (known_load), then the walk from its home slot to the first empty word.  A word of the record's tag
// names a probe below `limit` whose 48 bytes and K ordinal are compared in full; an equal one gets records + 1 and the
// set's hour into first_hour / last_hour.  A record that matches nothing reads one table word.
__global__ void __launch_bounds__(256) k_find_scan(FindSegs g, uint64_t n, FindTable t, FindProbes p, uint64_t limit, uint4* hits,
                                                   uint32_t* err) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t bad = 0u;
  if (i < n) {
    uint32_t set;
    unsigned long long len, s[5];
    bad = known_load(g.at(i, n, &set), len, s);
    if (!bad) {
      const uint32_t kord = g.kord[set];
      const int32_t hour = g.hour[set];
      const unsigned long long h = key_hash(find_meta(kord, len), s);
      const unsigned long long tag = (unsigned long long)key_tag(h);
      uint64_t j = h & t.mask;
      for (uint64_t k = 0; k <= t.mask; k++) {
        const unsigned long long w = t.words[j];
        if (w == 0ull) break;
        const uint64_t pi = (w & REF_MASK) - 1ull;
        if ((w >> 40) == tag && pi < limit) {
          unsigned long long plen, ps[5];
          known_load(p.rec(pi), plen, ps);
          const bool eq = (hits[pi].w == kord) & (plen == len) & (ps[0] == s[0]) & (ps[1] == s[1]) & (ps[2] == s[2]) &
                          (ps[3] == s[3]) & (ps[4] == s[4]);
          if (eq) {
            atomicAdd(&hits[pi].x, 1u);
            atomicMin((int*)&hits[pi].y, hour);
            atomicMax((int*)&hits[pi].z, hour);
          }
        }
        j = (j + 1ull) & t.mask;
      }
    }
  }
  known_report_bad(bad, err);
}

// The working hits → the caller's (in place when out == in): the hours of a probe without a record become 0, the
// reserved word 0; cnt[blk] = the block's probes with records > 0.
__global__ void __launch_bounds__(256) k_find_finish(const uint4* in, uint4* out, uint64_t n, unsigned long long* cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool found = false;
  if (i < n) {
    const uint4 h = in[i];
    found = h.x != 0u;
    out[i] = found ? make_uint4(h.x, h.y, h.z, 0u) : make_uint4(0u, 0u, 0u, 0u);
  }
  known_block_count((uint32_t)__popcll(__ballot(found)), cnt, blockIdx.x);
}

}  // namespace ctmr
