// kernels/split.h — a known image partitioned by a probe image, the hour as wildcard (include/ctmr.h
// ctmr_known_image_split*): the member records of K's kept sets that equal a probe go to one image, the
// others to a second one, both in K's order.  The probes are find.h's table (k_find_build, unchanged); the records are
// streamed twice: k_split_mark walks each against the table and leaves the flags of the pass (KnownFlags,
// kernels/image.h); after a scan of the counts k_split_place copies each record to its rank among the hits or
// among the misses, and k_split_sets says how many hits lie in front of every kept set.  One stable compaction over the
// virtual sequence of the kept sets is the per-set layout, because kept sets are contiguous there.
// No cross-workgroup publish, no spin-wait; the only global atomic is the bad-record report (known_report_bad).
// gfx950 (CDNA4, wave64) only; part of kernels.h, which includes the pieces in dependency order.
#pragma once
#include "find.h"

namespace ctmr {

// One lane per member record of the run (KnownSegs::at): three 16-byte loads, the record
// validated (known_load), then the walk from its home slot to the first empty word.  At the first probe below `limit`
// that is equal in full (48 bytes and K ordinal) the flag is set and the walk stops.  A record that matches nothing
// reads one table word.  hits: the working hits k_find_build wrote, read for the probes' K ordinals only.
__global__ void __launch_bounds__(256) k_split_mark(FindSegs g, uint64_t n, FindTable t, FindProbes p, uint64_t limit, const uint4* hits,
                                                    KnownFlags f, uint64_t blk0, uint32_t* err) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t bad = 0u;
  bool found = false;
  if (i < n) {
    uint32_t set;
    unsigned long long len, s[5];
    bad = known_load(g.at(i, n, &set), len, s);
    if (!bad) {
      const uint32_t kord = g.kord[set];
      const unsigned long long h = key_hash(find_meta(kord, len), s);
      const unsigned long long tag = (unsigned long long)key_tag(h);
      uint64_t j = h & t.mask;
      for (uint64_t k = 0; k <= t.mask && !found; k++) {
        const unsigned long long w = t.words[j];
        if (w == 0ull) break;
        const uint64_t pi = (w & REF_MASK) - 1ull;
        if ((w >> 40) == tag && pi < limit) {
          unsigned long long plen, ps[5];
          known_load(p.rec(pi), plen, ps);
          found = (hits[pi].w == kord) & (plen == len) & (ps[0] == s[0]) & (ps[1] == s[1]) & (ps[2] == s[2]) & (ps[3] == s[3]) &
                  (ps[4] == s[4]);
        }
        j = (j + 1ull) & t.mask;
      }
    }
  }
  known_report_bad(bad, err);
  known_flags_out(found, f, blk0 + blockIdx.x);
}

// One lane per record of the run again: virtual record v with `rank` hits in front of it goes to hit[rank] when its
// flag is set, else to miss[v − rank], as three 16-byte stores.  A side that is null is not stored.
__global__ void __launch_bounds__(256) k_split_place(FindSegs g, uint64_t n, KnownFlags f, uint64_t blk0, uint8_t* hit, uint8_t* miss) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint4* src = g.at(i, n);
  bool flag;
  const unsigned long long rank = known_flags_before(f.ball, f.cnt, (blk0 + blockIdx.x) * 256 + threadIdx.x, &flag);
  uint8_t* side = flag ? hit : miss;
  if (!side) return;
  const uint4 c0 = src[0], c1 = src[1], c2 = src[2];
  uint4* o = (uint4*)(side + (flag ? rank : g.dst[0] + i - rank) * KNOWN_REC_BYTES);
  o[0] = c0;
  o[1] = c1;
  o[2] = c2;
}

// One lane per kept set of the run: before[s] = the hits in front of the set's first virtual record.  The host takes
// both results' counts and first members from these and the total.
__global__ void __launch_bounds__(256) k_split_sets(FindSegs g, KnownFlags f, uint64_t blk0, unsigned long long* before) {
  const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= g.k) return;
  bool flag;
  before[s] = known_flags_before(f.ball, f.cnt, blk0 * 256 + (g.dst[s] - g.dst[0]), &flag);
}

}  // namespace ctmr
