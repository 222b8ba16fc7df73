// kernels/merge.h — set algebra on known-certificate images (include/ctmr.h ctmr_known_merge*): union,
// minus and intersect of two images' member records, set by set, with no table behind them.  Both operands are
// CANONICAL when the rank pass runs — every set ascending in the order of kernels/sort.h, each member once — so a member
// is looked up in the partner set by a binary search and its place in the result is a sum of counts:
//   k_merge_ascending  is every record strictly above its predecessor in its set?  (then the operand is used where it lies)
//   k_merge_unique     after known_sort_sets: the records that differ from their predecessor or start a set (a bit per
//                      record, a count per block); k_merge_place<MERGE_OWN> squeezes the repeats out, k_merge_first
//                      gives the new first[] of the sets
//   k_merge_rank       one record per lane: lower bound and found bit in the partner set; the kept records as a bit per
//                      record and a count per 256-record block
//   k_merge_sets       per pair of sets the members the result holds
//   k_merge_place      the kept records to their places in the result (three 16-byte loads and stores)
// The kept records are the flags of a pass (KnownFlags, kernels/image.h), blocks numbered by blockIdx.x: "kept records
// before position q of an operand" is everywhere known_flags_before.
// gfx950 (CDNA4, wave64) only; plain vector loads and stores, LDS and global atomics.
#pragma once
#include "sort.h"

namespace ctmr {

// A key both images may hold a set under: the set's records in A and in B (a count of 0: the key is not there; the first
// is then where the set would lie).
struct MergePair {
  unsigned long long first_a, count_a, first_b, count_b;
};

// An operand as the kernels see it: n records, ns sets (first[0..ns], first[ns] = n), pair_of[s] = the pair of set s.
struct MergeSide {
  const uint8_t* rec;
  uint64_t n;
  const uint64_t* first;
  const uint32_t* pair_of;
  uint32_t ns;
  uint32_t is_b;  // 0: the records are A's (partner ranges: first_b / count_b), 1: B's
};

// bits[i >> 6] bit (i & 63) = record i is kept; base[blk] = kept records before block blk (256 records), base[nb] = all.
// bits has 4 (nb + 1) words and base nb + 1 entries, so q = n may be asked about.
__device__ __forceinline__ uint64_t merge_kept_before(const unsigned long long* bits, const unsigned long long* base, uint64_t q) {
  bool flag;
  return known_flags_before(bits, base, q, &flag);
}

// the set of record i of a side: its sets are one run from record 0 on (known_run_set, kernels/image.h)
__device__ __forceinline__ uint32_t merge_set_of(const MergeSide& s, uint64_t i) { return known_run_set(s.first, s.ns, i, s.n); }

// A record as the order compares it: the five octet words as big-endian numbers, then serial_len.
struct MergeKey {
  unsigned long long w[5], len;
};

__device__ __forceinline__ MergeKey merge_key(const uint8_t* rec, uint64_t i) {
  const uint4* p = (const uint4*)(rec + i * KNOWN_REC_BYTES);
  const uint4 v0 = p[0], v1 = p[1], v2 = p[2];
  MergeKey k;
  k.len = (unsigned long long)v0.x | ((unsigned long long)v0.y << 32);
  k.w[0] = __builtin_bswap64((unsigned long long)v0.z | ((unsigned long long)v0.w << 32));
  k.w[1] = __builtin_bswap64((unsigned long long)v1.x | ((unsigned long long)v1.y << 32));
  k.w[2] = __builtin_bswap64((unsigned long long)v1.z | ((unsigned long long)v1.w << 32));
  k.w[3] = __builtin_bswap64((unsigned long long)v2.x | ((unsigned long long)v2.y << 32));
  k.w[4] = __builtin_bswap64((unsigned long long)v2.z | ((unsigned long long)v2.w << 32));
  return k;
}

// record j of rec against k: -1 below, 0 equal, 1 above.  One 16-byte load {serial_len, octets 0..7} decides unless the
// first eight octets agree; the further words are fetched only then.
__device__ __forceinline__ int merge_compare(const uint8_t* rec, uint64_t j, const MergeKey& k) {
  const uint4* p = (const uint4*)(rec + j * KNOWN_REC_BYTES);
  const uint4 v0 = p[0];
  const unsigned long long w0 = __builtin_bswap64((unsigned long long)v0.z | ((unsigned long long)v0.w << 32));
  if (w0 != k.w[0]) return w0 < k.w[0] ? -1 : 1;
  const uint4 v1 = p[1];
  const unsigned long long w1 = __builtin_bswap64((unsigned long long)v1.x | ((unsigned long long)v1.y << 32));
  if (w1 != k.w[1]) return w1 < k.w[1] ? -1 : 1;
  const unsigned long long w2 = __builtin_bswap64((unsigned long long)v1.z | ((unsigned long long)v1.w << 32));
  if (w2 != k.w[2]) return w2 < k.w[2] ? -1 : 1;
  const uint4 v2 = p[2];
  const unsigned long long w3 = __builtin_bswap64((unsigned long long)v2.x | ((unsigned long long)v2.y << 32));
  if (w3 != k.w[3]) return w3 < k.w[3] ? -1 : 1;
  const unsigned long long w4 = __builtin_bswap64((unsigned long long)v2.z | ((unsigned long long)v2.w << 32));
  if (w4 != k.w[4]) return w4 < k.w[4] ? -1 : 1;
  const unsigned long long len = (unsigned long long)v0.x | ((unsigned long long)v0.y << 32);
  return len == k.len ? 0 : (len < k.len ? -1 : 1);
}

// Canonical check: *flag |= 1 when a record is not strictly above its predecessor in its set.  One atomicOr per wave
// that found one, like the bad-record report of k_known_count.
__global__ void __launch_bounds__(256) k_merge_ascending(MergeSide s, uint32_t* flag) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (i < s.n) {
    const uint32_t set = merge_set_of(s, i);
    if (i > s.first[set]) bad = merge_compare(s.rec, i - 1u, merge_key(s.rec, i)) >= 0;
  }
  const unsigned long long m = __ballot(bad);
  if (m && (threadIdx.x & 63u) == 0) atomicOr(flag, 1u);
}

// Behind known_sort_sets: the heads — records that start a set or differ from their predecessor — as kept records.
__global__ void __launch_bounds__(256) k_merge_unique(MergeSide s, unsigned long long* bits, unsigned long long* cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool head = false;
  if (i < s.n) {
    const uint32_t set = merge_set_of(s, i);
    head = i == s.first[set] || merge_compare(s.rec, i - 1u, merge_key(s.rec, i)) != 0;
  }
  known_flags_out(head, KnownFlags{bits, cnt}, blockIdx.x);
}

// … and the first record of every set once the repeats are gone (behind the exclusive scan of cnt[]); first[ns] too.
__global__ void __launch_bounds__(256) k_merge_first(const uint64_t* first, uint32_t ns, const unsigned long long* bits,
                                                     const unsigned long long* base, uint64_t* out) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s <= ns) out[s] = merge_kept_before(bits, base, first[s]);
}

// Rank pass over one operand: the lower bound of record i in its partner set (relative to the set's first record) and
// whether the partner holds it — a binary search that ends at once on an equal record, since the partner holds every
// member once.  lb (may be null: MINUS and INTERSECT need no places in the partner) and the kept records: keep_found =
// 1 keeps the records the partner holds (INTERSECT's A), 0 those it does not (MINUS's A, UNION's B).
__global__ void __launch_bounds__(256) k_merge_rank(MergeSide s, const MergePair* pairs, const uint8_t* partner,
                                                    uint32_t keep_found, uint32_t* lb, unsigned long long* bits,
                                                    unsigned long long* cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool keep = false;
  if (i < s.n) {
    const MergePair p = pairs[s.pair_of[merge_set_of(s, i)]];
    const uint64_t pf = s.is_b ? p.first_a : p.first_b;
    uint64_t lo = 0, hi = s.is_b ? p.count_a : p.count_b;
    bool found = false;
    if (hi) {
      const MergeKey k = merge_key(s.rec, i);
      while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        const int c = merge_compare(partner, pf + mid, k);
        if (c == 0) {
          found = true;
          lo = mid;
          break;
        }
        if (c < 0) lo = mid + 1u;
        else hi = mid;
      }
    }
    if (lb) lb[i] = (uint32_t)lo;
    keep = found == (keep_found != 0u);
  }
  if (bits) known_flags_out(keep, KnownFlags{bits, cnt}, blockIdx.x);
}

// The members the result holds per pair (behind the exclusive scan of the block counts): UNION all of A's and B's kept
// ones (bits / base: B's), MINUS and INTERSECT A's kept ones (bits / base: A's).
__global__ void __launch_bounds__(256) k_merge_sets(const MergePair* pairs, uint64_t np, uint32_t is_union,
                                                    const unsigned long long* bits, const unsigned long long* base,
                                                    unsigned long long* out) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= np) return;
  const MergePair p = pairs[j];
  if (is_union) out[j] = p.count_a + merge_kept_before(bits, base, p.first_b + p.count_b) - merge_kept_before(bits, base, p.first_b);
  else out[j] = merge_kept_before(bits, base, p.first_a + p.count_a) - merge_kept_before(bits, base, p.first_a);
}

// Place pass.  The sets of the result lie in the order of the pairs, as both operands' do, so a record's place is a sum
// over whole images and no base per set is needed:
//   MERGE_OWN      (MINUS, INTERSECT, the repeats of k_merge_unique)  kept record i → kept records of its side before i
//   MERGE_UNION_A  record i, every one kept → i + B's kept records before (its partner set's first + its lower bound)
//   MERGE_UNION_B  kept record j → B's kept records before j + (its partner set's first in A + its lower bound)
enum { MERGE_OWN = 0, MERGE_UNION_A = 1, MERGE_UNION_B = 2 };
template <int MODE>
__global__ void __launch_bounds__(256) k_merge_place(MergeSide s, const MergePair* pairs, const uint32_t* lb,
                                                     const unsigned long long* bits, const unsigned long long* base,
                                                     uint8_t* out, uint64_t cap) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= s.n) return;
  if (MODE != MERGE_UNION_A && !((bits[i >> 6] >> (i & 63u)) & 1ull)) return;
  uint64_t pos;
  if (MODE == MERGE_OWN) {
    pos = merge_kept_before(bits, base, i);
  } else {
    const MergePair p = pairs[s.pair_of[merge_set_of(s, i)]];
    if (MODE == MERGE_UNION_A) pos = i + merge_kept_before(bits, base, p.first_b + lb[i]);
    else pos = merge_kept_before(bits, base, i) + p.first_a + lb[i];
  }
  if (pos >= cap) return;  // (cannot happen: the caller sized `out` by the counts of the same bits)
  const uint4* src = (const uint4*)(s.rec + i * KNOWN_REC_BYTES);
  const uint4 a = src[0], b = src[1], c = src[2];
  uint4* o = (uint4*)(out + pos * KNOWN_REC_BYTES);
  o[0] = a;
  o[1] = b;
  o[2] = c;
}

}  // namespace ctmr
