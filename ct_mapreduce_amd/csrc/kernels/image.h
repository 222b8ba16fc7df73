// kernels/image.h — the known-certificate image (include/ctmr.h): bulk export of the live members of the
// table into 48-byte member records, and the passes that turn an image's member records back into key records for the
// owner-computes insert (exchange.h: k_keys_insert / k_keys_insert2 / k_keys_resolve).
// gfx950 (CDNA4, wave64) only; part of kernels.h, which includes the pieces in dependency order.
#pragma once
#include "misc.h"

namespace ctmr {

// A member record of the image: u64 serial_len (0..40) | serial octets zero-padded to 40 — what k_list writes.
constexpr uint32_t KNOWN_REC_BYTES = 48;

// Export, step 1: the non-empty (expDate, issuer) pairs with the pair-table slot each lives in:
// out[3k] = key, out[3k+1] = count, out[3k+2] = slot.
__global__ void __launch_bounds__(256) k_pairs_slots(const PairSlot* pairs, uint64_t npairs, unsigned long long* out,
                                                     uint64_t cap, unsigned long long* count) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= npairs) return;
  const unsigned long long k = pairs[j].key, c = pairs[j].count;
  if (k == 0ull || c == 0ull) return;
  const unsigned long long at = atomicAdd(count, 1ull);
  if (at >= cap) return;
  out[3 * at] = k;
  out[3 * at + 1] = c;
  out[3 * at + 2] = j;
}

// Export, step 2: one index word per lane.  A live, non-SHADOW word's cell is read (3 × 16 B: meta and the serial), its
// set found in the pair table (the probe pair_add makes), and its output position taken from the set's cursor — ONE
// atomicAdd per (wave, set): the lanes of a wave that hold members of one set share a ballot and take consecutive
// positions.  A large set (one issuer-hour of a big CA) otherwise puts every lane of the chip on one cursor.  The index
// is in hash order, so a wave of a table of many small sets meets up to 64 sets: after KNOWN_AGG_ROUNDS groups the
// lanes left over take their positions with one atomic each, in one instruction, instead of a serial loop.  The record
// goes out as three 16-byte stores.  Positions at or above `cap` are not written (a set outside the chunk being staged
// has its cursor parked far above: KNOWN_CURSOR_OFF).
constexpr unsigned long long KNOWN_CURSOR_OFF = 1ull << 62;
constexpr int KNOWN_AGG_ROUNDS = 4;
__global__ void __launch_bounds__(256) k_known_export(Table t, uint64_t nslots, const PairSlot* pairs, uint64_t pmask,
                                                      unsigned long long* cursor, uint8_t* out, uint64_t cap) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long w = j < nslots ? t.index[j] : 0ull;
  bool live = (w != 0ull) & (w != IDX_TOMB);
  uint4 c0 = make_uint4(0u, 0u, 0u, 0u), c1 = c0, c2 = c0;
  uint32_t slot = 0;
  if (live) {
    const uint4* src = (const uint4*)(t.arena + (w & REF_MASK));
    c0 = src[0];
    c1 = src[1];
    c2 = src[2];
    const unsigned long long meta = (unsigned long long)c0.x | ((unsigned long long)c0.y << 32);
    live = (meta & CELL_SHADOW) == 0ull;
    if (live) {
      const uint32_t canon = (uint32_t)(meta >> 32) & 0xffffffu;
      const unsigned long long key = ((unsigned long long)(canon + 1u) << 32) | (uint32_t)meta;
      uint64_t q = mixk(key) & pmask;
      live = false;
      for (uint64_t probes = 0; probes <= pmask; probes++) {
        const unsigned long long k = pairs[q].key;
        if (k == key) { live = true; slot = (uint32_t)q; break; }
        if (k == 0ull) break;  // (cannot happen: the pair table was built from this index)
        q = (q + 1) & pmask;
      }
      c0.x = (uint32_t)((meta >> 56) & 0x3full);  // the record's head: u64 serial_len, then the serial words
      c0.y = 0u;
    }
  }
  unsigned long long pos = ~0ull;
  unsigned long long todo = __ballot(live);
  for (int round = 0; todo && round < KNOWN_AGG_ROUNDS; round++) {
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t k = __shfl(slot, leader);
    const unsigned long long same = __ballot(live && slot == k) & todo;
    unsigned long long base = 0ull;
    if ((int)lane == leader) base = atomicAdd(&cursor[k], (unsigned long long)__popcll(same));
    base = __shfl(base, leader);
    if ((same >> lane) & 1ull) pos = base + (unsigned long long)__popcll(same & ((1ull << lane) - 1ull));
    todo &= ~same;
  }
  if ((todo >> lane) & 1ull) pos = atomicAdd(&cursor[slot], 1ull);  // the rest: many sets in one wave, one atomic each
  if (!live || pos >= cap) return;
  uint4* o = (uint4*)(out + pos * KNOWN_REC_BYTES);
  o[0] = c0;
  o[1] = c1;
  o[2] = c2;
}

// Import.  set_first[0..n_sets] (the last = the chunk's end) and set_meta[s] = key_meta(exp_hour, canon, 0) of the set,
// 0 when its issuer is not registered here (those members go to the host-side store).  Member i of the chunk belongs to
// the last set whose first member is <= i: every lane searches between the sets of its wave's first and last record.
__device__ __forceinline__ uint32_t known_set_of(const uint64_t* first, uint32_t lo, uint32_t hi, uint64_t i) {
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (first[mid] <= i) lo = mid;
    else hi = mid - 1u;
  }
  return lo;
}

// The same for the lane of a wave whose records are virtual records wfirst..wlast of first[0..n_sets]: the search is
// narrowed to the sets of the wave's first and last record, which every lane finds alike, and then made for the
// lane's own record v between the two.  The one segment search of the image's kernels.
__device__ __forceinline__ uint32_t known_set_in_wave(const uint64_t* first, uint32_t n_sets, uint64_t v, uint64_t wfirst,
                                                      uint64_t wlast) {
  const uint32_t s_lo = known_set_of(first, 0u, n_sets - 1u, wfirst);
  const uint32_t s_hi = known_set_of(first, s_lo, n_sets - 1u, wlast);
  return known_set_of(first, s_lo, s_hi, v);
}

// The run walk, the one copy of the image's kernels.  A launch of 256-thread blocks, one lane per
// record, covers the n records of k whole sets: first[0..k] ascending, first[0] = the run's first virtual record,
// first[k] = first[0] + n.  → the set of record i of the launch, which is virtual record first[0] + i: the wave's first
// and last record (the last wave of the launch ends at record n − 1), then known_set_in_wave.  Call with i < n.
__device__ __forceinline__ uint32_t known_run_set(const uint64_t* first, uint32_t k, uint64_t i, uint64_t n) {
  const uint64_t v0 = first[0], wi = i - (threadIdx.x & 63u);
  const uint64_t wfirst = v0 + wi, wlast = wi + 63u < n ? wfirst + 63u : v0 + n - 1u;
  return known_set_in_wave(first, k, v0 + i, wfirst, wlast);
}

// The segment table of a run: segment s holds the virtual records [dst[s], dst[s + 1]) (every segment non-empty) and
// lies at records [src[s], src[s] + dst[s + 1] − dst[s]) of recs — whole sets of an image where they lie, in another
// order or with sets left out in between.  A plain aggregate, passed by value as a kernel argument.
struct KnownSegs {
  const uint8_t* recs;
  const uint64_t* dst;  // k + 1
  const uint64_t* src;  // k
  uint32_t k;
  // record i of a launch of n (known_run_set) → its index in recs and, where the caller wants it, its segment
  __device__ __forceinline__ uint64_t index(uint64_t i, uint64_t n, uint32_t* set = nullptr) const {
    const uint32_t s = known_run_set(dst, k, i, n);
    if (set) *set = s;
    return src[s] + (dst[0] + i - dst[s]);
  }
  // … → the record
  __device__ __forceinline__ const uint4* at(uint64_t i, uint64_t n, uint32_t* set = nullptr) const {
    return (const uint4*)(recs + index(i, n, set) * KNOWN_REC_BYTES);
  }
};

// The flags of a pass, the one copy of the image's kernels: one bit per record and one count per block
// of 256 records.  Block b owns the four ballot words ball[4 b ..] and cnt[b] — its flagged records after the pass, the
// flagged records in front of it after the exclusive scan of cnt[].  A call of several runs numbers its blocks through
// all of them: a run of n records takes (n + 255) / 256 blocks from the blocks in front of it on.
struct KnownFlags {
  unsigned long long* ball;
  unsigned long long* cnt;
};

// v, a wave's total (lane 0's counts) → cnt[blk] = the sum over the block's four waves; → that sum, in thread 0 alone.
// Every thread of the block calls.
__device__ __forceinline__ uint32_t known_block_count(uint32_t v, unsigned long long* cnt, uint64_t blk) {
  __shared__ uint32_t ws[4];
  if ((threadIdx.x & 63u) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t total = 0u;
  if (threadIdx.x == 0) {
    total = ws[0] + ws[1] + ws[2] + ws[3];
    cnt[blk] = (unsigned long long)total;
  }
  return total;
}

// Leaves this wave's ballot and this block's count at block blk.  Every thread of the block calls.
__device__ __forceinline__ void known_flags_out(bool flag, const KnownFlags& f, uint64_t blk) {
  const unsigned long long m = __ballot(flag);
  if ((threadIdx.x & 63u) == 0) f.ball[blk * 4 + (threadIdx.x >> 6)] = m;
  known_block_count((uint32_t)__popcll(m), f.cnt, blk);
}

// The flagged records in front of record q (block q >> 8), after the scan: the block's base, the popcounts of the
// block's earlier words, and the bits of q's word below q.  *flag: q's own bit.  (q = all records may be asked about
// where ball has four words and cnt one entry more than the blocks.)
__device__ __forceinline__ unsigned long long known_flags_before(const unsigned long long* ball, const unsigned long long* cnt,
                                                                 uint64_t q, bool* flag) {
  const uint64_t blk = q >> 8, w = q >> 6;
  unsigned long long r = cnt[blk];
  for (uint64_t k = blk * 4u; k < w; k++) r += (unsigned long long)__popcll(ball[k]);
  const unsigned long long m = ball[w];
  *flag = (m >> (q & 63u)) & 1ull;
  return r + (unsigned long long)__popcll(m & ((1ull << (q & 63u)) - 1ull));
}

// A member record loaded (three 16-byte loads) and held to the rule that makes it valid: serial_len is
// at most 40 and the octets behind it are zero.  → 0 with len and the five serial words, or 1 for a serial_len above
// 40, 2 for padding that is not zero — the bits of the error word the calls report (known_report_bad).
__device__ __forceinline__ uint32_t known_load(const uint4* p, unsigned long long& len, unsigned long long s[5]) {
  const uint4 v0 = p[0], v1 = p[1], v2 = p[2];
  len = (unsigned long long)v0.x | ((unsigned long long)v0.y << 32);
  s[0] = (unsigned long long)v0.z | ((unsigned long long)v0.w << 32);
  s[1] = (unsigned long long)v1.x | ((unsigned long long)v1.y << 32);
  s[2] = (unsigned long long)v1.z | ((unsigned long long)v1.w << 32);
  s[3] = (unsigned long long)v2.x | ((unsigned long long)v2.y << 32);
  s[4] = (unsigned long long)v2.z | ((unsigned long long)v2.w << 32);
  if (len > CTMR_MAX_SERIAL) return 1u;
  uint32_t bad = 0u;
#pragma unroll
  for (uint32_t q = 0; q < 5; q++) {  // octets behind serial_len are zero
    const uint64_t lo = 8ull * q;
    const unsigned long long pad = len <= lo ? ~0ull : (len >= lo + 8 ? 0ull : (~0ull << (8ull * (len - lo))));
    if (s[q] & pad) bad = 2u;
  }
  return bad;
}

// The member record of the L <= 40 octets at m (any alignment; no octet at or beyond m + L is read) → record `at` of out:
// u64 serial_len, the octets, zeros to 48 bytes
__device__ __forceinline__ void known_store_octets(uint32_t L, const uint8_t* m, uint8_t* out, uint64_t at) {
  uint32_t w[10];
#pragma unroll
  for (uint32_t q = 0; q < 10; q++) {
    uint32_t v = 0u;
#pragma unroll
    for (uint32_t b = 0; b < 4; b++)
      if (4u * q + b < L) v |= (uint32_t)m[4u * q + b] << (8u * b);
    w[q] = v;
  }
  uint4* o = (uint4*)(out + at * KNOWN_REC_BYTES);
  o[0] = make_uint4(L, 0u, w[0], w[1]);
  o[1] = make_uint4(w[2], w[3], w[4], w[5]);
  o[2] = make_uint4(w[6], w[7], w[8], w[9]);
}

// What a wave saw of bad records (bad: known_load's result, 0 in a lane without a record) → *err, one atomicOr by
// lane 0 of a wave that saw one.  Every lane of the wave calls it.
__device__ __forceinline__ void known_report_bad(uint32_t bad, uint32_t* err) {
  const unsigned long long mb1 = __ballot(bad == 1u), mb2 = __ballot(bad == 2u);
  if ((threadIdx.x & 63u) == 0 && (mb1 | mb2)) atomicOr(err, (mb1 ? 1u : 0u) | (mb2 ? 2u : 0u));
}

struct KnownImportArgs {
  const uint8_t* members;      // the chunk's member records
  uint64_t n;                  // records in the chunk
  uint64_t base;               // image index of the chunk's first record (set_first is in image indices)
  const uint64_t* set_first;   // n_sets + 1
  const unsigned long long* set_meta;
  uint32_t n_sets, world, rank;
  unsigned long long* cnt;     // [0, nb): records of 1..20 octets taken per 256-record block, [nb, 2 nb): 21..40 octets
  uint64_t nb;
  uint32_t* err;               // bit 0: a serial_len above 40, bit 1: padding octets that are not zero
};

// The sets records [wfirst, wlast] of the chunk lie in: what every lane of a wave searches between.
__device__ __forceinline__ void known_set_span(const KnownImportArgs& a, uint64_t wfirst, uint64_t wlast, uint32_t& s_lo,
                                               uint32_t& s_hi) {
  s_lo = known_set_of(a.set_first, 0u, a.n_sets - 1u, a.base + wfirst);
  s_hi = known_set_of(a.set_first, s_lo, a.n_sets - 1u, a.base + wlast);
}

// class of record i: 0 = not taken here, 1 = a KeyRec32 (serial of at most 20 octets), 2 = a KeyRec (21..40)
// (call with i < a.n, its set among s_lo..s_hi; bad: as err)
__device__ __forceinline__ uint32_t known_record_in(const KnownImportArgs& a, uint64_t i, uint32_t s_lo, uint32_t s_hi,
                                                    unsigned long long& meta, unsigned long long s[5], uint32_t& bad) {
  bad = 0u;
  // (known_load defines the rule; the import, query and remove hot loops keep these loads of their own: EXPERIMENTS.md)
  const uint4* p = (const uint4*)(a.members + i * KNOWN_REC_BYTES);
  const uint4 v0 = p[0], v1 = p[1], v2 = p[2];
  const unsigned long long len = (unsigned long long)v0.x | ((unsigned long long)v0.y << 32);
  s[0] = (unsigned long long)v0.z | ((unsigned long long)v0.w << 32);
  s[1] = (unsigned long long)v1.x | ((unsigned long long)v1.y << 32);
  s[2] = (unsigned long long)v1.z | ((unsigned long long)v1.w << 32);
  s[3] = (unsigned long long)v2.x | ((unsigned long long)v2.y << 32);
  s[4] = (unsigned long long)v2.z | ((unsigned long long)v2.w << 32);
  if (len > CTMR_MAX_SERIAL) {
    bad = 1u;
    return 0u;
  }
#pragma unroll
  for (uint32_t q = 0; q < 5; q++) {  // octets behind serial_len are zero
    const uint64_t lo = 8ull * q;
    const unsigned long long pad = len <= lo ? ~0ull : (len >= lo + 8 ? 0ull : (~0ull << (8ull * (len - lo))));
    if (s[q] & pad) bad = 2u;
  }
  if (bad) return 0u;
  const uint32_t set = known_set_of(a.set_first, s_lo, s_hi, a.base + i);
  const unsigned long long sm = a.set_meta[set];
  if (sm == 0ull) return 0u;  // issuer not registered here: the host takes the set's members (world = 1 only)
  meta = sm | ((unsigned long long)len << 56);
  if (a.world > 1u && key_owner_h(key_hash(meta, s), a.world) != a.rank) return 0u;
  return len <= 20u ? 1u : 2u;
}

// … of a kernel that gives lane l of a wave record (wave's first + l)
__device__ __forceinline__ uint32_t known_record(const KnownImportArgs& a, uint64_t i, unsigned long long& meta,
                                                 unsigned long long s[5], uint32_t& bad) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wfirst = i - lane;
  const uint64_t wlast = (wfirst + 63u < a.n ? wfirst + 63u : a.n - 1u);
  uint32_t s_lo, s_hi;
  known_set_span(a, wfirst, wlast, s_lo, s_hi);
  return known_record_in(a, i, s_lo, s_hi, meta, s, bad);
}

// Count pass: validates every record and counts the taken ones per 256-record block, by class.
__global__ void __launch_bounds__(256) k_known_count(KnownImportArgs a) {
  __shared__ uint32_t wc[2][4];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  unsigned long long meta = 0ull, s[5];
  uint32_t bad = 0u;
  const uint32_t cls = i < a.n ? known_record(a, i, meta, s, bad) : 0u;
  const unsigned long long m1 = __ballot(cls == 1u), m2 = __ballot(cls == 2u), mb1 = __ballot(bad == 1u),
                           mb2 = __ballot(bad == 2u);
  if (lane == 0) {
    wc[0][wv] = (uint32_t)__popcll(m1);
    wc[1][wv] = (uint32_t)__popcll(m2);
    if (mb1 | mb2) atomicOr(a.err, (mb1 ? 1u : 0u) | (mb2 ? 2u : 0u));
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const uint32_t c = threadIdx.x;
    a.cnt[(uint64_t)c * a.nb + blockIdx.x] = (unsigned long long)(wc[c][0] + wc[c][1] + wc[c][2] + wc[c][3]);
  }
}

// Pack pass (behind the exclusive scan of cnt[]: base[blk] / base[nb + blk]; base[nb] = the 32-byte records in all): the
// taken records as KeyRec32 / KeyRec, each carrying its position as its order — the insert settles duplicates of one
// image by it, so exactly one presenter of a key is new.
__global__ void __launch_bounds__(256) k_known_pack(KnownImportArgs a, const unsigned long long* base, KeyRec32* out32,
                                                    KeyRec* out64) {
  __shared__ uint32_t wc[2][4];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  unsigned long long meta = 0ull, s[5];
  uint32_t bad = 0u;
  const uint32_t cls = i < a.n ? known_record(a, i, meta, s, bad) : 0u;
  const unsigned long long m1 = __ballot(cls == 1u), m2 = __ballot(cls == 2u);
  if (lane == 0) {
    wc[0][wv] = (uint32_t)__popcll(m1);
    wc[1][wv] = (uint32_t)__popcll(m2);
  }
  __syncthreads();
  if (cls == 0u) return;
  const uint32_t c = cls - 1u;
  uint64_t at = base[(uint64_t)c * a.nb + blockIdx.x];
  for (uint32_t k = 0; k < wv; k++) at += wc[c][k];
  at += (uint64_t)__popcll((c ? m2 : m1) & ((1ull << lane) - 1ull));
  const uint64_t n32 = base[a.nb];
  if (c == 0u) {
    uint4* o = (uint4*)(out32 + at);
    o[0] = make_uint4((uint32_t)meta, (uint32_t)(meta >> 32), (uint32_t)s[0], (uint32_t)(s[0] >> 32));
    o[1] = make_uint4((uint32_t)s[1], (uint32_t)(s[1] >> 32), (uint32_t)s[2], (uint32_t)at);
  } else {
    const uint64_t k = at - n32;  // the 64-byte records follow the 32-byte ones in base[]
    uint4* o = (uint4*)(out64 + k);
    o[0] = make_uint4((uint32_t)meta, (uint32_t)(meta >> 32), (uint32_t)s[0], (uint32_t)(s[0] >> 32));
    o[1] = make_uint4((uint32_t)s[1], (uint32_t)(s[1] >> 32), (uint32_t)s[2], (uint32_t)(s[2] >> 32));
    o[2] = make_uint4((uint32_t)s[3], (uint32_t)(s[3] >> 32), (uint32_t)s[4], (uint32_t)(s[4] >> 32));
    o[3] = make_uint4((uint32_t)k, 0u, (uint32_t)at, 0u);  // src, owner, pad = order
  }
}

// Bloom-variant engines: every imported key gets its filter bits, as a point insert (k_set_op) gives them.
template <class Rec>
__global__ void __launch_bounds__(256) k_known_bloom(const Rec* keys, uint64_t n, unsigned long long* bloom, uint64_t wmask) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const KeyView k = load_key(keys, i);
  uint64_t word;
  unsigned long long bits;
  bloom_pos(key_hash(k.meta, k.s), wmask, word, bits);
  atomicOr(&bloom[word], bits);
}

// ---- bulk SetContains / SetRemove over an image's member records.  A taken record costs a chain of two
// dependent random reads — its index word, then on a tag match 48 of the cell's 64 bytes — and nothing else, so the time
// is memory latency ÷ reads in flight: every lane takes R CONSECUTIVE records and the probe advances all of them in
// rounds — the index words of every record still probing are requested before the first is looked at, then the cells of
// those whose tag matched.  A round is one step of index_upsert(insert = false): an empty word ends the probe (absent), a
// tombstone or another key is stepped over.  Records that are not taken (another rank's, an unregistered issuer's, a bad
// one) make no table access.
//   res[k]  0 = absent (remove: nothing removed), 1 = present (remove: this record removed it), 2 = not taken
//   dec[k]  remove: the canonical issuer whose counter goes down for record k, ~0u when none does (nothing removed, or
//           a SHADOW cell: counted by another rank)
// REMOVE: atomicCAS(word, the live word observed, IDX_TOMB) — of two presenters of one key exactly one sees its word.
template <int R, bool REMOVE>
__device__ __forceinline__ void known_probe(const KnownImportArgs& a, const Table& t, uint64_t i0, uint32_t nvalid,
                                            uint32_t (&res)[R], uint32_t (&dec)[R], uint32_t& bad) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wfirst = i0 - (uint64_t)lane * R;
  uint32_t s_lo = 0u, s_hi = 0u;
  if (wfirst < a.n) known_set_span(a, wfirst, wfirst + 64u * R <= a.n ? wfirst + 64u * R - 1u : a.n - 1u, s_lo, s_hi);
  unsigned long long meta[R], s[R][5];
  uint32_t tag[R], j[R], act = 0u;
  bad = 0u;
#pragma unroll
  for (int k = 0; k < R; k++) {
    res[k] = 2u;
    dec[k] = ~0u;
    meta[k] = 0ull;
    tag[k] = j[k] = 0u;
    if ((uint32_t)k < nvalid) {
      uint32_t b;
      if (known_record_in(a, i0 + k, s_lo, s_hi, meta[k], s[k], b)) {
        const unsigned long long h = key_hash(meta[k], s[k]);
        tag[k] = key_tag(h);
        j[k] = (uint32_t)(h & t.mask);  // (at most 2^31 slots)
        res[k] = 0u;
        act |= 1u << k;
      }
      bad |= b;
    }
  }
  for (uint64_t round = 0; act && round <= t.mask; round++) {
    unsigned long long w[R];
#pragma unroll
    for (int k = 0; k < R; k++)
      if ((act >> k) & 1u) w[k] = REMOVE ? ld_agent(&t.index[j[k]]) : t.index[j[k]];
    uint32_t cmp = 0u;
#pragma unroll
    for (int k = 0; k < R; k++)
      if ((act >> k) & 1u) {
        if (w[k] == 0ull) act &= ~(1u << k);
        else if (w[k] != IDX_TOMB && (uint32_t)(w[k] >> 40) == tag[k]) cmp |= 1u << k;
      }
    uint4 c0[R], c1[R], c2[R];
#pragma unroll
    for (int k = 0; k < R; k++)
      if ((cmp >> k) & 1u) {
        const uint4* c = (const uint4*)(t.arena + (w[k] & REF_MASK));
        c0[k] = c[0];
        c1[k] = c[1];
        c2[k] = c[2];
      }
#pragma unroll
    for (int k = 0; k < R; k++)
      if ((cmp >> k) & 1u) {
        const unsigned long long cm = (unsigned long long)c0[k].x | ((unsigned long long)c0[k].y << 32);
        const bool eq = ((cm & ~CELL_SHADOW) == meta[k]) &
                        (((unsigned long long)c0[k].z | ((unsigned long long)c0[k].w << 32)) == s[k][0]) &
                        (((unsigned long long)c1[k].x | ((unsigned long long)c1[k].y << 32)) == s[k][1]) &
                        (((unsigned long long)c1[k].z | ((unsigned long long)c1[k].w << 32)) == s[k][2]) &
                        (((unsigned long long)c2[k].x | ((unsigned long long)c2[k].y << 32)) == s[k][3]) &
                        (((unsigned long long)c2[k].z | ((unsigned long long)c2[k].w << 32)) == s[k][4]);
        if (eq) {
          act &= ~(1u << k);
          if constexpr (REMOVE) {
            if (atomicCAS(&t.index[j[k]], w[k], IDX_TOMB) == w[k]) {
              res[k] = 1u;
              if ((cm & CELL_SHADOW) == 0ull) dec[k] = (uint32_t)(meta[k] >> 32) & 0xffffffu;
            }
          } else {
            res[k] = 1u;
          }
        }
      }
#pragma unroll
    for (int k = 0; k < R; k++)
      if ((act >> k) & 1u) j[k] = (uint32_t)probe_next(j[k], round, t.mask);
  }
}

// Query: flags[i] = res of record i.  A lane's R flags are adjacent: one 1-, 2-, 4- or 8-byte store per lane (bytes at
// the ragged end of the chunk and under a flags pointer that is not R-aligned).  cnt[blk] = records taken,
// cnt[nb + blk] = taken records found, per block of 256 R records; errors as k_known_count reports them.
template <int R>
__global__ void __launch_bounds__(256) k_known_query(KnownImportArgs a, Table t, uint8_t* flags) {
  __shared__ uint32_t wc[2][4];
  const uint64_t i0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * R;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t nvalid = i0 >= a.n ? 0u : (a.n - i0 >= (uint64_t)R ? (uint32_t)R : (uint32_t)(a.n - i0));
  uint32_t res[R], dec[R], bad;
  known_probe<R, false>(a, t, i0, nvalid, res, dec, bad);
  uint8_t* out = flags + i0;
  if (nvalid == (uint32_t)R && ((uintptr_t)out & (uintptr_t)(R - 1)) == 0) {
    uint32_t lo = 0u, hi = 0u;
#pragma unroll
    for (int k = 0; k < R; k++) {
      if (k < 4) lo |= res[k] << (8 * k);
      else hi |= res[k] << (8 * (k - 4));
    }
    if constexpr (R == 1) out[0] = (uint8_t)lo;
    else if constexpr (R == 2) *(uint16_t*)out = (uint16_t)lo;
    else if constexpr (R == 4) *(uint32_t*)out = lo;
    else *(uint2*)out = make_uint2(lo, hi);
  } else {
#pragma unroll
    for (int k = 0; k < R; k++)
      if ((uint32_t)k < nvalid) out[k] = (uint8_t)res[k];
  }
  uint32_t n_taken = 0u, n_hit = 0u;
#pragma unroll
  for (int k = 0; k < R; k++) {
    n_taken += (uint32_t)__popcll(__ballot(res[k] != 2u));
    n_hit += (uint32_t)__popcll(__ballot(res[k] == 1u));
  }
  const unsigned long long mb1 = __ballot((bad & 1u) != 0u), mb2 = __ballot((bad & 2u) != 0u);
  if (lane == 0) {
    wc[0][wv] = n_taken;
    wc[1][wv] = n_hit;
    if (mb1 | mb2) atomicOr(a.err, (mb1 ? 1u : 0u) | (mb2 ? 2u : 0u));
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const uint32_t c = threadIdx.x;
    a.cnt[(uint64_t)c * a.nb + blockIdx.x] = (unsigned long long)(wc[c][0] + wc[c][1] + wc[c][2] + wc[c][3]);
  }
}

// Remove (behind k_known_count, which has validated every record of the image): cnt[blk] = members removed per block.
// The per-issuer counters go down by ONE atomic per (wave, canonical issuer): the match loop of wave_agg_add over the
// wave's 64 R (lane, record) pairs — the records of a wave lie in one or two sets, so it runs once or twice.
template <int R>
__global__ void __launch_bounds__(256) k_known_remove(KnownImportArgs a, Table t, unsigned long long* issuer_counts) {
  __shared__ uint32_t wc[4];
  const uint64_t i0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * R;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t nvalid = i0 >= a.n ? 0u : (a.n - i0 >= (uint64_t)R ? (uint32_t)R : (uint32_t)(a.n - i0));
  uint32_t res[R], dec[R], bad;
  known_probe<R, true>(a, t, i0, nvalid, res, dec, bad);
  uint32_t n_hit = 0u;
  unsigned long long todo[R];
#pragma unroll
  for (int k = 0; k < R; k++) {
    n_hit += (uint32_t)__popcll(__ballot(res[k] == 1u));
    todo[k] = __ballot(dec[k] != ~0u);
  }
#pragma unroll
  for (int k = 0; k < R; k++)
    while (todo[k]) {
      const int leader = __ffsll((long long)todo[k]) - 1;
      const uint32_t c = __shfl(dec[k], leader);
      uint32_t tot = 0u;
#pragma unroll
      for (int q = 0; q < R; q++) {
        const unsigned long long same = __ballot(dec[q] == c) & todo[q];
        tot += (uint32_t)__popcll(same);
        todo[q] &= ~same;
      }
      if ((int)lane == leader) atomicAdd(&issuer_counts[c], (unsigned long long)-(long long)tot);
    }
  if (lane == 0) wc[wv] = n_hit;
  __syncthreads();
  if (threadIdx.x == 0) a.cnt[blockIdx.x] = (unsigned long long)(wc[0] + wc[1] + wc[2] + wc[3]);
}

}  // namespace ctmr
