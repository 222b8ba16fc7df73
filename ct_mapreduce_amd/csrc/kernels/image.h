// kernels/image.h — the known-certificate image (include/ctmr.h): bulk export of the live members of the
// table into 48-byte member records, and the passes that turn an image's member records back into key records for the
// owner-computes insert (exchange.h: k_keys_insert / k_keys_insert2 / k_keys_resolve).
// gfx950 (CDNA4, wave64) only; part of kernels.h, which includes the pieces in dependency order.
#pragma once
#include "misc.h"

namespace ctmr {

// A member record of the image: u64 serial_len (0..40) | serial octets zero-padded to 40 — what k_list writes.
constexpr uint32_t KNOWN_REC_BYTES = 48;

// Export, step 1: the non-empty (expDate, issuer) pairs with the pair-table slot each lives in (k_pairs + the slot):
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

// class of record i: 0 = not taken here, 1 = a KeyRec32 (serial of at most 20 octets), 2 = a KeyRec (21..40)
// (call with i < a.n; bad: as err)
__device__ __forceinline__ uint32_t known_record(const KnownImportArgs& a, uint64_t i, unsigned long long& meta,
                                                 unsigned long long s[5], uint32_t& bad) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wfirst = i - lane;
  const uint64_t wlast = (wfirst + 63u < a.n ? wfirst + 63u : a.n - 1u);
  const uint32_t s_lo = known_set_of(a.set_first, 0u, a.n_sets - 1u, a.base + wfirst);
  const uint32_t s_hi = known_set_of(a.set_first, s_lo, a.n_sets - 1u, a.base + wlast);
  bad = 0u;
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

}  // namespace ctmr
