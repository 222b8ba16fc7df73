// kernels/resp.h — the Redis protocol stream of a known-certificate image (include/ctmr.h ctmr_known_image_resp*,
// DESIGN.md §18): per set the SADD commands of its member records, at most `per` members each, and the EXPIREAT
// KnownCertificates.setExpiryFlag puts on the key.  The stream is in key order, which is the image's own set order: the
// records are read where they lie, record i of a launch next to record i + 1.  A count pass (validates every record;
// per-block byte totals, then scan_u64) and a write pass that stages each block's text in LDS and
// stores it with 16-byte stores between two ragged ends, as lists_write_body does.
// The text of the record at position p of a set of c records:
//   p % per == 0      "*<argc>\r\n$4\r\nSADD\r\n$68\r\n<key>\r\n", argc = min(per, c − p) + 2
//   always            "$<L>\r\n<the L octets>\r\n"
//   p == c − 1        "*3\r\n$8\r\nEXPIREAT\r\n$68\r\n<key>\r\n$<len t>\r\n<t>\r\n", t = hour × 3600 in decimal — unless the
//                     key has host-section members too: then the host writes it behind them
// <key> = "serials::" ExpDate.ID(hour) "::" Issuer.ID, always 68 octets: the date is formatted here, the 44 characters of
// the ID come from a table the host encoded once per issuer.
// gfx950 (CDNA4, wave64) only; part of kernels.h, which includes the pieces in dependency order.
#pragma once
#include "image.h"

namespace ctmr {

constexpr uint32_t RESP_BLOCK = 256;
constexpr uint32_t RESP_KEY = 68, RESP_ID = 44, RESP_ID_ROW = 48;
// a one-member set with a 40-octet serial and a 12-character timestamp: 89 (SADD header) + 47 + 112 (EXPIREAT)
constexpr uint32_t RESP_REC_MAX = 248;
// The write pass stages a block's whole text in LDS.  256 worst records are 63 488 B, 256 records of 24 B (a 16-octet serial
// inside a command) 6 KiB: the count pass reports the largest block text of the launch, and the write pass is launched
// with that much dynamic LDS (RESP_LDS_FIXED more for the scan's words and the phase) — the occupancy the data allows.
constexpr uint32_t RESP_LDS_FIXED = 16 + 16;
__host__ __device__ constexpr uint32_t resp_lds_bytes(uint32_t max_block_text) { return RESP_LDS_FIXED + ((max_block_text + 15u) & ~15u); }
constexpr unsigned long long RESP_NO_EXPIRE = 1ull << 63;

// A launch covers the n records of k whole sets: set s holds the image's records [first[s], first[s + 1]) (first[0] = the
// launch's first record, recs points at it; the set of record i: known_run_set, kernels/image.h), meta[s] = (uint32_t)hour | ordinal << 32 | RESP_NO_EXPIRE.
struct RespArgs {
  const uint8_t* recs;
  const uint64_t* first;            // k + 1
  const unsigned long long* meta;   // k
  const uint8_t* ids;               // RESP_ID_ROW bytes per ordinal: the 44 characters of its Issuer.ID, then zeros
  uint32_t k, per;
};

// decimal digits of v (at most 12: |hour × 3600| of the years 0000..9999)
__device__ __forceinline__ uint32_t resp_digits(unsigned long long v) {
  uint32_t d = 1u;
  unsigned long long p = 10ull;
#pragma unroll
  for (int k = 0; k < 11; k++) {
    d += v >= p ? 1u : 0u;
    p *= 10ull;
  }
  return d;
}

// What record i of a set contributes besides its bulk string.
struct RespRec {
  uint32_t argc;             // != 0: it opens a SADD command of argc arguments
  bool expire;               // it is the set's last and the EXPIREAT follows it
  bool neg;
  unsigned long long t;      // |hour × 3600|
  int32_t hour;
  uint32_t ordinal;
};

__device__ __forceinline__ RespRec resp_rec(const RespArgs& a, uint32_t s, uint64_t i) {
  const uint64_t first = a.first[s], p = a.first[0] + i - first, c = a.first[s + 1] - first;
  const unsigned long long m = a.meta[s];
  RespRec r;
  r.hour = (int32_t)(uint32_t)m;
  r.ordinal = (uint32_t)(m >> 32) & 0x7fffffffu;
  const uint32_t per = a.per;
  const bool opens = (per & (per - 1u)) == 0u ? (p & (uint64_t)(per - 1u)) == 0ull
                                              : (p <= 0xffffffffull ? (uint32_t)p % per == 0u : p % per == 0ull);
  r.argc = opens ? (uint32_t)(c - p < per ? c - p : per) + 2u : 0u;
  r.expire = p == c - 1u && !(m & RESP_NO_EXPIRE);
  const long long t = (long long)r.hour * 3600ll;
  r.neg = t < 0;
  r.t = (unsigned long long)(t < 0 ? -t : t);
  return r;
}

// the text bytes of a record of serial_len len
__device__ __forceinline__ uint32_t resp_rec_bytes(const RespRec& r, uint32_t len) {
  uint32_t b = 5u + (len >= 10u ? 2u : 1u) + len;
  if (r.argc) b += 13u + resp_digits(r.argc) + 7u + RESP_KEY;
  if (r.expire) {
    const uint32_t tl = resp_digits(r.t) + (r.neg ? 1u : 0u);
    b += 18u + 7u + RESP_KEY + 5u + (tl >= 10u ? 2u : 1u) + tl;
  }
  return b;
}

// Count pass: cnt[blk] = the text bytes of the launch's records [256 blk, 256 blk + 256), and every record is validated
// (known_load) and a bad one reported in err[0] (known_report_bad).  err[1] = the largest cnt[blk] of the launch (the
// write pass's LDS): an atomicMax by the blocks that raise it.
__global__ void __launch_bounds__(RESP_BLOCK) k_image_resp_count(RespArgs a, uint64_t n, unsigned long long* cnt, uint32_t* err) {
  const uint64_t i = (uint64_t)blockIdx.x * RESP_BLOCK + threadIdx.x;
  uint32_t b = 0u, bad = 0u;
  if (i < n) {
    unsigned long long len, s[5];
    bad = known_load((const uint4*)(a.recs + i * KNOWN_REC_BYTES), len, s);
    const uint32_t l = (uint32_t)(len < (unsigned long long)CTMR_MAX_SERIAL ? len : (unsigned long long)CTMR_MAX_SERIAL);
    b = resp_rec_bytes(resp_rec(a, known_run_set(a.first, a.k, i, n), i), l);
  }
  known_report_bad(bad, err);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) b += __shfl_xor(b, d);
  const uint32_t total = known_block_count(b, cnt, blockIdx.x);
  // (every block's atomic on the one word would serialise: only a block above what the word held a moment ago tries)
  if (threadIdx.x == 0 && total > __hip_atomic_load(err + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(err + 1, total);
}

// v in decimal, nd = resp_digits(v) of them → behind the last
__device__ __forceinline__ uint8_t* resp_put_dec(uint8_t* t, unsigned long long v, uint32_t nd) {
  for (uint32_t k = nd; k-- > 0u;) {
    t[k] = (uint8_t)('0' + (uint32_t)(v % 10ull));
    v /= 10ull;
  }
  return t + nd;
}

__device__ __forceinline__ uint8_t* resp_put_dec32(uint8_t* t, uint32_t v, uint32_t nd) {
  for (uint32_t k = nd; k-- > 0u;) {
    t[k] = (uint8_t)('0' + v % 10u);
    v /= 10u;
  }
  return t + nd;
}

template <uint32_t N>
__device__ __forceinline__ uint8_t* resp_put_str(uint8_t* t, const char (&s)[N]) {
#pragma unroll
  for (uint32_t k = 0; k + 1u < N; k++) t[k] = (uint8_t)s[k];
  return t + (N - 1u);
}

__device__ __forceinline__ uint8_t* resp_put_2(uint8_t* t, uint32_t v) {  // two digits
  t[0] = (uint8_t)('0' + v / 10u);
  t[1] = (uint8_t)('0' + v % 10u);
  return t + 2;
}

// "$68\r\nserials::YYYY-MM-DD-HH::<Issuer.ID>\r\n": civil_from_days (synth.h) in 32-bit arithmetic, hours of the years
// 0000..9999 only (the host refuses any other before the first launch)
__device__ __forceinline__ uint8_t* resp_put_key(uint8_t* t, int32_t hour, const uint8_t* id) {
  int32_t days = hour / 24, hh = hour % 24;
  if (hh < 0) {
    hh += 24;
    days -= 1;
  }
  const int32_t z = days + 719468;
  const int32_t era = (z >= 0 ? z : z - 146096) / 146097;
  const uint32_t doe = (uint32_t)(z - era * 146097);
  const uint32_t yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;
  const uint32_t doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);
  const uint32_t mp = (5u * doy + 2u) / 153u;
  const uint32_t d = doy - (153u * mp + 2u) / 5u + 1u;
  const uint32_t m = mp < 10u ? mp + 3u : mp - 9u;
  const uint32_t y = (uint32_t)((int32_t)yoe + era * 400 + (m <= 2u ? 1 : 0));
  t = resp_put_str(t, "$68\r\nserials::");
  t = resp_put_2(t, y / 100u);
  t = resp_put_2(t, y % 100u);
  *t++ = '-';
  t = resp_put_2(t, m);
  *t++ = '-';
  t = resp_put_2(t, d);
  *t++ = '-';
  t = resp_put_2(t, (uint32_t)hh);
  t = resp_put_str(t, "::");
  const uint4* iv = (const uint4*)id;
  const uint4 i0 = iv[0], i1 = iv[1], i2 = iv[2];
  const uint32_t w[11] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w, i2.x, i2.y, i2.z};
#pragma unroll
  for (uint32_t q = 0; q < RESP_ID / 4u; q++) {
#pragma unroll
    for (uint32_t b = 0; b < 4; b++) t[4u * q + b] = (uint8_t)(w[q] >> (8u * b));
  }
  return resp_put_str(t + RESP_ID, "\r\n");
}

// Write pass, behind the exclusive scan of cnt[] (base[blk]); launched with resp_lds_bytes(the largest block text) of
// dynamic LDS.  Record i's text goes to out + base[blk] + (the bytes of the records before it in its block).  The block's
// text is laid out in LDS shifted by the 16-byte phase of its first global byte, so that every 16-byte aligned global
// chunk is one aligned 16-byte LDS word, and stored from there.
// pts[0..npts) (ascending record indices of the launch): pt_off[k] = the text offset of record pts[k] — the first record
// of a set in front of which a host piece goes (lists_write_body).
__global__ void __launch_bounds__(RESP_BLOCK) k_image_resp_write(RespArgs a, uint64_t n, const unsigned long long* base, uint8_t* out,
                                                                const uint64_t* pts, uint64_t npts, unsigned long long* pt_off) {
  extern __shared__ __attribute__((aligned(16))) uint8_t resp_lds[];  // every LDS byte is dynamic: the base stays 16-byte aligned
  uint32_t* const ws = (uint32_t*)resp_lds;
  uint8_t* const text = resp_lds + 16;
  const uint64_t i = (uint64_t)blockIdx.x * RESP_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint4 c0 = make_uint4(0u, 0u, 0u, 0u), c1 = c0, c2 = c0;
  RespRec r{};
  if (i < n) {
    const uint4* rec = (const uint4*)(a.recs + i * KNOWN_REC_BYTES);
    c0 = rec[0];
    c1 = rec[1];
    c2 = rec[2];
    r = resp_rec(a, known_run_set(a.first, a.k, i, n), i);
  }
  const uint32_t len = c0.x < (uint32_t)CTMR_MAX_SERIAL ? c0.x : (uint32_t)CTMR_MAX_SERIAL;
  const uint32_t bytes = i < n ? resp_rec_bytes(r, len) : 0u;
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
  for (uint32_t k = 0; k < RESP_BLOCK / 64; k++) {
    pre += k < wv ? ws[k] : 0u;
    total += ws[k];
  }
  const uint32_t local = pre + inc - bytes;
  const unsigned long long g0 = base[blockIdx.x];
  uint8_t* const gstart = out + g0;
  const uint32_t phase = (uint32_t)((uintptr_t)gstart & 15u);
  if (i < n) {
    uint8_t* t = text + phase + local;
    const uint8_t* id = a.ids + (size_t)r.ordinal * RESP_ID_ROW;
    if (r.argc) {
      *t++ = '*';
      t = resp_put_dec32(t, r.argc, resp_digits(r.argc));
      t = resp_put_str(t, "\r\n$4\r\nSADD\r\n");
      t = resp_put_key(t, r.hour, id);
    }
    *t++ = '$';
    if (len >= 10u) *t++ = (uint8_t)('0' + len / 10u);
    *t++ = (uint8_t)('0' + len % 10u);
    t = resp_put_str(t, "\r\n");
    const uint32_t sw[10] = {c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w};
#pragma unroll
    for (uint32_t q = 0; q < 10; q++) {
#pragma unroll
      for (uint32_t b = 0; b < 4; b++)
        if (4u * q + b < len) t[4u * q + b] = (uint8_t)(sw[q] >> (8u * b));
    }
    t = resp_put_str(t + len, "\r\n");
    if (r.expire) {
      t = resp_put_str(t, "*3\r\n$8\r\nEXPIREAT\r\n");
      t = resp_put_key(t, r.hour, id);
      const uint32_t nd = resp_digits(r.t), tl = nd + (r.neg ? 1u : 0u);
      *t++ = '$';
      if (tl >= 10u) *t++ = '1';
      *t++ = (uint8_t)('0' + tl % 10u);
      t = resp_put_str(t, "\r\n");
      if (r.neg) *t++ = '-';
      t = resp_put_dec(t, r.t, nd);
      t = resp_put_str(t, "\r\n");
    }
  }
  // the positions the host asked for that fall in this wave
  if (npts) {
    const uint64_t wfirst = (uint64_t)blockIdx.x * RESP_BLOCK + wv * 64u;
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
  const uint32_t head = (16u - phase) & 15u;  // bytes before the first 16-byte aligned global address
  if (head >= total) {
    if (threadIdx.x < total) gstart[threadIdx.x] = text[phase + threadIdx.x];
    return;
  }
  const uint32_t nvec = (total - head) >> 4, tail = (total - head) & 15u;
  if (threadIdx.x < head) gstart[threadIdx.x] = text[phase + threadIdx.x];
  uint4* gv = (uint4*)(gstart + head);
  const uint4* lv = (const uint4*)(text + phase + head);  // phase + head is 0 or 16: aligned
  for (uint32_t k = threadIdx.x; k < nvec; k += RESP_BLOCK) gv[k] = lv[k];
  if (threadIdx.x < tail) {
    const uint32_t x = head + 16u * nvec + threadIdx.x;
    gstart[x] = text[phase + x];
  }
}

}  // namespace ctmr
