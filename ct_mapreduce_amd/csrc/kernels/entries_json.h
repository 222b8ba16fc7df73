// kernels/entries_json.h — get-entries HTTP bodies {"entries":[{"leaf_input":"<base64>","extra_data":"<base64>"},…]} as
// they lie → the raw-entry batch ctmr_map_entries* takes (include/ctmr.h ctmr_entries_json*).
// No quote occurs inside a string of the grammar (a backslash is outside it wherever it stands), so whether a byte lies
// inside a string is the parity of the quotes between its response's start and itself.  The passes, each a launch:
//   quotes    per block of EJ_TILE bytes the quotes are counted; an exclusive scan of the counts, minus the prefix at a
//             response's start (k_ej_qstart), is the string state of any byte.
//   mark      outside a string a byte is white space, one of { } [ ] : , or a quote — anything else is a violation;
//             inside, a byte outside A-Za-z0-9+/ is an "odd byte".  Counted per block, scanned, then written: the token
//             list (position << 3 | kind, quotes as open / close) and, per token, the odd bytes before it.
//   resp      per response: its first token (a binary search), its token count T, which fixes its entries: T = 7 for
//             none, 6 + 14 n for n >= 1.
//   check     token j of a response has one legal kind.  The lane of an entry's '{' compares the keys with their
//             literals, checks the two values (length a multiple of 4; the odd bytes inside are exactly the one or two
//             '=' at the end) and writes the decoded lengths, leaf first whatever the order in the text.
//   decode    the hot path: one tile of EJ_DTILE characters of one string per block → EJ_DOUT bytes, staged in LDS at the
//             16-byte phase of the first global byte and stored as k_lists_write stores (16-byte body, byte-wide ends).
// Every body judged on its own (ctmr_entries_json_each*): mark, resp and check take EACH = true and report
// to a table of one word per response (ej_verdict) instead of the call's one pair; behind check, k_ej_drop zeroes the
// entry count of every response with a verdict and k_ej_gather moves the good entries' lengths and sources to their
// places under the new numbering.  EACH = false compiles to what the strict call has always run.
// The text lies at any alignment: quotes and mark read the aligned 16-byte chunks that cover it and mask what is outside
// the bounds, decode reads aligned dwords that hold at least one character of its string.  Non-temporal loads: the text
// is read and never needed again.  gfx950 (CDNA4, wave64) only; part of kernels.h.
#pragma once
#include "resp_parse.h"

namespace ctmr {

constexpr uint32_t EJ_BLOCK = 64, EJ_PER = 16, EJ_TILE = EJ_BLOCK * EJ_PER;  // mark: one wave, 16 bytes a lane
constexpr uint32_t EJ_DBLOCK = 256, EJ_DTILE = 4 * EJ_DBLOCK, EJ_DOUT = 3 * EJ_DBLOCK;  // decode: a quantum a lane
constexpr uint32_t EJ_LBRACE = 0, EJ_RBRACE = 1, EJ_LBRACK = 2, EJ_RBRACK = 3, EJ_COLON = 4, EJ_COMMA = 5, EJ_QOPEN = 6, EJ_QCLOSE = 7;
// A launch takes at most EJ_GRID blocks (a grid of 2^32 threads and more is not launched whole): the host launches in
// turns, b0 = the first block of the turn.
constexpr uint64_t EJ_GRID = 1ull << 22;
constexpr uint32_t EJ_FRAME = 5, EJ_ENTRY = 14;  // tokens before the first entry; of an entry with the comma behind it

// the text: response r is s[rb[r], rb[r + 1]); a0 = the address of s + rb[0] rounded down to 16
struct EjText {
  const uint8_t* s;
  const uint64_t* rb;  // R + 1, ascending (device)
  uint64_t R, lo, hi;  // lo = rb[0], hi = rb[R], lo < hi
  uint64_t a0;
};

// the response of the byte at p (lo <= p < hi): the largest r < R with rb[r] <= p
__device__ __forceinline__ uint64_t ej_resp_of(const uint64_t* rb, uint64_t R, uint64_t p) {
  uint64_t l = 0, h = R - 1;
  while (l < h) {
    const uint64_t mid = (l + h + 1) >> 1;
    if (rb[mid] <= p) l = mid;
    else h = mid - 1;
  }
  return l;
}

// the lane's chunk of block blk: its 16 bytes (zero when none is of the text), *p0 = the offset of its first byte from
// s (below lo, even negative, when the chunk begins before the text), *valid = the bytes that lie in [lo, hi)
__device__ __forceinline__ uint4 ej_chunk(const EjText& T, uint64_t blk, uint32_t lane, int64_t* p0, uint32_t* valid) {
  const uint64_t a = T.a0 + blk * EJ_TILE + lane * EJ_PER;
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

__device__ __forceinline__ uint32_t ej_byte(const uint4& v, uint32_t q) {
  const uint32_t w = q < 8u ? (q < 4u ? v.x : v.y) : (q < 12u ? v.z : v.w);
  return (w >> (8u * (q & 3u))) & 0xffu;
}

__device__ __forceinline__ uint32_t ej_quote_mask(const uint4& v) {
  uint32_t m = 0u;
#pragma unroll
  for (uint32_t q = 0; q < EJ_PER; q++) m |= (ej_byte(v, q) == 0x22u ? 1u : 0u) << q;
  return m;
}

// the exclusive prefix sum of v over the wave; *total = the wave's sum
__device__ __forceinline__ uint32_t ej_wave_scan(uint32_t v, uint32_t* total) {
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

// the lowest response outside the grammar and the lowest offset reported: every lane of the wave calls.  An offset lies
// inside its response, responses ascend, so the lowest offset belongs to the lowest response.
__device__ __forceinline__ void ej_report(unsigned long long* err, bool bad, uint64_t r, uint64_t off) {
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

// EACH = false: err is the call's pair (lowest response, lowest offset) and the wave reduces first (ej_report).
// EACH = true (ctmr_entries_json_each*): err is a table of one word per response, ~0 = inside the grammar so
// far, and a lane with a finding does its own atomicMin on its response's word — a wave holds lanes of any number of
// responses, so nothing is reduced over it; findings are rare.  r < R wherever bad is set.
template <bool EACH>
__device__ __forceinline__ void ej_verdict(unsigned long long* err, bool bad, uint64_t r, uint64_t off) {
  if (EACH) {
    if (bad) atomicMin(err + r, (unsigned long long)off);
  } else {
    ej_report(err, bad, r, off);
  }
}

// quotes: cnt[blk] = the quotes among the text's bytes of block blk
__global__ void __launch_bounds__(EJ_BLOCK) k_ej_quotes(EjText T, uint64_t b0, unsigned long long* cnt) {
  const uint64_t blk = b0 + blockIdx.x;
  int64_t p0;
  uint32_t valid, total;
  const uint4 v = ej_chunk(T, blk, threadIdx.x, &p0, &valid);
  (void)ej_wave_scan((uint32_t)__popc(ej_quote_mask(v) & valid), &total);
  if (threadIdx.x == 0) cnt[blk] = total;
}

// qstart[r] = the quotes of [lo, rb[r]): the scanned block count plus the quotes of rb[r]'s block before it; a wave per
// response
__global__ void __launch_bounds__(RP_BLOCK) k_ej_qstart(EjText T, uint64_t b0, const unsigned long long* qblk, unsigned long long* qstart) {
  const uint64_t r = (b0 + blockIdx.x) * (RP_BLOCK / 64) + (threadIdx.x >> 6);
  if (r >= T.R) return;  // (whole waves leave)
  const uint64_t at = T.rb[r];
  const uint64_t blk = ((uint64_t)(uintptr_t)T.s + at - T.a0) / EJ_TILE;
  int64_t p0;
  uint32_t valid, total;
  const uint4 v = ej_chunk(T, blk, threadIdx.x & 63u, &p0, &valid);
  uint32_t before = 0u;  // the lane's bytes below at
  const int64_t d = (int64_t)at - p0;
  if (d >= 16) before = 0xffffu;
  else if (d > 0) before = 0xffffu >> (16u - (uint32_t)d);
  (void)ej_wave_scan((uint32_t)__popc(ej_quote_mask(v) & valid & before), &total);
  if ((threadIdx.x & 63u) == 0) qstart[r] = qblk[blk] + total;
}

// mark.  WRITE = false: cnt_t[blk] / cnt_o[blk] = the tokens / odd bytes of block blk, and every violation is reported.
// WRITE = true, behind the exclusive scans: tok[] = position << 3 | kind of every token, oddb[] = the odd bytes before it.
// EACH (ej_verdict): a lane reports its first violation in every response its 16 bytes touch.
template <bool WRITE, bool EACH = false>
__global__ void __launch_bounds__(EJ_BLOCK) k_ej_mark(EjText T, uint64_t b0, const unsigned long long* qblk, const unsigned long long* qstart,
                                                      unsigned long long* cnt_t, unsigned long long* cnt_o, unsigned long long* tok,
                                                      unsigned long long* oddb, unsigned long long* err) {
  const uint32_t lane = threadIdx.x;
  const uint64_t blk = b0 + blockIdx.x;
  int64_t p0;
  uint32_t valid;
  const uint4 v = ej_chunk(T, blk, lane, &p0, &valid);
  uint32_t quote = 0u, ws = 0u, st = 0u, b64 = 0u;
#pragma unroll
  for (uint32_t q = 0; q < EJ_PER; q++) {
    const uint32_t c = ej_byte(v, q);
    quote |= (c == 0x22u ? 1u : 0u) << q;
    ws |= ((c == 0x20u || c == 0x09u || c == 0x0au || c == 0x0du) ? 1u : 0u) << q;
    st |= (((c | 0x20u) == 0x7bu || (c | 0x20u) == 0x7du || c == 0x3au || c == 0x2cu) ? 1u : 0u) << q;  // [ { ] } : ,
    b64 |= ((((c | 0x20u) - 0x61u) < 26u || (c - 0x30u) < 10u || c == 0x2bu || c == 0x2fu) ? 1u : 0u) << q;
  }
  quote &= valid;
  // the block's response, when it has one only: that of its first byte of the text, whose end lies behind the block
  const uint64_t s0 = (uint64_t)(uintptr_t)T.s;
  const uint64_t blk_lo = T.a0 + blk * EJ_TILE - s0 + (blk == 0 ? T.lo - (T.a0 - s0) : 0ull);
  const uint64_t blk_end = T.a0 + (blk + 1ull) * EJ_TILE - s0;
  const uint64_t r_lo = ej_resp_of(T.rb, T.R, blk_lo);
  const bool uniform = T.rb[r_lo + 1] >= (blk_end < T.hi ? blk_end : T.hi);
  uint32_t total;
  const uint32_t nq = (uint32_t)__popc(quote);
  const unsigned long long q_lane = qblk[blk] + ej_wave_scan(nq, &total);  // the quotes of [lo, the lane's first byte)
  uint32_t excl = quote;  // the parity of the lane's quotes before each byte
  excl ^= excl << 1;
  excl ^= excl << 2;
  excl ^= excl << 4;
  excl ^= excl << 8;
  excl = (excl ^ quote) & 0xffffu;
  uint32_t base = 0u;  // per byte: the parity of the quotes between its response's start and the lane's first byte
  if (uniform) {
    base = ((q_lane - qstart[r_lo]) & 1ull) ? 0xffffu : 0u;
  } else {
#pragma unroll 1
    for (uint32_t q = 0; q < EJ_PER; q++)
      if ((valid >> q) & 1u) base |= (uint32_t)((q_lane - qstart[ej_resp_of(T.rb, T.R, (uint64_t)(p0 + q))]) & 1ull) << q;
  }
  const uint32_t in = (excl ^ base) & valid;  // inside a string before this byte
  const uint32_t odd = in & ~quote & ~b64;
  const uint32_t outside = valid & ~in & ~quote;
  const uint32_t viol = outside & ~st & ~ws;
  const uint32_t tokm = (outside & st) | quote;
  if (!WRITE) {
    uint64_t vr = 0, voff = 0;
    if (viol) {
      voff = (uint64_t)(p0 + (int64_t)(__ffs(viol) - 1));
      vr = uniform ? r_lo : ej_resp_of(T.rb, T.R, voff);
    }
    ej_verdict<EACH>(err, viol != 0u, vr, voff);
    if (EACH && viol && !uniform) {  // the lane's later violations may lie in later responses
      uint32_t m = viol & (viol - 1u);
#pragma unroll 1
      while (m) {
        const uint64_t off = (uint64_t)(p0 + (int64_t)(__ffs(m) - 1));
        m &= m - 1u;
        const uint64_t r2 = ej_resp_of(T.rb, T.R, off);
        if (r2 != vr) ej_verdict<true>(err, true, r2, off);
        vr = r2;
      }
    }
  }
  const uint32_t packed = ej_wave_scan((uint32_t)__popc(tokm) | ((uint32_t)__popc(odd) << 16), &total);
  if (!WRITE) {
    if (lane == 0) {
      cnt_t[blk] = total & 0xffffu;
      cnt_o[blk] = total >> 16;
    }
    return;
  }
  unsigned long long at = cnt_t[blk] + (packed & 0xffffu);
  const unsigned long long odd_lane = cnt_o[blk] + (packed >> 16);
  uint32_t m = tokm;
  while (m) {
    const uint32_t q = (uint32_t)__ffs(m) - 1u;
    m &= m - 1u;
    const uint32_t c = ej_byte(v, q);
    uint32_t kind;
    if (c == 0x22u) kind = ((in >> q) & 1u) ? EJ_QCLOSE : EJ_QOPEN;
    else if (c == 0x7bu) kind = EJ_LBRACE;
    else if (c == 0x7du) kind = EJ_RBRACE;
    else if (c == 0x5bu) kind = EJ_LBRACK;
    else if (c == 0x5du) kind = EJ_RBRACK;
    else if (c == 0x3au) kind = EJ_COLON;
    else kind = EJ_COMMA;
    tok[at] = ((unsigned long long)(p0 + q) << 3) | kind;
    oddb[at] = odd_lane + (uint32_t)__popc(odd & ((1u << q) - 1u));
    at++;
  }
}

// resp: tfirst[r] = the tokens before rb[r] (r <= R); ecnt[r] = the entries the token count of response r stands for,
// 0 and a report when it stands for none; ecnt[R] = 0 (the scan's total)
template <bool EACH = false>
__global__ void __launch_bounds__(RP_BLOCK) k_ej_resp(EjText T, uint64_t b0, const unsigned long long* tok, uint64_t ntok,
                                                      unsigned long long* tfirst, unsigned long long* ecnt, unsigned long long* err) {
  const uint64_t r = (b0 + blockIdx.x) * RP_BLOCK + threadIdx.x;
  bool bad = false;
  uint64_t off = 0;
  if (r <= T.R) {
    uint64_t first[2];
#pragma unroll
    for (uint32_t k = 0; k < 2; k++) {
      const uint64_t at = T.rb[r + k < T.R ? r + k : T.R];
      uint64_t l = 0, h = ntok;
      while (l < h) {
        const uint64_t mid = (l + h) >> 1;
        if ((tok[mid] >> 3) < at) l = mid + 1;
        else h = mid;
      }
      first[k] = l;
    }
    tfirst[r] = first[0];
    uint64_t n = 0;
    if (r < T.R) {
      const uint64_t t = first[1] - first[0];
      if (t >= EJ_FRAME + EJ_ENTRY + 1 && (t - 6) % EJ_ENTRY == 0) n = (t - 6) / EJ_ENTRY;
      else if (t != 7) bad = true;
      off = T.rb[r];
    }
    ecnt[r] = n;
  }
  ej_verdict<EACH>(err, bad, r, off);
}

template <uint32_t N>
__device__ __forceinline__ bool ej_text_is(const uint8_t* s, uint64_t at, uint64_t len, const char (&lit)[N]) {
  if (len != N - 1u) return false;
  bool ok = true;
#pragma unroll
  for (uint32_t k = 0; k + 1u < N; k++) ok = ok && s[at + k] == (uint8_t)lit[k];
  return ok;
}

// the tables the check reads and writes
struct EjCheck {
  const unsigned long long* tok;
  const unsigned long long* oddb;
  uint64_t ntok;
  const unsigned long long* tfirst;  // R + 1
  const unsigned long long* efirst;  // R + 1: the entries before response r
  unsigned long long* len;           // 2 n + 1: the decoded length of leaf e at 2 e, of extra e at 2 e + 1
  unsigned long long* src;           // 2 n: where its characters start
};

// the value string between tokens o (open) and o + 1: *dec = its decoded length, *at = its first character
__device__ __forceinline__ bool ej_value(const EjText& T, const EjCheck& C, uint64_t o, unsigned long long* dec, unsigned long long* at) {
  const uint64_t a = (C.tok[o] >> 3) + 1, c = C.tok[o + 1] >> 3, L = c - a;
  uint32_t pad = 0u;
  if (L >= 1 && T.s[c - 1] == '=') pad = (L >= 2 && T.s[c - 2] == '=') ? 2u : 1u;
  *dec = (L & 3ull) ? 0ull : L / 4 * 3 - pad;
  *at = a;
  return (L & 3ull) == 0 && C.oddb[o + 1] - C.oddb[o] == pad;
}

// check: one lane per token
template <bool EACH = false>
__global__ void __launch_bounds__(RP_BLOCK) k_ej_check(EjText T, uint64_t b0, EjCheck C, unsigned long long* err) {
  const uint64_t t = (b0 + blockIdx.x) * RP_BLOCK + threadIdx.x;
  bool bad = false;
  uint64_t r = 0, pos = 0;
  if (t < C.ntok) {
    const unsigned long long tk = C.tok[t];
    pos = tk >> 3;
    const uint32_t kind = (uint32_t)(tk & 7ull);
    r = ej_resp_of(T.rb, T.R, pos);
    const uint64_t j = t - C.tfirst[r], nt = C.tfirst[r + 1] - C.tfirst[r], ne = C.efirst[r + 1] - C.efirst[r];
    if (nt == (ne ? 6 + EJ_ENTRY * ne : 7)) {  // (else k_ej_resp has reported the response)
      uint32_t want;
      if (j < EJ_FRAME) {
        want = j == 0 ? EJ_LBRACE : j == 1 ? EJ_QOPEN : j == 2 ? EJ_QCLOSE : j == 3 ? EJ_COLON : EJ_LBRACK;
        if (j == 1) bad = !ej_text_is(T.s, pos + 1, (C.tok[t + 1] >> 3) - pos - 1, "entries");
      } else if (j + 2 >= nt) {
        want = j + 2 == nt ? EJ_RBRACK : EJ_RBRACE;
      } else {
        const uint32_t k = (uint32_t)((j - EJ_FRAME) % EJ_ENTRY);
        want = (k == 0) ? EJ_LBRACE : (k == 12) ? EJ_RBRACE : (k == 6 || k == 13) ? EJ_COMMA : (k == 3 || k == 9) ? EJ_COLON
               : (k % 3 == 1) ? EJ_QOPEN : EJ_QCLOSE;  // 1 4 7 10 open, 2 5 8 11 close
        if (k == 0) {  // the entry: tokens t + 1 … t + 12 are of this response
          const uint64_t e = C.efirst[r] + (j - EJ_FRAME) / EJ_ENTRY;
          uint32_t key[2];
#pragma unroll
          for (uint32_t h = 0; h < 2; h++) {
            const uint64_t a = (C.tok[t + 1 + 6 * h] >> 3) + 1, len = (C.tok[t + 2 + 6 * h] >> 3) - a;
            key[h] = ej_text_is(T.s, a, len, "leaf_input") ? 0u : ej_text_is(T.s, a, len, "extra_data") ? 1u : 2u;
          }
          unsigned long long dec[2], at[2];
          const bool ok0 = ej_value(T, C, t + 4, &dec[0], &at[0]), ok1 = ej_value(T, C, t + 10, &dec[1], &at[1]);
          bad = !ok0 || !ok1 || key[0] + key[1] != 1u;  // one leaf_input (0), one extra_data (1)
          const uint32_t leaf = key[0] == 0u ? 0u : 1u;
          C.len[2 * e] = bad ? 0ull : dec[leaf];
          C.src[2 * e] = at[leaf];
          C.len[2 * e + 1] = bad ? 0ull : dec[leaf ^ 1u];
          C.src[2 * e + 1] = at[leaf ^ 1u];
        }
      }
      bad = bad || kind != want;
    }
  }
  ej_verdict<EACH>(err, bad, r, pos);
}

// each, behind check: the entry count of a response with a verdict, from whichever pass, goes to zero.  cnt[r] = the
// entries of response r when bad_at[r] says none, else 0; cnt[R] = 0 (the scan's total).  efirst0: the scan of k_ej_resp's
// counts, which k_ej_check numbered its entries by.
__global__ void __launch_bounds__(RP_BLOCK) k_ej_drop(uint64_t b0, uint64_t R, const unsigned long long* bad_at, const unsigned long long* efirst0,
                                                      unsigned long long* cnt) {
  const uint64_t r = (b0 + blockIdx.x) * RP_BLOCK + threadIdx.x;
  if (r > R) return;
  cnt[r] = (r < R && bad_at[r] == ~0ull) ? efirst0[r + 1] - efirst0[r] : 0ull;
}

// each, behind the scan of k_ej_drop's counts (efirst): the lengths and sources k_ej_check wrote, compacted over the good
// responses.  One lane per entry e0 of the old numbering (n0 = efirst0[R] > 0); its response is the last r with
// efirst0[r] <= e0, which has entries, so it is that one and no empty neighbour.
__global__ void __launch_bounds__(RP_BLOCK) k_ej_gather(uint64_t b0, uint64_t R, uint64_t n0, const unsigned long long* bad_at,
                                                        const unsigned long long* efirst0, const unsigned long long* efirst,
                                                        const unsigned long long* len0, const unsigned long long* src0, unsigned long long* len,
                                                        unsigned long long* src) {
  const uint64_t e0 = (b0 + blockIdx.x) * RP_BLOCK + threadIdx.x;
  if (e0 >= n0) return;
  const uint64_t r = ej_resp_of((const uint64_t*)efirst0, R, e0);
  if (bad_at[r] != ~0ull) return;
  const uint64_t e = efirst[r] + (e0 - efirst0[r]);
#pragma unroll
  for (uint32_t k = 0; k < 2; k++) {
    len[2 * e + k] = len0[2 * e0 + k];
    src[2 * e + k] = src0[2 * e0 + k];
  }
}

// tiles[i] = the decode tiles of string i (bounds: the scanned lengths)
__global__ void __launch_bounds__(RP_BLOCK) k_ej_tiles(uint64_t b0, const unsigned long long* bounds, uint64_t nstr, unsigned long long* tiles) {
  const uint64_t i = (b0 + blockIdx.x) * RP_BLOCK + threadIdx.x;
  if (i < nstr) tiles[i] = (bounds[i + 1] - bounds[i] + EJ_DOUT - 1) / EJ_DOUT;
}

// tile_str[t] = the string of tile t (tile_first: the scanned tiles[]).  A lane writes the first EJ_OWN tiles of its
// string; what a long string has beyond them the whole wave writes, one such string after the other.
constexpr uint32_t EJ_OWN = 8;
__global__ void __launch_bounds__(RP_BLOCK) k_ej_tile_list(uint64_t b0, const unsigned long long* tile_first, uint64_t nstr,
                                                           unsigned long long* tile_str) {
  const unsigned long long i = (b0 + blockIdx.x) * RP_BLOCK + threadIdx.x;
  const unsigned long long t0 = i < nstr ? tile_first[i] : 0ull, t1 = i < nstr ? tile_first[i + 1] : 0ull;
  for (unsigned long long t = t0; t < t1 && t < t0 + EJ_OWN; t++) tile_str[t] = i;
  unsigned long long big = __ballot(t1 - t0 > EJ_OWN);
  while (big) {  // (wave-uniform)
    const int l = __ffsll(big) - 1;
    big &= big - 1ull;
    const unsigned long long from = __shfl(t0, l) + EJ_OWN, to = __shfl(t1, l), str = __shfl(i, l);
    for (unsigned long long t = from + (threadIdx.x & 63u); t < to; t += 64ull) tile_str[t] = str;
  }
}

// A-Z a-z 0-9 + / → 0..63; '=' → 0 (its bits are dropped).  Range arithmetic: nothing else reaches the decoder.
__device__ __forceinline__ uint32_t ej_sextet(uint32_t c) {
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
__device__ __forceinline__ void ej_store_tile(const uint8_t* stage, uint32_t phase, uint32_t total, uint8_t* gstart) {
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

// decode: block = tile t of string i = tile_str[t]: its characters [EJ_DTILE k, …) → blob[bounds[i] + EJ_DOUT k, …)
__global__ void __launch_bounds__(EJ_DBLOCK) k_ej_decode(const uint8_t* s, uint64_t b0, const unsigned long long* tile_str, const unsigned long long* tile_first,
                                                         const unsigned long long* bounds, const unsigned long long* src, uint8_t* blob) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[EJ_DOUT + 16];
  const uint64_t t = b0 + blockIdx.x, i = tile_str[t], k = t - tile_first[i];
  const uint64_t at0 = bounds[i], dec = bounds[i + 1] - at0;
  const uint64_t left = dec - k * EJ_DOUT;
  const uint32_t total = left < EJ_DOUT ? (uint32_t)left : EJ_DOUT;  // 1 … EJ_DOUT
  const uint64_t dst = at0 + k * EJ_DOUT;
  const uint32_t phase = (uint32_t)(dst & 15ull);
  if (3u * threadIdx.x < total) {
    const uint64_t a = (uint64_t)(uintptr_t)s + src[i] + k * EJ_DTILE + 4ull * threadIdx.x;
    const uint32_t sh = 8u * (uint32_t)(a & 3ull);
    const uint32_t* w = (const uint32_t*)(uintptr_t)(a & ~3ull);
    uint32_t ch = __builtin_nontemporal_load(w);
    if (sh) ch = (ch >> sh) | (__builtin_nontemporal_load(w + 1) << (32u - sh));  // (the quantum reaches into w[1])
    const uint32_t x = (ej_sextet(ch & 0xffu) << 18) | (ej_sextet((ch >> 8) & 0xffu) << 12) | (ej_sextet((ch >> 16) & 0xffu) << 6) |
                       ej_sextet(ch >> 24);
    uint8_t* o = stage + phase + 3u * threadIdx.x;
    o[0] = (uint8_t)(x >> 16);
    o[1] = (uint8_t)(x >> 8);
    o[2] = (uint8_t)x;
  }
  __syncthreads();
  ej_store_tile(stage, phase, total, blob + dst);
}

}  // namespace ctmr
