// kernels/entries_json.h — get-entries HTTP bodies {"entries":[{"leaf_input":"<base64>","extra_data":"<base64>"},…]} as
// they lie → the raw-entry batch ctmr_map_entries* takes (include/ctmr.h ctmr_entries_json*).
// No quote occurs inside a string of the grammar (a backslash is outside it wherever it stands), so whether a byte lies
// inside a string is the parity of the quotes between its response's start and itself.  The passes, each a launch:
//   quotes    per block of TX_TILE bytes the quotes are counted; an exclusive scan of the counts, minus the prefix at a
//             response's start (k_ej_qstart), is the string state of any byte.
//   mark      outside a string a byte is white space, one of { } [ ] : , or a quote — anything else is a violation;
//             inside, a byte outside A-Za-z0-9+/ is an "odd byte".  Counted per block, scanned, then written: the token
//             list (position << 3 | kind, quotes as open / close) and, per token, the odd bytes before it.
//   resp      per response: its first token (a binary search), its token count T, which fixes its entries: T = 7 for
//             none, 6 + 14 n for n >= 1.
//   check     token j of a response has one legal kind.  The lane of an entry's '{' compares the keys with their
//             literals, checks the two values (length a multiple of 4; the odd bytes inside are exactly the one or two
//             '=' at the end) and writes the decoded lengths, leaf first whatever the order in the text.
//   decode    the hot path: one tile of TX_DTILE characters of one string per block → TX_DOUT bytes (tx_decode_tile).
// Every body judged on its own (ctmr_entries_json_each*): mark, resp and check take EACH = true and report
// to a table of one word per response (ej_verdict) instead of the call's one pair; behind check, k_ej_drop (kernels/text_scan.h) zeroes the
// entry count of every response with a verdict and k_ej_gather moves the good entries' lengths and sources to their
// places under the new numbering.  EACH = false compiles to what the strict call has always run.
// The text, its segments (here: the responses), the chunks and tiles it is read in, the wave's scan and report and the
// decode of a tile are those of kernels/text_scan.h, which kernels/pem_decode.h builds on as well; what is here is JSON.
// gfx950 (CDNA4, wave64) only; part of kernels.h.
#pragma once
#include "text_scan.h"

namespace ctmr {

constexpr uint32_t EJ_LBRACE = 0, EJ_RBRACE = 1, EJ_LBRACK = 2, EJ_RBRACK = 3, EJ_COLON = 4, EJ_COMMA = 5, EJ_QOPEN = 6, EJ_QCLOSE = 7;
constexpr uint32_t EJ_FRAME = 5, EJ_ENTRY = 14;  // tokens before the first entry; of an entry with the comma behind it

__device__ __forceinline__ uint32_t ej_quote_mask(const uint4& v) {
  uint32_t m = 0u;
#pragma unroll
  for (uint32_t q = 0; q < TX_PER; q++) m |= (tx_byte(v, q) == 0x22u ? 1u : 0u) << q;
  return m;
}

// EACH = false: err is the call's pair (lowest response, lowest offset) and the wave reduces first (tx_report).
// EACH = true (ctmr_entries_json_each*): err is a table of one word per response, ~0 = inside the grammar so
// far, and a lane with a finding does its own atomicMin on its response's word — a wave holds lanes of any number of
// responses, so nothing is reduced over it; findings are rare.  r < R wherever bad is set.
template <bool EACH>
__device__ __forceinline__ void ej_verdict(unsigned long long* err, bool bad, uint64_t r, uint64_t off) {
  if (EACH) {
    if (bad) atomicMin(err + r, (unsigned long long)off);
  } else {
    tx_report(err, bad, r, off);
  }
}

// quotes: cnt[blk] = the quotes among the text's bytes of block blk
__global__ void __launch_bounds__(TX_BLOCK) k_ej_quotes(TxText T, uint64_t b0, unsigned long long* cnt) {
  const uint64_t blk = b0 + blockIdx.x;
  int64_t p0;
  uint32_t valid, total;
  const uint4 v = tx_chunk(T, blk, threadIdx.x, &p0, &valid);
  (void)tx_wave_scan((uint32_t)__popc(ej_quote_mask(v) & valid), &total);
  if (threadIdx.x == 0) cnt[blk] = total;
}

// qstart[r] = the quotes of [lo, sb[r]); a wave per response
__global__ void __launch_bounds__(RP_BLOCK) k_ej_qstart(TxText T, uint64_t b0, const unsigned long long* qblk, unsigned long long* qstart) {
  const uint64_t r = (b0 + blockIdx.x) * (RP_BLOCK / 64) + (threadIdx.x >> 6);
  if (r >= T.S) return;  // (whole waves leave)
  const uint64_t at = T.sb[r];
  const unsigned long long q = tx_boundary_prefix<ej_quote_mask>(T, tx_block_of(T, at), at, qblk);
  if ((threadIdx.x & 63u) == 0) qstart[r] = q;
}

// mark.  WRITE = false: cnt_t[blk] / cnt_o[blk] = the tokens / odd bytes of block blk, and every violation is reported.
// WRITE = true, behind the exclusive scans: tok[] = position << 3 | kind of every token, oddb[] = the odd bytes before it.
// EACH (ej_verdict): a lane reports its first violation in every response its 16 bytes touch.
template <bool WRITE, bool EACH = false>
__global__ void __launch_bounds__(TX_BLOCK) k_ej_mark(TxText T, uint64_t b0, const unsigned long long* qblk, const unsigned long long* qstart,
                                                      unsigned long long* cnt_t, unsigned long long* cnt_o, unsigned long long* tok,
                                                      unsigned long long* oddb, unsigned long long* err) {
  const uint32_t lane = threadIdx.x;
  const uint64_t blk = b0 + blockIdx.x;
  int64_t p0;
  uint32_t valid;
  const uint4 v = tx_chunk(T, blk, lane, &p0, &valid);
  uint32_t quote = 0u, ws = 0u, st = 0u, b64 = 0u;
#pragma unroll
  for (uint32_t q = 0; q < TX_PER; q++) {
    const uint32_t c = tx_byte(v, q);
    quote |= (c == 0x22u ? 1u : 0u) << q;
    ws |= ((c == 0x20u || c == 0x09u || c == 0x0au || c == 0x0du) ? 1u : 0u) << q;
    st |= (((c | 0x20u) == 0x7bu || (c | 0x20u) == 0x7du || c == 0x3au || c == 0x2cu) ? 1u : 0u) << q;  // [ { ] } : ,
    b64 |= TX_ALPHABET_BIT(c) << q;
  }
  quote &= valid;
  bool uniform;  // the block lies in one response, r_lo
  const uint64_t r_lo = tx_block_segment(T, blk, &uniform);
  uint32_t total;
  const uint32_t nq = (uint32_t)__popc(quote);
  const unsigned long long q_lane = qblk[blk] + tx_wave_scan(nq, &total);  // the quotes of [lo, the lane's first byte)
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
    for (uint32_t q = 0; q < TX_PER; q++)
      if ((valid >> q) & 1u) base |= (uint32_t)((q_lane - qstart[tx_segment_of(T.sb, T.S, (uint64_t)(p0 + q))]) & 1ull) << q;
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
      vr = uniform ? r_lo : tx_segment_of(T.sb, T.S, voff);
    }
    ej_verdict<EACH>(err, viol != 0u, vr, voff);
    if (EACH && viol && !uniform) {  // the lane's later violations may lie in later responses
      uint32_t m = viol & (viol - 1u);
#pragma unroll 1
      while (m) {
        const uint64_t off = (uint64_t)(p0 + (int64_t)(__ffs(m) - 1));
        m &= m - 1u;
        const uint64_t r2 = tx_segment_of(T.sb, T.S, off);
        if (r2 != vr) ej_verdict<true>(err, true, r2, off);
        vr = r2;
      }
    }
  }
  const uint32_t packed = tx_wave_scan((uint32_t)__popc(tokm) | ((uint32_t)__popc(odd) << 16), &total);
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
    const uint32_t c = tx_byte(v, q);
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

// resp: tfirst[r] = the tokens before sb[r] (r <= R); ecnt[r] = the entries the token count of response r stands for,
// 0 and a report when it stands for none; ecnt[R] = 0 (the scan's total)
template <bool EACH = false>
__global__ void __launch_bounds__(RP_BLOCK) k_ej_resp(TxText T, uint64_t b0, const unsigned long long* tok, uint64_t ntok,
                                                      unsigned long long* tfirst, unsigned long long* ecnt, unsigned long long* err) {
  const uint64_t r = (b0 + blockIdx.x) * RP_BLOCK + threadIdx.x;
  bool bad = false;
  uint64_t off = 0;
  if (r <= T.S) {
    uint64_t first[2];
    tx_first_tokens(T, r, tok, ntok, 3u, first);
    tfirst[r] = first[0];
    uint64_t n = 0;
    if (r < T.S) {
      const uint64_t t = first[1] - first[0];
      if (t >= EJ_FRAME + EJ_ENTRY + 1 && (t - 6) % EJ_ENTRY == 0) n = (t - 6) / EJ_ENTRY;
      else if (t != 7) bad = true;
      off = T.sb[r];
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
__device__ __forceinline__ bool ej_value(const TxText& T, const EjCheck& C, uint64_t o, unsigned long long* dec, unsigned long long* at) {
  const uint64_t a = (C.tok[o] >> 3) + 1, c = C.tok[o + 1] >> 3, L = c - a;
  uint32_t pad = 0u;
  if (L >= 1 && T.s[c - 1] == '=') pad = (L >= 2 && T.s[c - 2] == '=') ? 2u : 1u;
  *dec = (L & 3ull) ? 0ull : L / 4 * 3 - pad;
  *at = a;
  return (L & 3ull) == 0 && C.oddb[o + 1] - C.oddb[o] == pad;
}

// check: one lane per token
template <bool EACH = false>
__global__ void __launch_bounds__(RP_BLOCK) k_ej_check(TxText T, uint64_t b0, EjCheck C, unsigned long long* err) {
  const uint64_t t = (b0 + blockIdx.x) * RP_BLOCK + threadIdx.x;
  bool bad = false;
  uint64_t r = 0, pos = 0;
  if (t < C.ntok) {
    const unsigned long long tk = C.tok[t];
    pos = tk >> 3;
    const uint32_t kind = (uint32_t)(tk & 7ull);
    r = tx_segment_of(T.sb, T.S, pos);
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

// each, behind the scan of k_ej_drop's counts (efirst): the lengths and sources k_ej_check wrote, compacted over the good
// responses.  One lane per entry e0 of the old numbering (n0 = efirst0[R] > 0); its response is the last r with
// efirst0[r] <= e0, which has entries, so it is that one and no empty neighbour.
__global__ void __launch_bounds__(RP_BLOCK) k_ej_gather(uint64_t b0, uint64_t R, uint64_t n0, const unsigned long long* bad_at,
                                                        const unsigned long long* efirst0, const unsigned long long* efirst,
                                                        const unsigned long long* len0, const unsigned long long* src0, unsigned long long* len,
                                                        unsigned long long* src) {
  const uint64_t e0 = (b0 + blockIdx.x) * RP_BLOCK + threadIdx.x;
  if (e0 >= n0) return;
  const uint64_t r = tx_segment_of((const uint64_t*)efirst0, R, e0);
  if (bad_at[r] != ~0ull) return;
  const uint64_t e = efirst[r] + (e0 - efirst0[r]);
#pragma unroll
  for (uint32_t k = 0; k < 2; k++) {
    len[2 * e + k] = len0[2 * e0 + k];
    src[2 * e + k] = src0[2 * e0 + k];
  }
}

// decode: block = tile t of string i = tile_str[t]: its characters [TX_DTILE k, …) → blob[bounds[i] + TX_DOUT k, …).  The
// characters of a string lie one behind the other.
__global__ void __launch_bounds__(TX_DBLOCK) k_ej_decode(const uint8_t* s, uint64_t b0, const unsigned long long* tile_str, const unsigned long long* tile_first,
                                                         const unsigned long long* bounds, const unsigned long long* src, uint8_t* blob) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[TX_DOUT + 16];
  const TxTile w = tx_tile(b0 + blockIdx.x, tile_str, tile_first, bounds);
  if (tx_has_quantum(w)) tx_stage_quantum(stage, w, (uint64_t)(uintptr_t)s + src[w.i] + w.k * TX_DTILE + 4ull * threadIdx.x);
  tx_tile_leaves(stage, w, blob);
}

}  // namespace ctmr
