// kernels/pem_decode.h — files of concatenated "-----BEGIN CERTIFICATE-----" blocks as they lie → the payload and offsets
// of a packed batch (include/ctmr.h ctmr_pem_decode*).  The inverse of kernels/pem.h.
// '-' is not in the base64 alphabet, so every dash of a valid file belongs to an armor line, and the armor lines of a
// file alternate BEGIN, END: that does here what quote parity does in kernels/entries_json.h.  The passes, each a launch:
//   mark      one wave per TX_TILE bytes.  Per byte a class: dash, LF, blank, alphabet, '=', other.  Counted per block —
//             armor tokens, body characters (alphabet and '='), '=' — scanned, then written: the token list
//             (position << 1 | kind) with the characters and the '=' in front of each.  Found here: an "other" byte; a
//             dash outside an armor line (a run of dashes starts a line and spells a literal, or closes one; no run is
//             longer than 5); and, through a summary byte per block that says what the block's last non-ws byte was, a
//             character behind a '=' and a character behind dashes with no LF between.
//   fstart    the characters in front of every file boundary (a wave each).
//   files     per file: its first token (a binary search), its token count (even), its certificates.
//   check     a lane per token: kinds alternate from BEGIN; no character lies between an END and the next BEGIN, before
//             the first BEGIN or behind the last END; between BEGIN and END C % 4 == 0 and at most two '='.  The END's
//             lane writes the decoded length and decides the block's layout: regular (L, e) — lines of L characters,
//             each ended by the same eol of e bytes, nothing else — or irregular.
//   squeeze   irregular blocks only: their characters copied contiguously into a working buffer.
//   decode    the hot path: one tile of TX_DTILE characters of one certificate per block → TX_DOUT bytes.  A lane finds
//             its quantum at body + (r / L)(L + e) + r % L, straight in the text, and packs 4 → 3 (tx_decode_tile).
// Every file judged on its own (ctmr_pem_decode_each*): mark, files and check take EACH = true and report to
// a table of one word per file (pd_verdict) instead of the call's one pair; behind check, k_ej_drop zeroes the certificate
// count of every file with a verdict and k_pd_gather moves the good certificates' five tables to their places under the
// new numbering.  EACH = false compiles to what the strict call has always run.
// The text, its segments (here: the files), the chunks and tiles it is read in, the wave's scan and report and the decode
// of a tile are those of kernels/text_scan.h; what is here is PEM.  gfx950 (CDNA4, wave64) only; part of kernels.h.
#pragma once
#include "text_scan.h"

namespace ctmr {

constexpr uint32_t PD_BEGIN = 0, PD_END = 1;
constexpr uint32_t PD_BEGIN_LEN = 27, PD_END_LEN = 25;      // the armor lines without their eol
constexpr uint32_t PD_BEGIN_CHARS = 16, PD_END_CHARS = 14;  // the letters in them: what the character count sees of them
constexpr uint32_t PD_LMAX = 1024;  // a regular block of two lines and more has lines of at most this; so has BEGIN's blank run
constexpr uint32_t PD_OWN = 32;     // the eols a lane checks itself; what a block has beyond them the whole wave checks
constexpr uint32_t PD_IRREGULAR = 3;  // lay[i] & 3: 1, 2 = the eol bytes of a regular block, 0 = a single line without need of one
constexpr uint32_t PD_S_ANY = 1, PD_S_EQ = 2, PD_S_DASH = 4, PD_S_LF = 8;  // the summary byte of a block

__device__ __forceinline__ bool pd_is_blank(uint32_t c) { return c == 0x20u || c == 0x09u || c == 0x0du; }
__device__ __forceinline__ bool pd_is_ws(uint32_t c) { return pd_is_blank(c) || c == 0x0au; }

template <uint32_t N>
__device__ __forceinline__ bool pd_spells(const uint8_t* s, uint64_t at, const char (&lit)[N]) {
  uint32_t diff = 0u;  // (no branch per byte: the caller has checked that all of them lie in the file)
#pragma unroll
  for (uint32_t k = 0; k + 1u < N; k++) diff |= (uint32_t)s[at + k] ^ (uint32_t)(uint8_t)lit[k];
  return diff == 0u;
}

// EACH = false: err is the call's pair (lowest file, lowest offset) and the wave reduces first (tx_report).
// EACH = true (ctmr_pem_decode_each*): err is a table of one word per file, ~0 = inside the grammar so far,
// and the word behind them, err[S], the lowest file with a verdict — the host reads that one word and fetches the table
// only when a file is bad.  A lane with a finding does its own atomicMin: a wave holds lanes of any number of files, so
// nothing is reduced over it; findings are rare.  f < S wherever bad is set.
template <bool EACH>
__device__ __forceinline__ void pd_verdict(unsigned long long* err, uint64_t S, bool bad, uint64_t f, uint64_t off) {
  if (EACH) {
    if (bad) {
      atomicMin(err + f, (unsigned long long)off);
      atomicMin(err + S, (unsigned long long)f);
    }
  } else {
    tx_report(err, bad, f, off);
  }
}

// the offset from s of the first byte of mark block blk (below lo, even negative, for block 0)
__device__ __forceinline__ int64_t pd_block_pos(const TxText& T, uint64_t blk) {
  return (int64_t)(T.a0 + blk * TX_TILE - (uint64_t)(uintptr_t)T.s);
}

// What precedes the byte at p, ws skipped, inside its file [fs, …): *lf = an LF lies between.  → 0 nothing (the file's
// start), else PD_S_ANY | PD_S_EQ or PD_S_DASH when it is one.  Bytes of p's own block are read; the blocks before it
// answer with their summary, unless the file starts inside one.
__device__ __forceinline__ uint32_t pd_before(const TxText& T, const uint8_t* sum, uint64_t blk, uint64_t p, uint64_t fs, bool* lf) {
  bool seen = false;
  uint32_t cls = 0u;
  int64_t q = (int64_t)p, start = pd_block_pos(T, blk);
  for (;;) {  // bytes down to `low`, then the summaries of the blocks in front
    const int64_t low = start > (int64_t)fs ? start : (int64_t)fs;
    while (q > low && !cls) {
      const uint32_t c = T.s[--q];
      if (c == 0x0au) seen = true;
      else if (!pd_is_blank(c)) cls = PD_S_ANY | (c == 0x3du ? PD_S_EQ : 0u) | (c == 0x2du ? PD_S_DASH : 0u);
    }
    if (cls || low == (int64_t)fs) break;
    for (;;) {  // q = start, the first byte of block blk, behind fs: blk >= 1
      start = pd_block_pos(T, --blk);
      if (start < (int64_t)fs) break;  // (the file starts inside this one: its bytes)
      const uint32_t m = sum[blk];
      q = start;
      if (m & PD_S_LF) seen = true;
      if (m & PD_S_ANY) cls = m & (PD_S_ANY | PD_S_EQ | PD_S_DASH);
      if (cls || start == (int64_t)fs) break;
    }
    if (cls || start == (int64_t)fs) break;
  }
  *lf = seen;
  return cls;
}

// mark.  WRITE = false: cnt_t / cnt_c / cnt_e[blk] = the armor tokens / body characters / '=' of block blk, sum[blk] its
// summary, and what a block can know alone is reported.  WRITE = true, behind the exclusive scans: tok[] = position << 1
// | kind of every armor line, ctok[] / etok[] = the characters / '=' of the text in front of it; what needs the
// summaries is reported.
// EACH (pd_verdict): a lane reports its first finding in every file its 16 bytes touch — a file can be one byte long, so
// up to 16 of them — and a character at a file's start counts as having nothing in front of it whatever the file before
// ends with.
template <bool WRITE, bool EACH = false>
__global__ void __launch_bounds__(TX_BLOCK) k_pd_mark(TxText T, uint64_t b0, unsigned long long* cnt_t, unsigned long long* cnt_c,
                                                      unsigned long long* cnt_e, uint8_t* sum, unsigned long long* tok,
                                                      unsigned long long* ctok, unsigned long long* etok, unsigned long long* err) {
  const uint32_t lane = threadIdx.x;
  const uint64_t blk = b0 + blockIdx.x;
  int64_t p0;
  uint32_t valid;
  const uint4 v = tx_chunk(T, blk, lane, &p0, &valid);
  uint32_t dash = 0u, lf = 0u, blank = 0u, alpha = 0u, eq = 0u;
#pragma unroll
  for (uint32_t q = 0; q < TX_PER; q++) {
    const uint32_t c = tx_byte(v, q);
    dash |= (c == 0x2du ? 1u : 0u) << q;
    lf |= (c == 0x0au ? 1u : 0u) << q;
    blank |= (pd_is_blank(c) ? 1u : 0u) << q;
    alpha |= TX_ALPHABET_BIT(c) << q;
    eq |= (c == 0x3du ? 1u : 0u) << q;
  }
  dash &= valid;
  lf &= valid;
  alpha &= valid;
  eq &= valid;
  const uint32_t chars = alpha | eq;
  const uint32_t other = valid & ~(dash | lf | blank | chars);
  bool uniform;  // the block lies in one file, r_lo
  const uint64_t r_lo = tx_block_segment(T, blk, &uniform);
  // runs of dashes.  A dash with a dash in front of it: some byte of the four before that is none (or the file's start).
  // A run's first dash at a line start is a token and spells a literal; elsewhere it closes one.
  const uint32_t prev_alpha = __shfl_up(alpha >> 15, 1);  // the byte in front of the lane's first (lane 0: unknown)
  uint32_t tokm = 0u, kinds = 0u;
  uint32_t viol = other;  // EACH: every finding of the lane
  bool bad = other != 0u;
  uint64_t bad_at = bad ? (uint64_t)(p0 + (int64_t)(__ffs(other) - 1)) : 0ull;
  {
    uint32_t m = dash;
    while (m) {
      const uint32_t q = (uint32_t)__ffs(m) - 1u;
      m &= m - 1u;
      const uint64_t p = (uint64_t)(p0 + (int64_t)q);
      const uint64_t f = uniform ? r_lo : tx_segment_of(T.sb, T.S, p);
      const uint64_t fs = T.sb[f], fe = T.sb[f + 1];
      const bool run = p > fs && T.s[p - 1] == 0x2du, line = !run && (p == fs || T.s[p - 1] == 0x0au);
      if (line) {  // a token, spelled right or not: BEGIN unless an E follows its dashes
        tokm |= 1u << q;
        if (p + 5u < fe && T.s[p + 5] == 0x45u) kinds |= 1u << q;
      }
      if (WRITE) continue;
      bool ok;
      if (run) {
        ok = false;
#pragma unroll 1
        for (uint32_t k = 2; k <= 5u && !ok; k++) ok = p - fs < k || T.s[p - k] != 0x2du;
      } else if (line) {
        ok = (p + PD_BEGIN_LEN <= fe && pd_spells(T.s, p, "-----BEGIN CERTIFICATE-----")) || (p + PD_END_LEN <= fe && pd_spells(T.s, p, "-----END CERTIFICATE-----"));
      } else {
        ok = (p - fs >= 22u && pd_spells(T.s, p - 22u, "-----BEGIN CERTIFICATE")) || (p - fs >= 20u && pd_spells(T.s, p - 20u, "-----END CERTIFICATE"));
      }
      if (EACH) {
        if (!ok) viol |= 1u << q;
      } else if (!ok && !bad) {
        bad = true;
        bad_at = p;
      }
    }
  }
  if (!WRITE) {
    if (EACH) {
      uint64_t last = ~0ull;
#pragma unroll 1
      while (viol) {  // ascending: the first finding of every file
        const uint64_t p = (uint64_t)(p0 + (int64_t)(__ffs(viol) - 1));
        viol &= viol - 1u;
        const uint64_t f = uniform ? r_lo : tx_segment_of(T.sb, T.S, p);
        if (f != last) pd_verdict<true>(err, T.S, true, f, p);
        last = f;
        if (uniform) break;
      }
    } else {
      uint64_t vr = 0;
      if (bad) vr = uniform ? r_lo : tx_segment_of(T.sb, T.S, bad_at);
      tx_report(err, bad, vr, bad_at);
    }
  }
  // counts: tokens and characters in one scan (each at most TX_TILE), the '=' in another
  uint32_t total, total_e;
  const uint32_t packed = tx_wave_scan((uint32_t)__popc(tokm) | ((uint32_t)__popc(chars) << 16), &total);
  const uint32_t eq_before = tx_wave_scan((uint32_t)__popc(eq), &total_e);
  if (!WRITE) {
    // the summary: the block's last non-ws byte and whether an LF lies behind it
    const uint32_t nonws = valid & ~(lf | blank);
    const unsigned long long has = __ballot(nonws != 0u), haslf = __ballot(lf != 0u);
    uint32_t m = 0u;
    if (has) {
      const uint32_t top = 63u - (uint32_t)__clzll(has);
      const uint32_t tq = 31u - (uint32_t)__clz(__shfl(nonws, top));
      const uint32_t td = __shfl(dash, top), te = __shfl(eq, top), tl = __shfl(lf, top);
      m = PD_S_ANY | (((td >> tq) & 1u) ? PD_S_DASH : 0u) | (((te >> tq) & 1u) ? PD_S_EQ : 0u);
      if ((tl >> tq) > 1u || (top < 63u && (haslf >> (top + 1u)))) m |= PD_S_LF;
    } else if (haslf) {
      m = PD_S_LF;
    }
    if (lane == 0) {
      cnt_t[blk] = total & 0xffffu;
      cnt_c[blk] = total >> 16;
      cnt_e[blk] = total_e;
      sum[blk] = (uint8_t)m;
    }
    return;
  }
  // a character with no alphabet character right in front of it: what precedes it, ws skipped, decides
  {
    uint32_t cont = (alpha << 1) | ((lane != 0u && prev_alpha) ? 1u : 0u);
    if (EACH && !uniform) {  // the files that start in this block (a wave-uniform walk): their first bytes continue nothing
      const int64_t blk_end = pd_block_pos(T, blk + 1);
#pragma unroll 1
      for (uint64_t r = r_lo + 1; r < T.S; r++) {
        const int64_t d = (int64_t)T.sb[r] - p0;
        if ((int64_t)T.sb[r] >= blk_end) break;
        if (d >= 0 && d < (int64_t)TX_PER) cont &= ~(1u << (uint32_t)d);
      }
    }
    uint32_t m = chars & ~cont;
    bool bad2 = false;
    uint64_t at2 = 0, f2 = 0, last = ~0ull;
    while (m) {
      const uint32_t q = (uint32_t)__ffs(m) - 1u;
      m &= m - 1u;
      const uint64_t p = (uint64_t)(p0 + (int64_t)q);
      const uint64_t f = uniform ? r_lo : tx_segment_of(T.sb, T.S, p);
      const uint64_t fs = T.sb[f];
      const bool is_eq = (eq >> q) & 1u;
      bool seen_lf = false, ok;
      const uint32_t cls = pd_before(T, sum, blk, p, fs, &seen_lf);
      if (!cls) ok = false;  // (a character at a file's start)
      else if (cls & PD_S_EQ) ok = is_eq;
      else if (cls & PD_S_DASH) {
        if (T.s[p - 1] == 0x2du) ok = !is_eq && p - fs >= 5u && (p - fs == 5u || T.s[p - 6] == 0x0au);  // the letter behind a line's first dashes
        else ok = seen_lf;
      } else ok = true;
      if (EACH) {
        if (!ok && f != last) {
          pd_verdict<true>(err, T.S, true, f, p);
          last = f;
        }
      } else if (!ok && !bad2) {
        bad2 = true;
        at2 = p;
        f2 = f;
      }
    }
    if (!EACH) tx_report(err, bad2, f2, at2);
  }
  unsigned long long at = cnt_t[blk] + (packed & 0xffffu);
  const unsigned long long c_lane = cnt_c[blk] + (packed >> 16), e_lane = cnt_e[blk] + eq_before;
  uint32_t m = tokm;
  while (m) {
    const uint32_t q = (uint32_t)__ffs(m) - 1u;
    m &= m - 1u;
    tok[at] = ((unsigned long long)(p0 + (int64_t)q) << 1) | ((kinds >> q) & 1u);
    ctok[at] = c_lane + (uint32_t)__popc(chars & ((1u << q) - 1u));
    etok[at] = e_lane + (uint32_t)__popc(eq & ((1u << q) - 1u));
    at++;
  }
}

// fstart: cfile[r] = the characters of [lo, sb[r]) (r <= R); a wave per boundary
__global__ void __launch_bounds__(RP_BLOCK) k_pd_fstart(TxText T, uint64_t b0, const unsigned long long* cnt_c, uint64_t nb, unsigned long long* cfile) {
  const uint64_t r = (b0 + blockIdx.x) * (RP_BLOCK / 64) + (threadIdx.x >> 6);
  if (r > T.S) return;  // (whole waves leave)
  const uint64_t at = T.sb[r];
  const uint64_t blk = tx_block_of(T, at);
  if (blk >= nb) {  // (hi at a block's edge)
    if ((threadIdx.x & 63u) == 0) cfile[r] = cnt_c[nb];
    return;
  }
  const unsigned long long c = tx_boundary_prefix<tx_alphabet_mask<true>>(T, blk, at, cnt_c);
  if ((threadIdx.x & 63u) == 0) cfile[r] = c;
}

// files: tfirst[r] = the tokens before sb[r] (r <= R); ccnt[r] = the certificates of file r, half its tokens — an odd
// count is reported; ccnt[R] = 0 (the scan's total)
template <bool EACH = false>
__global__ void __launch_bounds__(RP_BLOCK) k_pd_files(TxText T, uint64_t b0, const unsigned long long* tok, uint64_t ntok,
                                                       unsigned long long* tfirst, unsigned long long* ccnt, unsigned long long* err) {
  const uint64_t r = (b0 + blockIdx.x) * RP_BLOCK + threadIdx.x;
  bool bad = false;
  uint64_t off = 0;
  if (r <= T.S) {
    uint64_t first[2];
    tx_first_tokens(T, r, tok, ntok, 1u, first);
    tfirst[r] = first[0];
    uint64_t n = 0;
    if (r < T.S) {
      n = (first[1] - first[0]) >> 1;
      bad = (first[1] - first[0]) & 1ull;
      off = bad ? tok[first[1] - 1] >> 1 : 0ull;  // the armor line left alone
    }
    ccnt[r] = n;
  }
  pd_verdict<EACH>(err, T.S, bad, r, off);
}

// the tables the check reads and writes
struct PdCheck {
  const unsigned long long* tok;
  const unsigned long long* ctok;
  const unsigned long long* etok;
  uint64_t ntok;
  const unsigned long long* tfirst;  // R + 1
  const unsigned long long* ffirst;  // R + 1: the certificates before file r
  const unsigned long long* cfile;   // R + 1: the characters before file r
  unsigned long long* len;           // n + 1: the decoded length
  unsigned long long* src;           // n: regular: where the body starts (from s); irregular: the BEGIN's token
  unsigned long long* lay;           // n: L << 2 | e, L = 0: one line; PD_IRREGULAR
  unsigned long long* sqlen;         // n + 1: the characters of an irregular block, else 0
  unsigned long long* sqtiles;       // n + 1: the mark blocks its body touches, else 0
};

// check: one lane per token.  f_limit: the lowest file the passes before have reported, or none (~0).  The check relies on
// armor lines that are spelled right and come in pairs, so it looks at the files below that one only: a violation of its
// own in one of them is the lower one.  irr: the irregular blocks of the files looked at are added to it.
// EACH: the files looked at are those whose word in `gate` says none so far.  gate is a copy of the table made before the
// launch, not the table the check's own lanes write: which lanes run, and what they count, does not depend on timing.
template <bool EACH = false>
__global__ void __launch_bounds__(RP_BLOCK) k_pd_check(TxText T, uint64_t b0, PdCheck C, uint64_t f_limit, const unsigned long long* gate,
                                                       unsigned long long* irr, unsigned long long* err) {
  const uint64_t t = (b0 + blockIdx.x) * RP_BLOCK + threadIdx.x;
  bool bad = false, irregular = false, is_end = false;
  uint64_t f = 0, pos = 0, i = 0, cc = 0, ne = 0, p0 = 0, b = 0;
  uint32_t L = 0, e = 0;
  unsigned long long w_nl = 0;  // the eols of a long regular block: what lies beyond the first PD_OWN the wave checks together
  if (t < C.ntok) {
    const unsigned long long tk = C.tok[t];
    pos = tk >> 1;
    const uint32_t kind = (uint32_t)(tk & 1ull);
    f = tx_segment_of(T.sb, T.S, pos);
    const uint64_t j = t - C.tfirst[f], nt = C.tfirst[f + 1] - C.tfirst[f];
    if ((EACH ? gate[f] == ~0ull : f < f_limit) && !(nt & 1ull)) {  // (else the file has been reported, or lies behind one that has)
      bad = kind != (uint32_t)(j & 1ull);
      if (!(j & 1ull)) {
        bad = bad || C.ctok[t] != (j == 0 ? C.cfile[f] : C.ctok[t - 1] + PD_END_CHARS);
      } else {
        is_end = true;
        cc = C.ctok[t] - C.ctok[t - 1] - PD_BEGIN_CHARS;
        ne = C.etok[t] - C.etok[t - 1];
        bad = bad || (cc & 3ull) || ne > 2 || (C.tok[t - 1] & 1ull) != PD_BEGIN;
        if (j + 1 == nt) bad = bad || C.cfile[f + 1] != C.ctok[t] + PD_END_CHARS;
        i = C.ffirst[f] + (j >> 1);
        p0 = C.tok[t - 1] >> 1;
        const uint64_t p1 = pos;
        if (!bad && cc) {
          // the body starts behind BEGIN's blank* LF
          uint64_t q = p0 + PD_BEGIN_LEN;
          for (uint32_t k = 0; k < PD_LMAX && q < p1 && pd_is_blank(T.s[q]); k++) q++;
          if (q >= p1 || T.s[q] != 0x0au) irregular = true;
          else {
            b = q + 1;
            const uint64_t ws = p1 - b - cc;  // >= 1: an LF lies in front of END
            if (ws == 1) e = 1;               // one line, ended by that LF
            else if (ws == 2 && T.s[p1 - 2] == 0x0du) e = 2;
            else {
              uint32_t l0 = 0;
              while (l0 <= PD_LMAX && b + l0 < p1 && !pd_is_ws(T.s[b + l0])) l0++;  // (stops at that LF at the latest)
              const uint32_t c = T.s[b + l0];
              e = c == 0x0au ? 1u : (c == 0x0du && T.s[b + l0 + 1] == 0x0au) ? 2u : 0u;
              L = l0;
              if (l0 == 0 || l0 > PD_LMAX || (l0 & 3u) || !e || ws % e) irregular = true;
              else {
                const uint64_t nl = ws / e;
                if (nl < 2 || (nl - 1) * L >= cc || cc > nl * L) irregular = true;
                else {  // with every eol at its arithmetic place no other ws is left: ws = e nl
                  const uint64_t own = nl - 1 < PD_OWN ? nl - 1 : PD_OWN;
                  for (uint64_t k = 1; k <= own && !irregular; k++) {
                    const uint64_t at = k + 1 < nl ? b + k * (L + e) + L : p1 - e;
                    irregular = T.s[at + e - 1] != 0x0au || (e == 2 && T.s[at] != 0x0du);
                  }
                  if (!irregular && nl - 1 > PD_OWN) w_nl = nl;
                }
              }
            }
          }
        }
      }
    }
  }
  // the long ones, one after the other, by the whole wave
  unsigned long long big = __ballot(w_nl != 0);
  while (big) {  // (wave-uniform)
    const int l = __ffsll(big) - 1;
    big &= big - 1ull;
    const unsigned long long xb = __shfl((unsigned long long)b, l), xp1 = __shfl((unsigned long long)pos, l), xnl = __shfl(w_nl, l);
    const uint32_t xL = __shfl(L, l), xe = __shfl(e, l);
    bool miss = false;
    for (unsigned long long k = PD_OWN + 1 + (threadIdx.x & 63u); k < xnl && !miss; k += 64ull) {
      const uint64_t at = k + 1 < xnl ? xb + k * (xL + xe) + xL : xp1 - xe;
      miss = T.s[at + xe - 1] != 0x0au || (xe == 2 && T.s[at] != 0x0du);
    }
    if (__ballot(miss) && (int)(threadIdx.x & 63u) == l) irregular = true;
  }
  if (is_end) {
    C.len[i] = bad ? 0ull : cc / 4 * 3 - ne;
    C.src[i] = irregular ? t - 1 : b;
    C.lay[i] = irregular ? PD_IRREGULAR : ((unsigned long long)L << 2) | e;
    C.sqlen[i] = irregular ? cc : 0ull;
    const uint64_t s0 = (uint64_t)(uintptr_t)T.s;
    C.sqtiles[i] = irregular ? (s0 + pos - 1 - T.a0) / TX_TILE - (s0 + p0 + PD_BEGIN_LEN - T.a0) / TX_TILE + 1 : 0ull;
  }
  const unsigned long long irr_m = __ballot(irregular);
  if ((threadIdx.x & 63u) == 0 && irr_m) atomicAdd(irr, (unsigned long long)__popcll(irr_m));
  pd_verdict<EACH>(err, T.S, bad, f, pos);
}

// the tables of the gather: what k_pd_check wrote under the old numbering, and where it goes
struct PdGather {
  const unsigned long long* bad_at;   // F: the verdicts
  const unsigned long long* ffirst0;  // F + 1: the scan of k_pd_files' counts, which k_pd_check numbered its certificates by
  const unsigned long long* ffirst;   // F + 1: the scan of k_ej_drop's counts
  const unsigned long long *len0, *src0, *lay0, *sqlen0, *sqtiles0;
  unsigned long long *len, *src, *lay, *sqlen, *sqtiles;
};

// each, behind the scan of k_ej_drop's counts: the five tables of the check compacted over the good files.  One lane per
// certificate i0 of the old numbering (n0 = ffirst0[F] > 0); its file is the last f with ffirst0[f] <= i0, which has
// certificates, so it is that one and no empty neighbour.  src of an irregular block is a token index: tokens keep their
// numbers.  *irr += the irregular blocks among the good files' certificates: the check has counted those of the files it
// found bad itself as well.
__global__ void __launch_bounds__(RP_BLOCK) k_pd_gather(uint64_t b0, uint64_t F, uint64_t n0, PdGather G, unsigned long long* irr) {
  const uint64_t i0 = (b0 + blockIdx.x) * RP_BLOCK + threadIdx.x;
  bool irregular = false;
  if (i0 < n0) {
    const uint64_t f = tx_segment_of((const uint64_t*)G.ffirst0, F, i0);
    if (G.bad_at[f] == ~0ull) {
      const uint64_t i = G.ffirst[f] + (i0 - G.ffirst0[f]);
      const unsigned long long lay = G.lay0[i0];
      G.len[i] = G.len0[i0];
      G.src[i] = G.src0[i0];
      G.lay[i] = lay;
      G.sqlen[i] = G.sqlen0[i0];
      G.sqtiles[i] = G.sqtiles0[i0];
      irregular = (lay & 3ull) == PD_IRREGULAR;
    }
  }
  const unsigned long long m = __ballot(irregular);
  if ((threadIdx.x & 63u) == 0 && m) atomicAdd(irr, (unsigned long long)__popcll(m));
}

// issuer: the issuer index of every certificate from its file's (ctmr_submit_pem): a lane per certificate i < n, its file
// the last f with ffirst[f] <= i (k_pd_gather's argument)
__global__ void __launch_bounds__(RP_BLOCK) k_pd_issuer(uint64_t b0, uint64_t F, uint64_t n, const unsigned long long* ffirst,
                                                        const uint32_t* file_issuer, uint32_t* issuer_idx) {
  const uint64_t i = (b0 + blockIdx.x) * RP_BLOCK + threadIdx.x;
  if (i < n) issuer_idx[i] = file_issuer[tx_segment_of((const uint64_t*)ffirst, F, i)];
}

// squeeze: block = tile t of irregular certificate i = tile_cert[t]: the characters of one mark block between the
// certificate's armor lines → sq[sqoff[i] + their rank in the body]
__global__ void __launch_bounds__(TX_BLOCK) k_pd_squeeze(TxText T, uint64_t b0, const unsigned long long* tile_cert, const unsigned long long* tile_first,
                                                         const unsigned long long* src, const unsigned long long* tok, const unsigned long long* ctok,
                                                         const unsigned long long* cnt_c, const unsigned long long* sqoff, uint8_t* sq) {
  const uint64_t t = b0 + blockIdx.x, i = tile_cert[t], k = t - tile_first[i];
  const uint64_t tb = src[i];
  const uint64_t from = (tok[tb] >> 1) + PD_BEGIN_LEN, to = tok[tb + 1] >> 1;
  const uint64_t blk = tx_block_of(T, from) + k;
  int64_t p0;
  uint32_t valid, total;
  const uint4 v = tx_chunk(T, blk, threadIdx.x, &p0, &valid);
  const uint32_t chars = tx_alphabet_mask<true>(v) & valid;
  const unsigned long long rank = cnt_c[blk] + tx_wave_scan((uint32_t)__popc(chars), &total) - (ctok[tb] + PD_BEGIN_CHARS);
  uint8_t* out = sq + sqoff[i];
  uint32_t m = chars;
  while (m) {
    const uint32_t q = (uint32_t)__ffs(m) - 1u;
    m &= m - 1u;
    const int64_t p = p0 + (int64_t)q;
    if (p >= (int64_t)from && p < (int64_t)to) out[rank + (uint32_t)__popc(chars & ((1u << q) - 1u))] = (uint8_t)tx_byte(v, q);
  }
}

// the tables of the decode
struct PdDecode {
  const unsigned long long* tile_cert;
  const unsigned long long* tile_first;
  const unsigned long long* offsets;  // n + 1: the scanned lengths
  const unsigned long long* src;
  const unsigned long long* lay;
  const unsigned long long* sqoff;
  const uint8_t* sq;
};

// decode: block = tile t of certificate i: its characters [TX_DTILE k, …) → payload[offsets[i] + TX_DOUT k, …)
__global__ void __launch_bounds__(TX_DBLOCK) k_pd_decode(const uint8_t* s, uint64_t b0, PdDecode D, uint8_t* payload) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[TX_DOUT + 16];
  const TxTile w = tx_tile(b0 + blockIdx.x, D.tile_cert, D.tile_first, D.offsets);
  const unsigned long long lay = D.lay[w.i];
  const bool squeezed = (lay & 3ull) == PD_IRREGULAR;
  const uint32_t L = squeezed ? 0u : (uint32_t)(lay >> 2), e = squeezed ? 0u : (uint32_t)(lay & 3ull);
  const uint64_t base = squeezed ? (uint64_t)(uintptr_t)D.sq + D.sqoff[w.i] : (uint64_t)(uintptr_t)s + D.src[w.i];
  const uint64_t r0 = w.k * TX_DTILE;  // the tile's first character; the line it lies in and where (block-uniform)
  const uint64_t line0 = L ? r0 / L : 0ull;
  const uint64_t in0 = L ? r0 % L : r0;
  if (tx_has_quantum(w)) {
    uint64_t a;
    if (L) {  // a quantum never straddles a line: L % 4 == 0
      const uint32_t m = (uint32_t)in0 + 4u * threadIdx.x;
      a = base + (line0 + m / L) * (uint64_t)(L + e) + m % L;
    } else {
      a = base + in0 + 4ull * threadIdx.x;
    }
    tx_stage_quantum(stage, w, a);
  }
  tx_tile_leaves(stage, w, payload);
}

}  // namespace ctmr
