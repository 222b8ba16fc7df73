// kernels/resp_parse.h — a Redis protocol stream of SADD / EXPIREAT commands as it lies → the member records of a
// known-certificate image (include/ctmr.h ctmr_known_resp_image*): the inverse of kernels/resp.h.
// RESP is length-prefixed and members are raw octets, so a member may hold "\r\n$3\r\n": token starts cannot be found by
// pattern alone, and following the lengths from byte 0 is one dependent chain.  The passes, each a launch of its own:
//   mark      every byte is tested as a token start ("candidate": '*' or '$' behind a CRLF, a well-formed number, CRLF;
//             a '$' must land on a CRLF inside the stream); every true token is one.  Counted per block, scanned, then
//             compacted to cand[] (ascending) and nxt[] (where the token says the next one starts).
//   cuts      M[k] = the largest nxt of the candidates before k (an exclusive prefix maximum); k is a cut iff
//             M[k] <= cand[k]: no earlier candidate's span contains it.  The true chain passes through every cut — the true
//             token covering a cut's position would otherwise cross it strictly.
//   resolve   behind a cut whose next candidate is no cut lies a conflict region (a fake header inside a member): one
//             lane follows nxt[] through the candidates, marks what it visits and stops at a cut or at a position that is
//             no candidate.  Regions are independent.  Without fake headers every candidate is a cut and no lane walks.
//   tokens    the kept candidates compacted; k_resp_chain then proves the list is the chain: it starts at 0, every nxt is
//             the next kept position, the last is len.  Nothing else is needed for exactness: whatever the passes before
//             kept, a list that passes is the one sequential parse.
//   commands  per '*' token: the argument count against the tokens behind it, the name, the key parsed exactly as
//             known_image.parse_key does, and whether the key differs from the command before (a run of equal keys).
//   place     per eligible member: its rank among the eligible members of its run → one 48-byte record.
// Every read of the stream is a guarded byte load: the stream may lie at any alignment and no byte beyond len is read.
// gfx950 (CDNA4, wave64) only; part of kernels.h, which includes the pieces in dependency order.
#pragma once
#include "image.h"

namespace ctmr {

constexpr uint32_t RP_BLOCK = 256, RP_PER = 4, RP_TILE = RP_BLOCK * RP_PER;  // items of a block: item it × 256 + lane
constexpr uint64_t RP_MAX_LEN = (1ull << 32) - 64;
// a command's class (low bits) and RP_HEAD: its key differs from the command before it
constexpr uint8_t RP_IGNORED = 0, RP_SKIPPED = 1, RP_SET_KEY = 2, RP_HOST_KEY = 3, RP_HEAD = 0x10;
// a token's part: a member record, or a (key, member) pair of the host section
constexpr uint8_t RP_RECORD = 1, RP_PAIR = 2;

// the number behind the '*' or '$' at s[i]: 1..10 digits without a leading zero ("0" itself allowed), then CRLF, all
// inside the stream → hdr = the bytes up to and including that CRLF
__device__ __forceinline__ bool rp_number(const uint8_t* s, uint64_t len, uint64_t i, uint64_t* v, uint32_t* hdr) {
  uint64_t val = 0, q = i + 1;
  uint32_t nd = 0;
  while (nd < 10u && q < len) {
    const uint32_t c = s[q];
    if (c < '0' || c > '9') break;
    val = val * 10ull + (c - '0');
    nd++;
    q++;
  }
  if (nd == 0u || (nd > 1u && s[i + 1] == '0')) return false;
  if (q + 2 > len || s[q] != '\r' || s[q + 1] != '\n') return false;
  *v = val;
  *hdr = nd + 3u;
  return true;
}

__device__ __forceinline__ bool rp_candidate(const uint8_t* s, uint64_t len, uint64_t i, uint32_t* next) {
  const uint32_t c = s[i];
  if (c != '*' && c != '$') return false;
  if (i != 0 && (i < 2 || s[i - 2] != '\r' || s[i - 1] != '\n')) return false;
  uint64_t v;
  uint32_t hdr;
  if (!rp_number(s, len, i, &v, &hdr)) return false;
  uint64_t nx = i + hdr;  // <= len: rp_number saw the CRLF
  if (c == '$') {
    nx += v + 2;
    if (nx > len || s[nx - 2] != '\r' || s[nx - 1] != '\n') return false;
  }
  *next = (uint32_t)nx;
  return true;
}

// the first failure's offset: one atomicMin per wave that saw one (every lane of the wave calls)
__device__ __forceinline__ void rp_report(unsigned long long* err, bool bad, uint64_t off) {
  unsigned long long v = bad ? (unsigned long long)off : ~0ull;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(v, d);
    v = o < v ? o : v;
  }
  if ((threadIdx.x & 63u) == 0 && v != ~0ull) atomicMin(err, v);
}

// the items of the block before this one that are set (a block-wide exclusive count; every thread calls; ws: 4 words)
__device__ __forceinline__ uint32_t rp_block_rank(bool set, uint32_t* ws, uint32_t* total) {
  const unsigned long long b = __ballot(set);
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  __syncthreads();  // (ws of the item before is read)
  if (lane == 0) ws[wv] = (uint32_t)__popcll(b);
  __syncthreads();
  uint32_t pre = 0u, all = 0u;
#pragma unroll
  for (uint32_t k = 0; k < RP_BLOCK / 64; k++) {
    pre += k < wv ? ws[k] : 0u;
    all += ws[k];
  }
  *total = all;
  return pre + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
}

// the candidate predicate of a RESP stream, as k_resp_mark takes it: bytes() = how many to test, block() = what the
// predicate reads once per block (nothing here), (that, i, &next) = whether byte i is a candidate and where it says the
// next token starts
struct RespCand {
  const uint8_t* s;
  uint64_t len;
  struct Block {};
  __device__ __forceinline__ uint64_t bytes() const { return len; }
  __device__ __forceinline__ Block block() const { return {}; }
  __device__ __forceinline__ bool operator()(Block, uint64_t i, uint32_t* next) const { return rp_candidate(s, len, i, next); }
};

// mark.  WRITE = false: cnt[blk] = the candidates among the bytes [1024 blk, 1024 blk + 1024).
// WRITE = true, behind the exclusive scan of cnt[]: cand[] / nxt[] of those candidates, ascending.
template <bool WRITE, class Cand>
__global__ void __launch_bounds__(RP_BLOCK) k_resp_mark(Cand C, unsigned long long* cnt, uint32_t* cand, uint32_t* nxt) {
  __shared__ uint32_t ws[RP_BLOCK / 64];
  const uint64_t base = WRITE ? cnt[blockIdx.x] : 0ull;
  const auto blk = C.block();
  uint32_t run = 0u;
#pragma unroll 1
  for (uint32_t it = 0; it < RP_PER; it++) {
    const uint64_t i = (uint64_t)blockIdx.x * RP_TILE + it * RP_BLOCK + threadIdx.x;
    uint32_t nx = 0u, all;
    const bool c = i < C.bytes() && C(blk, i, &nx);
    const uint32_t rank = rp_block_rank(c, ws, &all);
    if (WRITE && c) {
      cand[base + run + rank] = (uint32_t)i;
      nxt[base + run + rank] = nx;
    }
    run += all;
  }
  if (!WRITE && threadIdx.x == 0) cnt[blockIdx.x] = run;
}

// cuts, 1: bm[blk] = the largest nxt of the block's candidates
__global__ void __launch_bounds__(RP_BLOCK) k_resp_blockmax(const uint32_t* nxt, uint64_t n, uint32_t* bm) {
  __shared__ uint32_t ws[RP_BLOCK / 64];
  uint32_t m = 0u;
  for (uint32_t it = 0; it < RP_PER; it++) {
    const uint64_t k = (uint64_t)blockIdx.x * RP_TILE + it * RP_BLOCK + threadIdx.x;
    if (k < n) m = max(m, nxt[k]);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor(m, d));
  if ((threadIdx.x & 63u) == 0) ws[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) bm[blockIdx.x] = max(max(ws[0], ws[1]), max(ws[2], ws[3]));
}

// cuts, 2: bm[] → its exclusive prefix maximum, in place; one block (k_scan64_sums with max for +)
__global__ void __launch_bounds__(1024) k_resp_maxscan(uint32_t* bm, uint64_t nb) {
  __shared__ uint32_t part[1024];
  const uint64_t per = (nb + 1023) / 1024;
  const uint64_t lo = (uint64_t)threadIdx.x * per < nb ? (uint64_t)threadIdx.x * per : nb;
  const uint64_t hi = lo + per < nb ? lo + per : nb;
  uint32_t m = 0u;
  for (uint64_t i = lo; i < hi; i++) m = max(m, bm[i]);
  part[threadIdx.x] = m;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    const uint32_t t = threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
    __syncthreads();
    part[threadIdx.x] = max(part[threadIdx.x], t);
    __syncthreads();
  }
  uint32_t run = threadIdx.x ? part[threadIdx.x - 1] : 0u;
  for (uint64_t i = lo; i < hi; i++) {
    const uint32_t v = bm[i];
    bm[i] = run;
    run = max(run, v);
  }
}

// cuts, 3: flag[k] = 1 iff no earlier candidate's nxt lies beyond cand[k]
__global__ void __launch_bounds__(RP_BLOCK) k_resp_cuts(const uint32_t* cand, const uint32_t* nxt, uint64_t n, const uint32_t* bm,
                                                        uint8_t* flag) {
  __shared__ uint32_t ws[RP_BLOCK / 64];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint32_t carry = bm[blockIdx.x];
#pragma unroll 1
  for (uint32_t it = 0; it < RP_PER; it++) {
    const uint64_t k = (uint64_t)blockIdx.x * RP_TILE + it * RP_BLOCK + threadIdx.x;
    const uint32_t v = k < n ? nxt[k] : 0u;
    uint32_t inc = v;  // the wave's inclusive prefix maximum
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(inc, d);
      if ((int)lane >= d) inc = max(inc, o);
    }
    uint32_t before = __shfl_up(inc, 1);
    if (lane == 0) before = 0u;
    __syncthreads();
    if (lane == 63u) ws[wv] = inc;
    __syncthreads();
    uint32_t all = carry;
#pragma unroll
    for (uint32_t w = 0; w < RP_BLOCK / 64; w++) {
      if (w < wv) before = max(before, ws[w]);
      all = max(all, ws[w]);
    }
    before = max(before, carry);
    if (k < n) flag[k] = before <= cand[k] ? 1u : 0u;
    carry = all;
  }
}

// resolve: the lane of a cut whose next candidate is no cut walks the region behind it
__global__ void __launch_bounds__(RP_BLOCK) k_resp_resolve(const uint32_t* cand, const uint32_t* nxt, uint64_t n, uint8_t* flag) {
  const uint64_t k = (uint64_t)blockIdx.x * RP_BLOCK + threadIdx.x;
  if (k + 1 >= n || !(flag[k] & 1u) || (flag[k + 1] & 1u)) return;
  uint32_t p = nxt[k];
  uint64_t from = k + 1;
  for (;;) {
    uint64_t lo = from, hi = n;  // the first candidate at or behind p
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (cand[mid] < p) lo = mid + 1;
      else hi = mid;
    }
    if (lo >= n || cand[lo] != p || (flag[lo] & 1u)) return;
    flag[lo] = 2u;
    p = nxt[lo];  // > cand[lo]: the walk ends
    from = lo + 1;
  }
}

// cnt[blk] = the items of flag[1024 blk ..) with a bit of mask set; then, behind the exclusive scan of cnt[]: idx[i] =
// the set items before item i (written for every item)
__global__ void __launch_bounds__(RP_BLOCK) k_resp_flag_count(const uint8_t* flag, uint64_t n, uint32_t mask, unsigned long long* cnt) {
  __shared__ uint32_t ws[RP_BLOCK / 64];
  uint32_t run = 0u;
  for (uint32_t it = 0; it < RP_PER; it++) {
    const uint64_t i = (uint64_t)blockIdx.x * RP_TILE + it * RP_BLOCK + threadIdx.x;
    run += (uint32_t)__popcll(__ballot(i < n && (flag[i] & mask)));
  }
  if ((threadIdx.x & 63u) == 0) ws[threadIdx.x >> 6] = run;
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

__global__ void __launch_bounds__(RP_BLOCK) k_resp_flag_index(const uint8_t* flag, uint64_t n, uint32_t mask, const unsigned long long* cnt,
                                                              uint32_t* idx) {
  __shared__ uint32_t ws[RP_BLOCK / 64];
  uint32_t run = (uint32_t)cnt[blockIdx.x];
#pragma unroll 1
  for (uint32_t it = 0; it < RP_PER; it++) {
    const uint64_t i = (uint64_t)blockIdx.x * RP_TILE + it * RP_BLOCK + threadIdx.x;
    uint32_t all;
    const uint32_t rank = rp_block_rank(i < n && (flag[i] & mask), ws, &all);
    if (i < n) idx[i] = run + rank;
    run += all;
  }
}

// tokens: the kept candidates (flag != 0) to their places tidx[k].  RESP: also hdr = the bytes of "*<N>\r\n" / "$<L>\r\n"
// and star = whether the token is a '*'; a caller with other tokens (kernels/crl.h) has neither table and s is not read
template <bool RESP>
__global__ void __launch_bounds__(RP_BLOCK) k_resp_tokens(const uint8_t* s, uint64_t len, const uint32_t* cand, const uint32_t* nxt,
                                                          const uint8_t* flag, const uint32_t* tidx, uint64_t n, uint32_t* tok_pos,
                                                          uint32_t* tok_nxt, uint8_t* tok_hdr, uint8_t* star) {
  const uint64_t k = (uint64_t)blockIdx.x * RP_BLOCK + threadIdx.x;
  if (k >= n || !flag[k]) return;
  const uint32_t t = tidx[k], pos = cand[k];
  uint64_t v;
  uint32_t hdr = 0u;
  if (RESP) (void)rp_number(s, len, pos, &v, &hdr);
  tok_pos[t] = pos;
  tok_nxt[t] = nxt[k];
  if (RESP) {
    tok_hdr[t] = (uint8_t)hdr;
    star[t] = s[pos] == '*' ? 1u : 0u;
  }
}

// chain: the tokens are the sequential parse iff this finds nothing: the list starts at 0 (STAR: with a '*'; a caller
// whose first token need not be one, kernels/crl.h, passes no star[]), every nxt is the next kept position, the last is len
template <bool STAR>
__global__ void __launch_bounds__(RP_BLOCK) k_resp_chain(const uint32_t* tok_pos, const uint32_t* tok_nxt, const uint8_t* star, uint64_t n,
                                                         uint64_t len, unsigned long long* err) {
  const uint64_t t = (uint64_t)blockIdx.x * RP_BLOCK + threadIdx.x;
  bool bad = false;
  uint64_t off = 0;
  if (t < n) {
    if (t == 0 && (tok_pos[0] != 0u || (STAR && !star[0]))) bad = true;  // (off = 0)
    else if (tok_nxt[t] != (t + 1 < n ? (uint64_t)tok_pos[t + 1] : len)) {
      bad = true;
      off = tok_nxt[t];
    }
  }
  rp_report(err, bad, off);
}

// cmd_tok[c] = the token of command c (cidx[t]: the '*' tokens before t)
__global__ void __launch_bounds__(RP_BLOCK) k_resp_cmdtok(const uint8_t* star, const uint32_t* cidx, uint64_t n, uint32_t* cmd_tok) {
  const uint64_t t = (uint64_t)blockIdx.x * RP_BLOCK + threadIdx.x;
  if (t < n && star[t]) cmd_tok[cidx[t]] = (uint32_t)t;
}

// the n octets at s + at against an upper-case name, in any ASCII case (x & 0xdf is a capital only for the two cases of it)
template <uint32_t N>
__device__ __forceinline__ bool rp_name_is(const uint8_t* s, uint64_t at, const char (&name)[N]) {
  bool ok = true;
#pragma unroll
  for (uint32_t k = 0; k + 1u < N; k++) ok = ok && (s[at + k] & 0xdfu) == (uint8_t)name[k];
  return ok;
}

__device__ __forceinline__ bool rp_digit(uint32_t c) { return c >= '0' && c <= '9'; }

// known_image.parse_key on a key that starts with "serials::": exactly 68 octets, "dddd-dd-dd-dd" of a real calendar date
// and an hour 00..23, "::", 43 characters of the url-safe alphabet with the two spare bits of the last zero, '='
__device__ __forceinline__ bool rp_set_key(const uint8_t* k, uint32_t n) {
  if (n != 68u) return false;
  uint32_t d[13];
#pragma unroll
  for (uint32_t i = 0; i < 13; i++) d[i] = k[9 + i];
  bool ok = d[4] == '-' && d[7] == '-' && d[10] == '-' && k[22] == ':' && k[23] == ':' && k[67] == '=';
#pragma unroll
  for (uint32_t i = 0; i < 13; i++)
    if (i != 4 && i != 7 && i != 10) ok = ok && rp_digit(d[i]);
  if (!ok) return false;
  const uint32_t y = (d[0] - '0') * 1000u + (d[1] - '0') * 100u + (d[2] - '0') * 10u + (d[3] - '0');
  const uint32_t m = (d[5] - '0') * 10u + (d[6] - '0'), day = (d[8] - '0') * 10u + (d[9] - '0'), h = (d[11] - '0') * 10u + (d[12] - '0');
  const bool leap = y % 4u == 0u && (y % 100u != 0u || y % 400u == 0u);
  const uint32_t dim = m == 2u ? (leap ? 29u : 28u) : ((m == 4u || m == 6u || m == 9u || m == 11u) ? 30u : 31u);
  if (m < 1u || m > 12u || day < 1u || day > dim || h > 23u) return false;
  uint32_t last = 0u;
  for (uint32_t i = 0; i < 43u; i++) {
    const uint32_t c = k[24 + i];
    uint32_t v;
    if (c >= 'A' && c <= 'Z') v = c - 'A';
    else if (c >= 'a' && c <= 'z') v = c - 'a' + 26u;
    else if (rp_digit(c)) v = c - '0' + 52u;
    else if (c == '-') v = 62u;
    else if (c == '_') v = 63u;
    else return false;
    last = v;
  }
  return (last & 3u) == 0u;
}

struct RespTokens {
  const uint8_t* s;
  uint64_t len;
  const uint32_t* pos;
  const uint32_t* nxt;
  const uint8_t* hdr;
  uint64_t n;
  __device__ __forceinline__ uint32_t data(uint64_t t) const { return pos[t] + hdr[t]; }              // a bulk string's octets
  __device__ __forceinline__ uint32_t size(uint64_t t) const { return nxt[t] - pos[t] - hdr[t] - 2u; }  // … and how many
};

// commands: cls[c] = the class of command c, | RP_HEAD when it opens a run; err[0] ← the offset of the first command that
// is not one of the four or has the wrong number of arguments; err[1] += the members of the skipped ones
__global__ void __launch_bounds__(RP_BLOCK) k_resp_commands(RespTokens T, const uint32_t* cmd_tok, uint64_t ncmd, uint8_t* cls,
                                                            unsigned long long* err) {
  const uint64_t c = (uint64_t)blockIdx.x * RP_BLOCK + threadIdx.x;
  bool bad = false;
  uint64_t off = 0;
  unsigned long long skipped = 0;
  if (c < ncmd) {
    const uint64_t t = cmd_tok[c], end = c + 1 < ncmd ? (uint64_t)cmd_tok[c + 1] : T.n;
    off = T.pos[t];
    uint64_t argc = 0;
    uint32_t hdr;
    (void)rp_number(T.s, T.len, off, &argc, &hdr);
    uint8_t k = RP_IGNORED;
    if (argc < 1 || t + 1 + argc != end) {
      bad = true;
    } else {
      const uint32_t at = T.data(t + 1), nl = T.size(t + 1);
      if (nl == 4u && rp_name_is(T.s, at, "SADD")) {
        if (argc < 3) {
          bad = true;
        } else {
          const uint32_t ka = T.data(t + 2), kl = T.size(t + 2);
          bool serials = kl >= 9u;
          if (serials) {
            const char pre[] = "serials::";
#pragma unroll
            for (uint32_t i = 0; i < 9; i++) serials = serials && T.s[ka + i] == (uint8_t)pre[i];
          }
          if (!serials) {
            k = RP_SKIPPED;
            skipped = argc - 2;
          } else {
            k = rp_set_key(T.s + ka, kl) ? RP_SET_KEY : RP_HOST_KEY;
            bool same = false;  // the command before is a SADD of the same key
            if (c > 0) {
              const uint64_t tp = cmd_tok[c - 1];
              if (t - tp >= 3 && T.size(tp + 1) == 4u && rp_name_is(T.s, T.data(tp + 1), "SADD") && T.size(tp + 2) == kl) {
                const uint32_t pa = T.data(tp + 2);
                same = true;
                for (uint32_t i = 0; i < kl && same; i++) same = T.s[pa + i] == T.s[ka + i];
              }
            }
            if (!same) k |= RP_HEAD;
          }
        }
      } else if ((nl == 8u && rp_name_is(T.s, at, "EXPIREAT")) || (nl == 9u && rp_name_is(T.s, at, "PEXPIREAT"))) {
        bad = argc != 3;
      } else if (nl == 6u && rp_name_is(T.s, at, "SELECT")) {
        bad = argc != 2;
      } else {
        bad = true;
      }
    }
    cls[c] = bad ? RP_IGNORED : k;
  }
  rp_report(err, bad, off);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) skipped += __shfl_xor(skipped, d);
  if ((threadIdx.x & 63u) == 0 && skipped) atomicAdd(err + 1, skipped);
}

// what the tables of the later passes say of a token's command
struct RespCmds {
  const uint32_t* cidx;     // per token: the '*' tokens before it
  const uint32_t* cmd_tok;  // per command: its token
  const uint8_t* cls;       // per command
  const uint32_t* ridx;     // per command: the run heads before it
  __device__ __forceinline__ uint32_t run(uint32_t c) const { return ridx[c] + ((cls[c] & RP_HEAD) ? 1u : 0u) - 1u; }
};

// part[t]: RP_RECORD for a member of at most 40 octets under a set key, RP_PAIR for every other member under serials::
__global__ void __launch_bounds__(RP_BLOCK) k_resp_parts(RespTokens T, const uint8_t* star, RespCmds C, uint8_t* part) {
  const uint64_t t = (uint64_t)blockIdx.x * RP_BLOCK + threadIdx.x;
  if (t >= T.n) return;
  uint8_t p = 0u;
  if (!star[t]) {
    const uint32_t c = C.cidx[t] - 1u;
    const uint32_t k = C.cls[c] & 0xfu;
    if (t - C.cmd_tok[c] >= 3u && k >= RP_SET_KEY)  // (behind the name and the key)
      p = k == RP_SET_KEY && T.size(t) <= (uint32_t)CTMR_MAX_SERIAL ? RP_RECORD : RP_PAIR;
  }
  part[t] = p;
}

// runs[r] = {offset of the key, its length, the records of the runs before (rec_before of its first member), class}
__global__ void __launch_bounds__(RP_BLOCK) k_resp_runs(RespTokens T, RespCmds C, uint64_t ncmd, const uint32_t* rec_before, uint4* runs) {
  const uint64_t c = (uint64_t)blockIdx.x * RP_BLOCK + threadIdx.x;
  if (c >= ncmd || !(C.cls[c] & RP_HEAD)) return;
  const uint64_t t = C.cmd_tok[c];
  runs[C.ridx[c]] = make_uint4(T.data(t + 2), T.size(t + 2), rec_before[t + 3], (uint32_t)(C.cls[c] & 0xfu));
}

// pairs[pair_before[t]] = {offset of the member, its length, its run, 0} for every RP_PAIR token
__global__ void __launch_bounds__(RP_BLOCK) k_resp_pairs(RespTokens T, RespCmds C, const uint8_t* part, const uint32_t* pair_before,
                                                         uint4* pairs) {
  const uint64_t t = (uint64_t)blockIdx.x * RP_BLOCK + threadIdx.x;
  if (t >= T.n || part[t] != RP_PAIR) return;
  pairs[pair_before[t]] = make_uint4(T.data(t), T.size(t), C.run(C.cidx[t] - 1u), 0u);
}

// gather: segment g = seg[g].y octets at stream offset seg[g].x → out + dst[g]; one wave per segment
__global__ void __launch_bounds__(RP_BLOCK) k_resp_gather(const uint8_t* s, const uint2* seg, const unsigned long long* dst, uint64_t n,
                                                          uint8_t* out) {
  const uint64_t g = (uint64_t)blockIdx.x * (RP_BLOCK / 64) + (threadIdx.x >> 6);
  if (g >= n) return;
  const uint2 sg = seg[g];
  uint8_t* o = out + dst[g];
  for (uint32_t i = threadIdx.x & 63u; i < sg.y; i += 64u) o[i] = s[(uint64_t)sg.x + i];
}

// place: the record of every RP_RECORD token → out[run_dst[run] + its rank among the records of its run]
__global__ void __launch_bounds__(RP_BLOCK) k_resp_place(RespTokens T, RespCmds C, const uint8_t* part, const uint32_t* rec_before,
                                                         const uint4* runs, const unsigned long long* run_dst, uint8_t* out) {
  const uint64_t t = (uint64_t)blockIdx.x * RP_BLOCK + threadIdx.x;
  if (t >= T.n || part[t] != RP_RECORD) return;
  const uint32_t r = C.run(C.cidx[t] - 1u);
  const uint64_t at = run_dst[r] + (rec_before[t] - runs[r].z);
  known_store_octets(T.size(t), T.s + T.data(t), out, at);
}

}  // namespace ctmr
