// kernels/crl.h — DER CertificateLists as they lie → the revoked serials as the member records of a probe image
// (include/ctmr.h ctmr_crl_probes*).  A revokedCertificates value is a run of length-prefixed entries whose
// serials and extension bodies are raw octets: an entry start cannot be found by pattern, and following the lengths is
// one dependent chain.  The shape is that of kernels/resp_parse.h, whose mark kernel is a template over the candidate
// predicate and whose cuts, conflict-region, compaction and chain kernels work on cand[] / nxt[] alone.  What is new here:
//   head      one lane per CRL walks the dozen outer TLVs → [lo, hi) of the revokedCertificates value, or the offset at
//             which the CRL leaves the grammar.
//   mark      CrlCand, the predicate k_resp_mark runs over: every byte inside some [lo, hi) is tested as an entry start
//             ("candidate": SEQUENCE { INTEGER, Time, optional SEQUENCE } filled exactly, ending at or before hi); every
//             true entry is one.  Two frame candidates
//             per CRL cover the bytes outside its value — its start → lo, hi → its end — so that the true chain runs
//             from 0 to len across all CRLs.
//   chain     (the each form) k_crl_chain: the chain proof with a finding per CRL instead of one for the blob.
//   class     per kept token, behind the chain proof: its CRL, whether it is a frame, a record (serial <= 40 octets) or a
//             host pair, and where its serial lies.
//   place     per record: its rank among the records of its CRL → one 48-byte member record of its issuer's set.
// Every read of the blob is a guarded byte load: the blob may lie at any alignment and no byte beyond len is read.
// gfx950 (CDNA4, wave64) only; part of kernels.h, which includes the pieces in dependency order.
#pragma once
#include "resp_parse.h"

namespace ctmr {

constexpr uint8_t CRL_FRAME = 0, CRL_RECORD = 1, CRL_PAIR = 2;  // a token's class

// the length octets at s[p] inside [.., end): definite and minimal — short form below 128, 81 from 128, 82 from 256, 83
// from 65 536, 84 from 2^24 — → where the contents start and where they end (<= end)
__device__ __forceinline__ bool crl_len(const uint8_t* s, uint64_t p, uint64_t end, uint64_t* body, uint64_t* next) {
  if (p >= end) return false;
  const uint32_t b = s[p];
  uint64_t v = b;
  uint32_t nb = 0u;
  if (b >= 0x80u) {
    nb = b - 0x80u;
    if (nb < 1u || nb > 4u || p + nb >= end) return false;
    v = 0;
    for (uint32_t k = 1; k <= nb; k++) v = (v << 8) | s[p + k];
    if (v < (nb == 1u ? 0x80ull : 1ull << (8u * (nb - 1u)))) return false;
  }
  *body = p + 1 + nb;
  *next = *body + v;
  return *next <= end;
}

__device__ __forceinline__ bool crl_tlv(const uint8_t* s, uint64_t p, uint64_t end, uint32_t* tag, uint64_t* body, uint64_t* next) {
  if (p >= end) return false;
  *tag = s[p];
  return crl_len(s, p + 1, end, body, next);
}

__device__ __forceinline__ bool crl_is_time(uint32_t tag) { return tag == 0x17u || tag == 0x18u; }

// the entry at s[i] inside a value that ends at hi: → its end, 0 when there is none; *serial = the offset of its serial's
// length octet.  One flag carried through and no early return, as der_walk.h does it.  (A first form with early returns
// and the end handed back through a pointer built into a mark pass that stored 0 for it: EXPERIMENTS.md has that
// form, the reproducer and the ISA; the cause is open.)
__device__ __forceinline__ uint64_t crl_entry(const uint8_t* s, uint64_t hi, uint64_t i, uint64_t* serial) {
  uint64_t b0 = 0, e = 0, body = 0, n1 = 0, n2 = 0, n3 = 0;
  uint32_t tag = 0;
  bool ok = s[i] == 0x30u && crl_len(s, i + 1, hi, &b0, &e);
  ok = ok && crl_tlv(s, b0, e, &tag, &body, &n1) && tag == 0x02u;
  ok = ok && crl_tlv(s, n1, e, &tag, &body, &n2) && crl_is_time(tag);
  if (ok && n2 != e) ok = crl_tlv(s, n2, e, &tag, &body, &n3) && tag == 0x30u && n3 == e;
  *serial = b0 + 1;
  return ok ? e : 0ull;
}

// the CRL of byte i among the CRLs k0..k1: the last one that starts at or before i (a CRL of 0 bytes holds no byte)
__device__ __forceinline__ uint32_t crl_of(const unsigned long long* off, uint32_t k0, uint32_t k1, uint64_t i) {
  while (k0 < k1) {
    const uint32_t mid = k0 + (k1 - k0 + 1u) / 2u;
    if (off[mid] <= i) k0 = mid;
    else k1 = mid - 1u;
  }
  return k0;
}

// head.  span[k] = [lo, hi) of CRL k's revokedCertificates value; lo == hi inside the CRL when it has none or an empty
// one; lo == hi == the CRL's end when the CRL is outside the grammar, and then err ← min(k << 32 | offset).
// EACH (ctmr_crl_probes_each*): err is bad_at, a word per CRL preset to all ones, and the CRL's own lane
// stores the offset into bad_at[k]: every refused CRL keeps its finding, nothing is reduced over the wave.
template <bool EACH>
__global__ void __launch_bounds__(RP_BLOCK) k_crl_head(const uint8_t* s, const unsigned long long* off, uint32_t n, uint2* span,
                                                       unsigned long long* err) {
  const uint64_t k = (uint64_t)blockIdx.x * RP_BLOCK + threadIdx.x;
  bool bad = false;
  uint64_t at = 0;
  if (k < n) {
    const uint64_t s0 = off[k], e = off[k + 1];
    uint64_t lo = e, hi = e, body, next, p = s0, tbs = 0;
    uint32_t tag = 0;
    // step by step; `at` is where the step that failed stood
    bool ok = crl_tlv(s, p, e, &tag, &body, &next) && tag == 0x30u;  // CertificateList
    at = p;
    if (ok && next != e) {
      ok = false;
      at = next;
    }
    if (ok) {
      p = body;
      at = p;
      ok = crl_tlv(s, p, e, &tag, &body, &tbs) && tag == 0x30u;  // tbsCertList
    }
    if (ok) {
      p = body;
      at = p;
      ok = crl_tlv(s, p, tbs, &tag, &body, &next);
      if (ok && tag == 0x02u) {  // version
        p = next;
        at = p;
        ok = crl_tlv(s, p, tbs, &tag, &body, &next);
      }
      ok = ok && tag == 0x30u;  // signature
      if (ok) {
        p = next;
        at = p;
        ok = crl_tlv(s, p, tbs, &tag, &body, &next) && tag == 0x30u;  // issuer
      }
      if (ok) {
        p = next;
        at = p;
        ok = crl_tlv(s, p, tbs, &tag, &body, &next) && crl_is_time(tag);  // thisUpdate
      }
      if (ok) {
        p = next;
        at = p;
        uint64_t vlo = p, vhi = p;
        bool have = p < tbs;
        if (have) ok = crl_tlv(s, p, tbs, &tag, &body, &next);
        if (ok && have && crl_is_time(tag)) {  // nextUpdate
          p = next;
          at = p;
          vlo = vhi = p;
          have = p < tbs;
          if (have) ok = crl_tlv(s, p, tbs, &tag, &body, &next);
        }
        if (ok && have && tag == 0x30u) {  // revokedCertificates
          vlo = body;
          vhi = next;
          p = next;
          at = p;
          have = p < tbs;
          if (have) ok = crl_tlv(s, p, tbs, &tag, &body, &next);
        }
        if (ok && have && tag == 0xA0u) {  // crlExtensions
          p = next;
          at = p;
          have = p < tbs;
        }
        ok = ok && !have;
        if (ok) {
          lo = vlo;
          hi = vhi;
        }
      }
    }
    if (ok) {
      p = tbs;
      at = p;
      ok = crl_tlv(s, p, e, &tag, &body, &next) && tag == 0x30u;  // signatureAlgorithm
    }
    if (ok) {
      p = next;
      at = p;
      ok = crl_tlv(s, p, e, &tag, &body, &next) && tag == 0x03u;  // signatureValue
    }
    if (ok && next != e) {
      ok = false;
      at = next;
    }
    if (!ok) lo = hi = e;
    span[k] = make_uint2((uint32_t)lo, (uint32_t)hi);
    bad = !ok;
  }
  if (EACH) {
    if (bad) err[k] = at;
  } else {
    rp_report(err, bad, (k << 32) | at);
  }
}

// tile_crl[t] = the CRL of byte 1024 t (t = 0 .. tiles; behind the blob: the last CRL)
__global__ void __launch_bounds__(RP_BLOCK) k_crl_tiles(const unsigned long long* off, uint32_t n, uint64_t tiles, uint32_t* tile_crl) {
  const uint64_t t = (uint64_t)blockIdx.x * RP_BLOCK + threadIdx.x;
  if (t <= tiles) tile_crl[t] = crl_of(off, 0u, n - 1u, t * RP_TILE);
}

struct CrlBlob {
  const uint8_t* s;
  uint64_t len;
  const unsigned long long* off;  // n + 1
  const uint2* span;              // n
  uint32_t n;
};

__device__ __forceinline__ bool crl_candidate(const CrlBlob& B, uint32_t k0, uint32_t k1, uint64_t i, uint32_t* next) {
  const uint32_t k = crl_of(B.off, k0, k1, i);
  const uint64_t s0 = B.off[k], e = B.off[k + 1];
  const uint2 sp = B.span[k];
  const bool front = i == s0;                  // the frame in front of the value (lo > s0 always)
  const bool behind = i == sp.y && sp.y < e;   // the frame behind it
  uint64_t end = 0, serial = 0;
  if (!front && !behind && i >= sp.x && i < sp.y) end = crl_entry(B.s, sp.y, i, &serial);
  *next = front ? sp.x : behind ? (uint32_t)e : (uint32_t)end;
  return front || behind || end != 0;
}

// the candidate predicate k_resp_mark takes (kernels/resp_parse.h RespCand): a block reads the CRLs of its tile's first
// byte and of the byte behind its last, and every byte is searched between the two
struct CrlCand {
  CrlBlob B;
  const uint32_t* tile_crl;
  __device__ __forceinline__ uint64_t bytes() const { return B.len; }
  __device__ __forceinline__ uint2 block() const { return make_uint2(tile_crl[blockIdx.x], tile_crl[blockIdx.x + 1]); }
  __device__ __forceinline__ bool operator()(uint2 k, uint64_t i, uint32_t* next) const { return crl_candidate(B, k.x, k.y, i, next); }
};

// chain, per CRL (EACH): the adjacency test of k_resp_chain<false>, and a lane with a mismatch blames its token's CRL:
// bad_at[k] ← min(the nxt that is not the next kept position).  The first byte of every CRL is a candidate no earlier
// one spans (no candidate reaches past its CRL's end), so it is kept: the tokens of CRL k are the sequential parse of
// CRL k iff no lane of CRL k reports, whatever its neighbours hold.  crl_of runs only on a mismatch.  A kernel of its
// own and not a parameter of k_resp_chain: that one knows a stream and one error word, this one needs the CRL table,
// and the RESP instantiation stays untouched.
__global__ void __launch_bounds__(RP_BLOCK) k_crl_chain(const uint32_t* tok_pos, const uint32_t* tok_nxt, uint64_t n, uint64_t len,
                                                        const unsigned long long* off, uint32_t n_crls, unsigned long long* bad_at) {
  const uint64_t t = (uint64_t)blockIdx.x * RP_BLOCK + threadIdx.x;
  if (t >= n) return;
  const uint64_t pos = tok_pos[t], nx = tok_nxt[t];
  const bool first = t == 0 && pos != 0;  // (off = 0, as k_resp_chain has it)
  if (!first && nx == (t + 1 < n ? (uint64_t)tok_pos[t + 1] : len)) return;
  atomicMin(bad_at + crl_of(off, 0u, n_crls - 1u, first ? 0ull : pos), first ? 0ull : (unsigned long long)nx);
}

// whether CRL k has a verdict: never without a bad_at table (the strict call), else bad_at[k] is not all ones
__device__ __forceinline__ bool crl_refused(uint32_t) { return false; }
__device__ __forceinline__ bool crl_refused(uint32_t k, const unsigned long long* bad_at) { return bad_at[k] != ~0ull; }

// class, behind the chain proof (every token is a frame or a true entry): cls[t], tok_crl[t], and for an entry tok_ser[t]
// = the offset of its serial's length octet.  EACH: behind k_crl_chain, where bad_at is final; every token of a CRL with
// a verdict is a frame, and crl_entry is not evaluated for it (its tokens are not proven to be entries).  bad_at is an
// argument of the EACH instantiation alone (BadAt = const unsigned long long*): <false> has the arguments, and so the
// code, it had before there was an each form.
template <bool EACH, class... BadAt>
__global__ void __launch_bounds__(RP_BLOCK) k_crl_class(CrlBlob B, const uint32_t* tok_pos, uint64_t n, uint8_t* cls, uint32_t* tok_crl,
                                                        uint32_t* tok_ser, BadAt... bad_at) {
  static_assert(sizeof...(BadAt) == (EACH ? 1 : 0), "bad_at with EACH, and only then");
  const uint64_t t = (uint64_t)blockIdx.x * RP_BLOCK + threadIdx.x;
  if (t >= n) return;
  const uint64_t i = tok_pos[t];
  const uint32_t k = crl_of(B.off, 0u, B.n - 1u, i);
  const uint2 sp = B.span[k];
  uint8_t c = CRL_FRAME;
  uint32_t ser = 0u;
  if (i != B.off[k] && i != sp.y && !crl_refused(k, bad_at...)) {
    uint64_t serial = 0, body = 0, next = 0;
    (void)crl_entry(B.s, sp.y, i, &serial);
    (void)crl_len(B.s, serial, sp.y, &body, &next);
    ser = (uint32_t)serial;
    c = next - body <= (uint64_t)CTMR_MAX_SERIAL ? CRL_RECORD : CRL_PAIR;
  }
  cls[t] = c;
  tok_crl[t] = k;
  tok_ser[t] = ser;
}

// crl_rec0[k] = the records in front of CRL k (rec_before of the frame at its start)
__global__ void __launch_bounds__(RP_BLOCK) k_crl_starts(CrlBlob B, const uint32_t* tok_pos, const uint32_t* tok_crl, const uint32_t* rec_before,
                                                         uint64_t n, uint32_t* crl_rec0) {
  const uint64_t t = (uint64_t)blockIdx.x * RP_BLOCK + threadIdx.x;
  if (t >= n) return;
  const uint32_t k = tok_crl[t];
  if (tok_pos[t] == B.off[k]) crl_rec0[k] = rec_before[t];
}

// pairs[pair_before[t]] = {offset of the serial, its length, its CRL, 0} for every CRL_PAIR token
__global__ void __launch_bounds__(RP_BLOCK) k_crl_pairs(CrlBlob B, const uint8_t* cls, const uint32_t* tok_crl, const uint32_t* tok_ser,
                                                        const uint32_t* pair_before, uint64_t n, uint4* pairs) {
  const uint64_t t = (uint64_t)blockIdx.x * RP_BLOCK + threadIdx.x;
  if (t >= n || cls[t] != CRL_PAIR) return;
  uint64_t body = 0, next = 0;
  (void)crl_len(B.s, tok_ser[t], B.len, &body, &next);
  pairs[pair_before[t]] = make_uint4((uint32_t)body, (uint32_t)(next - body), tok_crl[t], 0u);
}

// place: the record of every CRL_RECORD token → out[crl_dst[its CRL] + its rank among the records of that CRL]
__global__ void __launch_bounds__(RP_BLOCK) k_crl_place(const uint8_t* s, const uint8_t* cls, const uint32_t* tok_crl, const uint32_t* tok_ser,
                                                        const uint32_t* rec_before, const uint32_t* crl_rec0,
                                                        const unsigned long long* crl_dst, uint64_t n, uint8_t* out) {
  const uint64_t t = (uint64_t)blockIdx.x * RP_BLOCK + threadIdx.x;
  if (t >= n || cls[t] != CRL_RECORD) return;
  const uint32_t k = tok_crl[t];
  const uint64_t at = crl_dst[k] + (rec_before[t] - crl_rec0[k]);
  const uint8_t* m = s + tok_ser[t];
  known_store_octets(m[0], m + 1, out, at);  // (the length is <= 40: the short form)
}

}  // namespace ctmr
