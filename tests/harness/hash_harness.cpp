// Host build of the key hashing (csrc/ctmr_dev.h, csrc/kernels/keyrec.h) for the CPU tests: pins the Python port in
// tests/xchg_corpus.py to the product's own functions.
#include "../../ct_mapreduce_amd/csrc/kernels/keyrec.h"

extern "C" uint64_t harness_key_meta(int32_t exp_hour, uint32_t canon, uint32_t serial_len) {
  return ctmr::key_meta(exp_hour, canon, serial_len);
}
extern "C" uint64_t harness_mixk(uint64_t z) { return ctmr::mixk(z); }
extern "C" uint64_t harness_key_hash(uint64_t meta, const uint64_t* s) {
  const unsigned long long w[5] = {s[0], s[1], s[2], s[3], s[4]};
  return ctmr::key_hash(meta, w);
}
extern "C" uint32_t harness_key_tag(uint64_t h) { return ctmr::key_tag(h); }
extern "C" uint32_t harness_key_owner_h(uint64_t h, uint32_t world) { return ctmr::key_owner_h(h, world); }
extern "C" void harness_bloom_pos(uint64_t h, uint64_t wmask, uint64_t* word, uint64_t* bits) {
  uint64_t w;
  unsigned long long b;
  ctmr::bloom_pos(h, wmask, w, b);
  *word = w;
  *bits = b;
}
