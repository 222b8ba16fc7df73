// engine/synth.inc — synthetic generator entry points.
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after the engine state.

// ------------------------------------------------------------------ synthetic generator

uint32_t ctmr_synth_leaf_len(const ctmr_synth_config* c, uint64_t i) {
  const auto& cdf = host_cdf(c->n_issuers ? c->n_issuers : 1);
  SynthCfg s = to_synth(c, cdf.data());
  BackWriter w{nullptr, SYNTH_MAX_LEN};
  uint32_t iss; uint8_t et;
  synth_leaf_emit(s, i, w, iss, et);
  return SYNTH_MAX_LEN - w.pos;
}

uint32_t ctmr_synth_leaf(const ctmr_synth_config* c, uint64_t i, uint8_t* out, uint32_t cap,
                         uint32_t* issuer_idx, uint8_t* entry_type) {
  const auto& cdf = host_cdf(c->n_issuers ? c->n_issuers : 1);
  SynthCfg s = to_synth(c, cdf.data());
  uint8_t tmp[SYNTH_MAX_LEN];
  BackWriter w{tmp, SYNTH_MAX_LEN};
  uint32_t iss; uint8_t et;
  synth_leaf_emit(s, i, w, iss, et);
  const uint32_t len = SYNTH_MAX_LEN - w.pos;
  if (issuer_idx) *issuer_idx = iss;
  if (entry_type) *entry_type = et;
  if (out && len <= cap) memcpy(out, tmp + w.pos, len);
  return len;
}

uint32_t ctmr_synth_issuer(const ctmr_synth_config* c, uint32_t k, uint8_t* out, uint32_t cap) {
  SynthCfg s = to_synth(c, nullptr);
  uint8_t tmp[SYNTH_MAX_LEN];
  BackWriter w{tmp, SYNTH_MAX_LEN};
  synth_issuer_emit(s, k, w);
  const uint32_t len = SYNTH_MAX_LEN - w.pos;
  if (out && len <= cap) memcpy(out, tmp + w.pos, len);
  return len;
}

uint64_t ctmr_synth_host(const ctmr_synth_config* c, uint64_t first, uint64_t n, uint64_t* offsets,
                         uint8_t* payload, uint64_t cap, uint32_t* issuer_idx, uint8_t* entry_type) {
  const auto& cdf = host_cdf(c->n_issuers ? c->n_issuers : 1);
  SynthCfg s = to_synth(c, cdf.data());
  uint8_t tmp[SYNTH_MAX_LEN];
  uint64_t at = 0;
  if (offsets) offsets[0] = 0;
  for (uint64_t i = 0; i < n; i++) {
    BackWriter w{tmp, SYNTH_MAX_LEN};
    uint32_t iss; uint8_t et;
    synth_leaf_emit(s, first + i, w, iss, et);
    const uint32_t len = SYNTH_MAX_LEN - w.pos;
    if (payload && at + len <= cap) memcpy(payload + at, tmp + w.pos, len);
    at += len;
    if (offsets) offsets[i + 1] = at;
    if (issuer_idx) issuer_idx[i] = iss;
    if (entry_type) entry_type[i] = et;
  }
  return at;
}

int ctmr_synth_device(ctmr_engine* e, const ctmr_synth_config* c, uint64_t first, uint64_t n,
                      uint64_t* d_offsets, uint8_t* d_payload, uint64_t payload_cap,
                      uint32_t* d_issuer_idx, uint8_t* d_entry_type, uint64_t* payload_bytes) {
  if (!e || !c || !d_offsets) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (n == 0) return CTMR_OK;
  const uint32_t ni = c->n_issuers ? c->n_issuers : 1;
  const auto& cdf = host_cdf(ni);
  int r;
  if ((r = ensure(e, SC_MISC, (size_t)ni * 4))) return r;
  HIPCHK(e, hipMemcpyAsync(e->d_scratch[SC_MISC], cdf.data(), (size_t)ni * 4, hipMemcpyHostToDevice, e->stream));
  SynthCfg s = to_synth(c, (const uint32_t*)e->d_scratch[SC_MISC]);
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_synth_len, dim3(blocks), dim3(256), 0, e->stream, s, first, n, d_offsets);
  uint64_t total = 0;
  if ((r = scan_total(e, d_offsets + 1, n, true, SC_STAGE_B, &total, false))) return r;
  if (payload_bytes) *payload_bytes = total;
  if (!d_payload) return CTMR_OK;
  if (total + CTMR_PAYLOAD_PAD > payload_cap) return fail(e, CTMR_E_RANGE, "payload needs %llu bytes (+%d pad)", (unsigned long long)total, CTMR_PAYLOAD_PAD);
  if (!d_issuer_idx || !d_entry_type) return CTMR_E_INVAL;
  hipLaunchKernelGGL(k_synth_emit, dim3(blocks), dim3(256), 0, e->stream, s, first, n, (const uint64_t*)d_offsets,
                     d_payload, d_issuer_idx, d_entry_type);
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  return CTMR_OK;
}


int ctmr_synth_view_device(ctmr_engine* e, const ctmr_synth_config* c, uint64_t first, uint64_t n, uint32_t align,
                           uint64_t* d_starts, uint64_t* d_ends, uint8_t* d_payload, uint64_t payload_cap,
                           uint32_t* d_issuer_idx, uint8_t* d_entry_type, uint64_t* payload_bytes) {
  if (!e || !c || !d_starts || !d_ends || align == 0 || (align & (align - 1)) || align > 4096) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (n == 0) return CTMR_OK;
  const uint32_t ni = c->n_issuers ? c->n_issuers : 1;
  const auto& cdf = host_cdf(ni);
  int r;
  if ((r = ensure(e, SC_MISC, (size_t)ni * 4))) return r;
  HIPCHK(e, hipMemcpyAsync(e->d_scratch[SC_MISC], cdf.data(), (size_t)ni * 4, hipMemcpyHostToDevice, e->stream));
  SynthCfg s = to_synth(c, (const uint32_t*)e->d_scratch[SC_MISC]);
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_synth_len_view, dim3(blocks), dim3(256), 0, e->stream, s, first, n, align, d_starts, d_ends);
  uint64_t total = 0;
  if ((r = scan_total(e, d_starts + 1, n, true, SC_STAGE_B, &total, false))) return r;
  if (payload_bytes) *payload_bytes = total;
  if (!d_payload) return CTMR_OK;
  if (total + CTMR_PAYLOAD_PAD > payload_cap) return fail(e, CTMR_E_RANGE, "payload needs %llu bytes (+%d pad)", (unsigned long long)total, CTMR_PAYLOAD_PAD);
  if (!d_issuer_idx || !d_entry_type) return CTMR_E_INVAL;
  hipLaunchKernelGGL(k_synth_emit_view, dim3(blocks), dim3(256), 0, e->stream, s, first, n, (const uint64_t*)d_starts, d_ends,
                     d_payload, d_issuer_idx, d_entry_type);
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  return CTMR_OK;
}

uint64_t ctmr_synth_entries_host(const ctmr_synth_config* c, uint64_t first, uint64_t n, uint64_t* bounds,
                                 uint8_t* blob, uint64_t cap) {
  const auto& cdf = host_cdf(c->n_issuers ? c->n_issuers : 1);
  SynthCfg s = to_synth(c, cdf.data());
  std::vector<uint8_t> tmp(SYNTH_ENTRY_MAX);
  uint64_t at = 0;
  if (bounds) bounds[0] = 0;
  for (uint64_t i = 0; i < n; i++) {
    BackWriter w{tmp.data(), SYNTH_ENTRY_MAX};
    const uint32_t leaf = synth_entry_emit(s, first + i, w);
    const uint32_t len = SYNTH_ENTRY_MAX - w.pos;
    if (blob && at + len <= cap) memcpy(blob + at, tmp.data() + w.pos, len);
    if (bounds) {
      bounds[2 * i + 1] = at + leaf;
      bounds[2 * i + 2] = at + len;
    }
    at += len;
  }
  return at;
}

int ctmr_synth_entries_device(ctmr_engine* e, const ctmr_synth_config* c, uint64_t first, uint64_t n,
                              uint64_t* d_bounds, uint8_t* d_blob, uint64_t blob_cap, uint64_t* blob_bytes) {
  if (!e || !c || !d_bounds) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (n == 0) return CTMR_OK;
  const uint32_t ni = c->n_issuers ? c->n_issuers : 1;
  const auto& cdf = host_cdf(ni);
  int r;
  if ((r = ensure(e, SC_MISC, (size_t)ni * 4))) return r;
  HIPCHK(e, hipMemcpyAsync(e->d_scratch[SC_MISC], cdf.data(), (size_t)ni * 4, hipMemcpyHostToDevice, e->stream));
  SynthCfg s = to_synth(c, (const uint32_t*)e->d_scratch[SC_MISC]);
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_synth_entries_len, dim3(blocks), dim3(256), 0, e->stream, s, first, n, d_bounds);
  uint64_t total = 0;
  if ((r = scan_total(e, d_bounds + 1, 2 * n, true, SC_TMP, &total, false))) return r;
  if (blob_bytes) *blob_bytes = total;
  if (!d_blob) return CTMR_OK;
  if (total + CTMR_PAYLOAD_PAD > blob_cap) return fail(e, CTMR_E_RANGE, "blob needs %llu bytes (+%d pad)", (unsigned long long)total, CTMR_PAYLOAD_PAD);
  hipLaunchKernelGGL(k_synth_entries_emit, dim3(blocks), dim3(256), 0, e->stream, s, first, n, (const uint64_t*)d_bounds, d_blob);
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  return CTMR_OK;
}
