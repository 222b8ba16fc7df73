// engine/pem.inc — whole-certificate SHA-256 (auxiliary) and PEM write-back (N1).
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after the engine state.

// ------------------------------------------------------------------ whole-certificate SHA-256 (auxiliary)
int ctmr_fingerprint_device(ctmr_engine* e, const uint8_t* d_payload, const uint64_t* d_offsets,
                            const uint64_t* d_ends, uint64_t n, uint8_t* d_digests, float* ms) {
  if (!e || (n && (!d_payload || !d_offsets || !d_digests))) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (ms) *ms = 0.f;
  if (n == 0) return CTMR_OK;
  if (((uintptr_t)d_digests & 15) != 0) return fail(e, CTMR_E_INVAL, "digests must be 16-byte aligned");
  HIPCHK(e, hipEventRecord(e->ev[5], e->stream));
  hipLaunchKernelGGL(k_fingerprint, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, d_payload, d_offsets,
                     d_ends, n, (uint32_t*)d_digests);
  HIPCHK(e, hipEventRecord(e->ev[6], e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  if (ms) (void)hipEventElapsedTime(ms, e->ev[5], e->ev[6]);
  return CTMR_OK;
}

// ------------------------------------------------------------------ PEM write-back (N1)

static int pem_device_locked(ctmr_engine* e, const uint8_t* d_payload, const uint64_t* d_offsets,
                             const uint64_t* d_idx, uint64_t n_idx, uint8_t* d_pem, uint64_t pem_cap,
                             uint64_t* d_pem_offsets, uint64_t* pem_bytes, const uint64_t* d_ends = nullptr) {
  HIPCHK(e, hipSetDevice(e->device));
  if (pem_bytes) *pem_bytes = 0;
  if (n_idx == 0) {
    if (d_pem_offsets) HIPCHK(e, hipMemsetAsync(d_pem_offsets, 0, 8, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return CTMR_OK;
  }
  if (n_idx >= 0x7fffffffull) return fail(e, CTMR_E_INVAL, "too many certificates in one PEM call");
  int r;
  if ((r = ensure(e, SC_PEMINFO, n_idx * sizeof(PemCertInfo)))) return r;
  PemCertInfo* d_info = (PemCertInfo*)e->d_scratch[SC_PEMINFO];
  hipLaunchKernelGGL(k_pem_len, dim3((unsigned)((n_idx + 1 + 255) / 256)), dim3(256), 0, e->stream, d_offsets, d_ends,
                     d_idx, n_idx, d_pem_offsets, d_info);
  uint64_t total = 0;
  if ((r = scan_total(e, d_pem_offsets, n_idx + 1, false, SC_TMP, &total, false))) return r;
  if (pem_bytes) *pem_bytes = total;
  if (!d_pem) return CTMR_OK;  // size query
  if (total > pem_cap) return fail(e, CTMR_E_RANGE, "PEM buffer too small: need %llu bytes", (unsigned long long)total);
  {  // the stream is cut into 7 KiB output blocks on 16-byte boundaries of the OUTPUT ADDRESS (kernels/pem.h)
    const uint32_t a = (uint32_t)((uintptr_t)d_pem & 15u);
    const uint64_t nb = (total + a + PEM_S - 1) / PEM_S;
    if ((r = ensure(e, SC_PEMBLK, nb * 4))) return r;
    uint32_t* d_first = (uint32_t*)e->d_scratch[SC_PEMBLK];
    hipLaunchKernelGGL(k_pem_blocks, dim3((unsigned)((n_idx + 255) / 256)), dim3(256), 0, e->stream,
                       (const uint64_t*)d_pem_offsets, n_idx, a, d_first);
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device);
    int per_cu = 0;  // workgroups of this kernel a CU holds (registers and LDS decide): the grid is what is resident at once
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pem_encode, 64 * PEM_WAVES, PEM_LDS_BYTES) != hipSuccess || per_cu < 1) {
      (void)hipGetLastError();
      per_cu = 4;
    }
    const uint64_t wgs = (nb + PEM_WAVES - 1) / PEM_WAVES, resident = (uint64_t)cus * (uint64_t)per_cu;
    hipLaunchKernelGGL(k_pem_encode, dim3((unsigned)(wgs < resident ? wgs : resident)), dim3(64 * PEM_WAVES), PEM_LDS_BYTES,
                       e->stream, d_payload, (const PemCertInfo*)d_info, n_idx, (const uint64_t*)d_pem_offsets,
                       (const uint32_t*)d_first, nb, total, a, d_pem);
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  return CTMR_OK;
}

int ctmr_pem_encode_device(ctmr_engine* e, const uint8_t* d_payload, const uint64_t* d_offsets,
                           const uint64_t* d_idx, uint64_t n_idx, uint8_t* d_pem, uint64_t pem_cap,
                           uint64_t* d_pem_offsets, uint64_t* pem_bytes) {
  if (!e || !d_pem_offsets || (n_idx && (!d_payload || !d_offsets || !d_idx))) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  return pem_device_locked(e, d_payload, d_offsets, d_idx, n_idx, d_pem, pem_cap, d_pem_offsets, pem_bytes);
}

int ctmr_pem_encode_view_device(ctmr_engine* e, const uint8_t* d_blob, const ctmr_entry_view* v,
                                const uint64_t* d_idx, uint64_t n_idx, uint8_t* d_pem, uint64_t pem_cap,
                                uint64_t* d_pem_offsets, uint64_t* pem_bytes) {
  if (!e || !v || !d_pem_offsets || (n_idx && (!d_blob || !v->cert_start || !v->cert_end || !d_idx))) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  return pem_device_locked(e, d_blob, v->cert_start, d_idx, n_idx, d_pem, pem_cap, d_pem_offsets, pem_bytes, v->cert_end);
}

int ctmr_pem_new(ctmr_engine* e, uint8_t* out, size_t cap, uint64_t* pem_offsets, size_t* need, uint64_t* count) {
  if (!e) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  const uint64_t nn = e->last_n_new;
  if (count) *count = nn;
  if (need) *need = 0;
  if (nn == 0) {
    if (pem_offsets) pem_offsets[0] = 0;
    return CTMR_OK;
  }
  int r;
  if ((r = ensure(e, SC_PEMOFF, (nn + 1) * 8))) return r;
  uint8_t* B = (uint8_t*)e->d_scratch[SC_STAGE_B];
  uint64_t* d_po = (uint64_t*)e->d_scratch[SC_PEMOFF];
  uint64_t total = 0;
  const uint8_t* V = (const uint8_t*)e->d_scratch[SC_VIEW];
  const uint64_t* offs = e->last_is_view ? (const uint64_t*)(V + e->last_o_start) : (const uint64_t*)(B + e->last_o_off);
  const uint64_t* ends = e->last_is_view ? (const uint64_t*)(V + e->last_o_end) : nullptr;
  r = pem_device_locked(e, (const uint8_t*)e->d_scratch[SC_STAGE_A], offs,
                        (const uint64_t*)(B + e->last_o_new), nn, nullptr, 0, d_po, &total, ends);
  if (r) return r;
  if (need) *need = total;
  if (!out || cap < total) return out ? fail(e, CTMR_E_RANGE, "PEM buffer too small: need %llu bytes", (unsigned long long)total) : CTMR_E_RANGE;
  if ((r = ensure(e, SC_PEM, total + 64))) return r;
  r = pem_device_locked(e, (const uint8_t*)e->d_scratch[SC_STAGE_A], offs,
                        (const uint64_t*)(B + e->last_o_new), nn, (uint8_t*)e->d_scratch[SC_PEM], total + 64, d_po, &total, ends);
  if (r) return r;
  HIPCHK(e, hipMemcpy(out, e->d_scratch[SC_PEM], total, hipMemcpyDeviceToHost));
  if (pem_offsets) HIPCHK(e, hipMemcpy(pem_offsets, d_po, (nn + 1) * 8, hipMemcpyDeviceToHost));
  return CTMR_OK;
}
