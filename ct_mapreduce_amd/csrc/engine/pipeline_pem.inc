// engine/pipeline_pem.inc — the worker's step for a super-batch of PEM files (ctmr_submit_pem, DESIGN.md §23): every file
// judged alone, the good ones decoded into the slot's blob, their files' issuer indices expanded to one per certificate,
// then the packed map/reduce path.
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after engine/pem_decode.inc.

extern "C++" {
namespace {

// The engine's mutex is held and the slot's text has arrived (pipe_worker).  Everything sized by certificates is sized
// here, once ffirst is known: the payload (at most 3/4 of the text), offsets, issuer indices, records, NEW list.
// pipe_slot_reserve frees the meta buffers when it grows them; the files' bounds and issuers are in s.body_rb and
// s.file_iss, not there.  No DER, no offsets and no expanded index array cross the host on the way to the map: what goes
// back is what the tickets' info is made of.
int pipe_run_pem(ctmr_engine* e, PipeSlot& s) {
  const uint64_t F = s.body_rb.size() - 1;
  int r;
  PemDecode P;
  if ((r = pem_decode_core(e, s.d_payload, s.body_rb.data(), F, &P, true))) return r;
  const uint64_t n = P.info.certificates, pb = P.info.payload_bytes;
  try {
    s.body_bad.assign(F, ~0ull);
    s.body_first.assign(F + 1, 0);
    s.cert_lay.assign(n, 0);
  } catch (const std::bad_alloc&) {
    return fail(e, CTMR_E_NOMEM, "no host memory for the verdicts of %llu files", (unsigned long long)F);
  }
  if ((r = pipe_slot_reserve(e, s, n, 0)) || (r = pipe_blob_reserve(e, s, pb))) return r;
  if ((r = pem_decode_decode(e, P, s.d_blob))) return r;
  if ((r = pem_decode_file_bad(e, P, F, s.body_bad.data())) || (r = pem_decode_file_first(e, P, F, s.body_first.data()))) return r;
  HIPCHK(e, hipMemcpy(s.h_meta, P.offsets.p, (n + 1) * 8, hipMemcpyDeviceToHost));  // the tickets' payload bytes
  s.n = n;
  s.bytes = pb;
  if (!n) return CTMR_OK;
  HIPCHK(e, hipMemcpy(s.cert_lay.data(), P.lay.p, n * 8, hipMemcpyDeviceToHost));
  DevMem d_fiss;
  if (d_fiss.alloc(F * 4) != hipSuccess) return fail(e, CTMR_E_NOMEM, "no device memory for the issuers of %llu files", (unsigned long long)F);
  uint32_t* d_iss = (uint32_t*)(s.d_meta + (s.ent_cap + 1) * 8);
  HIPCHK(e, hipMemcpyAsync(d_fiss.p, s.file_iss.data(), F * 4, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(s.d_meta, P.offsets.p, (n + 1) * 8, hipMemcpyDeviceToDevice, e->stream));
  tx_turns(tx_blocks(n, RP_BLOCK), [&](uint64_t b0, dim3 g) {
    hipLaunchKernelGGL(k_pd_issuer, g, dim3(RP_BLOCK), 0, e->stream, b0, F, n, (const unsigned long long*)P.ffirst.p, (const uint32_t*)d_fiss.p, d_iss);
  });
  // (P's tables and d_fiss end with this call: the map drains the stream before it returns)
  return map_device_locked(e, s.d_blob, (const uint64_t*)s.d_meta, d_iss, nullptr, n, s.d_records, s.d_new, &s.stats, nullptr, 0, pb);
}

}  // namespace
}  // extern "C++"
