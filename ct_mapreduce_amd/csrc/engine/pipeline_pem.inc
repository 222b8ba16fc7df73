// engine/pipeline_pem.inc — the worker's step for a super-batch of PEM files (ctmr_submit_pem, DESIGN.md §23): every file
// judged alone, the good ones decoded into the slot's blob, their files' issuer indices expanded to one per certificate,
// then the packed map/reduce path.
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after engine/pem_decode.inc.

extern "C++" {
namespace {

// Everything sized by certificates is sized once ffirst is known (pipe_text_reserve): the payload, offsets, issuer
// indices, records, NEW list.  No DER, no offsets and no expanded index array cross the host on the way to the map: what
// goes back is what the tickets' info is made of.
int pipe_run_pem(ctmr_engine* e, PipeSlot& s, ctmr_entry_view*) {
  const uint64_t F = s.body_rb.size() - 1;
  int r;
  PemDecode P;
  if ((r = pem_decode_core(e, s.d_payload.u8(), s.body_rb.data(), F, &P, true))) return r;
  const uint64_t n = P.info.certificates, pb = P.info.payload_bytes;
  if ((r = pipe_text_reserve(e, s, n, pb))) return r;
  if ((r = pem_decode_decode(e, P, s.d_blob.u8()))) return r;
  if ((r = pem_decode_file_bad(e, P, F, s.body_bad.data())) || (r = pem_decode_file_first(e, P, F, s.body_first.data()))) return r;
  HIPCHK(e, hipMemcpy(s.h_meta.p, P.offsets.p, (n + 1) * 8, hipMemcpyDeviceToHost));  // the tickets' payload bytes
  s.n = n;
  s.bytes = pb;
  if (!n) return CTMR_OK;
  HIPCHK(e, hipMemcpy(s.cert_lay.data(), P.lay.p, n * 8, hipMemcpyDeviceToHost));
  DevMem d_fiss;
  if (d_fiss.alloc(F * 4) != hipSuccess) return fail(e, CTMR_E_NOMEM, "no device memory for the issuers of %llu files", (unsigned long long)F);
  HIPCHK(e, hipMemcpyAsync(d_fiss.p, s.file_iss.data(), F * 4, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(s.d_meta.p, P.offsets.p, (n + 1) * 8, hipMemcpyDeviceToDevice, e->stream));
  tx_turns(tx_blocks(n, RP_BLOCK), [&](uint64_t b0, dim3 g) {
    hipLaunchKernelGGL(k_pd_issuer, g, dim3(RP_BLOCK), 0, e->stream, b0, F, n, (const unsigned long long*)P.ffirst.p, (const uint32_t*)d_fiss.p,
                       slot_iss(s, s.d_meta.u8()));
  });
  // (P's tables and d_fiss end with this call: the map drains the stream before it returns)
  return pipe_map_packed(e, s, s.d_blob.u8(), nullptr, pb);
}

}  // namespace
}  // extern "C++"
