// engine/pipeline_json.inc — the worker's step for a super-batch of get-entries bodies (ctmr_submit_entries_json,
// DESIGN.md §22): every body judged alone, the good ones decoded into the slot's blob, then the raw-entry path.
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after engine/entries_json.inc.

extern "C++" {
namespace {

// Everything sized by entries is sized once efirst is known (pipe_text_reserve): the blob, records, NEW list, timestamps,
// entry types, Chain[0] lengths.
int pipe_run_json(ctmr_engine* e, PipeSlot& s, ctmr_entry_view* view) {
  const uint64_t R = s.body_rb.size() - 1;
  int r;
  EntriesJson J;
  if ((r = entries_json_core(e, s.d_payload.u8(), s.body_rb.data(), R, &J, true))) return r;
  const uint64_t n = J.info.entries;
  if ((r = pipe_text_reserve(e, s, n, J.info.blob_bytes))) return r;
  s.body_bad.swap(J.bad);  // (R verdicts either)
  if ((r = entries_json_decode(e, J, s.d_blob.u8()))) return r;
  if ((r = entries_json_resp_first(e, J, R, s.body_first.data()))) return r;
  HIPCHK(e, hipMemcpy(s.h_meta.p, J.bounds.p, (2 * n + 1) * 8, hipMemcpyDeviceToHost));  // the tickets' blob bytes
  HIPCHK(e, hipMemcpyAsync(s.d_meta.p, J.bounds.p, (2 * n + 1) * 8, hipMemcpyDeviceToDevice, e->stream));  // (J's tables end with this call)
  s.n = n;
  return pipe_map_raw(e, s, s.d_blob.u8(), view);
}

}  // namespace
}  // extern "C++"
