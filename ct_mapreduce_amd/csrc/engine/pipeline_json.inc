// engine/pipeline_json.inc — the worker's step for a super-batch of get-entries bodies (ctmr_submit_entries_json,
// DESIGN.md §22): every body judged alone, the good ones decoded into the slot's blob, then the raw-entry path.
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after engine/entries_json.inc.

extern "C++" {
namespace {

// The engine's mutex is held and the slot's text has arrived (pipe_worker).  Everything sized by entries is sized here,
// once efirst is known: the blob (at most 3/4 of the text), records, NEW list, timestamps, entry types, Chain[0] lengths.
// pipe_slot_reserve frees the meta buffers when it grows them; the bodies' bounds are in s.body_rb, not there.
int pipe_run_json(ctmr_engine* e, PipeSlot& s, ctmr_entry_view* view) {
  const uint64_t R = s.body_rb.size() - 1;
  int r;
  EntriesJson J;
  if ((r = entries_json_core(e, s.d_payload, s.body_rb.data(), R, &J, true))) return r;
  const uint64_t n = J.info.entries, bb = J.info.blob_bytes;
  try {
    s.body_bad = J.bad;
    s.body_first.assign(R + 1, 0);
  } catch (const std::bad_alloc&) {
    return fail(e, CTMR_E_NOMEM, "no host memory for the verdicts of %llu bodies", (unsigned long long)R);
  }
  if ((r = pipe_slot_reserve(e, s, n, 0))) return r;
  if ((r = pipe_blob_reserve(e, s, bb))) return r;
  if ((r = entries_json_decode(e, J, s.d_blob))) return r;
  if ((r = entries_json_resp_first(e, J, R, s.body_first.data()))) return r;
  HIPCHK(e, hipMemcpy(s.h_meta, J.bounds.p, (2 * n + 1) * 8, hipMemcpyDeviceToHost));  // the tickets' blob bytes
  HIPCHK(e, hipMemcpyAsync(s.d_meta, J.bounds.p, (2 * n + 1) * 8, hipMemcpyDeviceToDevice, e->stream));  // (J's tables end with this call)
  s.n = n;
  return map_entries_locked(e, s.d_blob, (const uint64_t*)s.d_meta, n, s.d_records, s.d_new, s.d_ts, &s.dstats, &s.stats, view);
}

}  // namespace
}  // extern "C++"
