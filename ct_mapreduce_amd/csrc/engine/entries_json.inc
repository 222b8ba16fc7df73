// engine/entries_json.inc — get-entries HTTP bodies as they lie → a raw-entry batch (include/ctmr.h ctmr_entries_json*,
// DESIGN.md §20; ctmr_entries_json_each*, every body judged alone, §22).  The text stays where it lies; the kernels of
// kernels/entries_json.h find its tokens, check the grammar and decode the base64.  The host sees counts only: tokens,
// entries, decoded bytes, tiles.
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after engine/text_decode.inc,
// which has the host steps this decoder shares with engine/pem_decode.inc.

extern "C++" {
namespace {

struct EntriesJson {
  DevMem rb, bounds, src, efirst;  // what the decode and the results need
  TxText text{};
  uint64_t n = 0;
  ctmr_entries_json_info info{};
  std::vector<uint64_t> bad;  // each: the verdict of every response, UINT64_MAX or an offset inside it
  bool no_text = false;       // each: no body holds a byte, nothing was launched: efirst is not there, all of it is zero
};

const char* const ENTRIES_JSON = "entries json";

void ej_info_none(ctmr_entries_json_info* info, uint64_t R) {
  memset(info, 0, sizeof *info);
  info->responses = R;
  info->bad_response = info->bad_offset = ~0ull;
}

int ej_alloc(ctmr_engine* e, DevMem* m, uint64_t words) { return tx_alloc(e, ENTRIES_JSON, m, words); }

// Everything but the blob: the text (device memory, any alignment; response r at s[rb[r], rb[r + 1])) validated, J->info
// made, the tables of the decode left on the device.  Drains the stream.
// each: a response outside the grammar fails nothing: J->bad[r] gets its offset, J->info names the lowest, and efirst,
// bounds, src are those of the responses inside the grammar alone, the others holding no entries.
int entries_json_core(ctmr_engine* e, const uint8_t* s, const uint64_t* rb, uint64_t R, EntriesJson* J, bool each = false) {
  int r;
  ctmr_entries_json_info& info = J->info;
  ej_info_none(&info, R);
  if (each) {
    try {
      J->bad.assign(R, ~0ull);
    } catch (const std::bad_alloc&) {
      return fail(e, CTMR_E_NOMEM, "%s: no host memory for %llu verdicts", ENTRIES_JSON, (unsigned long long)R);
    }
  }
  TxText& T = J->text;
  uint64_t nb = 0;
  if ((r = tx_open(e, ENTRIES_JSON, "resp_bounds", s, rb, R, &J->rb, &T, &nb)) || (r = ej_alloc(e, &J->bounds, 1))) return r;
  HIPCHK(e, hipMemsetAsync(J->bounds.p, 0, 8, e->stream));
  info.text_bytes = T.hi - T.lo;
  if (!R) {
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return CTMR_OK;
  }
  if (!nb && each) {  // empty bodies only: each has its verdict, and no kernel runs over an empty range
    std::copy(rb, rb + R, J->bad.begin());
    J->no_text = true;
    info.bad_response = 0;
    info.bad_offset = T.lo;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return CTMR_OK;
  }
  if (!nb) {
    info.bad_response = 0;
    info.bad_offset = T.lo;
    return fail(e, CTMR_E_INVAL, "%s: response 0 is empty", ENTRIES_JSON);
  }
  DevMem qblk_m, cnt_t_m, cnt_o_m, err_m, qstart_m, tfirst_m, tok_m, oddb_m;
  if ((r = ej_alloc(e, &qblk_m, nb + 1)) || (r = ej_alloc(e, &cnt_t_m, nb + 1)) || (r = ej_alloc(e, &cnt_o_m, nb + 1)) ||
      (r = ej_alloc(e, &err_m, each ? R : 2)) || (r = ej_alloc(e, &qstart_m, R)) || (r = ej_alloc(e, &tfirst_m, R + 1)) || (r = ej_alloc(e, &J->efirst, R + 1)))
    return r;
  unsigned long long* err = (unsigned long long*)err_m.p;
  unsigned long long* qblk = (unsigned long long*)qblk_m.p;
  unsigned long long* cnt_t = (unsigned long long*)cnt_t_m.p;
  unsigned long long* cnt_o = (unsigned long long*)cnt_o_m.p;
  HIPCHK(e, hipMemsetAsync(err, 0xff, (each ? R : 2) * 8, e->stream));
  // ---- string state
  tx_turns(nb, [&](uint64_t b0, dim3 g) { hipLaunchKernelGGL(k_ej_quotes, g, dim3(TX_BLOCK), 0, e->stream, T, b0, qblk); });
  if ((r = tx_scan(e, qblk_m, nb, nullptr))) return r;
  tx_turns(tx_blocks(R, RP_BLOCK / 64), [&](uint64_t b0, dim3 g) {
    hipLaunchKernelGGL(k_ej_qstart, g, dim3(RP_BLOCK), 0, e->stream, T, b0, (const unsigned long long*)qblk, (unsigned long long*)qstart_m.p);
  });
  // ---- tokens
  const auto k_count = each ? k_ej_mark<false, true> : k_ej_mark<false, false>;  // (each: the kernels that fill the table of verdicts)
  const auto k_resp = each ? k_ej_resp<true> : k_ej_resp<false>;
  const auto k_check = each ? k_ej_check<true> : k_ej_check<false>;
  tx_turns(nb, [&](uint64_t b0, dim3 g) {
    hipLaunchKernelGGL(k_count, g, dim3(TX_BLOCK), 0, e->stream, T, b0, (const unsigned long long*)qblk, (const unsigned long long*)qstart_m.p,
                       cnt_t, cnt_o, (unsigned long long*)nullptr, (unsigned long long*)nullptr, err);
  });
  uint64_t ntok = 0;
  if ((r = tx_scan(e, cnt_o_m, nb, nullptr)) || (r = tx_scan(e, cnt_t_m, nb, &ntok))) return r;
  if ((r = ej_alloc(e, &tok_m, ntok)) || (r = ej_alloc(e, &oddb_m, ntok))) return r;
  tx_turns(nb, [&](uint64_t b0, dim3 g) {
    hipLaunchKernelGGL((k_ej_mark<true>), g, dim3(TX_BLOCK), 0, e->stream, T, b0, (const unsigned long long*)qblk,
                       (const unsigned long long*)qstart_m.p, cnt_t, cnt_o, (unsigned long long*)tok_m.p, (unsigned long long*)oddb_m.p, err);
  });
  // ---- responses, entries
  tx_turns(tx_blocks(R + 1, RP_BLOCK), [&](uint64_t b0, dim3 g) {
    hipLaunchKernelGGL(k_resp, g, dim3(RP_BLOCK), 0, e->stream, T, b0, (const unsigned long long*)tok_m.p, ntok, (unsigned long long*)tfirst_m.p,
                       (unsigned long long*)J->efirst.p, err);
  });
  uint64_t n = 0;
  if ((r = scan_u64(e, (uint64_t*)J->efirst.p, R + 1, false, SC_MISC))) return r;
  HIPCHK(e, hipMemcpyAsync(&n, (uint64_t*)J->efirst.p + R, 8, hipMemcpyDeviceToHost, e->stream));
  if ((r = tx_drain(e))) return r;
  if ((r = ej_alloc(e, &J->bounds, 2 * n + 1)) || (r = ej_alloc(e, &J->src, 2 * n))) return r;
  if (ntok) {
    const EjCheck C{(const unsigned long long*)tok_m.p,    (const unsigned long long*)oddb_m.p,     ntok, (const unsigned long long*)tfirst_m.p,
                    (const unsigned long long*)J->efirst.p, (unsigned long long*)J->bounds.p, (unsigned long long*)J->src.p};
    tx_turns(tx_blocks(ntok, RP_BLOCK), [&](uint64_t b0, dim3 g) { hipLaunchKernelGGL(k_check, g, dim3(RP_BLOCK), 0, e->stream, T, b0, C, err); });
  }
  unsigned long long h_err[2] = {~0ull, ~0ull};
  if (each) {
    HIPCHK(e, hipMemcpyAsync(J->bad.data(), err, R * 8, hipMemcpyDeviceToHost, e->stream));
  } else {
    HIPCHK(e, hipMemcpyAsync(h_err, err, 16, hipMemcpyDeviceToHost, e->stream));
  }
  if ((r = tx_drain(e))) return r;
  if (each) {
    uint64_t n_bad = 0;
    for (uint64_t i = R; i-- > 0;)
      if (J->bad[i] != ~0ull) {
        n_bad++;
        info.bad_response = i;
        info.bad_offset = J->bad[i];
      }
    if (n_bad) {
      // the responses with a verdict leave: their counts to zero, efirst scanned again, and the lengths and sources the
      // check wrote under the old numbering gathered under the new one (entry-sized; a second check would be token-sized
      // and read the keys and pads from the text again)
      const uint64_t n0 = n;
      DevMem efirst2, len2, src2;
      if ((r = ej_alloc(e, &efirst2, R + 1)) || (r = tx_drop(e, R, err, J->efirst, efirst2, &n))) return r;
      if ((r = ej_alloc(e, &len2, 2 * n + 1)) || (r = ej_alloc(e, &src2, 2 * n))) return r;
      if (n)
        tx_turns(tx_blocks(n0, RP_BLOCK), [&](uint64_t b0, dim3 g) {
          hipLaunchKernelGGL(k_ej_gather, g, dim3(RP_BLOCK), 0, e->stream, b0, R, n0, (const unsigned long long*)err,
                             (const unsigned long long*)J->efirst.p, (const unsigned long long*)efirst2.p, (const unsigned long long*)J->bounds.p,
                             (const unsigned long long*)J->src.p, (unsigned long long*)len2.p, (unsigned long long*)src2.p);
        });
      if ((r = tx_drain(e))) return r;  // (the old tables are freed when this block ends)
      std::swap(J->efirst.p, efirst2.p);
      std::swap(J->bounds.p, len2.p);
      std::swap(J->src.p, src2.p);
    }
  }
  if (h_err[0] != ~0ull) {
    info.bad_response = h_err[0];
    info.bad_offset = h_err[1];
    return fail(e, CTMR_E_INVAL, "%s: response %llu is outside the grammar near offset %llu", ENTRIES_JSON, h_err[0], h_err[1]);
  }
  // ---- bounds
  uint64_t blob_bytes = 0;
  if ((r = tx_scan(e, J->bounds, 2 * n, &blob_bytes))) return r;
  J->n = n;
  info.entries = n;
  info.blob_bytes = blob_bytes;
  return CTMR_OK;
}

// The decode: the tiles of the 2 n strings, then info.blob_bytes bytes and the zero padding behind them to d_blob (16-byte
// aligned).  Drains the stream.
int entries_json_decode(ctmr_engine* e, const EntriesJson& J, uint8_t* d_blob) {
  DevMem tile_first, tile_str;
  uint64_t ntiles = 0;
  int r;
  if (J.n && (r = tx_tile_list(e, ENTRIES_JSON, &J.bounds, 2 * J.n, &tile_first, &tile_str, &ntiles))) return r;
  tx_turns(ntiles, [&](uint64_t b0, dim3 g) {
    hipLaunchKernelGGL(k_ej_decode, g, dim3(TX_DBLOCK), 0, e->stream, J.text.s, b0, (const unsigned long long*)tile_str.p,
                       (const unsigned long long*)tile_first.p, (const unsigned long long*)J.bounds.p, (const unsigned long long*)J.src.p, d_blob);
  });
  return tx_finish(e, d_blob, J.info.blob_bytes);
}

int entries_json_resp_first(ctmr_engine* e, const EntriesJson& J, uint64_t R, uint64_t* resp_first) {
  if (!resp_first) return CTMR_OK;
  if (!R || J.no_text) memset(resp_first, 0, (R + 1) * 8);
  else HIPCHK(e, hipMemcpy(resp_first, J.efirst.p, (R + 1) * 8, hipMemcpyDeviceToHost));
  return CTMR_OK;
}

// ctmr_entries_json* (host: text, blob and bounds are host memory, staged here) and ctmr_entries_json*_device; each, with
// resp_bad: the …_each* forms
int entries_json_call(ctmr_engine* e, bool host, const void* text, const uint64_t* resp_bounds, uint64_t n_responses, void* blob, size_t blob_cap,
                      uint64_t* bounds, uint64_t entries_cap, uint64_t* resp_first, uint64_t* resp_bad, bool each, ctmr_entries_json_info* info) {
  if (!e || !info) return CTMR_E_INVAL;
  ej_info_none(info, n_responses);  // (a bad argument names no response)
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (!resp_bounds) return fail(e, CTMR_E_INVAL, "%s: null resp_bounds", ENTRIES_JSON);
  if (each && !resp_bad) return fail(e, CTMR_E_INVAL, "%s: null resp_bad", ENTRIES_JSON);
  DevMem d_text, d_blob;
  const uint8_t* s;
  int r;
  if ((r = tx_stage(e, ENTRIES_JSON, (const uint8_t*)text, resp_bounds, n_responses, host ? &d_text : nullptr, &s))) return r;
  if (!host && ((uintptr_t)blob & 15u)) return fail(e, CTMR_E_INVAL, "%s: the blob is not 16-byte aligned", ENTRIES_JSON);
  EntriesJson J;
  r = entries_json_core(e, s, resp_bounds, n_responses, &J, each);
  *info = J.info;
  if (r) return r;
  if ((r = tx_fits(e, ENTRIES_JSON, J.n, "entries", J.info.blob_bytes, "blob", blob, blob_cap, bounds, entries_cap))) return r;
  if (host && d_blob.alloc(J.info.blob_bytes + CTMR_PAYLOAD_PAD) != hipSuccess)
    return fail(e, CTMR_E_NOMEM, "%s: no device memory for %llu decoded bytes", ENTRIES_JSON, (unsigned long long)J.info.blob_bytes);
  if ((r = entries_json_decode(e, J, host ? d_blob.u8() : (uint8_t*)blob))) return r;
  if (host) HIPCHK(e, hipMemcpy(blob, d_blob.p, J.info.blob_bytes + CTMR_PAYLOAD_PAD, hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(bounds, J.bounds.p, (2 * J.n + 1) * 8, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
  if (each && n_responses) memcpy(resp_bad, J.bad.data(), n_responses * 8);
  return entries_json_resp_first(e, J, n_responses, resp_first);
}

}  // namespace
}  // extern "C++"

int ctmr_entries_json_device(ctmr_engine* e, const void* d_text, const uint64_t* resp_bounds, uint64_t n_responses, void* d_blob,
                             size_t blob_cap, uint64_t* d_bounds, uint64_t entries_cap, uint64_t* resp_first, ctmr_entries_json_info* info) {
  return entries_json_call(e, false, d_text, resp_bounds, n_responses, d_blob, blob_cap, d_bounds, entries_cap, resp_first, nullptr, false, info);
}

int ctmr_entries_json(ctmr_engine* e, const uint8_t* text, const uint64_t* resp_bounds, uint64_t n_responses, uint8_t* blob, size_t blob_cap,
                      uint64_t* bounds, uint64_t entries_cap, uint64_t* resp_first, ctmr_entries_json_info* info) {
  return entries_json_call(e, true, text, resp_bounds, n_responses, blob, blob_cap, bounds, entries_cap, resp_first, nullptr, false, info);
}

int ctmr_entries_json_each_device(ctmr_engine* e, const void* d_text, const uint64_t* resp_bounds, uint64_t n_responses, void* d_blob,
                                  size_t blob_cap, uint64_t* d_bounds, uint64_t entries_cap, uint64_t* resp_first, uint64_t* resp_bad,
                                  ctmr_entries_json_info* info) {
  return entries_json_call(e, false, d_text, resp_bounds, n_responses, d_blob, blob_cap, d_bounds, entries_cap, resp_first, resp_bad, true, info);
}

int ctmr_entries_json_each(ctmr_engine* e, const uint8_t* text, const uint64_t* resp_bounds, uint64_t n_responses, uint8_t* blob, size_t blob_cap,
                           uint64_t* bounds, uint64_t entries_cap, uint64_t* resp_first, uint64_t* resp_bad, ctmr_entries_json_info* info) {
  return entries_json_call(e, true, text, resp_bounds, n_responses, blob, blob_cap, bounds, entries_cap, resp_first, resp_bad, true, info);
}
