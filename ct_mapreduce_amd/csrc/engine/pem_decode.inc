// engine/pem_decode.inc — files of concatenated CERTIFICATE blocks as they lie → the payload and offsets of a packed batch
// (include/ctmr.h ctmr_pem_decode*, DESIGN.md §21).  The text stays where it lies; the kernels of kernels/pem_decode.h
// find its armor lines, check the grammar and decode the base64.  The host sees counts only: tokens, certificates,
// decoded bytes, tiles.
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after engine/text_decode.inc,
// which has the host steps this decoder shares with engine/entries_json.inc.

extern "C++" {
namespace {

struct PemDecode {
  DevMem rb, tok, ctok, cnt_c, ffirst;         // what the squeeze and the results need
  DevMem offsets, src, lay, sqoff, sqtiles;    // per certificate
  TxText text{};
  uint64_t n = 0, sq_bytes = 0;
  ctmr_pem_decode_info info{};
  DevMem bad;            // each: the verdict of every file, UINT64_MAX or an offset inside it — fetched only when any_bad
  bool any_bad = false;  // each: some file is outside the grammar (info names the lowest)
};

const char* const PEM_DECODE = "pem decode";

void pd_info_none(ctmr_pem_decode_info* info, uint64_t F) {
  memset(info, 0, sizeof *info);
  info->files = F;
  info->bad_file = info->bad_offset = ~0ull;
}

int pd_alloc(ctmr_engine* e, DevMem* m, uint64_t words) { return tx_alloc(e, PEM_DECODE, m, words); }

// Everything but the payload: the text (device memory, any alignment; file f at s[fb[f], fb[f + 1])) validated, P->info
// made, the tables of the decode left on the device.  Drains the stream.
// each: a file outside the grammar fails nothing: P->bad[f] (device) gets its offset, P->info names the lowest, and ffirst
// and the tables of the decode are those of the files inside the grammar alone, the others holding no certificates.
int pem_decode_core(ctmr_engine* e, const uint8_t* s, const uint64_t* fb, uint64_t F, PemDecode* P, bool each = false) {
  int r;
  ctmr_pem_decode_info& info = P->info;
  pd_info_none(&info, F);
  TxText& T = P->text;
  uint64_t nb = 0;
  if ((r = tx_open(e, PEM_DECODE, "file_bounds", s, fb, F, &P->rb, &T, &nb)) || (r = pd_alloc(e, &P->offsets, 1)) ||
      (r = pd_alloc(e, &P->ffirst, F + 1)))
    return r;
  HIPCHK(e, hipMemsetAsync(P->offsets.p, 0, 8, e->stream));
  HIPCHK(e, hipMemsetAsync(P->ffirst.p, 0, (F + 1) * 8, e->stream));
  info.text_bytes = T.hi - T.lo;
  if (!nb) {  // no files, or empty ones only
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return CTMR_OK;
  }
  // each: the table of verdicts, F words and the lowest file with one behind them (pd_verdict); gate: its copy for the check
  DevMem cnt_t_m, cnt_e_m, sum_m, err_m, gate_m, cfile_m, tfirst_m, etok_m;
  if ((r = pd_alloc(e, &cnt_t_m, nb + 1)) || (r = pd_alloc(e, &P->cnt_c, nb + 1)) || (r = pd_alloc(e, &cnt_e_m, nb + 1)) ||
      (r = pd_alloc(e, &sum_m, (nb + 7) / 8)) || (r = pd_alloc(e, &err_m, 3)) || (r = pd_alloc(e, &cfile_m, F + 1)) ||
      (r = pd_alloc(e, &tfirst_m, F + 1)) || (each && ((r = pd_alloc(e, &P->bad, F + 1)) || (r = pd_alloc(e, &gate_m, F)))))
    return r;
  unsigned long long* err = (unsigned long long*)(each ? P->bad.p : err_m.p);
  unsigned long long* irr = (unsigned long long*)err_m.p + 2;
  unsigned long long* cnt_t = (unsigned long long*)cnt_t_m.p;
  unsigned long long* cnt_c = (unsigned long long*)P->cnt_c.p;
  unsigned long long* cnt_e = (unsigned long long*)cnt_e_m.p;
  HIPCHK(e, hipMemsetAsync(err, 0xff, each ? (F + 1) * 8 : 16, e->stream));
  HIPCHK(e, hipMemsetAsync(irr, 0, 8, e->stream));  // the irregular blocks
  const auto k_count = each ? k_pd_mark<false, true> : k_pd_mark<false, false>;  // (each: the kernels that fill the table of verdicts)
  const auto k_write = each ? k_pd_mark<true, true> : k_pd_mark<true, false>;
  const auto k_files = each ? k_pd_files<true> : k_pd_files<false>;
  const auto k_check = each ? k_pd_check<true> : k_pd_check<false>;
  // ---- armor lines
  tx_turns(nb, [&](uint64_t b0, dim3 g) {
    hipLaunchKernelGGL(k_count, g, dim3(TX_BLOCK), 0, e->stream, T, b0, cnt_t, cnt_c, cnt_e, sum_m.u8(), (unsigned long long*)nullptr,
                       (unsigned long long*)nullptr, (unsigned long long*)nullptr, err);
  });
  uint64_t ntok = 0;
  if ((r = tx_scan(e, P->cnt_c, nb, nullptr)) || (r = tx_scan(e, cnt_e_m, nb, nullptr)) || (r = tx_scan(e, cnt_t_m, nb, &ntok))) return r;
  if ((r = pd_alloc(e, &P->tok, ntok)) || (r = pd_alloc(e, &P->ctok, ntok)) || (r = pd_alloc(e, &etok_m, ntok))) return r;
  tx_turns(nb, [&](uint64_t b0, dim3 g) {
    hipLaunchKernelGGL(k_write, g, dim3(TX_BLOCK), 0, e->stream, T, b0, cnt_t, cnt_c, cnt_e, sum_m.u8(), (unsigned long long*)P->tok.p,
                       (unsigned long long*)P->ctok.p, (unsigned long long*)etok_m.p, err);
  });
  // ---- files, certificates
  tx_turns(tx_blocks(F + 1, RP_BLOCK / 64), [&](uint64_t b0, dim3 g) {
    hipLaunchKernelGGL(k_pd_fstart, g, dim3(RP_BLOCK), 0, e->stream, T, b0, (const unsigned long long*)cnt_c, nb, (unsigned long long*)cfile_m.p);
  });
  tx_turns(tx_blocks(F + 1, RP_BLOCK), [&](uint64_t b0, dim3 g) {
    hipLaunchKernelGGL(k_files, g, dim3(RP_BLOCK), 0, e->stream, T, b0, (const unsigned long long*)P->tok.p, ntok, (unsigned long long*)tfirst_m.p,
                       (unsigned long long*)P->ffirst.p, err);
  });
  uint64_t n = 0;
  if ((r = scan_u64(e, (uint64_t*)P->ffirst.p, F + 1, false, SC_MISC))) return r;
  unsigned long long h_err[3] = {0, 0, 0};
  HIPCHK(e, hipMemcpyAsync(&n, (uint64_t*)P->ffirst.p + F, 8, hipMemcpyDeviceToHost, e->stream));
  if (each) HIPCHK(e, hipMemcpyAsync(gate_m.p, err, F * 8, hipMemcpyDeviceToDevice, e->stream));
  else HIPCHK(e, hipMemcpyAsync(h_err, err, 24, hipMemcpyDeviceToHost, e->stream));
  if ((r = tx_drain(e))) return r;
  const uint64_t f_limit = h_err[0];  // the files from this one on are outside the grammar or need no verdict: the check skips them
  if ((r = pd_alloc(e, &P->offsets, n + 1)) || (r = pd_alloc(e, &P->src, n)) || (r = pd_alloc(e, &P->lay, n)) || (r = pd_alloc(e, &P->sqoff, n + 1)) ||
      (r = pd_alloc(e, &P->sqtiles, n + 1)))
    return r;
  if (ntok) {
    const PdCheck C{(const unsigned long long*)P->tok.p,    (const unsigned long long*)P->ctok.p,    (const unsigned long long*)etok_m.p, ntok,
                    (const unsigned long long*)tfirst_m.p,  (const unsigned long long*)P->ffirst.p,  (const unsigned long long*)cfile_m.p,
                    (unsigned long long*)P->offsets.p,      (unsigned long long*)P->src.p,           (unsigned long long*)P->lay.p,
                    (unsigned long long*)P->sqoff.p,        (unsigned long long*)P->sqtiles.p};
    tx_turns(tx_blocks(ntok, RP_BLOCK), [&](uint64_t b0, dim3 g) { hipLaunchKernelGGL(k_check, g, dim3(RP_BLOCK), 0, e->stream, T, b0, C, f_limit, (const unsigned long long*)gate_m.p, irr, err);
    });
  }
  if (each) {
    h_err[0] = h_err[1] = ~0ull;
    unsigned long long low = ~0ull;
    HIPCHK(e, hipMemcpyAsync(&low, err + F, 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(h_err + 2, irr, 8, hipMemcpyDeviceToHost, e->stream));
    if ((r = tx_drain(e))) return r;
    if (low != ~0ull) {
      // the files with a verdict leave: their counts to zero, ffirst scanned again, and the five tables the check wrote
      // under the old numbering gathered under the new one (certificate-sized; a second check would be token-sized and
      // read the layouts from the text again).  The irregular blocks are counted again over what stays.
      P->any_bad = true;
      info.bad_file = low;
      const uint64_t n0 = n;
      DevMem ffirst2, len2, src2, lay2, sqlen2, sqtiles2;
      if ((r = pd_alloc(e, &ffirst2, F + 1))) return r;
      HIPCHK(e, hipMemcpyAsync(&info.bad_offset, err + low, 8, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(e, hipMemsetAsync(irr, 0, 8, e->stream));
      if ((r = tx_drop(e, F, err, P->ffirst, ffirst2, &n))) return r;
      if ((r = pd_alloc(e, &len2, n + 1)) || (r = pd_alloc(e, &src2, n)) || (r = pd_alloc(e, &lay2, n)) || (r = pd_alloc(e, &sqlen2, n + 1)) ||
          (r = pd_alloc(e, &sqtiles2, n + 1)))
        return r;
      if (n) {
        const PdGather G{(const unsigned long long*)err,          (const unsigned long long*)P->ffirst.p,  (const unsigned long long*)ffirst2.p,
                         (const unsigned long long*)P->offsets.p, (const unsigned long long*)P->src.p,     (const unsigned long long*)P->lay.p,
                         (const unsigned long long*)P->sqoff.p,   (const unsigned long long*)P->sqtiles.p, (unsigned long long*)len2.p,
                         (unsigned long long*)src2.p,             (unsigned long long*)lay2.p,             (unsigned long long*)sqlen2.p,
                         (unsigned long long*)sqtiles2.p};
        tx_turns(tx_blocks(n0, RP_BLOCK), [&](uint64_t b0, dim3 g) { hipLaunchKernelGGL(k_pd_gather, g, dim3(RP_BLOCK), 0, e->stream, b0, F, n0, G, irr); });
      }
      HIPCHK(e, hipMemcpyAsync(h_err + 2, irr, 8, hipMemcpyDeviceToHost, e->stream));
      if ((r = tx_drain(e))) return r;  // (the old tables are freed when this block ends)
      std::swap(P->ffirst.p, ffirst2.p);
      std::swap(P->offsets.p, len2.p);
      std::swap(P->src.p, src2.p);
      std::swap(P->lay.p, lay2.p);
      std::swap(P->sqoff.p, sqlen2.p);
      std::swap(P->sqtiles.p, sqtiles2.p);
    }
  } else {
    HIPCHK(e, hipMemcpyAsync(h_err, err, 24, hipMemcpyDeviceToHost, e->stream));
    if ((r = tx_drain(e))) return r;
  }
  if (h_err[0] != ~0ull) {
    info.bad_file = h_err[0];
    info.bad_offset = h_err[1];
    return fail(e, CTMR_E_INVAL, "%s: file %llu is outside the grammar near offset %llu", PEM_DECODE, h_err[0], h_err[1]);
  }
  // ---- offsets, and where the characters of the irregular blocks go
  uint64_t payload_bytes = 0;
  if ((r = tx_scan(e, P->offsets, n, &payload_bytes)) || (r = tx_scan(e, P->sqoff, n, &P->sq_bytes))) return r;
  P->n = n;
  info.certificates = n;
  info.payload_bytes = payload_bytes;
  info.irregular = h_err[2];
  info.regular = n - h_err[2];
  return CTMR_OK;
}

// The squeeze and the decode: info.payload_bytes bytes and the zero padding behind them to d_payload (16-byte aligned).
// Every table and the squeezed copy are allocated before the first byte is written.  Drains the stream.
int pem_decode_decode(ctmr_engine* e, PemDecode& P, uint8_t* d_payload) {
  DevMem tile_first, tile_cert, sq_cert, sq;
  uint64_t ntiles = 0, nsq = 0;
  int r;
  const uint64_t n = P.n;
  if (n) {
    if ((r = tx_tile_list(e, PEM_DECODE, &P.offsets, n, &tile_first, &tile_cert, &ntiles))) return r;
    if (P.sq_bytes) {
      if (sq.alloc(P.sq_bytes + 16) != hipSuccess)
        return fail(e, CTMR_E_NOMEM, "%s: no device memory for %llu squeezed characters", PEM_DECODE, (unsigned long long)P.sq_bytes);
      if ((r = tx_tile_list(e, PEM_DECODE, nullptr, n, &P.sqtiles, &sq_cert, &nsq))) return r;
      tx_turns(nsq, [&](uint64_t b0, dim3 g) {
        hipLaunchKernelGGL(k_pd_squeeze, g, dim3(TX_BLOCK), 0, e->stream, P.text, b0, (const unsigned long long*)sq_cert.p,
                           (const unsigned long long*)P.sqtiles.p, (const unsigned long long*)P.src.p, (const unsigned long long*)P.tok.p,
                           (const unsigned long long*)P.ctok.p, (const unsigned long long*)P.cnt_c.p, (const unsigned long long*)P.sqoff.p, sq.u8());
      });
    }
    if (ntiles) {
      const PdDecode D{(const unsigned long long*)tile_cert.p, (const unsigned long long*)tile_first.p, (const unsigned long long*)P.offsets.p,
                       (const unsigned long long*)P.src.p,     (const unsigned long long*)P.lay.p,      (const unsigned long long*)P.sqoff.p,
                       sq.u8()};
      tx_turns(ntiles, [&](uint64_t b0, dim3 g) { hipLaunchKernelGGL(k_pd_decode, g, dim3(TX_DBLOCK), 0, e->stream, P.text.s, b0, D, d_payload); });
    }
  }
  return tx_finish(e, d_payload, P.info.payload_bytes);
}

int pem_decode_file_first(ctmr_engine* e, const PemDecode& P, uint64_t F, uint64_t* file_first) {
  if (file_first) HIPCHK(e, hipMemcpy(file_first, P.ffirst.p, (F + 1) * 8, hipMemcpyDeviceToHost));
  return CTMR_OK;
}

// each: the verdicts of the F files to host memory.  Only a call with a bad file fetches the table.
int pem_decode_file_bad(ctmr_engine* e, const PemDecode& P, uint64_t F, uint64_t* file_bad) {
  if (!F) return CTMR_OK;
  if (P.any_bad) HIPCHK(e, hipMemcpy(file_bad, P.bad.p, F * 8, hipMemcpyDeviceToHost));
  else memset(file_bad, 0xff, F * 8);
  return CTMR_OK;
}

// ctmr_pem_decode (host: text, payload and offsets are host memory, staged here) and ctmr_pem_decode_device; each, with
// file_bad: the …_each* forms
int pem_decode_call(ctmr_engine* e, bool host, const void* text, const uint64_t* file_bounds, uint64_t n_files, void* payload, size_t payload_cap,
                    uint64_t* offsets, uint64_t certs_cap, uint64_t* file_first, uint64_t* file_bad, bool each, ctmr_pem_decode_info* info) {
  if (!e || !info) return CTMR_E_INVAL;
  pd_info_none(info, n_files);  // (a bad argument names no file)
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (n_files && !file_bounds) return fail(e, CTMR_E_INVAL, "%s: null file_bounds", PEM_DECODE);
  if (each && !file_bad) return fail(e, CTMR_E_INVAL, "%s: null file_bad", PEM_DECODE);
  DevMem d_text, d_payload;
  const uint8_t* s;
  int r;
  if ((r = tx_stage(e, PEM_DECODE, (const uint8_t*)text, file_bounds, n_files, host ? &d_text : nullptr, &s))) return r;
  if (!host && ((uintptr_t)payload & 15u)) return fail(e, CTMR_E_INVAL, "%s: the payload is not 16-byte aligned", PEM_DECODE);
  PemDecode P;
  r = pem_decode_core(e, s, file_bounds, n_files, &P, each);
  *info = P.info;
  if (r) return r;
  if ((r = tx_fits(e, PEM_DECODE, P.n, "certificates", P.info.payload_bytes, "payload", payload, payload_cap, offsets, certs_cap))) return r;
  if (host && d_payload.alloc(P.info.payload_bytes + CTMR_PAYLOAD_PAD) != hipSuccess)
    return fail(e, CTMR_E_NOMEM, "%s: no device memory for %llu decoded bytes", PEM_DECODE, (unsigned long long)P.info.payload_bytes);
  if ((r = pem_decode_decode(e, P, host ? d_payload.u8() : (uint8_t*)payload))) return r;
  if (host) HIPCHK(e, hipMemcpy(payload, d_payload.p, P.info.payload_bytes + CTMR_PAYLOAD_PAD, hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(offsets, P.offsets.p, (P.n + 1) * 8, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
  if (each && (r = pem_decode_file_bad(e, P, n_files, file_bad))) return r;
  return pem_decode_file_first(e, P, n_files, file_first);
}

}  // namespace
}  // extern "C++"

int ctmr_pem_decode_device(ctmr_engine* e, const void* d_text, const uint64_t* file_bounds, uint64_t n_files, void* d_payload, size_t payload_cap,
                           uint64_t* d_offsets, uint64_t certs_cap, uint64_t* file_first, ctmr_pem_decode_info* info) {
  return pem_decode_call(e, false, d_text, file_bounds, n_files, d_payload, payload_cap, d_offsets, certs_cap, file_first, nullptr, false, info);
}

int ctmr_pem_decode(ctmr_engine* e, const uint8_t* text, const uint64_t* file_bounds, uint64_t n_files, uint8_t* payload, size_t payload_cap,
                    uint64_t* offsets, uint64_t certs_cap, uint64_t* file_first, ctmr_pem_decode_info* info) {
  return pem_decode_call(e, true, text, file_bounds, n_files, payload, payload_cap, offsets, certs_cap, file_first, nullptr, false, info);
}

int ctmr_pem_decode_each_device(ctmr_engine* e, const void* d_text, const uint64_t* file_bounds, uint64_t n_files, void* d_payload, size_t payload_cap,
                                uint64_t* d_offsets, uint64_t certs_cap, uint64_t* file_first, uint64_t* file_bad, ctmr_pem_decode_info* info) {
  return pem_decode_call(e, false, d_text, file_bounds, n_files, d_payload, payload_cap, d_offsets, certs_cap, file_first, file_bad, true, info);
}

int ctmr_pem_decode_each(ctmr_engine* e, const uint8_t* text, const uint64_t* file_bounds, uint64_t n_files, uint8_t* payload, size_t payload_cap,
                         uint64_t* offsets, uint64_t certs_cap, uint64_t* file_first, uint64_t* file_bad, ctmr_pem_decode_info* info) {
  return pem_decode_call(e, true, text, file_bounds, n_files, payload, payload_cap, offsets, certs_cap, file_first, file_bad, true, info);
}
