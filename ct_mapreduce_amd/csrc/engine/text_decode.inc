// engine/text_decode.inc — the host code the two text decoders share (engine/entries_json.inc, engine/pem_decode.inc;
// kernels/text_scan.h): launching a pass in turns, tables of words, scans that end in a total, dropping the judged-bad
// bodies, opening a text in segments for the kernels, staging a host text, listing the decode tiles of n items, the check
// of the caller's buffers and the end of a decode.  `who` is the caller's name in front of its error messages ("entries json", "pem decode").
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after engine/resp_parse.inc.

extern "C++" {
namespace {

// f(b0, blocks) for the nblocks blocks of a pass, TX_GRID at a time
template <class F>
void tx_turns(uint64_t nblocks, F f) {
  for (uint64_t b0 = 0; b0 < nblocks; b0 += TX_GRID) f(b0, dim3((unsigned)std::min<uint64_t>(TX_GRID, nblocks - b0)));
}
uint64_t tx_blocks(uint64_t n, uint64_t per) { return (n + per - 1) / per; }

int tx_alloc(ctmr_engine* e, const char* who, DevMem* m, uint64_t words) {
  if (m->alloc((size_t)(words ? words : 1) * 8) != hipSuccess)
    return fail(e, CTMR_E_NOMEM, "%s: no device memory for a table of %llu words", who, (unsigned long long)words);
  return CTMR_OK;
}

int tx_drain(ctmr_engine* e) {
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  return CTMR_OK;
}

// data[0, n) → its exclusive prefix sums, data[n] → the total, which also goes to *total when asked for.  Drains then.
int tx_scan(ctmr_engine* e, DevMem& data, uint64_t n, uint64_t* total) {
  HIPCHK(e, hipMemsetAsync((uint64_t*)data.p + n, 0, 8, e->stream));
  if (!total) return scan_u64(e, (uint64_t*)data.p, n + 1, false, SC_MISC);
  return scan_total(e, (uint64_t*)data.p, n + 1, false, SC_MISC, total);
}

// The bodies with a verdict leave (bad_at[i] != ~0, i < R): first2 (R + 1 words) gets the items of every body out of
// first0, the scan that counted them, those of the judged-bad ones as zero, and is scanned; *n = the items that stay.  Drains.
int tx_drop(ctmr_engine* e, uint64_t R, const unsigned long long* bad_at, const DevMem& first0, DevMem& first2, uint64_t* n) {
  tx_turns(tx_blocks(R + 1, RP_BLOCK), [&](uint64_t b0, dim3 g) {
    hipLaunchKernelGGL(k_ej_drop, g, dim3(RP_BLOCK), 0, e->stream, b0, R, bad_at, (const unsigned long long*)first0.p, (unsigned long long*)first2.p);
  });
  return scan_total(e, (uint64_t*)first2.p, R + 1, false, SC_MISC, n);
}

// Opens the text for the kernels: segment r at s[sb[r], sb[r + 1]) (s: device memory, any alignment; sb: S + 1 bounds on
// the host, `what` their name).  CTMR_E_INVAL unless they ascend.  T->lo and T->hi are set; when a byte lies between
// them the bounds go to the device (*d_sb), *T is complete and *nb = its mark blocks, else *nb = 0.
int tx_open(ctmr_engine* e, const char* who, const char* what, const uint8_t* s, const uint64_t* sb, uint64_t S, DevMem* d_sb, TxText* T,
            uint64_t* nb) {
  int r;
  for (uint64_t i = 0; i < S; i++)
    if (sb[i] > sb[i + 1]) return fail(e, CTMR_E_INVAL, "%s: %s[%llu] lies behind its successor", who, what, (unsigned long long)i);
  T->lo = S ? sb[0] : 0;
  T->hi = S ? sb[S] : 0;
  *nb = 0;
  if (T->lo == T->hi) return CTMR_OK;
  if ((r = tx_alloc(e, who, d_sb, S + 1))) return r;
  HIPCHK(e, hipMemcpyAsync(d_sb->p, sb, (S + 1) * 8, hipMemcpyHostToDevice, e->stream));
  T->s = s;
  T->sb = (const uint64_t*)d_sb->p;
  T->S = S;
  T->a0 = ((uint64_t)(uintptr_t)s + T->lo) & ~15ull;
  *nb = ((uint64_t)(uintptr_t)s + T->hi - T->a0 + TX_TILE - 1) / TX_TILE;
  return CTMR_OK;
}

// *s = the device pointer the bounds hold for.  CTMR_E_INVAL when they hold bytes and there is no text.  A text in device
// memory (no d_text) is that pointer; of a host text the bytes inside the bounds are staged once (*d_text).
int tx_stage(ctmr_engine* e, const char* who, const uint8_t* text, const uint64_t* sb, uint64_t S, DevMem* d_text, const uint8_t** s) {
  const uint64_t lo = S ? sb[0] : 0, hi = S ? sb[S] : 0;
  if (hi > lo && !text) return fail(e, CTMR_E_INVAL, "%s: null text", who);
  *s = text;
  if (!d_text) return CTMR_OK;
  if (hi > lo) {
    if (d_text->alloc(hi - lo) != hipSuccess) return fail(e, CTMR_E_NOMEM, "%s: no device memory to stage %llu bytes", who, (unsigned long long)(hi - lo));
    HIPCHK(e, hipMemcpyAsync(d_text->p, text + lo, hi - lo, hipMemcpyHostToDevice, e->stream));
  }
  *s = (const uint8_t*)((uintptr_t)d_text->p - lo);
  return CTMR_OK;
}

// The tiles of n items.  bounds (n + 1, the scanned decoded lengths): tile_first is made here, the decode tiles of each
// item; no bounds: tile_first holds the tiles of each item already.  tile_first is scanned in place to the tiles before
// an item, *ntiles = their sum, tile_item[t] = the item of tile t.  Drains.
int tx_tile_list(ctmr_engine* e, const char* who, const DevMem* bounds, uint64_t n, DevMem* tile_first, DevMem* tile_item, uint64_t* ntiles) {
  int r;
  if (bounds) {
    if ((r = tx_alloc(e, who, tile_first, n + 1))) return r;
    tx_turns(tx_blocks(n, RP_BLOCK), [&](uint64_t b0, dim3 g) {
      hipLaunchKernelGGL(k_ej_tiles, g, dim3(RP_BLOCK), 0, e->stream, b0, (const unsigned long long*)bounds->p, n, (unsigned long long*)tile_first->p);
    });
  }
  if ((r = tx_scan(e, *tile_first, n, ntiles)) || (r = tx_alloc(e, who, tile_item, *ntiles))) return r;
  if (*ntiles)
    tx_turns(tx_blocks(n, RP_BLOCK), [&](uint64_t b0, dim3 g) {
      hipLaunchKernelGGL(k_ej_tile_list, g, dim3(RP_BLOCK), 0, e->stream, b0, (const unsigned long long*)tile_first->p, n,
                         (unsigned long long*)tile_item->p);
    });
  return CTMR_OK;
}

// CTMR_E_RANGE unless the caller's buffers hold the result: n items (`items`) and bytes + the padding of the output (`out`)
int tx_fits(ctmr_engine* e, const char* who, uint64_t n, const char* items, uint64_t bytes, const char* out, const void* out_buf, size_t out_cap,
            const void* bounds_buf, uint64_t items_cap) {
  if (!out_buf || !bounds_buf || out_cap < bytes + CTMR_PAYLOAD_PAD || items_cap < n)
    return fail(e, CTMR_E_RANGE, "%s: %llu %s and %llu + %d %s bytes needed", who, (unsigned long long)n, items, (unsigned long long)bytes,
                CTMR_PAYLOAD_PAD, out);
  return CTMR_OK;
}

// the end of a decode: the zero padding behind the bytes written to d_out; drains
int tx_finish(ctmr_engine* e, uint8_t* d_out, uint64_t bytes) {
  HIPCHK(e, hipMemsetAsync(d_out + bytes, 0, CTMR_PAYLOAD_PAD, e->stream));
  return tx_drain(e);
}

}  // namespace
}  // extern "C++"
