// engine/pipeline_writeback.inc — the back of the ingestion pipeline (DESIGN.md §24): what FilesystemDatabase.Store does for a
// certificate that WasUnknown (storage/filesystemdatabase.go:158-211) — IssuerMetadata.Accumulate, AllocateExpDateAndIssuer on
// a first (issuer, expDate), StoreCertificatePEM(pem.EncodeToMemory(...)) — for the tickets of ctmr_submit_*.
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after engine/meta.inc and engine/pem.inc.
//   ctmr_set_pipeline_writeback  the opt-in, per engine; a super-batch takes the flags as they stand when it is opened.
//   pipe_writeback_run           the worker's step behind a form's pipe_run_*, the engine's mutex still held: k_meta_new
//                                (meta_collect_locked) and k_pem_encode (pem_device_locked) over the super-batch's NEW list,
//                                the items grouped, ordered, rebased and their bytes packed on the device (kernels/writeback.h),
//                                everything copied into pinned buffers the slot owns.
//   ctmr_ticket_writeback        a ticket's slice of them, cut out on the host: the NEW list ascends, so a ticket's new
//                                entries — and with them its PEM blocks, its items and their bytes — are one contiguous range.

extern "C++" {
namespace {

int wb_pin_reserve(ctmr_engine* e, PinMem& m, size_t& cap, size_t need, const char* what) {
  if (need <= cap) return CTMR_OK;
  cap = 0;
  const size_t want = (size_t)pow2_at_least(need);
  if (m.alloc(want) != hipSuccess) return fail(e, CTMR_E_NOMEM, "no pinned memory for %zu bytes of %s", need, what);
  cap = want;
  return CTMR_OK;
}

// The first sightings of the NEW list, as the tickets want them.
int wb_items_run(ctmr_engine* e, PipeSlot& s, const uint8_t* der, const uint64_t* offs, const uint64_t* ends, uint64_t nn) {
  int r;
  uint64_t ni = 0;
  if ((r = meta_collect_locked(e, der, offs, ends, (const ctmr_record*)s.d_records.p, (const uint64_t*)s.d_new.p, nn, &ni))) return r;
  if (ni == 0) return CTMR_OK;
  if (ni >= 0xffffffffull || nn >= 0xffffffffull) return fail(e, CTMR_E_RANGE, "pipeline write-back: %llu items", (unsigned long long)ni);
  // the tickets' first entries (text forms: the worker has them from the bodies' first entries; the tickets are told later)
  const uint64_t nt = s.tickets.size();
  try {
    s.wb_tfirst.resize(nt + 1);
  } catch (const std::bad_alloc&) {
    return fail(e, CTMR_E_NOMEM, "no host memory for the bounds of %llu tickets", (unsigned long long)nt);
  }
  for (uint64_t t = 0; t < nt; t++) s.wb_tfirst[t] = pipe_is_text(s.form) ? s.body_first[s.tickets[t].body0] : s.tickets[t].first;
  s.wb_tfirst[nt] = s.n;
  // SC_WB: istart u64[nn + 1] | boff u64[ni + 1] | src u64[ni] | ticket_first u64[nt + 1] | placed MetaItem[ni] | where uint2[ni] | err u32
  const size_t o_istart = 0, o_boff = o_istart + (nn + 1) * 8, o_src = o_boff + (ni + 1) * 8, o_tf = o_src + ni * 8,
               o_placed = o_tf + (nt + 1) * 8, o_where = o_placed + ni * sizeof(MetaItem), o_err = o_where + ni * 8;
  if ((r = ensure(e, SC_WB, o_err + 16))) return r;
  uint8_t* W = (uint8_t*)e->d_scratch[SC_WB];
  WbArgs a;
  a.items = (MetaItem*)e->d_scratch[SC_ITEMS]; a.placed = (MetaItem*)(W + o_placed); a.n_items = ni;
  a.new_idx = (const uint64_t*)s.d_new.p; a.n_new = nn;
  a.istart = (unsigned long long*)(W + o_istart); a.where = (uint2*)(W + o_where);
  a.offsets = offs; a.ends = ends;
  a.ticket_first = (const uint64_t*)(W + o_tf); a.n_tickets = (uint32_t)nt;
  a.src = (unsigned long long*)(W + o_src); a.boff = (unsigned long long*)(W + o_boff);
  a.err = (uint32_t*)(W + o_err);
  HIPCHK(e, hipMemsetAsync(W + o_istart, 0, o_src - o_istart, e->stream));  // the counts and the lengths
  HIPCHK(e, hipMemsetAsync(a.err, 0, 4, e->stream));
  HIPCHK(e, hipMemcpyAsync(W + o_tf, s.wb_tfirst.data(), (nt + 1) * 8, hipMemcpyHostToDevice, e->stream));  // (the slot's vector outlives the copy)
  const dim3 gi((unsigned)((ni + 255) / 256)), gn((unsigned)((nn + 255) / 256));
  hipLaunchKernelGGL(k_wb_count, gi, dim3(256), 0, e->stream, a);
  if ((r = scan_u64(e, (uint64_t*)a.istart, nn + 1, false, SC_TMP))) return r;
  hipLaunchKernelGGL(k_wb_place, gi, dim3(256), 0, e->stream, a);
  hipLaunchKernelGGL(k_wb_order, gn, dim3(256), 0, e->stream, a);
  if ((r = scan_u64(e, (uint64_t*)a.boff, ni + 1, false, SC_TMP))) return r;
  uint64_t total = 0;
  uint32_t err = 0;
  HIPCHK(e, hipMemcpyAsync(&total, a.boff + ni, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(&err, a.err, 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  if (err & WB_E_TOO_MANY)
    return fail(e, CTMR_E_RANGE, "pipeline write-back: a certificate brought more than %u first sightings", WB_MAX_ITEMS);
  if (err) return fail(e, CTMR_E_HIP, "pipeline write-back: inconsistent items (flags %u)", err);
  if ((r = wb_pin_reserve(e, s.h_items, s.h_items_cap, ni * sizeof(ctmr_meta_item), "items")) ||
      (r = wb_pin_reserve(e, s.h_istart, s.h_istart_cap, (nn + 1) * 8, "item ranges")) ||
      (r = wb_pin_reserve(e, s.h_iboff, s.h_iboff_cap, (ni + 1) * 8, "item byte offsets")) ||
      (r = wb_pin_reserve(e, s.h_ibytes, s.h_ibytes_cap, total, "item bytes")))
    return r;
  if (total) {
    if ((r = ensure(e, SC_WBBYTES, total + 16))) return r;
    hipLaunchKernelGGL(k_wb_gather, dim3((unsigned)((ni + 3) / 4)), dim3(256), 0, e->stream, der, (const unsigned long long*)a.src,
                       (const unsigned long long*)a.boff, ni, (uint8_t*)e->d_scratch[SC_WBBYTES], total);
    HIPCHK(e, hipMemcpyAsync(s.h_ibytes.p, e->d_scratch[SC_WBBYTES], total, hipMemcpyDeviceToHost, e->stream));
  }
  HIPCHK(e, hipMemcpyAsync(s.h_items.p, a.items, ni * sizeof(ctmr_meta_item), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(s.h_istart.p, a.istart, (nn + 1) * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(s.h_iboff.p, a.boff, (ni + 1) * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  s.wb_items = ni;
  s.wb_item_bytes = total;
  return CTMR_OK;
}

// The PEM blocks of the NEW list: sized, encoded, copied out (as ctmr_pem_new, into the slot's pinned memory).
int wb_pem_run(ctmr_engine* e, PipeSlot& s, const uint8_t* der, const uint64_t* offs, const uint64_t* ends, uint64_t nn) {
  int r;
  if ((r = ensure(e, SC_PEMOFF, (nn + 1) * 8))) return r;
  uint64_t* d_po = (uint64_t*)e->d_scratch[SC_PEMOFF];
  const uint64_t* d_new = (const uint64_t*)s.d_new.p;
  uint64_t total = 0;
  if ((r = pem_device_locked(e, der, offs, d_new, nn, nullptr, 0, d_po, &total, ends))) return r;
  if ((r = ensure(e, SC_PEM, total + 64))) return r;
  if ((r = wb_pin_reserve(e, s.h_pem, s.h_pem_cap, total, "PEM")) || (r = wb_pin_reserve(e, s.h_pemoff, s.h_pemoff_cap, (nn + 1) * 8, "PEM offsets")))
    return r;
  if ((r = pem_device_locked(e, der, offs, d_new, nn, (uint8_t*)e->d_scratch[SC_PEM], total + 64, d_po, &total, ends))) return r;
  HIPCHK(e, hipMemcpyAsync(s.h_pem.p, e->d_scratch[SC_PEM], total, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(s.h_pemoff.p, d_po, (nn + 1) * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  s.wb_pem_bytes = total;
  return CTMR_OK;
}

int pipe_writeback_run(ctmr_engine* e, PipeSlot& s, const ctmr_entry_view& view) {
  s.wb_pem_bytes = s.wb_items = s.wb_item_bytes = 0;
  const uint64_t nn = s.stats.n_new;
  if (!s.wb || nn == 0) return CTMR_OK;
  // the certificates of the super-batch, as its map read them: packed and PEM forms by the offsets in d_meta over
  // d_payload / d_blob, raw and JSON forms by the view's cert_start / cert_end over the blob
  const bool raw = pipe_is_raw(s.form);
  const uint8_t* der = pipe_is_text(s.form) ? s.d_blob.u8() : s.d_payload.u8();
  const uint64_t* offs = raw ? view.cert_start : (const uint64_t*)s.d_meta.p;
  const uint64_t* ends = raw ? view.cert_end : nullptr;
  if (!der || !offs || (raw && !ends)) return fail(e, CTMR_E_HIP, "pipeline write-back: the super-batch left no certificates to read");
  int r;
  if ((s.wb & CTMR_WB_META) && (r = wb_items_run(e, s, der, offs, ends, nn))) return r;
  if ((s.wb & CTMR_WB_PEM) && (r = wb_pem_run(e, s, der, offs, ends, nn))) return r;
  return CTMR_OK;
}

}  // namespace
}  // extern "C++"

int ctmr_set_pipeline_writeback(ctmr_engine* e, uint32_t flags) {
  if (!e) return CTMR_E_INVAL;
  if (flags & ~(uint32_t)(CTMR_WB_PEM | CTMR_WB_META)) return fail(e, CTMR_E_INVAL, "unknown write-back flags %#x", flags);
  if ((flags & CTMR_WB_META) && (!e->cfg.collect_meta || !e->d_meta_slots)) return fail(e, CTMR_E_INVAL, "engine created without collect_meta");
  e->pipe_wb.store(flags, std::memory_order_relaxed);
  return CTMR_OK;
}

int ctmr_ticket_writeback(ctmr_engine* e, ctmr_ticket ticket, uint8_t* pem, uint64_t pem_cap, uint64_t* pem_offsets,
                          ctmr_meta_item* items, uint64_t items_cap, uint8_t* bytes, uint64_t bytes_cap, ctmr_writeback_info* info) {
  if (!e) return CTMR_E_INVAL;
  if (info) memset(info, 0, sizeof *info);
  ctmr_pipeline* p;
  int r;
  if ((r = pipe_get(e, &p))) return r;
  const uint64_t seq = ticket >> 20, tix = ticket & ((1u << 20) - 1);
  std::unique_lock<std::mutex> lk(p->mu);
  PipeSlot* s = nullptr;
  for (auto& c : p->slots)
    if (c.state != PS_FREE && c.seq == seq) s = &c;
  if (!s || tix >= s->tickets.size() || s->tickets[tix].consumed) return fail(e, CTMR_E_NOTFOUND, "unknown or already collected ticket");
  if (s->state == PS_OPEN && (r = pipe_close_locked(e, p))) return r;  // nobody else will launch it
  // (the ticket cannot be collected while this call sleeps and the slot not be reused: only its own wait collects it, and a
  // caller that runs both at once on one ticket gets either answer)
  p->cv.wait(lk, [&] { return s->state == PS_DONE; });
  if (s->seq != seq || s->tickets[tix].consumed) return fail(e, CTMR_E_NOTFOUND, "unknown or already collected ticket");
  if (s->rc != CTMR_OK) return fail(e, s->rc, "%s", s->err.c_str());
  const PipeTicket& t = s->tickets[tix];
  ctmr_writeback_info w{};
  w.flags = s->wb;
  if (!s->wb) {
    if (info) *info = w;
    return CTMR_OK;
  }
  // the ticket's range of the super-batch's NEW list (ascending), as its wait cuts it
  const uint64_t* nb = (const uint64_t*)s->h_new.p;
  const uint64_t nn = s->stats.n_new;
  const uint64_t lo = (uint64_t)(std::lower_bound(nb, nb + nn, t.first) - nb);
  const uint64_t hi = (uint64_t)(std::lower_bound(nb + lo, nb + nn, t.first + t.n) - nb);
  w.n_new = hi - lo;
  const bool has_pem = (s->wb & CTMR_WB_PEM) && nn, has_items = (s->wb & CTMR_WB_META) && s->wb_items;
  const uint64_t* po = (const uint64_t*)s->h_pemoff.p;
  const uint64_t* is = (const uint64_t*)s->h_istart.p;
  const uint64_t* ib = (const uint64_t*)s->h_iboff.p;
  const uint64_t i0 = has_items ? is[lo] : 0, i1 = has_items ? is[hi] : 0;
  if (has_pem) w.pem_bytes = po[hi] - po[lo];
  w.n_items = i1 - i0;
  if (has_items) w.item_bytes = ib[i1] - ib[i0];
  if (info) *info = w;
  const bool want_pem = (s->wb & CTMR_WB_PEM) != 0;
  if ((want_pem && w.n_new && !pem_offsets) || (w.pem_bytes && (!pem || pem_cap < w.pem_bytes)) ||
      (w.n_items && (!items || items_cap < w.n_items)) || (w.item_bytes && (!bytes || bytes_cap < w.item_bytes)))
    return fail(e, CTMR_E_RANGE, "write-back buffers too small: %llu new, %llu PEM bytes, %llu items, %llu item bytes", (unsigned long long)w.n_new,
                (unsigned long long)w.pem_bytes, (unsigned long long)w.n_items, (unsigned long long)w.item_bytes);
  if (pem_offsets) pem_offsets[0] = 0;
  if (has_pem && w.n_new) {
    for (uint64_t k = 0; k <= w.n_new; k++) pem_offsets[k] = po[lo + k] - po[lo];
    memcpy(pem, s->h_pem.u8() + po[lo], w.pem_bytes);
  }
  if (w.n_items) memcpy(items, (const ctmr_meta_item*)s->h_items.p + i0, w.n_items * sizeof(ctmr_meta_item));
  if (w.item_bytes) memcpy(bytes, s->h_ibytes.u8() + ib[i0], w.item_bytes);
  return CTMR_OK;
}
