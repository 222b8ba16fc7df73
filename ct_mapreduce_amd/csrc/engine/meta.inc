// engine/meta.inc — IssuerMetadata memo (N3).
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after the engine state.

// ------------------------------------------------------------------ IssuerMetadata on device (N3)

constexpr size_t META_HOUR_PAGE_BYTES = (size_t)META_HOUR_PAGE * (META_HOUR_BITS / 8);

// one (issuer, hour) bitmap page per META_HOUR_PAGE registered issuers
static int meta_hour_pages_locked(ctmr_engine* e) {
  const size_t need = (e->issuers.size() + META_HOUR_PAGE - 1) / META_HOUR_PAGE;
  if (e->meta_hour_pages.size() >= need) return CTMR_OK;
  if (!e->d_meta_hour_pages) {
    const size_t cap = ((size_t)e->max_issuers + META_HOUR_PAGE - 1) / META_HOUR_PAGE;
    if (hipMalloc(&e->d_meta_hour_pages, cap * sizeof(uint32_t*)) != hipSuccess) {
      (void)hipGetLastError();
      return fail(e, CTMR_E_NOMEM, "expDate bitmap page table");
    }
  }
  while (e->meta_hour_pages.size() < need) {
    uint32_t* p = nullptr;
    if (hipMalloc(&p, META_HOUR_PAGE_BYTES) != hipSuccess) {
      (void)hipGetLastError();
      return fail(e, CTMR_E_NOMEM, "expDate bitmap page (%zu bytes)", META_HOUR_PAGE_BYTES);
    }
    HIPCHK(e, hipMemsetAsync(p, 0, META_HOUR_PAGE_BYTES, e->stream));
    e->meta_hour_pages.push_back(p);
  }
  HIPCHK(e, hipMemcpyAsync(e->d_meta_hour_pages, e->meta_hour_pages.data(), e->meta_hour_pages.size() * sizeof(uint32_t*),
                           hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));  // the vector may move before the copy has read it
  return CTMR_OK;
}

static int meta_reset_locked(ctmr_engine* e) {
  if (!e->d_meta_slots) return CTMR_OK;
  HIPCHK(e, hipMemsetAsync(e->d_meta_slots, 0, e->n_meta_slots * sizeof(MetaSlot), e->stream));
  HIPCHK(e, hipMemsetAsync(e->d_meta_refs, 0, (size_t)e->max_issuers * 16, e->stream));
  for (auto p : e->meta_hour_pages) HIPCHK(e, hipMemsetAsync(p, 0, META_HOUR_PAGE_BYTES, e->stream));
  HIPCHK(e, hipMemsetAsync(e->d_mcount, 0, 64, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->last_meta_valid = false;
  e->meta_precheck_n = 0;
  return CTMR_OK;
}

static int meta_device_locked(ctmr_engine* e, const uint8_t* d_payload, const uint64_t* d_offsets, const uint64_t* d_ends,
                              const ctmr_record* d_records, const uint64_t* d_new_idx, uint64_t n_new,
                              ctmr_meta_item* d_items, uint64_t items_cap, uint64_t* n_items) {
  HIPCHK(e, hipSetDevice(e->device));
  if (n_items) *n_items = 0;
  if (!e->cfg.collect_meta || !e->d_meta_slots) return fail(e, CTMR_E_INVAL, "engine created without collect_meta");
  if (n_new == 0) return CTMR_OK;
  if (!e->d_scratch[SC_META] || e->meta_n == 0) return fail(e, CTMR_E_INVAL, "no map call precedes ctmr_meta_new");
  MetaArgs a;
  a.payload = d_payload; a.offsets = d_offsets; a.ends = d_ends; a.records = d_records; a.canon = e->d_canon;
  a.meta_loc = (const uint2*)e->d_scratch[SC_META]; a.new_idx = d_new_idx; a.n_new = n_new;
  a.slots = e->d_meta_slots; a.mask = e->n_meta_slots - 1; a.arena = e->d_meta_arena; a.arena_cap = e->meta_arena_cap;
  a.counters = e->d_mcount; a.items = (MetaItem*)d_items; a.items_cap = items_cap;
  a.epoch = ++e->meta_epoch;
  a.refs = e->d_meta_refs; a.n_refs = e->max_issuers;
  int rp = meta_hour_pages_locked(e);
  if (rp) return rp;
  a.hour_pages = e->d_meta_hour_pages; a.n_hour_pages = (uint32_t)e->meta_hour_pages.size();
  // the map kernel's pre-check is valid for the batch it ran on, against the memo it saw: same entry count, no memo
  // reset since (a reset forgets what "seen" meant)
  a.ent = (e->meta_precheck_n == e->meta_n && e->meta_precheck_n != 0) ? e->meta_precheck_ent : nullptr;
  HIPCHK(e, hipMemsetAsync(e->d_mcount + 1, 0, 8, e->stream));
  hipLaunchKernelGGL(k_meta_new, dim3((unsigned)((n_new + 255) / 256)), dim3(256), 0, e->stream, a);
  unsigned long long hc[3];
  HIPCHK(e, hipMemcpyAsync(hc, e->d_mcount, 24, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  if (n_items) *n_items = hc[1];
  if (hc[1] > items_cap) {
    int r = meta_reset_locked(e);
    if (r) return r;
    return fail(e, CTMR_E_RANGE, "meta item buffer too small: %llu items (memo cleared; call again)", hc[1]);
  }
  return CTMR_OK;
}

// The first sightings among the nn new certificates of a batch into SC_ITEMS, sized here: ctmr_meta_new's and the ingestion
// pipeline's write-back (engine/pipeline_writeback.inc) both collect through this one loop.  An item buffer that turns out
// too small clears the memo (meta_device_locked) and the run is repeated, up to three runs.
static int meta_collect_locked(ctmr_engine* e, const uint8_t* d_payload, const uint64_t* d_offsets, const uint64_t* d_ends,
                               const ctmr_record* d_records, const uint64_t* d_new_idx, uint64_t nn, uint64_t* n_items) {
  *n_items = 0;
  if (nn == 0) return CTMR_OK;
  int r;
  uint64_t cap = std::min<uint64_t>(3 * nn + 1024, 16ull << 20);
  for (int attempt = 0;; attempt++) {
    if ((r = ensure(e, SC_ITEMS, cap * sizeof(ctmr_meta_item)))) return r;
    uint64_t got = 0;
    r = meta_device_locked(e, d_payload, d_offsets, d_ends, d_records, d_new_idx, nn, (ctmr_meta_item*)e->d_scratch[SC_ITEMS], cap, &got);
    if (r == CTMR_OK) {
      *n_items = got;
      return CTMR_OK;
    }
    if (r != CTMR_E_RANGE || attempt == 2) return r;
    // the memo was cleared: the next run re-reports everything into a buffer that fits.  `got` of the FIRST run counted
    // against the memo earlier batches left — a cold memo reports those items again, and when they are more than the
    // 1024 of slack the second run overflows too; its own count is the cold one, which the third run repeats.
    cap = got + 1024;
  }
}

int ctmr_meta_new_device(ctmr_engine* e, const uint8_t* d_payload, const uint64_t* d_offsets, const uint64_t* d_ends,
                         const ctmr_record* d_records, const uint64_t* d_new_idx, uint64_t n_new,
                         ctmr_meta_item* d_items, uint64_t items_cap, uint64_t* n_items) {
  if (!e || (n_new && (!d_payload || !d_offsets || !d_records || !d_new_idx || !d_items))) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  return meta_device_locked(e, d_payload, d_offsets, d_ends, d_records, d_new_idx, n_new, d_items, items_cap, n_items);
}

int ctmr_meta_reset(ctmr_engine* e) {
  if (!e) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  return meta_reset_locked(e);
}

int ctmr_meta_new(ctmr_engine* e, ctmr_meta_item* items, uint64_t items_cap, uint8_t* bytes, size_t bytes_cap,
                  uint64_t* n_items, size_t* bytes_need) {
  if (!e) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (n_items) *n_items = 0;
  if (bytes_need) *bytes_need = 0;
  const uint64_t nn = e->last_n_new;
  if (nn == 0) return CTMR_OK;
  uint8_t* B = (uint8_t*)e->d_scratch[SC_STAGE_B];
  const uint8_t* V = (const uint8_t*)e->d_scratch[SC_VIEW];
  const uint64_t* offs = e->last_is_view ? (const uint64_t*)(V + e->last_o_start) : (const uint64_t*)(B + e->last_o_off);
  const uint64_t* ends = e->last_is_view ? (const uint64_t*)(V + e->last_o_end) : nullptr;
  int r;
  if (!e->last_meta_valid) {
    if ((r = meta_collect_locked(e, (const uint8_t*)e->d_scratch[SC_STAGE_A], offs, ends, (const ctmr_record*)e->d_scratch[SC_RECORDS],
                                 (const uint64_t*)(B + e->last_o_new), nn, &e->last_meta_items)))
      return r;
    e->last_meta_valid = true;
  }
  const uint64_t ni = e->last_meta_items;
  if (n_items) *n_items = ni;
  std::vector<ctmr_meta_item> h(ni);
  if (ni) HIPCHK(e, hipMemcpy(h.data(), e->d_scratch[SC_ITEMS], ni * sizeof(ctmr_meta_item), hipMemcpyDeviceToHost));
  size_t need = 0;
  for (auto& it : h) {
    if (it.kind == CTMR_MK_HOST || it.kind == CTMR_MK_EXPDATE) it.len = 0;
    need += it.len;
  }
  if (bytes_need) *bytes_need = need;
  if (ni > items_cap || need > bytes_cap || (ni && !items) || (need && !bytes))
    return fail(e, CTMR_E_RANGE, "meta buffers too small: %llu items, %llu bytes", (unsigned long long)ni, (unsigned long long)need);
  size_t at = 0;
  for (uint64_t k = 0; k < ni; k++) {
    if (h[k].len) {
      uint64_t lo = 0;
      HIPCHK(e, hipMemcpy(&lo, offs + h[k].entry, 8, hipMemcpyDeviceToHost));
      HIPCHK(e, hipMemcpy(bytes + at, (const uint8_t*)e->d_scratch[SC_STAGE_A] + lo + h[k].off, h[k].len, hipMemcpyDeviceToHost));
      at += h[k].len;
    }
    items[k] = h[k];
  }
  return CTMR_OK;
}
