// engine/map.inc — filter constants, map launch (variant dispatch), the batched map + reduce: ctmr_map_batch(_device).
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after the engine state.

int ctmr_set_filter(ctmr_engine* e, const char* filter, size_t len, int log_expired, int64_t now) {
  if (!e || (len && !filter)) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  FilterDev f;
  memset(&f, 0, sizeof f);
  f.active = len != 0;
  f.log_expired = log_expired != 0;
  f.now = now;
  f.strict_spki = e->strict_spki ? 1u : 0u;
  f.strict_strings = e->strict_strings ? 1u : 0u;
  f.strict_ext = e->strict_ext ? 1u : 0u;
  // strings.Split(filter, ","): pieces are NOT trimmed (ct-fetch.go:58)
  size_t s = 0;
  uint32_t nw = 0;
  for (;;) {
    size_t t = s;
    while (t < len && filter[t] != ',') t++;
    const size_t pl = t - s;
    if (f.n_pieces >= 64 || nw + (pl + 3) / 4 > 1024)
      return fail(e, CTMR_E_INVAL, "issuerCNFilter too large (max 64 pieces / 4096 bytes)");
    f.piece_len[f.n_pieces] = (uint32_t)pl;
    f.piece_word[f.n_pieces] = nw;
    memcpy((uint8_t*)(f.words + nw), filter + s, pl);
    nw += (uint32_t)((pl + 3) / 4);
    f.n_pieces++;
    if (t >= len) break;
    s = t + 1;
  }
  e->h_filter = f;
  return upload_filter(e);
}

static int launch_map(ctmr_engine* e, const uint8_t* d_payload, const uint64_t* d_offsets,
                      const uint32_t* d_issuer_idx, const uint8_t* d_entry_type, uint64_t n,
                      ctmr_record* d_records, bool optimistic_new, const InsertArgs* fuse = nullptr,
                      const uint64_t* d_ends = nullptr, uint64_t limit = 0, int mode = XM_LOCAL,
                      const XchgArgs* xchg = nullptr, uint64_t first = 0) {
  // first: the launch covers entries [first, first + n) of a round mapped in chunks (round_launch_range): every pointer
  // the caller passes is already shifted; the per-entry scratch arrays this function hands out are shifted here
  MapArgs ma;
  ma.optimistic_new = optimistic_new ? 1u : 0u;
  ma.ends = d_ends; ma.limit = limit;
  ma.meta_loc = nullptr;
  if (e->cfg.collect_meta) {
    int mr;
    if ((mr = ensure(e, SC_META, (first + n) * 8))) return mr;
    ma.meta_loc = (uint2*)e->d_scratch[SC_META] + first;
    e->meta_n = first + n;
    e->last_meta_valid = false;
  }
  ma.payload = d_payload; ma.offsets = d_offsets; ma.issuer_idx = d_issuer_idx;
  ma.entry_type = d_entry_type; ma.records = d_records; ma.issuer_valid = e->d_issuer_valid;
  ma.filt = e->d_filter; ma.n = n; ma.n_issuers = (uint32_t)e->issuers.size();
  ma.certs_per_tile = 0; ma.lds_bytes = 0;
  ma.keypos = nullptr;
  if (e->strict_spki && n) {  // where the map leaves the EC points that owe the curve equation (k_ec_resolve)
    int kr;
    if ((kr = ensure(e, SC_KEYPOS, (first + n) * 8))) return kr;
    ma.keypos = (unsigned long long*)e->d_scratch[SC_KEYPOS] + first;
  }
  // 15 (default) = k_map_fused, the map fused with pass 1 of the insert; 13 = k_map_winc, the same map on its own
  // (`map_variant = 13` + k_insert).  ctmr_create rejects everything else, except in CTMR_SWEEP builds
  // (libctmr_sweep.so: 1 = whole-certificate LDS tile, 2 = direct global loads).
  uint32_t variant = e->cfg.map_variant ? e->cfg.map_variant : 15;
  e->meta_precheck_n = 0;  // whatever ent[] held belongs to the batch before
  if (variant == 15 && !fuse) variant = 13;
  const dim3 grid((unsigned)((n + 63) / 64));
#ifdef CTMR_SWEEP
  // occupancy experiment (sweep build): extra dynamic LDS per wave lowers the waves per CU (17 408 B → 9, +3 072 → 8,
  // +8 192 → 6, +17 408 → 4) — how the kernel's time scales with it tells latency-bound from bandwidth-bound
  static const size_t extra_lds = getenv("CTMR_EXTRA_LDS") ? (size_t)atoi(getenv("CTMR_EXTRA_LDS")) : 0;
#else
  constexpr size_t extra_lds = 0;
#endif
  // (each instantiation brings its own window geometry: readers.h WinGeo)
  const bool strict = e->strict_strings || e->strict_ext;
  if (variant == 15) {
    MetaCheck mc{};
    XchgArgs xa{};
    if (xchg) xa = *xchg;
    bool meta = false;
    if (e->cfg.collect_meta && e->d_meta_slots) {  // the memo as earlier ctmr_meta_new calls left it: pre-check in the map
      mc.slots = e->d_meta_slots; mc.mask = e->n_meta_slots - 1; mc.arena = e->d_meta_arena;
      mc.hour_pages = e->d_meta_hour_pages; mc.n_hour_pages = e->d_meta_hour_pages ? (uint32_t)e->meta_hour_pages.size() : 0u;
      mc.refs = e->d_meta_refs; mc.n_refs = e->max_issuers;
      mc.enabled = 1;
      meta = true;
      e->meta_precheck_n = first + n;  // ent[] of this batch carries ENT_META_UNSEEN (meta_device_locked)
      e->meta_precheck_ent = fuse->ent - first;
    }
  // strict_strings: instantiations of their own (the default kernels do not carry the check)
#define CTMR_LAUNCH_FUSED(META, MODE)                                                                                        \
  do {                                                                                                                       \
    if (strict)                                                                                                              \
      hipLaunchKernelGGL((k_map_fused<WIN_CH_STRICT, META, MODE, true>), grid, dim3(64),                                     \
                         WinGeo<WIN_CH_STRICT>::LDS_BYTES + extra_lds, e->stream, ma, *fuse, mc, xa);                        \
    else                                                                                                                     \
      hipLaunchKernelGGL((k_map_fused<WIN_CH_FAST, META, MODE, false>), grid, dim3(64),                                      \
                         WinGeo<WIN_CH_FAST>::LDS_BYTES + extra_lds, e->stream, ma, *fuse, mc, xa);                          \
  } while (0)
    if (mode == XM_OWNER) { if (meta) CTMR_LAUNCH_FUSED(true, XM_OWNER); else CTMR_LAUNCH_FUSED(false, XM_OWNER); }
    else if (mode == XM_BLOOM) { if (meta) CTMR_LAUNCH_FUSED(true, XM_BLOOM); else CTMR_LAUNCH_FUSED(false, XM_BLOOM); }
    else { if (meta) CTMR_LAUNCH_FUSED(true, XM_LOCAL); else CTMR_LAUNCH_FUSED(false, XM_LOCAL); }
#undef CTMR_LAUNCH_FUSED
  } else if (variant == 13) {
    if (strict) hipLaunchKernelGGL((k_map_winc<WIN_CH_STRICT, true>), grid, dim3(64), WinGeo<WIN_CH_STRICT>::LDS_BYTES + extra_lds, e->stream, ma);
    else hipLaunchKernelGGL((k_map_winc<WIN_CH_FAST, false>), grid, dim3(64), WinGeo<WIN_CH_FAST>::LDS_BYTES + extra_lds, e->stream, ma);
#ifdef CTMR_SWEEP
  } else if (variant == 2) {
    hipLaunchKernelGGL(k_map_direct, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, ma);
  } else if (variant == 1 && !d_ends) {  // the whole-certificate tile copy needs the packed layout
    uint32_t C = e->cfg.certs_per_tile ? e->cfg.certs_per_tile : 32;
    if (C > 64) C = 64;
    uint32_t lds = e->cfg.lds_tile_bytes ? e->cfg.lds_tile_bytes : 65536;
    if (lds > 160 * 1024) lds = 160 * 1024;
    ma.certs_per_tile = C; ma.lds_bytes = lds;
    if (!e->tile_attr_set) {  // per engine = per device (one process may drive several devices)
      HIPCHK(e, hipFuncSetAttribute((const void*)k_map_tile, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      e->tile_attr_set = true;
    }
    hipLaunchKernelGGL(k_map_tile, dim3((unsigned)((n + C - 1) / C)), dim3(64), lds, e->stream, ma);
#endif
  } else {
    return fail(e, CTMR_E_INVAL, "map_variant %u is not built into this library", variant);
  }
  return CTMR_OK;
}

// ------------------------------------------------------------------ one batch = one ROUND of the reduce, in steps
// round_begin    map + pass 1 + pass 2 of the set insert for this shard's own keys (one stream, no synchronisation)
// round_resolve  WasUnknown / per-issuer counts / NEW count per block from ent[]; optionally the NEW-list compaction
// round_collect  statistics to the host (the one synchronisation of a plain batch), host-side set of over-long serials
// round_stats    ctmr_batch_stats
// A plain batch runs them back to back (map_device_locked).  The global-dedup modes (engine/exchange.inc) put their
// phases in between: the owner-computes exchange inserts the key records it received before round_resolve, and both
// modes take WasUnknown away from the entries that lost to another rank before the NEW list is compacted.
static bool round_fused(const ctmr_engine* e) { return e->cfg.map_variant == 0 || e->cfg.map_variant == 15; }

static void round_insert_args(ctmr_engine* e, const RoundCtx& rc, InsertArgs& ia) {
  ia.records = rc.d_records; ia.payload = rc.d_payload; ia.offsets = rc.d_offsets; ia.ends = rc.d_ends; ia.canon = e->d_canon;
  ia.t = e->tbl(); ia.ref0 = rc.ref0; ia.slot_id = (uint32_t*)e->d_scratch[SC_SLOTID];
  ia.ent = (uint32_t*)e->d_scratch[SC_ENT]; ia.n = rc.n; ia.stats = e->d_stats; ia.ord_base = rc.ord_base;
  ia.keypos = (const unsigned long long*)e->d_scratch[SC_KEYPOS]; ia.stage = nullptr; ia.bloom = nullptr; ia.bloom_wmask = 0;
}

// round_begin = round_prepare (capacity, the batch's key cells, scratch — no kernel) + round_launch_range over the whole
// batch.  The owner-computes exchange calls the two halves itself (engine/exchange.inc: xchg_map_range), so that it may
// launch the range in CHUNKS (ctmr_xchg_map_chunk_device): inside one round that is free — pass-1 claims commute and pass 2
// settles by order, whatever ran first (DESIGN.md §6) — and it lets chunk c's key records travel while chunk c + 1 is
// being walked.
static int round_prepare(ctmr_engine* e, RoundCtx& rc) {
  HIPCHK(e, hipSetDevice(e->device));
  e->rd.valid = false;
  const uint64_t n = rc.n;
  if (n >= 0xfffffff0ull) return fail(e, CTMR_E_INVAL, "batch too large (n < 2^32-16)");
  if (((uintptr_t)rc.d_payload & 15) != 0) return fail(e, CTMR_E_INVAL, "payload must be 16-byte aligned");
  int r;
  if (!rc.d_records) {
    if ((r = ensure(e, SC_RECORDS, n * sizeof(ctmr_record)))) return r;
    rc.d_records = (ctmr_record*)e->d_scratch[SC_RECORDS];
  }
  const uint64_t nb = (n + 1023) / 1024;
  if ((r = ensure(e, SC_SLOTID, n * 4))) return r;
  if ((r = ensure(e, SC_ENT, n * 4))) return r;
  if ((r = ensure(e, SC_BLKNEW, nb * 4))) return r;
  if ((r = ensure(e, SC_BLKBASE, nb * 8))) return r;
  if (e->strict_spki && n && (r = ensure(e, SC_KEYPOS, n * 8))) return r;  // (whole batch: chunks must not move it)
  if (e->cfg.collect_meta && (r = ensure(e, SC_META, n * 8))) return r;
  if ((r = ensure_capacity(e, n, true))) return r;  // every entry may claim a slot: grow / compact first, or fail before inserting
  rc.ref0 = e->arena_used;  // the batch's key cells: one per entry, in entry order
  e->arena_used += n;
  e->epoch++;
  e->pairs_dirty = true;
  HIPCHK(e, hipMemsetAsync(e->d_stats, 0, 2 * sizeof(DevStats), e->stream));
  const bool fused = round_fused(e);
  if (!fused && rc.mode == XM_OWNER) return fail(e, CTMR_E_INVAL, "the owner-computes exchange needs the fused map kernel (map_variant 0 / 15)");
  if (rc.mode == XM_LOCAL && fused && e->d_bloom) {  // an engine with a filter keeps it complete whoever calls the map
    rc.mode = XM_BLOOM;
  }
  if (rc.mode == XM_BLOOM && !e->d_bloom) return fail(e, CTMR_E_INVAL, "ctmr_bloom_config has not been called");
  return CTMR_OK;
}

// map + pass 1 (+ the curve equations owed, + pass 2 of this shard's own keys) for entries [lo, hi) of the prepared round;
// lo is a multiple of 1024 (the staging array and its per-wave counts are addressed per wave).  No synchronisation.
static int round_launch_range(ctmr_engine* e, RoundCtx& rc, const XchgArgs* xchg, uint64_t lo, uint64_t hi) {
  const uint64_t n = hi - lo;
  if (!n) return CTMR_OK;
  const bool prof = e->cfg.profile != 0;
  int r;
  // ---- map (PASS records leave it with WAS_UNKNOWN set; the reduce clears it for duplicates)
  InsertArgs ia;
  round_insert_args(e, rc, ia);
  ia.records += lo; ia.offsets += lo; ia.slot_id += lo; ia.ent += lo; ia.n = n; ia.ref0 += lo; ia.ord_base += (uint32_t)lo;
  if (ia.ends) ia.ends += lo;
  if (ia.keypos) ia.keypos += lo;
  const bool fused = round_fused(e);
  XchgArgs xa{};
  if (xchg) xa = *xchg;
  if (xa.stage) xa.stage += lo;
  if (xa.wave_cnt) xa.wave_cnt += (lo / 64) * MAX_WORLD;
  if (rc.mode == XM_BLOOM) {
    xa.bloom = e->d_bloom;
    xa.bloom_wmask = e->bloom_words - 1;
  }
  if (prof && lo == 0) HIPCHK(e, hipEventRecord(e->ev[0], e->stream));
  // (an owner-computes round of ONE rank owns every key: the plain kernel, nothing is staged)
  const int kmode = !fused ? XM_LOCAL : (rc.mode == XM_OWNER && rc.world == 1) ? XM_LOCAL : rc.mode;
  if ((r = launch_map(e, rc.d_payload, rc.d_offsets + lo, rc.d_issuer_idx + lo, rc.d_entry_type ? rc.d_entry_type + lo : nullptr, n,
                      rc.d_records + lo, true, fused ? &ia : nullptr, rc.d_ends ? rc.d_ends + lo : nullptr,
                      rc.blob_bytes + CTMR_PAYLOAD_PAD, kmode, &xa, lo)))
    return r;
  if (prof && hi == rc.n) HIPCHK(e, hipEventRecord(e->ev[1], e->stream));
  // ---- insert (pass 1 ran inside the map kernel when fused)
  if (!fused) hipLaunchKernelGGL(k_insert, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, ia);
  if (e->strict_spki) {  // EC keys that owe the curve equation: check, then insert (a batch without any: blocks that leave at once)
    ia.stage = (kmode == XM_OWNER) ? xa.stage : nullptr;
    ia.bloom = (rc.mode == XM_BLOOM && fused) ? xa.bloom : nullptr;
    ia.bloom_wmask = xa.bloom_wmask;
    hipLaunchKernelGGL(k_ec_resolve<true>, dim3((unsigned)((n + EC_PER_BLOCK - 1) / EC_PER_BLOCK)), dim3(256), 0, e->stream, ia, rc.d_records + lo);
    hipLaunchKernelGGL(k_ec_resolve<false>, dim3((unsigned)((n + EC_PER_BLOCK - 1) / EC_PER_BLOCK)), dim3(256), 0, e->stream, ia, rc.d_records + lo);
  }
  hipLaunchKernelGGL(k_insert2, dim3((unsigned)((n + INSERT2_PER_BLOCK - 1) / INSERT2_PER_BLOCK)), dim3(256), 0, e->stream, ia, rc.d_records + lo);
  if (!fused && rc.mode == XM_BLOOM)  // the unfused map cannot add to the filter on the way: a pass of its own
    hipLaunchKernelGGL(k_bloom_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, ia, e->d_bloom, e->bloom_words - 1);
  if (prof && hi == rc.n) HIPCHK(e, hipEventRecord(e->ev[2], e->stream));
  return CTMR_OK;
}

static int round_begin(ctmr_engine* e, RoundCtx& rc, const XchgArgs* xchg) {
  int r;
  if ((r = round_prepare(e, rc))) return r;
  return round_launch_range(e, rc, xchg, 0, rc.n);
}

static void round_compact(ctmr_engine* e, const RoundCtx& rc) {
  const uint64_t nb = (rc.n + 1023) / 1024;
  uint32_t* d_blk_new = (uint32_t*)e->d_scratch[SC_BLKNEW];
  uint64_t* d_blk_base = (uint64_t*)e->d_scratch[SC_BLKBASE];
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, e->stream, d_blk_new, nb, d_blk_base);
  hipLaunchKernelGGL(k_compact, dim3((unsigned)nb), dim3(256), 0, e->stream, (const ctmr_record*)rc.d_records,
                     (const uint32_t*)e->d_scratch[SC_ENT], rc.n, (const uint64_t*)d_blk_base, rc.d_new_idx);
}

static int round_resolve(ctmr_engine* e, RoundCtx& rc, bool compact_now) {
  const bool prof = e->cfg.profile != 0;
  const uint64_t nb = (rc.n + 1023) / 1024;
  ResolveArgs ra;
  ra.ent = (uint32_t*)e->d_scratch[SC_ENT]; ra.issuer_counts = e->issuer_counts; ra.stats = e->d_stats;
  ra.blk_new = (uint32_t*)e->d_scratch[SC_BLKNEW]; ra.n = rc.n;
  hipLaunchKernelGGL(k_resolve, dim3((unsigned)(nb < 512 ? nb : 512)), dim3(1024), 0, e->stream, ra, nb);
  if (prof) HIPCHK(e, hipEventRecord(e->ev[3], e->stream));
  // ---- compaction of the NEW list, queued right behind the resolve: the common case needs ONE synchronisation per
  //      batch (a host that feeds 1 001-entry batches — one get-entries response — pays for every extra round trip)
  rc.compacted = false;
  if (compact_now && rc.d_new_idx) {
    round_compact(e, rc);
    rc.compacted = true;
  }
  if (prof) HIPCHK(e, hipEventRecord(e->ev[4], e->stream));
  return CTMR_OK;
}

static int round_collect(ctmr_engine* e, RoundCtx& rc) {
  const uint64_t n = rc.n;
  uint32_t* d_ent = (uint32_t*)e->d_scratch[SC_ENT];
  uint32_t* d_blk_new = (uint32_t*)e->d_scratch[SC_BLKNEW];
  DevStats both[2];
  uint64_t ends[2] = {0, rc.blob_bytes};
  HIPCHK(e, hipMemcpyAsync(both, e->d_stats, sizeof both, hipMemcpyDeviceToHost, e->stream));
  if (!rc.d_ends && rc.payload_bytes_known == ~0ull) {
    HIPCHK(e, hipMemcpyAsync(&ends[0], rc.d_offsets, 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(&ends[1], rc.d_offsets + n, 8, hipMemcpyDeviceToHost, e->stream));
  } else if (!rc.d_ends) {
    ends[1] = rc.payload_bytes_known;
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  rc.hs = both[0];
  rc.remote_new = both[1].n_new;  // owner-computes round: received keys that were new here (k_keys_resolve)
  rc.payload_bytes = ends[1] - ends[0];  // entry view: the whole blob (leaf_input + extra_data)
  // one claimed slot per key that was new HERE (a key that left for its owner claims its slot there; long serials live in
  // the host-side set)
  if (!rc.own_counted) {
    e->occupied += rc.hs.n_new - rc.hs.n_remote + rc.remote_new;
  } else {
    // The table was rebuilt behind the shard's own claims (ctmr_xchg_insert_device): the rebuild's live count holds them,
    // and a received record that took such a slot over by its lower order (settle_order) is new without claiming a slot —
    // live + remote_new counted those twice (tests/test_gpu_xchg_corpus.py).  No member has left since the rebuild, so
    // the claimed slots are the live ones: counted, on this rare path, as the rebuild counted them.
    unsigned long long alive = 0;
    HIPCHK(e, hipMemsetAsync(e->d_count, 0, 8, e->stream));
    hipLaunchKernelGGL(k_count_live, dim3((unsigned)((e->nslots + 255) / 256)), dim3(256), 0, e->stream,
                       (const unsigned long long*)e->index, e->nslots, e->d_count);
    HIPCHK(e, hipMemcpyAsync(&alive, e->d_count, 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipGetLastError());
    e->occupied = alive;
  }
  if (rc.hs.n_full || both[1].n_full)  // cannot happen after ensure_capacity; kept as the kernels' own guard
    return fail(e, CTMR_E_FULL, "known-certificate table full (%llu slots): %llu entries dropped",
                (unsigned long long)e->nslots, rc.hs.n_full + both[1].n_full);

  // ---- serials longer than CTMR_MAX_SERIAL: exact host-side set, in log order (rare: the NEW list is rebuilt)
  rc.host_new = 0;
  rc.host_list.clear();
  if (rc.hs.n_host) {
    std::vector<uint32_t> ent(n);
    HIPCHK(e, hipMemcpy(ent.data(), d_ent, n * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n; i++) {
      if (((ent[i] >> 3) & 7u) != ES_HOST) continue;
      uint64_t off[2];
      ctmr_record rec;
      HIPCHK(e, hipMemcpy(off, rc.d_offsets + i, rc.d_ends ? 8 : 16, hipMemcpyDeviceToHost));
      if (rc.d_ends) HIPCHK(e, hipMemcpy(off + 1, rc.d_ends + i, 8, hipMemcpyDeviceToHost));
      HIPCHK(e, hipMemcpy(&rec, rc.d_records + i, sizeof rec, hipMemcpyDeviceToHost));
      std::vector<uint8_t> der(off[1] - off[0] + 32);
      HIPCHK(e, hipMemcpy(der.data(), rc.d_payload + off[0], off[1] - off[0], hipMemcpyDeviceToHost));
      HostReader hr{der.data()};
      Walk w;
      if (!walk_cert(hr, (uint32_t)(off[1] - off[0]), w, nullptr, e->strict_spki)) continue;  // cannot happen: map accepted it
      const uint32_t canon = e->issuers[rec.issuer_idx].canon;
      std::string key = make_key(e, rec.exp_hour, canon);
      std::string member((const char*)der.data() + w.serial_off, w.serial_len);
      if (e->hstore[key].insert(member).second) {
        rc.host_new++;
        e->host_issuer_counts[canon]++;
        rc.host_list.push_back({i, rec.exp_hour, canon, member});
        uint8_t fl = rec.flags | CTMR_FL_WAS_UNKNOWN;
        HIPCHK(e, hipMemcpy((uint8_t*)(rc.d_records + i) + 1, &fl, 1, hipMemcpyHostToDevice));
        const uint32_t en = (ent[i] & ~(7u << 3)) | (ES_CLAIMED << 3);  // compaction reads ent[]
        HIPCHK(e, hipMemcpy(d_ent + i, &en, 4, hipMemcpyHostToDevice));
        uint32_t bn;
        HIPCHK(e, hipMemcpy(&bn, d_blk_new + i / 1024, 4, hipMemcpyDeviceToHost));
        bn++;
        HIPCHK(e, hipMemcpy(d_blk_new + i / 1024, &bn, 4, hipMemcpyHostToDevice));
      }
    }
    if (rc.host_new && rc.compacted) {
      round_compact(e, rc);
      HIPCHK(e, hipStreamSynchronize(e->stream));
      HIPCHK(e, hipGetLastError());
    }
  }
  return CTMR_OK;
}

// A group round found that other ranks hold these long-serial members already (or met them at a lower log index of this
// round): which[] indexes rc.host_list.  They leave this rank's host-side set and lose WasUnknown.
static int round_host_drop(ctmr_engine* e, RoundCtx& rc, const std::vector<size_t>& which) {
  if (which.empty()) return CTMR_OK;
  uint32_t* d_ent = (uint32_t*)e->d_scratch[SC_ENT];
  uint32_t* d_blk_new = (uint32_t*)e->d_scratch[SC_BLKNEW];
  for (size_t idx : which) {
    const RoundCtx::HostNew& h = rc.host_list[idx];
    const std::string key = make_key(e, h.exp_hour, h.canon);
    auto it = e->hstore.find(key);
    if (it != e->hstore.end()) {
      it->second.erase(h.member);
      if (it->second.empty()) e->hstore.erase(it);
    }
    auto ic = e->host_issuer_counts.find(h.canon);
    if (ic != e->host_issuer_counts.end() && ic->second) ic->second--;
    uint8_t fl;
    HIPCHK(e, hipMemcpy(&fl, (uint8_t*)(rc.d_records + h.i) + 1, 1, hipMemcpyDeviceToHost));
    fl &= (uint8_t)~CTMR_FL_WAS_UNKNOWN;
    HIPCHK(e, hipMemcpy((uint8_t*)(rc.d_records + h.i) + 1, &fl, 1, hipMemcpyHostToDevice));
    uint32_t en;
    HIPCHK(e, hipMemcpy(&en, d_ent + h.i, 4, hipMemcpyDeviceToHost));
    en = (en & ~(7u << 3)) | (ES_DUP << 3);
    HIPCHK(e, hipMemcpy(d_ent + h.i, &en, 4, hipMemcpyHostToDevice));
    uint32_t bn;
    HIPCHK(e, hipMemcpy(&bn, d_blk_new + h.i / 1024, 4, hipMemcpyDeviceToHost));
    bn--;
    HIPCHK(e, hipMemcpy(d_blk_new + h.i / 1024, &bn, 4, hipMemcpyHostToDevice));
  }
  rc.host_new -= which.size();
  if (rc.d_new_idx) {
    round_compact(e, rc);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipGetLastError());
  }
  return CTMR_OK;
}

static void round_stats(ctmr_engine* e, const RoundCtx& rc, ctmr_batch_stats* stats) {
  if (!stats) return;
  memset(stats, 0, sizeof *stats);
  stats->n = rc.n;
  for (int k = 0; k < CTMR_ST__COUNT; k++) stats->by_status[k] = rc.hs.by_status[k];
  stats->n_new = rc.hs.n_new + rc.host_new - rc.lost;
  stats->n_dup = rc.hs.n_dup + (rc.hs.n_host - rc.host_new) + rc.lost;
  stats->n_host_set = rc.hs.n_host;
  stats->payload_bytes = rc.payload_bytes;
  stats->map_launches = 1;
  if (e->cfg.profile) {
    (void)hipEventElapsedTime(&stats->ms_map, e->ev[0], e->ev[1]);
    (void)hipEventElapsedTime(&stats->ms_insert, e->ev[1], e->ev[2]);
    if (rc.mode != XM_OWNER) {  // (an owner round's resolve waits for the exchange: see ctmr_group_stats for its phases)
      (void)hipEventElapsedTime(&stats->ms_resolve, e->ev[2], e->ev[3]);
      (void)hipEventElapsedTime(&stats->ms_compact, e->ev[3], e->ev[4]);
      (void)hipEventElapsedTime(&stats->ms_total, e->ev[0], e->ev[4]);
    }
  }
}

static int map_device_locked(ctmr_engine* e, const uint8_t* d_payload, const uint64_t* d_offsets,
                             const uint32_t* d_issuer_idx, const uint8_t* d_entry_type, uint64_t n,
                             ctmr_record* d_records, uint64_t* d_new_idx, ctmr_batch_stats* stats,
                             const uint64_t* d_ends = nullptr, uint64_t blob_bytes = 0,
                             uint64_t payload_bytes_known = ~0ull, bool compact_now = true) {
  HIPCHK(e, hipSetDevice(e->device));
  if (stats) memset(stats, 0, sizeof *stats);
  e->rd.valid = false;
  if (n == 0) return CTMR_OK;
  RoundCtx rc;
  rc.d_payload = d_payload; rc.d_offsets = d_offsets; rc.d_ends = d_ends; rc.d_issuer_idx = d_issuer_idx;
  rc.d_entry_type = d_entry_type; rc.n = n; rc.blob_bytes = blob_bytes; rc.payload_bytes_known = payload_bytes_known;
  rc.d_records = d_records; rc.d_new_idx = d_new_idx;
  int r;
  if ((r = round_begin(e, rc, nullptr))) return r;
  if ((r = round_resolve(e, rc, compact_now))) return r;
  if ((r = round_collect(e, rc))) return r;
  round_stats(e, rc, stats);
  e->rd = rc;
  e->rd.valid = true;  // ent[] / blk_new[] describe this batch until the next map call (ctmr_bloom_apply_device continues it)
  return CTMR_OK;
}

int ctmr_map_batch_device(ctmr_engine* e, const uint8_t* d_payload, const uint64_t* d_offsets,
                          const uint32_t* d_issuer_idx, const uint8_t* d_entry_type, uint64_t n,
                          ctmr_record* d_records, uint64_t* d_new_idx, ctmr_batch_stats* stats) {
  if (!e || (n && (!d_payload || !d_offsets || !d_issuer_idx))) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  return map_device_locked(e, d_payload, d_offsets, d_issuer_idx, d_entry_type, n, d_records, d_new_idx, stats);
}

int ctmr_map_batch(ctmr_engine* e, const uint8_t* payload, const uint64_t* offsets,
                   const uint32_t* issuer_idx, const uint8_t* entry_type, uint64_t n,
                   ctmr_record* records, uint64_t* new_idx, ctmr_batch_stats* stats) {
  if (!e || (n && (!payload || !offsets || !issuer_idx))) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (stats) memset(stats, 0, sizeof *stats);
  if (n == 0) return CTMR_OK;
  for (uint64_t i = 0; i < n; i++)
    if (offsets[i + 1] < offsets[i]) return fail(e, CTMR_E_INVAL, "offsets not monotone at %llu", (unsigned long long)i);
  const uint64_t base = offsets[0], bytes = offsets[n] - base;
  // staging layout in SC_STAGE_A: payload | pad ; SC_STAGE_B: offsets | issuer_idx | entry_type | new_idx
  int r;
  if ((r = ensure(e, SC_STAGE_A, bytes + CTMR_PAYLOAD_PAD + 16))) return r;
  const size_t o_off = 0, o_iss = (n + 1) * 8, o_et = o_iss + n * 4, o_new = (o_et + n + 15) & ~(size_t)15;
  if ((r = ensure(e, SC_STAGE_B, o_new + n * 8))) return r;
  uint8_t* B = (uint8_t*)e->d_scratch[SC_STAGE_B];
  // rel[] lives in the engine: the uploads are ordered before the kernels on the stream and every caller buffer
  // is consumed before this call returns (the call ends with a synchronisation), so no sync is needed here
  std::vector<uint64_t>& rel = e->h_rel;
  rel.resize(n + 1);
  for (uint64_t i = 0; i <= n; i++) rel[i] = offsets[i] - base;
  HIPCHK(e, hipMemcpyAsync(e->d_scratch[SC_STAGE_A], payload + base, bytes, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(B + o_off, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(B + o_iss, issuer_idx, n * 4, hipMemcpyHostToDevice, e->stream));
  if (entry_type) HIPCHK(e, hipMemcpyAsync(B + o_et, entry_type, n, hipMemcpyHostToDevice, e->stream));
  ctmr_batch_stats st;
  r = map_device_locked(e, (const uint8_t*)e->d_scratch[SC_STAGE_A], (const uint64_t*)(B + o_off),
                        (const uint32_t*)(B + o_iss), entry_type ? B + o_et : nullptr, n, nullptr,
                        new_idx ? (uint64_t*)(B + o_new) : nullptr, &st, nullptr, 0, bytes);
  if (r) return r;
  if (records) HIPCHK(e, hipMemcpyAsync(records, e->d_scratch[SC_RECORDS], n * sizeof(ctmr_record), hipMemcpyDeviceToHost, e->stream));
  if (new_idx && st.n_new) HIPCHK(e, hipMemcpyAsync(new_idx, B + o_new, st.n_new * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (stats) *stats = st;
  e->last_n = n; e->last_n_new = new_idx ? st.n_new : 0; e->last_o_off = o_off; e->last_o_new = o_new;
  e->last_is_view = false;
  return CTMR_OK;
}
