// engine/exchange.inc — cross-GPU global dedup: owner-computes key exchange and the Bloom pre-filter variant.
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after the engine state.

// ------------------------------------------------------------------ cross-GPU key exchange (owner-computes), per rank
// One round on one rank = four calls (engine/group.inc drives them, with the two all-to-alls in between):
//   ctmr_xchg_map_device     this shard's map + the insert of the keys this rank owns (the fused kernel) + the keys it
//                            does not own as 32-byte records; tells how many go to each owner
//   ctmr_xchg_keys_device    those records, partitioned by owner, into the caller's send buffers
//   ctmr_xchg_insert_device  what the rank received: two-pass insert into the round of its own shard, one byte back per record;
//                            then this shard's WasUnknown / counts (entries beaten by a received record included)
//   ctmr_xchg_apply_device   the bytes that came back: entries whose key was known to its owner lose WasUnknown; NEW list; stats

static int xchg_round_check(ctmr_engine* e, const char* what) {
  if (!e->rd.valid || e->rd.mode != XM_OWNER) return fail(e, CTMR_E_INVAL, "%s: no owner-computes round is open (ctmr_xchg_map_device first)", what);
  return CTMR_OK;
}

// Opens the round of one shard: fills the RoundCtx, makes room, and leaves it in e->rd with `valid` false — a round that
// fails before its last range has run is never taken for an open one.  An empty shard still owns keys: its round (the one
// its received records are inserted in) is complete at once.
static int xchg_round_open(ctmr_engine* e, const ctmr_shard* sh, uint32_t world, uint32_t rank, uint32_t ord_base, bool chunked) {
  e->rd.valid = false;
  RoundCtx rc;
  rc.mode = XM_OWNER; rc.world = world; rc.rank = rank; rc.ord_base = ord_base;
  rc.d_payload = sh->d_payload; rc.d_offsets = sh->d_offsets; rc.d_ends = sh->d_ends; rc.d_issuer_idx = sh->d_issuer_idx;
  rc.d_entry_type = sh->d_entry_type; rc.n = sh->n; rc.blob_bytes = sh->blob_bytes;
  rc.d_records = sh->d_records; rc.d_new_idx = sh->d_new_idx;
  rc.counts32.assign(world, 0);
  rc.chunked = chunked;
  const uint64_t n = sh->n;
  if ((uint64_t)ord_base + n > 0xffffffffull) return fail(e, CTMR_E_INVAL, "a round holds fewer than 2^32 entries over all ranks");
  if (n == 0) {
    e->epoch++;
    rc.ref0 = e->arena_used;
    e->pairs_dirty = true;
    HIPCHK(e, hipMemsetAsync(e->d_stats, 0, 2 * sizeof(DevStats), e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->rd = rc;
    e->rd.valid = true;
    return CTMR_OK;
  }
  int r;
  if (world > 1) {
    const uint64_t nb = (n + 1023) / 1024, n_waves = (n + 63) / 64, ncnt = (uint64_t)world * nb;
    if ((r = ensure(e, SC_XSTAGE, n_waves * 64 * sizeof(KeyRec32)))) return r;
    if ((r = ensure(e, SC_XWCNT, n_waves * MAX_WORLD + 16))) return r;
    if ((r = ensure(e, SC_XCNT, (ncnt + 1) * 4))) return r;
    if ((r = ensure(e, SC_XBASE, (ncnt + 1) * 8))) return r;
  }
  if ((r = round_prepare(e, rc))) return r;
  e->rd = rc;
  return CTMR_OK;
}

// The key records that entries [lo, hi) export, counted per owner: per-block counts, their scan into partition bases
// (SC_XBASE, on the device), and the W + 1 bases on their way to the host — in `base` once the stream has been drained.
// With `deliver` the records are gathered at once into d_keys32_out (the gather needs the bases on the device only).
static int xchg_count_range(ctmr_engine* e, uint32_t world, uint64_t lo, uint64_t hi, bool deliver, void* d_keys32_out,
                            std::vector<uint64_t>& base) {
  const uint64_t cn = hi - lo, nb = (cn + 1023) / 1024, n_waves = (cn + 63) / 64, ncnt = (uint64_t)world * nb;
  uint32_t* d_cnt = (uint32_t*)e->d_scratch[SC_XCNT];
  uint64_t* d_base = (uint64_t*)e->d_scratch[SC_XBASE];
  const uint8_t* wc = (const uint8_t*)e->d_scratch[SC_XWCNT] + (lo / 64) * MAX_WORLD;
  HIPCHK(e, hipMemsetAsync(d_cnt, 0, (ncnt + 1) * 4, e->stream));
  hipLaunchKernelGGL(k_key_blockcount, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, e->stream, wc, n_waves, nb, world, d_cnt);
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, e->stream, d_cnt, ncnt + 1, d_base);
  if (deliver) {
    if (!d_keys32_out) return fail(e, CTMR_E_INVAL, "ctmr_xchg_map_chunk_device: null output buffer");
    hipLaunchKernelGGL(k_key_gather, dim3((unsigned)nb), dim3(1024), 0, e->stream, (const KeyRec32*)e->d_scratch[SC_XSTAGE] + lo, wc,
                       n_waves, nb, world, (const uint64_t*)d_base, (KeyRec32*)d_keys32_out);
  }
  // the W + 1 partition bases lie nb words apart: ONE strided copy (each small copy of its own costs ≈ 20 µs on the stream)
  base.resize(world + 1);
  HIPCHK(e, hipMemcpy2DAsync(base.data(), 8, d_base, nb * 8, 8, world + 1, hipMemcpyDeviceToHost, e->stream));
  return CTMR_OK;
}

// Both forms of the map: entries [lo, hi) of the shard are mapped, their own duplicates settled, and the key records they
// export counted per owner.  lo == 0 opens the round, hi == n completes it.  `chunked` says who delivers the 32-byte
// records: this call, range by range, into d_keys32_out — or ctmr_xchg_keys_device afterwards, for the whole shard.
// ONE stream synchronisation: the bases and n_xl are read behind it (and, chunked, the gather has finished: the caller may
// hand the buffer to the transport).
static int xchg_map_range(ctmr_engine* e, const ctmr_shard* sh, uint32_t world, uint32_t rank, uint32_t ord_base, uint64_t lo,
                          uint64_t hi, bool chunked, void* d_keys32_out, uint64_t* counts32, uint64_t* n_long) {
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  for (uint32_t w = 0; w < world; w++) counts32[w] = 0;
  *n_long = 0;
  const uint64_t n = sh->n;
  int r;
  if (lo == 0) {
    if ((r = xchg_round_open(e, sh, world, rank, ord_base, chunked))) return r;
    if (n == 0) return CTMR_OK;
  }
  RoundCtx& rc = e->rd;
  // (a later chunk continues the round its first chunk opened, and no other)
  if (lo && (!rc.chunked || rc.mode != XM_OWNER || rc.valid || rc.chunk_next != lo || rc.n != n || rc.world != world || rc.rank != rank))
    return fail(e, CTMR_E_INVAL, "ctmr_xchg_map_chunk_device: chunks must cover the shard in ascending order, starting at 0");
  XchgArgs xa{};
  xa.world = world; xa.rank = rank;
  if (world > 1) {
    xa.stage = (KeyRec32*)e->d_scratch[SC_XSTAGE];
    xa.wave_cnt = (uint8_t*)e->d_scratch[SC_XWCNT];
  }
  if ((r = round_launch_range(e, rc, &xa, lo, hi))) return r;
  std::vector<uint64_t> base;
  if (world > 1 && hi > lo && (r = xchg_count_range(e, world, lo, hi, chunked, d_keys32_out, base))) return r;
  const bool last = hi == n;
  unsigned long long nxl = 0;
  if (last && world > 1) HIPCHK(e, hipMemcpyAsync(&nxl, &e->d_stats->n_xl, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));  // (world 1 too: so that a caller's phase clock sees the map where it ran)
  HIPCHK(e, hipGetLastError());
  if (!base.empty())
    for (uint32_t w = 0; w < world; w++) {
      counts32[w] = base[w + 1] - base[w];
      rc.counts32[w] += counts32[w];
    }
  rc.chunk_next = hi;
  if (last) {  // the round is complete
    rc.n_xl = *n_long = nxl;
    rc.valid = true;
  }
  return CTMR_OK;
}

int ctmr_xchg_map_device(ctmr_engine* e, const ctmr_shard* sh, uint32_t world, uint32_t rank, uint32_t ord_base,
                         uint64_t* counts32, uint64_t* n_long) {
  if (!e || !sh || !counts32 || !n_long || world == 0 || world > MAX_WORLD || rank >= world ||
      (sh->n && (!sh->d_payload || !sh->d_offsets || !sh->d_issuer_idx || !sh->d_records)))
    return CTMR_E_INVAL;
  return xchg_map_range(e, sh, world, rank, ord_base, 0, sh->n, false, nullptr, counts32, n_long);
}

// The same map in CHUNKS (ctmr_group_set_chunks): entries [lo, hi) of the shard — lo a multiple of 1024, chunks in ascending
// order, the first with lo = 0, the last with hi = sh->n — are mapped, their own duplicates settled, and the key records
// they export are gathered at once into d_keys32_out (per-owner partitions of THIS chunk, ascending order inside;
// counts32[w] = how many for owner w).  The caller can put chunk c on the wire while chunk c + 1 is being walked: inside
// one round the order in which keys reach their owner does not matter (pass-1 claims commute, pass 2 settles by order).
// After the last chunk the round is where ctmr_xchg_map_device leaves it; ctmr_xchg_keys_device then delivers only the
// 64-byte records of 21..40-octet serials (*n_long, set by the last chunk).
int ctmr_xchg_map_chunk_device(ctmr_engine* e, const ctmr_shard* sh, uint32_t world, uint32_t rank, uint32_t ord_base,
                               uint64_t lo, uint64_t hi, void* d_keys32_out, uint64_t* counts32, uint64_t* n_long) {
  if (!e || !sh || !counts32 || !n_long || world == 0 || world > MAX_WORLD || rank >= world || lo > hi || hi > sh->n ||
      (lo & 1023) || (sh->n && (!sh->d_payload || !sh->d_offsets || !sh->d_issuer_idx || !sh->d_records)))
    return CTMR_E_INVAL;
  return xchg_map_range(e, sh, world, rank, ord_base, lo, hi, true, d_keys32_out, counts32, n_long);
}

int ctmr_xchg_keys_device(ctmr_engine* e, void* d_keys32_out, void* d_keys64_out, uint64_t* counts64) {
  if (!e) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  int r;
  if ((r = xchg_round_check(e, "ctmr_xchg_keys_device"))) return r;
  RoundCtx& rc = e->rd;
  if (counts64) for (uint32_t w = 0; w < rc.world; w++) counts64[w] = 0;
  if (rc.n == 0 || rc.world == 1) return CTMR_OK;
  uint64_t total = 0;
  for (auto c : rc.counts32) total += c;
  if (rc.chunked) total = 0;  // gathered chunk by chunk already (ctmr_xchg_map_chunk_device)
  if ((total && !d_keys32_out) || (rc.n_xl && (!d_keys64_out || !counts64))) return fail(e, CTMR_E_INVAL, "ctmr_xchg_keys_device: null output buffer");
  const uint64_t nb = (rc.n + 1023) / 1024, n_waves = (rc.n + 63) / 64;
  if (total)
    hipLaunchKernelGGL(k_key_gather, dim3((unsigned)nb), dim3(1024), 0, e->stream, (const KeyRec32*)e->d_scratch[SC_XSTAGE],
                       (const uint8_t*)e->d_scratch[SC_XWCNT], n_waves, nb, rc.world, (const uint64_t*)e->d_scratch[SC_XBASE],
                       (KeyRec32*)d_keys32_out);
  if (rc.n_xl) {  // rare: serials of 21..40 octets — collected unordered, put in (owner, order) order by the host
    if ((r = ensure(e, SC_XL, rc.n_xl * sizeof(KeyRec)))) return r;
    InsertArgs ia;
    round_insert_args(e, rc, ia);
    HIPCHK(e, hipMemsetAsync(e->d_count, 0, 8, e->stream));
    hipLaunchKernelGGL(k_xl_export, dim3((unsigned)((rc.n + 255) / 256)), dim3(256), 0, e->stream, ia, rc.world,
                       (KeyRec*)e->d_scratch[SC_XL], rc.n_xl, e->d_count);
    std::vector<KeyRec> xl(rc.n_xl);
    unsigned long long exported = 0;
    HIPCHK(e, hipMemcpyAsync(xl.data(), e->d_scratch[SC_XL], rc.n_xl * sizeof(KeyRec), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(&exported, e->d_count, 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (exported != rc.n_xl)  // the list would carry uninitialised records: never send those
      return fail(e, CTMR_E_HIP, "ctmr_xchg_keys_device: %llu long-serial key records collected, %llu counted by the map",
                  exported, (unsigned long long)rc.n_xl);
    std::sort(xl.begin(), xl.end(), [](const KeyRec& a, const KeyRec& b) {
      return a.owner != b.owner ? a.owner < b.owner : (uint32_t)a.pad < (uint32_t)b.pad;
    });
    for (auto& k : xl) counts64[k.owner]++;
    rc.xl = std::move(xl);  // kept alive until the copy below has run
    HIPCHK(e, hipMemcpyAsync(d_keys64_out, rc.xl.data(), rc.n_xl * sizeof(KeyRec), hipMemcpyHostToDevice, e->stream));
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  return CTMR_OK;
}

extern "C++" {
namespace {
template <class Rec>
static void xchg_owner_pass1(ctmr_engine* e, const Rec* keys, uint64_t n, uint64_t round_ref0, uint64_t recv_ref0, uint32_t* d_slot) {
  if (!n) return;
  hipLaunchKernelGGL((k_keys_insert<Rec>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, keys, n, e->tbl(),
                     (unsigned long long)round_ref0, (unsigned long long)recv_ref0, d_slot);
}
template <class Rec>
static void xchg_owner_pass2(ctmr_engine* e, const Rec* keys, uint64_t n, const InsertArgs& loc, uint64_t recv_ref0,
                             ctmr_record* rec_local, uint32_t* d_slot) {
  if (!n) return;
  hipLaunchKernelGGL((k_keys_insert2<Rec>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, keys, n, loc,
                     (unsigned long long)recv_ref0, rec_local, d_slot);
}
template <class Rec>
static void xchg_owner_resolve(ctmr_engine* e, const Rec* keys, uint64_t n, uint64_t recv_ref0, const uint32_t* d_slot,
                               uint8_t* d_flags, DevStats* d_st) {
  if (!n) return;
  const uint64_t nb = (n + 1023) / 1024;
  hipLaunchKernelGGL((k_keys_resolve<Rec>), dim3((unsigned)(nb < 512 ? nb : 512)), dim3(1024), 0, e->stream, keys, n, nb,
                     e->tbl(), (unsigned long long)recv_ref0, d_slot, d_flags, e->issuer_counts, d_st);
}

// The owner's insert of n32 32-byte and n64 64-byte key records whose cells start at recv_ref0 (the 64-byte records'
// behind the 32-byte ones): pass 1, pass 2 and the resolve, each over both arrays.  round_ref0: the first cell of the
// round a word of which pass 2 settles by order (an owner-computes round: the shard's entry 0; outside a round: recv_ref0).
// d_slot: n32 + n64 words; a "was unknown" byte per record goes to d_flags32 / d_flags64, the counts to d_st.
static void xchg_owner_insert(ctmr_engine* e, const KeyRec32* k32, uint64_t n32, const KeyRec* k64, uint64_t n64,
                              const InsertArgs& loc, uint64_t round_ref0, uint64_t recv_ref0, ctmr_record* rec_local,
                              uint32_t* d_slot, uint8_t* d_flags32, uint8_t* d_flags64, DevStats* d_st) {
  xchg_owner_pass1(e, k32, n32, round_ref0, recv_ref0, d_slot);
  xchg_owner_pass1(e, k64, n64, round_ref0, recv_ref0 + n32, d_slot + n32);
  xchg_owner_pass2(e, k32, n32, loc, recv_ref0, rec_local, d_slot);
  xchg_owner_pass2(e, k64, n64, loc, recv_ref0 + n32, rec_local, d_slot + n32);
  xchg_owner_resolve(e, k32, n32, recv_ref0, d_slot, d_flags32, d_st);
  xchg_owner_resolve(e, k64, n64, recv_ref0 + n32, d_slot + n32, d_flags64, d_st);
}
}  // namespace
}  // extern "C++"

int ctmr_xchg_insert_device(ctmr_engine* e, const void* d_keys32, uint64_t n32, const void* d_keys64, uint64_t n64,
                            uint8_t* d_flags32, uint8_t* d_flags64) {
  if (!e || (n32 && (!d_keys32 || !d_flags32)) || (n64 && (!d_keys64 || !d_flags64))) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  int r;
  if ((r = xchg_round_check(e, "ctmr_xchg_insert_device"))) return r;
  RoundCtx& rc = e->rd;
  if (rc.resolved) return fail(e, CTMR_E_INVAL, "ctmr_xchg_insert_device: already called for this round");
  const uint64_t N = n32 + n64;
  if (N >= 0xfffffff0ull) return fail(e, CTMR_E_INVAL, "too many keys");
  if (N) {
    // (this shard's own DEFER entries were settled in round_begin: a rebuild of the table may move slots now.)
    // `occupied` does not hold this round's own claims yet (round_collect adds them, behind this insert): reserve for both —
    // up to rc.n slots the shard's own entries may have claimed in round_begin, and N for the keys that arrive now.  Checking
    // N alone let occ + own + N pass the 3/4 bound on unbalanced shards (a small own shard, many received keys, a table at
    // its cap) and fail mid-round with CTMR_E_FULL (advisor, round 3).
    const unsigned long long rebuilds_before = e->rebuilds;
    if ((r = ensure_capacity(e, rc.n + N, false, N))) return r;  // (cells: only the received keys' — the shard's own are inside arena_used)
    if (e->rebuilds != rebuilds_before) rc.own_counted = true;  // the rebuild counted the live slots: own claims included
    if ((r = ensure(e, SC_XSLOT, N * 4))) return r;
    e->pairs_dirty = true;
  }
  uint32_t* d_slot = (uint32_t*)e->d_scratch[SC_XSLOT];
  // the received keys' cells: behind everything handed out so far (this shard's own cells included)
  rc.recv_ref0 = e->arena_used;
  e->arena_used += N;
  InsertArgs loc;
  round_insert_args(e, rc, loc);  // after ensure_capacity: index and arena may be new ones
  xchg_owner_insert(e, (const KeyRec32*)d_keys32, n32, (const KeyRec*)d_keys64, n64, loc, rc.ref0, rc.recv_ref0,
                    rc.d_records, d_slot, d_flags32, d_flags64, e->d_stats + 1);
  if (rc.n) {
    if ((r = round_resolve(e, rc, false))) return r;
    if ((r = round_collect(e, rc))) return r;
  } else {
    DevStats both[2];
    HIPCHK(e, hipMemcpyAsync(both, e->d_stats, sizeof both, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipGetLastError());
    rc.remote_new = both[1].n_new;
    e->occupied += rc.remote_new;
    if (both[1].n_full) return fail(e, CTMR_E_FULL, "known-certificate table full (%llu slots)", (unsigned long long)e->nslots);
  }
  rc.resolved = true;
  return CTMR_OK;
}

int ctmr_xchg_apply_device(ctmr_engine* e, const void* d_sent32, const uint8_t* d_flags32, uint64_t n32,
                           const void* d_sent64, const uint8_t* d_flags64, uint64_t n64, ctmr_batch_stats* stats) {
  if (!e || (n32 && (!d_sent32 || !d_flags32)) || (n64 && (!d_sent64 || !d_flags64))) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (stats) memset(stats, 0, sizeof *stats);
  int r;
  if ((r = xchg_round_check(e, "ctmr_xchg_apply_device"))) return r;
  RoundCtx& rc = e->rd;
  if (!rc.resolved) return fail(e, CTMR_E_INVAL, "ctmr_xchg_apply_device: ctmr_xchg_insert_device has not run for this round");
  if (rc.n == 0) return CTMR_OK;
  InsertArgs loc;
  round_insert_args(e, rc, loc);
  uint32_t* d_blk_new = (uint32_t*)e->d_scratch[SC_BLKNEW];
  HIPCHK(e, hipMemsetAsync(e->d_count, 0, 8, e->stream));
  if (n32)
    hipLaunchKernelGGL((k_apply_lost<KeyRec32>), dim3((unsigned)((n32 + 1023) / 1024)), dim3(256), 0, e->stream,
                       (const KeyRec32*)d_sent32, d_flags32, n32, loc, rc.d_records, d_blk_new, e->d_count);
  if (n64)
    hipLaunchKernelGGL((k_apply_lost<KeyRec>), dim3((unsigned)((n64 + 1023) / 1024)), dim3(256), 0, e->stream,
                       (const KeyRec*)d_sent64, d_flags64, n64, loc, rc.d_records, d_blk_new, e->d_count);
  if (rc.d_new_idx) {
    round_compact(e, rc);
    rc.compacted = true;
  }
  unsigned long long lost = 0;
  HIPCHK(e, hipMemcpyAsync(&lost, e->d_count, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  rc.lost = lost;
  round_stats(e, rc, stats);
  return CTMR_OK;
}

// ------------------------------------------------------------------ cross-GPU dedup, Bloom pre-filter variant

int ctmr_bloom_config(ctmr_engine* e, uint64_t bits, void* d_words) {
  if (!e) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (bits < 4096 || bits > (1ull << 40) || (bits & (bits - 1)))
    return fail(e, CTMR_E_INVAL, "Bloom filter size must be a power of two in [2^12, 2^40] bits");
  if ((uintptr_t)d_words & 7) return fail(e, CTMR_E_INVAL, "Bloom filter buffer must be 8-byte aligned");
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (e->d_bloom && e->bloom_owned) (void)hipFree(e->d_bloom);
  e->d_bloom = nullptr;
  e->bloom_words = 0;
  if (d_words) {
    e->d_bloom = (unsigned long long*)d_words;
    e->bloom_owned = false;
  } else {
    if (hipMalloc(&e->d_bloom, bits / 8) != hipSuccess) {
      (void)hipGetLastError();
      e->d_bloom = nullptr;
      return fail(e, CTMR_E_NOMEM, "Bloom filter: %llu bytes", (unsigned long long)(bits / 8));
    }
    e->bloom_owned = true;
  }
  e->bloom_words = bits / 64;
  e->bloom_round_ref0 = ~0ull;
  HIPCHK(e, hipMemsetAsync(e->d_bloom, 0, bits / 8, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return CTMR_OK;
}

int ctmr_bloom_device(ctmr_engine* e, void** d_words, uint64_t* n_words) {
  if (!e || !d_words) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  if (!e->d_bloom) return fail(e, CTMR_E_INVAL, "ctmr_bloom_config has not been called");
  *d_words = e->d_bloom;
  if (n_words) *n_words = e->bloom_words;
  return CTMR_OK;
}

static void bloom_args(ctmr_engine* e, InsertArgs& ia, const uint8_t* d_payload, const uint64_t* d_offsets,
                       const uint64_t* d_ends, uint64_t n, const ctmr_record* d_records) {
  ia.records = d_records; ia.payload = d_payload; ia.offsets = d_offsets; ia.ends = d_ends; ia.canon = e->d_canon;
  ia.t = e->tbl(); ia.ref0 = e->rd.valid ? e->rd.ref0 : e->arena_used; ia.slot_id = nullptr; ia.ent = nullptr; ia.n = n;
}

int ctmr_bloom_add_device(ctmr_engine* e, const uint8_t* d_payload, const uint64_t* d_offsets, const uint64_t* d_ends,
                          uint64_t n, const ctmr_record* d_records) {
  if (!e || (n && (!d_payload || !d_offsets))) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (!e->d_bloom) return fail(e, CTMR_E_INVAL, "ctmr_bloom_config has not been called");
  // "this round" for the peers' lookups = the cells of the batch this engine mapped last
  e->bloom_round_ref0 = (n && e->rd.valid) ? e->rd.ref0 : ~0ull;
  if (n == 0) return CTMR_OK;
  if (!d_records) d_records = (const ctmr_record*)e->d_scratch[SC_RECORDS];
  if (!d_records) return fail(e, CTMR_E_INVAL, "no records: run ctmr_map_*_device on this batch first");
  // Round 3: an engine with a filter adds to it INSIDE the map kernel (k_map_fused<…, XM_BLOOM>: the walking lane has
  // the key's hash in registers) — for the batch the engine mapped last there is nothing left to do here.
  if (e->rd.valid && e->rd.mode == XM_BLOOM && e->rd.d_records == d_records && e->rd.n == n) return CTMR_OK;
  InsertArgs ia;
  bloom_args(e, ia, d_payload, d_offsets, d_ends, n, d_records);
  hipLaunchKernelGGL(k_bloom_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, ia, e->d_bloom,
                     e->bloom_words - 1);
  HIPCHK(e, hipStreamSynchronize(e->stream));  // the caller all-gathers the filter on its own stream next
  HIPCHK(e, hipGetLastError());
  return CTMR_OK;
}

int ctmr_bloom_probe_device(ctmr_engine* e, const uint8_t* d_payload, const uint64_t* d_offsets,
                            const uint64_t* d_ends, uint64_t n, const ctmr_record* d_records, const void* d_filters,
                            uint32_t world, uint32_t rank, uint64_t order_base, void* d_keys_out, uint64_t keys_cap,
                            uint64_t* counts) {
  if (!e || !counts || !d_filters || world == 0 || world > MAX_WORLD || rank >= world ||
      (n && (!d_payload || !d_offsets)) || (keys_cap && !d_keys_out))
    return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (!e->d_bloom) return fail(e, CTMR_E_INVAL, "ctmr_bloom_config has not been called");
  for (uint32_t w = 0; w < world; w++) counts[w] = 0;
  if (n == 0) return CTMR_OK;
  if (!d_records) d_records = (const ctmr_record*)e->d_scratch[SC_RECORDS];
  if (!d_records) return fail(e, CTMR_E_INVAL, "no records: run ctmr_map_*_device on this batch first");
  const uint64_t nb = (n + 1023) / 1024;
  const uint64_t ncnt = (uint64_t)world * nb;
  int r;
  // (scratch of its own: the NEW counts per block and ent[] of the map call must survive until ctmr_bloom_apply_device)
  if ((r = ensure(e, SC_XSLOT, n * 4))) return r;               // hit mask u16 per entry
  if ((r = ensure(e, SC_XCNT, (ncnt + 1) * 4))) return r;
  if ((r = ensure(e, SC_XBASE, (ncnt + 1) * 8))) return r;
  uint16_t* d_hit = (uint16_t*)e->d_scratch[SC_XSLOT];
  uint32_t* d_cnt = (uint32_t*)e->d_scratch[SC_XCNT];
  uint64_t* d_base = (uint64_t*)e->d_scratch[SC_XBASE];
  // the gathered filters, word-major: one sector per key instead of one per peer (k_filter_interleave)
  if ((r = ensure(e, SC_XSTAGE, (size_t)world * e->bloom_words * 8))) return r;
  unsigned long long* d_inter = (unsigned long long*)e->d_scratch[SC_XSTAGE];
  hipLaunchKernelGGL(k_filter_interleave, dim3((unsigned)((e->bloom_words + 255) / 256)), dim3(256), 0, e->stream,
                     (const unsigned long long*)d_filters, e->bloom_words, world, d_inter);
  InsertArgs ia;
  bloom_args(e, ia, d_payload, d_offsets, d_ends, n, d_records);
  HIPCHK(e, hipMemsetAsync(d_cnt, 0, (ncnt + 1) * 4, e->stream));
  hipLaunchKernelGGL(k_bloom_probe, dim3((unsigned)nb), dim3(1024), 0, e->stream, ia,
                     (const unsigned long long*)d_inter, e->bloom_words, world, rank, nb, d_hit, d_cnt);
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, e->stream, d_cnt, ncnt + 1, d_base);
  std::vector<uint64_t> base(world + 1);
  for (uint32_t w = 0; w <= world; w++)
    HIPCHK(e, hipMemcpyAsync(&base[w], d_base + (uint64_t)w * nb, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  for (uint32_t w = 0; w < world; w++) counts[w] = base[w + 1] - base[w];
  if (base[world] > keys_cap)
    return fail(e, CTMR_E_RANGE, "key buffer too small: %llu records needed", (unsigned long long)base[world]);
  if (base[world] == 0) return CTMR_OK;
  hipLaunchKernelGGL(k_bloom_scatter, dim3((unsigned)nb), dim3(1024), 0, e->stream, ia, world, nb,
                     (const uint16_t*)d_hit, (const uint64_t*)d_base, (unsigned long long)order_base,
                     (KeyRec*)d_keys_out);
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  return CTMR_OK;
}

int ctmr_bloom_lookup_device(ctmr_engine* e, const void* d_keys, uint64_t n_keys, uint64_t order_base,
                             uint8_t* d_flags) {
  if (!e || (n_keys && (!d_keys || !d_flags))) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (n_keys == 0) return CTMR_OK;
  hipLaunchKernelGGL(k_keys_lookup, dim3((unsigned)((n_keys + 255) / 256)), dim3(256), 0, e->stream,
                     (const KeyRec*)d_keys, n_keys, e->tbl(), (unsigned long long)e->bloom_round_ref0,
                     (unsigned long long)order_base, d_flags);
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  return CTMR_OK;
}

int ctmr_bloom_apply_device(ctmr_engine* e, ctmr_record* d_records, uint64_t n, const void* d_keys_sent,
                            const uint8_t* d_flags, uint64_t n_keys, uint64_t* d_new_idx, ctmr_batch_stats* stats) {
  if (!e || (n_keys && (!d_keys_sent || !d_flags))) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (stats) memset(stats, 0, sizeof *stats);
  if (n == 0) return CTMR_OK;
  if (!d_records) d_records = (ctmr_record*)e->d_scratch[SC_RECORDS];
  // the round continues the engine's last map call: its ent[] / NEW counts per block are still in the scratch buffers,
  // so only the few entries that lose WasUnknown are touched and the NEW list is compacted once, from 4 bytes per entry
  RoundCtx& rc = e->rd;
  if (!rc.valid || rc.d_records != d_records || rc.n != n)
    return fail(e, CTMR_E_INVAL, "ctmr_bloom_apply_device: these are not the records of this engine's last ctmr_map_*_device call");
  HIPCHK(e, hipMemsetAsync(e->d_count, 0, 8, e->stream));
  if (n_keys) {
    e->pairs_dirty = true;
    hipLaunchKernelGGL(k_bloom_apply, dim3((unsigned)((n_keys + 255) / 256)), dim3(256), 0, e->stream,
                       (const KeyRec*)d_keys_sent, d_flags, n_keys, d_records, (uint32_t*)e->d_scratch[SC_ENT],
                       (uint32_t*)e->d_scratch[SC_BLKNEW], e->tbl(), e->issuer_counts, e->d_count);
  }
  if (d_new_idx) {
    rc.d_new_idx = d_new_idx;
    round_compact(e, rc);
    rc.compacted = true;
  }
  unsigned long long lost = 0;
  HIPCHK(e, hipMemcpyAsync(&lost, e->d_count, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  rc.lost += lost;
  round_stats(e, rc, stats);
  return CTMR_OK;
}
