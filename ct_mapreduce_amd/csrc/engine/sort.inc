// engine/sort.inc — the order inside a known-certificate set (include/ctmr.h ctmr_known_sort* / ctmr_set_known_order,
// DESIGN.md §15): member records sorted in place on the device, set by set, by the kernels of kernels/sort.h.  The same
// sort serves an image a caller holds and, under CTMR_KNOWN_ORDER_SORTED, every run of records known_export_members
// (engine/image.inc) stages for an export or for the per-issuer lists.
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after engine/lists.inc.

extern "C++" {
namespace {

constexpr uint64_t SORT_CHUNK = 1ull << 27;  // records per run (32-bit perm and group, bounded working memory)

uint64_t known_sort_chunk() { return known_chunk("CTMR_KNOWN_SORT_CHUNK", SORT_CHUNK); }

uint32_t bits_of(uint64_t v) {  // bits needed for the values 0..v
  uint32_t b = 0;
  while (v) { b++; v >>= 1; }
  return b;
}

// The working memory of a run of at most n records, in one allocation: two key buffers (16 B per record), the records
// aside (48 B), the digit counts of a pass (256 per SORT_TILE keys), the tie-group heads per 256 keys and the tied count.
struct SortWork {
  DevMem mem;
  uint4 *a = nullptr, *b = nullptr;
  uint8_t* aside = nullptr;
  unsigned long long *hist = nullptr, *cnt = nullptr, *tied = nullptr;
  int alloc(uint64_t n) {
    const uint64_t nb = (n + SORT_TILE - 1) / SORT_TILE, nb2 = (n + 255) / 256;
    const size_t keys = (n * 16 + 63) & ~(size_t)63, recs = (n * KNOWN_REC_BYTES + 63) & ~(size_t)63;
    const size_t hist_b = nb * 256 * 8, cnt_b = ((nb2 + 1) * 8 + 63) & ~(size_t)63;
    if (mem.alloc(2 * keys + recs + hist_b + cnt_b + 64) != hipSuccess) return CTMR_E_NOMEM;
    a = (uint4*)mem.u8();
    b = (uint4*)(mem.u8() + keys);
    aside = mem.u8() + 2 * keys;
    hist = (unsigned long long*)(aside + recs);
    cnt = (unsigned long long*)(aside + recs + hist_b);
    tied = (unsigned long long*)(aside + recs + hist_b + cnt_b);
    return CTMR_OK;
  }
};

struct SortInfo { uint64_t records = 0, runs = 0; uint32_t rounds = 0, passes = 0; };

// One run of d_rec's records: its sets are those of first[] (host) / d_first[] (device), both in records of d_rec.
int known_sort_run(ctmr_engine* e, uint8_t* d_rec, const KnownRun& run, const std::vector<uint64_t>& first,
                   const uint64_t* d_first, SortWork& w, SortInfo* si) {
  const size_t s0 = run.s_lo, s1 = run.s_hi;
  const uint64_t lo = run.lo, n = run.n;
  uint64_t tied = 0;  // records that share their set with another
  for (size_t s = s0; s < s1; s++)
    if (first[s + 1] - first[s] > 1) tied += first[s + 1] - first[s];
  si->runs++;
  if (!tied) return CTMR_OK;
  const uint64_t nb = (n + SORT_TILE - 1) / SORT_TILE, nb2 = run.blocks();
  int r;
  hipLaunchKernelGGL(k_sort_keys, dim3((unsigned)nb2), dim3(256), 0, e->stream, (const uint8_t*)d_rec, lo, n,
                     d_first + s0, (uint32_t)(s1 - s0), w.a);
  uint4 *cur = w.a, *alt = w.b;
  uint32_t gbits = bits_of(s1 - s0 - 1), rounds = 0;
  while (tied && rounds < SORT_ROUNDS) {
    // the digits that can differ, least significant first: the word's (serial_len: one), then the group's
    std::vector<uint32_t> digits;
    for (uint32_t d = 0; d < (rounds + 1 < SORT_ROUNDS ? 8u : 1u); d++) digits.push_back(d);
    for (uint32_t d = 0; d < (gbits + 7) / 8; d++) digits.push_back(8 + d);
    for (uint32_t d : digits) {
      hipLaunchKernelGGL(k_sort_hist, dim3((unsigned)nb), dim3(SORT_THREADS), 0, e->stream, (const uint4*)cur, n, d, w.hist, nb);
      if ((r = scan_u64(e, (uint64_t*)w.hist, 256 * nb, false, SC_TMP))) return r;
      hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)nb), dim3(SORT_THREADS), 0, e->stream, (const uint4*)cur, alt, n, d,
                         (const unsigned long long*)w.hist, nb);
      std::swap(cur, alt);
      si->passes++;
    }
    if (++rounds == SORT_ROUNDS) break;  // serial_len was the last thing two records could differ in
    HIPCHK(e, hipMemsetAsync(w.cnt + nb2, 0, 8, e->stream));
    HIPCHK(e, hipMemsetAsync(w.tied, 0, 8, e->stream));
    hipLaunchKernelGGL(k_sort_heads, dim3((unsigned)nb2), dim3(256), 0, e->stream, (const uint4*)cur, n, w.cnt, w.tied);
    if ((r = scan_u64(e, (uint64_t*)w.cnt, nb2 + 1, false, SC_TMP))) return r;
    unsigned long long heads = 0, t = 0;
    HIPCHK(e, hipMemcpyAsync(&heads, w.cnt + nb2, 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(&t, w.tied, 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipGetLastError());
    tied = t;
    if (!tied) break;
    hipLaunchKernelGGL(k_sort_regroup, dim3((unsigned)nb2), dim3(256), 0, e->stream, (const uint4*)cur, alt, n,
                       (const unsigned long long*)w.cnt, (const uint8_t*)d_rec, lo, rounds);
    std::swap(cur, alt);
    gbits = bits_of(heads - 1);
  }
  si->rounds = std::max(si->rounds, rounds);
  // the permuted records aside, complete, and only then over the run
  hipLaunchKernelGGL(k_sort_gather, dim3((unsigned)nb2), dim3(256), 0, e->stream, (const uint8_t*)d_rec, lo, (const uint4*)cur, n, w.aside);
  HIPCHK(e, hipMemcpyAsync(d_rec + lo * KNOWN_REC_BYTES, w.aside, n * KNOWN_REC_BYTES, hipMemcpyDeviceToDevice, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  return CTMR_OK;
}

// Sets of valid member records at d_rec, set s = records [first[s], first[s + 1]) (first[0] = 0): each sorted in place,
// in runs of whole sets of at most known_sort_chunk() records (a larger set alone).  Every buffer the call needs is
// allocated before the first record moves: CTMR_E_NOMEM leaves the records as they were.  Drains the stream.
int known_sort_sets(ctmr_engine* e, uint8_t* d_rec, const std::vector<uint64_t>& first) {
  const size_t ns = first.size() - 1;
  const uint64_t N = first[ns];
  SortInfo si;
  si.records = N;
  if (N > 1) {
    KnownExport x;  // (known_cut_sets reads the set ranges alone)
    for (size_t s = 0; s < ns; s++) x.set_range.push_back({first[s], first[s + 1] - first[s]});
    x.info.members = N;
    const std::vector<KnownRun> runs = known_cut_sets(x, known_sort_chunk());
    uint64_t max_n = 0;
    for (const KnownRun& run : runs) max_n = std::max(max_n, run.n);
    if (max_n > 0xffffffffull) return fail(e, CTMR_E_NOMEM, "known sort: a set of %llu members", (unsigned long long)max_n);
    SortWork w;
    DevMem d_first;
    int r;
    if (w.alloc(max_n) || d_first.alloc((ns + 1) * 8) != hipSuccess)
      return fail(e, CTMR_E_NOMEM, "known sort: no device memory for the working buffers of %llu member records", (unsigned long long)max_n);
    if ((r = ensure(e, SC_TMP, ((256 * ((max_n + SORT_TILE - 1) / SORT_TILE) + SCAN_TILE - 1) / SCAN_TILE) * 8))) return r;
    HIPCHK(e, hipMemcpyAsync(d_first.p, first.data(), (ns + 1) * 8, hipMemcpyHostToDevice, e->stream));
    for (const KnownRun& run : runs)
      if ((r = known_sort_run(e, d_rec, run, first, (const uint64_t*)d_first.p, w, &si))) return r;
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (env_u64("CTMR_KNOWN_SORT_INFO"))  // tests and scripts/bench_known_sort.py read the round count here
    fprintf(stderr, "ctmr known sort: records=%llu runs=%llu rounds=%u passes=%u\n", (unsigned long long)si.records,
            (unsigned long long)si.runs, si.rounds, si.passes);
  return CTMR_OK;
}

// What ctmr_known_sort and ctmr_known_sort_device share behind the meta checks: every record validated on the device,
// then the sort.
int known_sort_core(ctmr_engine* e, const KnownMeta& km, uint8_t* d_members) {
  int r;
  if ((r = known_bind(e, km, d_members, "known sort"))) return r;
  if ((r = known_validate_records(e, km, d_members, known_sort_chunk(), "known sort"))) return r;
  return known_sort_sets(e, d_members, km.set_first);
}

}  // namespace
}  // extern "C++"

int ctmr_set_known_order(ctmr_engine* e, int order) {
  if (!e) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  if (order != CTMR_KNOWN_ORDER_ANY && order != CTMR_KNOWN_ORDER_SORTED)
    return fail(e, CTMR_E_INVAL, "known order %d: CTMR_KNOWN_ORDER_ANY or CTMR_KNOWN_ORDER_SORTED", order);
  e->known_order = order;
  return CTMR_OK;
}

int ctmr_known_sort_device(ctmr_engine* e, const uint8_t* meta, size_t meta_len, void* d_members, uint64_t n_members) {
  if (!e || !meta) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  KnownMeta km;
  int r;
  if ((r = known_open(e, meta, meta_len, &n_members, "known sort", &km))) return r;
  return known_sort_core(e, km, (uint8_t*)d_members);
}

int ctmr_known_sort(ctmr_engine* e, uint8_t* image, size_t len) {
  if (!e || !image) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  KnownMeta km;
  DevMem d;
  int r;
  if ((r = known_open(e, image, len, nullptr, "known sort", &km))) return r;
  if ((r = known_stage_members(e, km, image, 0, "known sort", &d))) return r;
  if ((r = known_sort_core(e, km, d.u8()))) return r;
  if (km.n_members) HIPCHK(e, hipMemcpy(image + km.meta_bytes, d.p, km.n_members * KNOWN_REC_BYTES, hipMemcpyDeviceToHost));
  return CTMR_OK;
}
