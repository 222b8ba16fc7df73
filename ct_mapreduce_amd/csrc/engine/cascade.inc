// engine/cascade.inc — the CRLite filter cascade of a revoked / not-revoked image pair (include/ctmr.h ctmr_cascade_*,
// DESIGN.md §29).  Host side: both metas opened, each side's kept sets chosen by the rule of ctmr_known_image_lists
// (engine/lists.inc: lists_hour_kept, lists_parse_date) and laid out as the segments of a virtual record sequence
// (kernels/find.h: FindSegs; engine/image.inc: KnownPack), then layer by layer: the bits of the records the layer holds, the flags of the
// records it is tested with, one scan of the block counts and one count read by the host, the survivors compacted into
// the list the next layers read (kernels/cascade.h).  The query validates a cascade and walks it for a probe image.
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after engine/split.inc.

extern "C++" {
namespace {

constexpr char CASC_MAGIC[8] = {'C', 'T', 'M', 'R', 'C', 'A', 'S', 'C'};
constexpr uint32_t CASC_VERSION = 1, CASC_HASH_SHA256_32 = 2, CASC_HEADER = 64, CASC_LAYER_BYTES = 32;
constexpr uint64_t CASC_CHUNK = 1ull << 27;  // records per launch

uint64_t casc_chunk() { return known_chunk("CTMR_CASCADE_CHUNK", CASC_CHUNK); }

// One operand before anything is launched: its kept sets in image order as segments, its kept host pairs counted.
struct CascSide {
  const KnownMeta* m = nullptr;
  const uint8_t* d = nullptr;
  KnownExport x;  // the kept sets as (first virtual record, count): what known_cut_sets cuts into runs
  std::vector<uint64_t> dst, src;
  std::vector<uint32_t> ord;
  uint64_t kept = 0, host_skipped = 0;
  size_t o_dst = 0, o_src = 0, o_ord = 0, o_dig = 0;  // where its tables lie in the call's upload
};

int casc_side(ctmr_engine* e, const KnownMeta& k, const uint8_t* d, int64_t now, const char* what, CascSide* s) {
  s->m = &k;
  s->d = d;
  if (k.n_members >= (1ull << 32)) return fail(e, CTMR_E_INVAL, "%s: %llu member records, at most 2^32 - 1", what, (unsigned long long)k.n_members);
  for (uint64_t i = 0; i < k.n_sets; i++) {
    if (!lists_hour_kept(k.set_hour[i], now)) continue;
    const uint64_t cnt = k.set_first[i + 1] - k.set_first[i];
    s->x.set_range.push_back({s->kept, cnt});
    s->dst.push_back(s->kept);
    s->src.push_back(k.set_first[i]);
    s->ord.push_back(k.set_issuer[i]);
    s->kept += cnt;
  }
  s->dst.push_back(s->kept);
  s->x.info.members = s->kept;
  return known_kept_host_pairs(e, k, now, what, [&](size_t, bool, const std::string&, int64_t) { s->host_skipped++; });
}

void casc_pack_side(KnownPack* pk, CascSide* s) {
  s->o_dst = pk->put(s->dst);
  s->o_src = pk->put(s->src);
  s->o_ord = pk->put(s->ord);
  s->o_dig = pk->put(s->m->issuers, (size_t)s->m->n_issuers * 32);
}

// the kept sets [lo, hi) of a side as one run
CascSrc casc_run(const CascSide& s, const uint8_t* t8, size_t lo, size_t hi) {
  return CascSrc{FindSegs{{s.d, (const uint64_t*)(t8 + s.o_dst) + lo, (const uint64_t*)(t8 + s.o_src) + lo, (uint32_t)(hi - lo)},
                          nullptr, (const uint32_t*)(t8 + s.o_ord) + lo},
                 nullptr, (const uint32_t*)(t8 + s.o_dig)};
}

// A sequence of records a layer holds or is tested with: all kept records of a side where they lie, or a survivor list.
struct CascSeq {
  const CascSide* side = nullptr;
  const uint2* list = nullptr;  // null: the side's kept sets
  uint64_t n = 0;
};

// The runs of a sequence: a side's kept sets as known_cut_sets cuts them, or — the cascade's own — a survivor list cut
// into runs of `chunk` records, not into whole sets (lo: the run's first entry of the list; no sets).
std::vector<KnownRun> casc_runs(const CascSeq& q, uint64_t chunk) {
  if (!q.list) return q.n ? known_cut_sets(q.side->x, chunk) : std::vector<KnownRun>();
  std::vector<KnownRun> runs;
  for (uint64_t at = 0; at < q.n; at += chunk) {
    const uint64_t n = std::min(chunk, q.n - at);
    runs.push_back(KnownRun{0, 0, at, n, known_runs_blocks(runs)});
  }
  return runs;
}

// where the records of a run of the sequence lie
CascSrc casc_src(const CascSeq& q, const uint8_t* t8, const KnownRun& run) {
  CascSrc c = casc_run(*q.side, t8, run.s_lo, run.s_hi);
  if (q.list) c.list = q.list + run.lo;
  return c;
}

CascHash casc_prefix(const uint8_t* salt, uint32_t salt_len) {
  CascHash hp{};
  uint8_t b[24] = {0};
  memcpy(b, salt, salt_len);
  memcpy(hp.pre, b, 24);
  hp.salt_len = salt_len;
  return hp;
}

int casc_params_check(ctmr_engine* e, const ctmr_cascade_params& p) {
  auto k_ok = [](uint32_t k) { return k >= 1 && k <= 32; };
  auto b_ok = [](uint32_t b) { return b >= 1 && b <= 65536; };
  if (!k_ok(p.k_first) || !k_ok(p.k_rest) || !b_ok(p.bpk_first_q8) || !b_ok(p.bpk_rest_q8) || p.max_layers < 1 ||
      p.max_layers > CTMR_CASCADE_MAX_LAYERS || p.salt_len > 16)
    return fail(e, CTMR_E_INVAL, "cascade build: k in 1..32, bpk_q8 in 1..65536, max_layers in 1..255, salt_len in 0..16");
  return CTMR_OK;
}

// Both metas are parsed and the member records of both operands are on the device.  out: host memory (host = true) or
// device memory.
int cascade_core(ctmr_engine* e, const KnownMeta& rm, const uint8_t* d_r, const KnownMeta& sm, const uint8_t* d_s, int64_t now,
                 const ctmr_cascade_params& p, uint8_t* out, size_t out_cap, bool host, ctmr_cascade_info* info) {
  const char* what = "cascade build";
  int r;
  memset(info, 0, sizeof *info);
  if ((r = casc_params_check(e, p))) return r;
  if ((r = known_bind(e, rm, d_r, what)) || (r = known_bind(e, sm, d_s, what))) return r;
  if ((r = known_aligned16(e, (uintptr_t)d_r | (uintptr_t)d_s | (host ? 0 : (uintptr_t)out), what))) return r;
  CascSide R, S;
  if ((r = casc_side(e, rm, d_r, now, "cascade build (R)", &R)) || (r = casc_side(e, sm, d_s, now, "cascade build (S)", &S))) return r;
  info->r_records = R.kept;
  info->s_records = S.kept;
  info->r_sets_kept = R.x.set_range.size();
  info->s_sets_kept = S.x.set_range.size();
  info->r_host_skipped = R.host_skipped;
  info->s_host_skipped = S.host_skipped;
  // ---- the tables of both sides in one upload, the error word behind them
  KnownPack pk;
  casc_pack_side(&pk, &R);
  casc_pack_side(&pk, &S);
  const size_t o_err = pk.put_err();
  DevMem tabs;
  if (tabs.alloc(pk.b.size()) != hipSuccess) return fail(e, CTMR_E_NOMEM, "%s: no device memory for the tables", what);
  HIPCHK(e, hipMemcpyAsync(tabs.p, pk.b.data(), pk.b.size(), hipMemcpyHostToDevice, e->stream));
  const uint8_t* t8 = tabs.u8();
  uint32_t* d_err = (uint32_t*)(t8 + o_err);
  const CascHash hp = casc_prefix(p.salt, p.salt_len);
  const uint64_t chunk = casc_chunk();
  // ---- layer by layer
  std::vector<std::unique_ptr<DevMem>> bits, lists;
  CascSeq hold{&R, nullptr, R.kept}, test{&S, nullptr, S.kept};
  uint32_t err = 0;
  // The flags of every test pass, allocated once for the pass with the most blocks: a side where it lies, or all of
  // it as a list (a list is cut into runs of `chunk` records, whole sets are not: either can have more blocks).  No
  // buffer is released before the end of the call: a release would wait for the device in front of every layer.
  uint64_t NB_max = 0;
  for (const CascSide* side : {&R, &S}) {
    NB_max = std::max(NB_max, known_runs_blocks(casc_runs(CascSeq{side, nullptr, side->kept}, chunk)));
    NB_max = std::max(NB_max, known_runs_blocks(casc_runs(CascSeq{side, (const uint2*)t8, side->kept}, chunk)));
  }
  DevMem flags;
  if (NB_max && flags.alloc((NB_max + 1) * 8 + NB_max * 32) != hipSuccess)
    return fail(e, CTMR_E_NOMEM, "%s: no device memory for the flags of %llu blocks", what, (unsigned long long)NB_max);
  const KnownFlags fl{(unsigned long long*)(flags.u8() + (NB_max + 1) * 8), (unsigned long long*)flags.p};
  // a test pass over `q`, its scan, and the one count the host reads: how many records passed
  auto tested = [&](const CascSeq& q, const CascLayer& ly, uint64_t* passed) -> int {
    const std::vector<KnownRun> runs = casc_runs(q, chunk);
    const uint64_t NB = known_runs_blocks(runs);
    HIPCHK(e, hipMemsetAsync(flags.p, 0, (NB + 1) * 8, e->stream));
    for (const KnownRun& run : runs)
      hipLaunchKernelGGL(k_casc_test, dim3((unsigned)run.blocks()), dim3(256), 0, e->stream, casc_src(q, t8, run), run.n, hp, ly, fl,
                         run.blk0, d_err);
    HIPCHK(e, hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, e->stream));
    int rr;
    if ((rr = scan_total(e, (uint64_t*)fl.cnt, NB + 1, false, SC_MISC, passed))) return rr;
    info->syncs++;
    return known_record_error(e, err, what);
  };
  if (!R.kept && S.kept) {  // no layer: S is still validated (k = 0: no bit is read)
    uint64_t passed;
    if ((r = tested(test, CascLayer{nullptr, 1u, 0u, 1u}, &passed))) return r;
  }
  std::vector<ctmr_cascade_layer> table;
  while (hold.n) {
    const uint32_t level = (uint32_t)table.size() + 1;
    const uint32_t k = level == 1 ? p.k_first : p.k_rest, bpk = level == 1 ? p.bpk_first_q8 : p.bpk_rest_q8;
    const uint64_t m = std::max<uint64_t>(1, (hold.n * bpk + 255) / 256);
    if (m >= (1ull << 32)) return fail(e, CTMR_E_INVAL, "%s: layer %u would have %llu bits, at most 2^32 - 1", what, level, (unsigned long long)m);
    const size_t bytes = (size_t)(((m + 7) / 8 + 63) & ~63ull);
    bits.emplace_back(new DevMem);
    if (bits.back()->alloc(bytes) != hipSuccess) return fail(e, CTMR_E_NOMEM, "%s: no device memory for a layer of %llu bits", what, (unsigned long long)m);
    HIPCHK(e, hipMemsetAsync(bits.back()->p, 0, bytes, e->stream));
    const CascLayer ly{(uint32_t*)bits.back()->p, (uint32_t)m, k, level};
    table.push_back(ctmr_cascade_layer{level, k, m, 0, hold.n});
    for (const KnownRun& run : casc_runs(hold, chunk))
      hipLaunchKernelGGL(k_casc_insert, dim3((unsigned)run.blocks()), dim3(256), 0, e->stream, casc_src(hold, t8, run), run.n, hp, ly, d_err);
    if (!test.n) break;
    uint64_t passed = 0;
    if ((r = tested(test, ly, &passed))) return r;
    if (!passed) break;
    if (level == p.max_layers) {
      info->left = passed;
      return fail(e, CTMR_E_INVAL, "%s: %llu records left after %u layers (a key in both operands, or degenerate sizes)", what,
                  (unsigned long long)passed, level);
    }
    // ---- the survivors of the tested sequence, in its order: what the next layer holds; it is tested with what this held
    lists.emplace_back(new DevMem);
    if (lists.back()->alloc(passed * 8) != hipSuccess) return fail(e, CTMR_E_NOMEM, "%s: no device memory for %llu survivors", what, (unsigned long long)passed);
    uint2* d_list = (uint2*)lists.back()->p;
    for (const KnownRun& run : casc_runs(test, chunk))
      hipLaunchKernelGGL(k_casc_compact, dim3((unsigned)run.blocks()), dim3(256), 0, e->stream, casc_src(test, t8, run), run.n, fl, run.blk0,
                         d_list);
    const CascSeq next{test.side, d_list, passed};
    test = hold;
    hold = next;
  }
  // ---- every record read is valid (a side that was only inserted is judged here): the layout, the sizing
  HIPCHK(e, hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  info->syncs++;
  if ((r = known_record_error(e, err, what))) return r;
  uint64_t at = (CASC_HEADER + table.size() * CASC_LAYER_BYTES + 63) & ~63ull;
  const uint64_t head_bytes = at;
  for (auto& l : table) {
    l.offset = at;
    at += ((l.m_bits + 7) / 8 + 63) & ~63ull;
  }
  info->bytes = at;
  info->layers = (uint32_t)table.size();
  for (size_t i = 0; i < table.size(); i++) info->layer[i] = table[i];
  if (!out || out_cap < info->bytes)
    return fail(e, CTMR_E_RANGE, "%s: %llu bytes needed for %u layers", what, (unsigned long long)info->bytes, info->layers);
  std::vector<uint8_t> head;
  head.assign(CASC_MAGIC, CASC_MAGIC + 8);
  put32(head, CASC_VERSION);
  put32(head, CASC_HASH_SHA256_32);
  put32(head, info->layers);
  put32(head, p.salt_len);
  for (uint32_t i = 0; i < 16; i++) head.push_back(i < p.salt_len ? p.salt[i] : 0);
  put64(head, info->bytes);
  put64(head, R.kept);
  put64(head, S.kept);
  for (auto& l : table) {
    put32(head, l.level);
    put32(head, l.k);
    put64(head, l.m_bits);
    put64(head, l.offset);
    put64(head, l.n_held);
  }
  head.resize(head_bytes, 0);
  if (host) memcpy(out, head.data(), head.size());
  else HIPCHK(e, hipMemcpyAsync(out, head.data(), head.size(), hipMemcpyHostToDevice, e->stream));
  for (size_t i = 0; i < table.size(); i++) {
    const size_t bytes = (size_t)(((table[i].m_bits + 7) / 8 + 63) & ~63ull);
    HIPCHK(e, hipMemcpyAsync(out + table[i].offset, bits[i]->p, bytes, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, e->stream));
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  return CTMR_OK;
}

// A cascade's header and layer table (host memory: at least the first CASC_HEADER + 32 × layers bytes of it) held
// against the buffer's length.
int casc_parse(ctmr_engine* e, const uint8_t* c, size_t have, size_t len, uint32_t* layers, CascHash* hp, std::vector<ctmr_cascade_layer>* table) {
  const char* what = "cascade query";
  if (len < CASC_HEADER || have < CASC_HEADER) return fail(e, CTMR_E_INVAL, "%s: a cascade shorter than its header", what);
  if (memcmp(c, CASC_MAGIC, 8) != 0) return fail(e, CTMR_E_INVAL, "%s: bad magic", what);
  if (rd32(c + 8) != CASC_VERSION) return fail(e, CTMR_E_INVAL, "%s: version %u, expected 1", what, rd32(c + 8));
  if (rd32(c + 12) != CASC_HASH_SHA256_32) return fail(e, CTMR_E_INVAL, "%s: hash algorithm %u, expected 2", what, rd32(c + 12));
  const uint32_t n = rd32(c + 16), salt_len = rd32(c + 20);
  if (n > CTMR_CASCADE_MAX_LAYERS || salt_len > 16) return fail(e, CTMR_E_INVAL, "%s: %u layers, a salt of %u octets", what, n, salt_len);
  if (rd64(c + 40) != len) return fail(e, CTMR_E_INVAL, "%s: %llu bytes, the header says %llu", what, (unsigned long long)len, (unsigned long long)rd64(c + 40));
  const uint64_t head = CASC_HEADER + (uint64_t)n * CASC_LAYER_BYTES;
  if (head > len) return fail(e, CTMR_E_INVAL, "%s: the layer table reaches beyond the cascade", what);
  *layers = n;
  *hp = casc_prefix(c + 24, salt_len);
  if (have < head) return CTMR_OK;  // (the caller fetches the table and comes again)
  uint32_t prev = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint8_t* q = c + CASC_HEADER + (size_t)i * CASC_LAYER_BYTES;
    const ctmr_cascade_layer l{rd32(q), rd32(q + 4), rd64(q + 8), rd64(q + 16), rd64(q + 24)};
    if (l.level <= prev || l.level > 255) return fail(e, CTMR_E_INVAL, "%s: layer %u has level %u behind level %u", what, i, l.level, prev);
    if (l.k < 1 || l.k > 32 || l.m_bits < 1 || l.m_bits >= (1ull << 32))
      return fail(e, CTMR_E_INVAL, "%s: layer %u has k = %u, m = %llu", what, i, l.k, (unsigned long long)l.m_bits);
    if ((l.offset & 63u) || l.offset < head || l.offset > len || ((l.m_bits + 31) / 32) * 4 > len - l.offset)
      return fail(e, CTMR_E_INVAL, "%s: the bits of layer %u lie outside the cascade", what, i);
    prev = l.level;
    table->push_back(l);
  }
  return CTMR_OK;
}

// The cascade and P's member records are on the device; the table is parsed.  The answers are staged in working memory
// and go out — to d_out on the device or h_out on the host — once every record of P is known to be valid.
int cascade_query_core(ctmr_engine* e, const uint8_t* d_c, const CascHash& hp, const std::vector<ctmr_cascade_layer>& table,
                       const KnownMeta& pm, const uint8_t* d_p, uint8_t* d_out, uint8_t* h_out) {
  const char* what = "cascade query";
  int r;
  if (pm.n_members >= (1ull << 32)) return fail(e, CTMR_E_INVAL, "%s: %llu member records, at most 2^32 - 1", what, (unsigned long long)pm.n_members);
  // all sets of P answer, whatever their hour: the segments are P's own set records
  CascSide P;
  P.m = &pm;
  P.d = d_p;
  P.dst.assign(pm.set_first.begin(), pm.set_first.end());
  P.src.assign(pm.set_first.begin(), pm.set_first.end() - 1);
  P.ord = pm.set_issuer;
  for (uint64_t s = 0; s < pm.n_sets; s++) P.x.set_range.push_back({pm.set_first[s], pm.set_first[s + 1] - pm.set_first[s]});
  P.kept = P.x.info.members = pm.n_members;
  if (!P.kept) return CTMR_OK;
  KnownPack pk;
  casc_pack_side(&pk, &P);
  std::vector<CascLayer> ls;
  for (auto& l : table) ls.push_back(CascLayer{(uint32_t*)(d_c + l.offset), (uint32_t)l.m_bits, l.k, l.level});
  const size_t o_ls = pk.put(ls), o_err = pk.put_err();
  DevMem tabs, stage;
  if (tabs.alloc(pk.b.size()) != hipSuccess || stage.alloc(P.kept) != hipSuccess)
    return fail(e, CTMR_E_NOMEM, "%s: no device memory for the tables and %llu answers", what, (unsigned long long)P.kept);
  HIPCHK(e, hipMemcpyAsync(tabs.p, pk.b.data(), pk.b.size(), hipMemcpyHostToDevice, e->stream));
  const uint8_t* t8 = tabs.u8();
  uint32_t* d_err = (uint32_t*)(t8 + o_err);
  const CascSeq all{&P, nullptr, P.kept};
  for (const KnownRun& run : casc_runs(all, casc_chunk()))
    hipLaunchKernelGGL(k_casc_query, dim3((unsigned)run.blocks()), dim3(256), 0, e->stream, casc_src(all, t8, run), run.n, hp,
                       (const CascLayer*)(t8 + o_ls), (uint32_t)ls.size(), stage.u8(), d_err);
  uint32_t err = 0;
  HIPCHK(e, hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  if ((r = known_record_error(e, err, what))) return r;
  if (h_out) HIPCHK(e, hipMemcpyAsync(h_out, stage.p, P.kept, hipMemcpyDeviceToHost, e->stream));
  else HIPCHK(e, hipMemcpyAsync(d_out, stage.p, P.kept, hipMemcpyDeviceToDevice, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return CTMR_OK;
}

}  // namespace
}  // extern "C++"

int ctmr_cascade_build(ctmr_engine* e, const uint8_t* revoked, size_t revoked_len, const uint8_t* known, size_t known_len,
                       int64_t now_unix, const ctmr_cascade_params* params, uint8_t* out, size_t out_cap, ctmr_cascade_info* info) {
  if (!e || !revoked || !known || !params || !info) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  KnownMeta rm, sm;
  DevMem dr, ds;
  int r;
  if ((r = known_open(e, revoked, revoked_len, nullptr, "cascade build (R)", &rm))) return r;
  if ((r = known_open(e, known, known_len, nullptr, "cascade build (S)", &sm))) return r;
  if ((r = known_stage_members(e, rm, revoked, 0, "cascade build (R)", &dr))) return r;
  if ((r = known_stage_members(e, sm, known, 0, "cascade build (S)", &ds))) return r;
  return cascade_core(e, rm, dr.u8(), sm, ds.u8(), now_unix, *params, out, out ? out_cap : 0, true, info);
}

int ctmr_cascade_build_device(ctmr_engine* e, const uint8_t* r_meta, size_t r_meta_len, const void* d_r_members, uint64_t r_members,
                              const uint8_t* s_meta, size_t s_meta_len, const void* d_s_members, uint64_t s_members, int64_t now_unix,
                              const ctmr_cascade_params* params, void* d_out, size_t out_cap, ctmr_cascade_info* info) {
  if (!e || !r_meta || !s_meta || !params || !info) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  KnownMeta rm, sm;
  int r;
  if ((r = known_open(e, r_meta, r_meta_len, &r_members, "cascade build (R)", &rm))) return r;
  if ((r = known_open(e, s_meta, s_meta_len, &s_members, "cascade build (S)", &sm))) return r;
  return cascade_core(e, rm, (const uint8_t*)d_r_members, sm, (const uint8_t*)d_s_members, now_unix, *params, (uint8_t*)d_out,
                      d_out ? out_cap : 0, false, info);
}

int ctmr_cascade_query(ctmr_engine* e, const uint8_t* cascade, size_t cascade_len, const uint8_t* probes, size_t probes_len,
                       uint8_t* out, size_t out_cap, ctmr_cascade_query_info* info) {
  if (!e || !cascade || !probes || !info) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  memset(info, 0, sizeof *info);
  CascHash hp;
  std::vector<ctmr_cascade_layer> table;
  KnownMeta pm;
  DevMem dp, dc;
  int r;
  if ((r = casc_parse(e, cascade, cascade_len, cascade_len, &info->layers, &hp, &table))) return r;
  if ((r = known_open(e, probes, probes_len, nullptr, "cascade query (P)", &pm))) return r;
  info->probes = pm.n_members;
  info->host_probes = pm.host.size();
  if (pm.n_members && (!out || out_cap < pm.n_members))
    return fail(e, CTMR_E_RANGE, "cascade query: %llu answers needed", (unsigned long long)pm.n_members);
  if (!pm.n_members) return CTMR_OK;
  if ((r = known_stage_members(e, pm, probes, 0, "cascade query (P)", &dp))) return r;
  if (dc.alloc(cascade_len) != hipSuccess) return fail(e, CTMR_E_NOMEM, "cascade query: no device memory for the cascade");
  HIPCHK(e, hipMemcpyAsync(dc.p, cascade, cascade_len, hipMemcpyHostToDevice, e->stream));
  return cascade_query_core(e, dc.u8(), hp, table, pm, dp.u8(), nullptr, out);
}

int ctmr_cascade_query_device(ctmr_engine* e, const void* d_cascade, size_t cascade_len, const uint8_t* p_meta, size_t p_meta_len,
                              const void* d_p_members, uint64_t p_members, void* d_out, uint64_t out_cap,
                              ctmr_cascade_query_info* info) {
  if (!e || !d_cascade || !p_meta || !info) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  memset(info, 0, sizeof *info);
  int r;
  if ((r = known_aligned16(e, (uintptr_t)d_cascade | (uintptr_t)d_p_members | (uintptr_t)d_out, "cascade query"))) return r;
  if (cascade_len < CASC_HEADER) return fail(e, CTMR_E_INVAL, "cascade query: a cascade shorter than its header");
  // ---- the header, then the layer table it announces, to the host
  std::vector<uint8_t> head(CASC_HEADER);
  HIPCHK(e, hipMemcpy(head.data(), d_cascade, CASC_HEADER, hipMemcpyDeviceToHost));
  CascHash hp;
  std::vector<ctmr_cascade_layer> table;
  if ((r = casc_parse(e, head.data(), head.size(), cascade_len, &info->layers, &hp, &table))) return r;
  if (info->layers) {
    head.resize(CASC_HEADER + (size_t)info->layers * CASC_LAYER_BYTES);
    HIPCHK(e, hipMemcpy(head.data(), d_cascade, head.size(), hipMemcpyDeviceToHost));
    if ((r = casc_parse(e, head.data(), head.size(), cascade_len, &info->layers, &hp, &table))) return r;
  }
  KnownMeta pm;
  if ((r = known_open(e, p_meta, p_meta_len, &p_members, "cascade query (P)", &pm))) return r;
  if ((r = known_bind(e, pm, (const uint8_t*)d_p_members, "cascade query (P)"))) return r;
  info->probes = pm.n_members;
  info->host_probes = pm.host.size();
  if (pm.n_members && (!d_out || out_cap < pm.n_members))
    return fail(e, CTMR_E_RANGE, "cascade query: %llu answers needed", (unsigned long long)pm.n_members);
  return cascade_query_core(e, (const uint8_t*)d_cascade, hp, table, pm, (const uint8_t*)d_p_members, (uint8_t*)d_out, nullptr);
}
