// engine/find.inc — serials looked up in a known image whatever their expiration date (include/ctmr.h
// ctmr_known_image_find*, DESIGN.md §25): for every member of the probe image P, under how many kept sets of the known
// image K the same Issuer.ID holds the same serial, and the lowest and highest exp hour among them.  Host side: both
// metas opened, K's kept sets chosen by the rules of ctmr_known_image_lists (engine/lists.inc: lists_hour_kept,
// lists_parse_date), the Issuer.IDs of both images joined as strings, the two host sections matched against each other
// here and against the other image's member records on the device (kernels/find.h).
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after engine/merge.inc.

extern "C++" {
namespace {

constexpr uint64_t FIND_CHUNK = 1ull << 27;  // member records of K per launch

// what the host knows of a probe's answer before the device's part is added
struct FindAcc {
  uint64_t records = 0;
  int32_t first = INT32_MAX, last = INT32_MIN;
  void add(uint64_t n, int32_t lo, int32_t hi) {
    if (!n) return;
    records += n;
    first = std::min(first, lo);
    last = std::max(last, hi);
  }
};

// What a call knows of its two operands before anything is launched — shared with engine/split.inc.  K: the Issuer.IDs
// it names (K ordinals, per ID string: a digest the image lists twice is one ID), its kept sets in image order as the
// segments of a virtual record sequence, its kept host pairs.  P: the K ordinal of every set's issuer and of every
// host-section member's key, the host-section members a member record of K can equal as probes of their own (extra).
// hr_*: the pairs of K's host section the member section could carry — one more run, against P's member records.
struct FindHostPair { uint32_t kord; int32_t hour; const std::string* member; size_t at; };  // at: its index in K's host section

struct FindPrep {
  std::unordered_map<std::string, uint32_t> kord_of;
  KnownExport x;  // the kept sets as (first virtual record, count): what known_cut_sets cuts into runs
  std::vector<uint64_t> seg_src, seg_set;  // per kept set: its first record in K, the set record of K it is
  std::vector<int32_t> seg_hour;
  std::vector<uint32_t> seg_kord;
  uint64_t kept_records = 0, sets_kept = 0;
  std::vector<FindHostPair> kh;
  std::vector<uint32_t> p_set_kord, p_host_kord;
  bool main_named = false;  // a member record of P can match at all
  uint64_t n_main = 0, n_hostp = 0;
  std::vector<uint8_t> extra_rec;
  std::vector<uint32_t> extra_kord;
  std::vector<uint64_t> extra_of;  // the host-section member an extra probe stands for
  std::vector<uint8_t> hr_rec;
  std::vector<uint64_t> hr_dst, hr_src, hr_of;  // hr_of: the pair of kh a record of the run stands for
  std::vector<int32_t> hr_hour;
  std::vector<uint32_t> hr_kord;
  uint64_t n_extra() const { return extra_kord.size(); }
  uint64_t n_probes() const { return n_main + extra_kord.size(); }
  uint64_t n_hr() const { return hr_src.size(); }
};

int find_prepare(ctmr_engine* e, const KnownMeta& k, const uint8_t* d_k, const KnownMeta& p, const uint8_t* d_p, int64_t now,
                 const void* d_out0, const void* d_out1, const char* what, FindPrep* q) {
  int r;
  if ((r = known_bind(e, k, d_k, what)) || (r = known_bind(e, p, d_p, what))) return r;
  if ((r = known_aligned16(e, (uintptr_t)d_k | (uintptr_t)d_p | (uintptr_t)d_out0 | (uintptr_t)d_out1, what))) return r;
  // ---- K: the Issuer.IDs it names (K ordinals), its kept sets in image order, its kept host pairs
  auto kord = [&](const std::string& id) {
    return q->kord_of.emplace(id, (uint32_t)q->kord_of.size()).first->second;
  };
  std::vector<uint32_t> kord_of_ordinal(k.n_issuers);  // (a digest the image lists twice: one ID, one K ordinal)
  for (uint32_t o = 0; o < k.n_issuers; o++) kord_of_ordinal[o] = kord(k.ids[o]);
  q->x.set_range.reserve(k.n_sets);
  q->seg_src.reserve(k.n_sets);
  q->seg_set.reserve(k.n_sets);
  q->seg_hour.reserve(k.n_sets);
  q->seg_kord.reserve(k.n_sets);
  for (uint64_t s = 0; s < k.n_sets; s++) {  // (per set no string is touched: an image has many sets)
    if (!lists_hour_kept(k.set_hour[s], now)) continue;
    const uint64_t cnt = k.set_first[s + 1] - k.set_first[s];
    q->x.set_range.push_back({q->kept_records, cnt});
    q->seg_src.push_back(k.set_first[s]);
    q->seg_set.push_back(s);
    q->seg_hour.push_back(k.set_hour[s]);
    q->seg_kord.push_back(kord_of_ordinal[k.set_issuer[s]]);
    q->kept_records += cnt;
  }
  q->x.info.members = q->kept_records;
  q->sets_kept = q->x.set_range.size();
  uint32_t ko = 0;
  if ((r = known_kept_host_pairs(e, k, now, what, [&](size_t j, bool new_key, const std::string& id, int64_t start) {
        if (new_key) {
          ko = kord(id);
          q->sets_kept++;
        }
        q->kh.push_back({ko, (int32_t)(start / 3600), &k.host[j].second, j});
      })))
    return r;
  // ---- P: the K ordinal of every set's issuer; its host-section members, and those a member record of K can equal as
  // probes of their own
  auto find_kord = [&](const std::string& id) {
    auto it = q->kord_of.find(id);
    return it == q->kord_of.end() ? FIND_NO_ISSUER : it->second;
  };
  q->p_set_kord.resize(p.n_sets);
  for (uint64_t s = 0; s < p.n_sets; s++) {
    q->p_set_kord[s] = find_kord(p.ids[p.set_issuer[s]]);
    q->main_named = q->main_named || q->p_set_kord[s] != FIND_NO_ISSUER;
  }
  q->n_main = p.n_members;
  q->n_hostp = p.host.size();
  q->p_host_kord.assign(q->n_hostp, FIND_NO_ISSUER);
  {
    const std::string* prev = nullptr;
    uint32_t ko = FIND_NO_ISSUER;
    for (size_t j = 0; j < q->n_hostp; j++) {
      auto& hm = p.host[j];
      if (!prev || *prev != hm.first) {
        std::string date, id;  // (the date is not looked at: the hour is the wildcard)
        if (!known_split_key(hm.first, &date, &id)) return fail(e, CTMR_E_INVAL, "%s: unexpected key format: %s", what, hm.first.c_str());
        ko = find_kord(id);
        prev = &hm.first;
      }
      q->p_host_kord[j] = ko;
      if (ko == FIND_NO_ISSUER) continue;
      if (hm.second.size() <= CTMR_MAX_SERIAL && q->kept_records) {
        known_put_record(hm.second, &q->extra_rec);
        q->extra_kord.push_back(ko);
        q->extra_of.push_back(j);
      }
    }
  }
  // ---- the pairs of K's host section the member section could carry: one more run, against P's member records
  if (q->n_main && q->main_named)
    for (size_t i = 0; i < q->kh.size(); i++) {
      const FindHostPair& h = q->kh[i];
      if (h.member->size() <= CTMR_MAX_SERIAL) {
        q->hr_dst.push_back(q->hr_src.size());
        q->hr_src.push_back(q->hr_src.size());
        q->hr_of.push_back(i);
        q->hr_hour.push_back(h.hour);
        q->hr_kord.push_back(h.kord);
        known_put_record(*h.member, &q->hr_rec);
      }
    }
  q->hr_dst.push_back(q->hr_src.size());
  return CTMR_OK;
}

// The tables of a FindPrep packed for one upload, and what the kernels are given of them once they lie at t8.
struct FindTabs {
  KnownPack pk;
  size_t o_pfirst, o_pkord, o_xrec, o_xkord, o_dst, o_src, o_hour, o_kord, o_hrec, o_hdst, o_hsrc, o_hhour, o_hkord, o_err;
  void pack(const FindPrep& q, const KnownMeta& p) {
    const uint64_t K = q.x.set_range.size();
    std::vector<uint64_t> dst(K + 1);
    for (uint64_t s = 0; s <= K; s++) dst[s] = q.x.first(s);
    o_pfirst = pk.put(p.set_first); o_pkord = pk.put(q.p_set_kord); o_xrec = pk.put(q.extra_rec); o_xkord = pk.put(q.extra_kord);
    o_dst = pk.put(dst); o_src = pk.put(q.seg_src); o_hour = pk.put(q.seg_hour); o_kord = pk.put(q.seg_kord);
    o_hrec = pk.put(q.hr_rec); o_hdst = pk.put(q.hr_dst); o_hsrc = pk.put(q.hr_src); o_hhour = pk.put(q.hr_hour); o_hkord = pk.put(q.hr_kord);
    o_err = pk.put_err();
  }
  FindProbes probes(const FindPrep& q, const KnownMeta& p, const uint8_t* t8, const uint8_t* d_p) const {
    FindProbes fp{};
    fp.recs = d_p; fp.extra = t8 + o_xrec; fp.extra_kord = (const uint32_t*)(t8 + o_xkord);
    fp.set_first = (const uint64_t*)(t8 + o_pfirst); fp.set_kord = (const uint32_t*)(t8 + o_pkord);
    fp.n_main = q.n_main; fp.n_extra = q.n_extra(); fp.n_sets = (uint32_t)p.n_sets;
    return fp;
  }
  // the kept sets [s_lo, s_hi) of K as one run
  FindSegs run(const uint8_t* t8, const uint8_t* d_k, size_t s_lo, size_t s_hi) const {
    return FindSegs{{d_k, (const uint64_t*)(t8 + o_dst) + s_lo, (const uint64_t*)(t8 + o_src) + s_lo, (uint32_t)(s_hi - s_lo)},
                    (const int32_t*)(t8 + o_hour) + s_lo, (const uint32_t*)(t8 + o_kord) + s_lo};
  }
  // the host pairs' run
  FindSegs host_run(const FindPrep& q, const uint8_t* t8) const {
    return FindSegs{{t8 + o_hrec, (const uint64_t*)(t8 + o_hdst), (const uint64_t*)(t8 + o_hsrc), (uint32_t)q.n_hr()},
                    (const int32_t*)(t8 + o_hhour), (const uint32_t*)(t8 + o_hkord)};
  }
};

// Both metas are parsed and the member records of both images are on the device.  d_hits: device memory for
// p.n_members hits (the device variant's buffer), or null: then the hits of P's member records go to `hits` on the host.
int find_core(ctmr_engine* e, const KnownMeta& k, const uint8_t* d_k, const KnownMeta& p, const uint8_t* d_p, int64_t now,
              ctmr_known_find_hit* hits, uint8_t* d_hits, uint64_t hits_cap, ctmr_known_find_hit* host_hits, size_t host_hits_cap,
              ctmr_known_find_info* info) {
  const char* what = "known image find";
  int r;
  FindPrep q;
  if ((r = find_prepare(e, k, d_k, p, d_p, now, d_hits, nullptr, what, &q))) return r;
  const KnownExport& x = q.x;
  const uint64_t kept_records = q.kept_records, n_main = q.n_main, n_hostp = q.n_hostp;
  const uint64_t n_extra = q.n_extra(), n_probes = q.n_probes(), n_hr = q.n_hr();
  const std::vector<uint64_t>& extra_of = q.extra_of;
  // ---- the two host sections matched here: K's kept pairs by (K ordinal, member)
  std::map<std::pair<uint32_t, std::string>, FindAcc> kh_by;
  for (auto& h : q.kh) kh_by[{h.kord, *h.member}].add(1, h.hour, h.hour);
  std::vector<FindAcc> host_acc(n_hostp);
  for (size_t j = 0; j < n_hostp; j++) {
    if (q.p_host_kord[j] == FIND_NO_ISSUER) continue;
    auto it = kh_by.find({q.p_host_kord[j], p.host[j].second});
    if (it != kh_by.end()) host_acc[j] = it->second;
  }
  // ---- sizing
  memset(info, 0, sizeof *info);
  info->probes = n_main;
  info->host_probes = n_hostp;
  info->sets_kept = q.sets_kept;
  info->members_read = kept_records;
  if (hits_cap < n_main || host_hits_cap < n_hostp || (n_main && !hits && !d_hits) || (n_hostp && !host_hits))
    return fail(e, CTMR_E_RANGE, "%s: %llu hits and %llu host hits needed", what, (unsigned long long)n_main, (unsigned long long)n_hostp);
  // ---- every working buffer: the tables in one upload, the probe table, the working hits, the finish pass's counts
  const uint64_t K = x.set_range.size();
  if (K > 0xffffffffull || n_hr > 0xffffffffull || n_probes >= (1ull << 31))
    return fail(e, CTMR_E_NOMEM, "%s: %llu kept sets, %llu probes", what, (unsigned long long)K, (unsigned long long)n_probes);
  const uint64_t forced_slots = env_u64("CTMR_KNOWN_FIND_SLOTS");  // tests only: the smallest table, so that chains are long
  const uint64_t slots = forced_slots ? pow2_at_least(n_probes + 1) : pow2_at_least(std::max<uint64_t>(2 * n_probes, 64));
  const uint64_t nb_fin = (n_probes + 255) / 256;
  FindTabs tb;
  tb.pack(q, p);
  const KnownPack& pk = tb.pk;
  DevMem tabs, work;
  const size_t off_hits = slots * 8, off_cnt = off_hits + (size_t)n_probes * 16;
  if (tabs.alloc(pk.b.size()) != hipSuccess || work.alloc(off_cnt + (nb_fin + 1) * 8) != hipSuccess)
    return fail(e, CTMR_E_NOMEM, "%s: no device memory for a table of %llu words and %llu hits", what, (unsigned long long)slots,
                (unsigned long long)n_probes);
  if ((r = ensure(e, SC_MISC, ((nb_fin + SCAN_TILE) / SCAN_TILE) * 8))) return r;
  HIPCHK(e, hipMemcpyAsync(tabs.p, pk.b.data(), pk.b.size(), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemsetAsync(work.p, 0, off_hits, e->stream));
  const uint8_t* t8 = tabs.u8();
  uint32_t* d_err = (uint32_t*)(t8 + tb.o_err);
  uint4* d_work = (uint4*)(work.u8() + off_hits);
  unsigned long long* d_cnt = (unsigned long long*)(work.u8() + off_cnt);
  const FindProbes fp = tb.probes(q, p, t8, d_p);
  const FindTable ft{(unsigned long long*)work.p, slots - 1};
  // ---- build, then the runs of K: whole kept sets of at most FIND_CHUNK records, the host pairs' run last
  if (n_probes) hipLaunchKernelGGL(k_find_build, dim3((unsigned)nb_fin), dim3(256), 0, e->stream, fp, ft, d_work, d_err);
  if (n_probes && kept_records)
    for (const KnownRun& run : known_cut_sets(x, known_chunk("CTMR_KNOWN_FIND_CHUNK", FIND_CHUNK)))
      hipLaunchKernelGGL(k_find_scan, dim3((unsigned)run.blocks()), dim3(256), 0, e->stream, tb.run(t8, d_k, run.s_lo, run.s_hi), run.n, ft,
                         fp, n_probes, d_work, d_err);
  if (n_hr) {
    const FindSegs g = tb.host_run(q, t8);
    hipLaunchKernelGGL(k_find_scan, dim3((unsigned)((n_hr + 255) / 256)), dim3(256), 0, e->stream, g, n_hr, ft, fp, n_main, d_work, d_err);
  }
  uint32_t err = 0;
  HIPCHK(e, hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  if ((r = known_record_error(e, err, what))) return r;
  // ---- every record is valid: the hits go out
  uint64_t found = 0;
  std::vector<ctmr_known_find_hit> xh(n_extra);
  if (n_probes) {
    uint4* out_main = d_hits ? (uint4*)d_hits : d_work;
    const uint64_t nb_main = (n_main + 255) / 256, nb_x = (n_extra + 255) / 256;
    if (n_main) hipLaunchKernelGGL(k_find_finish, dim3((unsigned)nb_main), dim3(256), 0, e->stream, (const uint4*)d_work, out_main, n_main, d_cnt);
    if (n_extra) hipLaunchKernelGGL(k_find_finish, dim3((unsigned)nb_x), dim3(256), 0, e->stream, (const uint4*)(d_work + n_main),
                                    d_work + n_main, n_extra, d_cnt + nb_main);
    if (n_main) {
      if ((r = scan_u64(e, (uint64_t*)d_cnt, nb_main, true, SC_MISC))) return r;
      unsigned long long f = 0;
      HIPCHK(e, hipMemcpyAsync(&f, d_cnt + nb_main - 1, 8, hipMemcpyDeviceToHost, e->stream));
      if (!d_hits) HIPCHK(e, hipMemcpyAsync(hits, d_work, n_main * 16, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(e, hipStreamSynchronize(e->stream));
      found = f;
    }
    if (n_extra) HIPCHK(e, hipMemcpy(xh.data(), d_work + n_main, n_extra * 16, hipMemcpyDeviceToHost));
    HIPCHK(e, hipGetLastError());
  }
  for (uint64_t q = 0; q < n_extra; q++) host_acc[extra_of[q]].add(xh[q].records, xh[q].first_hour, xh[q].last_hour);
  uint64_t host_found = 0;
  for (uint64_t j = 0; j < n_hostp; j++) {
    const FindAcc& a = host_acc[j];
    host_hits[j] = ctmr_known_find_hit{(uint32_t)a.records, a.records ? a.first : 0, a.records ? a.last : 0, 0u};
    host_found += a.records != 0;
  }
  info->found = found;
  info->host_found = host_found;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return CTMR_OK;
}

}  // namespace
}  // extern "C++"

int ctmr_known_image_find(ctmr_engine* e, const uint8_t* known, size_t known_len, const uint8_t* probes, size_t probes_len,
                          int64_t now_unix, ctmr_known_find_hit* hits, size_t hits_cap, ctmr_known_find_hit* host_hits,
                          size_t host_hits_cap, ctmr_known_find_info* info) {
  if (!e || !known || !probes || !info) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  KnownMeta k, p;
  DevMem dk, dp;
  int r;
  if ((r = known_open(e, known, known_len, nullptr, "known image find (K)", &k))) return r;
  if ((r = known_open(e, probes, probes_len, nullptr, "known image find (P)", &p))) return r;
  if ((r = known_stage_members(e, k, known, 0, "known image find (K)", &dk))) return r;
  if ((r = known_stage_members(e, p, probes, 0, "known image find (P)", &dp))) return r;
  return find_core(e, k, dk.u8(), p, dp.u8(), now_unix, hits, nullptr, hits_cap, host_hits, host_hits_cap, info);
}

int ctmr_known_image_find_device(ctmr_engine* e, const uint8_t* k_meta, size_t k_meta_len, const void* d_k_members,
                                 uint64_t k_members, const uint8_t* p_meta, size_t p_meta_len, const void* d_p_members,
                                 uint64_t p_members, int64_t now_unix, void* d_hits, uint64_t hits_cap,
                                 ctmr_known_find_hit* host_hits, size_t host_hits_cap, ctmr_known_find_info* info) {
  if (!e || !k_meta || !p_meta || !info) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  KnownMeta k, p;
  int r;
  if ((r = known_open(e, k_meta, k_meta_len, &k_members, "known image find (K)", &k))) return r;
  if ((r = known_open(e, p_meta, p_meta_len, &p_members, "known image find (P)", &p))) return r;
  return find_core(e, k, (const uint8_t*)d_k_members, p, (const uint8_t*)d_p_members, now_unix, nullptr, (uint8_t*)d_hits, hits_cap,
                   host_hits, host_hits_cap, info);
}
