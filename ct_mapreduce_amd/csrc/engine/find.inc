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

// device tables of one call, packed into one upload: every piece 16-byte aligned
struct FindPack {
  std::vector<uint8_t> b;
  size_t put(const void* p, size_t n) {
    const size_t at = (b.size() + 15) & ~(size_t)15;
    b.resize(at + n);
    if (n) memcpy(&b[at], p, n);
    return at;
  }
  template <class T> size_t put(const std::vector<T>& v) { return put(v.data(), v.size() * sizeof(T)); }
};

// Both metas are parsed and the member records of both images are on the device.  d_hits: device memory for
// p.n_members hits (the device variant's buffer), or null: then the hits of P's member records go to `hits` on the host.
int find_core(ctmr_engine* e, const KnownMeta& k, const uint8_t* d_k, const KnownMeta& p, const uint8_t* d_p, int64_t now,
              ctmr_known_find_hit* hits, uint8_t* d_hits, uint64_t hits_cap, ctmr_known_find_hit* host_hits, size_t host_hits_cap,
              ctmr_known_find_info* info) {
  const char* what = "known image find";
  int r;
  if ((r = known_bind(e, k, d_k, what)) || (r = known_bind(e, p, d_p, what))) return r;
  if (((uintptr_t)d_k | (uintptr_t)d_p | (uintptr_t)d_hits) & 15u)
    return fail(e, CTMR_E_INVAL, "%s: device memory that is not 16-byte aligned", what);
  // ---- K: the Issuer.IDs it names (K ordinals), its kept sets in image order, its kept host pairs
  std::unordered_map<std::string, uint32_t> kord_of;
  auto kord = [&](const std::string& id) {
    return kord_of.emplace(id, (uint32_t)kord_of.size()).first->second;
  };
  KnownExport x;  // the kept sets as (first virtual record, count): what known_cut_sets cuts into runs
  std::vector<uint64_t> seg_src;
  std::vector<int32_t> seg_hour;
  std::vector<uint32_t> seg_kord;
  uint64_t kept_records = 0;
  std::vector<uint32_t> kord_of_ordinal(k.n_issuers);  // (a digest the image lists twice: one ID, one K ordinal)
  for (uint32_t o = 0; o < k.n_issuers; o++) kord_of_ordinal[o] = kord(k.ids[o]);
  x.set_range.reserve(k.n_sets);
  seg_src.reserve(k.n_sets);
  seg_hour.reserve(k.n_sets);
  seg_kord.reserve(k.n_sets);
  for (uint64_t s = 0; s < k.n_sets; s++) {  // (per set no string is touched: an image has many sets)
    if (!lists_hour_kept(k.set_hour[s], now)) continue;
    const uint64_t cnt = k.set_first[s + 1] - k.set_first[s];
    x.set_range.push_back({kept_records, cnt});
    seg_src.push_back(k.set_first[s]);
    seg_hour.push_back(k.set_hour[s]);
    seg_kord.push_back(kord_of_ordinal[k.set_issuer[s]]);
    kept_records += cnt;
  }
  x.info.members = kept_records;
  uint64_t sets_kept = x.set_range.size();
  struct HostPair { uint32_t kord; int32_t hour; const std::string* member; };
  std::vector<HostPair> kh;  // the kept pairs of K's host section
  std::map<std::pair<uint32_t, std::string>, FindAcc> kh_by;  // … by (K ordinal, member)
  {
    const std::string* prev = nullptr;
    bool prev_kept = false;
    uint32_t ko = 0;
    int32_t hour = 0;
    for (auto& hm : k.host) {
      if (!prev || *prev != hm.first) {  // (the section is in key order: a key's date is parsed once)
        std::string date, id;
        if (!known_split_key(hm.first, &date, &id)) return fail(e, CTMR_E_INVAL, "%s: unexpected key format: %s", what, hm.first.c_str());
        int64_t start, end;
        prev_kept = lists_parse_date(date, &start, &end) && now < end;
        prev = &hm.first;
        if (prev_kept) {
          ko = kord(id);
          hour = (int32_t)(start / 3600);
          sets_kept++;
        }
      }
      if (!prev_kept) continue;
      kh.push_back({ko, hour, &hm.second});
      kh_by[{ko, hm.second}].add(1, hour, hour);
    }
  }
  // ---- P: the K ordinal of every set's issuer; its host-section members, matched here against K's host pairs, and
  // those a member record of K can equal as probes of their own
  auto find_kord = [&](const std::string& id) {
    auto it = kord_of.find(id);
    return it == kord_of.end() ? FIND_NO_ISSUER : it->second;
  };
  std::vector<uint32_t> p_set_kord(p.n_sets);
  bool main_named = false;  // a member record of P can match at all
  for (uint64_t s = 0; s < p.n_sets; s++) {
    p_set_kord[s] = find_kord(p.ids[p.set_issuer[s]]);
    main_named = main_named || p_set_kord[s] != FIND_NO_ISSUER;
  }
  const uint64_t n_main = p.n_members, n_hostp = p.host.size();
  std::vector<FindAcc> host_acc(n_hostp);
  std::vector<uint8_t> extra_rec;
  std::vector<uint32_t> extra_kord;
  std::vector<uint64_t> extra_of;  // the host-section member an extra probe stands for
  {
    const std::string* prev = nullptr;
    uint32_t ko = FIND_NO_ISSUER;
    for (size_t j = 0; j < n_hostp; j++) {
      auto& hm = p.host[j];
      if (!prev || *prev != hm.first) {
        std::string date, id;  // (the date is not looked at: the hour is the wildcard)
        if (!known_split_key(hm.first, &date, &id)) return fail(e, CTMR_E_INVAL, "%s: unexpected key format: %s", what, hm.first.c_str());
        ko = find_kord(id);
        prev = &hm.first;
      }
      if (ko == FIND_NO_ISSUER) continue;
      auto it = kh_by.find({ko, hm.second});
      if (it != kh_by.end()) host_acc[j] = it->second;
      if (hm.second.size() <= CTMR_MAX_SERIAL && kept_records) {
        known_put_record(hm.second, &extra_rec);
        extra_kord.push_back(ko);
        extra_of.push_back(j);
      }
    }
  }
  const uint64_t n_extra = extra_kord.size(), n_probes = n_main + n_extra;
  // ---- the pairs of K's host section the member section could carry: one more run, against P's member records
  std::vector<uint8_t> hr_rec;
  std::vector<uint64_t> hr_dst, hr_src;
  std::vector<int32_t> hr_hour;
  std::vector<uint32_t> hr_kord;
  if (n_main && main_named)
    for (auto& h : kh)
      if (h.member->size() <= CTMR_MAX_SERIAL) {
        hr_dst.push_back(hr_src.size());
        hr_src.push_back(hr_src.size());
        hr_hour.push_back(h.hour);
        hr_kord.push_back(h.kord);
        known_put_record(*h.member, &hr_rec);
      }
  const uint64_t n_hr = hr_src.size();
  hr_dst.push_back(n_hr);
  // ---- sizing
  memset(info, 0, sizeof *info);
  info->probes = n_main;
  info->host_probes = n_hostp;
  info->sets_kept = sets_kept;
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
  std::vector<uint64_t> dst(K + 1);
  for (uint64_t s = 0; s <= K; s++) dst[s] = x.first(s);
  FindPack pk;
  const size_t o_pfirst = pk.put(p.set_first), o_pkord = pk.put(p_set_kord), o_xrec = pk.put(extra_rec), o_xkord = pk.put(extra_kord);
  const size_t o_dst = pk.put(dst), o_src = pk.put(seg_src), o_hour = pk.put(seg_hour), o_kord = pk.put(seg_kord);
  const size_t o_hrec = pk.put(hr_rec), o_hdst = pk.put(hr_dst), o_hsrc = pk.put(hr_src), o_hhour = pk.put(hr_hour), o_hkord = pk.put(hr_kord);
  const size_t o_err = pk.put(nullptr, 0);
  pk.b.resize(o_err + 16, 0);
  DevMem tabs, work;
  const size_t off_hits = slots * 8, off_cnt = off_hits + (size_t)n_probes * 16;
  if (tabs.alloc(pk.b.size()) != hipSuccess || work.alloc(off_cnt + (nb_fin + 1) * 8) != hipSuccess)
    return fail(e, CTMR_E_NOMEM, "%s: no device memory for a table of %llu words and %llu hits", what, (unsigned long long)slots,
                (unsigned long long)n_probes);
  if ((r = ensure(e, SC_MISC, ((nb_fin + SCAN_TILE) / SCAN_TILE) * 8))) return r;
  HIPCHK(e, hipMemcpyAsync(tabs.p, pk.b.data(), pk.b.size(), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemsetAsync(work.p, 0, off_hits, e->stream));
  const uint8_t* t8 = tabs.u8();
  uint32_t* d_err = (uint32_t*)(t8 + o_err);
  uint4* d_work = (uint4*)(work.u8() + off_hits);
  unsigned long long* d_cnt = (unsigned long long*)(work.u8() + off_cnt);
  FindProbes fp{};
  fp.recs = d_p; fp.extra = t8 + o_xrec; fp.extra_kord = (const uint32_t*)(t8 + o_xkord);
  fp.set_first = (const uint64_t*)(t8 + o_pfirst); fp.set_kord = (const uint32_t*)(t8 + o_pkord);
  fp.n_main = n_main; fp.n_extra = n_extra; fp.n_sets = (uint32_t)p.n_sets;
  const FindTable ft{(unsigned long long*)work.p, slots - 1};
  // ---- build, then the runs of K: whole kept sets of at most FIND_CHUNK records, the host pairs' run last
  if (n_probes) hipLaunchKernelGGL(k_find_build, dim3((unsigned)nb_fin), dim3(256), 0, e->stream, fp, ft, d_work, d_err);
  if (n_probes && kept_records) {
    const uint64_t forced = env_u64("CTMR_KNOWN_FIND_CHUNK");  // tests only: several runs
    const std::vector<size_t> cut = known_cut_sets(x, forced ? forced : FIND_CHUNK);
    for (size_t c = 0; c + 1 < cut.size(); c++) {
      const uint64_t n = x.first(cut[c + 1]) - x.first(cut[c]);
      const FindSegs g{d_k, (const uint64_t*)(t8 + o_dst) + cut[c], (const uint64_t*)(t8 + o_src) + cut[c],
                       (const int32_t*)(t8 + o_hour) + cut[c], (const uint32_t*)(t8 + o_kord) + cut[c], (uint32_t)(cut[c + 1] - cut[c])};
      hipLaunchKernelGGL(k_find_scan, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, g, n, ft, fp, n_probes, d_work, d_err);
    }
  }
  if (n_hr) {
    const FindSegs g{t8 + o_hrec, (const uint64_t*)(t8 + o_hdst), (const uint64_t*)(t8 + o_hsrc), (const int32_t*)(t8 + o_hhour),
                     (const uint32_t*)(t8 + o_hkord), (uint32_t)n_hr};
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
