// engine/lists.inc — per-issuer known-serial lists (include/ctmr.h ctmr_known_lists*, DESIGN.md §13): for every Issuer.ID,
// the serials of its sets that have not expired, as the text LocalDiskBackend.StoreKnownCertificateList writes
// (storage/localdiskbackend.go).  The sets are chosen and ordered on the host (GetIssuerAndDatesFromCache, IsExpiredAt),
// their members staged with k_known_export (engine/image.inc) and turned into text by k_lists_count / k_lists_write.
// ctmr_known_image_lists* (DESIGN.md §17) chooses and orders the sets of an IMAGE by the same rules and runs the same
// write loop over its member records where they lie (k_image_lists_count / k_image_lists_write): no table, no staging.
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after engine/image.inc.

extern "C++" {
namespace {

constexpr uint64_t LISTS_CHUNK = 1ull << 27;  // member records staged per pass (6 GiB; export stages all at once)

// NewExpDate(s) as storage/types.go parses it: "2006-01-02-15" (hour resolution; time.Parse takes one or two hour
// digits) or "2006-01-02" (day resolution), four-digit years.  → the first second of the date and the first second
// at which IsExpiredAt is true (lastGood + 1 ms: date + 1 h or + 24 h).
bool lists_parse_date(const std::string& s, int64_t* start, int64_t* end) {
  auto dig = [&](size_t i) { return i < s.size() && s[i] >= '0' && s[i] <= '9'; };
  if (s.size() < 10 || s[4] != '-' || s[7] != '-') return false;
  for (size_t i : {0, 1, 2, 3, 5, 6, 8, 9})
    if (!dig(i)) return false;
  const int y = (s[0] - '0') * 1000 + (s[1] - '0') * 100 + (s[2] - '0') * 10 + (s[3] - '0');
  const uint32_t m = (s[5] - '0') * 10 + (s[6] - '0'), d = (s[8] - '0') * 10 + (s[9] - '0');
  int h = -1;
  if (s.size() == 12 && s[10] == '-' && dig(11)) h = s[11] - '0';
  else if (s.size() == 13 && s[10] == '-' && dig(11) && dig(12)) h = (s[11] - '0') * 10 + (s[12] - '0');
  else if (s.size() != 10) return false;
  if (m < 1 || m > 12 || d < 1 || d > 31 || h > 23) return false;
  const int64_t days = days_from_civil(y, m, d);
  int32_t yy; uint32_t mm, dd;
  civil_from_days(days, yy, mm, dd);
  if (yy != y || mm != m || dd != d) return false;  // e.g. Feb 30
  *start = days * 86400 + (h < 0 ? 0 : h) * 3600;
  *end = *start + (h < 0 ? 86400 : 3600);
  return true;
}

void lists_hex(const std::string& m, std::string* out) {
  static const char H[] = "0123456789abcdef";
  for (unsigned char c : m) {
    out->push_back(H[c >> 4]);
    out->push_back(H[c & 15]);
  }
  out->push_back('\n');
}

struct KnownLists {
  KnownExport x;                         // the kept device sets in list order: cursors, record ranges, info.members
  std::vector<uint64_t> set_slot;        // … and what each was given as: its pair-table slot, or its first record in an image
  std::vector<std::string> ids;          // Issuer.ID of each list, bytewise ascending
  std::vector<uint64_t> id_rec, id_hb;   // per list: device records before it, host-store bytes before it
  struct Host { uint64_t rec, hb; std::string text; };  // the lines of one host-store key: after device record rec - 1
  std::vector<Host> host;                // ... and after hb bytes of host-store lines; in list order
  uint64_t host_bytes = 0, host_members = 0, sets = 0;
};

// a device set as integers: key = (rank of its Issuer.ID among ids[]) << 32 | (hour − KNOWN_HOUR_LO) — the per-set work
// of many sets stays off strings; an hour's ExpDate.ID is formatted only where a host key of the same issuer and second
// compares to it
struct ListDev { uint64_t key, count, slot; };

// a host-side key as strings.Split(key, "::") splits it: serials, expDate and Issuer.ID — exactly three parts, or false
bool known_split_key(const std::string& k, std::string* date, std::string* id) {
  const size_t a = k.find("::"), b = a == std::string::npos ? a : k.find("::", a + 2);
  if (b == std::string::npos || k.find("::", b + 2) != std::string::npos) return false;
  *date = k.substr(a + 2, b - a - 2);
  *id = k.substr(b + 2);
  return true;
}

// The kept host pairs of a meta: f(j, new_key, id, start) for every pair j of km.host, in order, whose key's expDate has
// not ended at `now` (id, start: the key's Issuer.ID and the first second of its expDate; new_key: the pair is the
// first kept one of its key).  The section is in key order, so a key is split and its date parsed once; a key that
// does not split is an error where it is met.
template <class F>
int known_kept_host_pairs(ctmr_engine* e, const KnownMeta& km, int64_t now, const char* what, F f) {
  const std::string* prev = nullptr;
  bool kept = false;
  std::string date, id;
  int64_t start = 0, end = 0;
  for (size_t j = 0; j < km.host.size(); j++) {
    const std::string& key = km.host[j].first;
    const bool new_key = !prev || *prev != key;
    if (new_key) {
      if (!known_split_key(key, &date, &id)) return fail(e, CTMR_E_INVAL, "%s: unexpected key format: %s", what, key.c_str());
      kept = lists_parse_date(date, &start, &end) && now < end;
      prev = &key;
    }
    if (kept) f(j, new_key, id, start);
  }
  return CTMR_OK;
}

// Which sets, grouped and ordered: the device sets `dev` (kept ones only; ids[rank] = the Issuer.ID of a rank, ascending)
// and the serials:: keys of `store`, kept while now < the end of their expDate; per Issuer.ID ascending, expDates
// ascending (by their first second, then as strings).
int known_lists_arrange(ctmr_engine* e, const std::map<std::string, std::set<std::string>>& store, std::vector<ListDev>& dev,
                        const std::vector<const std::string*>& ids, int64_t now, KnownLists* L) {
  struct Block { const std::set<std::string>* host = nullptr; };
  std::map<std::string, std::map<std::pair<int64_t, std::string>, Block>> by_id;  // the host-store keys
  for (auto& kv : store) {
    const std::string& k = kv.first;
    if (k.compare(0, 9, "serials::") != 0 || kv.second.empty()) continue;
    std::string date, id;
    if (!known_split_key(k, &date, &id)) return fail(e, CTMR_E_INVAL, "known lists: unexpected key format: %s", k.c_str());
    int64_t start, end;
    if (!lists_parse_date(date, &start, &end) || now >= end) continue;  // unparsable: skipped, as the reference does
    by_id[id][{start, date}].host = &kv.second;
  }
  std::sort(dev.begin(), dev.end(), [](const ListDev& p, const ListDev& q) { return p.key < q.key; });
  KnownExport& x = L->x;
  uint64_t rec = 0, hb = 0;
  auto put_host = [&](const std::set<std::string>* hs) {
    KnownLists::Host h{rec, hb, std::string()};
    for (auto& m : *hs) lists_hex(m, &h.text);
    L->host_members += hs->size();
    hb += h.text.size();
    L->host.push_back(std::move(h));
  };
  size_t d = 0;
  auto hi_it = by_id.begin();
  while (d < dev.size() || hi_it != by_id.end()) {
    // the next Issuer.ID: of the device sets, of the host-store keys, or of both
    const std::string* dev_id = d < dev.size() ? ids[dev[d].key >> 32] : nullptr;
    const bool take_dev = dev_id && (hi_it == by_id.end() || *dev_id <= hi_it->first);
    const bool take_host = hi_it != by_id.end() && (!dev_id || hi_it->first <= *dev_id);
    L->ids.push_back(take_dev ? *dev_id : hi_it->first);
    L->id_rec.push_back(rec);
    L->id_hb.push_back(hb);
    const uint64_t rk = take_dev ? dev[d].key >> 32 : 0;
    auto hb_it = take_host ? hi_it->second.begin() : decltype(hi_it->second.begin())();
    auto hb_end = take_host ? hi_it->second.end() : hb_it;
    while ((take_dev && d < dev.size() && (dev[d].key >> 32) == rk) || hb_it != hb_end) {
      int cmp = 0;  // < 0: the device set comes first, > 0: the host-store key, 0: one expDate (one key) in both
      const bool dv = take_dev && d < dev.size() && (dev[d].key >> 32) == rk;
      const int32_t eh = dv ? (int32_t)(uint32_t)(dev[d].key & 0xffffffffull) + (int32_t)KNOWN_HOUR_LO : 0;
      if (!dv) cmp = 1;
      else if (hb_it == hb_end) cmp = -1;
      else if ((int64_t)eh * 3600 != hb_it->first.first) cmp = (int64_t)eh * 3600 < hb_it->first.first ? -1 : 1;
      else cmp = exp_date_id(eh).compare(hb_it->first.second);
      L->sets++;
      if (cmp <= 0) {
        L->set_slot.push_back(dev[d].slot);
        x.set_range.push_back({rec, dev[d].count});
        rec += dev[d].count;
        d++;
      }
      if (cmp >= 0) {
        put_host(hb_it->second.host);
        ++hb_it;
      }
    }
    if (take_host) ++hi_it;
  }
  L->host_bytes = hb;
  x.info.members = rec;
  return CTMR_OK;
}

// a device set of exp hour h is kept: its ExpDate.ID has four year digits and now < (h + 1) × 3600
bool lists_hour_kept(int32_t h, int64_t now) { return hour_fixed(h) && now < ((int64_t)h + 1) * 3600; }

// … of an engine: the pair table's sets and the host-side store
int known_lists_prepare(ctmr_engine* e, int64_t now, KnownLists* L) {
  int r;
  std::vector<PairRec> pr;
  if ((r = list_pairs(e, &pr))) return r;
  std::vector<uint32_t> by_rank, rank_of;
  issuers_by_id(e, &by_rank, &rank_of);
  std::vector<const std::string*> ids(by_rank.size());
  for (size_t k = 0; k < by_rank.size(); k++) ids[k] = &e->issuers[by_rank[k]].id;
  std::vector<ListDev> dev;
  for (auto& p : pr)
    if (lists_hour_kept(p.exp_hour, now))
      dev.push_back({((uint64_t)rank_of[p.canon] << 32) | (uint64_t)(p.exp_hour - KNOWN_HOUR_LO), p.count, p.slot});
  if ((r = known_lists_arrange(e, e->hstore, dev, ids, now, L))) return r;
  KnownExport& x = L->x;
  x.cursor.assign(e->npairs, KNOWN_CURSOR_OFF);  // sets not kept stay parked: their members are never written
  for (size_t k = 0; k < L->set_slot.size(); k++) x.cursor[L->set_slot[k]] = x.set_range[k].first;
  return CTMR_OK;
}

// … of an image: its set records (the ID of a set = the padded base64url of its digest in the image: km.ids) and the
// keys of its host section.  host: the section's pairs as a store, which L points into.
int image_lists_prepare(ctmr_engine* e, const KnownMeta& km, int64_t now, std::map<std::string, std::set<std::string>>* host,
                        KnownLists* L) {
  for (auto& hm : km.host) (*host)[hm.first].insert(hm.second);
  std::vector<uint32_t> by_rank(km.n_issuers), rank_of(km.n_issuers);
  for (uint32_t k = 0; k < km.n_issuers; k++) by_rank[k] = k;
  std::sort(by_rank.begin(), by_rank.end(), [&](uint32_t a, uint32_t b) { return km.ids[a] != km.ids[b] ? km.ids[a] < km.ids[b] : a < b; });
  std::vector<const std::string*> ids;
  for (uint32_t k = 0; k < km.n_issuers; k++) {  // (a digest the image lists twice: one ID, one rank)
    if (!k || km.ids[by_rank[k]] != km.ids[by_rank[k - 1]]) ids.push_back(&km.ids[by_rank[k]]);
    rank_of[by_rank[k]] = (uint32_t)ids.size() - 1u;
  }
  std::vector<ListDev> dev;
  for (uint64_t s = 0; s < km.n_sets; s++)
    if (lists_hour_kept(km.set_hour[s], now))
      dev.push_back({((uint64_t)rank_of[km.set_issuer[s]] << 32) | (uint64_t)(km.set_hour[s] - KNOWN_HOUR_LO),
                     km.set_first[s + 1] - km.set_first[s], km.set_first[s]});
  return known_lists_arrange(e, *host, dev, ids, now, L);
}

// Where the write loop's records come from: staged by k_known_export into a buffer of the loop's (an engine's lists), or
// the segments of an image — the kept sets in list order, set k the records [seg_src[k], …) of `image`.
struct ListSource {
  bool segments = false;           // false: stage with k_known_export
  const uint8_t* image = nullptr;  // segments: the image's member records on the device
  DevMem seg;                      // seg_dst[K + 1], seg_src[K], then the error word
  size_t K = 0;
  const char* what = "known lists";
  const uint64_t* dst() const { return (const uint64_t*)seg.p; }
  const uint64_t* src() const { return dst() + K + 1; }
  uint32_t* err() const { return (uint32_t*)(dst() + 2 * K + 1); }
  ListSegs segs(size_t s_lo, size_t s_hi) const { return ListSegs{image, dst() + s_lo, src() + s_lo, (uint32_t)(s_hi - s_lo)}; }
};

int image_lists_upload(ctmr_engine* e, const KnownLists& L, ListSource* src) {
  const size_t K = L.x.set_range.size();
  src->K = K;
  if (!K) return CTMR_OK;
  if (K > 0xffffffffull) return fail(e, CTMR_E_NOMEM, "%s: %zu sets", src->what, K);
  std::vector<uint64_t> t(2 * K + 2, 0ull);
  for (size_t k = 0; k <= K; k++) t[k] = L.x.first(k);
  for (size_t k = 0; k < K; k++) t[K + 1 + k] = L.set_slot[k];
  if (src->seg.alloc(t.size() * 8) != hipSuccess) return fail(e, CTMR_E_NOMEM, "%s: no device memory for %zu segments", src->what, K);
  HIPCHK(e, hipMemcpyAsync(src->seg.p, t.data(), t.size() * 8, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));  // (t goes out of scope)
  return CTMR_OK;
}

// The device records of a run of the list order, staged and counted: *bytes = their text, cnt[] their block offsets.
// ordered: as known_export_members takes it (the text's size does not depend on the order).
// An image's segments are counted where they lie, and every record read is validated.
int known_lists_count(ctmr_engine* e, KnownLists& L, const ListSource& src, const KnownRun& run, uint8_t* d_rec,
                      unsigned long long* cnt, uint64_t* bytes, bool ordered) {
  int r;
  if (!src.segments && (r = known_export_members(e, L.x, run.s_lo, run.s_hi, d_rec, ordered))) return r;
  const uint64_t n = run.n, nb = run.blocks();
  HIPCHK(e, hipMemsetAsync(cnt + nb, 0, 8, e->stream));
  if (!src.segments) hipLaunchKernelGGL(k_lists_count, dim3((unsigned)nb), dim3(LIST_BLOCK), 0, e->stream, (const uint8_t*)d_rec, n, cnt);
  else if (n) hipLaunchKernelGGL(k_image_lists_count, dim3((unsigned)nb), dim3(LIST_BLOCK), 0, e->stream, src.segs(run.s_lo, run.s_hi), n, cnt, src.err());
  if ((r = scan_u64(e, (uint64_t*)cnt, nb + 1, false, SC_MISC))) return r;
  unsigned long long b;
  uint32_t err = 0;
  HIPCHK(e, hipMemcpyAsync(&b, cnt + nb, 8, hipMemcpyDeviceToHost, e->stream));
  if (src.segments && n) HIPCHK(e, hipMemcpyAsync(&err, src.err(), 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  *bytes = b;
  return known_record_error(e, err, src.what);
}

// The sizing and the write loop over the sets L arranged, their records from src.
int known_lists_emit(ctmr_engine* e, KnownLists& L, const ListSource& src, bool device, uint8_t* text, size_t text_cap,
                     uint8_t* ids, size_t ids_cap, uint64_t* offs, size_t offs_cap, ctmr_known_lists_info* info) {
  int r;
  const uint64_t N = L.x.info.members, G = L.ids.size();
  uint64_t ids_bytes = 0;
  for (auto& s : L.ids) ids_bytes += s.size();
  memset(info, 0, sizeof *info);
  info->issuers = G;
  info->sets = L.sets;
  info->members = N;
  info->host_members = L.host_members;
  info->ids_bytes = ids_bytes;
  // chunks: the runs of whole sets (known_cut_sets)
  const std::vector<KnownRun> runs = known_cut_sets(L.x, known_chunk("CTMR_KNOWN_LISTS_CHUNK", LISTS_CHUNK));
  const size_t nch = runs.size();
  // points: the device record at which each list starts and each host-store piece goes in (ascending, unique)
  std::vector<uint64_t> pts;
  {
    size_t a = 0, b = 0;
    while (a < L.id_rec.size() || b < L.host.size()) {
      const uint64_t v = b == L.host.size() || (a < L.id_rec.size() && L.id_rec[a] <= L.host[b].rec) ? L.id_rec[a++] : L.host[b++].rec;
      if (pts.empty() || pts.back() != v) pts.push_back(v);
    }
  }
  size_t max_pts = 0;
  uint64_t max_n = 0;
  for (size_t c = 0; c < nch; c++) {
    const uint64_t lo = runs[c].lo, hi = lo + runs[c].n;
    max_n = std::max(max_n, runs[c].n);
    max_pts = std::max(max_pts, (size_t)(std::lower_bound(pts.begin(), pts.end(), hi) - std::lower_bound(pts.begin(), pts.end(), lo)));
  }
  DevMem d_rec, tmp, d_text;
  const uint64_t nbmax = (max_n + LIST_BLOCK - 1) / LIST_BLOCK;
  const size_t off_pts = (nbmax + 1) * 8, off_po = off_pts + max_pts * 8;
  if (N && ((!src.segments && d_rec.alloc(max_n * KNOWN_REC_BYTES) != hipSuccess) || tmp.alloc(off_po + max_pts * 8 + 8) != hipSuccess))
    return fail(e, CTMR_E_NOMEM, "%s: no device memory to stage %llu member records", src.what, (unsigned long long)max_n);
  unsigned long long* cnt = (unsigned long long*)tmp.p;
  std::vector<uint64_t> chunk_bytes(nch, ~0ull);
  // sizing: one count pass over every chunk, unless every buffer holds its bound (81 B per member for the text) and
  // the pass that writes can size as it goes; a single chunk is staged once either way
  const bool caps_ok = (!G || (ids && ids_cap >= ids_bytes)) && offs && offs_cap >= 2 * (G + 1);
  const bool roomy = caps_ok && text && text_cap >= (uint64_t)LIST_LINE_MAX * N + L.host_bytes;
  const bool sized = nch <= 1 || !roomy || src.segments;  // (an image's records are validated before the first text byte)
  if (sized) {
    uint64_t dev_bytes = 0;
    for (size_t c = 0; c < nch; c++) {
      if ((r = known_lists_count(e, L, src, runs[c], d_rec.u8(), cnt, &chunk_bytes[c], nch <= 1))) return r;
      dev_bytes += chunk_bytes[c];
    }
    info->text_bytes = dev_bytes + L.host_bytes;
    if (!caps_ok || (info->text_bytes && (!text || text_cap < info->text_bytes)))
      return fail(e, CTMR_E_RANGE, "%s: %llu text bytes, %llu ID bytes and %llu offsets needed", src.what,
                  (unsigned long long)info->text_bytes, (unsigned long long)ids_bytes, (unsigned long long)(2 * (G + 1)));
  }
  // ---- write: chunk by chunk, each at its place among the host-store pieces
  std::vector<uint64_t> D(pts.size(), 0);  // the device text offset at each point
  size_t text_cap_dev = 0;
  uint64_t base = 0;
  auto splits = [&](uint64_t lo, uint64_t hi) {  // host pieces strictly inside records [lo, hi)
    const auto h = std::upper_bound(L.host.begin(), L.host.end(), lo, [](uint64_t v, const KnownLists::Host& x) { return v < x.rec; });
    return h != L.host.end() && h->rec < hi;
  };
  if (src.segments) {  // every buffer before the first text byte: the largest chunk that is staged as text
    for (size_t c = 0; c < nch; c++)
      if (!device || splits(runs[c].lo, runs[c].lo + runs[c].n)) text_cap_dev = std::max<size_t>(text_cap_dev, chunk_bytes[c]);
    if (text_cap_dev && d_text.alloc(text_cap_dev) != hipSuccess)
      return fail(e, CTMR_E_NOMEM, "%s: no device memory to stage %llu text bytes", src.what, (unsigned long long)text_cap_dev);
  }
  auto hb_le = [&](uint64_t rec) {  // host-store bytes of the pieces that go in at or before device record rec
    size_t k = std::upper_bound(L.host.begin(), L.host.end(), rec, [](uint64_t v, const KnownLists::Host& h) { return v < h.rec; }) - L.host.begin();
    return k ? L.host[k - 1].hb + L.host[k - 1].text.size() : 0ull;
  };
  for (size_t c = 0; c < nch; c++) {
    const uint64_t lo = runs[c].lo, n = runs[c].n, hi = lo + n, nb = runs[c].blocks();
    uint64_t bytes = chunk_bytes[c];
    if (nch > 1)  // (one chunk: still staged and scanned from the sizing pass)
      if ((r = known_lists_count(e, L, src, runs[c], d_rec.u8(), cnt, &bytes, true))) return r;
    const size_t p0 = std::lower_bound(pts.begin(), pts.end(), lo) - pts.begin();
    const size_t p1 = std::lower_bound(pts.begin(), pts.end(), hi) - pts.begin();
    std::vector<uint64_t> rel(p1 - p0);
    for (size_t k = p0; k < p1; k++) rel[k - p0] = pts[k] - lo;
    // host pieces strictly inside the chunk split its text: then it is staged and copied piece by piece
    const auto h0 = std::upper_bound(L.host.begin(), L.host.end(), lo, [](uint64_t v, const KnownLists::Host& h) { return v < h.rec; });
    const bool split = splits(lo, hi);
    uint8_t* dest;
    if (device && !split) {
      dest = text + base + hb_le(lo);
    } else {
      if (text_cap_dev < bytes) {
        if (d_text.alloc(bytes) != hipSuccess)
          return fail(e, CTMR_E_NOMEM, "%s: no device memory to stage %llu text bytes", src.what, (unsigned long long)bytes);
        text_cap_dev = bytes;
      }
      dest = d_text.u8();
    }
    uint64_t* d_pts = (uint64_t*)(tmp.u8() + off_pts);
    unsigned long long* d_po = (unsigned long long*)(tmp.u8() + off_po);
    if (!rel.empty()) HIPCHK(e, hipMemcpyAsync(d_pts, rel.data(), rel.size() * 8, hipMemcpyHostToDevice, e->stream));
    if (!src.segments)
      hipLaunchKernelGGL(k_lists_write, dim3((unsigned)nb), dim3(LIST_BLOCK), 0, e->stream, (const uint8_t*)d_rec.p, n,
                         (const unsigned long long*)cnt, dest, (const uint64_t*)d_pts, (uint64_t)rel.size(), d_po);
    else if (n)
      hipLaunchKernelGGL(k_image_lists_write, dim3((unsigned)nb), dim3(LIST_BLOCK), 0, e->stream, src.segs(runs[c].s_lo, runs[c].s_hi), n,
                         (const unsigned long long*)cnt, dest, (const uint64_t*)d_pts, (uint64_t)rel.size(), d_po);
    if (!rel.empty()) HIPCHK(e, hipMemcpyAsync(&D[p0], d_po, rel.size() * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipGetLastError());
    for (size_t k = p0; k < p1; k++) D[k] += base;
    if (!device || split) {  // the runs between host pieces, each to its place
      std::vector<uint64_t> cuts{lo};
      for (auto h = h0; h != L.host.end() && h->rec < hi; ++h)
        if (cuts.back() != h->rec) cuts.push_back(h->rec);
      cuts.push_back(hi);
      for (size_t k = 0; k + 1 < cuts.size(); k++) {
        auto Dat = [&](uint64_t p) -> uint64_t {
          if (p == lo) return base;
          if (p == hi) return base + bytes;
          return D[std::lower_bound(pts.begin(), pts.end(), p) - pts.begin()];
        };
        const uint64_t a = Dat(cuts[k]), b = Dat(cuts[k + 1]);
        if (b == a) continue;
        HIPCHK(e, hipMemcpyAsync(text + a + hb_le(cuts[k]), d_text.u8() + (a - base), b - a,
                                 device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, e->stream));
      }
      HIPCHK(e, hipStreamSynchronize(e->stream));
    }
    base += bytes;
  }
  const uint64_t total = base + L.host_bytes;
  info->text_bytes = total;
  for (size_t k = 0; k < pts.size(); k++)
    if (pts[k] == N) D[k] = base;  // points behind the last device record
  auto Dpt = [&](uint64_t p) { return D[std::lower_bound(pts.begin(), pts.end(), p) - pts.begin()]; };
  for (auto& h : L.host) {
    const uint64_t at = Dpt(h.rec) + h.hb;
    if (device) HIPCHK(e, hipMemcpyAsync(text + at, h.text.data(), h.text.size(), hipMemcpyHostToDevice, e->stream));
    else memcpy(text + at, h.text.data(), h.text.size());
  }
  uint64_t io = 0;
  for (uint64_t g = 0; g < G; g++) {
    offs[g] = Dpt(L.id_rec[g]) + L.id_hb[g];
    offs[G + 1 + g] = io;
    memcpy(ids + io, L.ids[g].data(), L.ids[g].size());
    io += L.ids[g].size();
  }
  offs[G] = total;
  offs[2 * G + 1] = io;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return CTMR_OK;
}

int known_lists_core(ctmr_engine* e, int64_t now, bool device, uint8_t* text, size_t text_cap, uint8_t* ids, size_t ids_cap,
                     uint64_t* offs, size_t offs_cap, ctmr_known_lists_info* info) {
  KnownLists L;
  int r;
  if ((r = known_lists_prepare(e, now, &L))) return r;
  return known_lists_emit(e, L, ListSource(), device, text, text_cap, ids, ids_cap, offs, offs_cap, info);
}

// The lists of an image whose meta is parsed and whose member records are on the device.
int image_lists_core(ctmr_engine* e, const KnownMeta& km, const uint8_t* d_members, int64_t now, bool device, uint8_t* text,
                     size_t text_cap, uint8_t* ids, size_t ids_cap, uint64_t* offs, size_t offs_cap, ctmr_known_lists_info* info) {
  ListSource src;
  src.what = "known image lists";
  int r;
  if ((r = known_bind(e, km, d_members, src.what))) return r;
  std::map<std::string, std::set<std::string>> host;
  KnownLists L;
  if ((r = image_lists_prepare(e, km, now, &host, &L))) return r;
  src.segments = true;
  src.image = d_members;
  if ((r = image_lists_upload(e, L, &src))) return r;
  return known_lists_emit(e, L, src, device, text, text_cap, ids, ids_cap, offs, offs_cap, info);
}

}  // namespace
}  // extern "C++"

int ctmr_known_lists(ctmr_engine* e, int64_t now_unix, uint8_t* text, size_t text_cap, uint8_t* ids, size_t ids_cap,
                     uint64_t* offs, size_t offs_cap, ctmr_known_lists_info* info) {
  if (!e || !info) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  return known_lists_core(e, now_unix, false, text, text_cap, ids, ids_cap, offs, offs_cap, info);
}

int ctmr_known_lists_device(ctmr_engine* e, int64_t now_unix, void* d_text, size_t text_cap, uint8_t* ids, size_t ids_cap,
                            uint64_t* offs, size_t offs_cap, ctmr_known_lists_info* info) {
  if (!e || !info) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  return known_lists_core(e, now_unix, true, (uint8_t*)d_text, text_cap, ids, ids_cap, offs, offs_cap, info);
}

int ctmr_known_image_lists(ctmr_engine* e, const uint8_t* image, size_t len, int64_t now_unix, uint8_t* text, size_t text_cap,
                           uint8_t* ids, size_t ids_cap, uint64_t* offs, size_t offs_cap, ctmr_known_lists_info* info) {
  if (!e || !image || !info) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  KnownMeta km;
  DevMem d;
  int r;
  if ((r = known_open(e, image, len, nullptr, "known image lists", &km))) return r;
  if ((r = known_stage_members(e, km, image, 0, "known image lists", &d))) return r;
  return image_lists_core(e, km, d.u8(), now_unix, false, text, text_cap, ids, ids_cap, offs, offs_cap, info);
}

int ctmr_known_image_lists_device(ctmr_engine* e, const uint8_t* meta, size_t meta_len, const void* d_members, uint64_t n_members,
                                  int64_t now_unix, void* d_text, size_t text_cap, uint8_t* ids, size_t ids_cap,
                                  uint64_t* offs, size_t offs_cap, ctmr_known_lists_info* info) {
  if (!e || !meta || !info) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  KnownMeta km;
  int r;
  if ((r = known_open(e, meta, meta_len, &n_members, "known image lists", &km))) return r;
  return image_lists_core(e, km, (const uint8_t*)d_members, now_unix, true, (uint8_t*)d_text, text_cap, ids, ids_cap, offs,
                          offs_cap, info);
}
