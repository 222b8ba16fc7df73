// engine/lists.inc — per-issuer known-serial lists (include/ctmr.h ctmr_known_lists*, DESIGN.md §13): for every Issuer.ID,
// the serials of its sets that have not expired, as the text LocalDiskBackend.StoreKnownCertificateList writes
// (storage/localdiskbackend.go).  The sets are chosen and ordered on the host (GetIssuerAndDatesFromCache, IsExpiredAt),
// their members staged with k_known_export (engine/image.inc) and turned into text by k_lists_count / k_lists_write.
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
  std::vector<std::string> ids;          // Issuer.ID of each list, bytewise ascending
  std::vector<uint64_t> id_rec, id_hb;   // per list: device records before it, host-store bytes before it
  struct Host { uint64_t rec, hb; std::string text; };  // the lines of one host-store key: after device record rec - 1
  std::vector<Host> host;                // ... and after hb bytes of host-store lines; in list order
  uint64_t host_bytes = 0, host_members = 0, sets = 0;
};

// Which sets, grouped and ordered: the pair table's sets and the host store's serials:: keys, kept while
// now < the end of their expDate; per Issuer.ID ascending, expDates ascending (by their first second, then as strings).
int known_lists_prepare(ctmr_engine* e, int64_t now, KnownLists* L) {
  struct Block { const std::set<std::string>* host = nullptr; };
  std::map<std::string, std::map<std::pair<int64_t, std::string>, Block>> by_id;  // the host-store keys
  for (auto& kv : e->hstore) {
    const std::string& k = kv.first;
    if (k.compare(0, 9, "serials::") != 0 || kv.second.empty()) continue;
    std::vector<std::string> parts;  // strings.Split(key, "::")
    for (size_t a = 0;;) {
      const size_t b = k.find("::", a);
      parts.push_back(k.substr(a, b == std::string::npos ? std::string::npos : b - a));
      if (b == std::string::npos) break;
      a = b + 2;
    }
    if (parts.size() != 3) return fail(e, CTMR_E_INVAL, "known lists: unexpected key format: %s", k.c_str());
    int64_t start, end;
    if (!lists_parse_date(parts[1], &start, &end) || now >= end) continue;  // unparsable: skipped, as the reference does
    by_id[parts[2]][{start, parts[1]}].host = &kv.second;
  }
  int r;
  std::vector<PairRec> pr;
  if ((r = list_pairs(e, &pr))) return r;
  // the device sets as integers: (rank of the issuer's ID, hour) — the per-set work of a table of many sets stays off
  // strings; an hour's ExpDate.ID is formatted only where a host-store key of the same issuer and second compares to it
  std::vector<uint32_t> by_rank, rank_of;
  issuers_by_id(e, &by_rank, &rank_of);
  struct Dev { uint64_t key, count, slot; };  // key = rank << 32 | (hour − KNOWN_HOUR_LO)
  std::vector<Dev> dev;
  for (auto& p : pr) {
    if (!hour_fixed(p.exp_hour) || now >= ((int64_t)p.exp_hour + 1) * 3600) continue;
    dev.push_back({((uint64_t)rank_of[p.canon] << 32) | (uint64_t)(p.exp_hour - KNOWN_HOUR_LO), p.count, p.slot});
  }
  std::sort(dev.begin(), dev.end(), [](const Dev& p, const Dev& q) { return p.key < q.key; });
  KnownExport& x = L->x;
  x.cursor.assign(e->npairs, KNOWN_CURSOR_OFF);  // sets not kept stay parked: their members are never written
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
    const std::string* dev_id = d < dev.size() ? &e->issuers[by_rank[dev[d].key >> 32]].id : nullptr;
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
        x.cursor[dev[d].slot] = rec;
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

// Device records [lo, hi) of the list order, staged and counted: *bytes = their text, cnt[] their block offsets.
// ordered: as known_export_members takes it (the text's size does not depend on the order).
int known_lists_count(ctmr_engine* e, KnownLists& L, size_t s_lo, size_t s_hi, uint8_t* d_rec, unsigned long long* cnt,
                      uint64_t* bytes, bool ordered) {
  int r;
  if ((r = known_export_members(e, L.x, s_lo, s_hi, d_rec, ordered))) return r;
  const uint64_t n = L.x.first(s_hi) - L.x.first(s_lo), nb = (n + LIST_BLOCK - 1) / LIST_BLOCK;
  HIPCHK(e, hipMemsetAsync(cnt + nb, 0, 8, e->stream));
  hipLaunchKernelGGL(k_lists_count, dim3((unsigned)nb), dim3(LIST_BLOCK), 0, e->stream, (const uint8_t*)d_rec, n, cnt);
  if ((r = scan_u64(e, (uint64_t*)cnt, nb + 1, false, SC_MISC))) return r;
  unsigned long long b;
  HIPCHK(e, hipMemcpyAsync(&b, cnt + nb, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  *bytes = b;
  return CTMR_OK;
}

int known_lists_core(ctmr_engine* e, int64_t now, bool device, uint8_t* text, size_t text_cap, uint8_t* ids, size_t ids_cap,
                     uint64_t* offs, size_t offs_cap, ctmr_known_lists_info* info) {
  KnownLists L;
  int r;
  if ((r = known_lists_prepare(e, now, &L))) return r;
  const uint64_t N = L.x.info.members, G = L.ids.size();
  uint64_t ids_bytes = 0;
  for (auto& s : L.ids) ids_bytes += s.size();
  memset(info, 0, sizeof *info);
  info->issuers = G;
  info->sets = L.sets;
  info->members = N;
  info->host_members = L.host_members;
  info->ids_bytes = ids_bytes;
  // chunks: runs of whole sets of at most `chunk` records (a larger set alone); the test-only override forces small ones
  const uint64_t forced = env_u64("CTMR_KNOWN_LISTS_CHUNK");
  const std::vector<size_t> cut = known_cut_sets(L.x, forced ? forced : LISTS_CHUNK);  // set index at each chunk start, then the end
  const size_t nch = cut.size() - 1;
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
    const uint64_t lo = L.x.first(cut[c]), hi = L.x.first(cut[c + 1]);
    max_n = std::max(max_n, hi - lo);
    max_pts = std::max(max_pts, (size_t)(std::lower_bound(pts.begin(), pts.end(), hi) - std::lower_bound(pts.begin(), pts.end(), lo)));
  }
  DevMem d_rec, tmp, d_text;
  const uint64_t nbmax = (max_n + LIST_BLOCK - 1) / LIST_BLOCK;
  const size_t off_pts = (nbmax + 1) * 8, off_po = off_pts + max_pts * 8;
  if (N && (d_rec.alloc(max_n * KNOWN_REC_BYTES) != hipSuccess || tmp.alloc(off_po + max_pts * 8 + 8) != hipSuccess))
    return fail(e, CTMR_E_NOMEM, "known lists: no device memory to stage %llu member records", (unsigned long long)max_n);
  unsigned long long* cnt = (unsigned long long*)tmp.p;
  std::vector<uint64_t> chunk_bytes(nch, ~0ull);
  // sizing: one count pass over every chunk, unless every buffer holds its bound (81 B per member for the text) and
  // the pass that writes can size as it goes; a single chunk is staged once either way
  const bool caps_ok = (!G || (ids && ids_cap >= ids_bytes)) && offs && offs_cap >= 2 * (G + 1);
  const bool roomy = caps_ok && text && text_cap >= (uint64_t)LIST_LINE_MAX * N + L.host_bytes;
  const bool sized = nch <= 1 || !roomy;
  if (sized) {
    uint64_t dev_bytes = 0;
    for (size_t c = 0; c < nch; c++) {
      if ((r = known_lists_count(e, L, cut[c], cut[c + 1], d_rec.u8(), cnt, &chunk_bytes[c], nch <= 1))) return r;
      dev_bytes += chunk_bytes[c];
    }
    info->text_bytes = dev_bytes + L.host_bytes;
    if (!caps_ok || (info->text_bytes && (!text || text_cap < info->text_bytes)))
      return fail(e, CTMR_E_RANGE, "known lists: %llu text bytes, %llu ID bytes and %llu offsets needed",
                  (unsigned long long)info->text_bytes, (unsigned long long)ids_bytes, (unsigned long long)(2 * (G + 1)));
  }
  // ---- write: chunk by chunk, each at its place among the host-store pieces
  std::vector<uint64_t> D(pts.size(), 0);  // the device text offset at each point
  size_t text_cap_dev = 0;
  uint64_t base = 0;
  auto hb_le = [&](uint64_t rec) {  // host-store bytes of the pieces that go in at or before device record rec
    size_t k = std::upper_bound(L.host.begin(), L.host.end(), rec, [](uint64_t v, const KnownLists::Host& h) { return v < h.rec; }) - L.host.begin();
    return k ? L.host[k - 1].hb + L.host[k - 1].text.size() : 0ull;
  };
  for (size_t c = 0; c < nch; c++) {
    const uint64_t lo = L.x.first(cut[c]), hi = L.x.first(cut[c + 1]);
    uint64_t bytes = chunk_bytes[c];
    if (nch > 1)  // (one chunk: still staged and scanned from the sizing pass)
      if ((r = known_lists_count(e, L, cut[c], cut[c + 1], d_rec.u8(), cnt, &bytes, true))) return r;
    const size_t p0 = std::lower_bound(pts.begin(), pts.end(), lo) - pts.begin();
    const size_t p1 = std::lower_bound(pts.begin(), pts.end(), hi) - pts.begin();
    std::vector<uint64_t> rel(p1 - p0);
    for (size_t k = p0; k < p1; k++) rel[k - p0] = pts[k] - lo;
    // host pieces strictly inside the chunk split its text: then it is staged and copied piece by piece
    const auto h0 = std::upper_bound(L.host.begin(), L.host.end(), lo, [](uint64_t v, const KnownLists::Host& h) { return v < h.rec; });
    const bool split = h0 != L.host.end() && h0->rec < hi;
    uint8_t* dest;
    if (device && !split) {
      dest = text + base + hb_le(lo);
    } else {
      if (text_cap_dev < bytes) {
        if (d_text.alloc(bytes) != hipSuccess)
          return fail(e, CTMR_E_NOMEM, "known lists: no device memory to stage %llu text bytes", (unsigned long long)bytes);
        text_cap_dev = bytes;
      }
      dest = d_text.u8();
    }
    uint64_t* d_pts = (uint64_t*)(tmp.u8() + off_pts);
    unsigned long long* d_po = (unsigned long long*)(tmp.u8() + off_po);
    if (!rel.empty()) HIPCHK(e, hipMemcpyAsync(d_pts, rel.data(), rel.size() * 8, hipMemcpyHostToDevice, e->stream));
    const uint64_t n = hi - lo, nb = (n + LIST_BLOCK - 1) / LIST_BLOCK;
    hipLaunchKernelGGL(k_lists_write, dim3((unsigned)nb), dim3(LIST_BLOCK), 0, e->stream, (const uint8_t*)d_rec.p, n,
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
