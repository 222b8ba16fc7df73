// engine/resp.inc — the Redis protocol stream of a known-certificate image (include/ctmr.h ctmr_known_image_resp*,
// DESIGN.md §18): the SADD commands of every serials:: key and the EXPIREAT KnownCertificates.setExpiryFlag puts on it
// (storage/knowncertificates.go), as `redis-cli --pipe` takes them.  The member records are turned into text where they
// lie by k_image_resp_count / k_image_resp_write (kernels/resp.h); the host section's keys are encoded here, one piece
// per key, and copied to their places between the sets.
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after engine/lists.inc.

extern "C++" {
namespace {

constexpr uint64_t RESP_CHUNK = 1ull << 27;  // member records per pass
constexpr uint32_t RESP_PER_MAX = 1u << 20;

void resp_bulk(const std::string& s, std::string* out) {
  char head[32];
  out->append(head, (size_t)snprintf(head, sizeof head, "$%zu\r\n", s.size()));
  out->append(s);
  out->append("\r\n");
}

void resp_array(size_t argc, std::string* out) {
  char head[32];
  out->append(head, (size_t)snprintf(head, sizeof head, "*%zu\r\n", argc));
}

// The commands of one host-section key: in front of the image's record `rec` (n_members: behind the last) and behind hb
// bytes of the pieces before it.
struct RespPiece { uint64_t rec, hb; std::string text; };

struct KnownResp {
  KnownExport x;                            // the sets as known_cut_sets takes them
  std::vector<unsigned long long> meta;     // per set, as RespArgs takes it
  std::vector<RespPiece> pieces;            // in key order
  uint64_t host_bytes = 0, host_commands = 0, host_keys = 0;  // host_keys: keys of the host section alone
};

std::string resp_set_key(const KnownMeta& km, uint64_t s) {
  return "serials::" + exp_date_id(km.set_hour[s]) + "::" + km.ids[km.set_issuer[s]];
}

int known_resp_prepare(ctmr_engine* e, const KnownMeta& km, uint32_t per, KnownResp* R) {
  const uint64_t S = km.n_sets;
  R->meta.resize(S);
  for (uint64_t s = 0; s < S; s++) {
    if (!hour_fixed(km.set_hour[s]))
      return fail(e, CTMR_E_INVAL, "known image resp: set %llu: hour %d lies outside the years 0000..9999", (unsigned long long)s,
                  km.set_hour[s]);
    R->meta[s] = (unsigned long long)(uint32_t)km.set_hour[s] | ((unsigned long long)km.set_issuer[s] << 32);
    R->x.set_range.push_back({km.set_first[s], km.set_first[s + 1] - km.set_first[s]});
  }
  R->x.info.members = km.n_members;
  uint64_t hb = 0;
  for (size_t a = 0; a < km.host.size();) {  // the host section is in (key, member) order: one run per key
    size_t b = a + 1;
    while (b < km.host.size() && km.host[b].first == km.host[a].first) b++;
    const std::string& key = km.host[a].first;
    // the first set whose key is not below this one (the sets ascend by key: known_parse_meta)
    uint64_t lo = 0, hi = S;
    while (lo < hi) {
      const uint64_t mid = (lo + hi) / 2;
      if (resp_set_key(km, mid) < key) lo = mid + 1;
      else hi = mid;
    }
    const bool both = lo < S && resp_set_key(km, lo) == key;
    RespPiece p{both ? km.set_first[lo + 1] : km.set_first[lo], hb, std::string()};
    for (size_t i = a; i < b; i += per) {
      const size_t m = std::min<size_t>(per, b - i);
      resp_array(m + 2, &p.text);
      resp_bulk("SADD", &p.text);
      resp_bulk(key, &p.text);
      for (size_t j = i; j < i + m; j++) resp_bulk(km.host[j].second, &p.text);
      R->host_commands++;
    }
    // EXPIREAT: the first second of the key's expDate — the set record's hour, or what NewExpDate makes of the text
    // between "serials::" and the next "::"; a key without one, or a date it cannot parse, gets none
    int64_t start = 0, end = 0;
    bool expire = both;
    if (both) {
      start = (int64_t)km.set_hour[lo] * 3600;
      R->meta[lo] |= RESP_NO_EXPIRE;
    } else {
      R->host_keys++;
      const size_t sep = key.find("::", 9);
      expire = sep != std::string::npos && lists_parse_date(key.substr(9, sep - 9), &start, &end);
    }
    if (expire) {
      resp_array(3, &p.text);
      resp_bulk("EXPIREAT", &p.text);
      resp_bulk(key, &p.text);
      resp_bulk(std::to_string((long long)start), &p.text);
      R->host_commands++;
    }
    hb += p.text.size();
    R->pieces.push_back(std::move(p));
    a = b;
  }
  R->host_bytes = hb;
  return CTMR_OK;
}

// The device side: first[S + 1], meta[S], the issuers' IDs, two words of the count pass (the error bits, the largest
// block's text), the per-block counts of the largest chunk and the points of the chunk with most, in one allocation.
struct RespDev {
  DevMem tmp;
  size_t off_meta = 0, off_ids = 0, off_err = 0, off_cnt = 0, off_pts = 0, off_po = 0;
  const uint8_t* members = nullptr;
  uint32_t per = 0;
  uint8_t* t8() const { return tmp.u8(); }
  uint32_t* err() const { return (uint32_t*)(t8() + off_err); }
  unsigned long long* cnt() const { return (unsigned long long*)(t8() + off_cnt); }
  uint64_t* pts() const { return (uint64_t*)(t8() + off_pts); }
  unsigned long long* pt_off() const { return (unsigned long long*)(t8() + off_po); }
  RespArgs args(const KnownRun& run) const {
    return RespArgs{members + run.lo * KNOWN_REC_BYTES, (const uint64_t*)t8() + run.s_lo,
                    (const unsigned long long*)(t8() + off_meta) + run.s_lo, t8() + off_ids, (uint32_t)(run.s_hi - run.s_lo), per};
  }
};

// The count pass over a run and its scan: cnt[] = the block offsets, *bytes = the text of the chunk,
// *max_block = the text of its largest block.
int known_resp_count(ctmr_engine* e, const RespDev& d, const KnownRun& run, uint64_t* bytes, uint32_t* max_block) {
  const uint64_t n = run.n, nb = run.blocks();
  int r;
  HIPCHK(e, hipMemsetAsync(d.cnt() + nb, 0, 8, e->stream));
  HIPCHK(e, hipMemsetAsync(d.err() + 1, 0, 4, e->stream));
  hipLaunchKernelGGL(k_image_resp_count, dim3((unsigned)nb), dim3(RESP_BLOCK), 0, e->stream, d.args(run), n, d.cnt(), d.err());
  if ((r = scan_u64(e, (uint64_t*)d.cnt(), nb + 1, false, SC_MISC))) return r;
  unsigned long long b = 0;
  uint32_t err[2] = {0u, 0u};  // the error bits, the largest block
  HIPCHK(e, hipMemcpyAsync(&b, d.cnt() + nb, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(err, d.err(), 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  *bytes = b;
  *max_block = err[1];
  return known_record_error(e, err[0], "known image resp");
}

// The stream of an image whose meta is parsed and whose member records are on the device.
int known_resp_core(ctmr_engine* e, const KnownMeta& km, const uint8_t* d_members, uint32_t per, bool device, uint8_t* text,
                    size_t text_cap, ctmr_known_resp_info* info) {
  const char* what = "known image resp";
  if (per < 1 || per > RESP_PER_MAX) return fail(e, CTMR_E_INVAL, "%s: %u members per command, 1..2^20 expected", what, per);
  int r;
  if ((r = known_bind(e, km, d_members, what))) return r;
  if (km.n_sets > 0xffffffffull) return fail(e, CTMR_E_NOMEM, "%s: %llu sets", what, (unsigned long long)km.n_sets);
  KnownResp R;
  if ((r = known_resp_prepare(e, km, per, &R))) return r;
  const uint64_t N = km.n_members, S = km.n_sets;
  memset(info, 0, sizeof *info);
  info->sets = S + R.host_keys;
  info->members = N;
  info->host_members = km.host.size();
  info->commands = R.host_commands;
  for (uint64_t s = 0; s < S; s++)
    info->commands += (R.x.set_range[s].second + per - 1) / per + ((R.meta[s] & RESP_NO_EXPIRE) ? 0 : 1);
  // chunks: the runs of whole sets (known_cut_sets)
  const std::vector<KnownRun> runs = known_cut_sets(R.x, known_chunk("CTMR_KNOWN_RESP_CHUNK", RESP_CHUNK));
  const size_t nch = runs.size();
  // points: the records in front of which host pieces go (ascending, unique); those strictly inside a chunk split its text
  std::vector<uint64_t> pts;
  for (auto& p : R.pieces)
    if (pts.empty() || pts.back() != p.rec) pts.push_back(p.rec);
  auto inner = [&](uint64_t lo, uint64_t hi, size_t* p0, size_t* p1) {
    *p0 = std::upper_bound(pts.begin(), pts.end(), lo) - pts.begin();
    *p1 = std::lower_bound(pts.begin(), pts.end(), hi) - pts.begin();
  };
  uint64_t max_n = 0;
  size_t max_pts = 0;
  for (size_t c = 0; c < nch; c++) {
    size_t p0, p1;
    inner(runs[c].lo, runs[c].lo + runs[c].n, &p0, &p1);
    max_n = std::max(max_n, runs[c].n);
    max_pts = std::max(max_pts, p1 - p0);
  }
  RespDev d;
  d.members = d_members;
  d.per = per;
  if (N) {
    const uint64_t nbmax = (max_n + RESP_BLOCK - 1) / RESP_BLOCK;
    d.off_meta = (S + 1) * 8;
    d.off_ids = (d.off_meta + S * 8 + 15) & ~(size_t)15;
    d.off_err = d.off_ids + (size_t)km.n_issuers * RESP_ID_ROW;
    d.off_cnt = d.off_err + 16;
    d.off_pts = d.off_cnt + (nbmax + 1) * 8;
    d.off_po = d.off_pts + max_pts * 8;
    const size_t tmp_bytes = d.off_po + max_pts * 8 + 8;
    if (d.tmp.alloc(tmp_bytes) != hipSuccess)
      return fail(e, CTMR_E_NOMEM, "%s: no device memory for the tables of %llu sets", what, (unsigned long long)S);
    std::vector<uint8_t> h(d.off_cnt, 0);
    memcpy(h.data(), km.set_first.data(), (S + 1) * 8);
    memcpy(h.data() + d.off_meta, R.meta.data(), S * 8);
    for (uint32_t k = 0; k < km.n_issuers; k++) memcpy(h.data() + d.off_ids + (size_t)k * RESP_ID_ROW, km.ids[k].data(), RESP_ID);
    HIPCHK(e, hipMemcpyAsync(d.t8(), h.data(), h.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));  // (h goes out of scope)
  }
  // ---- sizing: every chunk counted, and so validated, before the first text byte
  std::vector<uint64_t> chunk_bytes(nch, 0);
  uint64_t dev_bytes = 0;
  uint32_t max_block = 0;
  for (size_t c = 0; c < nch; c++) {
    if ((r = known_resp_count(e, d, runs[c], &chunk_bytes[c], &max_block))) return r;
    dev_bytes += chunk_bytes[c];
  }
  info->text_bytes = dev_bytes + R.host_bytes;
  if (info->text_bytes && (!text || text_cap < info->text_bytes))
    return fail(e, CTMR_E_RANGE, "%s: %llu text bytes needed", what, (unsigned long long)info->text_bytes);
  // … and every buffer: the largest chunk that is staged as text (the host variant's all, the device variant's split ones)
  DevMem d_text;
  size_t stage = 0;
  for (size_t c = 0; c < nch; c++) {
    size_t p0, p1;
    inner(runs[c].lo, runs[c].lo + runs[c].n, &p0, &p1);
    if (!device || p1 > p0) stage = std::max<size_t>(stage, chunk_bytes[c]);
  }
  if (stage && d_text.alloc(stage) != hipSuccess)
    return fail(e, CTMR_E_NOMEM, "%s: no device memory to stage %llu text bytes", what, (unsigned long long)stage);
  // ---- write: chunk by chunk, each run between two host pieces to its place
  auto hb_le = [&](uint64_t rec) {  // the bytes of the pieces that go in front of record rec or earlier
    const size_t k = std::upper_bound(R.pieces.begin(), R.pieces.end(), rec, [](uint64_t v, const RespPiece& p) { return v < p.rec; }) -
                     R.pieces.begin();
    return k ? R.pieces[k - 1].hb + R.pieces[k - 1].text.size() : 0ull;
  };
  std::vector<uint64_t> D(pts.size(), 0);  // the device text in front of each point
  uint64_t base = 0;
  for (size_t c = 0; c < nch; c++) {
    const uint64_t lo = runs[c].lo, n = runs[c].n, hi = lo + n, nb = runs[c].blocks();
    uint64_t bytes = chunk_bytes[c];
    if (nch > 1)  // (one chunk: cnt[] still holds the sizing pass's scan)
      if ((r = known_resp_count(e, d, runs[c], &bytes, &max_block))) return r;
    size_t p0, p1;
    inner(lo, hi, &p0, &p1);
    const bool split = p1 > p0;
    std::vector<uint64_t> rel(p1 - p0);
    for (size_t k = p0; k < p1; k++) rel[k - p0] = pts[k] - lo;
    if (split) HIPCHK(e, hipMemcpyAsync(d.pts(), rel.data(), rel.size() * 8, hipMemcpyHostToDevice, e->stream));
    uint8_t* dest = device && !split ? text + base + hb_le(lo) : d_text.u8();
    hipLaunchKernelGGL(k_image_resp_write, dim3((unsigned)nb), dim3(RESP_BLOCK), resp_lds_bytes(max_block), e->stream, d.args(runs[c]), n,
                       (const unsigned long long*)d.cnt(), dest, (const uint64_t*)d.pts(), (uint64_t)rel.size(), d.pt_off());
    if (split) HIPCHK(e, hipMemcpyAsync(&D[p0], d.pt_off(), rel.size() * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipGetLastError());
    if (!device || split) {
      uint64_t a = 0, at = lo;  // the run that starts at text offset a of the chunk, in front of record `at`
      for (size_t k = p0; k <= p1; k++) {
        const uint64_t b = k < p1 ? D[k] : bytes;
        if (b > a)
          HIPCHK(e, hipMemcpyAsync(text + base + a + hb_le(at), d_text.u8() + a, b - a,
                                   device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, e->stream));
        a = b;
        if (k < p1) at = pts[k];
      }
      HIPCHK(e, hipStreamSynchronize(e->stream));
    }
    for (size_t k = p0; k < p1; k++) D[k] += base;
    const size_t at_lo = std::lower_bound(pts.begin(), pts.end(), lo) - pts.begin();
    if (at_lo < pts.size() && pts[at_lo] == lo) D[at_lo] = base;
    base += bytes;
  }
  if (!pts.empty() && pts.back() == N) D.back() = base;  // pieces behind the last record
  for (auto& p : R.pieces) {
    const uint64_t at = D[std::lower_bound(pts.begin(), pts.end(), p.rec) - pts.begin()] + p.hb;
    if (device) HIPCHK(e, hipMemcpyAsync(text + at, p.text.data(), p.text.size(), hipMemcpyHostToDevice, e->stream));
    else memcpy(text + at, p.text.data(), p.text.size());
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return CTMR_OK;
}

}  // namespace
}  // extern "C++"

int ctmr_known_image_resp(ctmr_engine* e, const uint8_t* image, size_t len, uint32_t members_per_command, uint8_t* text,
                          size_t text_cap, ctmr_known_resp_info* info) {
  if (!e || !image || !info) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  KnownMeta km;
  DevMem d;
  int r;
  if ((r = known_open(e, image, len, nullptr, "known image resp", &km))) return r;
  if ((r = known_stage_members(e, km, image, 0, "known image resp", &d))) return r;
  return known_resp_core(e, km, d.u8(), members_per_command, false, text, text_cap, info);
}

int ctmr_known_image_resp_device(ctmr_engine* e, const uint8_t* meta, size_t meta_len, const void* d_members, uint64_t n_members,
                                 uint32_t members_per_command, void* d_text, size_t text_cap, ctmr_known_resp_info* info) {
  if (!e || !meta || !info) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  KnownMeta km;
  int r;
  if ((r = known_open(e, meta, meta_len, &n_members, "known image resp", &km))) return r;
  return known_resp_core(e, km, (const uint8_t*)d_members, members_per_command, true, (uint8_t*)d_text, text_cap, info);
}
