// engine/image.inc — the known-certificate image: bulk export and import of the serials:: sets (include/ctmr.h,
// DESIGN.md §12).  What a restart of a reference deployment finds still in Redis, carried across a restart of the engine.
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after the engine state.

extern "C++" {
namespace {

constexpr char KNOWN_MAGIC[8] = {'C', 'T', 'M', 'R', 'K', 'N', 'W', 'N'};
constexpr uint32_t KNOWN_VERSION = 1, KNOWN_HEADER = 64;
constexpr uint64_t KNOWN_CHUNK = 1ull << 27;  // import: records per pass (32-bit orders and slot ids, bounded scratch)

struct KnownMeta {
  uint32_t n_issuers = 0;
  uint64_t n_sets = 0, n_members = 0, host_bytes = 0, n_host_members = 0, meta_bytes = 0;
  const uint8_t* issuers = nullptr;  // n_issuers × 32
  const uint8_t* sets = nullptr;     // n_sets × 24
  std::vector<std::string> ids;      // Issuer.ID of each ordinal
  std::vector<int32_t> set_hour;
  std::vector<uint32_t> set_issuer;
  std::vector<uint64_t> set_first;   // n_sets + 1
  std::vector<std::pair<std::string, std::string>> host;  // (key, member)
};

// Hours whose ExpDate.ID has four year digits (0000-01-01-00 .. 9999-12-31-23): there the keys serials::<date>::<id>
// order as (hour, id) do — the date part is fixed-width and chronological.  Other hours compare as strings.
const int64_t KNOWN_HOUR_LO = days_from_civil(0, 1, 1) * 24, KNOWN_HOUR_HI = days_from_civil(10000, 1, 1) * 24;
bool hour_fixed(int32_t h) { return h >= KNOWN_HOUR_LO && h < KNOWN_HOUR_HI; }
bool key_less(int32_t ha, const std::string& ia, int32_t hb, const std::string& ib) {
  if (hour_fixed(ha) && hour_fixed(hb)) return ha != hb ? ha < hb : ia < ib;
  return "serials::" + exp_date_id(ha) + "::" + ia < "serials::" + exp_date_id(hb) + "::" + ib;
}

uint64_t rd64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }
uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
void put64(std::vector<uint8_t>& o, uint64_t v) { o.insert(o.end(), (const uint8_t*)&v, (const uint8_t*)&v + 8); }
void put32(std::vector<uint8_t>& o, uint32_t v) { o.insert(o.end(), (const uint8_t*)&v, (const uint8_t*)&v + 4); }

// the member record of a member of at most 40 octets, appended to *out: u64 serial_len, the octets, zeros to 48 bytes
void known_put_record(const std::string& m, std::vector<uint8_t>* out) {
  const uint64_t len = m.size();
  const size_t at = out->size();
  out->resize(at + KNOWN_REC_BYTES, 0);
  memcpy(&(*out)[at], &len, 8);
  memcpy(&(*out)[at + 8], m.data(), m.size());
}

// The meta part of an image (header, issuers, sets, host section, padding): every check but the member records' own,
// which the count pass makes on the device.  len = the meta part's length (device variant) or the whole image's.
int known_parse_meta(ctmr_engine* e, const uint8_t* m, size_t len, bool whole, KnownMeta* km) {
  if (!m || len < KNOWN_HEADER) return fail(e, CTMR_E_INVAL, "known image: shorter than its header");
  if (memcmp(m, KNOWN_MAGIC, 8) != 0) return fail(e, CTMR_E_INVAL, "known image: bad magic");
  if (rd32(m + 8) != KNOWN_VERSION) return fail(e, CTMR_E_INVAL, "known image: version %u, expected 1", rd32(m + 8));
  if (rd32(m + 12) != KNOWN_HEADER || rd32(m + 20) != 0 || rd64(m + 56) != 0)
    return fail(e, CTMR_E_INVAL, "known image: header size, flags or reserved field");
  km->n_issuers = rd32(m + 16);
  km->n_sets = rd64(m + 24);
  km->n_members = rd64(m + 32);
  km->host_bytes = rd64(m + 40);
  km->n_host_members = rd64(m + 48);
  const uint64_t L = len;
  if (km->n_sets > L / 24 || km->host_bytes > L || km->n_members > (1ull << 56) / KNOWN_REC_BYTES)
    return fail(e, CTMR_E_INVAL, "known image: section sizes disagree with its length");
  const uint64_t content = KNOWN_HEADER + (uint64_t)km->n_issuers * 32 + km->n_sets * 24 + km->host_bytes;
  km->meta_bytes = (content + 63) & ~63ull;
  const uint64_t want = whole ? km->meta_bytes + km->n_members * KNOWN_REC_BYTES : km->meta_bytes;
  if (want != L) return fail(e, CTMR_E_INVAL, "known image: %llu bytes, the header says %llu", (unsigned long long)L,
                             (unsigned long long)want);
  for (uint64_t p = content; p < km->meta_bytes; p++)
    if (m[p]) return fail(e, CTMR_E_INVAL, "known image: padding before the members is not zero");
  km->issuers = m + KNOWN_HEADER;
  km->sets = km->issuers + (size_t)km->n_issuers * 32;
  std::vector<std::string>& ids = km->ids;
  ids.resize(km->n_issuers);
  for (uint32_t k = 0; k < km->n_issuers; k++) ids[k] = b64url(km->issuers + (size_t)k * 32, 32);
  km->set_hour.resize(km->n_sets);
  km->set_issuer.resize(km->n_sets);
  km->set_first.resize(km->n_sets + 1);
  uint64_t at = 0;
  for (uint64_t s = 0; s < km->n_sets; s++) {
    const uint8_t* p = km->sets + s * 24;
    const int32_t eh = (int32_t)rd32(p);
    const uint32_t ord = rd32(p + 4);
    const uint64_t first = rd64(p + 8), count = rd64(p + 16);
    if (ord >= km->n_issuers) return fail(e, CTMR_E_INVAL, "known image: set %llu names issuer %u of %u", (unsigned long long)s, ord, km->n_issuers);
    if (first != at || count == 0 || count > km->n_members - at)
      return fail(e, CTMR_E_INVAL, "known image: set %llu does not follow its predecessor (gap, overlap or empty)", (unsigned long long)s);
    if (s && !key_less(km->set_hour[s - 1], ids[km->set_issuer[s - 1]], eh, ids[ord]))
      return fail(e, CTMR_E_INVAL, "known image: sets out of key order");
    km->set_hour[s] = eh;
    km->set_issuer[s] = ord;
    km->set_first[s] = first;
    at += count;
  }
  km->set_first[km->n_sets] = at;
  if (at != km->n_members) return fail(e, CTMR_E_INVAL, "known image: the sets cover %llu of %llu members", (unsigned long long)at,
                                       (unsigned long long)km->n_members);
  const uint8_t* h = km->sets + km->n_sets * 24;
  uint64_t q = 0;
  while (q < km->host_bytes) {
    if (km->host_bytes - q < 4) return fail(e, CTMR_E_INVAL, "known image: host section truncated");
    const uint32_t kl = rd32(h + q);
    if (km->host_bytes - q - 4 < (uint64_t)kl + 4) return fail(e, CTMR_E_INVAL, "known image: host section truncated");
    std::string key((const char*)h + q + 4, kl);
    q += 4 + kl;
    const uint32_t ml = rd32(h + q);
    if (km->host_bytes - q - 4 < ml) return fail(e, CTMR_E_INVAL, "known image: host section truncated");
    std::string mem((const char*)h + q + 4, ml);
    q += 4 + ml;
    if (key.compare(0, 9, "serials::") != 0) return fail(e, CTMR_E_INVAL, "known image: a host-section key outside serials::");
    if (!km->host.empty() && !(km->host.back() < std::make_pair(key, mem)))
      return fail(e, CTMR_E_INVAL, "known image: host section out of (key, member) order");
    km->host.emplace_back(std::move(key), std::move(mem));
  }
  if (km->host.size() != km->n_host_members) return fail(e, CTMR_E_INVAL, "known image: host section holds %llu members, the header says %llu",
                                                         (unsigned long long)km->host.size(), (unsigned long long)km->n_host_members);
  return CTMR_OK;
}

// The one writer of what known_parse_meta reads: the meta part of the image whose issuers are `digs` (32 bytes each, in
// ordinal order), whose sets are `sets` (in key order; each set's first member is worked out here) and whose host
// section is `host` (in (key, member) order) → *meta, padded to 64 bytes, and *info (an image's, or a longer struct
// that begins as it does).
struct KnownSetEntry { int32_t hour; uint32_t ordinal; uint64_t count; };
using KnownHostPairs = std::vector<std::pair<std::string, std::string>>;

// What its callers do before it.  Issuers: the digests the sets name (32 bytes each, any order, repeats) → the distinct
// ones ascending, which is their ordinal order, and a digest's ordinal among them.  Host section: the pairs as found →
// in order, each once.
void known_number_digests(std::vector<const uint8_t*>* digs) {
  std::sort(digs->begin(), digs->end(), [](const uint8_t* x, const uint8_t* y) { return memcmp(x, y, 32) < 0; });
  digs->erase(std::unique(digs->begin(), digs->end(), [](const uint8_t* x, const uint8_t* y) { return memcmp(x, y, 32) == 0; }), digs->end());
}

uint32_t known_digest_ordinal(const std::vector<const uint8_t*>& digs, const uint8_t* d) {
  return (uint32_t)(std::lower_bound(digs.begin(), digs.end(), d, [](const uint8_t* x, const uint8_t* y) { return memcmp(x, y, 32) < 0; }) - digs.begin());
}

void known_finish_pairs(KnownHostPairs* host) {
  std::sort(host->begin(), host->end());
  host->erase(std::unique(host->begin(), host->end()), host->end());
}

template <class Info>
void known_write_meta(const std::vector<const uint8_t*>& digs, const std::vector<KnownSetEntry>& sets, const KnownHostPairs& host,
                      std::vector<uint8_t>* meta, Info* info) {
  uint64_t n_members = 0, host_bytes = 0;
  for (auto& s : sets) n_members += s.count;
  for (auto& hm : host) host_bytes += 8 + hm.first.size() + hm.second.size();
  std::vector<uint8_t>& o = *meta;
  o.reserve(((KNOWN_HEADER + digs.size() * 32 + sets.size() * 24 + host_bytes + 63) & ~(size_t)63));
  o.assign(KNOWN_MAGIC, KNOWN_MAGIC + 8);
  put32(o, KNOWN_VERSION);
  put32(o, KNOWN_HEADER);
  put32(o, (uint32_t)digs.size());
  put32(o, 0);
  put64(o, sets.size());
  put64(o, n_members);
  put64(o, host_bytes);
  put64(o, host.size());
  put64(o, 0);
  for (const uint8_t* d : digs) o.insert(o.end(), d, d + 32);
  {  // the set records in one piece: an image has many (a field-by-field append cost 19 ms for 0.55 M sets)
    const size_t at = o.size();
    o.resize(at + sets.size() * 24);
    uint8_t* p = o.data() + at;
    uint64_t first = 0;
    for (auto& s : sets) {
      const uint32_t w[2] = {(uint32_t)s.hour, s.ordinal};
      const uint64_t q[2] = {first, s.count};
      memcpy(p, w, 8);
      memcpy(p + 8, q, 16);
      p += 24;
      first += s.count;
    }
  }
  for (auto& hm : host) {
    put32(o, (uint32_t)hm.first.size());
    o.insert(o.end(), hm.first.begin(), hm.first.end());
    put32(o, (uint32_t)hm.second.size());
    o.insert(o.end(), hm.second.begin(), hm.second.end());
  }
  o.resize((o.size() + 63) & ~(size_t)63, 0);
  info->members = n_members;
  info->sets = sets.size();
  info->host_members = host.size();
  info->meta_bytes = o.size();
  info->image_bytes = o.size() + n_members * KNOWN_REC_BYTES;
  info->issuers = (uint32_t)digs.size();
  info->reserved = 0;
}

// What an entry point is given, step 1: the meta part parsed and, for the device variants (n_given: their record
// count), held against the header.  `what` names the call in the message.
int known_open(ctmr_engine* e, const uint8_t* m, size_t len, const uint64_t* n_given, const char* what, KnownMeta* km) {
  int r;
  if ((r = known_parse_meta(e, m, len, !n_given, km))) return r;
  if (n_given && km->n_members != *n_given)
    return fail(e, CTMR_E_INVAL, "%s: %llu member records given, the header says %llu", what, (unsigned long long)*n_given,
                (unsigned long long)km->n_members);
  return CTMR_OK;
}

// Step 2, where the call's own checks have it today: the member records a core works on are there.  The host variants
// have staged theirs by then (known_stage_members), so this refuses the device variants' null pointer.
int known_bind(ctmr_engine* e, const KnownMeta& km, const uint8_t* d_members, const char* what) {
  if (km.n_members && !d_members) return fail(e, CTMR_E_INVAL, "%s: null member records", what);
  return CTMR_OK;
}

// Export, host side: the sets in key order with their first members, the issuers they name, the host section.
struct KnownExport {
  std::vector<uint8_t> meta;
  std::vector<unsigned long long> cursor;   // per pair-table slot: the first member of its set
  std::vector<std::pair<uint64_t, uint64_t>> set_range;  // (first, count) in key order
  ctmr_known_image_info info{};
  // the first record of set s, or info.members past the last set
  uint64_t first(size_t s) const { return s < set_range.size() ? set_range[s].first : info.members; }
};

// The runs of a call, the one copy of the image's calls (DESIGN.md §12): the sets cut into runs of whole sets of at most
// `limit` records, a larger set standing alone.  A run is the sets [s_lo, s_hi): n records from record `lo` on, which
// a launch of one lane per record takes as blocks() blocks of 256 — blk0 of them lie in front of it in the runs before
// (where a call numbers its blocks through all its runs: kernels/image.h, KnownFlags).
struct KnownRun {
  size_t s_lo, s_hi;
  uint64_t lo, n, blk0;
  uint64_t blocks() const { return (n + 255) / 256; }
};

std::vector<KnownRun> known_cut_sets(const KnownExport& x, uint64_t limit) {
  std::vector<KnownRun> runs;
  uint64_t blk0 = 0;
  for (size_t s = 0; s < x.set_range.size();) {
    size_t t = s + 1;
    while (t < x.set_range.size() && x.first(t + 1) - x.first(s) <= limit) t++;
    runs.push_back(KnownRun{s, t, x.first(s), x.first(t) - x.first(s), blk0});
    blk0 += runs.back().blocks();
    s = t;
  }
  return runs;
}

// the blocks of all runs
uint64_t known_runs_blocks(const std::vector<KnownRun>& runs) { return runs.empty() ? 0 : runs.back().blk0 + runs.back().blocks(); }

// The call's chunk, records per run: the override `name` (a CTMR_*_CHUNK variable, tests only: it forces several small
// runs), else the call's default.
uint64_t known_chunk(const char* name, uint64_t dflt) {
  const uint64_t v = env_u64(name);
  return v && v < dflt ? v : dflt;
}

// The device tables of one call, packed into one upload: every piece 16-byte aligned.
struct KnownPack {
  std::vector<uint8_t> b;
  size_t put(const void* p, size_t n) {
    const size_t at = (b.size() + 15) & ~(size_t)15;
    b.resize(at + n);
    if (n) memcpy(&b[at], p, n);
    return at;
  }
  template <class T> size_t put(const std::vector<T>& v) { return put(v.data(), v.size() * sizeof(T)); }
  // the error word of the call's kernels (kernels/image.h: known_report_bad), zeroed, behind what was put so far
  size_t put_err() {
    const size_t at = put(nullptr, 0);
    b.resize(at + 16, 0);
    return at;
  }
};

// The calls that read member records with 16-byte loads from wherever the caller has them refuse other addresses
// (ptrs: the call's device pointers or-ed together).
int known_aligned16(ctmr_engine* e, uintptr_t ptrs, const char* what) {
  if (ptrs & 15u) return fail(e, CTMR_E_INVAL, "%s: device memory that is not 16-byte aligned", what);
  return CTMR_OK;
}

int known_export_prepare(ctmr_engine* e, KnownExport* x) {
  int r;
  std::vector<PairRec> sets;
  if ((r = list_pairs(e, &sets))) return r;
  // key order: (hour, rank of the Issuer.ID) as one integer when every hour has a four-digit year, else the strings
  std::vector<uint32_t> by_id, id_rank;
  issuers_by_id(e, &by_id, &id_rank);
  bool fixed = true;
  for (auto& s : sets) fixed = fixed && hour_fixed(s.exp_hour);
  if (fixed) {
    std::vector<std::pair<uint64_t, uint32_t>> ord(sets.size());
    for (uint32_t k = 0; k < sets.size(); k++)
      ord[k] = {((uint64_t)(sets[k].exp_hour - KNOWN_HOUR_LO) << 24) | id_rank[sets[k].canon], k};
    std::sort(ord.begin(), ord.end());
    std::vector<PairRec> sorted(sets.size());
    for (size_t k = 0; k < ord.size(); k++) sorted[k] = sets[ord[k].second];
    sets.swap(sorted);
  } else {
    std::sort(sets.begin(), sets.end(), [e](const PairRec& a, const PairRec& b) {
      return key_less(a.exp_hour, e->issuers[a.canon].id, b.exp_hour, e->issuers[b.canon].id);
    });
  }
  // issuer ordinals: the referenced issuers in digest order (process-independent, like the digests themselves)
  std::vector<uint32_t> canons;
  for (auto& s : sets) canons.push_back(s.canon);
  std::sort(canons.begin(), canons.end());
  canons.erase(std::unique(canons.begin(), canons.end()), canons.end());
  std::sort(canons.begin(), canons.end(), [e](uint32_t a, uint32_t b) { return memcmp(e->issuers[a].digest, e->issuers[b].digest, 32) < 0; });
  std::vector<uint32_t> ordinal(e->issuers.size(), 0);
  for (uint32_t k = 0; k < canons.size(); k++) ordinal[canons[k]] = k;
  KnownHostPairs host;
  for (auto& kv : e->hstore)
    if (kv.first.compare(0, 9, "serials::") == 0)
      for (auto& m : kv.second) host.emplace_back(kv.first, m);
  std::vector<const uint8_t*> digs;
  for (uint32_t c : canons) digs.push_back(e->issuers[c].digest);
  std::vector<KnownSetEntry> entries;
  x->cursor.assign(e->npairs, 0ull);
  uint64_t first = 0;
  for (auto& s : sets) {
    entries.push_back({s.exp_hour, ordinal[s.canon], s.count});
    x->cursor[s.slot] = first;
    x->set_range.push_back({first, s.count});
    first += s.count;
  }
  known_write_meta(digs, entries, host, &x->meta, &x->info);
  return CTMR_OK;
}

int known_sort_sets(ctmr_engine* e, uint8_t* d_rec, const std::vector<uint64_t>& first);  // engine/sort.inc

// Export, device side: the member records of sets [s_lo, s_hi) into out (positions relative to the first of s_lo).
// ordered: under CTMR_KNOWN_ORDER_SORTED each set's records are sorted where they were staged (a caller that only
// counts bytes passes false).
int known_export_members(ctmr_engine* e, KnownExport& x, size_t s_lo, size_t s_hi, uint8_t* d_out, bool ordered = true) {
  const uint64_t lo = x.first(s_lo), hi = x.first(s_hi);
  if (hi == lo) return CTMR_OK;
  // sets outside [lo, hi) get a cursor far above the chunk: their members are counted but not written (the slots of no
  // set are never reached by a live cell)
  std::vector<unsigned long long> cur(x.cursor.size(), KNOWN_CURSOR_OFF);
  for (size_t j = 0; j < x.cursor.size(); j++)
    if (x.cursor[j] >= lo && x.cursor[j] < hi) cur[j] = x.cursor[j] - lo;
  int r;
  if ((r = ensure(e, SC_TMP, cur.size() * 8))) return r;
  HIPCHK(e, hipMemcpyAsync(e->d_scratch[SC_TMP], cur.data(), cur.size() * 8, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_known_export, dim3((unsigned)((e->nslots + 255) / 256)), dim3(256), 0, e->stream, e->tbl(), e->nslots,
                     (const PairSlot*)e->pairs, e->npairs - 1, (unsigned long long*)e->d_scratch[SC_TMP], d_out, hi - lo);
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  if (ordered && e->known_order == CTMR_KNOWN_ORDER_SORTED) {
    std::vector<uint64_t> first(s_hi - s_lo + 1);
    for (size_t s = s_lo; s <= s_hi; s++) first[s - s_lo] = x.first(s) - lo;
    return known_sort_sets(e, d_out, first);
  }
  return CTMR_OK;
}

// What the kernels' error word says about the member records (kernels/image.h: KnownImportArgs.err).
int known_record_error(ctmr_engine* e, uint32_t err, const char* what) {
  if (err & 1u) return fail(e, CTMR_E_INVAL, "%s: a member record's serial_len is above %d", what, CTMR_MAX_SERIAL);
  if (err) return fail(e, CTMR_E_INVAL, "%s: a member record's padding octets are not zero", what);
  return CTMR_OK;
}

// What import, query and remove share in front of the member records: the call's checks (`what` names it in messages),
// the image's issuer ordinals mapped to canonical indices here, and per set the key meta (0: issuer not registered — the
// host side takes the set, world = 1 only).
struct KnownSets {
  std::vector<unsigned long long> set_meta;
  std::vector<size_t> unreg;
  uint64_t unreg_members = 0;
};

int known_sets_prepare(ctmr_engine* e, const KnownMeta& km, const uint8_t* d_members, uint32_t world, uint32_t rank,
                       const char* what, KnownSets* ks) {
  if (world == 0 || rank >= world) return fail(e, CTMR_E_INVAL, "%s: rank %u of world %u", what, rank, world);
  if (e->rd.valid && e->rd.mode == XM_OWNER && !e->rd.resolved)
    return fail(e, CTMR_E_INVAL, "%s: an owner-computes round is open on this engine", what);
  int r;
  if ((r = known_bind(e, km, d_members, what))) return r;
  // image issuer ordinal → canonical index here (0xffffffff: not registered)
  std::vector<uint32_t> remap(km.n_issuers, 0xffffffffu);
  for (uint32_t k = 0; k < km.n_issuers; k++) {
    auto it = e->id_to_canon.find(b64url(km.issuers + (size_t)k * 32, 32));
    if (it != e->id_to_canon.end()) remap[k] = it->second;
  }
  ks->set_meta.resize(km.n_sets);
  for (uint64_t s = 0; s < km.n_sets; s++) {
    const uint32_t c = remap[km.set_issuer[s]];
    if (c == 0xffffffffu) {
      ks->unreg.push_back(s);
      ks->unreg_members += km.set_first[s + 1] - km.set_first[s];
      ks->set_meta[s] = 0ull;
    } else {
      ks->set_meta[s] = key_meta(km.set_hour[s], c, 0);
    }
  }
  if (world > 1 && !ks->unreg.empty())
    return fail(e, CTMR_E_INVAL, "%s: world %u needs every set's issuer registered (%zu sets are not)", what, world,
                ks->unreg.size());
  return CTMR_OK;
}

// The device side of the same: set_first[] and set_meta[], the per-block counts of a chunk of at most `chunk` records,
// the error word and a DevStats, in one allocation; args(c) describes chunk c to the kernels of kernels/image.h.
struct KnownDev {
  DevMem tmp;
  size_t off_meta = 0, off_cnt = 0, off_err = 0, off_stats = 0;
  uint64_t n = 0, chunk = 0, nch = 0, nbmax = 0;
  const uint8_t* members = nullptr;
  uint32_t n_sets = 0, world = 1, rank = 0;
  uint8_t* t8() const { return tmp.u8(); }
  uint32_t* err() const { return (uint32_t*)(t8() + off_err); }
  DevStats* stats() const { return (DevStats*)(t8() + off_stats); }
  KnownImportArgs args(uint64_t c) const {
    KnownImportArgs a{};
    const uint64_t lo = c * chunk, cn = std::min(n - lo, chunk);
    a.members = members + lo * KNOWN_REC_BYTES; a.n = cn; a.base = lo;
    a.set_first = (const uint64_t*)t8(); a.set_meta = (const unsigned long long*)(t8() + off_meta);
    a.n_sets = n_sets; a.world = world; a.rank = rank;
    a.cnt = (unsigned long long*)(t8() + off_cnt); a.nb = (cn + 255) / 256; a.err = err();
    return a;
  }
};

int known_dev_upload(ctmr_engine* e, const KnownMeta& km, const KnownSets& ks, const uint8_t* d_members, uint32_t world,
                     uint32_t rank, uint64_t chunk, KnownDev* kd) {
  const uint64_t N = km.n_members, CH = N < chunk ? N : chunk;
  kd->n = N; kd->chunk = chunk; kd->nch = (N + chunk - 1) / chunk; kd->nbmax = (CH + 255) / 256;
  kd->members = d_members; kd->n_sets = (uint32_t)km.n_sets; kd->world = world; kd->rank = rank;
  kd->off_meta = (km.n_sets + 1) * 8;
  kd->off_cnt = (kd->off_meta + km.n_sets * 8 + 63) & ~(size_t)63;
  kd->off_err = kd->off_cnt + ((2 * kd->nbmax + 1) * 8 + 63) / 64 * 64;
  kd->off_stats = kd->off_err + 64;
  if (!N) return CTMR_OK;
  HIPCHK(e, kd->tmp.alloc(kd->off_stats + sizeof(DevStats)));
  HIPCHK(e, hipMemcpyAsync(kd->t8(), km.set_first.data(), kd->off_meta, hipMemcpyHostToDevice, e->stream));
  if (km.n_sets) HIPCHK(e, hipMemcpyAsync(kd->t8() + kd->off_meta, ks.set_meta.data(), km.n_sets * 8, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemsetAsync(kd->t8() + kd->off_err, 0, 64 + sizeof(DevStats), e->stream));
  return CTMR_OK;
}

// The count pass over a chunk (k_known_count: validates every record) and its scan, queued on the stream.
int known_count_launch(ctmr_engine* e, const KnownImportArgs& a) {
  HIPCHK(e, hipMemsetAsync(a.cnt + 2 * a.nb, 0, 8, e->stream));
  hipLaunchKernelGGL(k_known_count, dim3((unsigned)a.nb), dim3(256), 0, e->stream, a);
  return scan_u64(e, (uint64_t*)a.cnt, 2 * a.nb + 1, false, SC_TMP);
}

// The same over chunk c, read back and checked; drains the stream.
// → tot[0] = records of at most 20 octets taken, tot[1] = all records taken.
int known_count_chunk(ctmr_engine* e, const KnownDev& kd, uint64_t c, const char* what, unsigned long long tot[2]) {
  const KnownImportArgs a = kd.args(c);
  int r;
  if ((r = known_count_launch(e, a))) return r;
  uint32_t err = 0;
  HIPCHK(e, hipMemcpyAsync(&tot[0], a.cnt + a.nb, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(&tot[1], a.cnt + 2 * a.nb, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(&err, a.err, 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  return known_record_error(e, err, what);
}

// Every member record validated and nothing else (the sort, an operand of the merge): the count pass with no set
// taken, in chunks of `chunk` records.  Drains the stream.
int known_validate_records(ctmr_engine* e, const KnownMeta& km, const uint8_t* d_members, uint64_t chunk, const char* what) {
  KnownSets ks;
  ks.set_meta.assign(km.n_sets, 0ull);
  KnownDev kd;
  int r;
  if ((r = known_dev_upload(e, km, ks, d_members, 1, 0, chunk, &kd))) return r;
  for (uint64_t c = 0; c < kd.nch; c++) {
    unsigned long long tot[2];
    if ((r = known_count_chunk(e, kd, c, what, tot))) return r;
  }
  return CTMR_OK;
}

// Set s, of an issuer not registered here: its records copied down, f(key, member, index in the set) for each.
template <class F>
int known_unreg_walk(ctmr_engine* e, const KnownMeta& km, const uint8_t* d_members, size_t s, F f) {
  const uint64_t first = km.set_first[s], cnt = km.set_first[s + 1] - first;
  std::vector<uint8_t> buf(cnt * KNOWN_REC_BYTES);
  HIPCHK(e, hipMemcpy(buf.data(), d_members + first * KNOWN_REC_BYTES, buf.size(), hipMemcpyDeviceToHost));
  const std::string key = "serials::" + exp_date_id(km.set_hour[s]) + "::" + km.ids[km.set_issuer[s]];
  for (uint64_t i = 0; i < cnt; i++) {
    const uint8_t* p = &buf[i * KNOWN_REC_BYTES];
    f(key, std::string((const char*)p + 8, (size_t)rd64(p)), i);
  }
  return CTMR_OK;
}

// Import: owner round check, issuer remap, then the members on the device (d_members: km.n_members records).
int known_import_core(ctmr_engine* e, const KnownMeta& km, const uint8_t* d_members, uint32_t world, uint32_t rank,
                      ctmr_known_import_stats* st) {
  KnownSets ks;
  int r;
  if ((r = known_sets_prepare(e, km, d_members, world, rank, "known import", &ks))) return r;
  const std::vector<size_t>& unreg = ks.unreg;
  const uint64_t unreg_members = ks.unreg_members;
  // host section (rank 0): members ctmr_set_insert would put into the device table are point inserts
  uint64_t host_point = 0;
  if (rank == 0)
    for (auto& hm : km.host) {
      int32_t eh; uint32_t cn;
      host_point += set_point(e, hm.first.data(), hm.first.size(), hm.second.size(), &eh, &cn);
    }
  memset(st, 0, sizeof *st);
  st->members = km.n_members;
  // ---- device records: count (and validate) every chunk, reserve, then pack and insert chunk by chunk
  KnownDev kd;
  if ((r = known_dev_upload(e, km, ks, d_members, world, rank, KNOWN_CHUNK, &kd))) return r;
  const uint64_t nch = kd.nch;
  uint64_t taken = 0;
  std::vector<uint64_t> n32(nch), n64(nch);
  for (uint64_t c = 0; c < nch; c++) {
    unsigned long long tot[2];
    if ((r = known_count_chunk(e, kd, c, "known import", tot))) return r;
    n32[c] = tot[0];
    n64[c] = tot[1] - tot[0];
    taken += tot[1];
  }
  st->taken = taken + unreg_members;
  // every slot and cell the call may claim, before anything is applied ("applied completely or not at all")
  if (taken + host_point) {
    if ((r = ensure_capacity(e, taken + host_point))) return r;
  }
  uint64_t inserted = 0;
  if (taken) {
    e->epoch++;
    e->pairs_dirty = true;
    DevStats* d_st = kd.stats();
    for (uint64_t c = 0; c < nch; c++) {
      if (!n32[c] && !n64[c]) continue;
      const KnownImportArgs a = kd.args(c);
      const uint64_t nb = a.nb;
      if (nch > 1)  // cnt[] holds the counts of the last chunk counted: with several chunks, each counts again
        if ((r = known_count_launch(e, a))) return r;
      const uint64_t m32 = n32[c], m64 = n64[c], M = m32 + m64;
      DevMem recs;
      const size_t off64 = m32 * sizeof(KeyRec32), off_slot = off64 + m64 * sizeof(KeyRec), off_fl = off_slot + M * 4;
      HIPCHK(e, recs.alloc(off_fl + M + 64));
      uint8_t* r8 = recs.u8();
      KeyRec32* k32 = (KeyRec32*)r8;
      KeyRec* k64 = (KeyRec*)(r8 + off64);
      uint32_t* d_slot = (uint32_t*)(r8 + off_slot);
      uint8_t* d_fl = r8 + off_fl;
      hipLaunchKernelGGL(k_known_pack, dim3((unsigned)nb), dim3(256), 0, e->stream, a, (const unsigned long long*)a.cnt, k32, k64);
      // the owner-computes receive path outside a round: this chunk's cells start at ref0 — a word with a lower ref is an
      // older key (compared at once), a same-tag word of the chunk is settled in pass 2 by the records' orders
      const unsigned long long ref0 = e->arena_used;
      e->arena_used += M;
      InsertArgs loc{};
      loc.t = e->tbl();
      loc.ref0 = ref0;
      loc.n = 0;  // no entries of a batch to mark
      loc.ord_base = 0;
      xchg_owner_insert(e, k32, m32, k64, m64, loc, ref0, ref0, nullptr, d_slot, d_fl, d_fl + m32, d_st);
      if (e->d_bloom) {
        if (m32) hipLaunchKernelGGL((k_known_bloom<KeyRec32>), dim3((unsigned)((m32 + 255) / 256)), dim3(256), 0, e->stream,
                                    (const KeyRec32*)k32, m32, e->d_bloom, e->bloom_words - 1);
        if (m64) hipLaunchKernelGGL((k_known_bloom<KeyRec>), dim3((unsigned)((m64 + 255) / 256)), dim3(256), 0, e->stream,
                                    (const KeyRec*)k64, m64, e->d_bloom, e->bloom_words - 1);
      }
      DevStats ds;
      HIPCHK(e, hipMemcpyAsync(&ds, d_st, sizeof ds, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(e, hipMemsetAsync(d_st, 0, sizeof ds, e->stream));
      HIPCHK(e, hipStreamSynchronize(e->stream));
      HIPCHK(e, hipGetLastError());
      e->occupied += ds.n_new;
      inserted += ds.n_new;
      if (ds.n_full) return fail(e, CTMR_E_FULL, "known-certificate table full (%llu slots)", (unsigned long long)e->nslots);
    }
  }
  // ---- sets of issuers not registered here (world = 1): their members go where ctmr_set_insert puts them
  for (size_t s : unreg)
    if ((r = known_unreg_walk(e, km, d_members, s, [&](const std::string& key, const std::string& m, uint64_t) {
          inserted += host_insert(e, key, m);
        })))
      return r;
  st->inserted = inserted;
  st->known = st->taken - inserted;
  // ---- the host section (rank 0 alone): ctmr_set_insert, member by member
  if (rank == 0) {
    st->host_members = km.host.size();
    for (auto& hm : km.host) {
      int was_new = 0;
      if ((r = set_op(e, 0, hm.first, hm.second, &was_new))) return r;
      st->host_inserted += was_new;
    }
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return CTMR_OK;
}

// ---- bulk SetContains / SetRemove over an image's member records (include/ctmr.h ctmr_known_query* / ctmr_known_remove*,
// DESIGN.md §14)

// records per pass, as import's
uint64_t known_probe_chunk() { return known_chunk("CTMR_KNOWN_PROBE_CHUNK", KNOWN_CHUNK); }

// records per lane of k_known_query / k_known_remove: KNOWN_PROBE_RPL was the fastest of 1, 2, 4, 8 (DESIGN.md §14);
// CTMR_KNOWN_PROBE_RPL selects another for scripts/bench_known_query.py's sweep and the tests of every instantiation
constexpr uint32_t KNOWN_PROBE_RPL = 4;
uint32_t known_probe_rpl() {
  const uint64_t v = env_u64("CTMR_KNOWN_PROBE_RPL");
  return v == 1 || v == 2 || v == 4 || v == 8 ? (uint32_t)v : KNOWN_PROBE_RPL;
}

template <int R>
void known_probe_launch(ctmr_engine* e, const KnownImportArgs& a, bool remove, uint8_t* d_flags) {
  if (remove) hipLaunchKernelGGL((k_known_remove<R>), dim3((unsigned)a.nb), dim3(256), 0, e->stream, a, e->tbl(), e->issuer_counts);
  else hipLaunchKernelGGL((k_known_query<R>), dim3((unsigned)a.nb), dim3(256), 0, e->stream, a, e->tbl(), d_flags);
}

// Query (d_flags: km.n_members bytes of device memory, host_flags: km.host.size() bytes) or remove.  The callers have
// checked the buffer sizes.
int known_probe_core(ctmr_engine* e, const KnownMeta& km, const uint8_t* d_members, uint32_t world, uint32_t rank,
                     bool remove, uint8_t* d_flags, uint8_t* host_flags, ctmr_known_probe_stats* st) {
  const char* what = remove ? "known remove" : "known query";
  KnownSets ks;
  int r;
  if ((r = known_sets_prepare(e, km, d_members, world, rank, what, &ks))) return r;
  const uint64_t N = km.n_members;
  KnownDev kd;
  if ((r = known_dev_upload(e, km, ks, d_members, world, rank, known_probe_chunk(), &kd))) return r;
  uint64_t taken = 0, hits = 0;
  if (remove) {  // every record of every chunk is validated before the first word is touched
    for (uint64_t c = 0; c < kd.nch; c++) {
      unsigned long long tot[2];
      if ((r = known_count_chunk(e, kd, c, what, tot))) return r;
      taken += tot[1];
    }
    if (taken) e->pairs_dirty = true;
  }
  const uint32_t R = known_probe_rpl();
  for (uint64_t c = 0; c < kd.nch && (taken || !remove); c++) {
    KnownImportArgs a = kd.args(c);
    a.nb = (a.n + 256ull * R - 1) / (256ull * R);  // the probe kernels' blocks take 256 R records
    uint8_t* fl = remove ? nullptr : d_flags + c * kd.chunk;
    switch (R) {
      case 1: known_probe_launch<1>(e, a, remove, fl); break;
      case 2: known_probe_launch<2>(e, a, remove, fl); break;
      case 8: known_probe_launch<8>(e, a, remove, fl); break;
      default: known_probe_launch<4>(e, a, remove, fl); break;
    }
    // per block: remove cnt[blk] = removed; query cnt[blk] = taken, cnt[nb + blk] = found — summed by an inclusive scan
    const uint64_t ncnt = remove ? a.nb : 2 * a.nb;
    if ((r = scan_u64(e, (uint64_t*)a.cnt, ncnt, true, SC_TMP))) return r;
    unsigned long long tot[2] = {0ull, 0ull};
    uint32_t err = 0;
    HIPCHK(e, hipMemcpyAsync(&tot[0], a.cnt + a.nb - 1, 8, hipMemcpyDeviceToHost, e->stream));
    if (!remove) {
      HIPCHK(e, hipMemcpyAsync(&tot[1], a.cnt + 2 * a.nb - 1, 8, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(e, hipMemcpyAsync(&err, a.err, 4, hipMemcpyDeviceToHost, e->stream));
    }
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipGetLastError());
    if ((r = known_record_error(e, err, what))) return r;
    if (remove) {
      hits += tot[0];
    } else {
      taken += tot[0];
      hits += tot[1] - tot[0];
    }
  }
  // ---- sets of issuers not registered here (world = 1): where ctmr_set_insert puts their members, the host-side store
  for (size_t s : ks.unreg) {
    std::vector<uint8_t> fl(km.set_first[s + 1] - km.set_first[s]);
    if ((r = known_unreg_walk(e, km, d_members, s, [&](const std::string& key, const std::string& m, uint64_t i) {
          fl[i] = remove ? host_erase(e, key, m) : host_contains(e, key, m);
          hits += fl[i];
        })))
      return r;
    if (!remove) HIPCHK(e, hipMemcpy(d_flags + km.set_first[s], fl.data(), fl.size(), hipMemcpyHostToDevice));
  }
  memset(st, 0, sizeof *st);
  st->members = N;
  st->taken = taken + ks.unreg_members;
  st->hits = hits;
  // ---- the host section (rank 0 alone): ctmr_set_contains / ctmr_set_remove, member by member
  if (!remove && rank != 0) memset(host_flags, 2, km.host.size());
  if (rank == 0) {
    st->host_members = km.host.size();
    for (size_t i = 0; i < km.host.size(); i++) {
      int hit = 0;
      if ((r = set_op(e, remove ? 2 : 1, km.host[i].first, km.host[i].second, &hit))) return r;
      if (!remove) host_flags[i] = (uint8_t)(hit != 0);
      st->host_hits += hit != 0;
    }
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return CTMR_OK;
}

// a query's buffers against the image: CTMR_E_RANGE with the stats filled as far as known, nothing written
int known_query_room(ctmr_engine* e, const KnownMeta& km, uint32_t rank, const void* flags, uint64_t flags_cap,
                     const uint8_t* host_flags, size_t host_flags_cap, ctmr_known_probe_stats* st) {
  if (flags_cap >= km.n_members && host_flags_cap >= km.host.size() && (flags || !km.n_members) &&
      (host_flags || km.host.empty()))
    return CTMR_OK;
  memset(st, 0, sizeof *st);
  st->members = km.n_members;
  st->host_members = rank == 0 ? km.host.size() : 0;
  return fail(e, CTMR_E_RANGE, "known query: %llu flags and %llu host flags needed", (unsigned long long)km.n_members,
              (unsigned long long)km.host.size());
}

// the member records of a whole image, copied to the device (+ extra bytes behind them: a query's flags)
int known_stage_members(ctmr_engine* e, const KnownMeta& km, const uint8_t* image, size_t extra, const char* what, DevMem* d) {
  const size_t bytes = km.n_members * KNOWN_REC_BYTES;
  if (!km.n_members) return CTMR_OK;
  if (d->alloc(bytes + extra) != hipSuccess)
    return fail(e, CTMR_E_NOMEM, "%s: no device memory for %llu member records", what, (unsigned long long)km.n_members);
  HIPCHK(e, hipMemcpyAsync(d->p, image + km.meta_bytes, bytes, hipMemcpyHostToDevice, e->stream));
  return CTMR_OK;
}

}  // namespace
}  // extern "C++"

int ctmr_known_export(ctmr_engine* e, uint8_t* out, size_t cap, ctmr_known_image_info* info) {
  if (!e || !info) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  KnownExport x;
  int r;
  if ((r = known_export_prepare(e, &x))) return r;
  *info = x.info;
  if (!out || cap < x.info.image_bytes) return fail(e, CTMR_E_RANGE, "known export: %llu bytes needed", (unsigned long long)x.info.image_bytes);
  const uint64_t N = x.info.members;
  if (N) {
    // stage the member records on the device: all at once when that fits, else set range by set range
    uint64_t stage = N;
    DevMem d;
    while (d.alloc(stage * KNOWN_REC_BYTES) != hipSuccess) {
      if (stage <= (1ull << 20)) return fail(e, CTMR_E_NOMEM, "known export: no device memory to stage the member records");
      stage /= 2;
    }
    for (const KnownRun& run : known_cut_sets(x, stage)) {
      const uint64_t n = run.n;
      DevMem big;  // one set larger than the staging buffer: staged alone
      if (n > stage && big.alloc(n * KNOWN_REC_BYTES) != hipSuccess)
        return fail(e, CTMR_E_NOMEM, "known export: no device memory to stage a set of %llu members", (unsigned long long)n);
      uint8_t* buf = n > stage ? big.u8() : d.u8();
      if ((r = known_export_members(e, x, run.s_lo, run.s_hi, buf))) return r;
      HIPCHK(e, hipMemcpy(out + x.info.meta_bytes + run.lo * KNOWN_REC_BYTES, buf, n * KNOWN_REC_BYTES, hipMemcpyDeviceToHost));
    }
  }
  memcpy(out, x.meta.data(), x.meta.size());
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return CTMR_OK;
}

int ctmr_known_export_device(ctmr_engine* e, uint8_t* meta, size_t meta_cap, void* d_members, uint64_t members_cap,
                             ctmr_known_image_info* info) {
  if (!e || !info) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  KnownExport x;
  int r;
  if ((r = known_export_prepare(e, &x))) return r;
  *info = x.info;
  if (!meta || meta_cap < x.info.meta_bytes || members_cap < x.info.members || (x.info.members && !d_members))
    return fail(e, CTMR_E_RANGE, "known export: %llu meta bytes and %llu member records needed",
                (unsigned long long)x.info.meta_bytes, (unsigned long long)x.info.members);
  if ((r = known_export_members(e, x, 0, x.set_range.size(), (uint8_t*)d_members))) return r;
  memcpy(meta, x.meta.data(), x.meta.size());
  return CTMR_OK;
}

int ctmr_known_import(ctmr_engine* e, const uint8_t* image, size_t len, uint32_t world, uint32_t rank,
                      ctmr_known_import_stats* st) {
  if (!e || !image || !st) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  KnownMeta km;
  DevMem d;
  int r;
  if ((r = known_open(e, image, len, nullptr, "known import", &km))) return r;
  if ((r = known_stage_members(e, km, image, 0, "known import", &d))) return r;
  return known_import_core(e, km, d.u8(), world, rank, st);
}

int ctmr_known_import_device(ctmr_engine* e, const uint8_t* meta, size_t meta_len, const void* d_members,
                             uint64_t n_members, uint32_t world, uint32_t rank, ctmr_known_import_stats* st) {
  if (!e || !meta || !st) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  KnownMeta km;
  int r;
  if ((r = known_open(e, meta, meta_len, &n_members, "known import", &km))) return r;
  return known_import_core(e, km, (const uint8_t*)d_members, world, rank, st);
}

int ctmr_known_query(ctmr_engine* e, const uint8_t* image, size_t len, uint32_t world, uint32_t rank, uint8_t* flags,
                     size_t flags_cap, uint8_t* host_flags, size_t host_flags_cap, ctmr_known_probe_stats* st) {
  if (!e || !image || !st) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  KnownMeta km;
  DevMem d;
  int r;
  if ((r = known_open(e, image, len, nullptr, "known query", &km))) return r;
  if ((r = known_query_room(e, km, rank, flags, flags_cap, host_flags, host_flags_cap, st))) return r;
  if ((r = known_stage_members(e, km, image, km.n_members, "known query", &d))) return r;
  uint8_t* d_flags = d.p ? d.u8() + km.n_members * KNOWN_REC_BYTES : nullptr;
  if ((r = known_probe_core(e, km, d.u8(), world, rank, false, d_flags, host_flags, st))) return r;
  if (km.n_members) HIPCHK(e, hipMemcpy(flags, d_flags, km.n_members, hipMemcpyDeviceToHost));
  return CTMR_OK;
}

int ctmr_known_query_device(ctmr_engine* e, const uint8_t* meta, size_t meta_len, const void* d_members,
                            uint64_t n_members, uint32_t world, uint32_t rank, void* d_flags, uint64_t flags_cap,
                            uint8_t* host_flags, size_t host_flags_cap, ctmr_known_probe_stats* st) {
  if (!e || !meta || !st) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  KnownMeta km;
  int r;
  if ((r = known_open(e, meta, meta_len, &n_members, "known query", &km))) return r;
  if ((r = known_query_room(e, km, rank, d_flags, flags_cap, host_flags, host_flags_cap, st))) return r;
  return known_probe_core(e, km, (const uint8_t*)d_members, world, rank, false, (uint8_t*)d_flags, host_flags, st);
}

int ctmr_known_remove(ctmr_engine* e, const uint8_t* image, size_t len, uint32_t world, uint32_t rank,
                      ctmr_known_probe_stats* st) {
  if (!e || !image || !st) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  KnownMeta km;
  DevMem d;
  int r;
  if ((r = known_open(e, image, len, nullptr, "known remove", &km))) return r;
  if ((r = known_stage_members(e, km, image, 0, "known remove", &d))) return r;
  return known_probe_core(e, km, d.u8(), world, rank, true, nullptr, nullptr, st);
}

int ctmr_known_remove_device(ctmr_engine* e, const uint8_t* meta, size_t meta_len, const void* d_members,
                             uint64_t n_members, uint32_t world, uint32_t rank, ctmr_known_probe_stats* st) {
  if (!e || !meta || !st) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  KnownMeta km;
  int r;
  if ((r = known_open(e, meta, meta_len, &n_members, "known remove", &km))) return r;
  return known_probe_core(e, km, (const uint8_t*)d_members, world, rank, true, nullptr, nullptr, st);
}
