// engine/merge.inc — set algebra on known-certificate images (include/ctmr.h ctmr_known_merge*, DESIGN.md §16): the
// canonical image of A ∪ B, A \ B or A ∩ B from two images v1, by the kernels of kernels/merge.h, with no table behind
// it.  Host side: the two metas opened, each operand made canonical (used where it lies when it already is), the set
// lists merged by key into pairs, the host sections' algebra, and the meta of the result.
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after engine/sort.inc.

extern "C++" {
namespace {

// a set of an operand or of the result: its key as ctmr_keys returns it, and what the image's set entry says of it
struct MergeSetKey {
  std::string key;
  int32_t hour = 0;
  uint8_t digest[32] = {};
};

int b64url_value(char c) {
  if (c >= 'A' && c <= 'Z') return c - 'A';
  if (c >= 'a' && c <= 'z') return c - 'a' + 26;
  if (c >= '0' && c <= '9') return c - '0' + 52;
  return c == '-' ? 62 : (c == '_' ? 63 : -1);
}

// serials::<expDate>::<Issuer.ID> with an hour-resolution date and the padded base64url of a 32-byte digest, exactly as
// an image's set entry spells it → the entry; every other key can only live in the host section.
bool merge_parse_key(const std::string& key, MergeSetKey* out) {
  if (key.size() != 9 + 13 + 2 + 44 || key.compare(0, 9, "serials::") != 0 || key[22] != ':' || key[23] != ':') return false;
  if (!parse_exp_date_id(key.data() + 9, 13, &out->hour)) return false;
  const char* s = key.data() + 24;
  if (s[43] != '=') return false;
  uint8_t d[33];
  for (int g = 0; g < 11; g++) {
    uint32_t v = 0;
    for (int k = 0; k < 4; k++) {
      const int q = g == 10 && k == 3 ? 0 : b64url_value(s[4 * g + k]);
      if (q < 0) return false;
      v = (v << 6) | (uint32_t)q;
    }
    d[3 * g] = (uint8_t)(v >> 16); d[3 * g + 1] = (uint8_t)(v >> 8); d[3 * g + 2] = (uint8_t)v;
  }
  if (b64url(d, 32) != key.substr(24)) return false;  // (bits behind the 32nd octet)
  memcpy(out->digest, d, 32);
  out->key = key;
  return true;
}

// An operand on its way to canonical form.
struct MergeOperand {
  KnownMeta km;
  std::vector<MergeSetKey> sets;
  std::vector<uint64_t> first;   // sets.size() + 1
  const uint8_t* rec = nullptr;  // the canonical records: the caller's, or `work`
  uint64_t n = 0;
  DevMem work, squeezed;
  std::vector<std::pair<std::string, std::string>> host;  // the host-section pairs that stay there
  bool in_place = true;
  // on the device: first[] and pair_of[]
  DevMem dev;
  MergeSide side(bool is_b) const {
    MergeSide s{};
    s.rec = rec; s.n = n; s.first = (const uint64_t*)dev.p;
    s.pair_of = (const uint32_t*)(dev.u8() + (sets.size() + 1) * 8);
    s.ns = (uint32_t)sets.size(); s.is_b = is_b ? 1u : 0u;
    return s;
  }
};

// bit words and block counts of the kept records of n records (kernels/merge.h: merge_kept_before), zeroed
struct MergeKept {
  DevMem mem;
  uint64_t nb = 0;
  unsigned long long* bits() const { return (unsigned long long*)mem.p; }
  unsigned long long* cnt() const { return bits() + 4 * (nb + 1); }
  int alloc(ctmr_engine* e, uint64_t n) {
    nb = (n + 255) / 256;
    if (mem.alloc(5 * (nb + 1) * 8) != hipSuccess) return fail(e, CTMR_E_NOMEM, "known merge: no device memory for the kept-record bits of %llu records", (unsigned long long)n);
    HIPCHK(e, hipMemsetAsync(mem.p, 0, 5 * (nb + 1) * 8, e->stream));
    return CTMR_OK;
  }
  // cnt[] → kept records before each block, cnt[nb] = all of them (*total)
  int scan(ctmr_engine* e, uint64_t* total) { return scan_total(e, (uint64_t*)cnt(), nb + 1, false, SC_TMP, total); }
};

int merge_upload_first(ctmr_engine* e, MergeOperand& o, const std::vector<uint32_t>& pair_of) {
  const size_t ns = o.sets.size();
  if (o.dev.alloc((ns + 1) * 8 + (ns + 1) * 4) != hipSuccess) return fail(e, CTMR_E_NOMEM, "known merge: no device memory for %zu sets", ns);
  HIPCHK(e, hipMemcpyAsync(o.dev.p, o.first.data(), (ns + 1) * 8, hipMemcpyHostToDevice, e->stream));
  if (!pair_of.empty()) HIPCHK(e, hipMemcpyAsync(o.dev.u8() + (ns + 1) * 8, pair_of.data(), pair_of.size() * 4, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));  // (the host vectors may go before the copies ran)
  return CTMR_OK;
}

// An operand whose meta known_open has parsed into o->km (no meta: the empty image), its records at d_rec: they are
// validated, and then made canonical — the sets in key order, each ascending with every member once, the host-section
// pairs the member section can carry among them.  A sorted export passes the check and is used where it lies; anything
// else is copied aside, sorted (known_sort_sets) and squeezed.
int merge_open(ctmr_engine* e, const uint8_t* d_rec, const char* what, MergeOperand* o) {
  int r;
  const KnownMeta& km = o->km;
  if (km.set_first.empty()) {  // the empty image (a parsed meta has n_sets + 1 firsts)
    o->first.assign(1, 0ull);
    return CTMR_OK;
  }
  if ((r = known_bind(e, km, d_rec, what))) return r;
  if ((r = known_validate_records(e, km, d_rec, known_sort_chunk(), what))) return r;
  std::vector<MergeSetKey> own(km.n_sets);
  for (uint64_t s = 0; s < km.n_sets; s++) {
    own[s].hour = km.set_hour[s];
    memcpy(own[s].digest, km.issuers + (size_t)km.set_issuer[s] * 32, 32);
    own[s].key = "serials::" + exp_date_id(km.set_hour[s]) + "::" + km.ids[km.set_issuer[s]];
  }
  // host-section pairs that belong in the member section (in (key, member) order, as the section is)
  std::vector<std::pair<MergeSetKey, std::string>> moved;
  for (auto& hm : km.host) {
    MergeSetKey k;
    if (hm.second.size() <= CTMR_MAX_SERIAL && merge_parse_key(hm.first, &k)) moved.emplace_back(k, hm.second);
    else o->host.push_back(hm);
  }
  for (uint64_t s = 0; s < km.n_sets; s++)
    if (km.set_first[s + 1] - km.set_first[s] > 0xffffffffull)
      return fail(e, CTMR_E_NOMEM, "%s: a set of %llu members", what, (unsigned long long)(km.set_first[s + 1] - km.set_first[s]));
  if (moved.empty()) {
    o->sets.swap(own);
    o->first = km.set_first;
    o->n = km.n_members;
    o->rec = d_rec;
    if (o->n < 2) return CTMR_OK;
    if ((r = merge_upload_first(e, *o, {}))) return r;
    DevMem flag;
    HIPCHK(e, flag.alloc(64));
    HIPCHK(e, hipMemsetAsync(flag.p, 0, 4, e->stream));
    hipLaunchKernelGGL(k_merge_ascending, dim3((unsigned)((o->n + 255) / 256)), dim3(256), 0, e->stream, o->side(false), (uint32_t*)flag.p);
    uint32_t bad = 0;
    HIPCHK(e, hipMemcpyAsync(&bad, flag.p, 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipGetLastError());
    if (!bad) return CTMR_OK;
    o->in_place = false;
    if (o->work.alloc(o->n * KNOWN_REC_BYTES) != hipSuccess)
      return fail(e, CTMR_E_NOMEM, "%s: no device memory for a copy of %llu member records", what, (unsigned long long)o->n);
    HIPCHK(e, hipMemcpyAsync(o->work.p, d_rec, o->n * KNOWN_REC_BYTES, hipMemcpyDeviceToDevice, e->stream));
  } else {
    // the working copy: per set its records, then the pairs that moved in (a key of their own: a set of their own)
    o->in_place = false;
    o->n = km.n_members + moved.size();
    if (o->work.alloc(o->n * KNOWN_REC_BYTES) != hipSuccess)
      return fail(e, CTMR_E_NOMEM, "%s: no device memory for a copy of %llu member records", what, (unsigned long long)o->n);
    std::vector<uint8_t> recs;
    for (auto& mv : moved) known_put_record(mv.second, &recs);
    uint64_t at = 0, run_src = 0, run_dst = 0;  // the records of sets not yet copied: [run_src, first of s) → run_dst
    size_t s = 0, m = 0;
    auto flush = [&](uint64_t src_end) -> int {
      if (src_end > run_src)
        HIPCHK(e, hipMemcpyAsync(o->work.u8() + run_dst * KNOWN_REC_BYTES, d_rec + run_src * KNOWN_REC_BYTES,
                                 (src_end - run_src) * KNOWN_REC_BYTES, hipMemcpyDeviceToDevice, e->stream));
      return CTMR_OK;
    };
    while (s < own.size() || m < moved.size()) {
      const bool take_own = m == moved.size() || (s < own.size() && own[s].key <= moved[m].first.key);
      const MergeSetKey& k = take_own ? own[s] : moved[m].first;
      o->sets.push_back(k);
      o->first.push_back(at);
      if (take_own) {
        at += km.set_first[s + 1] - km.set_first[s];
        s++;
      }
      size_t m1 = m;
      while (m1 < moved.size() && moved[m1].first.key == k.key) m1++;
      if (m1 > m) {
        if ((r = flush(km.set_first[s]))) return r;
        HIPCHK(e, hipMemcpyAsync(o->work.u8() + at * KNOWN_REC_BYTES, &recs[m * KNOWN_REC_BYTES], (m1 - m) * KNOWN_REC_BYTES,
                                 hipMemcpyHostToDevice, e->stream));
        at += m1 - m;
        run_src = km.set_first[s];
        run_dst = at;
        m = m1;
      }
    }
    if ((r = flush(km.n_members))) return r;
    o->first.push_back(at);
    HIPCHK(e, hipStreamSynchronize(e->stream));  // (recs goes out of scope)
  }
  // sorted aside, then every member once
  if ((r = known_sort_sets(e, o->work.u8(), o->first))) return r;
  o->rec = o->work.u8();
  if ((r = merge_upload_first(e, *o, {}))) return r;
  MergeKept heads;
  if ((r = heads.alloc(e, o->n))) return r;
  hipLaunchKernelGGL(k_merge_unique, dim3((unsigned)heads.nb), dim3(256), 0, e->stream, o->side(false), heads.bits(), heads.cnt());
  uint64_t left = 0;
  if ((r = heads.scan(e, &left))) return r;
  if (left == o->n) return CTMR_OK;
  if (o->squeezed.alloc(left * KNOWN_REC_BYTES) != hipSuccess)
    return fail(e, CTMR_E_NOMEM, "%s: no device memory for %llu member records without their repeats", what, (unsigned long long)left);
  const size_t ns = o->sets.size();
  DevMem nf;
  HIPCHK(e, nf.alloc((ns + 1) * 8));
  hipLaunchKernelGGL((k_merge_place<MERGE_OWN>), dim3((unsigned)heads.nb), dim3(256), 0, e->stream, o->side(false),
                     (const MergePair*)nullptr, (const uint32_t*)nullptr, (const unsigned long long*)heads.bits(),
                     (const unsigned long long*)heads.cnt(), o->squeezed.u8(), left);
  hipLaunchKernelGGL(k_merge_first, dim3((unsigned)((ns + 256) / 256)), dim3(256), 0, e->stream, (const uint64_t*)o->dev.p,
                     (uint32_t)ns, (const unsigned long long*)heads.bits(), (const unsigned long long*)heads.cnt(), (uint64_t*)nf.p);
  HIPCHK(e, hipMemcpyAsync(o->first.data(), nf.p, (ns + 1) * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  o->rec = o->squeezed.u8();
  o->n = left;
  { DevMem done; std::swap(done.p, o->work.p); }  // the sorted copy with its repeats is done with
  return CTMR_OK;
}

// What a merge has worked out before the first record of the result is placed: the meta and sizes of the result and
// everything the place pass reads.
struct MergePlan {
  int op = 0;
  MergeOperand a, b;
  std::vector<MergePair> pairs;
  DevMem d_pairs, d_lb_a, d_lb_b;
  MergeKept kept;  // UNION: B's records A does not hold; MINUS / INTERSECT: A's kept records
  std::vector<uint8_t> meta;
  ctmr_known_image_info info{};
};

int merge_prepare(ctmr_engine* e, MergePlan* mp) {
  MergeOperand &a = mp->a, &b = mp->b;
  const int op = mp->op;
  int r;
  // the set lists merged by key
  std::vector<uint32_t> pair_a(a.sets.size()), pair_b(b.sets.size());
  std::vector<const MergeSetKey*> pkey;
  for (size_t i = 0, j = 0; i < a.sets.size() || j < b.sets.size();) {
    const int c = i == a.sets.size() ? 1 : (j == b.sets.size() ? -1 : a.sets[i].key.compare(b.sets[j].key));
    MergePair p{a.first[i], 0ull, b.first[j], 0ull};
    pkey.push_back(c <= 0 ? &a.sets[i] : &b.sets[j]);
    if (c <= 0) { p.count_a = a.first[i + 1] - a.first[i]; pair_a[i++] = (uint32_t)mp->pairs.size(); }
    if (c >= 0) { p.count_b = b.first[j + 1] - b.first[j]; pair_b[j++] = (uint32_t)mp->pairs.size(); }
    mp->pairs.push_back(p);
  }
  const size_t np = mp->pairs.size();
  if (np > 0xffffffffull) return fail(e, CTMR_E_NOMEM, "known merge: %zu sets", np);
  if ((r = merge_upload_first(e, a, pair_a)) || (r = merge_upload_first(e, b, pair_b))) return r;
  DevMem d_counts;
  if (mp->d_pairs.alloc((np + 1) * sizeof(MergePair)) != hipSuccess || d_counts.alloc((np + 1) * 8) != hipSuccess)
    return fail(e, CTMR_E_NOMEM, "known merge: no device memory for %zu pairs of sets", np);
  if (np) HIPCHK(e, hipMemcpyAsync(mp->d_pairs.p, mp->pairs.data(), np * sizeof(MergePair), hipMemcpyHostToDevice, e->stream));
  const MergePair* d_pairs = (const MergePair*)mp->d_pairs.p;
  // rank pass
  const bool is_union = op == CTMR_KNOWN_UNION;
  if ((r = mp->kept.alloc(e, is_union ? b.n : a.n))) return r;
  if (is_union) {
    if (mp->d_lb_a.alloc((a.n + 1) * 4) != hipSuccess || mp->d_lb_b.alloc((b.n + 1) * 4) != hipSuccess)
      return fail(e, CTMR_E_NOMEM, "known merge: no device memory for the places of %llu member records", (unsigned long long)(a.n + b.n));
    if (a.n) hipLaunchKernelGGL(k_merge_rank, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, e->stream, a.side(false), d_pairs,
                                b.rec, 0u, (uint32_t*)mp->d_lb_a.p, (unsigned long long*)nullptr, (unsigned long long*)nullptr);
    if (b.n) hipLaunchKernelGGL(k_merge_rank, dim3((unsigned)mp->kept.nb), dim3(256), 0, e->stream, b.side(true), d_pairs, a.rec,
                                0u, (uint32_t*)mp->d_lb_b.p, mp->kept.bits(), mp->kept.cnt());
  } else if (a.n) {
    hipLaunchKernelGGL(k_merge_rank, dim3((unsigned)mp->kept.nb), dim3(256), 0, e->stream, a.side(false), d_pairs, b.rec,
                       op == CTMR_KNOWN_INTERSECT ? 1u : 0u, (uint32_t*)nullptr, mp->kept.bits(), mp->kept.cnt());
  }
  uint64_t kept = 0;
  if ((r = mp->kept.scan(e, &kept))) return r;
  // the members of the result per pair
  std::vector<unsigned long long> counts(np);
  if (np) {
    hipLaunchKernelGGL(k_merge_sets, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, e->stream, d_pairs, (uint64_t)np,
                       is_union ? 1u : 0u, (const unsigned long long*)mp->kept.bits(), (const unsigned long long*)mp->kept.cnt(),
                       (unsigned long long*)d_counts.p);
    HIPCHK(e, hipMemcpyAsync(counts.data(), d_counts.p, np * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipGetLastError());
  }
  // the host sections' algebra
  std::vector<std::pair<std::string, std::string>> host;
  if (is_union) std::set_union(a.host.begin(), a.host.end(), b.host.begin(), b.host.end(), std::back_inserter(host));
  else if (op == CTMR_KNOWN_MINUS) std::set_difference(a.host.begin(), a.host.end(), b.host.begin(), b.host.end(), std::back_inserter(host));
  else std::set_intersection(a.host.begin(), a.host.end(), b.host.begin(), b.host.end(), std::back_inserter(host));
  // the meta: the sets that are left, the issuers they name in digest order
  std::vector<const uint8_t*> digs;
  for (size_t p = 0; p < np; p++)
    if (counts[p]) digs.push_back(pkey[p]->digest);
  known_number_digests(&digs);
  std::vector<KnownSetEntry> sets;
  for (size_t p = 0; p < np; p++)
    if (counts[p]) sets.push_back({pkey[p]->hour, known_digest_ordinal(digs, pkey[p]->digest), counts[p]});
  known_write_meta(digs, sets, host, &mp->meta, &mp->info);
  if (mp->info.members != (is_union ? a.n + kept : kept))
    return fail(e, CTMR_E_HIP, "known merge: the sets hold %llu members, the kept records are %llu", (unsigned long long)mp->info.members,
                (unsigned long long)(is_union ? a.n + kept : kept));
  return CTMR_OK;
}

// The place pass: info.members records to d_out.  Drains the stream.
int merge_place(ctmr_engine* e, MergePlan* mp, uint8_t* d_out) {
  MergeOperand &a = mp->a, &b = mp->b;
  const MergePair* d_pairs = (const MergePair*)mp->d_pairs.p;
  const unsigned long long *bits = mp->kept.bits(), *base = mp->kept.cnt();
  const uint64_t cap = mp->info.members;
  if (mp->op == CTMR_KNOWN_UNION) {
    if (a.n) hipLaunchKernelGGL((k_merge_place<MERGE_UNION_A>), dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, e->stream,
                                a.side(false), d_pairs, (const uint32_t*)mp->d_lb_a.p, bits, base, d_out, cap);
    if (b.n) hipLaunchKernelGGL((k_merge_place<MERGE_UNION_B>), dim3((unsigned)((b.n + 255) / 256)), dim3(256), 0, e->stream,
                                b.side(true), d_pairs, (const uint32_t*)mp->d_lb_b.p, bits, base, d_out, cap);
  } else if (a.n && cap) {
    hipLaunchKernelGGL((k_merge_place<MERGE_OWN>), dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, e->stream, a.side(false),
                       d_pairs, (const uint32_t*)nullptr, bits, base, d_out, cap);
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  if (env_u64("CTMR_KNOWN_MERGE_INFO"))  // tests and scripts/bench_known_merge.py read which path an operand took
    fprintf(stderr, "ctmr known merge: op=%d a=%s b=%s a_records=%llu b_records=%llu members=%llu\n", mp->op,
            a.in_place ? "in_place" : "sorted", b.in_place ? "in_place" : "sorted", (unsigned long long)a.n,
            (unsigned long long)b.n, (unsigned long long)cap);
  return CTMR_OK;
}

int merge_check_op(ctmr_engine* e, int op) {
  if (op == CTMR_KNOWN_UNION || op == CTMR_KNOWN_MINUS || op == CTMR_KNOWN_INTERSECT) return CTMR_OK;
  return fail(e, CTMR_E_INVAL, "known merge: op %d: CTMR_KNOWN_UNION, CTMR_KNOWN_MINUS or CTMR_KNOWN_INTERSECT", op);
}

}  // namespace
}  // extern "C++"

int ctmr_known_merge_device(ctmr_engine* e, int op, const uint8_t* a_meta, size_t a_meta_len, const void* d_a, uint64_t a_members,
                            const uint8_t* b_meta, size_t b_meta_len, const void* d_b, uint64_t b_members,
                            uint8_t* out_meta, size_t out_meta_cap, void* d_out, uint64_t out_members_cap,
                            ctmr_known_image_info* info) {
  if (!e || !a_meta || !info || (!b_meta && b_meta_len)) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  MergePlan mp;
  mp.op = op;
  int r;
  if ((r = merge_check_op(e, op))) return r;
  if (!b_meta && b_members) return fail(e, CTMR_E_INVAL, "known merge: %llu member records given for the empty image", (unsigned long long)b_members);
  if ((r = known_open(e, a_meta, a_meta_len, &a_members, "known merge (A)", &mp.a.km))) return r;
  if ((r = merge_open(e, (const uint8_t*)d_a, "known merge (A)", &mp.a))) return r;
  if (b_meta && (r = known_open(e, b_meta, b_meta_len, &b_members, "known merge (B)", &mp.b.km))) return r;
  if ((r = merge_open(e, (const uint8_t*)d_b, "known merge (B)", &mp.b))) return r;
  if ((r = merge_prepare(e, &mp))) return r;
  *info = mp.info;
  if (!out_meta || out_meta_cap < mp.info.meta_bytes || out_members_cap < mp.info.members || (mp.info.members && !d_out))
    return fail(e, CTMR_E_RANGE, "known merge: %llu meta bytes and %llu member records needed", (unsigned long long)mp.info.meta_bytes,
                (unsigned long long)mp.info.members);
  if ((r = merge_place(e, &mp, (uint8_t*)d_out))) return r;
  memcpy(out_meta, mp.meta.data(), mp.meta.size());
  return CTMR_OK;
}

int ctmr_known_merge(ctmr_engine* e, int op, const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, uint8_t* out,
                     size_t cap, ctmr_known_image_info* info) {
  if (!e || !a || !info || (!b && b_len)) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  MergePlan mp;
  mp.op = op;
  DevMem da, db, d_out;
  int r;
  if ((r = merge_check_op(e, op))) return r;
  // both metas before anything is staged
  if ((r = known_open(e, a, a_len, nullptr, "known merge (A)", &mp.a.km))) return r;
  if (b && (r = known_open(e, b, b_len, nullptr, "known merge (B)", &mp.b.km))) return r;
  if ((r = known_stage_members(e, mp.a.km, a, 0, "known merge (A)", &da))) return r;
  if (b && (r = known_stage_members(e, mp.b.km, b, 0, "known merge (B)", &db))) return r;
  if ((r = merge_open(e, da.u8(), "known merge (A)", &mp.a))) return r;
  if ((r = merge_open(e, db.u8(), "known merge (B)", &mp.b))) return r;
  if ((r = merge_prepare(e, &mp))) return r;
  *info = mp.info;
  if (!out || cap < mp.info.image_bytes) return fail(e, CTMR_E_RANGE, "known merge: %llu bytes needed", (unsigned long long)mp.info.image_bytes);
  if (mp.info.members) {
    if (d_out.alloc(mp.info.members * KNOWN_REC_BYTES) != hipSuccess)
      return fail(e, CTMR_E_NOMEM, "known merge: no device memory for %llu member records of the result", (unsigned long long)mp.info.members);
  }
  if ((r = merge_place(e, &mp, d_out.u8()))) return r;
  if (mp.info.members)
    HIPCHK(e, hipMemcpy(out + mp.info.meta_bytes, d_out.p, mp.info.members * KNOWN_REC_BYTES, hipMemcpyDeviceToHost));
  memcpy(out, mp.meta.data(), mp.meta.size());
  return CTMR_OK;
}
