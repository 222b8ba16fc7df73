// engine/split.inc — a known image partitioned by a probe image, the hour as wildcard (include/ctmr.h
// ctmr_known_image_split*, DESIGN.md §28): the member records and host pairs of K's kept sets that equal a probe of P go
// to the image HIT, the others to the image MISS, both in K's order.  Host side: the preparation of the find
// (engine/find.inc: find_prepare, FindTabs), the runs of the mark pass, the scan of the block counts, both results'
// metas from the hits in front of every kept set, the sizing, then the place pass (kernels/split.h).  The two host
// sections meet here by (K ordinal, member).
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after engine/find.inc.

extern "C++" {
namespace {

// One result as the caller wants it.  Host variant: out / cap, the records staged on the device by the core.  Device
// variant: meta / meta_cap and d_rec / rec_cap.  want = false: declined — sized in *info, not written.
struct SplitSide {
  bool want = false, host = false;
  uint8_t* out = nullptr;
  size_t cap = 0;
  uint8_t* meta = nullptr;
  size_t meta_cap = 0;
  uint8_t* d_rec = nullptr;
  uint64_t rec_cap = 0;
  bool fits(const ctmr_known_image_info& i) const {
    if (!want) return true;
    if (host) return cap >= i.image_bytes;
    return meta_cap >= i.meta_bytes && rec_cap >= i.members && (d_rec || !i.members);
  }
};

// The meta of one result: the kept sets of K with a count on this side, in K's order with K's hour; the distinct digests
// they name, ascending; the kept host pairs on this side, in K's order.
void split_meta(const KnownMeta& k, const FindPrep& q, const std::vector<uint64_t>& count, const std::vector<uint8_t>& pair_here,
                std::vector<uint8_t>* meta, ctmr_known_image_info* info) {
  // (an image has many sets and few issuers: the digests are numbered per ordinal of K, not per set)
  std::vector<uint8_t> named(k.n_issuers, 0);
  for (size_t s = 0; s < count.size(); s++)
    if (count[s]) named[k.set_issuer[q.seg_set[s]]] = 1;
  std::vector<const uint8_t*> digs;
  for (uint32_t o = 0; o < k.n_issuers; o++)
    if (named[o]) digs.push_back(k.issuers + (size_t)o * 32);
  known_number_digests(&digs);
  std::vector<uint32_t> renumbered(k.n_issuers, 0);
  for (uint32_t o = 0; o < k.n_issuers; o++)
    if (named[o]) renumbered[o] = known_digest_ordinal(digs, k.issuers + (size_t)o * 32);
  std::vector<KnownSetEntry> sets;
  sets.reserve(count.size());
  for (size_t s = 0; s < count.size(); s++)
    if (count[s]) sets.push_back({q.seg_hour[s], renumbered[k.set_issuer[q.seg_set[s]]], count[s]});
  KnownHostPairs host;
  for (size_t i = 0; i < q.kh.size(); i++)
    if (pair_here[i]) host.push_back(k.host[q.kh[i].at]);
  known_write_meta(digs, sets, host, meta, info);
}

// Both metas are parsed and the member records of both operands are on the device.
int split_core(ctmr_engine* e, const KnownMeta& k, const uint8_t* d_k, const KnownMeta& p, const uint8_t* d_p, int64_t now,
               SplitSide hit, SplitSide miss, ctmr_known_split_info* info) {
  const char* what = "known image split";
  int r;
  FindPrep q;
  if ((r = find_prepare(e, k, d_k, p, d_p, now, hit.d_rec, miss.d_rec, what, &q))) return r;
  const KnownExport& x = q.x;
  const uint64_t K = x.set_range.size(), n_probes = q.n_probes(), n_hr = q.n_hr();
  memset(info, 0, sizeof *info);
  info->probes = q.n_main;
  info->host_probes = q.n_hostp;
  info->sets_kept = q.sets_kept;
  info->members_read = q.kept_records;
  if (K > 0xffffffffull || n_hr > 0xffffffffull || n_probes >= (1ull << 31))
    return fail(e, CTMR_E_NOMEM, "%s: %llu kept sets, %llu probes", what, (unsigned long long)K, (unsigned long long)n_probes);
  // ---- the runs: whole kept sets of at most FIND_CHUNK records; blocks are numbered through all of them, the host
  // pairs' run behind the last
  const std::vector<KnownRun> runs = known_cut_sets(x, known_chunk("CTMR_KNOWN_SPLIT_CHUNK", FIND_CHUNK));
  const uint64_t NB = known_runs_blocks(runs), nb_hr = (n_hr + 255) / 256, nb_build = (n_probes + 255) / 256;
  // ---- every working buffer but the host variant's staged results: the tables in one upload, the probe table and the
  // working hits (the probes' K ordinals), the flags
  const uint64_t forced_slots = env_u64("CTMR_KNOWN_FIND_SLOTS");  // tests only: the smallest table, so that chains are long
  const uint64_t slots = forced_slots ? pow2_at_least(n_probes + 1) : pow2_at_least(std::max<uint64_t>(2 * n_probes, 64));
  FindTabs tb;
  tb.pack(q, p);
  DevMem tabs, work, flags;
  const size_t off_hits = slots * 8;
  const size_t off_ball = (NB + 1) * 8, off_hcnt = off_ball + (NB + nb_hr) * 32, off_before = off_hcnt + nb_hr * 8;
  if (tabs.alloc(tb.pk.b.size()) != hipSuccess || work.alloc(off_hits + (size_t)n_probes * 16 + 16) != hipSuccess ||
      flags.alloc(off_before + (K + 1) * 8) != hipSuccess)
    return fail(e, CTMR_E_NOMEM, "%s: no device memory for a table of %llu words and the flags of %llu records", what,
                (unsigned long long)slots, (unsigned long long)q.kept_records);
  if ((r = ensure(e, SC_MISC, ((NB + 1 + SCAN_TILE) / SCAN_TILE) * 8))) return r;
  HIPCHK(e, hipMemcpyAsync(tabs.p, tb.pk.b.data(), tb.pk.b.size(), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemsetAsync(work.p, 0, off_hits, e->stream));
  HIPCHK(e, hipMemsetAsync(flags.p, 0, off_ball, e->stream));
  const uint8_t* t8 = tabs.u8();
  uint32_t* d_err = (uint32_t*)(t8 + tb.o_err);
  uint4* d_work = (uint4*)(work.u8() + off_hits);
  unsigned long long* d_cnt = (unsigned long long*)flags.p;
  unsigned long long* d_before = (unsigned long long*)(flags.u8() + off_before);
  const KnownFlags sf{(unsigned long long*)(flags.u8() + off_ball), d_cnt};
  const KnownFlags sf_hr{sf.ball + NB * 4, (unsigned long long*)(flags.u8() + off_hcnt)};
  const FindProbes fp = tb.probes(q, p, t8, d_p);
  const FindTable ft{(unsigned long long*)work.p, slots - 1};
  // ---- build, then the mark pass over the runs of K and over the host pairs' run: every record of P and of a kept set
  // of K is validated here, before anything is written
  if (n_probes) hipLaunchKernelGGL(k_find_build, dim3((unsigned)nb_build), dim3(256), 0, e->stream, fp, ft, d_work, d_err);
  for (const KnownRun& run : runs)
    hipLaunchKernelGGL(k_split_mark, dim3((unsigned)run.blocks()), dim3(256), 0, e->stream, tb.run(t8, d_k, run.s_lo, run.s_hi), run.n, ft,
                       fp, n_probes, (const uint4*)d_work, sf, run.blk0, d_err);
  if (n_hr)
    hipLaunchKernelGGL(k_split_mark, dim3((unsigned)nb_hr), dim3(256), 0, e->stream, tb.host_run(q, t8), n_hr, ft, fp, q.n_main,
                       (const uint4*)d_work, sf_hr, (uint64_t)0, d_err);
  // ---- the hits in front of every block (one scan through all runs: the base carries from run to run in cnt[]) and
  // in front of every kept set
  if ((r = scan_u64(e, (uint64_t*)d_cnt, NB + 1, false, SC_MISC))) return r;
  for (const KnownRun& run : runs)
    hipLaunchKernelGGL(k_split_sets, dim3((unsigned)((run.s_hi - run.s_lo + 255) / 256)), dim3(256), 0, e->stream,
                       tb.run(t8, d_k, run.s_lo, run.s_hi), sf, run.blk0, d_before + run.s_lo);
  uint32_t err = 0;
  std::vector<unsigned long long> before(K + 1, 0ull), hr_ball(nb_hr * 4);
  HIPCHK(e, hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, e->stream));
  if (K) HIPCHK(e, hipMemcpyAsync(before.data(), d_before, K * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(&before[K], d_cnt + NB, 8, hipMemcpyDeviceToHost, e->stream));
  if (n_hr) HIPCHK(e, hipMemcpyAsync(hr_ball.data(), sf_hr.ball, nb_hr * 32, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  if ((r = known_record_error(e, err, what))) return r;
  // ---- every record is valid: both results' sets, the host pairs' sides, the metas
  std::vector<uint64_t> n_hit(K), n_miss(K);
  for (uint64_t s = 0; s < K; s++) {
    n_hit[s] = before[s + 1] - before[s];
    n_miss[s] = x.set_range[s].second - n_hit[s];
  }
  std::vector<uint8_t> pair_hit(q.kh.size(), 0), pair_miss(q.kh.size(), 0);
  {
    std::set<std::pair<uint32_t, std::string>> p_host;  // P's host-section members by (K ordinal, member)
    for (size_t j = 0; j < q.n_hostp; j++)
      if (q.p_host_kord[j] != FIND_NO_ISSUER) p_host.insert({q.p_host_kord[j], p.host[j].second});
    for (size_t i = 0; i < q.kh.size(); i++) pair_hit[i] = p_host.count({q.kh[i].kord, *q.kh[i].member}) != 0;
    for (uint64_t i = 0; i < n_hr; i++)
      if ((hr_ball[i >> 6] >> (i & 63)) & 1ull) pair_hit[q.hr_of[i]] = 1;
    for (size_t i = 0; i < q.kh.size(); i++) pair_miss[i] = !pair_hit[i];
  }
  std::vector<uint8_t> hit_meta, miss_meta;
  split_meta(k, q, n_hit, pair_hit, &hit_meta, &info->hit);
  split_meta(k, q, n_miss, pair_miss, &miss_meta, &info->miss);
  if (!hit.fits(info->hit) || !miss.fits(info->miss))
    return fail(e, CTMR_E_RANGE, "%s: %llu meta bytes and %llu member records needed for HIT, %llu and %llu for MISS", what,
                (unsigned long long)info->hit.meta_bytes, (unsigned long long)info->hit.members, (unsigned long long)info->miss.meta_bytes,
                (unsigned long long)info->miss.members);
  // ---- the host variant's results are staged on the device: the last working buffers
  DevMem stage_hit, stage_miss;
  if (hit.want && hit.host && info->hit.members) {
    if (stage_hit.alloc(info->hit.members * KNOWN_REC_BYTES) != hipSuccess)
      return fail(e, CTMR_E_NOMEM, "%s: no device memory to stage %llu member records", what, (unsigned long long)info->hit.members);
    hit.d_rec = stage_hit.u8();
  }
  if (miss.want && miss.host && info->miss.members) {
    if (stage_miss.alloc(info->miss.members * KNOWN_REC_BYTES) != hipSuccess)
      return fail(e, CTMR_E_NOMEM, "%s: no device memory to stage %llu member records", what, (unsigned long long)info->miss.members);
    miss.d_rec = stage_miss.u8();
  }
  // ---- the place pass: a side that is declined, or empty, is not stored
  uint8_t* to_hit = hit.want && info->hit.members ? hit.d_rec : nullptr;
  uint8_t* to_miss = miss.want && info->miss.members ? miss.d_rec : nullptr;
  if (to_hit || to_miss)
    for (const KnownRun& run : runs)
      hipLaunchKernelGGL(k_split_place, dim3((unsigned)run.blocks()), dim3(256), 0, e->stream, tb.run(t8, d_k, run.s_lo, run.s_hi), run.n, sf,
                         run.blk0, to_hit, to_miss);
  // ---- each wanted image out: its meta, and for the host variant the staged records behind it
  auto deliver = [&](const SplitSide& s, const std::vector<uint8_t>& m, uint64_t members) -> int {
    if (!s.want) return CTMR_OK;
    memcpy(s.host ? s.out : s.meta, m.data(), m.size());
    if (s.host && members)
      HIPCHK(e, hipMemcpyAsync(s.out + m.size(), s.d_rec, members * KNOWN_REC_BYTES, hipMemcpyDeviceToHost, e->stream));
    return CTMR_OK;
  };
  if ((r = deliver(hit, hit_meta, info->hit.members)) || (r = deliver(miss, miss_meta, info->miss.members))) return r;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  return CTMR_OK;
}

}  // namespace
}  // extern "C++"

int ctmr_known_image_split(ctmr_engine* e, const uint8_t* known, size_t known_len, const uint8_t* probes, size_t probes_len,
                           int64_t now_unix, uint8_t* hit_out, size_t hit_cap, uint8_t* miss_out, size_t miss_cap,
                           ctmr_known_split_info* info) {
  if (!e || !known || !probes || !info) return CTMR_E_INVAL;
  if ((!hit_out && hit_cap) || (!miss_out && miss_cap)) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  KnownMeta k, p;
  DevMem dk, dp;
  int r;
  if ((r = known_open(e, known, known_len, nullptr, "known image split (K)", &k))) return r;
  if ((r = known_open(e, probes, probes_len, nullptr, "known image split (P)", &p))) return r;
  if ((r = known_stage_members(e, k, known, 0, "known image split (K)", &dk))) return r;
  if ((r = known_stage_members(e, p, probes, 0, "known image split (P)", &dp))) return r;
  SplitSide hit, miss;
  hit.want = hit_out != nullptr; hit.host = true; hit.out = hit_out; hit.cap = hit_cap;
  miss.want = miss_out != nullptr; miss.host = true; miss.out = miss_out; miss.cap = miss_cap;
  return split_core(e, k, dk.u8(), p, dp.u8(), now_unix, hit, miss, info);
}

int ctmr_known_image_split_device(ctmr_engine* e, const uint8_t* k_meta, size_t k_meta_len, const void* d_k_members, uint64_t k_members,
                                  const uint8_t* p_meta, size_t p_meta_len, const void* d_p_members, uint64_t p_members, int64_t now_unix,
                                  uint8_t* hit_meta, size_t hit_meta_cap, void* d_hit, uint64_t hit_members_cap,
                                  uint8_t* miss_meta, size_t miss_meta_cap, void* d_miss, uint64_t miss_members_cap,
                                  ctmr_known_split_info* info) {
  if (!e || !k_meta || !p_meta || !info) return CTMR_E_INVAL;
  if ((!hit_meta && (hit_meta_cap || d_hit || hit_members_cap)) || (!miss_meta && (miss_meta_cap || d_miss || miss_members_cap)))
    return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  KnownMeta k, p;
  int r;
  if ((r = known_open(e, k_meta, k_meta_len, &k_members, "known image split (K)", &k))) return r;
  if ((r = known_open(e, p_meta, p_meta_len, &p_members, "known image split (P)", &p))) return r;
  SplitSide hit, miss;
  hit.want = hit_meta != nullptr; hit.meta = hit_meta; hit.meta_cap = hit_meta_cap; hit.d_rec = (uint8_t*)d_hit; hit.rec_cap = hit_members_cap;
  miss.want = miss_meta != nullptr; miss.meta = miss_meta; miss.meta_cap = miss_meta_cap; miss.d_rec = (uint8_t*)d_miss; miss.rec_cap = miss_members_cap;
  return split_core(e, k, (const uint8_t*)d_k_members, p, (const uint8_t*)d_p_members, now_unix, hit, miss, info);
}
