// engine/crl.inc — DER CertificateLists → a probe image (include/ctmr.h ctmr_crl_probes*, DESIGN.md §26).  The blob stays
// where it lies; kernels/crl.h walks every CRL's outer TLVs and marks the entry candidates, the cuts, conflict-region,
// compaction and chain kernels of kernels/resp_parse.h keep the sequential parse, and the place pass writes the member
// records.  The host sees one span and one record count per CRL and the serials above 40 octets, which are rare: it
// folds the CRLs into sets by digest, orders the sets by Issuer.ID, gives every CRL its place and writes the meta.
// ctmr_crl_probes_each* (DESIGN.md §27) is the same core with a finding per CRL: the head and the chain check write
// bad_at[k], the class pass makes every token of a CRL with a finding a frame, and the fold leaves those CRLs out.
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after engine/resp_parse.inc.

extern "C++" {
namespace {

struct CrlProbes {
  // the tables the place pass reads
  DevMem cls, tok_crl, tok_ser, rec_before, crl_rec0, crl_dst;
  const uint8_t* s = nullptr;
  uint64_t ntok = 0;
  std::vector<uint8_t> meta;
  ctmr_known_image_info info{};
  ctmr_crl_info cinfo{};
  std::vector<ctmr_crl_verdict> verdicts;  // the each form: one per CRL
};

const char* const CRL_PROBES = "crl probes";

int crl_bad(ctmr_engine* e, CrlProbes* P, uint64_t crl, uint64_t at, const char* saying) {
  P->cinfo.bad_crl = crl;
  P->cinfo.bad_offset = at;
  return fail(e, CTMR_E_INVAL, "%s: CRL %llu, offset %llu: %s", CRL_PROBES, (unsigned long long)crl, (unsigned long long)at, saying);
}

// What needs no byte of the blob: the length, the pointers, the offsets.
int crl_args(ctmr_engine* e, const void* crls, uint64_t len, const uint64_t* offsets, uint32_t n, const uint8_t* digests, CrlProbes* P) {
  memset(&P->cinfo, 0, sizeof P->cinfo);
  P->cinfo.crls = n;
  P->cinfo.bad_crl = P->cinfo.bad_offset = UINT64_MAX;
  if (len >= RP_MAX_LEN)
    return fail(e, CTMR_E_INVAL, "%s: %llu bytes: a blob of 2^32 - 64 bytes or more is split between two CRLs", CRL_PROBES, (unsigned long long)len);
  if (!offsets || (len && !crls) || (n && !digests)) return fail(e, CTMR_E_INVAL, "%s: null blob, offsets or digests", CRL_PROBES);
  if (offsets[0] != 0) return crl_bad(e, P, 0, 0, "offsets[0] is not 0");
  for (uint32_t k = 0; k < n; k++)
    if (offsets[k + 1] < offsets[k]) return crl_bad(e, P, k, offsets[k], "the offsets do not ascend");
  if (offsets[n] != len) return crl_bad(e, P, n, len, "the last offset is not the blob's length");
  return CTMR_OK;
}

// Everything but the records: the blob (device memory, any alignment) validated, P->meta, P->info and P->cinfo made, the
// tables of the place pass left on the device.  Drains the stream.  each: a CRL outside the grammar fails nothing; it
// gets its verdict in P->verdicts and contributes nothing.
int crl_core(ctmr_engine* e, const uint8_t* s, uint64_t len, const uint64_t* offsets, uint32_t n, const uint8_t* digests, CrlProbes* P,
             bool each) {
  int r;
  P->s = s;
  memset(&P->info, 0, sizeof P->info);
  if (each) P->verdicts.assign(n, ctmr_crl_verdict{UINT64_MAX, 0u, 0u});
  if (!n) {  // (len == 0: the offsets said so)
    known_write_meta({}, {}, {}, &P->meta, &P->info);
    return CTMR_OK;
  }
  if (!len && !each) return crl_bad(e, P, 0, 0, "a CRL of 0 bytes");
  if (!len) {  // every CRL is one of 0 bytes, bad at offset 0: no launch over an empty range
    for (ctmr_crl_verdict& v : P->verdicts) v.bad_offset = 0;
    P->cinfo.bad_crl = P->cinfo.bad_offset = 0;
    known_write_meta({}, {}, {}, &P->meta, &P->info);
    return CTMR_OK;
  }
  const uint64_t nb = (len + RP_TILE - 1) / RP_TILE;
  DevMem off_m, span_m, tile_m, tok_pos;
  RpStage st;  // err[0]: the head's finding (CRL << 32 | offset), err[1]: the chain's (offset); each: err[2 + k] = bad_at[k]
  if ((r = rp_alloc(e, &off_m, ((size_t)n + 1) * 8, CRL_PROBES)) || (r = rp_alloc(e, &span_m, (size_t)n * 8, CRL_PROBES)) ||
      (r = rp_alloc(e, &tile_m, (nb + 1) * 4, CRL_PROBES)) || (r = st.begin(e, CRL_PROBES, len, ~0ull, each ? n : 0u)))
    return r;
  unsigned long long* const cnt = st.cnt;
  HIPCHK(e, hipMemcpyAsync(off_m.p, offsets, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, e->stream));
  const CrlBlob B{s, len, (const unsigned long long*)off_m.p, (const uint2*)span_m.p, n};
  const CrlCand C{B, (const uint32_t*)tile_m.p};
  // ---- head, then candidates → tokens (engine/resp_parse.inc RpStage)
  unsigned long long* const bad_at = st.err + 2;
  if (each)
    hipLaunchKernelGGL(k_crl_head<true>, dim3(rp_grid(n, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, s, B.off, n, (uint2*)span_m.p, bad_at);
  else
    hipLaunchKernelGGL(k_crl_head<false>, dim3(rp_grid(n, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, s, B.off, n, (uint2*)span_m.p, st.err);
  hipLaunchKernelGGL(k_crl_tiles, dim3(rp_grid(nb + 1, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, B.off, n, nb, (uint32_t*)tile_m.p);
  if ((r = st.count(e, C))) return r;
  std::vector<uint2> span(n);
  HIPCHK(e, hipMemcpy(span.data(), span_m.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  std::vector<unsigned long long> h(2 + (each ? (size_t)n : 0), 0);  // each: h[2 + k] = bad_at[k]
  {  // (nc >= 1: byte 0 starts a CRL and is a frame)
    DevMem tok_nxt;
    if ((r = st.tokens<false>(e, C, s, &tok_pos, &tok_nxt, nullptr, nullptr, nullptr, each ? nullptr : st.err + 1))) return r;
    if (each)
      hipLaunchKernelGGL(k_crl_chain, dim3(rp_grid(st.ntok, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, (const uint32_t*)tok_pos.p,
                         (const uint32_t*)tok_nxt.p, st.ntok, len, B.off, n, bad_at);
    HIPCHK(e, hipMemcpyAsync(h.data(), st.err, h.size() * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipGetLastError());
    // the lowest CRL: a CRL the head refused has no entry candidates, so the two findings never name the same one
    // (the each form leaves both words as they were preset: its findings are in bad_at)
    const uint64_t head_crl = h[0] == ~0ull ? UINT64_MAX : h[0] >> 32;
    uint64_t chain_crl = UINT64_MAX;
    if (h[1] != ~0ull) chain_crl = (uint64_t)(std::upper_bound(offsets, offsets + n + 1, (uint64_t)h[1]) - offsets) - 1;
    if (head_crl != UINT64_MAX && head_crl < chain_crl)
      return crl_bad(e, P, head_crl, h[0] & 0xffffffffull, "not the TLV a CertificateList has here, or not a definite minimal length inside its structure");
    if (chain_crl != UINT64_MAX)
      return crl_bad(e, P, chain_crl, h[1], "not SEQUENCE { INTEGER, Time, optional SEQUENCE } filled exactly inside revokedCertificates");
    st.drop();
  }
  const uint64_t nc = st.nc, nt = P->ntok = st.ntok;
  // ---- classes, records per CRL, host pairs
  uint64_t nrec = 0, npair = 0;
  DevMem pair_before, pairs_m;
  if ((r = rp_alloc(e, &P->cls, nt, CRL_PROBES)) || (r = rp_alloc(e, &P->tok_crl, nt * 4, CRL_PROBES)) ||
      (r = rp_alloc(e, &P->tok_ser, nt * 4, CRL_PROBES)) || (r = rp_alloc(e, &P->rec_before, nt * 4, CRL_PROBES)) ||
      (r = rp_alloc(e, &pair_before, nt * 4, CRL_PROBES)) || (r = rp_alloc(e, &P->crl_rec0, (size_t)n * 4, CRL_PROBES)) ||
      (r = rp_alloc(e, &P->crl_dst, (size_t)n * 8, CRL_PROBES)))
    return r;
  if (each)
    hipLaunchKernelGGL((k_crl_class<true, const unsigned long long*>), dim3(rp_grid(nt, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, B,
                       (const uint32_t*)tok_pos.p, nt, P->cls.u8(), (uint32_t*)P->tok_crl.p, (uint32_t*)P->tok_ser.p,
                       (const unsigned long long*)bad_at);
  else
    hipLaunchKernelGGL(k_crl_class<false>, dim3(rp_grid(nt, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, B, (const uint32_t*)tok_pos.p, nt,
                       P->cls.u8(), (uint32_t*)P->tok_crl.p, (uint32_t*)P->tok_ser.p);
  if ((r = rp_flag_scan(e, P->cls.u8(), nt, CRL_RECORD, cnt, (uint32_t*)P->rec_before.p, &nrec))) return r;
  if ((r = rp_flag_scan(e, P->cls.u8(), nt, CRL_PAIR, cnt, (uint32_t*)pair_before.p, &npair))) return r;
  hipLaunchKernelGGL(k_crl_starts, dim3(rp_grid(nt, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, B, (const uint32_t*)tok_pos.p,
                     (const uint32_t*)P->tok_crl.p, (const uint32_t*)P->rec_before.p, nt, (uint32_t*)P->crl_rec0.p);
  std::vector<uint32_t> rec0(n);
  std::vector<uint4> pairs(npair);
  HIPCHK(e, hipMemcpyAsync(rec0.data(), P->crl_rec0.p, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
  if (npair) {
    if ((r = rp_alloc(e, &pairs_m, npair * 16, CRL_PROBES))) return r;
    hipLaunchKernelGGL(k_crl_pairs, dim3(rp_grid(nt, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, B, (const uint8_t*)P->cls.u8(),
                       (const uint32_t*)P->tok_crl.p, (const uint32_t*)P->tok_ser.p, (const uint32_t*)pair_before.p, nt, (uint4*)pairs_m.p);
    HIPCHK(e, hipMemcpyAsync(pairs.data(), pairs_m.p, npair * 16, hipMemcpyDeviceToHost, e->stream));
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  // ---- the serials above 40 octets
  std::vector<uint2> seg;
  seg.reserve(npair);
  for (const uint4& x : pairs) seg.push_back(make_uint2(x.x, x.y));
  std::vector<unsigned long long> dst;
  std::vector<uint8_t> bytes;
  if ((r = rp_gather(e, CRL_PROBES, s, seg, &dst, &bytes))) return r;
  // ---- CRLs → sets by digest, the sets in Issuer.ID order, every CRL's place in its set
  auto dig = [&](uint32_t k) { return digests + (size_t)k * 32; };
  std::vector<uint64_t> count(n);
  std::vector<const uint8_t*> digs;
  // a CRL of 0 bytes has no byte, no front frame and so no crl_rec0 of its own (the each form gets here with some): it
  // starts where the CRL behind it starts
  for (uint32_t k = n; k-- > 0;)
    if (offsets[k + 1] == offsets[k]) rec0[k] = k + 1 < n ? rec0[k + 1] : (uint32_t)nrec;
  auto bad = [&](uint32_t k) { return each && h[2 + k] != ~0ull; };  // (its tokens are frames: it has no record and no pair)
  for (uint32_t k = 0; k < n; k++) {
    count[k] = (k + 1 < n ? rec0[k + 1] : nrec) - rec0[k];
    if (bad(k)) continue;
    if (count[k]) digs.push_back(dig(k));
    if (span[k].x == span[k].y) P->cinfo.empty_crls++;
  }
  known_number_digests(&digs);
  std::vector<std::string> ids(digs.size());
  std::vector<uint32_t> by_id(digs.size());
  for (size_t i = 0; i < digs.size(); i++) {
    ids[i] = b64url(digs[i], 32);
    by_id[i] = (uint32_t)i;
  }
  std::sort(by_id.begin(), by_id.end(), [&](uint32_t a, uint32_t b) { return ids[a] < ids[b]; });
  std::vector<uint64_t> set_count(digs.size(), 0), set_at(digs.size(), 0);
  std::vector<uint32_t> ord(n, 0);
  for (uint32_t k = 0; k < n; k++)
    if (count[k]) {
      ord[k] = known_digest_ordinal(digs, dig(k));
      set_count[ord[k]] += count[k];
    }
  std::vector<KnownSetEntry> sets;
  uint64_t first = 0;
  for (uint32_t o : by_id) {
    sets.push_back({0, o, set_count[o]});
    set_at[o] = first;
    first += set_count[o];
  }
  std::vector<unsigned long long> crl_dst(n, 0);
  for (uint32_t k = 0; k < n; k++)
    if (count[k]) {
      crl_dst[k] = set_at[ord[k]];
      set_at[ord[k]] += count[k];
    }
  if (first != nrec) return fail(e, CTMR_E_HIP, "%s: the CRLs hold %llu records, the blob %llu", CRL_PROBES, (unsigned long long)first, (unsigned long long)nrec);
  KnownHostPairs host(npair);
  for (uint64_t p = 0; p < npair; p++)
    host[p] = {"serials::" + exp_date_id(0) + "::" + b64url(dig(pairs[p].z), 32),
               std::string((const char*)bytes.data() + dst[p], (size_t)(dst[p + 1] - dst[p]))};
  known_finish_pairs(&host);
  known_write_meta(digs, sets, host, &P->meta, &P->info);
  P->cinfo.candidates = nc;
  P->cinfo.entries = nrec + npair;
  P->cinfo.records = nrec;
  P->cinfo.host_members = host.size();
  if (each) {
    for (uint32_t k = n; k-- > 0;)
      if (bad(k)) {
        P->verdicts[k].bad_offset = h[2 + k];
        P->cinfo.bad_crl = k;
        P->cinfo.bad_offset = h[2 + k];
      } else {
        P->verdicts[k].records = (uint32_t)count[k];
      }
    for (const uint4& x : pairs) P->verdicts[x.z].long_entries++;
  }
  HIPCHK(e, hipMemcpyAsync(P->crl_dst.p, crl_dst.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));  // (crl_dst goes out of scope)
  return CTMR_OK;
}

// The place pass as rp_emit_* take it: info.members records to d.
auto crl_place(ctmr_engine* e, const CrlProbes& P) {
  return [e, &P](uint8_t* d) {
    hipLaunchKernelGGL(k_crl_place, dim3(rp_grid(P.ntok, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, P.s, (const uint8_t*)P.cls.u8(),
                       (const uint32_t*)P.tok_crl.p, (const uint32_t*)P.tok_ser.p, (const uint32_t*)P.rec_before.p,
                       (const uint32_t*)P.crl_rec0.p, (const unsigned long long*)P.crl_dst.p, P.ntok, d);
  };
}

}  // namespace
}  // extern "C++"

int ctmr_crl_probes_device(ctmr_engine* e, const void* d_crls, uint64_t len, const uint64_t* offsets, uint32_t n_crls, const uint8_t* digests,
                           uint8_t* meta, size_t meta_cap, void* d_members, uint64_t members_cap, ctmr_known_image_info* info,
                           ctmr_crl_info* cinfo) {
  if (!e || !info || !cinfo) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  CrlProbes P;
  int r = crl_args(e, d_crls, len, offsets, n_crls, digests, &P);
  if (!r) r = crl_core(e, (const uint8_t*)d_crls, len, offsets, n_crls, digests, &P, false);
  *cinfo = P.cinfo;
  if (r) return r;
  return rp_emit_device(e, CRL_PROBES, P.meta, P.info, crl_place(e, P), meta, meta_cap, d_members, members_cap, info);
}

int ctmr_crl_probes_each_device(ctmr_engine* e, const void* d_crls, uint64_t len, const uint64_t* offsets, uint32_t n_crls,
                                const uint8_t* digests, uint8_t* meta, size_t meta_cap, void* d_members, uint64_t members_cap,
                                ctmr_known_image_info* info, ctmr_crl_info* cinfo, ctmr_crl_verdict* verdicts) {
  if (!e || !info || !cinfo) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  CrlProbes P;
  int r = crl_args(e, d_crls, len, offsets, n_crls, digests, &P);
  if (!r) r = crl_core(e, (const uint8_t*)d_crls, len, offsets, n_crls, digests, &P, true);
  *cinfo = P.cinfo;
  if (!r) r = rp_emit_device(e, CRL_PROBES, P.meta, P.info, crl_place(e, P), meta, meta_cap, d_members, members_cap, info);
  if (!r && verdicts && n_crls) memcpy(verdicts, P.verdicts.data(), (size_t)n_crls * sizeof *verdicts);
  return r;
}

int ctmr_crl_probes(ctmr_engine* e, const uint8_t* crls, size_t len, const uint64_t* offsets, uint32_t n_crls, const uint8_t* digests, uint8_t* out,
                    size_t cap, ctmr_known_image_info* info, ctmr_crl_info* cinfo) {
  if (!e || !info || !cinfo) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  CrlProbes P;
  DevMem d_crls;
  int r = crl_args(e, crls, len, offsets, n_crls, digests, &P);
  if (!r) r = rp_stage(e, CRL_PROBES, crls, len, &d_crls);
  if (!r) r = crl_core(e, d_crls.u8(), len, offsets, n_crls, digests, &P, false);
  *cinfo = P.cinfo;
  if (r) return r;
  return rp_emit_host(e, CRL_PROBES, P.meta, P.info, crl_place(e, P), out, cap, info);
}

int ctmr_crl_probes_each(ctmr_engine* e, const uint8_t* crls, size_t len, const uint64_t* offsets, uint32_t n_crls, const uint8_t* digests,
                         uint8_t* out, size_t cap, ctmr_known_image_info* info, ctmr_crl_info* cinfo, ctmr_crl_verdict* verdicts) {
  if (!e || !info || !cinfo) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  CrlProbes P;
  DevMem d_crls;
  int r = crl_args(e, crls, len, offsets, n_crls, digests, &P);
  if (!r) r = rp_stage(e, CRL_PROBES, crls, len, &d_crls);
  if (!r) r = crl_core(e, d_crls.u8(), len, offsets, n_crls, digests, &P, true);
  *cinfo = P.cinfo;
  if (!r) r = rp_emit_host(e, CRL_PROBES, P.meta, P.info, crl_place(e, P), out, cap, info);
  if (!r && verdicts && n_crls) memcpy(verdicts, P.verdicts.data(), (size_t)n_crls * sizeof *verdicts);
  return r;
}
