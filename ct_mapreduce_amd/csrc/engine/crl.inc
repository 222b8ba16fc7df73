// engine/crl.inc — DER CertificateLists → a probe image (include/ctmr.h ctmr_crl_probes*, DESIGN.md §26).  The blob stays
// where it lies; kernels/crl.h walks every CRL's outer TLVs and marks the entry candidates, the cuts, conflict-region,
// compaction and chain kernels of kernels/resp_parse.h keep the sequential parse, and the place pass writes the member
// records.  The host sees one span and one record count per CRL and the serials above 40 octets, which are rare: it
// folds the CRLs into sets by digest, orders the sets by Issuer.ID, gives every CRL its place and writes the meta.
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
};

const char* const CRL_PROBES = "crl probes";

int crl_alloc(ctmr_engine* e, DevMem* m, size_t bytes) { return rp_alloc(e, m, bytes, CRL_PROBES); }

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
// tables of the place pass left on the device.  Drains the stream.
int crl_core(ctmr_engine* e, const uint8_t* s, uint64_t len, const uint64_t* offsets, uint32_t n, const uint8_t* digests, CrlProbes* P) {
  int r;
  P->s = s;
  memset(&P->info, 0, sizeof P->info);
  if (!n) {  // (len == 0: the offsets said so)
    known_write_meta({}, {}, {}, &P->meta, &P->info);
    return CTMR_OK;
  }
  if (!len) return crl_bad(e, P, 0, 0, "a CRL of 0 bytes");
  const uint64_t nb = (len + RP_TILE - 1) / RP_TILE;
  DevMem off_m, span_m, tile_m, cnt_m, err_m, cand_m, nxt_m, flag_m, bm_m, tidx_m, tok_pos, tok_nxt, tok_hdr, star;
  if ((r = crl_alloc(e, &off_m, ((size_t)n + 1) * 8)) || (r = crl_alloc(e, &span_m, (size_t)n * 8)) || (r = crl_alloc(e, &tile_m, (nb + 1) * 4)) ||
      (r = crl_alloc(e, &cnt_m, (nb + 2) * 8)) || (r = crl_alloc(e, &err_m, 16)))
    return r;
  unsigned long long* cnt = (unsigned long long*)cnt_m.p;
  unsigned long long* err = (unsigned long long*)err_m.p;
  const unsigned long long err0[2] = {~0ull, ~0ull};  // the head's finding (CRL << 32 | offset), the chain's (offset)
  HIPCHK(e, hipMemcpyAsync(err, err0, 16, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(off_m.p, offsets, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, e->stream));
  const CrlBlob B{s, len, (const unsigned long long*)off_m.p, (const uint2*)span_m.p, n};
  // ---- head, mark
  hipLaunchKernelGGL(k_crl_head, dim3(rp_grid(n, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, s, B.off, n, (uint2*)span_m.p, err);
  hipLaunchKernelGGL(k_crl_tiles, dim3(rp_grid(nb + 1, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, B.off, n, nb, (uint32_t*)tile_m.p);
  HIPCHK(e, hipMemsetAsync(cnt + nb, 0, 8, e->stream));
  hipLaunchKernelGGL((k_crl_mark<false>), dim3((unsigned)nb), dim3(RP_BLOCK), 0, e->stream, B, (const uint32_t*)tile_m.p, cnt, (uint32_t*)nullptr,
                     (uint32_t*)nullptr);
  uint64_t nc = 0;
  if ((r = scan_total(e, (uint64_t*)cnt, nb + 1, false, SC_MISC, &nc))) return r;
  std::vector<uint2> span(n);
  HIPCHK(e, hipMemcpy(span.data(), span_m.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  // (nc >= 1: byte 0 starts a CRL and is a frame)
  const uint64_t ncb = (nc + RP_TILE - 1) / RP_TILE;
  if ((r = crl_alloc(e, &cand_m, nc * 4)) || (r = crl_alloc(e, &nxt_m, nc * 4)) || (r = crl_alloc(e, &flag_m, nc)) ||
      (r = crl_alloc(e, &bm_m, ncb * 4)) || (r = crl_alloc(e, &tidx_m, nc * 4)))
    return r;
  uint32_t* cand = (uint32_t*)cand_m.p;
  uint32_t* nxt = (uint32_t*)nxt_m.p;
  hipLaunchKernelGGL((k_crl_mark<true>), dim3((unsigned)nb), dim3(RP_BLOCK), 0, e->stream, B, (const uint32_t*)tile_m.p, cnt, cand, nxt);
  // ---- cuts, conflict regions, the kept candidates, and the proof that they are the chain: kernels/resp_parse.h
  hipLaunchKernelGGL(k_resp_blockmax, dim3((unsigned)ncb), dim3(RP_BLOCK), 0, e->stream, (const uint32_t*)nxt, (uint64_t)nc, (uint32_t*)bm_m.p);
  hipLaunchKernelGGL(k_resp_maxscan, dim3(1), dim3(1024), 0, e->stream, (uint32_t*)bm_m.p, ncb);
  hipLaunchKernelGGL(k_resp_cuts, dim3((unsigned)ncb), dim3(RP_BLOCK), 0, e->stream, (const uint32_t*)cand, (const uint32_t*)nxt, (uint64_t)nc,
                     (const uint32_t*)bm_m.p, flag_m.u8());
  hipLaunchKernelGGL(k_resp_resolve, dim3(rp_grid(nc, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, (const uint32_t*)cand, (const uint32_t*)nxt,
                     (uint64_t)nc, flag_m.u8());
  if ((r = rp_flag_scan(e, flag_m.u8(), nc, 3u, cnt, (uint32_t*)tidx_m.p, &P->ntok))) return r;
  const uint64_t nt = P->ntok;  // (>= 1: candidate 0 is a cut)
  if ((r = crl_alloc(e, &tok_pos, nt * 4)) || (r = crl_alloc(e, &tok_nxt, nt * 4)) || (r = crl_alloc(e, &tok_hdr, nt)) || (r = crl_alloc(e, &star, nt)))
    return r;
  hipLaunchKernelGGL(k_resp_tokens, dim3(rp_grid(nc, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, s, len, (const uint32_t*)cand, (const uint32_t*)nxt,
                     (const uint8_t*)flag_m.u8(), (const uint32_t*)tidx_m.p, (uint64_t)nc, (uint32_t*)tok_pos.p, (uint32_t*)tok_nxt.p, tok_hdr.u8(),
                     star.u8());
  hipLaunchKernelGGL(k_resp_chain_from0, dim3(rp_grid(nt, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, (const uint32_t*)tok_pos.p,
                     (const uint32_t*)tok_nxt.p, nt, len, err + 1);
  unsigned long long h[2] = {0, 0};
  HIPCHK(e, hipMemcpyAsync(h, err, 16, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  // the lowest CRL: a CRL the head refused has no entry candidates, so the two findings never name the same one
  const uint64_t head_crl = h[0] == ~0ull ? UINT64_MAX : h[0] >> 32;
  uint64_t chain_crl = UINT64_MAX;
  if (h[1] != ~0ull) chain_crl = (uint64_t)(std::upper_bound(offsets, offsets + n + 1, (uint64_t)h[1]) - offsets) - 1;
  if (head_crl != UINT64_MAX && head_crl < chain_crl)
    return crl_bad(e, P, head_crl, h[0] & 0xffffffffull, "not the TLV a CertificateList has here, or not a definite minimal length inside its structure");
  if (chain_crl != UINT64_MAX)
    return crl_bad(e, P, chain_crl, h[1], "not SEQUENCE { INTEGER, Time, optional SEQUENCE } filled exactly inside revokedCertificates");
  rp_free(&cand_m);
  rp_free(&nxt_m);
  rp_free(&flag_m);
  rp_free(&bm_m);
  rp_free(&tidx_m);
  rp_free(&tok_nxt);
  rp_free(&tok_hdr);
  rp_free(&star);
  // ---- classes, records per CRL, host pairs
  uint64_t nrec = 0, npair = 0;
  DevMem pair_before, pairs_m;
  if ((r = crl_alloc(e, &P->cls, nt)) || (r = crl_alloc(e, &P->tok_crl, nt * 4)) || (r = crl_alloc(e, &P->tok_ser, nt * 4)) ||
      (r = crl_alloc(e, &P->rec_before, nt * 4)) || (r = crl_alloc(e, &pair_before, nt * 4)) || (r = crl_alloc(e, &P->crl_rec0, (size_t)n * 4)) ||
      (r = crl_alloc(e, &P->crl_dst, (size_t)n * 8)))
    return r;
  hipLaunchKernelGGL(k_crl_class, dim3(rp_grid(nt, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, B, (const uint32_t*)tok_pos.p, nt, P->cls.u8(),
                     (uint32_t*)P->tok_crl.p, (uint32_t*)P->tok_ser.p);
  if ((r = rp_flag_scan(e, P->cls.u8(), nt, CRL_RECORD, cnt, (uint32_t*)P->rec_before.p, &nrec))) return r;
  if ((r = rp_flag_scan(e, P->cls.u8(), nt, CRL_PAIR, cnt, (uint32_t*)pair_before.p, &npair))) return r;
  hipLaunchKernelGGL(k_crl_starts, dim3(rp_grid(nt, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, B, (const uint32_t*)tok_pos.p,
                     (const uint32_t*)P->tok_crl.p, (const uint32_t*)P->rec_before.p, nt, (uint32_t*)P->crl_rec0.p);
  std::vector<uint32_t> rec0(n);
  std::vector<uint4> pairs(npair);
  HIPCHK(e, hipMemcpyAsync(rec0.data(), P->crl_rec0.p, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
  if (npair) {
    if ((r = crl_alloc(e, &pairs_m, npair * 16))) return r;
    hipLaunchKernelGGL(k_crl_pairs, dim3(rp_grid(nt, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, B, (const uint8_t*)P->cls.u8(),
                       (const uint32_t*)P->tok_crl.p, (const uint32_t*)P->tok_ser.p, (const uint32_t*)pair_before.p, nt, (uint4*)pairs_m.p);
    HIPCHK(e, hipMemcpyAsync(pairs.data(), pairs_m.p, npair * 16, hipMemcpyDeviceToHost, e->stream));
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  // ---- the serials above 40 octets: gathered on the device, copied once
  std::vector<unsigned long long> dst(npair + 1, 0);
  std::vector<uint2> seg(npair);
  for (uint64_t g = 0; g < npair; g++) {
    seg[g] = make_uint2(pairs[g].x, pairs[g].y);
    dst[g + 1] = dst[g] + pairs[g].y;
  }
  std::vector<uint8_t> bytes(dst[npair]);
  if (npair) {
    DevMem seg_m, dst_m, out_m;
    if ((r = crl_alloc(e, &seg_m, npair * 8)) || (r = crl_alloc(e, &dst_m, npair * 8)) || (r = crl_alloc(e, &out_m, bytes.size()))) return r;
    HIPCHK(e, hipMemcpyAsync(seg_m.p, seg.data(), npair * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(dst_m.p, dst.data(), npair * 8, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_resp_gather, dim3(rp_grid(npair, RP_BLOCK / 64)), dim3(RP_BLOCK), 0, e->stream, s, (const uint2*)seg_m.p,
                       (const unsigned long long*)dst_m.p, npair, out_m.u8());
    HIPCHK(e, hipMemcpyAsync(bytes.data(), out_m.p, bytes.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipGetLastError());
  }
  // ---- CRLs → sets by digest, the sets in Issuer.ID order, every CRL's place in its set
  auto dig = [&](uint32_t k) { return digests + (size_t)k * 32; };
  auto dig_less = [](const uint8_t* x, const uint8_t* y) { return memcmp(x, y, 32) < 0; };
  auto dig_same = [](const uint8_t* x, const uint8_t* y) { return memcmp(x, y, 32) == 0; };
  std::vector<uint64_t> count(n);
  std::vector<const uint8_t*> digs;
  for (uint32_t k = 0; k < n; k++) {
    count[k] = (k + 1 < n ? rec0[k + 1] : nrec) - rec0[k];
    if (count[k]) digs.push_back(dig(k));
    if (span[k].x == span[k].y) P->cinfo.empty_crls++;
  }
  std::sort(digs.begin(), digs.end(), dig_less);
  digs.erase(std::unique(digs.begin(), digs.end(), dig_same), digs.end());
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
      ord[k] = (uint32_t)(std::lower_bound(digs.begin(), digs.end(), dig(k), dig_less) - digs.begin());
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
  std::sort(host.begin(), host.end());
  host.erase(std::unique(host.begin(), host.end()), host.end());
  known_write_meta(digs, sets, host, &P->meta, &P->info);
  P->cinfo.candidates = nc;
  P->cinfo.entries = nrec + npair;
  P->cinfo.records = nrec;
  P->cinfo.host_members = host.size();
  HIPCHK(e, hipMemcpyAsync(P->crl_dst.p, crl_dst.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));  // (crl_dst goes out of scope)
  return CTMR_OK;
}

// The place pass: info.members records to d_out.  Drains the stream.
int crl_place(ctmr_engine* e, const CrlProbes& P, uint8_t* d_out) {
  if (!P.info.members) return CTMR_OK;
  hipLaunchKernelGGL(k_crl_place, dim3(rp_grid(P.ntok, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, P.s, (const uint8_t*)P.cls.u8(),
                     (const uint32_t*)P.tok_crl.p, (const uint32_t*)P.tok_ser.p, (const uint32_t*)P.rec_before.p, (const uint32_t*)P.crl_rec0.p,
                     (const unsigned long long*)P.crl_dst.p, P.ntok, d_out);
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  return CTMR_OK;
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
  if (!r) r = crl_core(e, (const uint8_t*)d_crls, len, offsets, n_crls, digests, &P);
  *cinfo = P.cinfo;
  if (r) return r;
  *info = P.info;
  if (!meta || meta_cap < P.info.meta_bytes || members_cap < P.info.members || (P.info.members && !d_members))
    return fail(e, CTMR_E_RANGE, "%s: %llu meta bytes and %llu member records needed", CRL_PROBES, (unsigned long long)P.info.meta_bytes,
                (unsigned long long)P.info.members);
  if ((r = crl_place(e, P, (uint8_t*)d_members))) return r;
  memcpy(meta, P.meta.data(), P.meta.size());
  return CTMR_OK;
}

int ctmr_crl_probes(ctmr_engine* e, const uint8_t* crls, size_t len, const uint64_t* offsets, uint32_t n_crls, const uint8_t* digests, uint8_t* out,
                    size_t cap, ctmr_known_image_info* info, ctmr_crl_info* cinfo) {
  if (!e || !info || !cinfo) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  CrlProbes P;
  DevMem d_crls, d_out;
  int r = crl_args(e, crls, len, offsets, n_crls, digests, &P);
  if (!r && len) {
    if (d_crls.alloc(len) != hipSuccess) {
      *cinfo = P.cinfo;
      return fail(e, CTMR_E_NOMEM, "%s: no device memory to stage %llu bytes", CRL_PROBES, (unsigned long long)len);
    }
    HIPCHK(e, hipMemcpyAsync(d_crls.p, crls, len, hipMemcpyHostToDevice, e->stream));
  }
  if (!r) r = crl_core(e, d_crls.u8(), len, offsets, n_crls, digests, &P);
  *cinfo = P.cinfo;
  if (r) return r;
  *info = P.info;
  if (!out || cap < P.info.image_bytes) return fail(e, CTMR_E_RANGE, "%s: %llu bytes needed", CRL_PROBES, (unsigned long long)P.info.image_bytes);
  if (P.info.members && d_out.alloc(P.info.members * KNOWN_REC_BYTES) != hipSuccess)
    return fail(e, CTMR_E_NOMEM, "%s: no device memory for %llu member records", CRL_PROBES, (unsigned long long)P.info.members);
  if ((r = crl_place(e, P, d_out.u8()))) return r;
  if (P.info.members) HIPCHK(e, hipMemcpy(out + P.info.meta_bytes, d_out.p, P.info.members * KNOWN_REC_BYTES, hipMemcpyDeviceToHost));
  memcpy(out, P.meta.data(), P.meta.size());
  return CTMR_OK;
}
