// engine/resp_parse.inc — a Redis protocol stream of SADD / EXPIREAT commands → a known-certificate image (include/ctmr.h
// ctmr_known_resp_image*, DESIGN.md §19): the inverse of engine/resp.inc.  The stream stays where it lies; the kernels of
// kernels/resp_parse.h find its tokens, check its grammar and commands, and write the member records.  The host sees
// one entry per run of commands of one key (its key text, how many records it has) and the host-section pairs, which
// are rare: it orders the runs by key into sets, numbers the issuers, gives every run its place and writes the meta.
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after engine/merge.inc.

extern "C++" {
namespace {

struct RespImage {
  // the tables the place pass reads
  DevMem tok_pos, tok_nxt, tok_hdr, star, cidx, cmd_tok, cls, ridx, part, rec_before, runs, run_dst;
  const uint8_t* s = nullptr;
  uint64_t len = 0, ntok = 0, ncmd = 0, nrun = 0;
  std::vector<uint8_t> meta;
  ctmr_known_resp_image_info info{};
  RespTokens tokens() const {
    return RespTokens{s, len, (const uint32_t*)tok_pos.p, (const uint32_t*)tok_nxt.p, tok_hdr.u8(), ntok};
  }
  RespCmds cmds() const { return RespCmds{(const uint32_t*)cidx.p, (const uint32_t*)cmd_tok.p, cls.u8(), (const uint32_t*)ridx.p}; }
};

const char* const RESP_IMAGE = "known resp image";

unsigned rp_grid(uint64_t n, uint32_t per) { return (unsigned)((n + per - 1) / per); }

int rp_alloc(ctmr_engine* e, DevMem* m, size_t bytes, const char* what = RESP_IMAGE) {  // what: the call, for the message
  if (m->alloc(bytes ? bytes : 1) != hipSuccess)
    return fail(e, CTMR_E_NOMEM, "%s: no device memory for a table of %llu bytes", what, (unsigned long long)bytes);
  return CTMR_OK;
}

void rp_free(DevMem* m) {
  if (m->p) (void)hipFree(m->p);
  m->p = nullptr;
}

// idx[i] = the items of flag[0, i) with a bit of mask set, *total = those of all n; cnt: n / 1024 + 2 words
int rp_flag_scan(ctmr_engine* e, const uint8_t* flag, uint64_t n, uint32_t mask, unsigned long long* cnt, uint32_t* idx, uint64_t* total) {
  *total = 0;
  if (!n) return CTMR_OK;
  const uint64_t nb = (n + RP_TILE - 1) / RP_TILE;
  int r;
  HIPCHK(e, hipMemsetAsync(cnt + nb, 0, 8, e->stream));
  hipLaunchKernelGGL(k_resp_flag_count, dim3((unsigned)nb), dim3(RP_BLOCK), 0, e->stream, flag, n, mask, cnt);
  if ((r = scan_u64(e, (uint64_t*)cnt, nb + 1, false, SC_MISC))) return r;
  hipLaunchKernelGGL(k_resp_flag_index, dim3((unsigned)nb), dim3(RP_BLOCK), 0, e->stream, flag, n, mask, (const unsigned long long*)cnt, idx);
  unsigned long long t = 0;
  HIPCHK(e, hipMemcpyAsync(&t, cnt + nb, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  *total = t;
  return CTMR_OK;
}

// the first offset a pass reported, if any
int rp_check(ctmr_engine* e, unsigned long long* d_err, const char* saying, unsigned long long* second = nullptr) {
  unsigned long long h[2] = {0, 0};
  HIPCHK(e, hipMemcpyAsync(h, d_err, 16, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  if (second) *second = h[1];
  if (h[0] != ~0ull) return fail(e, CTMR_E_INVAL, "%s: offset %llu: %s", RESP_IMAGE, h[0], saying);
  return CTMR_OK;
}

// Everything but the records: the stream (device memory, any alignment) validated, R->meta and R->info made, the tables
// of the place pass left on the device.  Drains the stream.
int resp_parse_core(ctmr_engine* e, const uint8_t* s, uint64_t len, RespImage* R) {
  int r;
  R->s = s;
  R->len = len;
  memset(&R->info, 0, sizeof R->info);
  if (!len) {
    known_write_meta({}, {}, {}, &R->meta, &R->info);
    return CTMR_OK;
  }
  const uint64_t nb = (len + RP_TILE - 1) / RP_TILE;
  DevMem cnt_m, err_m, cand_m, nxt_m, flag_m, bm_m, tidx_m;
  if ((r = rp_alloc(e, &cnt_m, (nb + 2) * 8)) || (r = rp_alloc(e, &err_m, 16))) return r;
  unsigned long long* cnt = (unsigned long long*)cnt_m.p;
  unsigned long long* err = (unsigned long long*)err_m.p;
  const unsigned long long err0[2] = {~0ull, 0ull};
  HIPCHK(e, hipMemcpyAsync(err, err0, 16, hipMemcpyHostToDevice, e->stream));
  // ---- mark
  HIPCHK(e, hipMemsetAsync(cnt + nb, 0, 8, e->stream));
  hipLaunchKernelGGL((k_resp_mark<false>), dim3((unsigned)nb), dim3(RP_BLOCK), 0, e->stream, s, len, cnt, (uint32_t*)nullptr, (uint32_t*)nullptr);
  uint64_t nc = 0;
  if ((r = scan_total(e, (uint64_t*)cnt, nb + 1, false, SC_MISC, &nc))) return r;
  if (!nc) return fail(e, CTMR_E_INVAL, "%s: offset 0: no command starts here", RESP_IMAGE);
  const uint64_t ncb = (nc + RP_TILE - 1) / RP_TILE;
  if ((r = rp_alloc(e, &cand_m, nc * 4)) || (r = rp_alloc(e, &nxt_m, nc * 4)) || (r = rp_alloc(e, &flag_m, nc)) ||
      (r = rp_alloc(e, &bm_m, ncb * 4)) || (r = rp_alloc(e, &tidx_m, nc * 4)))
    return r;
  uint32_t* cand = (uint32_t*)cand_m.p;
  uint32_t* nxt = (uint32_t*)nxt_m.p;
  hipLaunchKernelGGL((k_resp_mark<true>), dim3((unsigned)nb), dim3(RP_BLOCK), 0, e->stream, s, len, cnt, cand, nxt);
  // ---- cuts, conflict regions
  hipLaunchKernelGGL(k_resp_blockmax, dim3((unsigned)ncb), dim3(RP_BLOCK), 0, e->stream, (const uint32_t*)nxt, (uint64_t)nc, (uint32_t*)bm_m.p);
  hipLaunchKernelGGL(k_resp_maxscan, dim3(1), dim3(1024), 0, e->stream, (uint32_t*)bm_m.p, ncb);
  hipLaunchKernelGGL(k_resp_cuts, dim3((unsigned)ncb), dim3(RP_BLOCK), 0, e->stream, (const uint32_t*)cand, (const uint32_t*)nxt, (uint64_t)nc,
                     (const uint32_t*)bm_m.p, flag_m.u8());
  hipLaunchKernelGGL(k_resp_resolve, dim3(rp_grid(nc, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, (const uint32_t*)cand, (const uint32_t*)nxt,
                     (uint64_t)nc, flag_m.u8());
  // ---- tokens, and the proof that they are the chain
  if ((r = rp_flag_scan(e, flag_m.u8(), nc, 3u, cnt, (uint32_t*)tidx_m.p, &R->ntok))) return r;
  const uint64_t nt = R->ntok;  // (>= 1: candidate 0 is a cut)
  if ((r = rp_alloc(e, &R->tok_pos, nt * 4)) || (r = rp_alloc(e, &R->tok_nxt, nt * 4)) || (r = rp_alloc(e, &R->tok_hdr, nt)) ||
      (r = rp_alloc(e, &R->star, nt)) || (r = rp_alloc(e, &R->cidx, nt * 4)))
    return r;
  hipLaunchKernelGGL(k_resp_tokens, dim3(rp_grid(nc, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, s, len, (const uint32_t*)cand, (const uint32_t*)nxt,
                     (const uint8_t*)flag_m.u8(), (const uint32_t*)tidx_m.p, (uint64_t)nc, (uint32_t*)R->tok_pos.p, (uint32_t*)R->tok_nxt.p,
                     R->tok_hdr.u8(), R->star.u8());
  hipLaunchKernelGGL(k_resp_chain, dim3(rp_grid(nt, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, (const uint32_t*)R->tok_pos.p,
                     (const uint32_t*)R->tok_nxt.p, (const uint8_t*)R->star.u8(), nt, len, err);
  if ((r = rp_check(e, err, "not the start of a command or of a bulk string that ends in CRLF inside the stream"))) return r;
  rp_free(&cand_m);
  rp_free(&nxt_m);
  rp_free(&flag_m);
  rp_free(&bm_m);
  rp_free(&tidx_m);
  // ---- commands
  if ((r = rp_flag_scan(e, R->star.u8(), nt, 1u, cnt, (uint32_t*)R->cidx.p, &R->ncmd))) return r;
  const uint64_t ncmd = R->ncmd;
  if ((r = rp_alloc(e, &R->cmd_tok, ncmd * 4)) || (r = rp_alloc(e, &R->cls, ncmd)) || (r = rp_alloc(e, &R->ridx, ncmd * 4))) return r;
  hipLaunchKernelGGL(k_resp_cmdtok, dim3(rp_grid(nt, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, (const uint8_t*)R->star.u8(),
                     (const uint32_t*)R->cidx.p, nt, (uint32_t*)R->cmd_tok.p);
  hipLaunchKernelGGL(k_resp_commands, dim3(rp_grid(ncmd, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, R->tokens(), (const uint32_t*)R->cmd_tok.p, ncmd,
                     R->cls.u8(), err);
  unsigned long long skipped = 0;
  if ((r = rp_check(e, err, "not SADD key member..., EXPIREAT / PEXPIREAT key time or SELECT db with exactly its arguments", &skipped)))
    return r;
  R->info.commands = ncmd;
  R->info.skipped_members = skipped;
  // ---- runs of one key, member records, host pairs
  uint64_t nrec = 0, npair = 0;
  if ((r = rp_flag_scan(e, R->cls.u8(), ncmd, RP_HEAD, cnt, (uint32_t*)R->ridx.p, &R->nrun))) return r;
  const uint64_t nrun = R->nrun;
  DevMem pair_before, pairs_m;
  if ((r = rp_alloc(e, &R->part, nt)) || (r = rp_alloc(e, &R->rec_before, nt * 4)) || (r = rp_alloc(e, &pair_before, nt * 4))) return r;
  hipLaunchKernelGGL(k_resp_parts, dim3(rp_grid(nt, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, R->tokens(), (const uint8_t*)R->star.u8(), R->cmds(),
                     R->part.u8());
  if ((r = rp_flag_scan(e, R->part.u8(), nt, RP_RECORD, cnt, (uint32_t*)R->rec_before.p, &nrec))) return r;
  if ((r = rp_flag_scan(e, R->part.u8(), nt, RP_PAIR, cnt, (uint32_t*)pair_before.p, &npair))) return r;
  std::vector<uint4> runs(nrun), pairs(npair);
  if (nrun) {
    if ((r = rp_alloc(e, &R->runs, nrun * 16)) || (r = rp_alloc(e, &R->run_dst, nrun * 8))) return r;
    hipLaunchKernelGGL(k_resp_runs, dim3(rp_grid(ncmd, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, R->tokens(), R->cmds(), ncmd,
                       (const uint32_t*)R->rec_before.p, (uint4*)R->runs.p);
    HIPCHK(e, hipMemcpyAsync(runs.data(), R->runs.p, nrun * 16, hipMemcpyDeviceToHost, e->stream));
  }
  if (npair) {
    if ((r = rp_alloc(e, &pairs_m, npair * 16))) return r;
    hipLaunchKernelGGL(k_resp_pairs, dim3(rp_grid(nt, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, R->tokens(), R->cmds(), (const uint8_t*)R->part.u8(),
                       (const uint32_t*)pair_before.p, (uint4*)pairs_m.p);
    HIPCHK(e, hipMemcpyAsync(pairs.data(), pairs_m.p, npair * 16, hipMemcpyDeviceToHost, e->stream));
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  // ---- the bytes the host needs: every run's key, every pair's member — gathered on the device, copied once
  const uint64_t nseg = nrun + npair;
  std::vector<uint2> seg(nseg);
  std::vector<unsigned long long> dst(nseg + 1, 0);
  for (uint64_t g = 0; g < nseg; g++) {
    const uint4& x = g < nrun ? runs[g] : pairs[g - nrun];
    seg[g] = make_uint2(x.x, x.y);
    dst[g + 1] = dst[g] + x.y;
  }
  std::vector<uint8_t> bytes(dst[nseg]);
  if (nseg) {
    DevMem seg_m, dst_m, out_m;
    if ((r = rp_alloc(e, &seg_m, nseg * 8)) || (r = rp_alloc(e, &dst_m, nseg * 8)) || (r = rp_alloc(e, &out_m, bytes.size()))) return r;
    HIPCHK(e, hipMemcpyAsync(seg_m.p, seg.data(), nseg * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(dst_m.p, dst.data(), nseg * 8, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_resp_gather, dim3(rp_grid(nseg, RP_BLOCK / 64)), dim3(RP_BLOCK), 0, e->stream, s, (const uint2*)seg_m.p,
                       (const unsigned long long*)dst_m.p, nseg, out_m.u8());
    if (!bytes.empty()) HIPCHK(e, hipMemcpyAsync(bytes.data(), out_m.p, bytes.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipGetLastError());
  }
  auto text = [&](uint64_t g) { return std::string((const char*)bytes.data() + dst[g], (size_t)(dst[g + 1] - dst[g])); };
  // ---- the runs that have records, in key order (stable: a key's runs stay in stream order) → sets, issuers, places
  std::vector<std::string> key(nrun);
  std::vector<uint64_t> count(nrun);
  std::vector<uint32_t> order;
  for (uint64_t q = 0; q < nrun; q++) {
    key[q] = text(q);
    count[q] = (q + 1 < nrun ? runs[q + 1].z : nrec) - runs[q].z;
    if (runs[q].w == RP_SET_KEY && count[q]) order.push_back((uint32_t)q);
  }
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
  std::vector<MergeSetKey> set_key;
  std::vector<KnownSetEntry> sets;
  std::vector<unsigned long long> run_dst(nrun, 0);
  uint64_t first = 0;
  for (size_t i = 0; i < order.size(); i++) {
    const uint32_t q = order[i];
    if (i == 0 || key[q] != key[order[i - 1]]) {
      MergeSetKey mk;
      if (!merge_parse_key(key[q], &mk)) return fail(e, CTMR_E_HIP, "%s: the device took a key the host does not: %s", RESP_IMAGE, key[q].c_str());
      set_key.push_back(mk);
      sets.push_back({mk.hour, 0u, 0ull});
    }
    run_dst[q] = first;
    sets.back().count += count[q];
    first += count[q];
  }
  if (first != nrec) return fail(e, CTMR_E_HIP, "%s: the runs hold %llu records, the stream %llu", RESP_IMAGE, (unsigned long long)first, (unsigned long long)nrec);
  std::vector<const uint8_t*> digs;
  for (auto& mk : set_key) digs.push_back(mk.digest);
  auto dig_less = [](const uint8_t* x, const uint8_t* y) { return memcmp(x, y, 32) < 0; };
  std::sort(digs.begin(), digs.end(), dig_less);
  digs.erase(std::unique(digs.begin(), digs.end(), [](const uint8_t* x, const uint8_t* y) { return memcmp(x, y, 32) == 0; }), digs.end());
  for (size_t i = 0; i < sets.size(); i++) sets[i].ordinal = (uint32_t)(std::lower_bound(digs.begin(), digs.end(), set_key[i].digest, dig_less) - digs.begin());
  KnownHostPairs host(npair);
  for (uint64_t p = 0; p < npair; p++) host[p] = {key[pairs[p].z], text(nrun + p)};
  std::sort(host.begin(), host.end());
  host.erase(std::unique(host.begin(), host.end()), host.end());
  known_write_meta(digs, sets, host, &R->meta, &R->info);
  if (nrun) {
    HIPCHK(e, hipMemcpyAsync(R->run_dst.p, run_dst.data(), nrun * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));  // (run_dst goes out of scope)
  }
  return CTMR_OK;
}

// The place pass: info.members records to d_out.  Drains the stream.
int resp_parse_place(ctmr_engine* e, const RespImage& R, uint8_t* d_out) {
  if (!R.info.members) return CTMR_OK;
  hipLaunchKernelGGL(k_resp_place, dim3(rp_grid(R.ntok, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, R.tokens(), R.cmds(), (const uint8_t*)R.part.u8(),
                     (const uint32_t*)R.rec_before.p, (const uint4*)R.runs.p, (const unsigned long long*)R.run_dst.p, d_out);
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  return CTMR_OK;
}

int resp_parse_len(ctmr_engine* e, size_t len) {
  if ((uint64_t)len >= RP_MAX_LEN)
    return fail(e, CTMR_E_INVAL, "%s: %llu bytes: a stream of 2^32 - 64 bytes or more is split at a command start", RESP_IMAGE, (unsigned long long)len);
  return CTMR_OK;
}

}  // namespace
}  // extern "C++"

int ctmr_known_resp_image_device(ctmr_engine* e, const void* d_stream, size_t len, uint8_t* out_meta, size_t out_meta_cap, void* d_out,
                                 uint64_t out_members_cap, ctmr_known_resp_image_info* info) {
  if (!e || !info) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  int r;
  if ((r = resp_parse_len(e, len))) return r;
  if (len && !d_stream) return fail(e, CTMR_E_INVAL, "%s: null stream", RESP_IMAGE);
  RespImage R;
  if ((r = resp_parse_core(e, (const uint8_t*)d_stream, len, &R))) return r;
  *info = R.info;
  if (!out_meta || out_meta_cap < R.info.meta_bytes || out_members_cap < R.info.members || (R.info.members && !d_out))
    return fail(e, CTMR_E_RANGE, "%s: %llu meta bytes and %llu member records needed", RESP_IMAGE, (unsigned long long)R.info.meta_bytes,
                (unsigned long long)R.info.members);
  if ((r = resp_parse_place(e, R, (uint8_t*)d_out))) return r;
  memcpy(out_meta, R.meta.data(), R.meta.size());
  return CTMR_OK;
}

int ctmr_known_resp_image(ctmr_engine* e, const uint8_t* stream, size_t len, uint8_t* out, size_t cap, ctmr_known_resp_image_info* info) {
  if (!e || !info) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  int r;
  if ((r = resp_parse_len(e, len))) return r;
  if (len && !stream) return fail(e, CTMR_E_INVAL, "%s: null stream", RESP_IMAGE);
  DevMem d_stream, d_out;
  if (len) {
    if (d_stream.alloc(len) != hipSuccess) return fail(e, CTMR_E_NOMEM, "%s: no device memory to stage %llu bytes", RESP_IMAGE, (unsigned long long)len);
    HIPCHK(e, hipMemcpyAsync(d_stream.p, stream, len, hipMemcpyHostToDevice, e->stream));
  }
  RespImage R;
  if ((r = resp_parse_core(e, d_stream.u8(), len, &R))) return r;
  *info = R.info;
  if (!out || cap < R.info.image_bytes) return fail(e, CTMR_E_RANGE, "%s: %llu bytes needed", RESP_IMAGE, (unsigned long long)R.info.image_bytes);
  if (R.info.members && d_out.alloc(R.info.members * KNOWN_REC_BYTES) != hipSuccess)
    return fail(e, CTMR_E_NOMEM, "%s: no device memory for %llu member records", RESP_IMAGE, (unsigned long long)R.info.members);
  if ((r = resp_parse_place(e, R, d_out.u8()))) return r;
  if (R.info.members)
    HIPCHK(e, hipMemcpy(out + R.info.meta_bytes, d_out.p, R.info.members * KNOWN_REC_BYTES, hipMemcpyDeviceToHost));
  memcpy(out, R.meta.data(), R.meta.size());
  return CTMR_OK;
}
