// engine/resp_parse.inc — a Redis protocol stream of SADD / EXPIREAT commands → a known-certificate image (include/ctmr.h
// ctmr_known_resp_image*, DESIGN.md §19): the inverse of engine/resp.inc.  The stream stays where it lies; the kernels of
// kernels/resp_parse.h find its tokens, check its grammar and commands, and write the member records.  The host sees
// one entry per run of commands of one key (its key text, how many records it has) and the host-section pairs, which
// are rare: it orders the runs by key into sets, numbers the issuers, gives every run its place and writes the meta.
// The first half of the file is what any parser of a length-prefixed input shares (engine/crl.inc is the second): the
// token stage RpStage, the gather, and the two ways out of a call.
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

// Candidates → tokens: the stage every parser of a length-prefixed input runs (DESIGN.md §19).  Its one variable part
// is the candidate predicate Cand the two mark launches carry (kernels/resp_parse.h RespCand, kernels/crl.h CrlCand);
// the cuts, conflict-region, compaction and chain kernels work on cand[] / nxt[] alone.  In three steps, because the
// callers have work of their own between them: begin (the counters and the two error words), count (the count pass and
// its scan → nc), tokens (the write pass … the chain kernel → ntok and the token tables).  The caller reads err its own
// way, then calls drop(): the candidate tables go before the later tables of the call are allocated.
struct RpStage {
  const char* what = nullptr;  // the call, for the messages
  uint64_t len = 0, nb = 0, nc = 0, ntok = 0;
  DevMem cnt_m, err_m, cand_m, nxt_m, flag_m, bm_m, tidx_m;
  unsigned long long* cnt = nullptr;  // nb + 2 words: the later flag scans of the call use them too
  unsigned long long* err = nullptr;  // two words, err[0] = ~0; err[1] = err1 and its meaning are the caller's
  unsigned long long err0[2] = {~0ull, 0ull};

  // more: words behind the two, preset to all ones (a finding per input of the call: they come back in err's copy)
  int begin(ctmr_engine* e, const char* call, uint64_t bytes, unsigned long long err1, uint64_t more = 0) {
    int r;
    what = call;
    len = bytes;
    nb = (len + RP_TILE - 1) / RP_TILE;
    err0[1] = err1;
    if ((r = rp_alloc(e, &cnt_m, (nb + 2) * 8, what)) || (r = rp_alloc(e, &err_m, 16 + more * 8, what))) return r;
    cnt = (unsigned long long*)cnt_m.p;
    err = (unsigned long long*)err_m.p;
    HIPCHK(e, hipMemcpyAsync(err, err0, 16, hipMemcpyHostToDevice, e->stream));
    if (more) HIPCHK(e, hipMemsetAsync(err + 2, 0xff, more * 8, e->stream));
    return CTMR_OK;
  }

  template <class Cand>
  int count(ctmr_engine* e, const Cand& C) {
    HIPCHK(e, hipMemsetAsync(cnt + nb, 0, 8, e->stream));
    hipLaunchKernelGGL((k_resp_mark<false, Cand>), dim3((unsigned)nb), dim3(RP_BLOCK), 0, e->stream, C, cnt, (uint32_t*)nullptr, (uint32_t*)nullptr);
    return scan_total(e, (uint64_t*)cnt, nb + 1, false, SC_MISC, &nc);
  }

  // nc >= 1.  RESP: the tokens are a RESP stream's, s is read for tok_hdr / star, and the first token is a '*'; more: a
  // table of a word per token the caller wants allocated behind them (may be null).  Else only tok_pos / tok_nxt are made.
  template <bool RESP, class Cand>
  int tokens(ctmr_engine* e, const Cand& C, const uint8_t* s, DevMem* tok_pos, DevMem* tok_nxt, DevMem* tok_hdr, DevMem* star, DevMem* more,
             unsigned long long* chain_err) {
    int r;
    const uint64_t ncb = (nc + RP_TILE - 1) / RP_TILE;
    if ((r = rp_alloc(e, &cand_m, nc * 4, what)) || (r = rp_alloc(e, &nxt_m, nc * 4, what)) || (r = rp_alloc(e, &flag_m, nc, what)) ||
        (r = rp_alloc(e, &bm_m, ncb * 4, what)) || (r = rp_alloc(e, &tidx_m, nc * 4, what)))
      return r;
    uint32_t* cand = (uint32_t*)cand_m.p;
    uint32_t* nxt = (uint32_t*)nxt_m.p;
    hipLaunchKernelGGL((k_resp_mark<true, Cand>), dim3((unsigned)nb), dim3(RP_BLOCK), 0, e->stream, C, cnt, cand, nxt);
    // cuts, conflict regions
    hipLaunchKernelGGL(k_resp_blockmax, dim3((unsigned)ncb), dim3(RP_BLOCK), 0, e->stream, (const uint32_t*)nxt, (uint64_t)nc, (uint32_t*)bm_m.p);
    hipLaunchKernelGGL(k_resp_maxscan, dim3(1), dim3(1024), 0, e->stream, (uint32_t*)bm_m.p, ncb);
    hipLaunchKernelGGL(k_resp_cuts, dim3((unsigned)ncb), dim3(RP_BLOCK), 0, e->stream, (const uint32_t*)cand, (const uint32_t*)nxt, (uint64_t)nc,
                       (const uint32_t*)bm_m.p, flag_m.u8());
    hipLaunchKernelGGL(k_resp_resolve, dim3(rp_grid(nc, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, (const uint32_t*)cand, (const uint32_t*)nxt,
                       (uint64_t)nc, flag_m.u8());
    // the kept candidates, and the proof that they are the chain
    if ((r = rp_flag_scan(e, flag_m.u8(), nc, 3u, cnt, (uint32_t*)tidx_m.p, &ntok))) return r;
    const uint64_t nt = ntok;  // (>= 1: candidate 0 is a cut)
    if ((r = rp_alloc(e, tok_pos, nt * 4, what)) || (r = rp_alloc(e, tok_nxt, nt * 4, what))) return r;
    if (RESP && ((r = rp_alloc(e, tok_hdr, nt, what)) || (r = rp_alloc(e, star, nt, what)))) return r;
    if (more && (r = rp_alloc(e, more, nt * 4, what))) return r;
    hipLaunchKernelGGL((k_resp_tokens<RESP>), dim3(rp_grid(nc, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, s, len, (const uint32_t*)cand,
                       (const uint32_t*)nxt, (const uint8_t*)flag_m.u8(), (const uint32_t*)tidx_m.p, (uint64_t)nc, (uint32_t*)tok_pos->p,
                       (uint32_t*)tok_nxt->p, RESP ? tok_hdr->u8() : nullptr, RESP ? star->u8() : nullptr);
    if (chain_err)  // (null: the caller runs a chain check of its own over tok_pos / tok_nxt)
      hipLaunchKernelGGL((k_resp_chain<RESP>), dim3(rp_grid(nt, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, (const uint32_t*)tok_pos->p,
                         (const uint32_t*)tok_nxt->p, RESP ? (const uint8_t*)star->u8() : nullptr, nt, len, chain_err);
    return CTMR_OK;
  }

  void drop() {
    for (DevMem* m : {&cand_m, &nxt_m, &flag_m, &bm_m, &tidx_m}) rp_free(m);
  }
};

// gather: the segments {offset, length} of the input → *bytes, segment g at (*dst)[g], behind the last (*dst)[n]; gathered
// on the device, copied once.  Drains the stream.
int rp_gather(ctmr_engine* e, const char* what, const uint8_t* s, const std::vector<uint2>& seg, std::vector<unsigned long long>* dst,
              std::vector<uint8_t>* bytes) {
  int r;
  const uint64_t nseg = seg.size();
  dst->assign(nseg + 1, 0);
  for (uint64_t g = 0; g < nseg; g++) (*dst)[g + 1] = (*dst)[g] + seg[g].y;
  bytes->resize((*dst)[nseg]);
  if (!nseg) return CTMR_OK;
  DevMem seg_m, dst_m, out_m;
  if ((r = rp_alloc(e, &seg_m, nseg * 8, what)) || (r = rp_alloc(e, &dst_m, nseg * 8, what)) || (r = rp_alloc(e, &out_m, bytes->size(), what)))
    return r;
  HIPCHK(e, hipMemcpyAsync(seg_m.p, seg.data(), nseg * 8, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(dst_m.p, dst->data(), nseg * 8, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_resp_gather, dim3(rp_grid(nseg, RP_BLOCK / 64)), dim3(RP_BLOCK), 0, e->stream, s, (const uint2*)seg_m.p,
                     (const unsigned long long*)dst_m.p, nseg, out_m.u8());
  if (!bytes->empty()) HIPCHK(e, hipMemcpyAsync(bytes->data(), out_m.p, bytes->size(), hipMemcpyDeviceToHost, e->stream));  // (keys of no octets)
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  return CTMR_OK;
}

// The way in of a host variant: the input's len bytes to device memory.
int rp_stage(ctmr_engine* e, const char* what, const void* src, uint64_t len, DevMem* d) {
  if (!len) return CTMR_OK;
  if (d->alloc(len) != hipSuccess) return fail(e, CTMR_E_NOMEM, "%s: no device memory to stage %llu bytes", what, (unsigned long long)len);
  HIPCHK(e, hipMemcpyAsync(d->p, src, len, hipMemcpyHostToDevice, e->stream));
  return CTMR_OK;
}

// The two ways out of a call whose core has made `meta` and `info` (an image's, or a longer struct that begins as it
// does): *out_info, the refusal of short buffers, the place pass — place(d) launches it, info.members records to d — and
// the meta.  Nothing is written to a buffer before the last thing that can fail.  Drain the stream.
template <class Place>
int rp_place(ctmr_engine* e, uint64_t members, Place place, uint8_t* d_out) {
  if (!members) return CTMR_OK;
  place(d_out);
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  return CTMR_OK;
}

template <class Info, class Place>
int rp_emit_device(ctmr_engine* e, const char* what, const std::vector<uint8_t>& meta, const Info& info, Place place, uint8_t* out_meta,
                   size_t meta_cap, void* d_out, uint64_t members_cap, Info* out_info) {
  int r;
  *out_info = info;
  if (!out_meta || meta_cap < info.meta_bytes || members_cap < info.members || (info.members && !d_out))
    return fail(e, CTMR_E_RANGE, "%s: %llu meta bytes and %llu member records needed", what, (unsigned long long)info.meta_bytes,
                (unsigned long long)info.members);
  if ((r = rp_place(e, info.members, place, (uint8_t*)d_out))) return r;
  memcpy(out_meta, meta.data(), meta.size());
  return CTMR_OK;
}

template <class Info, class Place>
int rp_emit_host(ctmr_engine* e, const char* what, const std::vector<uint8_t>& meta, const Info& info, Place place, uint8_t* out, size_t cap,
                 Info* out_info) {
  int r;
  DevMem d_out;
  *out_info = info;
  if (!out || cap < info.image_bytes) return fail(e, CTMR_E_RANGE, "%s: %llu bytes needed", what, (unsigned long long)info.image_bytes);
  if (info.members && d_out.alloc(info.members * KNOWN_REC_BYTES) != hipSuccess)
    return fail(e, CTMR_E_NOMEM, "%s: no device memory for %llu member records", what, (unsigned long long)info.members);
  if ((r = rp_place(e, info.members, place, d_out.u8()))) return r;
  if (info.members) HIPCHK(e, hipMemcpy(out + info.meta_bytes, d_out.p, info.members * KNOWN_REC_BYTES, hipMemcpyDeviceToHost));
  memcpy(out, meta.data(), meta.size());
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
  // ---- candidates → tokens
  RpStage st;
  const RespCand C{s, len};
  if ((r = st.begin(e, RESP_IMAGE, len, 0ull)) || (r = st.count(e, C))) return r;
  if (!st.nc) return fail(e, CTMR_E_INVAL, "%s: offset 0: no command starts here", RESP_IMAGE);
  if ((r = st.tokens<true>(e, C, s, &R->tok_pos, &R->tok_nxt, &R->tok_hdr, &R->star, &R->cidx, st.err))) return r;
  if ((r = rp_check(e, st.err, "not the start of a command or of a bulk string that ends in CRLF inside the stream"))) return r;
  st.drop();
  unsigned long long* const cnt = st.cnt;
  unsigned long long* const err = st.err;
  const uint64_t nt = R->ntok = st.ntok;
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
  std::vector<uint2> seg;
  seg.reserve(nrun + npair);
  for (const uint4& x : runs) seg.push_back(make_uint2(x.x, x.y));
  for (const uint4& x : pairs) seg.push_back(make_uint2(x.x, x.y));
  std::vector<unsigned long long> dst;
  std::vector<uint8_t> bytes;
  if ((r = rp_gather(e, RESP_IMAGE, s, seg, &dst, &bytes))) return r;
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
  known_number_digests(&digs);
  for (size_t i = 0; i < sets.size(); i++) sets[i].ordinal = known_digest_ordinal(digs, set_key[i].digest);
  KnownHostPairs host(npair);
  for (uint64_t p = 0; p < npair; p++) host[p] = {key[pairs[p].z], text(nrun + p)};
  known_finish_pairs(&host);
  known_write_meta(digs, sets, host, &R->meta, &R->info);
  if (nrun) {
    HIPCHK(e, hipMemcpyAsync(R->run_dst.p, run_dst.data(), nrun * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));  // (run_dst goes out of scope)
  }
  return CTMR_OK;
}

// The place pass as rp_emit_* take it: info.members records to d.
auto resp_parse_place(ctmr_engine* e, const RespImage& R) {
  return [e, &R](uint8_t* d) {
    hipLaunchKernelGGL(k_resp_place, dim3(rp_grid(R.ntok, RP_BLOCK)), dim3(RP_BLOCK), 0, e->stream, R.tokens(), R.cmds(),
                       (const uint8_t*)R.part.u8(), (const uint32_t*)R.rec_before.p, (const uint4*)R.runs.p,
                       (const unsigned long long*)R.run_dst.p, d);
  };
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
  return rp_emit_device(e, RESP_IMAGE, R.meta, R.info, resp_parse_place(e, R), out_meta, out_meta_cap, d_out, out_members_cap, info);
}

int ctmr_known_resp_image(ctmr_engine* e, const uint8_t* stream, size_t len, uint8_t* out, size_t cap, ctmr_known_resp_image_info* info) {
  if (!e || !info) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> g(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  int r;
  if ((r = resp_parse_len(e, len))) return r;
  if (len && !stream) return fail(e, CTMR_E_INVAL, "%s: null stream", RESP_IMAGE);
  DevMem d_stream;
  if ((r = rp_stage(e, RESP_IMAGE, stream, len, &d_stream))) return r;
  RespImage R;
  if ((r = resp_parse_core(e, d_stream.u8(), len, &R))) return r;
  return rp_emit_host(e, RESP_IMAGE, R.meta, R.info, resp_parse_place(e, R), out, cap, info);
}
