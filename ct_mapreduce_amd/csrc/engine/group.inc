// engine/group.inc — multi-GPU groups behind the C ABI: the shared set service of a sharded deployment.
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after the engine entry points.
//
// The reference shards a log between ct-fetch processes by -offset/-limit (cmd/ct-fetch/ct-fetch.go:288-305) and
// makes their dedup global through ONE Redis server (storage/rediscache.go:21-65: SADD answers "was new" for all of
// them).  Here the set is partitioned over the GPUs of a node and the ranks exchange keys — all of it native: a Go
// host makes three calls (create, map_batch, issuer_counts), no Python, no torch.
//
// A group has `world` ranks; each rank is one engine on one GPU.  Two transports behind the same phase drivers:
//   LOCAL  every rank lives in this process (one engine per device, or several engines on one device in the tests):
//          "collectives" are device-to-device copies.
//   RCCL   one process per GPU (the deployment shape): ncclSend/ncclRecv all-to-all, ncclAllGather of the Bloom
//          filters, ncclAllReduce of the per-issuer counts, over xGMI.  librccl is loaded on demand (dlopen) so that a
//          single-GPU host does not carry the dependency.
// Both run exactly the same per-rank steps (ctmr_xchg_* / ctmr_bloom_* above) in the same order.

extern "C++" {
namespace {

struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};

// dlopen("librccl.so.1"): when the host process already carries an RCCL (PyTorch-ROCm bundles one under the same
// SONAME) the loader hands that one back, so one process never runs two copies.
const RcclApi* rccl_api(std::string* why) {
  static std::mutex mu;
  static RcclApi api;
  static bool tried = false;
  static std::string err;
  std::lock_guard<std::mutex> g(mu);
  if (!tried) {
    tried = true;
    // CTMR_RCCL_LIB names the library explicitly (a site's own build — or the tests' in-process stand-in that lets several
    // ranks live as threads on one GPU, tests/harness/fake_rccl.cpp)
    const char* forced = getenv("CTMR_RCCL_LIB");
    if (forced && *forced) {
      api.lib = dlopen(forced, RTLD_NOW | RTLD_LOCAL);
    } else {
      for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (api.lib) break;
      }
    }
    if (!api.lib) {
      err = std::string("librccl not loadable: ") + dlerror();
    } else {
#define SYM(field, sym)                                                         \
  api.field = (decltype(api.field))dlsym(api.lib, sym);                         \
  if (!api.field && err.empty()) err = std::string("librccl lacks ") + sym
      SYM(GetUniqueId, "ncclGetUniqueId");
      SYM(CommInitRank, "ncclCommInitRank");
      SYM(CommDestroy, "ncclCommDestroy");
      SYM(AllReduce, "ncclAllReduce");
      SYM(AllGather, "ncclAllGather");
      SYM(Send, "ncclSend");
      SYM(Recv, "ncclRecv");
      SYM(GroupStart, "ncclGroupStart");
      SYM(GroupEnd, "ncclGroupEnd");
      SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
    }
  }
  if (!err.empty()) {
    if (why) *why = err;
    return nullptr;
  }
  return &api;
}

struct DevBuf {  // grow-only device buffer on one engine's device
  void* p = nullptr;
  size_t cap = 0;
};

struct GroupRank {
  ctmr_engine* e = nullptr;
  uint32_t rank = 0;  // rank in the world
  ncclComm_t comm = nullptr;
  DevBuf keys, recv, flags_out, flags_mine, small, filters;
  DevBuf keys64, recv64, flags_out64, flags_mine64;  // owner-computes exchange: the rare 64-byte records (21..40-octet serials)
  std::vector<uint64_t> send_counts, recv_counts;      // per peer, of the exchange in flight
  std::vector<uint64_t> send_counts64, recv_counts64;
  std::vector<uint64_t> ctl_out, ctl_in;               // control rows: mine, and every rank's (world x K)
  uint64_t n_keys = 0, n_keys64 = 0;
  uint64_t ord_base = 0;     // where this rank's shard lies in the round's log order
  std::vector<uint64_t> hk;  // this round's long-serial members of this rank, serialised (round_finish)
  int rc = CTMR_OK;  // first failure of this rank inside the round in flight
  ctmr_batch_stats st{};
  // chunked owner-computes rounds (ctmr_group_set_chunks): a second stream that carries chunk c's key records while the
  // engine's own stream maps chunk c + 1, and where each chunk lies in the send / receive buffers (in records)
  hipStream_t xfer = nullptr;
  // … over a communicator of its own (RCCL groups): operations on ONE communicator from two streams are serialised by the
  // library at best and undefined at worst — the chunk transfers must never queue behind, or in front of, the control
  // all-gathers that go over `comm` on the engine's stream (VERDICT r04 #3)
  ncclComm_t xcomm = nullptr;
  std::vector<std::vector<uint64_t>> csend, crecv;  // per chunk: counts per peer
  std::vector<uint64_t> csend_off, crecv_off;       // per chunk: first record in keys / recv
};

}  // namespace
}  // extern "C++"

struct ctmr_group {
  std::mutex mu;
  std::mutex err_mu;  // the ranks of a LOCAL group run their phases on threads of their own
  std::string err;
  uint32_t world = 0;
  bool rccl = false;
  std::vector<GroupRank> local;
  uint64_t bloom_words = 0;
  int mode = -1;  // the dedup mode of the group's first round: the only one it accepts afterwards (ctmr_group_map_batch)
  uint32_t chunks = 1;  // owner-computes rounds: shards are mapped in this many chunks (ctmr_group_set_chunks)
  // statistics of the last ctmr_group_map_batch (what moved between ranks)
  uint64_t last_keys_sent = 0, last_keys_received = 0, last_filter_bytes_received = 0, last_wire_bytes = 0;
  float ms_phase[8] = {};
};

extern "C++" {
namespace {

int gfail(ctmr_group* g, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  std::lock_guard<std::mutex> lk(g->err_mu);
  g->err = buf;
  return code;
}

#define GHIP(g, call)                                                                              \
  do {                                                                                             \
    hipError_t _r = (call);                                                                        \
    if (_r != hipSuccess)                                                                          \
      return gfail(g, _r == hipErrorOutOfMemory ? CTMR_E_NOMEM : CTMR_E_HIP, "%s: %s", #call,      \
                   hipGetErrorString(_r));                                                         \
  } while (0)
// … and a stream drain on the host: counted (ctmr_group_stats.ms_phase[7]) — a round's host synchronisations are latency no
// kernel hides, the first thing to fold when a real node is at hand (VERDICT r05 #8)
#define GSYNC(g, stream) do { (g)->ms_phase[7] += 1.f; GHIP(g, hipStreamSynchronize stream); } while (0)
#define GNCCL(g, api, call)                                                                        \
  do {                                                                                             \
    ncclResult_t _r = (call);                                                                      \
    if (_r != ncclSuccess) return gfail(g, CTMR_E_HIP, "%s: %s", #call, (api)->GetErrorString(_r)); \
  } while (0)
// an engine call failed: its message becomes the group's
#define GENG(g, rk, call)                                                                          \
  do {                                                                                             \
    int _r = (call);                                                                               \
    if (_r != CTMR_OK) return gfail(g, _r, "rank %u: %s", (rk).rank, ctmr_last_error((rk).e));     \
  } while (0)

int gbuf(ctmr_group* g, GroupRank& r, DevBuf& b, size_t bytes) {
  if (b.cap >= bytes && b.p) return CTMR_OK;
  GHIP(g, hipSetDevice(r.e->device));
  if (b.p) {
    GSYNC(g, (r.e->stream));
    (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
  }
  const size_t cap = bytes + bytes / 8 + 256;
  GHIP(g, hipMalloc(&b.p, cap));
  b.cap = cap;
  return CTMR_OK;
}

uint64_t prefix(const std::vector<uint64_t>& v, uint32_t k) {
  uint64_t s = 0;
  for (uint32_t i = 0; i < k; i++) s += v[i];
  return s;
}

int sync_all(ctmr_group* g) {
  for (auto& r : g->local) {
    GHIP(g, hipSetDevice(r.e->device));
    GSYNC(g, (r.e->stream));
  }
  return CTMR_OK;
}

// fn(k) for every local rank k.  A LOCAL group with several ranks runs them on threads of their own: every engine has
// its own mutex and stream (and usually its own device), every engine call ends by draining its stream — called one
// after the other the ranks' kernels would queue behind each other's synchronisations (round 2: a single-process group
// over 8 devices mapped one GPU at a time).  The first failure of a rank is remembered in its GroupRank; the round goes
// on (see ctmr.h: "errors").
template <class Fn>
void par_ranks(ctmr_group* g, Fn fn) {
  const size_t n = g->local.size();
  auto one = [&](size_t k) {
    GroupRank& r = g->local[k];
    if (r.rc != CTMR_OK) return;  // this rank has already failed: it only takes part in the collectives from now on
    (void)hipSetDevice(r.e->device);
    const int rc = fn(k);
    if (rc != CTMR_OK) r.rc = rc;
  };
  if (n == 1) {
    one(0);
    return;
  }
  std::vector<std::thread> th;
  th.reserve(n);
  size_t started = 0;
  try {
    for (; started < n; started++) th.emplace_back(one, started);
  } catch (const std::system_error&) {
    // no more threads to be had: the remaining ranks run here, one after the other (slower, not wrong)
  }
  for (auto& t : th) t.join();
  for (size_t k = started; k < n; k++) one(k);
}

struct PhaseClock {
  ctmr_group* g;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void lap(int phase) {
    const auto t1 = std::chrono::steady_clock::now();
    g->ms_phase[phase] += std::chrono::duration<float, std::milli>(t1 - t0).count();
    t0 = t1;
  }
};

// Control all-gather: every rank contributes K u64 (r.ctl_out) and learns everybody's (r.ctl_in = world x K, rank-major).
// Column 0 of a row is, by convention, the rank's status: the ranks agree here whether the round goes on.
int control_gather(ctmr_group* g, uint32_t K) {
  const uint32_t W = g->world;
  if (!g->rccl) {
    for (auto& r : g->local) {
      r.ctl_in.assign((size_t)W * K, 0);
      for (auto& s : g->local)
        for (uint32_t k = 0; k < K; k++) r.ctl_in[(size_t)s.rank * K + k] = s.ctl_out[k];
    }
    return CTMR_OK;
  }
  const RcclApi* api = rccl_api(nullptr);
  GroupRank& r = g->local[0];
  int rc;
  if ((rc = gbuf(g, r, r.small, (size_t)W * K * 8 + 4096))) return rc;
  GHIP(g, hipSetDevice(r.e->device));
  unsigned long long* d_all = (unsigned long long*)r.small.p;
  unsigned long long* d_mine = d_all + (size_t)r.rank * K;  // in-place all-gather: my row of the W x K matrix
  GHIP(g, hipMemcpyAsync(d_mine, r.ctl_out.data(), (size_t)K * 8, hipMemcpyHostToDevice, r.e->stream));
  GNCCL(g, api, api->AllGather(d_mine, d_all, K, ncclUint64, r.comm, r.e->stream));
  r.ctl_in.assign((size_t)W * K, 0);
  GHIP(g, hipMemcpyAsync(r.ctl_in.data(), d_all, (size_t)W * K * 8, hipMemcpyDeviceToHost, r.e->stream));
  GSYNC(g, (r.e->stream));
  return CTMR_OK;
}

// status column of the control matrix: the first failed rank's code (0 = every rank is fine)
int control_status(ctmr_group* g, uint32_t K) {
  const GroupRank& r = g->local[0];
  for (uint32_t w = 0; w < g->world; w++) {
    const int rc = (int)(int64_t)r.ctl_in[(size_t)w * K];
    if (rc != CTMR_OK) {
      bool mine = false;
      for (auto& l : g->local) mine = mine || (l.rank == w && l.rc != CTMR_OK);
      if (!mine) (void)gfail(g, rc, "rank %u failed in this round (code %d); see its own error message", w, rc);
      return rc;
    }
  }
  return CTMR_OK;
}

// All-to-all of `unit`-byte records.  Rank r sends, to every peer p, send_cnt(r)[p] records starting at record
// prefix(send_cnt(r), p) of its send buffer, and receives recv_cnt(r)[s] records from every s at record
// prefix(recv_cnt(r), s) of its receive buffer — sender-rank order, which is global log order for log-index shards.
template <class SendPtr, class RecvPtr, class SendCnt, class RecvCnt>
int all_to_all_v(ctmr_group* g, size_t unit, SendPtr send_ptr, SendCnt send_cnt, RecvPtr recv_ptr, RecvCnt recv_cnt) {
  if (!g->rccl) {
    for (auto& d : g->local) {  // pull model: every destination copies its pieces, on its own stream
      GHIP(g, hipSetDevice(d.e->device));
      for (auto& s : g->local) {
        const uint64_t cnt = send_cnt(s)[d.rank];
        if (!cnt) continue;
        if (s.rank != d.rank) g->last_wire_bytes += cnt * unit;
        const uint8_t* src = (const uint8_t*)send_ptr(s) + prefix(send_cnt(s), d.rank) * unit;
        uint8_t* dst = (uint8_t*)recv_ptr(d) + prefix(recv_cnt(d), s.rank) * unit;
        if (s.e->device == d.e->device) GHIP(g, hipMemcpyAsync(dst, src, cnt * unit, hipMemcpyDeviceToDevice, d.e->stream));
        else GHIP(g, hipMemcpyPeerAsync(dst, d.e->device, src, s.e->device, cnt * unit, d.e->stream));
      }
    }
    return sync_all(g);
  }
  const RcclApi* api = rccl_api(nullptr);
  GroupRank& r = g->local[0];
  GHIP(g, hipSetDevice(r.e->device));
  const auto& sc = send_cnt(r);
  const auto& rc = recv_cnt(r);
  if (sc[r.rank])  // own partition: a local copy, no self send/recv
    GHIP(g, hipMemcpyAsync((uint8_t*)recv_ptr(r) + prefix(rc, r.rank) * unit,
                           (const uint8_t*)send_ptr(r) + prefix(sc, r.rank) * unit, sc[r.rank] * unit,
                           hipMemcpyDeviceToDevice, r.e->stream));
  GNCCL(g, api, api->GroupStart());
  for (uint32_t p = 0; p < g->world; p++) {
    if (p == r.rank) continue;
    if (rc[p]) GNCCL(g, api, api->Recv((uint8_t*)recv_ptr(r) + prefix(rc, p) * unit, rc[p] * unit, ncclUint8, (int)p, r.comm, r.e->stream));
    if (sc[p]) {
      GNCCL(g, api, api->Send((const uint8_t*)send_ptr(r) + prefix(sc, p) * unit, sc[p] * unit, ncclUint8, (int)p, r.comm, r.e->stream));
      g->last_wire_bytes += sc[p] * unit;
    }
  }
  GNCCL(g, api, api->GroupEnd());
  GSYNC(g, (r.e->stream));
  return CTMR_OK;
}

// The same exchange for ONE CHUNK of a chunked owner-computes round, asynchronous: it runs on the ranks' transfer streams
// (GroupRank::xfer) and is not waited for — the engines' own streams go on with the next chunk's map meanwhile.  Chunk c
// of rank r lies at record csend_off[c] of its send buffer, partitioned by owner (csend[c]); what it receives goes to
// record crecv_off[c] of its receive buffer, in sender order (crecv[c]).  xfer_wait() drains the transfer streams.
int control_gather(ctmr_group* g, uint32_t K);
int xfer_streams(ctmr_group* g) {
  // A rank-local failure in here must not return before the collective below: the peers would block in its all-gather or in
  // CommInitRank for ever (ADVICE r05).  The local status travels in column 0 of the gathered row and every rank fails
  // together — or none does.
  int local_rc = CTMR_OK;
  for (auto& r : g->local)
    if (!r.xfer) {
      if (hipSetDevice(r.e->device) != hipSuccess || hipStreamCreateWithFlags(&r.xfer, hipStreamNonBlocking) != hipSuccess) {
        r.xfer = nullptr;
        local_rc = CTMR_E_HIP;
      }
    }
  if (g->rccl && !g->local[0].xcomm) {
    // the second communicator: rank 0 draws a fresh id, one control all-gather (over the first communicator) hands it to
    // everybody, every rank joins.  Collective: all ranks reach this point together — in ctmr_group_set_chunks (every rank
    // calls it with the same count), or, for a group whose count was set before it had a transport, in the first chunked
    // round (the count is agreed in the opening control row).
    const RcclApi* api = rccl_api(nullptr);
    GroupRank& r = g->local[0];
    constexpr uint32_t K = 1 + CTMR_GROUP_ID_BYTES / 8;
    ncclUniqueId u;
    memset(&u, 0, sizeof u);
    if (r.rank == 0 && api->GetUniqueId(&u) != ncclSuccess) local_rc = CTMR_E_HIP;
    const std::vector<uint64_t> keep_out = r.ctl_out, keep_in = r.ctl_in;  // (a round's opening row may still be being read)
    r.ctl_out.assign(K, 0);
    r.ctl_out[0] = (uint64_t)(int64_t)local_rc;
    memcpy(r.ctl_out.data() + 1, &u, CTMR_GROUP_ID_BYTES);
    int rc;
    if ((rc = control_gather(g, K))) return rc;
    memcpy(&u, r.ctl_in.data() + 1, CTMR_GROUP_ID_BYTES);  // rank 0's row
    rc = control_status(g, K);
    r.ctl_out = keep_out;
    r.ctl_in = keep_in;
    if (rc != CTMR_OK) return local_rc != CTMR_OK ? gfail(g, local_rc, "no transfer stream / communicator id on this rank") : rc;
    GHIP(g, hipSetDevice(r.e->device));
    GNCCL(g, api, api->CommInitRank(&r.xcomm, (int)g->world, u, (int)r.rank));
  } else if (local_rc != CTMR_OK) {
    return gfail(g, local_rc, "hipStreamCreateWithFlags failed: no transfer stream");
  }
  return CTMR_OK;
}
int xfer_wait(ctmr_group* g) {
  for (auto& r : g->local)
    if (r.xfer) {
      GHIP(g, hipSetDevice(r.e->device));
      GSYNC(g, (r.xfer));
    }
  return CTMR_OK;
}
int chunk_all_to_all_async(ctmr_group* g, size_t c) {
  const size_t unit = 32;
  if (!g->rccl) {
    for (auto& d : g->local) {  // pull model, as all_to_all_v — on the destination's transfer stream
      GHIP(g, hipSetDevice(d.e->device));
      for (auto& s : g->local) {
        const uint64_t cnt = s.csend[c][d.rank];
        if (!cnt) continue;
        if (s.rank != d.rank) g->last_wire_bytes += cnt * unit;
        const uint8_t* src = (const uint8_t*)s.keys.p + (s.csend_off[c] + prefix(s.csend[c], d.rank)) * unit;
        uint8_t* dst = (uint8_t*)d.recv.p + (d.crecv_off[c] + prefix(d.crecv[c], s.rank)) * unit;
        if (s.e->device == d.e->device) GHIP(g, hipMemcpyAsync(dst, src, cnt * unit, hipMemcpyDeviceToDevice, d.xfer));
        else GHIP(g, hipMemcpyPeerAsync(dst, d.e->device, src, s.e->device, cnt * unit, d.xfer));
      }
    }
    return CTMR_OK;
  }
  const RcclApi* api = rccl_api(nullptr);
  GroupRank& r = g->local[0];
  GHIP(g, hipSetDevice(r.e->device));
  const auto& sc = r.csend[c];
  const auto& rc = r.crecv[c];
  const uint8_t* sbase = (const uint8_t*)r.keys.p + r.csend_off[c] * unit;
  uint8_t* rbase = (uint8_t*)r.recv.p + r.crecv_off[c] * unit;
  if (sc[r.rank])
    GHIP(g, hipMemcpyAsync(rbase + prefix(rc, r.rank) * unit, sbase + prefix(sc, r.rank) * unit, sc[r.rank] * unit,
                           hipMemcpyDeviceToDevice, r.xfer));
  GNCCL(g, api, api->GroupStart());
  for (uint32_t p = 0; p < g->world; p++) {
    if (p == r.rank) continue;
    if (rc[p]) GNCCL(g, api, api->Recv(rbase + prefix(rc, p) * unit, rc[p] * unit, ncclUint8, (int)p, r.xcomm, r.xfer));
    if (sc[p]) {
      GNCCL(g, api, api->Send(sbase + prefix(sc, p) * unit, sc[p] * unit, ncclUint8, (int)p, r.xcomm, r.xfer));
      g->last_wire_bytes += sc[p] * unit;
    }
  }
  GNCCL(g, api, api->GroupEnd());
  return CTMR_OK;
}

// The Bloom all-gather: rank r's filter is row r of its own world x n_words buffer; afterwards every rank holds all rows.
int all_gather_filters(ctmr_group* g) {
  const size_t row = (size_t)g->bloom_words * 8;
  if (!g->rccl) {
    for (auto& d : g->local) {
      GHIP(g, hipSetDevice(d.e->device));
      for (auto& s : g->local) {
        if (s.rank == d.rank) continue;
        const uint8_t* src = (const uint8_t*)s.filters.p + (size_t)s.rank * row;
        uint8_t* dst = (uint8_t*)d.filters.p + (size_t)s.rank * row;
        if (s.e->device == d.e->device) GHIP(g, hipMemcpyAsync(dst, src, row, hipMemcpyDeviceToDevice, d.e->stream));
        else GHIP(g, hipMemcpyPeerAsync(dst, d.e->device, src, s.e->device, row, d.e->stream));
      }
    }
    return sync_all(g);
  }
  const RcclApi* api = rccl_api(nullptr);
  GroupRank& r = g->local[0];
  GHIP(g, hipSetDevice(r.e->device));
  GNCCL(g, api, api->AllGather((const uint8_t*)r.filters.p + (size_t)r.rank * row, r.filters.p, g->bloom_words, ncclUint64,
                               r.comm, r.e->stream));
  GSYNC(g, (r.e->stream));
  return CTMR_OK;
}

// Σ over ranks of n u64 per rank (host vectors in, the sum out): the all-reduce of the per-issuer counts.
int all_reduce_sum(ctmr_group* g, std::vector<std::vector<uint64_t>>& per_local, uint32_t n, uint64_t* out) {
  for (uint32_t i = 0; i < n; i++) out[i] = 0;
  if (!g->rccl) {
    for (auto& v : per_local)
      for (uint32_t i = 0; i < n; i++) out[i] += v[i];
    return CTMR_OK;
  }
  if (n == 0) return CTMR_OK;
  const RcclApi* api = rccl_api(nullptr);
  GroupRank& r = g->local[0];
  int rc;
  if ((rc = gbuf(g, r, r.small, (size_t)n * 8 + 4096))) return rc;
  GHIP(g, hipSetDevice(r.e->device));
  GHIP(g, hipMemcpyAsync(r.small.p, per_local[0].data(), (size_t)n * 8, hipMemcpyHostToDevice, r.e->stream));
  GNCCL(g, api, api->AllReduce(r.small.p, r.small.p, n, ncclUint64, ncclSum, r.comm, r.e->stream));
  GHIP(g, hipMemcpyAsync(out, r.small.p, (size_t)n * 8, hipMemcpyDeviceToHost, r.e->stream));
  GSYNC(g, (r.e->stream));
  return CTMR_OK;
}

// offsets[n] - offsets[0] of a packed shard (the whole blob for an entry view): ctmr_batch_stats.payload_bytes
int shard_payload_bytes(ctmr_group* g, GroupRank& r, const ctmr_shard& s, uint64_t* out) {
  *out = 0;
  if (!s.n) return CTMR_OK;
  if (s.d_ends) { *out = s.blob_bytes; return CTMR_OK; }
  uint64_t ends[2];
  GHIP(g, hipSetDevice(r.e->device));
  GHIP(g, hipMemcpy(&ends[0], s.d_offsets, 8, hipMemcpyDeviceToHost));
  GHIP(g, hipMemcpy(&ends[1], s.d_offsets + s.n, 8, hipMemcpyDeviceToHost));
  *out = ends[1] - ends[0];
  return CTMR_OK;
}

ctmr_entry_view shard_view(const ctmr_shard& s) {
  ctmr_entry_view v;
  memset(&v, 0, sizeof v);
  v.cert_start = (uint64_t*)s.d_offsets;
  v.cert_end = (uint64_t*)s.d_ends;
  v.issuer_idx = (uint32_t*)s.d_issuer_idx;
  v.entry_type = (uint8_t*)s.d_entry_type;
  return v;
}

int rank_fail(ctmr_group* g, GroupRank& r, int code) {
  return gfail(g, code, "rank %u: %s", r.rank, ctmr_last_error(r.e));
}

// the round's first failure on this process, or OK
int round_result(ctmr_group* g) {
  for (auto& r : g->local)
    if (r.rc != CTMR_OK) return r.rc;
  return CTMR_OK;
}

// End of a round: every rank learns whether every rank got through (a rank that failed late has still taken part in
// every collective, so nobody is left waiting).
int round_agree(ctmr_group* g) {
  const int mine = round_result(g);
  if (!g->rccl) return mine;
  for (auto& r : g->local) r.ctl_out.assign(1, (uint64_t)(int64_t)r.rc);
  const int rc = control_gather(g, 1);
  if (rc) return rc;
  if (mine != CTMR_OK) return mine;
  return control_status(g, 1);
}

// A one-column status row in the middle of a round: every rank learns whether every rank is still able to go on (the
// receive buffers, whose sizes only the previous row told, have just been allocated).  A rank that could not allocate says
// so here and every rank leaves the round together — instead of its peers entering an exchange against a rank that has
// returned (advisor, round 3).
int status_row(ctmr_group* g) {
  for (auto& r : g->local) r.ctl_out.assign(1, (uint64_t)(int64_t)r.rc);
  int rc;
  if ((rc = control_gather(g, 1))) return rc;
  if ((rc = round_result(g))) return rc;
  return control_status(g, 1);
}

// Start of an exact round: nothing of an earlier round's long-serial list may be taken for this round's (a rank whose
// shard is empty does not run the map).
void round_open(ctmr_group* g) {
  for (auto& r : g->local) {
    std::lock_guard<std::mutex> lk(r.e->mu);
    r.e->rd.host_list.clear();
  }
}

// End of an exact round.  Members whose serial is longer than CTMR_MAX_SERIAL live in a host-side set per rank and were
// decided by each rank for itself; here the ranks settle them between each other, so that they too are stored once and
// WasUnknown goes to the lowest log index, as with the reference's single Redis set.  The common case (no such member in
// the round: RFC 5280 allows 20 octets) costs nothing beyond the closing status row, which carries the list sizes:
//   1. every rank lists the members it ADDED in this round (order, expiry hour, issuer, serial)  → control all-gather;
//   2. every rank says which of all listed members it has held since BEFORE this round          → all-reduce (sum);
//   3. every rank derives the same verdict: a member somebody held before is known to everybody; otherwise the lowest
//      (order, rank) keeps it — the others take it out of their set again and clear WasUnknown.
int round_finish(ctmr_group* g, ctmr_batch_stats* stats) {
  const uint32_t W = g->world;
  for (auto& r : g->local) {
    r.hk.clear();
    if (r.rc == CTMR_OK)
      for (const auto& h : r.e->rd.host_list) host_keys_append(r.hk, r.ord_base + h.i, h.exp_hour, h.canon, h.member);
    r.ctl_out.assign(2, 0);
    r.ctl_out[0] = (uint64_t)(int64_t)r.rc;
    r.ctl_out[1] = r.hk.size();
  }
  int rc;
  if ((rc = control_gather(g, 2))) return rc;
  if ((rc = round_result(g))) return rc;
  if ((rc = control_status(g, 2))) return rc;
  std::vector<uint64_t> words(W);
  uint64_t maxw = 0;
  for (uint32_t w = 0; w < W; w++) {
    words[w] = g->local[0].ctl_in[(size_t)w * 2 + 1];
    if (words[w] > maxw) maxw = words[w];
  }
  if (!maxw || W == 1) return CTMR_OK;
  if (maxw > (1u << 24)) return gfail(g, CTMR_E_RANGE, "more than 128 MiB of serials longer than %d octets in one round", CTMR_MAX_SERIAL);
  for (auto& r : g->local) {
    r.ctl_out.assign(maxw, 0);
    std::copy(r.hk.begin(), r.hk.end(), r.ctl_out.begin());
  }
  if ((rc = control_gather(g, (uint32_t)maxw))) return rc;
  std::vector<HostKeyCand> cands;
  const std::vector<uint64_t>& all = g->local[0].ctl_in;
  for (uint32_t w = 0; w < W; w++)
    if (!host_keys_parse(&all[(size_t)w * maxw], words[w], w, cands))
      return gfail(g, CTMR_E_INVAL, "rank %u sent a malformed long-serial list", w);
  const uint32_t nc = (uint32_t)cands.size();
  // 2. held here since before this round = in the set, and not one of this round's own additions
  std::vector<std::vector<uint64_t>> known(g->local.size(), std::vector<uint64_t>(nc, 0));
  for (size_t k = 0; k < g->local.size(); k++) {
    GroupRank& r = g->local[k];
    if (r.rc != CTMR_OK) continue;
    std::lock_guard<std::mutex> lk(r.e->mu);
    for (uint32_t c = 0; c < nc; c++) {
      const HostKeyCand& cd = cands[c];
      if (cd.rank == r.rank) continue;  // its own additions were new to it
      auto it = r.e->hstore.find(make_key(r.e, cd.exp_hour, cd.canon));
      if (it == r.e->hstore.end() || !it->second.count(cd.member)) continue;
      bool mine_now = false;
      for (const auto& h : r.e->rd.host_list)
        mine_now = mine_now || (h.exp_hour == cd.exp_hour && h.canon == cd.canon && h.member == cd.member);
      known[k][c] = !mine_now;
    }
  }
  std::vector<uint64_t> held(nc, 0);
  if ((rc = all_reduce_sum(g, known, nc, held.data()))) return rc;
  // 3. the verdict, the same on every rank (host_keys.h)
  std::vector<uint8_t> lost;
  host_keys_verdict(cands, held, lost);
  for (size_t k = 0; k < g->local.size(); k++) {
    GroupRank& r = g->local[k];
    if (r.rc != CTMR_OK) continue;
    std::vector<size_t> which;
    for (uint32_t c = 0; c < nc; c++)
      if (cands[c].rank == r.rank && lost[c]) which.push_back(cands[c].at);
    if (which.empty()) continue;
    std::lock_guard<std::mutex> lk(r.e->mu);
    (void)hipSetDevice(r.e->device);
    const int e1 = round_host_drop(r.e, r.e->rd, which);
    if (e1) {
      r.rc = rank_fail(g, r, e1);
      continue;
    }
    round_stats(r.e, r.e->rd, &r.st);
    if (stats) stats[k] = r.st;
  }
  return round_agree(g);
}

// A shard through the engine's plain map, as a packed batch or as an entry view.  No collective.
int map_shard(GroupRank& r, const ctmr_shard& s, uint64_t* d_new_idx, ctmr_batch_stats* st) {
  if (s.d_ends) {
    const ctmr_entry_view v = shard_view(s);
    return ctmr_map_view_device(r.e, s.d_payload, s.blob_bytes, &v, s.n, s.d_records, d_new_idx, st);
  }
  return ctmr_map_batch_device(r.e, s.d_payload, s.d_offsets, s.d_issuer_idx, s.d_entry_type, s.n, s.d_records, d_new_idx, st);
}

int group_map_local(ctmr_group* g, const ctmr_shard* sh, ctmr_batch_stats* stats) {
  PhaseClock clk{g};
  par_ranks(g, [&](size_t k) -> int {
    GroupRank& r = g->local[k];
    memset(&r.st, 0, sizeof r.st);
    if (!sh[k].n) return CTMR_OK;
    const int rc = map_shard(r, sh[k], sh[k].d_new_idx, &r.st);
    return rc ? rank_fail(g, r, rc) : CTMR_OK;
  });
  clk.lap(0);
  if (stats)
    for (size_t k = 0; k < g->local.size(); k++) stats[k] = g->local[k].st;
  return round_result(g);  // no collective in this mode: nobody waits for a failed rank
}

// The opening control row of an exact round: status | mode | filter words | order_base | n of every rank.  Whatever a
// rank has to refuse — an unknown mode, a mode other than the group's, a Bloom round without a configured filter, a bad
// shard — it says HERE and every rank leaves the round together, before any collective whose size depends on the answer
// (advisor, round 3: these paths used to return at once and left the peers waiting in the filter all-gather).  The row also
// lets every rank check what only the whole group can: that all ranks mean the same mode and the same filter size, and —
// for Bloom rounds, whose orders come from the host — that the shards' order ranges ascend with the rank and do not
// overlap: equal orders on two ranks would let both keep WasUnknown for one key (k_keys_lookup decides by order alone).
constexpr uint32_t KH = 5;  // columns of the opening row
int round_header(ctmr_group* g, int mode, const ctmr_shard* sh) {
  const uint32_t W = g->world;
  for (size_t k = 0; k < g->local.size(); k++) {
    GroupRank& r = g->local[k];
    if (r.rc == CTMR_OK && sh[k].n && !sh[k].d_records) r.rc = gfail(g, CTMR_E_INVAL, "an exact round needs d_records");
    r.ctl_out.assign(KH, 0);
    r.ctl_out[0] = (uint64_t)(int64_t)r.rc;
    r.ctl_out[1] = (uint64_t)(uint32_t)mode | ((uint64_t)g->chunks << 32);  // the mode, and in how many chunks shards are mapped
    r.ctl_out[2] = g->bloom_words;
    r.ctl_out[3] = sh[k].order_base;
    r.ctl_out[4] = sh[k].n;
  }
  int rc;
  if ((rc = control_gather(g, KH))) return rc;
  if ((rc = round_result(g))) return rc;
  if ((rc = control_status(g, KH))) return rc;
  const std::vector<uint64_t>& m = g->local[0].ctl_in;
  uint64_t next = 0;
  for (uint32_t w = 0; w < W; w++) {
    if ((int)(uint32_t)m[(size_t)w * KH + 1] != mode)
      return gfail(g, CTMR_E_INVAL, "rank %u runs this round in mode %d, this rank in mode %d", w, (int)(uint32_t)m[(size_t)w * KH + 1], mode);
    if ((uint32_t)(m[(size_t)w * KH + 1] >> 32) != g->chunks)
      return gfail(g, CTMR_E_INVAL, "rank %u maps its shard in %u chunks, this rank in %u (ctmr_group_set_chunks)", w,
                   (uint32_t)(m[(size_t)w * KH + 1] >> 32), g->chunks);
    if (mode != CTMR_DEDUP_BLOOM) continue;
    if (m[(size_t)w * KH + 2] != g->bloom_words)
      return gfail(g, CTMR_E_INVAL, "rank %u holds a filter of %llu words, this rank one of %llu", w,
                   (unsigned long long)m[(size_t)w * KH + 2], (unsigned long long)g->bloom_words);
    const uint64_t ob = m[(size_t)w * KH + 3], n = m[(size_t)w * KH + 4];
    if (n && ob < next)
      return gfail(g, CTMR_E_INVAL, "the shards' order ranges must ascend with the rank and not overlap: rank %u starts at %llu, "
                   "the ranks below it end at %llu (ctmr_shard.order_base)", w, (unsigned long long)ob, (unsigned long long)next);
    if (n) next = ob + n;
  }
  return CTMR_OK;
}

// ------------------------------------------------------------------ the steps the exact rounds share
// One copy of each, so that the invariant of a round — a rank that has failed still enters every collective its peers
// enter, in the same order and with the same sizes — is kept in one place per step.  The drivers below only say which
// steps a mode runs, in which order, and where the phase clock laps.

// The round's log order, from the opening row (round_header, already gathered): Σ n over all ranks, and for every local
// rank where its shard begins — Σ n of the lower ranks.  No collective; every rank reads the same row, so all return here
// or none does.
int round_log_order(ctmr_group* g, uint64_t* total_n) {
  const uint32_t W = g->world;
  *total_n = 0;
  for (uint32_t w = 0; w < W; w++) *total_n += g->local[0].ctl_in[(size_t)w * KH + 4];
  if (*total_n > 0xffffffffull) return gfail(g, CTMR_E_INVAL, "a round holds fewer than 2^32 entries over all ranks");
  for (auto& r : g->local) {
    r.ord_base = 0;
    for (uint32_t w = 0; w < r.rank; w++) r.ord_base += r.ctl_in[(size_t)w * KH + 4];
  }
  return CTMR_OK;
}

// The buffers and count vectors of one record stream of a rank: what leaves (keys, send), what arrives (recv, got), and
// the one byte per record that comes back (flags_out at the owner → flags_mine at the sender).
struct Chan {
  DevBuf GroupRank::*keys, GroupRank::*recv, GroupRank::*flags_out, GroupRank::*flags_mine;
  std::vector<uint64_t> GroupRank::*send, GroupRank::*got;
};
constexpr Chan MAIN{&GroupRank::keys, &GroupRank::recv, &GroupRank::flags_out, &GroupRank::flags_mine,
                    &GroupRank::send_counts, &GroupRank::recv_counts};
// … and the side channel of the owner-computes rounds: the rare 64-byte records (21..40-octet serials)
constexpr Chan SIDE64{&GroupRank::keys64, &GroupRank::recv64, &GroupRank::flags_out64, &GroupRank::flags_mine64,
                      &GroupRank::send_counts64, &GroupRank::recv_counts64};

struct CountCols {  // one set of W columns of a counts row: what the rank sends to each peer, what each peer sends it
  const std::vector<uint64_t>* send;
  std::vector<uint64_t>* got;
};
CountCols counts_of(GroupRank& r, const Chan& c) { return {&(r.*c.send), &(r.*c.got)}; }

// A counts row: every rank publishes status | ncol x W send counts (cols(r, j) names rank r's vectors of column set j),
// the row is gathered and its status column judged, and every rank reads its own column of each set: what every peer will
// send it.  totals[j] (optional) = Σ of set j over all senders and owners.  A failed rank enters the gather like its peers,
// with its code and zero counts; the verdict is the same on every rank, so all return here or none does — before any
// exchange whose sizes the row told.
template <class Cols>
int counts_row(ctmr_group* g, uint32_t ncol, Cols cols, uint64_t* totals = nullptr) {
  const uint32_t W = g->world, K = 1 + ncol * W;
  for (auto& r : g->local) {
    r.ctl_out.assign(K, 0);
    r.ctl_out[0] = (uint64_t)(int64_t)r.rc;
    if (r.rc != CTMR_OK) continue;
    for (uint32_t j = 0; j < ncol; j++)
      for (uint32_t w = 0; w < W; w++) r.ctl_out[1 + j * W + w] = (*cols(r, j).send)[w];
  }
  int rc;
  if ((rc = control_gather(g, K))) return rc;
  if ((rc = control_status(g, K))) return rc;
  for (auto& r : g->local)
    for (uint32_t j = 0; j < ncol; j++) {
      std::vector<uint64_t>& got = *cols(r, j).got;
      got.assign(W, 0);
      for (uint32_t s = 0; s < W; s++) got[s] = r.ctl_in[(size_t)s * K + 1 + j * W + r.rank];
    }
  if (totals)
    for (uint32_t j = 0; j < ncol; j++) {
      totals[j] = 0;
      for (uint32_t s = 0; s < W; s++)
        for (uint32_t w = 0; w < W; w++) totals[j] += g->local[0].ctl_in[(size_t)s * K + 1 + j * W + w];
    }
  return CTMR_OK;
}

// Room on rank r for what an exchange of `unit`-byte records brings: nrecv records in, a byte for each of them out, and a
// byte back for each of the nsend records that leave.  The first failure is returned, for note_failure: the status row
// that follows tells every rank, and all leave the round together.
int recv_buffers(ctmr_group* g, GroupRank& r, const Chan& c, size_t unit, uint64_t nsend, uint64_t nrecv) {
  int e1 = gbuf(g, r, r.*c.recv, (size_t)(nrecv ? nrecv : 1) * unit);
  if (!e1) e1 = gbuf(g, r, r.*c.flags_out, nrecv ? nrecv : 1);
  if (!e1) e1 = gbuf(g, r, r.*c.flags_mine, nsend ? nsend : 1);
  return e1;
}
void note_failure(GroupRank& r, int e1) {
  if (e1 && r.rc == CTMR_OK) r.rc = e1;
}

// One all-to-all: ends(r) names the buffer and the count vector rank r sends from and those it receives into.  A
// collective: every rank calls it, also one that failed after the status row before it (its buffers exist, what they
// hold is not used).
struct Ends {
  void* send;
  const std::vector<uint64_t>* send_cnt;
  void* recv;
  const std::vector<uint64_t>* recv_cnt;
};
template <class F>
int exchange(ctmr_group* g, size_t unit, F ends) {
  return all_to_all_v(g, unit, [&](GroupRank& r) { return ends(r).send; },
                      [&](GroupRank& r) -> const std::vector<uint64_t>& { return *ends(r).send_cnt; },
                      [&](GroupRank& r) { return ends(r).recv; },
                      [&](GroupRank& r) -> const std::vector<uint64_t>& { return *ends(r).recv_cnt; });
}
// key records → the ranks that answer for them …
int keys_there(ctmr_group* g, size_t unit, const Chan& c) {
  return exchange(g, unit, [&](GroupRank& r) { return Ends{(r.*c.keys).p, &(r.*c.send), (r.*c.recv).p, &(r.*c.got)}; });
}
// … and one byte per record back the way the keys came: the roles of the count vectors swapped
int flags_back(ctmr_group* g, const Chan& c) {
  return exchange(g, 1, [&](GroupRank& r) { return Ends{(r.*c.flags_out).p, &(r.*c.got), (r.*c.flags_mine).p, &(r.*c.send)}; });
}

// The 64-byte side channel of both owner-computes drivers.  any64 = Σ of the 64-byte counts over ALL ranks, from a counts
// row: the same on every rank, so either every rank enters the side channel's status row and exchanges or none does —
// whatever a rank's own counts are, and whether it has failed or not.
int side64_buffers(ctmr_group* g, GroupRank& r) {
  const int e1 = gbuf(g, r, r.keys64, (size_t)(r.n_keys64 ? r.n_keys64 : 1) * 64);
  return e1 ? e1 : recv_buffers(g, r, SIDE64, 64, r.n_keys64, prefix(r.recv_counts64, g->world));
}
int side64_there(ctmr_group* g, uint64_t any64) { return any64 ? keys_there(g, 64, SIDE64) : CTMR_OK; }
int side64_back(ctmr_group* g, uint64_t any64) { return any64 ? flags_back(g, SIDE64) : CTMR_OK; }

// The owner side of both owner-computes drivers: every rank inserts the records it received (r.recv_counts / 64 say how
// many, over all chunks), one "was unknown" byte per record, then resolves its own shard; and the round's traffic is
// counted.  No collective: a rank that fails here goes on into the exchange back with whatever its buffers hold.
void owner_insert(ctmr_group* g) {
  const uint32_t W = g->world;
  const bool alone = W == 1;  // one rank: it owns every key, nothing was exported
  g->last_keys_sent = g->last_keys_received = 0;
  par_ranks(g, [&](size_t k) -> int {
    GroupRank& r = g->local[k];
    const uint64_t nrecv = alone ? 0 : prefix(r.recv_counts, W), nrecv64 = alone ? 0 : prefix(r.recv_counts64, W);
    int e1 = ctmr_xchg_insert_device(r.e, r.recv.p, nrecv, r.recv64.p, nrecv64, (uint8_t*)r.flags_out.p, (uint8_t*)r.flags_out64.p);
    return e1 ? rank_fail(g, r, e1) : CTMR_OK;
  });
  for (auto& r : g->local) {
    g->last_keys_sent += r.n_keys + r.n_keys64 - r.send_counts[r.rank] - r.send_counts64[r.rank];
    g->last_keys_received += prefix(r.recv_counts, W) + prefix(r.recv_counts64, W) - r.recv_counts[r.rank] - r.recv_counts64[r.rank];
  }
}
// … and the sender side afterwards: the returned bytes → records, NEW list, stats.  No collective.
void owner_apply(ctmr_group* g, uint64_t any64) {
  const bool alone = g->world == 1;
  par_ranks(g, [&](size_t k) -> int {
    GroupRank& r = g->local[k];
    memset(&r.st, 0, sizeof r.st);
    int e1 = ctmr_xchg_apply_device(r.e, r.keys.p, (const uint8_t*)r.flags_mine.p, alone ? 0 : r.n_keys, r.keys64.p,
                                    (const uint8_t*)r.flags_mine64.p, (alone || !any64) ? 0 : r.n_keys64, &r.st);
    return e1 ? rank_fail(g, r, e1) : CTMR_OK;
  });
}

// The end of every exact round: the statistics out, then round_finish — the long-serial settlement and the closing row,
// collectives that every rank enters, failed or not — and the clock's last lap.
int round_tail(ctmr_group* g, ctmr_batch_stats* stats, PhaseClock& clk) {
  if (stats)
    for (size_t k = 0; k < g->local.size(); k++) stats[k] = g->local[k].st;
  const int rc = round_finish(g, stats);
  clk.lap(6);
  return rc;
}

// Owner-computes key exchange (SURVEY.md §8(e)(ii)): map (+ insert of the keys the rank owns) → key records all-to-all →
// owner insert → flags back → apply.
int group_map_owner(ctmr_group* g, const ctmr_shard* sh, ctmr_batch_stats* stats) {
  const uint32_t W = g->world;
  int rc;
  PhaseClock clk{g};
  round_open(g);
  uint64_t total_n;
  if ((rc = round_log_order(g, &total_n))) return rc;
  clk.lap(6);
  // ---- phase 1: map + insert of the locally owned keys + the other keys as records, partitioned by owner
  par_ranks(g, [&](size_t k) -> int {
    GroupRank& r = g->local[k];
    r.send_counts.assign(W, 0);
    r.send_counts64.assign(W, 0);
    r.n_keys64 = 0;
    int e1 = ctmr_xchg_map_device(r.e, &sh[k], W, r.rank, (uint32_t)r.ord_base, r.send_counts.data(), &r.n_keys64);
    return e1 ? rank_fail(g, r, e1) : CTMR_OK;
  });
  clk.lap(0);
  par_ranks(g, [&](size_t k) -> int {
    GroupRank& r = g->local[k];
    r.n_keys = prefix(r.send_counts, W);
    const uint64_t n_long = r.n_keys64;
    int e1;
    if ((e1 = gbuf(g, r, r.keys, (size_t)(r.n_keys ? r.n_keys : 1) * 32))) return e1;
    if (n_long && (e1 = gbuf(g, r, r.keys64, (size_t)n_long * 64))) return e1;
    if ((e1 = ctmr_xchg_keys_device(r.e, r.keys.p, r.keys64.p, r.send_counts64.data()))) return rank_fail(g, r, e1);
    return CTMR_OK;
  });
  clk.lap(1);
  // ---- control: who sends how much to whom (and: is everybody still there — a rank failed before anything was
  // exchanged: every rank stops here)
  uint64_t tot[2];
  if ((rc = counts_row(g, 2, [](GroupRank& r, uint32_t j) { return counts_of(r, j ? SIDE64 : MAIN); }, tot))) return rc;
  const uint64_t any64 = tot[1];
  clk.lap(6);
  const bool alone = W == 1;  // one rank: it owns every key, nothing was exported
  // from here on a failed rank still takes part in every collective (with whatever its buffers hold)
  for (auto& r : g->local) {
    int e1 = CTMR_OK;
    if (!alone) {
      e1 = recv_buffers(g, r, MAIN, 32, r.n_keys, prefix(r.recv_counts, W));
      if (any64 && !e1) e1 = side64_buffers(g, r);
    }
    note_failure(r, e1);  // no memory for the receive buffers: said in the row below
  }
  if (!alone && (rc = status_row(g))) return rc;
  // ---- exchange A: key partitions → owners
  if (!alone) {
    if ((rc = keys_there(g, 32, MAIN))) return rc;
    if ((rc = side64_there(g, any64))) return rc;
  }
  clk.lap(2);
  owner_insert(g);  // ---- phase 2
  clk.lap(3);
  // ---- exchange B: the bytes go back the way the keys came
  if (!alone) {
    if ((rc = flags_back(g, MAIN))) return rc;
    if ((rc = side64_back(g, any64))) return rc;
  }
  clk.lap(4);
  owner_apply(g, any64);  // ---- phase 3
  clk.lap(5);
  return round_tail(g, stats, clk);
}

// The owner-computes round with every shard mapped in K CHUNKS (ctmr_group_set_chunks): chunk c's key records travel — on
// the ranks' transfer streams — while chunk c + 1 is being walked on the engines' own streams; the owner-side insert, the
// bytes back and the apply run once, over everything, exactly as in group_map_owner.  Inside one round this changes no
// result: pass-1 claims commute and pass 2 settles by order whatever arrived first (DESIGN.md §6).  Costs: one control
// row per chunk (the counts of a grouped send/recv must be known on both sides), and send / receive buffers sized for the
// worst case before the first chunk is mapped (every key of the shard may leave, every key of the other shards may arrive).
int group_map_owner_chunked(ctmr_group* g, const ctmr_shard* sh, ctmr_batch_stats* stats) {
  const uint32_t W = g->world, K = g->chunks;
  int rc;
  PhaseClock clk{g};
  round_open(g);
  if ((rc = xfer_streams(g))) return rc;
  uint64_t total_n;
  if ((rc = round_log_order(g, &total_n))) return rc;
  for (size_t k = 0; k < g->local.size(); k++) {
    GroupRank& r = g->local[k];
    const uint64_t n = sh[k].n, others = total_n - n;
    r.csend.assign(K, std::vector<uint64_t>(W, 0));
    r.crecv.assign(K, std::vector<uint64_t>(W, 0));
    r.csend_off.assign(K, 0);
    r.crecv_off.assign(K, 0);
    r.send_counts.assign(W, 0);  // Σ over the chunks so far; r.n_keys = how many records that is
    r.recv_counts.assign(W, 0);
    r.send_counts64.assign(W, 0);
    r.recv_counts64.assign(W, 0);
    r.n_keys = r.n_keys64 = 0;
    int e1 = gbuf(g, r, r.keys, (size_t)(n ? n : 1) * 32);
    if (!e1) e1 = recv_buffers(g, r, MAIN, 32, n, others);
    note_failure(r, e1);
  }
  if ((rc = status_row(g))) return rc;
  clk.lap(6);
  // once a chunk may be on the wire, a round that stops early stops behind the transfers already in flight
  auto stop = [&](int code) {
    (void)xfer_wait(g);
    return code;
  };
  // ---- the chunks: map c, tell the counts, put c on the wire, go on with c + 1
  for (uint32_t c = 0; c < K; c++) {
    par_ranks(g, [&](size_t k) -> int {
      GroupRank& r = g->local[k];
      const ctmr_shard& s = sh[k];
      const uint64_t cs = ((s.n + K - 1) / K + 1023) & ~1023ull;
      const uint64_t lo = (uint64_t)c * cs < s.n ? (uint64_t)c * cs : s.n;
      const uint64_t hi = (c + 1 == K || (uint64_t)(c + 1) * cs > s.n) ? s.n : (uint64_t)(c + 1) * cs;
      if (lo == hi && !(s.n == 0 && c == 0)) return CTMR_OK;  // nothing of this shard in this chunk
      uint64_t n_long = 0;
      int e1 = ctmr_xchg_map_chunk_device(r.e, &s, W, r.rank, (uint32_t)r.ord_base, lo, hi, (uint8_t*)r.keys.p + r.n_keys * 32,
                                          r.csend[c].data(), &n_long);
      if (e1) return rank_fail(g, r, e1);
      if (hi == s.n) r.n_keys64 = n_long;
      return CTMR_OK;
    });
    clk.lap(0);
    if ((rc = counts_row(g, 1, [c](GroupRank& r, uint32_t) { return CountCols{&r.csend[c], &r.crecv[c]}; }))) return stop(rc);
    for (auto& r : g->local) {  // where chunk c lies in the send / receive buffers: behind the chunks before it
      r.csend_off[c] = r.n_keys;
      r.crecv_off[c] = prefix(r.recv_counts, W);
      for (uint32_t w = 0; w < W; w++) {
        r.send_counts[w] += r.csend[c][w];
        r.recv_counts[w] += r.crecv[c][w];
      }
      r.n_keys = prefix(r.send_counts, W);
    }
    clk.lap(6);
    if ((rc = chunk_all_to_all_async(g, c))) return stop(rc);
  }
  // ---- the rare 64-byte records (21..40-octet serials) of the whole shard, after the last chunk: one more row, one exchange
  par_ranks(g, [&](size_t k) -> int {
    GroupRank& r = g->local[k];
    if (!r.n_keys64) return CTMR_OK;
    int e1;
    if ((e1 = gbuf(g, r, r.keys64, (size_t)r.n_keys64 * 64))) return e1;
    if ((e1 = ctmr_xchg_keys_device(r.e, nullptr, r.keys64.p, r.send_counts64.data()))) return rank_fail(g, r, e1);
    return CTMR_OK;
  });
  uint64_t any64 = 0;
  if ((rc = counts_row(g, 1, [](GroupRank& r, uint32_t) { return counts_of(r, SIDE64); }, &any64))) return stop(rc);
  if (any64) {
    for (auto& r : g->local) note_failure(r, side64_buffers(g, r));
    if ((rc = status_row(g))) return stop(rc);
    if ((rc = side64_there(g, any64))) return stop(rc);
  }
  if ((rc = xfer_wait(g))) return rc;  // every chunk has arrived
  clk.lap(2);
  owner_insert(g);  // ---- all chunks at once
  clk.lap(3);
  // ---- the bytes go back the way the keys came, chunk by chunk: flags_back, with each chunk where it lies in the buffers
  for (uint32_t c = 0; c < K; c++)
    if ((rc = exchange(g, 1, [c](GroupRank& r) {
           return Ends{(uint8_t*)r.flags_out.p + r.crecv_off[c], &r.crecv[c], (uint8_t*)r.flags_mine.p + r.csend_off[c], &r.csend[c]};
         })))
      return rc;
  if ((rc = side64_back(g, any64))) return rc;
  clk.lap(4);
  owner_apply(g, any64);
  clk.lap(5);
  return round_tail(g, stats, clk);
}

// Bloom pre-filter variant (north_star: "all-gather of per-GPU Bloom fingerprints"; SURVEY.md §8(e)(i)), exact:
// local fused map + insert + filter add (one kernel) → all-gather → probe → key records to the peers whose filter matched
// → exact lookup there → flags back → apply.
int group_map_bloom(ctmr_group* g, const ctmr_shard* sh, ctmr_batch_stats* stats) {
  const uint32_t W = g->world;
  int rc;
  PhaseClock clk{g};
  round_open(g);
  par_ranks(g, [&](size_t k) -> int {  // phases 1 + 2: the map adds the keys it finds new to the rank's filter on the way
    GroupRank& r = g->local[k];
    const ctmr_shard& s = sh[k];
    r.ord_base = s.order_base;
    int e1 = s.n ? map_shard(r, s, nullptr, nullptr) : CTMR_OK;
    if (!e1 && W > 1) e1 = ctmr_bloom_add_device(r.e, s.d_payload, s.d_offsets, s.d_ends, s.n, s.d_records);
    return e1 ? rank_fail(g, r, e1) : CTMR_OK;
  });
  clk.lap(0);
  // the filters are exchanged whatever happened (a failed rank's filter is as good as any: its answers are not used)
  if (W > 1 && (rc = all_gather_filters(g))) return rc;
  g->last_filter_bytes_received = (uint64_t)(W - 1) * g->bloom_words * 8;
  if (W > 1) g->last_wire_bytes += (uint64_t)g->local.size() * (W - 1) * g->bloom_words * 8;
  par_ranks(g, [&](size_t k) -> int {  // phase 3: probe the peers' filters
    GroupRank& r = g->local[k];
    const ctmr_shard& s = sh[k];
    r.send_counts.assign(W, 0);
    r.n_keys = 0;
    if (W == 1) return CTMR_OK;  // nobody to ask
    uint64_t cap = r.keys.cap / 64;
    if (cap < 1024) cap = 1024;
    if (cap < s.n / 4) cap = s.n / 4;
    for (;;) {
      int e1;
      if ((e1 = gbuf(g, r, r.keys, (size_t)cap * 64))) return e1;
      const int pr = ctmr_bloom_probe_device(r.e, s.d_payload, s.d_offsets, s.d_ends, s.n, s.d_records, r.filters.p, W,
                                             r.rank, s.order_base, r.keys.p, cap, r.send_counts.data());
      if (pr == CTMR_OK) break;
      if (pr != CTMR_E_RANGE) return rank_fail(g, r, pr);
      cap = prefix(r.send_counts, W);  // counts are filled: exactly what is needed
    }
    r.n_keys = prefix(r.send_counts, W);
    return CTMR_OK;
  });
  clk.lap(1);
  if ((rc = counts_row(g, 1, [](GroupRank& r, uint32_t) { return counts_of(r, MAIN); }))) return rc;
  clk.lap(6);
  for (auto& r : g->local) {
    int e1 = gbuf(g, r, r.keys, 64);
    if (!e1) e1 = recv_buffers(g, r, MAIN, 64, r.n_keys, prefix(r.recv_counts, W));
    note_failure(r, e1);  // said in the row below: every rank leaves together
  }
  if (W > 1 && (rc = status_row(g))) return rc;
  if (W > 1 && (rc = keys_there(g, 64, MAIN))) return rc;
  clk.lap(2);
  g->last_keys_sent = g->last_keys_received = 0;
  par_ranks(g, [&](size_t k) -> int {  // phase 4: exact, read-only lookup at the peer
    GroupRank& r = g->local[k];
    const uint64_t nrecv = prefix(r.recv_counts, W);
    if (!nrecv) return CTMR_OK;
    int e1 = ctmr_bloom_lookup_device(r.e, r.recv.p, nrecv, sh[k].order_base, (uint8_t*)r.flags_out.p);
    return e1 ? rank_fail(g, r, e1) : CTMR_OK;
  });
  for (auto& r : g->local) {
    g->last_keys_sent += r.n_keys;
    g->last_keys_received += prefix(r.recv_counts, W);
  }
  clk.lap(3);
  if (W > 1 && (rc = flags_back(g, MAIN))) return rc;
  clk.lap(4);
  par_ranks(g, [&](size_t k) -> int {  // phase 5
    GroupRank& r = g->local[k];
    const ctmr_shard& s = sh[k];
    memset(&r.st, 0, sizeof r.st);
    int e1 = ctmr_bloom_apply_device(r.e, s.d_records, s.n, r.keys.p, (const uint8_t*)r.flags_mine.p, r.n_keys, s.d_new_idx, &r.st);
    return e1 ? rank_fail(g, r, e1) : CTMR_OK;
  });
  clk.lap(5);
  return round_tail(g, stats, clk);
}

}  // namespace
}  // extern "C++"

int ctmr_group_create_local(ctmr_engine* const* engines, uint32_t n, ctmr_group** out) {
  if (!engines || !out || n == 0 || n > MAX_WORLD) return CTMR_E_INVAL;
  for (uint32_t i = 0; i < n; i++) {
    if (!engines[i]) return CTMR_E_INVAL;
    for (uint32_t j = 0; j < i; j++)
      if (engines[j] == engines[i]) return CTMR_E_INVAL;
  }
  ctmr_group* g = new ctmr_group();
  g->world = n;
  g->rccl = false;
  g->local.resize(n);
  for (uint32_t i = 0; i < n; i++) {
    g->local[i].e = engines[i];
    g->local[i].rank = i;
  }
  // peer access between the devices of the group, where the platform offers it (copies fall back to staging otherwise)
  for (uint32_t i = 0; i < n; i++)
    for (uint32_t j = 0; j < n; j++) {
      const int a = engines[i]->device, b = engines[j]->device;
      if (a == b) continue;
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, a, b) == hipSuccess && can && hipSetDevice(a) == hipSuccess) {
        const hipError_t r = hipDeviceEnablePeerAccess(b, 0);
        if (r != hipSuccess) (void)hipGetLastError();  // already enabled
      }
    }
  *out = g;
  return CTMR_OK;
}

int ctmr_group_unique_id(uint8_t id[CTMR_GROUP_ID_BYTES]) {
  if (!id) return CTMR_E_INVAL;
  static_assert(CTMR_GROUP_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");
  std::string why;
  const RcclApi* api = rccl_api(&why);
  if (!api) { fprintf(stderr, "ctmr_group_unique_id: %s\n", why.c_str()); return CTMR_E_HIP; }
  ncclUniqueId u;
  if (api->GetUniqueId(&u) != ncclSuccess) return CTMR_E_HIP;
  memcpy(id, &u, CTMR_GROUP_ID_BYTES);
  return CTMR_OK;
}

int ctmr_group_create_rccl(ctmr_engine* engine, const uint8_t id[CTMR_GROUP_ID_BYTES], uint32_t rank, uint32_t world,
                           ctmr_group** out) {
  if (!engine || !id || !out || world == 0 || world > MAX_WORLD || rank >= world) return CTMR_E_INVAL;
  std::string why;
  const RcclApi* api = rccl_api(&why);
  if (!api) return fail(engine, CTMR_E_HIP, "%s", why.c_str());
  std::lock_guard<std::mutex> lk(engine->mu);
  HIPCHK(engine, hipSetDevice(engine->device));
  ncclUniqueId u;
  memcpy(&u, id, CTMR_GROUP_ID_BYTES);
  ncclComm_t comm = nullptr;
  const ncclResult_t r = api->CommInitRank(&comm, (int)world, u, (int)rank);
  if (r != ncclSuccess) return fail(engine, CTMR_E_HIP, "ncclCommInitRank: %s", api->GetErrorString(r));
  ctmr_group* g = new ctmr_group();
  g->world = world;
  g->rccl = true;
  g->local.resize(1);
  g->local[0].e = engine;
  g->local[0].rank = rank;
  g->local[0].comm = comm;
  *out = g;
  return CTMR_OK;
}

void ctmr_group_destroy(ctmr_group* g) {
  if (!g) return;
  for (auto& r : g->local) {
    (void)hipSetDevice(r.e->device);
    (void)hipStreamSynchronize(r.e->stream);
    if (g->bloom_words && g->world > 1) {  // the engine's filter lives in r.filters: detach before freeing
      std::lock_guard<std::mutex> lk(r.e->mu);
      if (!r.e->bloom_owned) { r.e->d_bloom = nullptr; r.e->bloom_words = 0; }
    }
    for (DevBuf* b : {&r.keys, &r.recv, &r.flags_out, &r.flags_mine, &r.small, &r.filters, &r.keys64, &r.recv64, &r.flags_out64,
                      &r.flags_mine64})
      if (b->p) (void)hipFree(b->p);
    if (r.xfer) (void)hipStreamDestroy(r.xfer);
    if (r.comm || r.xcomm) {
      const RcclApi* api = rccl_api(nullptr);
      if (api && r.xcomm) (void)api->CommDestroy(r.xcomm);
      if (api && r.comm) (void)api->CommDestroy(r.comm);
    }
  }
  delete g;
}

// copied for the calling thread, like ctmr_last_error: the ranks of a LOCAL group report from threads of their own
const char* ctmr_group_last_error(const ctmr_group* g) {
  if (!g) return "null group";
  static thread_local std::string copy;
  {
    std::lock_guard<std::mutex> lk(const_cast<ctmr_group*>(g)->err_mu);
    copy = g->err;
  }
  return copy.c_str();
}

int ctmr_group_info(ctmr_group* g, ctmr_group_stats* out) {
  if (!g || !out) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> lk(g->mu);
  memset(out, 0, sizeof *out);
  out->world = g->world;
  out->n_local = (uint32_t)g->local.size();
  out->transport = g->rccl ? CTMR_TRANSPORT_RCCL : CTMR_TRANSPORT_LOCAL;
  out->first_local_rank = g->local[0].rank;
  out->keys_sent = g->last_keys_sent;
  out->keys_received = g->last_keys_received;
  out->filter_bytes_received = g->last_filter_bytes_received;
  out->wire_bytes_sent = g->last_wire_bytes;
  for (int k = 0; k < 8; k++) out->ms_phase[k] = g->ms_phase[k];
  return CTMR_OK;
}

int ctmr_group_set_chunks(ctmr_group* g, uint32_t chunks) {
  if (!g) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> lk(g->mu);
  if (chunks < 1 || chunks > 64) return gfail(g, CTMR_E_INVAL, "chunks per shard: 1..64");
  g->chunks = chunks;
  // COLLECTIVE on an RCCL group when chunks > 1 (every rank calls it with the same count): the transfer streams and the
  // second communicator are made here, not inside the first chunked round (ADVICE r05)
  if (chunks > 1) return xfer_streams(g);
  return CTMR_OK;
}

int ctmr_group_bloom_config(ctmr_group* g, uint64_t bits) {
  if (!g) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> lk(g->mu);
  if (bits < 4096 || bits > (1ull << 40) || (bits & (bits - 1)))
    return gfail(g, CTMR_E_INVAL, "Bloom filter size must be a power of two in [2^12, 2^40] bits");
  const uint64_t words = bits / 64;
  if (g->world == 1) {  // a group of one has no peer to ask: no filter is kept, the round is the plain reduce
    g->bloom_words = words;
    return CTMR_OK;
  }
  for (auto& r : g->local) {
    int rc;
    if (g->bloom_words) {  // re-configuration: detach the old buffer first
      std::lock_guard<std::mutex> lk2(r.e->mu);
      if (!r.e->bloom_owned) { r.e->d_bloom = nullptr; r.e->bloom_words = 0; }
    }
    if ((rc = gbuf(g, r, r.filters, (size_t)g->world * words * 8))) return rc;
    GHIP(g, hipSetDevice(r.e->device));
    GHIP(g, hipMemsetAsync(r.filters.p, 0, (size_t)g->world * words * 8, r.e->stream));
    GSYNC(g, (r.e->stream));
    GENG(g, r, ctmr_bloom_config(r.e, bits, (uint8_t*)r.filters.p + (size_t)r.rank * words * 8));
  }
  g->bloom_words = words;
  return CTMR_OK;
}

int ctmr_group_map_batch(ctmr_group* g, int mode, const ctmr_shard* shards, ctmr_batch_stats* stats) {
  if (!g || !shards) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> lk(g->mu);
  g->last_keys_sent = g->last_keys_received = g->last_filter_bytes_received = g->last_wire_bytes = 0;
  for (auto& r : g->local) r.rc = CTMR_OK;
  for (auto& m : g->ms_phase) m = 0.f;
  const bool known = mode == CTMR_DEDUP_LOCAL || mode == CTMR_DEDUP_OWNER || mode == CTMR_DEDUP_BLOOM;
  // One mode per group.  Where a key lives differs between the modes — at its owner (OWNER), at the rank that saw it first
  // with the other ranks' filters knowing it (BLOOM), at whoever mapped it (LOCAL) — and neither exact mode can see what
  // another mode stored: an OWNER round never sets Bloom bits, so a later BLOOM round would miss a key stored at its
  // owner and count the certificate twice, silently (advisor, round 3).
  // A call this rank has to refuse is refused THROUGH the opening control row of the round (round_header) unless the mode
  // is LOCAL on both sides of the comparison (LOCAL rounds have no collective): the peers of a multi-process group may be
  // on their way into that row already.
  int refuse = CTMR_OK;
  if (!known) refuse = gfail(g, CTMR_E_INVAL, "unknown dedup mode %d", mode);
  else if (g->mode >= 0 && mode != g->mode)
    refuse = gfail(g, CTMR_E_INVAL, "this group deduplicates in mode %d since its first round; mode %d needs a group of its own", g->mode, mode);
  else if (mode == CTMR_DEDUP_BLOOM && !g->bloom_words)
    refuse = gfail(g, CTMR_E_INVAL, "ctmr_group_bloom_config has not been called");
  if (refuse) {
    const bool collective = (!known || mode != CTMR_DEDUP_LOCAL) && g->mode != CTMR_DEDUP_LOCAL;
    if (!collective) return refuse;
    for (auto& r : g->local) r.rc = refuse;
    (void)round_header(g, mode, shards);
    return refuse;
  }
  if (g->mode < 0) g->mode = mode;
  for (size_t k = 0; k < g->local.size(); k++) {
    const ctmr_shard& s = shards[k];
    // a rank with a bad shard does not return here: its peers are about to enter the round's collectives — it reports
    // through the round's status rows like any other failure
    if (s.n && (!s.d_payload || !s.d_offsets || !s.d_issuer_idx)) g->local[k].rc = gfail(g, CTMR_E_INVAL, "shard %zu: null input", k);
  }
  if (mode != CTMR_DEDUP_LOCAL) {
    const int rc = round_header(g, mode, shards);
    if (rc) return rc;
  }
  switch (mode) {
    case CTMR_DEDUP_LOCAL: return group_map_local(g, shards, stats);
    case CTMR_DEDUP_OWNER:
      return (g->chunks > 1 && g->world > 1) ? group_map_owner_chunked(g, shards, stats) : group_map_owner(g, shards, stats);
    case CTMR_DEDUP_BLOOM: return group_map_bloom(g, shards, stats);
    default: return gfail(g, CTMR_E_INVAL, "unknown dedup mode %d", mode);
  }
}

int ctmr_group_issuer_counts(ctmr_group* g, uint64_t* out, uint32_t n) {
  if (!g || (n && !out)) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> lk(g->mu);
  std::vector<std::vector<uint64_t>> per(g->local.size(), std::vector<uint64_t>(n ? n : 1, 0));
  for (size_t k = 0; k < g->local.size(); k++) GENG(g, g->local[k], ctmr_issuer_counts(g->local[k].e, per[k].data(), n));
  return all_reduce_sum(g, per, n, out);
}

int ctmr_group_total_count(ctmr_group* g, uint64_t* out) {
  if (!g || !out) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> lk(g->mu);
  std::vector<std::vector<uint64_t>> per(g->local.size(), std::vector<uint64_t>(1, 0));
  for (size_t k = 0; k < g->local.size(); k++) GENG(g, g->local[k], ctmr_total_count(g->local[k].e, per[k].data()));
  return all_reduce_sum(g, per, 1, out);
}

// Σ / max over the ranks of a few host-side u64 values: what a multi-process host needs besides the data path (the
// global NEW count of a round, the slowest rank's time) without bringing a second communication library.
int ctmr_group_all_reduce_u64(ctmr_group* g, uint64_t* values, uint32_t n, int op_max) {
  if (!g || (n && !values) || n > 4096) return CTMR_E_INVAL;
  std::lock_guard<std::mutex> lk(g->mu);
  if (!g->rccl || n == 0) return CTMR_OK;  // LOCAL: the caller holds every rank's values already
  const RcclApi* api = rccl_api(nullptr);
  GroupRank& r = g->local[0];
  int rc;
  if ((rc = gbuf(g, r, r.small, (size_t)n * 8 + 4096))) return rc;
  GHIP(g, hipSetDevice(r.e->device));
  GHIP(g, hipMemcpyAsync(r.small.p, values, (size_t)n * 8, hipMemcpyHostToDevice, r.e->stream));
  GNCCL(g, api, api->AllReduce(r.small.p, r.small.p, n, ncclUint64, op_max ? ncclMax : ncclSum, r.comm, r.e->stream));
  GHIP(g, hipMemcpyAsync(values, r.small.p, (size_t)n * 8, hipMemcpyDeviceToHost, r.e->stream));
  GSYNC(g, (r.e->stream));
  return CTMR_OK;
}

int ctmr_group_barrier(ctmr_group* g) {
  uint64_t v = 1;
  return ctmr_group_all_reduce_u64(g, &v, 1, 0);
}
