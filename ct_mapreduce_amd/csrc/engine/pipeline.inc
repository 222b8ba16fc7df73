// engine/pipeline.inc — asynchronous host ingestion: ctmr_submit_batch / ctmr_wait / ctmr_flush, the raw-entry and
// get-entries JSON forms of both (ctmr_submit_entries*, ctmr_wait_entries*) and the PEM form (ctmr_submit_pem, ctmr_wait_pem).
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after engine/map.inc; the
// worker's step for the JSON form is engine/pipeline_json.inc, behind engine/entries_json.inc, and the one for the PEM
// form engine/pipeline_pem.inc, behind engine/pem_decode.inc.
//
// The reference's downloader hands insertCTWorker one get-entries response at a time — at most 1 001 entries
// (cmd/ct-fetch/ct-fetch.go:417-424) — through a 16 384-entry channel (:132), and the workers drain it concurrently
// (:140-145, :191).  A synchronous ctmr_map_batch per response pays a full host↔device round trip for 1.5 MB of DER
// (7 M certificates/s, DESIGN.md §7).  This is the channel's counterpart in front of the GPU:
//   submit   the batch's small arrays are appended to the OPEN super-batch (pinned memory) and its DER goes to HBM
//            with one asynchronous copy on a copy stream, landing back to back behind the previous submit's bytes — the
//            device-side layout IS the packed layout, nothing is repacked.  Straight DMA from the caller's buffer when
//            it came from ctmr_alloc_pinned (the caller keeps it untouched until ctmr_wait); pageable memory is staged
//            by the runtime before the call returns.  Returns a ticket at once.
//   launch   when the open super-batch reaches 65 536 entries / 96 MB (or on ctmr_flush / a ctmr_wait for one of its
//            tickets) it is closed and queued for the engine's worker thread, which runs the ordinary map + reduce over
//            it — while the submitters are already filling, and the copy engine is already feeding, the next one.
//   wait     blocks until the ticket's super-batch is done, then hands out that batch's slice of the results.
// Super-batches run in submission order on one stream and entries keep their order inside one, so the lowest log index
// of a key still wins WasUnknown across everything in flight — exactly what a sequence of synchronous calls over the
// concatenated batches gives (tests/test_gpu_pipeline.py).

extern "C++" {
namespace {

constexpr uint32_t PIPE_SLOTS = 4;
constexpr uint32_t PIPE_MAX_STREAMS = 4;  // copy streams: consecutive submits' DMA transfers overlap their set-up
constexpr uint64_t PIPE_CLOSE_ENTRIES = 65536, PIPE_CLOSE_BYTES = 96ull << 20;
constexpr uint64_t PIPE_CLOSE_BODIES = 4096;  // JSON super-batches: the entries are not known before the worker has run
constexpr uint64_t PIPE_CLOSE_FILES = 65536;  // PEM super-batches: nor are the certificates; the reference writes one a file

// What a super-batch holds: the packed form (ctmr_submit_batch), blob + bounds u64[2n+1] (ctmr_submit_entries), or
// get-entries bodies as text (ctmr_submit_entries_json), or PEM files as text (ctmr_submit_pem).  One form per super-batch.
enum PipeForm : uint8_t { PF_PACKED = 0, PF_RAW, PF_JSON, PF_PEM };
// the two text forms: bodies (JSON: responses, PEM: files) judged alone by the worker, the tickets sized by what it finds
bool pipe_is_text(PipeForm f) { return f == PF_JSON || f == PF_PEM; }
// the forms whose entries are raw get-entries pairs: timestamps, entry types and Chain[0] lengths come back with them
bool pipe_is_raw(PipeForm f) { return f == PF_RAW || f == PF_JSON; }

struct PipeTicket {
  uint64_t first, n;  // its entries in the super-batch (JSON, PEM: known when the worker is done)
  bool consumed;
  uint64_t body0 = 0, nbody = 0;  // JSON, PEM: its bodies (responses, files) in the super-batch,
  uint64_t text_at = 0;           //   where its text starts in the slot's,
  uint64_t text_base = 0;         //   and resp_bounds[0] of the submit: offsets go back to the caller's text pointer
};

enum PipeState { PS_FREE = 0, PS_OPEN, PS_QUEUED, PS_DONE };

struct PipeSlot {
  PipeState state = PS_FREE;
  uint64_t seq = 0;
  // device side
  uint8_t* d_payload = nullptr; size_t payload_cap = 0;
  uint8_t* d_meta = nullptr; size_t meta_cap = 0;       // offsets u64[cap+1] | issuer_idx u32[cap] | entry_type u8[cap] — or, raw: bounds u64[2cap+1]
  ctmr_record* d_records = nullptr;
  uint64_t* d_new = nullptr;
  uint64_t ent_cap = 0;
  // pinned host side
  uint8_t* h_meta = nullptr;                            // same layout as d_meta
  ctmr_record* h_records = nullptr;
  uint64_t* h_new = nullptr;
  uint64_t* d_ts = nullptr;                             // raw super-batches: TimestampedEntry.Timestamp per entry
  uint64_t* h_ts = nullptr;
  uint8_t* h_etype = nullptr;                           // raw super-batches: the decoded entry types and Chain[0] lengths
  uint32_t* h_c0len = nullptr;                          //   (per-ticket decode stats)
  // fill state
  uint64_t n = 0, bytes = 0;
  bool any_type = false;
  PipeForm form = PF_PACKED;
  // JSON and PEM super-batches: d_payload holds the text.  The bodies' bounds in it live here, not in the meta buffers, which
  // pipe_slot_reserve frees when the worker sizes the slot by the entries found.
  std::vector<uint64_t> body_rb;                        // bodies + 1
  std::vector<uint64_t> body_first, body_bad;           // the worker's: each body's first entry (bodies + 1), its verdict
  uint8_t* d_blob = nullptr; size_t blob_cap = 0;       // the decoded entries; h_meta: their bounds u64[2n+1] (PEM: offsets u64[n+1])
  std::vector<uint32_t> file_iss;                       // PEM: the issuer index of every file
  std::vector<uint64_t> cert_lay;                       // PEM, the worker's: the layout of every certificate (a ticket's regular / irregular)
  ctmr_decode_stats dstats{};
  std::vector<PipeTicket> tickets;
  hipEvent_t ev_h2d[PIPE_MAX_STREAMS] = {};
  // result
  int rc = CTMR_OK;
  std::string err;
  ctmr_batch_stats stats{};
};

}  // namespace
}  // extern "C++"

struct ctmr_pipeline {
  std::mutex mu;                   // slots, queue, tickets (never held while the GPU is waited for)
  std::condition_variable cv;
  PipeSlot slots[PIPE_SLOTS];
  std::deque<uint32_t> queue;      // closed slots, submission order
  uint64_t next_seq = 1;
  int open = -1;
  hipStream_t copy_stream[PIPE_MAX_STREAMS] = {};
  uint32_t n_streams = 2, rr = 0;
  std::thread worker;
  bool stop = false;
};

extern "C++" {
namespace {

size_t pipe_meta_bytes(uint64_t cap) { return (2 * cap + 1) * 8; }  // the larger of the two layouts

int pipe_slot_reserve(ctmr_engine* e, PipeSlot& s, uint64_t entries, uint64_t bytes) {
  HIPCHK(e, hipSetDevice(e->device));
  for (auto& ev : s.ev_h2d)
    if (!ev) HIPCHK(e, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  if (entries > s.ent_cap) {
    uint64_t cap = s.ent_cap ? s.ent_cap : 2 * PIPE_CLOSE_ENTRIES;
    while (cap < entries) cap *= 2;
    (void)hipFree(s.d_meta); (void)hipFree(s.d_records); (void)hipFree(s.d_new); (void)hipFree(s.d_ts);
    (void)hipHostFree(s.h_meta); (void)hipHostFree(s.h_records); (void)hipHostFree(s.h_new); (void)hipHostFree(s.h_ts);
    (void)hipHostFree(s.h_etype); (void)hipHostFree(s.h_c0len);
    s.d_meta = nullptr; s.d_records = nullptr; s.d_new = nullptr; s.h_meta = nullptr; s.h_records = nullptr; s.h_new = nullptr;
    s.d_ts = nullptr; s.h_ts = nullptr; s.h_etype = nullptr; s.h_c0len = nullptr;
    s.ent_cap = 0;
    HIPCHK(e, hipMalloc(&s.d_meta, pipe_meta_bytes(cap)));
    HIPCHK(e, hipMalloc(&s.d_records, cap * sizeof(ctmr_record)));
    HIPCHK(e, hipMalloc(&s.d_new, cap * 8));
    HIPCHK(e, hipHostMalloc((void**)&s.h_meta, pipe_meta_bytes(cap), hipHostMallocDefault));
    HIPCHK(e, hipHostMalloc((void**)&s.h_records, cap * sizeof(ctmr_record), hipHostMallocDefault));
    HIPCHK(e, hipHostMalloc((void**)&s.h_new, cap * 8, hipHostMallocDefault));
    HIPCHK(e, hipMalloc(&s.d_ts, cap * 8));
    HIPCHK(e, hipHostMalloc((void**)&s.h_ts, cap * 8, hipHostMallocDefault));
    HIPCHK(e, hipHostMalloc((void**)&s.h_etype, cap, hipHostMallocDefault));
    HIPCHK(e, hipHostMalloc((void**)&s.h_c0len, cap * 4, hipHostMallocDefault));
    s.meta_cap = pipe_meta_bytes(cap);
    s.ent_cap = cap;
  }
  if (bytes + CTMR_PAYLOAD_PAD + 16 > s.payload_cap) {
    size_t cap = s.payload_cap ? s.payload_cap : 2 * PIPE_CLOSE_BYTES;
    while (cap < bytes + CTMR_PAYLOAD_PAD + 16) cap *= 2;
    (void)hipFree(s.d_payload);
    s.d_payload = nullptr;
    s.payload_cap = 0;
    HIPCHK(e, hipMalloc(&s.d_payload, cap));
    s.payload_cap = cap;
  }
  return CTMR_OK;
}

uint64_t* slot_h_offsets(PipeSlot& s) { return (uint64_t*)s.h_meta; }
uint32_t* slot_h_iss(PipeSlot& s) { return (uint32_t*)(s.h_meta + (s.ent_cap + 1) * 8); }
uint8_t* slot_h_et(PipeSlot& s) { return s.h_meta + (s.ent_cap + 1) * 8 + s.ent_cap * 4; }

// Close the open super-batch: its small arrays follow the DER on the copy stream; the worker takes it from the queue.
int pipe_close_locked(ctmr_engine* e, ctmr_pipeline* p) {
  if (p->open < 0) return CTMR_OK;
  PipeSlot& s = p->slots[p->open];
  HIPCHK(e, hipSetDevice(e->device));
  if (pipe_is_text(s.form)) {
    // (the bodies' bounds go to the device with the worker's call)
  } else if (s.form == PF_RAW) {
    slot_h_offsets(s)[2 * s.n] = s.bytes;
    HIPCHK(e, hipMemcpyAsync(s.d_meta, s.h_meta, (2 * s.n + 1) * 8, hipMemcpyHostToDevice, p->copy_stream[0]));
  } else {
    slot_h_offsets(s)[s.n] = s.bytes;
    HIPCHK(e, hipMemcpyAsync(s.d_meta, s.h_meta, (s.n + 1) * 8, hipMemcpyHostToDevice, p->copy_stream[0]));
    HIPCHK(e, hipMemcpyAsync(s.d_meta + (s.ent_cap + 1) * 8, slot_h_iss(s), s.n * 4, hipMemcpyHostToDevice, p->copy_stream[0]));
    HIPCHK(e, hipMemcpyAsync(s.d_meta + (s.ent_cap + 1) * 8 + s.ent_cap * 4, slot_h_et(s), s.n, hipMemcpyHostToDevice, p->copy_stream[0]));
  }
  for (uint32_t k = 0; k < p->n_streams; k++) HIPCHK(e, hipEventRecord(s.ev_h2d[k], p->copy_stream[k]));
  s.state = PS_QUEUED;
  p->queue.push_back((uint32_t)p->open);
  p->open = -1;
  p->cv.notify_all();
  return CTMR_OK;
}

int pipe_run_json(ctmr_engine* e, PipeSlot& s, ctmr_entry_view* view);  // engine/pipeline_json.inc
int pipe_run_pem(ctmr_engine* e, PipeSlot& s);                          // engine/pipeline_pem.inc

// The slot's blob holds `bytes` decoded bytes and the padding behind them (the text forms, sized by the worker).
int pipe_blob_reserve(ctmr_engine* e, PipeSlot& s, uint64_t bytes) {
  if (bytes + CTMR_PAYLOAD_PAD + 16 <= s.blob_cap) return CTMR_OK;
  (void)hipFree(s.d_blob);
  s.d_blob = nullptr;
  s.blob_cap = 0;
  const size_t cap = (size_t)pow2_at_least(bytes + CTMR_PAYLOAD_PAD + 16);
  if (hipMalloc(&s.d_blob, cap) != hipSuccess) {
    (void)hipGetLastError();
    s.d_blob = nullptr;
    return fail(e, CTMR_E_NOMEM, "no device memory for %llu decoded bytes", (unsigned long long)bytes);
  }
  s.blob_cap = cap;
  return CTMR_OK;
}

void pipe_worker(ctmr_engine* e) {
  ctmr_pipeline* p = e->pipe.load(std::memory_order_acquire);
  (void)hipSetDevice(e->device);
  for (;;) {
    uint32_t k;
    {
      std::unique_lock<std::mutex> lk(p->mu);
      p->cv.wait(lk, [&] { return p->stop || !p->queue.empty(); });
      if (p->queue.empty()) return;  // stop requested and nothing left to run
      k = p->queue.front();
      p->queue.pop_front();
    }
    PipeSlot& s = p->slots[k];
    int rc;
    std::string err;
    {
      std::lock_guard<std::mutex> eg(e->mu);  // the engine's scratch buffers and table belong to one batch at a time
      rc = CTMR_OK;
      for (uint32_t q = 0; q < p->n_streams; q++)
        if (hipStreamWaitEvent(e->stream, s.ev_h2d[q], 0) != hipSuccess) rc = CTMR_E_HIP;
      ctmr_entry_view view{};
      if (rc == CTMR_OK && s.form == PF_JSON)  // every body judged, the good ones decoded into s.d_blob, then as a raw super-batch
        rc = pipe_run_json(e, s, &view);
      else if (rc == CTMR_OK && s.form == PF_PEM)  // every file judged, the good ones decoded into s.d_blob, then as a packed super-batch
        rc = pipe_run_pem(e, s);
      else if (rc == CTMR_OK && s.form == PF_RAW)  // decode + Chain[0] match (issuers registered on the way) + map/reduce, as ctmr_map_entries_device
        rc = s.n ? map_entries_locked(e, s.d_payload, (const uint64_t*)s.d_meta, s.n, s.d_records, s.d_new, s.d_ts, &s.dstats,
                                      &s.stats, &view)
                 : CTMR_OK;
      else if (rc == CTMR_OK)
        rc = map_device_locked(e, s.d_payload, (const uint64_t*)s.d_meta, (const uint32_t*)(s.d_meta + (s.ent_cap + 1) * 8),
                               s.any_type ? s.d_meta + (s.ent_cap + 1) * 8 + s.ent_cap * 4 : nullptr, s.n, s.d_records, s.d_new,
                               &s.stats, nullptr, 0, s.bytes);
      if (rc == CTMR_OK) {
        hipError_t h = hipMemcpyAsync(s.h_records, s.d_records, s.n * sizeof(ctmr_record), hipMemcpyDeviceToHost, e->stream);
        if (h == hipSuccess && pipe_is_raw(s.form) && s.n) {
          h = hipMemcpyAsync(s.h_ts, s.d_ts, s.n * 8, hipMemcpyDeviceToHost, e->stream);
          if (h == hipSuccess) h = hipMemcpyAsync(s.h_etype, view.entry_type, s.n, hipMemcpyDeviceToHost, e->stream);
          if (h == hipSuccess) h = hipMemcpyAsync(s.h_c0len, view.chain0_len, s.n * 4, hipMemcpyDeviceToHost, e->stream);
        }
        if (h == hipSuccess && s.stats.n_new)
          h = hipMemcpyAsync(s.h_new, s.d_new, s.stats.n_new * 8, hipMemcpyDeviceToHost, e->stream);
        if (h == hipSuccess) h = hipStreamSynchronize(e->stream);
        if (h != hipSuccess) rc = fail(e, CTMR_E_HIP, "%s", hipGetErrorString(h));
      }
      if (rc != CTMR_OK) {
        std::lock_guard<std::mutex> eg2(e->err_mu);  // submitters may fail() concurrently under err_mu only
        err = e->err;
      }
    }
    {
      std::lock_guard<std::mutex> lk(p->mu);
      if (pipe_is_text(s.form) && rc == CTMR_OK)  // now the tickets' entries are known
        for (auto& t : s.tickets) {
          t.first = s.body_first[t.body0];
          t.n = s.body_first[t.body0 + t.nbody] - t.first;
        }
      s.rc = rc;
      s.err = err;
      s.state = PS_DONE;
    }
    p->cv.notify_all();
  }
}

int pipe_get(ctmr_engine* e, ctmr_pipeline** out) {
  ctmr_pipeline* p = e->pipe.load(std::memory_order_acquire);
  if (!p) {
    std::lock_guard<std::mutex> g(e->pipe_mu);  // not the engine mutex: the worker holds that one while a batch runs
    p = e->pipe.load(std::memory_order_acquire);
    if (!p) {
      HIPCHK(e, hipSetDevice(e->device));
      p = new ctmr_pipeline();
      if (const char* ns = getenv("CTMR_PIPE_STREAMS")) {
        const int v = atoi(ns);
        if (v >= 1 && v <= (int)PIPE_MAX_STREAMS) p->n_streams = (uint32_t)v;
      }
      for (uint32_t k = 0; k < p->n_streams; k++)
        if (hipStreamCreateWithFlags(&p->copy_stream[k], hipStreamNonBlocking) != hipSuccess) {
          delete p;
          return fail(e, CTMR_E_HIP, "pipeline: cannot create the copy streams");
        }
      e->pipe.store(p, std::memory_order_release);
      p->worker = std::thread(pipe_worker, e);
    }
  }
  *out = p;
  return CTMR_OK;
}

void pipe_shutdown(ctmr_engine* e) {
  ctmr_pipeline* p = e->pipe.load(std::memory_order_acquire);
  if (!p) return;
  {
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->open >= 0) (void)pipe_close_locked(e, p);  // nothing submitted is dropped silently: it runs, results are discarded
    p->stop = true;
  }
  p->cv.notify_all();
  if (p->worker.joinable()) p->worker.join();
  (void)hipSetDevice(e->device);
  for (auto& s : p->slots) {
    (void)hipFree(s.d_payload); (void)hipFree(s.d_meta); (void)hipFree(s.d_records); (void)hipFree(s.d_new); (void)hipFree(s.d_ts);
    (void)hipFree(s.d_blob);
    (void)hipHostFree(s.h_meta); (void)hipHostFree(s.h_records); (void)hipHostFree(s.h_new); (void)hipHostFree(s.h_ts);
    (void)hipHostFree(s.h_etype); (void)hipHostFree(s.h_c0len);
    for (auto ev : s.ev_h2d)
      if (ev) (void)hipEventDestroy(ev);
  }
  for (auto cs : p->copy_stream)
    if (cs) (void)hipStreamDestroy(cs);
  delete p;
  e->pipe.store(nullptr, std::memory_order_release);
}

}  // namespace
}  // extern "C++"

extern "C++" {
namespace {

// Make sure a super-batch of the wanted form is open and has room for n entries / `bytes` bytes (p->mu held through lk).
int pipe_open_for(ctmr_engine* e, ctmr_pipeline* p, std::unique_lock<std::mutex>& lk, PipeForm form, uint64_t n, uint64_t bytes) {
  int r;
  int k = -1;
  // Everything is decided again after every wait: while this submitter slept (the wait releases p->mu) another one may
  // have opened a super-batch — taking a second FREE slot then would orphan the first one in PS_OPEN for ever (nobody
  // closes a slot that is not p->open) and break the submission order across slots.
  for (;;) {
    if (p->open >= 0) {
      PipeSlot& s = p->slots[p->open];
      if (s.form != form || s.n + n > s.ent_cap || s.bytes + bytes + CTMR_PAYLOAD_PAD + 16 > s.payload_cap)
        if ((r = pipe_close_locked(e, p))) return r;
    }
    if (p->open >= 0) return CTMR_OK;
    for (uint32_t i = 0; i < PIPE_SLOTS; i++)
      if (p->slots[i].state == PS_FREE) { k = (int)i; break; }
    if (k >= 0) break;
    // every slot is in flight or holds results nobody has collected.  Results are only released by ctmr_wait: if no
    // slot is still running, waiting here could never end — the caller has to collect earlier tickets first.
    bool running = false;
    for (auto& s : p->slots) running = running || s.state == PS_QUEUED;
    if (!running)
      return fail(e, CTMR_E_RANGE, "ingestion pipeline full: %u super-batches hold uncollected results — ctmr_wait "
                  "for earlier tickets first", PIPE_SLOTS);
    p->cv.wait(lk);
  }
  PipeSlot& s = p->slots[k];
  if ((r = pipe_slot_reserve(e, s, n > 2 * PIPE_CLOSE_ENTRIES ? n : 2 * PIPE_CLOSE_ENTRIES,
                             bytes > 2 * PIPE_CLOSE_BYTES ? bytes : 2 * PIPE_CLOSE_BYTES))) return r;
  s.state = PS_OPEN;
  s.seq = p->next_seq++;
  s.n = s.bytes = 0;
  s.any_type = false;
  s.form = form;
  s.tickets.clear();
  s.body_rb.assign(1, 0);
  s.body_first.clear();
  s.body_bad.clear();
  s.file_iss.clear();
  s.rc = CTMR_OK;
  s.err.clear();
  memset(&s.stats, 0, sizeof s.stats);
  memset(&s.dstats, 0, sizeof s.dstats);
  p->open = k;
  return CTMR_OK;
}

// The batch's bytes follow the previous submit's; ticket; close when full.
int pipe_append(ctmr_engine* e, ctmr_pipeline* p, const uint8_t* src, uint64_t bytes, uint64_t n, ctmr_ticket* ticket) {
  PipeSlot& s = p->slots[p->open];
  if (bytes) {
    HIPCHK(e, hipMemcpyAsync(s.d_payload + s.bytes, src, bytes, hipMemcpyHostToDevice, p->copy_stream[p->rr]));
    p->rr = (p->rr + 1) % p->n_streams;
  }
  s.tickets.push_back({s.n, n, false});
  *ticket = (s.seq << 20) | (uint64_t)(s.tickets.size() - 1);  // ≤ 2^20 tickets per super-batch (it closes at 65 536 entries; empty batches: see below)
  s.n += n;
  s.bytes += bytes;
  if (s.n >= PIPE_CLOSE_ENTRIES || s.bytes >= PIPE_CLOSE_BYTES || s.tickets.size() >= (1u << 20) - 1 ||
      s.body_rb.size() > (s.form == PF_PEM ? PIPE_CLOSE_FILES : PIPE_CLOSE_BODIES))
    return pipe_close_locked(e, p);
  return CTMR_OK;
}

}  // namespace
}  // extern "C++"

int ctmr_submit_batch(ctmr_engine* e, const uint8_t* payload, const uint64_t* offsets, const uint32_t* issuer_idx,
                      const uint8_t* entry_type, uint64_t n, ctmr_ticket* ticket) {
  if (!e || !ticket || (n && (!payload || !offsets || !issuer_idx))) return CTMR_E_INVAL;
  for (uint64_t i = 0; i < n; i++)
    if (offsets[i + 1] < offsets[i]) return fail(e, CTMR_E_INVAL, "offsets not monotone at %llu", (unsigned long long)i);
  ctmr_pipeline* p;
  int r;
  if ((r = pipe_get(e, &p))) return r;
  const uint64_t base = n ? offsets[0] : 0, bytes = n ? offsets[n] - base : 0;
  if (n >= (1ull << 31)) return fail(e, CTMR_E_INVAL, "batch too large");
  std::unique_lock<std::mutex> lk(p->mu);
  HIPCHK(e, hipSetDevice(e->device));
  // (a batch larger than a whole slot gets a slot of its own, grown to fit)
  if ((r = pipe_open_for(e, p, lk, PF_PACKED, n, bytes))) return r;
  PipeSlot& s = p->slots[p->open];
  uint64_t* ho = slot_h_offsets(s) + s.n;
  for (uint64_t i = 0; i < n; i++) ho[i] = s.bytes + (offsets[i] - base);
  memcpy(slot_h_iss(s) + s.n, issuer_idx, n * 4);
  if (entry_type) { memcpy(slot_h_et(s) + s.n, entry_type, n); s.any_type = true; }
  else memset(slot_h_et(s) + s.n, 0, n);
  return pipe_append(e, p, payload + base, bytes, n, ticket);
}

int ctmr_submit_entries(ctmr_engine* e, const uint8_t* blob, const uint64_t* bounds, uint64_t n, ctmr_ticket* ticket) {
  if (!e || !ticket || (n && (!blob || !bounds))) return CTMR_E_INVAL;
  for (uint64_t i = 0; i < 2 * n; i++)
    if (bounds[i + 1] < bounds[i]) return fail(e, CTMR_E_INVAL, "bounds not monotone at %llu", (unsigned long long)i);
  ctmr_pipeline* p;
  int r;
  if ((r = pipe_get(e, &p))) return r;
  const uint64_t base = n ? bounds[0] : 0, bytes = n ? bounds[2 * n] - base : 0;
  if (n >= (1ull << 30)) return fail(e, CTMR_E_INVAL, "batch too large");
  std::unique_lock<std::mutex> lk(p->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if ((r = pipe_open_for(e, p, lk, PF_RAW, n, bytes))) return r;
  PipeSlot& s = p->slots[p->open];
  uint64_t* hb = slot_h_offsets(s) + 2 * s.n;  // bounds of the super-batch: this batch's, moved behind the bytes already there
  for (uint64_t i = 0; i < 2 * n; i++) hb[i] = s.bytes + (bounds[i] - base);
  return pipe_append(e, p, blob + base, bytes, n, ticket);
}

int ctmr_submit_entries_json(ctmr_engine* e, const uint8_t* text, const uint64_t* resp_bounds, uint64_t n_responses, ctmr_ticket* ticket) {
  if (!e || !ticket || (n_responses && !resp_bounds)) return CTMR_E_INVAL;
  for (uint64_t i = 0; i < n_responses; i++)
    if (resp_bounds[i + 1] < resp_bounds[i]) return fail(e, CTMR_E_INVAL, "resp_bounds not monotone at %llu", (unsigned long long)i);
  const uint64_t base = n_responses ? resp_bounds[0] : 0, bytes = n_responses ? resp_bounds[n_responses] - base : 0;
  if (bytes && !text) return fail(e, CTMR_E_INVAL, "null text");
  if (n_responses >= (1ull << 30)) return fail(e, CTMR_E_INVAL, "batch too large");
  ctmr_pipeline* p;
  int r;
  if ((r = pipe_get(e, &p))) return r;
  std::unique_lock<std::mutex> lk(p->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if ((r = pipe_open_for(e, p, lk, PF_JSON, 0, bytes))) return r;
  PipeSlot& s = p->slots[p->open];
  const uint64_t body0 = s.body_rb.size() - 1, at = s.bytes;
  try {
    for (uint64_t i = 1; i <= n_responses; i++) s.body_rb.push_back(at + (resp_bounds[i] - base));
  } catch (const std::bad_alloc&) {
    s.body_rb.resize(body0 + 1);
    return fail(e, CTMR_E_NOMEM, "no host memory for the bounds of %llu bodies", (unsigned long long)n_responses);
  }
  const size_t had = s.tickets.size();
  r = pipe_append(e, p, bytes ? text + base : nullptr, bytes, 0, ticket);
  if (s.tickets.size() == had) {  // the copy failed: no ticket, no bodies
    s.body_rb.resize(body0 + 1);
    return r;
  }
  PipeTicket& t = s.tickets[had];  // (p->mu is held: the worker has not seen the slot, closed or not)
  t.body0 = body0;
  t.nbody = n_responses;
  t.text_at = at;
  t.text_base = base;
  return r;
}

int ctmr_submit_pem(ctmr_engine* e, const uint8_t* text, const uint64_t* file_bounds, uint64_t n_files, const uint32_t* issuer_idx,
                    ctmr_ticket* ticket) {
  if (!e || !ticket || (n_files && (!file_bounds || !issuer_idx))) return CTMR_E_INVAL;
  for (uint64_t i = 0; i < n_files; i++)
    if (file_bounds[i + 1] < file_bounds[i]) return fail(e, CTMR_E_INVAL, "file_bounds not monotone at %llu", (unsigned long long)i);
  const uint64_t base = n_files ? file_bounds[0] : 0, bytes = n_files ? file_bounds[n_files] - base : 0;
  if (bytes && !text) return fail(e, CTMR_E_INVAL, "null text");
  if (n_files >= (1ull << 30)) return fail(e, CTMR_E_INVAL, "batch too large");
  ctmr_pipeline* p;
  int r;
  if ((r = pipe_get(e, &p))) return r;
  std::unique_lock<std::mutex> lk(p->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if ((r = pipe_open_for(e, p, lk, PF_PEM, 0, bytes))) return r;
  PipeSlot& s = p->slots[p->open];
  const uint64_t body0 = s.body_rb.size() - 1, at = s.bytes;
  try {
    for (uint64_t i = 1; i <= n_files; i++) s.body_rb.push_back(at + (file_bounds[i] - base));
    s.file_iss.insert(s.file_iss.end(), issuer_idx, issuer_idx + n_files);
  } catch (const std::bad_alloc&) {
    s.body_rb.resize(body0 + 1);
    s.file_iss.resize(body0);
    return fail(e, CTMR_E_NOMEM, "no host memory for the bounds of %llu files", (unsigned long long)n_files);
  }
  const size_t had = s.tickets.size();
  r = pipe_append(e, p, bytes ? text + base : nullptr, bytes, 0, ticket);
  if (s.tickets.size() == had) {  // the copy failed: no ticket, no files
    s.body_rb.resize(body0 + 1);
    s.file_iss.resize(body0);
    return r;
  }
  PipeTicket& t = s.tickets[had];  // (p->mu is held: the worker has not seen the slot, closed or not)
  t.body0 = body0;
  t.nbody = n_files;
  t.text_at = at;
  t.text_base = base;
  return r;
}

int ctmr_flush(ctmr_engine* e) {
  if (!e) return CTMR_E_INVAL;
  ctmr_pipeline* p;
  int r;
  if ((r = pipe_get(e, &p))) return r;
  std::lock_guard<std::mutex> lk(p->mu);
  return pipe_close_locked(e, p);
}

// What ctmr_wait_entries_json and ctmr_wait_pem have beyond the others: each alone collects a ticket of its text form (the
// others have no capacity argument) and collects no other.  first / bad: resp_first / resp_bad, or file_first / file_bad.
struct PipeTextWait {
  PipeForm form;
  uint64_t cap;
  uint64_t *first, *bad;
  ctmr_entries_json_info* jinfo;
  ctmr_pem_decode_info* pinfo;
};

static int pipe_wait(ctmr_engine* e, ctmr_ticket ticket, ctmr_record* records, uint64_t* new_idx, uint64_t* timestamp,
                     ctmr_decode_stats* dstats, ctmr_batch_stats* stats, const PipeTextWait* tw = nullptr) {
  if (!e) return CTMR_E_INVAL;
  ctmr_pipeline* p;
  int r;
  if ((r = pipe_get(e, &p))) return r;
  const uint64_t seq = ticket >> 20, tix = ticket & ((1u << 20) - 1);
  std::unique_lock<std::mutex> lk(p->mu);
  PipeSlot* s = nullptr;
  for (auto& c : p->slots)
    if (c.state != PS_FREE && c.seq == seq) s = &c;
  if (!s || tix >= s->tickets.size() || s->tickets[tix].consumed)
    return fail(e, CTMR_E_NOTFOUND, "unknown or already collected ticket");
  if (pipe_is_text(s->form) ? (!tw || tw->form != s->form) : tw != nullptr)  // (the ticket stays collectable)
    return fail(e, CTMR_E_INVAL, s->form == PF_JSON  ? "a ticket of ctmr_submit_entries_json: ctmr_wait_entries_json collects it"
                                 : s->form == PF_PEM ? "a ticket of ctmr_submit_pem: ctmr_wait_pem collects it"
                                 : tw->form == PF_PEM ? "not a ticket of ctmr_submit_pem"
                                                      : "not a ticket of ctmr_submit_entries_json");
  const bool json = tw && tw->form == PF_JSON, pem = tw && tw->form == PF_PEM;
  ctmr_entries_json_info* const info = tw ? tw->jinfo : nullptr;
  ctmr_pem_decode_info* const pinfo = tw ? tw->pinfo : nullptr;
  if (s->state == PS_OPEN && (r = pipe_close_locked(e, p))) return r;  // nobody else will launch it
  p->cv.wait(lk, [&] { return s->state == PS_DONE; });
  PipeTicket& t = s->tickets[tix];
  int rc = s->rc;
  if (rc != CTMR_OK && json && info) {  // the super-batch failed: no body was judged
    memset(info, 0, sizeof *info);
    info->responses = t.nbody;
    info->bad_response = info->bad_offset = ~0ull;
  }
  if (rc != CTMR_OK && pem && pinfo) {  // the super-batch failed: no file was judged
    memset(pinfo, 0, sizeof *pinfo);
    pinfo->files = t.nbody;
    pinfo->bad_file = pinfo->bad_offset = ~0ull;
  }
  if (rc == CTMR_OK && tw) {
    const uint64_t* rb = s->body_rb.data() + t.body0;
    const uint64_t* bad = s->body_bad.data() + t.body0;
    const uint64_t back = t.text_base - t.text_at;  // an offset in the slot's text → one from the submit's text pointer
    if (json && info) {
      memset(info, 0, sizeof *info);
      info->responses = t.nbody;
      info->entries = t.n;
      info->text_bytes = rb[t.nbody] - rb[0];
      info->blob_bytes = slot_h_offsets(*s)[2 * (t.first + t.n)] - slot_h_offsets(*s)[2 * t.first];
      info->bad_response = info->bad_offset = ~0ull;
      for (uint64_t i = t.nbody; i-- > 0;)
        if (bad[i] != ~0ull) {
          info->bad_response = i;
          info->bad_offset = bad[i] + back;
        }
    }
    if (pem && pinfo) {
      memset(pinfo, 0, sizeof *pinfo);
      pinfo->files = t.nbody;
      pinfo->certificates = t.n;
      pinfo->text_bytes = rb[t.nbody] - rb[0];
      pinfo->payload_bytes = slot_h_offsets(*s)[t.first + t.n] - slot_h_offsets(*s)[t.first];
      for (uint64_t i = 0; i < t.n; i++) pinfo->irregular += (s->cert_lay[t.first + i] & 3ull) == PD_IRREGULAR;
      pinfo->regular = t.n - pinfo->irregular;
      pinfo->bad_file = pinfo->bad_offset = ~0ull;
      for (uint64_t i = t.nbody; i-- > 0;)
        if (bad[i] != ~0ull) {
          pinfo->bad_file = i;
          pinfo->bad_offset = bad[i] + back;
        }
    }
    if (tw->cap < t.n)
      return fail(e, CTMR_E_RANGE, "the ticket holds %llu %s", (unsigned long long)t.n, pem ? "certificates" : "entries");
    if (tw->first)
      for (uint64_t i = 0; i <= t.nbody; i++) tw->first[i] = s->body_first[t.body0 + i] - t.first;
    if (tw->bad)
      for (uint64_t i = 0; i < t.nbody; i++) tw->bad[i] = bad[i] == ~0ull ? ~0ull : bad[i] + back;
  }
  if (rc == CTMR_OK) {
    if (records && t.n) memcpy(records, s->h_records + t.first, t.n * sizeof(ctmr_record));
    // this batch's slice of the super-batch's NEW list (ascending), rebased to the batch
    const uint64_t* nb = s->h_new;
    const uint64_t* lo = std::lower_bound(nb, nb + s->stats.n_new, t.first);
    const uint64_t* hi = std::lower_bound(lo, nb + s->stats.n_new, t.first + t.n);
    if (new_idx)
      for (const uint64_t* q = lo; q < hi; q++) new_idx[q - lo] = *q - t.first;
    if (stats) {
      memset(stats, 0, sizeof *stats);
      stats->n = t.n;
      uint64_t host_set = 0, new_flag = 0;
      for (uint64_t i = 0; i < t.n; i++) {
        const ctmr_record& rc2 = s->h_records[t.first + i];
        stats->by_status[rc2.status < CTMR_ST__COUNT ? rc2.status : CTMR_ST_PARSE_ERROR]++;
        host_set += rc2.status == CTMR_ST_PASS && rc2.serial_len > CTMR_MAX_SERIAL;
        new_flag += (rc2.flags & CTMR_FL_WAS_UNKNOWN) != 0;
      }
      stats->n_new = (uint64_t)(hi - lo);
      stats->n_dup = stats->by_status[CTMR_ST_PASS] - stats->n_new;
      stats->n_host_set = host_set;
      stats->payload_bytes = pipe_is_raw(s->form) ? slot_h_offsets(*s)[2 * (t.first + t.n)] - slot_h_offsets(*s)[2 * t.first]
                                    : slot_h_offsets(*s)[t.first + t.n] - slot_h_offsets(*s)[t.first];
      stats->map_launches = 1;
      stats->ms_map = s->stats.ms_map; stats->ms_insert = s->stats.ms_insert; stats->ms_resolve = s->stats.ms_resolve;
      stats->ms_compact = s->stats.ms_compact; stats->ms_total = s->stats.ms_total;  // of the whole super-batch
      (void)new_flag;
    }
    if (timestamp) {
      if (pipe_is_raw(s->form)) memcpy(timestamp, s->h_ts + t.first, t.n * 8);
      else memset(timestamp, 0, t.n * 8);  // a packed batch carries no timestamps
    }
    if (dstats) {
      memset(dstats, 0, sizeof *dstats);
      if (pipe_is_raw(s->form)) {
        dstats->n = t.n;
        for (uint64_t i = 0; i < t.n; i++) {
          const uint8_t et = s->h_etype[t.first + i];
          dstats->n_x509 += et == 0;
          dstats->n_precert += et == 1;
          dstats->n_decode_error += et == CTMR_ENTRY_INVALID;
          dstats->n_no_chain += et != CTMR_ENTRY_INVALID && s->h_c0len[t.first + i] == 0;
        }
        dstats->blob_bytes = slot_h_offsets(*s)[2 * (t.first + t.n)] - slot_h_offsets(*s)[2 * t.first];
        dstats->n_issuers_added = s->dstats.n_issuers_added;  // of the whole super-batch
        dstats->ms_decode = s->dstats.ms_decode; dstats->ms_match = s->dstats.ms_match;
      }
    }
  } else {
    (void)fail(e, rc, "%s", s->err.c_str());
  }
  t.consumed = true;
  bool all = true;
  for (auto& q : s->tickets) all = all && q.consumed;
  if (all) {
    s->state = PS_FREE;
    p->cv.notify_all();
  }
  return rc;
}

int ctmr_wait(ctmr_engine* e, ctmr_ticket ticket, ctmr_record* records, uint64_t* new_idx, ctmr_batch_stats* stats) {
  return pipe_wait(e, ticket, records, new_idx, nullptr, nullptr, stats);
}

int ctmr_wait_entries(ctmr_engine* e, ctmr_ticket ticket, ctmr_record* records, uint64_t* new_idx, uint64_t* timestamp,
                      ctmr_decode_stats* dstats, ctmr_batch_stats* stats) {
  return pipe_wait(e, ticket, records, new_idx, timestamp, dstats, stats);
}

int ctmr_wait_entries_json(ctmr_engine* e, ctmr_ticket ticket, uint64_t entries_cap, ctmr_record* records, uint64_t* new_idx, uint64_t* timestamp,
                           uint64_t* resp_first, uint64_t* resp_bad, ctmr_entries_json_info* info, ctmr_decode_stats* dstats,
                           ctmr_batch_stats* stats) {
  const PipeTextWait tw{PF_JSON, entries_cap, resp_first, resp_bad, info, nullptr};
  return pipe_wait(e, ticket, records, new_idx, timestamp, dstats, stats, &tw);
}

int ctmr_wait_pem(ctmr_engine* e, ctmr_ticket ticket, uint64_t certs_cap, ctmr_record* records, uint64_t* new_idx, uint64_t* file_first,
                  uint64_t* file_bad, ctmr_pem_decode_info* info, ctmr_batch_stats* stats) {
  const PipeTextWait tw{PF_PEM, certs_cap, file_first, file_bad, nullptr, info};
  return pipe_wait(e, ticket, records, new_idx, nullptr, nullptr, stats, &tw);
}
