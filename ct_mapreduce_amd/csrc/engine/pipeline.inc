// engine/pipeline.inc — asynchronous host ingestion: ctmr_submit_batch / ctmr_wait / ctmr_flush, the raw-entry and
// get-entries JSON forms of both (ctmr_submit_entries*, ctmr_wait_entries*) and the PEM form (ctmr_submit_pem, ctmr_wait_pem).
// Part of ctmr_engine.hip (one translation unit): included inside its extern "C" block, after engine/map.inc; the
// worker's step for the JSON form is engine/pipeline_json.inc, behind engine/entries_json.inc, and the one for the PEM
// form engine/pipeline_pem.inc, behind engine/pem_decode.inc.
// What the four forms share stands once: a slot owns its buffers (DevMem, PinMem), the layout of a meta buffer and the decoded
// bytes of a ticket have one spelling each (slot_iss, slot_et, slot_ticket_bytes), the worker runs a pipe_run_* of one
// signature per form, and the two text forms have one submit (pipe_submit_text), one opening of their worker steps
// (pipe_text_reserve) and one account of a ticket's bodies (PipeTextWait::info), put into either public struct.
// The back of the pipeline — PEM and first sightings of what a super-batch found new, per ticket (ctmr_set_pipeline_writeback,
// ctmr_ticket_writeback) — is engine/pipeline_writeback.inc, behind engine/meta.inc and engine/pem.inc.
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
  // device side (the slot owns its buffers: freed with it, pipe_shutdown)
  DevMem d_payload; size_t payload_cap = 0;
  DevMem d_meta;                                        // offsets u64[cap+1] | issuer_idx u32[cap] | entry_type u8[cap] — or, raw: bounds u64[2cap+1]
  DevMem d_records;                                     // ctmr_record[cap]
  DevMem d_new;                                         // u64[cap]
  uint64_t ent_cap = 0;
  // pinned host side
  PinMem h_meta;                                        // same layout as d_meta
  PinMem h_records;
  PinMem h_new;
  DevMem d_ts;                                          // raw super-batches: TimestampedEntry.Timestamp per entry, u64[cap]
  PinMem h_ts;
  PinMem h_etype;                                       // raw super-batches: the decoded entry types u8[cap] and Chain[0] lengths
  PinMem h_c0len;                                       //   u32[cap] (per-ticket decode stats)
  // fill state
  uint64_t n = 0, bytes = 0;
  bool any_type = false;
  PipeForm form = PF_PACKED;
  // JSON and PEM super-batches: d_payload holds the text.  The bodies' bounds in it live here, not in the meta buffers, which
  // pipe_slot_reserve replaces when the worker sizes the slot by the entries found.
  std::vector<uint64_t> body_rb;                        // bodies + 1
  std::vector<uint64_t> body_first, body_bad;           // the worker's: each body's first entry (bodies + 1), its verdict
  DevMem d_blob; size_t blob_cap = 0;                   // the decoded entries; h_meta: their bounds u64[2n+1] (PEM: offsets u64[n+1])
  std::vector<uint32_t> file_iss;                       // PEM: the issuer index of every file
  std::vector<uint64_t> cert_lay;                       // PEM, the worker's: the layout of every certificate (a ticket's regular / irregular)
  ctmr_decode_stats dstats{};
  std::vector<PipeTicket> tickets;
  // write-back (engine/pipeline_writeback.inc): CTMR_WB_* as they stood when the super-batch was opened, and what the worker
  // left for its tickets.  Pinned, grown by need, allocated only when a flag is on.
  uint32_t wb = 0;
  PinMem h_pem; size_t h_pem_cap = 0;                   // the PEM blocks of the NEW list, back to back
  PinMem h_pemoff; size_t h_pemoff_cap = 0;             // u64[n_new + 1]
  PinMem h_items; size_t h_items_cap = 0;               // ctmr_meta_item[wb_items]: by new entry, (kind, off) inside, entry from its ticket's first
  PinMem h_istart; size_t h_istart_cap = 0;             // u64[n_new + 1]: where each new entry's items begin
  PinMem h_iboff; size_t h_iboff_cap = 0;               // u64[wb_items + 1]: where each item's bytes begin
  PinMem h_ibytes; size_t h_ibytes_cap = 0;             // the items' bytes, back to back in item order
  uint64_t wb_pem_bytes = 0, wb_items = 0, wb_item_bytes = 0;
  std::vector<uint64_t> wb_tfirst;                      // the tickets' first entries and the slot's n: the item passes rebase by it
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
    s.ent_cap = 0;  // (until all ten stand)
    HIPCHK(e, s.d_meta.alloc(pipe_meta_bytes(cap)));
    HIPCHK(e, s.d_records.alloc(cap * sizeof(ctmr_record)));
    HIPCHK(e, s.d_new.alloc(cap * 8));
    HIPCHK(e, s.h_meta.alloc(pipe_meta_bytes(cap)));
    HIPCHK(e, s.h_records.alloc(cap * sizeof(ctmr_record)));
    HIPCHK(e, s.h_new.alloc(cap * 8));
    HIPCHK(e, s.d_ts.alloc(cap * 8));
    HIPCHK(e, s.h_ts.alloc(cap * 8));
    HIPCHK(e, s.h_etype.alloc(cap));
    HIPCHK(e, s.h_c0len.alloc(cap * 4));
    s.ent_cap = cap;
  }
  if (bytes + CTMR_PAYLOAD_PAD + 16 > s.payload_cap) {
    size_t cap = s.payload_cap ? s.payload_cap : 2 * PIPE_CLOSE_BYTES;
    while (cap < bytes + CTMR_PAYLOAD_PAD + 16) cap *= 2;
    s.payload_cap = 0;
    HIPCHK(e, s.d_payload.alloc(cap));
    s.payload_cap = cap;
  }
  return CTMR_OK;
}

uint64_t* slot_h_offsets(const PipeSlot& s) { return (uint64_t*)s.h_meta.p; }
// The packed layout of a meta buffer: where the issuer indices and the entry types lie behind `meta` (h_meta's or d_meta's bytes).
uint32_t* slot_iss(const PipeSlot& s, uint8_t* meta) { return (uint32_t*)(meta + (s.ent_cap + 1) * 8); }
uint8_t* slot_et(const PipeSlot& s, uint8_t* meta) { return (uint8_t*)(slot_iss(s, meta) + s.ent_cap); }
// The decoded bytes of a ticket (its DER, or its leaf_input and extra_data: the raw forms keep two bounds an entry).
uint64_t slot_ticket_bytes(const PipeSlot& s, const PipeTicket& t) {
  const uint64_t per = pipe_is_raw(s.form) ? 2 : 1;
  return slot_h_offsets(s)[per * (t.first + t.n)] - slot_h_offsets(s)[per * t.first];
}

// Close the open super-batch: its small arrays follow the DER on the copy stream; the worker takes it from the queue.
int pipe_close_locked(ctmr_engine* e, ctmr_pipeline* p) {
  if (p->open < 0) return CTMR_OK;
  PipeSlot& s = p->slots[p->open];
  HIPCHK(e, hipSetDevice(e->device));
  // (the text forms copy nothing here: the bodies' bounds go to the device with the worker's call)
  if (s.form == PF_RAW) {
    slot_h_offsets(s)[2 * s.n] = s.bytes;
    HIPCHK(e, hipMemcpyAsync(s.d_meta.p, s.h_meta.p, (2 * s.n + 1) * 8, hipMemcpyHostToDevice, p->copy_stream[0]));
  } else if (s.form == PF_PACKED) {
    slot_h_offsets(s)[s.n] = s.bytes;
    HIPCHK(e, hipMemcpyAsync(s.d_meta.p, s.h_meta.p, (s.n + 1) * 8, hipMemcpyHostToDevice, p->copy_stream[0]));
    HIPCHK(e, hipMemcpyAsync(slot_iss(s, s.d_meta.u8()), slot_iss(s, s.h_meta.u8()), s.n * 4, hipMemcpyHostToDevice, p->copy_stream[0]));
    HIPCHK(e, hipMemcpyAsync(slot_et(s, s.d_meta.u8()), slot_et(s, s.h_meta.u8()), s.n, hipMemcpyHostToDevice, p->copy_stream[0]));
  }
  for (uint32_t k = 0; k < p->n_streams; k++) HIPCHK(e, hipEventRecord(s.ev_h2d[k], p->copy_stream[k]));
  s.state = PS_QUEUED;
  p->queue.push_back((uint32_t)p->open);
  p->open = -1;
  p->cv.notify_all();
  return CTMR_OK;
}

// The worker's step for each form, the engine's mutex held and the slot's bytes on their way (pipe_worker).  view: what the
// raw forms' decode leaves on the device, for the tickets' decode stats.
int pipe_run_json(ctmr_engine* e, PipeSlot& s, ctmr_entry_view* view);  // engine/pipeline_json.inc
int pipe_run_pem(ctmr_engine* e, PipeSlot& s, ctmr_entry_view* view);   // engine/pipeline_pem.inc
// … and behind whichever ran, when the super-batch asks for it (s.wb): PEM and first sightings of its NEW list
int pipe_writeback_run(ctmr_engine* e, PipeSlot& s, const ctmr_entry_view& view);  // engine/pipeline_writeback.inc

// The map + reduce over s.n certificates at `der` (s.d_payload, or what the PEM step decoded), their offsets in s.d_meta.
int pipe_map_packed(ctmr_engine* e, PipeSlot& s, const uint8_t* der, const uint8_t* entry_type, uint64_t bytes) {
  return map_device_locked(e, der, (const uint64_t*)s.d_meta.p, slot_iss(s, s.d_meta.u8()), entry_type, s.n, (ctmr_record*)s.d_records.p,
                           (uint64_t*)s.d_new.p, &s.stats, nullptr, 0, bytes);
}
int pipe_run_packed(ctmr_engine* e, PipeSlot& s, ctmr_entry_view*) {
  return pipe_map_packed(e, s, s.d_payload.u8(), s.any_type ? slot_et(s, s.d_meta.u8()) : nullptr, s.bytes);
}

// Decode + Chain[0] match (issuers registered on the way) + map/reduce, as ctmr_map_entries_device, over s.n raw entries at
// `blob` (s.d_payload, or what the JSON step decoded), their bounds in s.d_meta.
int pipe_map_raw(ctmr_engine* e, PipeSlot& s, const uint8_t* blob, ctmr_entry_view* view) {
  return map_entries_locked(e, blob, (const uint64_t*)s.d_meta.p, s.n, (ctmr_record*)s.d_records.p, (uint64_t*)s.d_new.p, (uint64_t*)s.d_ts.p,
                            &s.dstats, &s.stats, view);
}
int pipe_run_raw(ctmr_engine* e, PipeSlot& s, ctmr_entry_view* view) { return s.n ? pipe_map_raw(e, s, s.d_payload.u8(), view) : CTMR_OK; }

// The slot's blob holds `bytes` decoded bytes and the padding behind them (the text forms, sized by the worker).
int pipe_blob_reserve(ctmr_engine* e, PipeSlot& s, uint64_t bytes) {
  if (bytes + CTMR_PAYLOAD_PAD + 16 <= s.blob_cap) return CTMR_OK;
  s.blob_cap = 0;
  const size_t cap = (size_t)pow2_at_least(bytes + CTMR_PAYLOAD_PAD + 16);
  if (s.d_blob.alloc(cap) != hipSuccess) return fail(e, CTMR_E_NOMEM, "no device memory for %llu decoded bytes", (unsigned long long)bytes);
  s.blob_cap = cap;
  return CTMR_OK;
}

// The opening of the two text steps, once the decoder's core has judged the slot's bodies and found n items of `bytes`
// decoded bytes in the good ones: room for every body's verdict and first item, and everything sized by items, the blob
// among it (at most 3/4 of the text).  pipe_slot_reserve replaces the meta buffers when it grows them; the bodies' bounds
// (and the files' issuers) are in s.body_rb (s.file_iss), not there.
int pipe_text_reserve(ctmr_engine* e, PipeSlot& s, uint64_t n, uint64_t bytes) {
  const uint64_t B = s.body_rb.size() - 1;
  int r;
  try {
    s.body_bad.assign(B, ~0ull);
    s.body_first.assign(B + 1, 0);
    s.cert_lay.assign(s.form == PF_PEM ? n : 0, 0);
  } catch (const std::bad_alloc&) {
    return fail(e, CTMR_E_NOMEM, "no host memory for the verdicts of %llu %s", (unsigned long long)B, s.form == PF_PEM ? "files" : "bodies");
  }
  if ((r = pipe_slot_reserve(e, s, n, 0))) return r;
  return pipe_blob_reserve(e, s, bytes);
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
      if (rc == CTMR_OK) {
        switch (s.form) {
          case PF_PACKED: rc = pipe_run_packed(e, s, &view); break;
          case PF_RAW: rc = pipe_run_raw(e, s, &view); break;
          case PF_JSON: rc = pipe_run_json(e, s, &view); break;  // every body judged, the good ones decoded into s.d_blob, then as a raw super-batch
          case PF_PEM: rc = pipe_run_pem(e, s, &view); break;    // every file judged, the good ones decoded into s.d_blob, then as a packed one
        }
      }
      if (rc == CTMR_OK) {
        hipError_t h = hipMemcpyAsync(s.h_records.p, s.d_records.p, s.n * sizeof(ctmr_record), hipMemcpyDeviceToHost, e->stream);
        if (h == hipSuccess && pipe_is_raw(s.form) && s.n) {
          h = hipMemcpyAsync(s.h_ts.p, s.d_ts.p, s.n * 8, hipMemcpyDeviceToHost, e->stream);
          if (h == hipSuccess) h = hipMemcpyAsync(s.h_etype.p, view.entry_type, s.n, hipMemcpyDeviceToHost, e->stream);
          if (h == hipSuccess) h = hipMemcpyAsync(s.h_c0len.p, view.chain0_len, s.n * 4, hipMemcpyDeviceToHost, e->stream);
        }
        if (h == hipSuccess && s.stats.n_new)
          h = hipMemcpyAsync(s.h_new.p, s.d_new.p, s.stats.n_new * 8, hipMemcpyDeviceToHost, e->stream);
        if (h == hipSuccess) h = hipStreamSynchronize(e->stream);
        if (h != hipSuccess) rc = fail(e, CTMR_E_HIP, "%s", hipGetErrorString(h));
      }
      if (rc == CTMR_OK && s.wb) rc = pipe_writeback_run(e, s, view);
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
  for (auto& s : p->slots)
    for (auto ev : s.ev_h2d)
      if (ev) (void)hipEventDestroy(ev);
  for (auto cs : p->copy_stream)
    if (cs) (void)hipStreamDestroy(cs);
  delete p;  // (the slots free their buffers)
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
  s.wb = e->pipe_wb.load(std::memory_order_relaxed);
  s.wb_pem_bytes = s.wb_items = s.wb_item_bytes = 0;
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
    HIPCHK(e, hipMemcpyAsync(s.d_payload.u8() + s.bytes, src, bytes, hipMemcpyHostToDevice, p->copy_stream[p->rr]));
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
  memcpy(slot_iss(s, s.h_meta.u8()) + s.n, issuer_idx, n * 4);
  if (entry_type) { memcpy(slot_et(s, s.h_meta.u8()) + s.n, entry_type, n); s.any_type = true; }
  else memset(slot_et(s, s.h_meta.u8()) + s.n, 0, n);
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

// The submit of the two text forms: n bodies at text[bounds[i], bounds[i + 1]), and for PEM the issuer index of each.
static int pipe_submit_text(ctmr_engine* e, PipeForm form, const uint8_t* text, const uint64_t* bounds, uint64_t n,
                            const uint32_t* issuer_idx /* PEM only */, ctmr_ticket* ticket) {
  const bool pem = form == PF_PEM;
  for (uint64_t i = 0; i < n; i++)
    if (bounds[i + 1] < bounds[i])
      return fail(e, CTMR_E_INVAL, "%s not monotone at %llu", pem ? "file_bounds" : "resp_bounds", (unsigned long long)i);
  const uint64_t base = n ? bounds[0] : 0, bytes = n ? bounds[n] - base : 0;
  if (bytes && !text) return fail(e, CTMR_E_INVAL, "null text");
  if (n >= (1ull << 30)) return fail(e, CTMR_E_INVAL, "batch too large");
  ctmr_pipeline* p;
  int r;
  if ((r = pipe_get(e, &p))) return r;
  std::unique_lock<std::mutex> lk(p->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if ((r = pipe_open_for(e, p, lk, form, 0, bytes))) return r;
  PipeSlot& s = p->slots[p->open];
  const uint64_t body0 = s.body_rb.size() - 1, at = s.bytes;
  const auto undo = [&] {  // no ticket, no bodies
    s.body_rb.resize(body0 + 1);
    if (pem) s.file_iss.resize(body0);
  };
  try {
    for (uint64_t i = 1; i <= n; i++) s.body_rb.push_back(at + (bounds[i] - base));
    if (pem) s.file_iss.insert(s.file_iss.end(), issuer_idx, issuer_idx + n);
  } catch (const std::bad_alloc&) {
    undo();
    return fail(e, CTMR_E_NOMEM, "no host memory for the bounds of %llu %s", (unsigned long long)n, pem ? "files" : "bodies");
  }
  const size_t had = s.tickets.size();
  r = pipe_append(e, p, bytes ? text + base : nullptr, bytes, 0, ticket);
  if (s.tickets.size() == had) {  // the copy failed
    undo();
    return r;
  }
  PipeTicket& t = s.tickets[had];  // (p->mu is held: the worker has not seen the slot, closed or not)
  t.body0 = body0;
  t.nbody = n;
  t.text_at = at;
  t.text_base = base;
  return r;
}

int ctmr_submit_entries_json(ctmr_engine* e, const uint8_t* text, const uint64_t* resp_bounds, uint64_t n_responses, ctmr_ticket* ticket) {
  if (!e || !ticket || (n_responses && !resp_bounds)) return CTMR_E_INVAL;
  return pipe_submit_text(e, PF_JSON, text, resp_bounds, n_responses, nullptr, ticket);
}

int ctmr_submit_pem(ctmr_engine* e, const uint8_t* text, const uint64_t* file_bounds, uint64_t n_files, const uint32_t* issuer_idx,
                    ctmr_ticket* ticket) {
  if (!e || !ticket || (n_files && (!file_bounds || !issuer_idx))) return CTMR_E_INVAL;
  return pipe_submit_text(e, PF_PEM, text, file_bounds, n_files, issuer_idx, ticket);
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
// info: what the ticket's bodies (responses, files) came to, in neither call's names; each puts it into its public struct
// when `judged` says it was filled — not for an unknown ticket or one of another form, which stays collectable.
struct PipeTextWait {
  PipeForm form;
  uint64_t cap;
  uint64_t *first, *bad;
  bool judged = false;
  struct {
    uint64_t bodies, items, text_bytes, decoded_bytes;
    uint64_t bad_body, bad_offset;  // the lowest body outside the grammar, or ~0
    uint64_t irregular;             // PEM: the items decoded through the squeezed copy
  } info{};
};

static int pipe_wait(ctmr_engine* e, ctmr_ticket ticket, ctmr_record* records, uint64_t* new_idx, uint64_t* timestamp,
                     ctmr_decode_stats* dstats, ctmr_batch_stats* stats, PipeTextWait* tw = nullptr) {
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
  if (s->state == PS_OPEN && (r = pipe_close_locked(e, p))) return r;  // nobody else will launch it
  p->cv.wait(lk, [&] { return s->state == PS_DONE; });
  PipeTicket& t = s->tickets[tix];
  int rc = s->rc;
  if (tw) {
    tw->judged = true;
    tw->info = {t.nbody, 0, 0, 0, ~0ull, ~0ull, 0};  // should the super-batch have failed: no body was judged
  }
  if (rc == CTMR_OK && tw) {
    const uint64_t* rb = s->body_rb.data() + t.body0;
    const uint64_t* bad = s->body_bad.data() + t.body0;
    const uint64_t back = t.text_base - t.text_at;  // an offset in the slot's text → one from the submit's text pointer
    tw->info.items = t.n;
    tw->info.text_bytes = rb[t.nbody] - rb[0];
    tw->info.decoded_bytes = slot_ticket_bytes(*s, t);
    for (uint64_t i = t.nbody; i-- > 0;)
      if (bad[i] != ~0ull) {
        tw->info.bad_body = i;
        tw->info.bad_offset = bad[i] + back;
      }
    if (s->form == PF_PEM)
      for (uint64_t i = 0; i < t.n; i++) tw->info.irregular += (s->cert_lay[t.first + i] & 3ull) == PD_IRREGULAR;
    if (tw->cap < t.n)
      return fail(e, CTMR_E_RANGE, "the ticket holds %llu %s", (unsigned long long)t.n, s->form == PF_PEM ? "certificates" : "entries");
    if (tw->first)
      for (uint64_t i = 0; i <= t.nbody; i++) tw->first[i] = s->body_first[t.body0 + i] - t.first;
    if (tw->bad)
      for (uint64_t i = 0; i < t.nbody; i++) tw->bad[i] = bad[i] == ~0ull ? ~0ull : bad[i] + back;
  }
  if (rc == CTMR_OK) {
    const ctmr_record* recs = (const ctmr_record*)s->h_records.p + t.first;
    if (records && t.n) memcpy(records, recs, t.n * sizeof(ctmr_record));
    // this batch's slice of the super-batch's NEW list (ascending), rebased to the batch
    const uint64_t* nb = (const uint64_t*)s->h_new.p;
    const uint64_t* lo = std::lower_bound(nb, nb + s->stats.n_new, t.first);
    const uint64_t* hi = std::lower_bound(lo, nb + s->stats.n_new, t.first + t.n);
    if (new_idx)
      for (const uint64_t* q = lo; q < hi; q++) new_idx[q - lo] = *q - t.first;
    if (stats) {
      memset(stats, 0, sizeof *stats);
      stats->n = t.n;
      uint64_t host_set = 0;
      for (uint64_t i = 0; i < t.n; i++) {
        const ctmr_record& rc2 = recs[i];
        stats->by_status[rc2.status < CTMR_ST__COUNT ? rc2.status : CTMR_ST_PARSE_ERROR]++;
        host_set += rc2.status == CTMR_ST_PASS && rc2.serial_len > CTMR_MAX_SERIAL;
      }
      stats->n_new = (uint64_t)(hi - lo);
      stats->n_dup = stats->by_status[CTMR_ST_PASS] - stats->n_new;
      stats->n_host_set = host_set;
      stats->payload_bytes = slot_ticket_bytes(*s, t);
      stats->map_launches = 1;
      stats->ms_map = s->stats.ms_map; stats->ms_insert = s->stats.ms_insert; stats->ms_resolve = s->stats.ms_resolve;
      stats->ms_compact = s->stats.ms_compact; stats->ms_total = s->stats.ms_total;  // of the whole super-batch
    }
    if (timestamp) {
      if (pipe_is_raw(s->form)) memcpy(timestamp, (const uint64_t*)s->h_ts.p + t.first, t.n * 8);
      else memset(timestamp, 0, t.n * 8);  // a packed batch carries no timestamps
    }
    if (dstats) {
      memset(dstats, 0, sizeof *dstats);
      if (pipe_is_raw(s->form)) {
        dstats->n = t.n;
        const uint8_t* etype = s->h_etype.u8() + t.first;
        const uint32_t* c0len = (const uint32_t*)s->h_c0len.p + t.first;
        for (uint64_t i = 0; i < t.n; i++) {
          const uint8_t et = etype[i];
          dstats->n_x509 += et == 0;
          dstats->n_precert += et == 1;
          dstats->n_decode_error += et == CTMR_ENTRY_INVALID;
          dstats->n_no_chain += et != CTMR_ENTRY_INVALID && c0len[i] == 0;
        }
        dstats->blob_bytes = slot_ticket_bytes(*s, t);
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
  PipeTextWait tw{PF_JSON, entries_cap, resp_first, resp_bad};
  const int rc = pipe_wait(e, ticket, records, new_idx, timestamp, dstats, stats, &tw);
  const auto& w = tw.info;
  if (info && tw.judged) *info = {w.bodies, w.items, w.text_bytes, w.decoded_bytes, w.bad_body, w.bad_offset};
  return rc;
}

int ctmr_wait_pem(ctmr_engine* e, ctmr_ticket ticket, uint64_t certs_cap, ctmr_record* records, uint64_t* new_idx, uint64_t* file_first,
                  uint64_t* file_bad, ctmr_pem_decode_info* info, ctmr_batch_stats* stats) {
  PipeTextWait tw{PF_PEM, certs_cap, file_first, file_bad};
  const int rc = pipe_wait(e, ticket, records, new_idx, nullptr, nullptr, stats, &tw);
  const auto& w = tw.info;
  if (info && tw.judged) *info = {w.bodies, w.items, w.text_bytes, w.decoded_bytes, w.items - w.irregular, w.irregular, w.bad_body, w.bad_offset};
  return rc;
}
