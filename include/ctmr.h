/*
 * ctmr.h — C ABI of libctmr (MI355X-native ct-mapreduce map/reduce hot path).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  A Go host
 * binds it through cgo (INTEGRATION.md shows the stub); the C++ host mirror in
 * ct_mapreduce_amd/csrc/storage.hpp and the Python ctypes binding in
 * ct_mapreduce_amd/_native.py bind exactly the same symbols.
 *
 * Every entry point cites the reference interface it replaces (paths relative to
 * jcjones/ct-mapreduce).  The reference has no FFI of its own (100 % Go): the seam is the
 * `entryChan` consumer (cmd/ct-fetch/ct-fetch.go:191) for the batched map, and the
 * storage.RemoteCache set methods (storage/types.go:83-102) for the reduce state.
 *
 * Conventions
 *   - every function returns CTMR_OK (0) or a negative CTMR_E_* code; ctmr_last_error()
 *     gives the message of the last failure on that engine.
 *   - strings/members are (ptr,len) byte ranges, never NUL-terminated (serials contain \0).
 *   - no pointer passed in is retained after the call returns (cgo rule).
 *   - all entry points are thread-safe (one mutex per engine; GPU work is stream-ordered).
 *   - there is NO CPU fallback: without a usable HIP device ctmr_create fails loudly.
 */
#ifndef CTMR_H
#define CTMR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTMR_ABI_VERSION 7

enum {
  CTMR_OK = 0,
  CTMR_E_INVAL = -1,     /* bad argument */
  CTMR_E_HIP = -2,       /* HIP runtime error (message has the hipError string) */
  CTMR_E_NOMEM = -3,     /* device or host allocation failed */
  CTMR_E_FULL = -4,      /* known-certificate table (at max_table_slots) / issuer table / pair table is full; a map /
                            insert call that returns it has not been applied (no slot claimed, no counter changed) */
  CTMR_E_NOTFOUND = -5,
  CTMR_E_RANGE = -6      /* caller buffer too small; *need tells the size */
};

/* Per-entry status, in the order insertCTWorker tests things
 * (cmd/ct-fetch/ct-fetch.go:191-235). */
enum {
  CTMR_ST_PASS = 0,               /* reached database.Store (:229) */
  CTMR_ST_PARSE_ERROR = 1,        /* x509.ParseCertificate(leaf) failed (:202-209) */
  CTMR_ST_FILTERED_CA = 2,        /* certIsFilteredOut :47-50 */
  CTMR_ST_FILTERED_EXPIRED = 3,   /* :52-55 */
  CTMR_ST_FILTERED_CN = 4,        /* :57-69 */
  CTMR_ST_NO_ISSUER = 5,          /* len(Chain) < 1 (:215-219) */
  CTMR_ST_ISSUER_PARSE_ERROR = 6, /* x509.ParseCertificate(Chain[0]) failed (:221-225) */
  CTMR_ST_ENTRY_DECODE_ERROR = 7, /* ct.LogEntryFromLeaf failed: the downloader drops the entry before entryChan
                                     (:452-459); only produced by the raw-entry calls (ctmr_decode_entries_*) */
  CTMR_ST__COUNT = 8
};

/* record.flags */
#define CTMR_FL_PRECERT 0x01      /* entry_type == 1 (ct.PrecertLogEntryType, :201) */
#define CTMR_FL_WAS_UNKNOWN 0x02  /* KnownCertificates.WasUnknown == true (knowncertificates.go:38) */
#define CTMR_FL_LONG_SERIAL 0x04  /* serial_len > 20: serial[] holds only the first 20 octets */

#define CTMR_NO_ISSUER 0xFFFFFFFFu /* issuer_idx value meaning "len(Chain) < 1" */
#define CTMR_ENTRY_INVALID 0xFFu   /* entry_type value meaning "LogEntryFromLeaf failed" → CTMR_ST_ENTRY_DECODE_ERROR */
#define CTMR_PAYLOAD_PAD 32        /* readable bytes required after offsets[n] (device inputs) */
#define CTMR_MAX_SERIAL 40         /* longest serial the in-HBM set stores; longer → host set */

/* One 32-byte output record per entry (the "+32 B" of B_alg). */
typedef struct {
  uint8_t status;       /* CTMR_ST_* */
  uint8_t flags;        /* CTMR_FL_* */
  uint16_t serial_len;  /* raw INTEGER content length (storage/types.go:171-178) */
  int32_t exp_hour;     /* floor(NotAfter/3600): NewExpDateFromTime (types.go:339-346) */
  uint32_t issuer_idx;  /* as passed in */
  uint8_t serial[20];   /* first min(20,serial_len) raw serial octets, zero padded */
} ctmr_record;

typedef struct {
  uint32_t struct_size;       /* sizeof(ctmr_config) */
  int32_t device;             /* HIP device ordinal */
  uint64_t table_slots;       /* known-certificate table: index slots (8-byte words; rounded up to 2^k); 0 = 2^24.
                                 The 64-byte key cells live in an arena of slots/2 cells that grows on demand */
  uint64_t pair_slots;        /* (expDate,issuer) cardinality table capacity; 0 = 2^22 */
  uint32_t max_issuers;       /* 0 = 65536 */
  uint32_t certs_per_tile;    /* sweep build only (variant 1); 0 = default */
  uint32_t lds_tile_bytes;    /* sweep build only (variant 1); 0 = default */
  uint32_t map_variant;       /* 0 = default (15).  15 = k_map_fused: the map fused with pass 1 of the known-certificate
                                 insert; 13 = k_map_winc + k_insert: the same map and insert as separate kernels.  Any other
                                 value: CTMR_E_INVAL (the baseline designs 1 = whole-certificate LDS tile and 2 = direct
                                 global loads exist only in the sweep build, scripts/sweep.py) */
  uint32_t profile;           /* 1 = bracket every kernel with hipEvents (ctmr_batch_stats.ms_*) */
  uint32_t collect_meta;      /* 1 = the map also records where each certificate's issuer Name and
                                 cRLDistributionPoints lie (8 B per entry) so that ctmr_meta_new* can run */
  uint64_t max_table_slots;   /* growth limit of the known-certificate table; 0 = 2^31.  Redis grows until OOM
                                 (storage/rediscache.go:57-65); here, before a call that may claim more slots than keep
                                 the load under 3/4, the table is rebuilt on the GPU into the power of two that holds
                                 (live members + incoming) at load <= 1/2 — tombstones (expiry sweeps, SetRemove) are
                                 dropped by the rebuild.  When even this limit cannot hold the call, it fails with
                                 CTMR_E_FULL BEFORE anything is inserted: a batch is applied completely or not at all. */
} ctmr_config;

typedef struct {
  uint64_t n;                          /* entries in the batch */
  uint64_t by_status[CTMR_ST__COUNT];  /* histogram of record.status */
  uint64_t n_new;                      /* PASS entries whose key was unknown (first by log index) */
  uint64_t n_dup;                      /* PASS entries already known */
  uint64_t n_host_set;                 /* PASS entries with serial_len > CTMR_MAX_SERIAL (host-side set) */
  uint64_t payload_bytes;              /* offsets[n]-offsets[0] */
  /* filled when config.profile: per-kernel GPU time of this batch, milliseconds */
  float ms_map, ms_insert, ms_resolve, ms_compact, ms_total;
  uint32_t map_launches;
} ctmr_batch_stats;

typedef struct {
  int32_t valid;          /* the issuer certificate parsed (else entries get ISSUER_PARSE_ERROR) */
  uint32_t canonical_idx; /* first registered issuer with the same SPKI digest */
  uint8_t spki_sha256[32];/* SHA-256(RawSubjectPublicKeyInfo), computed on the GPU */
  char issuer_id[48];     /* Issuer.ID(): padded base64url of the digest, NUL terminated (types.go:124-130) */
} ctmr_issuer_info;

typedef struct ctmr_engine ctmr_engine;

/* ---- lifecycle (no reference equivalent; engine.GetConfiguredStorage engine/engine.go:19-48
 *      is where a Go host would construct it) ---- */
int ctmr_abi_version(void);
int ctmr_create(const ctmr_config* cfg, ctmr_engine** out);
void ctmr_destroy(ctmr_engine* e);
/* The message of the last failure on that engine, copied for the calling thread: valid until this thread's next
 * ctmr_last_error call (other threads may fail concurrently; nobody is handed a pointer into a string in flux). */
const char* ctmr_last_error(const ctmr_engine* e);
/* Launch all GPU work on this hipStream_t (default: a stream the engine owns). */
int ctmr_set_stream(ctmr_engine* e, void* hip_stream);
int ctmr_synchronize(ctmr_engine* e);

/* Page-locked host memory for the host-buffer entry points (ctmr_map_batch, ctmr_map_entries, ctmr_add_issuers):
 * buffers obtained here are copied to HBM by DMA at full PCIe rate without the driver's bounce copy.  A cgo host
 * fills them through unsafe.Slice; they are C memory, so the "no Go pointer is retained" rule is not involved. */
int ctmr_alloc_pinned(ctmr_engine* e, size_t bytes, void** out);
int ctmr_free_pinned(ctmr_engine* e, void* p);

/* ---- issuer table: replaces x509.ParseCertificate(Chain[0]) + NewIssuer + Issuer.ID()
 *      (ct-fetch.go:221; storage/types.go:109-130,155-159).  Appends n issuer certificates
 *      (DER blob + n+1 offsets); *first_idx receives the index of the first one. ---- */
int ctmr_add_issuers(ctmr_engine* e, const uint8_t* der, const uint64_t* offsets, uint32_t n,
                     uint32_t* first_idx);
int ctmr_issuer_count(ctmr_engine* e, uint32_t* n);
/* SHA-256 of one byte string, on the GPU: SPKI.Sha256DigestURLEncodedBase64 for an Issuer constructed from raw
 * SPKI bytes instead of a chain certificate (storage/types.go:155-159).  Not a hot-path call. */
int ctmr_sha256(ctmr_engine* e, const uint8_t* data, size_t len, uint8_t out[32]);
int ctmr_issuer_info_get(ctmr_engine* e, uint32_t idx, ctmr_issuer_info* out);

/* ---- filter configuration: *ctconfig.IssuerCNFilter, *ctconfig.LogExpiredEntries and the
 *      time.Now() of certIsFilteredOut (ct-fetch.go:44-70; config/config.go:194-196).  A refused call
 *      (CTMR_E_INVAL: more than 64 pieces or 1024 words) leaves the earlier filter in force. ---- */
int ctmr_set_filter(ctmr_engine* e, const char* issuer_cn_filter, size_t len, int log_expired,
                    int64_t now_unix);

/* ---- the batched map + reduce: replaces the body of insertCTWorker's loop
 *      (ct-fetch.go:191-235) through FilesystemDatabase.Store's WasUnknown
 *      (storage/filesystemdatabase.go:158-183; storage/knowncertificates.go:38-55).
 *   payload      packed leaf DER (the X509 cert or Precert.Submitted.Data, :198-204)
 *   offsets      n+1 byte offsets into payload
 *   issuer_idx   per entry index into the issuer table, or CTMR_NO_ISSUER
 *   entry_type   per entry 0 = X509LogEntryType, 1 = PrecertLogEntryType (may be NULL = all 0)
 *   records      n records out (may be NULL)
 *   new_idx      indices (ascending) of entries with CTMR_FL_WAS_UNKNOWN; capacity n (may be NULL)
 * Host variant: all pointers are host memory; the library stages through pinned buffers. */
int ctmr_map_batch(ctmr_engine* e, const uint8_t* payload, const uint64_t* offsets,
                   const uint32_t* issuer_idx, const uint8_t* entry_type, uint64_t n,
                   ctmr_record* records, uint64_t* new_idx, ctmr_batch_stats* stats);
/* Device variant: payload/offsets/issuer_idx/entry_type/records/new_idx are DEVICE pointers
 * (payload 16-byte aligned, CTMR_PAYLOAD_PAD readable bytes after offsets[n]); stats is host. */
int ctmr_map_batch_device(ctmr_engine* e, const uint8_t* d_payload, const uint64_t* d_offsets,
                          const uint32_t* d_issuer_idx, const uint8_t* d_entry_type, uint64_t n,
                          ctmr_record* d_records, uint64_t* d_new_idx, ctmr_batch_stats* stats);

/* ---- asynchronous host ingestion: the counterpart, in front of the GPU, of the channel between the reference's
 *      downloader and its insertCTWorker goroutines (cmd/ct-fetch/ct-fetch.go:132,140-145,191): the downloader hands
 *      over one get-entries response at a time, at most 1 001 entries (:417-424), and a synchronous ctmr_map_batch per
 *      response is bound by the host↔device round trip, not by the GPU.
 *   submit: same arguments as ctmr_map_batch; returns a ticket at once.  The DER goes to HBM with an asynchronous copy
 *           behind the previous submit's bytes (straight DMA from buffers of ctmr_alloc_pinned — keep them untouched
 *           until ctmr_wait; pageable memory is staged before the call returns); consecutive submits coalesce into a
 *           super-batch that is mapped as ONE batch when it reaches 65 536 entries / 96 MB, on ctmr_flush, or when one
 *           of its tickets is waited for — while the next one is already filling.
 *   wait:   blocks until the ticket's super-batch is done; records / new_idx (indices relative to THIS batch, ascending)
 *           / stats as ctmr_map_batch returns them (any may be NULL).  A ticket is collected once.
 *      Super-batches run in submission order and entries keep their order inside one: the lowest log index of a key
 *      wins WasUnknown across everything in flight, as in a sequence of synchronous calls.  Up to 4 super-batches may
 *      be unfinished or uncollected; a submit that would need a fifth blocks while one is still running and fails
 *      with CTMR_E_RANGE when all four only wait to be collected.  Thread-safe (several downloader threads may submit
 *      and wait).  ctmr_pem_new / ctmr_meta_new refer to synchronous calls only; what they give, a ticket gets through
 *      ctmr_set_pipeline_writeback / ctmr_ticket_writeback (below, behind ctmr_meta_new). ---- */
typedef uint64_t ctmr_ticket;
int ctmr_submit_batch(ctmr_engine* e, const uint8_t* payload, const uint64_t* offsets, const uint32_t* issuer_idx,
                      const uint8_t* entry_type, uint64_t n, ctmr_ticket* ticket);
int ctmr_flush(ctmr_engine* e);
int ctmr_wait(ctmr_engine* e, ctmr_ticket ticket, ctmr_record* records, uint64_t* new_idx, ctmr_batch_stats* stats);
/* (raw get-entries responses: ctmr_submit_entries / ctmr_wait_entries, and get-entries bodies as text:
 * ctmr_submit_entries_json / ctmr_wait_entries_json, with the raw-entry calls below; ctmr_wait refuses a ticket of the
 * text form with CTMR_E_INVAL and leaves it collectable) */

/* ---- storage.RemoteCache set methods on byte strings (storage/types.go:83-102;
 *      Redis impl storage/rediscache.go:57-120,153-169; mock storage/mockcache.go:38-166).
 *      Keys of the form "serials::<expDateID-with-hour>::<issuerID of a registered issuer>"
 *      live in the HBM table; every other key lives in a host-side string-set store. ---- */
int ctmr_set_insert(ctmr_engine* e, const char* key, size_t key_len, const uint8_t* member,
                    size_t member_len, int* was_new);                      /* SetInsert  */
int ctmr_set_contains(ctmr_engine* e, const char* key, size_t key_len, const uint8_t* member,
                      size_t member_len, int* present);                    /* SetContains */
int ctmr_set_remove(ctmr_engine* e, const char* key, size_t key_len, const uint8_t* member,
                    size_t member_len, int* removed);                      /* SetRemove  */
int ctmr_set_cardinality(ctmr_engine* e, const char* key, size_t key_len, int64_t* n); /* SetCardinality */
int ctmr_exists(ctmr_engine* e, const char* key, size_t key_len, int* exists);         /* Exists */
/* SetList / SetToChan: members serialised [u32 len][bytes]…, sorted bytewise.  *need = bytes
 * required; returns CTMR_E_RANGE (and copies nothing) when cap < *need. */
int ctmr_set_members(ctmr_engine* e, const char* key, size_t key_len, uint8_t* out, size_t cap,
                     size_t* need, uint64_t* count);
/* KeysToChan(pattern): glob as path.Match ('*', '?', '[..]', '\\'); same serialisation, sorted. */
int ctmr_keys(ctmr_engine* e, const char* pattern, size_t pattern_len, uint8_t* out, size_t cap,
              size_t* need, uint64_t* count);
/* ExpireAt: records the key's expiry; ctmr_expire_sweep(now) drops every key whose expiry
 * is <= now (what Redis does lazily).  map_batch records ExpireAt(key, expDate hour) for
 * every serials key it creates (knowncertificates.go:44-47,98-104). */
int ctmr_expire_at(ctmr_engine* e, const char* key, size_t key_len, int64_t unix_seconds);
int ctmr_expire_sweep(ctmr_engine* e, int64_t now_unix, uint64_t* members_removed);

/* ---- per-issuer unique counts: Σ_expDate SCARD(serials::expDate::issuer), the quantity
 *      storage-statistics reports (cmd/storage-statistics/storage-statistics.go:44-53).
 *      out[i] is the count for registered issuer i (equal for issuers sharing an SPKI). ---- */
int ctmr_issuer_counts(ctmr_engine* e, uint64_t* out, uint32_t n);
int ctmr_total_count(ctmr_engine* e, uint64_t* out);
/* Device pointer to the live u64[max_issuers] canonical-issuer counters (for an RCCL
 * all-reduce by the multi-GPU driver). */
int ctmr_issuer_counts_device(ctmr_engine* e, void** d_counts, uint32_t* n);
/* Drop every known certificate (table, pair counts, counters, host-side sets keep keys). */
int ctmr_reset_known(ctmr_engine* e);

/* How full the known-certificate table is (what `INFO memory` / `DBSIZE` tell the operator of the reference's Redis,
 * storage/rediscache.go:21-45).  The table is an index of 8-byte words (slots) over an arena of 64-byte key cells; a batch
 * takes one cell per entry and cells of entries that were not new are squeezed out again when the arena runs short
 * (arena_compactions), before it is grown (arena_growths); the index is rebuilt at load 3/4 (rebuilds). */
typedef struct {
  uint64_t slots;              /* index words */
  uint64_t occupied;           /* index words claimed since the last rebuild: live members + tombstones */
  uint64_t arena_cells;        /* capacity of the key-cell arena */
  uint64_t arena_used;         /* cells handed out (live + not yet squeezed out) */
  uint64_t rebuilds, arena_compactions, arena_growths;
  uint64_t reserved;
} ctmr_table_info;
int ctmr_table_info_get(ctmr_engine* e, ctmr_table_info* out);

/* ---- the known-certificate image: bulk snapshot and restore of every serials::<expDate>::<issuerID> set.  Replaces
 *      what a restart of the reference finds in its persistent RemoteCache (storage/rediscache.go: Redis outlives
 *      ct-fetch restarts, redeploys and reshards): export on shutdown, import on start.  DESIGN.md §12.
 *
 * Image v1, little-endian: image = meta ‖ members.
 *   header, 64 B   "CTMRKNWN" | u32 version = 1 | u32 header_bytes = 64 | u32 n_issuers | u32 flags = 0 | u64 n_sets |
 *                  u64 n_members | u64 host_bytes | u64 n_host_members | u64 reserved = 0
 *   issuers        n_issuers × 32 B: SHA-256(SPKI) of each issuer the sets name (Issuer.ID = its padded base64url);
 *                  the ordinal is process-independent (export: digest order), canonical indices are not
 *   sets           n_sets × 24 B {i32 exp_hour, u32 issuer_ordinal, u64 first_member, u64 count}, in bytewise order of
 *                  the key serials::<expDate>::<Issuer.ID> (the order ctmr_keys returns); contiguous, covering the
 *                  members exactly, none empty
 *   host section   host_bytes of {u32 key_len, key, u32 member_len, member} sorted by (key, member): the serials::
 *                  members of the host-side store (serials longer than CTMR_MAX_SERIAL; issuers not registered)
 *   members        at the next multiple of 64 B: n_members × 48 B {u64 serial_len (0..40), serial[40] zero-padded}
 *                  (k_list's record); the order inside a set is unspecified unless the writer sorted it (below:
 *                  ctmr_set_known_order, ctmr_known_sort)
 * The bytes before the members ("meta") are small and live on the host; the device variants take meta and members as
 * separate buffers.  Exported members are the live members SetList / SetCardinality see (a Bloom-mode rank's SHADOW
 * keys are not: the union of a group's images holds each key once).  ExpireAt overrides, crl:: / issuer:: / log:: keys
 * and the IssuerMetadata memo are not carried (redis_dump covers the RemoteCache keys). */
typedef struct {
  uint64_t members;       /* member records (device section) */
  uint64_t sets;
  uint64_t host_members;  /* members of the host section */
  uint64_t meta_bytes;    /* header + issuers + sets + host section, padded to 64 */
  uint64_t image_bytes;   /* meta_bytes + 48 × members */
  uint32_t issuers, reserved;
} ctmr_known_image_info;
typedef struct {
  uint64_t members;        /* member records of the image */
  uint64_t taken;          /* … this rank took (its keys; world = 1: all) */
  uint64_t inserted;       /* … of them new here (device table, or the host-side store for issuers not registered) */
  uint64_t known;          /* taken − inserted: already present, or a repeat inside the image */
  uint64_t host_members;   /* host-section members taken (rank 0 alone) */
  uint64_t host_inserted;  /* … of them new here */
} ctmr_known_import_stats;
/* Export.  Fills *info; when out (cap bytes) is too small returns CTMR_E_RANGE and writes nothing.  Returns after the
 * engine's stream has drained.  The member records are staged on the device (in set ranges when the whole does not fit). */
int ctmr_known_export(ctmr_engine* e, uint8_t* out, size_t cap, ctmr_known_image_info* info);
/* Export into a host meta buffer and a device buffer of members_cap 48-byte records (CTMR_E_RANGE as above). */
int ctmr_known_export_device(ctmr_engine* e, uint8_t* meta, size_t meta_cap, void* d_members, uint64_t members_cap,
                             ctmr_known_image_info* info);
/* Import = ctmr_set_insert(key, member) for every member this rank takes — the union with what the engine holds;
 * members of issuers not registered here and serials longer than CTMR_MAX_SERIAL go to the host-side store (registering
 * the issuer later moves them, as it does after a redis_load).  Per-issuer counts, the pair statistics and the Bloom
 * filter (when configured) come out as those inserts leave them.  world / rank: the rank takes the keys whose owner
 * (the owner-computes exchange's owner function) is `rank` among `world` — every rank of a group restored from the same
 * image(s) holds each key once, on its owner, whatever world size exported it; host-section members go to rank 0.
 * world = 1, rank = 0 takes everything.  CTMR_E_INVAL, nothing applied: bad magic / version, sizes that disagree, sets
 * out of order / overlapping / leaving gaps, an issuer ordinal out of range, a serial_len above 40 or non-zero padding
 * (checked on the device before the first insert), world == 0 or rank >= world, world > 1 with a set whose issuer is not
 * registered, an owner-computes round open on the engine.  CTMR_E_FULL / CTMR_E_NOMEM as for a batch: the call reserves
 * for every member it takes before it inserts one. */
int ctmr_known_import(ctmr_engine* e, const uint8_t* image, size_t len, uint32_t world, uint32_t rank,
                      ctmr_known_import_stats* st);
int ctmr_known_import_device(ctmr_engine* e, const uint8_t* meta, size_t meta_len, const void* d_members,
                             uint64_t n_members, uint32_t world, uint32_t rank, ctmr_known_import_stats* st);

/* ---- bulk SetContains / SetRemove (storage/types.go:83-102) with an image as the batch: one call asks about, or
 *      removes, every member record of an image v1 (above; nothing about the format changes).  DESIGN.md §14.
 *
 * world / rank as for import: the rank is asked about exactly the records ctmr_known_import with the same world / rank
 * would take (the keys it owns; host-section members: rank 0 alone); world > 1 with a set whose issuer is not registered
 * here is CTMR_E_INVAL.  Records of sets whose issuer is not registered (world = 1) and the host section are answered
 * from / erased in the host-side store, where ctmr_set_insert would have put them.
 *
 * Query: flags[i], one byte per member record in image order: 1 = ctmr_set_contains(key of record i's set, member i)
 *   would answer true at the time of the call, 0 = it would answer false, 2 = this rank was not asked.  A Bloom-mode
 *   rank's SHADOW keys count as present, as they do for ctmr_set_contains.  host_flags: one byte per host-section member
 *   in section order (rank 0; every other rank: 2).  Duplicate records get the same answer each.  A flags or host_flags
 *   buffer that is too small: CTMR_E_RANGE, *st filled as far as known (members, host_members), nothing written.
 *   Read-only: table, arena, pair statistics, counters, Bloom filter, host-side store, expiry records and
 *   ctmr_table_info are as before.  The records are validated in the pass that probes: on CTMR_E_INVAL the flags are
 *   unspecified.
 * Remove: the effect of ctmr_set_remove(key, member) for every record the rank takes, in any order: the member's index
 *   word becomes a tombstone, its canonical issuer's counter goes down by one (not for a SHADOW key: another rank counts
 *   it), the pair statistics are rebuilt before their next use, a host-side member is erased (its key with its last
 *   member); Bloom bits stay, as after a point remove.  A member the image names twice is removed and counted once:
 *   hits = members removed, taken − hits = records that found nothing (absent, or a repeat).  All or nothing on a bad
 *   image: everything ctmr_known_import rejects (magic, version, sizes, set order / gaps / overlaps, ordinals, a
 *   serial_len above 40 or non-zero padding — checked on the device before the first word is touched — world == 0,
 *   rank >= world, an open owner-computes round) is CTMR_E_INVAL with nothing removed.
 * Both return after the engine's stream has drained.  Images above 2^27 records are worked through in passes of 2^27. */
typedef struct {
  uint64_t members;       /* member records of the image */
  uint64_t taken;         /* … this rank was asked about (world = 1: all) */
  uint64_t hits;          /* query: taken records whose member is held; remove: members removed */
  uint64_t host_members;  /* host-section members taken (rank 0 alone) */
  uint64_t host_hits;     /* … of them held / removed */
  uint64_t reserved;
} ctmr_known_probe_stats;
int ctmr_known_query(ctmr_engine* e, const uint8_t* image, size_t len, uint32_t world, uint32_t rank, uint8_t* flags,
                     size_t flags_cap, uint8_t* host_flags, size_t host_flags_cap, ctmr_known_probe_stats* st);
/* … the member records (meta's n_members × 48 B) and the flags (flags_cap bytes) in device memory */
int ctmr_known_query_device(ctmr_engine* e, const uint8_t* meta, size_t meta_len, const void* d_members,
                            uint64_t n_members, uint32_t world, uint32_t rank, void* d_flags, uint64_t flags_cap,
                            uint8_t* host_flags, size_t host_flags_cap, ctmr_known_probe_stats* st);
int ctmr_known_remove(ctmr_engine* e, const uint8_t* image, size_t len, uint32_t world, uint32_t rank,
                      ctmr_known_probe_stats* st);
int ctmr_known_remove_device(ctmr_engine* e, const uint8_t* meta, size_t meta_len, const void* d_members,
                             uint64_t n_members, uint32_t world, uint32_t rank, ctmr_known_probe_stats* st);

/* ---- per-issuer known-serial lists: what this map/reduce exists to produce.  For each Issuer.ID, the serials of its
 *      certificates that have not expired, as FilesystemDatabase hands them to StorageBackend.StoreKnownCertificateList
 *      (storage/types.go) — the composition of GetIssuerAndDatesFromCache (storage/filesystemdatabase.go), IsExpiredAt
 *      and KnownCertificates.Known() per expDate.  LocalDiskBackend writes one list as the file <root>/<Issuer.ID>.
 *      DESIGN.md §13.
 *
 * Which sets.  Every set the engine holds (the device table and the serials:: keys of the host-side store) whose expDate
 *   is not expired at now_unix: !NewExpDate(<expDate of its key>).IsExpiredAt(now).  An hour-resolution key of exp hour h
 *   is kept iff now_unix < (h + 1) × 3600 (lastGood = h·3600 + 1 h − 1 ms): kept at (h+1)·3600 − 1, dropped at
 *   (h+1)·3600.  A day-resolution host key ("2006-01-02") uses lastGood = day + 24 h − 1 ms.  A key whose date NewExpDate
 *   cannot parse is skipped, as GetIssuerAndDatesFromCache skips it — among them every hour outside the years 0000..9999.
 *   A serials:: key that does not split into exactly three "::" parts fails the call with CTMR_E_INVAL (the reference
 *   returns an error for it).  The call does not sweep: ctmr_expire_sweep(now) first gives Redis's TTL behaviour, and
 *   ExpireAt overrides play no part.
 * Grouping.  One list per Issuer.ID string: registered issuers that share an SPKI share one canonical ID and one list;
 *   host-store keys of issuers not registered here give their key's issuer string; long-serial members (above
 *   CTMR_MAX_SERIAL octets, in the host-side store) join their issuer's list.
 * Lines.  hex.EncodeToString(serial) + "\n": lowercase, every raw octet, leading 00 kept; an empty serial is a line "\n".
 *   One line per set member, not deduplicated: a serial known under two expDates of one issuer is listed twice.  Within
 *   a list the lines of one expDate are contiguous and expDates ascend (by their first second, then bytewise as strings);
 *   the order inside an expDate is unspecified under CTMR_KNOWN_ORDER_ANY; under CTMR_KNOWN_ORDER_SORTED (below) the
 *   lines of one expDate are in `LC_ALL=C sort` order ("\n" sorts before every hex digit, so a serial comes before
 *   the serials it is a proper prefix of, as in the image).  Lists are ordered by Issuer.ID bytewise.
 * Left out.  A Bloom-mode rank's SHADOW keys, as in the image: the union of a group's ranks holds each key once, so the
 *   per-issuer concatenation of the ranks' lists is the group's list (up to the order inside an expDate).
 * Read-only: table, pair statistics, counters, host-side store and expiry records are as before.
 *
 * Output: text = the lists back to back; ids = the Issuer.IDs back to back; offs = 2 × (issuers + 1) u64: the text
 * offset of each list and text_bytes, then the offset of each ID in ids and ids_bytes (offs_cap counts u64).  Two-call
 * convention as ctmr_known_export: when a buffer is too small, *info is filled and the call returns CTMR_E_RANGE and
 * writes nothing.  text_bytes depends on every member's serial length: a call that cannot size by the bound
 * 81 B × members counts on the device first.  The members are staged on the device in set ranges of at most 2^26
 * records (a larger set alone).  Returns after the engine's stream has drained. */
typedef struct {
  uint64_t issuers;       /* lists */
  uint64_t sets;          /* (expDate, Issuer.ID) sets kept */
  uint64_t members;       /* lines from the device table */
  uint64_t host_members;  /* lines from the host-side store */
  uint64_t text_bytes;
  uint64_t ids_bytes;
} ctmr_known_lists_info;
int ctmr_known_lists(ctmr_engine* e, int64_t now_unix, uint8_t* text, size_t text_cap, uint8_t* ids, size_t ids_cap,
                     uint64_t* offs, size_t offs_cap, ctmr_known_lists_info* info);
/* The same with text in device memory (of this engine's device); host-store lines are copied into it at their places. */
int ctmr_known_lists_device(ctmr_engine* e, int64_t now_unix, void* d_text, size_t text_cap, uint8_t* ids, size_t ids_cap,
                            uint64_t* offs, size_t offs_cap, ctmr_known_lists_info* info);

/* ---- the order inside a set: member records sorted on the GPU.  DESIGN.md §15.
 *
 * The order.  Within a set, member records ascend by serial as byte strings — octet by octet, unsigned, a proper prefix
 *   before the longer string (what sorted() does to Python bytes).  On the 48-byte record this is the order of the 40
 *   zero-padded octets compared big-endian, then serial_len: the serials "", 00, 00 00 have identical padding and
 *   serial_len decides between them.  Equal records are indistinguishable, so the sorted bytes of a set are unique.
 * ctmr_known_sort_device sorts the member records of an image v1 in place, set by set; the meta is read, not changed.
 *   It validates as ctmr_known_import_device does — magic, version, sizes, set order / gaps / overlaps, issuer ordinals,
 *   and on the device, before the first record moves, serial_len <= 40 and zero padding: CTMR_E_INVAL leaves the
 *   buffer as it was.  The issuers the image names need not be registered here; nothing of the engine's state is read
 *   or changed (table, pair statistics, counters, host-side store, Bloom filter, ctmr_table_info).  Repeated records
 *   stay, next to each other.  The working buffers (about 82 B per record of a run: two 16-byte key buffers, the permuted
 *   records aside, digit counts) are allocated before the first record moves: CTMR_E_NOMEM leaves the buffer as it was.
 *   The records are sorted in runs of whole sets of at most 2^27 records (a larger set alone); a run's permuted records
 *   are built aside and copied over it only when complete.  Returns after the engine's stream has drained.
 * ctmr_known_sort does the same for an image in host memory (members staged on the device and copied back; the host
 *   section is already ordered by (key, member) and stays).
 * Cost.  A run is sorted in ROUNDS of a stable radix sort over (tie group, 8 serial octets): one round per 8 octets
 *   while two records of a set still agree in every octet compared so far, the sixth and last on serial_len — AT MOST
 *   SIX ROUNDS WHATEVER THE DATA HOLDS, and none for a run of one-member sets.  CT serials (16..20 random octets) take
 *   one; a CA that starts every serial with the same 8 octets pays one more round, never a quadratic tie-break.
 * ctmr_set_known_order: CTMR_KNOWN_ORDER_ANY (the default) leaves every call as it was.  Under
 *   CTMR_KNOWN_ORDER_SORTED ctmr_known_export, ctmr_known_export_device, ctmr_known_lists and ctmr_known_lists_device
 *   write each set's members / each expDate's lines in the order above, and nothing else about them changes (two-call
 *   sizing, CTMR_E_RANGE writing nothing, the places of the host-store pieces — whose lines std::set already orders).
 *   A sorted export is a pure function of the sets the engine holds: engines that reached the same sets by different
 *   batch orders, by import, or under different issuer numberings export identical bytes (every issuer registered, no
 *   serial above CTMR_MAX_SERIAL octets: exact; the host section is deterministic too).  Any other value: CTMR_E_INVAL. */
#define CTMR_KNOWN_ORDER_ANY 0
#define CTMR_KNOWN_ORDER_SORTED 1
int ctmr_set_known_order(ctmr_engine* e, int order);
int ctmr_known_sort(ctmr_engine* e, uint8_t* image, size_t len);
int ctmr_known_sort_device(ctmr_engine* e, const uint8_t* meta, size_t meta_len, void* d_members, uint64_t n_members);

/* ---- set algebra on images: union, minus and intersect of two images v1 on the GPU, with no table behind them.
 *      DESIGN.md §16.
 *
 * Result.  The canonical image of the operation applied key by key to the sets the two images denote — byte for byte
 *   what the canonical writer (known_image.build) makes of op(sets of A, sets of B): the issuers the surviving sets name
 *   and no others, in digest order; the sets in key order, none empty; every set's members ascending in the order of
 *   ctmr_known_sort, each member once; the host section's (key, member) pairs in order.
 * Host-section pairs that belong in the member section.  The canonical writer puts a pair into the member section
 *   whenever its key spells an (hour, issuer digest) as a set entry does and its member is at most CTMR_MAX_SERIAL octets.
 *   An operand's exporter may have put such a pair into the host section (it had not registered the issuer): in the
 *   result it is a member record, and it is compared with the other operand's member records as if it had been one.
 * b == NULL with b_len == 0 (device variant: b_meta == NULL, b_meta_len == 0, b_members == 0) is the empty image:
 *   CTMR_KNOWN_UNION then normalises A — sorts it, drops repeats and moves those host pairs.
 * Operands.  Any image ctmr_known_import accepts, sorted or not, with repeated records or not.  Everything the import
 *   rejects in either operand — magic, version, sizes, set order / gaps / overlaps, ordinals, and on the device a
 *   serial_len above 40 or non-zero padding — and an unknown op are CTMR_E_INVAL with nothing written.  The issuers the
 *   images name need not be registered here.
 * Read-only.  Nothing of the engine's state is read or changed (table, pair statistics, counters, host-side store,
 *   Bloom filter, ctmr_table_info), as for ctmr_known_sort; the operands are const and stay byte for byte as they were.
 * Sizing.  The two-call convention of ctmr_known_export: a buffer that is too small gives CTMR_E_RANGE with *info filled
 *   and nothing written.  A caller can size without a first call: at most |A| + |B| member records for CTMR_KNOWN_UNION
 *   (host-section members counted in) and |A| for the other two; the meta is at most the two metas' bytes together.
 * Memory.  Every working buffer is allocated before the first byte of the result is written: CTMR_E_NOMEM leaves the
 *   output buffers as they were.  An operand whose sets are already ascending and free of repeats (a sorted export, an
 *   earlier result) is used where it lies; any other is copied aside, sorted as ctmr_known_sort does and squeezed.
 * Both return after the engine's stream has drained.  ctmr_known_merge takes and writes whole images in host memory
 * (members staged on the device and copied back); ctmr_known_merge_device takes each operand's meta and member records
 * (device memory of this engine's device, 16-byte aligned) apart and writes the result's the same way. */
#define CTMR_KNOWN_UNION 0     /* A ∪ B */
#define CTMR_KNOWN_MINUS 1     /* A \ B */
#define CTMR_KNOWN_INTERSECT 2 /* A ∩ B */
int ctmr_known_merge(ctmr_engine* e, int op, const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len, uint8_t* out,
                     size_t cap, ctmr_known_image_info* info);
int ctmr_known_merge_device(ctmr_engine* e, int op, const uint8_t* a_meta, size_t a_meta_len, const void* d_a, uint64_t a_members,
                            const uint8_t* b_meta, size_t b_meta_len, const void* d_b, uint64_t b_members,
                            uint8_t* out_meta, size_t out_meta_cap, void* d_out, uint64_t out_members_cap,
                            ctmr_known_image_info* info);

/* ---- per-issuer known-serial lists straight from an image v1, with no table behind them.  DESIGN.md §17.
 *
 * Output.  text, ids, offs and *info are exactly those of ctmr_known_lists (info.members = lines from member records,
 *   info.host_members = lines from the host section), with the same two-call convention — a buffer that is too small
 *   gives CTMR_E_RANGE with *info filled and nothing written — and the same bound to size in one call: 81 B × member
 *   records plus the host section's lines (2 × octets + 1 each).
 * Which sets.  Every set record of the image and every key of its host section, under the expiry rules of
 *   ctmr_known_lists: a set of exp hour h is kept iff now_unix < (h + 1) × 3600, and hours outside the years 0000..9999
 *   are skipped; a host key's date is parsed as NewExpDate parses it (hour or day resolution) and a key it cannot parse
 *   is skipped; a host key that does not split into exactly three "::" parts fails the call with CTMR_E_INVAL.
 * Grouping.  One list per Issuer.ID string.  A set record's ID is the padded base64url of its digest in the image: the
 *   engine's issuer registry plays no part and the issuers need not be registered here.  A host key gives its own issuer
 *   string.  Lists ascend bytewise by ID; inside a list expDates ascend by their first second, then bytewise as strings.
 *   A set record and a host key of the same expDate string and issuer form ONE block: the member records first, then
 *   the host members — where ctmr_known_lists puts the host-side store's members of a key the table holds too.
 * Lines.  One line per member record, in the image's order inside its set; repeated records stay: the call neither sorts
 *   nor deduplicates.  A canonical image (a sorted export, any ctmr_known_merge result) therefore gives every expDate's
 *   lines in `LC_ALL=C sort` order, and for an image an engine exported under CTMR_KNOWN_ORDER_SORTED the text is byte
 *   for byte what that engine's ctmr_known_lists writes under CTMR_KNOWN_ORDER_SORTED at the same now_unix.  A caller
 *   with an unsorted image normalises it first: ctmr_known_merge(CTMR_KNOWN_UNION, image, NULL).
 * Validation.  The meta is checked as ctmr_known_import checks it (magic, version, sizes, set order / gaps / overlaps,
 *   ordinals).  On the device, before the first text byte is written, every record of a KEPT set is checked for
 *   serial_len <= 40 and zero padding; the records of sets that are not kept are not read.  CTMR_E_INVAL and
 *   CTMR_E_NOMEM leave every output buffer as it was.
 * Read-only.  Nothing of the engine's state is read or changed (table, pair statistics, counters, host-side store,
 *   Bloom filter, ctmr_table_info), as for ctmr_known_sort; the operand is const and stays as it was.
 * The member records are read where they lie, twice (a count pass, then the pass that writes), in runs of whole kept
 * sets of at most 2^27 records.  ctmr_known_image_lists takes a whole image in host memory (its member section staged
 * on the device once); ctmr_known_image_lists_device takes the meta and the member records (device memory of this
 * engine's device, 16-byte aligned) apart and writes the text to device memory, the host section's lines copied into it
 * at their places.  Both return after the engine's stream has drained. */
int ctmr_known_image_lists(ctmr_engine* e, const uint8_t* image, size_t len, int64_t now_unix, uint8_t* text, size_t text_cap,
                           uint8_t* ids, size_t ids_cap, uint64_t* offs, size_t offs_cap, ctmr_known_lists_info* info);
int ctmr_known_image_lists_device(ctmr_engine* e, const uint8_t* meta, size_t meta_len, const void* d_members,
                                  uint64_t n_members, int64_t now_unix, void* d_text, size_t text_cap, uint8_t* ids,
                                  size_t ids_cap, uint64_t* offs, size_t offs_cap, ctmr_known_lists_info* info);

/* ---- serials looked up in an image v1 whatever their expiration date: what a CRL entry, an OCSP response or an incident
 *      report asks, which name an issuer and a serial and nothing else.  DESIGN.md §25.
 *
 * Operands.  Two images v1: K, the known image — any image ctmr_known_import accepts, sorted or not, with or without
 *   repeated records — and P, the probe image.  P's member records and the members of its host section are the probes;
 *   the hours in P's set records and in its host keys are ignored: the hour is the wildcard.
 * Probes.  A probe is the Issuer.ID string of its set and its serial octets.  A set record's ID is the padded base64url
 *   of the digest the image names (as in ctmr_known_image_lists); a host key's ID is the key's own third part.  A host
 *   key that does not split into exactly three "::" parts fails the call with CTMR_E_INVAL, in either operand.
 * Answer.  For every probe, over the KEPT sets of K with the same Issuer.ID that hold a member equal to the probe's
 *   serial (same length, same octets), a ctmr_known_find_hit (below).
 * Kept sets.  Exactly the sets ctmr_known_image_lists keeps at now_unix: a set of exp hour h is kept iff
 *   now_unix < (h + 1) × 3600, and hours outside the years 0000..9999 are skipped; a host key's date is parsed as
 *   NewExpDate parses it (hour or day resolution; its hour is its first second / 3600, a day key is kept until its last
 *   second) and a key it cannot parse is skipped.  now_unix = INT64_MIN keeps everything that parses.
 * Sections.  Both sections of both operands count and a member matches wherever it lies: a pair of K's host section
 *   whose member has at most CTMR_MAX_SERIAL octets is compared with P's member records as if it were a member record,
 *   and the other way round (the rule of ctmr_known_merge).  Members above 40 octets can only meet in the two host
 *   sections.
 * Repeats.  The call neither sorts nor deduplicates: a record repeated in K counts each time, probes repeated in P each
 *   get the full answer, a probe whose issuer K does not name gets zeros.
 * Output.  hits[i] answers P's member record i in image order, host_hits[j] P's host-section member j in section order.
 *   The two-call convention: a buffer that is too small gives CTMR_E_RANGE with *info filled (found and host_found 0)
 *   and nothing written; a caller can size from P's header alone.
 * Validation.  Both metas are checked as ctmr_known_import checks them.  On the device, before the first hit is written,
 *   every record of P and every record of a kept set of K is checked for serial_len <= 40 and zero padding; the records
 *   of sets that are not kept are not read.  CTMR_E_INVAL and CTMR_E_NOMEM leave both output buffers as they were; every
 *   working buffer is allocated before the first output byte.
 * Read-only.  Nothing of the engine's state is read or changed (table, pair statistics, counters, host-side store,
 *   Bloom filter, ctmr_table_info), as for ctmr_known_sort: the issuers need not be registered, the operands are const.
 * K's kept member records are read once where they lie, in runs of whole kept sets of at most 2^27 records, against a
 * hash table of the probes.  ctmr_known_image_find takes whole images in host memory (both member sections staged on the
 * device once); ctmr_known_image_find_device takes each operand's meta and member records (device memory of this
 * engine's device, 16-byte aligned) apart and leaves the hits of P's member records in device memory (16-byte aligned).
 * Both return after the engine's stream has drained. */
typedef struct {
  uint32_t records;     /* member records / host-section members of kept sets equal to the probe.  In an image without
                           repeated records (a sorted export, any ctmr_known_merge result) this is the number of expDates
                           under which the issuer's serial is known.  Modulo 2^32. */
  int32_t first_hour;   /* lowest exp hour among them; 0 when records == 0 */
  int32_t last_hour;    /* highest: until when the certificate matters; 0 when records == 0 */
  uint32_t reserved;    /* 0 */
} ctmr_known_find_hit;
typedef struct {
  uint64_t probes, host_probes;  /* P's member records, P's host-section members */
  uint64_t found, host_found;    /* … of them with records > 0 */
  uint64_t sets_kept;            /* K's kept set records plus its kept host-section keys (a key of both sections twice) */
  uint64_t members_read;         /* the member records of K's kept sets */
} ctmr_known_find_info;
int ctmr_known_image_find(ctmr_engine* e, const uint8_t* known, size_t known_len, const uint8_t* probes, size_t probes_len,
                          int64_t now_unix, ctmr_known_find_hit* hits, size_t hits_cap, ctmr_known_find_hit* host_hits,
                          size_t host_hits_cap, ctmr_known_find_info* info);
int ctmr_known_image_find_device(ctmr_engine* e, const uint8_t* k_meta, size_t k_meta_len, const void* d_k_members,
                                 uint64_t k_members, const uint8_t* p_meta, size_t p_meta_len, const void* d_p_members,
                                 uint64_t p_members, int64_t now_unix, void* d_hits, uint64_t hits_cap,
                                 ctmr_known_find_hit* host_hits, size_t host_hits_cap, ctmr_known_find_info* info);

/* ---- an image v1 partitioned by a probe image, the hour as wildcard: the known certificates that are revoked and those
 *      that are not, each with its expDate — the revoked/<Issuer.ID> and known/<Issuer.ID> lists of a revocation filter.
 *      The semi-join of ctmr_known_image_find* that keeps K's records instead of counting them.  DESIGN.md §28.
 *
 * Operands, probes, kept sets, sections.  Word for word those of ctmr_known_image_find*: K is any image
 *   ctmr_known_import accepts; P's member records and host-section members are the probes (Issuer.ID string, serial
 *   octets), P's hours are ignored; K's kept sets are exactly those ctmr_known_image_lists keeps at now_unix (INT64_MIN
 *   keeps all that parse, hours outside the years 0000..9999 are skipped, a host date that does not parse is skipped); a
 *   host key of other than three "::" parts is CTMR_E_INVAL in either operand; a member matches wherever it lies (a
 *   pair of K's host section of at most CTMR_MAX_SERIAL octets meets P's member records, P's host members of at most
 *   CTMR_MAX_SERIAL octets meet K's member records, longer members meet in the two host sections only); a probe whose
 *   Issuer.ID K does not name matches nothing.
 * Results.  Two images v1.  HIT holds every member record and every host pair of a kept set of K that equals at least
 *   one probe, MISS every other member record and host pair of a kept set.  Sets that are not kept appear in neither and
 *   their records are not read.  A record repeated in K is carried each time; repeated probes change nothing.
 * Layout.  The call is stable: it does not sort, deduplicate or move anything between the sections.  The set records of
 *   a result are K's kept sets in K's order with K's hour, the new count and the new first_member, a set left empty
 *   dropped; inside a set the surviving records keep K's order.  The issuer table holds the distinct digests the
 *   surviving set records name, ascending, each once, and the set records' ordinals are renumbered to it.  The host
 *   section holds the surviving kept pairs in K's order.
 * Consequence.  If K is canonical (a sorted export, any ctmr_known_merge result) both results are canonical byte for
 *   byte, and ctmr_known_merge(CTMR_KNOWN_UNION, HIT, MISS) is the canonical image of K's kept sets.  A caller with
 *   another K normalises a result with ctmr_known_merge(CTMR_KNOWN_UNION, x, NULL).
 * Declining.  Either result may be declined — host variant: hit_out == NULL with hit_cap == 0; device variant:
 *   hit_meta == NULL, hit_meta_cap == 0, d_hit == NULL, hit_members_cap == 0; the same for MISS.  A declined image is
 *   not written and its part of *info is still filled.  Declining both is allowed: the call then only sizes.  A null
 *   buffer with a capacity is CTMR_E_INVAL.
 * Sizing.  The two-call convention: a wanted buffer that is too small gives CTMR_E_RANGE with *info filled and nothing
 *   written to any buffer.  A caller can size without a first call: each result has at most K's member records and at
 *   most K's meta bytes.
 * Validation.  Both metas are checked as ctmr_known_import checks them.  On the device, before the first output byte,
 *   every record of P and every record of a kept set of K is checked for serial_len <= 40 and zero padding.
 *   CTMR_E_INVAL and CTMR_E_NOMEM leave all four output buffers as they were; every working buffer is allocated before
 *   the first output byte.  Device pointers are 16-byte aligned, else CTMR_E_INVAL.
 * Read-only.  Nothing of the engine's state is read or changed, as for ctmr_known_image_find*: the issuers need not be
 *   registered, the operands are const and stay byte for byte.
 * K's kept member records are read twice where they lie (a pass that flags them against a hash table of the probes, a
 *   pass that copies them), in runs of whole kept sets of at most 2^27 records.  ctmr_known_image_split takes whole
 *   images in host memory (both member sections staged on the device once, the results staged there and copied out as
 *   meta ‖ members); ctmr_known_image_split_device takes each operand's meta and member records apart and leaves the
 *   results' member records in device memory.  Both return after the engine's stream has drained. */
typedef struct {
  ctmr_known_image_info hit, miss;   /* the two results, as ctmr_known_export fills them */
  uint64_t probes, host_probes;      /* P's member records, P's host-section members */
  uint64_t sets_kept, members_read;  /* as in ctmr_known_find_info */
} ctmr_known_split_info;
int ctmr_known_image_split(ctmr_engine* e, const uint8_t* known, size_t known_len, const uint8_t* probes, size_t probes_len,
                           int64_t now_unix, uint8_t* hit_out, size_t hit_cap, uint8_t* miss_out, size_t miss_cap,
                           ctmr_known_split_info* info);
int ctmr_known_image_split_device(ctmr_engine* e, const uint8_t* k_meta, size_t k_meta_len, const void* d_k_members, uint64_t k_members,
                                  const uint8_t* p_meta, size_t p_meta_len, const void* d_p_members, uint64_t p_members, int64_t now_unix,
                                  uint8_t* hit_meta, size_t hit_meta_cap, void* d_hit, uint64_t hit_members_cap,
                                  uint8_t* miss_meta, size_t miss_meta_cap, void* d_miss, uint64_t miss_members_cap,
                                  ctmr_known_split_info* info);

/* ---- the filter cascade of a revoked / not-revoked image pair: the CRLite filter the two results of
 *      ctmr_known_image_split* are the lists of.  A stack of Bloom filter layers that answers "revoked" for every record
 *      of R and "not revoked" for every record of S, with no error on either.  DESIGN.md §29.
 *
 * Operands.  R (revoked) and S (not revoked) are images v1, canonical or not, each any image ctmr_known_import accepts.
 *   Only the member records of KEPT sets take part: exactly the sets ctmr_known_image_lists keeps at now_unix (a set of
 *   exp hour h is kept iff now_unix < (h + 1) × 3600, hours outside the years 0000..9999 are skipped, INT64_MIN keeps
 *   all of those).  The records of sets that are not kept are not read.
 * Key.  The key of a member record is the 32-byte SPKI digest its set's issuer ordinal names in that image's own issuer
 *   table, followed by the record's serial_len serial octets: 32 to 72 octets.  The hour is not part of the key, and the
 *   issuer tables of the two images are not joined.
 * Hash.  Hash function i (0-based) of layer `level` (1-based) of an m-bit layer is
 *       u32le(SHA-256(salt ‖ u32le(i) ‖ u8(level) ‖ key)[0:4]) mod m
 *   with the caller's salt of 0 to 16 octets: a message of 37 to 93 octets.  This is the construction filtercascade's
 *   format 2 with hash algorithm 2 (rust-cascade's SHA-256/32) is understood to use; neither is available to this
 *   project and no golden vector exists, so compatibility with them is UNPINNED (as DESIGN.md §2 says of the CT
 *   parser).  What is pinned is this text, which the tests hold against hashlib.
 * Layers.  Layer 1 holds every kept record of R; the kept records of S that pass it (all k bits set) are its false
 *   positives F1.  Layer 2 holds F1; the kept records of R that pass it are F2.  Layer 3 holds F2 and is tested with F1,
 *   and so on: layer l is tested with the list layer l − 1 holds.  The build ends at the first layer whose list of false
 *   positives is empty.  No kept record in R: no layer.  No kept record in S: one layer, no test.  A key that occurs
 *   twice on a side is inserted and counted twice: nothing is deduplicated.
 * Sizes.  Integer arithmetic only.  A layer that holds n records has m = max(1, ceil(n × bpk_q8 / 256)) bits and k hash
 *   functions: (k_first, bpk_first_q8) for layer 1, (k_rest, bpk_rest_q8) for the others.  k lies in 1..32, bpk_q8 in
 *   1..65536, max_layers in 1..255, salt_len in 0..16 (the octets of salt[] behind it are ignored), else CTMR_E_INVAL;
 *   m must be below 2^32 and each side must have fewer than 2^32 member records, else CTMR_E_INVAL.
 * Non-convergence.  If layer max_layers still has false positives the operands share a key or the sizes are degenerate:
 *   CTMR_E_INVAL, info.left = how many records were left, nothing written.
 * Host sections.  Members of more than 40 octets, and every other pair of a host section, are NOT in the filter:
 *   info.r_host_skipped / s_host_skipped count the pairs under keys kept at now_unix (a key's date parsed as
 *   ctmr_known_image_find* parses it; a key of other than three "::" parts is CTMR_E_INVAL).  A caller answers them
 *   from the lists.
 * Format CTMRCASC v1, little-endian.  A 64-byte header: "CTMRCASC", u32 version = 1, u32 hash algorithm = 2, u32 layer
 *   count, u32 salt_len, salt[16] (zeros behind salt_len), u64 total length, u64 kept records of R, u64 of S.  Then one
 *   32-byte ctmr_cascade_layer per layer, levels 1, 2, ….  Each layer's bits start at the next multiple of 64 bytes
 *   (layer.offset, from the start of the cascade); bit b is byte b >> 3, mask 1 << (b & 7); the bits at and above m and
 *   all padding are zero; the total length is a multiple of 64.  A filtercascade format 2 file is a re-framing of the
 *   same bit arrays (not written here).
 * Build.  ctmr_cascade_build takes whole images in host memory and writes the cascade to host memory;
 *   ctmr_cascade_build_device takes each operand's meta and its member records in device memory and writes the cascade
 *   to device memory (all device pointers 16-byte aligned, else CTMR_E_INVAL).  The two-call convention: out == NULL or
 *   out_cap < info.bytes fills *info (layers, bytes, the layer table, the counts) and returns CTMR_E_RANGE with nothing
 *   written.  The layers are built in working memory and copied out only when they fit, so a call that only sizes costs
 *   a whole build: a caller who can bound the size (layer 1 is ceil(n × bpk_first_q8 / 256) bits, the others together
 *   are usually smaller) does better with one call and a generous buffer.  Every failure leaves `out` as it was.  Before the first output byte every record of a kept set of either operand is checked for serial_len <= 40
 *   and zero padding (CTMR_E_INVAL).  Nothing of the engine's state is read or changed; the operands stay byte for byte.
 *   info.syncs counts the times the host waited for the device: one per tested layer and one at the end.
 * Query.  For every member record of the probe image P — all its sets, whatever their hour, in record order — one byte:
 *   1 = the cascade says revoked, 0 = not.  A record that fails layer 1 is not revoked; one that passes layers 1..j and
 *   fails layer j + 1 is revoked iff j is odd; one that passes every layer is revoked iff the layer count is odd (no
 *   layer: not revoked).  The answer is exact for the kept records of R and S the cascade was built from and a guess
 *   for anything else.  The cascade is validated before anything is launched: magic, version, hash algorithm, the total
 *   length against the buffer's, salt_len, strictly ascending levels in 1..255, k in 1..32, m in 1..2^32 − 1, offsets
 *   that are multiples of 64 with the bits inside the buffer, else CTMR_E_INVAL.  P's host section is counted
 *   (info.host_probes), not answered.  out_cap < P's member records: CTMR_E_RANGE with *info filled, nothing written.
 *   ctmr_cascade_query takes everything in host memory; ctmr_cascade_query_device takes the cascade and P's member
 *   records in device memory (16-byte aligned) and leaves the answers there.
 * All four return after the engine's stream has drained. */
#define CTMR_CASCADE_MAX_LAYERS 255
typedef struct {
  uint32_t k_first, bpk_first_q8;  /* layer 1: hash functions, bits per held record × 256 */
  uint32_t k_rest, bpk_rest_q8;    /* the other layers */
  uint32_t max_layers;
  uint32_t salt_len;
  uint8_t salt[16];
} ctmr_cascade_params;
typedef struct {
  uint32_t level, k;
  uint64_t m_bits, offset, n_held;
} ctmr_cascade_layer;
typedef struct {
  uint64_t bytes;                           /* the cascade's total length */
  uint32_t layers, syncs;
  uint64_t r_records, s_records;            /* the member records of kept sets */
  uint64_t r_sets_kept, s_sets_kept;
  uint64_t r_host_skipped, s_host_skipped;
  uint64_t left;                            /* CTMR_E_INVAL by max_layers: the false positives of the last layer */
  ctmr_cascade_layer layer[CTMR_CASCADE_MAX_LAYERS];
} ctmr_cascade_info;
typedef struct {
  uint64_t probes, host_probes;  /* P's member records, P's host-section members */
  uint32_t layers, reserved;
} ctmr_cascade_query_info;
int ctmr_cascade_build(ctmr_engine* e, const uint8_t* revoked, size_t revoked_len, const uint8_t* known, size_t known_len,
                       int64_t now_unix, const ctmr_cascade_params* params, uint8_t* out, size_t out_cap, ctmr_cascade_info* info);
int ctmr_cascade_build_device(ctmr_engine* e, const uint8_t* r_meta, size_t r_meta_len, const void* d_r_members, uint64_t r_members,
                              const uint8_t* s_meta, size_t s_meta_len, const void* d_s_members, uint64_t s_members, int64_t now_unix,
                              const ctmr_cascade_params* params, void* d_out, size_t out_cap, ctmr_cascade_info* info);
int ctmr_cascade_query(ctmr_engine* e, const uint8_t* cascade, size_t cascade_len, const uint8_t* probes, size_t probes_len,
                       uint8_t* out, size_t out_cap, ctmr_cascade_query_info* info);
int ctmr_cascade_query_device(ctmr_engine* e, const void* d_cascade, size_t cascade_len, const uint8_t* p_meta, size_t p_meta_len,
                              const void* d_p_members, uint64_t p_members, void* d_out, uint64_t out_cap,
                              ctmr_cascade_query_info* info);

/* ---- the Redis protocol stream of an image v1: the SADD commands of every serials:: key and the EXPIREAT
 *      KnownCertificates.setExpiryFlag puts on it (storage/knowncertificates.go:98-104), as `redis-cli --pipe` loads them
 *      into the Redis of a reference deployment.  DESIGN.md §18.
 *
 * Keys.  Those of the image's set records and those of its host section, in ascending bytewise key order; a key that
 *   occurs in both sections is one key.  info.sets counts keys.
 * Per key, in this order: its member records in the image's order, in SADD commands of at most members_per_command
 *   members each; its host-section members in section order, in SADD commands of their own under the same cap; one
 *   EXPIREAT key <seconds>.  The call neither sorts nor deduplicates: a caller with an unsorted image normalises it
 *   first with ctmr_known_merge(CTMR_KNOWN_UNION, image, NULL).
 * Encoding.  A command is a RESP array of bulk strings: "*<argc>\r\n", then "$<len>\r\n<octets>\r\n" per argument
 *   (SADD, the key, the members; EXPIREAT, the key, the seconds in decimal).  Members are raw octets; an empty serial is
 *   "$0\r\n\r\n".
 * EXPIREAT seconds.  For a set record: hour × 3600, negative before 1970.  For a key of the host section alone: the
 *   first second of the date between "serials::" and the next "::", parsed as NewExpDate parses it (hour or day
 *   resolution); a key without a second "::", or with a date that does not parse, gets its SADD commands and no
 *   EXPIREAT — the reference would never have put a TTL on it.
 * members_per_command is 1..2^20; anything else is CTMR_E_INVAL.
 * Validation.  The meta is checked as ctmr_known_import checks it.  A set record whose hour lies outside the years
 *   0000..9999 cannot be spelled as a key: CTMR_E_INVAL.  On the device every record is checked for serial_len <= 40 and
 *   zero padding before the first text byte is written, and every working buffer is allocated before it too:
 *   CTMR_E_INVAL and CTMR_E_NOMEM leave the output as it was.
 * Sizing.  The two-call convention: a buffer that is too small gives CTMR_E_RANGE with *info filled and nothing
 *   written.  A caller can size without a first call: with n member records, `sets` set records, host_bytes octets of
 *   host section holding host_members members (all four in the image's header) the text is at most
 *     47 n + 95 (n / members_per_command + sets) + 112 sets + 2 host_bytes + 208 host_members   octets
 *   (n / members_per_command rounded down).
 * Read-only.  Nothing of the engine's state is read or changed (table, pair statistics, counters, host-side store,
 *   Bloom filter, ctmr_table_info), as for ctmr_known_sort; the issuers need not be registered; the operand is const
 *   and stays as it was.
 * The member records are read where they lie, twice (a count pass, then the pass that writes), in runs of whole sets of
 * at most 2^27 records.  ctmr_known_image_resp takes a whole image in host memory (its member section staged on the
 * device once); ctmr_known_image_resp_device takes the meta and the member records (device memory of this engine's
 * device, 16-byte aligned) apart and writes the text to device memory, the host section's commands copied into it at
 * their places.  Both return after the engine's stream has drained. */
typedef struct {
  uint64_t sets, members, host_members, commands, text_bytes;  /* keys; member records; host-section members; SADD + EXPIREAT */
} ctmr_known_resp_info;
int ctmr_known_image_resp(ctmr_engine* e, const uint8_t* image, size_t len, uint32_t members_per_command, uint8_t* text,
                          size_t text_cap, ctmr_known_resp_info* info);
int ctmr_known_image_resp_device(ctmr_engine* e, const uint8_t* meta, size_t meta_len, const void* d_members,
                                 uint64_t n_members, uint32_t members_per_command, void* d_text, size_t text_cap,
                                 ctmr_known_resp_info* info);

/* ---- a Redis protocol stream as it lies → an image v1: the inverse of ctmr_known_image_resp*.  What a reference
 *      deployment holds in its Redis (`redis-cli --rdb` replayed, a rewritten AOF without an RDB preamble, the stream
 *      ctmr_known_image_resp wrote) becomes member records on the device without one Python or host step per member.
 *      DESIGN.md §19.
 *
 * Grammar.  Zero or more commands back to back and nothing else.  A command is "*<N>\r\n" followed by N >= 1 bulk
 *   strings "$<L>\r\n<L octets>\r\n"; <N> and <L> are 1..10 decimal digits without sign or leading zero ("0" itself is
 *   allowed).  Argument 0 is the command's name in any ASCII case: SADD key member… (N >= 3), EXPIREAT / PEXPIREAT key time
 *   (N = 3) and SELECT db (N = 2); the last three are accepted and ignored — the image implies the expiry.  Everything
 *   else is CTMR_E_INVAL: another command, an inline command, a null bulk string, a missing CRLF, a truncated tail,
 *   trailing bytes; ctmr_last_error() names the byte offset where the device knows it.  Members are raw octets and may
 *   hold anything, "\r\n$3\r\n" included.
 * Which members.  A SADD whose key does not start with "serials::" is skipped (info.skipped_members counts its
 *   members).  Under a serials:: key a member of at most CTMR_MAX_SERIAL octets becomes a member record when the key
 *   spells an (hour, issuer digest) exactly as a set entry does — 68 octets, "YYYY-MM-DD-HH" of a real calendar date and an
 *   hour 00..23, the padded base64url of a 32-byte digest; every other (key, member) pair goes to the host section.
 * Result.  An image ctmr_known_import accepts, not necessarily canonical (the contract of ctmr_known_image_resp's
 *   operand): the issuers of the keys that have a member record, in digest order; one set per such key, in key order;
 *   the member records of a set in STREAM ORDER across all commands of its key, adjacent or not, repeats kept; the host
 *   section's pairs sorted, each once.  The call neither sorts nor deduplicates: ctmr_known_merge(CTMR_KNOWN_UNION,
 *   image, NULL) does.  An empty stream gives the empty image (64 B of meta).
 * Sizing.  The two-call convention: a buffer that is too small gives CTMR_E_RANGE with *info filled and nothing
 *   written.  A caller can bound the member records without a first call: at most len / 6, the shortest member being
 *   "$0\r\n\r\n".  The meta has NO linear bound in len — every host-section pair repeats its key —, so a caller sizes
 *   it by a first call (or generously: a stream written from an image has the meta of that image).
 * Length.  len >= 2^32 − 64 is CTMR_E_INVAL, decided before the first byte is read: a longer stream is split by the
 *   caller at a command start and the images joined with CTMR_KNOWN_UNION.
 * CTMR_E_INVAL and CTMR_E_NOMEM leave every output buffer as it was: all working memory is allocated, and the whole
 *   stream validated, before the first output byte.
 * Read-only.  Nothing of the engine's state is read or changed (table, pair statistics, counters, host-side store,
 *   Bloom filter, ctmr_table_info), as for ctmr_known_sort; the stream is const and no byte beyond len is read.
 * Cost.  The stream is read where it lies; token starts are found in parallel (a candidate test per byte, then the
 *   candidates no earlier one spans).  A member that contains a well-formed fake header which lands on a CRLF opens a
 *   conflict region that one lane resolves by walking it; the region is as long as the span the fake header claims,
 *   which a hostile stream can make the whole stream — slow then, not wrong.
 * ctmr_known_resp_image takes the stream in host memory (staged on the device once) and writes the whole image to host
 * memory; ctmr_known_resp_image_device takes it in device memory of this engine's device at ANY alignment, writes the
 * meta to host memory and the member records to device memory (16-byte aligned).  Both return after the engine's
 * stream has drained. */
typedef struct {
  uint64_t members;        /* member records (device section) */
  uint64_t sets;
  uint64_t host_members;   /* members of the host section */
  uint64_t meta_bytes;     /* header + issuers + sets + host section, padded to 64 */
  uint64_t image_bytes;    /* meta_bytes + 48 × members */
  uint32_t issuers, reserved;
  uint64_t commands;       /* commands of the stream, the ignored ones counted in */
  uint64_t skipped_members;  /* members of SADD commands under keys outside serials:: */
} ctmr_known_resp_image_info;
int ctmr_known_resp_image(ctmr_engine* e, const uint8_t* stream, size_t len, uint8_t* out, size_t cap,
                          ctmr_known_resp_image_info* info);
int ctmr_known_resp_image_device(ctmr_engine* e, const void* d_stream, size_t len, uint8_t* out_meta, size_t out_meta_cap,
                                 void* d_out, uint64_t out_members_cap, ctmr_known_resp_image_info* info);

/* ---- DER CertificateLists as they lie → a probe image: the revoked serials of every CRL as member records, which
 *      ctmr_known_image_find* takes as P.  The CRL distribution points of an issuer are what k_meta_new collects into the
 *      crl::<Issuer.ID> sets; this is the step between fetching those CRLs and asking which revoked serials are known.
 *      DESIGN.md §26.
 *
 * Input.  CRL k is crls[offsets[k], offsets[k + 1]); offsets is a HOST array u64[n_crls + 1] that ascends and is
 *   contiguous: offsets[0] == 0, offsets[n_crls] == len.  digests is a HOST array of n_crls × 32 octets: for each CRL the
 *   SHA-256 of its issuer's SubjectPublicKeyInfo, as ctmr_issuer_info gives it.  The CRL's issuer Name is not matched
 *   against anything: the caller knows the issuer from the crl:: set the URL came from.  n_crls = 0 with len = 0 gives
 *   the empty image.
 * Grammar of one CRL.  Binary DER, no PEM armour.
 *   Lengths.  Every length is definite and minimal: one octet below 128, 81 xx from 128, 82 xx xx from 256, 83 … from
 *     65 536, 84 … from 2^24.  Nothing else is a length (80, 81 7f, 82 00 80, 85 …).
 *   CertificateList = SEQUENCE { tbsCertList SEQUENCE, signatureAlgorithm SEQUENCE, signatureValue BIT STRING (03) },
 *     filling its slice exactly; a slice of 0 bytes is outside the grammar.
 *   tbsCertList holds, in this order and filling it exactly: optional INTEGER (02) version; SEQUENCE signature; SEQUENCE
 *     issuer; Time thisUpdate; optional Time nextUpdate; optional SEQUENCE revokedCertificates; optional [0] (A0)
 *     crlExtensions.  A Time is a TLV of tag 17 or 18.
 *   The contents of version, the two AlgorithmIdentifiers, issuer, the Times, crlExtensions and signatureValue are spanned
 *     by their lengths and NOT read: they may hold anything, a whole CRL included.
 *   revokedCertificates holds entries back to back, filling its value exactly; an empty value is accepted.  An entry is
 *     SEQUENCE { INTEGER userCertificate, Time revocationDate, optional SEQUENCE crlEntryExtensions }, filled exactly by
 *     those two or three TLVs.  The contents of the three are not read.
 *   Serial.  The content octets of userCertificate, raw, of any length from 0: the octets NewSerial keeps of a
 *     certificate's serial (a leading 00 stays, nothing is normalised), so a probe equals the member the map stored for
 *     the same certificate.
 *   Dates and reason codes are neither validated nor output.
 *   EVERYTHING ELSE fails the whole call with CTMR_E_INVAL and writes nothing: cinfo.bad_crl is the LOWEST-numbered CRL
 *     outside the grammar and cinfo.bad_offset the offset in `crls` of the first TLV of that CRL that is not what the
 *     grammar wants there (its tag octet; where a structure ends early, the offset at which the missing TLV would start;
 *     for trailing bytes, the first of them).  A CRL's outer TLVs are judged before its entries; inside
 *     revokedCertificates the offset is the start of the first entry that is not one — whatever is wrong inside it, and
 *     also when it would run past the end of the value.  ctmr_last_error() says the same in words.
 *   The offsets themselves are judged first, before a byte of `crls` is read: offsets[0] != 0 gives bad_crl 0 and
 *     bad_offset 0; offsets[k + 1] < offsets[k] gives bad_crl k and bad_offset offsets[k] (the lowest such k);
 *     offsets[n_crls] != len gives bad_crl n_crls and bad_offset len.
 * Result.  An image v1 that ctmr_known_import and ctmr_known_image_find* accept, not necessarily canonical: the issuers
 *   are the distinct digests that have at least one member record, in digest order; one set per such digest under exp
 *   hour 0 (a probe's hour is ignored), in key order — the order of the Issuer.ID text, which is not digest order; a
 *   set's member records in INPUT ORDER, CRL by CRL and entry by entry, repeats kept: the CRLs of one digest (shards of
 *   a partitioned CRL, or the same CRL twice) share a set.  A serial above CTMR_MAX_SERIAL octets becomes the host-section
 *   pair ("serials::1970-01-01-00::<Issuer.ID>", serial); the pairs are sorted, each once.  The call neither sorts nor
 *   deduplicates: ctmr_known_merge(CTMR_KNOWN_UNION, image, NULL) does.
 * Sizing.  The two-call convention of ctmr_known_resp_image*: a buffer that is too small gives CTMR_E_RANGE with *info
 *   and *cinfo filled and nothing written.  A caller can bound the member records without a first call: at most
 *   len / 6, the shortest entry being 30 04 02 00 17 00.  The meta is 64 + 56 × distinct digests + the host section,
 *   padded to 64.
 * Length.  len >= 2^32 − 64 is CTMR_E_INVAL, decided before the first byte is read: a larger collection is split
 *   between two CRLs and the images joined with CTMR_KNOWN_UNION.
 * CTMR_E_INVAL and CTMR_E_NOMEM leave every output buffer as it was: all working memory is allocated, and every CRL
 *   validated, before the first output byte.
 * Read-only.  Nothing of the engine's state is read or changed (table, pair statistics, counters, host-side store,
 *   Bloom filter, ctmr_table_info), as for ctmr_known_sort; the blob is const and no byte beyond len is read.
 * Cost.  The blob is read where it lies; entry starts are found in parallel (a candidate test per byte of a
 *   revokedCertificates value, then the candidates no earlier one spans).  A serial or an extension body that holds a
 *   well-formed fake entry opens a conflict region that one lane resolves by walking it, as in ctmr_known_resp_image.
 * ctmr_crl_probes takes the blob in host memory (staged on the device once) and writes the whole image to host memory;
 * ctmr_crl_probes_device takes it in device memory of this engine's device at ANY alignment, writes the meta to host
 * memory and the member records to device memory (16-byte aligned).  Both return after the engine's stream has drained. */
typedef struct {
  uint64_t crls;          /* n_crls */
  uint64_t entries;       /* revoked entries of all CRLs */
  uint64_t records;       /* … whose serial has at most CTMR_MAX_SERIAL octets: the member records */
  uint64_t host_members;  /* the host section's pairs: the DISTINCT (issuer, serial) among the other entries */
  uint64_t empty_crls;    /* CRLs without an entry: revokedCertificates absent or empty */
  uint64_t candidates;    /* entry candidates the mark pass found, the two frames per CRL counted in; candidates −
                             entries − frames = the fake entries the passes behind it threw out */
  uint64_t bad_crl;       /* on CTMR_E_INVAL from the grammar or the offsets: see above; else UINT64_MAX */
  uint64_t bad_offset;    /* … and its offset in `crls`; else UINT64_MAX */
} ctmr_crl_info;
int ctmr_crl_probes(ctmr_engine* e, const uint8_t* crls, size_t len, const uint64_t* offsets, uint32_t n_crls,
                    const uint8_t* digests, uint8_t* out, size_t cap, ctmr_known_image_info* info, ctmr_crl_info* cinfo);
int ctmr_crl_probes_device(ctmr_engine* e, const void* d_crls, uint64_t len, const uint64_t* offsets, uint32_t n_crls,
                           const uint8_t* digests, uint8_t* meta, size_t meta_cap, void* d_members, uint64_t members_cap,
                           ctmr_known_image_info* info, ctmr_crl_info* cinfo);

/* Every CRL judged on its own: ctmr_crl_probes* with a verdict per CRL instead of one for the call.  DESIGN.md §27.
 * Arguments as above, and verdicts, a HOST array [n_crls] that may be NULL (then nothing is lost but the verdicts: cinfo
 * still names the lowest bad CRL).  The grammar is exactly the one above, not a byte wider.
 * Return value.  A CRL outside the grammar fails nothing: the call returns CTMR_OK.
 *   verdicts[k].bad_offset = UINT64_MAX: CRL k is inside the grammar.  Any other value: it is outside, and the value is
 *   EXACT, not advisory: offsets[k] + the bad_offset ctmr_crl_probes* reports for CRL k submitted alone.  A CRL of 0 bytes
 *   is bad at offsets[k].  Nothing in a neighbour changes a CRL's verdict: the first byte of every CRL is the start of a
 *   frame no earlier token reaches past, so the rules above — the outer TLVs before the entries, inside
 *   revokedCertificates the start of the first entry that is not one — hold CRL by CRL.
 *   verdicts[k].records / .long_entries: the member records CRL k contributed, and its entries whose serials are above
 *   CTMR_MAX_SERIAL octets, counted before the host section makes them unique; both 0 for a bad CRL.  Over all k,
 *   the records sum to info.members and records + long_entries to cinfo.entries.
 * The image.  A bad CRL contributes nothing: meta and member records are byte for byte what ctmr_crl_probes* writes for
 *   the sub-sequence of good CRLs with their digests.  A digest whose every CRL is bad is not an issuer of the image; a bad
 *   shard leaves the good shards of its digest in input order; a long serial of a bad CRL — also of one that is bad
 *   only behind that entry — is not in the host section.  With no bad CRL every output of ctmr_crl_probes* is
 *   reproduced bit for bit.
 * cinfo.  crls is n_crls; entries, records, host_members and empty_crls count the good CRLs only; candidates is what
 *   the mark pass found over the whole blob, the bad CRLs' included; bad_crl / bad_offset name the LOWEST bad CRL and
 *   its verdict's offset, or are both UINT64_MAX.
 * What still fails the whole call, being no CRL's fault: the three errors of the offsets (CTMR_E_INVAL, cinfo as
 *   above), len >= 2^32 − 64, null arguments, CTMR_E_RANGE and CTMR_E_NOMEM.  Sizing is by the good CRLs, in the two-call
 *   convention above: CTMR_E_RANGE with *info and *cinfo filled.  On every error every output buffer, verdicts included,
 *   is as it was: verdicts is written last, behind the last thing that can fail.
 * Empty input.  n_crls > 0 with len == 0 says every CRL has 0 bytes: every verdict is bad at offset 0, the call returns
 *   CTMR_OK and the empty image, and nothing is launched.  n_crls = 0 gives the empty image and writes no verdict.
 * Cost.  That of ctmr_crl_probes*: the blob is read by the two mark passes once, however many CRLs are bad; a bad CRL's
 *   tokens are dropped behind them. */
typedef struct {
  uint64_t bad_offset;    /* UINT64_MAX: inside the grammar; else the offset in `crls`, see above */
  uint32_t records;       /* member records this CRL contributed (serials <= CTMR_MAX_SERIAL octets); 0 when bad */
  uint32_t long_entries;  /* its entries with longer serials, before the host section makes them unique; 0 when bad */
} ctmr_crl_verdict;       /* 16 bytes */
int ctmr_crl_probes_each(ctmr_engine* e, const uint8_t* crls, size_t len, const uint64_t* offsets, uint32_t n_crls,
                         const uint8_t* digests, uint8_t* out, size_t cap, ctmr_known_image_info* info, ctmr_crl_info* cinfo,
                         ctmr_crl_verdict* verdicts);
int ctmr_crl_probes_each_device(ctmr_engine* e, const void* d_crls, uint64_t len, const uint64_t* offsets, uint32_t n_crls,
                                const uint8_t* digests, uint8_t* meta, size_t meta_cap, void* d_members, uint64_t members_cap,
                                ctmr_known_image_info* info, ctmr_crl_info* cinfo, ctmr_crl_verdict* verdicts);

/* One rank's input of a multi-GPU round (ctmr_group_map_batch, ctmr_xchg_map_device): device pointers on that rank's
 * GPU, as ctmr_map_batch_device takes them; d_ends != NULL: an entry view (d_offsets = cert_start, d_ends = cert_end,
 * blob_bytes set).  order_base = log index of the shard's entry 0 (Bloom mode: the lowest order keeps WasUnknown; owner
 * mode derives the orders itself from the shards' sizes).  The shards of one Bloom round must cover order ranges
 * [order_base, order_base + n) that ASCEND WITH THE RANK AND DO NOT OVERLAP — log-index shards do —: two ranks presenting
 * the same new key under the same order would both keep WasUnknown.  ctmr_group_map_batch checks this over the whole
 * group in the round's opening control row and fails on every rank with CTMR_E_INVAL otherwise (a host that leaves every
 * order_base at 0 is told so, before anything is inserted). */
typedef struct {
  const uint8_t* d_payload;
  const uint64_t* d_offsets;
  const uint64_t* d_ends;       /* NULL = packed batch */
  const uint32_t* d_issuer_idx;
  const uint8_t* d_entry_type;  /* may be NULL */
  uint64_t n;
  uint64_t blob_bytes;          /* entry view only */
  uint64_t order_base;
  ctmr_record* d_records;
  uint64_t* d_new_idx;          /* may be NULL */
} ctmr_shard;

/* ---- cross-GPU global dedup, owner-computes: replaces the shared Redis set service
 *      (storage/rediscache.go:57-65: one SADD answers "was new" for every ct-fetch process) between shards.
 *      owner(key) = a hash of the key → [0, world).  One round on one rank is four calls; a multi-process host with its
 *      own transport puts its two all-to-alls between them (ctmr_group_map_batch does exactly that, natively):
 *   map:    maps the shard.  A key THIS rank owns is inserted on the spot by the map kernel (the fused path of
 *           ctmr_map_batch_device); a key another rank owns leaves as a 32-byte record (serials of 21..40 octets: a
 *           64-byte record).  ord_base = Σ n of the lower ranks in this round: the round's global log order, < 2^32 —
 *           among entries that bring the same new key in one round the lowest order keeps WasUnknown, as in the reference
 *           loop over one log.  counts32[w] (host) = 32-byte records for owner w; *n_long = 64-byte records (all owners).
 *   keys:   writes the records, partitioned by owner, ascending order inside a partition, into the caller's send
 *           buffers (Σ counts32 × 32 bytes; n_long × 64 bytes, counts64[w] of them for owner w).
 *   insert: the owner inserts what it received (any order of senders) into the round of its own shard and writes one byte
 *           per record: 1 = was unknown.  Bumps the owner's per-issuer counters (a key is counted where it is stored).
 *           Must be called once per round on every rank, received records or not: it also settles the rank's own shard.
 *   apply:  the sender's records left the map with CTMR_FL_WAS_UNKNOWN set; the returned bytes (same order as the
 *           records were sent) take it away from the entries whose key was known; compacts d_new_idx, fills stats.
 *   Every rank must have registered the same issuers in the same order.  Serials longer than CTMR_MAX_SERIAL are not
 *   exchanged by these per-rank steps (each rank's host-side set decides them for its shard); ctmr_group_map_batch
 *   settles them between the ranks at the end of the round.  shard.d_records is required. ---- */
int ctmr_xchg_map_device(ctmr_engine* e, const ctmr_shard* shard, uint32_t world, uint32_t rank, uint32_t ord_base,
                         uint64_t* counts32, uint64_t* n_long);
/* ctmr_xchg_map_device for entries [lo, hi) of the shard (lo a multiple of 1024; chunks in ascending order from 0, the
 * last ends at sh->n): map + this chunk's exported records gathered into d_keys32_out at once (per-owner partitions of the
 * chunk; counts32[w] of them for owner w).  After the last chunk the round stands as after ctmr_xchg_map_device;
 * ctmr_xchg_keys_device then delivers only the 64-byte records (*n_long, set by the last chunk). */
int ctmr_xchg_map_chunk_device(ctmr_engine* e, const ctmr_shard* sh, uint32_t world, uint32_t rank, uint32_t ord_base,
                               uint64_t lo, uint64_t hi, void* d_keys32_out, uint64_t* counts32, uint64_t* n_long);
int ctmr_xchg_keys_device(ctmr_engine* e, void* d_keys32_out, void* d_keys64_out, uint64_t* counts64);
int ctmr_xchg_insert_device(ctmr_engine* e, const void* d_keys32, uint64_t n32, const void* d_keys64, uint64_t n64,
                            uint8_t* d_flags32, uint8_t* d_flags64);
int ctmr_xchg_apply_device(ctmr_engine* e, const void* d_sent32, const uint8_t* d_flags32, uint64_t n32,
                           const void* d_sent64, const uint8_t* d_flags64, uint64_t n64, ctmr_batch_stats* stats);

/* ---- cross-GPU global dedup, Bloom pre-filter variant (the "all-gather of per-GPU Bloom fingerprints" of
 *      BASELINE.json's north_star) — exact, same results as the owner-computes exchange above.
 *      Every rank keeps its own known-certificate table (plain ctmr_map_*_device calls) plus a cumulative Bloom
 *      filter of the keys it found locally new.  One round = one map call per rank, then:
 *   add:    makes sure the filter holds the batch's CTMR_FL_WAS_UNKNOWN keys and opens the round.  Since ABI v4 an engine
 *           with a filter adds to it INSIDE the map kernel, so for the batch the engine mapped last this costs nothing
 *           (ctmr_set_insert sets the bits of its member too: every key a rank holds is in its filter).  The host all-gathers the filters
 *           (ctmr_bloom_device gives the pointer; n_words × 8 bytes per rank, rank-major in the gathered buffer).
 *   probe:  tests the batch's locally-new keys against the OTHER ranks' filters and writes one 64-byte key record per
 *           (key, peer whose filter holds it) into d_keys_out, partitioned by peer, ascending log index inside a
 *           partition; counts[p] (host) = records for peer p.  A key that hits no peer filter is on no other rank and
 *           is not exchanged at all.  order_base = global order of entry 0 of this rank's batch (its log index):
 *           between ranks that meet the same key in the same round the LOWEST order keeps WasUnknown.  When more
 *           than keys_cap records are needed: CTMR_E_RANGE, counts[] filled, nothing written — call again.
 *   lookup: the peer looks the received records up in its table (exact, read-only) and writes one byte per record:
 *           1 = known here before the asker's entry (since an earlier round, or this round under a lower order).
 *           order_base as given to this rank's own probe.
 *   apply:  the asker clears CTMR_FL_WAS_UNKNOWN of every flagged entry (once per entry), takes it out of its
 *           per-issuer count, marks the key's slot as counted elsewhere (it stays known for dedup, but is left out of
 *           SetCardinality / SetList / the per-issuer counts, so that sums over ranks are the global values),
 *           compacts new_idx and fills stats.  d_records must be the records of this engine's LAST map call (the
 *           round continues it: only the entries that lose the flag are touched).
 *   d_ends NULL = packed batch (d_offsets has n+1 entries); otherwise entry-view ranges (ctmr_entry_view).
 *   d_records NULL = the engine's own records of the last map call.  Same issuers in the same order on every rank.
 *   Serials longer than CTMR_MAX_SERIAL: as above (settled between the ranks by ctmr_group_map_batch). ---- */
/* bits: power of two, 2^12..2^40, ≈16 per key this rank will ever hold.  d_words NULL: the library allocates the
 * filter; otherwise a caller-owned device buffer of bits/8 bytes (e.g. this rank's row of the all-gather buffer),
 * zeroed by the call, which must outlive the engine's use of it.  Same size on every rank. */
int ctmr_bloom_config(ctmr_engine* e, uint64_t bits, void* d_words);
int ctmr_bloom_device(ctmr_engine* e, void** d_words, uint64_t* n_words);
int ctmr_bloom_add_device(ctmr_engine* e, const uint8_t* d_payload, const uint64_t* d_offsets, const uint64_t* d_ends,
                          uint64_t n, const ctmr_record* d_records);
int ctmr_bloom_probe_device(ctmr_engine* e, const uint8_t* d_payload, const uint64_t* d_offsets,
                            const uint64_t* d_ends, uint64_t n, const ctmr_record* d_records, const void* d_filters,
                            uint32_t world, uint32_t rank, uint64_t order_base, void* d_keys_out, uint64_t keys_cap,
                            uint64_t* counts);
int ctmr_bloom_lookup_device(ctmr_engine* e, const void* d_keys, uint64_t n_keys, uint64_t order_base,
                             uint8_t* d_flags);
int ctmr_bloom_apply_device(ctmr_engine* e, ctmr_record* d_records, uint64_t n, const void* d_keys_sent,
                            const uint8_t* d_flags, uint64_t n_keys, uint64_t* d_new_idx, ctmr_batch_stats* stats);

/* ---- multi-GPU groups: the shared set service of a sharded deployment, natively behind this ABI.  Replaces what one
 *      Redis server gives N ct-fetch processes that split a log by -offset/-limit (cmd/ct-fetch/ct-fetch.go:288-305;
 *      storage/rediscache.go:21-65: SADD answers "was new" for all of them).  A group has `world` ranks, each an
 *      engine on one GPU that maps the entries of its log-index shard; one ctmr_group_map_batch call per round runs the
 *      shard maps AND the exchange that makes the dedup global; ctmr_group_issuer_counts is the all-reduce of the
 *      per-issuer counts.  Two transports, the same per-rank kernels in the same order:
 *        ctmr_group_create_local  every rank lives in this process (one engine per device — a single host process
 *                                 driving the node's GPUs — or several engines on one device): device-to-device copies
 *        ctmr_group_create_rccl   one process per GPU: RCCL over xGMI (ncclSend/ncclRecv all-to-all, ncclAllGather of
 *                                 the Bloom filters, ncclAllReduce of the counts); librccl is loaded on demand.
 *                                 id = the bytes ctmr_group_unique_id produced on one rank, handed to the others by the
 *                                 host over any channel it has.
 *      Engines must have registered the same issuers in the same order (key records carry canonical issuer indices);
 *      they stay usable on their own; destroy the group before its engines.
 *   modes   CTMR_DEDUP_LOCAL  shard-local dedup only (exact when no key spans two shards: BASELINE config 4)
 *           CTMR_DEDUP_OWNER  owner-computes key exchange (ctmr_xchg_* above): map (+ insert of the keys the rank owns)
 *                             → key records all-to-all → owner insert → flags back → apply.  Every key is stored once,
 *                             on its owner.
 *           CTMR_DEDUP_BLOOM  all-gather of per-GPU Bloom filters as an exact pre-filter (ctmr_bloom_* above; needs
 *                             ctmr_group_bloom_config): local insert → filter all-gather → probe → key records only to
 *                             the peers whose filter matched → exact lookup → flags back → apply
 *           Both exact modes also settle the members with serials longer than CTMR_MAX_SERIAL (host-side sets) between
 *           the ranks at the end of a round: the lists of such members added in the round are all-gathered with the
 *           closing status row, a member some rank held before is known to every rank, otherwise the lowest log index
 *           keeps it — stored once, like every other key.  A round without such members pays nothing for it.
 *   shards  one ctmr_shard (above) per LOCAL rank, rank order.  Ranks hold CONTIGUOUS log-index ranges in rank order
 *           (rank r's entries all precede rank r+1's: ct-fetch's -offset/-limit split).  d_records is required in the
 *           OWNER and BLOOM modes.  stats: one per local rank (may be NULL).
 *   errors  an exact round opens with a control row (status, mode, filter size, order range of every rank): a call a rank
 *           must refuse — unknown mode, another mode than the group's, no filter configured, a bad shard, ranks that
 *           disagree about any of these — fails THERE, on every rank together and before anything is inserted.  A rank
 *           that fails later keeps taking part in the round's collectives (its peers would block for ever otherwise)
 *           and every rank's call returns the error at the end; the sets of a round that failed after its opening row
 *           are unspecified — destroy the group. ---- */
typedef struct ctmr_group ctmr_group;
#define CTMR_GROUP_ID_BYTES 128
enum { CTMR_DEDUP_LOCAL = 0, CTMR_DEDUP_OWNER = 1, CTMR_DEDUP_BLOOM = 2 };
enum { CTMR_TRANSPORT_LOCAL = 0, CTMR_TRANSPORT_RCCL = 1 };
typedef struct {
  uint32_t world, n_local, transport, first_local_rank;
  /* what the last ctmr_group_map_batch moved between ranks, summed over the local ranks */
  uint64_t keys_sent, keys_received;   /* key records to / from OTHER ranks */
  uint64_t filter_bytes_received;      /* Bloom mode: the peers' filters, per local rank */
  uint64_t wire_bytes_sent;            /* every byte handed to the transport for another rank: key records (32 B; 64 B for
                                          Bloom candidates and 21..40-octet serials), flag bytes, filters */
  /* wall time of the last round's phases on this process, ms (each phase ends with the ranks' streams drained):
   * [0] map (+ the insert of locally owned keys, + filter add)  [1] key export / filter all-gather + probe
   * [2] key records all-to-all  [3] owner insert / exact lookup (+ this shard's resolve)  [4] flags all-to-all
   * [5] apply + NEW-list compaction  [6] the control collectives (counts, status)
   * [7] NOT a time: how often the round drained a stream on the host (ABI v7) — every control row, every all-to-all and
   *     every phase boundary is one; with RCCL each is a latency no kernel hides */
  float ms_phase[8];
} ctmr_group_stats;
int ctmr_group_create_local(ctmr_engine* const* engines, uint32_t n, ctmr_group** out);
int ctmr_group_unique_id(uint8_t id[CTMR_GROUP_ID_BYTES]);
int ctmr_group_create_rccl(ctmr_engine* engine, const uint8_t id[CTMR_GROUP_ID_BYTES], uint32_t rank, uint32_t world,
                           ctmr_group** out);
void ctmr_group_destroy(ctmr_group* g);
const char* ctmr_group_last_error(const ctmr_group* g);
int ctmr_group_info(ctmr_group* g, ctmr_group_stats* out);
/* Owner-computes rounds map every shard in `chunks` pieces (1..64; default 1 = as one): the key records of chunk c travel on
 * a second stream per rank while chunk c + 1 is being walked, and the owner-side insert, the bytes back and the apply run
 * once at the end over everything.  Results are those of the unchunked round, entry for entry (inside one round the order
 * in which keys reach their owner does not matter: storage/rediscache.go:57-65 answers per key, not per batch).  Costs one
 * small control collective per chunk and exchange buffers sized for the worst case.  Every rank of the group sets the same
 * value (checked in the round's opening control row); Bloom and LOCAL rounds ignore it.  With chunks > 1 on an RCCL group
 * the call is COLLECTIVE (ABI v7): it makes the transfer streams and the second communicator the chunk transfers run on —
 * every rank calls it, with the same count; a rank-local failure fails every rank's call together. */
int ctmr_group_set_chunks(ctmr_group* g, uint32_t chunks);
/* bits per rank: power of two, ≈16 per key a rank will ever hold; same on every rank.  (A group of ONE rank has no peer
 * to ask: it keeps no filter and its Bloom rounds are the plain reduce.)  * One mode per group: the first round's mode is the only one the group accepts afterwards (CTMR_E_INVAL otherwise) — the
 * modes keep a key in different places and cannot see each other's.
 */
int ctmr_group_bloom_config(ctmr_group* g, uint64_t bits);
int ctmr_group_map_batch(ctmr_group* g, int mode, const ctmr_shard* shards, ctmr_batch_stats* stats);
/* Σ over ALL ranks of ctmr_issuer_counts / ctmr_total_count (storage-statistics.go:44-53 over the whole deployment):
 * the ncclAllReduce of the per-issuer count vector in the RCCL transport. */
int ctmr_group_issuer_counts(ctmr_group* g, uint64_t* out, uint32_t n);
int ctmr_group_total_count(ctmr_group* g, uint64_t* out);
/* Sum (op_max = 0) or maximum (1) over the ranks of n host-side u64 values, in place, and a barrier: what a
 * multi-process host needs besides the data path (the round's global NEW count, the slowest rank's time) without a
 * second communication library.  No-ops for a local group (the caller holds every rank's values). */
int ctmr_group_all_reduce_u64(ctmr_group* g, uint64_t* values, uint32_t n, int op_max);
int ctmr_group_barrier(ctmr_group* g);

/* ---- PEM write-back: replaces pem.EncodeToMemory(&pem.Block{Type: "CERTIFICATE",
 *      Bytes: aCert.Raw}) of FilesystemDatabase.Store (storage/filesystemdatabase.go:167-175,196-200); the host
 *      hands each PEM to StorageBackend.StoreCertificatePEM (storage/localdiskbackend.go:194-199).
 *   device variant: d_idx = n_idx entry indices (e.g. the new_idx list of ctmr_map_batch_device); PEM r is written
 *           at d_pem + d_pem_offsets[r]; d_pem_offsets has n_idx+1 slots; *pem_bytes = total.  With d_pem == NULL
 *           only the offsets and the total are produced (size query).
 *   ctmr_pem_new: PEM of every CTMR_FL_WAS_UNKNOWN entry of the LAST ctmr_map_batch (host variant, called with
 *           new_idx != NULL), ascending entry order; *need = bytes required (CTMR_E_RANGE when cap is smaller),
 *           *count = number of PEMs, pem_offsets = count+1 offsets into out (may be NULL). ---- */
int ctmr_pem_encode_device(ctmr_engine* e, const uint8_t* d_payload, const uint64_t* d_offsets,
                           const uint64_t* d_idx, uint64_t n_idx, uint8_t* d_pem, uint64_t pem_cap,
                           uint64_t* d_pem_offsets, uint64_t* pem_bytes);
int ctmr_pem_new(ctmr_engine* e, uint8_t* out, size_t cap, uint64_t* pem_offsets, size_t* need, uint64_t* count);
/* The device variant over an entry view (raw get-entries batches): certificate i is [cert_start[i], cert_end[i]) of
 * d_blob.  Declared behind ctmr_entry_view below. */

/* ---- CT get-entries leaf decode: replaces ct.LogEntryFromLeaf
 *      (cmd/ct-fetch/ct-fetch.go:452; RFC 6962 §3.4 MerkleTreeLeaf, §4.6 extra_data) and insertCTWorker's choice of
 *      certificate and issuer (:198-204 X509Cert | Precert.Submitted.Data; :215 len(Chain) < 1; :221 Chain[0]).
 *   raw entries: ONE blob holding, back to back, leaf_input_0 ‖ extra_data_0 ‖ leaf_input_1 ‖ extra_data_1 ‖ … (the
 *           base64-decoded "leaf_input"/"extra_data" members of get-entries); bounds u64[2n+1]: leaf_input_i =
 *           [bounds[2i], bounds[2i+1]), extra_data_i = [bounds[2i+1], bounds[2i+2]).  The blob is 16-byte aligned
 *           with CTMR_PAYLOAD_PAD readable bytes behind bounds[2n] (device inputs).
 *   decode: per entry the byte range of the certificate the map parses (inside the blob — nothing is copied), the
 *           entry type, the timestamp and the index of Chain[0] in the issuer table.  Chain[0] is matched bytewise
 *           against the certificates registered so far; one that is not registered yet is registered by the call
 *           (exactly what ctmr_add_issuers does), so a host that feeds raw entries never manages the issuer table.
 *           An entry ct.LogEntryFromLeaf would reject gets entry_type CTMR_ENTRY_INVALID.
 *   map_view: the batched map + reduce of ctmr_map_batch_device over such a view (certificates addressed by
 *           [cert_start, cert_end) instead of n+1 packed offsets).
 *           The ranges of a view may lie in the blob in ANY order — descending, permuted, with gaps, several entries
 *           on one range, empty ones — and the result is exact and that of the packed batch in ENTRY order (the first entry
 *           carrying a key is the unknown one).  The same holds for every call that takes offsets + ends.  Ascending
 *           cert_start is the FAST path: a wave of 64 entries reads through one descriptor based on its first entry's
 *           certificate, and an entry whose certificate lies below that one (or 0x7e000000 bytes or more beyond it) is read
 *           lane by lane and, by the default kernel, walked twice.
 *   map_entries: decode + map_view in one call; host variant stages the blob through the engine's buffers. ---- */
typedef struct {
  uint64_t* cert_start;   /* n: first byte of the certificate inside the blob */
  uint64_t* cert_end;     /* n: one past its last byte */
  uint32_t* issuer_idx;   /* n: issuer table index of Chain[0]; CTMR_NO_ISSUER when len(Chain) < 1 */
  uint8_t* entry_type;    /* n: 0 X509LogEntryType, 1 PrecertLogEntryType, CTMR_ENTRY_INVALID */
  uint64_t* timestamp;    /* n or NULL: TimestampedEntry.Timestamp, ms since the epoch (ct-fetch.go:476) */
  uint64_t* chain0_start; /* n or NULL: Chain[0].Data inside the blob */
  uint32_t* chain0_len;   /* n or NULL: 0 when len(Chain) < 1 */
} ctmr_entry_view;

typedef struct {
  uint64_t n;
  uint64_t n_x509, n_precert, n_decode_error;
  uint64_t n_no_chain;        /* decoded entries with len(Chain) < 1 */
  uint64_t n_issuers_added;   /* distinct Chain[0] certificates this call registered */
  uint64_t blob_bytes;        /* bounds[2n] - bounds[0] */
  float ms_decode, ms_match;  /* filled when config.profile; decode and the first match round run as one kernel: ms_match = both;
                                 ms_decode = what runs in front of it: strict_leaf's TBSCertificate walk (k_leaf_tbs_check), else ≈ 0 */
} ctmr_decode_stats;

int ctmr_decode_entries_device(ctmr_engine* e, const uint8_t* d_blob, const uint64_t* d_bounds, uint64_t n,
                               const ctmr_entry_view* d_view, ctmr_decode_stats* stats);
int ctmr_map_view_device(ctmr_engine* e, const uint8_t* d_blob, uint64_t blob_bytes, const ctmr_entry_view* d_view,
                         uint64_t n, ctmr_record* d_records, uint64_t* d_new_idx, ctmr_batch_stats* stats);
int ctmr_map_entries_device(ctmr_engine* e, const uint8_t* d_blob, const uint64_t* d_bounds, uint64_t n,
                            ctmr_record* d_records, uint64_t* d_new_idx, uint64_t* d_timestamp,
                            ctmr_decode_stats* dstats, ctmr_batch_stats* stats);
int ctmr_map_entries(ctmr_engine* e, const uint8_t* blob, const uint64_t* bounds, uint64_t n, ctmr_record* records,
                     uint64_t* new_idx, uint64_t* timestamp, ctmr_decode_stats* dstats, ctmr_batch_stats* stats);

/* ---- get-entries HTTP bodies as they lie → a raw-entry batch: what the reference's downloader holds before CT-go's
 *      GetRawEntries has run encoding/json and encoding/base64 over it, one entry at a time (ct-fetch.go:424-452).
 *      The JSON is tokenised, checked and its base64 decoded on the device.  DESIGN.md §20.
 *
 * Input.  Response r is text[resp_bounds[r], resp_bounds[r + 1]); resp_bounds is a HOST array u64[n_responses + 1],
 *   ascending: several bodies lie in one buffer, as a downloader collects them.  No byte outside the bounds decides
 *   anything.  n_responses = 0 gives the empty batch.
 * Grammar of one response (ws: any run of the bytes 0x20 0x09 0x0A 0x0D):
 *       ws { ws "entries" ws : ws [ ws ( entry ( ws , ws entry )* )? ws ] ws } ws
 *       entry = { ws K ws : ws V ws , ws K' ws : ws V ws }
 *   {K, K'} = {"leaf_input", "extra_data"} in either order, each exactly once, spelled exactly.  V = '"' b64 '"': zero or
 *   more characters of A-Z a-z 0-9 + /, the total length a multiple of 4, the last quantum may end in "=" or "==";
 *   the bits left over in a padded quantum may hold any value and are dropped (as Go's non-strict StdEncoding and
 *   Python's b64decode do).  {"entries":[]} is a valid response of no entries.  The string state starts afresh at
 *   every response boundary: a body that ends inside a string is invalid whatever the next body begins with.
 *   EVERYTHING ELSE is outside the grammar and fails the call with CTMR_E_INVAL, info.bad_response naming the lowest
 *   such response: a backslash anywhere (so the escapes \/ and \u0041, which JSON allows); any other key, a repeated key, a key
 *   in another letter case; a value that is not such a string; a trailing comma; bytes behind the closing brace other
 *   than ws; a byte-order mark; an empty or all-ws body; an unpadded or URL-safe alphabet.
 *   This is the language CT log servers emit, NOT all of what encoding/json would accept into ct.GetEntriesResponse:
 *   Go's decoder matches keys case-insensitively, ignores unknown keys and resolves escapes.  The host keeps its own
 *   decoder for a response named in bad_response.  Like the rest of the CT-go boundary this is recalled, not pinned
 *   (DESIGN.md §2).
 * Output.  blob = leaf_input_0 ‖ extra_data_0 ‖ leaf_input_1 ‖ … and bounds u64[2n + 1], exactly ctmr_map_entries*'
 *   input: always leaf first, then extra, whatever their order in the text, back to back, bounds[0] = 0; the
 *   CTMR_PAYLOAD_PAD bytes behind bounds[2n] are zeroed, so the output is a valid raw-entry batch as it stands.
 *   resp_first is a HOST array u64[n_responses + 1] or NULL: the index of each response's first entry
 *   (resp_first[n_responses] = n), which is how the host maps entries back to log indices.
 * Sizing.  The two-call convention: a blob_cap below blob_bytes + CTMR_PAYLOAD_PAD or an entries_cap below entries
 *   gives CTMR_E_RANGE with *info filled and nothing written.  Bounds a caller may use without a first call:
 *   blob_bytes <= 3/4 text_bytes, entries <= text_bytes / 34.
 * CTMR_E_INVAL and CTMR_E_NOMEM leave every output buffer as it was: all working memory is allocated, and the whole
 *   text validated, before the first output byte.  Every position is 64-bit: a text of 2^32 bytes and more is one call
 *   (the working tables are about 6 % of a text of 4 KB entries, so no run-splitting is imposed on the caller).
 * Read-only.  Nothing of the engine's state is read or changed; the text is const.
 * ctmr_entries_json takes the text in host memory (the bytes inside the bounds staged on the device once) and writes
 * blob and bounds to host memory; ctmr_entries_json_device takes the text in device memory of this engine's device at
 * ANY alignment and writes d_blob (16-byte aligned) and d_bounds on the device.  Both return after the engine's stream
 * has drained. */
typedef struct {
  uint64_t responses, entries;
  uint64_t text_bytes;      /* resp_bounds[R] - resp_bounds[0] */
  uint64_t blob_bytes;      /* bounds[2n]; the call needs blob_bytes + CTMR_PAYLOAD_PAD of capacity */
  uint64_t bad_response;    /* on CTMR_E_INVAL: the LOWEST-numbered response outside the grammar; else UINT64_MAX */
  uint64_t bad_offset;      /* on CTMR_E_INVAL: a byte offset inside that response's bounds (advisory) */
} ctmr_entries_json_info;
int ctmr_entries_json(ctmr_engine* e, const uint8_t* text, const uint64_t* resp_bounds, uint64_t n_responses,
                      uint8_t* blob, size_t blob_cap, uint64_t* bounds, uint64_t entries_cap, uint64_t* resp_first,
                      ctmr_entries_json_info* info);
int ctmr_entries_json_device(ctmr_engine* e, const void* d_text, const uint64_t* resp_bounds, uint64_t n_responses,
                             void* d_blob, size_t blob_cap, uint64_t* d_bounds, uint64_t entries_cap,
                             uint64_t* resp_first, ctmr_entries_json_info* info);

/* Every body judged on its own: ctmr_entries_json* with a verdict per response instead of one for the call.  DESIGN.md §22.
 * Arguments as above, and resp_bad, a HOST array u64[n_responses], required (NULL: CTMR_E_INVAL).  The grammar is
 * exactly the one above, not a byte wider.
 *   resp_bad[r] = UINT64_MAX: body r is inside the grammar.  Any other value: it is outside, and the value is an
 *   advisory byte offset in [resp_bounds[r], max(resp_bounds[r + 1], resp_bounds[r] + 1)).
 * A body outside the grammar fails nothing and contributes no entries: resp_first[r + 1] == resp_first[r] for it, the
 *   call returns CTMR_OK, info.bad_response / info.bad_offset name the LOWEST such body (UINT64_MAX: none), and
 *   info.entries / info.blob_bytes count the other bodies only.  blob, bounds, entries and blob_bytes are byte for byte
 *   what ctmr_entries_json* returns for the sub-sequence of good bodies; with no bad body every output of
 *   ctmr_entries_json* is reproduced bit for bit.  The host decodes the bodies named in resp_bad itself and nothing is
 *   handed over twice.
 * n_responses = 0, bodies that are all empty and a single empty body give CTMR_OK, the verdicts (an empty body is
 *   outside the grammar, its offset resp_bounds[r]) and the empty batch.
 * Sizing is by the good bodies: CTMR_E_RANGE as above, with *info filled.  CTMR_E_RANGE, CTMR_E_NOMEM and argument
 *   errors leave every output buffer, resp_bad included, as it was. */
int ctmr_entries_json_each(ctmr_engine* e, const uint8_t* text, const uint64_t* resp_bounds, uint64_t n_responses,
                           uint8_t* blob, size_t blob_cap, uint64_t* bounds, uint64_t entries_cap, uint64_t* resp_first,
                           uint64_t* resp_bad, ctmr_entries_json_info* info);
int ctmr_entries_json_each_device(ctmr_engine* e, const void* d_text, const uint64_t* resp_bounds, uint64_t n_responses,
                                  void* d_blob, size_t blob_cap, uint64_t* d_bounds, uint64_t entries_cap,
                                  uint64_t* resp_first, uint64_t* resp_bad, ctmr_entries_json_info* info);

/* ---- PEM certificate files as they lie → a packed batch: what LocalDiskBackend.StoreCertificatePEM wrote
 *      (storage/filesystemdatabase.go:167-201, storage/localdiskbackend.go:194-199) read back without encoding/pem and
 *      encoding/base64 on a host core: the inverse of ctmr_pem_new / ctmr_pem_encode_device.  The armor lines are found,
 *      the grammar checked and the base64 decoded on the device.  DESIGN.md §21.
 *
 * Input.  File f is text[file_bounds[f], file_bounds[f + 1]); file_bounds is a HOST array u64[n_files + 1], ascending.
 *   No byte outside the bounds decides anything, and the state starts afresh at every file boundary.  n_files = 0 gives
 *   the empty batch.  ws = 0x20 0x09 0x0D 0x0A; blank = 0x20 0x09 0x0D.
 *       file  = gap ( block gap )*              gap = zero or more ws bytes
 *       block = BEGIN body END
 *       BEGIN = "-----BEGIN CERTIFICATE-----" blank* LF    its first dash is the file's first byte or follows an LF
 *       body  = any run of ws and of the characters A-Z a-z 0-9 + / =
 *       END   = "-----END CERTIFICATE-----" blank* ( LF | end of file )    its first dash follows an LF
 *   The body's non-ws characters are its base64 text: their count is a multiple of 4; '=' occurs only as the last one or
 *   the last two of them; ws may lie anywhere between them, inside a quantum and between the two pads included; the
 *   spare bits of a padded quantum may hold any value and are dropped (the rule of ctmr_entries_json).  A body with no
 *   characters is a certificate of 0 bytes: the map will call it a parse error, the decoder does not.  A file of ws
 *   only, or of 0 bytes, holds no certificates and is valid.
 *   EVERYTHING ELSE is outside the grammar and fails the call with CTMR_E_INVAL, info.bad_file naming the LOWEST such
 *   file and info.bad_offset an advisory byte offset inside it: a '-' that is not part of such an armor line (4 or 6
 *   dashes, a dash inside a body, the URL-safe alphabet); any other block type (X509 CRL, TRUSTED CERTIFICATE, another
 *   letter case); a "Key: value" header line; any byte that is neither ws nor part of a block (a "# Label:" comment,
 *   OpenSSL's "subject=" lines, a byte-order mark, NUL, a byte >= 0x80); a BEGIN without END, an END without BEGIN, two
 *   BEGINs; a non-blank byte behind the closing dashes; a BEGIN not at a line start; a character count that is not a
 *   multiple of 4, a '=' followed by an alphabet character, three '=', an unpadded last quantum.
 *   This is a subset of what encoding/pem takes: Go's  for { block, rest = pem.Decode(rest) }  skips text between blocks
 *   and blocks that fail, and parses headers.  For every file inside this grammar it yields the same blocks — Type
 *   CERTIFICATE, no headers, the same bytes.  The host keeps its own decoder for a file named in bad_file.  Like the
 *   rest of the Go boundary this is recalled, not pinned.
 * Output.  payload = DER_0 ‖ DER_1 ‖ … back to back in text order and offsets u64[n + 1], offsets[0] = 0: exactly
 *   ctmr_map_batch*' input; the CTMR_PAYLOAD_PAD bytes behind offsets[n] are zeroed, so the output is a valid packed
 *   payload as it stands.  file_first is a HOST array u64[n_files + 1] or NULL: the index of each file's first
 *   certificate, file_first[n_files] = n.
 * Sizing.  The two-call convention: a payload_cap below payload_bytes + CTMR_PAYLOAD_PAD or a certs_cap below
 *   certificates gives CTMR_E_RANGE with *info filled and nothing written.  Bounds a caller may use without a first
 *   call: payload_bytes <= 3/4 text_bytes, and certificates <= (text_bytes + n_files) / 54 — a block takes its two
 *   armor lines, 27 + 25 bytes, the LF behind BEGIN and the LF in front of the next BEGIN, 54 in all; only the last
 *   block of a file may end with the file and save that LF, one byte per file.
 * CTMR_E_INVAL and CTMR_E_NOMEM leave every output buffer as it was: all working memory is allocated, and the whole
 *   text validated, before the first output byte.  Every position is 64-bit: a text of 2^32 bytes and more is one call.
 * info.regular / info.irregular say how the blocks were read.  A block is regular when its body is lines of one length
 *   L (a multiple of 4, at most 1024 when there are two lines or more; the last line may be shorter), every line ended
 *   by the same eol, LF or CR LF, with no other ws in the body, and at most 1024 blanks stand behind BEGIN's dashes:
 *   what pem.EncodeToMemory, ctmr_pem_new and OpenSSL write.  Its base64 is decoded from the text where it lies.  A
 *   body of no characters is regular.  Every other block of the grammar is irregular: its characters are first copied
 *   together into working memory.  The result is the same.
 * Read-only.  Nothing of the engine's state is read or changed; the text is const.
 * ctmr_pem_decode takes the text in host memory (the bytes inside the bounds staged on the device once) and writes
 * payload, offsets to host memory; ctmr_pem_decode_device takes the text in device memory of this engine's device at
 * ANY alignment and writes d_payload (16-byte aligned) and d_offsets on the device.  Both return after the engine's
 * stream has drained. */
typedef struct {
  uint64_t files, certificates;
  uint64_t text_bytes;      /* file_bounds[F] - file_bounds[0] */
  uint64_t payload_bytes;   /* offsets[n]; the call needs payload_bytes + CTMR_PAYLOAD_PAD of capacity */
  uint64_t regular;         /* blocks decoded from the text where it lies */
  uint64_t irregular;       /* blocks decoded through the squeezed copy */
  uint64_t bad_file;        /* on CTMR_E_INVAL: the LOWEST-numbered file outside the grammar; else UINT64_MAX */
  uint64_t bad_offset;      /* on CTMR_E_INVAL: a byte offset inside that file's bounds (advisory); else UINT64_MAX */
} ctmr_pem_decode_info;
int ctmr_pem_decode(ctmr_engine* e, const uint8_t* text, const uint64_t* file_bounds, uint64_t n_files,
                    uint8_t* payload, size_t payload_cap, uint64_t* offsets, uint64_t certs_cap, uint64_t* file_first,
                    ctmr_pem_decode_info* info);
int ctmr_pem_decode_device(ctmr_engine* e, const void* d_text, const uint64_t* file_bounds, uint64_t n_files,
                           void* d_payload, size_t payload_cap, uint64_t* d_offsets, uint64_t certs_cap,
                           uint64_t* file_first, ctmr_pem_decode_info* info);

/* Every file judged on its own: ctmr_pem_decode* with a verdict per file instead of one for the call.  DESIGN.md §23.
 * Arguments as above, and file_bad, a HOST array u64[n_files], required (NULL: CTMR_E_INVAL).  The grammar is exactly
 * the one above, not a byte wider.
 *   file_bad[f] = UINT64_MAX: file f is inside the grammar.  Any other value: it is outside, and the value is an advisory
 *   byte offset in [file_bounds[f], file_bounds[f + 1]).  A file of ws only, or of 0 bytes, is valid here as above.  The
 *   verdict of file f is what ctmr_pem_decode says of that file alone: nothing in a neighbour changes it.
 * A file outside the grammar fails nothing and contributes no certificates: file_first[f + 1] == file_first[f] for it, the
 *   call returns CTMR_OK, info.bad_file / info.bad_offset name the LOWEST such file (UINT64_MAX: none), and
 *   info.certificates, payload_bytes, regular and irregular count the other files only.  payload, offsets, certificates
 *   and payload_bytes are byte for byte what ctmr_pem_decode* returns for the sub-sequence of good files, the zeroed
 *   CTMR_PAYLOAD_PAD included; with no bad file every output of ctmr_pem_decode* is reproduced bit for bit.  The host
 *   decodes the files named in file_bad itself and nothing is handed over twice.
 * n_files = 0 and files that are all empty give CTMR_OK, all-good verdicts and the empty batch.
 * Sizing is by the good files: CTMR_E_RANGE as above, with *info filled.  CTMR_E_RANGE, CTMR_E_NOMEM and argument
 *   errors leave every output buffer, file_bad included, as it was. */
int ctmr_pem_decode_each(ctmr_engine* e, const uint8_t* text, const uint64_t* file_bounds, uint64_t n_files,
                         uint8_t* payload, size_t payload_cap, uint64_t* offsets, uint64_t certs_cap, uint64_t* file_first,
                         uint64_t* file_bad, ctmr_pem_decode_info* info);
int ctmr_pem_decode_each_device(ctmr_engine* e, const void* d_text, const uint64_t* file_bounds, uint64_t n_files,
                                void* d_payload, size_t payload_cap, uint64_t* d_offsets, uint64_t certs_cap,
                                uint64_t* file_first, uint64_t* file_bad, ctmr_pem_decode_info* info);

/* Asynchronous ingestion (ctmr_submit_batch above) for RAW get-entries responses — what the reference's downloader actually holds (ct-fetch.go:446-462):
 * blob = leaf_input_0 ‖ extra_data_0 ‖ leaf_input_1 ‖ …, bounds u64[2n+1] (ctmr_map_entries' input).  Submits of
 * either form share the pipeline and its ordering; a super-batch holds one form (a change of form closes the open one).
 * The super-batch is decoded, matched (Chain[0] certificates met for the first time are registered on the way, unless
 * ctmr_set_issuer_autoregister(e, 0): then it fails with CTMR_E_NOTFOUND like ctmr_map_entries) and mapped as ONE batch.
 * ctmr_wait_entries additionally hands out the entries' timestamps (ms, :476) and this batch's decode statistics
 * (n_issuers_added, ms_*: of the whole super-batch); it accepts tickets of ctmr_submit_batch too (timestamps 0,
 * dstats zeroed), and ctmr_wait accepts raw tickets. */
int ctmr_submit_entries(ctmr_engine* e, const uint8_t* blob, const uint64_t* bounds, uint64_t n, ctmr_ticket* ticket);
int ctmr_wait_entries(ctmr_engine* e, ctmr_ticket ticket, ctmr_record* records, uint64_t* new_idx, uint64_t* timestamp,
                      ctmr_decode_stats* dstats, ctmr_batch_stats* stats);
/* The third form: get-entries HTTP bodies as they lie (the text ctmr_entries_json_each takes), one or more per submit; a
 * downloader submits the one resp.Body it holds (ct-fetch.go:417-424).  DESIGN.md §22.
 * ctmr_submit_entries_json returns at once: the bytes inside the bounds go to HBM behind the previous submit's on the
 *   copy streams — straight DMA when text came from ctmr_alloc_pinned (keep it untouched until the wait), otherwise
 *   staged before the call returns — and the bodies' bounds are kept with the ticket.  Submits coalesce into a
 *   super-batch of this form; it closes at 96 MB of text, at 4 096 bodies, on ctmr_flush, when one of its tickets is
 *   waited for, and when a submit of another form arrives (the number of entries is not known before it runs).
 * The worker judges every body alone (ctmr_entries_json_each_device), then decodes, matches and maps the good bodies'
 *   entries as ONE batch, like a raw super-batch.  A body outside the grammar costs its own ticket its entries and no
 *   other ticket anything.  Failures of the whole super-batch (CTMR_E_NOTFOUND under ctmr_set_issuer_autoregister(e, 0),
 *   CTMR_E_FULL, CTMR_E_HIP) reach every ticket of it, as for the raw form.
 * ctmr_wait_entries_json blocks until the ticket's super-batch is done.  info: responses, text_bytes, entries = n and
 *   blob_bytes of THIS ticket, bad_response the lowest bad body of the ticket (UINT64_MAX: none), bad_offset its offset.
 *   entries_cap < n: CTMR_E_RANGE with *info filled, nothing written and the ticket NOT consumed — a first call with
 *   entries_cap = 0 is the size query.  Otherwise records[n], new_idx (relative to the ticket, ascending), timestamp[n],
 *   dstats and stats as ctmr_wait_entries slices them, resp_first u64[R + 1] relative to the ticket, resp_bad u64[R]
 *   with offsets relative to the text pointer the submit was given; any output pointer may be NULL.  A ticket with bad
 *   bodies still returns CTMR_OK.
 * ctmr_wait and ctmr_wait_entries have no capacity argument: they refuse a ticket of this form with CTMR_E_INVAL and
 *   leave it collectable.
 * Ordering: bodies keep submission order, entries body order, super-batches run in order with the other forms: records,
 *   NEW lists, timestamps, issuer indices and the engine's sets are those of one synchronous call per submit over its
 *   good bodies, in submission order. */
int ctmr_submit_entries_json(ctmr_engine* e, const uint8_t* text, const uint64_t* resp_bounds, uint64_t n_responses,
                             ctmr_ticket* ticket);
int ctmr_wait_entries_json(ctmr_engine* e, ctmr_ticket ticket, uint64_t entries_cap, ctmr_record* records,
                           uint64_t* new_idx, uint64_t* timestamp, uint64_t* resp_first, uint64_t* resp_bad,
                           ctmr_entries_json_info* info, ctmr_decode_stats* dstats, ctmr_batch_stats* stats);
/* The fourth form: PEM certificate files as they lie (the text ctmr_pem_decode_each takes), one or more per submit: the
 * warm start from what LocalDiskBackend wrote, one certificate a file.  DESIGN.md §23.
 * ctmr_submit_pem returns at once: the bytes inside the bounds go to HBM behind the previous submit's on the copy
 *   streams — straight DMA when text came from ctmr_alloc_pinned (keep it untouched until the wait), otherwise staged
 *   before the call returns — and the files' bounds and issuer_idx, u32[n_files], one issuer table index per FILE or
 *   CTMR_NO_ISSUER (under the reference's layout a file lies below its issuer's directory), are kept with the ticket.
 *   Submits coalesce into a super-batch of this form; it closes at 96 MB of text, at 65 536 files, on ctmr_flush, when
 *   one of its tickets is waited for, and when a submit of another form arrives (the number of certificates is not
 *   known before it runs).
 * The worker judges every file alone (ctmr_pem_decode_each_device), decodes the good files' certificates, expands the
 *   issuer indices to one per certificate on the device (entry_type is 0 throughout) and maps them as ONE batch, like a
 *   packed super-batch.  A file outside the grammar costs its own ticket its certificates and no other ticket
 *   anything.  Failures of the whole super-batch (CTMR_E_FULL, CTMR_E_HIP) reach every ticket of it.
 * ctmr_wait_pem blocks until the ticket's super-batch is done.  info: files, text_bytes, certificates = n,
 *   payload_bytes, regular and irregular of THIS ticket, bad_file the lowest bad file of the ticket (UINT64_MAX: none),
 *   bad_offset its offset.  certs_cap < n: CTMR_E_RANGE with *info filled, nothing written and the ticket NOT consumed —
 *   a first call with certs_cap = 0 is the size query.  Otherwise records[n], new_idx (relative to the ticket,
 *   ascending) and stats as ctmr_wait slices them, file_first u64[F + 1] relative to the ticket, file_bad u64[F] with
 *   offsets relative to the text pointer the submit was given; any output pointer may be NULL.  A ticket with bad files
 *   still returns CTMR_OK.
 * ctmr_wait, ctmr_wait_entries and ctmr_wait_entries_json refuse a ticket of this form with CTMR_E_INVAL and leave it
 *   collectable; ctmr_wait_pem refuses the tickets of the other forms in the same way.
 * Ordering: files keep submission order, certificates file order, super-batches run in order with the other forms:
 *   records, NEW lists and the engine's sets are those of one synchronous ctmr_pem_decode_each + ctmr_map_batch per
 *   submit, in submission order. */
int ctmr_submit_pem(ctmr_engine* e, const uint8_t* text, const uint64_t* file_bounds, uint64_t n_files,
                    const uint32_t* issuer_idx, ctmr_ticket* ticket);
int ctmr_wait_pem(ctmr_engine* e, ctmr_ticket ticket, uint64_t certs_cap, ctmr_record* records, uint64_t* new_idx,
                  uint64_t* file_first, uint64_t* file_bad, ctmr_pem_decode_info* info, ctmr_batch_stats* stats);
/* Issuer registration policy of the raw-entry calls.  on = 1 (default): a Chain[0] certificate met for the first time
 * is registered by the call.  on = 0: nothing is registered; when a batch contains unregistered Chain[0]
 * certificates the decode fails with CTMR_E_NOTFOUND and ctmr_pending_issuers lists them (distinct, [u32 len][DER]…,
 * ascending log index of first appearance) — for hosts that must keep the issuer tables of several engines
 * identical (multi-GPU key exchange: DESIGN.md §8): gather the pending lists of all ranks, register the union in
 * one agreed order with ctmr_add_issuers on every rank, call again. */
/* strict_extensions (ON by default since ABI v7: part of CTMR_PROFILE_REFERENCE, the engine's default).  Go 1.13's crypto/x509 parseCertificate parses
 * the VALUE of the extensions it knows and fails the certificate when that fails; with on != 0 the walk does the same:
 *   by plain encoding/asn1 struct rules, each filling its OCTET STRING ("trailing data") — keyUsage (one BIT STRING),
 *     subjectKeyIdentifier (one OCTET STRING), extKeyUsage (SEQUENCE OF OID), authorityKeyIdentifier (SEQUENCE with an
 *     optional [0]), certificatePolicies (SEQUENCE OF SEQUENCE { OID, … }), authorityInfoAccess (SEQUENCE OF SEQUENCE
 *     { OID, any element }), cRLDistributionPoints (SEQUENCE OF distributionPoint: three optional fields in order, a
 *     nameRelativeToCRLIssuer parsed like a Name) [the last one: ABI v6];
 *   subjectAltName [v6] — one universal SEQUENCE of elements that fit, dispatched on the tag NUMBER: a URI (6) goes
 *     through net/url's Parse and, when it has a host, x509's domainToReverseLabels;
 *   nameConstraints [v6] — as golang.org/x/crypto/cryptobyte reads it: SEQUENCE { [0] permitted, [1] excluded }, not both
 *     absent or empty; dNSName / rfc822Name / URI constraints IA5 and well-formed (parseRFC2821Mailbox, not an IP literal,
 *     no empty label), iPAddress 8 or 32 octets with a contiguous mask.
 * A violation is a FATAL parse error in every role (leaf, precertificate, Chain[0], the strict_leaf TBSCertificate).
 * NON-FATAL findings, as CT-go files them (an X509 entry keeps its certificate; a precertificate and a Chain[0] issuer are
 * dropped) [v6]: a subjectAltName iPAddress that is not 4 or 16 octets long; an embedded SCT list
 * (1.3.6.1.4.1.11129.2.4.2) that does not decode; an INTEGER inside a nameRelativeToCRLIssuer that is not minimally
 * encoded (with strict_strings: also its string values' character sets).
 * These are the standard library's rules plus what is recalled of certificate-transparency-go v1.1.0's changes to them;
 * neither can be verified without CT-go's source — hence a switch: on = 0 is for a host that has parsed the
 * certificates already.  Set it before the issuers are
 * registered (a Chain[0] is judged when it is registered). */
int ctmr_set_strict_extensions(ctmr_engine* e, int on);
int ctmr_set_issuer_autoregister(ctmr_engine* e, int on);
int ctmr_pending_issuers(ctmr_engine* e, uint8_t* out, size_t cap, size_t* need, uint64_t* count);
/* How Chain[0] is identified (cmd/ct-fetch/ct-fetch.go:221 parses it in full for every entry).
 *   CTMR_CHAIN0_EXACT (default): every byte of every entry's Chain[0] is compared with the registered certificate —
 *     equal means identical, whatever the log serves; the identification costs 871 B of HBM reads per entry on the
 *     synthetic corpus and bounds the raw path.
 *   CTMR_CHAIN0_TRUSTED_LOG: a certificate is parsed in full when it is REGISTERED (its first sighting, or
 *     ctmr_add_issuers); afterwards an entry is attributed to it when length, first 16 and last 16 bytes (the end of
 *     the signature) agree — no byte of Chain[0] beyond the lines the framing decode touches anyway is read.  Identical results on
 *     everything a log that serves the chains it validated can produce (two certificates with the same last 16
 *     signature bytes do not occur); a Chain[0] that agrees with a registered certificate in those 36 bytes but not
 *     in between — a damaged copy — is attributed to that certificate, where the reference would parse the bytes
 *     it was given (a parse error, or another issuer).  Which certificate a (length, head, tail) triple stands for
 *     is decided by the lowest log index that carries it in the call that registers it — not by scheduling.  extra_data is not covered
 *     by the log's Merkle tree and the reference verifies neither STH nor inclusion, so its own trust in the log is no
 *     narrower; the choice is the host's.  Registered certificates that agree in those 36 bytes with another
 *     registered certificate are always compared bytewise. */
#define CTMR_CHAIN0_EXACT 0
#define CTMR_CHAIN0_TRUSTED_LOG 1
int ctmr_set_chain0_match(ctmr_engine* e, int mode);
/* Precertificate entries: ct.LogEntryFromLeaf (cmd/ct-fetch/ct-fetch.go:452) also parses the TBSCertificate the
 * MerkleTreeLeaf carries (CT-go x509.ParseTBSCertificate) and the downloader drops the entry when that fails fatally
 * (:453-459).  on = 0 (CTMR_PROFILE_FAST): the leaf TBSCertificate is length-checked only — identical results on every
 * entry a log that validated its submissions can serve, and one pass less over ≈ 400 bytes of every precertificate entry.
 * on = 1 (the default since ABI v7): the raw-entry calls walk it (the certificate walk without the outer wrapper and the signature) before anything
 * else looks at the entry; an entry whose leaf TBSCertificate does not parse gets CTMR_ENTRY_INVALID /
 * CTMR_ST_ENTRY_DECODE_ERROR and its Chain[0] is never registered, as in the reference. */
int ctmr_set_strict_leaf(ctmr_engine* e, int on);
/* The public key inside subjectPublicKeyInfo.  x509.ParseCertificate (cmd/ct-fetch/ct-fetch.go:202, :221, :452) ends in
 * CT-go's parsePublicKey: an RSA key that is not SEQUENCE { INTEGER n, INTEGER e > 0 } with nothing behind it, a DSA key or
 * parameter set that is not positive INTEGERs, an EC key whose parameters do not name P-224/256/384/521 (or secp192r1)
 * or whose point is not an uncompressed point ON that curve is a FATAL parse error — the entry never reaches Store, in
 * any role; RSA parameters other than NULL, an INTEGER of the key that is not minimally encoded, a modulus <= 0 and
 * secp192r1 are non-fatal findings (an X509 entry keeps its certificate, a precertificate and a Chain[0] issuer are
 * dropped, like every other finding).  Other algorithms' keys are not looked at.  ON by default since ABI v5 (rounds
 * 1-3 skipped the key bits by length and accepted such certificates); on = 0 restores that, for a host that has
 * already parsed the keys.  Applies to the map, to issuers registered AFTER the call and, with strict_leaf, to the leaf
 * TBSCertificate.  Rules and their provenance (recalled from CT-go v1.1.0, cross-checked against OpenSSL): spki_key.h,
 * DESIGN.md §3.1. */
int ctmr_set_strict_spki(ctmr_engine* e, int on);
/* Character sets of the string values in the issuer and subject Names.  Go's encoding/asn1 rejects a PrintableString
 * with an octet outside A-Z a-z 0-9 space ' ( ) + , - . / : = ? (and '*', '&', which it tolerates), a NumericString
 * with anything but digits and space, an IA5String with an octet >= 0x80 and a UTF8String that is not valid UTF-8.
 * certificate-transparency-go's fork of that package is more lenient towards some of these — which, cannot be verified
 * without its source — so the rules are a SWITCH (on by default since ABI v7, as part of the reference profile; 0: not
 * checked, as in ABI v1-v6's defaults) and a violation is filed as a NON-FATAL finding: an X509 entry keeps its certificate, a precertificate and a Chain[0] issuer are
 * dropped (cmd/ct-fetch/ct-fetch.go:202-209, 221-225, 452-459).  on = 1: the map checks the two Names of every
 * precertificate while its walk holds them (since round 4; a pre-pass over every certificate before); issuers are
 * judged when they are registered (set the switch before registering them). */
int ctmr_set_strict_strings(ctmr_engine* e, int on);
/* The accept/reject profile as ONE choice (ABI v6) — what x509.ParseCertificate / ct.LogEntryFromLeaf decide at
 * cmd/ct-fetch/ct-fetch.go:202-209, :221-225, :452-459:
 *   CTMR_PROFILE_REFERENCE  THE DEFAULT of ctmr_create (since ABI v7): all four switches on — what the reference does, as
 *                           far as it can be known without CT-go's source (DESIGN.md §3.1 says which rules are recalled
 *                           from where).  The map reads the subjectAltName and checks the Names' character sets; it is
 *                           what bench.py's headline measures.
 *   CTMR_PROFILE_FAST       the opt-in of a host that has ALREADY parsed its certificates (or trusts its log to have):
 *                           strict_spki on; strict_leaf, strict_strings, strict_extensions off — every rule whose bytes
 *                           the path reads anyway.  Looser than the reference on malformed extension bodies, Name
 *                           character sets and the leaf TBSCertificate of precertificate entries; identical on everything
 *                           a CA's encoder and a log that validated its submissions produce (bench.py reports it as
 *                           secondary.fast_profile).
 * Equivalent to the four ctmr_set_strict_* calls; like them, set it BEFORE the issuers are registered. */
#define CTMR_PROFILE_FAST 0
#define CTMR_PROFILE_REFERENCE 1
int ctmr_set_profile(ctmr_engine* e, int profile);
/* ctmr_pem_encode_device for an entry view: PEM of the certificates d_idx[0..n_idx) names, straight out of the blob. */
int ctmr_pem_encode_view_device(ctmr_engine* e, const uint8_t* d_blob, const ctmr_entry_view* d_view,
                                const uint64_t* d_idx, uint64_t n_idx, uint8_t* d_pem, uint64_t pem_cap,
                                uint64_t* d_pem_offsets, uint64_t* pem_bytes);

/* ---- IssuerMetadata on device: replaces the per-new-certificate part of
 *      IssuerMetadata.Accumulate (storage/issuermetadata.go:92-138) — its three per-issuer memo maps knownExpDates,
 *      knownCrlDPs, knownIssuerDNs live in HBM — so that the host only handles FIRST sightings:
 *        CTMR_MK_EXPDATE  (issuer, expDate hour) not seen before → seenExpDateBefore == false →
 *                         backend.AllocateExpDateAndIssuer (storage/filesystemdatabase.go:189-195)
 *        CTMR_MK_CRL      a CRLDistributionPoints URI not seen for this issuer → addCRL (issuermetadata.go:48-73);
 *                         off/len = the URI bytes inside the certificate
 *        CTMR_MK_DN       an issuer Name not seen for this issuer → addIssuerDN(aCert.Issuer.String()) (:75-87);
 *                         off/len = the Name TLV inside the certificate (the host formats pkix.Name.String())
 *        CTMR_MK_HOST     this certificate must be parsed by the host (an element does not fit the device fast
 *                         path: > 64 KiB offsets, > 4 KiB strings, a repeated extension)
 *      Needs config.collect_meta; call right after the map call of the same batch.  Items are in no particular
 *      order.  Device variant: d_offsets/d_ends/d_records/d_new_idx as given to / produced by that map call
 *      (d_ends NULL for a packed batch); when more than items_cap items exist the call fails with CTMR_E_RANGE,
 *      *n_items = the number needed, and the memo is cleared (a retry re-reports earlier sightings, which the
 *      host's sets tolerate — "Must tolerate duplicate information", issuermetadata.go:89).
 *      Host variant (after ctmr_map_batch / ctmr_map_entries called with new_idx != NULL): items plus their bytes
 *      (item k's bytes follow item k-1's; CTMR_MK_HOST and CTMR_MK_EXPDATE carry none); buffers too small →
 *      CTMR_E_RANGE with *n_items / *bytes_need set, nothing lost — call again. ---- */
enum { CTMR_MK_EXPDATE = 0, CTMR_MK_CRL = 1, CTMR_MK_DN = 2, CTMR_MK_HOST = 3 };
typedef struct {
  uint64_t entry;       /* index into the batch */
  uint32_t kind;        /* CTMR_MK_* */
  uint32_t issuer_idx;  /* as in the record */
  int32_t exp_hour;
  uint32_t off, len;    /* byte range inside the certificate */
  uint32_t pad;
} ctmr_meta_item;
int ctmr_meta_new_device(ctmr_engine* e, const uint8_t* d_payload, const uint64_t* d_offsets, const uint64_t* d_ends,
                         const ctmr_record* d_records, const uint64_t* d_new_idx, uint64_t n_new,
                         ctmr_meta_item* d_items, uint64_t items_cap, uint64_t* n_items);
int ctmr_meta_new(ctmr_engine* e, ctmr_meta_item* items, uint64_t items_cap, uint8_t* bytes, size_t bytes_cap,
                  uint64_t* n_items, size_t* bytes_need);
int ctmr_meta_reset(ctmr_engine* e);

/* ---- write-back for the tickets of the asynchronous pipeline: what FilesystemDatabase.Store does for a certificate that
 *      WasUnknown (storage/filesystemdatabase.go:158-211) — IssuerMetadata.Accumulate, AllocateExpDateAndIssuer on a first
 *      (issuer, expDate), StoreCertificatePEM(pem.EncodeToMemory(...)) — without a synchronous call per response.
 *   ctmr_set_pipeline_writeback: the opt-in, per engine.  flags: CTMR_WB_PEM (the PEM blocks of the new entries, as
 *      ctmr_pem_new) | CTMR_WB_META (their first sightings, as ctmr_meta_new; needs config.collect_meta, else
 *      CTMR_E_INVAL); unknown bits → CTMR_E_INVAL.  The flags apply to super-batches OPENED after the call — call
 *      ctmr_flush first to cut the stream exactly here.  0 (the default): the pipeline allocates, launches and copies
 *      nothing for it.  With a flag on, the worker encodes / collects for every super-batch it has mapped, before its
 *      tickets complete.
 *   ctmr_ticket_writeback: the ticket's own slice, for the tickets of all four forms (ctmr_submit_batch,
 *      ctmr_submit_entries, ctmr_submit_entries_json, ctmr_submit_pem).  Blocks as ctmr_wait* does (and launches the open
 *      super-batch when the ticket is in it); does NOT collect the ticket: it may be called any number of times, with the
 *      same answer, until the ticket's own ctmr_wait* collects it — afterwards CTMR_E_NOTFOUND.  When the super-batch
 *      failed: the code the ticket's wait returns.  Thread-safe as the waits are.
 *      Two-call convention: *info is always filled (all zero for a super-batch opened with flags 0: CTMR_OK, nothing
 *      needed); a buffer that is NULL or too small for a non-empty part → CTMR_E_RANGE, nothing written; a part whose
 *      flag was off reports 0 and needs no buffer.
 *        PEM    pem[pem_offsets[k], pem_offsets[k+1]) is the block of the ticket's k-th new entry, in the order of the
 *               new_idx its wait returns; pem_offsets has n_new + 1 slots, pem_offsets[0] == 0.  The bytes are those
 *               ctmr_pem_new gives after a synchronous call over the same entries.
 *        items  ctmr_meta_item as ctmr_meta_new returns them, `entry` relative to the TICKET, ordered by (entry, kind,
 *               off); their bytes back to back in `bytes`, in item order (CTMR_MK_HOST and CTMR_MK_EXPDATE carry none and
 *               have len 0).
 *      ONE memo per engine, shared with the synchronous calls: a first sighting is reported once in the engine's life (until
 *      ctmr_meta_reset), to ONE ticket — the one whose entry claimed it — and never again by a later ctmr_meta_new.  When
 *      two new certificates of one super-batch bring the same item either of them may get it, hence either of their
 *      tickets (as inside one synchronous batch; the host's sets "Must tolerate duplicate information",
 *      issuermetadata.go:89).  The item-buffer overflow rule of ctmr_meta_new holds for the worker too: the memo is
 *      cleared and the run repeated (up to three runs), so such a super-batch re-reports earlier sightings. ---- */
enum { CTMR_WB_PEM = 1, CTMR_WB_META = 2 };
int ctmr_set_pipeline_writeback(ctmr_engine* e, uint32_t flags);
typedef struct {
  uint64_t n_new, pem_bytes, n_items, item_bytes;  /* of this ticket */
  uint32_t flags, pad;                             /* CTMR_WB_* of the ticket's super-batch */
} ctmr_writeback_info;
int ctmr_ticket_writeback(ctmr_engine* e, ctmr_ticket t,
                          uint8_t* pem, uint64_t pem_cap, uint64_t* pem_offsets /* n_new + 1 */,
                          ctmr_meta_item* items, uint64_t items_cap, uint8_t* bytes, uint64_t bytes_cap,
                          ctmr_writeback_info* info);

/* ---- whole-certificate SHA-256 fingerprints (auxiliary; NOT on the reference's path, which never hashes a leaf —
 *      SURVEY.md D2; this is the one-certificate-per-lane SHA-256 kernel BASELINE.json's north_star names).
 *      d_digests receives n × 32 bytes (the digest as crypto/sha256.Sum256 prints it); certificate i is
 *      [d_offsets[i], d_offsets[i+1]) of d_payload, or [d_offsets[i], d_ends[i]) when d_ends != NULL (entry view).
 *      VALU-bound, not HBM-bound: priced against its own roofline in DESIGN.md §5. ---- */
int ctmr_fingerprint_device(ctmr_engine* e, const uint8_t* d_payload, const uint64_t* d_offsets,
                            const uint64_t* d_ends, uint64_t n, uint8_t* d_digests, float* ms);

/* The synthetic CT corpus generator bench.py and the tests use (ctmr_synth_*) is declared in ctmr_bench.h: the same
 * library exports it, but it is NOT part of the drop-in ABI — a host of the reference never binds it. */

#ifdef __cplusplus
}
#endif
#endif /* CTMR_H */
