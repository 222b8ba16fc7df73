"""Host mirror of the reference's per-entry path over the C ABI (include/ctmr.h).

Names follow the reference: `Engine.map_batch` is the batched body of insertCTWorker
(cmd/ct-fetch/ct-fetch.go:191-235) through FilesystemDatabase.Store's WasUnknown
(storage/filesystemdatabase.go:158-183); the set_* methods are storage.RemoteCache
(storage/types.go:83-102) on byte strings.
"""
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import _native as N

RECORD_DTYPE = np.dtype([("status", "u1"), ("flags", "u1"), ("serial_len", "<u2"),
                         ("exp_hour", "<i4"), ("issuer_idx", "<u4"), ("serial", "u1", (20,))])
assert RECORD_DTYPE.itemsize == 32


NONE = 2**64 - 1   # no index: bad_response, bad_file, bad_crl, a good item's word in a `bad` array


def _addr(a):
    """an array's or a torch tensor's address; a raw address (an int: e.g. a pinned buffer) or None as it is"""
    return a.ctypes.data if hasattr(a, "ctypes") else a.data_ptr() if hasattr(a, "data_ptr") else a


def _bad_list(bad, n):
    """the `bad` array of an _each call or a text wait → per item None, or the offset that puts it outside the grammar"""
    return [None if int(b) == NONE else int(b) for b in bad[:n]]


def _text_arg(bodies, join):
    """(text, bounds) with text an array or an address, or a list of bytes → (text: array, address or None, bounds u64)"""
    if isinstance(bodies, tuple):
        return bodies[0], np.ascontiguousarray(bodies[1], dtype=np.uint64)
    text, bounds = join(bodies)
    return (np.frombuffer(text, np.uint8) if text else None), bounds   # pageable: staged before the call returns


class CtmrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ctmr error {code}: {msg}")
        self.code = code


class EntriesJsonError(CtmrError):
    """A get-entries response outside the grammar of ctmr_entries_json*: the host decodes that one itself."""

    def __init__(self, code, msg, bad_response, bad_offset):
        super().__init__(code, msg)
        self.bad_response = bad_response
        self.bad_offset = bad_offset


class PemDecodeError(CtmrError):
    """A PEM file outside the grammar of ctmr_pem_decode*: the host decodes that one itself."""

    def __init__(self, code, msg, bad_file, bad_offset):
        super().__init__(code, msg)
        self.bad_file = bad_file
        self.bad_offset = bad_offset


@dataclass
class Batch:
    """Packed CT-entry batch (SURVEY.md §8(d) layout), host side."""
    payload: np.ndarray      # u8, leaf DER back to back
    offsets: np.ndarray      # u64[n+1]
    issuer_idx: np.ndarray   # u32[n], NO_ISSUER = chain empty
    entry_type: np.ndarray   # u8[n], 0 = X509, 1 = precert

    @property
    def n(self):
        return len(self.offsets) - 1

    def cert(self, i):
        return self.payload[int(self.offsets[i]):int(self.offsets[i + 1])].tobytes()

    @staticmethod
    def from_certs(certs, issuer_idx, entry_type=None):
        offs = np.zeros(len(certs) + 1, dtype=np.uint64)
        if certs:
            offs[1:] = np.cumsum([len(c) for c in certs], dtype=np.uint64)
        payload = np.frombuffer(b"".join(certs), dtype=np.uint8).copy() if certs else np.zeros(0, np.uint8)
        et = np.zeros(len(certs), np.uint8) if entry_type is None else np.asarray(entry_type, np.uint8)
        return Batch(payload, offs, np.asarray(issuer_idx, dtype=np.uint32), et)


@dataclass
class RawEntries:
    """Raw get-entries batch: blob = leaf_input_0 ‖ extra_data_0 ‖ leaf_input_1 ‖ …, bounds u64[2n+1] (include/ctmr.h)."""
    blob: np.ndarray         # u8
    bounds: np.ndarray       # u64[2n+1]
    resp_first: np.ndarray = None   # u64[R+1] when the batch came from R get-entries bodies: each body's first entry
    bad: list = None                # entries_json_each: per body None, or the offset that puts it outside the grammar

    @property
    def n(self):
        return (len(self.bounds) - 1) // 2

    def leaf_input(self, i):
        return self.blob[int(self.bounds[2 * i]):int(self.bounds[2 * i + 1])].tobytes()

    def extra_data(self, i):
        return self.blob[int(self.bounds[2 * i + 1]):int(self.bounds[2 * i + 2])].tobytes()

    @staticmethod
    def from_pairs(pairs):
        """pairs: [(leaf_input bytes, extra_data bytes)] — the base64-decoded members of a get-entries response."""
        parts, bounds, at = [], [0], 0
        for leaf, extra in pairs:
            for b in (leaf, extra):
                parts.append(bytes(b))
                at += len(b)
                bounds.append(at)
        blob = np.frombuffer(b"".join(parts), np.uint8).copy() if at else np.zeros(0, np.uint8)
        return RawEntries(blob, np.asarray(bounds, np.uint64))


@dataclass
class EntriesResult:
    records: np.ndarray      # RECORD_DTYPE[n]
    new_idx: np.ndarray      # u64[n_new], ascending
    timestamp: np.ndarray    # u64[n], ms
    stats: N.BatchStats
    decode: N.DecodeStats
    resp_first: np.ndarray = None   # wait_entries_json: u64[R+1], each body's first entry in this ticket
    bad: list = None                # wait_entries_json: per body None, or the offset (from the submit's first byte) that
                                    # puts it outside the grammar; such a body has no entries


@dataclass
class BatchResult:
    records: np.ndarray      # RECORD_DTYPE[n]
    new_idx: np.ndarray      # u64[n_new], ascending
    stats: N.BatchStats
    file_first: np.ndarray = None   # wait_pem: u64[F+1], each file's first certificate in this ticket
    bad: list = None                # wait_pem: per file None, or the offset (from the submit's first byte) that puts it
                                    # outside the grammar; such a file has no certificates
    info: N.PemDecodeInfo = None    # wait_pem: the ticket's own


@dataclass
class Writeback:
    """Engine.ticket_writeback: what a ticket's super-batch wrote back for it."""
    pem_buf: np.ndarray      # u8: the PEM blocks of the ticket's new entries, back to back, in the order of its new_idx
    pem_offsets: np.ndarray  # u64[n_new + 1] (pem on), else [0]; both arrays go to HostWriter.submit as they are
    items: list              # [(kind, entry, issuer_idx, exp_hour, bytes)] as Engine.meta_new(), entry relative to the ticket,
                             # ordered by (entry, kind, off)
    info: N.WritebackInfo = None
    offs: list = None        # per item: where its bytes lie in its certificate (ctmr_meta_item.off)

    def pem_blocks(self):
        """The list of bytes Engine.pem_new() gives."""
        raw = self.pem_buf.tobytes()
        return [raw[int(self.pem_offsets[k]):int(self.pem_offsets[k + 1])] for k in range(len(self.pem_offsets) - 1)]


class Engine:
    def __init__(self, device=0, table_slots=0, pair_slots=0, max_issuers=0, certs_per_tile=0,
                 lds_tile_bytes=0, map_variant=0, profile=False, collect_meta=False, max_table_slots=0):
        self._lib = N.lib()
        if not map_variant:   # kernel experiments (scripts/run.sh TAG lib:PATH STEP… with a sweep build of the library): whole test suites on another variant
            map_variant = int(os.environ.get("CTMR_MAP_VARIANT", "0"))
        cfg = N.Config(struct_size=C.sizeof(N.Config), device=device, table_slots=table_slots,
                       pair_slots=pair_slots, max_issuers=max_issuers, certs_per_tile=certs_per_tile,
                       lds_tile_bytes=lds_tile_bytes, map_variant=map_variant, profile=int(profile),
                       collect_meta=int(collect_meta), max_table_slots=max_table_slots)
        h = C.c_void_p()
        rc = self._lib.ctmr_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise CtmrError(rc, "ctmr_create failed (no usable HIP device? there is no CPU fallback)")
        self._h = h
        self.device = device
        self.collect_meta = bool(collect_meta)
        self._text_tickets = {}   # ticket of submit_entries_json / submit_pem → (which, its bodies): the wait sizes first and bad by it

    # ---- lifecycle
    def close(self):
        if getattr(self, "_h", None):
            self.free_pinned()
            self._lib.ctmr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise CtmrError(rc, self._lib.ctmr_last_error(self._h).decode(errors="replace"))

    def _ck_at(self, rc, index, error):
        """_ck, but CTMR_E_INVAL with an index that is not NONE — the input item outside the grammar — raises
        error(the library's message): the typed error of the call."""
        if rc == N.E_INVAL and index != NONE:
            raise error(self._lib.ctmr_last_error(self._h).decode(errors="replace"))
        self._ck(rc)

    @property
    def handle(self):
        return self._h

    # ---- the sizing convention (include/ctmr.h): a call whose buffers are short fails with CTMR_E_RANGE and leaves the
    # sizes in its `info`.  The wrappers of such calls go through one of these two.
    def _sized_call(self, call, caps, need, check=None):
        """A first guess, and a second call only when it was short: call(*caps) → (rc, the buffers it made of `caps`),
        once with the caller's guess and once more with need() — the caps the call's `info` asks for after
        CTMR_E_RANGE.  check(rc) raises for any other failure (default: _ck).  → (the buffers, the caps they were made of)"""
        for _ in range(2):
            rc, bufs = call(*caps)
            if rc != N.E_RANGE:
                break
            caps = need()
        (check or self._ck)(rc)
        return bufs, caps

    def _sizes_first(self, call, nothing, alloc, check=None):
        """The sizes first, then the exact call: call(*nothing) → rc without buffers, alloc() → the arguments made of
        what `info` says then, call(*those) to collect.  A first call that returns 0 had nothing to hand over: alloc()
        makes the empty result and there is no second call.  → what alloc() gave"""
        check = check or self._ck
        rc = call(*nothing)
        if rc != N.E_RANGE:
            check(rc)
        args = alloc()
        if rc == N.E_RANGE:
            check(call(*args))
        return args

    # ---- what the device wrappers share
    @property
    def _dev(self):
        return "cuda:%d" % self.device

    def _empty(self, n, device, dtype=np.uint8):
        """n uninitialised uint8 or uint64: a numpy array, or (device) a torch tensor on this engine's device, u64 as int64"""
        if not device:
            return np.empty(n, dtype)
        import torch
        return torch.empty(n, dtype=torch.int64 if dtype is np.uint64 else torch.uint8, device=self._dev)

    def _upload(self, data, floor=0):
        """bytes → a torch uint8 tensor on this engine's device (of `floor` zero bytes when there are none)"""
        import torch
        return torch.from_numpy(np.frombuffer(data, np.uint8).copy() if data else np.zeros(floor, np.uint8)).to(self._dev)

    @staticmethod
    def _tensor(t, name):
        if not hasattr(t, "data_ptr"):
            raise TypeError(name + ": a torch tensor on this engine's device")

    @staticmethod
    def _text_bounds(d_text, bounds, name):
        """The text of a device decoder and where its n items lie in it → (bounds u64[n + 1], the bytes they span)"""
        Engine._tensor(d_text, "d_text")
        b = np.ascontiguousarray(bounds, dtype=np.uint64)
        n = len(b) - 1
        if n < 0 or (n and ((b[1:] < b[:-1]).any() or int(b[n]) > d_text.numel())):
            raise ValueError(name + " do not ascend or reach beyond the text")
        return b, int(b[n] - b[0]) if n else 0

    def set_stream(self, hip_stream):
        self._ck(self._lib.ctmr_set_stream(self._h, hip_stream))

    def synchronize(self):
        self._ck(self._lib.ctmr_synchronize(self._h))

    # ---- page-locked host buffers for the host-buffer entry points
    def pinned_array(self, nbytes):
        """uint8 numpy array over hipHostMalloc memory (freed when the array's owner object is collected)."""
        p = C.c_void_p()
        self._ck(self._lib.ctmr_alloc_pinned(self._h, nbytes, C.byref(p)))
        buf = (C.c_uint8 * max(nbytes, 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=np.uint8, count=nbytes)
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p.value)
        return arr

    def free_pinned(self):
        for p in getattr(self, "_pinned", []):
            self._lib.ctmr_free_pinned(self._h, p)
        self._pinned = []

    # ---- issuers / filter
    def add_issuers(self, certs):
        blob = b"".join(certs)
        offs = np.zeros(len(certs) + 1, dtype=np.uint64)
        if certs:
            offs[1:] = np.cumsum([len(c) for c in certs], dtype=np.uint64)
        first = C.c_uint32()
        buf = np.frombuffer(blob, dtype=np.uint8) if blob else np.zeros(1, np.uint8)
        self._ck(self._lib.ctmr_add_issuers(self._h, buf.ctypes.data, offs.ctypes.data, len(certs),
                                            C.byref(first)))
        return first.value

    def issuer_count(self):
        n = C.c_uint32()
        self._ck(self._lib.ctmr_issuer_count(self._h, C.byref(n)))
        return n.value

    def issuer_info(self, idx):
        info = N.IssuerInfo()
        self._ck(self._lib.ctmr_issuer_info_get(self._h, idx, C.byref(info)))
        return info

    def issuer_id(self, idx):
        return self.issuer_info(idx).issuer_id.decode()

    def set_filter(self, issuer_cn_filter=b"", log_expired=False, now=0):
        if isinstance(issuer_cn_filter, str):
            issuer_cn_filter = issuer_cn_filter.encode()
        self._ck(self._lib.ctmr_set_filter(self._h, issuer_cn_filter, len(issuer_cn_filter),
                                           int(log_expired), int(now)))

    # ---- the batched map + reduce
    def map_batch(self, batch: Batch, want_records=True, want_new=True) -> BatchResult:
        n = batch.n
        payload = np.ascontiguousarray(batch.payload, dtype=np.uint8)
        if payload.size == 0:
            payload = np.zeros(1, np.uint8)
        offsets = np.ascontiguousarray(batch.offsets, dtype=np.uint64)
        iss = np.ascontiguousarray(batch.issuer_idx, dtype=np.uint32)
        et = np.ascontiguousarray(batch.entry_type, dtype=np.uint8)
        records = np.zeros(n, dtype=RECORD_DTYPE)
        new_idx = np.zeros(max(n, 1), dtype=np.uint64)
        st = N.BatchStats()
        self._ck(self._lib.ctmr_map_batch(
            self._h, payload.ctypes.data, offsets.ctypes.data, iss.ctypes.data if n else None,
            et.ctypes.data if n else None, n, records.ctypes.data if (want_records and n) else None,
            new_idx.ctypes.data if (want_new and n) else None, C.byref(st)))
        return BatchResult(records, new_idx[:st.n_new] if want_new else new_idx[:0], st)

    # ---- asynchronous host ingestion (ctmr_submit_batch / ctmr_wait / ctmr_flush)
    def submit_batch(self, payload, offsets, issuer_idx, entry_type, n) -> int:
        """Arrays (numpy, contiguous) or raw addresses (ints: e.g. pinned buffers of alloc_pinned).  Returns the ticket.
        The caller keeps the arrays alive — and pinned payloads untouched — until wait(ticket)."""
        t = C.c_uint64(0)
        self._ck(self._lib.ctmr_submit_batch(self._h, _addr(payload), _addr(offsets), _addr(issuer_idx), _addr(entry_type), n, C.byref(t)))
        return t.value

    def flush(self):
        self._ck(self._lib.ctmr_flush(self._h))

    def wait(self, ticket: int, n: int, want_records=True, want_new=True) -> BatchResult:
        records = np.zeros(n, dtype=RECORD_DTYPE)
        new_idx = np.zeros(max(n, 1), dtype=np.uint64)
        st = N.BatchStats()
        self._ck(self._lib.ctmr_wait(self._h, ticket, records.ctypes.data if (want_records and n) else None,
                                     new_idx.ctypes.data if (want_new and n) else None, C.byref(st)))
        return BatchResult(records, new_idx[:st.n_new] if want_new else new_idx[:0], st)

    def submit_entries(self, blob, bounds, n) -> int:
        """Raw get-entries form of submit_batch (ctmr_submit_entries): blob u8, bounds u64[2n+1] — arrays or addresses."""
        t = C.c_uint64(0)
        self._ck(self._lib.ctmr_submit_entries(self._h, _addr(blob), _addr(bounds), n, C.byref(t)))
        return t.value

    def wait_entries(self, ticket: int, n: int) -> EntriesResult:
        records = np.zeros(n, dtype=RECORD_DTYPE)
        new_idx = np.zeros(max(n, 1), dtype=np.uint64)
        ts = np.zeros(max(n, 1), dtype=np.uint64)
        st, ds = N.BatchStats(), N.DecodeStats()
        self._ck(self._lib.ctmr_wait_entries(self._h, ticket, records.ctypes.data if n else None,
                                             new_idx.ctypes.data if n else None, ts.ctypes.data if n else None,
                                             C.byref(ds), C.byref(st)))
        return EntriesResult(records, new_idx[:st.n_new], ts[:n], st, ds)

    def _wait_text(self, name, ticket, items, call):
        """The two text waits: call(cap, records, new_idx, timestamp, first, bad) → rc, as the size query first (a ticket
        without items is collected by it, so the verdicts are asked for there too), then, knowing items(), to collect.
        → (records, new_idx, timestamp, first, bad as a list of None or offsets)"""
        name_of, B = self._text_tickets.get(ticket, (None, 0))
        if name_of != name:
            raise CtmrError(N.E_NOTFOUND, f"not a ticket of {name}, or already collected")
        first = np.zeros(B + 1, np.uint64)
        bad = np.zeros(max(B, 1), np.uint64)

        def alloc():
            n = items()
            return n, np.zeros(n, dtype=RECORD_DTYPE), np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
        try:
            n, records, new_idx, ts = self._sizes_first(lambda *bufs: call(*bufs, first, bad), (0, None, None, None), alloc)
        finally:
            del self._text_tickets[ticket]   # collected, or failed with its super-batch: either way it is gone
        return records, new_idx, ts[:n], first, _bad_list(bad, B)

    def submit_entries_json(self, bodies) -> int:
        """get-entries HTTP bodies as they lie (a list of bytes — a downloader submits one; or (text, resp_bounds) with
        text an array or an address, e.g. a pinned buffer of pinned_array kept untouched until the wait).  Returns the
        ticket (ctmr_submit_entries_json)."""
        from . import get_entries
        text, rb = _text_arg(bodies, get_entries.join)
        t = C.c_uint64(0)
        self._ck(self._lib.ctmr_submit_entries_json(self._h, _addr(text), rb.ctypes.data, len(rb) - 1, C.byref(t)))
        self._text_tickets[t.value] = ("submit_entries_json", len(rb) - 1)
        return t.value

    def wait_entries_json(self, ticket: int) -> EntriesResult:
        """The ticket's result (ctmr_wait_entries_json; the size query is done here): EntriesResult with resp_first and
        bad.  A body outside the grammar has no entries and its offset in bad; the call does not fail for it."""
        info, st, ds = N.EntriesJsonInfo(), N.BatchStats(), N.DecodeStats()
        records, new_idx, ts, first, bad = self._wait_text(
            "submit_entries_json", ticket, lambda: int(info.entries),
            lambda cap, rec, new, ts, first, bad: self._lib.ctmr_wait_entries_json(
                self._h, ticket, cap, _addr(rec), _addr(new), _addr(ts), first.ctypes.data, bad.ctypes.data, C.byref(info), C.byref(ds), C.byref(st)))
        return EntriesResult(records, new_idx[:st.n_new], ts, st, ds, first, bad)

    def submit_pem(self, files, issuer_idx) -> int:
        """PEM certificate files as they lie (a list of bytes; or (text, file_bounds) with text an array or an address,
        e.g. a pinned buffer of pinned_array kept untouched until the wait) and one issuer table index per FILE, or
        NO_ISSUER.  Returns the ticket (ctmr_submit_pem)."""
        from . import pem_text
        text, fb = _text_arg(files, pem_text.join)
        F = len(fb) - 1
        iss = np.ascontiguousarray(issuer_idx, dtype=np.uint32)
        if iss.shape != (F,):
            raise ValueError("issuer_idx: one per file")
        t = C.c_uint64(0)
        self._ck(self._lib.ctmr_submit_pem(self._h, _addr(text), fb.ctypes.data, F, iss.ctypes.data if F else None, C.byref(t)))
        self._text_tickets[t.value] = ("submit_pem", F)
        return t.value

    def wait_pem(self, ticket: int) -> BatchResult:
        """The ticket's result (ctmr_wait_pem; the size query is done here): BatchResult with file_first, bad and info.
        A file outside the grammar has no certificates and its offset in bad; the call does not fail for it."""
        info, st = N.PemDecodeInfo(), N.BatchStats()
        records, new_idx, _, first, bad = self._wait_text(
            "submit_pem", ticket, lambda: int(info.certificates),
            lambda cap, rec, new, ts, first, bad: self._lib.ctmr_wait_pem(
                self._h, ticket, cap, _addr(rec), _addr(new), first.ctypes.data, bad.ctypes.data, C.byref(info), C.byref(st)))
        return BatchResult(records, new_idx[:st.n_new], st, first, bad, info)

    # ---- write-back for tickets (ctmr_set_pipeline_writeback / ctmr_ticket_writeback): PEM and first sightings of what a
    # ticket found new, without a synchronous call
    def set_pipeline_writeback(self, pem=False, meta=False):
        """For the super-batches opened from now on (flush() first to cut the stream here): pem — the PEM blocks of every
        ticket's new entries, meta — their first sightings (needs collect_meta=True)."""
        self._ck(self._lib.ctmr_set_pipeline_writeback(self._h, (N.WB_PEM if pem else 0) | (N.WB_META if meta else 0)))

    def ticket_writeback(self, ticket: int) -> "Writeback":
        """The ticket's slice of its super-batch's write-back (the size query is done here).  Call it BEFORE the ticket's
        wait, any number of times; afterwards it raises CtmrError(E_NOTFOUND)."""
        info = N.WritebackInfo()

        def alloc():
            pem, buf = np.zeros(max(int(info.pem_bytes), 1), np.uint8), np.zeros(max(int(info.item_bytes), 1), np.uint8)
            return (pem, pem.size, np.zeros(int(info.n_new) + 1, np.uint64), (N.MetaItem * max(int(info.n_items), 1))(), int(info.n_items),
                    buf, buf.size)
        pem, _, offs, items, _, buf, _ = self._sizes_first(
            lambda pem, pem_cap, offs, items, n_items, buf, buf_cap: self._lib.ctmr_ticket_writeback(
                self._h, ticket, _addr(pem), pem_cap, _addr(offs), items, n_items, _addr(buf), buf_cap, C.byref(info)),
            (None, 0, None, None, 0, None, 0), alloc)
        raw, at, out = buf.tobytes(), 0, []
        for it in items[:int(info.n_items)]:
            out.append((it.kind, int(it.entry), it.issuer_idx, it.exp_hour, raw[at:at + it.len]))
            at += it.len
        n_new = int(info.n_new) if info.flags & N.WB_PEM else 0
        return Writeback(pem[:int(info.pem_bytes)], offs[:n_new + 1], out, info, [int(it.off) for it in items[:int(info.n_items)]])

    def map_batch_device(self, d_payload, d_offsets, d_issuer_idx, d_entry_type, n, d_records=0,
                         d_new_idx=0) -> N.BatchStats:
        """All pointers are device addresses (ints), e.g. torch tensors' data_ptr()."""
        st = N.BatchStats()
        self._ck(self._lib.ctmr_map_batch_device(self._h, d_payload, d_offsets, d_issuer_idx, d_entry_type, n, d_records, d_new_idx,
                                                 C.byref(st)))
        return st

    # ---- raw get-entries input (N2): ct.LogEntryFromLeaf + the choice of certificate and Chain[0] on the GPU
    def map_entries(self, raw: RawEntries) -> EntriesResult:
        """Downloader decode (ct-fetch.go:452) + insertCTWorker (:191-235) over raw entries.  Chain[0] certificates
        are registered as issuers by the call; entries LogEntryFromLeaf rejects get ST_ENTRY_DECODE_ERROR."""
        n = raw.n
        blob = np.ascontiguousarray(raw.blob, dtype=np.uint8)
        if blob.size == 0:
            blob = np.zeros(1, np.uint8)
        bounds = np.ascontiguousarray(raw.bounds, dtype=np.uint64)
        records = np.zeros(n, dtype=RECORD_DTYPE)
        new_idx = np.zeros(max(n, 1), dtype=np.uint64)
        ts = np.zeros(max(n, 1), dtype=np.uint64)
        st, ds = N.BatchStats(), N.DecodeStats()
        self._ck(self._lib.ctmr_map_entries(self._h, blob.ctypes.data, bounds.ctypes.data, n,
                                            records.ctypes.data if n else None, new_idx.ctypes.data if n else None,
                                            ts.ctypes.data if n else None, C.byref(ds), C.byref(st)))
        return EntriesResult(records, new_idx[:st.n_new], ts[:n], st, ds)

    def decode_entries_device(self, d_blob, d_bounds, n, view: N.EntryView) -> N.DecodeStats:
        ds = N.DecodeStats()
        self._ck(self._lib.ctmr_decode_entries_device(self._h, d_blob, d_bounds, n, C.byref(view), C.byref(ds)))
        return ds

    def map_view_device(self, d_blob, blob_bytes, view: N.EntryView, n, d_records=0, d_new_idx=0) -> N.BatchStats:
        st = N.BatchStats()
        self._ck(self._lib.ctmr_map_view_device(self._h, d_blob, blob_bytes, C.byref(view), n, d_records, d_new_idx, C.byref(st)))
        return st

    def map_entries_device(self, d_blob, d_bounds, n, d_records=0, d_new_idx=0, d_timestamp=0):
        st, ds = N.BatchStats(), N.DecodeStats()
        self._ck(self._lib.ctmr_map_entries_device(self._h, d_blob, d_bounds, n, d_records, d_new_idx, d_timestamp, C.byref(ds),
                                                   C.byref(st)))
        return st, ds

    # ---- get-entries HTTP bodies as they lie (include/ctmr.h ctmr_entries_json*; CPU twin: get_entries.parse)
    def _ej_ck(self, rc, info):
        self._ck_at(rc, info.bad_response, lambda msg: EntriesJsonError(rc, msg, info.bad_response, info.bad_offset))

    def _entries_json(self, text, text_bytes, rb, device, each):
        """The one call of the four entries_json forms, its buffers sized by the bounds 3/4 text_bytes and
        text_bytes / 34.  text: the address rb counts from.  → (blob, bounds, resp_first, bad or None, info)"""
        R = len(rb) - 1
        blob_cap, entries_cap = text_bytes * 3 // 4 + N.PAYLOAD_PAD, text_bytes // 34
        blob, bounds = self._empty(blob_cap, device), self._empty(2 * entries_cap + 1, device, np.uint64)
        first = np.empty(R + 1, np.uint64)
        bad = np.empty(max(R, 1), np.uint64) if each else None
        info = N.EntriesJsonInfo()
        fn = getattr(self._lib, "ctmr_entries_json" + ("_each" if each else "") + ("_device" if device else ""))
        rc = fn(self._h, text, rb.ctypes.data, R, _addr(blob), blob_cap, _addr(bounds), entries_cap, first.ctypes.data,
                *((bad.ctypes.data,) if each else ()), C.byref(info))
        if each:   # (every body is judged alone: no typed error)
            self._ck(rc)
        else:
            self._ej_ck(rc, info)
        return blob[:info.blob_bytes + N.PAYLOAD_PAD], bounds[:2 * info.entries + 1], first, _bad_list(bad, R) if each else None, info

    def _entries_json_host(self, bodies, each) -> RawEntries:
        from . import get_entries
        text, rb = get_entries.join(bodies)
        buf = np.frombuffer(text, np.uint8) if text else np.zeros(1, np.uint8)
        return RawEntries(*self._entries_json(buf.ctypes.data, len(text), rb, False, each)[:4])

    def _entries_json_device(self, d_text, resp_bounds, each):
        rb, text_bytes = self._text_bounds(d_text, resp_bounds, "resp_bounds")
        return self._entries_json(d_text.data_ptr() if text_bytes else None, text_bytes, rb, True, each)

    def entries_json(self, bodies) -> RawEntries:
        """The raw entries of get-entries bodies (a list of bytes, in log order): JSON and base64 decoded on the GPU,
        text and result in host memory; the blob keeps the PAYLOAD_PAD zero bytes behind bounds[2n], as
        synth.host_entries' does.  A body outside the grammar raises EntriesJsonError with its number."""
        return self._entries_json_host(bodies, False)

    def entries_json_device(self, d_text, resp_bounds):
        """entries_json of a torch uint8 tensor on this engine's device (any alignment; body r at
        d_text[resp_bounds[r]:resp_bounds[r + 1]]) → (d_blob, d_bounds, resp_first, info): torch tensors on the device —
        blob_bytes + PAYLOAD_PAD bytes and u64[2n + 1] as int64, views of buffers sized in one call by the bounds
        3/4 text_bytes and text_bytes / 34 — and the host array u64[R + 1]."""
        d_blob, d_bounds, first, _, info = self._entries_json_device(d_text, resp_bounds, False)
        return d_blob, d_bounds, first, info

    def entries_json_each(self, bodies) -> RawEntries:
        """entries_json with every body judged on its own (ctmr_entries_json_each; CPU twin:
        get_entries.parse_each): nothing is raised for a body outside the grammar — it has no entries, and .bad[r] holds
        its offset (None for the others)."""
        return self._entries_json_host(bodies, True)

    def entries_json_each_device(self, d_text, resp_bounds):
        """entries_json_device with every body judged on its own → (d_blob, d_bounds, resp_first, bad, info); bad as in
        entries_json_each, offsets counted as resp_bounds counts."""
        return self._entries_json_device(d_text, resp_bounds, True)

    def map_entries_json(self, bodies) -> EntriesResult:
        """map_entries over get-entries bodies (a list of bytes): text → raw entries on the device → map_entries_device,
        no blob in host memory."""
        import torch
        from . import get_entries
        text, rb = get_entries.join(bodies)
        dev = self._dev
        d_text = self._upload(text, 1)
        d_blob, d_bounds, _, info = self.entries_json_device(d_text, rb)
        n = int(info.entries)
        if not n:   # nothing to map
            return EntriesResult(np.zeros(0, RECORD_DTYPE), np.zeros(0, np.uint64), np.zeros(0, np.uint64), N.BatchStats(),
                                 N.DecodeStats())
        d_rec = torch.zeros(max(n, 1) * RECORD_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_new = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        d_ts = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        st, ds = self.map_entries_device(d_blob.data_ptr(), d_bounds.data_ptr(), n, d_rec.data_ptr() if n else 0,
                                         d_new.data_ptr() if n else 0, d_ts.data_ptr() if n else 0)
        records = d_rec.cpu().numpy().view(RECORD_DTYPE)[:n].copy()
        return EntriesResult(records, d_new.cpu().numpy().view(np.uint64)[:st.n_new].copy(),
                             d_ts.cpu().numpy().view(np.uint64)[:n].copy(), st, ds)

    # ---- PEM certificate files as they lie (include/ctmr.h ctmr_pem_decode*; CPU twin: pem_text.parse)
    def _pem_decode(self, text, fb, device, each):
        """The two calls of the four pem_decode forms (sizes first: CTMR_E_RANGE fills `info`, then into buffers of
        exactly that size).  text: the address fb counts from.  A file outside the grammar raises PemDecodeError with
        its number.  → (payload, offsets, file_first, info[, bad])"""
        F = len(fb) - 1
        bad = np.empty(max(F, 1), np.uint64) if each else None
        info = N.PemDecodeInfo()
        fn = getattr(self._lib, "ctmr_pem_decode" + ("_each" if each else "") + ("_device" if device else ""))

        def call(payload, payload_cap, offsets, n, first):
            return fn(self._h, text, fb.ctypes.data, F, _addr(payload), payload_cap, _addr(offsets), n, _addr(first),
                      *((bad.ctypes.data,) if each else ()), C.byref(info))

        def alloc():
            cap = info.payload_bytes + N.PAYLOAD_PAD
            return (self._empty(cap, device), cap, self._empty(info.certificates + 1, device, np.uint64), info.certificates,
                    np.empty(info.files + 1, np.uint64))

        def check(rc):
            self._ck_at(rc, info.bad_file, lambda msg: PemDecodeError(rc, msg, info.bad_file, info.bad_offset))
        payload, _, offsets, _, first = self._sizes_first(call, (None, 0, None, 0, None), alloc, check)
        return (payload, offsets, first, info) + ((_bad_list(bad, F),) if each else ())

    def _pem_decode_host(self, files, each):
        from . import pem_text
        text, fb = pem_text.join(files)
        buf = np.frombuffer(text, np.uint8) if text else np.zeros(1, np.uint8)
        return self._pem_decode(buf.ctypes.data, fb, False, each)

    def _pem_decode_device(self, d_text, file_bounds, each):
        import torch
        fb, text_bytes = self._text_bounds(d_text, file_bounds, "file_bounds")
        torch.cuda.synchronize(self.device)     # the engine runs on a stream of its own: what was queued to write d_text is done first
        return self._pem_decode(d_text.data_ptr() if text_bytes else None, fb, True, each)

    def pem_decode(self, files):
        """The certificates of PEM files (a list of bytes: concatenated CERTIFICATE blocks each), armor and base64
        decoded on the GPU, text and result in host memory → (payload: numpy uint8 of payload_bytes + PAYLOAD_PAD, the
        padding zeroed; offsets u64[n + 1]; file_first u64[F + 1]; info).  With issuer indices and entry types this is a
        Batch."""
        return self._pem_decode_host(files, False)

    def pem_decode_device(self, d_text, file_bounds):
        """pem_decode of a torch uint8 tensor on this engine's device (any alignment; file f at
        d_text[file_bounds[f]:file_bounds[f + 1]]) → (d_payload, d_offsets, file_first, info): torch tensors on the
        device — payload_bytes + PAYLOAD_PAD bytes and u64[n + 1] as int64 — and the host array u64[F + 1]."""
        return self._pem_decode_device(d_text, file_bounds, False)

    def pem_decode_each(self, files):
        """pem_decode with every file judged on its own (ctmr_pem_decode_each; CPU twin:
        pem_text.parse_each) → (payload, offsets, file_first, info, bad): nothing is raised for a file outside the
        grammar — it has no certificates, and bad[f] holds its offset (None for the others)."""
        return self._pem_decode_host(files, True)

    def pem_decode_each_device(self, d_text, file_bounds):
        """pem_decode_device with every file judged on its own → (d_payload, d_offsets, file_first, info, bad); bad as in
        pem_decode_each, offsets counted as file_bounds counts."""
        return self._pem_decode_device(d_text, file_bounds, True)

    def map_pem(self, files, issuer_idx, want_records=True, want_new=True) -> BatchResult:
        """map_batch over PEM files (a list of bytes): text → packed batch on the device → map_batch_device, no DER in
        host memory.  issuer_idx: one issuer table index per FILE, or NO_ISSUER — under the reference's layout a file
        lies below its issuer's directory — expanded to one per certificate on the device.  entry_type is 0
        throughout: a certificate on disk was accepted once, and as an X509 entry it is accepted again, findings or not."""
        import torch
        from . import pem_text
        text, fb = pem_text.join(files)
        iss = np.ascontiguousarray(issuer_idx, dtype=np.uint32)
        if iss.shape != (len(files),):
            raise ValueError("issuer_idx: one per file")
        dev = self._dev
        d_text = self._upload(text, 1)
        d_payload, d_offsets, first, info = self.pem_decode_device(d_text, fb)
        n = int(info.certificates)
        if not n:   # nothing to map
            return BatchResult(np.zeros(0, RECORD_DTYPE), np.zeros(0, np.uint64), N.BatchStats())
        counts = torch.from_numpy(np.diff(first.astype(np.int64))).to(dev)
        d_iss = torch.repeat_interleave(torch.from_numpy(iss.view(np.int32).copy()).to(dev), counts).contiguous()
        d_et = torch.zeros(n, dtype=torch.uint8, device=dev)
        d_rec = torch.zeros(n * RECORD_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_new = torch.zeros(n, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(self.device)     # (the issuer indices and the zeroed outputs are whole before the engine's stream starts)
        st = self.map_batch_device(d_payload.data_ptr(), d_offsets.data_ptr(), d_iss.data_ptr(), d_et.data_ptr(), n,
                                   d_rec.data_ptr() if want_records else 0, d_new.data_ptr() if want_new else 0)
        records = d_rec.cpu().numpy().view(RECORD_DTYPE)[:n].copy() if want_records else np.zeros(n, RECORD_DTYPE)
        new_idx = d_new.cpu().numpy().view(np.uint64)[:st.n_new].copy() if want_new else np.zeros(0, np.uint64)
        return BatchResult(records, new_idx, st)

    def synth_entries_device(self, cfg: N.SynthConfig, first, n, d_bounds, d_blob, blob_cap) -> int:
        out = C.c_uint64()
        self._ck(self._lib.ctmr_synth_entries_device(self._h, C.byref(cfg), first, n, d_bounds, d_blob, blob_cap, C.byref(out)))
        return out.value

    # ---- IssuerMetadata on device (N3): first sightings among the new certificates of the last host batch
    def meta_new(self):
        """[(kind, entry, issuer_idx, exp_hour, bytes)] — kind N.MK_EXPDATE / MK_CRL (URI bytes) / MK_DN (issuer Name
        TLV) / MK_HOST (parse certificate `entry` on the host).  Needs collect_meta=True."""
        ni, need = C.c_uint64(0), C.c_size_t(0)
        rc = self._lib.ctmr_meta_new(self._h, None, 0, None, 0, C.byref(ni), C.byref(need))
        if rc not in (0, N.E_RANGE):
            self._ck(rc)
        if ni.value == 0:
            return []
        items = (N.MetaItem * ni.value)()
        buf = np.zeros(max(need.value, 1), np.uint8)
        self._ck(self._lib.ctmr_meta_new(self._h, items, ni.value, buf.ctypes.data, need.value, C.byref(ni),
                                         C.byref(need)))
        raw, at, out = buf.tobytes(), 0, []
        for it in items:
            out.append((it.kind, int(it.entry), it.issuer_idx, it.exp_hour, raw[at:at + it.len]))
            at += it.len
        return out

    def meta_new_device(self, d_payload, d_offsets, d_ends, d_records, d_new_idx, n_new, d_items, items_cap) -> int:
        n = C.c_uint64(0)
        self._ck(self._lib.ctmr_meta_new_device(self._h, d_payload, d_offsets, d_ends, d_records, d_new_idx, n_new, d_items, items_cap,
                                                C.byref(n)))
        return n.value

    def meta_reset(self):
        self._ck(self._lib.ctmr_meta_reset(self._h))

    # ---- whole-certificate SHA-256 (auxiliary: not on the reference's path)
    def fingerprint_device(self, d_payload, d_offsets, d_ends, n, d_digests) -> float:
        """n × 32-byte SHA-256 digests of the certificates into d_digests; returns the kernel time in ms."""
        ms = C.c_float(0)
        self._ck(self._lib.ctmr_fingerprint_device(self._h, d_payload, d_offsets, d_ends, n, d_digests, C.byref(ms)))
        return ms.value

    # ---- PEM write-back (N1): pem.EncodeToMemory of the newly unknown certificates, on the GPU
    def pem_new(self):
        """PEM blocks (bytes) of every WAS_UNKNOWN entry of the last map_batch(), ascending entry order."""
        need, count = C.c_size_t(0), C.c_uint64(0)
        rc = self._lib.ctmr_pem_new(self._h, None, 0, None, C.byref(need), C.byref(count))
        if rc not in (0, N.E_RANGE):
            self._ck(rc)
        if count.value == 0:
            return []
        out = np.zeros(need.value, np.uint8)
        offs = np.zeros(count.value + 1, np.uint64)
        self._ck(self._lib.ctmr_pem_new(self._h, out.ctypes.data, out.size, offs.ctypes.data, C.byref(need),
                                        C.byref(count)))
        raw = out.tobytes()
        return [raw[int(offs[k]):int(offs[k + 1])] for k in range(count.value)]

    def pem_encode_device(self, d_payload, d_offsets, d_idx, n_idx, d_pem, pem_cap, d_pem_offsets) -> int:
        total = C.c_uint64(0)
        self._ck(self._lib.ctmr_pem_encode_device(self._h, d_payload, d_offsets, d_idx, n_idx, d_pem, pem_cap, d_pem_offsets,
                                                  C.byref(total)))
        return int(total.value)

    def pem_encode_view_device(self, d_blob, view: N.EntryView, d_idx, n_idx, d_pem, pem_cap, d_pem_offsets) -> int:
        total = C.c_uint64(0)
        self._ck(self._lib.ctmr_pem_encode_view_device(self._h, d_blob, C.byref(view), d_idx, n_idx, d_pem, pem_cap, d_pem_offsets,
                                                       C.byref(total)))
        return int(total.value)

    # ---- cross-GPU key exchange, owner-computes (ctmr.h: ctmr_xchg_*): one round on this rank, device pointers as ints.
    # ctmr_mapreduce_amd.distributed.Group drives whole rounds natively; these are the per-rank steps for a host with a
    # transport of its own, and for tests.
    KEY_BYTES = 32          # a key record (serial of up to 20 octets)
    KEY_BYTES_LONG = 64     # … of 21..40 octets

    def xchg_map(self, shard: N.Shard, world: int, rank: int, ord_base: int):
        """→ (records per owner, number of 64-byte records)."""
        counts = (C.c_uint64 * world)()
        n_long = C.c_uint64(0)
        self._ck(self._lib.ctmr_xchg_map_device(self._h, C.byref(shard), world, rank, ord_base, counts, C.byref(n_long)))
        return [int(c) for c in counts], int(n_long.value)

    def xchg_keys(self, world: int, d_keys32_out=0, d_keys64_out=0):
        """Partitioned key records into the caller's buffers → 64-byte records per owner."""
        counts64 = (C.c_uint64 * world)()
        self._ck(self._lib.ctmr_xchg_keys_device(self._h, d_keys32_out, d_keys64_out, counts64))
        return [int(c) for c in counts64]

    def xchg_insert(self, d_keys32=0, n32=0, d_flags32=0, d_keys64=0, n64=0, d_flags64=0):
        self._ck(self._lib.ctmr_xchg_insert_device(
            self._h, d_keys32 if n32 else None, n32, d_keys64 if n64 else None, n64,
            d_flags32 if n32 else None, d_flags64 if n64 else None))

    def xchg_apply(self, d_sent32=0, d_flags32=0, n32=0, d_sent64=0, d_flags64=0, n64=0) -> N.BatchStats:
        st = N.BatchStats()
        self._ck(self._lib.ctmr_xchg_apply_device(
            self._h, d_sent32 if n32 else None, d_flags32 if n32 else None, n32,
            d_sent64 if n64 else None, d_flags64 if n64 else None, n64, C.byref(st)))
        return st

    def set_issuer_autoregister(self, on: bool):
        self._ck(self._lib.ctmr_set_issuer_autoregister(self._h, int(bool(on))))

    def set_chain0_match(self, mode: int):
        """N.CHAIN0_EXACT (default: every byte of every Chain[0] compared) or N.CHAIN0_TRUSTED_LOG (compared on the
        first sighting per call, then identified by length + first/last 16 bytes) — include/ctmr.h."""
        self._ck(self._lib.ctmr_set_chain0_match(self._h, int(mode)))

    def set_strict_extensions(self, on: bool):
        """The bodies of the extensions Go unmarshals by plain struct rules become a fatal parse error (include/ctmr.h); off
        by default."""
        self._ck(self._lib.ctmr_set_strict_extensions(self._h, int(bool(on))))

    def set_profile(self, profile):
        """ctmr_set_profile: "fast" (the defaults) or "reference" (strict_spki + strict_leaf + strict_strings +
        strict_extensions: what the reference does, as far as it can be known here).  Before the issuers are registered."""
        p = {"fast": N.PROFILE_FAST, "reference": N.PROFILE_REFERENCE}.get(profile, profile)
        self._ck(self._lib.ctmr_set_profile(self._h, int(p)))

    def set_strict_leaf(self, on: bool):
        """Walk the leaf TBSCertificate of precertificate entries as ct.LogEntryFromLeaf does (include/ctmr.h); default off."""
        self._ck(self._lib.ctmr_set_strict_leaf(self._h, int(bool(on))))

    def set_strict_spki(self, on: bool):
        """parsePublicKey's verdict on the key inside subjectPublicKeyInfo (ctmr_set_strict_spki): ON by default."""
        self._ck(self._lib.ctmr_set_strict_spki(self._h, int(bool(on))))

    def set_strict_strings(self, on: bool):
        """Go-stdlib character-set rules for the string values of both Names, filed as a non-fatal finding (include/ctmr.h);
        default off.  Set it before registering issuers."""
        self._ck(self._lib.ctmr_set_strict_strings(self._h, int(bool(on))))

    def pending_issuers(self):
        """Distinct Chain[0] certificates the last raw-entry call found unregistered (auto-registration off)."""
        need, cnt = C.c_size_t(), C.c_uint64()
        rc = self._lib.ctmr_pending_issuers(self._h, None, 0, C.byref(need), C.byref(cnt))
        if rc not in (0, N.E_RANGE):
            self._ck(rc)
        if cnt.value == 0:
            return []
        buf = (C.c_uint8 * need.value)()
        self._ck(self._lib.ctmr_pending_issuers(self._h, buf, need.value, C.byref(need), C.byref(cnt)))
        raw, out, o = bytes(buf), [], 0
        while o < len(raw):
            l = int.from_bytes(raw[o:o + 4], "little")
            out.append(raw[o + 4:o + 4 + l])
            o += 4 + l
        return out

    # ---- cross-GPU global dedup, Bloom pre-filter variant (ctmr.h: ctmr_bloom_*), device pointers as ints
    def bloom_config(self, bits: int, d_words=0):
        """d_words: caller-owned device buffer of bits/8 bytes (0 = the library allocates the filter)."""
        self._ck(self._lib.ctmr_bloom_config(self._h, bits, d_words))

    def bloom_device(self):
        """(device pointer, n_words) of this rank's cumulative filter (u64 words)."""
        p, nw = C.c_void_p(), C.c_uint64()
        self._ck(self._lib.ctmr_bloom_device(self._h, C.byref(p), C.byref(nw)))
        return int(p.value), int(nw.value)

    def bloom_add(self, d_payload, d_offsets, d_ends, n, d_records=0):
        self._ck(self._lib.ctmr_bloom_add_device(self._h, d_payload if n else None, d_offsets if n else None, d_ends, n, d_records))

    def bloom_probe(self, d_payload, d_offsets, d_ends, n, d_records, d_filters, world, rank, order_base,
                    d_keys_out, keys_cap):
        """→ (counts per peer, fits): fits False = keys_cap too small, nothing written, call again."""
        counts = (C.c_uint64 * world)()
        rc = self._lib.ctmr_bloom_probe_device(self._h, d_payload if n else None, d_offsets if n else None, d_ends, n, d_records, d_filters,
                                               world, rank, order_base, d_keys_out if keys_cap else None, keys_cap, counts)
        if rc == N.E_RANGE:
            return [int(c) for c in counts], False
        self._ck(rc)
        return [int(c) for c in counts], True

    def bloom_lookup(self, d_keys, n_keys, order_base, d_flags):
        self._ck(self._lib.ctmr_bloom_lookup_device(self._h, d_keys if n_keys else None, n_keys, order_base, d_flags if n_keys else None))

    def bloom_apply(self, d_records, n, d_keys_sent, d_flags, n_keys, d_new_idx=0) -> N.BatchStats:
        st = N.BatchStats()
        self._ck(self._lib.ctmr_bloom_apply_device(self._h, d_records, n, d_keys_sent if n_keys else None, d_flags if n_keys else None,
                                                   n_keys, d_new_idx, C.byref(st)))
        return st

    # ---- storage.RemoteCache set methods (storage/types.go:83-102)
    @staticmethod
    def _b(x):
        return x.encode() if isinstance(x, str) else bytes(x)

    def set_insert(self, key, member) -> bool:
        key, member = self._b(key), self._b(member)
        out = C.c_int()
        self._ck(self._lib.ctmr_set_insert(self._h, key, len(key), member, len(member), C.byref(out)))
        return bool(out.value)

    def set_contains(self, key, member) -> bool:
        key, member = self._b(key), self._b(member)
        out = C.c_int()
        self._ck(self._lib.ctmr_set_contains(self._h, key, len(key), member, len(member), C.byref(out)))
        return bool(out.value)

    def set_remove(self, key, member) -> bool:
        key, member = self._b(key), self._b(member)
        out = C.c_int()
        self._ck(self._lib.ctmr_set_remove(self._h, key, len(key), member, len(member), C.byref(out)))
        return bool(out.value)

    def set_cardinality(self, key) -> int:
        key = self._b(key)
        out = C.c_int64()
        self._ck(self._lib.ctmr_set_cardinality(self._h, key, len(key), C.byref(out)))
        return out.value

    def exists(self, key) -> bool:
        key = self._b(key)
        out = C.c_int()
        self._ck(self._lib.ctmr_exists(self._h, key, len(key), C.byref(out)))
        return bool(out.value)

    def _listing(self, fn, arg):
        need = C.c_size_t()
        cnt = C.c_uint64()
        rc = fn(self._h, arg, len(arg), None, 0, C.byref(need), C.byref(cnt))
        if rc not in (0, N.E_RANGE):
            self._ck(rc)
        buf = (C.c_uint8 * max(need.value, 1))()
        self._ck(fn(self._h, arg, len(arg), buf, need.value, C.byref(need), C.byref(cnt)))
        raw = bytes(buf)[:need.value]
        out, o = [], 0
        while o < len(raw):
            l = int.from_bytes(raw[o:o + 4], "little")
            out.append(raw[o + 4:o + 4 + l])
            o += 4 + l
        return out

    def set_list(self, key):
        """SetList / SetToChan: members, sorted bytewise."""
        return self._listing(self._lib.ctmr_set_members, self._b(key))

    def keys(self, pattern=b"*"):
        """KeysToChan(pattern)."""
        return self._listing(self._lib.ctmr_keys, self._b(pattern))

    def expire_at(self, key, unix_seconds):
        key = self._b(key)
        self._ck(self._lib.ctmr_expire_at(self._h, key, len(key), int(unix_seconds)))

    def expire_sweep(self, now) -> int:
        out = C.c_uint64()
        self._ck(self._lib.ctmr_expire_sweep(self._h, int(now), C.byref(out)))
        return out.value

    # ---- counts (cmd/storage-statistics/storage-statistics.go:44-53)
    def issuer_counts(self):
        n = self.issuer_count()
        out = np.zeros(max(n, 1), dtype=np.uint64)
        self._ck(self._lib.ctmr_issuer_counts(self._h, out.ctypes.data, n))
        return out[:n]

    def total_count(self) -> int:
        out = C.c_uint64()
        self._ck(self._lib.ctmr_total_count(self._h, C.byref(out)))
        return out.value

    def issuer_counts_device(self):
        p = C.c_void_p()
        n = C.c_uint32()
        self._ck(self._lib.ctmr_issuer_counts_device(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def reset_known(self):
        self._ck(self._lib.ctmr_reset_known(self._h))

    def table_info(self) -> N.TableInfo:
        """How full the known-certificate table is: index slots / occupied, arena cells / used, rebuilds, compactions."""
        out = N.TableInfo()
        self._ck(self._lib.ctmr_table_info_get(self._h, C.byref(out)))
        return out

    # ---- the known-certificate image (include/ctmr.h; parsed and written without a GPU by known_image.py)
    @staticmethod
    def _stats_dict(st) -> dict:
        return {f: getattr(st, f) for f, _ in st._fields_ if f != "reserved"}

    @staticmethod
    def _members_ptr(d_members):
        Engine._tensor(d_members, "d_members")
        n = d_members.numel() // 48
        return n, (d_members.data_ptr() if n else None)

    def _known_export_call(self, fn, alloc):
        """One export call sized up front — the live members are at most table_info().occupied, the meta part as large
        as last time — and a second one only when that was short (CTMR_E_RANGE fills `info` with the sizes)."""
        info = N.KnownImageInfo()

        def call(meta_cap, members_cap):
            bufs = alloc(meta_cap, members_cap)
            return fn(bufs, meta_cap, members_cap, info), bufs
        bufs, (meta_cap, _) = self._sized_call(call, (getattr(self, "_known_meta_cap", 1 << 16), max(self.table_info().occupied, 1)),
                                               lambda: (max(info.meta_bytes, 64), max(info.members, 1)))
        self._known_meta_cap = max(meta_cap, info.meta_bytes)
        return bufs, info

    def known_export(self) -> bytes:
        """Snapshot of every serials:: set as one image (what a restarted reference finds in Redis)."""
        (buf,), info = self._known_export_call(
            lambda b, mc, nc, info: self._lib.ctmr_known_export(self._h, b[0].ctypes.data, b[0].nbytes, C.byref(info)),
            lambda mc, nc: (np.empty(mc + 48 * nc, np.uint8),))
        return buf[:info.image_bytes].tobytes()

    def known_export_device(self):
        """→ (meta bytes, torch uint8 tensor of the 48-byte member records on this engine's device; a view)."""
        (meta, members), info = self._known_export_call(
            lambda b, mc, nc, info: self._lib.ctmr_known_export_device(self._h, b[0].ctypes.data, mc, b[1].data_ptr(), nc, C.byref(info)),
            lambda mc, nc: (np.empty(mc, np.uint8), self._empty(nc * 48, True)))
        return meta[:info.meta_bytes].tobytes(), members[:info.members * 48]

    def known_import(self, image, world=1, rank=0) -> dict:
        """Every member of `image` this rank takes, as SetInsert would add it (world = 1: all of them)."""
        image = bytes(image)
        st = N.KnownImportStats()
        self._ck(self._lib.ctmr_known_import(self._h, image, len(image), world, rank, C.byref(st)))
        return self._stats_dict(st)

    def known_import_device(self, meta, d_members, world=1, rank=0) -> dict:
        """known_import with the member records in device memory: a torch uint8 tensor (or a device pointer)."""
        meta = bytes(meta)
        n, ptr = self._members_ptr(d_members)
        st = N.KnownImportStats()
        self._ck(self._lib.ctmr_known_import_device(self._h, meta, len(meta), ptr, n, world, rank, C.byref(st)))
        return self._stats_dict(st)

    # ---- bulk SetContains / SetRemove over an image's member records (include/ctmr.h ctmr_known_query* /
    # ctmr_known_remove*; CPU twins: known_image.query / known_image.subtract)
    @staticmethod
    def _header_counts(buf):
        """(member records, host-section members) as the header of an image or its meta part has them, held to what
        `buf` could carry (a damaged header: the library refuses it)."""
        from .known_image import _HEADER
        if len(buf) < 64:
            return 0, 0
        h = _HEADER.unpack_from(buf, 0)
        return min(h[6], len(buf) // 48), min(h[8], len(buf) // 8)

    def known_query(self, image, world=1, rank=0):
        """SetContains for every member of `image` → (flags: numpy uint8 per member record, 1 = held, 0 = not, 2 = another
        rank's; host_flags: the same per host-section member; stats dict).  Read-only."""
        image = bytes(image)
        n, n_host = self._header_counts(image)
        flags, host_flags = np.empty(max(n, 1), np.uint8), np.empty(max(n_host, 1), np.uint8)
        st = N.KnownProbeStats()
        self._ck(self._lib.ctmr_known_query(self._h, image, len(image), world, rank, flags.ctypes.data, n,
                                            host_flags.ctypes.data, n_host, C.byref(st)))
        return flags[:n], host_flags[:n_host], self._stats_dict(st)

    def known_query_device(self, meta, d_members, world=1, rank=0):
        """known_query with the member records in device memory (a torch uint8 tensor) → (flags: torch uint8 tensor on
        this engine's device, host_flags: numpy uint8, stats dict)."""
        meta = bytes(meta)
        n, ptr = self._members_ptr(d_members)
        n_host = self._header_counts(meta)[1]
        flags = self._empty(max(n, 1), True)
        host_flags = np.empty(max(n_host, 1), np.uint8)
        st = N.KnownProbeStats()
        self._ck(self._lib.ctmr_known_query_device(self._h, meta, len(meta), ptr, n, world, rank, flags.data_ptr(), n,
                                                   host_flags.ctypes.data, n_host, C.byref(st)))
        return flags[:n], host_flags[:n_host], self._stats_dict(st)

    def known_remove(self, image, world=1, rank=0) -> dict:
        """SetRemove for every member of `image` this rank takes; all or nothing on a malformed image.  → stats dict
        (hits = members removed)."""
        image = bytes(image)
        st = N.KnownProbeStats()
        self._ck(self._lib.ctmr_known_remove(self._h, image, len(image), world, rank, C.byref(st)))
        return self._stats_dict(st)

    def known_remove_device(self, meta, d_members, world=1, rank=0) -> dict:
        """known_remove with the member records in device memory (a torch uint8 tensor)."""
        meta = bytes(meta)
        n, ptr = self._members_ptr(d_members)
        st = N.KnownProbeStats()
        self._ck(self._lib.ctmr_known_remove_device(self._h, meta, len(meta), ptr, n, world, rank, C.byref(st)))
        return self._stats_dict(st)

    # ---- per-issuer known-serial lists (include/ctmr.h ctmr_known_lists*; CPU twin: known_image.known_lists)
    def _lists_call(self, fn, device, caps):
        """The call of the four list writers: fn(text address, text_cap, ids address, ids_cap, offsets address, n_offs,
        info), first with the caller's guess caps = (text_cap, ids_cap, n_offs), and a second, exact time only when
        that was short (CTMR_E_RANGE fills `info`).  → (text: numpy uint8 or (device) a torch tensor, ids: bytes, text
        offsets, ID offsets (u64, issuers + 1 each), info, the caps of the last call)"""
        info = N.KnownListsInfo()

        def call(text_cap, ids_cap, n_offs):
            bufs = self._empty(max(text_cap, 1), device), np.empty(max(ids_cap, 1), np.uint8), np.empty(max(n_offs, 2), np.uint64)
            return fn(_addr(bufs[0]), text_cap, bufs[1].ctypes.data, ids_cap, bufs[2].ctypes.data, n_offs, C.byref(info)), bufs
        (text, ids, offs), caps = self._sized_call(call, caps, lambda: (info.text_bytes, info.ids_bytes, 2 * (info.issuers + 1)))
        g = info.issuers
        return text[:info.text_bytes], ids[:info.ids_bytes].tobytes(), offs[:g + 1].copy(), offs[g + 1:2 * g + 2].copy(), info, caps

    @staticmethod
    def _list_ids(ids, ioff, info):
        return [ids[ioff[k]:ioff[k + 1]] for k in range(info.issuers)]

    @staticmethod
    def _list_pairs(text, ids, toff, ioff, info):
        return [(i, text[toff[k]:toff[k + 1]].tobytes()) for k, i in enumerate(Engine._list_ids(ids, ioff, info))]

    def _known_lists_call(self, device, now):
        """One call sized by the bound (81 B per live member, the host-store text as large as last time), which writes
        without a separate count pass, and a second, exact one only when that was short."""
        fn = self._lib.ctmr_known_lists_device if device else self._lib.ctmr_known_lists
        caps = (81 * self.table_info().occupied + getattr(self, "_known_lists_host", 1 << 12),
                getattr(self, "_known_lists_ids", 1 << 12), getattr(self, "_known_lists_offs", 256))
        *out, info, (_, ids_cap, n_offs) = self._lists_call(lambda *args: fn(self._h, int(now), *args), device, caps)
        self._known_lists_host = max(info.text_bytes - 81 * info.members, 1 << 12)
        self._known_lists_ids, self._known_lists_offs = max(ids_cap, info.ids_bytes), max(n_offs, 2 * (info.issuers + 1))
        return (*out, info)

    def known_lists_raw(self, now):
        """→ (text: numpy uint8 of info.text_bytes, ids: bytes, text offsets, ID offsets (u64, issuers + 1 each), info)."""
        return self._known_lists_call(False, now)

    def known_lists(self, now) -> list:
        """[(Issuer.ID bytes, list text bytes)] in ID order: the serials of every set not expired at `now` (unix seconds),
        one lowercase hex line each — what LocalDiskBackend.StoreKnownCertificateList writes per issuer."""
        return self._list_pairs(*self.known_lists_raw(now))

    def known_lists_device(self, now):
        """→ ([Issuer.ID bytes], text offsets (numpy u64, issuers + 1), torch uint8 tensor of the text on this engine's
        device; a view)."""
        text, ids, toff, ioff, info = self._known_lists_call(True, now)
        return self._list_ids(ids, ioff, info), toff, text

    def store_known_lists(self, writer, now) -> int:
        """StoreKnownCertificateList for every list at `now` through a host_writeback.HostWriter (LocalDiskBackend: one
        file <root>/<Issuer.ID> per list; NoopBackend: nothing).  → the lists handed to the backend."""
        text, ids, toff, ioff, info = self.known_lists_raw(now)
        writer.store_known_lists(ids, ioff, text, toff)
        return int(info.issuers)

    # ---- the same lists straight from an image, with no table behind them (include/ctmr.h ctmr_known_image_lists*,
    # DESIGN.md §17; CPU twin: known_image.image_lists)
    def _known_image_lists_call(self, fn, device, n, buf):
        """One call sized by the bound — 81 B per member record, the host section's lines at most 2 B per octet of the
        section, as the header of the image or meta part `buf` has it, held to what `buf` could carry — and a second,
        exact one only for IDs or offsets beyond the guess."""
        from .known_image import _HEADER
        host_bytes = min(_HEADER.unpack_from(buf, 0)[7], len(buf)) if len(buf) >= 64 else 0
        return self._lists_call(fn, device, (81 * n + 2 * host_bytes + 1, 1 << 12, 256))[:5]

    def known_image_lists_raw(self, image, now):
        """known_lists_raw of the sets `image` holds, read where they lie: one line per member record in the image's
        order (a canonical image gives sorted lists).  The engine's own sets and issuers play no part.
        → (text: numpy uint8, ids: bytes, text offsets, ID offsets (u64, issuers + 1 each), info)."""
        image = bytes(image)
        return self._known_image_lists_call(lambda *args: self._lib.ctmr_known_image_lists(self._h, image, len(image), int(now), *args),
                                            False, self._header_counts(image)[0], image)

    def known_image_lists(self, image, now) -> list:
        """[(Issuer.ID bytes, list text bytes)] in ID order of the sets `image` holds that are not expired at `now`."""
        return self._list_pairs(*self.known_image_lists_raw(image, now))

    def known_image_lists_device(self, meta, d_members, now):
        """known_image_lists with the member records in device memory (a torch uint8 tensor) → ([Issuer.ID bytes], text
        offsets (numpy u64, issuers + 1), torch uint8 tensor of the text on this engine's device; a view)."""
        meta = bytes(meta)
        n, ptr = self._members_ptr(d_members)
        text, ids, toff, ioff, info = self._known_image_lists_call(
            lambda *args: self._lib.ctmr_known_image_lists_device(self._h, meta, len(meta), ptr, n, int(now), *args), True, n, meta)
        return self._list_ids(ids, ioff, info), toff, text

    def store_image_lists(self, writer, image, now) -> int:
        """store_known_lists for the lists of `image` at `now`.  → the lists handed to the backend."""
        text, ids, toff, ioff, info = self.known_image_lists_raw(image, now)
        writer.store_known_lists(ids, ioff, text, toff)
        return int(info.issuers)

    # ---- serials looked up in an image whatever their expiration date (include/ctmr.h ctmr_known_image_find*, DESIGN.md
    # §25; CPU twin: known_image.find)
    def known_image_find(self, known, probes, now):
        """For every member of the probe image `probes` (known_image.probes builds one): under how many sets of `known`
        kept at `now` the same Issuer.ID holds the same serial, and the lowest and highest exp hour among them.
        → (hits per member record of `probes`, host_hits per host-section member: numpy known_image.HIT_DTYPE; info dict).
        The engine's own sets and issuers play no part."""
        from .known_image import HIT_DTYPE
        known, probes = bytes(known), bytes(probes)
        n, n_host = self._header_counts(probes)
        hits, host_hits = np.zeros(max(n, 1), HIT_DTYPE), np.zeros(max(n_host, 1), HIT_DTYPE)
        info = N.KnownFindInfo()
        self._ck(self._lib.ctmr_known_image_find(self._h, known, len(known), probes, len(probes), int(now), hits.ctypes.data, n,
                                                 host_hits.ctypes.data, n_host, C.byref(info)))
        return hits[:n], host_hits[:n_host], self._stats_dict(info)

    def known_image_find_device(self, k_meta, d_k_members, p_meta, d_p_members, now):
        """known_image_find with the member records of both images in device memory (torch uint8 tensors) → (hits: torch
        int32 tensor of shape (probes, 4) on this engine's device — records, first_hour, last_hour, 0 —, host_hits: numpy
        known_image.HIT_DTYPE, info dict)."""
        import torch
        from .known_image import HIT_DTYPE
        k_meta, p_meta = bytes(k_meta), bytes(p_meta)
        nk, kptr = self._members_ptr(d_k_members)
        n, pptr = self._members_ptr(d_p_members)
        n_host = self._header_counts(p_meta)[1]
        hits = torch.empty((max(n, 1), 4), dtype=torch.int32, device=self._dev)
        host_hits = np.zeros(max(n_host, 1), HIT_DTYPE)
        info = N.KnownFindInfo()
        self._ck(self._lib.ctmr_known_image_find_device(self._h, k_meta, len(k_meta), kptr, nk, p_meta, len(p_meta), pptr, n,
                                                        int(now), hits.data_ptr(), n, host_hits.ctypes.data, n_host,
                                                        C.byref(info)))
        return hits[:n], host_hits[:n_host], self._stats_dict(info)

    def known_find(self, probes, now):
        """known_image_find over the engine's own sets: known_export_device followed by known_image_find_device, nothing
        cleverer.  → (hits, host_hits: numpy known_image.HIT_DTYPE; info dict)."""
        from .known_image import HIT_DTYPE
        hits, host_hits, info = self.known_image_find_device(*self._own_and_probes(probes), now)
        return hits.cpu().numpy().view(HIT_DTYPE).reshape(-1), host_hits, info

    def _own_and_probes(self, probes):
        """The operands of known_find and known_split: the engine's own sets exported to the device, and the probe image
        cut into its meta part and its member records on the device → (k_meta, d_k, p_meta, d_p)"""
        probes = bytes(probes)
        at = len(probes) - 48 * self._header_counts(probes)[0]
        k_meta, d_k = self.known_export_device()
        return k_meta, d_k, probes[:at], self._upload(probes[at:])

    # ---- an image partitioned by a probe image, the hour as wildcard (include/ctmr.h ctmr_known_image_split*, DESIGN.md
    # §28; CPU twin: known_image.split)
    @staticmethod
    def _split_info(info) -> dict:
        out = {f: getattr(info, f) for f in ("probes", "host_probes", "sets_kept", "members_read")}
        out["hit"], out["miss"] = Engine._stats_dict(info.hit), Engine._stats_dict(info.miss)
        return out

    @staticmethod
    def _split_want(want):
        want = tuple(want)
        if set(want) - {"hit", "miss"}:
            raise ValueError("want: \"hit\" and / or \"miss\", not %r" % (want,))
        return "hit" in want, "miss" in want

    def known_image_split(self, known, probes, now, want=("hit", "miss")):
        """`known` partitioned by the probe image `probes` with the hour as wildcard → (hit, miss, info dict): two images
        (bytes; None for a side `want` leaves out).  hit holds every member record and host pair of a set of `known`
        kept at `now` that equals a probe — same Issuer.ID, same serial —, miss every other one of a kept set; both in
        the order of `known`, nothing sorted, deduplicated or moved between the sections.  One call, the buffers sized by
        the bound (each result is at most as large as `known`).  The engine's own sets and issuers play no part."""
        known, probes = bytes(known), bytes(probes)
        sides = [np.empty(len(known), np.uint8) if w else None for w in self._split_want(want)]
        info = N.KnownSplitInfo()
        args = [a for s in sides for a in ((s.ctypes.data, s.nbytes) if s is not None else (None, 0))]
        self._ck(self._lib.ctmr_known_image_split(self._h, known, len(known), probes, len(probes), int(now), *args, C.byref(info)))
        hit, miss = (s[:i.image_bytes].tobytes() if s is not None else None for s, i in zip(sides, (info.hit, info.miss)))
        return hit, miss, self._split_info(info)

    def known_image_split_device(self, k_meta, d_k_members, p_meta, d_p_members, now, want=("hit", "miss")):
        """known_image_split with the member records of both operands in device memory (torch uint8 tensors) →
        ((hit meta bytes, torch uint8 tensor of hit's member records on this engine's device; a view), the same for miss,
        info dict); None for a side `want` leaves out.  One call, the buffers sized by the bound."""
        k_meta, p_meta = bytes(k_meta), bytes(p_meta)
        nk, kptr = self._members_ptr(d_k_members)
        n, pptr = self._members_ptr(d_p_members)
        sides = [(np.empty(len(k_meta), np.uint8), self._empty(max(nk, 1) * 48, True)) if w else None for w in self._split_want(want)]
        info = N.KnownSplitInfo()
        args = [a for s in sides for a in ((s[0].ctypes.data, s[0].nbytes, s[1].data_ptr(), nk) if s else (None, 0, None, 0))]
        self._ck(self._lib.ctmr_known_image_split_device(self._h, k_meta, len(k_meta), kptr, nk, p_meta, len(p_meta), pptr, n, int(now),
                                                         *args, C.byref(info)))
        hit, miss = ((s[0][:i.meta_bytes].tobytes(), s[1][:i.members * 48]) if s else None for s, i in zip(sides, (info.hit, info.miss)))
        return hit, miss, self._split_info(info)

    def known_split(self, probes, now, want=("hit", "miss")):
        """known_image_split over the engine's own sets: known_export_device followed by known_image_split_device, as
        known_find does.  → (hit, miss, info dict): images as bytes."""
        hit, miss, info = self.known_image_split_device(*self._own_and_probes(probes), now, want)
        return tuple(s[0] + s[1].cpu().numpy().tobytes() if s else None for s in (hit, miss)) + (info,)

    # ---- the filter cascade of a revoked / not-revoked image pair (include/ctmr.h ctmr_cascade_*; CPU
    # twin: cascade.build / cascade.query)
    @staticmethod
    def _cascade_params(params):
        salt = bytes(params.salt)
        if len(salt) > 16:
            raise ValueError("a salt of at most 16 octets")
        return N.CascadeParams(params.k_first, params.bpk_first_q8, params.k_rest, params.bpk_rest_q8, params.max_layers, len(salt),
                               (C.c_uint8 * 16)(*salt))

    @staticmethod
    def _cascade_info(info) -> dict:
        out = {f: getattr(info, f) for f, _ in info._fields_ if f != "layer"}
        out["layer"] = [(l.level, l.k, l.m_bits, l.offset, l.n_held) for l in info.layer[:info.layers]]
        return out

    def _cascade_build(self, fn, n_revoked, params, device):
        """The first guess — twice the first layer of n_revoked records, plus the tables — and one exact second call
        when it was short: fn(params, out address, cap, info).  A call that is short has still built every layer (the
        size is known only then), so the second call builds the cascade again: the guess is made generous for that
        reason.  → (the buffer, info)"""
        from .cascade import HEADER_BYTES, LAYER_BYTES, layer_bits
        p, info = self._cascade_params(params), N.CascadeInfo()
        first = ((layer_bits(n_revoked, params.bpk_first_q8) + 7) // 8 + 63) & ~63

        def call(cap):
            out = self._empty(cap, device)
            return fn(C.byref(p), _addr(out), cap, C.byref(info)), out
        out, _ = self._sized_call(call, (2 * first + ((HEADER_BYTES + LAYER_BYTES * params.max_layers + 63) & ~63),),
                                  lambda: (max(info.bytes, 64),))
        return out[:info.bytes], self._cascade_info(info)

    def cascade_build(self, revoked, known, now, params):
        """The filter cascade (cascade.py, format CTMRCASC v1) that answers 1 for every member record of the sets of the
        image `revoked` kept at `now` and 0 for every one of `known`; params: cascade.Params (cascade.crlite_params
        makes CRLite's choice).  → (cascade bytes, info dict).  Raises CtmrError (CTMR_E_INVAL) when max_layers layers do
        not finish it — the operands share a key.  The engine's own sets and issuers play no part."""
        revoked, known = bytes(revoked), bytes(known)
        out, info = self._cascade_build(
            lambda p, out, cap, info: self._lib.ctmr_cascade_build(self._h, revoked, len(revoked), known, len(known), int(now), p, out, cap, info),
            self._header_counts(revoked)[0], params, False)
        return out.tobytes(), info

    def cascade_build_device(self, r_meta, d_r_members, s_meta, d_s_members, now, params):
        """cascade_build with the member records of both operands in device memory (torch uint8 tensors) → (the cascade:
        a torch uint8 tensor on this engine's device; a view, info dict)."""
        r_meta, s_meta = bytes(r_meta), bytes(s_meta)
        nr, rptr = self._members_ptr(d_r_members)
        ns, sptr = self._members_ptr(d_s_members)
        return self._cascade_build(
            lambda p, out, cap, info: self._lib.ctmr_cascade_build_device(self._h, r_meta, len(r_meta), rptr, nr, s_meta, len(s_meta), sptr, ns,
                                                                          int(now), p, out, cap, info),
            nr, params, True)

    def cascade_query(self, cascade, probes):
        """One byte per member record of the image `probes`, all sets, in record order: 1 = `cascade` says revoked.
        → (numpy uint8, info dict)"""
        cascade, probes = bytes(cascade), bytes(probes)
        n = self._header_counts(probes)[0]
        out, info = np.zeros(max(n, 1), np.uint8), N.CascadeQueryInfo()
        self._ck(self._lib.ctmr_cascade_query(self._h, cascade, len(cascade), probes, len(probes), out.ctypes.data, n, C.byref(info)))
        return out[:n], self._stats_dict(info)

    def cascade_query_device(self, d_cascade, p_meta, d_p_members):
        """cascade_query with the cascade and the member records of the probe image in device memory (torch uint8
        tensors) → (torch uint8 tensor of the answers on this engine's device, info dict)."""
        self._tensor(d_cascade, "d_cascade")
        p_meta = bytes(p_meta)
        n, pptr = self._members_ptr(d_p_members)
        out, info = self._empty(max(n, 1), True), N.CascadeQueryInfo()
        self._ck(self._lib.ctmr_cascade_query_device(self._h, d_cascade.data_ptr(), d_cascade.numel(), p_meta, len(p_meta), pptr, n,
                                                     out.data_ptr(), n, C.byref(info)))
        return out[:n], self._stats_dict(info)

    def known_revoked_cascade(self, crls, digests, now, params=None, each=False):
        """The filter cascade of the engine's known certificates against `crls`: crl_probes[_each]_device →
        known_export_device → known_image_split_device → cascade_build_device, with no member record in host memory.
        crls, digests, each: as for known_revoked.  params: cascade.Params; None: cascade.crlite_params of the two
        results' record counts, no salt.  → (the cascade on the device, info dict with the split's under "split"[,
        verdicts])."""
        from .cascade import crlite_params
        p_meta, d_p, verdicts = self._crl_probes_staged(crls, digests, each)
        k_meta, d_k = self.known_export_device()
        (hit_meta, d_hit), (miss_meta, d_miss), split = self.known_image_split_device(k_meta, d_k, p_meta, d_p, now)
        if params is None:
            params = crlite_params(split["hit"]["members"], split["miss"]["members"])
        d_cascade, info = self.cascade_build_device(hit_meta, d_hit, miss_meta, d_miss, now, params)
        info["split"] = split
        return (d_cascade, info, verdicts) if each else (d_cascade, info)

    # ---- the Redis protocol stream of an image (include/ctmr.h ctmr_known_image_resp*; CPU twin:
    # known_image.image_resp)
    def _known_resp_call(self, fn, device, buf, n, members_per_command):
        """One call sized by the bound the header of the image or meta part `buf` gives (include/ctmr.h) and a second,
        exact one only when the header understated the image: fn(per, text address, text_cap, info).  → the stream"""
        from .known_image import _HEADER, resp_bound
        per = int(members_per_command)
        if not 0 <= per < 1 << 32:
            raise ValueError("members_per_command %r" % (members_per_command,))
        h = _HEADER.unpack_from(buf, 0) if len(buf) >= 64 else (0,) * 10
        bound = resp_bound(n, min(h[5], len(buf) // 24), min(h[7], len(buf)), min(h[8], len(buf) // 8), min(max(per, 1), 1 << 20))
        info = N.KnownRespInfo()

        def call(cap):
            text = self._empty(max(cap, 1), device)
            return fn(per, _addr(text), cap, C.byref(info)), text
        return self._sized_call(call, (bound,), lambda: (info.text_bytes,))[0][:info.text_bytes]

    def known_image_resp(self, image, members_per_command=512) -> bytes:
        """The SADD + EXPIREAT stream of the sets `image` holds, as `redis-cli --pipe` loads it: the keys in order, the
        member records in the image's order, at most `members_per_command` members per SADD.  The engine's own sets and
        issuers play no part."""
        image = bytes(image)
        return self._known_resp_call(lambda per, *args: self._lib.ctmr_known_image_resp(self._h, image, len(image), per, *args),
                                     False, image, self._header_counts(image)[0], members_per_command).tobytes()

    def known_image_resp_device(self, meta, d_members, members_per_command=512):
        """known_image_resp with the member records in device memory (a torch uint8 tensor) → torch uint8 tensor of the
        stream on this engine's device; a view."""
        meta = bytes(meta)
        n, ptr = self._members_ptr(d_members)
        return self._known_resp_call(lambda per, *args: self._lib.ctmr_known_image_resp_device(self._h, meta, len(meta), ptr, n, per, *args),
                                     True, meta, n, members_per_command)

    def known_resp(self, members_per_command=512) -> bytes:
        """The stream of the engine's own sets: known_image_resp of its sorted export.  The order setting
        (set_known_order) is left as it was found."""
        was = self._known_order
        self.set_known_order(N.KNOWN_ORDER_SORTED)
        try:
            image = self.known_export()
        finally:
            self.set_known_order(was)
        return self.known_image_resp(image, members_per_command)

    # ---- a Redis protocol stream as it lies → an image (include/ctmr.h ctmr_known_resp_image*; CPU twin:
    # known_image.resp_image)
    def known_resp_image(self, stream) -> bytes:
        """The image of a stream of SADD / EXPIREAT commands (what `redis-cli --pipe` loads, what known_image_resp
        writes): member records in stream order, neither sorted nor deduplicated — known_merge(N.KNOWN_UNION, image)
        does that.  The engine's own sets and issuers play no part."""
        stream = bytes(stream)
        info = N.KnownRespImageInfo()

        def call(cap):
            out = np.empty(cap, np.uint8)
            return self._lib.ctmr_known_resp_image(self._h, stream, len(stream), out.ctypes.data, cap, C.byref(info)), out
        out, _ = self._sized_call(call, (1 << 16,), lambda: (info.image_bytes,))
        return out[:info.image_bytes].tobytes()

    def known_resp_image_device(self, d_stream, n=None):
        """known_resp_image of the first n bytes of a torch uint8 tensor on this engine's device (all of it by default;
        any alignment) → (meta bytes, torch uint8 tensor of the member records on the device; a view).  The records are
        sized by their bound (n / 6), the meta by a second call when 64 KiB were short."""
        self._tensor(d_stream, "d_stream")
        n = d_stream.numel() if n is None else int(n)
        if not 0 <= n <= d_stream.numel():
            raise ValueError("n = %r of %d bytes" % (n, d_stream.numel()))
        ptr = d_stream.data_ptr() if n else None
        info = N.KnownRespImageInfo()
        members_cap = max(n // 6, 1)
        out = self._empty(members_cap * 48, True)

        def call(meta_cap):
            meta = np.empty(meta_cap, np.uint8)
            return self._lib.ctmr_known_resp_image_device(self._h, ptr, n, meta.ctypes.data, meta_cap, out.data_ptr(), members_cap,
                                                          C.byref(info)), meta
        meta, (meta_cap,) = self._sized_call(call, (getattr(self, "_resp_meta_cap", 1 << 16),), lambda: (info.meta_bytes,))
        self._resp_meta_cap = max(meta_cap, info.meta_bytes)
        return meta[:info.meta_bytes].tobytes(), out[:info.members * 48]

    # ---- DER CertificateLists → a probe image (include/ctmr.h ctmr_crl_probes*; CPU twin:
    # crl.probes_image)
    @staticmethod
    def _crl_args(crls, digests):
        """A list of CRLs (bytes each) or (blob, offsets) → (blob or None, total length, offsets u64[n + 1], n, digests)."""
        if isinstance(crls, tuple):
            blob, offsets = crls
            offsets = np.ascontiguousarray(offsets, np.uint64)
            total = blob.numel() if hasattr(blob, "data_ptr") else len(blob)
        else:
            crls = [bytes(c) for c in crls]
            blob = b"".join(crls)
            offsets = np.zeros(len(crls) + 1, np.uint64)
            offsets[1:] = np.cumsum([len(c) for c in crls], dtype=np.uint64)
            total = len(blob)
        n = len(offsets) - 1
        digests = b"".join(bytes(d) for d in digests) if not isinstance(digests, (bytes, bytearray)) else bytes(digests)
        if n < 0 or len(digests) != 32 * n:
            raise ValueError("one 32-byte digest per CRL")
        return blob, total, offsets, n, digests

    def _crl_fail(self, rc, cinfo):
        def error(msg):
            from .crl import CrlError
            return CrlError(cinfo.bad_offset, msg, cinfo.bad_crl)
        self._ck_at(rc, cinfo.bad_crl, error)

    def crl_probes(self, crls, digests):
        """The probe image of the revoked serials of `crls` — a list of DER CRLs, or (blob bytes, offsets) — whose
        issuers' SPKI digests are `digests`: one set per digest under exp hour 0, member records in input order, what
        known_image_find takes as `probes`.  → (image bytes, info dict).  Raises crl.CrlError naming the lowest CRL
        outside the grammar and the offset.  The engine's own sets and issuers play no part."""
        return self._crl_probes(crls, digests, False)[:2]

    def crl_probes_each(self, crls, digests):
        """crl_probes with every CRL judged on its own (ctmr_crl_probes_each; CPU twin: crl.probes_each): a
        CRL outside the grammar raises nothing and contributes nothing.  → (image bytes of the good CRLs, info dict,
        verdicts: (bad_offset, records, long_entries) per CRL, bad_offset crl.NONE for a good one)."""
        return self._crl_probes(crls, digests, True)

    @staticmethod
    def _crl_verdicts(n, each):
        """→ (the ctmr_crl_verdict array of a call or None, what reads it into a list)"""
        if not each:
            return None, lambda: None
        v = (N.CrlVerdict * max(n, 1))()
        return v, lambda: [(x.bad_offset, x.records, x.long_entries) for x in v[:n]]

    def _crl_probes(self, crls, digests, each):
        blob, total, offsets, n, digests = self._crl_args(crls, digests)
        blob = bytes(blob)
        info, cinfo = N.KnownImageInfo(), N.CrlInfo()
        verdicts, read = self._crl_verdicts(n, each)

        def call(cap):
            out = np.empty(max(cap, 64), np.uint8)
            args = (self._h, blob, total, offsets.ctypes.data, n, digests, out.ctypes.data, out.nbytes, C.byref(info), C.byref(cinfo))
            return (self._lib.ctmr_crl_probes_each(*args, C.byref(verdicts)) if each else self._lib.ctmr_crl_probes(*args)), out
        out, _ = self._sized_call(call, (64 + 56 * n + 48 * (total // 6),), lambda: (info.image_bytes,), lambda rc: self._crl_fail(rc, cinfo))
        return out[:info.image_bytes].tobytes(), self._stats_dict(cinfo), read()

    def crl_probes_device(self, d_crls, offsets, digests, exact=None):
        """crl_probes of a torch uint8 tensor on this engine's device (any alignment) holding the CRLs back to back;
        offsets: u64[n + 1], ascending from 0 to the tensor's length → (meta bytes, torch uint8 tensor of the member
        records on the device; a view, info dict).
        Sizing.  The bound of the records is length / 6 of them, 8 bytes of records per byte of blob; a real CRL needs
        about 1.3.  exact=False allocates the bound and makes one call (a second only when the meta's first guess was
        short); exact=True asks for the sizes first (the two-call convention: every pass but the last runs twice) and
        allocates what they say.  The default takes the bound while it is at most a quarter of the device's free memory,
        and asks first otherwise."""
        return self._crl_probes_device(d_crls, offsets, digests, exact, False)[:3]

    def crl_probes_each_device(self, d_crls, offsets, digests, exact=None):
        """crl_probes_device with every CRL judged on its own (ctmr_crl_probes_each_device) → (meta bytes, member records
        on the device, info dict, verdicts as crl_probes_each gives them)."""
        return self._crl_probes_device(d_crls, offsets, digests, exact, True)

    def _crl_probes_device(self, d_crls, offsets, digests, exact, each):
        import torch
        self._tensor(d_crls, "d_crls")
        _, total, offsets, n, digests = self._crl_args((d_crls, offsets), digests)
        ptr = d_crls.data_ptr() if total else None
        info, cinfo = N.KnownImageInfo(), N.CrlInfo()
        verdicts, read = self._crl_verdicts(n, each)
        members_cap = max(total // 6, 1)
        if exact is None:
            exact = 48 * members_cap > torch.cuda.mem_get_info(self.device)[0] // 4

        def fn(meta, meta_cap, d_out, members_cap):
            args = (self._h, ptr, total, offsets.ctypes.data, n, digests, _addr(meta), meta_cap, _addr(d_out), members_cap, C.byref(info),
                    C.byref(cinfo))
            return self._lib.ctmr_crl_probes_each_device(*args, C.byref(verdicts)) if each else self._lib.ctmr_crl_probes_device(*args)

        def check(rc):
            self._crl_fail(rc, cinfo)
        if exact:
            meta, _, out, _ = self._sizes_first(fn, (None, 0, None, 0), lambda: (
                np.empty(info.meta_bytes, np.uint8), info.meta_bytes, self._empty(max(info.members, 1) * 48, True), max(info.members, 1)), check)
        else:
            out = self._empty(members_cap * 48, True)

            def call(meta_cap):
                meta = np.empty(meta_cap, np.uint8)
                return fn(meta, meta_cap, out, members_cap), meta
            meta, _ = self._sized_call(call, (64 + 56 * n + (1 << 12),), lambda: (info.meta_bytes,), check)
        return meta[:info.meta_bytes].tobytes(), out[:info.members * 48], self._stats_dict(cinfo), read()

    def known_revoked(self, crls, digests, now, each=False):
        """Which revoked serials the engine knows, and until when they matter: crl_probes_device → known_export_device →
        known_image_find_device, with no probe image in host memory.  crls: a list of DER CRLs, or (torch uint8 tensor
        on this engine's device, offsets).  → (the probe image's meta, hits: numpy known_image.HIT_DTYPE per member
        record of the probe image in its order, host_hits per host-section pair).  each=True: every CRL is judged on its
        own (crl_probes_each_device): the CRLs outside the grammar are left out instead of failing the call, and the
        verdicts of all CRLs are a fourth element."""
        from .known_image import HIT_DTYPE
        p_meta, d_p, verdicts = self._crl_probes_staged(crls, digests, each)
        k_meta, d_k = self.known_export_device()
        hits, host_hits, _ = self.known_image_find_device(k_meta, d_k, p_meta, d_p, now)
        out = (p_meta, hits.cpu().numpy().view(HIT_DTYPE).reshape(-1), host_hits)
        return out + (verdicts,) if each else out

    def _crl_probes_staged(self, crls, digests, each):
        """The probe image of known_revoked and known_revoked_split: a list of CRLs goes to the device as one blob first
        → (the probe image's meta, its member records on the device, the verdicts (each) or None)"""
        if not isinstance(crls, tuple):
            blob, _, offsets, _, digests = self._crl_args(crls, digests)
            crls = (self._upload(blob), offsets)
        p_meta, d_p, _, verdicts = self._crl_probes_device(crls[0], crls[1], digests, None, each)
        return p_meta, d_p, verdicts

    def known_revoked_split(self, crls, digests, now, each=False):
        """The engine's known certificates in two images, the revoked and the others: crl_probes_device →
        known_export_device → known_image_split_device, with no probe image and no member record in host memory.  crls,
        digests, each: as for known_revoked.  → ((hit meta, hit's member records on the device), (miss meta, miss's
        member records), info dict[, verdicts]).  The per-issuer lists of a revocation filter are two more calls:

            (hit_meta, d_hit), (miss_meta, d_miss), info = e.known_revoked_split(crls, digests, now)
            ids, offs, text = e.known_image_lists_device(hit_meta, d_hit, now)      # revoked/<Issuer.ID>
            ids, offs, text = e.known_image_lists_device(miss_meta, d_miss, now)    # known/<Issuer.ID>
        """
        p_meta, d_p, verdicts = self._crl_probes_staged(crls, digests, each)
        k_meta, d_k = self.known_export_device()
        out = self.known_image_split_device(k_meta, d_k, p_meta, d_p, now)
        return out + (verdicts,) if each else out

    def known_import_resp(self, stream, world=1, rank=0) -> dict:
        """The warm start from a reference deployment's Redis contents: every serials:: member of the stream (bytes, or
        a torch uint8 tensor on this engine's device) this rank takes, as SetInsert would add it.  Stream → member
        records on the device → known_import_device: no image in host memory."""
        if not hasattr(stream, "data_ptr"):
            stream = self._upload(bytes(stream))
        meta, d_members = self.known_resp_image_device(stream)
        return self.known_import_device(meta, d_members, world, rank)

    # ---- the order inside a set (include/ctmr.h ctmr_known_sort* / ctmr_set_known_order; CPU twin:
    # known_image.sort)
    _known_order = N.KNOWN_ORDER_ANY   # what set_known_order last set

    def set_known_order(self, order):
        """N.KNOWN_ORDER_SORTED: known_export* and known_lists* write each set's members / each expDate's lines in
        ascending byte-string order, so an export is a pure function of the sets held; N.KNOWN_ORDER_ANY (the default):
        any order."""
        self._ck(self._lib.ctmr_set_known_order(self._h, int(order)))
        self._known_order = int(order)

    def known_sort(self, image) -> bytes:
        """`image` with the member records of every set sorted on the GPU (repeats kept, meta unchanged)."""
        buf = np.frombuffer(bytes(image), np.uint8).copy()
        self._ck(self._lib.ctmr_known_sort(self._h, buf.ctypes.data if len(buf) else None, len(buf)))
        return buf.tobytes()

    def known_sort_device(self, meta, d_members):
        """Sorts the member records (a torch uint8 tensor on this engine's device) of the image whose meta part is
        `meta` in place, set by set."""
        meta = bytes(meta)
        n, ptr = self._members_ptr(d_members)
        self._ck(self._lib.ctmr_known_sort_device(self._h, meta, len(meta), ptr, n))

    # ---- set algebra on images (include/ctmr.h ctmr_known_merge*; CPU twins: known_image.union / minus /
    # intersect)
    def known_merge(self, op, a, b=None) -> bytes:
        """The canonical image of a ∪ b (N.KNOWN_UNION), a \\ b (N.KNOWN_MINUS) or a ∩ b (N.KNOWN_INTERSECT), set by set,
        on the GPU with no table behind it; b=None is the empty image (UNION then normalises a).  The engine's own sets
        play no part.  Sized by the bounds (|a| + |b| members, the two metas), so one call."""
        a = bytes(a)
        b = None if b is None else bytes(b)
        len_b = len(b) if b is not None else 0
        info = N.KnownImageInfo()

        def call(cap):
            out = np.empty(cap, np.uint8)
            return self._lib.ctmr_known_merge(self._h, int(op), a, len(a), b, len_b, out.ctypes.data, cap, C.byref(info)), out
        # (a second call only when host-section pairs moved into sets and issuers of their own)
        out, _ = self._sized_call(call, (len(a) + len_b + 64,), lambda: (info.image_bytes,))
        return out[:info.image_bytes].tobytes()

    def known_merge_device(self, op, a_meta, d_a, b_meta=None, d_b=None):
        """known_merge with the member records in device memory (torch uint8 tensors on this engine's device)
        → (meta bytes, torch uint8 tensor of the result's member records; a view)."""
        a_meta = bytes(a_meta)
        na, pa = self._members_ptr(d_a)
        nb, pb = (0, None) if b_meta is None else self._members_ptr(d_b)
        b_meta = None if b_meta is None else bytes(b_meta)
        hosts = self._header_counts(a_meta)[1] + (self._header_counts(b_meta)[1] if b_meta is not None else 0)
        meta_cap = len(a_meta) + (len(b_meta) if b_meta is not None else 0) + 64
        cap = (na + nb if op == N.KNOWN_UNION else na) + hosts
        meta = np.empty(meta_cap, np.uint8)
        out = self._empty(max(cap, 1) * 48, True)
        info = N.KnownImageInfo()
        self._ck(self._lib.ctmr_known_merge_device(self._h, int(op), a_meta, len(a_meta), pa, na, b_meta,
                                                   len(b_meta) if b_meta is not None else 0, pb, nb, meta.ctypes.data, meta_cap,
                                                   out.data_ptr(), cap, C.byref(info)))
        return meta[:info.meta_bytes].tobytes(), out[:info.members * 48]

    # ---- synthetic input (bench / tests)
    def synth_view_device(self, cfg: N.SynthConfig, first, n, align, d_starts, d_ends, d_payload, payload_cap,
                          d_issuer_idx, d_entry_type) -> int:
        """The synthetic certificates as an entry view, every certificate at a multiple of `align` bytes."""
        out = C.c_uint64()
        self._ck(self._lib.ctmr_synth_view_device(self._h, C.byref(cfg), first, n, align, d_starts, d_ends, d_payload, payload_cap,
                                                  d_issuer_idx, d_entry_type, C.byref(out)))
        return out.value

    def synth_device(self, cfg: N.SynthConfig, first, n, d_offsets, d_payload, payload_cap,
                     d_issuer_idx, d_entry_type) -> int:
        out = C.c_uint64()
        self._ck(self._lib.ctmr_synth_device(self._h, C.byref(cfg), first, n, d_offsets, d_payload, payload_cap, d_issuer_idx, d_entry_type,
                                             C.byref(out)))
        return out.value
