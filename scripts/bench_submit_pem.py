"""PEM certificate files through the ingestion pipeline as text (include/ctmr.h ctmr_submit_pem / ctmr_wait_pem; DESIGN.md
§23): one JSON line, also written to --out (default profiles/bench_submit_pem.json).  Nothing here is gated; nothing of it
had been measured before.

--submits distinct submits of --files one-certificate files each (the reference writes one file per certificate), every
submit's text in a buffer of ctmr_alloc_pinned.  Wall time, after one warm-up pass over all submits on the same engine (so
every certificate is known in the timed part of every leg, as in a warm start over a disk already read), of --rounds
passes:
  pem_async     ctmr_submit_pem, --in-flight tickets outstanding, ctmr_wait_pem for the oldest,
  sync_text     one ctmr_pem_decode + one ctmr_map_batch per submit, the issuer indices expanded by the host: the only
                route for PEM text before,
  packed_async  ctmr_submit_batch / ctmr_wait over the same certificates decoded beforehand, the DER in pinned buffers
                too, --in-flight tickets outstanding.
The text is about 4/3 of the DER's bytes and more (armor lines, eols): where the host link is the bound, pem_async sits
below 3/4 of packed_async; where the worker's host work per super-batch is, it sits lower still."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import pem_text as pt, synth, _native as N  # noqa: E402
from ct_mapreduce_amd.engine import RECORD_DTYPE  # noqa: E402

NONE = 2**64 - 1


def pinned(e, data):
    buf = e.pinned_array(len(data) + N.PAYLOAD_PAD)
    buf[:len(data)] = np.frombuffer(data, np.uint8)
    buf[len(data):] = 0
    return buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--submits", type=int, default=64)
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--in-flight", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_submit_pem.json"))
    args = ap.parse_args()
    cfg = synth.config(seed=20261020, n_issuers=64, dup_permille=100)
    K, per = args.submits, args.files
    n1 = K * per

    def engine():
        e = ctmr.Engine(device=0, table_slots=1 << 22, pair_slots=1 << 14)
        e.add_issuers(synth.issuers(cfg))
        e.set_filter(b"", False, synth.BASE_TIME)
        return e

    batch = synth.host_batch(cfg, 0, n1)
    off = batch.offsets.astype(np.uint64)
    texts, fbs = [], []
    for k in range(K):
        t, fb = pt.join([pt.write([batch.cert(i)]) for i in range(k * per, (k + 1) * per)])
        texts.append(t)
        fbs.append(fb)
    iss = [np.ascontiguousarray(batch.issuer_idx[k * per:(k + 1) * per], np.uint32) for k in range(K)]
    text_bytes, der_bytes = sum(len(t) for t in texts), int(off[n1] - off[0])
    rec = np.zeros(per, RECORD_DTYPE)
    new, first, bad = np.zeros(per, np.uint64), np.zeros(per + 1, np.uint64), np.zeros(per, np.uint64)
    info, st = N.PemDecodeInfo(), N.BatchStats()
    out = {"metric": "submit_pem", "submits": K, "files_per_submit": per, "in_flight": args.in_flight, "rounds": args.rounds,
           "text_bytes_per_pass": text_bytes, "der_bytes_per_pass": der_bytes}

    def rate(s, passes):
        return {"s": round(s, 4), "certs_per_s": n1 * passes / s, "text_GB_per_s": text_bytes * passes / s / 1e9,
                "der_GB_per_s": der_bytes * passes / s / 1e9}

    def in_flight(submit, wait, passes):
        pending, t0 = [], time.perf_counter()
        for k in range(K * passes):
            if len(pending) == args.in_flight:
                wait(pending.pop(0))
            pending.append(submit(k % K))
        for t in pending:
            wait(t)
        return time.perf_counter() - t0

    # ---- pem_async
    e = engine()
    lib, h = e._lib, e._h
    bufs = [pinned(e, t) for t in texts]

    def submit_pem(k):
        t = C.c_uint64(0)
        e._ck(lib.ctmr_submit_pem(h, bufs[k].ctypes.data, fbs[k].ctypes.data, per, iss[k].ctypes.data, C.byref(t)))
        return t.value

    def wait_pem(t):
        e._ck(lib.ctmr_wait_pem(h, t, per, rec.ctypes.data, new.ctypes.data, first.ctypes.data, bad.ctypes.data, C.byref(info), C.byref(st)))
        assert info.certificates == per and info.bad_file == NONE
    in_flight(submit_pem, wait_pem, 1)
    out["pem_async"] = rate(in_flight(submit_pem, wait_pem, args.rounds), args.rounds)
    e.close()
    # ---- sync_text: pageable or pinned makes no difference to a call that stages and drains; the same pinned buffers
    e = engine()
    lib, h = e._lib, e._h
    bufs = [pinned(e, t) for t in texts]
    pay = np.zeros(max(len(t) for t in texts) * 3 // 4 + N.PAYLOAD_PAD, np.uint8)
    offs = np.zeros(per + 1, np.uint64)
    et = np.zeros(per, np.uint8)

    def sync_pass(passes):
        t0 = time.perf_counter()
        for k in range(K * passes):
            k %= K
            e._ck(lib.ctmr_pem_decode(h, bufs[k].ctypes.data, fbs[k].ctypes.data, per, pay.ctypes.data, len(pay), offs.ctypes.data, per,
                                      first.ctypes.data, C.byref(info)))
            idx = np.repeat(iss[k], np.diff(first.astype(np.int64)))
            e._ck(lib.ctmr_map_batch(h, pay.ctypes.data, offs.ctypes.data, idx.ctypes.data, et.ctypes.data, per, rec.ctypes.data, new.ctypes.data,
                                     C.byref(st)))
        return time.perf_counter() - t0
    sync_pass(1)
    out["sync_text"] = rate(sync_pass(args.rounds), args.rounds)
    e.close()
    # ---- packed_async
    e = engine()
    lib, h = e._lib, e._h
    ders, doffs = [], []
    for k in range(K):
        lo, hi = int(off[k * per]), int(off[(k + 1) * per])
        ders.append(pinned(e, batch.payload[lo:hi].tobytes()))
        doffs.append(np.ascontiguousarray(off[k * per:(k + 1) * per + 1] - np.uint64(lo)))

    def submit_packed(k):
        t = C.c_uint64(0)
        e._ck(lib.ctmr_submit_batch(h, ders[k].ctypes.data, doffs[k].ctypes.data, iss[k].ctypes.data, None, per, C.byref(t)))
        return t.value

    def wait_packed(t):
        e._ck(lib.ctmr_wait(h, t, rec.ctypes.data, new.ctypes.data, C.byref(st)))
    in_flight(submit_packed, wait_packed, 1)
    out["packed_async"] = rate(in_flight(submit_packed, wait_packed, args.rounds), args.rounds)
    e.close()
    out["pem_async_over_sync_text"] = round(out["pem_async"]["certs_per_s"] / out["sync_text"]["certs_per_s"], 2)
    out["pem_async_over_packed_async"] = round(out["pem_async"]["certs_per_s"] / out["packed_async"]["certs_per_s"], 3)
    text = json.dumps(out)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
