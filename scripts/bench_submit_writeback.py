"""What the write-back for pipeline tickets costs and buys (include/ctmr.h ctmr_set_pipeline_writeback / ctmr_ticket_writeback;
DESIGN.md §24): one JSON line, also written to --out.  Nothing here is gated.

The set-up of scripts/bench_submit_entries_json.py's pipeline legs, for the packed form: submits of 1 001 synthetic
certificates each from buffers of ctmr_alloc_pinned, --in-flight tickets outstanding.  Unlike there, every certificate of the
timed pass is NEW to the engine — write-back has nothing to do for a known one: each repetition of a leg runs on a fresh
engine, first over --warm batches of other certificates (as many as are timed, so that every slot's buffers have the size they
keep; the issuers' Names in the memo), then timed over --batches batches.  --reps repetitions a leg; the rate is the median,
the spread is reported.
  off        flags 0 on a default engine: ctmr_submit_batch / ctmr_wait as before (--legs off runs on any older library)
  off_meta   flags 0 on an engine created with collect_meta (the map's memo pre-check runs): the base of meta and both
  pem        CTMR_WB_PEM: ctmr_ticket_writeback, then ctmr_wait
  meta       CTMR_WB_META
  both       CTMR_WB_PEM | CTMR_WB_META
  sync       the route before: ctmr_map_batch + ctmr_pem_new + ctmr_meta_new per submit, on a collect_meta engine"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

if "ct_mapreduce_amd" not in sys.modules:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import synth, _native as N  # noqa: E402
from ct_mapreduce_amd.engine import RECORD_DTYPE  # noqa: E402

PER = 1001
LEGS = {"off": (False, 0), "off_meta": (True, 0), "pem": (False, 1), "meta": (True, 2), "both": (True, 3), "sync": (True, None)}


def corpus(cfg, first, count):
    out = []
    for k in range(count):
        b = synth.host_batch(cfg, first + k * PER, PER)
        out.append((b.payload, b.offsets.astype(np.uint64), b.issuer_idx.astype(np.uint32), b.entry_type.astype(np.uint8)))
    return out


def run_leg(name, cfg, issuers, warm, timed, in_flight):
    """one repetition on a fresh engine → seconds of the timed pass, and what came back in it"""
    meta, flags = LEGS[name]
    e = ctmr.Engine(device=0, table_slots=1 << 22, pair_slots=1 << 14, collect_meta=meta)
    e.add_issuers(issuers)
    e.set_filter(b"", True, synth.BASE_TIME)
    lib, h = e._lib, e._h
    if flags:
        e._ck(lib.ctmr_set_pipeline_writeback(h, flags))

    def pin(batches):
        out = []
        for pay, off, iss, et in batches:
            buf = e.pinned_array(len(pay))
            buf[:] = pay
            out.append((buf, off, iss, et))
        return out
    warm, timed = pin(warm), pin(timed)
    rec = np.zeros(PER, RECORD_DTYPE)
    new = np.zeros(PER, np.uint64)
    st = N.BatchStats()
    pem = np.zeros(PER * 4096, np.uint8)
    poff = np.zeros(PER + 1, np.uint64)
    items = (N.MetaItem * (6 * PER))()
    ibytes = np.zeros(6 * PER * 4096, np.uint8)
    got = {"new": 0, "pem_bytes": 0, "items": 0, "item_bytes": 0}

    def submit(b):
        t = C.c_uint64(0)
        e._ck(lib.ctmr_submit_batch(h, b[0].ctypes.data, b[1].ctypes.data, b[2].ctypes.data, b[3].ctypes.data, PER, C.byref(t)))
        return t.value

    def wait(t):
        if flags:
            info = N.WritebackInfo()
            e._ck(lib.ctmr_ticket_writeback(h, t, pem.ctypes.data, pem.size, poff.ctypes.data, items, len(items), ibytes.ctypes.data, ibytes.size,
                                            C.byref(info)))
            got["pem_bytes"] += info.pem_bytes
            got["items"] += info.n_items
            got["item_bytes"] += info.item_bytes
        e._ck(lib.ctmr_wait(h, t, rec.ctypes.data, new.ctypes.data, C.byref(st)))
        got["new"] += st.n_new

    def async_pass(batches):
        pending, t0 = [], time.perf_counter()
        for b in batches:
            if len(pending) == in_flight:
                wait(pending.pop(0))
            pending.append(submit(b))
        for t in pending:
            wait(t)
        return time.perf_counter() - t0

    def sync_pass(batches):
        need, count, ni, bneed = C.c_size_t(0), C.c_uint64(0), C.c_uint64(0), C.c_size_t(0)
        t0 = time.perf_counter()
        for b in batches:
            e._ck(lib.ctmr_map_batch(h, b[0].ctypes.data, b[1].ctypes.data, b[2].ctypes.data, b[3].ctypes.data, PER, rec.ctypes.data, new.ctypes.data,
                                     C.byref(st)))
            e._ck(lib.ctmr_pem_new(h, pem.ctypes.data, pem.size, poff.ctypes.data, C.byref(need), C.byref(count)))
            e._ck(lib.ctmr_meta_new(h, items, len(items), ibytes.ctypes.data, ibytes.size, C.byref(ni), C.byref(bneed)))
            got["new"] += st.n_new
            got["pem_bytes"] += need.value
            got["items"] += ni.value
            got["item_bytes"] += bneed.value
        return time.perf_counter() - t0
    run = sync_pass if flags is None else async_pass
    run(warm)
    for k in got:
        got[k] = 0
    s = run(timed)
    e.close()
    return s, got


def leg(name, args, cfg, issuers, warm, timed):
    secs, got = [], None
    for _ in range(args.reps):
        s, got = run_leg(name, cfg, issuers, warm, timed, args.in_flight)
        secs.append(s)
    n = len(timed) * PER
    rates = sorted(n / s for s in secs)
    return dict(got, s_all=[round(s, 4) for s in secs], certs_per_s=rates[len(rates) // 2], certs_per_s_min=rates[0], certs_per_s_max=rates[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="off,off_meta,pem,meta,both,sync")
    ap.add_argument("--batches", type=int, default=256)
    ap.add_argument("--warm", type=int, default=256)
    ap.add_argument("--in-flight", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_submit_writeback.json"))
    args = ap.parse_args()
    cfg = synth.config(seed=20261021, n_issuers=64, dup_permille=100)
    issuers = synth.issuers(cfg)
    warm = corpus(cfg, 0, args.warm)
    timed = corpus(cfg, args.warm * PER, args.batches)
    line = {"metric": "submit_writeback", "certs_per_submit": PER, "batches": args.batches, "warm_batches": args.warm, "in_flight": args.in_flight,
            "reps": args.reps, "payload_bytes": int(sum(int(b[1][-1]) for b in timed)), "legs": {}}
    for name in args.legs.split(","):
        line["legs"][name] = leg(name, args, cfg, issuers, warm, timed)
    L = line["legs"]

    def ratio(a, b):
        return round(L[a]["certs_per_s"] / L[b]["certs_per_s"], 3) if a in L and b in L else None
    line["both_over_off"] = ratio("both", "off")
    line["both_over_off_meta"] = ratio("both", "off_meta")
    line["both_over_sync"] = ratio("both", "sync")
    line["pem_over_off"] = ratio("pem", "off")
    line["meta_over_off_meta"] = ratio("meta", "off_meta")
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
