"""get-entries bodies through the ingestion pipeline as text, and the price of a verdict per body (include/ctmr.h
ctmr_submit_entries_json / ctmr_wait_entries_json, ctmr_entries_json_each*): one JSON line, also written
to --out.  Nothing here is gated; nothing of it had been measured before.

pipeline  --bodies distinct bodies of 1 001 synthetic entries each (what a downloader holds, ct-fetch.go:417-424), every
          body in a buffer of ctmr_alloc_pinned.  Wall time, after one warm-up pass over all bodies on the same engine (so
          every certificate is known in the timed part of every leg, as in a re-read log), of --rounds passes:
            json_async   ctmr_submit_entries_json, --in-flight tickets outstanding, ctmr_wait_entries_json for the oldest,
            sync_text    one ctmr_entries_json + one ctmr_map_entries per body: the only route for text before,
            raw_async    ctmr_submit_entries / ctmr_wait_entries over the same entries decoded beforehand, the blobs in
                         pinned buffers too, --in-flight tickets outstanding.
          The text is 4/3 of the blob's bytes: where the host link is the bound, json_async sits near 3/4 of raw_async.
each      ctmr_entries_json_each_device against ctmr_entries_json_device on the input of scripts/bench_entries_json.py
          (--entries, tiled on the device), HIP-event times round the whole call, --reps each; all outputs compared.
          The strict leg runs once more behind the each leg (strict_again): what the order of the legs alone is worth.
verdict   the same text with the first key of one body in 64 spelled "Entries": ctmr_entries_json_each_device over it —
          the cost of a verdict (one more response-sized pass, a scan, an entry-sized gather) — and what it returned.
--legs chooses among them."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import get_entries as ge, synth, _native as N  # noqa: E402
from ct_mapreduce_amd.engine import RawEntries, RECORD_DTYPE  # noqa: E402
from bench_known_image import timed  # noqa: E402

PER_BODY = 1001
PER = 256
NONE = 2**64 - 1


def synth_raw(e, cfg, n):
    cap = n * 6144 + 64
    d_blob = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    d_bounds = torch.zeros(2 * n + 1, dtype=torch.int64, device="cuda:0")
    used = e.synth_entries_device(cfg, 0, n, d_bounds.data_ptr(), d_blob.data_ptr(), cap)
    return d_blob, d_bounds, used


def pinned(e, data):
    buf = e.pinned_array(len(data) + N.PAYLOAD_PAD)
    buf[:len(data)] = np.frombuffer(data, np.uint8)
    buf[len(data):] = 0
    return buf


def pipeline_legs(args):
    cfg = synth.config(seed=20261020, n_issuers=64, dup_permille=100)
    K, n1 = args.bodies, args.bodies * PER_BODY

    def engine():
        e = ctmr.Engine(device=0, table_slots=1 << 22, pair_slots=1 << 14)
        e.set_filter(b"", False, synth.BASE_TIME)
        return e

    e = engine()
    d_blob, d_bounds, used = synth_raw(e, cfg, n1)
    raw = RawEntries(d_blob[:used].cpu().numpy(), d_bounds.cpu().numpy().view(np.uint64))
    del d_blob, d_bounds
    pairs = [(raw.leaf_input(i), raw.extra_data(i)) for i in range(n1)]
    bodies = ge.write(pairs, PER_BODY)
    assert len(bodies) == K
    text_bytes, blob_bytes = sum(len(b) for b in bodies), used
    rec = np.zeros(PER_BODY, RECORD_DTYPE)
    new, ts = np.zeros(PER_BODY, np.uint64), np.zeros(PER_BODY, np.uint64)
    first, bad = np.zeros(2, np.uint64), np.zeros(1, np.uint64)
    info, st, ds = N.EntriesJsonInfo(), N.BatchStats(), N.DecodeStats()
    out = {"bodies": K, "entries_per_body": PER_BODY, "in_flight": args.in_flight, "rounds": args.rounds,
           "text_bytes_per_pass": text_bytes, "blob_bytes_per_pass": blob_bytes}

    def rate(s, passes):
        return {"s": round(s, 4), "entries_per_s": n1 * passes / s, "text_GB_per_s": text_bytes * passes / s / 1e9,
                "blob_GB_per_s": blob_bytes * passes / s / 1e9}

    def in_flight(submit, wait, passes):
        pending, t0 = [], time.perf_counter()
        for k in range(K * passes):
            if len(pending) == args.in_flight:
                wait(pending.pop(0))
            pending.append(submit(k % K))
        for t in pending:
            wait(t)
        return time.perf_counter() - t0

    lib, h = e._lib, e._h
    # ---- json_async
    texts = [pinned(e, b) for b in bodies]
    rbs = [np.asarray([0, len(b)], np.uint64) for b in bodies]

    def submit_json(k):
        t = C.c_uint64(0)
        e._ck(lib.ctmr_submit_entries_json(h, texts[k].ctypes.data, rbs[k].ctypes.data, 1, C.byref(t)))
        return t.value

    def wait_json(t):
        e._ck(lib.ctmr_wait_entries_json(h, t, PER_BODY, rec.ctypes.data, new.ctypes.data, ts.ctypes.data, first.ctypes.data, bad.ctypes.data,
                                         C.byref(info), C.byref(ds), C.byref(st)))
        assert info.entries == PER_BODY and bad[0] == NONE
    in_flight(submit_json, wait_json, 1)
    out["json_async"] = rate(in_flight(submit_json, wait_json, args.rounds), args.rounds)
    e.close()
    # ---- sync_text: pageable or pinned makes no difference to a call that stages and drains; the same pinned buffers
    e = engine()
    lib, h = e._lib, e._h
    texts = [pinned(e, b) for b in bodies]
    blob = np.zeros(max(len(b) for b in bodies) * 3 // 4 + N.PAYLOAD_PAD, np.uint8)
    bounds = np.zeros(2 * PER_BODY + 1, np.uint64)

    def sync_pass(passes):
        t0 = time.perf_counter()
        for k in range(K * passes):
            k %= K
            e._ck(lib.ctmr_entries_json(h, texts[k].ctypes.data, rbs[k].ctypes.data, 1, blob.ctypes.data, len(blob), bounds.ctypes.data, PER_BODY,
                                        None, C.byref(info)))
            e._ck(lib.ctmr_map_entries(h, blob.ctypes.data, bounds.ctypes.data, PER_BODY, rec.ctypes.data, new.ctypes.data, ts.ctypes.data,
                                       C.byref(ds), C.byref(st)))
        return time.perf_counter() - t0
    sync_pass(1)
    out["sync_text"] = rate(sync_pass(args.rounds), args.rounds)
    e.close()
    # ---- raw_async
    e = engine()
    lib, h = e._lib, e._h
    blobs, bnds = [], []
    for k in range(K):
        lo, hi = int(raw.bounds[2 * PER_BODY * k]), int(raw.bounds[2 * PER_BODY * (k + 1)])
        blobs.append(pinned(e, raw.blob[lo:hi].tobytes()))
        bnds.append(np.ascontiguousarray(raw.bounds[2 * PER_BODY * k:2 * PER_BODY * (k + 1) + 1] - np.uint64(lo)))

    def submit_raw(k):
        t = C.c_uint64(0)
        e._ck(lib.ctmr_submit_entries(h, blobs[k].ctypes.data, bnds[k].ctypes.data, PER_BODY, C.byref(t)))
        return t.value

    def wait_raw(t):
        e._ck(lib.ctmr_wait_entries(h, t, rec.ctypes.data, new.ctypes.data, ts.ctypes.data, C.byref(ds), C.byref(st)))
    in_flight(submit_raw, wait_raw, 1)
    out["raw_async"] = rate(in_flight(submit_raw, wait_raw, args.rounds), args.rounds)
    e.close()
    out["json_async_over_sync_text"] = round(out["json_async"]["entries_per_s"] / out["sync_text"]["entries_per_s"], 2)
    out["json_async_over_raw_async"] = round(out["json_async"]["entries_per_s"] / out["raw_async"]["entries_per_s"], 3)
    return out


def each_legs(args, legs):
    dev = "cuda:0"
    K, n1 = args.responses, args.responses * PER
    tiles = max(args.entries // n1, 1)
    n = n1 * tiles
    cfg = synth.config(seed=20261019, n_issuers=64, dup_permille=100)
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    d_blob1, d_bounds1, b1 = synth_raw(e, cfg, n1)
    raw = RawEntries(d_blob1[:b1].cpu().numpy(), d_bounds1.cpu().numpy().view(np.uint64))
    del d_blob1, d_bounds1
    text1, rb1 = ge.join(ge.write([(raw.leaf_input(i), raw.extra_data(i)) for i in range(n1)], PER))
    S1 = len(text1)
    d_text = torch.from_numpy(np.frombuffer(text1, np.uint8).copy()).to(dev).repeat(tiles)
    S, R, B = S1 * tiles, K * tiles, b1 * tiles
    rb = np.concatenate([(np.arange(tiles, dtype=np.uint64)[:, None] * np.uint64(S1) + rb1[None, :-1]).reshape(-1), np.asarray([S], np.uint64)])
    outs = {}

    def buffers():
        return (torch.zeros(B + N.PAYLOAD_PAD, dtype=torch.uint8, device=dev), torch.zeros(2 * n + 1, dtype=torch.int64, device=dev),
                np.zeros(R + 1, np.uint64), np.zeros(R, np.uint64), N.EntriesJsonInfo())

    def run(name, each):
        d_blob, d_bounds, first, bad, info = outs[name] = buffers()

        def call():
            if each:
                e._ck(e._lib.ctmr_entries_json_each_device(e._h, C.c_void_p(d_text.data_ptr()), rb.ctypes.data, R, C.c_void_p(d_blob.data_ptr()),
                                                           B + N.PAYLOAD_PAD, C.c_void_p(d_bounds.data_ptr()), n, first.ctypes.data, bad.ctypes.data,
                                                           C.byref(info)))
            else:
                e._ej_ck(e._lib.ctmr_entries_json_device(e._h, C.c_void_p(d_text.data_ptr()), rb.ctypes.data, R, C.c_void_p(d_blob.data_ptr()),
                                                         B + N.PAYLOAD_PAD, C.c_void_p(d_bounds.data_ptr()), n, first.ctypes.data, C.byref(info)), info)
        f, ms, _ = timed(call, args.reps)
        med = sorted(ms)[len(ms) // 2]
        return {"first_ms": round(f, 3), "ms_all": [round(x, 3) for x in ms], "ms_median": round(med, 3), "entries_per_s": info.entries / (med * 1e-3)}

    out = {"entries": n, "responses": R, "text_bytes": S, "blob_bytes": B}
    if "each" in legs:
        out["strict"] = run("strict", False)
        out["each"] = run("each", True)
        a, b = outs["strict"], outs["each"]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and (a[2] == b[2]).all() and bytes(a[4]) == bytes(b[4])
        assert (b[3] == NONE).all() and a[4].entries == n and a[4].blob_bytes == B
        out["each_over_strict"] = round(out["each"]["ms_median"] / out["strict"]["ms_median"], 4)
        outs.clear()
        out["strict_again"] = run("strict", False)   # the same leg behind the other: what the order alone is worth
        outs.clear()
    if "verdict" in legs:
        if "each" not in out:
            out["each"] = run("each", True)
            outs.clear()
        which = np.arange(0, R, 64)
        at = torch.from_numpy((rb[which] + np.uint64(2)).astype(np.int64)).to(dev)   # {"entries" → {"Entries"
        assert bool((d_text[at] == ord("e")).all())
        d_text[at] = ord("E")
        out["verdict"] = run("verdict", True)
        _, _, first, bad, info = outs["verdict"]
        assert (np.nonzero(bad != NONE)[0] == which).all() and info.entries == n - PER * len(which) and info.bad_response == 0
        assert (np.diff(first)[which] == 0).all()
        out["verdict"]["bad_bodies"] = len(which)
        out["verdict_over_each"] = round(out["verdict"]["ms_median"] / out["each"]["ms_median"], 4)
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="pipeline,each,verdict")
    ap.add_argument("--bodies", type=int, default=64)
    ap.add_argument("--in-flight", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=32)
    ap.add_argument("--entries", type=int, default=4_000_000)
    ap.add_argument("--responses", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_submit_entries_json.json"))
    args = ap.parse_args()
    legs = set(args.legs.split(","))
    line = {"metric": "submit_entries_json"}
    if "pipeline" in legs:
        line["pipeline"] = pipeline_legs(args)
    if legs & {"each", "verdict"}:
        line["each_device"] = each_legs(args, legs)
    text = json.dumps(line)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
