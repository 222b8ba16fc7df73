#!/usr/bin/env python3
"""bench_known_image.py — the known-certificate image at scale: one JSON line.

Builds a table of --members members by mapping synthetic batches, then times with HIP events (one warm-up, then --reps)
  * known_export_device                                  (export: 8 B per index slot + 64 B per cell + 48 B per member)
  * known_import_device into a reset engine, world = 1   (import: 48 B read + 64 B per cell written + a 64-byte index
  * known_import_device, world = 4, rank = 0              line per taken member)
and, for comparison, the point path: set_insert of --point members.  The import targets are reset (reset_known) between
reps: the warm-up grows their tables, the timed reps insert into a table of the final size.

    python scripts/bench_known_image.py [--members 100000000] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import synth, _native as N  # noqa: E402


def build_table(eng, cfg, want, batch):
    dev = torch.device("cuda:%d" % eng.device)
    first = 0
    while eng.total_count() < want:
        n = batch
        d_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        total = eng.synth_device(cfg, first, n, d_off.data_ptr(), 0, 0, 0, 0)
        d_pay = torch.empty(total + N.PAYLOAD_PAD + 16, dtype=torch.uint8, device=dev)
        d_iss = torch.empty(n, dtype=torch.int32, device=dev)
        d_et = torch.empty(n, dtype=torch.uint8, device=dev)
        eng.synth_device(cfg, first, n, d_off.data_ptr(), d_pay.data_ptr(), d_pay.numel(), d_iss.data_ptr(), d_et.data_ptr())
        eng.map_batch_device(d_pay.data_ptr(), d_off.data_ptr(), d_iss.data_ptr(), d_et.data_ptr(), n, 0, 0)
        del d_off, d_pay, d_iss, d_et
        first += n
    return first


def timed(fn, reps, before=None):
    """(first call ms, [ms of the reps]) by HIP events on the current stream (the engines run on it)."""
    out = []
    for r in range(reps + 1):
        if before:
            before()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out[0], out[1:], res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=100_000_000)
    ap.add_argument("--batch", type=int, default=25_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--point", type=int, default=20_000)
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    cfg = synth.config(seed=20260921 + 7, n_issuers=256, zipf=1, dup_permille=20, ca_permille=10, expired_permille=10)
    issuers = synth.issuers(cfg)

    def engine(slots):
        e = ctmr.Engine(device=0, table_slots=slots, pair_slots=1 << 21)    # ≈ 0.55 M (issuer, hour) sets: load ≈ 1/4
        e.set_stream(stream)
        e.add_issuers(issuers)
        e.set_filter(b"", False, synth.BASE_TIME)
        return e

    a = engine(1 << 28)
    t0 = time.perf_counter()
    entries = build_table(a, cfg, args.members, args.batch)
    build_s = time.perf_counter() - t0
    M = a.total_count()
    ti = a.table_info()
    keep = {}

    def export():
        keep["img"] = None
        keep["img"] = a.known_export_device()

    ex_first, ex, _ = timed(export, args.reps)
    meta, d = keep["img"]
    assert d.numel() // 48 == M
    n_sets = int.from_bytes(meta[24:32], "little")
    b, c = engine(1 << 20), engine(1 << 20)
    st1 = {}
    im_first, im, st1 = timed(lambda: b.known_import_device(meta, d), args.reps, before=b.reset_known)
    assert st1["inserted"] == st1["taken"] == M == b.total_count()
    i4_first, i4, st4 = timed(lambda: c.known_import_device(meta, d, world=4, rank=0), args.reps, before=c.reset_known)
    assert 0.2 * M < st4["taken"] < 0.3 * M
    # the point path: SetInsert one member at a time (what redis_load does)
    p = engine(1 << 16)
    ident = p.issuer_id(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(args.point):
        p.set_insert("serials::2026-06-01-00::%s" % ident, k.to_bytes(8, "big"))
    point_s = time.perf_counter() - t0

    def leg(ms_list, members, nbytes):
        ms = sorted(ms_list)[len(ms_list) // 2]
        return {"ms_median": round(ms, 3), "ms_all": [round(x, 3) for x in ms_list], "members": members,
                "members_per_s": members / (ms * 1e-3), "image_members_per_s": M / (ms * 1e-3),
                "GB": round(nbytes / 1e9, 3), "GB_per_s": nbytes / (ms * 1e-3) / 1e9}

    line = {
        "metric": "known_image", "members": M, "sets": n_sets, "entries_mapped": entries, "build_s": round(build_s, 1),
        "table": {"slots": ti.slots, "arena_used": ti.arena_used},
        "export": leg(ex, M, 8 * ti.slots + 64 * M + 48 * M),
        "export_first_ms": round(ex_first, 3),
        "import_w1": leg(im, st1["taken"], 48 * M + 64 * st1["taken"] + 64 * st1["taken"]),
        "import_w1_first_ms_with_growth": round(im_first, 3),
        "import_w4_r0": leg(i4, st4["taken"], 48 * M + 64 * st4["taken"] + 64 * st4["taken"]),
        "import_w4_r0_first_ms_with_growth": round(i4_first, 3),
        "point_set_insert": {"members": args.point, "s": round(point_s, 3), "members_per_s": args.point / point_s},
    }
    print(json.dumps(line))
    for e in (a, b, c, p):
        e.close()


if __name__ == "__main__":
    main()
