"""Per-issuer lists straight from an image (include/ctmr.h ctmr_known_image_lists*) at scale: one JSON line.

A table of ≥ --members live members (the synthetic corpus mapped on the GPU: scripts/bench_known_image.build_table) under
CTMR_KNOWN_ORDER_SORTED, then HIP-event times, after a warm-up, medians of --reps, one process, of
  engine   Engine.known_lists_device(now): the sorted lists from the table (index gather, sort, staging, text),
  image    Engine.known_image_lists_device(meta, d_members, now) on the same engine's sorted device export: the same
           bytes from the member records where they lie,
  table    the route a snapshot needed before: a fresh engine, known_import_device of that export, known_lists_device.
Model bytes per member: engine = the 8-byte index word per slot, the 48-byte cell, the 48-byte record staged and read
back twice, the text; image = the 48-byte record read twice and the text; table = the import's 48-byte read, 8-byte index
word and 64-byte cell write, then the engine leg over the fresh table.  The bar DESIGN.md §17 sets: image no slower than
engine in the same run (ratio_engine_over_image >= 1).  Kernel times: run under `rocprofv3 --kernel-trace --stats`
separately; --kernels-only runs just the image leg for that."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import synth, _native as N  # noqa: E402
from bench_known_image import build_table, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=120_000_000)
    ap.add_argument("--batch", type=int, default=25_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slots", type=int, default=1 << 28)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    cfg = synth.config(seed=20260921 + 7, n_issuers=256, zipf=1, dup_permille=20, ca_permille=10, expired_permille=10)
    issuers = synth.issuers(cfg)

    def engine():
        e = ctmr.Engine(device=0, table_slots=args.slots, pair_slots=1 << 21)
        e.set_stream(stream)
        e.add_issuers(issuers)
        e.set_filter(b"", False, synth.BASE_TIME)
        e.set_known_order(N.KNOWN_ORDER_SORTED)
        return e

    a = engine()
    t0 = time.perf_counter()
    entries = build_table(a, cfg, args.members, args.batch)
    build_s = time.perf_counter() - t0
    M = a.total_count()
    slots = a.table_info().slots
    now = 0
    meta, d_members = a.known_export_device()
    d_members = d_members.clone()                    # (the export returns a view of a larger buffer)
    keep = {}

    def image():
        keep["i"] = None
        keep["i"] = a.known_image_lists_device(meta, d_members, now)

    i_first, i_ms, _ = timed(image, args.reps)
    ids_i, toff_i, text_i = keep["i"]
    text_bytes = int(toff_i[-1])
    line = {"metric": "known_image_lists", "members": M, "issuers": len(ids_i), "text_bytes": text_bytes,
            "entries_mapped": entries, "build_s": round(build_s, 1), "table_slots": slots}

    def leg(ms_list, nbytes):
        ms = sorted(ms_list)[len(ms_list) // 2]
        return {"ms_median": round(ms, 3), "ms_all": [round(x, 3) for x in ms_list], "members_per_s": M / (ms * 1e-3),
                "model_GB": round(nbytes / 1e9, 3), "model_GB_per_s": nbytes / (ms * 1e-3) / 1e9}

    model_engine = 8 * slots + 48 * M + 48 * M + 2 * 48 * M + text_bytes
    model_image = 2 * 48 * M + text_bytes
    line["image"] = leg(i_ms, model_image)
    line["image_first_ms"] = round(i_first, 3)
    if not args.kernels_only:
        def device():
            keep["d"] = None
            keep["d"] = a.known_lists_device(now)

        d_first, d_ms, _ = timed(device, args.reps)
        ids_d, toff_d, text_d = keep["d"]
        assert ids_d == ids_i and list(toff_d) == list(toff_i) and bool(torch.equal(text_d, text_i)), "the legs disagree"
        line["engine"] = leg(d_ms, model_engine)
        line["engine_first_ms"] = round(d_first, 3)
        keep.clear()
        del text_d, text_i

        fresh = {}

        def new_engine():
            if "e" in fresh:
                fresh.pop("e").close()
            keep.clear()
            fresh["e"] = engine()

        def table():
            fresh["e"].known_import_device(meta, d_members)
            keep["t"] = fresh["e"].known_lists_device(now)

        t_first, t_ms, _ = timed(table, args.reps, before=new_engine)
        assert int(keep["t"][1][-1]) == text_bytes
        line["table"] = leg(t_ms, 48 * M + 8 * M + 64 * M + model_engine)
        line["table_first_ms"] = round(t_first, 3)
        fresh.pop("e").close()
        med = {k: line[k]["ms_median"] for k in ("engine", "image", "table")}
        line["ratio_engine_over_image"] = round(med["engine"] / med["image"], 3)
        line["ratio_table_over_image"] = round(med["table"] / med["image"], 3)
    print(json.dumps(line))
    a.close()


if __name__ == "__main__":
    main()
