"""The order inside a known-certificate set (include/ctmr.h ctmr_known_sort* / ctmr_set_known_order) at
scale: one JSON line.

A table of ≥ --members live members (the synthetic corpus mapped on the GPU: scripts/bench_known_image.build_table), then
HIP-event times, median of --reps after a warm-up, in one process, of
  export_any / export_sorted   Engine.known_export_device under CTMR_KNOWN_ORDER_ANY (the yardstick) and _SORTED,
  lists_any / lists_sorted     Engine.known_lists_device under both orders,
  sort_random                  Engine.known_sort_device alone over the unsorted export (16- and 17-octet serials),
  sort_prefix                  the same sets, every serial 40 octets of which the first 32 are one constant: the worst legal
                               input for the round count short of repeats (five rounds),
  host_numpy                   known_image.sort's lexsort of the first --host-members records on one core, for context.
Rounds and radix passes are read from the library's CTMR_KNOWN_SORT_INFO line.  Traffic model per member and sort:
16 B read of the record and 16 B of key written once, (16 + 16 + 16) B per radix pass (histogram read, scatter read and
write; the digit counts add 2 B), 16 + 48 + 48 B for the gather and 96 B for the copy back.  Kernel times: run this
under `rocprofv3 --kernel-trace --stats` separately; --kernels-only runs just the two sort legs for that."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import synth, known_image as KI, _native as N  # noqa: E402
from bench_known_image import build_table, timed  # noqa: E402

INFO = re.compile(r"ctmr known sort: records=(\d+) runs=(\d+) rounds=(\d+) passes=(\d+)")


def sort_info(fn):
    """fn() with the library's info line caught → {"runs", "rounds", "passes"} of the last sort it made."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["CTMR_KNOWN_SORT_INFO"] = "1"
        try:
            fn()
        finally:
            del os.environ["CTMR_KNOWN_SORT_INFO"]
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        found = INFO.findall(tmp.read().decode(errors="replace"))
    if not found:
        return None
    _, runs, rounds, passes = (int(x) for x in found[-1])
    return {"runs": runs, "rounds": rounds, "passes": passes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=100_000_000)
    ap.add_argument("--batch", type=int, default=25_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-members", type=int, default=10_000_000)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    cfg = synth.config(seed=20260921 + 7, n_issuers=256, zipf=1, dup_permille=20, ca_permille=10, expired_permille=10)
    a = ctmr.Engine(device=0, table_slots=1 << 28, pair_slots=1 << 21)
    a.set_stream(stream)
    a.add_issuers(synth.issuers(cfg))
    a.set_filter(b"", False, synth.BASE_TIME)
    t0 = time.perf_counter()
    entries = build_table(a, cfg, args.members, args.batch)
    build_s = time.perf_counter() - t0
    M = a.total_count()
    line = {"metric": "known_sort", "members": M, "entries_mapped": entries, "build_s": round(build_s, 1)}

    def leg(ms_list, info=None, bytes_per_member=None):
        ms = sorted(ms_list)[len(ms_list) // 2]
        out = {"ms_median": round(ms, 3), "ms_all": [round(x, 3) for x in ms_list], "members_per_s": M / (ms * 1e-3)}
        if info:
            out.update(info)
            per = 32 + 50 * info["passes"] + 112 + 96
            out["model_bytes_per_member"] = per
            out["model_TB_per_s"] = per * M / (ms * 1e-3) / 1e12
        return out

    keep = {}

    def export():
        keep["x"] = None
        keep["x"] = a.known_export_device()

    def lists():
        keep["l"] = None
        keep["l"] = a.known_lists_device(0)

    if not args.kernels_only:
        for name, order in (("any", N.KNOWN_ORDER_ANY), ("sorted", N.KNOWN_ORDER_SORTED)):
            a.set_known_order(order)
            info = sort_info(export) if order else None
            _, ms, _ = timed(export, args.reps)
            line["export_" + name] = leg(ms, info)
            keep.clear()
            info = sort_info(lists) if order else None
            _, ms, _ = timed(lists, args.reps)
            line["lists_" + name] = leg(ms, info)
            keep.clear()
        line["export_sorted_over_any"] = round(line["export_sorted"]["ms_median"] / line["export_any"]["ms_median"], 3)
        line["lists_sorted_over_any"] = round(line["lists_sorted"]["ms_median"] / line["lists_any"]["ms_median"], 3)
    a.set_known_order(N.KNOWN_ORDER_ANY)
    meta, src = a.known_export_device()
    src = src.clone()
    line["sets"] = KI._HEADER.unpack_from(meta, 0)[5]
    work = torch.empty_like(src)

    def fresh():
        work.copy_(src)

    def sort():
        a.known_sort_device(meta, work)

    fresh()
    info = sort_info(sort)
    _, ms, _ = timed(sort, args.reps, before=fresh)
    line["sort_random"] = leg(ms, info)
    if not args.kernels_only and args.host_members:
        n = min(args.host_members, M)
        rec = np.frombuffer(src[:48 * n].cpu().numpy().tobytes(), KI.MEMBER_DTYPE)
        t0 = time.perf_counter()
        words = np.ascontiguousarray(rec["serial"]).view(">u8").astype(np.uint64)
        order = np.lexsort((rec["len"],) + tuple(words[:, k] for k in (4, 3, 2, 1, 0)))
        rec = rec[order]
        line["host_numpy"] = {"members": n, "s": round(time.perf_counter() - t0, 3)}
        del rec, words, order
    # the same sets, 40-octet serials with a common 32-octet prefix
    rows = src.view(-1, 48)
    rows[:, :8] = 0
    rows[:, 0] = 40
    rows[:, 8:40] = torch.arange(1, 33, dtype=torch.uint8, device=src.device)
    rows[:, 40:48] = torch.randint(0, 256, (rows.shape[0], 8), dtype=torch.uint8, device=src.device)
    fresh()
    info = sort_info(sort)
    _, ms, _ = timed(sort, args.reps, before=fresh)
    line["sort_prefix"] = leg(ms, info)
    line["prefix_over_random"] = round(line["sort_prefix"]["ms_median"] / line["sort_random"]["ms_median"], 3)
    print(json.dumps(line))
    a.close()


if __name__ == "__main__":
    main()
