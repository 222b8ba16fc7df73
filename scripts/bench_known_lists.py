"""Per-issuer known-serial lists (include/ctmr.h ctmr_known_lists*) at scale: one JSON line.

A table of ≥ --members live members (the synthetic corpus mapped on the GPU: scripts/bench_known_image.build_table), then
HIP-event times, after a warm-up, of
  device    Engine.known_lists_device(now): the lists in device memory (staging by k_known_export, k_lists_count, scan,
            k_lists_write),
  host      Engine.known_lists_raw(now): the same into host memory, end to end (the device-to-host copy of the text),
  writer    HostWriter(root).store_known_lists of those lists into --root (a tmpfs directory; one file per issuer).
Needed bytes per member: the 8-byte index word and the 48-byte cell of the gather, the 48-byte record staged and read
back twice (count and write passes), and the 2L+1 bytes of text written.  Kernel times: run this under
`rocprofv3 --kernel-trace --stats` separately; --kernels-only runs just the device leg for that."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import synth, host_writeback as HW  # noqa: E402
from bench_known_image import build_table, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=100_000_000)
    ap.add_argument("--batch", type=int, default=25_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--root", default="/dev/shm")
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    cfg = synth.config(seed=20260921 + 7, n_issuers=256, zipf=1, dup_permille=20, ca_permille=10, expired_permille=10)
    issuers = synth.issuers(cfg)
    a = ctmr.Engine(device=0, table_slots=1 << 28, pair_slots=1 << 21)
    a.set_stream(stream)
    a.add_issuers(issuers)
    a.set_filter(b"", False, synth.BASE_TIME)
    t0 = time.perf_counter()
    entries = build_table(a, cfg, args.members, args.batch)
    build_s = time.perf_counter() - t0
    M = a.total_count()
    ti = a.table_info()
    now = 0
    keep = {}

    def device():
        keep["d"] = None
        keep["d"] = a.known_lists_device(now)

    d_first, d_ms, _ = timed(device, args.reps)
    ids, toff, d_text = keep["d"]
    text_bytes = int(toff[-1])
    keep.clear()
    line = {"metric": "known_lists", "members": M, "issuers": len(ids), "text_bytes": text_bytes,
            "entries_mapped": entries, "build_s": round(build_s, 1), "table_slots": ti.slots}

    def leg(ms_list, nbytes):
        ms = sorted(ms_list)[len(ms_list) // 2]
        return {"ms_median": round(ms, 3), "ms_all": [round(x, 3) for x in ms_list],
                "members_per_s": M / (ms * 1e-3), "text_GB_per_s": text_bytes / (ms * 1e-3) / 1e9,
                "needed_GB": round(nbytes / 1e9, 3), "needed_GB_per_s": nbytes / (ms * 1e-3) / 1e9}

    needed = 8 * ti.slots + 48 * M + 48 * M + 2 * 48 * M + text_bytes
    line["device"] = leg(d_ms, needed)
    line["device_first_ms"] = round(d_first, 3)
    line["needed_bytes_per_member"] = round(needed / M, 2)
    if not args.kernels_only:
        h_first, h_ms, res = timed(lambda: a.known_lists_raw(now), args.reps)
        assert res[4].text_bytes == text_bytes
        line["host"] = leg(h_ms, needed + text_bytes)
        text, ids_b, toff_h, ioff, info = res
        root = tempfile.mkdtemp(prefix="ctmr_lists_", dir=args.root)
        try:
            w = HW.HostWriter(root, [])
            t0 = time.perf_counter()
            w.store_known_lists(ids_b, ioff, text, toff_h)
            wr_s = time.perf_counter() - t0
            w.close()
            files = len(os.listdir(root))
        finally:
            shutil.rmtree(root, ignore_errors=True)
        line["writer"] = {"s": round(wr_s, 3), "files": files, "GB_per_s": text_bytes / wr_s / 1e9, "root": args.root}
        del text, res
    print(json.dumps(line))
    a.close()


if __name__ == "__main__":
    main()
