"""A known image partitioned by a probe image (include/ctmr.h ctmr_known_image_split*) at scale: one JSON
line, also written to --out (default profiles/bench_known_split.json).

K and P are those of scripts/bench_known_find.py: a table of ≥ --members live members exported sorted to the device, and
--probes probes, half of them member records of K drawn at random, half random serials K does not hold.  Then HIP-event
times round the whole call, after a warm-up, medians of --reps, one process, of
  split      Engine.known_image_split_device(K, P, 0), both sides wanted,
  split_hit  the same with HIT only,
  find       Engine.known_image_find_device(K, P, 0),
  lists      Engine.known_image_lists_device(K, 0).
Before any of it the device's two results on the image of K's first --python-members member records (whole sets) are
held to known_image.split's, byte for byte.
Model bytes per member: the split reads each kept record twice, one table word and an eighth of a byte of
flags, and writes the record once; the lists read it twice and write the text.  The bar, inside one run: the split's
median with both sides wanted does not exceed the lists' median times the ratio of the two models' bytes, computed here
from the actual image.  Kernel times: run under `rocprofv3 --kernel-trace --stats` separately; --kernels-only runs just
the split leg."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import known_image as KI, synth, _native as N  # noqa: E402
from bench_known_find import probe_image  # noqa: E402
from bench_known_image import build_table, timed  # noqa: E402
from bench_known_image_resp import head_image  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=120_000_000)
    ap.add_argument("--probes", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=25_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slots", type=int, default=1 << 28)
    ap.add_argument("--python-members", type=int, default=1_000_000)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_known_split.json"))
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    cfg = synth.config(seed=20260921 + 7, n_issuers=256, zipf=1, dup_permille=20, ca_permille=10, expired_permille=10)
    a = ctmr.Engine(device=0, table_slots=args.slots, pair_slots=1 << 21)
    a.set_stream(stream)
    a.add_issuers(synth.issuers(cfg))
    a.set_filter(b"", False, synth.BASE_TIME)
    a.set_known_order(N.KNOWN_ORDER_SORTED)
    t0 = time.perf_counter()
    entries = build_table(a, cfg, args.members, args.batch)
    build_s = time.perf_counter() - t0
    meta, d_members = a.known_export_device()
    d_members = d_members.clone()                    # (the export returns a view of a larger buffer)
    a.close()                                        # the table is not needed any more: no leg reads it
    M = d_members.numel() // 48
    p_meta, d_probes, drawn = probe_image(meta, d_members, args.probes, 11)
    P = d_probes.numel() // 48
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
    e.set_stream(stream)
    line = {"metric": "known_image_split", "members": M, "sets": KI._HEADER.unpack_from(meta, 0)[5], "probes": P,
            "entries_mapped": entries, "build_s": round(build_s, 1)}
    if not args.kernels_only:
        # the twin on a slice of K, and the device held to it there
        small = head_image(meta, d_members, args.python_members)
        probes = p_meta + d_probes.cpu().numpy().tobytes()
        t0 = time.perf_counter()
        want = KI.split(small, probes, 0)
        py_s = time.perf_counter() - t0
        hit, miss, info = e.known_image_split(small, probes, 0)
        assert (hit, miss) == want, "the device differs from the twin"
        line["python"] = {"members": info["members_read"], "probes": P, "hit_members": info["hit"]["members"], "s": round(py_s, 3),
                          "members_per_s": info["members_read"] / py_s}
    keep = {}

    def split(want):
        def run():
            keep["s"] = None
            keep["s"] = e.known_image_split_device(meta, d_members, p_meta, d_probes, 0, want=want)
        return run

    def leg(ms_list, nbytes):
        ms = sorted(ms_list)[len(ms_list) // 2]
        return {"ms_median": round(ms, 3), "ms_all": [round(x, 3) for x in ms_list], "members_per_s": M / (ms * 1e-3),
                "model_GB": round(nbytes / 1e9, 3), "model_GB_per_s": nbytes / (ms * 1e-3) / 1e9}

    s_first, s_ms, _ = timed(split(("hit", "miss")), args.reps)
    info = keep["s"][2]
    assert info["members_read"] == M and 0 < info["hit"]["members"] <= drawn and info["hit"]["members"] + info["miss"]["members"] == M, info
    split_bytes = (2 * 48 + 8) * M + M // 8 + 48 * M + 48 * P
    line.update(hit_members=info["hit"]["members"], hit_sets=info["hit"]["sets"], miss_sets=info["miss"]["sets"])
    line["split"] = leg(s_ms, split_bytes)
    line["split_first_ms"] = round(s_first, 3)
    if not args.kernels_only:
        h_first, h_ms, _ = timed(split(("hit",)), args.reps)
        line["split_hit"] = leg(h_ms, (2 * 48 + 8) * M + M // 8 + 48 * info["hit"]["members"] + 48 * P)
        keep.clear()

        def find():
            keep["f"] = None
            keep["f"] = e.known_image_find_device(meta, d_members, p_meta, d_probes, 0)

        f_first, f_ms, _ = timed(find, args.reps)
        line["find"] = leg(f_ms, 48 * M + (48 + 16) * P)
        keep.clear()

        def lists():
            keep["l"] = None
            keep["l"] = e.known_image_lists_device(meta, d_members, 0)

        l_first, l_ms, _ = timed(lists, args.reps)
        lists_bytes = int(keep["l"][1][-1])
        keep.clear()
        line["lists"] = leg(l_ms, 2 * 48 * M + lists_bytes)
        line["lists_bytes"] = lists_bytes
        line["model_ratio_split_over_lists"] = round(split_bytes / (2 * 48 * M + lists_bytes), 4)
        line["ratio_split_over_lists"] = round(line["split"]["ms_median"] / line["lists"]["ms_median"], 3)
        line["ratio_split_over_find"] = round(line["split"]["ms_median"] / line["find"]["ms_median"], 3)
        line["bar_ms"] = round(line["lists"]["ms_median"] * split_bytes / (2 * 48 * M + lists_bytes), 3)
        line["bar_met"] = line["split"]["ms_median"] <= line["bar_ms"]
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    e.close()


if __name__ == "__main__":
    main()
