"""The Redis protocol stream of an image (include/ctmr.h ctmr_known_image_resp*) at scale: one JSON line.

A table of ≥ --members live members (the synthetic corpus mapped on the GPU: scripts/bench_known_image.build_table) under
CTMR_KNOWN_ORDER_SORTED, its sorted device export, then HIP-event times, after a warm-up, medians of --reps, one process, of
  resp     Engine.known_image_resp_device(meta, d_members): the SADD + EXPIREAT stream from the member records where
           they lie,
  lists    Engine.known_image_lists_device(meta, d_members, 0) on the same image in the same run: the per-issuer lists,
and the wall time of
  python   known_image.to_resp on an image of the first --python-members member records (whole sets): the rate of the
           pure-Python stream this call replaces.
Model bytes per member: resp and lists = the 48-byte record read twice and the text.  The bar DESIGN.md §18 sets: resp no
slower than lists of the same run by more than 10 % (ratio_lists_over_resp >= 0.9).  Kernel times: run under
`rocprofv3 --kernel-trace --stats` separately; --kernels-only runs just the resp leg for that."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import known_image as KI, synth, _native as N  # noqa: E402
from bench_known_image import build_table, timed  # noqa: E402


def head_image(meta, d_members, want):
    """The image of the first whole sets of (meta, d_members) that hold at least `want` member records (all, if fewer),
    without its host section."""
    _, _, _, n_iss, _, n_sets, n_mem, _, _, _ = KI._HEADER.unpack_from(meta, 0)
    so = KI.HEADER_BYTES + 32 * n_iss
    sets = np.frombuffer(meta, np.dtype([("hour", "<i4"), ("ord", "<u4"), ("first", "<u8"), ("count", "<u8")]), n_sets, so)
    ends = sets["first"] + sets["count"]
    k = min(int(np.searchsorted(ends, want)) + 1, n_sets)
    n = int(ends[k - 1]) if k else 0
    head = KI._HEADER.pack(KI.MAGIC, KI.VERSION, KI.HEADER_BYTES, n_iss, 0, k, n, 0, 0, 0) + meta[KI.HEADER_BYTES:so] + \
        sets[:k].tobytes()
    head += b"\0" * (-len(head) % 64)
    return head + d_members[:n * 48].cpu().numpy().tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=120_000_000)
    ap.add_argument("--batch", type=int, default=25_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slots", type=int, default=1 << 28)
    ap.add_argument("--per", type=int, default=512)
    ap.add_argument("--python-members", type=int, default=1_000_000)
    ap.add_argument("--kernels-only", action="store_true")
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
    a.close()                                        # the table is not needed any more: neither leg reads it
    M = d_members.numel() // 48
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
    e.set_stream(stream)
    keep = {}

    def resp():
        keep["r"] = None
        keep["r"] = e.known_image_resp_device(meta, d_members, args.per)

    r_first, r_ms, _ = timed(resp, args.reps)
    resp_bytes = int(keep["r"].numel())
    line = {"metric": "known_image_resp", "members": M, "sets": KI._HEADER.unpack_from(meta, 0)[5], "per": args.per,
            "resp_bytes": resp_bytes, "entries_mapped": entries, "build_s": round(build_s, 1)}

    def leg(ms_list, nbytes):
        ms = sorted(ms_list)[len(ms_list) // 2]
        return {"ms_median": round(ms, 3), "ms_all": [round(x, 3) for x in ms_list], "members_per_s": M / (ms * 1e-3),
                "model_GB": round(nbytes / 1e9, 3), "model_GB_per_s": nbytes / (ms * 1e-3) / 1e9}

    line["resp"] = leg(r_ms, 2 * 48 * M + resp_bytes)
    line["resp_first_ms"] = round(r_first, 3)
    if not args.kernels_only:
        # the stream against the twin on the slice the Python leg takes, before the buffers go
        small = head_image(meta, d_members, args.python_members)
        m_small = KI._HEADER.unpack_from(small, 0)[6]
        want = KI.image_resp(small, args.per)
        assert keep["r"][:len(want)].cpu().numpy().tobytes() == want, "the stream differs from the twin"
        keep.clear()

        def lists():
            keep["l"] = None
            keep["l"] = e.known_image_lists_device(meta, d_members, 0)

        l_first, l_ms, _ = timed(lists, args.reps)
        lists_bytes = int(keep["l"][1][-1])
        keep.clear()
        line["lists"] = leg(l_ms, 2 * 48 * M + lists_bytes)
        line["lists_first_ms"] = round(l_first, 3)
        line["lists_bytes"] = lists_bytes
        t0 = time.perf_counter()
        out = io.BytesIO()
        KI.to_resp(small, out)
        py_s = time.perf_counter() - t0
        assert out.getvalue() == want or args.per != 512
        line["python"] = {"members": m_small, "s": round(py_s, 3), "members_per_s": m_small / py_s}
        line["ratio_lists_over_resp"] = round(line["lists"]["ms_median"] / line["resp"]["ms_median"], 3)
        line["ratio_resp_over_python_rate"] = round(line["resp"]["members_per_s"] / line["python"]["members_per_s"], 1)
    print(json.dumps(line))
    e.close()


if __name__ == "__main__":
    main()
