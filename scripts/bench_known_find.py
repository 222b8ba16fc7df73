"""Serials looked up in a known image whatever their expiration date (include/ctmr.h ctmr_known_image_find*, DESIGN.md
§25) at scale: one JSON line, also written to --out.

K is the image of scripts/bench_known_image_resp.py: a table of ≥ --members live members (the synthetic corpus mapped on
the GPU) exported sorted to the device.  P is --probes probes, half of them member records of K drawn at random (under
their own issuer), half random 16-octet serials K does not hold.  Then HIP-event times, after a warm-up, medians of --reps,
one process, of
  find     Engine.known_image_find_device(K, P, 0): K's records read once where they lie against a table of the probes,
  lists    Engine.known_image_lists_device(K, 0) of the same image in the same run: the per-issuer lists,
and the wall time of
  python   known_image.find on the image of K's first --python-members member records (whole sets) and the same P — the
           device's answer on that slice is held to it first.
Model bytes per member: find = the 48-byte record once (+ 16 B per probe written); lists = the record twice and the text.
The bar DESIGN.md §25 sets, inside one run: the find's median does not exceed the lists' median (ratio_lists_over_find
>= 1).  Kernel times: run under `rocprofv3 --kernel-trace --stats` separately; --kernels-only runs just the find leg."""
import argparse
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
from bench_known_image_resp import head_image  # noqa: E402

SET_DTYPE = np.dtype([("hour", "<i4"), ("ord", "<u4"), ("first", "<u8"), ("count", "<u8")])


def probe_image(meta, d_members, n_probes, seed):
    """→ (meta of P, its member records on the device, probes drawn from K): n_probes // 2 member records of K drawn at
    random, each under its set's issuer, and as many random 16-octet serials under random issuers; one set per issuer
    under hour 0, in key order, the records in drawn order."""
    _, _, _, n_iss, _, n_sets, n_mem, _, _, _ = KI._HEADER.unpack_from(meta, 0)
    so = KI.HEADER_BYTES + 32 * n_iss
    sets = np.frombuffer(meta, SET_DTYPE, n_sets, so)
    rng = np.random.default_rng(seed)
    n_hit = n_probes // 2
    idx = np.sort(rng.integers(0, n_mem, n_hit))
    ords = sets["ord"][np.searchsorted(sets["first"], idx, side="right") - 1]
    rec = d_members.view(-1, 48)[torch.from_numpy(idx).to(d_members.device)].cpu().numpy()
    miss = np.zeros((n_probes - n_hit, 48), np.uint8)
    miss[:, 0] = 16
    miss[:, 8:24] = rng.integers(0, 256, (len(miss), 16), dtype=np.uint8)
    rec = np.concatenate([rec, miss])
    ords = np.concatenate([ords, rng.integers(0, n_iss, len(miss)).astype(np.uint32)])
    ids = [KI.issuer_id(meta[KI.HEADER_BYTES + 32 * k:KI.HEADER_BYTES + 32 * (k + 1)]) for k in range(n_iss)]
    rank = np.empty(n_iss, np.int64)
    rank[np.asarray(sorted(range(n_iss), key=lambda k: ids[k]))] = np.arange(n_iss)
    order = np.argsort(rank[ords], kind="stable")
    rec, ords = rec[order], ords[order]
    used, counts = np.unique(rank[ords], return_counts=True)
    by_rank = {int(rank[k]): k for k in range(n_iss)}
    p_sets = np.zeros(len(used), SET_DTYPE)
    p_sets["ord"] = [by_rank[int(r)] for r in used]
    p_sets["count"] = counts
    p_sets["first"] = np.cumsum(counts) - counts
    head = KI._HEADER.pack(KI.MAGIC, KI.VERSION, KI.HEADER_BYTES, n_iss, 0, len(used), len(rec), 0, 0, 0) + \
        meta[KI.HEADER_BYTES:so] + p_sets.tobytes()
    head += b"\0" * (-len(head) % 64)
    return head, torch.from_numpy(rec.reshape(-1)).to(d_members.device), n_hit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=120_000_000)
    ap.add_argument("--probes", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=25_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slots", type=int, default=1 << 28)
    ap.add_argument("--python-members", type=int, default=1_000_000)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default="")
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
    p_meta, d_probes, drawn = probe_image(meta, d_members, args.probes, 11)
    P = d_probes.numel() // 48
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
    e.set_stream(stream)
    keep = {}

    def find():
        keep["f"] = None
        keep["f"] = e.known_image_find_device(meta, d_members, p_meta, d_probes, 0)

    f_first, f_ms, _ = timed(find, args.reps)
    info = keep["f"][2]
    assert info["members_read"] == M and info["probes"] == P and info["found"] >= drawn, info
    line = {"metric": "known_image_find", "members": M, "sets": KI._HEADER.unpack_from(meta, 0)[5], "probes": P,
            "found": info["found"], "entries_mapped": entries, "build_s": round(build_s, 1)}

    def leg(ms_list, nbytes):
        ms = sorted(ms_list)[len(ms_list) // 2]
        return {"ms_median": round(ms, 3), "ms_all": [round(x, 3) for x in ms_list], "members_per_s": M / (ms * 1e-3),
                "model_GB": round(nbytes / 1e9, 3), "model_GB_per_s": nbytes / (ms * 1e-3) / 1e9}

    line["find"] = leg(f_ms, 48 * M + (48 + 16) * P)
    line["find_first_ms"] = round(f_first, 3)
    if not args.kernels_only:
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
        line["ratio_lists_over_find"] = round(line["lists"]["ms_median"] / line["find"]["ms_median"], 3)
        line["bar_met"] = line["find"]["ms_median"] <= line["lists"]["ms_median"]
        # the twin on a slice of K, and the device held to it there
        small = head_image(meta, d_members, args.python_members)
        m_small = KI._HEADER.unpack_from(small, 0)[6]
        probes = p_meta + d_probes.cpu().numpy().tobytes()
        t0 = time.perf_counter()
        want, _ = KI.find(small, probes, 0)
        py_s = time.perf_counter() - t0
        got, _, _ = e.known_image_find(small, probes, 0)
        assert np.array_equal(got, want), "the device differs from the twin"
        line["python"] = {"members": m_small, "probes": P, "found": int((want["records"] > 0).sum()), "s": round(py_s, 3),
                          "members_per_s": m_small / py_s}
        line["ratio_find_over_python_rate"] = round(line["find"]["members_per_s"] / line["python"]["members_per_s"], 1)
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    e.close()


if __name__ == "__main__":
    main()
