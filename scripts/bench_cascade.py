"""The filter cascade of a revoked / not-revoked image pair (include/ctmr.h ctmr_cascade_*) at scale: one
JSON line, also written to --out (default profiles/bench_cascade.json).

K and P are those of scripts/bench_known_split.py: a table of ≥ --members live members exported sorted to the device, and
--probes probes, half of them member records of K drawn at random.  Then HIP-event times round the whole call, after a
warm-up, medians of --reps, one process, of
  split       Engine.known_image_split_device(K, P, 0), both sides wanted,
  build       Engine.cascade_build_device(HIT, MISS, 0, cascade.crlite_params(|HIT|, |MISS|)),
  query_hit   Engine.cascade_query_device(cascade, HIT)   — every answer must be 1,
  query_miss  Engine.cascade_query_device(cascade, MISS)  — every answer must be 0.
The build is reported as a ratio to the split of the same run and to the rate of the CPU twin cascade.build on a sample
of --python-members records (a tenth of them from HIT, the rest from MISS; whole sets), where the device's cascade is held
to the twin's byte for byte.  No threshold: the numbers are recorded, not gated.  --kernels-only leaves the twin out."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import cascade as CA, known_image as KI, synth, _native as N  # noqa: E402
from bench_known_find import probe_image  # noqa: E402
from bench_known_image import build_table, timed  # noqa: E402
from bench_known_image_resp import head_image  # noqa: E402


def twin_sample(e, args, line, hit_meta, d_hit, miss_meta, d_miss):
    """The twin on a sample, and the device held to it there."""
    small_r, small_s = head_image(hit_meta, d_hit, args.python_members // 10), head_image(miss_meta, d_miss, args.python_members * 9 // 10)
    sample = CA.crlite_params(KI._HEADER.unpack_from(small_r, 0)[6], KI._HEADER.unpack_from(small_s, 0)[6], b"bench")
    t0 = time.perf_counter()
    want = CA.build(small_r, small_s, 0, sample)
    py_s = time.perf_counter() - t0
    got, sinfo = e.cascade_build(small_r, small_s, 0, sample)
    assert got == want, "the device differs from the twin"
    n_sample = sinfo["r_records"] + sinfo["s_records"]
    line["python"] = {"records": n_sample, "layers": sinfo["layers"], "s": round(py_s, 3), "records_per_s": n_sample / py_s}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=120_000_000)
    ap.add_argument("--probes", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=25_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slots", type=int, default=1 << 28)
    ap.add_argument("--python-members", type=int, default=100_000)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_cascade.json"))
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    cfg = synth.config(seed=20260921 + 7, n_issuers=256, zipf=1, dup_permille=20, ca_permille=10, expired_permille=10)
    a = ctmr.Engine(device=0, table_slots=args.slots, pair_slots=1 << 21)
    a.set_stream(stream)
    a.add_issuers(synth.issuers(cfg))
    a.set_filter(b"", False, synth.BASE_TIME)
    a.set_known_order(N.KNOWN_ORDER_SORTED)
    entries = build_table(a, cfg, args.members, args.batch)
    meta, d_members = a.known_export_device()
    d_members = d_members.clone()                    # (the export returns a view of a larger buffer)
    a.close()
    M = d_members.numel() // 48
    p_meta, d_probes, _ = probe_image(meta, d_members, args.probes, 11)
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
    e.set_stream(stream)
    keep = {}

    def split():
        keep["s"] = None
        keep["s"] = e.known_image_split_device(meta, d_members, p_meta, d_probes, 0)

    def leg(ms_list, records):
        ms = sorted(ms_list)[len(ms_list) // 2]
        return {"ms_median": round(ms, 3), "ms_all": [round(x, 3) for x in ms_list], "records_per_s": records / (ms * 1e-3)}

    _, s_ms, _ = timed(split, args.reps)
    (hit_meta, d_hit), (miss_meta, d_miss), info = keep["s"]
    d_hit, d_miss = d_hit.clone(), d_miss.clone()
    keep.clear()
    n_hit, n_miss = info["hit"]["members"], info["miss"]["members"]
    params = CA.crlite_params(n_hit, n_miss, b"bench")
    line = {"metric": "cascade_build", "members": M, "probes": d_probes.numel() // 48, "entries_mapped": entries, "revoked": n_hit,
            "not_revoked": n_miss, "params": [params.k_first, params.bpk_first_q8, params.k_rest, params.bpk_rest_q8, params.max_layers],
            "split": leg(s_ms, M)}
    if not args.kernels_only:
        twin_sample(e, args, line, hit_meta, d_hit, miss_meta, d_miss)

    def build():
        keep["c"] = None
        keep["c"] = e.cascade_build_device(hit_meta, d_hit, miss_meta, d_miss, 0, params)

    b_first, b_ms, _ = timed(build, args.reps)
    d_cascade, binfo = keep["c"]
    d_cascade = d_cascade.clone()
    keep.clear()
    assert binfo["r_records"] == n_hit and binfo["s_records"] == n_miss, binfo
    line["build"] = leg(b_ms, n_hit + n_miss)
    line["build_first_ms"] = round(b_first, 3)
    line.update(layers=binfo["layers"], cascade_bytes=binfo["bytes"], syncs=binfo["syncs"], held=[l[4] for l in binfo["layer"]])

    def query(m, d):
        def run():
            keep["q"] = None
            keep["q"] = e.cascade_query_device(d_cascade, m, d)[0]
        return run

    _, qh_ms, _ = timed(query(hit_meta, d_hit), args.reps)
    assert bool((keep["q"] == 1).all()), "a revoked record answers 0"
    _, qm_ms, _ = timed(query(miss_meta, d_miss), args.reps)
    assert bool((keep["q"] == 0).all()), "a record that is not revoked answers 1"
    keep.clear()
    line["query_hit"] = leg(qh_ms, n_hit)
    line["query_miss"] = leg(qm_ms, n_miss)
    line["ratio_build_over_split"] = round(line["build"]["ms_median"] / line["split"]["ms_median"], 3)
    if not args.kernels_only:
        line["ratio_build_rate_over_python"] = round(line["build"]["records_per_s"] / line["python"]["records_per_s"], 1)
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    e.close()


if __name__ == "__main__":
    main()
