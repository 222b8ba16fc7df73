#!/usr/bin/env python3
"""bench_known_query.py — bulk SetContains / SetRemove over an image at scale: one JSON line.

Builds the table of bench_known_image.py (--members members, 256 issuers, same seed and table sizes), exports it to
device memory and times with HIP events, one warm-up round then --reps rounds, the legs taking turns inside a round:
  (a) import   known_import_device of the image into a reset engine (the yardstick: code this feature does not touch)
  (b) query    known_query_device of the image against the full table: every member present
  (c) absent   the same records with every set's hour shifted to one the table does not hold: every member absent
  (d) remove   known_remove_device of the image from the freshly imported copy of leg (a)
then leg (b) again for each records-per-lane instantiation of k_known_query (CTMR_KNOWN_PROBE_RPL = 1, 2, 4, 8), and,
for the record, set_contains in a loop over --point members.  Bytes per leg: 48 B per record + 32 B per index sector +
64 B per cell touched + the flag byte.  The bar: median(b) <= median(a) and median(d) <= median(a), same run.

    python scripts/bench_known_query.py [--members 100000000] [--reps 5]
"""
import argparse
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import synth  # noqa: E402
from scripts.bench_known_image import build_table  # noqa: E402

HOUR_SHIFT = 24 * 366 * 40          # forty years on: hours no synthetic certificate expires in


def shifted(meta):
    """The meta part with every set's hour moved by HOUR_SHIFT (the order of the keys is kept)."""
    m = bytearray(meta)
    n_iss, n_sets = struct.unpack_from("<I", m, 16)[0], struct.unpack_from("<Q", m, 24)[0]
    for s in range(n_sets):
        at = 64 + 32 * n_iss + 24 * s
        struct.pack_into("<i", m, at, struct.unpack_from("<i", m, at)[0] + HOUR_SHIFT)
    return bytes(m)


def event_ms(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), res


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
        e = ctmr.Engine(device=0, table_slots=slots, pair_slots=1 << 21)
        e.set_stream(stream)
        e.add_issuers(issuers)
        e.set_filter(b"", False, synth.BASE_TIME)
        return e

    a = engine(1 << 28)
    t0 = time.perf_counter()
    build_table(a, cfg, args.members, args.batch)
    build_s = time.perf_counter() - t0
    M = a.total_count()
    ti = a.table_info()
    meta, d = a.known_export_device()
    assert d.numel() // 48 == M
    meta_absent = shifted(meta)
    b = engine(1 << 20)
    os.environ.pop("CTMR_KNOWN_PROBE_RPL", None)
    ms = {"import": [], "query": [], "absent": [], "remove": []}
    for rnd in range(args.reps + 1):
        b.reset_known()
        t, st = event_ms(lambda: b.known_import_device(meta, d))
        assert st["inserted"] == st["taken"] == M
        ms["import"].append(t)
        t, (fl, _, st) = event_ms(lambda: a.known_query_device(meta, d))
        assert st["hits"] == st["taken"] == M and int(fl.min()) == 1
        ms["query"].append(t)
        t, (fl, _, st) = event_ms(lambda: a.known_query_device(meta_absent, d))
        assert st["hits"] == 0 and st["taken"] == M and int(fl.max()) == 0
        ms["absent"].append(t)
        del fl
        t, st = event_ms(lambda: b.known_remove_device(meta, d))
        assert st["hits"] == st["taken"] == M and b.total_count() == 0
        ms["remove"].append(t)
    sweep = {}
    for rpl in (1, 2, 4, 8):
        os.environ["CTMR_KNOWN_PROBE_RPL"] = str(rpl)
        got = [event_ms(lambda: a.known_query_device(meta, d))[0] for _ in range(args.reps + 1)][1:]
        sweep[str(rpl)] = round(sorted(got)[len(got) // 2], 3)
    os.environ.pop("CTMR_KNOWN_PROBE_RPL", None)
    # the point path: SetContains one member at a time
    keys = a.keys(b"serials::*")[:64]
    members = [(k, m) for k in keys for m in a.set_list(k)][:args.point]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    found = sum(a.set_contains(k, m) for k, m in members)
    point_s = time.perf_counter() - t0
    assert found == len(members)

    def leg(name, nbytes):
        reps = ms[name][1:]
        med = sorted(reps)[len(reps) // 2]
        return {"ms_median": round(med, 3), "ms_all": [round(x, 3) for x in reps], "first_ms": round(ms[name][0], 3),
                "members_per_s": M / (med * 1e-3), "GB": round(nbytes / 1e9, 3), "GB_per_s": nbytes / (med * 1e-3) / 1e9}

    line = {
        "metric": "known_query", "members": M, "build_s": round(build_s, 1),
        "table": {"slots": ti.slots, "arena_used": ti.arena_used},
        "import_w1": leg("import", (48 + 32 + 64) * M),
        "query_present": leg("query", (48 + 32 + 64 + 1) * M),
        "query_absent": leg("absent", (48 + 32 + 1) * M),
        "remove": leg("remove", (48 + 32 + 64) * M),
        "query_present_ms_by_records_per_lane": sweep,
        "point_set_contains": {"members": len(members), "s": round(point_s, 3), "members_per_s": len(members) / point_s},
    }
    line["query_within_import"] = line["query_present"]["ms_median"] <= line["import_w1"]["ms_median"]
    line["remove_within_import"] = line["remove"]["ms_median"] <= line["import_w1"]["ms_median"]
    print(json.dumps(line))
    a.close()
    b.close()


if __name__ == "__main__":
    main()
