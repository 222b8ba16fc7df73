"""A Redis protocol stream into an image (include/ctmr.h ctmr_known_resp_image*) at scale: one JSON line.

The table and sorted device export of scripts/bench_known_image_resp.py (≥ --members live members of the synthetic
corpus), its stream written by Engine.known_image_resp_device in the same run, then HIP-event times round the whole
call, host work included, after a warm-up, medians of --reps, one process, of
  parse    Engine.known_resp_image_device(stream): stream → meta and member records on the device,
  load     Engine.known_import_resp(stream) into a fresh engine per repetition: stream → records → the table,
  import   Engine.known_import_device(meta, d_members) of the same image into a fresh engine: the in-run yardstick,
and the wall time of
  python   known_image.from_resp on the stream of the first --python-members member records (whole sets): the rate of
           the pure-Python path this call replaces.
Model bytes: parse = the stream read three times and the records written; load = that plus import's; import = the
records read twice.  The parsed image is compared with the export it came from (byte for byte: the export is sorted).
No bar is set: nothing of this had been measured before."""
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
from bench_known_image import build_table, timed  # noqa: E402
from bench_known_image_resp import head_image  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=120_000_000)
    ap.add_argument("--batch", type=int, default=25_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slots", type=int, default=1 << 28)
    ap.add_argument("--per", type=int, default=512)
    ap.add_argument("--python-members", type=int, default=1_000_000)
    ap.add_argument("--kernels-only", action="store_true", help="the parse leg alone: for an A/B of two libraries, or a run under rocprofv3")
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    cfg = synth.config(seed=20260921 + 7, n_issuers=256, zipf=1, dup_permille=20, ca_permille=10, expired_permille=10)
    issuers = synth.issuers(cfg)
    a = ctmr.Engine(device=0, table_slots=args.slots, pair_slots=1 << 21)
    a.set_stream(stream)
    a.add_issuers(issuers)
    a.set_filter(b"", False, synth.BASE_TIME)
    a.set_known_order(N.KNOWN_ORDER_SORTED)
    t0 = time.perf_counter()
    entries = build_table(a, cfg, args.members, args.batch)
    build_s = time.perf_counter() - t0
    meta, d_members = a.known_export_device()
    d_members = d_members.clone()                    # (the export returns a view of a larger buffer)
    a.close()
    M = d_members.numel() // 48
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
    e.set_stream(stream)
    d_stream = e.known_image_resp_device(meta, d_members, args.per).clone()
    S = int(d_stream.numel())
    assert S < (1 << 32) - 64, "the stream of %d members does not fit one call" % M
    keep = {}

    def parse():
        keep["p"] = None
        keep["p"] = e.known_resp_image_device(d_stream)

    p_first, p_ms, _ = timed(parse, args.reps)
    got_meta, got = keep["p"]
    assert torch.equal(got, d_members), "the parsed records differ from the export's"
    meta_equal = got_meta == meta
    keep.clear()
    del got
    line = {"metric": "known_resp_image", "members": M, "sets": KI._HEADER.unpack_from(meta, 0)[5], "per": args.per,
            "stream_bytes": S, "meta_equal": meta_equal, "entries_mapped": entries, "build_s": round(build_s, 1)}

    def leg(ms_list, nbytes):
        ms = sorted(ms_list)[len(ms_list) // 2]
        return {"ms_median": round(ms, 3), "ms_all": [round(x, 3) for x in ms_list], "members_per_s": M / (ms * 1e-3),
                "model_GB": round(nbytes / 1e9, 3), "model_GB_per_s": nbytes / (ms * 1e-3) / 1e9}

    line["parse"] = leg(p_ms, 3 * S + 48 * M)
    line["parse_first_ms"] = round(p_first, 3)
    if args.kernels_only:
        print(json.dumps(line))
        e.close()
        return

    def fresh():
        if keep.get("e"):
            keep["e"].close()
        x = ctmr.Engine(device=0, table_slots=args.slots, pair_slots=1 << 21)
        x.set_stream(stream)
        x.add_issuers(issuers)
        x.set_filter(b"", False, synth.BASE_TIME)
        keep["e"] = x

    _, i_ms, st = timed(lambda: keep["e"].known_import_device(meta, d_members), args.reps, before=fresh)
    assert st["inserted"] == M, st
    line["import"] = leg(i_ms, 2 * 48 * M)
    _, l_ms, st = timed(lambda: keep["e"].known_import_resp(d_stream), args.reps, before=fresh)
    assert st["inserted"] == M, st
    line["load"] = leg(l_ms, 3 * S + 3 * 48 * M)
    keep["e"].close()
    keep.clear()
    small = head_image(meta, d_members, args.python_members)
    m_small = KI._HEADER.unpack_from(small, 0)[6]
    text = KI.image_resp(small, args.per)
    twin = KI.resp_image(text)                       # (names the issuers of these sets only, unlike `small`)
    assert e.known_resp_image(text) == twin
    t0 = time.perf_counter()
    back = KI.from_resp(text)
    py_s = time.perf_counter() - t0
    assert back == twin                              # (the export is sorted and free of repeats)
    line["python"] = {"members": m_small, "s": round(py_s, 3), "members_per_s": m_small / py_s}
    line["ratio_load_over_import"] = round(line["load"]["ms_median"] / line["import"]["ms_median"], 3)
    line["ratio_parse_over_python_rate"] = round(line["parse"]["members_per_s"] / line["python"]["members_per_s"], 1)
    print(json.dumps(line))
    e.close()


if __name__ == "__main__":
    main()
