"""get-entries JSON bodies into raw entries (include/ctmr.h ctmr_entries_json*) at scale: one JSON line.

--responses distinct responses of 256 synthetic raw entries each (Engine.synth_entries_device), base64-encoded and
written as compact bodies on the host, uploaded once and tiled on the device with torch.repeat to --entries.  Text,
blob and the yardstick copy lie in HBM together; the line says how many bytes each took.  HIP-event times round the
whole call, host work included, after a warm-up, medians of --reps, one process, of
  decode   ctmr_entries_json_device: text → blob and bounds on the device,
  map      Engine.map_entries_device on the decoded blob: the in-run yardstick — what share of a raw batch the new step
           costs (one engine; after the warm-up every certificate is known, as in a re-read log),
  copy     a device-to-device copy of text_bytes: the floor for one pass over the text,
and the wall time of
  python   json.loads + base64.b64decode over --python-entries entries: a stand-in for the host step this call
           replaces.  The rate of Go's encoding/json + encoding/base64 is NOT measured here.
Model bytes of decode: the text read four times (quotes, mark count, mark write, decode) and the blob written once.
The decoded blob is compared on the device with the synthetic blob tiled the same way, the bounds with numpy's
arithmetic.  No bar is set: nothing of this had been measured before.
--decode-only stops behind the decode leg (reps + 1 calls): what `rocprofv3 --kernel-trace --stats` is run on, in a run of
its own, for the split of the call over its kernels (profiles/entries_json_kernel_stats_4m.csv)."""
import argparse
import base64
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import get_entries as ge, synth, _native as N  # noqa: E402
from ct_mapreduce_amd.engine import RawEntries  # noqa: E402
from bench_known_image import timed  # noqa: E402

PER = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=20_000_000)
    ap.add_argument("--responses", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--python-entries", type=int, default=32768)
    ap.add_argument("--decode-only", action="store_true", help="the decode leg alone: for a kernel trace of its own")
    args = ap.parse_args()
    dev = "cuda:0"
    stream = torch.cuda.current_stream().cuda_stream
    K = args.responses
    n1 = K * PER
    tiles = max(args.entries // n1, 1)
    n = n1 * tiles
    cfg = synth.config(seed=20261019, n_issuers=64, dup_permille=100)
    e = ctmr.Engine(device=0, table_slots=1 << 27, pair_slots=1 << 16)
    e.set_stream(stream)
    e.set_filter(b"", False, synth.BASE_TIME)
    cap = n1 * 6144 + 64
    d_blob1 = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_bounds1 = torch.zeros(2 * n1 + 1, dtype=torch.int64, device=dev)
    b1 = e.synth_entries_device(cfg, 0, n1, d_bounds1.data_ptr(), d_blob1.data_ptr(), cap)
    bounds1 = d_bounds1.cpu().numpy().view(np.uint64)
    raw = RawEntries(d_blob1[:b1].cpu().numpy(), bounds1)
    bodies = ge.write([(raw.leaf_input(i), raw.extra_data(i)) for i in range(n1)], PER)
    text1, rb1 = ge.join(bodies)
    S1 = len(text1)
    d_text = torch.from_numpy(np.frombuffer(text1, np.uint8).copy()).to(dev).repeat(tiles)
    S = S1 * tiles
    rb = (np.arange(tiles, dtype=np.uint64)[:, None] * np.uint64(S1) + rb1[None, :-1]).reshape(-1)
    rb = np.concatenate([rb, np.asarray([S], np.uint64)])
    R = K * tiles
    B = b1 * tiles
    d_blob = torch.empty(B + N.PAYLOAD_PAD, dtype=torch.uint8, device=dev)
    d_bounds = torch.empty(2 * n + 1, dtype=torch.int64, device=dev)
    first = np.empty(R + 1, np.uint64)
    info = N.EntriesJsonInfo()

    def decode():
        e._ej_ck(e._lib.ctmr_entries_json_device(e._h, C.c_void_p(d_text.data_ptr()), rb.ctypes.data, R, C.c_void_p(d_blob.data_ptr()),
                                                 B + N.PAYLOAD_PAD, C.c_void_p(d_bounds.data_ptr()), n, first.ctypes.data, C.byref(info)), info)

    d_first, d_ms, _ = timed(decode, args.reps)
    assert (info.entries, info.blob_bytes, info.text_bytes, info.responses) == (n, B, S, R)
    row = d_blob1[:b1]
    rows = d_blob[:B].view(tiles, b1)
    for lo in range(0, tiles, 64):
        assert bool((rows[lo:lo + 64] == row).all()), "the decoded blob differs from the synthetic blob in rows %d…" % lo
    want = (np.arange(tiles, dtype=np.uint64)[:, None] * np.uint64(b1) + bounds1[None, :-1]).reshape(-1)
    got = d_bounds.cpu().numpy().view(np.uint64)
    assert (got[:-1] == want).all() and int(got[-1]) == B
    assert (first == np.arange(R + 1, dtype=np.uint64) * np.uint64(PER)).all()
    del want, got

    def leg(ms_list, nbytes):
        ms = sorted(ms_list)[len(ms_list) // 2]
        return {"ms_median": round(ms, 3), "ms_all": [round(x, 3) for x in ms_list], "entries_per_s": n / (ms * 1e-3),
                "model_GB": round(nbytes / 1e9, 3), "model_GB_per_s": nbytes / (ms * 1e-3) / 1e9}

    line = {"metric": "entries_json", "entries": n, "responses": R, "distinct_responses": K, "text_bytes": S, "blob_bytes": B,
            "copy_bytes": S, "hbm_bytes_text_blob_copy": 2 * S + B}
    line["decode"] = leg(d_ms, 4 * S + B)
    line["decode_first_ms"] = round(d_first, 3)
    line["decode_text_GB_per_s"] = S / (line["decode"]["ms_median"] * 1e-3) / 1e9
    if args.decode_only:
        line["decode_calls"] = args.reps + 1
        print(json.dumps(line))
        e.close()
        return
    d_rec = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    _, m_ms, _ = timed(lambda: e.map_entries_device(d_blob.data_ptr(), d_bounds.data_ptr(), n, d_rec.data_ptr()), args.reps)
    line["map"] = leg(m_ms, B)
    del d_rec
    d_copy = torch.empty(S, dtype=torch.uint8, device=dev)
    _, c_ms, _ = timed(lambda: d_copy.copy_(d_text), args.reps)
    line["copy"] = leg(c_ms, 2 * S)
    del d_copy
    m = min(args.python_entries, n1) // PER
    some = bodies[:max(m, 1)]
    t0 = time.perf_counter()
    got = []
    for b in some:
        for x in json.loads(b)["entries"]:
            got.append(base64.b64decode(x["leaf_input"]))
            got.append(base64.b64decode(x["extra_data"]))
    py_s = time.perf_counter() - t0
    assert b"".join(got) == raw.blob[:int(bounds1[2 * PER * len(some)])].tobytes()
    line["python"] = {"entries": PER * len(some), "s": round(py_s, 4), "entries_per_s": PER * len(some) / py_s,
                      "text_GB_per_s": sum(len(b) for b in some) / py_s / 1e9}
    line["ratio_decode_over_map"] = round(line["decode"]["ms_median"] / line["map"]["ms_median"], 3)
    line["ratio_decode_over_copy"] = round(line["decode"]["ms_median"] / line["copy"]["ms_median"], 3)
    line["ratio_decode_over_python_rate"] = round(line["decode"]["entries_per_s"] / line["python"]["entries_per_s"], 1)
    print(json.dumps(line))
    e.close()


if __name__ == "__main__":
    main()
