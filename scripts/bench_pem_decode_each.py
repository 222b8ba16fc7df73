"""The price of a verdict per PEM file (include/ctmr.h ctmr_pem_decode_each*) at the shape of
scripts/bench_pem_decode.py: one JSON line, written to --out (default profiles/bench_pem_decode_each.json) and printed.
Nothing here is gated; nothing of it had been measured before.

--certs synthetic certificates are encoded to PEM by pem_encode_device in the same run.  HIP-event times round the whole
call, host work included, after a warm-up, medians of --reps, one process, of
  strict_one_file   ctmr_pem_decode_device over the text as ONE file: the leg of scripts/bench_pem_decode.py, for the
                    comparison of this call across commits on one box (its spread is ms_all),
  strict            ctmr_pem_decode_device over the same text as one file per certificate, the reference's layout,
  each              ctmr_pem_decode_each_device over the same files: no file is bad; every output compared with strict's,
  strict_again      the strict leg once more behind the each leg: what the order of the legs alone is worth,
  verdict           the same files with a byte of no class written into one file in 64: ctmr_pem_decode_each_device over
                    them — the cost of the verdicts (the table fetched, one more file-sized pass, a scan, a
                    certificate-sized gather) — and what it returned."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import synth, _native as N  # noqa: E402
from bench_known_image import timed  # noqa: E402

NONE = 2**64 - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--certs", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="strict_one_file,each,verdict")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_pem_decode_each.json"))
    args = ap.parse_args()
    legs = set(args.legs.split(","))
    dev = "cuda:0"
    n = args.certs
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    cfg = synth.config(seed=20261019, n_issuers=64, dup_permille=100)
    d_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    B = e.synth_device(cfg, 0, n, d_off.data_ptr(), 0, 0, 0, 0)
    d_pay = torch.zeros(B + N.PAYLOAD_PAD + 16, dtype=torch.uint8, device=dev)
    d_iss = torch.empty(n, dtype=torch.int32, device=dev)
    d_et = torch.empty(n, dtype=torch.uint8, device=dev)
    e.synth_device(cfg, 0, n, d_off.data_ptr(), d_pay.data_ptr(), d_pay.numel(), d_iss.data_ptr(), d_et.data_ptr())
    del d_iss, d_et
    d_idx = torch.arange(n, dtype=torch.int64, device=dev)
    d_po = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    S = e.pem_encode_device(d_pay.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(), n, 0, 0, d_po.data_ptr())
    d_text = torch.empty(S, dtype=torch.uint8, device=dev)
    e.pem_encode_device(d_pay.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(), n, d_text.data_ptr(), S, d_po.data_ptr())
    torch.cuda.synchronize()
    per_cert = d_po.cpu().numpy().view(np.uint64).copy()
    off = d_off.cpu().numpy().view(np.uint64)
    del d_idx
    outs = {}

    def run(name, fb, each, want_n, want_bytes):
        F = len(fb) - 1
        d_out = torch.zeros(B + N.PAYLOAD_PAD, dtype=torch.uint8, device=dev)
        d_oo = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        first, bad, info = np.zeros(F + 1, np.uint64), np.zeros(F, np.uint64), N.PemDecodeInfo()
        outs[name] = (d_out, d_oo, first, bad, info)

        def call():
            if each:
                rc = e._lib.ctmr_pem_decode_each_device(e._h, C.c_void_p(d_text.data_ptr()), fb.ctypes.data, F, C.c_void_p(d_out.data_ptr()),
                                                        B + N.PAYLOAD_PAD, C.c_void_p(d_oo.data_ptr()), n, first.ctypes.data, bad.ctypes.data,
                                                        C.byref(info))
            else:
                rc = e._lib.ctmr_pem_decode_device(e._h, C.c_void_p(d_text.data_ptr()), fb.ctypes.data, F, C.c_void_p(d_out.data_ptr()),
                                                   B + N.PAYLOAD_PAD, C.c_void_p(d_oo.data_ptr()), n, first.ctypes.data, C.byref(info))
            assert rc == 0, (rc, e._lib.ctmr_last_error(e._h))
        f, ms, _ = timed(call, args.reps)
        assert (info.certificates, info.payload_bytes, info.text_bytes) == (want_n, want_bytes, S)
        med = sorted(ms)[len(ms) // 2]
        return {"files": F, "first_ms": round(f, 3), "ms_all": [round(x, 3) for x in ms], "ms_median": round(med, 3),
                "ms_spread": round(max(ms) - min(ms), 3), "certs_per_s": want_n / (med * 1e-3)}

    line = {"metric": "pem_decode_each", "certs": n, "text_bytes": S, "payload_bytes": B, "reps": args.reps}
    if "strict_one_file" in legs:
        line["strict_one_file"] = run("one", np.asarray([0, S], np.uint64), False, n, B)
        a = outs.pop("one")
        assert bool((a[0][:B] == d_pay[:B]).all()) and bool((a[1] == d_off).all())
        del a
    if "each" in legs:
        line["strict"] = run("strict", per_cert, False, n, B)
        line["each"] = run("each", per_cert, True, n, B)
        a, b = outs["strict"], outs["each"]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and (a[2] == b[2]).all() and bytes(a[4]) == bytes(b[4])
        assert (b[3] == NONE).all() and bool((a[0][:B] == d_pay[:B]).all()) and bool((a[1] == d_off).all())
        line["each_over_strict"] = round(line["each"]["ms_median"] / line["strict"]["ms_median"], 4)
        outs.clear()
        del a, b
        line["strict_again"] = run("strict", per_cert, False, n, B)
        outs.clear()
    if "verdict" in legs:
        if "each" not in line:
            line["each"] = run("each", per_cert, True, n, B)
            outs.clear()
        which = np.arange(0, n, 64)
        at = torch.from_numpy((per_cert[which] + np.uint64(30)).astype(np.int64)).to(dev)   # a character of the first body line
        d_text[at] = ord("#")
        torch.cuda.synchronize()
        lens = np.diff(off)
        line["verdict"] = run("verdict", per_cert, True, n - len(which), B - int(lens[which].sum()))
        d_out, d_oo, first, bad, info = outs["verdict"]
        assert (np.nonzero(bad != NONE)[0] == which).all() and info.bad_file == 0 and (bad[which] == per_cert[which] + np.uint64(30)).all()
        assert (np.diff(first)[which] == 0).all() and int(first[-1]) == n - len(which)
        keep = np.ones(n, bool)
        keep[which] = False
        want_off = np.concatenate([[0], np.cumsum(lens[keep])]).astype(np.int64)
        assert bool((d_oo[:len(want_off)] == torch.from_numpy(want_off).to(dev)).all())
        line["verdict"]["bad_files"] = len(which)
        line["verdict_over_each"] = round(line["verdict"]["ms_median"] / line["each"]["ms_median"], 4)
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    e.close()


if __name__ == "__main__":
    main()
