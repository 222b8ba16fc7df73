"""PEM certificate files into a packed batch (include/ctmr.h ctmr_pem_decode*) at scale: one JSON line,
written to --out (default profiles/bench_pem_decode.json) and printed.

--certs synthetic certificates (Engine.synth_device) are encoded to PEM by pem_encode_device in the same run: that text,
one file, is what the regular leg decodes.  HIP-event times round the whole call, host work included, after a warm-up,
medians of --reps, one process, of
  decode   ctmr_pem_decode_device: text → payload and offsets on the device,
  encode   ctmr_pem_encode_device of the same certificates: the way there, the in-run yardstick,
  copy     a device-to-device copy of text_bytes: the floor for one pass over the text.
The irregular leg decodes a text in which every second LF has become CR LF, so that every block of two lines and more
mixes its eols and goes through the squeezed copy: the first --unit blocks changed so with torch and tiled to about the
same size.  Model bytes of decode: the text read three times (mark count, mark write, decode) and the payload written
once; an irregular block adds a read of the text, a write and a read of its characters.
The decoded payload and offsets are compared on the device with what was encoded.  No bar is set: nothing of this had
been measured before.
--decode-only stops behind the regular decode leg (reps + 1 calls): what `rocprofv3 --kernel-trace --stats` is run on, in a
run of its own, for the split of the call over its kernels."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--certs", type=int, default=4_000_000)
    ap.add_argument("--unit", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--decode-only", action="store_true", help="the regular decode leg alone: for a kernel trace of its own")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_pem_decode.json"))
    args = ap.parse_args()
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
    _, enc_ms, _ = timed(lambda: e.pem_encode_device(d_pay.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(), n, d_text.data_ptr(), S,
                                                     d_po.data_ptr()), args.reps)

    def decode_leg(d_t, total, want_n, want_bytes):
        fb = np.asarray([0, total], np.uint64)
        d_out = torch.empty(want_bytes + N.PAYLOAD_PAD, dtype=torch.uint8, device=dev)
        d_oo = torch.empty(want_n + 1, dtype=torch.int64, device=dev)
        first = np.empty(2, np.uint64)
        info = N.PemDecodeInfo()

        def call():
            rc = e._lib.ctmr_pem_decode_device(e._h, C.c_void_p(d_t.data_ptr()), fb.ctypes.data, 1, C.c_void_p(d_out.data_ptr()),
                                               want_bytes + N.PAYLOAD_PAD, C.c_void_p(d_oo.data_ptr()), want_n, first.ctypes.data, C.byref(info))
            assert rc == 0, (rc, e._lib.ctmr_last_error(e._h))
        first_ms, ms, _ = timed(call, args.reps)
        assert (info.certificates, info.payload_bytes, info.text_bytes) == (want_n, want_bytes, total)
        return d_out, d_oo, info, first_ms, ms

    def leg(ms_list, nbytes, certs):
        ms = sorted(ms_list)[len(ms_list) // 2]
        return {"ms_median": round(ms, 3), "ms_all": [round(x, 3) for x in ms_list], "certs_per_s": certs / (ms * 1e-3),
                "model_GB": round(nbytes / 1e9, 3), "model_GB_per_s": nbytes / (ms * 1e-3) / 1e9}

    d_out, d_oo, info, first_ms, d_ms = decode_leg(d_text, S, n, B)
    assert bool((d_out[:B] == d_pay[:B]).all()) and bool((d_oo == d_off).all()) and info.irregular == 0
    line = {"metric": "pem_decode", "certs": n, "text_bytes": S, "payload_bytes": B, "regular": int(info.regular)}
    line["decode"] = leg(d_ms, 3 * S + B, n)
    line["decode_first_ms"] = round(first_ms, 3)
    line["decode_text_GB_per_s"] = S / (line["decode"]["ms_median"] * 1e-3) / 1e9
    if args.decode_only:
        line["decode_calls"] = args.reps + 1
        print(json.dumps(line))
        e.close()
        return
    del d_out, d_oo
    line["encode"] = leg(enc_ms, S + B, n)
    d_copy = torch.empty(S, dtype=torch.uint8, device=dev)
    _, c_ms, _ = timed(lambda: d_copy.copy_(d_text), args.reps)
    line["copy"] = leg(c_ms, 2 * S, n)
    del d_copy
    # ---- the irregular leg: every second LF of the first `unit` blocks becomes CR LF; tiled
    n1 = min(args.unit, n)
    off1 = d_off[:n1 + 1].cpu().numpy()
    S1, B1 = int(d_po[n1]), int(off1[n1])
    t = d_text[:S1]
    lf = t == 10
    ins = lf & ((torch.cumsum(lf, 0) & 1) == 0)
    pos = torch.arange(S1, device=dev) + torch.cumsum(ins, 0)
    unit = torch.empty(S1 + int(ins.sum()), dtype=torch.uint8, device=dev)
    unit[pos] = t
    unit[pos[ins] - 1] = 13
    tiles = max(n // n1, 1)
    d_irr = unit.repeat(tiles)
    torch.cuda.synchronize()
    del d_text, t, lf, ins, pos
    Si, ni, Bi = unit.numel() * tiles, n1 * tiles, B1 * tiles
    d_out, d_oo, info, first_ms, i_ms = decode_leg(d_irr, Si, ni, Bi)
    rows = d_out[:Bi].view(tiles, B1)
    for lo in range(0, tiles, 64):
        assert bool((rows[lo:lo + 64] == d_pay[:B1]).all()), "the decoded payload differs in rows %d…" % lo
    chars = (Bi + 2) // 3 * 4
    line["irregular"] = dict(leg(i_ms, 4 * Si + Bi + 2 * chars, ni), certs=ni, text_bytes=Si, payload_bytes=Bi, regular=int(info.regular),
                             irregular=int(info.irregular), first_ms=round(first_ms, 3))
    line["ratio_decode_over_copy"] = round(line["decode"]["ms_median"] / line["copy"]["ms_median"], 3)
    line["ratio_decode_over_encode"] = round(line["decode"]["ms_median"] / line["encode"]["ms_median"], 3)
    line["ratio_irregular_over_regular_per_cert"] = round((line["irregular"]["ms_median"] / ni) / (line["decode"]["ms_median"] / n), 3)
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    e.close()


if __name__ == "__main__":
    main()
