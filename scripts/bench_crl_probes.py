"""DER CRLs → a probe image (include/ctmr.h ctmr_crl_probes*) at scale: one JSON line, also written to --out.

The blob is --crls synthetic CRLs of --entries entries in all: serials of 16 and 17 octets in turn (first octet 01..7f,
the others random; fake_candidates says how many fake entries chance made of them), UTCTime, one in eight with a reason-code
extension; one of 64 issuer digests per CRL.  Then HIP-event times, after a warm-up, medians of --reps, one process, of
  crl      Engine.crl_probes_device(blob, offsets, digests),
  copy     a device-to-device copy of the blob's bytes,
  resp     Engine.known_resp_image_device on the SADD stream of the image `crl` wrote: the same number of member records
           through the call's nearest relative (kernels/resp_parse.h), in the same run,
  revoked  Engine.known_revoked(blob, now = 0) on an engine that holds ≥ --members members of the synthetic corpus,
and the wall time of
  python   crl.probes_image on the first CRLs that hold --python-entries entries — the device's image of that slice is
           held to it first.
No speed is asserted anywhere; ratio_crl_over_resp_per_record > 1 means the call costs more per record than its relative.
Kernel times: run under `rocprofv3 --kernel-trace --stats` separately; --kernels-only runs just the crl leg.

--each runs four other legs instead, all through the C ABI with buffers allocated once, so that nothing but
the call is between the events:
  strict         ctmr_crl_probes_device of this build,
  strict_parent  the same call of the library --parent-lib names, built from the parent commit (left out without it),
  each           ctmr_crl_probes_each_device on the same blob: no bad CRL,
  each_bad       … on the blob with one CRL in 64 cut short by one byte: the head refuses those,
with the ratios strict / strict_parent, each / strict and each_bad / each, and whether strict's median lies inside the
spread of strict_parent's calls.  --kernels-only with --each leaves strict_parent out: in a kernel trace the three legs
are told apart by their k_crl_head dispatches, strict's first."""
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
from ct_mapreduce_amd import crl as CRL, synth  # noqa: E402
from bench_known_image import build_table, timed  # noqa: E402


def tlv(tag, content):
    n = len(content)
    head = bytes([n]) if n < 0x80 else bytes([0x80 | (n.bit_length() + 7) // 8]) + n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([tag]) + head + content


UTC = tlv(0x17, b"250101000000Z")
REASON = tlv(0x30, tlv(0x30, tlv(0x06, b"\x55\x1d\x15") + tlv(0x04, tlv(0x0a, b"\x01"))))
SIGALG = bytes.fromhex("300d06092a864886f70d01010b0500")


def one_crl(n):
    """→ (a CRL of n entries with zero serials as a numpy array, the offsets of the serial octets in it as a flat index
    array, the serial lengths)"""
    value, at, lens = [], [], []
    pos = 0
    for k in range(n):
        L = 16 + k % 2
        e = tlv(0x30, tlv(0x02, b"\0" * L) + UTC + (REASON if k % 8 == 0 else b""))
        at.append(pos + 4)
        lens.append(L)
        value.append(e)
        pos += len(e)
    value = b"".join(value)
    pre = tlv(0x02, b"\x01") + SIGALG + tlv(0x30, tlv(0x31, tlv(0x30, tlv(0x06, b"\x55\x04\x03") + tlv(0x0c, b"Bench CA")))) + UTC + UTC
    tbs = tlv(0x30, pre + tlv(0x30, value))
    c = tlv(0x30, tbs + SIGALG + tlv(0x03, b"\x00" + b"\x5a" * 64))
    lo = c.index(value[:40])
    idx = np.concatenate([np.arange(lo + a, lo + a + L) for a, L in zip(at, lens)])
    first = np.asarray([lo + a for a in at])
    return np.frombuffer(c, np.uint8), idx, first


def make_blob(n_crls, n_entries, seed):
    per = max(n_entries // n_crls, 1)
    c, idx, first = one_crl(per)
    rng = np.random.default_rng(seed)
    blob = np.tile(c, n_crls).reshape(n_crls, len(c))
    blob[:, idx] = rng.integers(0, 256, (n_crls, len(idx)), dtype=np.uint8)
    blob[:, first] = rng.integers(1, 0x80, (n_crls, len(first)), dtype=np.uint8)
    offsets = np.arange(n_crls + 1, dtype=np.uint64) * np.uint64(len(c))
    digests = [bytes(np.random.default_rng(900 + k % 64).integers(0, 256, 32, dtype=np.uint8).tolist()) for k in range(n_crls)]
    return blob.reshape(-1), offsets, digests, per


def each_legs(args, blob, offsets, digests, n_entries, stream):
    """The four legs of --each → the JSON line's dict."""
    import ctypes as C
    from ct_mapreduce_amd import _native as N
    n = len(offsets) - 1
    cut = np.arange(63, n, 64)                                                   # the CRLs that lose their last byte
    short = np.delete(blob, (offsets[cut + 1] - np.uint64(1)).astype(np.int64))
    short_offsets = offsets - np.searchsorted(cut, np.arange(n + 1), side="left").astype(np.uint64)
    assert short_offsets[-1] == short.size
    d_blob, d_short = torch.from_numpy(blob).to("cuda:0"), torch.from_numpy(short).to("cuda:0")
    d_out = torch.empty(48 * n_entries, dtype=torch.uint8, device="cuda:0")
    meta = np.empty(64 + 56 * n + (1 << 12), np.uint8)
    dig = b"".join(digests)
    verdicts = (N.CrlVerdict * n)()
    info, cinfo = N.KnownImageInfo(), N.CrlInfo()

    def engine(lib):
        cfg = N.Config(struct_size=C.sizeof(N.Config), device=0, table_slots=1 << 12, pair_slots=1 << 10)
        h = C.c_void_p()
        assert lib.ctmr_create(C.byref(cfg), C.byref(h)) == 0
        assert lib.ctmr_set_stream(h, C.c_void_p(stream)) == 0
        return h

    def caller(lib, h, name, d, offs):
        fn = getattr(lib, name)
        fn.restype = C.c_int
        args = [h, C.c_void_p(d.data_ptr()), C.c_uint64(d.numel()), C.c_void_p(offs.ctypes.data), C.c_uint32(n), dig, C.c_void_p(meta.ctypes.data),
                C.c_size_t(meta.nbytes), C.c_void_p(d_out.data_ptr()), C.c_uint64(n_entries), C.byref(info), C.byref(cinfo)]
        args += [C.byref(verdicts)] if "each" in name else []

        def call():
            rc = fn(*args)
            assert rc == 0, (name, rc)
            return info.members, cinfo.bad_crl
        return call

    def leg(ms_list):
        return {"ms_median": round(sorted(ms_list)[len(ms_list) // 2], 3), "ms_all": [round(x, 3) for x in ms_list]}

    line = {"metric": "crl_probes_each", "crls": n, "entries": n_entries, "blob_bytes": int(blob.size), "bad_crls": int(len(cut))}
    here = N.lib()
    h = engine(here)
    legs = [("strict", here, h, "ctmr_crl_probes_device", d_blob, offsets)]
    parent = hp = None
    if args.parent_lib and not args.kernels_only:
        parent = C.CDLL(args.parent_lib)
        hp = engine(parent)
        legs.append(("strict_parent", parent, hp, "ctmr_crl_probes_device", d_blob, offsets))
    legs += [("each", here, h, "ctmr_crl_probes_each_device", d_blob, offsets),
             ("each_bad", here, h, "ctmr_crl_probes_each_device", d_short, short_offsets)]
    for nm, lib, hh, fn, d, offs in legs:
        _, ms, (members, bad) = timed(caller(lib, hh, fn, d, offs), args.reps)
        want = n_entries - (len(cut) * (n_entries // n) if nm == "each_bad" else 0)
        assert members == want and bad == (63 if nm == "each_bad" else CRL.NONE), (nm, members, want, bad)
        line[nm] = leg(ms)
    line["ratio_each_over_strict"] = round(line["each"]["ms_median"] / line["strict"]["ms_median"], 4)
    line["ratio_each_bad_over_each"] = round(line["each_bad"]["ms_median"] / line["each"]["ms_median"], 4)
    if parent is not None:
        p = line["strict_parent"]["ms_all"]
        line["ratio_strict_over_parent"] = round(line["strict"]["ms_median"] / line["strict_parent"]["ms_median"], 4)
        line["strict_inside_parent_spread"] = bool(min(p) <= line["strict"]["ms_median"] <= max(p))
        parent.ctmr_destroy(hp)
    here.ctmr_destroy(h)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crls", type=int, default=2048)
    ap.add_argument("--entries", type=int, default=20_000_000)
    ap.add_argument("--members", type=int, default=100_000_000)
    ap.add_argument("--batch", type=int, default=25_000_000)
    ap.add_argument("--slots", type=int, default=1 << 28)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--python-entries", type=int, default=1_000_000)
    ap.add_argument("--kernels-only", action="store_true", help="the crl leg alone: for a run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--each", action="store_true", help="the legs of the each form (DESIGN.md §27) instead")
    ap.add_argument("--parent-lib", default="", help="--each: a libctmr.so built from the parent commit, for the strict_parent leg")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    blob, offsets, digests, per = make_blob(args.crls, args.entries, 26)
    n_entries = per * args.crls
    if args.each:
        text = json.dumps(each_legs(args, blob, offsets, digests, n_entries, stream))
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    d_blob = torch.from_numpy(blob).to("cuda:0")
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
    e.set_stream(stream)
    keep = {}

    def crl():
        keep["c"] = None
        keep["c"] = e.crl_probes_device(d_blob, offsets, digests)

    c_first, c_ms, _ = timed(crl, args.reps)
    p_meta, d_rec, info = keep["c"]
    assert info["entries"] == info["records"] == n_entries == d_rec.numel() // 48, info
    line = {"metric": "crl_probes", "crls": args.crls, "entries": n_entries, "blob_bytes": int(blob.size), "candidates": info["candidates"],
            "fake_candidates": info["candidates"] - n_entries - 2 * args.crls}

    def leg(ms_list, n, nbytes):
        ms = sorted(ms_list)[len(ms_list) // 2]
        return {"ms_median": round(ms, 3), "ms_all": [round(x, 3) for x in ms_list], "records_per_s": n / (ms * 1e-3),
                "ns_per_record": ms * 1e6 / n, "bytes_in_GB_per_s": nbytes / (ms * 1e-3) / 1e9}

    line["crl"] = leg(c_ms, n_entries, blob.size)
    line["crl_first_ms"] = round(c_first, 3)
    if args.kernels_only:
        print(json.dumps(line))
        e.close()
        return
    d_copy = torch.empty_like(d_blob)
    _, k_ms, _ = timed(lambda: d_copy.copy_(d_blob), args.reps)
    line["copy"] = leg(k_ms, n_entries, blob.size)
    del d_copy
    # the nearest relative on the same records
    d_rec = d_rec.clone()
    d_text = e.known_image_resp_device(p_meta, d_rec, 512).clone()

    def resp():
        keep["r"] = None
        keep["r"] = e.known_resp_image_device(d_text)

    r_first, r_ms, _ = timed(resp, args.reps)
    assert keep["r"][1].numel() == d_rec.numel()
    line["resp"] = leg(r_ms, n_entries, d_text.numel())
    line["resp_stream_bytes"] = int(d_text.numel())
    line["ratio_crl_over_resp_per_record"] = round(line["crl"]["ms_median"] / line["resp"]["ms_median"], 3)
    line["ratio_crl_over_copy"] = round(line["crl"]["ms_median"] / line["copy"]["ms_median"], 1)
    keep.pop("r")
    del d_text
    # the twin on the first CRLs, and the device held to it there
    n_small = max(min(args.python_entries // per, args.crls), 1)
    small = [blob[int(offsets[k]):int(offsets[k + 1])].tobytes() for k in range(n_small)]
    t0 = time.perf_counter()
    want = CRL.probes_image(small, digests[:n_small])
    py_s = time.perf_counter() - t0
    got, _ = e.crl_probes(small, digests[:n_small])
    assert got == want, "the device differs from the twin"
    line["python"] = {"crls": n_small, "entries": n_small * per, "s": round(py_s, 3), "records_per_s": n_small * per / py_s}
    line["ratio_crl_over_python_rate"] = round(line["crl"]["records_per_s"] / line["python"]["records_per_s"], 1)
    # which revoked serials a big engine knows
    if args.members:
        del d_rec
        keep.clear()
        cfg = synth.config(seed=20260921 + 7, n_issuers=256, zipf=1, dup_permille=20, ca_permille=10, expired_permille=10)
        a = ctmr.Engine(device=0, table_slots=args.slots, pair_slots=1 << 21)
        a.set_stream(stream)
        a.add_issuers(synth.issuers(cfg))
        a.set_filter(b"", False, synth.BASE_TIME)
        t0 = time.perf_counter()
        build_table(a, cfg, args.members, args.batch)
        build_s = time.perf_counter() - t0

        def revoked():
            keep["v"] = None
            keep["v"] = a.known_revoked((d_blob, offsets), digests, 0)

        v_first, v_ms, _ = timed(revoked, args.reps)
        hits = keep["v"][1]
        line["revoked"] = dict(leg(v_ms, n_entries, blob.size), members=int(a.total_count()), found=int((hits["records"] > 0).sum()),
                               build_s=round(build_s, 1), first_ms=round(v_first, 3))
        a.close()
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    e.close()


if __name__ == "__main__":
    main()
