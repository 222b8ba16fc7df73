"""Set algebra on known-certificate images (include/ctmr.h ctmr_known_merge*) at scale: one JSON line.

Two images A and B of --members members each under --issuers registered issuers (× --hours expDates), --shared permille of
the members common to both (built on the GPU: random 16-octet serials, each image made canonical by
Engine.known_sort_device).  HIP-event times, median of --reps after a warm-up, in one process, of
  union / minus / intersect         Engine.known_merge_device on the canonical operands (both used where they lie),
  union_unsorted                    UNION of the same images with their records shuffled (copy, sort and squeeze first),
  table_union                       the only route without the call: a fresh engine, known_import_device(A),
                                    known_import_device(B), known_export_device under CTMR_KNOWN_ORDER_SORTED,
  table_minus                       fresh engine, known_import_device(A), known_remove_device(B), the sorted export.
(INTERSECT has no table route that ends in an image: known_query gives flags; it is held against table_minus.)
Traffic model per member of the operands: the validation reads 48 B, the ascending check 48 B, the rank pass reads 48 B
and about log2(set) × 16 B of probes (mostly cache hits: neighbours probe neighbours) and writes 4 B, the place pass reads
48 + 4 B and writes 48 B per member of the result.  model_bytes = 200 B × operand members ranked + 48 B × result members.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` separately; --kernels-only runs just the merge legs."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import synth, known_image as KI, _native as N  # noqa: E402
from bench_known_image import timed  # noqa: E402


def build_images(eng, digests, hours, members, shared_permille, dev):
    """→ ((meta_a, d_a), (meta_b, d_b)): per set a universe of records of which A holds the first and B the last part."""
    keys = sorted((KI.set_key(h, d), h, d) for h in hours for d in digests)
    ns = len(keys)
    own = members * (1000 - shared_permille) // 1000          # members of A alone (and of B alone)
    per_u = (members + own + ns - 1) // ns                    # universe records per set
    per_own = own // ns
    per = per_u - per_own                                     # records per set of each image
    order = sorted(set(d for _, _, d in keys))
    ordinal = {d: i for i, d in enumerate(order)}
    uni = torch.zeros((ns, per_u, 48), dtype=torch.uint8, device=dev)
    uni[:, :, 0] = 16
    uni[:, :, 8:24] = torch.randint(0, 256, (ns, per_u, 16), dtype=torch.uint8, device=dev)
    out = []
    for lo in (0, per_own):
        rec = uni[:, lo:lo + per, :].contiguous().view(-1)
        sets = b"".join(KI._SET.pack(h, ordinal[d], s * per, per) for s, (_, h, d) in enumerate(keys))
        meta = KI._HEADER.pack(KI.MAGIC, KI.VERSION, 64, len(order), 0, ns, ns * per, 0, 0, 0) + b"".join(order) + sets
        meta += b"\0" * (-len(meta) % 64)
        eng.known_sort_device(meta, rec)
        out.append((meta, rec))
    return out, ns * per, ns * (per - per_own)


def shuffle_records(rec, ns, seed):
    """The records in a random order inside each of the ns equally large sets."""
    g = torch.Generator(device=rec.device)
    g.manual_seed(seed)
    rows = rec.view(ns, -1, 48)
    perm = torch.argsort(torch.rand(rows.shape[:2], generator=g, device=rec.device), dim=1)
    return torch.gather(rows, 1, perm.unsqueeze(-1).expand(-1, -1, 48)).contiguous().view(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=100_000_000)
    ap.add_argument("--issuers", type=int, default=256)
    ap.add_argument("--hours", type=int, default=4)
    ap.add_argument("--shared", type=int, default=900, help="permille of each image's members the other holds too")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    cfg = synth.config(seed=20260921 + 8, n_issuers=args.issuers)
    issuers = synth.issuers(cfg)

    def fresh_engine(slots):
        e = ctmr.Engine(device=0, table_slots=slots, pair_slots=1 << 14)
        e.set_stream(stream)
        e.add_issuers(issuers)
        e.set_filter(b"", False, synth.BASE_TIME)
        return e

    eng = fresh_engine(1 << 12)
    import base64
    digests = sorted(set(base64.urlsafe_b64decode(eng.issuer_id(k)) for k in range(len(issuers))))
    hours = [synth.BASE_TIME // 3600 + 24 * 400 + k for k in range(args.hours)]
    ((ma, da), (mb, db)), M, shared = build_images(eng, digests, hours, args.members, args.shared, dev)
    line = {"metric": "known_merge", "members_each": M, "shared": shared, "sets": len(digests) * len(hours),
            "issuers": len(digests)}
    ranked = {N.KNOWN_UNION: 2 * M, N.KNOWN_MINUS: M, N.KNOWN_INTERSECT: M}
    result = {N.KNOWN_UNION: 2 * M - shared, N.KNOWN_MINUS: M - shared, N.KNOWN_INTERSECT: shared}

    def leg(ms_list, op=None):
        ms = sorted(ms_list)[len(ms_list) // 2]
        out = {"ms_median": round(ms, 3), "ms_all": [round(x, 3) for x in ms_list],
               "operand_members_per_s": 2 * M / (ms * 1e-3)}
        if op is not None:
            model = 200 * ranked[op] + 48 * result[op]
            out["model_bytes"] = model
            out["model_TB_per_s"] = model / (ms * 1e-3) / 1e12
        return out

    keep = {}
    names = {N.KNOWN_UNION: "union", N.KNOWN_MINUS: "minus", N.KNOWN_INTERSECT: "intersect"}
    for op, name in names.items():
        def run():
            keep["r"] = None
            keep["r"] = eng.known_merge_device(op, ma, da, mb, db)
        _, ms, _ = timed(run, args.reps)
        line[name] = leg(ms, op)
        line[name]["members"] = keep["r"][1].numel() // 48
        assert line[name]["members"] == result[op], (name, line[name]["members"], result[op])
    want_union = None
    if not args.kernels_only:
        keep["r"] = eng.known_merge_device(N.KNOWN_UNION, ma, da, mb, db)
        want_union = (keep["r"][0], keep["r"][1].clone())
        keep["r"] = eng.known_merge_device(N.KNOWN_MINUS, ma, da, mb, db)
        want_minus = (keep["r"][0], keep["r"][1].clone())
    keep.clear()
    sa, sb = shuffle_records(da, line["sets"], 1), shuffle_records(db, line["sets"], 2)

    def run_unsorted():
        keep["r"] = None
        keep["r"] = eng.known_merge_device(N.KNOWN_UNION, ma, sa, mb, sb)
    _, ms, _ = timed(run_unsorted, args.reps)
    line["union_unsorted"] = leg(ms)
    if want_union is not None:
        line["union_unsorted"]["equals_union"] = bool(keep["r"][0] == want_union[0] and torch.equal(keep["r"][1], want_union[1]))
    keep.clear()
    del sa, sb
    if not args.kernels_only:
        slots = 1 << max(int(np.ceil(np.log2(4 * M))), 12)

        tab = {}

        def fresh():                                   # the engine is made outside the timed part
            keep["r"] = None
            if tab.get("e") is not None:
                tab["e"].close()
            tab["e"] = fresh_engine(slots)
            tab["e"].set_known_order(N.KNOWN_ORDER_SORTED)

        def table(remove):
            def run():
                e = tab["e"]
                e.known_import_device(ma, da)
                if remove:
                    e.known_remove_device(mb, db)
                else:
                    e.known_import_device(mb, db)
                keep["r"] = e.known_export_device()
            return run
        for name, remove, want in (("table_union", False, want_union), ("table_minus", True, want_minus)):
            _, ms, _ = timed(table(remove), args.reps, before=fresh)
            line[name] = leg(ms)
            line[name]["equals_merge"] = bool(keep["r"][0] == want[0] and torch.equal(keep["r"][1], want[1]))
            keep.clear()
        for name, route in (("union", "table_union"), ("minus", "table_minus"), ("intersect", "table_minus")):
            line[name + "_over_" + route] = round(line[name]["ms_median"] / line[route]["ms_median"], 4)
        tab["e"].close()
    print(json.dumps(line))
    eng.close()


if __name__ == "__main__":
    main()
