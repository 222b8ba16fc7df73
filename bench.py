#!/usr/bin/env python3
"""bench.py — certificates/sec + achieved HBM GB/s of the map/reduce hot path on MI355X.

A "step" is one pass of the hot path (packed DER → TBS walk → 3 filters → known-certificate set
insert → WasUnknown resolve → per-issuer counts → NEW-list compaction) over one synthetic CT
batch that is already resident in HBM.  The known-certificate table is cleared inside every
timed step, so every step does the same "first sighting" work.

    python bench.py --gpus 1 --steps 5 --warmup 1
    python bench.py --gpus 1 --steps 5 --warmup 1 --dump-outputs DIR    # … and what the last timed step computed, as DIR/*.npy
    python bench.py --gpus 1 --steps 5 --warmup 1 --full                # … and everything else the line measures and checks
    python bench.py --gpus N                       # spawns its own N rank processes (one per GPU), rank 0 prints the line
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W          # … or runs under a launcher's RANK/WORLD_SIZE

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line: `value`, `ms_per_step`, the
kernel times and the algorithmic roofline.  --full adds what takes time or runs of its own: the PMC traffic passes
(--traffic), the checks against the generator, the oracle-checked sample and the CPU baseline legs (--no-cpu), the
bytes the walk needs, and the secondary legs of the one-GPU line (--no-secondary).

N > 1 (BASELINE configs[3]): ONE batch of --total-entries (default 100 M) is split by log-index range — rank r owns
[r·T/N, (r+1)·T/N), strong scaling — and the dedup is GLOBAL and exact by default (--dedup bloom: the all-gather of
per-GPU Bloom filters as an exact pre-filter; --dedup owner: the owner-computes key exchange), what one Redis SADD gives
the reference's processes (storage/rediscache.go:57-65; cmd/ct-fetch/ct-fetch.go:288-305).  --dedup local keeps per-shard
sets and says so.  --entries E instead gives every GPU E entries (weak scaling).  Everything on the data path — shard
maps, exchanges, the all-reduce of the per-issuer counts, barriers, the max of the step time — goes through the library's
own RCCL group; the host only hands the 128-byte group id to its ranks (environment of the spawned processes, or one
broadcast over the launcher's rendezvous).  At every N a --full run checks itself: Σ NEW and every entry's WasUnknown against
the generator's duplicate structure, the all-reduced per-issuer counts against the generator, and a strided sample of
every rank's shard (+ the out-of-shard sources of its duplicates) against the oracle.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0   # MI355X HBM3E peak, /opt/skills/guides/MI355X_MICROARCH.md
ALG_BYTES_FIXED = 45     # offsets 8 + issuer_idx 4 + entry_type 1 + record 32


MAP_KERNELS = {1: "k_map_tile", 2: "k_map_direct", 13: "k_map_winc<13, false>", 15: "k_map_fused<13, false, 0, false>"}   # 1, 2: sweep build only
# … under the reference profile (and with strict_strings / strict_extensions alone): the STRICT instantiation
MAP_KERNELS_STRICT = {13: "k_map_winc<14, true>", 15: "k_map_fused<14, false, 0, true>"}


def map_kernel_name(args):
    v = args.variant or DEFAULT_VARIANT
    strict = args.profile == "reference" or args.strict_strings or args.strict_extensions
    return MAP_KERNELS_STRICT.get(v, MAP_KERNELS[v]) if strict else MAP_KERNELS[v]
DEFAULT_VARIANT = 15
FUSED = (15,)          # map kernels that also do pass 1 of the known-certificate insert
ALG_BYTES_PROBE = 64   # per PASS entry: 32 B slot read + 32 B slot write — fused kernels only


def pow2_at_least(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def cpu_baseline(batch_arrays, issuers, filt, now, sample, entry_type=None, profile="reference"):
    """The oracle's restatement of the reference loop, timed on one host core (kind "port"), over `sample` entries of
    the SAME batch the GPU processed (payload, offsets, issuer_idx[, entry_type]), in the SAME accept/reject profile."""
    import numpy as np
    from oracle import oracle as orc
    payload, offsets, issuer_idx = batch_arrays
    io = np.zeros(len(issuers) + 1, np.uint64)
    io[1:] = np.cumsum([len(x) for x in issuers])
    blob = np.frombuffer(b"".join(issuers), np.uint8)
    o = orc.Engine(filt, False, now)
    o.set_profile(profile)
    t0 = time.perf_counter()
    st, unk, eh = o.batch(payload, offsets, issuer_idx, blob, io, entry_type=entry_type)
    dt = time.perf_counter() - t0
    return {"value": sample / dt, "unit": "certificates/sec", "cores": 1, "kind": "port",
            "sample": f"{sample} entries, oracle/ctmr_oracle.c "
                      f"(in-process hash set stands in for Redis; not the Go binary), {dt:.1f} s",
            "host_cores_available": os.cpu_count()}, (st, unk)


def cpu_quota():
    """CPUs this process may use at once: the cgroup quota when there is one (a 256-thread box may be shared out in
    16-CPU pods), else the affinity mask."""
    aff = len(os.sched_getaffinity(0))
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]            # cgroup v2
        if q != "max":
            return min(aff, max(1, -(-int(q) // int(per)))), int(q) / int(per)
    except (OSError, ValueError):
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())           # cgroup v1
        per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        if q > 0:
            return min(aff, max(1, -(-q // per))), q / per
    except (OSError, ValueError):
        pass
    return aff, None


def cpu_baseline_threads(batch_arrays, issuers, filt, now, sample, threads, profile="reference"):
    """The same restatement on `threads` host threads: contiguous slices of the sample, one oracle engine (its own
    in-process sets) per thread — T reference processes with -offset/-limit, minus the Redis they would share, so
    this flatters the CPU side slightly.  ctypes releases the GIL for the duration of each call."""
    import threading
    import numpy as np
    from oracle import oracle as orc
    payload, offsets, issuer_idx = batch_arrays
    io = np.zeros(len(issuers) + 1, np.uint64)
    io[1:] = np.cumsum([len(x) for x in issuers])
    blob = np.frombuffer(b"".join(issuers), np.uint8)
    engines = [orc.Engine(filt, False, now) for _ in range(threads)]
    for e in engines:
        e.set_profile(profile)
    bounds = [sample * t // threads for t in range(threads + 1)]
    gate = threading.Barrier(threads + 1)
    n_pass = [0] * threads

    def work(t):
        lo, hi = bounds[t], bounds[t + 1]
        gate.wait()
        if hi > lo:
            st, _, _ = engines[t].batch(payload, offsets[lo:hi + 1], issuer_idx[lo:hi], blob, io)
            n_pass[t] = int((st == 0).sum())
        gate.wait()

    ths = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
    for th in ths:
        th.start()
    gate.wait()
    t0 = time.perf_counter()
    gate.wait()
    dt = time.perf_counter() - t0
    for th in ths:
        th.join()
    for e in engines:
        e.close()
    return sample / dt, dt, sum(n_pass)


def _mix64(z, np):
    z = z + np.uint64(0x9e3779b97f4a7c15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def synth_is_dup(seed, first, n, dup_permille, np):
    """numpy restatement of csrc/synth.h synth_is_dup for entries [first, first+n)."""
    with np.errstate(over="ignore"):
        i = np.arange(first, first + n, dtype=np.uint64)
        base = _mix64(np.uint64(seed) ^ np.uint64((1 * 0xd6e8feb86659fd93) & 0xffffffffffffffff), np)
        h = _mix64(base + i, np)
        return (i > 0) & ((h % np.uint64(1000)) < np.uint64(dup_permille))


def lib_hash():
    """sha256 of the library the kernels come from: traffic measured on another build is refused."""
    import hashlib
    from ct_mapreduce_amd import _native as N
    return hashlib.sha256(open(N.LIB_PATH, "rb").read()).hexdigest()[:16]


def parse_pmc_csv(outdir, counter, kernel_substr):
    """Average per-launch value of one rocprofv3 --pmc counter over the launches of one kernel."""
    import csv
    import glob
    vals = []
    for f in glob.glob(os.path.join(outdir, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if row.get("Counter_Name") == counter and kernel_substr in row.get("Kernel_Name", ""):
                vals.append(float(row["Counter_Value"]))
    return (sum(vals) / len(vals), len(vals)) if vals else (None, 0)


def measure_traffic(args, entries, kernels, mode_args=()):
    """HBM traffic of the named kernels, measured NOW on this build: re-executes this script on a smaller batch of the
    same corpus under `rocprofv3 --pmc FETCH_SIZE` and `--pmc WRITE_SIZE` (separate passes, no trace flags:
    MI355X_MICROARCH.md §HBM / §rocprofv3 PMC slots) and returns bytes per ENTRY per kernel.  gfx950 correction: FETCH_SIZE
    tallies 128-byte requests at 64 bytes — x2 (calibrated on this access pattern too: scripts/calib_fetch.hip,
    profiles/r01/s2); WRITE_SIZE as is.  Both are reported in KiB by rocprofv3.  `kernels`: name substrings; the first
    one is the line's dominant kernel.  `mode_args`: what selects this line's mode in the child (--raw, --meta, …)."""
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None, "rocprofv3 not on PATH"
    tmp = tempfile.mkdtemp(prefix="ctmr_pmc_", dir=os.environ.get("TMPDIR", "/tmp"))
    env = dict(os.environ, CTMR_BENCH_CHILD="1", TMPDIR=os.environ.get("TMPDIR", "/tmp"))
    child = [sys.executable, os.path.abspath(__file__), "--entries", str(entries), "--steps", "2", "--warmup", "1",
             "--no-cpu", "--traffic", "off", "--no-secondary", "--issuers", str(args.issuers), "--variant", str(args.variant),
             "--dup-permille", str(args.dup_permille)] + list(mode_args)
    out = {"entries": entries, "kernels": {}}
    for c in ("FETCH_SIZE", "WRITE_SIZE"):
        d = os.path.join(tmp, c)
        try:
            r = subprocess.run([exe, "--pmc", c, "-d", d, "-o", "pmc", "--output-format", "csv", "--"] + child,
                               cwd=tmp, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=420)
        except subprocess.TimeoutExpired:
            return None, f"rocprofv3 --pmc {c} pass timed out"
        for k in kernels:
            v, n = parse_pmc_csv(d, c, k)
            if v is None:
                return None, f"rocprofv3 --pmc {c}: no rows for {k} (rc {r.returncode}): " + r.stdout.decode(errors="replace")[-300:]
            out["kernels"].setdefault(k, {})[c + "_KB_per_launch"] = v
            out["kernels"][k]["launches"] = n
    shutil.rmtree(tmp, ignore_errors=True)
    for k, t in out["kernels"].items():
        t["fetch_bytes_per_cert"] = 2.0 * t["FETCH_SIZE_KB_per_launch"] * 1024.0 / entries
        t["write_bytes_per_cert"] = t["WRITE_SIZE_KB_per_launch"] * 1024.0 / entries
        t["traffic_bytes_per_cert"] = t["fetch_bytes_per_cert"] + t["write_bytes_per_cert"]
    first = out["kernels"][kernels[0]]
    for f in ("FETCH_SIZE_KB_per_launch", "WRITE_SIZE_KB_per_launch", "launches", "fetch_bytes_per_cert", "write_bytes_per_cert",
              "traffic_bytes_per_cert"):
        out[f] = first[f]                     # the dominant kernel's figures at the top level (the r02 file format)
    out["lib_sha256_16"] = lib_hash()
    return out, None


def needed_bytes_per_cert(certs, starts, filt, reference_profile=True):
    """What the walk READS of a certificate (the product's walk compiled for the host with a marking reader,
    tests/harness): bytes covered by its reads, and the distinct 128-byte HBM lines they lie in at the certificate's
    real position in the payload — the floor of the map kernel's fetch traffic at line granularity."""
    from tests import harness
    nb = nl = 0
    for der, st in zip(certs, starts):
        _, b, l = harness.walk_touched(der, int(st) & 127, filt, reference_profile)
        nb += b
        nl += l
    return nb / len(certs), nl * 128.0 / len(certs)


def strided_sample(E, slices, per_slice):
    """[lo, hi) ranges of `slices` equally spaced slices of `per_slice` entries over [0, E)."""
    per_slice = min(per_slice, max(1, E // slices))
    return [(k * (E // slices), k * (E // slices) + per_slice) for k in range(slices)]


def gather_sample(d_off, d_pay, d_iss, d_et, ranges, extra_idx, extra_certs, pad, np, base=0):
    """One host batch = the sampled slices copied back from HBM + `extra` single entries (index → (der, issuer_idx,
    entry_type)), all in ascending log-index order.  `ranges` index the device arrays (a rank's shard); `base` = log
    index of the shard's entry 0; `extra_idx` are log indices.  Returns (payload, offsets, issuer_idx, entry_type, log_index)."""
    pieces = []          # (first_index, payload u8, lens u64, iss u32, et u8)
    for lo, hi in ranges:
        offs = d_off[lo:hi + 1].cpu().numpy().astype(np.uint64)
        pay = d_pay[int(offs[0]):int(offs[-1])].cpu().numpy()
        pieces.append((base + lo, pay, np.diff(offs), d_iss[lo:hi].cpu().numpy().astype(np.uint32),
                       d_et[lo:hi].cpu().numpy().astype(np.uint8), np.arange(base + lo, base + hi, dtype=np.uint64)))
    for i, (der, iss, et) in zip(extra_idx, extra_certs):
        pieces.append((int(i), np.frombuffer(der, np.uint8), np.array([len(der)], np.uint64),
                       np.array([iss], np.uint32), np.array([et], np.uint8), np.array([i], np.uint64)))
    pieces.sort(key=lambda t: t[0])
    payload = np.concatenate([t[1] for t in pieces] + [np.zeros(pad, np.uint8)])
    lens = np.concatenate([t[2] for t in pieces])
    offsets = np.zeros(len(lens) + 1, np.uint64)
    offsets[1:] = np.cumsum(lens)
    return (payload, offsets, np.concatenate([t[3] for t in pieces]), np.concatenate([t[4] for t in pieces]),
            np.concatenate([t[5] for t in pieces]))


def synth_src(seed, idx, dup_permille, np):
    """numpy restatement of csrc/synth.h synth_src: the entry whose key entry i repeats (i itself if it is no duplicate)."""
    with np.errstate(over="ignore"):
        idx = np.asarray(idx, dtype=np.uint64)
        src = idx.copy()
        dup = synth_is_dup_at(seed, idx, dup_permille, np)
        base = _mix64(np.uint64(seed) ^ np.uint64((2 * 0xd6e8feb86659fd93) & 0xffffffffffffffff), np)
        j = _mix64(base + idx[dup], np) % idx[dup]
        while True:                                  # walk down to the nearest entry that is no duplicate itself
            d = synth_is_dup_at(seed, j, dup_permille, np)
            if not d.any():
                break
            j = np.where(d, j - np.uint64(1), j)
        src[dup] = j
        return src, dup


def synth_is_dup_at(seed, idx, dup_permille, np):
    with np.errstate(over="ignore"):
        idx = np.asarray(idx, dtype=np.uint64)
        base = _mix64(np.uint64(seed) ^ np.uint64((1 * 0xd6e8feb86659fd93) & 0xffffffffffffffff), np)
        h = _mix64(base + idx, np)
        return (idx > 0) & ((h % np.uint64(1000)) < np.uint64(dup_permille))


def _mix64_t(z, torch):
    """_mix64 on int64 tensors (two's-complement wrap-around is the uint64 arithmetic; shifts made logical by masking)."""
    def c(v):
        return v - (1 << 64) if v >= (1 << 63) else v
    def lsr(x, k):
        return (x >> k) & ((1 << (64 - k)) - 1)
    z = z + c(0x9e3779b97f4a7c15)
    z = (z ^ lsr(z, 30)) * c(0xbf58476d1ce4e5b9)
    z = (z ^ lsr(z, 27)) * c(0x94d049bb133111eb)
    return z ^ lsr(z, 31)


def synth_is_dup_torch(seed, first, n, dup_permille, torch, dev):
    """synth_is_dup for entries [first, first+n) as a bool tensor on `dev` (the numpy form takes seconds at 100 M entries)."""
    import numpy as np
    i = torch.arange(first, first + n, dtype=torch.int64, device=dev)
    with np.errstate(over="ignore"):
        base = int(_mix64(np.uint64(seed) ^ np.uint64((1 * 0xd6e8feb86659fd93) & 0xffffffffffffffff), np))
    base = base - (1 << 64) if base >= (1 << 63) else base
    h = _mix64_t(i + base, torch)
    hi, lo = (h >> 32) & 0xffffffff, h & 0xffffffff            # h mod 1000 without an unsigned type
    r = ((hi % 1000) * ((1 << 32) % 1000) + lo % 1000) % 1000
    return (i > 0) & (r < dup_permille)


def spawn_ranks(n):
    """`python bench.py --gpus N` with no launcher environment: this process becomes the launcher.  It makes the group id
    (ncclGetUniqueId through the library — the bootstrap listener lives in this process, which therefore stays until the
    ranks are done), starts one copy of itself per rank with RANK / LOCAL_RANK / WORLD_SIZE and the id in the
    environment, lets rank 0's line through and returns the worst exit code."""
    import subprocess
    import torch  # noqa: F401  (the ranks import torch before the library loads librccl: the id must come from the SAME
    #                             librccl — PyTorch-ROCm bundles one under the same SONAME — not from another version's bootstrap)
    from ct_mapreduce_amd.distributed import Group
    gid = Group.unique_id()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), CTMR_GROUP_ID=gid.hex(),
                   CTMR_BENCH_SPAWNED="1")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    out0, _ = procs[0].communicate()
    codes = [procs[0].returncode] + [p.wait() for p in procs[1:]]
    sys.stdout.write(out0.decode(errors="replace"))
    sys.stdout.flush()
    if any(codes):
        sys.stderr.write(f"bench: rank exit codes {codes}\n")
    return max(abs(c) for c in codes)


def group_id_from_launcher(rank, make_id):
    """Under a launcher (torchrun: RANK / WORLD_SIZE / MASTER_* in the environment): rank 0 makes the 128-byte group id
    and one broadcast over the launcher's rendezvous (gloo, 127.0.0.1) hands it to the others — the only thing
    torch.distributed carries; the process group is torn down right after."""
    import torch.distributed as dist
    dist.init_process_group(os.environ.get("CTMR_DIST_BACKEND", "gloo"))
    box = [make_id() if rank == 0 else None]
    dist.broadcast_object_list(box, src=0)
    dist.destroy_process_group()
    return box[0]


class WriteBack:
    """BASELINE configs[4]'s other half: what FilesystemDatabase.Store does behind WasUnknown (storage/filesystemdatabase.go:
    183-208) for every wave of the stream — IssuerMetadata.Accumulate's first sightings (k_meta_new over the NEW list), the
    PEM block of every new certificate (k_pem_encode, in chunks of the NEW list) and backend.StoreCertificatePEM +
    markDirty through the C++ restatement of the reference's backends (ct_mapreduce_amd/host_writeback.py).
    noop: the reference with certPath unset — the PEM bytes are produced (pem.EncodeToMemory runs before the backend is asked)
    and dropped on the device.  disk: device → pinned host → LocalDiskBackend files, two chunks in flight: the GPU goes on
    with the next chunk / wave while the host writes; when it must wait for the host, that time is the STALL."""
    CHUNK = 8_000_000

    def __init__(self, args, eng, synth, cfg, torch, np, dev, Wr, rank, filt, now, N):
        import tempfile
        from ct_mapreduce_amd.host_writeback import HostWriter
        self.torch, self.np, self.eng, self.dev, self.synth, self.cfg, self.N = torch, np, eng, dev, synth, cfg, N
        self.filt, self.now, self.rank = filt, now, rank
        self.disk = args.write_back == "disk"
        self.ch = min(Wr, self.CHUNK)
        self.pem_cap = self.ch * 2900 + 4096
        nbuf = 2 if self.disk else 1
        self.d_pem = [torch.empty(self.pem_cap, dtype=torch.uint8, device=dev) for _ in range(nbuf)]
        self.d_pemoff = [torch.empty(self.ch + 1, dtype=torch.int64, device=dev) for _ in range(nbuf)]
        self.d_items = torch.empty(32 * (1 << 20), dtype=torch.uint8, device=dev)
        self.root = self.cwd0 = None
        if self.disk:
            base = args.write_back_dir or tempfile.mkdtemp(prefix="ctmr_wb_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
            self.root = os.path.join(base, "certs%d" % rank)
            os.makedirs(self.root, exist_ok=True)
            # LocalDiskBackend.MarkDirty writes <day>/dirty relative to the CURRENT directory (localdiskbackend.go:89-91)
            self.cwd0 = os.getcwd()
            self.dirty_dir = os.path.join(base, "cwd%d" % rank)
            os.makedirs(self.dirty_dir, exist_ok=True)
            os.chdir(self.dirty_dir)
            self.h_pem = [torch.empty(self.pem_cap, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            self.h_off = [torch.empty(self.ch + 1, dtype=torch.int64, pin_memory=True) for _ in range(2)]
            self.h_rec = [torch.empty(self.ch * 32, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        n_iss = len(synth.issuers(cfg))
        self.writer = HostWriter(self.root, [eng.issuer_id(k) for k in range(n_iss)], args.write_back_threads)
        self.jobs = [None, None]
        self.turn = 0
        self.files = self.pem_bytes = self.skipped = self.meta_items = self.new_total = 0
        self.t_stall = self.t_meta = self.t_pem = self.t_host_busy = 0.0
        self.check = None
        self.days = set()

    def _retire(self, b):
        if self.jobs[b] is not None:
            t0 = time.perf_counter()
            f, by, sk, sec = self.writer.wait(self.jobs[b])
            self.t_stall += time.perf_counter() - t0
            self.files += f; self.pem_bytes += by; self.skipped += sk; self.t_host_busy += sec
            self.jobs[b] = None

    def wave(self, k, first, n, n_new, d_pay, d_off, d_iss, d_et, d_rec, d_new):
        torch = self.torch
        self.new_total += n_new
        if n_new:
            t0 = time.perf_counter()
            self.meta_items += self.eng.meta_new_device(d_pay.data_ptr(), d_off.data_ptr(), 0, d_rec.data_ptr(), d_new.data_ptr(),
                                                        n_new, self.d_items.data_ptr(), 1 << 20)
            torch.cuda.synchronize()
            self.t_meta += time.perf_counter() - t0
        recs = d_rec.view(-1, 32)[:n]
        if self.disk and n:     # markDirty: every entry that reached Store marks its day (filesystemdatabase.go:204-208)
            hours = recs[recs[:, 0] == 0][:, 4:8].contiguous().view(torch.int32).view(-1)
            days = torch.unique(torch.div(hours, 24, rounding_mode="floor")).tolist()
            fresh = [d for d in days if d not in self.days]
            self.days.update(fresh)
            if fresh:
                self.writer.mark_dirty(fresh)
        for c in range(0, n_new, self.ch):
            m = min(self.ch, n_new - c)
            b = self.turn
            self._retire(b)                       # the buffers of two chunks ago are free again (disk) / nothing (noop)
            t0 = time.perf_counter()
            nbytes = self.eng.pem_encode_device(d_pay.data_ptr(), d_off.data_ptr(), d_new.data_ptr() + 8 * c, m,
                                                self.d_pem[b % len(self.d_pem)].data_ptr(), self.pem_cap,
                                                self.d_pemoff[b % len(self.d_pemoff)].data_ptr())
            torch.cuda.synchronize()
            self.t_pem += time.perf_counter() - t0
            if not self.disk:
                self.files += m; self.pem_bytes += nbytes     # NoopBackend.StoreCertificatePEM: nothing to do with them
                continue
            idx = d_new[c:c + m]
            self.h_rec[b][:m * 32].copy_(d_rec.view(-1, 32)[idx].reshape(-1), non_blocking=True)
            self.h_off[b][:m + 1].copy_(self.d_pemoff[b][:m + 1], non_blocking=True)
            self.h_pem[b][:nbytes].copy_(self.d_pem[b][:nbytes], non_blocking=True)
            torch.cuda.synchronize()
            self.jobs[b] = self.writer.submit(self.h_pem[b].data_ptr(), self.h_off[b].data_ptr(), self.h_rec[b].data_ptr(), m)
            self.turn ^= 1
        if self.disk and k == 0 and self.check is None:
            self._retire(0); self._retire(1)
            t0 = time.perf_counter()
            self.check = self._check_wave0(first, n, n_new, d_pay, d_off, d_iss, d_et)
            return time.perf_counter() - t0       # the checker's time is not the product's
        return 0.0

    def _check_wave0(self, first, n, n_new, d_pay, d_off, d_iss, d_et):
        """The files on disk after wave 0 = the oracle's NEW set of wave 0: same paths, same bytes (every file when there
        are at most 300 000, else 20 000 of them)."""
        from oracle import oracle as orc
        np = self.np
        t0 = time.perf_counter()
        off = d_off[:n + 1].cpu().numpy().astype(np.uint64)
        pay = d_pay[:int(off[n]) + self.N.PAYLOAD_PAD].cpu().numpy()
        iss = d_iss[:n].cpu().numpy().astype(np.uint32)
        et = d_et[:n].cpu().numpy()
        issuers = self.synth.issuers(self.cfg)
        io = np.zeros(len(issuers) + 1, np.uint64)
        io[1:] = np.cumsum([len(x) for x in issuers])
        o = orc.Engine(self.filt, False, self.now)
        st, unk, eh = o.batch(pay, off, iss, np.frombuffer(b"".join(issuers), np.uint8), io, entry_type=et)
        want = {}
        ids = [self.eng.issuer_id(k) for k in range(len(issuers))]
        import base64
        for i in np.nonzero(unk)[0]:
            der = pay[int(off[i]):int(off[i + 1])].tobytes()
            c = orc.parse_cert(der)
            serial = der[c.serial_off:c.serial_off + c.serial_len]
            want[os.path.join(orc.exp_date_id(int(eh[i])), ids[int(iss[i])], base64.urlsafe_b64encode(serial).decode())] = int(i)
        have = set()
        for dp, _, fs in os.walk(self.root):
            rel = os.path.relpath(dp, self.root)
            have.update(os.path.join(rel, f) for f in fs)
        same_paths = have == set(want)
        paths = sorted(want)
        if len(paths) > 300_000:
            paths = paths[::max(1, len(paths) // 20_000)]
        bad = 0
        for pth in paths:
            i = want[pth]
            try:
                bad += open(os.path.join(self.root, pth), "rb").read() != orc.pem_encode(pay[int(off[i]):int(off[i + 1])].tobytes())
            except OSError:
                bad += 1
        dirty = sorted(os.listdir(self.dirty_dir))
        want_days = sorted({orc.day_id(int(orc.parse_cert(pay[int(off[i]):int(off[i + 1])].tobytes()).not_after))
                            for i in np.nonzero(st == 0)[0][::max(1, int((st == 0).sum()) // 5000)]})
        return {"wave": 0, "entries": int(n), "oracle_new": int(unk.sum()), "gpu_new": int(n_new), "files_on_disk": len(have),
                "paths_equal_the_oracles_new_set": bool(same_paths), "files_compared_bytewise": len(paths),
                "files_differing": int(bad), "dirty_markers_cover_the_sampled_days": bool(set(want_days) <= set(dirty)),
                "seconds": round(time.perf_counter() - t0, 1)}

    def finish(self):
        self._retire(0); self._retire(1)

    def report(self, wall, t_timed):
        if self.cwd0:
            os.chdir(self.cwd0)
        self.writer.close()
        ok = self.files + self.skipped == self.new_total and (self.check is None or (
            self.check["paths_equal_the_oracles_new_set"] and self.check["files_differing"] == 0 and
            self.check["oracle_new"] == self.check["gpu_new"] and self.check["dirty_markers_cover_the_sampled_days"]))
        out = {"backend": "LocalDiskBackend" if self.disk else "NoopBackend", "new_certificates": self.new_total,
               "files_handed_to_the_backend": self.files, "long_serials_left_to_the_host_parse": self.skipped,
               "pem_bytes": self.pem_bytes, "pem_GB_per_s_of_the_encode_kernels": self.pem_bytes / max(self.t_pem, 1e-9) / 1e9,
               # what the PEM calls move: the DER they read (recovered from the PEM size: 54 framing bytes per certificate, 65 output
               # bytes per 48 input bytes; exact to the padding) plus the PEM they write, over the calls' wall time (k_pem_len,
               # the scan, k_pem_blocks and k_pem_encode of every chunk) against the 8 TB/s HBM peak
               "pem_read_plus_written_GB_per_s": (self.pem_bytes + (self.pem_bytes - 54 * self.new_total) * 48 / 65) / max(self.t_pem, 1e-9) / 1e9,
               "pem_frac_of_hbm_peak": (self.pem_bytes + (self.pem_bytes - 54 * self.new_total) * 48 / 65) / max(self.t_pem, 1e-9) / 1e9 / HBM_PEAK_GBPS,
               "ms_meta_total": self.t_meta * 1e3, "ms_pem_total": self.t_pem * 1e3,
               "meta_first_sightings": self.meta_items, "ok": bool(ok)}
        if self.disk:
            out.update({"root": self.root, "host_threads": self.writer.threads,
                        "host_files_per_s": self.files / max(self.t_host_busy, 1e-9),
                        "host_busy_s": self.t_host_busy, "stall_s_waiting_for_the_host": self.t_stall,
                        "stall_fraction_of_the_timed_region": self.t_stall / max(t_timed, 1e-9),
                        "check_wave0_vs_oracle": self.check,
                        "note": "device → pinned host copies of PEM bytes are inside the timed region (PCIe-inclusive by nature); "
                                "the host writer runs while the GPU maps the next chunk / wave, the GPU waits only when both "
                                "host buffers are still being written"})
        else:
            out["note"] = ("storage.NoopBackend ignores the PEM bytes: they are encoded on the GPU (the reference runs "
                           "pem.EncodeToMemory before it asks the backend) and never copied to the host")
        return out


def run_stream(args, ctmr, synth, N, torch, np, dev, local, rank, world, cfg, filt, now, issuers, gid=None):
    """BASELINE configs[4]: a long stream with 10 % duplicates, the known-certificate sets persisting across waves.  One GPU:
    one engine, one table.  N > 1: every wave is split by log-index range over the ranks and deduplicated GLOBALLY through
    the group (owner-computes by default — in a long stream it moves fewer bytes than ever-growing filters; --dedup bloom for
    the north_star's variant); the sets persist on the ranks across the waves."""
    from ct_mapreduce_amd.distributed import Group, shard as make_shard, shard_range
    T = args.stream
    wb = args.write_back
    W = min(args.entries or (50_000_000 if not wb else 25_000_000 if wb == "noop" else 1_000_000), T)   # entries per wave, over all ranks
    cfg = synth.config(seed=20260921 + 5, n_issuers=args.issuers, zipf=1, dup_permille=100, ca_permille=10,
                       expired_permille=10)
    mode = "plain" if world == 1 else (args.dedup if args.dedup != "auto" else "owner")
    per_rank_keys = (T + world - 1) // world
    slots = min(pow2_at_least(int(per_rank_keys * 1.6)), 1 << 31)
    eng = ctmr.Engine(device=local, table_slots=slots, pair_slots=1 << 22, map_variant=args.variant, profile=True,
                      collect_meta=bool(wb))
    eng.set_profile(args.profile)          # before the issuers are registered
    eng.add_issuers(synth.issuers(cfg))
    eng.set_filter(filt, False, now)
    group = None
    if world > 1:
        group = Group.rccl(eng, gid, rank, world)
        if args.chunks > 1:
            group.set_chunks(args.chunks)
        if mode == "bloom":
            group.bloom_config(pow2_at_least(16 * per_rank_keys))
    Wr = (W + world - 1) // world + 1                    # the largest shard of a wave
    d_off = torch.empty(Wr + 1, dtype=torch.int64, device=dev)
    d_iss = torch.empty(Wr, dtype=torch.int32, device=dev)
    d_et = torch.empty(Wr, dtype=torch.uint8, device=dev)
    d_rec = torch.empty(Wr * 32, dtype=torch.uint8, device=dev)
    d_new = torch.empty(Wr, dtype=torch.int64, device=dev)
    d_pay = torch.empty(int(Wr * 1600) + 4096, dtype=torch.uint8, device=dev)
    t_gpu = t_map = 0.0
    tot_new = tot_dup = tot_pass = tot_bytes = 0
    bad_entries = 0
    wire = 0
    ok = True
    waves = 0
    first = 0
    wbs = WriteBack(args, eng, synth, cfg, torch, np, dev, Wr, rank, filt, now, N) if wb else None
    t_wall0 = time.perf_counter()
    while first < T:
        n_wave = min(W, T - first)
        lo, hi = shard_range(n_wave, rank, world)
        n = hi - lo
        if n:
            eng.synth_device(cfg, first + lo, n, d_off.data_ptr(), d_pay.data_ptr(), d_pay.numel(), d_iss.data_ptr(),
                             d_et.data_ptr())
        torch.cuda.synchronize()
        if group is not None:
            group.barrier()
        t0 = time.perf_counter()
        if group is not None:
            st = group.map_batch(mode, [make_shard(d_pay.data_ptr(), d_off.data_ptr(), d_iss.data_ptr(), d_et.data_ptr(), n,
                                                   d_rec.data_ptr(), d_new.data_ptr(), order_base=first + lo)])[0]
            wire += int(group.info().wire_bytes_sent)
        else:
            st = eng.map_batch_device(d_pay.data_ptr(), d_off.data_ptr(), d_iss.data_ptr(), d_et.data_ptr(), n,
                                      d_rec.data_ptr(), d_new.data_ptr())
        if wbs is not None:   # FilesystemDatabase.Store behind WasUnknown, for the wave (filesystemdatabase.go:183-208)
            t0 += wbs.wave(waves, first + lo, n, int(st.n_new), d_pay, d_off, d_iss, d_et, d_rec, d_new)
        t_gpu += time.perf_counter() - t0
        t_map += st.ms_map
        # the generator's structure: entry i duplicates an EARLIER entry's key iff synth_is_dup(i) — in this wave or
        # any earlier one, on this rank or any other — so PASS ∧ dup must be known and PASS ∧ ¬dup must be new, wave by wave
        recs = d_rec.view(-1, 32)[:n]
        passed = recs[:, 0] == 0
        is_new = (recs[:, 1] & 2) != 0
        dupm = synth_is_dup_torch(cfg.seed, first + lo, n, 100, torch, dev)
        exp_new = int((passed & ~dupm).sum().item())
        exp_dup = int((passed & dupm).sum().item())
        bad_entries += int((is_new != (passed & ~dupm)).sum().item())
        good = exp_new == int(st.n_new) and exp_dup == int(st.n_dup)
        ok = ok and good
        sys.stderr.write(f"stream: rank {rank} wave {waves} [{first + lo}, {first + hi}) new {st.n_new} dup {st.n_dup} "
                         f"({'ok' if good else 'MISMATCH: expected %d/%d' % (exp_new, exp_dup)}) "
                         f"map {st.ms_map:.2f} ms total {st.ms_total:.2f} ms\n")
        tot_new += int(st.n_new); tot_dup += int(st.n_dup); tot_pass += int(st.by_status[0])
        tot_bytes += int(st.payload_bytes) + ALG_BYTES_FIXED * n + ALG_BYTES_PROBE * int(st.by_status[0])
        first += n_wave
        waves += 1
    dumped = None
    if args.dump_outputs and rank == 0:      # the last wave: its records and NEW list; the sets' counts after it
        dumped = dump_outputs(args.dump_outputs, torch, np, dev, n, d_rec, d_new, int(st.n_new), eng.issuer_counts(), st)
    wb_out = None
    if wbs is not None:
        t0 = time.perf_counter()
        wbs.finish()
        t_gpu += time.perf_counter() - t0
        wb_out = wbs.report(time.perf_counter() - t_wall0, t_gpu)
        ok = ok and wb_out["ok"]
    total_count = eng.total_count()
    if group is not None:
        # the slowest rank's time; the sums over the ranks; every rank must have matched the generator in every wave
        t_gpu = float(group.all_reduce_u64([int(t_gpu * 1e9)], op_max=True)[0]) * 1e-9
        tot_new, tot_dup, tot_pass, bad_entries, not_ok, total_count = (int(v) for v in group.all_reduce_u64(
            [tot_new, tot_dup, tot_pass, bad_entries, 0 if ok else 1, total_count]))
        ok = not_ok == 0
    ok = ok and total_count == tot_new and bad_entries == 0
    achieved = tot_bytes / (t_map * 1e-3) / 1e9
    # measured HBM traffic of the map kernel in this mode: a 40 M-entry stream in 4 waves of 10 M under rocprofv3 --pmc
    # (the table persists across the waves, as here; bytes per entry averaged over the launches) — with --full
    traffic_info = traffic_err = None
    if args.full and world == 1 and args.traffic == "auto" and not wb and not os.environ.get("CTMR_BENCH_CHILD"):
        kname = MAP_KERNELS[args.variant or DEFAULT_VARIANT].split("<")[0]
        traffic_info, traffic_err = measure_traffic(args, 10_000_000, [kname], ["--stream", "40000000"])
    out = {"metric": "certificates/sec whole-node + achieved HBM GB/s, 100M-entry synthetic CT batch",
           "value": T / t_gpu, "unit": "certificates/sec", "n_gpus": world, "steps": waves, "warmup": 0,
           "ms_per_step": t_gpu / waves * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
           "dtype": "u8", "data": "synthetic",
           "config": {"workload": f"STREAM of {T} entries with 10% duplicates in {waves} waves of {W}"
                                  + (" through one known-certificate table (BASELINE configs[4] on one GPU)" if world == 1 else
                                     f", every wave split by log-index range over {world} GPUs, sets persisting on the ranks "
                                     "(BASELINE configs[4])") + "; generation untimed",
                      "dedup": mode, "table_slots_per_rank": int(slots), "map_variant": args.variant or DEFAULT_VARIANT},
           "roofline": {"bound": "hbm", "kernel": map_kernel_name(args).split("<")[0] if world > 1 else
                        map_kernel_name(args), "achieved": achieved,
                        "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS, "traffic": None,
                        "achieved_basis": "ALGORITHMIC bytes of rank 0 / its map kernel time",
                        "achieved_algorithmic": achieved, "frac_algorithmic": achieved / HBM_PEAK_GBPS,
                        "alg_bytes_formula": "sum(L_i) + 45*E + 64*PASS (table probe), summed over the waves"},
           "result": {"n_new": tot_new, "n_dup": tot_dup, "n_pass": tot_pass, "total_count": total_count,
                      "entries_disagreeing_with_generator": bad_entries,
                      "duplicate_structure_matches_generator_in_every_wave": bool(ok)}}
    if dumped is not None:
        out["dump_outputs"] = dumped
    if group is not None:
        out["exchange"] = {"mode": mode, "transport": "rccl", "wire_bytes_sent_by_rank0_over_the_stream": wire}
    if wb_out is not None:
        out["write_back"] = wb_out
        out["config"]["workload"] += (f"; WITH storage.Backend write-back ({wb}): IssuerMetadata first sightings, PEM of every new "
                                      "certificate on the GPU, " + ("storage.NoopBackend" if wb == "noop" else
                                      "storage.LocalDiskBackend through pinned host buffers and the native host writer") +
                                      " — `value` counts the whole of it")
    if traffic_info:
        r = out["roofline"]
        r["traffic"] = traffic_info["traffic_bytes_per_cert"] * T          # over the whole stream
        r["traffic_measurement"] = traffic_info
        r["achieved_physical"] = r["traffic"] / (t_map * 1e-3) / 1e9
        r["frac_physical"] = r["achieved_physical"] / HBM_PEAK_GBPS
        if r["achieved_physical"] < r["achieved_algorithmic"]:   # the smaller of the two byte counts is priced (see the plain line)
            r["achieved"], r["frac"] = r["achieved_physical"], r["frac_physical"]
            r["achieved_basis"] = "measured HBM traffic (FETCH_SIZE x2 + WRITE_SIZE, 40 M-entry stream of the same corpus) / map kernel time"
    elif traffic_err:
        out["roofline"]["traffic_error"] = traffic_err
    if rank == 0:
        print(json.dumps(out))
    if group is not None:
        group.close()
    eng.close()


def oracle_sample_check(np, torch, ctmr, synth, N, cfg, dup_permille, issuers, filt, now, dev, base, E, d_off, d_pay, d_iss,
                        d_et, d_rec, slices, per, profile="reference"):
    """The oracle-checked sample of ONE rank's shard = the one-core cpu_baseline leg: `slices` equally spaced slices of
    the shard, copied back from HBM, plus — generated on the host, byte-identical to the device generator
    (tests/test_gpu_parity.py) — every entry outside them whose key a sampled duplicate repeats, WHEREVER in the log it
    lies (mostly in other ranks' shards when the batch is split), all in log order.  The generator repeats keys of
    NON-duplicate entries only (csrc/synth.h synth_src), so the oracle's WasUnknown over this closed set is the whole
    batch's answer for every entry in it (tests/test_bench_helpers_cpu.py) — provided the dedup is global."""
    ranges = strided_sample(E, slices, per)
    per = ranges[0][1] - ranges[0][0]
    in_sample = np.concatenate([np.arange(base + lo, base + hi, dtype=np.uint64) for lo, hi in ranges])
    src, isdup = synth_src(cfg.seed, in_sample, dup_permille, np)
    extra = np.setdiff1d(src[isdup], in_sample)
    extra_certs = [synth.leaf(cfg, int(i)) for i in extra]
    arrays = gather_sample(d_off, d_pay, d_iss, d_et, ranges, extra, extra_certs, N.PAYLOAD_PAD, np, base=base)
    sample = len(arrays[4])
    cpu, (ost, ounk) = cpu_baseline(arrays[:3], issuers, filt, now, sample, arrays[3], profile)
    cpu["sample"] = (f"{slices} equally spaced slices of {per} entries of the same synthetic batch, copied back from HBM, + the "
                     f"{len(extra)} entries outside them whose keys sampled duplicates repeat; " + cpu["sample"])
    mine = (arrays[4] >= base) & (arrays[4] < base + E)            # the rest are sources that live in other shards
    gidx = torch.from_numpy((arrays[4][mine] - np.uint64(base)).astype(np.int64)).to(dev)
    rec = d_rec.view(-1, 32)[gidx].cpu().numpy().reshape(-1).view(ctmr.engine.RECORD_DTYPE)
    gnew = (rec["flags"] & 2) != 0
    ost_m, ounk_m = ost[mine], ounk[mine]
    info = {"entries": int(sample), "entries_of_this_shard": int(mine.sum()), "slices": slices, "entries_per_slice": per,
            "sources_outside_the_slices": int(len(extra)),
            "pass": int((ost_m == 0).sum()), "was_unknown": int((ounk_m != 0).sum()),
            "known_duplicates": int(((ost_m == 0) & (ounk_m == 0)).sum()),
            "status_mismatches": int((rec["status"] != ost_m).sum()),
            "was_unknown_mismatches": int((gnew != (ounk_m != 0)).sum())}
    return cpu, info, arrays, ranges


# per-entry arrays of --dump-outputs: this many records, 116 B each as written (sample_index 8, status / flags / serial_len
# 3 x 4, exp_hour and issuer_idx 2 x 8, serial 20 x 4; 124 B with the raw mode's timestamps), and as many NEW entries,
# 16 B each (new_pos, new_idx): ≈37 MB at most
DUMP_SAMPLE = 1 << 18
DUMP_SEED = 20260921


def dump_outputs(outdir, torch, np, dev, E, d_rec, d_new, n_new, counts, stats, timestamps=None):
    """--dump-outputs DIR: what the timed path handed its caller in its last step, as float32 / float64 .npy files
    (under 40 MB).  The per-entry record fields and the NEW list are a fixed, seeded sample when they are longer than
    DUMP_SAMPLE; records_digest.npy and new_digest.npy are sums over ALL records and the WHOLE NEW list, so two
    builds that differ anywhere outside the sample still differ there."""
    from ct_mapreduce_amd.engine import RECORD_DTYPE
    os.makedirs(outdir, exist_ok=True)
    rng = np.random.default_rng(DUMP_SEED)
    idx = np.arange(E) if E <= DUMP_SAMPLE else np.sort(rng.choice(E, DUMP_SAMPLE, replace=False))
    recs = d_rec.view(-1, 32)[:E]
    rec = recs[torch.from_numpy(idx).to(dev)].cpu().numpy().reshape(-1).view(RECORD_DTYPE)
    out = {"sample_index": idx.astype(np.float64),
           "status": rec["status"].astype(np.float32), "flags": rec["flags"].astype(np.float32),
           "serial_len": rec["serial_len"].astype(np.float32), "exp_hour": rec["exp_hour"].astype(np.float64),
           "issuer_idx": rec["issuer_idx"].astype(np.float64), "serial": rec["serial"].astype(np.float32)}
    if timestamps is not None:
        out["timestamp"] = timestamps[:E][torch.from_numpy(idx).to(dev)].cpu().numpy().astype(np.float64)
    # digest of every record: per byte column, the plain sum and the sum weighted by (i mod 65521) + 1
    dig = torch.zeros(2, 32, dtype=torch.int64, device=dev)
    for lo in range(0, E, 1 << 20):
        c = recs[lo:lo + (1 << 20)].to(torch.int64)
        w = torch.arange(lo, lo + c.shape[0], dtype=torch.int64, device=dev) % 65521 + 1
        dig[0] += c.sum(0)
        dig[1] += (c * w[:, None]).sum(0)
    out["records_digest"] = dig.cpu().numpy().astype(np.float64)
    new = d_new[:n_new]
    pos = np.arange(n_new) if n_new <= DUMP_SAMPLE else np.sort(rng.choice(n_new, DUMP_SAMPLE, replace=False))
    out["new_pos"] = pos.astype(np.float64)
    out["new_idx"] = new[torch.from_numpy(pos).to(dev)].cpu().numpy().astype(np.float64)
    out["new_digest"] = np.array([n_new, int(new.sum().item()) if n_new else 0,
                                  int((new % 65521).sum().item()) if n_new else 0], np.float64)
    out["issuer_counts"] = np.asarray(counts, np.uint64).astype(np.float64)
    out["stats"] = np.array([int(stats.n), int(stats.n_new), int(stats.n_dup), int(stats.n_host_set)]
                            + [int(x) for x in stats.by_status], np.float64)
    for name, a in out.items():
        np.save(os.path.join(outdir, name + ".npy"), a)
    return {"dir": outdir, "files": sorted(n + ".npy" for n in out), "records_sampled": int(len(idx)),
            "bytes": int(sum(a.nbytes for a in out.values()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--total-entries", type=int, default=0,
                    help="ONE batch of this many entries split over the GPUs by log-index range (strong scaling; BASELINE "
                         "configs[3]).  Default: BASELINE's 100M-entry batch (≈152 GB of DER; halved automatically if a "
                         "shard does not fit its GPU)")
    ap.add_argument("--entries", type=int, default=0,
                    help="entries PER GPU instead (weak scaling); at --gpus 1 the same thing as --total-entries")
    ap.add_argument("--dedup", default="auto", choices=["auto", "bloom", "owner", "local"],
                    help="N > 1: how the known-certificate sets of the ranks relate.  bloom (auto): global, exact — all-gather "
                         "of per-GPU Bloom filters as a pre-filter + exact lookups; owner: global, exact — owner-computes key "
                         "exchange; local: per-shard sets (NOT the reference's one set: duplicates across shards are counted "
                         "twice — the line says so)")
    ap.add_argument("--chunks", type=int, default=1,
                    help="N > 1, --dedup owner: every shard is mapped in this many chunks, chunk c's key records travelling on a "
                         "second stream while chunk c + 1 is walked (ctmr_group_set_chunks); same results")
    ap.add_argument("--issuers", type=int, default=256)
    ap.add_argument("--table-slots-log2", type=int, default=0,
                    help="known-certificate table size (default: the power of two >= 2 x entries: load 0.35-0.47 when full)")
    ap.add_argument("--variant", type=int, default=0)
    ap.add_argument("--certs-per-tile", type=int, default=0)
    ap.add_argument("--lds-bytes", type=int, default=0)
    ap.add_argument("--cpu-sample", type=int, default=6_000_000)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="host threads of the all-core cpu_baseline leg (0 = the CPUs this process may use at once: the "
                         "cgroup quota if there is one, else the affinity mask; 1 = only the one-core leg)")
    ap.add_argument("--cpu-sample-mt", type=int, default=0,
                    help="entries of the all-core leg (default ≈400 k per thread, at most 16 M)")
    ap.add_argument("--meta", action="store_true",
                    help="also run the IssuerMetadata memo kernel (k_meta_new, SURVEY §8(f) N3) over the NEW list of "
                         "every step (engine created with collect_meta) and report its time")
    ap.add_argument("--fingerprint", action="store_true",
                    help="also time the auxiliary whole-certificate SHA-256 kernel (k_fingerprint; VALU-bound, not on "
                         "the reference's path) over the batch")
    ap.add_argument("--stream", type=int, default=0, metavar="TOTAL",
                    help="BASELINE configs[4]: stream TOTAL entries with 10%% duplicates in waves of --entries (default 50M, over "
                         "all ranks), the known-certificate sets persisting across waves; with --gpus N every wave is split by "
                         "log index over the ranks and deduplicated through the group (--dedup, default owner); checks every "
                         "wave and every entry's WasUnknown against the generator's duplicate structure")
    ap.add_argument("--write-back", choices=["noop", "disk"], default=None,
                    help="with --stream: BASELINE configs[4] WHOLE — per wave, behind the map/reduce: IssuerMetadata first "
                         "sightings (k_meta_new), PEM of the NEW list on the GPU (k_pem_encode) and the storage backend: "
                         "noop = storage.NoopBackend (certPath unset: the PEM bytes are produced and dropped, nothing leaves "
                         "the GPU), disk = storage.LocalDiskBackend on --write-back-dir (default: a fresh directory under "
                         "/dev/shm or $TMPDIR) fed through pinned host buffers by the native host writer, double-buffered so "
                         "that wave k's files are written while wave k+1 is mapped; wave 0's files are compared with the oracle")
    ap.add_argument("--write-back-dir", default=None)
    ap.add_argument("--write-back-threads", type=int, default=0, help="host writer threads (default: the cores, at most 32)")
    ap.add_argument("--mixed", action="store_true",
                    help="the mixed synthetic corpus (half EC P-256 keys, 40%% OV-like subjects of 120-260 bytes, longer "
                         "issuer names, one GeneralizedTime in four) instead of the SURVEY §8(d) corpus: how the map "
                         "behaves when the lanes of a wave do not walk identical layouts.  A --full run reports it as "
                         "secondary.mixed; this flag makes it the line's workload")
    ap.add_argument("--no-secondary", action="store_true", help="skip the secondary legs (mixed corpus, 128-byte aligned layout, fast profile, raw entries) of a --full run")
    ap.add_argument("--profile", choices=("fast", "reference"), default="reference",
                    help="ctmr_set_profile: 'reference' (the engine's default and the headline) = strict_spki + strict_leaf + "
                         "strict_strings + strict_extensions — what the reference's x509.ParseCertificate decides, as far as it can be "
                         "known here (DESIGN.md §3.1); 'fast' = strict_spki only, for a host that has parsed already.  A --full "
                         "run reports it as secondary.fast_profile")
    ap.add_argument("--strict-extensions", action="store_true",
                    help="ctmr_set_strict_extensions(1) alone: the extension bodies Go parses (what it costs on top of the default walk)")
    ap.add_argument("--strict-strings", action="store_true",
                    help="ctmr_set_strict_strings(1): the opt-in character-set check of the Names' string values, inside the walk (what it costs: ms_per_step "
                         "and kernel_ms.map of this line against the default line)")
    ap.add_argument("--no-strict-spki", action="store_true",
                    help="ctmr_set_strict_spki(0): skip the public key by length as rounds 1-3 did (the A/B of what parsing the "
                         "key — parsePublicKey, on by default like in the reference — costs the map kernel)")
    ap.add_argument("--aligned", type=int, default=0, metavar="BYTES",
                    help="lay every certificate at a multiple of BYTES (an entry view instead of the packed layout; payload grows "
                         "by the padding): what the map moves per certificate depends on where certificates start inside "
                         "128-byte lines.  A --full run reports --aligned 128 as secondary.aligned128")
    ap.add_argument("--pem", action="store_true",
                    help="also time the PEM write-back kernels (k_pem_len + scan + k_pem_encode, SURVEY §8(f) N1) over "
                         "the first 16M entries of the NEW list")
    ap.add_argument("--global-dedup", nargs="?", const="owner", default=None, choices=["owner", "bloom"],
                    help="BASELINE config 5's corpus (10%% duplicates, anywhere earlier in the stream) through the group "
                         "layer's exact modes even at N = 1, where there is no peer and the line prices what each mode "
                         "costs a rank on top of the plain reduce (phase times and bytes handed to the transport in "
                         "`exchange`).  At N > 1 the same as --dedup owner|bloom with that corpus")
    ap.add_argument("--raw", action="store_true",
                    help="feed raw get-entries blobs (leaf_input ‖ extra_data, ≈3.06 KB per entry): adds the "
                         "LogEntryFromLeaf decode and the Chain[0] → issuer match in front of the map (SURVEY §8(f) N2); "
                         "not the default workload")
    ap.add_argument("--trusted-chain", action="store_true",
                    help="with --raw: CTMR_CHAIN0_TRUSTED_LOG — a registered Chain[0] certificate is compared bytewise on its "
                         "first sighting per call and identified by length + first/last 16 bytes afterwards "
                         "(include/ctmr.h); the default compares every byte of every entry's Chain[0]")
    ap.add_argument("--traffic", default="auto", choices=["auto", "off"],
                    help="auto (default; with --full, N=1 only): after the timed steps re-execute this script on --traffic-entries "
                         "entries of the same corpus and mode under `rocprofv3 --pmc FETCH_SIZE` and `--pmc WRITE_SIZE` "
                         "(separate passes) and report the measured HBM traffic of the line's kernels; off: roofline.traffic = null")
    ap.add_argument("--traffic-entries", type=int, default=10_000_000)
    ap.add_argument("--traffic-file", default=None,
                    help="use this earlier measurement (the JSON this script writes to gpurun_out/traffic_map.json) instead "
                         "of measuring; refused unless it was taken on the same build of libctmr.so")
    ap.add_argument("--dup-permille", type=int, default=20,
                    help="entries that repeat an earlier entry's (issuer, serial, notAfter) — anywhere earlier in the "
                         "batch — so that the DEFER / duplicate paths of the insert run at headline scale (default 2 %%)")
    ap.add_argument("--sample-slices", type=int, default=60,
                    help="the oracle-checked sample (= the one-core cpu_baseline leg) is this many equally spaced slices "
                         "of every rank's shard …")
    ap.add_argument("--sample-per-slice", type=int, default=0,
                    help="… of this many entries each (default: --cpu-sample / ranks / --sample-slices), plus every entry "
                         "outside the slices whose key a sampled duplicate repeats")
    ap.add_argument("--full", action="store_true",
                    help="besides the timed steps, everything else the line measures and checks: the PMC traffic passes "
                         "(--traffic), the checks against the generator, the oracle-checked sample and the CPU baseline legs "
                         "(--no-cpu), the bytes the walk needs and the secondary legs (--no-secondary).  Without it a run "
                         "sets up, warms up, times the steps, writes --dump-outputs and prints the line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step computed (rank 0's records, NEW list, "
                         "per-issuer counts and stats; a fixed seeded sample of the per-entry arrays plus digests over all "
                         "of them) as DIR/<name>.npy in float32/float64, under 40 MB: same arguments, same inputs, so two "
                         "builds can be compared output for output")
    args = ap.parse_args()

    if args.stream and (args.raw or args.global_dedup or args.meta or args.pem or args.fingerprint):
        ap.error("--stream runs the plain map/reduce (with --gpus N: through the group); --write-back adds metadata + PEM + backend")
    if args.write_back and not args.stream:
        ap.error("--write-back belongs to --stream")
    if args.aligned and (args.raw or args.global_dedup or args.gpus > 1 or args.stream or args.pem or args.fingerprint or args.meta):
        ap.error("--aligned is a layout variant of the plain one-GPU line")
    if args.aligned & (args.aligned - 1):
        ap.error("--aligned takes a power of two")

    # ---- N > 1 without a launcher: become the launcher
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))

    import numpy as np
    import torch
    import ct_mapreduce_amd as ctmr
    from ct_mapreduce_amd import synth, _native as N
    from ct_mapreduce_amd.distributed import Group, shard as make_shard, shard_range

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    local %= max(torch.cuda.device_count(), 1)      # (the tests let several ranks share the one reachable GPU)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # placement experiment (EXPERIMENTS.md, "run-to-run spread"): an allocation of this many KiB made — and kept — before
    # everything else shifts where the batch, the index and the arena come to lie
    _pad = torch.empty(int(os.environ.get("CTMR_BENCH_PAD_KIB", "0")) << 10, dtype=torch.uint8, device=dev) \
        if os.environ.get("CTMR_BENCH_PAD_KIB") else None
    gid = None
    if world > 1:
        # CONTROL path: the 128-byte group id reaches the ranks through the environment (spawned by this script) or by
        # one broadcast over the launcher's rendezvous.  Everything on the data path — shard maps, key exchange, Bloom
        # all-gather, the all-reduce of the per-issuer counts, the barriers and the max-over-ranks of the step time —
        # goes through the library's own RCCL group (ctmr_group_*, csrc/engine/group.inc).
        gid = bytes.fromhex(os.environ["CTMR_GROUP_ID"]) if os.environ.get("CTMR_GROUP_ID") else \
            group_id_from_launcher(rank, Group.unique_id)

    filt = b"Synth Issuer 0,Synth Issuer 1"      # BASELINE config 3: passes issuers 000-199
    # the --global-dedup lines run BASELINE config 5's corpus: 10 % of the entries repeat an earlier entry's key —
    # anywhere earlier in the stream, i.e. usually in another rank's shard
    dup_permille = 100 if args.global_dedup else args.dup_permille
    mode = args.global_dedup or (args.dedup if args.dedup != "auto" else ("bloom" if world > 1 else "plain"))
    if world == 1 and not args.global_dedup and args.dedup in ("auto", "local"):
        mode = "plain"                            # one rank: its own set IS the global set — no group layer in the way
    cfg = synth.config(seed=20260921 + 4, n_issuers=args.issuers, zipf=1, dup_permille=dup_permille,
                       ca_permille=10, expired_permille=10, profile=1 if args.mixed else 0)
    now = synth.BASE_TIME
    issuers = synth.issuers(cfg)

    if args.stream:
        return run_stream(args, ctmr, synth, N, torch, np, dev, local, rank, world, cfg, filt, now, issuers, gid)

    # ---- the workload: one batch split by log index (strong), or E entries per GPU (weak)
    env_total = int(os.environ.get("CTMR_BENCH_ENTRIES", 0))
    weak = args.entries > 0 and world > 1
    total = (args.entries * world) if args.entries else (args.total_entries or env_total or 100_000_000)
    if args.raw and not (args.entries or args.total_entries or env_total):
        total = 40_000_000          # ≈122 GB of raw entries + the table

    raw_view = {}

    def make_engine(E, this_cfg):
        """The engine and its known-certificate table — the one allocation every rank can always make; the group is
        created on it BEFORE the batch is generated, so that a rank whose shard does not fit can still tell the others."""
        # index slots: 4 per entry (load ≤ 0.25 at 8 bytes a slot — 4 GB for the 100 M batch; rounds 1–3 sized their 64-byte
        # slots 2 per entry).  Same-box sweep, round 4: 2^27 / 2^28 / 2^29 slots → map 24.9 / 22.3 / 21.6 ms per 100 M.
        eng = ctmr.Engine(device=local, table_slots=(1 << args.table_slots_log2) if args.table_slots_log2 else pow2_at_least(int(E * 4)),
                          pair_slots=1 << 22, map_variant=args.variant, certs_per_tile=args.certs_per_tile,
                          lds_tile_bytes=args.lds_bytes, profile=True, collect_meta=args.meta)
        eng.set_filter(filt, False, now)
        eng.set_profile(args.profile)          # "reference" is also what ctmr_create gives (ABI v7); said explicitly here
        if args.strict_strings:
            eng.set_strict_strings(True)
        if args.strict_extensions:
            eng.set_strict_extensions(True)
        if args.no_strict_spki:
            eng.set_strict_spki(False)
        if not args.raw or world > 1:
            # raw entries register their Chain[0] certificates themselves — in shard order, so issuer index k would name
            # different issuers on different ranks and the count all-reduce would add apples to oranges: with several
            # ranks, register the same list up front
            eng.add_issuers(synth.issuers(this_cfg))
        return eng

    def fill_raw(eng, first, E, this_cfg):
        d_bounds = torch.empty(2 * E + 1, dtype=torch.int64, device=dev)
        nbytes = eng.synth_entries_device(this_cfg, first, E, d_bounds.data_ptr(), 0, 0)
        d_blob = torch.empty(nbytes + N.PAYLOAD_PAD + 16, dtype=torch.uint8, device=dev)
        eng.synth_entries_device(this_cfg, first, E, d_bounds.data_ptr(), d_blob.data_ptr(), d_blob.numel())
        d_rec = torch.empty(E * 32, dtype=torch.uint8, device=dev)
        d_new = torch.empty(E, dtype=torch.int64, device=dev)
        d_ts = torch.empty(E, dtype=torch.int64, device=dev)
        # caller-owned entry view: the decode fills it, map / meta / PEM read certificates through it
        raw_view["start"] = torch.empty(E, dtype=torch.int64, device=dev)
        raw_view["end"] = torch.empty(E, dtype=torch.int64, device=dev)
        raw_view["iss"] = torch.empty(E, dtype=torch.int32, device=dev)
        raw_view["et"] = torch.empty(E, dtype=torch.uint8, device=dev)
        raw_view["c0len"] = torch.empty(E, dtype=torch.int32, device=dev)
        raw_view["c0start"] = torch.empty(E, dtype=torch.int64, device=dev)
        raw_view["view"] = N.EntryView(cert_start=raw_view["start"].data_ptr(), cert_end=raw_view["end"].data_ptr(),
                                       issuer_idx=raw_view["iss"].data_ptr(), entry_type=raw_view["et"].data_ptr(),
                                       timestamp=d_ts.data_ptr(), chain0_start=raw_view["c0start"].data_ptr(),
                                       chain0_len=raw_view["c0len"].data_ptr())
        raw_view["blob_bytes"] = nbytes
        torch.cuda.synchronize()
        return d_bounds, d_blob, d_ts, None, d_rec, d_new

    def fill(eng, first, E, this_cfg):
        if args.raw:
            return fill_raw(eng, first, E, this_cfg)
        if args.aligned:
            return fill_aligned(eng, first, E, this_cfg, args.aligned)
        # ---- synthetic shard [first, first + E), generated directly in HBM
        d_off = torch.empty(E + 1, dtype=torch.int64, device=dev)
        nbytes = eng.synth_device(this_cfg, first, E, d_off.data_ptr(), 0, 0, 0, 0)
        d_pay = torch.empty(nbytes + N.PAYLOAD_PAD + 16, dtype=torch.uint8, device=dev)
        d_iss = torch.empty(E, dtype=torch.int32, device=dev)
        d_et = torch.empty(E, dtype=torch.uint8, device=dev)
        eng.synth_device(this_cfg, first, E, d_off.data_ptr(), d_pay.data_ptr(), d_pay.numel(),
                         d_iss.data_ptr(), d_et.data_ptr())
        d_rec = torch.empty(E * 32, dtype=torch.uint8, device=dev)
        d_new = torch.empty(E, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        return d_off, d_pay, d_iss, d_et, d_rec, d_new

    def fill_aligned(eng, first, E, this_cfg, align):
        """The same certificates as an entry view, each starting at a multiple of `align` bytes."""
        d_off = torch.empty(E + 1, dtype=torch.int64, device=dev)
        d_end = torch.empty(E, dtype=torch.int64, device=dev)
        nbytes = eng.synth_view_device(this_cfg, first, E, align, d_off.data_ptr(), d_end.data_ptr(), 0, 0, 0, 0)
        d_pay = torch.empty(nbytes + N.PAYLOAD_PAD + 16, dtype=torch.uint8, device=dev)
        d_iss = torch.empty(E, dtype=torch.int32, device=dev)
        d_et = torch.empty(E, dtype=torch.uint8, device=dev)
        eng.synth_view_device(this_cfg, first, E, align, d_off.data_ptr(), d_end.data_ptr(), d_pay.data_ptr(), d_pay.numel(),
                              d_iss.data_ptr(), d_et.data_ptr())
        d_rec = torch.empty(E * 32, dtype=torch.uint8, device=dev)
        d_new = torch.empty(E, dtype=torch.int64, device=dev)
        raw_view["aligned"] = (d_end, nbytes, N.EntryView(cert_start=d_off.data_ptr(), cert_end=d_end.data_ptr(),
                                                          issuer_idx=d_iss.data_ptr(), entry_type=d_et.data_ptr(),
                                                          timestamp=None, chain0_start=None, chain0_len=None))
        torch.cuda.synchronize()
        return d_off, d_pay, d_iss, d_et, d_rec, d_new

    def setup(first, E, this_cfg):
        eng = make_engine(E, this_cfg)
        try:
            return (eng,) + fill(eng, first, E, this_cfg)
        except (ctmr.CtmrError, RuntimeError):
            eng.close()
            raise

    t_gen = time.perf_counter()
    group = None

    def my_shard():
        return (rank * args.entries, (rank + 1) * args.entries) if weak else shard_range(total, rank, world)

    first, hi = my_shard()
    E = hi - first
    if world > 1:
        eng = make_engine(E, cfg)
        group = Group.rccl(eng, gid, rank, world)       # every rank joins before any of them can run out of memory
        if args.chunks > 1:
            group.set_chunks(args.chunks)
    while True:
        first, hi = my_shard()
        E = hi - first
        fits = 1
        try:
            if world > 1:
                d_off, d_pay, d_iss, d_et, d_rec, d_new = fill(eng, first, E, cfg)
            else:
                eng, d_off, d_pay, d_iss, d_et, d_rec, d_new = setup(first, E, cfg)
        except (ctmr.CtmrError, RuntimeError) as ex:   # does not fit in this GPU's HBM
            fits = 0
            sys.stderr.write(f"bench: rank {rank}: {E} entries do not fit ({ex})\n")
            d_off = d_pay = d_iss = d_et = d_rec = d_new = None
            raw_view.clear()
            torch.cuda.empty_cache()
        if world > 1:
            fits = int(int(group.all_reduce_u64([0 if fits else 1])[0]) == 0)      # the ranks halve together or not at all
        if fits:
            break
        if total <= 1_000_000:
            raise SystemExit("bench: even 1 M entries do not fit")
        d_off = d_pay = d_iss = d_et = d_rec = d_new = None
        raw_view.clear()
        torch.cuda.empty_cache()
        total //= 2
        if weak:
            args.entries //= 2
        sys.stderr.write(f"bench: trying {total} entries\n")
    t_gen = time.perf_counter() - t_gen
    if args.raw and args.trusted_chain:
        eng.set_chain0_match(N.CHAIN0_TRUSTED_LOG)
    if world == 1 and mode != "plain":
        group = Group.local([eng])          # N = 1: no peer — this prices each mode's kernels on one rank
    if mode == "bloom":
        per_rank = max(E, (total + world - 1) // world)
        bits_per_key = int(os.environ.get("CTMR_BLOOM_BITS_PER_KEY", 16))
        group.bloom_config(pow2_at_least(bits_per_key * per_rank))   # ≈16 filter bits per key held; same size on every rank
    global_counts = [None]
    dstats = []
    meta_ms, meta_items = [], []
    d_items = torch.empty(32 * (1 << 22), dtype=torch.uint8, device=dev) if args.meta else None
    phase_ms = np.zeros(8)
    wire = [0, 0, 0]

    def step():
        eng.reset_known()
        if args.raw:   # d_off = bounds, d_pay = blob, d_iss = timestamps
            ds = eng.decode_entries_device(d_pay.data_ptr(), d_off.data_ptr(), E, raw_view["view"])
            st = eng.map_view_device(d_pay.data_ptr(), raw_view["blob_bytes"], raw_view["view"], E, d_rec.data_ptr(),
                                     d_new.data_ptr())
            dstats.append(ds)
        elif group is not None:
            # one native call: this rank's shard map + (owner | Bloom) exchange over RCCL (nothing to exchange when N = 1)
            st = group.map_batch("local" if mode == "local" else mode,
                                 [make_shard(d_pay.data_ptr(), d_off.data_ptr(), d_iss.data_ptr(), d_et.data_ptr(), E,
                                             d_rec.data_ptr(), d_new.data_ptr(), order_base=first)])[0]
            gi = group.info()
            phase_ms[:] += np.array(list(gi.ms_phase))
            wire[0] += int(gi.wire_bytes_sent); wire[1] += int(gi.keys_sent); wire[2] += int(gi.filter_bytes_received)
        elif args.aligned:
            st = eng.map_view_device(d_pay.data_ptr(), raw_view["aligned"][1], raw_view["aligned"][2], E, d_rec.data_ptr(),
                                     d_new.data_ptr())
        else:
            st = eng.map_batch_device(d_pay.data_ptr(), d_off.data_ptr(), d_iss.data_ptr(), d_et.data_ptr(),
                                      E, d_rec.data_ptr(), d_new.data_ptr())
        if args.meta:
            t_m = time.perf_counter()
            offs_p = raw_view["start"].data_ptr() if args.raw else d_off.data_ptr()
            ends_p = raw_view["end"].data_ptr() if args.raw else 0
            meta_items.append(eng.meta_new_device(d_pay.data_ptr(), offs_p, ends_p, d_rec.data_ptr(),
                                                  d_new.data_ptr(), int(st.n_new), d_items.data_ptr(), 1 << 22))
            meta_ms.append((time.perf_counter() - t_m) * 1e3)
        if group is not None and world > 1:
            # per-issuer unique counts merged over xGMI: ncclAllReduce inside ctmr_group_issuer_counts (2 KiB)
            global_counts[0] = group.issuer_counts(len(issuers))
        return st

    def barrier():
        if group is not None and world > 1:
            group.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    phase_ms[:] = 0
    wire[:] = [0, 0, 0]
    ms_map = []
    stats = None
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        stats = step()
        ms_map.append(stats.ms_map)
    barrier()
    dt = time.perf_counter() - t0
    if group is not None and world > 1:
        dt = float(group.all_reduce_u64([int(dt * 1e9)], op_max=True)[0]) * 1e-9      # the slowest rank's time
    if world == 1:
        global_counts[0] = eng.issuer_counts()[:len(issuers)]
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, torch, np, dev, E, d_rec, d_new, int(stats.n_new), global_counts[0], stats,
                              timestamps=d_iss if args.raw else None)

    # ---- with --full the run checks itself, at every N ------------------------------------------------------------
    # (a) every entry's WasUnknown and Σ NEW against the generator's duplicate structure: entry i repeats an EARLIER
    #     entry's key iff synth_is_dup(i), wherever in the log that earlier entry lies — so, with a global set, a rank's
    #     NEW entries are exactly its PASS ∧ ¬dup ones; (b) the all-reduced per-issuer vector against the same structure.
    checks = None
    if args.full and not args.raw:
        recs = d_rec.view(-1, 32)[:E]
        passed = recs[:, 0] == 0
        is_new = (recs[:, 1] & 2) != 0
        dupm = synth_is_dup_torch(cfg.seed, first, E, dup_permille, torch, dev)
        want_new = passed & ~dupm
        bad = int((is_new != want_new).sum().item()) + int(int(stats.n_new) != int(is_new.sum().item()))
        want_counts = torch.bincount(d_iss[:E][want_new].to(torch.int64), minlength=len(issuers))[:len(issuers)].cpu().numpy().astype(np.uint64)
        tot = np.concatenate([[bad, int(stats.n_new), int(want_new.sum().item())], want_counts]).astype(np.uint64)
        if world > 1:
            tot = group.all_reduce_u64(tot)
        checks = {"entries_disagreeing_with_generator": int(tot[0]), "n_new_all_ranks": int(tot[1]),
                  "n_new_expected_from_generator": int(tot[2]),
                  "per_issuer_counts_match_generator": bool((np.asarray(global_counts[0], np.uint64) == tot[3:]).all()),
                  "issuer_counts_all_ranks_sum": int(np.asarray(global_counts[0], np.uint64).sum())}

    # HBM traffic of the line's kernels per launch: PMC counters can only be collected under rocprofv3, in their own
    # passes — this script re-executes itself under the profiler on a smaller batch of the same corpus and mode (bytes
    # per entry do not depend on the batch size: every launch streams ≫ the 256 MB of on-die cache) and scales.
    traffic = traffic_info = traffic_err = None
    vname = map_kernel_name(args)
    kname = vname.split("<")[0]
    kernels = [kname] + (["k_decode_match"] if args.raw else []) + (["k_meta_new"] if args.meta else [])
    mode_args = (["--mixed"] if args.mixed else []) + (["--aligned", str(args.aligned)] if args.aligned else []) + (["--raw"] if args.raw else []) + (["--meta"] if args.meta else []) + \
                (["--trusted-chain"] if args.trusted_chain else []) + (["--global-dedup", args.global_dedup] if args.global_dedup else []) + \
                (["--strict-strings"] if args.strict_strings else []) + (["--no-strict-spki"] if args.no_strict_spki else []) + \
                ["--profile", args.profile] + (["--strict-extensions"] if args.strict_extensions else [])
    plain = not (args.raw or args.global_dedup or args.meta)
    if rank == 0 and world == 1 and not os.environ.get("CTMR_BENCH_CHILD"):
        if args.traffic_file and plain:
            try:
                t = json.load(open(args.traffic_file))
                if t.get("lib_sha256_16") == lib_hash() and "traffic_bytes_per_cert" in t:
                    traffic_info = dict(t, source=os.path.relpath(args.traffic_file, ROOT))
                else:
                    traffic_err = "traffic file refused: taken on another build of libctmr.so"
            except (ValueError, OSError) as ex:
                traffic_err = f"traffic file unreadable: {ex}"
        elif args.full and args.traffic == "auto":
            t_tr = time.perf_counter()
            traffic_info, traffic_err = measure_traffic(args, min(E, args.traffic_entries), kernels, mode_args)
            if traffic_info:
                traffic_info["source"] = "measured by this run (rocprofv3 --pmc, two passes)"
                traffic_info["seconds"] = round(time.perf_counter() - t_tr, 1)
                if plain and not args.mixed:
                    try:
                        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
                        json.dump(traffic_info, open(os.path.join(ROOT, "gpurun_out", "traffic_map.json"), "w"))
                    except OSError:
                        pass
        if traffic_info:
            traffic = traffic_info["traffic_bytes_per_cert"] * E

    n_total = total if not weak else args.entries * world
    value = n_total * args.steps / dt
    # ALGORITHMIC bytes of the map kernel: Σ L_i + 45·E (+ 64 per PASS entry for the fused probe).  Raw
    # mode: L_i is the certificate the map parses (cert_end − cert_start), not the blob — decode + match are priced below.
    if args.raw:
        cert_bytes = int((raw_view["end"] - raw_view["start"]).sum().item())
    elif args.aligned:
        cert_bytes = int((raw_view["aligned"][0] - d_off[:E]).sum().item())
    else:
        cert_bytes = int(stats.payload_bytes)
    alg_bytes = cert_bytes + ALG_BYTES_FIXED * E
    fused_variant = (args.variant or DEFAULT_VARIANT) in FUSED
    if fused_variant:
        alg_bytes += ALG_BYTES_PROBE * int(stats.by_status[0])
    avg_ms = sum(ms_map) / len(ms_map)
    achieved = alg_bytes / (avg_ms * 1e-3) / 1e9
    shard_note = (f"{n_total} entries in one batch on one GPU" if world == 1 else
                  f"{n_total} entries in ONE batch split by log-index range over {world} GPUs" if not weak
                  else f"{args.entries} entries per GPU x {world}")
    parallelism = {"plain": "1 GPU, one known-certificate set",
                   "local": f"log-index shards x{world}, PER-SHARD sets (NOT the reference's single set: a key that spans two shards "
                            "is counted on both) + per-issuer count all-reduce over RCCL",
                   "bloom": f"log-index shards x{world}, GLOBAL exact dedup: Bloom-filter all-gather pre-filter + exact lookups "
                            "+ per-issuer count all-reduce, over RCCL inside the library",
                   "owner": f"log-index shards x{world}, GLOBAL exact dedup: owner-computes key exchange (32-byte records) "
                            "+ per-issuer count all-reduce, over RCCL inside the library"}[mode]
    out = {
        "metric": "certificates/sec whole-node + achieved HBM GB/s, 100M-entry synthetic CT batch",
        "value": value, "unit": "certificates/sec", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
        "scaling": "weak" if weak else "strong", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
        "config": {"workload": f"{shard_note}: synthetic ~1.5 KB DER CT entries, {args.issuers} issuers (Zipf), "
                               f"{dup_permille / 10:g} % duplicates of earlier entries (anywhere in the log), "
                               "issuerCN prefix filter + known-certificate dedup + per-issuer unique counts "
                               "(BASELINE configs[2]/[3] shape)",
                   "total_entries": n_total, "entries_on_rank0": E, "mean_der_bytes": cert_bytes / E,
                   "dedup": mode, "parallelism": parallelism,
                   "map_variant": args.variant or DEFAULT_VARIANT,
                   **({"strict_strings": True} if args.strict_strings else {}),
                   **({"strict_extensions": True} if args.strict_extensions else {}),
                   "profile": args.profile,
                   **({"strict_spki": False} if args.no_strict_spki else {}),
                   "gen_seconds": round(t_gen, 2)},
        # roofline of the dominant kernel.  `achieved` / `frac` price the SMALLER of two byte counts: the SURVEY §8(d)
        # algorithmic bytes (every certificate byte "read once" + arrays + the table probe) and the HBM traffic the kernel was
        # measured to move (PMC counters).  Under the fast profile the walk skips key, SAN body and signature by length — the
        # algorithmic figure counts bytes that never move, and the physical one is the honest fraction; under the reference
        # profile the kernel moves MORE than the algorithmic bytes (sector-granular windows), and the algorithmic one is.
        # Both are always in the line: `frac_physical`, `frac_algorithmic`.
        "roofline": {"bound": "hbm", "kernel": vname if (mode == "plain" and not args.meta) else kname,
                     "achieved": (min(traffic, alg_bytes) if traffic else alg_bytes) / (avg_ms * 1e-3) / 1e9,
                     "achieved_basis": ("measured HBM traffic (FETCH_SIZE x2 + WRITE_SIZE) / avg launch time: less than the algorithmic bytes"
                                        if traffic < alg_bytes else
                                        "ALGORITHMIC bytes / avg launch time (the kernel moves more: traffic_over_algorithmic)") if traffic
                                       else "ALGORITHMIC bytes / avg launch time (no PMC measurement in this run"
                                            + (": " + traffic_err if traffic_err else "") + ")",
                     "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": (min(traffic, alg_bytes) if traffic else alg_bytes) / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS,
                     "achieved_physical": (traffic / (avg_ms * 1e-3) / 1e9) if traffic else None,
                     "frac_physical": (traffic / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS) if traffic else None,
                     "traffic": traffic, "traffic_measurement": traffic_info,
                     "traffic_over_algorithmic": (traffic / alg_bytes) if traffic else None,
                     "frac_of_streaming_ceiling": (traffic / (avg_ms * 1e-3) / 1e9 / 6290.0) if traffic else None,
                     "achieved_algorithmic": achieved, "frac_algorithmic": achieved / HBM_PEAK_GBPS,
                     "alg_bytes_per_launch": alg_bytes, "avg_launch_ms": avg_ms,
                     "launch_ms": [round(m, 3) for m in ms_map],
                     "alg_bytes_formula": "sum(L_i) + 45*E" + (" + 64*PASS (table probe)" if fused_variant else "")
                                          + (" with L_i = the certificate the map parses (not the blob)" if args.raw else "")},
        "kernel_ms": {"map": stats.ms_map, "insert": stats.ms_insert, "resolve": stats.ms_resolve,
                      "compact": stats.ms_compact, "total": stats.ms_total},
        "result": {"n_new": int(stats.n_new), "n_dup": int(stats.n_dup), "by_status": [int(x) for x in stats.by_status]},
    }
    if checks is not None:
        out["checks"] = checks
    if dumped is not None:
        out["dump_outputs"] = dumped
    if out["roofline"]["frac"] > 1.0 or out["roofline"]["frac_algorithmic"] > 1.0:
        out["roofline"]["invalid"] = "a fraction above 1 is a pricing error, not a result"
    if args.pem:
        m = min(int(stats.n_new), 16_000_000)
        d_po = torch.empty(m + 1, dtype=torch.int64, device=dev)

        def pem_call(d_pem_ptr, cap):
            if args.raw:
                return eng.pem_encode_view_device(d_pay.data_ptr(), raw_view["view"], d_new.data_ptr(), m, d_pem_ptr, cap,
                                                  d_po.data_ptr())
            return eng.pem_encode_device(d_pay.data_ptr(), d_off.data_ptr(), d_new.data_ptr(), m, d_pem_ptr, cap,
                                         d_po.data_ptr())
        pem_total = pem_call(0, 0)
        d_pem = torch.empty(pem_total + 64, dtype=torch.uint8, device=dev)
        t_p = []
        for _ in range(3):
            t0p = time.perf_counter()
            pem_call(d_pem.data_ptr(), pem_total + 64)
            t_p.append(time.perf_counter() - t0p)
        import base64
        po = d_po[:3].cpu().numpy()
        first_new = int(d_new[0].item())
        starts_t = raw_view["start"] if args.raw else d_off[:-1]
        ends_t = raw_view["end"] if args.raw else d_off[1:]
        der = d_pay[int(starts_t[first_new].item()):int(ends_t[first_new].item())].cpu().numpy().tobytes()
        b64 = base64.b64encode(der)                  # pem.EncodeToMemory: 64-column base64 between the two marker lines
        want = (b"-----BEGIN CERTIFICATE-----\n" + b"".join(b64[k:k + 64] + b"\n" for k in range(0, len(b64), 64)) +
                b"-----END CERTIFICATE-----\n")
        ok_pem = d_pem[int(po[0]):int(po[1])].cpu().numpy().tobytes() == want
        in_bytes = int((ends_t[d_new[:m]] - starts_t[d_new[:m]]).sum().item())
        out["pem"] = {"certificates": m, "pem_bytes": int(pem_total), "der_bytes": in_bytes, "ms_wall": min(t_p) * 1e3,
                      "certs_per_s": m / min(t_p), "GBps_read_plus_written": (in_bytes + pem_total) / min(t_p) / 1e9,
                      "first_block_matches_stdlib_base64": bool(ok_pem)}
    if group is not None:
        # what the exact mode costs on top of the map: wall time of the round's phases on rank 0 (each ends with the
        # stream drained) and what was handed to the transport for OTHER ranks, per step
        names = ["map_and_local_insert", "key_export_or_filter_gather_and_probe", "key_records_all_to_all",
                 "owner_insert_or_exact_lookup_and_resolve", "flags_all_to_all", "apply_and_compaction", "control_collectives"]
        gi = group.info()
        out["exchange"] = {"mode": mode, "transport": "rccl" if gi.transport else "local (one rank: nothing to exchange)",
                           "ms_phase_rank0": {nm: float(phase_ms[k]) / args.steps for k, nm in enumerate(names)},
                           "ms_control": float(phase_ms[6]) / args.steps,
                           "host_syncs_per_round": float(phase_ms[7]) / args.steps,
                           "wire_bytes_sent_by_rank0_per_step": wire[0] / args.steps,
                           "key_records_sent_by_rank0_per_step": wire[1] / args.steps,
                           "filter_bytes_received_by_rank0_per_step": wire[2] / args.steps,
                           "key_record_bytes": {"owner": 32, "bloom": 64}.get(mode)}
        if args.global_dedup:
            out["config"]["workload"] = out["config"]["workload"].replace(
                "(BASELINE configs[2]/[3] shape)", "(BASELINE configs[4] corpus, one round)")
    if args.fingerprint and not args.raw:
        d_dg = torch.empty(E * 32, dtype=torch.uint8, device=dev)
        fp_ms = [eng.fingerprint_device(d_pay.data_ptr(), d_off.data_ptr(), 0, E, d_dg.data_ptr()) for _ in range(3)]
        import hashlib
        okfp = True
        offs_h = d_off[:1001].cpu().numpy()
        pay_h = d_pay[: int(offs_h[-1])].cpu().numpy().tobytes()
        dg_h = d_dg[: 1000 * 32].cpu().numpy().tobytes()
        for k in range(1000):
            okfp = okfp and hashlib.sha256(pay_h[int(offs_h[k]):int(offs_h[k + 1])]).digest() == dg_h[32 * k:32 * k + 32]
        ms_fp = min(fp_ms)
        out["fingerprint"] = {"kernel": "k_fingerprint", "ms": ms_fp, "certs_per_s": E / (ms_fp * 1e-3),
                              "hashed_GBps": stats.payload_bytes / (ms_fp * 1e-3) / 1e9,
                              "bound": "valu", "blocks_per_s": (stats.payload_bytes / 64 + 1.5 * E) / (ms_fp * 1e-3),
                              "matches_hashlib_on_first_1000": bool(okfp),
                              "note": "auxiliary op, not on the reference's path (SURVEY D2); VALU roofline in DESIGN.md §5"}
    if args.aligned:
        out["config"]["workload"] = (f"ALIGNED layout (every certificate at a multiple of {args.aligned} bytes, an entry view; "
                                     f"{raw_view['aligned'][1] / E:.0f} B of payload per entry with the padding): " + out["config"]["workload"])
    if args.mixed:
        out["config"]["workload"] = "MIXED corpus (EC/RSA keys, OV-like subjects, GeneralizedTime): " + out["config"]["workload"]
    if args.meta and meta_ms:
        out["kernel_ms"]["meta_new_cold_wall"] = meta_ms[0]
        out["kernel_ms"]["meta_new_warm_wall"] = sum(meta_ms[1:]) / max(len(meta_ms) - 1, 1)
        out["meta"] = {"first_sightings_cold": meta_items[0], "first_sightings_warm": meta_items[-1],
                       "new_certificates": int(stats.n_new),
                       "note": "cold = first call (empty memo: every (issuer, expDate), DN and CRL DP is a first "
                               "sighting); warm = later steps (the known-certificate table is cleared every step, the "
                               "memo is not: every certificate is new again, nothing is a first sighting)"}
        if traffic_info and "k_meta_new" in traffic_info["kernels"]:
            tm = traffic_info["kernels"]["k_meta_new"]
            out["meta"]["k_meta_new_traffic_bytes_per_new_certificate"] = tm["traffic_bytes_per_cert"] * min(E, args.traffic_entries) / max(int(stats.n_new) * min(E, args.traffic_entries) / E, 1)
    if args.raw:
        ds = dstats[-1]
        c0_bytes = int(raw_view["c0len"].to(torch.int64).sum().item())
        # decode + match: bounds (16 B) and the leaf header (≈ 15 B) in, the view (37 B) out, and — exact mode — every
        # byte of every Chain[0]; trusted-log mode reads 32 of them
        dm_alg = (c0_bytes if not args.trusted_chain else 32 * E) + 68 * E
        dm_ms = ds.ms_match + ds.ms_decode
        out["config"]["workload"] = (f"{E} RAW get-entries (leaf_input+extra_data, {stats.payload_bytes / E:.0f} B/entry): "
                                     "LogEntryFromLeaf decode + Chain[0] issuer match + " + out["config"]["workload"])
        out["raw"] = {"blob_bytes": int(ds.blob_bytes), "ms_decode": ds.ms_decode, "ms_match": ds.ms_match,
                      "n_x509": int(ds.n_x509), "n_precert": int(ds.n_precert),
                      "issuers_registered_by_the_engine": eng.issuer_count(),
                      "chain0_match": "trusted-log (bytewise on first sighting per call, then length + first/last 16 B)"
                                      if args.trusted_chain else "exact (every byte of every Chain[0])",
                      "chain0_bytes": c0_bytes, "certificate_bytes_the_map_parses": cert_bytes,
                      "note": "decode and the first match round are one kernel (ms_match = both); ms_decode = strict_leaf's walk of the precertificate entries' leaf TBSCertificates (k_leaf_tbs_check; reference profile), else 0",
                      "parity_note": "the decode's oracle follows RFC 6962 3.4/4.6 and CT-go's struct tags; the reference holds "
                                     "no raw-entry fixture, so parity with CT-go's LogEntryFromLeaf is UNPINNED (DESIGN.md 3.2)"}
        rdm = {"bound": "hbm", "kernel": "k_decode_match", "alg_bytes_per_launch": dm_alg, "avg_launch_ms": dm_ms,
               "alg_bytes_formula": ("sum(chain0_len)" if not args.trusted_chain else "32*E") + " + 68*E (bounds 16 + leaf header 15 + view 37)",
               "achieved_algorithmic": dm_alg / (dm_ms * 1e-3) / 1e9, "frac_algorithmic": dm_alg / (dm_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS,
               "peak": HBM_PEAK_GBPS, "unit": "GB/s", "traffic": None}
        if traffic_info and "k_decode_match" in traffic_info["kernels"]:
            td = traffic_info["kernels"]["k_decode_match"]
            rdm["traffic"] = td["traffic_bytes_per_cert"] * E
            rdm["traffic_bytes_per_entry"] = td["traffic_bytes_per_cert"]
            rdm["achieved"] = rdm["traffic"] / (dm_ms * 1e-3) / 1e9
            rdm["frac"] = rdm["achieved"] / HBM_PEAK_GBPS
        out["roofline_decode_match"] = rdm
        out["kernel_ms"]["decode"] = ds.ms_decode
        out["kernel_ms"]["match"] = ds.ms_match

    # ---- with --full: oracle-checked sample of every rank's shard; the CPU baseline legs on rank 0 at N = 1
    if args.full and not args.no_cpu and not args.raw and not args.aligned:
        per_rank_sample = max(min(args.cpu_sample, total) // world, 1)
        per = args.sample_per_slice or max(1, min(per_rank_sample, E) // args.sample_slices)
        base_cpu, pinfo, arrays, ranges = oracle_sample_check(np, torch, ctmr, synth, N, cfg, dup_permille, issuers, filt, now, dev,
                                                              first, E, d_off, d_pay, d_iss, d_et, d_rec, args.sample_slices, per,
                                                              profile=args.profile)
        mism = np.array([pinfo["status_mismatches"], pinfo["was_unknown_mismatches"], pinfo["entries_of_this_shard"],
                         pinfo["known_duplicates"]], np.uint64)
        if world > 1:
            mism = group.all_reduce_u64(mism)
        out["parity_vs_oracle_on_sample"] = bool(mism[0] == 0 and mism[1] == 0)
        out["parity_sample"] = dict(pinfo, ranks=world, status_mismatches_all_ranks=int(mism[0]),
                                    was_unknown_mismatches_all_ranks=int(mism[1]), entries_checked_all_ranks=int(mism[2]),
                                    known_duplicates_all_ranks=int(mism[3]),
                                    note="rank 0's figures, then the sums over all ranks" if world > 1 else "")
        if mode == "local" and world > 1:
            out["parity_sample"]["note"] += "; per-shard sets: mismatches against the single-set oracle are expected"
        if rank == 0 and world == 1:
            out["cpu_baseline"] = base_cpu
            # what the walk must read of these certificates, against the measured traffic
            k = min(20000, per)
            offs_k = arrays[1][:k + 1]
            certs_k = [arrays[0][int(offs_k[i]):int(offs_k[i + 1])].tobytes() for i in range(k)]
            starts_k = d_off[ranges[0][0]:ranges[0][0] + k].cpu().numpy()
            try:
                nb, nl = needed_bytes_per_cert(certs_k, starts_k, filt, args.profile == "reference")
            except (OSError, subprocess.CalledProcessError) as ex:    # the host walk could not be built or loaded here
                nb = nl = None
                out["roofline"]["needed_error"] = f"host build of the walk unavailable: {ex}"
            if nb is not None:
                n_pass = int(stats.by_status[0])
                fixed = ALG_BYTES_FIXED * E + 4 * E + ALG_BYTES_PROBE * n_pass      # arrays + record + ent[] word; slot read + write
                out["roofline"]["needed_bytes"] = nb * E + fixed
                out["roofline"]["needed_line_bytes"] = nl * E + fixed + 64 * n_pass   # … when every touched 128-B line moves whole (slot lines too)
                out["roofline"]["needed_note"] = (f"per certificate the walk's reads cover {nb:.0f} bytes lying in {nl / 128:.2f} lines of 128 B "
                                                  f"(product walk on the host with a marking reader, first {k} sampled certificates); "
                                                  "+ 45 B arrays/record + 4 B reduce state per entry + the 64-B slot (a 128-B line) per PASS entry")
                if traffic:
                    out["roofline"]["over_fetch_vs_needed_bytes"] = traffic / out["roofline"]["needed_bytes"]
                    out["roofline"]["over_fetch_vs_needed_lines"] = traffic / out["roofline"]["needed_line_bytes"]
            quota_threads, quota = cpu_quota()
            threads = args.cpu_threads or quota_threads
            if threads > 1:
                # … and on every host CPU this process may use: a contiguous sample of the same batch (≈400 k entries per thread)
                del arrays
                sample_mt = min(E, args.cpu_sample_mt or min(400_000 * threads, 16_000_000))
                offs_mt = d_off[: sample_mt + 1].cpu().numpy().astype(np.uint64)
                nb_mt = int(offs_mt[-1])
                pay_mt = torch.zeros(nb_mt + N.PAYLOAD_PAD, dtype=torch.uint8)
                pay_mt[:nb_mt].copy_(d_pay[:nb_mt])
                arrays_mt = (pay_mt.numpy(), offs_mt, d_iss[:sample_mt].cpu().numpy().astype(np.uint32))
                best = None
                for _ in range(3):
                    v, dt_mt, npass = cpu_baseline_threads(arrays_mt, issuers, filt, now, sample_mt, threads, args.profile)
                    if best is None or v > best[0]:
                        best = (v, dt_mt, npass)
                ok_mt = best[2] == int((d_rec.view(-1, 32)[:sample_mt, 0] == 0).sum().item())
                out["cpu_baseline"] = {
                    "value": best[0], "unit": "certificates/sec", "cores": threads, "kind": "port",
                    "sample": f"first {sample_mt} entries of the same synthetic batch in {threads} contiguous slices, one "
                              f"oracle/ctmr_oracle.c engine per thread (per-thread in-process sets stand in for the "
                              f"shared Redis; not the Go binary), best of 3, {best[1]:.2f} s",
                    "host_cores_available": os.cpu_count(), "cgroup_cpu_quota": quota,
                    "pass_count_matches_gpu": bool(ok_mt),
                    "one_core": {"value": base_cpu["value"], "sample": base_cpu["sample"]}}
                del arrays_mt, pay_mt

    # ---- secondary lines inside a --full run (the driver's record carries them next to the headline):
    #      mixed      the same batch on the corpus that looks like a real log
    #      aligned128 the headline corpus with every certificate laid at a multiple of 128 bytes (what the layout is worth)
    if (args.full and rank == 0 and world == 1 and plain and not args.mixed and not args.aligned and not args.no_secondary
            and not os.environ.get("CTMR_BENCH_CHILD") and not args.variant and not args.pem and not args.fingerprint):
        out["secondary"] = {}
        legs = (("mixed", 1, 0, "the same batch on the MIXED corpus (half EC P-256 keys, 40 % OV-like subjects of 120-260 B, longer "
                 "issuer names, one GeneralizedTime in four): the lanes of a wave do not walk identical layouts", ["--mixed"]),
                ("aligned128", 0, 128, "the headline corpus with every certificate laid at a multiple of 128 bytes (an entry view; "
                 "the payload grows by the padding): the front window of a certificate then starts on a line boundary", ["--aligned", "128"]),
                ("fast_profile", 0, 0, "the headline batch under ctmr_set_profile(CTMR_PROFILE_FAST), the opt-in of a host that has "
                 "already parsed its certificates: strict_spki only — extension bodies, Name character sets and the subjectAltName "
                 "are skipped by length (looser than the reference on malformed ones); same results on this (well-formed) corpus",
                 ["--profile", "fast"]))
        headline_profile = args.profile
        for name, profile, align, what, leg_args in legs:
            try:
                if eng is not None:
                    eng.close()
                eng = d_off = d_pay = d_iss = d_et = d_rec = d_new = None
                raw_view.clear()
                torch.cuda.empty_cache()
                lcfg = synth.config(seed=20260921 + 4, n_issuers=args.issuers, zipf=1, dup_permille=dup_permille,
                                    ca_permille=10, expired_permille=10, profile=profile)
                args.aligned = align
                args.profile = "fast" if name == "fast_profile" else headline_profile
                eng, d_off, d_pay, d_iss, d_et, d_rec, d_new = setup(0, E, lcfg)
                mms, mst = [], None
                for k in range(1 + 3):
                    torch.cuda.synchronize()
                    t0m = time.perf_counter()
                    eng.reset_known()
                    if align:
                        mst = eng.map_view_device(d_pay.data_ptr(), raw_view["aligned"][1], raw_view["aligned"][2], E,
                                                  d_rec.data_ptr(), d_new.data_ptr())
                    else:
                        mst = eng.map_batch_device(d_pay.data_ptr(), d_off.data_ptr(), d_iss.data_ptr(), d_et.data_ptr(), E,
                                                   d_rec.data_ptr(), d_new.data_ptr())
                    if k:
                        mms.append((time.perf_counter() - t0m, mst.ms_map))
                m_step = sum(t for t, _ in mms) / len(mms)
                m_map = sum(m for _, m in mms) / len(mms)
                l_bytes = int((raw_view["aligned"][0] - d_off[:E]).sum().item()) if align else int(mst.payload_bytes)
                m_alg = l_bytes + ALG_BYTES_FIXED * E + ALG_BYTES_PROBE * int(mst.by_status[0])
                sec = {"workload": what, "value": E / m_step, "unit": "certificates/sec", "ms_per_step": m_step * 1e3, "steps": len(mms),
                       "note": "step = table clear + one map/reduce call, host-timed like the headline",
                       "map_ms": m_map, "mean_der_bytes": l_bytes / E, "n_new": int(mst.n_new),
                       "frac_algorithmic": m_alg / (m_map * 1e-3) / 1e9 / HBM_PEAK_GBPS, "traffic": None, "frac": None}
                if name == "fast_profile":
                    sec["same_results_as_the_reference_profile"] = bool(int(mst.n_new) == int(stats.n_new) and
                                                                   [int(x) for x in mst.by_status] == [int(x) for x in stats.by_status])
                if align:
                    sec["payload_bytes_per_entry_with_padding"] = raw_view["aligned"][1] / E
                    sec["same_results_as_the_packed_layout"] = bool(int(mst.n_new) == int(stats.n_new) and
                                                                    [int(x) for x in mst.by_status] == [int(x) for x in stats.by_status])
                if args.traffic == "auto":
                    targs = argparse.Namespace(**dict(vars(args), aligned=0))
                    mt, merr = measure_traffic(targs, min(E, args.traffic_entries), [kname],
                                               leg_args if name == "fast_profile" else leg_args + ["--profile", headline_profile])
                    if mt:
                        sec["traffic_bytes_per_cert"] = mt["traffic_bytes_per_cert"]
                        sec["traffic"] = mt["traffic_bytes_per_cert"] * E
                        sec["frac"] = sec["traffic"] / (m_map * 1e-3) / 1e9 / HBM_PEAK_GBPS
                    else:
                        sec["traffic_error"] = merr
                out["secondary"][name] = sec
            except (ctmr.CtmrError, RuntimeError) as ex:
                out["secondary"][name] = {"error": str(ex)}
        args.aligned = 0
        args.profile = headline_profile
        # raw_reference (round 6, VERDICT r05 #4a): the step IN FRONT of the path under the same profile — raw get-entries
        # buffers through LogEntryFromLeaf's decode (with strict_leaf: the leaf TBSCertificate of every precertificate entry
        # walked), the exact Chain[0] match and the map.  Decode parity with CT-go stays UNPINNED (no raw-entry vector in
        # the reference): the leg is a measurement, not a parity claim.
        try:
            if eng is not None:
                eng.close()
            eng = d_off = d_pay = d_iss = d_et = d_rec = d_new = None
            raw_view.clear()
            torch.cuda.empty_cache()
            E_raw = min(E, int(os.environ.get("CTMR_BENCH_RAW_ENTRIES", 20_000_000)))
            args.raw = True
            rcfg = synth.config(seed=20260921 + 4, n_issuers=args.issuers, zipf=1, dup_permille=dup_permille,
                                ca_permille=10, expired_permille=10, profile=0)
            eng, r_bounds, r_blob, r_ts, _, r_rec, r_new = setup(0, E_raw, rcfg)
            rms = []
            for k in range(1 + 3):
                torch.cuda.synchronize()
                t0r = time.perf_counter()
                eng.reset_known()
                rds = eng.decode_entries_device(r_blob.data_ptr(), r_bounds.data_ptr(), E_raw, raw_view["view"])
                rst = eng.map_view_device(r_blob.data_ptr(), raw_view["blob_bytes"], raw_view["view"], E_raw, r_rec.data_ptr(),
                                          r_new.data_ptr())
                if k:
                    rms.append((time.perf_counter() - t0r, rds.ms_decode, rds.ms_match, rst.ms_map))
            r_step = sum(t[0] for t in rms) / len(rms)
            out["secondary"]["raw_reference"] = {
                "workload": f"{E_raw} RAW get-entries ({raw_view['blob_bytes'] / E_raw:.0f} B/entry) under the {headline_profile} profile: "
                            "leaf TBSCertificate walk of the precertificate entries (strict_leaf) + LogEntryFromLeaf decode + exact "
                            "Chain[0] match + map/reduce; issuers registered by the engine",
                "value": E_raw / r_step, "unit": "entries/sec", "ms_per_step": r_step * 1e3, "steps": len(rms),
                "kernel_ms": {"leaf_tbs_check": sum(t[1] for t in rms) / len(rms), "decode_match": sum(t[2] for t in rms) / len(rms),
                              "map": sum(t[3] for t in rms) / len(rms)},
                "n_new": int(rst.n_new), "by_status": [int(x) for x in rst.by_status],
                "parity_note": "decode parity with CT-go's LogEntryFromLeaf is UNPINNED (the reference holds no raw-entry vector)"}
            del r_bounds, r_blob, r_ts, r_rec, r_new
        except (ctmr.CtmrError, RuntimeError) as ex:
            out["secondary"]["raw_reference"] = {"error": str(ex)}
        args.raw = False
    if rank == 0:
        print(json.dumps(out))
    if group is not None:
        group.close()
    if eng is not None:
        eng.close()


if __name__ == "__main__":
    main()
