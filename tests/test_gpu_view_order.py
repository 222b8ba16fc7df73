"""-m gpu: entry views in ANY byte order (ctmr_map_view_device and every call that takes `offsets` + `ends`).

The map kernels read through one buffer descriptor per wave whose base is the certificate of the wave's first lane; a lane
whose certificate lies below that base, or REL_SPAN or more beyond it, is out of the descriptor's reach (kernels/readers.h
lrel == REL_NONE) and takes the exact readers.  Every view of the rest of the suite ascends, so none of it ever produced such
a lane; tests/view_corpus.py builds views that do (tests/test_view_corpus_cpu.py holds the builder to its per-wave
properties; tests/test_view_order_cpu.py holds the walk of such a lane to terminating, on the CPU).

Reference: the ORACLE over the packed batch in ENTRY order (order in the blob is invisible to it) — status, flags, serial,
exp_hour, issuer_idx, the NEW list, by_status, the known sets.  In addition an engine of the same configuration fed the
packed batch through map_batch_device must give bit-identical records, NEW list and issuer counts, and a second
map_view_device of the same view finds nothing new.

Cells of the matrix (byte order x n x map_variant x profile x collect_meta x corpus) that run:
  A  all seven orders x map_variant {0 (k_map_fused), 13 (k_map_winc)} x reference profile, corpus "dups" (synthetic, 20 %
     duplicates: first occurrence in ENTRY order differs from first in byte order), n = 64*6 + 37 (a partial last wave)
  B  corpora {"dups", "mixed" (profile=1: EC keys, long subjects), "damaged" (one certificate in seven hurt, the fifteen kinds
     of tests/damage.py in turn, the finding kinds as X509 and as precertificate entries so that findings drop entries)} x {reversed, shuffled} x both
     variants x reference profile, n = 64*8
  C  fast profile: {reversed, shuffled, one_lane_low} x both variants, corpus "mixed", n = 64*4 + 37
  D  collect_meta on: {reversed, shuffled, aliased} x both variants x reference, and shuffled x both variants x fast, corpus
     "dups", n = 64*6 + 37: the first sightings (meta_new_device over the view) against tests/test_gpu_meta.py's expectation
  E  n = 5 (fewer than one wave): all seven orders x both variants x reference, corpus "dups"
Beyond the map: PEM over shuffled and aliased views, ranged SHA-256 over shuffled ranges, one Bloom round and one
owner-computes round of a world of 2 whose shards are shuffled views, and lanes out of reach by DISTANCE in a blob of a
little over 2^31 bytes."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import synth, _native as N  # noqa: E402
from ct_mapreduce_amd.distributed import Group, shard, shard_range  # noqa: E402
from ct_mapreduce_amd.engine import Batch, BatchResult, RECORD_DTYPE  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import view_corpus as V  # noqa: E402
from tests.damage import hurt, KINDS_FATAL, KINDS_FINDING  # noqa: E402
from tests.gpu_common import run_oracle, assert_records_equal, assert_state_equal  # noqa: E402
from tests.test_gpu_bloom import check_round, check_state  # noqa: E402
from tests.test_gpu_exchange import make_engine  # noqa: E402
from tests.test_gpu_meta import expected_first_sightings  # noqa: E402

DEV = torch.device("cuda:0")
NOW = synth.BASE_TIME
FILT = b"Synth Issuer 0"
REL_SPAN = 0x7e000000           # kernels/readers.h: certificates this far or farther from the wave's base take the exact reader
STRICT = {"reference": dict(strict_strings=True, strict_spki=True, strict_ext=True),
          "fast": dict(strict_strings=False, strict_spki=True, strict_ext=False)}
ITEM_DTYPE = np.dtype([("entry", "<u8"), ("kind", "<u4"), ("issuer_idx", "<u4"), ("exp_hour", "<i4"), ("off", "<u4"),
                       ("len", "<u4"), ("pad", "<u4")])


def damage_plan(n):
    """[(entry, kind, entry type or None = the generator's)]: every seventh entry is hurt, the fifteen kinds in turn; a kind
    whose cost is a non-fatal FINDING (it drops precertificates only) meets both entry types in turn."""
    kinds, out = KINDS_FATAL + KINDS_FINDING, []
    for j, i in enumerate(range(3, n, 7)):
        kind = kinds[j % len(kinds)]
        out.append((i, kind, j // len(kinds) % 2 if kind in KINDS_FINDING else None))
    return out


def corpus(name, n):
    """(config, batch): the batch carries its entry types; "damaged" hurts one certificate in seven in place (damage_plan)."""
    if name == "dups":
        cfg = synth.config(seed=20261016, n_issuers=16, dup_permille=200, ca_permille=20, expired_permille=20)
    elif name == "mixed":
        cfg = synth.config(seed=20261017, n_issuers=12, dup_permille=100, ca_permille=20, expired_permille=20, profile=1)
    else:
        cfg = synth.config(seed=20261018, n_issuers=16, dup_permille=100, ca_permille=20, expired_permille=20)
    b = synth.host_batch(cfg, 0, n)
    if name == "dups":   # … and every ninth entry repeats an earlier one BYTE FOR BYTE (the generator's duplicates repeat a key): "aliased" shares their ranges
        src = [i // 2 if i % 9 == 8 else i for i in range(n)]
        b = Batch.from_certs([b.cert(j) for j in src], [int(b.issuer_idx[j]) for j in src], b.entry_type.copy())
    if name == "damaged":
        certs, et = [b.cert(i) for i in range(n)], b.entry_type.copy()
        for i, kind, precert in damage_plan(n):
            certs[i] = hurt(certs[i], kind, orc.parse_cert(certs[i]))
            et[i] = precert if precert is not None else et[i]
        b = Batch.from_certs(certs, b.issuer_idx.copy(), et)
    return cfg, b


def engine(issuers, variant, profile, meta=False):
    e = ctmr.Engine(device=0, table_slots=1 << 15, pair_slots=1 << 12, map_variant=variant, collect_meta=meta)
    e.set_profile(profile)
    e.add_issuers(issuers)
    e.set_filter(FILT, False, NOW)
    return e


def up(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    return torch.from_numpy(a.copy()).to(DEV)


class DevView:
    """A view of tests/view_corpus.py on the device, with record and NEW-list buffers."""

    def __init__(self, batch, blob, start, end):
        n = batch.n
        self.n, self.blob_bytes = n, len(blob) - N.PAYLOAD_PAD
        self.blob = up(np.concatenate([blob, np.full(16, 0x5A, np.uint8)]))
        self.start, self.end = up(start, np.int64), up(end, np.int64)
        self.iss, self.et = up(batch.issuer_idx, np.int32), up(batch.entry_type, np.uint8)
        self.rec = torch.zeros(max(n, 1) * 32, dtype=torch.uint8, device=DEV)
        self.new = torch.zeros(max(n, 1), dtype=torch.int64, device=DEV)
        self.view = N.EntryView(cert_start=self.start.data_ptr(), cert_end=self.end.data_ptr(), issuer_idx=self.iss.data_ptr(),
                                entry_type=self.et.data_ptr(), timestamp=None, chain0_start=None, chain0_len=None)

    def map(self, eng):
        st = eng.map_view_device(self.blob.data_ptr(), self.blob_bytes, self.view, self.n, self.rec.data_ptr(), self.new.data_ptr())
        return BatchResult(self.rec.cpu().numpy()[:self.n * 32].view(RECORD_DTYPE).copy(),
                           self.new[:st.n_new].cpu().numpy().astype(np.uint64), st)


def map_packed(eng, b):
    pay = up(np.concatenate([b.payload, np.full(N.PAYLOAD_PAD + 16, 0x5A, np.uint8)]))
    off, iss, et = up(b.offsets, np.int64), up(b.issuer_idx, np.int32), up(b.entry_type, np.uint8)
    rec = torch.zeros(b.n * 32, dtype=torch.uint8, device=DEV)
    new = torch.zeros(b.n, dtype=torch.int64, device=DEV)
    st = eng.map_batch_device(pay.data_ptr(), off.data_ptr(), iss.data_ptr(), et.data_ptr(), b.n, rec.data_ptr(), new.data_ptr())
    return BatchResult(rec.cpu().numpy().view(RECORD_DTYPE).copy(), new[:st.n_new].cpu().numpy().astype(np.uint64), st)


def first_sightings(eng, dv, res):
    cap = 8 * dv.n + 64
    d_items = torch.zeros(cap * 32, dtype=torch.uint8, device=DEV)
    got = eng.meta_new_device(dv.blob.data_ptr(), dv.start.data_ptr(), dv.end.data_ptr(), dv.rec.data_ptr(), dv.new.data_ptr(),
                              int(res.stats.n_new), d_items.data_ptr(), cap)
    return np.frombuffer(d_items[:got * 32].cpu().numpy().tobytes(), dtype=ITEM_DTYPE)


def run_case(name, order, n, variant, profile, meta=False):
    cfg, b = corpus(name, n)
    if order == "with_empties":
        b = V.with_empty_entries(b, 7)
    issuers = synth.issuers(cfg)
    # (a seeded permutation of a handful of entries may leave entry 0 lowest: the first seed whose view has what the case is
    #  about — the same one for both map variants, which so meet identical bytes)
    for fill in range(n, n + 64):
        blob, start, end = V.make_view(b, order, fill=fill, lead=133, gap=90)
        below = V.lanes_below_lane0(start)
        if below.sum() > 0 or order in ("ascending", "with_empties"):
            break
    if order not in ("ascending", "with_empties") and n > 1:
        assert below.sum() > 0                                   # the view really has lanes out of reach
    if order == "aliased" and n > 9:
        assert len(set(start.tolist())) < n                      # … and entries that share one byte range
    o = orc.Engine(FILT, False, NOW)
    o.set_profile(profile)
    o, st, unk, eh = run_oracle(b, issuers, engine=o)
    eng = engine(issuers, variant, profile, meta)
    dv = DevView(b, blob, start, end)
    res = dv.map(eng)
    assert_records_equal(res, b, st, unk, eh, **STRICT[profile])
    assert_state_equal(eng, o, len(issuers))
    if meta:
        items = first_sightings(eng, dv, res)
        certs = [b.cert(i) for i in range(b.n)]
        canon = [eng.issuer_info(int(k)).canonical_idx for k in b.issuer_idx]
        want = expected_first_sightings(certs, canon, [int(i) for i in res.new_idx], res.records["exp_hour"])
        got = set()
        for it in items:
            c = eng.issuer_info(int(it["issuer_idx"])).canonical_idx
            der = certs[int(it["entry"])]
            if it["kind"] == N.MK_HOST:
                got.add((N.MK_HOST, int(it["entry"])))
            elif it["kind"] == N.MK_EXPDATE:
                got.add((N.MK_EXPDATE, c, int(it["exp_hour"]), b""))
            else:
                got.add((int(it["kind"]), c, 0, der[int(it["off"]):int(it["off"]) + int(it["len"])]))
        assert len(items) == len(got) and got == want
        assert {k[0] for k in want} >= {N.MK_EXPDATE, N.MK_DN} or not len(res.new_idx)
    counts = eng.issuer_counts().copy()
    # the same view once more: everything is known
    again = dv.map(eng)
    assert again.stats.n_new == 0 and len(again.new_idx) == 0
    assert (again.records["status"] == st).all() and ((again.records["flags"] & 2) == 0).all()
    assert (eng.issuer_counts() == counts).all()
    eng.close()
    # the packed batch through an engine of the same configuration: bit-identical
    eng2 = engine(issuers, variant, profile, meta)
    packed = map_packed(eng2, b)
    assert packed.records.tobytes() == res.records.tobytes()
    assert (packed.new_idx == res.new_idx).all() and packed.stats.n_new == res.stats.n_new
    assert list(packed.stats.by_status) == list(res.stats.by_status) and (eng2.issuer_counts() == counts).all()
    eng2.close()
    return res, st, unk, start


VARIANTS = (0, 13)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("order", V.ORDERS)
def test_every_byte_order_under_the_reference_profile(order, variant):                       # cell A
    res, st, unk, _ = run_case("dups", order, 64 * 6 + 37, variant, "reference")
    assert 0 < unk.sum() < (st == 0).sum()                       # duplicates: first occurrence in ENTRY order decides


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("order", ["reversed", "shuffled"])
@pytest.mark.parametrize("name", ["dups", "mixed", "damaged"])
def test_every_corpus_reversed_and_shuffled(name, order, variant):                            # cell B
    n = 64 * 8
    res, st, unk, start = run_case(name, order, n, variant, "reference")
    if name == "damaged":
        plan = damage_plan(n)
        low = np.array([start[i] < start[i - i % 64] for i in range(n)])          # out of reach: below its wave's lane 0
        fatal = [i for i, kind, _ in plan if kind in KINDS_FATAL]
        assert len(fatal) > 40 and (st[fatal] == orc.ST_PARSE_ERROR).all() and low[fatal].sum() > 10
        # a finding costs a precertificate its place and an X509 entry nothing (the oracle's call, met by the records above)
        # — for every finding kind, and in out-of-reach lanes too
        for kind in KINDS_FINDING:
            pre = [i for i, k, et in plan if k == kind and et == 1]
            x509 = [i for i, k, et in plan if k == kind and et == 0]
            assert len(pre) >= 2 and len(x509) >= 2
            assert (st[pre] == orc.ST_PARSE_ERROR).all() and (st[x509] != orc.ST_PARSE_ERROR).all(), kind
            assert (res.records["status"][pre] == orc.ST_PARSE_ERROR).all() and (res.records["status"][x509] != orc.ST_PARSE_ERROR).all()
        fpre = [i for i, k, et in plan if k in KINDS_FINDING and et == 1]
        fx = [i for i, k, et in plan if k in KINDS_FINDING and et == 0]
        assert low[fpre].any() and low[fx].any()
        assert low[[i for i, k, et in plan if k == "san_ip_length"]].any()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("order", ["reversed", "shuffled", "one_lane_low"])
def test_fast_profile(order, variant):                                                        # cell C
    run_case("mixed", order, 64 * 4 + 37, variant, "fast")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("order,profile", [("reversed", "reference"), ("shuffled", "reference"), ("aliased", "reference"),
                                           ("shuffled", "fast")])
def test_first_sightings_over_a_view(order, profile, variant):                                # cell D
    run_case("dups", order, 64 * 6 + 37, variant, profile, meta=True)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("order", V.ORDERS)
def test_fewer_entries_than_one_wave(order, variant):                                         # cell E
    run_case("dups", order, 5, variant, "reference")


# ---- beyond the map -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["shuffled", "aliased"])
def test_pem_over_a_view(order):
    n = 64 * 5 + 11
    cfg, b = corpus("dups", n)
    if order == "aliased":                                       # byte-identical entries, so that ranges are shared
        certs = [b.cert(i // 2 if i % 5 == 4 else i) for i in range(n)]
        b = Batch.from_certs(certs, [int(b.issuer_idx[i // 2 if i % 5 == 4 else i]) for i in range(n)], b.entry_type.copy())
    blob, start, end = V.make_view(b, order, fill=77, lead=61, gap=33)
    assert order != "aliased" or len(set(start.tolist())) < n
    eng = engine(synth.issuers(cfg), 0, "reference")
    dv = DevView(b, blob, start, end)
    res = dv.map(eng)
    rng = np.random.default_rng(5)
    anyidx = rng.integers(0, n, size=300)                        # an arbitrary index list: any order, with repeats
    for idx in (res.new_idx.astype(np.int64), anyidx.astype(np.int64)):
        m = len(idx)
        assert m > 50
        d_idx = up(idx, np.int64)
        d_po = torch.zeros(m + 1, dtype=torch.int64, device=DEV)
        total = eng.pem_encode_view_device(dv.blob.data_ptr(), dv.view, d_idx.data_ptr(), m, 0, 0, d_po.data_ptr())
        d_pem = torch.zeros(total, dtype=torch.uint8, device=DEV)
        eng.pem_encode_view_device(dv.blob.data_ptr(), dv.view, d_idx.data_ptr(), m, d_pem.data_ptr(), total, d_po.data_ptr())
        po, pem = d_po.cpu().numpy(), d_pem.cpu().numpy().tobytes()
        for k in range(m):
            assert pem[po[k]:po[k + 1]] == orc.pem_encode(b.cert(int(idx[k]))), (order, k)
        assert po[m] == total == len(pem)
    eng.close()


def test_fingerprints_over_shuffled_ranges():
    n = 64 * 4 + 29
    cfg, b = corpus("mixed", n)
    b = V.with_empty_entries(b, 50)
    blob, start, end = V.make_view(b, "shuffled", fill=78, lead=9, gap=70)
    eng = engine(synth.issuers(cfg), 0, "reference")
    dv = DevView(b, blob, start, end)
    d_dg = torch.zeros(n * 32, dtype=torch.uint8, device=DEV)
    eng.fingerprint_device(dv.blob.data_ptr(), dv.start.data_ptr(), dv.end.data_ptr(), n, d_dg.data_ptr())
    got = d_dg.cpu().numpy().tobytes()
    for i in range(n):
        assert got[32 * i:32 * i + 32] == hashlib.sha256(b.cert(i)).digest(), i
    eng.close()


@pytest.mark.parametrize("mode", ["bloom", "owner"])
def test_a_group_round_whose_shards_are_shuffled_views(mode):
    """World 2, one round: each rank's shard is a shuffled view of its part of the stream.  These steps run k_map_winc in the
    default configuration (reference profile).  Same dedup result as the oracle over the whole stream."""
    world, n_total = 2, 64 * 14 + 21
    cfg = synth.config(seed=20261019, n_issuers=16, dup_permille=300, ca_permille=30, expired_permille=30)
    issuers = synth.issuers(cfg)
    o, st, unk, eh = run_oracle(synth.host_batch(cfg, 0, n_total), issuers, FILT, False, NOW)
    assert 0 < unk.sum() < (st == 0).sum()
    engines = [make_engine(issuers) for _ in range(world)]
    g = Group.local(engines)
    if mode == "bloom":
        g.bloom_config(1 << 16)
    shards, keep, ranges, views = [], [], [], []
    for r in range(world):
        lo, hi = shard_range(n_total, r, world)
        b = synth.host_batch(cfg, lo, hi - lo)
        blob, start, end = V.make_view(b, "shuffled", fill=90 + r, lead=40, gap=64)
        assert V.lanes_below_lane0(start).sum() > b.n // 4
        dv = DevView(b, blob, start, end)
        views.append(dv)
        keep.append((dv.blob, dv.start, dv.iss, dv.et, dv.rec, dv.new))
        shards.append(shard(dv.blob.data_ptr(), dv.start.data_ptr(), dv.iss.data_ptr(), dv.et.data_ptr(), b.n, dv.rec.data_ptr(),
                            dv.new.data_ptr(), order_base=lo, d_ends=dv.end.data_ptr(), blob_bytes=dv.blob_bytes))
        ranges.append((lo, hi))
    stats = g.map_batch(mode, shards)
    assert g.info().keys_sent > 0
    check_round(keep, ranges, stats, st, unk)
    check_state(engines, g, o, len(issuers))
    stats2 = g.map_batch(mode, shards)
    assert all(s.n_new == 0 for s in stats2)
    check_state(engines, g, o, len(issuers))
    g.close()
    for e in engines:
        e.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_lanes_out_of_reach_by_distance(variant):
    """One blob of a little over 2^31 bytes; three waves, each ascending from a lane 0 near the blob's front, with lanes at
    REL_SPAN - 4096, REL_SPAN - 1, REL_SPAN, REL_SPAN + 128 from the wave's base (lane 0's start rounded down to 128) and just
    below the blob's end: in reach, the last in reach, the first out of reach, out of reach."""
    n = 64 * 3
    cfg, b = corpus("dups", n)
    issuers = synth.issuers(cfg)
    size = (1 << 31) + (48 << 20)
    try:
        d_blob = torch.full((size,), 0xA5, dtype=torch.uint8, device=DEV)
    except (RuntimeError, MemoryError) as e:
        pytest.skip("no room for a blob of %d bytes: %s" % (size, str(e)[:80]))
    blob_bytes = size - N.PAYLOAD_PAD - 16
    lens = np.diff(b.offsets.astype(np.int64))
    start = np.zeros(n, np.int64)
    far = {0: [REL_SPAN - 4096, REL_SPAN + 128, REL_SPAN + 8192], 1: [REL_SPAN - 1, REL_SPAN + 4096 + 3],
           2: [REL_SPAN - 8192 - 7, REL_SPAN, REL_SPAN + 2 * 8192 + 1]}
    for w in range(3):
        base = (1 << 20) * w + 128 * 3                           # the wave's descriptor base: lane 0 starts 5 octets behind it
        at, lanes = base + 5, list(range(64 * w, 64 * w + 64))
        n_far = len(far[w]) + 1
        for i in lanes[:64 - n_far]:
            start[i] = at
            at += int(lens[i]) + 17
        assert at < (1 << 20) * (w + 1)
        for i, d in zip(lanes[64 - n_far:], far[w]):
            start[i] = base + d
        last = lanes[-1]                                         # just below the blob's end, each wave a little lower
        start[last] = blob_bytes - (3 - w) * 4096 + (4096 - int(lens[last]) if w == 2 else 0)
        assert (np.diff(start[lanes]) > 0).all()                 # ascending within the wave: out of reach by distance only
    end = start + lens
    assert int(end.max()) == blob_bytes
    # which lanes the descriptor reaches: distance from the wave's base (lane 0's start rounded down to 128) below REL_SPAN
    dist = np.array([start[i] - (start[i - i % 64] & ~127) for i in range(n)])
    out = dist >= REL_SPAN
    assert [int(out[64 * w:64 * w + 64].sum()) for w in range(3)] == [3, 2, 3]
    assert [int(d) - REL_SPAN for d in dist[out][[0, 1, 3, 5, 6]]] == [128, 8192, 4096 + 3, 0, 2 * 8192 + 1]
    assert sorted(int(d) - REL_SPAN for d in dist[~out] if d > REL_SPAN - (1 << 20)) == [-8192 - 7, -4096, -1]
    order = np.argsort(start)
    assert (end[order][:-1] <= start[order][1:]).all()           # no two certificates overlap
    for i in range(n):
        d_blob[int(start[i]):int(end[i])] = up(np.frombuffer(b.cert(i), np.uint8))
    o = orc.Engine(FILT, False, NOW)
    o.set_profile("reference")
    o, st, unk, eh = run_oracle(b, issuers, engine=o)
    eng = engine(issuers, variant, "reference")
    d_st, d_en = up(start), up(end)
    d_iss, d_et = up(b.issuer_idx, np.int32), up(b.entry_type, np.uint8)
    d_rec = torch.zeros(n * 32, dtype=torch.uint8, device=DEV)
    d_new = torch.zeros(n, dtype=torch.int64, device=DEV)
    view = N.EntryView(cert_start=d_st.data_ptr(), cert_end=d_en.data_ptr(), issuer_idx=d_iss.data_ptr(), entry_type=d_et.data_ptr(),
                       timestamp=None, chain0_start=None, chain0_len=None)
    stt = eng.map_view_device(d_blob.data_ptr(), blob_bytes, view, n, d_rec.data_ptr(), d_new.data_ptr())
    res = BatchResult(d_rec.cpu().numpy().view(RECORD_DTYPE).copy(), d_new[:stt.n_new].cpu().numpy().astype(np.uint64), stt)
    assert_records_equal(res, b, st, unk, eh, **STRICT["reference"])
    assert_state_equal(eng, o, len(issuers))
    assert 0 < unk.sum() < (st == 0).sum()
    eng.close()
    del d_blob
    torch.cuda.empty_cache()
