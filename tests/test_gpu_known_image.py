"""-m gpu: the known-certificate image (include/ctmr.h ctmr_known_*).  Export → import carries every
serials:: set across engines whose issuer numbering differs; a warm restart maps like no restart (and like the oracle);
an import equals SetInsert of the same members; a restore into a group of another world size puts every key on its
owner; growth, rejection and the Redis stream behave as the header says."""
import io
import struct
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr
from ct_mapreduce_amd import known_image as KI, synth, _native as N
from ct_mapreduce_amd.distributed import Group, shard_range
from ct_mapreduce_amd.engine import RECORD_DTYPE
from ct_mapreduce_amd.remote_cache import GpuRemoteCache, redis_dump, redis_load
from tests.gpu_common import run_oracle
from tests.test_gpu_exchange import to_dev, dev_shard, FILT, NOW, DEV
from tests.test_gpu_scale import device_batch

CFG = synth.config(seed=71, n_issuers=6, dup_permille=150, ca_permille=20, expired_permille=20)
UNREG_ID = KI.issuer_id(bytes(range(32))).decode()


def engine(issuers, order=None, **kw):
    kw.setdefault("table_slots", 1 << 16)
    kw.setdefault("pair_slots", 1 << 12)
    e = ctmr.Engine(device=0, **kw)
    if order is not None:
        issuers = [issuers[k] for k in order]
    e.add_issuers(issuers)
    e.set_filter(FILT, False, NOW)
    return e


def state(e):
    """Everything a host can see of the serials:: sets, independent of the issuer numbering."""
    keys = sorted(e.keys(b"serials::*"))
    counts = e.issuer_counts()
    by_id = {}
    for k in range(e.issuer_count()):
        info = e.issuer_info(k)
        if info.valid:
            by_id[info.issuer_id] = int(counts[k])
    return {"keys": keys, "lists": {k: e.set_list(k) for k in keys}, "card": {k: e.set_cardinality(k) for k in keys},
            "by_id": by_id, "total": e.total_count()}


def add_point_members(e, issuers_ids):
    """Members the map never makes: serials of 41..60 octets, and members under an issuer ID nobody registered."""
    hour = KI.exp_date_id(491000).decode()
    for k, ident in enumerate(issuers_ids[:2]):
        for L in (41, 50, 60):
            e.set_insert("serials::%s::%s" % (hour, ident), bytes([k + 1]) * L)
    for j in range(5):
        e.set_insert("serials::%s::%s" % (hour, UNREG_ID), b"\x42" * (3 + j))
    e.set_insert("serials::%s::%s" % (hour, UNREG_ID), b"\x43" * 45)


def mapped(e, batch):
    return e.map_batch(batch)


def test_round_trip_across_issuer_numbering():
    issuers = synth.issuers(CFG)
    a = engine(issuers)
    mapped(a, synth.host_batch(CFG, 0, 6000))
    ids = [a.issuer_id(k) for k in range(len(issuers))]
    add_point_members(a, ids)
    img = a.known_export()
    b = engine(issuers, order=[5, 3, 1, 0, 2, 4])
    assert [b.issuer_info(k).canonical_idx for k in range(6)] == list(range(6))
    st = b.known_import(img)
    assert st["members"] == KI.parse(img).n_members and st["taken"] == st["inserted"] == st["members"]
    assert st["known"] == 0 and st["host_members"] == st["host_inserted"] == KI.parse(img).n_host_members > 0
    assert state(a) == state(b)
    assert KI.parse(b.known_export()).sets == KI.parse(img).sets
    # the device variant: the same image, the members on the device
    meta, d = a.known_export_device()
    assert meta == img[:len(meta)] and KI.parse(meta + d.cpu().numpy().tobytes()).sets == KI.parse(img).sets
    c = engine(issuers, order=[2, 0, 1, 3, 4, 5])
    c.known_import_device(meta, d)
    assert state(c) == state(a)
    for x in (a, b, c):
        x.close()


@pytest.mark.parametrize("profile", ["reference", "fast"])
def test_warm_restart_maps_like_no_restart(profile):
    cfg = synth.config(seed=72, n_issuers=6, dup_permille=150, ca_permille=20, expired_permille=20)
    issuers = synth.issuers(cfg)
    b1 = synth.host_batch(cfg, 0, 5000)
    b2_lo = synth.host_batch(cfg, 2500, 2500)        # the last half of batch 1 again ...
    b2_hi = synth.host_batch(cfg, 5000, 3000)        # ... and new entries: ≥ 30 % of batch 2's keys come from batch 1
    from ct_mapreduce_amd.engine import Batch
    b2 = Batch.from_certs([b2_lo.cert(i) for i in range(b2_lo.n)] + [b2_hi.cert(i) for i in range(b2_hi.n)],
                          np.concatenate([b2_lo.issuer_idx, b2_hi.issuer_idx]), np.concatenate([b2_lo.entry_type, b2_hi.entry_type]))
    a = engine(issuers)
    a.set_profile(profile)
    a.map_batch(b1)
    b = engine(issuers)
    b.set_profile(profile)
    b.known_import(a.known_export())
    ra, rb = a.map_batch(b2), b.map_batch(b2)
    assert (ra.records.view(np.uint8) == rb.records.view(np.uint8)).all()
    assert (ra.new_idx == rb.new_idx).all()
    for f in ("n", "n_new", "n_dup", "n_host_set"):
        assert getattr(ra.stats, f) == getattr(rb.stats, f), f
    assert list(ra.stats.by_status) == list(rb.stats.by_status)
    assert (a.issuer_counts() == b.issuer_counts()).all()
    # both equal the oracle fed batch 1 then batch 2
    o, _, _, _ = run_oracle(b1, issuers, FILT, False, NOW)
    o, st, unk, eh = run_oracle(b2, issuers, FILT, False, NOW, engine=o)
    assert (rb.records["status"] == st).all()
    assert (((rb.records["flags"] & N.FL_WAS_UNKNOWN) != 0) == (unk != 0)).all()
    assert 0.3 * (st == 0).sum() <= ((st == 0) & (unk == 0)).sum() and unk.sum() > 0
    assert b.total_count() == o.total_count()
    a.close()
    b.close()


def test_import_equals_set_insert():
    issuers = synth.issuers(CFG)
    src = engine(issuers)
    src.map_batch(synth.host_batch(CFG, 0, 800))
    ids = [src.issuer_id(k) for k in range(len(issuers))]
    add_point_members(src, ids)
    img = src.known_export()
    sets = KI.parse(img).sets
    x, y = engine(issuers), engine(issuers)
    # both already hold every third member (and one member of their own)
    pre = [(k, m) for k in sorted(sets) for m in sets[k]][::3]
    for e in (x, y):
        for k, m in pre:
            e.set_insert(k, m)
        e.set_insert(sorted(sets)[0], b"\x99\x98")
    st = x.known_import(img)
    ins = host_ins = 0
    im = KI.parse(img)
    host_pairs = set()
    off = 0
    # which members are in the host section: rebuild from the raw image (the parse merges both sections)
    _, _, _, n_iss, _, n_sets, n_mem, host_bytes, n_host, _ = KI._HEADER.unpack_from(img, 0)
    h = 64 + 32 * n_iss + 24 * n_sets
    while off < host_bytes:
        kl = int.from_bytes(img[h + off:h + off + 4], "little")
        key = img[h + off + 4:h + off + 4 + kl]
        ml = int.from_bytes(img[h + off + 4 + kl:h + off + 8 + kl], "little")
        host_pairs.add((key, img[h + off + 8 + kl:h + off + 8 + kl + ml]))
        off += 8 + kl + ml
    for k in sorted(sets):
        for m in sets[k]:
            new = y.set_insert(k, m)
            if (k, m) in host_pairs:
                host_ins += new
            else:
                ins += new
    assert st["inserted"] == ins and st["known"] == st["taken"] - ins and st["host_inserted"] == host_ins
    assert st["taken"] == im.n_members and st["host_members"] == n_host
    assert state(x) == state(y)
    ti = x.table_info()
    assert ti.occupied == y.table_info().occupied
    for e in (src, x, y):
        e.close()


def test_resharded_restore_puts_every_key_on_its_owner():
    cfg = synth.config(seed=73, n_issuers=8, dup_permille=200, ca_permille=20, expired_permille=20)
    issuers = synth.issuers(cfg)
    b1 = synth.host_batch(cfg, 0, 6000)
    b2 = synth.host_batch(cfg, 3000, 6000)
    a = engine(issuers)
    a.map_batch(b1)
    img = a.known_export()
    sets_a = KI.parse(img).sets
    a_total_1 = a.total_count()
    ra = a.map_batch(b2)
    for world in (2, 3):
        for mode in ("owner", "bloom"):
            engines = [engine(issuers) for _ in range(world)]
            g = Group.local(engines)
            if mode == "bloom":
                g.bloom_config(1 << 16)
            stats = [e.known_import(img, world=world, rank=r) for r, e in enumerate(engines)]
            assert sum(s["taken"] for s in stats) == sum(len(v) for v in sets_a.values()) - stats[0]["host_members"]
            assert all(s["host_members"] == 0 for s in stats[1:])
            assert sum(sum(e.issuer_counts().astype(np.int64) for e in engines)) == a_total_1
            union = {}
            for e in engines:
                for k, v in KI.parse(e.known_export()).sets.items():
                    for m in v:
                        assert m not in union.get(k, set()), "a key on two ranks"
                        union.setdefault(k, set()).add(m)
            assert {k: sorted(v) for k, v in union.items()} == sets_a
            # batch 2 through the group: the same WasUnknown flags and totals as A mapping batch 2
            shards, keep = [], []
            for r in range(world):
                lo, hi = shard_range(b2.n, r, world)
                from ct_mapreduce_amd.engine import Batch
                sub = Batch.from_certs([b2.cert(i) for i in range(lo, hi)], b2.issuer_idx[lo:hi], b2.entry_type[lo:hi])
                t = to_dev(sub)
                keep.append((t, lo, hi))
                shards.append(dev_shard(t, sub.n, order_base=lo))
            g.map_batch(mode, shards)
            for (t, lo, hi) in keep:
                rec = t[4].cpu().numpy().view(RECORD_DTYPE)
                assert (((rec["flags"] & 2) != 0) == ((ra.records["flags"][lo:hi] & 2) != 0)).all(), (world, mode)
            assert g.total_count() == a.total_count()
            assert (g.issuer_counts(len(issuers)) == a.issuer_counts()).all()
            if mode == "bloom":
                # the inverse direction: every rank's image, imported into one engine, is A's state
                one = engine(issuers)
                for e in engines:
                    one.known_import(e.known_export())
                assert state(one) == state(a)
                one.close()
            g.close()
            for e in engines:
                e.close()
    a.close()


def test_growth_during_import():
    n = 2_100_000
    rng = np.random.default_rng(5)
    ident = KI.issuer_id(bytes(32))
    ser = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    ser[:, 0] = 1
    hours = 491000 + (np.arange(n) % 40)
    # a hand-built image: 40 sets of one (unregistered-name) issuer digest — registered below through a synthetic issuer
    cfg = synth.config(seed=74, n_issuers=1)
    issuers = synth.issuers(cfg)
    src = engine(issuers)
    ident = src.issuer_id(0)
    digest = __import__("base64").urlsafe_b64decode(ident)
    order = np.argsort(hours, kind="stable")
    rec = np.zeros(n, KI.MEMBER_DTYPE)
    rec["len"] = 16
    rec["serial"][:, :16] = ser[order]
    sets, first = [], 0
    for h in range(40):
        c = int((hours == 491000 + h).sum())
        sets.append((491000 + h, c, first))
        first += c
    body = digest + b"".join(struct.pack("<iIQQ", h, 0, f, c) for h, c, f in sets)
    head = KI._HEADER.pack(KI.MAGIC, 1, 64, 1, 0, 40, n, 0, 0, 0)
    meta = head + body
    meta += b"\0" * (-len(meta) % 64)
    img = meta + rec.tobytes()
    e = engine(issuers, table_slots=1 << 10)
    t0 = e.table_info()
    st = e.known_import(img)
    ti = e.table_info()
    assert ti.rebuilds > t0.rebuilds and st["taken"] == n
    assert st["inserted"] == len({bytes(r) for r in ser}) and e.total_count() == st["inserted"]
    assert ti.arena_used - t0.arena_used <= st["taken"]
    q = engine(issuers, table_slots=1 << 10)
    t1 = q.table_info()
    s4 = q.known_import(img, world=4, rank=0)
    assert 0.23 * n < s4["taken"] < 0.27 * n
    assert q.table_info().arena_used - t1.arena_used <= s4["taken"]
    for x in (src, e, q):
        x.close()


def test_rejection_leaves_no_trace():
    issuers = synth.issuers(CFG)
    a = engine(issuers)
    a.map_batch(synth.host_batch(CFG, 0, 2000))
    add_point_members(a, [a.issuer_id(k) for k in range(6)])
    img = a.known_export()
    b = engine(issuers)
    b.map_batch(synth.host_batch(CFG, 5000, 500))
    before = (state(b), tuple(getattr(b.table_info(), f) for f, _ in N.TableInfo._fields_))
    _, _, _, n_iss, _, n_sets, n_mem, host_bytes, n_host, _ = KI._HEADER.unpack_from(img, 0)
    so = 64 + 32 * n_iss
    bad_len = bytearray(img)
    bad_len[-48] = 41                                                   # serial_len 41 in the last record
    gap = bytearray(img)
    struct.pack_into("<Q", gap, so + 24 + 8, struct.unpack_from("<Q", img, so + 24 + 8)[0] + 1)   # set 1 starts late
    unreg = KI.build(KI.parse(img).sets)      # the short members under the unregistered issuer ID now form a set
    assert UNREG_ID.encode() in b"".join(KI.parse(unreg).sets) and len(KI.parse(unreg).issuers) == 7
    for bad, kw in ((bytes(bad_len), {}), (bytes(gap), {}), (unreg, {"world": 2, "rank": 0})):
        with pytest.raises(ctmr.CtmrError) as ex:
            b.known_import(bad, **kw)
        assert ex.value.code == N.E_INVAL
        assert (state(b), tuple(getattr(b.table_info(), f) for f, _ in N.TableInfo._fields_)) == before
    a.close()
    b.close()


def test_resp_equivalence():
    issuers = synth.issuers(CFG)
    a = engine(issuers)
    a.map_batch(synth.host_batch(CFG, 0, 3000))
    add_point_members(a, [a.issuer_id(k) for k in range(6)])
    want = io.BytesIO()
    redis_dump(GpuRemoteCache(a), want, patterns=("serials::*",))
    got = io.BytesIO()
    KI.to_resp(a.known_export(), got)
    assert got.getvalue() == want.getvalue()
    x, y = engine(issuers), engine(issuers)
    x.known_import(KI.from_resp(want.getvalue()))
    redis_load(GpuRemoteCache(y), io.BytesIO(want.getvalue()))
    assert state(x) == state(y) == state(a)
    for e in (a, x, y):
        e.close()


def test_scale_twenty_million():
    n = 20_000_000
    cfg = synth.config(seed=20260921 + 4, n_issuers=64, zipf=1, dup_permille=100, ca_permille=10, expired_permille=10)
    issuers = synth.issuers(cfg)
    a = ctmr.Engine(device=0, table_slots=1 << 26, pair_slots=1 << 16)
    a.add_issuers(issuers)
    a.set_filter(b"", False, NOW)
    d_off, d_pay, d_iss, d_et, total = device_batch(a, cfg, 0, n, DEV)
    a.map_batch_device(d_pay.data_ptr(), d_off.data_ptr(), d_iss.data_ptr(), d_et.data_ptr(), n, 0, 0)
    del d_off, d_pay, d_iss, d_et
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    meta, d = a.known_export_device()
    t1 = time.perf_counter()
    b = ctmr.Engine(device=0, table_slots=1 << 20, pair_slots=1 << 16)
    b.add_issuers(issuers[::-1])
    t2 = time.perf_counter()
    st = b.known_import_device(meta, d)
    t3 = time.perf_counter()
    print("known image at %d members: export %.1f ms, import %.1f ms" % (d.numel() // 48, (t1 - t0) * 1e3, (t3 - t2) * 1e3))
    assert st["inserted"] == st["taken"] == d.numel() // 48 == a.total_count() == b.total_count()
    ca, cb = a.issuer_counts(), b.issuer_counts()
    for k in range(len(issuers)):
        assert int(ca[k]) == int(cb[len(issuers) - 1 - k])
    keys = sorted(a.keys(b"serials::*"))
    assert keys == sorted(b.keys(b"serials::*"))
    for key in keys[::max(1, len(keys) // 200)][:200]:
        assert a.set_list(key) == b.set_list(key)
    a.close()
    b.close()
