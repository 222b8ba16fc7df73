"""-m gpu: bulk SetContains / SetRemove over an image's member records (include/ctmr.h ctmr_known_query* /
ctmr_known_remove*; kernels/image.h k_known_query / k_known_remove).

Expected answers come from the CPU twins (known_image.query / known_image.subtract) over the sets the test itself built;
on small images they are also compared with a replay of Engine.set_contains / set_remove, the point path.  The engines
are made the way tests/test_gpu_known_image.py makes them, the corpora come from tests/known_corpus.py.
"""
import base64
import ctypes as C
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr
from ct_mapreduce_amd import known_image as KI, synth, _native as N
from ct_mapreduce_amd.distributed import Group, shard_range
from ct_mapreduce_amd.engine import Batch
from tests import known_corpus as KC
from tests.test_gpu_exchange import to_dev, dev_shard, DEV
from tests.test_gpu_known_image import engine, state, add_point_members, UNREG_ID

CFG = synth.config(seed=93, n_issuers=6, dup_permille=150, ca_permille=20, expired_permille=20)
ORDER = [5, 3, 1, 0, 2, 4]
HOURS = [490999, 491000, 491016, 491040]
SIZES = {"uniform": [900, 1, 255, 256, 257, 40, 3000], "tiny": [400, 1, 255, 256, 257, 2, 3, 700],
         "interleaved": [700, 1, 255, 256, 257, 130, 2000], "runs": [1800, 1, 255, 256, 257, 3100], "twins": 0}
RPLS = (1, 2, 4, 8)             # the instantiations of the probe kernels (CTMR_KNOWN_PROBE_RPL)
GUARD = 64


@pytest.fixture(scope="module")
def issuers():
    return synth.issuers(CFG)


@pytest.fixture(scope="module")
def digests(issuers):
    e = engine(issuers)
    out = [base64.urlsafe_b64decode(e.issuer_id(k)) for k in range(len(issuers))]
    e.close()
    return out


def on_device(rec):
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1).copy()).to(DEV)


def table(e):
    return tuple(getattr(e.table_info(), f) for f, _ in N.TableInfo._fields_)


def query_both(e, img, **kw):
    """The host and the device variant, which must agree → (flags, host_flags, stats)."""
    fl, hf, st = e.known_query(img, **kw)
    meta, rec = KC.split(img)
    dfl, dhf, dst = e.known_query_device(meta, on_device(rec), **kw)
    assert (dfl.cpu().numpy() == fl).all() and (dhf == hf).all() and dst == st
    return fl, hf, st


def replay_contains(e, img):
    dev, host = KI.records(img)
    return (np.array([e.set_contains(k, m) for k, m in dev], np.uint8),
            np.array([e.set_contains(k, m) for k, m in host], np.uint8))


def check_query(e, img, held, replay=False, **kw):
    want, want_host = KI.query(img, held)
    fl, hf, st = query_both(e, img, **kw)
    assert (fl == want).all() and (hf == want_host).all()
    assert st == {"members": len(want), "taken": len(want), "hits": int(want.sum()), "host_members": len(want_host),
                  "host_hits": int(want_host.sum())}
    if replay:
        r, rh = replay_contains(e, img)
        assert (r == want).all() and (rh == want_host).all()
    return fl, hf


def sorted_export(e):
    img = e.known_export()
    meta, rec = KC.split(img)
    sets_of = KC.record_sets(img)
    rows = rec.view(np.uint8).reshape(-1, 48)
    out = [meta]
    for s in range(int(sets_of.max()) + 1 if len(sets_of) else 0):
        out.append(b"".join(sorted(bytes(r) for r in rows[sets_of == s])))
    return out


def subset_image(pairs):
    sets = {}
    for k, m in pairs:
        sets.setdefault(k, []).append(m)
    return KI.build(sets)


# ---- 1. an engine's own export

def test_own_export_is_all_present(issuers):
    a = engine(issuers)
    a.map_batch(synth.host_batch(CFG, 0, 3000))
    add_point_members(a, [a.issuer_id(k) for k in range(len(issuers))])
    img = a.known_export()
    held = KI.parse(img).sets
    im = KI.parse(img)
    assert im.n_members > 1000 and im.n_host_members > 0
    b = engine(issuers, order=ORDER)
    b.known_import(img)
    for e in (a, b):
        fl, hf = check_query(e, img, held, replay=True)
        assert (fl == 1).all() and (hf == 1).all() and len(fl) == im.n_members and len(hf) == im.n_host_members
    # an engine that registered fewer issuers answers the sets of the others from its host-side store
    c = engine(issuers[:3])
    c.known_import(img)
    fl, hf = check_query(c, img, held, replay=True)
    assert (fl == 1).all() and (hf == 1).all()
    empty = engine(issuers[:3])
    fl, hf = check_query(empty, img, {}, replay=True)
    assert not fl.any() and not hf.any()
    for e in (a, b, c, empty):
        e.close()


# ---- 2. near misses

def test_near_misses(issuers, digests, golden_certs):
    shared = [golden_certs["kEmptySPKI"], golden_certs["kRealSPKI"], golden_certs["kLeadingZeroes"]]
    e = engine(issuers + shared)
    assert e.issuer_info(8).canonical_idx == 6                   # two certificates, one SPKI: one canonical issuer
    d_shared = base64.urlsafe_b64decode(e.issuer_id(8))
    rng = np.random.default_rng(3)
    h0, h1 = HOURS[1], HOURS[2]
    base = [bytes(rng.integers(1, 256, size=L, dtype=np.uint8).tolist()) for L in (1, 8, 16, 19, 20, 21, 24, 39, 40)
            for _ in range(40)]
    held = {KI.set_key(h0, digests[0]): sorted(set(base)), KI.set_key(h0, d_shared): [b"\x07" * 9, b"\x08" * 30]}
    for k, ms in held.items():
        for m in ms:
            assert e.set_insert(k, m)
    ask = {k: set(v) for k, v in held.items()}
    k0 = KI.set_key(h0, digests[0])
    for m in base:
        other = bytes([m[0] ^ 0x55]) + m[1:]
        ask[k0] |= {other, m[:-1], m + b"\x00"}                  # another serial; one shorter; one longer ending in 00
        ask.setdefault(KI.set_key(h1, digests[0]), set()).add(m)  # another hour
        ask.setdefault(KI.set_key(h0, digests[1]), set()).add(m)  # another registered issuer
    img = KI.build(ask)
    want, _ = KI.query(img, held)
    assert 0.1 < want.mean() < 0.5 and KI.parse(img).n_host_members > 0     # the 41-octet twins are host members
    fl, hf = check_query(e, img, held, replay=True)
    by_key = dict(zip(KI.records(img)[0], fl))
    assert by_key[(KI.set_key(h0, d_shared), b"\x07" * 9)] == 1
    e.close()


# ---- 3. every serial length, both record classes, ragged sizes, every instantiation

@pytest.fixture(scope="module", params=KC.MIXES)
def loaded(request, issuers, digests):
    mix = request.param
    c = KC.make(mix, digests, HOURS, SIZES[mix], seed=17)
    other = KC.make(mix, digests, HOURS, SIZES[mix], seed=18)
    e = engine(issuers, order=ORDER)
    e.known_import(c.image)
    yield mix, c, other, e
    e.close()


def test_every_length_and_class(loaded):
    mix, c, other, e = loaded
    fl, hf = check_query(e, c.image, c.sets)
    assert (fl == 1).all() and (hf == 1).all()
    union = {k: sorted(set(c.sets[k]) | set(other.sets[k])) for k in c.sets}
    fl, _ = check_query(e, KC.image(union), c.sets)
    assert mix == "twins" or (0 < fl.sum() < len(fl))


@pytest.mark.parametrize("rpl", RPLS)
def test_ragged_sizes_in_every_instantiation(loaded, rpl, monkeypatch):
    mix, c, other, e = loaded
    monkeypatch.setenv("CTMR_KNOWN_PROBE_RPL", str(rpl))
    union = {k: sorted(set(c.sets[k]) | set(other.sets[k])) for k in c.sets}
    pairs = [(k, m) for k in sorted(union) for m in union[k] if len(m) <= 40]
    sizes = [0, 1, 63, 64, 65, 255, 257, 64 * rpl - 1, 64 * rpl + 1, 256 * rpl - 1, 256 * rpl, 256 * rpl + 1,
             3 * 256 * rpl + 77]
    for n in sorted(set(s for s in sizes if s <= len(pairs))):
        step = max(1, len(pairs) // max(n, 1))
        check_query(e, subset_image(pairs[::step][:n]), c.sets)
    check_query(e, KC.image(union), c.sets)


# ---- 4. world / rank

@pytest.mark.parametrize("world", [2, 3, 4])
def test_world_and_rank(world, issuers, digests):
    c = KC.make("uniform", digests, HOURS[:2], [700, 300, 1, 257], seed=43)
    other = KC.make("uniform", digests, HOURS[:2], [300], seed=44)
    union = {k: sorted(set(c.sets[k]) | set(other.sets[k])) for k in c.sets}
    img = KC.image(union)
    dev, _ = KI.records(img)
    full = engine(issuers)
    full.known_import(c.image)
    f1, _ = check_query(full, img, c.sets)
    asked = np.zeros(len(dev), np.int64)
    engines = [engine(issuers) for r in range(world)]      # (the owner of a key depends on the issuer numbering)
    g = Group.local(engines)
    for r, er in enumerate(engines):
        st_imp = er.known_import(img, world=world, rank=r)
        fl, hf, st = query_both(full, img, world=world, rank=r)
        mine = fl != 2
        assert st["taken"] == int(mine.sum()) == st_imp["taken"] and st["hits"] == int((fl == 1).sum())
        assert (fl[mine] == f1[mine]).all()
        asked += mine
        # what the rank took, by its state: exactly the records it is asked about
        want = {}
        for (k, m), t in zip(dev, mine):
            if t:
                want.setdefault(k, []).append(m)
        assert KI.parse(er.known_export()).sets == want
        # … and it finds every one of them
        fl_r, _, st_r = query_both(er, img, world=world, rank=r)
        assert ((fl_r != 2) == mine).all() and (fl_r[mine] == 1).all() and st_r["hits"] == st_r["taken"]
    assert (asked == 1).all()
    for bad in ({"world": 0, "rank": 0}, {"world": world, "rank": world}):
        for call in (full.known_query, full.known_remove):
            with pytest.raises(ctmr.CtmrError) as ex:
                call(img, **bad)
            assert ex.value.code == N.E_INVAL
    # hand-over: every rank gives up what the others own; the group then holds each key once
    whole = [engine(issuers) for _ in range(world)]
    for r, er in enumerate(whole):
        er.known_import(img)
        for o in range(world):
            if o != r:
                er.known_remove(img, world=world, rank=o)
        assert state(er) == state(engines[r])
    g.close()
    for e in engines + whole + [full]:
        e.close()


# ---- 5. a query changes nothing

@pytest.mark.parametrize("bloom", [False, True])
def test_query_is_read_only(bloom, issuers, digests):
    e = engine(issuers, table_slots=1 << 12)
    g = None
    if bloom:
        g = Group.local([e])
        g.bloom_config(1 << 16)
    e.map_batch(synth.host_batch(CFG, 0, 1500))
    add_point_members(e, [e.issuer_id(k) for k in range(len(issuers))])
    c = KC.make("uniform", digests + [bytes(range(32))], HOURS[:2], [300, 301, 299], seed=37)
    imgs = [e.known_export(), c.image]
    before = (state(e), table(e), sorted_export(e))
    for img in imgs:
        for rpl_kw in ({}, {"world": 1, "rank": 0}):
            e.known_query(img, **rpl_kw)
            meta, rec = KC.split(img)
            e.known_query_device(meta, on_device(rec))
    assert (state(e), table(e), sorted_export(e)) == before
    if g:
        g.close()
    e.close()


# ---- 6. remove = replayed SetRemove

def replay_remove(e, img):
    dev, host = KI.records(img)
    return sum(e.set_remove(k, m) for k, m in dev), sum(e.set_remove(k, m) for k, m in host)


def with_repeats(img, seed=5):
    """Copies of records inside their set: next to the original, in another wave and in another 256-block."""
    meta, rec = KC.split(img)
    sets_of = KC.record_sets(img)
    rng = np.random.default_rng(seed)
    n = 0
    for s in np.unique(sets_of):
        at = np.nonzero(sets_of == s)[0]
        if len(at) < 8:
            continue
        src = int(at[0])
        for dst in (int(at[1]), int(at[len(at) // 2]), int(at[-1])) + tuple(int(x) for x in rng.choice(at[2:], 3)):
            rec[dst] = rec[src]
            n += 1
    assert n
    return meta + rec.tobytes()


def test_remove_equals_replayed_set_remove(issuers, digests):
    c = KC.make("interleaved", digests[:3] + [bytes(range(32))], HOURS[:2], [700, 300, 900, 130, 6], seed=23)
    tw = KC.make("twins", digests[:2], HOURS[:1], 0, seed=24)                # host members of 41..43 octets
    absent = KC.make("uniform", digests[:3], HOURS[:3], [200], seed=25)
    x, y = engine(issuers), engine(issuers, order=ORDER)
    for e in (x, y):
        e.known_import(c.image)
        e.known_import(tw.image)
        e.set_insert(sorted(c.sets)[0], b"\x99\x98")                        # a member no image names
    small = sorted(c.sets, key=lambda k: len(c.sets[k]))[0]
    assert len(c.sets[small]) == 6 and small in x.keys(b"serials::*")
    both = {k: c.sets.get(k, []) + tw.sets.get(k, []) for k in set(c.sets) | set(tw.sets)}
    held = dict(both)
    held[sorted(c.sets)[0]] = sorted(held[sorted(c.sets)[0]] + [b"\x99\x98"])
    # image 1: every second member, repeats inside sets, members nobody holds; the small set goes completely
    half = {k: v[::2] for k, v in both.items()}
    half[small] = list(both[small])
    for k, v in absent.sets.items():
        half[k] = sorted(set(half.get(k, [])) | set(v))
    img1 = with_repeats(KC.image(half))
    st = x.known_remove(img1)
    dev_hits, host_hits = replay_remove(y, img1)
    assert st["hits"] == dev_hits and st["host_hits"] == host_hits > 0 and st["taken"] == st["members"] > st["hits"] > 0
    assert state(x) == state(y)
    assert small not in x.keys(b"serials::*")
    left = KI.subtract(held, img1)
    assert KI.parse(x.known_export()).sets == left
    fl, hf = check_query(x, img1, left)
    assert not fl.any() and not hf.any()
    # image 2, the device variant: the rest; then nothing is left
    img2 = KC.image(held)
    meta, rec = KC.split(img2)
    st2 = x.known_remove_device(meta, on_device(rec))
    d2, h2 = replay_remove(y, img2)
    assert (st2["hits"], st2["host_hits"]) == (d2, h2)
    assert state(x) == state(y) and x.total_count() == 0 and x.keys(b"serials::*") == []
    assert x.known_remove(img2)["hits"] == 0
    x.close()
    y.close()


def bloom_group(issuers, world, mode):
    """`world` ranks that mapped overlapping shards of one log in a group round."""
    engines = [engine(issuers) for _ in range(world)]
    g = Group.local(engines)
    if mode == "bloom":
        g.bloom_config(1 << 16)
    b = synth.host_batch(CFG, 0, 2400)
    shards, keep, base = [], [], 0
    for r in range(world):
        lo, hi = shard_range(b.n, r, world)
        lo = max(0, lo - 300)                                              # the previous rank's tail again: duplicates
        sub = Batch.from_certs([b.cert(i) for i in range(lo, hi)], b.issuer_idx[lo:hi], b.entry_type[lo:hi])
        t = to_dev(sub)
        keep.append(t)
        shards.append(dev_shard(t, sub.n, order_base=base))
        base += sub.n
    g.map_batch(mode, shards)
    torch.cuda.synchronize()
    return g, engines


def union_sets(engines):
    out = {}
    for e in engines:
        for k, v in KI.parse(e.known_export()).sets.items():
            out.setdefault(k, set()).update(v)
    return {k: sorted(v) for k, v in out.items()}


def test_shadow_cells_are_removed_and_not_counted(issuers):
    ga, a = bloom_group(issuers, 2, "bloom")
    gb, b = bloom_group(issuers, 2, "bloom")
    img = KI.build(union_sets(a))
    n = KI.parse(img).n_members
    total = ga.total_count()
    assert total == n
    shadow = 0
    for r in (0, 1):
        fl, _, st = a[r].known_query(img)
        exported = sum(len(v) for v in KI.parse(a[r].known_export()).sets.values())
        shadow += int(fl.sum()) - exported                                  # held for dedup, counted by the other rank
        st_rm = a[r].known_remove(img)
        dev_hits, _ = replay_remove(b[r], img)
        assert st_rm["hits"] == dev_hits == int(fl.sum())
        assert (a[r].issuer_counts() == b[r].issuer_counts()).all()
        assert state(a[r]) == state(b[r])
    assert shadow > 0 and ga.total_count() == gb.total_count() == 0
    for g in (ga, gb):
        g.close()
    for e in a + b:
        e.close()


# ---- 7. tombstones, chains, rebuilds

def test_tombstones_and_chains(issuers, digests):
    c = KC.make("uniform", digests, HOURS[:1], [480], seed=51)
    assert c.members == 6 * 480
    e = engine(issuers, table_slots=1 << 12)                               # load 0.70: long chains, no rebuild yet
    t0 = e.table_info()
    e.known_import(c.image)
    assert e.table_info().rebuilds == t0.rebuilds and e.table_info().slots == 1 << 12
    gone = {k: v[::2] for k, v in c.sets.items()}
    img_gone = KC.image(gone)
    st = e.known_remove(img_gone)
    assert st["hits"] == st["taken"] == c.members // 2
    left = KI.subtract(c.sets, img_gone)
    fl, _ = check_query(e, c.image, left, replay=True)                     # the others now sit behind tombstones
    assert fl.sum() == c.members // 2
    assert e.table_info().rebuilds == t0.rebuilds and e.table_info().occupied == c.members
    # the removed members again: new again, across the rebuild their tombstones force
    st = e.known_import(img_gone)
    assert st["inserted"] == c.members // 2 and e.table_info().rebuilds > t0.rebuilds
    fl, _ = check_query(e, c.image, c.sets)
    assert fl.all()
    e.close()


def test_across_arena_compactions(issuers):
    cfg = synth.config(seed=31, n_issuers=6, dup_permille=100)
    e = ctmr.Engine(device=0, table_slots=1 << 13, pair_slots=1 << 14)     # arena: 4 096 cells to begin with
    e.add_issuers(synth.issuers(cfg))
    e.set_filter(b"", True, synth.BASE_TIME)
    b = synth.host_batch(cfg, 0, 1500)
    e.map_batch(b)
    img = e.known_export()
    held = KI.parse(img).sets
    half = {k: v[::2] for k, v in held.items()}
    assert e.known_remove(KI.build(half))["hits"] == sum(len(v) for v in half.values())
    c0 = e.table_info().arena_compactions
    for _ in range(8):
        e.map_batch(b)                                                      # the removed ones are new once, then known
    assert e.table_info().arena_compactions > c0
    fl, hf = check_query(e, img, held)
    assert fl.all()
    st = e.known_remove(img)
    assert st["hits"] == st["taken"] and e.total_count() == 0
    e.close()


# ---- 8. rejection

def damaged(img, edit):
    meta, rec = KC.split(img)
    edit(rec)
    return meta + rec.tobytes()


def test_rejection_and_small_buffers(issuers, digests, monkeypatch):
    c = KC.make("uniform", digests, HOURS[:2], [300, 301, 299], seed=37)
    n = c.members
    assert n % 256 not in (0, 1)
    e = engine(issuers)
    e.known_import(c.image)
    e.set_insert(sorted(c.sets)[0], b"\x05" * 44)
    before = (state(e), table(e))
    lens = KC.record_lens(c.image)
    _, _, _, n_iss, _, n_sets, _, _, _, _ = KI._HEADER.unpack_from(c.image, 0)
    so = 64 + 32 * n_iss
    bad = []
    for i in (0, n - 1):
        bad.append(damaged(c.image, lambda rec: rec["len"].__setitem__(i, 41)))
        for edge in (8, 16, 24, 32, 39):
            if lens[i] <= edge:
                bad.append(damaged(c.image, lambda rec: rec["serial"].__setitem__((i, edge), 1)))
    at = int(np.nonzero(lens < 16)[0][-1])
    bad.append(damaged(c.image, lambda rec: rec["serial"].__setitem__((at, 16), 0x80)))
    magic = bytearray(c.image)
    magic[0] ^= 1
    gap = bytearray(c.image)
    struct.pack_into("<Q", gap, so + 24 + 8, struct.unpack_from("<Q", c.image, so + 24 + 8)[0] + 1)
    ordinal = bytearray(c.image)
    struct.pack_into("<I", ordinal, so + 4, n_iss)
    bad += [bytes(magic), bytes(gap), bytes(ordinal)]
    for chunk in (None, 200):
        if chunk:
            monkeypatch.setenv("CTMR_KNOWN_PROBE_CHUNK", str(chunk))         # the damaged last record: in the last chunk
        for img in bad:
            meta, rec = KC.split(img)
            for call in (lambda: e.known_query(img), lambda: e.known_remove(img),
                         lambda: e.known_query_device(meta, on_device(rec)),
                         lambda: e.known_remove_device(meta, on_device(rec))):
                with pytest.raises(ctmr.CtmrError) as ex:
                    call()
                assert ex.value.code == N.E_INVAL
            assert (state(e), table(e)) == before
    monkeypatch.delenv("CTMR_KNOWN_PROBE_CHUNK")
    # flags buffers one byte short: CTMR_E_RANGE, the sizes in the stats, nothing written
    tw = KC.make("twins", digests[:2], HOURS[:1], 0, seed=24)
    im = KI.parse(tw.image)
    lib = N.lib()
    for short_dev, short_host in ((1, 0), (0, 1)):
        fl = np.full(im.n_members + 2 * GUARD, 0xA5, np.uint8)
        hf = np.full(im.n_host_members + 2 * GUARD, 0xA5, np.uint8)
        st = N.KnownProbeStats()
        rc = lib.ctmr_known_query(e._h, tw.image, len(tw.image), 1, 0, fl.ctypes.data + GUARD, im.n_members - short_dev,
                                  hf.ctypes.data + GUARD, im.n_host_members - short_host, C.byref(st))
        assert rc == N.E_RANGE and (fl == 0xA5).all() and (hf == 0xA5).all()
        assert st.members == im.n_members and st.host_members == im.n_host_members
        meta, rec = KC.split(tw.image)
        d, dfl = on_device(rec), torch.full((im.n_members + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        rc = lib.ctmr_known_query_device(e._h, meta, len(meta), C.c_void_p(d.data_ptr()), im.n_members, 1, 0,
                                         C.c_void_p(dfl.data_ptr() + GUARD), im.n_members - short_dev,
                                         hf.ctypes.data + GUARD, im.n_host_members - short_host, C.byref(st))
        assert rc == N.E_RANGE and (dfl == 0xA5).all() and (hf == 0xA5).all()
    # exact buffers: the guards stay
    fl = np.full(im.n_members + 2 * GUARD, 0xA5, np.uint8)
    hf = np.full(im.n_host_members + 2 * GUARD, 0xA5, np.uint8)
    st = N.KnownProbeStats()
    assert lib.ctmr_known_query(e._h, tw.image, len(tw.image), 1, 0, fl.ctypes.data + GUARD, im.n_members,
                                hf.ctypes.data + GUARD, im.n_host_members, C.byref(st)) == 0
    for buf in (fl, hf):
        assert (buf[:GUARD] == 0xA5).all() and (buf[-GUARD:] == 0xA5).all() and (buf[GUARD:-GUARD] <= 1).all()
    assert (state(e), table(e)) == before
    e.close()


# ---- 9. chunks

@pytest.mark.parametrize("chunk", [300, 257])
def test_chunks_give_the_same_answers(chunk, issuers, digests, monkeypatch):
    c = KC.make("runs", digests, HOURS[:2], [1800, 1, 255, 256, 257, 700], seed=61)
    other = KC.make("runs", digests, HOURS[:2], [500], seed=62)
    union = {k: sorted(set(c.sets[k]) | set(other.sets[k])) for k in c.sets}
    img = KC.image(union)
    x, y = engine(issuers), engine(issuers)
    for e in (x, y):
        e.known_import(c.image)
        add_point_members(e, [e.issuer_id(k) for k in range(len(issuers))])
    own = x.known_export()
    plain = [query_both(x, i) for i in (img, own)]
    monkeypatch.setenv("CTMR_KNOWN_PROBE_CHUNK", str(chunk))
    for rpl in RPLS:
        monkeypatch.setenv("CTMR_KNOWN_PROBE_RPL", str(rpl))
        for i, (fl, hf, st) in zip((img, own), plain):
            fl2, hf2, st2 = query_both(x, i)
            assert (fl2 == fl).all() and (hf2 == hf).all() and st2 == st
    check_query(x, img, c.sets)
    # a member named in two chunks is removed once
    half = with_repeats(KC.image({k: v[::2] for k, v in union.items()}))
    meta, rec = KC.split(half)
    sets_of = KC.record_sets(half)
    big = np.nonzero(sets_of == np.bincount(sets_of).argmax())[0]
    assert len(big) > 2 * chunk
    rec[big[-1]] = rec[big[0]]                                              # far apart: in different chunks
    assert big[-1] // chunk != big[0] // chunk
    half = meta + rec.tobytes()
    st = x.known_remove(half)
    monkeypatch.delenv("CTMR_KNOWN_PROBE_CHUNK")
    monkeypatch.delenv("CTMR_KNOWN_PROBE_RPL")
    st_plain = y.known_remove(half)
    assert st == st_plain and st["hits"] == len({(k, m) for k, m in KI.records(half)[0] if m in set(c.sets[k])})
    assert state(x) == state(y)
    x.close()
    y.close()


# ---- 10. groups

@pytest.mark.parametrize("mode", ["owner", "bloom"])
@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_group_query_and_remove(world, mode, issuers):
    g, engines = bloom_group(issuers, world, mode)
    sets = union_sets(engines)
    img = KI.build(sets)
    assert g.total_count() == sum(len(v) for v in sets.values()) > 1000
    fl, hf = g.known_query(img)
    assert fl.all() and len(fl) == KI.parse(img).n_members and hf.all()
    g.known_remove(img)
    fl, hf = g.known_query(img)
    assert not fl.any() and not hf.any() and g.total_count() == 0
    assert all(e.keys(b"serials::*") == [] for e in engines)
    g.close()
    for e in engines:
        e.close()
