"""-m gpu: the known-set image and the per-issuer lists (kernels/image.h, kernels/lists.h) at every
serial length.  The synthetic corpus has serials of 16 or 17 octets; here the sets come from tests/known_corpus.py
(lengths 0..40 in several mixes, twins that differ in length alone, 41..60-octet host members) and from hand-built
certificates, and every result is compared exactly with the CPU twin (known_image) over the dict the test built.

What each test is for:
  test_import_state_export, test_import_twice, test_import_equals_set_insert_in_both_classes, test_duplicate_records,
  test_large_uniform_grows_and_passes_one_scan_tile — k_known_pack's 64-byte branch and the KeyRec insert, resolve and
      Bloom passes behind it; key identity by length (the twins mix);
  test_rejected_* and test_accepting_edges — the padding and serial_len checks of known_record at every word edge;
  test_lists_*, test_exact_buffers_*, test_chunk_sizes, test_host_store_pieces_* — k_lists_write at every line length
      and phase, the head >= total return, stores between the ragged ends, the points;
  test_export_many_sets_per_wave_and_one_dominant_set — both position paths of k_known_export;
  test_warm_restart_with_long_serials — imported 21..40-octet keys looked up by the map, alone and through a group.
Known gap: an import of more than KNOWN_CHUNK = 1 << 27 records (engine/image.inc) takes a second chunk; reaching it
needs a 6 GiB image or a test-only switch in the library, so that path stays untested here.
"""
import base64
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr
from ct_mapreduce_amd import known_image as KI, synth, _native as N
from ct_mapreduce_amd.distributed import Group, shard_range
from ct_mapreduce_amd.engine import Batch, RECORD_DTYPE
from tests import der as D, known_corpus as KC
from tests.gpu_common import run_oracle
from tests.test_gpu_exchange import to_dev, dev_shard, DEV
from tests.test_gpu_known_image import engine, state, UNREG_ID
from tests.test_gpu_known_lists import lines, check, block_canon, canon

CFG = synth.config(seed=91, n_issuers=6)
ORDER = [5, 3, 1, 0, 2, 4]
# 490999 = 2026-01-05-07 and 491016 = 2026-01-06-00: an hour with a one-digit spelling and the first hour of a day
HOURS = [490999, 491000, 491016, 491040]
SIZES = {"uniform": [900, 1, 255, 256, 257, 40, 3000], "tiny": [400, 1, 255, 256, 257, 2, 3, 700],
         "interleaved": [700, 1, 255, 256, 257, 130, 2000], "runs": [1800, 1, 255, 256, 257, 3100], "twins": 0}
CHUNKS = (1, 2, 7, 63, 64, 65, 255, 256, 257, 4097)
GUARD = 64


@pytest.fixture(scope="module")
def issuers():
    return synth.issuers(CFG)


@pytest.fixture(scope="module")
def digests(issuers):
    e = engine(issuers)
    out = [base64.urlsafe_b64decode(e.issuer_id(k)) for k in range(len(issuers))]
    e.close()
    assert len(set(out)) == 6
    return out


def on_device(rec):
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1).copy()).to(DEV)


def import_device(e, img, **kw):
    meta, rec = KC.split(img)
    return e.known_import_device(meta, on_device(rec), **kw)


def expected_state(sets, digests):
    """test_gpu_known_image.state() of an engine that holds exactly `sets` (keys of registered issuers only)."""
    by_id = {KI.issuer_id(d): 0 for d in digests}
    for k, v in sets.items():
        by_id[k.split(b"::")[2]] += len(v)
    return {"keys": sorted(sets), "lists": {k: sorted(v) for k, v in sets.items()}, "card": {k: len(v) for k, v in sets.items()},
            "by_id": by_id, "total": sum(len(v) for v in sets.values())}


def table(e):
    return tuple(getattr(e.table_info(), f) for f, _ in N.TableInfo._fields_)


@pytest.fixture(scope="module", params=KC.MIXES)
def loaded(request, issuers, digests):
    """One corpus per mix in two engines: `a` took the image from the host, `b` (issuers registered in another order)
    from the device."""
    mix = request.param
    c = KC.make(mix, digests, HOURS, SIZES[mix], seed=17)
    assert not c.capped
    a, b = engine(issuers), engine(issuers, order=ORDER)
    st_a, st_b = a.known_import(c.image), import_device(b, c.image)
    yield mix, c, a, b, st_a, st_b
    a.close()
    b.close()


# ---- 1. import, state and export

def test_import_state_export(loaded, digests):
    mix, c, a, b, st_a, st_b = loaded
    im = KI.parse(c.image)
    assert im.sets == c.sets
    lens = KC.record_lens(c.image)
    assert mix == "tiny" or ((lens <= 20).any() and (lens > 20).any())   # both record classes
    want = expected_state(c.sets, digests)
    for e, st in ((a, st_a), (b, st_b)):
        assert st["members"] == st["taken"] == st["inserted"] == im.n_members and st["known"] == 0
        assert st["host_members"] == st["host_inserted"] == im.n_host_members
        assert (im.n_host_members > 0) == (mix == "twins")
        got = state(e)
        for f in ("total", "by_id", "keys", "card"):
            assert got[f] == want[f], f
        for k in want["keys"]:
            assert got["lists"][k] == want["lists"][k], k
        assert e.table_info().occupied == im.n_members
    # export: the same sets; the meta part (header, issuers in digest order, sets in key order, the host section in
    # (key, member) order) is the canonical one byte for byte — only the order of the records inside a set is free
    meta = KC.split(KI.build(c.sets))[0]
    assert meta == KC.split(c.image)[0]
    for e in (a, b):
        img = e.known_export()
        assert img[:len(meta)] == meta and len(img) == len(c.image)
        assert KI.parse(img).sets == c.sets
        m2, d = e.known_export_device()
        assert m2 == meta
        assert KI.parse(m2 + d.cpu().numpy().tobytes()).sets == c.sets


def test_import_twice(loaded):
    mix, c, a, b, st_a, st_b = loaded
    for e, imp in ((a, lambda: a.known_import(c.image)), (b, lambda: import_device(b, c.image))):
        t0, s0 = e.table_info(), state(e)
        st = imp()
        t1 = e.table_info()
        assert st["inserted"] == 0 and st["known"] == st["taken"] == st_a["taken"] and st["host_inserted"] == 0
        assert t1.occupied == t0.occupied and t1.arena_used - t0.arena_used <= st["taken"]
        assert state(e) == s0


@pytest.mark.parametrize("mix", ["interleaved", "twins"])
def test_import_equals_set_insert_in_both_classes(mix, issuers, digests):
    c = KC.make(mix, digests[:3], HOURS[:2], [700, 300, 900, 130], seed=23)
    pairs = [(k, m) for k in sorted(c.sets) for m in c.sets[k]]
    assert 1500 < len(pairs) or mix == "twins"
    x, y = engine(issuers), engine(issuers, order=ORDER)
    for e in (x, y):
        for k, m in pairs[::3]:
            e.set_insert(k, m)
        e.set_insert(pairs[0][0], b"\x99\x98")
    st = x.known_import(c.image)
    new = sum(y.set_insert(k, m) for k, m in pairs)
    assert st["inserted"] + st["host_inserted"] == new == len(pairs) - len(pairs[::3])
    assert st["known"] == st["taken"] - st["inserted"]
    assert state(x) == state(y)
    assert x.table_info().occupied == y.table_info().occupied
    x.close()
    y.close()


def test_duplicate_records(issuers, digests):
    """k copies of one record inside a set, in both classes and at both sides of 20/21, some in other 256-blocks."""
    rng = np.random.default_rng(29)
    base = KC.make("uniform", digests[:2], HOURS[:2], [600, 300], seed=29)
    meta, rec = KC.split(base.image)
    sets_of = KC.record_sets(base.image)
    # a hand-built set 0: 600 records of which many are copies
    special = [b"\x11" * 20, b"\x11" * 20 + b"\x00", b"\x22" * 40, b"", b"\x00", b"\x33" * 21, b"\x33" * 20]
    n0 = int((sets_of == 0).sum())
    assert n0 == 600
    own = [bytes(r["serial"][:int(r["len"])]) for r in rec[:n0]]
    members = list(own[:200])
    for s in special:
        members += [s] * 5
    members += own[:100] + own[50:150]                                  # 200 copies, far from their originals
    members += [own[7]] * (n0 - len(members))
    order = rng.permutation(n0)
    members = [members[i] for i in order]
    first_at = {}
    for i, m in enumerate(members):
        first_at.setdefault(m, []).append(i)
    assert any(max(v) // 256 != min(v) // 256 for v in first_at.values())   # copies in different 256-blocks
    for i, m in enumerate(members):
        rec["len"][i] = len(m)
        rec["serial"][i] = np.frombuffer(m.ljust(40, b"\0"), np.uint8)
    img = meta + rec.tobytes()
    want = dict(base.sets)
    want[sorted(want)[0]] = sorted(set(members))
    distinct = sum(len(v) for v in want.values())
    for dev in (False, True):
        e = engine(issuers)
        st = import_device(e, img) if dev else e.known_import(img)
        assert st["taken"] == st["members"] == len(rec) and st["inserted"] == distinct < len(rec)
        assert st["known"] == len(rec) - distinct
        assert state(e) == expected_state(want, digests)
        assert e.table_info().occupied == distinct
        assert KI.parse(e.known_export()).sets == want
        e.close()


def test_large_uniform_grows_and_passes_one_scan_tile(issuers, digests):
    """About 1.2 M members, the table started small.  kernels/reduce.h: SCAN_TILE = 4096 — the import scans 2·nb + 1
    block counts and the lists nb + 1, nb = ceil(members / 256): both pass one tile when members > 4095 · 256."""
    c = KC.make("uniform", digests, [491000 + 3 * k for k in range(8)], 25000, seed=31)
    n = c.members
    assert n == 48 * 25000 > 4095 * 256 and (n + 255) // 256 + 1 > 4096
    e = engine(issuers, table_slots=1 << 10)
    t0 = e.table_info()
    st = e.known_import(c.image)
    t1 = e.table_info()
    assert st["taken"] == st["inserted"] == n and st["known"] == 0
    assert t1.rebuilds > t0.rebuilds and t1.occupied == n and t1.arena_used - t0.arena_used <= n
    assert e.total_count() == n
    want = expected_state(c.sets, digests)
    assert sorted(e.keys(b"serials::*")) == want["keys"]
    by_id = {e.issuer_info(k).issuer_id: int(v) for k, v in enumerate(e.issuer_counts())}
    assert by_id == want["by_id"]
    for k in want["keys"][::5]:
        assert e.set_cardinality(k) == 25000 and e.set_list(k) == c.sets[k], k
    assert KI.parse(e.known_export()).sets == c.sets
    got = e.known_lists(0)
    assert sum(len(t) for _, t in got) == int((2 * KC.record_lens(c.image) + 1).sum())
    assert block_canon(got, c.sets, 0) == block_canon(KI.lists_of_sets(c.sets, 0), c.sets, 0)
    # the device path into a second engine, then again: nothing is new
    b = engine(issuers, order=ORDER, table_slots=1 << 10)
    meta, rec = KC.split(c.image)
    t = on_device(rec)
    assert b.known_import_device(meta, t)["inserted"] == n
    again = b.known_import_device(meta, t)
    assert again["inserted"] == 0 and again["known"] == n and b.table_info().occupied == n
    for k in want["keys"][2::7]:
        assert b.set_list(k) == c.sets[k], k
    e.close()
    b.close()


# ---- 2. rejection

@pytest.fixture(scope="module")
def victim(issuers):
    """An engine that holds other members; every refused import must leave it as it is."""
    e = engine(issuers)
    e.map_batch(synth.host_batch(CFG, 0, 400))
    e.set_insert("serials::%s::%s" % (KI.exp_date_id(491000).decode(), e.issuer_id(0)), b"\x05" * 44)
    yield e
    e.close()


@pytest.fixture(scope="module")
def valid(digests):
    """uniform over the six registered issuers and one nobody registered; 300 · 14 + … records: a final partial block."""
    c = KC.make("uniform", digests + [bytes(range(32))], HOURS[:2], [300, 301, 299], seed=37)
    assert c.members % 256 not in (0, 1)
    return c


def refused(e, img, what, **kw):
    before = (state(e), table(e))
    with pytest.raises(KI.ImageError, match=what):
        KI.parse(img)
    with pytest.raises(ctmr.CtmrError, match=what) as ex:
        e.known_import(img, **kw)
    assert ex.value.code == N.E_INVAL
    with pytest.raises(ctmr.CtmrError, match=what) as ex:
        import_device(e, img, **kw)
    assert ex.value.code == N.E_INVAL
    assert (state(e), table(e)) == before


def damaged(c, edit):
    meta, rec = KC.split(c.image)
    edit(rec)
    return meta + rec.tobytes()


def pick(rec, length, k=0):
    at = np.nonzero(rec["len"] == length)[0]
    return int(at[k % len(at)])


@pytest.mark.parametrize("length,index", [(L, L) for L in (0, 1, 7, 8, 9, 15, 16, 17, 20, 21, 24, 31, 32, 33, 39)]
                         + [(0, 39), (38, 39)])
def test_rejected_padding(victim, valid, length, index):
    def edit(rec):
        rec["serial"][pick(rec, length, 3), index] = 0x01
    refused(victim, damaged(valid, edit), "padding")
    def edit_top(rec):                                                   # the highest bit of that octet alone
        rec["serial"][pick(rec, length), index] = 0x80
    refused(victim, damaged(valid, edit_top), "padding")


@pytest.mark.parametrize("value", [41, 255, 1 << 32, (1 << 32) | 5, 2 ** 64 - 1])
def test_rejected_serial_len(victim, valid, value):
    def edit(rec):
        i = pick(rec, 5, 1)
        rec["len"][i] = value
        if value == 1 << 32:                     # low word zero: a valid empty serial, were the upper word not read
            rec["serial"][i] = 0
    refused(victim, damaged(valid, edit), "serial_len")


def test_rejected_wherever_the_record_is(victim, valid, issuers, digests):
    meta, rec0 = KC.split(valid.image)
    n = len(rec0)
    unreg = np.nonzero(KC.record_sets(valid.image) == [k.split(b"::")[2] for k in sorted(valid.sets)].index(UNREG_ID.encode()))[0]
    assert len(unreg) and n % 256 > 1
    for i in (0, n - 1, 63, 127, 256 * (n // 256) + 1, int(unreg[0]), int(unreg[-1])):
        def edit(rec):
            if rec["len"][i] < 40:
                rec["serial"][i, 39] = 0x40
            else:
                rec["len"][i] = 41
        refused(victim, damaged(valid, edit), "padding" if rec0["len"][i] < 40 else "serial_len")
    # both kinds in one image: the serial_len message
    def both(rec):
        rec["serial"][pick(rec, 12), 12] = 1
        rec["len"][pick(rec, 30)] = 41
    refused(victim, damaged(valid, both), "serial_len")
    # world = 2 (every issuer registered there): the bad record belongs to one rank and is refused on both
    reg = KC.make("uniform", digests, HOURS[:2], [300, 301], seed=41)
    for what, edit in (("padding", lambda rec: rec["serial"].__setitem__((pick(rec, 21), 21), 1)),
                       ("serial_len", lambda rec: rec["len"].__setitem__(pick(rec, 9), 41))):
        for rank in (0, 1):
            refused(victim, damaged(reg, edit), what, world=2, rank=rank)
    # the library stays usable: the undamaged images go in
    e = engine(issuers)
    st = e.known_import(valid.image)
    assert st["inserted"] == st["taken"] == n
    assert KI.parse(e.known_export()).sets == valid.sets
    stats = [victim.known_import(reg.image, world=2, rank=r) for r in (0, 1)]
    assert sum(s["inserted"] for s in stats) == reg.members and all(s["inserted"] for s in stats)
    e.close()


def test_accepting_edges(issuers, digests):
    key = KI.set_key(491000, digests[0])
    sets = {key: [b"", b"\xff" * 40, b"\x00" * 40, b"\xff" * 20, b"\xff" * 21]}
    img = KI.build(sets)
    meta, rec = KC.split(img)
    assert sorted(rec["len"].tolist()) == [0, 20, 21, 40, 40] and (rec["serial"][rec["len"] == 0] == 0).all()
    e = engine(issuers)
    assert e.known_import(img)["inserted"] == 5 and import_device(e, img)["known"] == 5
    assert e.set_list(key) == sorted(sets[key])
    assert sorted(lines(dict(e.known_lists(0))[KI.issuer_id(digests[0])])) == sorted(m.hex().encode() for m in sets[key])
    e.close()


# ---- 3. lists

def text_bytes(sets, now):
    return sum(2 * len(m) + 1 for _, bl in KI.list_blocks(sets, now) for _, ms in bl for m in ms)


def device_lists(e, now):
    ids, toff, t = e.known_lists_device(now)
    tb = t.cpu().numpy().tobytes()
    assert toff[-1] == len(tb)
    return [(i, tb[toff[k]:toff[k + 1]]) for k, i in enumerate(ids)]


def same_lists(got, sets, now):
    ref = KI.lists_of_sets(sets, now)
    check(got, sets, now)
    assert block_canon(got, sets, now) == block_canon(ref, sets, now)
    assert [len(t) for _, t in got] == [len(t) for _, t in ref]
    assert sum(len(t) for _, t in got) == text_bytes(sets, now)


def test_lists_at_every_length_and_cut(loaded):
    mix, c, a, b, st_a, st_b = loaded
    before = [(state(e), table(e)) for e in (a, b)]
    end = (HOURS[1] + 1) * 3600
    for now in (0, HOURS[1] * 3600 + 1800, end - 1, end, (HOURS[-1] + 1) * 3600):
        for e in (a, b):
            same_lists(e.known_lists(now), c.sets, now)
            same_lists(device_lists(e, now), c.sets, now)
    assert a.known_lists((HOURS[-1] + 1) * 3600) == []
    assert text_bytes(c.sets, end - 1) > text_bytes(c.sets, end) > 0
    got = dict(a.known_lists(0))
    if mix in ("uniform", "tiny", "twins"):                               # the empty serial: a bare newline, counted
        assert sum(lines(t).count(b"") for t in got.values()) == sum(b"" in v for v in c.sets.values()) > 0
    if mix == "twins":
        for ident, t in got.items():
            ls = lines(t)
            assert ls.count(b"") == ls.count(b"00") == ls.count(b"0000") == len(HOURS)
            assert {len(x) // 2 for x in ls} >= {20, 21, 40, 41, 42, 43}
        # the 41..43-octet twins are host-store lines, at their expDate's place (check() holds them to their block)
        assert a.known_lists_raw(0)[4].host_members == KI.parse(c.image).n_host_members > 0
    assert [(state(e), table(e)) for e in (a, b)] == before


def raw_lists(e, now, device, ptr, cap):
    info = N.KnownListsInfo()
    ids = np.zeros(1 << 12, np.uint8)
    offs = np.zeros(64, np.uint64)
    fn = e._lib.ctmr_known_lists_device if device else e._lib.ctmr_known_lists
    rc = fn(e._h, now, C.c_void_p(ptr), cap, ids.ctypes.data, ids.nbytes, offs.ctypes.data, offs.size, C.byref(info))
    return rc, info, ids, offs


def split_text(text, info, ids, offs):
    g = info.issuers
    idb = ids.tobytes()
    return [(idb[int(offs[g + 1 + k]):int(offs[g + 2 + k])], text[int(offs[k]):int(offs[k + 1])]) for k in range(g)]


def test_exact_buffers_with_guards_at_every_phase(loaded):
    mix, c, a, b, st_a, st_b = loaded
    now = 0
    roomy = a.known_lists(now)
    want = block_canon(roomy, c.sets, now)
    rc, info, _, _ = raw_lists(a, now, False, 0, 0)                       # the sizing call
    assert rc == N.E_RANGE and info.text_bytes == text_bytes(c.sets, now) == sum(len(t) for _, t in roomy)
    tb = int(info.text_bytes)
    buf = np.full(tb + 2 * GUARD, 0xEE, np.uint8)
    rc, info, ids, offs = raw_lists(a, now, False, buf.ctypes.data + GUARD, tb)
    assert rc == 0 and (buf[:GUARD] == 0xEE).all() and (buf[GUARD + tb:] == 0xEE).all()
    assert block_canon(split_text(buf[GUARD:GUARD + tb].tobytes(), info, ids, offs), c.sets, now) == want
    for e in (a, b):
        for shift in range(16):
            t = torch.full((256 + tb + 2 * GUARD + 16,), 0xEE, dtype=torch.uint8, device=DEV)
            pad = (-t.data_ptr()) % 256
            lo = pad + GUARD + shift                                      # 64 + shift past a 256-byte boundary
            view = t[lo:lo + tb]
            assert view.data_ptr() % 16 == shift
            rc, info, ids, offs = raw_lists(e, now, True, view.data_ptr(), tb)
            assert rc == 0 and info.text_bytes == tb
            h = t.cpu().numpy()
            assert (h[:lo] == 0xEE).all() and (h[lo + tb:] == 0xEE).all(), shift
            assert block_canon(split_text(h[lo:lo + tb].tobytes(), info, ids, offs), c.sets, now) == want, shift


@pytest.mark.parametrize("chunk", CHUNKS)
def test_chunk_sizes(loaded, chunk, monkeypatch):
    mix, c, a, b, st_a, st_b = loaded
    sizes = sorted(len([m for m in v if len(m) <= 40]) for v in c.sets.values())
    if mix != "twins":
        assert {1, 255, 256, 257} <= set(sizes)
    ref = block_canon(KI.lists_of_sets(c.sets, 0), c.sets, 0)
    monkeypatch.setenv("CTMR_KNOWN_LISTS_CHUNK", str(chunk))
    for e in (a, b):
        assert block_canon(e.known_lists(0), c.sets, 0) == ref
        same_lists(device_lists(e, 0), c.sets, 0)
    # exactly sized, guarded, unaligned device buffer: every chunk's first block has a phase of its own
    tb = text_bytes(c.sets, 0)
    t = torch.full((tb + 2 * GUARD + 32,), 0xEE, dtype=torch.uint8, device=DEV)
    lo = GUARD + (-t.data_ptr()) % 16 + 5
    rc, info, ids, offs = raw_lists(a, 0, True, t[lo:].data_ptr(), tb)
    h = t.cpu().numpy()
    assert rc == 0 and (h[:lo] == 0xEE).all() and (h[lo + tb:] == 0xEE).all()
    assert block_canon(split_text(h[lo:lo + tb].tobytes(), info, ids, offs), c.sets, 0) == ref


def test_host_store_pieces_between_device_records(issuers, digests, monkeypatch):
    """Host-store lines between device records, with the points (list starts and host pieces) at the first lane of a
    wave, the last lane, mid-wave, several in one wave, and behind the last device record."""
    rng = np.random.default_rng(43)
    reg = sorted(KI.issuer_id(d) for d in digests)
    hours = HOURS[:3]
    # device sets in list order (Issuer.ID, then hour) and their sizes: the cumulative sums are the points
    sizes = [64, 63, 1, 30, 2, 1, 1, 1, 129, 255, 256, 257, 3, 700, 5, 190, 64, 64]
    list_keys = [b"serials::" + KI.exp_date_id(h) + b"::" + i for i in reg for h in hours]
    assert len(list_keys) == len(sizes)
    sets = {k: KC._random_members(rng, s, tuple(range(41))) for k, s in zip(list_keys, sizes)}
    cum = np.concatenate([[0], np.cumsum(sizes)])
    n_dev = int(cum[-1])
    host = {}
    for j, k in enumerate(list_keys):
        if j % 3 != 2 or j == len(list_keys) - 1:                         # the same key also holds 41..60-octet members
            host[k] = [bytes(rng.integers(0, 256, size=int(L), dtype=np.uint8).tolist()) for L in rng.integers(41, 61, size=1 + j % 3)]
    pts = sorted({int(cum[j + 1]) for j, k in enumerate(list_keys) if k in host} | {int(cum[3 * g]) for g in range(6)})
    assert any(p % 64 == 0 for p in pts) and any(p % 64 == 63 for p in pts) and any(5 < p % 64 < 60 for p in pts)
    assert n_dev in pts and max(np.bincount(np.asarray(pts) // 64)) >= 3
    day = KI.exp_date_id(491016)[:10]
    extra = {
        b"serials::" + day + b"::" + reg[1]: [b"\x01\x02", b""],          # day resolution: the first second of hour 491016
        b"serials::2026-01-05-7::" + reg[2]: [b"\x07", b"\x07" * 41],     # one-digit hour: the second of 490999
        b"serials::2026-01-05-7::" + reg[5]: [b"\x77" * 40],
        b"serials::" + KI.exp_date_id(491000) + b"::-before": [b"\x0a", b"\x0b" * 50],
        b"serials::" + KI.exp_date_id(491000) + b"::" + reg[2] + b"x": [b"\x0c" * 3],
        b"serials::" + KI.exp_date_id(491016) + b"::" + reg[2] + b"x": [b"\x0c" * 4, b""],
        b"serials::" + KI.exp_date_id(491000) + b"::zzzz-after": [b"\x0d" * 60, b"\x0e"],
        b"serials::" + KI.exp_date_id(491000) + b"::" + UNREG_ID.encode(): [b"\x0f" * 7],
    }
    assert b"-before" < reg[0] and reg[2] < reg[2] + b"x" < reg[3] and reg[5] < b"zzzz-after"
    whole = {k: sorted(v + host.get(k, [])) for k, v in sets.items()}
    whole.update({k: sorted(v) for k, v in extra.items()})
    e = engine(issuers)
    assert e.known_import(KC.image(sets))["inserted"] == n_dev
    for k in list(host) + list(extra):
        for m in (host.get(k) or extra[k]):
            assert e.set_insert(k, m)
    assert {k: e.set_list(k) for k in e.keys(b"serials::*")} == whole
    before = (state(e), table(e))
    ref = KI.lists_of_sets(whole, 0)
    assert len(ref) == 6 + 4
    for chunk in (None,) + CHUNKS:
        if chunk is None:
            monkeypatch.delenv("CTMR_KNOWN_LISTS_CHUNK", raising=False)
        else:
            monkeypatch.setenv("CTMR_KNOWN_LISTS_CHUNK", str(chunk))
        for now in (0, 491000 * 3600, (491016 + 1) * 3600):
            same_lists(e.known_lists(now), whole, now)
            same_lists(device_lists(e, now), whole, now)
        text, ids, toff, ioff, info = e.known_lists_raw(0)
        assert list(toff) == list(np.cumsum([0] + [len(t) for _, t in ref])) and info.members == n_dev
        assert info.host_members == sum(len(v) for v in host.values()) + sum(len(v) for v in extra.values())
        assert list(device_lists(e, 0)) and list(e.known_lists_device(0)[1]) == list(toff)
    assert (state(e), table(e)) == before
    e.close()


# ---- 4. export with many sets per wave and one dominant set

def test_export_many_sets_per_wave_and_one_dominant_set(issuers, digests, monkeypatch):
    hours = [491000 + k for k in range(520)]
    sizes = [1, 2, 3] * (6 * 520 // 3)
    sizes[1700] = 200_000
    c = KC.make("uniform", digests, hours, sizes, seed=47)
    assert len(c.sets) >= 3000 and max(len(v) for v in c.sets.values()) >= 200_000 and not c.capped
    assert sum(1 for v in c.sets.values() if len(v) <= 3) == len(c.sets) - 1
    e = engine(issuers, table_slots=1 << 19, pair_slots=1 << 14)
    assert e.known_import(c.image)["inserted"] == c.members
    assert KI.parse(e.known_export()).sets == c.sets
    meta, d = e.known_export_device()
    assert KI.parse(meta + d.cpu().numpy().tobytes()).sets == c.sets
    ref = block_canon(KI.lists_of_sets(c.sets, 0), c.sets, 0)
    assert block_canon(e.known_lists(0), c.sets, 0) == ref
    monkeypatch.setenv("CTMR_KNOWN_LISTS_CHUNK", "1000")
    assert block_canon(e.known_lists(0), c.sets, 0) == ref
    same_lists(device_lists(e, 0), c.sets, 0)
    e.close()


# ---- 5. warm restart with long serials, alone and in groups

def test_warm_restart_with_long_serials():
    rng = random.Random(5353)
    issuer = synth.issuer(synth.config(n_issuers=1), 0)
    name = D.name(D.rdn(3, b"Synth Issuer 000"))

    seen = set()

    def cert(ln):
        while True:
            s = bytes([rng.randrange(1, 0x7f)] + [rng.randrange(256) for _ in range(ln - 1)])
            if s not in seen:
                break
        seen.add(s)
        return D.cert(serial=s, issuer=name, not_after=D.utctime("270101000000Z"))

    def batch(certs):
        b = Batch.from_certs(certs, [0] * len(certs))
        b.payload = np.concatenate([b.payload, np.zeros(N.PAYLOAD_PAD, np.uint8)])
        return b

    uniq = [cert(ln) for ln in list(range(1, 46)) * 5]
    first = uniq + [uniq[rng.randrange(len(uniq))] for _ in range(150)]
    rng.shuffle(first)
    fresh = [cert(ln) for ln in list(range(1, 46)) * 2]
    second = fresh + fresh[::3] + [uniq[rng.randrange(len(uniq))] for _ in range(len(fresh))]
    rng.shuffle(second)
    b1, b2 = batch(first), batch(second)
    o, st1, unk1, _ = run_oracle(b1, [issuer], b"", True, 0)
    assert (st1 == 0).all() and int(unk1.sum()) == len(uniq)
    o, st2, unk2, _ = run_oracle(b2, [issuer], b"", True, 0, engine=o)
    assert (st2 == 0).all() and int(unk2.sum()) == len(fresh)

    def fresh_engine():
        e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
        e.add_issuers([issuer])
        e.set_filter(b"", True, 0)
        return e

    a = fresh_engine()
    ra = a.map_batch(b1)
    assert (ra.records["status"] == st1).all() and (((ra.records["flags"] & N.FL_WAS_UNKNOWN) != 0) == (unk1 != 0)).all()
    img = a.known_export()
    im = KI.parse(img)
    sets_a = im.sets
    assert sum(len(v) for v in sets_a.values()) == len(uniq) and im.n_host_members == 5 * 5
    assert {len(m) for v in sets_a.values() for m in v} == set(range(1, 46))
    lists_a = a.known_lists(0)
    check(lists_a, sets_a, 0)
    # world 1
    w1 = fresh_engine()
    st = w1.known_import(img)
    assert st["inserted"] == im.n_members and st["host_inserted"] == im.n_host_members
    r1 = w1.map_batch(b1)
    assert r1.stats.n_new == 0 and not (r1.records["flags"] & N.FL_WAS_UNKNOWN).any()
    r2 = w1.map_batch(b2)
    assert (r2.records["status"] == st2).all() and (((r2.records["flags"] & N.FL_WAS_UNKNOWN) != 0) == (unk2 != 0)).all()
    assert w1.total_count() == o.total_count()
    w1.close()
    for world in (2, 3):
        for mode in ("owner", "bloom"):
            engines = [fresh_engine() for _ in range(world)]
            g = Group.local(engines)
            if mode == "bloom":
                g.bloom_config(1 << 14)
            stats = [e.known_import(img, world=world, rank=r) for r, e in enumerate(engines)]
            assert stats[0]["host_members"] == im.n_host_members > 0 and all(s["host_members"] == 0 for s in stats[1:])
            assert sum(s["inserted"] for s in stats) == im.n_members and all(s["inserted"] for s in stats)
            union = {}
            for e in engines:
                for k, v in KI.parse(e.known_export()).sets.items():
                    for m in v:
                        assert m not in union.get(k, set()), "a key on two ranks"
                        union.setdefault(k, set()).add(m)
            assert {k: sorted(v) for k, v in union.items()} == sets_a
            assert canon(g.known_lists(0)) == canon(lists_a), (world, mode)

            def through_group(b):
                keep, shards = [], []
                for r in range(world):
                    lo, hi = shard_range(b.n, r, world)
                    sub = Batch.from_certs([b.cert(i) for i in range(lo, hi)], [0] * (hi - lo))
                    t = to_dev(sub)
                    keep.append((t, lo, hi))
                    shards.append(dev_shard(t, hi - lo, order_base=lo))
                return g.map_batch(mode, shards), keep

            stats1, keep1 = through_group(b1)
            assert all(s.n_new == 0 for s in stats1), (world, mode)
            for t, lo, hi in keep1:
                rec = t[4].cpu().numpy().view(RECORD_DTYPE)
                assert (rec["status"] == 0).all() and not (rec["flags"] & N.FL_WAS_UNKNOWN).any(), (world, mode)
            stats2, keep2 = through_group(b2)
            for t, lo, hi in keep2:
                rec = t[4].cpu().numpy().view(RECORD_DTYPE)
                assert (((rec["flags"] & N.FL_WAS_UNKNOWN) != 0) == (unk2[lo:hi] != 0)).all(), (world, mode)
            assert sum(s.n_new for s in stats2) == len(fresh) and g.total_count() == o.total_count()
            g.close()
            for e in engines:
                e.close()
    a.close()
