"""-m gpu: the order inside a known-certificate set (include/ctmr.h ctmr_known_sort* / ctmr_set_known_order;
kernels/sort.h).

Expected bytes come from known_image.sort, the CPU twin (tests/test_known_sort_cpu.py holds it to sorted()), never from
the code under test.  The round count of a sort is read from the line the library prints under CTMR_KNOWN_SORT_INFO.
Engines are made the way tests/test_gpu_known_image.py makes them, the corpora come from tests/known_corpus.py.
"""
import base64
import ctypes as C
import re
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr
from ct_mapreduce_amd import known_image as KI, synth, _native as N
from tests import known_corpus as KC
from tests.test_gpu_exchange import DEV
from tests.test_gpu_known_image import engine, state, add_point_members

CFG = synth.config(seed=93, n_issuers=6, dup_permille=150, ca_permille=20, expired_permille=20)
ORDER = [5, 3, 1, 0, 2, 4]
HOURS = [490999, 491000, 491016, 491040]
TILE = 1024                      # kernels/sort.h SORT_TILE: the keys a block of the scatter kernel ranks
SIZES = {"uniform": [900, 1, 255, 256, 257, 40, TILE - 1, TILE, TILE + 1, 3000], "tiny": [400, 1, 255, 256, 257, 2, 3, 700],
         "interleaved": [700, 1, 255, 256, 257, 130, 2000], "runs": [1800, 1, 255, 256, 257, 3100], "twins": 0}
GUARD = 4 * 48
INFO = re.compile(rb"ctmr known sort: records=(\d+) runs=(\d+) rounds=(\d+) passes=(\d+)")


@pytest.fixture(scope="module")
def issuers():
    return synth.issuers(CFG)


@pytest.fixture(scope="module")
def digests(issuers):
    e = engine(issuers)
    out = [base64.urlsafe_b64decode(e.issuer_id(k)) for k in range(len(issuers))]
    e.close()
    return out


@pytest.fixture(scope="module")
def eng():
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)   # no issuer registered: the sort needs none
    yield e
    e.close()


def shuffled(img, seed=1):
    """The image with the records of every set in a random order."""
    meta, rec = KC.split(img)
    sets_of = KC.record_sets(img)
    rng = np.random.default_rng(seed)
    order = np.lexsort((rng.random(len(rec)), sets_of))
    return meta + rec[order].tobytes()


def table(e):
    return tuple(getattr(e.table_info(), f) for f, _ in N.TableInfo._fields_)


def sort_both(e, img):
    """Engine.known_sort and known_sort_device (guard records on both sides), which must agree → the sorted image."""
    host = e.known_sort(img)
    meta, rec = KC.split(img)
    raw = rec.view(np.uint8).reshape(-1)
    buf = np.full(len(raw) + 2 * GUARD, 0xEE, np.uint8)
    buf[GUARD:GUARD + len(raw)] = raw
    t = torch.from_numpy(buf).to(DEV)
    e.known_sort_device(meta, t[GUARD:GUARD + len(raw)])
    h = t.cpu().numpy()
    assert (h[:GUARD] == 0xEE).all() and (h[GUARD + len(raw):] == 0xEE).all()
    assert meta + h[GUARD:GUARD + len(raw)].tobytes() == host
    return host


def check_sort(e, img):
    want = KI.sort(img)
    got = sort_both(e, img)
    assert len(got) == len(want)
    if got != want:
        a, b = KC.split(got)[1], KC.split(want)[1]
        bad = np.nonzero(a != b)[0]
        raise AssertionError("%d of %d records differ, first at %d" % (len(bad), len(a), bad[0]))
    return got


def rounds_of(capfd, call):
    """call() → (its result, the rounds / passes / runs of the LAST sort it made, as the library reports them)."""
    capfd.readouterr()
    out = call()
    found = INFO.findall(capfd.readouterr().err.encode())
    assert found, "no CTMR_KNOWN_SORT_INFO line"
    records, runs, rounds, passes = (int(x) for x in found[-1])
    return out, {"records": records, "runs": runs, "rounds": rounds, "passes": passes}


def one_set_image(members, digest=bytes([7]) * 32, hour=491000):
    """An image of one set whose records are `members` in the order given (repeats allowed)."""
    rec = np.zeros(len(members), KI.MEMBER_DTYPE)
    for i, m in enumerate(members):
        rec["len"][i] = len(m)
        rec["serial"][i, :len(m)] = np.frombuffer(m, np.uint8)
    sets = KI._SET.pack(hour, 0, 0, len(members)) if members else b""
    meta = KI._HEADER.pack(KI.MAGIC, KI.VERSION, KI.HEADER_BYTES, 1 if members else 0, 0, 1 if members else 0,
                           len(members), 0, 0, 0) + (digest if members else b"") + sets
    meta += b"\0" * (-len(meta) % 64)
    return meta + rec.tobytes()


# ---- 1. images and corpora

def test_first_sorts_a_shuffled_image(eng, digests):
    c = KC.make("uniform", digests, HOURS[:2], [900, 1, 257, 3000], seed=11)
    img = shuffled(c.image)
    assert img != c.image
    assert check_sort(eng, img) == c.image == KI.build(c.sets)
    assert check_sort(eng, c.image) == c.image                                # already sorted: stays


@pytest.mark.parametrize("mix", KC.MIXES)
def test_every_mix_and_every_length(mix, eng, digests):
    c = KC.make(mix, digests, HOURS, SIZES[mix], seed=17)
    lens = KC.record_lens(c.image)
    if mix in ("uniform", "twins"):
        assert set(lens.tolist()) >= ({0, 1, 17, 18, 19, 20, 37, 38, 39, 40} if mix == "twins" else set(range(41)))
    counts = np.bincount(KC.record_sets(c.image))
    if mix != "twins":
        assert {1, 255, 256, 257} <= set(counts.tolist())
    if mix == "uniform":
        assert {TILE - 1, TILE, TILE + 1} <= set(counts.tolist())
    for seed in (1, 2):
        assert check_sort(eng, shuffled(c.image, seed)) == c.image


def test_each_serial_length_alone(eng, digests):
    for L in range(41):
        c = KC.make("uniform", digests[:2], HOURS[:1], [300, 5], seed=100 + L, lengths=(L,))
        assert check_sort(eng, shuffled(c.image, L)) == c.image


def test_thousands_of_sets_in_one_wave_and_one_set_alone(eng, digests, capfd, monkeypatch):
    monkeypatch.setenv("CTMR_KNOWN_SORT_INFO", "1")
    hours = [491000 + k for k in range(700)]
    c = KC.make("uniform", digests, hours, [1, 2, 1, 3, 1, 1, 2], seed=19)    # up to 64 sets in a wave of 64 records
    assert len(c.sets) == 4200
    assert check_sort(eng, shuffled(c.image)) == c.image
    ones = KC.make("uniform", digests, hours, 1, seed=20)                     # sets of one member: nothing to sort
    _, info = rounds_of(capfd, lambda: check_sort(eng, ones.image))
    assert info["rounds"] == 0 and info["passes"] == 0
    whole = KC.make("uniform", digests[:1], HOURS[:1], [70_000], seed=21, lengths=(16, 17, 20))   # one set is the image
    got, info = rounds_of(capfd, lambda: check_sort(eng, shuffled(whole.image)))
    assert got == whole.image and info["rounds"] == 1 and info["records"] == 70_000


def test_zero_and_one_records(eng, digests):
    empty = KI.build({})
    assert sort_both(eng, empty) == empty
    one = KI.build({KI.set_key(HOURS[0], digests[0]): [b"\x01\x02\x03"]})
    assert sort_both(eng, one) == one == KI.sort(one)
    two = one_set_image([b"\x02", b"\x01"])
    assert check_sort(eng, two) == one_set_image([b"\x01", b"\x02"])


# ---- 2. ties: the round count is what the data requires, never above six

def tied_members(rng, shared, n):
    """n distinct members of 40 octets that share their first `shared` octets."""
    head = bytes(rng.integers(0, 256, size=shared, dtype=np.uint8).tolist())
    tails = {bytes(rng.integers(0, 256, size=40 - shared, dtype=np.uint8).tolist()) for _ in range(n)}
    if shared == 39:
        tails = {bytes([v]) for v in range(256)}
    return [head + t for t in tails]


@pytest.mark.parametrize("shared,rounds", [(0, 1), (8, 2), (16, 3), (24, 4), (32, 5), (39, 5)])
def test_shared_prefixes_cost_one_round_per_eight_octets(shared, rounds, eng, capfd, monkeypatch):
    monkeypatch.setenv("CTMR_KNOWN_SORT_INFO", "1")
    rng = np.random.default_rng(shared)
    ms = tied_members(rng, shared, 2500)
    ms += [b"\x01\x02\x03", b"\xff" * 20]                                     # and members that are alone at once
    order = rng.permutation(len(ms))
    img = one_set_image([ms[i] for i in order])
    got, info = rounds_of(capfd, lambda: check_sort(eng, img))
    assert got == one_set_image(sorted(ms))
    assert info["rounds"] == rounds <= 6


def test_members_that_differ_in_length_alone(eng, capfd, monkeypatch):
    monkeypatch.setenv("CTMR_KNOWN_SORT_INFO", "1")
    rng = np.random.default_rng(4)
    ms = [b"\x00" * L for L in range(41)] + [b"\x05" * 9 + b"\x00" * L for L in range(32)]
    img = one_set_image([ms[i] for i in rng.permutation(len(ms))])
    got, info = rounds_of(capfd, lambda: check_sort(eng, img))
    assert got == one_set_image(sorted(ms)) and info["rounds"] == 6
    five = one_set_image([b"\x01", b"\x00\x01", b"\x00\x00", b"", b"\x00"])
    assert check_sort(eng, five) == one_set_image([b"", b"\x00", b"\x00\x00", b"\x00\x01", b"\x01"])


def test_repeated_records_stay_and_end_at_six_rounds(eng, digests, capfd, monkeypatch):
    monkeypatch.setenv("CTMR_KNOWN_SORT_INFO", "1")
    c = KC.make("uniform", digests[:3], HOURS[:2], [700, 40, 300], seed=23)
    meta, rec = KC.split(c.image)
    sets_of = KC.record_sets(c.image)
    n = 0
    for s in np.unique(sets_of):
        at = np.nonzero(sets_of == s)[0]
        for dst in (at[1], at[len(at) // 2], at[-1]):
            rec[dst] = rec[at[0]]
            n += 1
    img = shuffled(meta + rec.tobytes(), 3)
    got, info = rounds_of(capfd, lambda: check_sort(eng, img))
    assert info["rounds"] == 6
    a = KC.split(got)[1].view(np.uint8).reshape(-1, 48)
    assert int((a[1:] == a[:-1]).all(axis=1).sum()) == n                      # every repeat next to its original
    assert check_sort(eng, got) == got


# ---- 3. runs

@pytest.mark.parametrize("chunk", [300, 257, 5000])
def test_runs_forced_small(chunk, eng, digests, capfd, monkeypatch):
    c = KC.make("runs", digests, HOURS[:2], [1800, 1, 255, 256, 257, 700], seed=61)
    img = shuffled(c.image)
    monkeypatch.setenv("CTMR_KNOWN_SORT_INFO", "1")
    monkeypatch.setenv("CTMR_KNOWN_SORT_CHUNK", str(chunk))
    got, info = rounds_of(capfd, lambda: check_sort(eng, img))
    assert got == c.image and info["runs"] > 1


# ---- 4. an engine's order

def loaded_engines(issuers):
    """The same sets reached by different batch orders, by import of a shuffled image, and under another numbering."""
    b1, b2, b3 = (synth.host_batch(CFG, lo, 2500) for lo in (0, 2000, 4000))
    a = engine(issuers)
    for b in (b1, b2, b3):
        a.map_batch(b)
    r = engine(issuers)                                # (a batch's issuer_idx is in the engine's numbering)
    for b in (b3, b1, b2):
        r.map_batch(b)
    ids = [a.issuer_id(k) for k in range(len(issuers))]
    for e in (a, r):
        add_point_members(e, ids)
    i = engine(issuers, order=ORDER[::-1])
    i.known_import(shuffled(a.known_export(), 9))
    return a, r, i


def export_device(e):
    meta, rec = e.known_export_device()
    return meta + rec.cpu().numpy().tobytes()


def test_sorted_exports_are_identical_bytes(issuers):
    a, r, i = loaded_engines(issuers)
    assert state(a) == state(r) == state(i)
    any_order = [e.known_export() for e in (a, r, i)]
    assert all(KI.parse(x).sets == KI.parse(any_order[0]).sets for x in any_order)
    want = KI.sort(any_order[0])
    im = KI.parse(want)
    assert im.n_members > 3000 and im.n_host_members > 0
    before = [(state(e), table(e)) for e in (a, r, i)]
    for e in (a, r, i):
        e.set_known_order(N.KNOWN_ORDER_SORTED)
        assert e.known_export() == want
        assert export_device(e) == want
    assert want == KI.sort(any_order[1]) == KI.sort(any_order[2])
    # the default again: any order, the same sets
    for e in (a, r, i):
        e.set_known_order(N.KNOWN_ORDER_ANY)
        assert KI.parse(e.known_export()).sets == im.sets and KI.sort(e.known_export()) == want
    assert [(state(e), table(e)) for e in (a, r, i)] == before
    for bad in (2, -1):
        with pytest.raises(ctmr.CtmrError) as ex:
            a.set_known_order(bad)
        assert ex.value.code == N.E_INVAL
    for e in (a, r, i):
        e.close()


def test_sorted_export_in_forced_runs(issuers, monkeypatch):
    a, r, i = loaded_engines(issuers)
    want = KI.sort(a.known_export())
    monkeypatch.setenv("CTMR_KNOWN_SORT_CHUNK", "400")
    for e in (a, r, i):
        e.set_known_order(N.KNOWN_ORDER_SORTED)
        assert e.known_export() == want and export_device(e) == want
        e.close()


# ---- 5. lists

def sorted_lists(e, sets, now):
    """What a SORTED engine holding `sets` writes: per expDate block the lines of the members its table holds (at most
    40 octets, under a registered issuer), sorted, then the lines of its host-store piece, sorted."""
    reg = {e.issuer_id(k).encode() for k in range(e.issuer_count())}
    out = []
    for ident, blocks in KI.list_blocks(sets, now):
        text = b""
        for date, ms in blocks:
            dev = [m for m in ms if len(m) <= 40 and ident in reg and len(date) == 13]
            host = [m for m in ms if not (len(m) <= 40 and ident in reg and len(date) == 13)]
            text += b"".join(sorted(KI.line(m) for m in dev)) + b"".join(sorted(KI.line(m) for m in host))
        out.append((ident, text))
    return out


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


def device_lists(e, now):
    ids, toff, t = e.known_lists_device(now)
    tb = t.cpu().numpy().tobytes()
    return [(i, tb[toff[k]:toff[k + 1]]) for k, i in enumerate(ids)]


@pytest.fixture(scope="module")
def listed(issuers, digests):
    c = KC.make("uniform", digests, HOURS, [900, 1, 255, 256, 257, 40, 1500], seed=31)
    e = engine(issuers, order=ORDER)
    e.known_import(shuffled(c.image, 5))
    add_point_members(e, [e.issuer_id(k) for k in range(len(issuers))])
    sets = KI.parse(e.known_export()).sets
    e.set_known_order(N.KNOWN_ORDER_SORTED)
    yield e, sets
    e.close()


def test_sorted_lists(listed, monkeypatch):
    e, sets = listed
    end = (HOURS[1] + 1) * 3600
    for now in (0, end - 1, end):
        want = sorted_lists(e, sets, now)
        twin = KI.known_lists(e.known_export(), now)
        assert [i for i, _ in want] == [i for i, _ in twin]
        # the twin's blocks hold the same lines; a block without host-store lines is the twin's, sorted
        for (_, t), (_, tw) in zip(want, twin):
            assert sorted(t.split(b"\n")) == sorted(tw.split(b"\n"))
        assert e.known_lists(now) == want
        assert device_lists(e, now) == want
    assert any(len(m) > 40 for v in sets.values() for m in v)
    for lists_chunk, sort_chunk in ((300, None), (None, 300), (257, 100), (5000, 256)):
        for name, v in (("CTMR_KNOWN_LISTS_CHUNK", lists_chunk), ("CTMR_KNOWN_SORT_CHUNK", sort_chunk)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(v))
        want = sorted_lists(e, sets, 0)
        assert e.known_lists(0) == want and device_lists(e, 0) == want


def test_sorted_lists_exact_and_bound_buffers_at_every_phase(listed):
    e, sets = listed
    now = 0
    want = sorted_lists(e, sets, now)
    rc, info, _, _ = raw_lists(e, now, False, 0, 0)                           # the sizing call
    tb = int(info.text_bytes)
    assert rc == N.E_RANGE and tb == sum(len(t) for _, t in want)
    guard = 64
    buf = np.full(tb + 2 * guard, 0xEE, np.uint8)
    rc, info, ids, offs = raw_lists(e, now, False, buf.ctypes.data + guard, tb)
    assert rc == 0 and (buf[:guard] == 0xEE).all() and (buf[guard + tb:] == 0xEE).all()
    assert split_text(buf[guard:guard + tb].tobytes(), info, ids, offs) == want
    bound = 81 * int(info.members) + tb                                       # sized by the bound: no count pass
    for cap in (tb, bound):
        for shift in range(16):
            t = torch.full((256 + cap + 2 * guard + 16,), 0xEE, dtype=torch.uint8, device=DEV)
            lo = (-t.data_ptr()) % 256 + guard + shift
            assert t[lo:].data_ptr() % 16 == shift
            rc, info, ids, offs = raw_lists(e, now, True, t[lo:].data_ptr(), cap)
            assert rc == 0 and info.text_bytes == tb
            h = t.cpu().numpy()
            assert (h[:lo] == 0xEE).all() and (h[lo + tb:] == 0xEE).all(), shift
            assert split_text(h[lo:lo + tb].tobytes(), info, ids, offs) == want, shift


# ---- 6. rejections and side effects

def test_rejected_images_leave_the_buffer_as_it_was(eng, digests, monkeypatch):
    c = KC.make("uniform", digests, HOURS[:2], [300, 301, 299], seed=37)
    img = shuffled(c.image)
    n = c.members
    lens = KC.record_lens(img)
    n_iss = KI._HEADER.unpack_from(img, 0)[3]
    so = 64 + 32 * n_iss

    def damaged(edit):
        meta, rec = KC.split(img)
        edit(rec)
        return meta + rec.tobytes()

    bad = []
    for i in (0, n - 1):                                                      # the last record: in the last run
        bad.append(damaged(lambda rec: rec["len"].__setitem__(i, 41)))
        for edge in (8, 16, 24, 32, 39):
            if lens[i] <= edge:
                bad.append(damaged(lambda rec: rec["serial"].__setitem__((i, edge), 1)))
    magic = bytearray(img)
    magic[0] ^= 1
    version = bytearray(img)
    struct.pack_into("<I", version, 8, 2)
    gap = bytearray(img)
    struct.pack_into("<Q", gap, so + 24 + 8, struct.unpack_from("<Q", img, so + 24 + 8)[0] + 1)
    ordinal = bytearray(img)
    struct.pack_into("<I", ordinal, so + 4, n_iss)
    order = bytearray(img)
    order[so:so + 24], order[so + 24:so + 48] = img[so + 24:so + 48], img[so:so + 24]
    bad += [bytes(magic), bytes(version), bytes(gap), bytes(ordinal), bytes(order)]
    assert len(bad) >= 8
    before = table(eng)
    for chunk in (None, 200):
        if chunk:
            monkeypatch.setenv("CTMR_KNOWN_SORT_CHUNK", str(chunk))
        for b in bad:
            with pytest.raises(KI.ImageError):
                KI.sort(b)
            # host variant: the caller's bytes, guarded on both sides
            buf = np.full(len(b) + 128, 0xEE, np.uint8)
            buf[64:64 + len(b)] = np.frombuffer(b, np.uint8)
            rc = eng._lib.ctmr_known_sort(eng._h, buf.ctypes.data + 64, len(b))
            assert rc == N.E_INVAL
            assert buf[64:64 + len(b)].tobytes() == b and (buf[:64] == 0xEE).all() and (buf[64 + len(b):] == 0xEE).all()
            # device variant
            meta, rec = KC.split(b)
            raw = rec.view(np.uint8).reshape(-1)
            dbuf = np.full(len(raw) + 2 * GUARD, 0xEE, np.uint8)
            dbuf[GUARD:GUARD + len(raw)] = raw
            t = torch.from_numpy(dbuf).to(DEV)
            with pytest.raises(ctmr.CtmrError) as ex:
                eng.known_sort_device(meta, t[GUARD:GUARD + len(raw)])
            assert ex.value.code == N.E_INVAL
            assert (t.cpu().numpy() == dbuf).all()
    # a record count that disagrees with the header
    meta, rec = KC.split(img)
    t = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(DEV)
    with pytest.raises(ctmr.CtmrError) as ex:
        eng.known_sort_device(meta, t[:-48])
    assert ex.value.code == N.E_INVAL
    assert table(eng) == before


def test_sort_call_changes_nothing_of_the_engine(issuers, digests):
    e = engine(issuers, table_slots=1 << 13)
    e.map_batch(synth.host_batch(CFG, 0, 1500))
    add_point_members(e, [e.issuer_id(k) for k in range(len(issuers))])
    own = e.known_export()
    before = (state(e), table(e), KI.sort(own))
    other = KC.make("uniform", digests + [bytes(range(32))], HOURS[:2], [300, 301, 299], seed=38)
    for img in (own, shuffled(other.image)):
        assert sort_both(e, img) == KI.sort(img)
    assert (state(e), table(e), KI.sort(e.known_export())) == before
    e.close()


def test_a_sorted_image_imports_queries_and_removes_as_the_unsorted_one(issuers, eng):
    src = engine(issuers)
    src.map_batch(synth.host_batch(CFG, 0, 3000))
    add_point_members(src, [src.issuer_id(k) for k in range(len(issuers))])
    img = src.known_export()
    srt = eng.known_sort(img)
    assert srt == KI.sort(img) and srt != img
    x, y = engine(issuers, order=ORDER), engine(issuers, order=ORDER)
    st_x, st_y = x.known_import(img), y.known_import(srt)
    assert st_x == st_y and state(x) == state(y) == state(src)
    for e in (x, y):
        for i in (img, srt):
            fl, hf, st = e.known_query(i)
            assert fl.all() and hf.all() and st["hits"] == st["taken"] == st["members"]
    assert x.known_remove(img) == y.known_remove(srt)
    assert state(x) == state(y) and x.total_count() == 0
    for e in (src, x, y):
        e.close()
