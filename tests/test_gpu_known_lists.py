"""-m gpu: per-issuer known-serial lists (include/ctmr.h ctmr_known_lists*).  The lists equal what the
oracle's sets give through the CPU twin (known_image.list_blocks), cut at `now` as IsExpiredAt cuts them; host-store
members, removals and sweeps show; the call is read-only; chunking, the device variant and a group's ranks give the same
lines; the host writer puts them on disk."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr
from ct_mapreduce_amd import known_image as KI, synth, _native as N
from ct_mapreduce_amd import host_writeback as HW
from ct_mapreduce_amd.distributed import Group
from oracle import oracle as orc
from tests.test_gpu_known_image import state, UNREG_ID
from tests.test_gpu_scale import device_batch

NOW = synth.BASE_TIME
DEV = torch.device("cuda:0")


def lines(text):
    return text.split(b"\n")[:-1]


def canon(lists):
    """{Issuer.ID: [sorted lines of each expDate block]} needs the blocks; without them: sorted lines per issuer."""
    return {bytes(i): sorted(lines(t)) for i, t in lists}


def check(lists, sets, now):
    """Engine lists against the twin's blocks of `sets` at `now`: same IDs in order, and per issuer the lines of each
    expDate block contiguous, in ascending expDate order, as multisets."""
    blocks = KI.list_blocks(sets, now)
    assert [i for i, _ in lists] == [i for i, _ in blocks]
    for (ident, text), (_, bl) in zip(lists, blocks):
        ls = lines(text)
        assert len(ls) == sum(len(ms) for _, ms in bl), ident
        at = 0
        for date, ms in bl:
            assert sorted(ls[at:at + len(ms)]) == sorted(KI.line(m)[:-1] for m in ms), (ident, date)
            at += len(ms)


def block_canon(lists, sets, now):
    """The lists with each expDate block's lines sorted (the order inside a block is unspecified)."""
    out = []
    for (ident, text), (_, bl) in zip(lists, KI.list_blocks(sets, now)):
        ls, at, t = lines(text), 0, []
        for _, ms in bl:
            t += sorted(ls[at:at + len(ms)])
            at += len(ms)
        out.append((ident, t))
    return out


@pytest.fixture(scope="module")
def big():
    """≥ 1 M synthetic entries with duplicates over 8 issuers, plus a ninth registered issuer sharing issuer 0's SPKI."""
    n = 1_000_000
    cfg = synth.config(seed=81, n_issuers=8, dup_permille=120, ca_permille=10, expired_permille=10)
    issuers = synth.issuers(cfg) + [synth.issuers(cfg)[0]]
    eng = ctmr.Engine(device=0, table_slots=1 << 21, pair_slots=1 << 16)
    eng.add_issuers(issuers)
    eng.set_filter(b"", False, NOW)
    d_off, d_pay, d_iss, d_et, total = device_batch(eng, cfg, 0, n, DEV)
    odd = (torch.arange(n, device=DEV) % 2) == 1
    d_iss[(d_iss == 0) & odd] = 8
    d_rec = torch.empty(n * 32, dtype=torch.uint8, device=DEV)
    d_new = torch.empty(n, dtype=torch.int64, device=DEV)
    eng.map_batch_device(d_pay.data_ptr(), d_off.data_ptr(), d_iss.data_ptr(), d_et.data_ptr(), n, d_rec.data_ptr(),
                         d_new.data_ptr())
    o = orc.Engine(b"", False, NOW)
    blob = np.frombuffer(b"".join(issuers), np.uint8)
    io = np.concatenate([[0], np.cumsum([len(x) for x in issuers])]).astype(np.uint64)
    o.batch(d_pay.cpu().numpy(), d_off.cpu().numpy().astype(np.uint64), d_iss.cpu().numpy().astype(np.uint32), blob, io)
    sets = {k: o.members(k) for k in o.keys() if k.startswith(b"serials::")}
    o.close()
    del d_off, d_pay, d_iss, d_et, d_rec, d_new
    yield eng, issuers, sets
    eng.close()


def test_lists_equal_the_oracle_sets_and_the_twin(big):
    eng, issuers, sets = big
    assert eng.issuer_id(8) == eng.issuer_id(0)
    hours = sorted({KI.exp_date_span(k.split(b"::")[1])[0] // 3600 for k in sets})
    assert len(hours) > 4 and len({k.split(b"::")[2] for k in sets}) == 8
    before = state(eng)
    ti = eng.table_info()
    img = eng.known_export()
    cut = hours[len(hours) // 2]
    for now in (0, (cut + 1) * 3600 - 1, (cut + 1) * 3600, (hours[-1] + 1) * 3600):
        got = eng.known_lists(now)
        check(got, sets, now)
        assert canon(got) == canon(KI.known_lists(img, now))
        kept = {k for k in sets if KI.exp_date_span(k.split(b"::")[1])[1] > now}
        assert sum(len(lines(t)) for _, t in got) == sum(len(sets[k]) for k in kept)
    assert eng.known_lists((hours[-1] + 1) * 3600) == []
    # exactly the sets of the cut hour go between now = end - 1 and now = end
    a, b = eng.known_lists((cut + 1) * 3600 - 1), eng.known_lists((cut + 1) * 3600)
    dropped = sum(len(v) for k, v in sets.items() if KI.exp_date_span(k.split(b"::")[1])[0] == cut * 3600)
    assert sum(len(lines(t)) for _, t in a) - sum(len(lines(t)) for _, t in b) == dropped > 0
    assert state(eng) == before
    ti2 = eng.table_info()
    assert (ti2.occupied, ti2.slots) == (ti.occupied, ti.slots)


def test_device_variant_chunks_and_range(big, monkeypatch):
    eng, issuers, sets = big
    now = 0
    ref = eng.known_lists(now)
    ids, toff, d_text = eng.known_lists_device(now)
    assert ids == [i for i, _ in ref]
    host_text = b"".join(t for _, t in ref)
    dev_text = d_text.cpu().numpy().tobytes()
    assert len(dev_text) == len(host_text)
    assert list(toff) == list(np.cumsum([0] + [len(t) for _, t in ref]))
    dev_lists = [(i, dev_text[toff[k]:toff[k + 1]]) for k, i in enumerate(ids)]
    assert block_canon(dev_lists, sets, now) == block_canon(ref, sets, now)
    # forced small chunks: several staging passes, the same lines in the same blocks
    monkeypatch.setenv("CTMR_KNOWN_LISTS_CHUNK", "50000")
    small = eng.known_lists(now)
    assert block_canon(small, sets, now) == block_canon(ref, sets, now)
    ids2, toff2, d2 = eng.known_lists_device(now)
    assert block_canon([(i, d2.cpu().numpy().tobytes()[toff2[k]:toff2[k + 1]]) for k, i in enumerate(ids2)], sets, now) \
        == block_canon(ref, sets, now)
    monkeypatch.delenv("CTMR_KNOWN_LISTS_CHUNK")
    # too small a buffer: CTMR_E_RANGE, the sizes, nothing written
    info = N.KnownListsInfo()
    text = np.full(64, 0xEE, np.uint8)
    ids_b = np.zeros(4096, np.uint8)
    offs = np.zeros(64, np.uint64)
    rc = eng._lib.ctmr_known_lists(eng._h, now, text.ctypes.data, text.nbytes, ids_b.ctypes.data, ids_b.nbytes,
                                   offs.ctypes.data, offs.size, C.byref(info))
    assert rc == N.E_RANGE
    assert (text == 0xEE).all() and not offs.any()
    assert info.text_bytes == len(host_text) and info.issuers == len(ref) == 8
    assert info.ids_bytes == sum(len(i) for i, _ in ref) and info.members == sum(len(v) for v in sets.values())
    assert info.host_members == 0


def test_host_store_members_removals_and_sweep(tmp_path):
    cfg = synth.config(seed=82, n_issuers=3, dup_permille=100)
    issuers = synth.issuers(cfg)
    e = ctmr.Engine(device=0, table_slots=1 << 16, pair_slots=1 << 12)
    e.add_issuers(issuers)
    e.set_filter(b"", False, NOW)
    e.map_batch(synth.host_batch(cfg, 0, 3000))
    ids = [e.issuer_id(k) for k in range(3)]
    h = 491000
    k0 = "serials::%s::%s" % (KI.exp_date_id(h).decode(), ids[0])
    k0b = "serials::%s::%s" % (KI.exp_date_id(h + 3).decode(), ids[0])
    for m in (b"", b"\x00\x01", b"\x21" * 21, b"\x40" * 40, b"\x41" * 41, b"\x00" * 60):
        e.set_insert(k0, m)
    e.set_insert(k0b, b"\x00\x01")                                   # the same serial under a second expDate
    for j in range(4):
        e.set_insert("serials::%s::%s" % (KI.exp_date_id(h).decode(), UNREG_ID), bytes([7]) * (j + 1))
    e.set_insert("serials::%s::%s" % (KI.exp_date_id(h).decode(), UNREG_ID), b"\x08" * 50)
    day = KI.exp_date_id(h)[:10].decode()
    e.set_insert("serials::%s::dayissuer" % day, b"\x99")
    e.set_insert("serials::2026-02-30-01::badday", b"\x98")           # unparsable date: skipped
    e.set_remove(k0, b"\x40" * 40)
    e.set_remove(k0, b"\x00" * 60)

    def expected():
        return {k: e.set_list(k) for k in e.keys(b"serials::*")}
    before = state(e)
    sets = expected()
    got = e.known_lists(0)
    check(got, sets, 0)
    assert state(e) == before
    d = dict(got)
    mine = lines(d[ids[0].encode()])
    assert mine.count(b"0001") == 2 and b"" in mine and (b"21" * 21) in mine and (b"41" * 41) in mine
    assert (b"40" * 40) not in mine and (b"00" * 60) not in mine
    assert sorted(lines(d[UNREG_ID.encode()])) == sorted([b"07" * (j + 1) for j in range(4)] + [b"08" * 50])
    assert d[b"dayissuer"] == b"99\n" and b"badday" not in d
    # the device variant puts the host-store lines at the same places
    ids_d, toff, t = e.known_lists_device(0)
    tb = t.cpu().numpy().tobytes()
    assert block_canon([(i, tb[toff[k]:toff[k + 1]]) for k, i in enumerate(ids_d)], sets, 0) == block_canon(got, sets, 0)
    # several chunks with host-store pieces between them
    os.environ["CTMR_KNOWN_LISTS_CHUNK"] = "7"
    try:
        assert block_canon(e.known_lists(0), sets, 0) == block_canon(got, sets, 0)
        ids_d, toff, t = e.known_lists_device(0)
        tb = t.cpu().numpy().tobytes()
        assert block_canon([(i, tb[toff[k]:toff[k + 1]]) for k, i in enumerate(ids_d)], sets, 0) == block_canon(got, sets, 0)
    finally:
        del os.environ["CTMR_KNOWN_LISTS_CHUNK"]
    # the writer: one file per list with exactly those bytes
    root = tmp_path / "lists"
    w = HW.HostWriter(str(root), [])
    assert e.store_known_lists(w, 0) == len(got)
    w.close()
    files = [(p.encode(), (root / p).read_bytes()) for p in sorted(os.listdir(root), key=str.encode)]
    assert [i for i, _ in files] == [i for i, _ in got]              # (the order inside a set may differ per call)
    assert block_canon(files, sets, 0) == block_canon(got, sets, 0)
    # a sweep at the end of hour h takes every set of hour h and before
    now = (h + 1) * 3600
    e.expire_sweep(now)
    sets2 = expected()
    after = e.known_lists(now)
    check(after, sets2, now)
    assert k0.encode() not in sets2 and k0b.encode() in sets2   # (host keys of unregistered issuers carry no expiry)
    assert lines(dict(after)[ids[0].encode()]).count(b"0001") == 1
    # a serials:: key with four parts fails the call
    e.set_insert("serials::%s::a::b" % KI.exp_date_id(h + 9).decode(), b"\x01")
    with pytest.raises(ctmr.CtmrError) as ex:
        e.known_lists(0)
    assert ex.value.code == N.E_INVAL
    e.close()


@pytest.mark.parametrize("mode", ["owner", "bloom"])
def test_group_ranks_merge_to_the_world_one_lists(mode):
    cfg = synth.config(seed=83, n_issuers=8, dup_permille=200, ca_permille=20, expired_permille=20)
    issuers = synth.issuers(cfg)
    a = ctmr.Engine(device=0, table_slots=1 << 16, pair_slots=1 << 12)
    a.add_issuers(issuers)
    a.set_filter(b"", False, NOW)
    a.map_batch(synth.host_batch(cfg, 0, 6000))
    img = a.known_export()
    sets = KI.parse(img).sets
    ref = a.known_lists(0)
    check(ref, sets, 0)
    for world in (2, 4):
        engines = []
        for _ in range(world):
            x = ctmr.Engine(device=0, table_slots=1 << 16, pair_slots=1 << 12)
            x.add_issuers(issuers)
            x.set_filter(b"", False, NOW)
            engines.append(x)
        g = Group.local(engines)
        if mode == "bloom":
            g.bloom_config(1 << 16)
        for r, x in enumerate(engines):
            x.known_import(img, world=world, rank=r)
        merged = g.known_lists(0)
        assert canon(merged) == canon(ref), (world, mode)
        assert canon(KI.merge_lists([x.known_lists(0) for x in engines])) == canon(merged)
        g.close()
        for x in engines:
            x.close()
    a.close()


def test_scale_twenty_million_chunked_equals_the_twin(monkeypatch):
    n = 20_000_000
    cfg = synth.config(seed=84, n_issuers=16, dup_permille=20)
    issuers = synth.issuers(cfg)
    eng = ctmr.Engine(device=0, table_slots=1 << 26, pair_slots=1 << 18)
    eng.add_issuers(issuers)
    eng.set_filter(b"", False, NOW)
    for first in range(0, n, 5_000_000):
        d_off, d_pay, d_iss, d_et, total = device_batch(eng, cfg, first, 5_000_000, DEV)
        eng.map_batch_device(d_pay.data_ptr(), d_off.data_ptr(), d_iss.data_ptr(), d_et.data_ptr(), 5_000_000, 0, 0)
        del d_off, d_pay, d_iss, d_et
    members = eng.total_count()
    assert members > 15_000_000
    monkeypatch.setenv("CTMR_KNOWN_LISTS_CHUNK", str(3_000_000))
    got = eng.known_lists(0)
    sets = KI.parse(eng.known_export()).sets
    twin = KI.lists_of_sets(sets, 0)
    assert [i for i, _ in got] == [i for i, _ in twin]
    for (i, t), (_, u) in zip(got, twin):
        assert len(t) == len(u) and sorted(lines(t)) == sorted(lines(u)), i
    eng.close()
