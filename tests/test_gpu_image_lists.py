"""-m gpu: per-issuer known-serial lists straight from an image (include/ctmr.h ctmr_known_image_lists*; kernels/lists.h
k_image_lists_count / k_image_lists_write).

Expected bytes come from the CPU twin known_image.image_lists (tests/test_image_lists_cpu.py holds it to Python dicts),
never from the code under test; every comparison is exact bytes and runs through both variants.  Engines are made the
way tests/test_gpu_known_image.py makes them, the corpora come from tests/known_corpus.py.

A set record is "not kept" when it has expired or when its hour lies outside the years 0000..9999.  The sets of an image
are in key order — hour-major for four-digit years — so sets that have EXPIRED are always the first ones of the image; the
shapes "the last set only" and "every second set" are made with five-digit years, whose keys sort as strings in between
and behind the four-digit ones.
"""
import ctypes as C
import functools
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr
from ct_mapreduce_amd import known_image as KI, synth, _native as N
from ct_mapreduce_amd import host_writeback as HW
from ct_mapreduce_amd.distributed import Group, shard_range
from ct_mapreduce_amd.engine import Batch
from tests import der as D, known_corpus as KC
from tests.test_gpu_exchange import DEV, dev_shard, to_dev
from tests.test_gpu_known_image import engine, state, add_point_members
from tests.test_gpu_known_sort import shuffled, table
from tests.test_image_lists_cpu import raw_image
from tests.test_known_merge_cpu import with_host_pairs

CFG = synth.config(seed=101, n_issuers=6, dup_permille=150, ca_permille=20, expired_permille=20)
HOURS = [491000, 491003, 491027]
DIGESTS = [bytes(np.random.default_rng(1000 + k).integers(0, 256, size=32, dtype=np.uint8).tolist()) for k in range(72)]
GUARD = 64
TWIN = functools.lru_cache(256)(KI.image_lists)


@pytest.fixture(scope="module")
def eng():
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)   # no issuer registered: the call needs none
    yield e
    e.close()


def fields(info):
    return tuple(getattr(info, f) for f, _ in N.KnownListsInfo._fields_)


def sizes_of(want):
    """(text bytes, ID bytes, offsets) of the twin's lists."""
    return sum(len(t) for _, t in want), sum(len(i) for i, _ in want), 2 * (len(want) + 1)


def unpack(text, ids, offs, info):
    g = info.issuers
    idb = ids.tobytes()
    assert int(offs[g]) == info.text_bytes and int(offs[2 * g + 1]) == info.ids_bytes and int(offs[0]) == 0
    return [(idb[int(offs[g + 1 + k]):int(offs[g + 2 + k])], text[int(offs[k]):int(offs[k + 1])]) for k in range(g)]


def call(e, img, now, device, text_cap, ids_cap, n_offs, phase=0):
    """One raw call with guard bytes round every buffer → (rc, info, lists or None).  device: the text pointer lies
    `phase` bytes behind a 16-byte boundary and the member records are given apart; the operand must stay as it was.
    A call that fails must leave every buffer as it was."""
    info = N.KnownListsInfo()
    ids = np.full(ids_cap + 2 * GUARD, 0xEE, np.uint8)
    offs = np.full(n_offs + 2, 0xEEEEEEEEEEEEEEEE, np.uint64)
    if device:
        n_mem = min(KI._HEADER.unpack_from(img, 0)[6], len(img) // 48) if len(img) >= 64 else 0
        at = len(img) - 48 * n_mem
        raw = np.frombuffer(img[at:], np.uint8)
        d_rec = torch.from_numpy(np.concatenate([raw, np.zeros(16, np.uint8)])).to(DEV)
        t = torch.full((text_cap + 2 * GUARD + 16,), 0xEE, dtype=torch.uint8, device=DEV)
        assert t.data_ptr() % 16 == 0
        rc = e._lib.ctmr_known_image_lists_device(
            e._h, img[:at], at, C.c_void_p(d_rec.data_ptr()) if n_mem else None, n_mem, int(now),
            C.c_void_p(t.data_ptr() + GUARD + phase), text_cap, ids.ctypes.data + GUARD, ids_cap, offs.ctypes.data + 8, n_offs,
            C.byref(info))
        assert (d_rec.cpu().numpy()[:len(raw)] == raw).all()
        buf = t.cpu().numpy()
        lo = GUARD + phase
    else:
        buf = np.full(text_cap + 2 * GUARD, 0xEE, np.uint8)
        rc = e._lib.ctmr_known_image_lists(e._h, img, len(img), int(now), buf.ctypes.data + GUARD, text_cap,
                                           ids.ctypes.data + GUARD, ids_cap, offs.ctypes.data + 8, n_offs, C.byref(info))
        lo = GUARD
    assert (buf[:lo] == 0xEE).all() and (buf[lo + text_cap:] == 0xEE).all(), "text guards"
    assert (ids[:GUARD] == 0xEE).all() and (ids[GUARD + ids_cap:] == 0xEE).all(), "ID guards"
    assert offs[0] == offs[-1] == 0xEEEEEEEEEEEEEEEE, "offset guards"
    if rc:
        assert (buf == 0xEE).all() and (ids == 0xEE).all() and (offs == 0xEEEEEEEEEEEEEEEE).all(), "written on failure"
        return rc, info, None
    assert (buf[lo + info.text_bytes:] == 0xEE).all(), "text behind text_bytes"
    return rc, info, unpack(buf[lo:lo + info.text_bytes].tobytes(), ids[GUARD:GUARD + ids_cap], offs[1:1 + n_offs], info)


def differ(got, want):
    assert [i for i, _ in got] == [i for i, _ in want]
    for (i, t), (_, w) in zip(got, want):
        if t != w:
            assert len(t) == len(w), (i, len(t), len(w))
            bad = np.nonzero(np.frombuffer(t, np.uint8) != np.frombuffer(w, np.uint8))[0]
            raise AssertionError("list %r: %d bytes differ, first at %d of %d" % (i, len(bad), bad[0], len(w)))


def check(e, img, now, phases=(0,), want=None):
    """Both variants at exact-size buffers against the twin (or `want`) → the lists."""
    want = TWIN(img, now) if want is None else want
    tb, ib, no = sizes_of(want)
    rc, info, got = call(e, img, now, False, tb, ib, no)
    assert rc == 0, rc
    differ(got, want)
    for phase in phases:
        rc, dinfo, dgot = call(e, img, now, True, tb, ib, no, phase=phase)
        assert rc == 0 and fields(dinfo) == fields(info)
        differ(dgot, want)
    assert (info.issuers, info.text_bytes, info.ids_bytes) == (len(want), tb, ib)
    return got, info


def list_order_is_a_permutation(img, now=0):
    """The kept sets in list order are not in image order (issuer-major against hour-major)."""
    n_iss, n_sets = KI._HEADER.unpack_from(img, 0)[3], KI._HEADER.unpack_from(img, 0)[5]
    so = 64 + 32 * n_iss
    ents = [KI._SET.unpack_from(img, so + 24 * s) for s in range(n_sets)]
    kept = [(KI.issuer_id(img[64 + 32 * o:96 + 32 * o]), eh, first) for eh, o, first, _ in ents if now < (eh + 1) * 3600]
    firsts = [f for _, _, f in sorted(kept)]
    return firsts != sorted(firsts) and len({i for i, _, _ in kept}) >= 70 and min(
        sum(1 for i, _, _ in kept if i == j) for j in {i for i, _, _ in kept}) >= 3


# ---- 1. shapes

@pytest.mark.parametrize("mix", KC.MIXES)
def test_every_mix_in_a_list_order_that_permutes_the_image(mix, eng):
    c = KC.make(mix, DIGESTS, HOURS, [1, 63, 64, 65, 2, 255, 256, 257, 1, 7, 3], seed=3)
    assert list_order_is_a_permutation(c.image)
    _, info = check(eng, c.image, 0, phases=(0, 5))
    assert info.members == KI.parse(c.image).n_members and info.host_members == KI.parse(c.image).n_host_members
    assert info.sets == 3 * len(DIGESTS)
    end = (HOURS[0] + 1) * 3600
    check(eng, c.image, end - 1)
    _, info = check(eng, c.image, end)                                        # the sets of the first hour are gone
    assert info.sets == 2 * len(DIGESTS)
    # the Python surface, and a shuffled image in the image's order
    assert eng.known_image_lists(c.image, 0) == TWIN(c.image, 0)
    sh = shuffled(c.image, 4)
    assert TWIN(sh, 0) != TWIN(c.image, 0) or mix == "twins"
    check(eng, sh, 0)
    meta, rec = KC.split(sh)
    ids, toff, t = eng.known_image_lists_device(meta, torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(DEV), 0)
    tb = t.cpu().numpy().tobytes()
    assert [(i, tb[int(toff[k]):int(toff[k + 1])]) for k, i in enumerate(ids)] == TWIN(sh, 0)


def test_sets_of_one_member_across_several_waves(eng):
    c = KC.make("uniform", DIGESTS, HOURS, 1, seed=5)                         # 216 sets: every lane a segment of its own
    assert KI.parse(c.image).n_members == KI.parse(c.image).n_sets == 3 * len(DIGESTS) > 3 * 64
    check(eng, c.image, 0, phases=(0, 9))
    check(eng, c.image, (HOURS[1] + 1) * 3600)


def test_set_sizes_round_the_wave_the_block_and_four_blocks(eng):
    for size in (63, 64, 65, 255, 256, 257, 1023, 1024, 1025):
        c = KC.make("uniform", DIGESTS[:3], HOURS, [size, 1], seed=size)
        check(eng, c.image, 0, phases=(0, 3))


def test_images_of_zero_one_and_two_records(eng):
    k = KI.set_key(HOURS[0], DIGESTS[0])
    empty, one, two = KI.build({}), KI.build({k: [b"\x01\x02\x03"]}), KI.build({k: [b"\x01\x02\x03", b"\x09"]})
    apart = KI.build({k: [b"\x0a"], KI.set_key(HOURS[1], DIGESTS[1]): [b""]})
    for img in (empty, one, two, apart):
        for now in (0, (HOURS[0] + 1) * 3600, (HOURS[2] + 1) * 3600):
            got, info = check(eng, img, now, phases=(0, 15))
    assert check(eng, empty, 0)[0] == [] and check(eng, one, 0)[0] == [(KI.issuer_id(DIGESTS[0]), b"010203\n")]
    only_host = with_host_pairs({}, [(b"serials::2026-01-05::x", b"\x01")])
    assert check(eng, only_host, 0)[0] == [(b"x", b"01\n")]


def year_hour(y, k=0):
    return KI._days_from_civil(y, 1, 1) * 24 + k


def test_sets_that_are_not_kept(eng):
    rng = np.random.default_rng(7)

    def ms(n):
        return [bytes(rng.integers(0, 256, size=int(L), dtype=np.uint8).tolist()) for L in rng.integers(0, 41, size=n)]
    # expired: all of them (empty output, the offsets still valid), the first set only
    sets = [(HOURS[0] + k, DIGESTS[k % 3], ms(40 + 37 * k)) for k in range(8)]
    img = raw_image(sets)
    got, info = check(eng, img, (HOURS[0] + 8) * 3600)
    assert got == [] and fields(info) == (0, 0, 0, 0, 0, 0)
    got, info = check(eng, img, (HOURS[0] + 1) * 3600)
    assert info.sets == 7 and info.members == sum(len(m) for _, _, m in sets[1:])
    # not kept: the last set only (a five-digit year sorts behind), and every second set (2026, 20260, 2027, 20270, …)
    last = raw_image(sets + [(year_hour(30000), DIGESTS[0], ms(100))])
    assert KC.record_sets(last)[-1] == 8
    got, info = check(eng, last, 0)
    assert info.sets == 8 and info.members == sum(len(m) for _, _, m in sets)
    alt = []
    for k in range(6):
        alt += [(year_hour(2026 + k), DIGESTS[k % 2], ms(30 + 70 * k)), (year_hour(20260 + 10 * k), DIGESTS[k % 2], ms(65))]
    img = raw_image(alt)
    hours = [KI._SET.unpack_from(img, 64 + 64 + 24 * s)[0] for s in range(12)]
    assert [KI._HOUR_LO <= h < KI._HOUR_HI for h in hours] == [True, False] * 6
    got, info = check(eng, img, 0, phases=(0, 7))
    assert info.sets == 6 and info.members == sum(len(m) for _, _, m in alt[::2])
    got, info = check(eng, img, (year_hour(2028) + 1) * 3600)
    assert info.sets == 3


def test_serial_lengths_alone_and_mixed_and_tiny_texts(eng):
    for L in range(41):
        img = raw_image([(HOURS[0], DIGESTS[0], [bytes([L + 1]) * L] * 3), (HOURS[1], DIGESTS[0], [bytes([L]) * L])])
        check(eng, img, 0, phases=(0, 11))
    mixed = [bytes([L ^ 0x5a]) * L for L in range(41)]
    check(eng, raw_image([(HOURS[0], DIGESTS[1], mixed + mixed[::-1]), (HOURS[0], DIGESTS[0], mixed[::3])]), 0, phases=(0, 1))
    # whole texts under 16 bytes, at every phase of the text pointer
    for members in ([b""], [b"", b""], [b"\x01"], [b"\x01\x02\x03", b""], [b"\xaa" * 7], [b"\x01", b"\x02", b"\x03", b"\x04", b"\x05"]):
        img = raw_image([(HOURS[0], DIGESTS[0], members)])
        assert sizes_of(TWIN(img, 0))[0] < 16
        check(eng, img, 0, phases=range(16))


# ---- 2. buffers

def test_every_phase_of_the_text_pointer(eng):
    c = KC.make("uniform", DIGESTS[:5], HOURS, [300, 1, 70], seed=9)
    check(eng, c.image, 0, phases=range(16))
    check(eng, shuffled(KC.make("tiny", DIGESTS[:5], HOURS, [300, 1, 70], seed=9).image), 0, phases=range(16))


def test_exact_bound_and_short_buffers(eng):
    c = KC.make("twins", DIGESTS[:4], HOURS, 0, seed=11)                      # member records and host members
    img, now = c.image, 0
    want = TWIN(img, now)
    tb, ib, no = sizes_of(want)
    im = KI.parse(img)
    host_lines = sum(2 * len(m) + 1 for _, m in KI.records(img)[1])
    bound = 81 * im.n_members + host_lines
    assert tb < bound
    for device in (False, True):
        rc, info, got = call(eng, img, now, device, tb, ib, no)
        assert rc == 0 and got == want
        rc, binfo, got = call(eng, img, now, device, bound, ib + 5, no + 3)      # sized by the bound: one call
        assert rc == 0 and got == want and fields(binfo) == fields(info)
        for caps in ((tb - 1, ib, no), (tb, ib - 1, no), (tb, ib, no - 1), (0, 0, 0)):
            rc, short, got = call(eng, img, now, device, *caps)
            assert rc == N.E_RANGE and got is None and fields(short) == fields(info), caps
    assert (info.members, info.host_members) == (im.n_members, im.n_host_members) and info.host_members > 0


def host_piece_image(n_first=64 * 3):
    """Host pieces before the first record, at the first lane of a wave, at the last lane, mid-wave and behind the last
    record: issuer "A…" (host only) sorts first; the sets of one digest have 64, 63, 30 and n members, each followed by
    the host members of its own key; issuer "zz" (host only) sorts last."""
    d = DIGESTS[0]
    ident = KI.issuer_id(d)
    rng = np.random.default_rng(13)
    sizes = [64, 63, 30, n_first]
    sets, pairs = {}, []
    for k, n in enumerate(sizes):
        key = KI.set_key(HOURS[0] + k, d)
        sets[key] = sorted({bytes(rng.integers(0, 256, size=int(L), dtype=np.uint8).tolist()) for L in rng.integers(1, 41, size=2 * n)})[:n]
        assert len(sets[key]) == n
        pairs += [(key, bytes([k + 1]) * 41), (key, bytes([k + 1]) * 50)]
    pairs += [(b"serials::" + KI.exp_date_id(HOURS[0]) + b"::" + b"\x21" + ident[1:], b"\x01\x02"),
              (b"serials::" + KI.exp_date_id(HOURS[0])[:10] + b"::zz", b"\x03" * 60),
              (b"serials::" + KI.exp_date_id(HOURS[0] + 1) + b"::" + ident + b"x", b"")]
    img = with_host_pairs(sets, pairs)
    assert KI._HEADER.unpack_from(img, 0)[6] == sum(sizes)
    return img


@pytest.mark.parametrize("chunk", [None, 257, 300, 7])
def test_host_pieces_at_every_place_and_in_split_chunks(chunk, eng, monkeypatch):
    if chunk is not None:
        monkeypatch.setenv("CTMR_KNOWN_LISTS_CHUNK", str(chunk))
    img = host_piece_image()
    got, info = check(eng, img, 0, phases=(0, 6))
    assert info.host_members == 11 and got[0][1] == b"0102\n" and got[-1][0] == b"zz"
    check(eng, img, (HOURS[0] + 2) * 3600)
    # a chunk split by a host piece: sets of 100 and 150 records with a piece between them fit one chunk of 257 / 300
    d = DIGESTS[1]
    sets = {KI.set_key(HOURS[0], d): [struct.pack(">H", v) for v in range(100)],
            KI.set_key(HOURS[1], d): [struct.pack(">H", v) * 9 for v in range(150)],
            KI.set_key(HOURS[2], d): [struct.pack(">H", v) * 20 for v in range(299)]}
    img = with_host_pairs(sets, [(KI.set_key(HOURS[0], d), b"\x77" * 44), (KI.set_key(HOURS[2], d), b"\x78" * 41)])
    check(eng, img, 0, phases=(0, 13))
    c = KC.make("uniform", DIGESTS[:9], HOURS, [1, 63, 64, 65, 255, 256, 257, 300], seed=15)
    check(eng, c.image, 0)


# ---- 3. rejection

def damaged(img, edit):
    meta, rec = KC.split(img)
    edit(rec)
    return meta + rec.tobytes()


def rejected(e, img, now):
    tb = 81 * (len(img) // 48) + 2 * len(img)
    for device in (False, True):
        rc, _, got = call(e, img, now, device, tb, 1 << 12, 1 << 9)
        assert rc == N.E_INVAL and got is None


def test_bad_records_in_kept_and_in_expired_sets(eng):
    c = KC.make("uniform", DIGESTS[:3], HOURS, [300, 301, 299], seed=17)
    img = shuffled(c.image)
    lens, sets_of = KC.record_lens(img), KC.record_sets(img)
    n = len(lens)
    expired_end = int(np.nonzero(sets_of == 3)[0][0])                         # the three sets of HOURS[0]
    late = (HOURS[0] + 1) * 3600
    want_late = TWIN(img, late)
    before = table(eng)
    for i in (0, expired_end - 1, expired_end, n - 1):
        bad = [damaged(img, lambda rec: rec["len"].__setitem__(i, 41)),
               damaged(img, lambda rec: rec["len"].__setitem__(i, 1 << 32))]
        for edge in (8, 16, 24, 32, 39):
            if lens[i] <= edge:
                bad.append(damaged(img, lambda rec: rec["serial"].__setitem__((i, edge), 1)))
        if lens[i] < 40:
            bad.append(damaged(img, lambda rec: rec["serial"].__setitem__((i, int(lens[i])), 0x80)))
        assert len(bad) >= 3
        for x in bad:
            with pytest.raises(KI.ImageError):
                KI.parse(x)
            rejected(eng, x, 0)
            if i < expired_end:                                                  # inside an expired set: not read
                check(eng, x, late, want=want_late)
            else:
                rejected(eng, x, late)
    assert table(eng) == before


def test_meta_damage_the_import_rejects(eng):
    c = KC.make("uniform", DIGESTS[:3], HOURS[:2], [30, 31, 29], seed=19)
    img = c.image
    n_iss = KI._HEADER.unpack_from(img, 0)[3]
    so = 64 + 32 * n_iss
    gap = bytearray(img)
    struct.pack_into("<Q", gap, so + 24 + 8, struct.unpack_from("<Q", img, so + 24 + 8)[0] + 1)
    empty = bytearray(img)
    struct.pack_into("<Q", empty, so + 16, 0)
    ordinal = bytearray(img)
    struct.pack_into("<I", ordinal, so + 4, n_iss)
    order = bytearray(img)
    order[so:so + 24], order[so + 24:so + 48] = img[so + 24:so + 48], img[so:so + 24]
    magic = bytearray(img)
    magic[0] ^= 1
    version = bytearray(img)
    struct.pack_into("<I", version, 8, 2)
    members = bytearray(img)
    struct.pack_into("<Q", members, 32, struct.unpack_from("<Q", img, 32)[0] + 1)
    for x in (gap, empty, ordinal, order, magic, version, members, img[:-48], img + b"\0" * 48, img[:40]):
        with pytest.raises(KI.ImageError):
            KI.parse(bytes(x))
        rejected(eng, bytes(x), 0)
    # a host key of two or of four parts
    for key in (b"serials::x", b"serials::" + KI.exp_date_id(HOURS[0]) + b"::a::b"):
        x = with_host_pairs(c.sets, [(key, b"\x01")])
        with pytest.raises(KI.ListsError):
            KI.image_lists(x, 0)
        rejected(eng, x, 0)
        with pytest.raises(ctmr.CtmrError) as ex:
            eng.known_image_lists(x, 0)
        assert ex.value.code == N.E_INVAL


# ---- 4. against the engine

def hand_built_engine():
    """Certificates of two issuers and a third that shares the first one's SPKI, serials of 1..45 octets under three
    expDates, then the point members of add_point_members (41..60 octets, an unregistered issuer)."""
    import random
    rng = random.Random(23)
    cfg = synth.config(n_issuers=2)
    issuers = [synth.issuer(cfg, 0), synth.issuer(cfg, 1), synth.issuer(cfg, 0)]
    names = [D.name(D.rdn(3, b"Synth Issuer 000")), D.name(D.rdn(3, b"Synth Issuer 001"))]
    ends = ["270101000000Z", "270101050000Z", "270102000000Z"]
    certs, idx, seen = [], [], set()
    for ln in list(range(1, 46)) * 4:
        for which in (0, 1, 2):
            s = bytes([rng.randrange(1, 0x7f)] + [rng.randrange(256) for _ in range(ln - 1)])
            if s in seen:
                continue
            seen.add(s)
            certs.append(D.cert(serial=s, issuer=names[which % 2], not_after=D.utctime(ends[rng.randrange(3)])))
            idx.append(which)
    certs += certs[::5]
    idx += idx[::5]
    b = Batch.from_certs(certs, idx)
    b.payload = np.concatenate([b.payload, np.zeros(N.PAYLOAD_PAD, np.uint8)])
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
    e.add_issuers(issuers)
    e.set_filter(b"", True, 0)
    r = e.map_batch(b)
    assert (r.records["status"] == 0).all() and e.issuer_id(2) == e.issuer_id(0) != e.issuer_id(1)
    add_point_members(e, [e.issuer_id(0), e.issuer_id(1)])
    return e


def test_a_sorted_export_gives_the_engine_s_sorted_lists(tmp_path):
    e = hand_built_engine()
    e.set_known_order(N.KNOWN_ORDER_SORTED)
    img = e.known_export()
    im = KI.parse(img)
    assert im.n_host_members > 6 and {len(m) for v in im.sets.values() for m in v} >= set(range(1, 46))
    hours = sorted({KI._SET.unpack_from(img, 64 + 32 * len(im.issuers) + 24 * s)[0] for s in range(im.n_sets)})
    assert len(hours) >= 3
    before = (state(e), table(e), e.issuer_counts().tobytes())
    other = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)       # an engine that knows no issuer
    cut = (hours[1] + 1) * 3600
    for now in (0, cut - 1, cut, (hours[-1] + 1) * 3600 - 1, (hours[-1] + 1) * 3600):
        want = e.known_lists(now)
        assert e.known_image_lists(img, now) == want
        assert other.known_image_lists(img, now) == want
        differ(check(other, img, now)[0], want)
    assert len(e.known_lists(cut - 1)) >= len(e.known_lists(cut)) and e.known_lists(cut - 1) != e.known_lists(cut)
    assert (state(e), table(e), e.issuer_counts().tobytes()) == before and e.known_export() == img
    # the writer: one file per list with exactly those bytes
    root = tmp_path / "lists"
    w = HW.HostWriter(str(root), [])
    assert other.store_image_lists(w, img, 0) == len(e.known_lists(0))
    w.close()
    files = [(p.encode(), (root / p).read_bytes()) for p in sorted(os.listdir(root), key=str.encode)]
    assert files == e.known_lists(0)
    other.close()
    e.close()


def test_an_engine_of_synthetic_batches_and_a_shuffled_image():
    issuers = synth.issuers(CFG)
    e = engine(issuers, table_slots=1 << 13)
    e.map_batch(synth.host_batch(CFG, 0, 2500))
    add_point_members(e, [e.issuer_id(k) for k in range(len(issuers))])
    e.set_known_order(N.KNOWN_ORDER_SORTED)
    img = e.known_export()
    before = (state(e), table(e), e.issuer_counts().tobytes())
    assert e.known_image_lists(img, 0) == e.known_lists(0) == TWIN(img, 0)
    sh = shuffled(img, 6)
    assert TWIN(sh, 0) != TWIN(img, 0)
    check(e, sh, 0)
    assert e.known_image_lists(e.known_merge(N.KNOWN_UNION, sh), 0) == e.known_lists(0)   # normalised first
    assert (state(e), table(e), e.issuer_counts().tobytes()) == before and e.known_export() == img
    e.close()


# ---- 5. groups

@pytest.mark.parametrize("mode", ["owner", "bloom"])
@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_a_group_s_canonical_lists_are_the_single_engine_s(mode, world):
    issuers = synth.issuers(CFG)
    single = engine(issuers)
    batches = [synth.host_batch(CFG, lo, 2400) for lo in (0, 1800)]
    for b in batches:
        single.map_batch(b)
    single.set_known_order(N.KNOWN_ORDER_SORTED)
    engines = [engine(issuers) for _ in range(world)]
    g = Group.local(engines)
    if mode == "bloom":
        g.bloom_config(1 << 16)
    base = 0
    for b in batches:
        shards, keep = [], []
        for r in range(world):
            lo, hi = shard_range(b.n, r, world)
            sub = Batch.from_certs([b.cert(i) for i in range(lo, hi)], b.issuer_idx[lo:hi], b.entry_type[lo:hi])
            t = to_dev(sub)
            keep.append(t)
            shards.append(dev_shard(t, sub.n, order_base=base + lo))
        g.map_batch(mode, shards)
        torch.cuda.synchronize()
        base += b.n
    want = single.known_lists(0)
    # every issuer has at least two expDates, spread over the ranks
    per_rank = [KI.parse(x.known_export()).sets for x in engines]
    for ident, _ in want:
        dates = {k.split(b"::")[1] for s in per_rank for k in s if k.split(b"::")[2] == ident}
        assert len(dates) >= 2
        if world > 1:
            assert sum(any(k.split(b"::")[2] == ident for k in s) for s in per_rank) >= 2
    hours = sorted({KI.exp_date_span(k.split(b"::")[1])[0] // 3600 for s in per_rank for k in s})
    nows = (0, (hours[len(hours) // 2] + 1) * 3600)
    for now in nows:
        assert g.known_lists(now, canonical=True) == single.known_lists(now)
    # the default: every rank's lists concatenated per Issuer.ID, as before (the ranks SORTED, so that two calls of one
    # rank write the same bytes: under CTMR_KNOWN_ORDER_ANY the order inside an expDate differs from call to call)
    for x in engines:
        x.set_known_order(N.KNOWN_ORDER_SORTED)
    for now in nows:
        assert g.known_lists(now) == KI.merge_lists([x.known_lists(now) for x in engines])
        assert g.known_lists(now, canonical=True) == single.known_lists(now)
    if world > 1:
        assert g.known_lists(0) != want
    g.close()
    for x in engines + [single]:
        x.close()
