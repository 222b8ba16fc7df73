"""-m gpu: the Redis protocol stream of an image (include/ctmr.h ctmr_known_image_resp*; kernels/resp.h
k_image_resp_count / k_image_resp_write).

Expected bytes come from the CPU twin known_image.image_resp (tests/test_image_resp_cpu.py holds it to redis_dump and
redis_load), never from the code under test; every comparison is exact bytes and runs through both variants, with guard
bytes round every buffer.  Engines are made the way tests/test_gpu_known_image.py makes them.
"""
import ctypes as C
import functools
import io
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr
from ct_mapreduce_amd import known_image as KI, synth, _native as N
from ct_mapreduce_amd.distributed import Group, shard_range
from ct_mapreduce_amd.engine import Batch
from ct_mapreduce_amd.remote_cache import GpuRemoteCache, redis_load
from tests import known_corpus as KC
from tests.test_gpu_exchange import DEV, dev_shard, to_dev
from tests.test_gpu_image_lists import CFG, hand_built_engine
from tests.test_gpu_known_image import engine, state
from tests.test_gpu_known_sort import shuffled, table
from tests.test_image_lists_cpu import raw_image
from tests.test_image_resp_cpu import commands, header_counts
from tests.test_known_merge_cpu import with_host_pairs

HOURS = [491000, 491003, 491027]
DIGESTS = [bytes(np.random.default_rng(2000 + k).integers(0, 256, size=32, dtype=np.uint8).tolist()) for k in range(72)]
GUARD = 64
TWIN = functools.lru_cache(256)(KI.image_resp)
WORST_HOUR = KI._HOUR_HI - 1                                       # a 12-character timestamp


@pytest.fixture(scope="module")
def eng():
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)   # no issuer registered: the call needs none
    yield e
    e.close()


def fields(info):
    return tuple(getattr(info, f) for f, _ in N.KnownRespInfo._fields_)


def call(e, img, per, device, text_cap, phase=0):
    """One raw call with guard bytes round the text → (rc, info, text or None).  device: the text pointer lies `phase`
    bytes behind a 16-byte boundary and the member records are given apart; the operand must stay as it was.  A call
    that fails must leave the buffer as it was."""
    info = N.KnownRespInfo()
    if device:
        n_mem = min(KI._HEADER.unpack_from(img, 0)[6], len(img) // 48) if len(img) >= 64 else 0
        at = len(img) - 48 * n_mem
        raw = np.frombuffer(img[at:], np.uint8)
        d_rec = torch.from_numpy(np.concatenate([raw, np.zeros(16, np.uint8)])).to(DEV)
        t = torch.full((text_cap + 2 * GUARD + 16,), 0xEE, dtype=torch.uint8, device=DEV)
        assert t.data_ptr() % 16 == 0 and d_rec.data_ptr() % 16 == 0
        rc = e._lib.ctmr_known_image_resp_device(e._h, img[:at], at, C.c_void_p(d_rec.data_ptr()) if n_mem else None, n_mem,
                                                 per, C.c_void_p(t.data_ptr() + GUARD + phase), text_cap, C.byref(info))
        assert (d_rec.cpu().numpy()[:len(raw)] == raw).all()
        buf = t.cpu().numpy()
        lo = GUARD + phase
    else:
        buf = np.full(text_cap + 2 * GUARD, 0xEE, np.uint8)
        rc = e._lib.ctmr_known_image_resp(e._h, img, len(img), per, buf.ctypes.data + GUARD, text_cap, C.byref(info))
        lo = GUARD
    assert (buf[:lo] == 0xEE).all() and (buf[lo + text_cap:] == 0xEE).all(), "text guards"
    if rc:
        assert (buf == 0xEE).all(), "written on failure"
        return rc, info, None
    assert (buf[lo + info.text_bytes:] == 0xEE).all(), "text behind text_bytes"
    return rc, info, buf[lo:lo + info.text_bytes].tobytes()


def differ(got, want):
    if got != want:
        assert len(got) == len(want), (len(got), len(want))
        bad = np.nonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[0]
        raise AssertionError("%d bytes differ, first at %d of %d: %r, expected %r" % (
            len(bad), bad[0], len(want), got[max(bad[0] - 20, 0):bad[0] + 20], want[max(bad[0] - 20, 0):bad[0] + 20]))


def check(e, img, per=512, phases=(0,)):
    """Both variants at exact-size buffers against the twin → info."""
    want = TWIN(img, per)
    rc, info, got = call(e, img, per, False, len(want))
    assert rc == 0, rc
    differ(got, want)
    for phase in phases:
        rc, dinfo, dgot = call(e, img, per, True, len(want), phase=phase)
        assert rc == 0 and fields(dinfo) == fields(info)
        differ(dgot, want)
    n_mem, n_sets, host_bytes, n_host = header_counts(img)
    dev_keys, host_keys = ({k for k, _ in part} for part in KI.records(img))
    assert fields(info) == (len(dev_keys | host_keys), n_mem, n_host, len(commands(want)), len(want))
    assert len(want) <= KI.resp_bound(n_mem, n_sets, host_bytes, n_host, per)
    return info


def ms(rng, n, lo=0, hi=41):
    return [bytes(rng.integers(0, 256, size=int(L), dtype=np.uint8).tolist()) for L in rng.integers(lo, hi, size=n)]


# ---- 1. images and sizes

@pytest.mark.parametrize("mix", KC.MIXES)
def test_every_mix(mix, eng):
    c = KC.make(mix, DIGESTS, HOURS, [1, 63, 64, 65, 2, 255, 256, 257, 1, 7, 3, 127, 128, 129], seed=3)
    info = check(eng, c.image, 512, phases=(0, 5))
    assert info.members == KI.parse(c.image).n_members and info.sets == 3 * len(DIGESTS)
    check(eng, c.image, 3)
    sh = shuffled(c.image, 4)
    assert TWIN(sh, 512) != TWIN(c.image, 512) or mix == "twins"
    check(eng, sh, 64)
    # the Python surface
    assert eng.known_image_resp(c.image) == TWIN(c.image, 512)
    meta, rec = KC.split(sh)
    t = eng.known_image_resp_device(meta, torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(DEV), 7)
    assert t.cpu().numpy().tobytes() == TWIN(sh, 7)


def test_images_of_zero_one_and_two_records(eng):
    k = KI.set_key(HOURS[0], DIGESTS[0])
    empty, one, two = KI.build({}), KI.build({k: [b"\x01\x02\x03"]}), KI.build({k: [b"\x01\x02\x03", b"\x09"]})
    apart = KI.build({k: [b"\x0a"], KI.set_key(HOURS[1], DIGESTS[1]): [b""]})
    only_host = with_host_pairs({}, [(b"serials::2026-01-05::x", b"\x01"), (b"serials::y", b"")])
    for img in (empty, one, two, apart, only_host):
        for per in (1, 2, 512):
            check(eng, img, per, phases=(0, 15))
    assert TWIN(empty, 512) == b"" and fields(check(eng, empty)) == (0, 0, 0, 0, 0)
    assert check(eng, only_host).sets == 2 and check(eng, only_host).commands == 3


def test_set_sizes_round_the_wave_and_the_block_next_to_one_member_sets(eng):
    for size in (63, 64, 65, 127, 128, 129, 255, 256, 257):
        c = KC.make("uniform", DIGESTS[:3], HOURS, [size, 1], seed=size)
        check(eng, c.image, 512, phases=(0, 3))
        check(eng, c.image, 64)


def test_more_than_one_block_of_the_worst_records(eng):
    # one-member sets, 40-octet serials, 12-character timestamps: 248 B per record, 128 × 248 B per block
    sets = [(WORST_HOUR - k // len(DIGESTS), DIGESTS[k % len(DIGESTS)], [bytes([k % 251 + 1]) * 40]) for k in range(300)]
    img = raw_image(sets)
    assert len(TWIN(img, 512)) == 300 * 248
    check(eng, img, 512, phases=range(16))
    check(eng, img, 1, phases=(0, 15))
    early = raw_image([(KI._HOUR_LO + k // len(DIGESTS), DIGESTS[k % len(DIGESTS)], [bytes([k % 251 + 1]) * 40]) for k in range(300)])
    assert len(TWIN(early, 512)) == 300 * 248                       # "-62167219200": 12 characters too
    check(eng, early, 512, phases=(0, 7))


# ---- 2. commands and fields

@pytest.mark.parametrize("per", [1, 2, 3])
def test_small_commands_and_sets_round_their_multiples(per, eng):
    rng = np.random.default_rng(per)
    sizes = sorted({n for k in (1, 2, 3, 22, 43, 64, 100) for n in (per * k - 1, per * k, per * k + 1) if n > 0})
    sets = [(HOURS[0] + j, DIGESTS[j % 5], ms(rng, n)) for j, n in enumerate(sizes)]
    check(eng, raw_image(sets), per, phases=(0, 9))


def test_512_members_per_command(eng):
    rng = np.random.default_rng(5)
    sets = [(HOURS[0] + j, DIGESTS[j % 3], ms(rng, n, 1, 21)) for j, n in enumerate((511, 512, 513, 1, 1023, 1024, 1025))]
    info = check(eng, raw_image(sets), 512, phases=(0, 2))
    assert info.commands == (1 + 1 + 2 + 1 + 2 + 2 + 3) + 7


def test_the_largest_command(eng):
    rng = np.random.default_rng(6)
    sets = [(HOURS[0], DIGESTS[0], ms(rng, 1500, 0, 9)), (HOURS[1], DIGESTS[0], ms(rng, 3, 0, 9))]
    img = raw_image(sets)
    assert TWIN(img, 1 << 20).startswith(b"*1502\r\n")
    assert check(eng, img, 1 << 20, phases=(0, 4)).commands == 4


def test_serial_lengths_alone_and_mixed(eng):
    for L in range(41):
        img = raw_image([(HOURS[0], DIGESTS[0], [bytes([L + 1]) * L] * 3), (HOURS[1], DIGESTS[0], [bytes([L]) * L])])
        check(eng, img, 2, phases=(0, 11))
    mixed = [bytes([L ^ 0x5a]) * L for L in range(41)]
    check(eng, raw_image([(HOURS[0], DIGESTS[1], mixed + mixed[::-1]), (HOURS[0], DIGESTS[0], mixed[::3])]), 512, phases=(0, 1))
    nine_ten = [b"\x09" * 9, b"\x0a" * 10] * 70
    img = raw_image([(HOURS[0], DIGESTS[0], nine_ten)])
    assert b"$9\r\n" in TWIN(img, 512) and b"$10\r\n" in TWIN(img, 512)
    check(eng, img, 512, phases=(0, 8))


def test_the_argument_count_gains_a_digit(eng):
    rng = np.random.default_rng(8)
    for argc in (9, 10, 99, 100):
        sets = [(HOURS[0] + j, DIGESTS[0], ms(rng, n, 1, 5)) for j, n in enumerate((argc - 3, argc - 2, argc - 1, 2 * (argc - 2) + 1))]
        img = raw_image(sets)
        assert TWIN(img, argc - 2).count(b"*%d\r\n" % argc) == 4
        check(eng, img, argc - 2, phases=(0, 6))
        check(eng, img, 512)


def test_expiry_hours_at_the_edges(eng):
    lo, hi = KI._HOUR_LO, KI._HOUR_HI
    hours = [0, 1, -1, lo, lo + 1, lo + 24 * 59, lo + 24 * 60, hi - 1, hi - 2, -24 * 365 * 1000, 24 * 366 * 30, 278, 27778]
    img = raw_image([(h, DIGESTS[k % 2], [b"\x01", b"\x02"]) for k, h in enumerate(hours)])
    check(eng, img, 512, phases=(0, 10))


# ---- 3. buffers

def test_every_phase_of_the_text_pointer(eng):
    c = KC.make("uniform", DIGESTS[:5], HOURS, [300, 1, 70], seed=9)
    check(eng, c.image, 512, phases=range(16))
    check(eng, shuffled(KC.make("tiny", DIGESTS[:5], HOURS, [300, 1, 70], seed=9).image), 3, phases=range(16))


def test_exact_bound_and_short_buffers(eng):
    c = KC.make("twins", DIGESTS[:4], HOURS, 0, seed=11)                      # member records and host members
    img = c.image
    for per in (2, 512):
        want = TWIN(img, per)
        bound = KI.resp_bound(*header_counts(img), per)
        assert len(want) < bound
        for device in (False, True):
            rc, info, got = call(eng, img, per, device, len(want))
            assert rc == 0 and got == want
            rc, binfo, got = call(eng, img, per, device, bound)                  # sized by the bound: one call
            assert rc == 0 and got == want and fields(binfo) == fields(info)
            for cap in (len(want) - 1, 0):
                rc, short, got = call(eng, img, per, device, cap)
                assert rc == N.E_RANGE and got is None and fields(short) == fields(info), cap
        assert info.host_members == KI.parse(img).n_host_members > 0


# ---- 4. host pieces

def host_piece_image():
    """Host keys before the first record, between two sets, under keys that also have records (at the first and last
    lane of a wave and mid-wave) and behind the last record; one without a second "::" and one whose date does not parse."""
    d = DIGESTS[0]
    ident = KI.issuer_id(d)
    rng = np.random.default_rng(13)
    sizes = [64, 63, 30, 192]
    sets, pairs = {}, []
    for k, n in enumerate(sizes):
        key = KI.set_key(HOURS[0] + k, d)
        sets[key] = sorted(set(ms(rng, 2 * n, 1, 41)))[:n]
        assert len(sets[key]) == n
        pairs += [(key, bytes([k + 1]) * 41), (key, bytes([k + 1]) * 50)]
    pairs += [(b"serials::" + KI.exp_date_id(HOURS[0] - 1) + b"::" + ident, b"\x01\x02"),
              (b"serials::" + KI.exp_date_id(HOURS[0])[:10] + b"::zz", b"\x03" * 60),
              (b"serials::" + KI.exp_date_id(HOURS[0] + 1) + b"::" + ident + b"x", b""),
              (b"serials::" + KI.exp_date_id(HOURS[0] + 1) + b"::" + ident + b"y", b"\x04"),
              (b"serials::zzz", b"\x05"), (b"serials::9999-99-99::q", b"\x06")]
    img = with_host_pairs(sets, pairs)
    assert KI._HEADER.unpack_from(img, 0)[6] == sum(sizes)
    return img


@pytest.mark.parametrize("chunk", [None, 257, 300, 7])
def test_host_pieces_at_every_place_and_in_split_chunks(chunk, eng, monkeypatch):
    if chunk is not None:
        monkeypatch.setenv("CTMR_KNOWN_RESP_CHUNK", str(chunk))
    img = host_piece_image()
    for per in (1, 512):
        info = check(eng, img, per, phases=(0, 6))
        assert info.host_members == 14 and info.sets == 4 + 6
    want = TWIN(img, 512)
    assert want.startswith(b"*3\r\n$4\r\nSADD\r\n$68\r\nserials::" + KI.exp_date_id(HOURS[0] - 1) + b"::") and want.endswith(b"*3\r\n$4\r\nSADD\r\n$12\r\nserials::zzz\r\n$1\r\n\x05\r\n")
    # a chunk split by a host piece: sets of 100 and 150 records with a piece between them fit one chunk of 257 / 300
    d = DIGESTS[1]
    sets = {KI.set_key(HOURS[0], d): [struct.pack(">H", v) for v in range(100)],
            KI.set_key(HOURS[1], d): [struct.pack(">H", v) * 9 for v in range(150)],
            KI.set_key(HOURS[2], d): [struct.pack(">H", v) * 20 for v in range(299)]}
    img = with_host_pairs(sets, [(KI.set_key(HOURS[0], d), b"\x77" * 44), (KI.set_key(HOURS[2], d), b"\x78" * 41)])
    check(eng, img, 64, phases=(0, 13))
    c = KC.make("uniform", DIGESTS[:9], HOURS, [1, 63, 64, 65, 255, 256, 257, 300], seed=15)
    check(eng, c.image, 512)
    check(eng, KC.make("twins", DIGESTS[:4], HOURS, 0, seed=11).image, 3)


# ---- 5. rejection

def damaged(img, edit):
    meta, rec = KC.split(img)
    edit(rec)
    return meta + rec.tobytes()


def rejected(e, img, per=512):
    cap = 256 * (len(img) // 48) + 4 * len(img) + 256
    for device in (False, True):
        rc, _, got = call(e, img, per, device, cap)
        assert rc == N.E_INVAL and got is None


def test_bad_records(eng):
    c = KC.make("uniform", DIGESTS[:3], HOURS, [300, 301, 299], seed=17)
    img = shuffled(c.image)
    lens = KC.record_lens(img)
    n = len(lens)
    before = table(eng)
    for i in (0, 127, 128, n // 2, n - 1):
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
                KI.image_resp(x)
            rejected(eng, x)
    assert table(eng) == before


def test_a_bad_record_in_a_later_chunk_leaves_nothing_written(eng, monkeypatch):
    monkeypatch.setenv("CTMR_KNOWN_RESP_CHUNK", "300")
    c = KC.make("uniform", DIGESTS[:3], HOURS, [300, 301, 299], seed=17)
    n = len(KC.record_lens(c.image))
    rejected(eng, damaged(c.image, lambda rec: rec["len"].__setitem__(n - 1, 41)))
    check(eng, c.image)


def test_hours_outside_the_years_and_members_per_command(eng):
    ok = raw_image([(HOURS[0], DIGESTS[0], [b"\x01"]), (HOURS[1], DIGESTS[1], [b"\x02"])])
    for h in (KI._HOUR_LO - 1, KI._HOUR_HI, 2 ** 31 - 1, -2 ** 31):
        bad = raw_image([(HOURS[0], DIGESTS[0], [b"\x01"]), (h, DIGESTS[1], [b"\x02"])])
        KI.parse(bad)
        with pytest.raises(KI.ImageError):
            KI.image_resp(bad)
        rejected(eng, bad)
    for per in (0, (1 << 20) + 1, 0xffffffff):
        rejected(eng, ok, per)
        with pytest.raises(ctmr.CtmrError) as ex:
            eng.known_image_resp(ok, per)
        assert ex.value.code == N.E_INVAL
    check(eng, ok, 1 << 20)


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
    outside = with_host_pairs(c.sets, [(b"crl::x", b"\x01")])
    before = table(eng)
    for x in (gap, empty, ordinal, order, magic, version, members, outside, img[:-48], img + b"\0" * 48, img[:40]):
        with pytest.raises(KI.ImageError):
            KI.image_resp(bytes(x))
        with pytest.raises(ctmr.CtmrError) as ex:
            eng.known_import(bytes(x))
        assert ex.value.code == N.E_INVAL
        rejected(eng, bytes(x))
    assert table(eng) == before and eng.known_export() == KI.build({})


# ---- 6. the whole path

def test_the_stream_loads_into_a_fresh_engine():
    issuers = synth.issuers(CFG)
    e = engine(issuers, table_slots=1 << 13)
    e.map_batch(synth.host_batch(CFG, 0, 2500))
    for k in range(2):                                                        # host-section members: above 40 octets
        for L in (41, 50, 60):
            e.set_insert("serials::%s::%s" % (KI.exp_date_id(491000).decode(), e.issuer_id(k)), bytes([k + 1]) * L)
    e.set_known_order(N.KNOWN_ORDER_SORTED)
    img = e.known_export()
    e.set_known_order(N.KNOWN_ORDER_ANY)
    assert KI.parse(img).n_host_members == 6
    sh = shuffled(img, 6)
    before = (state(e), table(e), e.issuer_counts().tobytes())
    stream = e.known_image_resp(sh, 100)
    assert stream == TWIN(sh, 100) != TWIN(img, 100)
    assert e.known_resp(100) == TWIN(img, 100) and e._known_order == N.KNOWN_ORDER_ANY
    assert (state(e), table(e), e.issuer_counts().tobytes()) == before
    e.set_known_order(N.KNOWN_ORDER_SORTED)
    assert e.known_resp() == TWIN(img, 512) and e._known_order == N.KNOWN_ORDER_SORTED and e.known_export() == img
    fresh = engine(issuers, order=[5, 3, 1, 0, 2, 4], table_slots=1 << 13)
    st = redis_load(GpuRemoteCache(fresh), io.BytesIO(stream))
    assert st["inserted"] == KI.parse(img).total
    fresh.set_known_order(N.KNOWN_ORDER_SORTED)
    assert fresh.known_export() == e.known_merge(N.KNOWN_UNION, sh) == img
    fresh.close()
    e.close()


def test_an_engine_of_hand_built_certificates():
    e = hand_built_engine()       # serials of 1..45 octets, two issuers sharing an SPKI, an unregistered issuer
    before = (state(e), table(e), e.issuer_counts().tobytes())
    e.set_known_order(N.KNOWN_ORDER_SORTED)
    img = e.known_export()
    e.set_known_order(N.KNOWN_ORDER_ANY)
    im = KI.parse(img)
    assert im.n_host_members > 6 and {len(m) for v in im.sets.values() for m in v} >= set(range(1, 46))
    other = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)       # an engine that knows no issuer
    for per in (1, 5, 512):
        want = TWIN(img, per)
        assert e.known_resp(per) == want == other.known_image_resp(img, per)
        check(other, img, per)
    assert KI.from_resp(TWIN(img, 512)) == KI.union(img)
    assert (state(e), table(e), e.issuer_counts().tobytes()) == before and e._known_order == N.KNOWN_ORDER_ANY
    other.close()
    e.close()


@pytest.mark.parametrize("mode", ["owner", "bloom"])
@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_a_group_s_stream_is_the_twin_of_its_image(mode, world):
    issuers = synth.issuers(CFG)
    engines = [engine(issuers) for _ in range(world)]
    g = Group.local(engines)
    if mode == "bloom":
        g.bloom_config(1 << 16)
    base = 0
    for b in [synth.host_batch(CFG, lo, 2400) for lo in (0, 1800)]:
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
    img = g.known_export()
    assert KI.parse(img).n_members > 2000
    assert g.known_resp() == TWIN(img, 512)
    assert g.known_resp(members_per_command=3) == TWIN(img, 3)
    g.close()
    for x in engines:
        x.close()
