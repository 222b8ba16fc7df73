"""The Redis protocol stream of an image without a GPU (include/ctmr.h ctmr_known_image_resp): the CPU
twin known_image.image_resp against remote_cache.redis_dump of the parsed sets, against redis_load / from_resp of its own
output, and against the per-record byte formula and the sizing bound the library's count pass and header state."""
import io
import struct

import numpy as np
import pytest

from ct_mapreduce_amd import known_image as KI
from ct_mapreduce_amd.remote_cache import _resp, redis_dump, redis_load
from tests import known_corpus as KC
from tests.test_image_lists_cpu import raw_image
from tests.test_known_merge_cpu import with_host_pairs
from tests.test_known_sort_cpu import shuffled, with_repeats

DIGESTS = [bytes([k]) * 31 + bytes([255 - k]) for k in range(1, 6)]
HOURS = [491000, 491003, 491027]
H = HOURS[0]
PERS = (1, 2, 3, 512)


def dump(sets, per):
    out = io.BytesIO()
    redis_dump(KI._SetsCache(sets), out, patterns=("serials::*",), members_per_command=per)
    return out.getvalue()


def commands(stream):
    """[[argument bytes]] of a stream of RESP arrays of bulk strings."""
    out, pos = [], 0
    while pos < len(stream):
        e = stream.index(b"\r\n", pos)
        assert stream[pos:pos + 1] == b"*"
        argc, pos, args = int(stream[pos + 1:e]), e + 2, []
        for _ in range(argc):
            e = stream.index(b"\r\n", pos)
            assert stream[pos:pos + 1] == b"$"
            n = int(stream[pos + 1:e])
            args.append(stream[e + 2:e + 2 + n])
            assert stream[e + 2 + n:e + 4 + n] == b"\r\n"
            pos = e + 4 + n
        out.append(args)
    return out


def loaded(stream):
    """({key: sorted members}, {key: EXPIREAT seconds}) of a stream, through redis_load."""
    class Cache(KI._SetsCache):
        def __init__(self):
            super().__init__()
            self.expire = {}

        def ExpireAt(self, key, unix_seconds):
            assert key not in self.expire
            self.expire[bytes(key)] = unix_seconds
    c = Cache()
    redis_load(c, io.BytesIO(stream))
    return {k: sorted(v) for k, v in c.sets.items()}, c.expire


def round_trips(img, per):
    s = KI.image_resp(img, per)
    assert KI.from_resp(s) == KI.union(img)
    sets, _ = loaded(s)
    assert sets == KI.parse(img).sets
    return s


def header_counts(img):
    _, _, _, _, _, n_sets, n_mem, host_bytes, n_host, _ = KI._HEADER.unpack_from(img, 0)
    return n_mem, n_sets, host_bytes, n_host


def formula_bytes(img, per):
    """Σ resp_record_bytes over the member records of an image without a host section."""
    n_iss, n_sets = KI._HEADER.unpack_from(img, 0)[3], KI._HEADER.unpack_from(img, 0)[5]
    lens = KC.record_lens(img)
    total = 0
    for s in range(n_sets):
        eh, _, first, count = KI._SET.unpack_from(img, 64 + 32 * n_iss + 24 * s)
        total += sum(KI.resp_record_bytes(p, count, int(lens[first + p]), eh, per) for p in range(count))
    return total


@pytest.mark.parametrize("mix", KC.MIXES)
def test_canonical_images_of_every_mix_equal_redis_dump(mix):
    c = KC.make(mix, DIGESTS, HOURS, [1, 2, 3, 65, 300], seed=5)
    dev_keys = {k for k, _ in KI.records(c.image)[0]}
    host_keys = {k for k, _ in KI.records(c.image)[1]}
    for per in PERS:
        s = round_trips(c.image, per)
        if mix != "twins":
            assert not dev_keys & host_keys
            assert s == dump(KI.parse(c.image).sets, per)
            assert len(s) == formula_bytes(c.image, per)
        else:
            # serials above 40 octets sit in the host section under their set's key: SADD commands of their own
            assert dev_keys & host_keys
            assert s != dump(KI.parse(c.image).sets, per)
        assert len(s) <= KI.resp_bound(*header_counts(c.image), per)
    # a corpus whose only host keys have no member records: still redis_dump's bytes
    sets = dict(c.sets) if mix != "twins" else {k: [m for m in v if len(m) <= 40] for k, v in c.sets.items()}
    sets[b"serials::2026-01-05::day"] = [b"\x01", b"\x02" * 50, b""]
    sets[KI.PREFIX + KI.exp_date_id(H) + b"::someone"] = [b"\x07" * 41]
    img = KC.image(sets)
    for per in PERS:
        assert KI.image_resp(img, per) == dump(KI.parse(img).sets, per)


def test_the_default_is_512_members_per_command():
    img = raw_image([(H, DIGESTS[0], [struct.pack(">H", v) for v in range(1025)])])
    cmds = commands(KI.image_resp(img))
    assert [(c[0], len(c)) for c in cmds] == [(b"SADD", 514), (b"SADD", 514), (b"SADD", 3), (b"EXPIREAT", 3)]
    assert KI.image_resp(img) == KI.image_resp(img, 512) != KI.image_resp(img, 513)
    for bad in (0, -1, (1 << 20) + 1):
        with pytest.raises(ValueError):
            KI.image_resp(img, bad)
    assert len(commands(KI.image_resp(img, 1 << 20))) == 2


def test_shuffled_and_repeated_records_stay_as_they_lie():
    c = KC.make("uniform", DIGESTS[:3], HOURS, [40, 1, 7], seed=9)
    sh = with_repeats(shuffled(c.image, 3))
    assert KI.sort(sh) != sh
    want = [m for _, m in KI.records(sh)[0]]
    for per in PERS:
        s = round_trips(sh, per)
        got = [m for cmd in commands(s) if cmd[0] == b"SADD" for m in cmd[2:]]
        assert got == want                                   # image order, repeats kept
        assert len(s) == formula_bytes(sh, per)
        assert s != KI.image_resp(KI.union(sh), per)
    empty = raw_image([(H, DIGESTS[0], [b"", b"", b"\x00"])])
    assert KI.image_resp(empty, 2).count(b"$0\r\n\r\n") == 2
    round_trips(empty, 2)


def test_a_key_in_both_sections_is_one_key_with_the_expireat_last():
    i0 = KI.issuer_id(DIGESTS[0])
    k = KI.set_key(H, DIGESTS[0])
    k2 = KI.set_key(H + 2, DIGESTS[0])
    between = KI.PREFIX + KI.exp_date_id(H + 1) + b"::" + i0 + b"x"
    sets = {k: [b"\x05", b"\x07" * 40, b"\x09"], k2: [b"\x06"]}
    pairs = [(k, b"\x00" * 41), (k, b"\x08" * 50), (k, b"\x0a" * 41), (between, b"\x01")]
    img = with_host_pairs(sets, pairs)
    t, t2 = str(H * 3600).encode(), str((H + 2) * 3600).encode()
    assert KI.image_resp(img, 2) == b"".join([
        _resp(b"SADD", k, b"\x05", b"\x07" * 40), _resp(b"SADD", k, b"\x09"),
        _resp(b"SADD", k, b"\x00" * 41, b"\x08" * 50), _resp(b"SADD", k, b"\x0a" * 41), _resp(b"EXPIREAT", k, t),
        _resp(b"SADD", between, b"\x01"), _resp(b"EXPIREAT", between, str((H + 1) * 3600).encode()),
        _resp(b"SADD", k2, b"\x06"), _resp(b"EXPIREAT", k2, t2)])
    for per in PERS:
        s = round_trips(img, per)
        assert [c[1] for c in commands(s) if c[0] == b"EXPIREAT"] == [k, between, k2]
        assert len(s) <= KI.resp_bound(*header_counts(img), per)


def test_day_resolution_unparsable_and_short_keys():
    i0 = KI.issuer_id(DIGESTS[0])
    day = KI.exp_date_id(H)[:10]
    sets = {KI.set_key(H, DIGESTS[0]): [b"\x01"]}
    pairs = [(KI.PREFIX + day + b"::odd", b"\xaa" * 300),              # day resolution: the day's first second
             (KI.PREFIX + KI.exp_date_id(H)[:11] + b"5::" + i0, b"\x02"),  # a one-digit hour
             (KI.PREFIX + b"2026-02-30-01::odd", b"\xbb"),              # no such day
             (KI.PREFIX + b"10000-01-01-00::odd", b"\xcc"),             # five year digits
             (KI.PREFIX + b"2026-13-01::odd", b"\xdd"),
             (KI.PREFIX + b"x", b"\xee"), (KI.PREFIX, b"\xef"),         # no second "::"
             (KI.PREFIX + day + b":odd", b"\xf0"),
             (KI.PREFIX + b"::odd", b"\xf1"), (KI.PREFIX + day + b"::", b"\xf2"), (KI.PREFIX + day + b"::a::b", b"\xf3")]
    img = with_host_pairs(sets, pairs)
    for per in (1, 512):
        s = round_trips(img, per)
        _, expire = loaded(s)
        d0 = (H // 24) * 86400
        assert expire == {KI.set_key(H, DIGESTS[0]): H * 3600, KI.PREFIX + day + b"::odd": d0,
                          KI.PREFIX + KI.exp_date_id(H)[:11] + b"5::" + i0: d0 + 5 * 3600,
                          KI.PREFIX + day + b"::": d0, KI.PREFIX + day + b"::a::b": d0}
        keys = [c[1] for c in commands(s) if c[0] == b"SADD"]
        assert keys == sorted(keys) and len(set(keys)) == len(pairs) + 1
        assert len(s) <= KI.resp_bound(*header_counts(img), per)


def test_expiry_hours_at_the_edges_and_outside():
    lo, hi = KI._HOUR_LO, KI._HOUR_HI
    assert KI.exp_date_id(lo) == b"0000-01-01-00" and KI.exp_date_id(hi - 1) == b"9999-12-31-23"
    hours = [0, 1, -1, lo, lo + 1, hi - 1, hi - 2, -24 * 365 * 1000]
    img = raw_image([(h, DIGESTS[0], [b"\x01", b"\x02"]) for h in hours])
    s = round_trips(img, 512)
    _, expire = loaded(s)
    assert expire == {KI.set_key(h, DIGESTS[0]): h * 3600 for h in hours}
    assert b"$12\r\n-62167219200\r\n" in s and b"$12\r\n253402297200\r\n" in s and b"$1\r\n0\r\n" in s and b"$5\r\n-3600\r\n" in s
    assert len(s) == formula_bytes(img, 512)
    # year 0000 is beyond calendar.timegm, and so beyond redis_dump; from 0001 on the two agree
    ok = raw_image([(h, DIGESTS[0], [b"\x01", b"\x02"]) for h in hours if h >= KI._days_from_civil(1, 1, 1) * 24])
    assert KI.image_resp(ok, 512) == dump(KI.parse(ok).sets, 512)
    for h in (lo - 1, hi, 2 ** 31 - 1, -2 ** 31):
        bad = raw_image([(H, DIGESTS[0], [b"\x01"]), (h, DIGESTS[1], [b"\x02"])])
        KI.parse(bad)
        with pytest.raises(KI.ImageError):
            KI.image_resp(bad, 512)


def test_everything_parse_rejects_is_rejected():
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
    long_ = bytearray(img)
    struct.pack_into("<Q", long_, len(img) - 48, 41)
    pad = bytearray(img)
    pad[-1] = 1
    outside = with_host_pairs(c.sets, [(b"crl::x", b"\x01")])
    for x in (gap, empty, ordinal, order, magic, version, long_, pad, outside, img[:-48], img + b"\0" * 48, img[:40]):
        with pytest.raises(KI.ImageError):
            KI.parse(bytes(x))
        with pytest.raises(KI.ImageError):
            KI.image_resp(bytes(x), 512)


def test_the_byte_formula_its_maximum_and_the_bound():
    # the worst record: a one-member set, 40 octets, a 12-character timestamp
    assert KI.resp_record_bytes(0, 1, 40, KI._HOUR_HI - 1, 512) == KI.resp_record_bytes(0, 1, 40, KI._HOUR_LO, 1) == 248
    worst = max(KI.resp_record_bytes(p, c, L, h, per)
                for per in (1, 2, 512, 999_998, 1 << 20) for c in (1, 2, per, per + 1, (1 << 20) + 5) for p in {0, c - 1, min(per, c - 1)}
                for L in (9, 10, 40) for h in (KI._HOUR_LO, 0, KI._HOUR_HI - 1))
    assert worst == 248
    rng = np.random.default_rng(23)
    for trial in range(12):
        sizes = [int(v) for v in rng.integers(1, 40, size=9)]
        sets = [(int(H + rng.integers(-10 ** 6, 10 ** 6)), DIGESTS[k % 5],
                 [bytes(rng.integers(0, 256, size=int(L), dtype=np.uint8).tolist()) for L in rng.integers(0, 41, size=n)])
                for k, n in enumerate(sizes)]
        sets = list({KI.set_key(h, d): (h, d, ms) for h, d, ms in sets}.values())
        img = raw_image(sets)
        for per in (1, 2, 3, 5, 512):
            s = KI.image_resp(img, per)
            assert len(s) == formula_bytes(img, per)
            assert len(s) <= KI.resp_bound(*header_counts(img), per)
    # the bound with the largest argument counts and a host section of long keys and members
    big = raw_image([(H, DIGESTS[0], [struct.pack(">I", v) for v in range(100_001)])])
    assert len(commands(KI.image_resp(big, 99_998))[0]) == 100_000
    assert len(KI.image_resp(big, 99_998)) == formula_bytes(big, 99_998) <= KI.resp_bound(*header_counts(big), 99_998)
    pairs = [(KI.PREFIX + KI.exp_date_id(H + k) + b"::" + b"k" * (1 + 37 * k), b"\x01" * (k * 101)) for k in range(12)]
    pairs += [(pairs[3][0], b"\x02")]
    img = with_host_pairs({KI.set_key(H, DIGESTS[0]): [b"\x01"]}, pairs)
    for per in (1, 2, 512):
        assert len(round_trips(img, per)) <= KI.resp_bound(*header_counts(img), per)
