"""The known-certificate image without a GPU: ct_mapreduce_amd.known_image writes, reads and refuses images as the
library does (include/ctmr.h), and converts them to and from redis_dump's stream."""
import hashlib
import io
import struct

import numpy as np
import pytest

from ct_mapreduce_amd import known_image as KI
from ct_mapreduce_amd import _native as N
from ct_mapreduce_amd.remote_cache import redis_dump
from tests.storage_mirror import MockRemoteCache
from tests.test_abi import declared_functions

HOUR0 = 491000   # 2026-01-05-08


def _digest(i):
    return hashlib.sha256(b"issuer %d" % i).digest()


def sample_sets():
    """Two issuers over three hours, short and long serials, a key whose issuer ID is not a digest."""
    sets = {}
    for i in range(2):
        for h in range(3):
            key = KI.set_key(HOUR0 + h * 7, _digest(i))
            sets[key] = [bytes([i, h, k]) * (1 + k % 7) for k in range(5 + 3 * h + i)]
    key = KI.set_key(HOUR0, _digest(1))
    sets[key] += [b"\x01" * 41, b"\x02" * 60, b"\x00" * 40, b""]
    sets[b"serials::2026-01-05-08::not-an-issuer-id"] = [b"\x07\x08", b"\x09" * 45]
    return sets


def _norm(sets):
    return {k: sorted(set(v)) for k, v in sets.items()}


def test_build_parse_round_trip():
    sets = sample_sets()
    img = KI.build(sets)
    k = KI.parse(img)
    assert k.sets == _norm(sets)
    assert k.n_host_members == 2 + 2 and k.n_members == sum(len(set(v)) for v in sets.values()) - 4
    assert k.n_sets == 6 and len(k.issuers) == 2 and k.issuers == sorted(k.issuers)
    assert KI.build(k.sets) == img                       # canonical
    magic, version, hdr, n_iss, flags, n_sets, n_mem, host_bytes, n_host, res = KI._HEADER.unpack_from(img, 0)
    meta = (64 + 32 * n_iss + 24 * n_sets + host_bytes + 63) // 64 * 64
    assert (magic, version, hdr, flags, res) == (b"CTMRKNWN", 1, 64, 0, 0) and len(img) == meta + 48 * n_mem
    # the sets of the members section are in the order of their keys (the order ctmr_keys returns)
    keys = [KI.set_key(struct.unpack_from("<i", img, 64 + 32 * n_iss + 24 * s)[0],
                       k.issuers[struct.unpack_from("<I", img, 64 + 32 * n_iss + 24 * s + 4)[0]]) for s in range(n_sets)]
    assert keys == sorted(keys)


def test_empty_image():
    img = KI.build({})
    assert len(img) == 64 and KI.parse(img).sets == {}


def test_exp_date_id_matches_the_reference_format():
    assert KI.exp_date_id(0) == b"1970-01-01-00"
    assert KI.exp_date_id(-1) == b"1969-12-31-23"
    assert KI.exp_date_id(HOUR0) == b"2026-01-05-08"
    assert KI.parse_key(KI.set_key(HOUR0, _digest(3))) == (HOUR0, _digest(3))
    assert KI.parse_key(b"serials::2026-02-30-01::" + KI.issuer_id(_digest(3))) is None     # no Feb 30
    assert KI.parse_key(b"serials::2026-01-05-08::abc") is None


def _patch(img, off, fmt, value):
    b = bytearray(img)
    struct.pack_into(fmt, b, off, value)
    return bytes(b)


def _layout(img):
    _, _, _, n_iss, _, n_sets, n_mem, host_bytes, n_host, _ = KI._HEADER.unpack_from(img, 0)
    so = 64 + 32 * n_iss
    meta = (so + 24 * n_sets + host_bytes + 63) // 64 * 64
    return so, so + 24 * n_sets, meta, n_sets, n_mem


def malformed_images():
    """(name, image) for every malformation the library refuses with CTMR_E_INVAL."""
    img = KI.build(sample_sets())
    so, ho, meta, n_sets, n_mem = _layout(img)
    out = [
        ("magic", b"X" + img[1:]),
        ("version", _patch(img, 8, "<I", 2)),
        ("header_bytes", _patch(img, 12, "<I", 128)),
        ("flags", _patch(img, 20, "<I", 1)),
        ("reserved", _patch(img, 56, "<Q", 1)),
        ("short", img[:-48]),
        ("long", img + b"\0" * 48),
        ("n_members", _patch(img, 32, "<Q", n_mem + 1)),
        ("ordinal", _patch(img, so + 4, "<I", 2)),
        ("gap", _patch(img, so + 24 + 8, "<Q", struct.unpack_from("<Q", img, so + 24 + 8)[0] + 1)),
        ("overlap", _patch(img, so + 24 + 8, "<Q", struct.unpack_from("<Q", img, so + 24 + 8)[0] - 1)),
        ("empty", _patch(img, so + 16, "<Q", 0)),
        ("cover", _patch(img, so + 24 * (n_sets - 1) + 16, "<Q", struct.unpack_from("<Q", img, so + 24 * (n_sets - 1) + 16)[0] - 1)),
        ("order", img[:so] + img[so + 24:so + 32] + img[so + 8:so + 24] + img[so:so + 8] + img[so + 32:]),
        ("serial_len", _patch(img, len(img) - 48, "<Q", 41)),
        ("padding", _patch(img, len(img) - 1, "<B", 1)),
        ("meta_padding", _patch(img, meta - 1, "<B", 1) if (ho + struct.unpack_from("<Q", img, 40)[0]) < meta else None),
        ("host_count", _patch(img, 48, "<Q", 3)),
        ("host_order", None),
        ("host_prefix", None),
    ]
    # host section: swap the first two entries; rename the first key's prefix
    hb = img[ho:ho + struct.unpack_from("<Q", img, 40)[0]]
    ents, q = [], 0
    while q < len(hb):
        kl = struct.unpack_from("<I", hb, q)[0]
        ml = struct.unpack_from("<I", hb, q + 4 + kl)[0]
        ents.append(hb[q:q + 8 + kl + ml])
        q += 8 + kl + ml
    swapped = ents[1] + ents[0] + b"".join(ents[2:])
    out[-2] = ("host_order", img[:ho] + swapped + img[ho + len(hb):])
    out[-1] = ("host_prefix", img[:ho + 4] + b"X" + img[ho + 5:])
    return [(n, b) for n, b in out if b is not None]


@pytest.mark.parametrize("name,bad", malformed_images(), ids=[n for n, _ in malformed_images()])
def test_malformed_images_are_refused(name, bad):
    with pytest.raises(KI.ImageError):
        KI.parse(bad)


def _mock_cache(sets):
    c = MockRemoteCache()
    for k, ms in sets.items():
        for m in ms:
            c.SetInsert(k, m)
    c.SetInsert(b"crl::x", b"y")                        # not a known-certificate set: not in the image, not dumped
    return c


def test_to_resp_is_redis_dump_of_the_same_sets():
    sets = sample_sets()
    sets[KI.set_key(HOUR0 + 100, _digest(5))] = [b"%04d" % i for i in range(1300)]   # more than one SADD of 512
    want = io.BytesIO()
    redis_dump(_mock_cache(sets), want, patterns=("serials::*",))
    got = io.BytesIO()
    KI.to_resp(KI.build(sets), got)
    assert got.getvalue() == want.getvalue()


def test_from_resp_round_trips_redis_dump():
    sets = sample_sets()
    s = io.BytesIO()
    redis_dump(_mock_cache(sets), s)                    # every set pattern: crl:: is skipped by from_resp
    img = KI.from_resp(s.getvalue())
    assert img == KI.build(sets)
    assert KI.parse(img).sets == _norm(sets)
    again = io.BytesIO()
    KI.to_resp(img, again)
    assert KI.from_resp(again.getvalue()) == img


def test_the_header_declares_the_image_entry_points():
    names = declared_functions()
    for n in ("ctmr_known_export", "ctmr_known_export_device", "ctmr_known_import", "ctmr_known_import_device"):
        assert n in names and n in N.SIGNATURES
    import ctypes as C
    assert C.sizeof(N.KnownImageInfo) == 5 * 8 + 2 * 4
    assert C.sizeof(N.KnownImportStats) == 6 * 8
    assert KI.MEMBER_DTYPE.itemsize == 48 and np.dtype(KI.MEMBER_DTYPE)["len"].itemsize == 8
