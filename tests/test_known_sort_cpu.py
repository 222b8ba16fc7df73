"""known_image.sort, the CPU twin of Engine.known_sort (include/ctmr.h ctmr_known_sort*): the order inside
a set is the order sorted() gives the members' bytes.  No GPU needed; tests/test_gpu_known_sort.py takes its expected
bytes from here."""
import struct

import numpy as np
import pytest

from ct_mapreduce_amd import known_image as KI, _native as N
from tests import known_corpus as KC

DIGESTS = [bytes([k]) * 32 for k in (9, 3, 200)]
HOURS = [490999, 491000]


def shuffled(img, seed=1):
    """The image with the records of every set in a random order."""
    meta, rec = KC.split(img)
    sets_of = KC.record_sets(img)
    rng = np.random.default_rng(seed)
    for s in np.unique(sets_of):
        at = np.nonzero(sets_of == s)[0]
        rec[at] = rec[rng.permutation(at)]
    return meta + rec.tobytes()


def members_by_set(img):
    """[[member bytes in record order] per set of the members section]."""
    _, rec = KC.split(img)
    sets_of = KC.record_sets(img)
    out = [[] for _ in range(int(sets_of.max()) + 1 if len(sets_of) else 0)]
    for s, l, m in zip(sets_of, rec["len"], rec["serial"]):
        out[s].append(bytes(m[:int(l)]))
    return out


def with_repeats(img):
    meta, rec = KC.split(img)
    sets_of = KC.record_sets(img)
    for s in np.unique(sets_of):
        at = np.nonzero(sets_of == s)[0]
        if len(at) >= 6:
            rec[at[1]] = rec[at[-1]]
            rec[at[len(at) // 2]] = rec[at[-1]]
    return meta + rec.tobytes()


@pytest.mark.parametrize("mix", KC.MIXES)
def test_orders_every_set_as_sorted_orders_bytes(mix):
    c = KC.make(mix, DIGESTS, HOURS, [300, 1, 2, 257, 64, 700], seed=3)
    img = shuffled(c.image)
    assert img != c.image
    out = KI.sort(img)
    meta, _ = KC.split(img)
    assert len(out) == len(img) and out[:len(meta)] == meta
    for before, after in zip(members_by_set(img), members_by_set(out)):
        assert after == sorted(before)
    # canonical: no repeats and every key parses, so the canonical writer gives the same bytes
    assert out == c.image == KI.build(KI.parse(img).sets) == KC.image(KI.parse(img).sets)
    assert KI.sort(out) == out


def test_keeps_repeats():
    c = KC.make("uniform", DIGESTS, HOURS, [40, 7, 300], seed=5)
    img = shuffled(with_repeats(c.image), seed=2)
    out = KI.sort(img)
    n = 0
    for before, after in zip(members_by_set(img), members_by_set(out)):
        assert after == sorted(before)
        n += len(before) - len(set(before))
    assert n > 0 and KI.sort(out) == out
    assert sorted(bytes(r) for r in KC.split(out)[1].view(np.uint8).reshape(-1, 48)) == \
        sorted(bytes(r) for r in KC.split(img)[1].view(np.uint8).reshape(-1, 48))


def test_a_prefix_comes_before_the_longer_string():
    want = [b"", b"\x00", b"\x00\x00", b"\x00\x01", b"\x01"]
    key = KI.set_key(HOURS[0], DIGESTS[0])
    img = KC.image({key: want})
    assert members_by_set(img) == [want]
    meta, rec = KC.split(img)
    for perm in ([4, 3, 2, 1, 0], [2, 0, 4, 1, 3], [1, 2, 0, 3, 4]):
        out = KI.sort(meta + rec[perm].tobytes())
        assert members_by_set(out) == [want] and out == img
    # padding alone cannot tell b"", 00 and 00 00 apart: serial_len does
    assert (rec["serial"][:3] == 0).all() and rec["len"][:3].tolist() == [0, 1, 2]


def test_octets_compare_unsigned_and_past_the_first_word():
    key = KI.set_key(HOURS[0], DIGESTS[0])
    ms = [b"\x7f" * 9, b"\x80", b"\xff" * 40, b"\x00" * 40, b"\x01" * 8 + b"\x02", b"\x01" * 8 + b"\x80", b"\x01" * 8,
          b"\x05" * 39 + b"\x01", b"\x05" * 39 + b"\xfe", b"\x05" * 39]
    img = KC.image({key: ms})
    meta, rec = KC.split(img)
    out = KI.sort(meta + rec[::-1].tobytes())
    assert members_by_set(out) == [sorted(ms)] and out == img


def test_empty_and_single():
    assert KI.sort(KI.build({})) == KI.build({})
    one = KI.build({KI.set_key(HOURS[0], DIGESTS[0]): [b"\x01\x02"]})
    assert KI.sort(one) == one


def test_the_host_section_stays():
    key = KI.set_key(HOURS[0], DIGESTS[0])
    img = KI.build({key: [b"\x09" * 41, b"\x03", b"\x02"], b"serials::odd": [b"z", b"a"]})
    assert KI.parse(img).n_host_members == 3
    meta, rec = KC.split(img)
    out = KI.sort(meta + rec[::-1].tobytes())
    assert out == img


def test_rejects_what_parse_rejects():
    c = KC.make("uniform", DIGESTS, HOURS, [30], seed=7)
    n_iss = KI._HEADER.unpack_from(c.image, 0)[3]
    so = 64 + 32 * n_iss
    bad = []
    b = bytearray(c.image); b[0] ^= 1; bad.append(bytes(b))
    b = bytearray(c.image); b[-48] = 41; bad.append(bytes(b))
    meta, rec = KC.split(c.image)
    short = int(np.nonzero(rec["len"] < 40)[0][-1])
    rec["serial"][short, 39] = 1                                                 # padding that is not zero
    bad.append(meta + rec.tobytes())
    b = bytearray(c.image); struct.pack_into("<I", b, so + 4, n_iss); bad.append(bytes(b))
    b = bytearray(c.image); struct.pack_into("<Q", b, so + 24 + 8, 31); bad.append(bytes(b))
    bad.append(c.image[:-1])
    for img in bad:
        with pytest.raises(KI.ImageError):
            KI.parse(img)
        with pytest.raises(KI.ImageError):
            KI.sort(img)


def test_binding_names_the_calls_and_the_orders():
    assert (N.KNOWN_ORDER_ANY, N.KNOWN_ORDER_SORTED) == (0, 1)
    for name in ("ctmr_set_known_order", "ctmr_known_sort", "ctmr_known_sort_device"):
        assert name in N.SIGNATURES and hasattr(N.lib(), name)
