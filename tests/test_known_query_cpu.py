"""known_image.query / subtract / records: the CPU twins of Engine.known_query / known_remove, against
hand-written cases and every tests/known_corpus mix.  No GPU."""
import numpy as np
import pytest

from ct_mapreduce_amd import known_image as KI
from tests import known_corpus as KC

D0, D1 = bytes(range(32)), bytes(range(1, 33))
H0, H1 = 491000, 491016
K00, K01, K10 = KI.set_key(H0, D0), KI.set_key(H0, D1), KI.set_key(H1, D0)


def test_records_keep_image_order_and_sections():
    sets = {K00: [b"\x02", b"\x01", b"\x01\x00", b"z" * 41], K10: [b""], b"serials::odd": [b"q"]}
    img = KI.build(sets)
    dev, host = KI.records(img)
    assert dev == [(K00, b"\x01"), (K00, b"\x01\x00"), (K00, b"\x02"), (K10, b"")]
    assert host == [(K00, b"z" * 41), (b"serials::odd", b"q")]
    assert KI.records(KI.build({})) == ([], [])


def test_near_misses_by_hand():
    m = bytes(range(1, 21))
    held = {K00: [m, m + b"\x00", b"", b"y" * 50]}
    ask = {K00: [m, bytes([9]) + m[1:], m[:-1], m + b"\x00", m + b"\x00\x00", b"", b"\x00", b"y" * 50, b"y" * 51],
           K10: [m], K01: [m]}
    img = KI.build(ask)
    dev, host = KI.records(img)
    fl, hf = KI.query(img, held)
    assert fl.dtype == hf.dtype == np.uint8
    got = {r: int(f) for r, f in zip(dev, fl)}
    assert got == {(K00, m): 1, (K00, bytes([9]) + m[1:]): 0, (K00, m[:-1]): 0, (K00, m + b"\x00"): 1,
                   (K00, m + b"\x00\x00"): 0, (K00, b""): 1, (K00, b"\x00"): 0, (K10, m): 0, (K01, m): 0}
    assert dict(zip(host, hf.tolist())) == {(K00, b"y" * 50): 1, (K00, b"y" * 51): 0}
    assert KI.query(img, {}) [0].sum() == 0 and KI.query(img, ask)[0].all() and KI.query(img, ask)[1].all()


def test_duplicate_records_get_the_same_answer_and_are_subtracted_once():
    held = {K00: [b"a", b"b", b"c"], K01: [b"a"]}
    meta, rec = KC.split(KI.build({K00: [b"a", b"b", b"x"], K01: [b"a", b"d"]}))
    rec[1] = rec[0]                                   # K00: a, a, x
    img = meta + rec.tobytes()
    dev, _ = KI.records(img)
    assert dev == [(K00, b"a"), (K00, b"a"), (K00, b"x"), (K01, b"a"), (K01, b"d")]
    assert KI.query(img, held)[0].tolist() == [1, 1, 0, 1, 0]
    assert KI.subtract(held, img) == {K00: [b"b", b"c"]}          # K01 lost its last member: the key is gone


def test_empty_image_and_empty_sets():
    img = KI.build({})
    fl, hf = KI.query(img, {K00: [b"a"]})
    assert len(fl) == len(hf) == 0
    assert KI.subtract({K00: [b"b", b"a"]}, img) == {K00: [b"a", b"b"]}
    assert KI.subtract({}, KI.build({K00: [b"a"]})) == {}


def test_a_malformed_image_is_refused():
    img = bytearray(KI.build({K00: [b"a"]}))
    img[-1] = 1                                       # a padding octet
    for f in (lambda: KI.records(bytes(img)), lambda: KI.query(bytes(img), {}), lambda: KI.subtract({}, bytes(img))):
        with pytest.raises(KI.ImageError):
            f()


@pytest.mark.parametrize("mix", KC.MIXES)
def test_subtract_then_query_is_all_zero(mix):
    sizes = {"uniform": [300, 1, 257], "tiny": [200, 3], "interleaved": [300, 130], "runs": [1000, 257], "twins": 0}[mix]
    c = KC.make(mix, [D0, D1], [H0, H1], sizes, seed=7)
    fl, hf = KI.query(c.image, c.sets)
    assert fl.all() and hf.all() and len(fl) + len(hf) == c.members
    half = {k: v[::2] for k, v in c.sets.items()}
    img = KC.image(half)
    left = KI.subtract(c.sets, img)
    assert sum(len(v) for v in left.values()) == c.members - sum(len(v) for v in half.values())
    assert all(set(left.get(k, [])) == set(v[1::2]) for k, v in c.sets.items())
    fl, hf = KI.query(img, left)
    assert not fl.any() and not hf.any()
    fl, hf = KI.query(c.image, left)
    assert int(fl.sum()) + int(hf.sum()) == sum(len(v) for v in left.values())
    assert KI.subtract(c.sets, c.image) == {}
