"""Set algebra on known-certificate images without a GPU (known_image.union / minus / intersect; include/ctmr.h
ctmr_known_merge*): the twins against plain Python set algebra on dicts, the laws as exact bytes, and
where host-section pairs and vanishing issuers end up.  tests/test_gpu_known_merge.py holds the library to these twins."""
import hashlib
import struct

import pytest

from ct_mapreduce_amd import known_image as KI
from tests import known_corpus as KC

DIGESTS = sorted(hashlib.sha256(b"merge issuer %d" % k).digest() for k in range(5))
HOURS = [490999, 491000, 491016]
EMPTY = KI.build({})


def pair_of_dicts(mix, seed=3):
    """Two {key: members} dicts from one corpus: keys in one alone, identical, disjoint, nested and interleaved sets."""
    c = KC.make(mix, DIGESTS, HOURS, [40, 1, 17, 64, 9, 130, 2], seed=seed)
    a, b = {}, {}
    for k, (key, ms) in enumerate(sorted(c.sets.items())):
        case = k % 7
        ms = list(ms)
        if case == 0:
            a[key] = ms
        elif case == 1:
            b[key] = ms
        elif case == 2:
            a[key], b[key] = ms, list(ms)
        elif case == 3:
            a[key], b[key] = ms[:len(ms) // 2], ms[len(ms) // 2:]
        elif case == 4:
            a[key], b[key] = ms[::3], ms
        elif case == 5:
            a[key], b[key] = ms, ms[1::2]
        else:
            a[key], b[key] = ms[::2] + ms[1::4], ms[1::2] + ms[::4]
    return {k: v for k, v in a.items() if v}, {k: v for k, v in b.items() if v}


def algebra(op, a, b):
    keys = set(a) | set(b)
    f = {"union": lambda x, y: x | y, "minus": lambda x, y: x - y, "intersect": lambda x, y: x & y}[op]
    out = {k: f(set(a.get(k, ())), set(b.get(k, ()))) for k in keys}
    return {k: sorted(v) for k, v in out.items() if v}


@pytest.mark.parametrize("mix", KC.MIXES)
def test_twins_against_python_sets(mix):
    a, b = pair_of_dicts(mix)
    ia, ib = KC.image(a), KC.image(b)
    assert ia == KI.build(a) and ib == KI.build(b)
    for op, fn in (("union", KI.union), ("minus", KI.minus), ("intersect", KI.intersect)):
        want = algebra(op, a, b)
        got = fn(ia, ib)
        assert got == KI.build(want) == KC.image(want)
        assert KI.parse(got).sets == want
    assert KI.merge(KI.KNOWN_UNION, ia, ib) == KI.union(ia, ib)
    assert KI.merge(KI.KNOWN_MINUS, ia, ib) == KI.minus(ia, ib)
    assert KI.merge(KI.KNOWN_INTERSECT, ia, ib) == KI.intersect(ia, ib)
    assert KI.merge(KI.KNOWN_UNION, ia) == KI.union(ia) == ia
    assert (KI.KNOWN_UNION, KI.KNOWN_MINUS, KI.KNOWN_INTERSECT) == (0, 1, 2)
    with pytest.raises(ValueError):
        KI.merge(3, ia, ib)


@pytest.mark.parametrize("mix", KC.MIXES)
def test_laws_as_exact_bytes(mix):
    a, b = pair_of_dicts(mix, seed=5)
    ia, ib = KC.image(a), KC.image(b)
    assert KI.union(ia, ia) == KI.union(ia)
    assert KI.union(ia, ib) == KI.union(ib, ia)
    assert KI.minus(ia, ia) == EMPTY and len(EMPTY) == 64
    assert KI.intersect(ia, ib) == KI.minus(ia, KI.minus(ia, ib))
    new = KI.union(ia, ib)                                                    # old ⊆ new
    assert KI.union(ia, KI.minus(new, ia)) == KI.union(new) == new
    assert KI.union(ia, None) == ia and KI.minus(ia, None) == ia and KI.intersect(ia, None) == EMPTY
    assert KI.union(ia, ib, ia, None) == new


def with_host_pairs(sets, pairs):
    """The canonical image of `sets` with `pairs` added to its HOST section, whatever they are — as an exporter that had
    not registered the issuer writes them."""
    img = KI.build(sets)
    meta, rec = KC.split(img)
    _, _, _, n_iss, _, n_sets, n_mem, host_bytes, n_host, _ = KI._HEADER.unpack_from(meta, 0)
    end = 64 + 32 * n_iss + 24 * n_sets + host_bytes
    old = KI.records(img)[1]
    host = sorted(set(old) | set(pairs))
    part = b"".join(struct.pack("<I", len(k)) + k + struct.pack("<I", len(m)) + m for k, m in host)
    body = meta[64:end - host_bytes] + part
    head = KI._HEADER.pack(KI.MAGIC, KI.VERSION, 64, n_iss, 0, n_sets, n_mem, len(part), len(host), 0)
    m2 = head + body
    m2 += b"\0" * (-len(m2) % 64)
    return m2 + rec.tobytes()


def test_host_section_pairs_that_belong_in_the_member_section():
    key = KI.set_key(HOURS[1], DIGESTS[2])
    other = KI.set_key(HOURS[0], DIGESTS[4])                                  # a set and an issuer of the pair's own
    odd = b"serials::2026-01-05::" + KI.issuer_id(DIGESTS[2])                 # a day-resolution key: does not parse
    assert KI.parse_key(key) and KI.parse_key(other) and KI.parse_key(odd) is None
    sets = {key: [b"\x01\x02", b"\x05" * 20]}
    pairs = [(key, b"\x03" * 40), (key, b"\x04" * 41), (other, b""), (odd, b"\x07\x08")]
    img = with_host_pairs(sets, pairs)
    im = KI.parse(img)
    assert im.n_host_members == 4 and im.n_members == 2
    norm = KI.union(img)
    dev, host = KI.records(norm)
    assert dev == [(other, b""), (key, b"\x01\x02"), (key, b"\x03" * 40), (key, b"\x05" * 20)]
    assert host == sorted([(odd, b"\x07\x08"), (key, b"\x04" * 41)])           # 41 octets; a key that does not parse
    assert KI.parse(norm).issuers == sorted([DIGESTS[2], DIGESTS[4]])
    # the moved pair meets the other operand's member record as one
    b = KI.build({key: [b"\x03" * 40]})
    assert KI.records(KI.union(img, b))[0].count((key, b"\x03" * 40)) == 1
    assert (key, b"\x03" * 40) not in KI.records(KI.minus(img, b))[0]
    assert KI.records(KI.intersect(img, b)) == ([(key, b"\x03" * 40)], [])


def test_an_issuer_whose_sets_all_vanish_leaves_the_issuer_list():
    d = DIGESTS
    a = {KI.set_key(HOURS[0], d[0]): [b"\x01"], KI.set_key(HOURS[0], d[1]): [b"\x02", b"\x03"],
         KI.set_key(HOURS[1], d[1]): [b"\x04"], KI.set_key(HOURS[0], d[3]): [b"\x05"]}
    b = {KI.set_key(HOURS[0], d[1]): [b"\x03", b"\x02"], KI.set_key(HOURS[1], d[1]): [b"\x04", b"\x09"]}
    ia, ib = KI.build(a), KI.build(b)
    assert KI.parse(ia).issuers == [d[0], d[1], d[3]]
    out = KI.minus(ia, ib)
    im = KI.parse(out)
    assert im.issuers == [d[0], d[3]] and im.n_sets == 2
    ordinals = [KI._SET.unpack_from(out, 64 + 64 + 24 * s)[1] for s in range(2)]
    assert sorted(ordinals) == [0, 1]                                         # d[3] moved down from 2 to 1
    assert im.sets == {KI.set_key(HOURS[0], d[0]): [b"\x01"], KI.set_key(HOURS[0], d[3]): [b"\x05"]}
