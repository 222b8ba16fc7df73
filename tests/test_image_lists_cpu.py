"""Per-issuer lists straight from an image without a GPU (include/ctmr.h ctmr_known_image_lists): the CPU
twin known_image.image_lists against lists built directly from Python dicts — the image's order inside a set, repeats
kept, the host-section members of a key behind its member records, the expiry rules of ctmr_known_lists."""
import struct

import numpy as np
import pytest

from ct_mapreduce_amd import known_image as KI
from tests import known_corpus as KC
from tests.test_known_merge_cpu import with_host_pairs

DIGESTS = [bytes([k]) * 31 + bytes([255 - k]) for k in range(1, 6)]
HOURS = [491000, 491003, 491027]
H = HOURS[0]


def key(hour, ident):
    return KI.PREFIX + KI.exp_date_id(hour) + b"::" + ident


def expect(blocks):
    """[(Issuer.ID, text)] of {(Issuer.ID, first second, date string): [members in order]}: grouped and ordered by hand."""
    out = {}
    for ident, start, date in sorted(blocks):
        out.setdefault(ident, []).extend(blocks[(ident, start, date)])
    return [(i, b"".join(m.hex().encode() + b"\n" for m in out[i])) for i in sorted(out)]


def raw_image(sets):
    """An image of [(hour, digest, [members in the order given])] (repeats allowed), the sets put in key order."""
    sets = sorted(sets, key=lambda s: KI.set_key(s[0], s[1]))
    digests = sorted({d for _, d, _ in sets})
    entries, first, members = [], 0, []
    for h, d, ms in sets:
        entries.append(KI._SET.pack(h, digests.index(d), first, len(ms)))
        first += len(ms)
        members += ms
    meta = KI._HEADER.pack(KI.MAGIC, KI.VERSION, 64, len(digests), 0, len(sets), first, 0, 0, 0) + b"".join(digests) + \
        b"".join(entries)
    meta += b"\0" * (-len(meta) % 64)
    rec = np.zeros(first, KI.MEMBER_DTYPE)
    for i, m in enumerate(members):
        rec["len"][i] = len(m)
        rec["serial"][i, :len(m)] = np.frombuffer(m, np.uint8)
    return meta + rec.tobytes()


@pytest.mark.parametrize("mix", KC.MIXES)
def test_canonical_images_of_every_mix_equal_known_lists(mix):
    c = KC.make(mix, DIGESTS, HOURS, [1, 2, 65, 300], seed=5)
    dev_keys = {k for k, _ in KI.records(c.image)[0]}
    host_keys = {k for k, _ in KI.records(c.image)[1]}
    if mix != "twins":
        assert not dev_keys & host_keys              # no key with both member records and host pairs
        for now in (0, (HOURS[0] + 1) * 3600, (HOURS[1] + 1) * 3600 - 1, (HOURS[2] + 1) * 3600):
            assert KI.image_lists(c.image, now) == KI.known_lists(c.image, now)
        assert KI.image_lists(c.image, (HOURS[2] + 1) * 3600) == []
    else:
        # twins put serials above 40 octets into the host section under their set's key: image_lists keeps them behind
        # the member records, known_lists merges and sorts the two
        assert dev_keys & host_keys
        a, b = KI.image_lists(c.image, 0), KI.known_lists(c.image, 0)
        assert [i for i, _ in a] == [i for i, _ in b]
        assert [sorted(t.split(b"\n")) for _, t in a] == [sorted(t.split(b"\n")) for _, t in b]
    # … and against the dicts themselves
    blocks = {}
    for k, ms in c.sets.items():
        _, date, ident = k.split(b"::")
        short, long_ = [m for m in ms if len(m) <= 40], [m for m in ms if len(m) > 40]
        blocks[(ident, KI.exp_date_span(date)[0], date)] = short + long_
    assert KI.image_lists(c.image, 0) == expect(blocks)


def test_image_order_and_repeats_are_kept():
    rng = np.random.default_rng(3)
    ms = [bytes(rng.integers(0, 256, size=int(L), dtype=np.uint8).tolist()) for L in rng.integers(0, 41, size=50)]
    ms += [ms[3], ms[3], ms[17], b"", b""]
    order = [ms[i] for i in rng.permutation(len(ms))]
    assert order != sorted(order)
    two = [b"\x09", b"\x01", b"\x09"]
    img = raw_image([(H, DIGESTS[0], order), (H + 1, DIGESTS[0], two), (H, DIGESTS[1], two[::-1])])
    i0, i1 = KI.issuer_id(DIGESTS[0]), KI.issuer_id(DIGESTS[1])
    want = expect({(i0, H * 3600, KI.exp_date_id(H)): order, (i0, (H + 1) * 3600, KI.exp_date_id(H + 1)): two,
                   (i1, H * 3600, KI.exp_date_id(H)): two[::-1]})
    assert KI.image_lists(img, 0) == want
    assert dict(want)[i0].count(ms[3].hex().encode() + b"\n") >= 3
    # known_lists sorts and drops the repeats: not the same text
    assert KI.known_lists(img, 0) != want
    assert KI.image_lists(KI.sort(img), 0) == expect({(i0, H * 3600, b"a"): sorted(order), (i0, (H + 1) * 3600, b"b"): sorted(two),
                                                      (i1, H * 3600, b"a"): sorted(two)})


def test_expiry_edges_days_and_years():
    i0 = KI.issuer_id(DIGESTS[0])
    day = KI.exp_date_id(H)[:10]
    day_start = (H // 24) * 86400
    lo, hi = KI._HOUR_LO, KI._HOUR_HI
    assert KI.exp_date_id(lo) == b"0000-01-01-00" and KI.exp_date_id(hi - 1) == b"9999-12-31-23"
    sets = {key(H, i0): [b"\x01"], key(H + 1, i0): [b"\x02"]}
    pairs = [(KI.PREFIX + day + b"::odd", b"\xaa"), (KI.PREFIX + b"2026-02-30-01::odd", b"\xbb"),
             (KI.PREFIX + b"10000-01-01-00::odd", b"\xcc"), (KI.PREFIX + b"2026-13-01::odd", b"\xdd")]
    img = with_host_pairs(sets, pairs)
    end = (H + 1) * 3600
    assert KI.image_lists(img, end - 1) == [(i0, b"01\n02\n"), (b"odd", b"aa\n")]
    assert KI.image_lists(img, end) == [(i0, b"02\n"), (b"odd", b"aa\n")]
    assert KI.image_lists(img, day_start + 86399)[-1] == (b"odd", b"aa\n")
    assert b"odd" not in dict(KI.image_lists(img, day_start + 86400))
    assert KI.image_lists(img, end + 3600) == ([(b"odd", b"aa\n")] if end + 3600 < day_start + 86400 else [])
    # set records of hours outside the years 0000..9999 are never listed; the first and last hour inside are
    far = raw_image([(lo - 1, DIGESTS[0], [b"\x01"]), (lo, DIGESTS[0], [b"\x02"]), (hi - 1, DIGESTS[0], [b"\x03"]),
                     (hi, DIGESTS[0], [b"\x04"]), (2 ** 31 - 1, DIGESTS[0], [b"\x05"]), (-2 ** 31, DIGESTS[0], [b"\x06"])])
    assert KI.image_lists(far, lo * 3600 - 10 ** 9) == [(i0, b"02\n03\n")]
    assert KI.image_lists(far, (lo + 1) * 3600) == [(i0, b"03\n")]
    assert KI.image_lists(far, hi * 3600) == []


def test_keys_of_two_and_four_parts_raise():
    sets = {key(H, KI.issuer_id(DIGESTS[0])): [b"\x01"]}
    for bad in (b"serials::x", KI.PREFIX + KI.exp_date_id(H) + b"::a::b"):
        with pytest.raises(KI.ListsError):
            KI.image_lists(with_host_pairs(sets, [(bad, b"\x01")]), 0)
    assert KI.image_lists(with_host_pairs(sets, [(KI.PREFIX + KI.exp_date_id(H) + b"::a", b"\x01")]), 0)[-1] == (b"a", b"01\n")


def test_host_pairs_of_a_set_s_own_key_come_behind_its_records():
    i0 = KI.issuer_id(DIGESTS[0])
    k = key(H, i0)
    sets = {k: [b"\x05", b"\x07" * 40], key(H + 2, i0): [b"\x06"]}
    pairs = [(k, b"\x00"), (k, b"\x08" * 41), (key(H + 1, i0), b"\x01")]
    got = KI.image_lists(with_host_pairs(sets, pairs), 0)
    assert got == [(i0, b"05\n" + b"07" * 40 + b"\n" + b"00\n" + b"08" * 41 + b"\n" + b"01\n" + b"06\n")]


def test_two_spellings_of_one_hour_are_ordered_by_string():
    base = KI.exp_date_id(H)[:11]
    hh = 5
    h5 = (H // 24) * 24 + hh
    assert KI.exp_date_id(h5) == base + b"05"
    i0 = KI.issuer_id(DIGESTS[0])
    sets = {key(h5, i0): [b"\x02"]}
    img = with_host_pairs(sets, [(KI.PREFIX + base + b"5::" + i0, b"\x01"), (KI.PREFIX + base + b"05::" + i0, b"\x03")])
    # "…-05" < "…-5" as strings: the set record's block (with the host pair of its own spelling), then the other spelling
    assert KI.image_lists(img, 0) == [(i0, b"02\n03\n01\n")]
    assert KI.image_lists(img, (h5 + 1) * 3600) == []


def test_a_damaged_image_is_refused():
    img = bytearray(raw_image([(H, DIGESTS[0], [b"\x01"])]))
    struct.pack_into("<Q", img, len(img) - 48, 41)
    with pytest.raises(KI.ImageError):
        KI.image_lists(bytes(img), 0)
