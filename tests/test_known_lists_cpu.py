"""Per-issuer known-serial lists without a GPU (include/ctmr.h ctmr_known_lists): the CPU twin
known_image.known_lists on hand-built images, and the host writer's StoreKnownCertificateList against the Python mirror of
the reference's LocalDiskBackend."""
import os

import numpy as np
import pytest

from ct_mapreduce_amd import known_image as KI
from ct_mapreduce_amd import host_writeback as HW
from tests import storage_mirror as SM

D1, D2 = bytes(range(32)), bytes(range(1, 33))
ID1, ID2 = KI.issuer_id(D1), KI.issuer_id(D2)
H = 491000                                      # an exp hour (2026)


def key(hour, ident):
    return KI.PREFIX + KI.exp_date_id(hour) + b"::" + ident


def lines(text):
    return text.split(b"\n")[:-1]


def test_expiry_boundary_is_the_end_of_the_hour():
    img = KI.build({key(H, ID1): [b"\x01"], key(H + 1, ID1): [b"\x02"]})
    end = (H + 1) * 3600
    assert KI.known_lists(img, end - 1) == [(ID1, b"01\n02\n")]
    assert KI.known_lists(img, end) == [(ID1, b"02\n")]
    assert KI.known_lists(img, end + 3600) == []


def test_day_resolution_unparsable_and_malformed_keys():
    day = KI.exp_date_id(H)[:10]                # "YYYY-MM-DD": lastGood = day + 24 h - 1 ms
    day_start = (H // 24) * 86400
    sets = {KI.PREFIX + day + b"::odd": [b"\xaa"], KI.PREFIX + b"2026-02-30-01::odd": [b"\xbb"],
            KI.PREFIX + b"10000-01-01-00::odd": [b"\xcc"], KI.PREFIX + b"2026-13-01::odd": [b"\xdd"]}
    assert KI.lists_of_sets(sets, day_start + 86399) == [(b"odd", b"aa\n")]
    assert KI.lists_of_sets(sets, day_start + 86400) == []
    with pytest.raises(KI.ListsError):
        KI.lists_of_sets({KI.PREFIX + KI.exp_date_id(H) + b"::a::b": [b"\x01"]}, 0)
    with pytest.raises(KI.ListsError):
        KI.lists_of_sets({b"serials::x": [b"\x01"]}, 0)
    # one-digit hours parse as time.Parse takes them
    assert KI.exp_date_span(b"2026-01-02-5") == KI.exp_date_span(b"2026-01-02-05")


def test_blocks_order_duplicates_and_hex():
    s41 = bytes([0x00, 0xAB]) + b"\x7f" * 39
    sets = {key(H + 5, ID1): [b"\x00\x01", b"\xff"], key(H, ID1): [b"\x00\x01", b"", s41],
            key(H, ID2): [b"\x10"]}
    img = KI.build(sets)
    out = KI.known_lists(img, 0)
    assert [i for i, _ in out] == sorted([ID1, ID2])
    got = dict(out)
    # two expDates of one issuer: two blocks, ascending; a serial under both appears twice; empty → "\n"; 41 octets kept
    blocks = KI.list_blocks(KI.parse(img).sets, 0)
    assert [d for d, _ in dict(blocks)[ID1]] == [KI.exp_date_id(H), KI.exp_date_id(H + 5)]
    first = sorted(lines(got[ID1])[:3])
    assert first == sorted([b"", b"0001", s41.hex().encode()])
    assert sorted(lines(got[ID1])[3:]) == [b"0001", b"ff"]
    assert lines(got[ID1]).count(b"0001") == 2
    assert got[ID2] == b"10\n"
    assert all(l == l.lower() for l in lines(got[ID1]))


def test_issuer_ids_order_bytewise_and_merge():
    a, b = b"Zz", b"aa"
    sets = {key(H, b): [b"\x01"], key(H, a): [b"\x02"], key(H + 1, a): [b"\x03"]}
    assert [i for i, _ in KI.lists_of_sets(sets, 0)] == [a, b]
    r0 = KI.lists_of_sets({key(H, a): [b"\x01"]}, 0)
    r1 = KI.lists_of_sets({key(H, a): [b"\x02"], key(H, b): [b"\x03"]}, 0)
    assert KI.merge_lists([r0, r1]) == [(a, b"01\n02\n"), (b, b"03\n")]


def _mirror_files(root, lists):
    be = SM.LocalDiskBackend(0o644, root)
    for ident, text in lists:
        be.StoreKnownCertificateList(SM.Issuer.FromString(ident.decode()), [SM.Serial(bytes.fromhex(l.decode())) for l in lines(text)])


def _read_tree(root):
    out = {}
    for name in sorted(os.listdir(root)):
        with open(os.path.join(root, name), "rb") as f:
            out[name] = f.read()
    return out


def test_host_writer_matches_the_mirror(tmp_path):
    sets = {key(H, ID1): [b"\x00\x01", b"\xfe" * 20, b""], key(H + 2, ID1): [b"\x00\x01"], key(H, ID2): [b"\x42" * 45]}
    lists = KI.known_lists(KI.build(sets), 0)
    mine, theirs = tmp_path / "a" / "deeper", tmp_path / "b"
    w = HW.HostWriter(str(mine), [])
    w.store_lists(lists)
    w.close()
    os.makedirs(theirs)
    _mirror_files(str(theirs), lists)
    assert _read_tree(str(mine)) == _read_tree(str(theirs))
    assert set(_read_tree(str(mine))) == {ID1.decode(), ID2.decode()}
    for name in os.listdir(mine):
        assert (os.stat(mine / name).st_mode & 0o777) == 0o644 & ~_umask()


def _umask():
    m = os.umask(0)
    os.umask(m)
    return m


def test_host_writer_truncates_refuses_and_noop(tmp_path):
    root = tmp_path / "r"
    os.makedirs(root)
    (root / "ID").write_bytes(b"x" * 1000)
    w = HW.HostWriter(str(root), [])
    w.store_lists([(b"ID", b"01\n")])
    assert (root / "ID").read_bytes() == b"01\n"
    for bad in (b"../x", b"a/b", b"..", b".", b"", b"a\0b"):
        with pytest.raises(RuntimeError):
            w.store_lists([(b"fine", b"02\n"), (bad, b"01\n")])
        assert not (root / "fine").exists()      # nothing is written when one ID is refused
    assert not (tmp_path / "x").exists()
    w.close()
    noop = HW.HostWriter(None, [])
    before = sorted(os.listdir(tmp_path))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        noop.store_lists([(b"ID2", b"01\n")])
    finally:
        os.chdir(cwd)
    assert sorted(os.listdir(tmp_path)) == before
    noop.close()


def test_twin_lists_equal_the_mirror_serial_encoding():
    s = [b"", b"\x00", b"\x00\x00\xff", bytes(range(41))]
    text = KI.lists_of_sets({key(H, ID1): s}, 0)[0][1]
    assert text == b"".join((SM.Serial(m).HexString() + "\n").encode() for m in s)
    assert np.array_equal(np.frombuffer(text, np.uint8)[-1:], np.frombuffer(b"\n", np.uint8))
