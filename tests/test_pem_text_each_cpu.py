"""pem_text.parse_each (the CPU twin of ctmr_pem_decode_each*) held to its definition — the verdict of a
file is parse_one's of that file alone — over tests/pem_text_corpus.py, and the corpora of tests/pem_each_corpus.py held to
what they claim.  No GPU."""
import pytest

from ct_mapreduce_amd import pem_text as pt
from tests import pem_each_corpus as ec
from tests import pem_text_corpus as pc


def alone(t):
    """parse_one's verdict of the file alone: None, or the offset inside it"""
    try:
        pt.parse_one(t)
        return None
    except pt._Bad as b:
        return max(b.at, 0)


def check(files, bad_files=None):
    ders, first, bad = pt.parse_each(files)
    text, fb = pt.join(files)
    assert len(bad) == len(files) and len(first) == len(files) + 1
    for f, t in enumerate(files):
        a = alone(t)
        assert (bad[f] is None) == (a is None), f
        if a is not None:
            assert bad[f] == int(fb[f]) + a and int(fb[f]) <= bad[f] < max(int(fb[f + 1]), int(fb[f]) + 1)
            assert first[f + 1] == first[f]
    good = [t for f, t in enumerate(files) if bad[f] is None]
    pay, off, gfirst = pt.parse(good)
    assert b"".join(ders) == pay and [len(d) for d in ders] == [int(off[k + 1] - off[k]) for k in range(len(off) - 1)]
    counts = [int(first[f + 1] - first[f]) for f in range(len(files))]
    assert [c for f, c in enumerate(counts) if bad[f] is None] == [int(gfirst[k + 1] - gfirst[k]) for k in range(len(good))]
    if bad_files is not None:
        assert [f for f, b in enumerate(bad) if b is not None] == list(bad_files)
    return ders, first, bad


@pytest.mark.parametrize("name", sorted(pc.REJECTIONS))
def test_every_rejection_in_every_place(name):
    for file_at in pc.PLACES:
        for block_at in pc.PLACES:
            files, f = pc.place(pc.REJECTIONS[name][0], file_at, block_at)
            check(files, [f])


@pytest.mark.parametrize("name", sorted(pc.TRUNCATIONS))
def test_every_truncation_in_every_place(name):
    for file_at in pc.PLACES:
        files, f = pc.place(pc.TRUNCATIONS[name], file_at, "last", truncated=True)
        check(files, [f])


def test_with_no_bad_file_parse_each_is_parse():
    fams = list(pc.regular_files().values()) + list(pc.irregular_files().values()) + [[pc.mixed_file()], [], [b""], [b"", b" \n"]]
    for files in fams:
        ders, first, bad = check(files, [])
        pay, off, pfirst = pt.parse(files)
        assert b"".join(ders) == pay and (first == pfirst).all() and len(ders) == len(off) - 1 and bad == [None] * len(files)


def test_the_constructed_files_are_found_by_the_pass_they_name():
    assert ec.found_by(ec.GOOD_REGULAR) is None and ec.found_by(ec.GOOD_IRREGULAR) is None
    assert pt.layout([ec.GOOD_REGULAR])[0][0] == "regular" and pt.layout([ec.GOOD_IRREGULAR]) == [("irregular",)]
    for which, t in ec.BADS.items():
        assert ec.found_by(t) == which and alone(t) is not None
    assert len(ec.armor_lines(ec.BAD_FILES)) == 1
    lines = ec.armor_lines(ec.BAD_CHECK)
    assert lines == [pt.BEGIN, pt.END] and sum(c in pt.ALPHABET + b"=" for c in ec.BAD_CHECK.split(b"\n", 1)[1].rsplit(b"-----END", 1)[0]) % 4 == 3
    # rejected by mark, yet its armor lines are paired and its blocks, without the byte of no class, all irregular
    t = ec.BAD_MARK_PAIRED_IRREGULAR
    assert ec.found_by(t) == "mark" and ec.armor_lines(t) == [pt.BEGIN, pt.END] * 3
    assert pt.layout([t.replace(b"#", b"")]) == [("irregular",)] * 3


@pytest.mark.parametrize("name", sorted(ec.several_bad()))
def test_several_bad_files(name):
    files, bad = ec.several_bad()[name]
    check(files, bad)
    assert {ec.found_by(files[f]) for f in bad} <= {"mark", "files", "check"} and all(ec.found_by(files[f]) for f in bad)
    if name in ("adjacent", "all bad"):
        assert [ec.found_by(files[f]) for f in bad] == ["mark", "files", "check"]


def test_one_lane_many_files():
    for at in list(range(16)) + [1022, 1023, 1024, 1025, 1026]:
        files, bad = ec.one_lane(at)
        text, fb = pt.join(files)
        assert int(fb[bad[0]]) % 1024 == at % 1024 and len(bad) == 16 and all(files[f] == b"x" for f in bad)
        assert int(fb[bad[-1]]) - int(fb[bad[0]]) == 15 and any(t == b"" for t in files)
        check(files, bad)


def test_the_gather_corpora():
    check(ec.one_block_files(257, (0, 63, 64, 255, 256)), [0, 63, 64, 255, 256])
    files = [ec.GOOD_REGULAR, ec.many_blocks(65, 1, bad=True), ec.GOOD_IRREGULAR]
    _, first, _ = check(files, [1])
    assert first.tolist() == [0, 1, 1, 2] and len(ec.armor_lines(files[1])) == 130
    files = [ec.BAD_MARK, ec.many_blocks(300, 2)]
    _, first, _ = check(files, [0])
    assert first.tolist() == [0, 0, 300]
