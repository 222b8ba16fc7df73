"""ct_mapreduce_amd.get_entries.parse_each, the CPU twin of ctmr_entries_json_each* (include/ctmr.h):
every body judged on its own.  Against `parse` over the good bodies alone; no GPU."""
import pytest

from ct_mapreduce_amd import get_entries as ge
from tests import get_entries_corpus as gc

N_BODIES, PER = 5, 5
ENTRIES = gc.small_entries(N_BODIES * PER, seed=21)
GOOD = ge.write(ENTRIES, PER)


def bad_bodies():
    """(name, body) of every rejection of the corpus: the entry-level ones applied to the first, the middle and the last
    entry in turn"""
    for k, rej in enumerate(gc.REJECTIONS):
        yield rej["name"], gc.reject_body(rej, ENTRIES[:PER], (0, PER // 2, PER - 1)[k % 3])
    yield from gc.BAD_BODIES


def check(bodies, bad_at):
    """parse_each of `bodies`, of which those at bad_at are outside the grammar, against parse of the others"""
    blob, bounds, first, bad = ge.parse_each(bodies)
    good = [b for r, b in enumerate(bodies) if r not in bad_at]
    blob_w, bounds_w, first_w = ge.parse(good)
    assert blob == blob_w and (bounds == bounds_w).all()
    k = 0
    for r in range(len(bodies)):     # a bad body's slot repeats its successor's value
        assert int(first[r]) == int(first_w[k])
        k += r not in bad_at
    assert int(first[-1]) == int(first_w[-1]) and k == len(good)
    _, rb = ge.join(bodies)
    for r in range(len(bodies)):
        if r in bad_at:
            assert bad[r] is not None and int(rb[r]) <= bad[r] < max(int(rb[r + 1]), int(rb[r]) + 1), (r, bad[r])
            assert first[r + 1] == first[r]
        else:
            assert bad[r] is None


def test_parse_each_is_parse_when_nothing_is_bad():
    for bodies in (GOOD, [], [b'{"entries":[]}'], ge.write(ENTRIES, [0, 12, 0, 13], "indent")):
        blob, bounds, first, bad = ge.parse_each(bodies)
        blob_w, bounds_w, first_w = ge.parse(bodies)
        assert blob == blob_w and (bounds == bounds_w).all() and (first == first_w).all() and bad == [None] * len(bodies)


@pytest.mark.parametrize("name,body", list(bad_bodies()), ids=[n for n, _ in bad_bodies()])
def test_a_bad_body_first_in_the_middle_and_last_of_five(name, body):
    with pytest.raises(ge.GetEntriesError):
        ge.parse([body])
    for r in (0, N_BODIES // 2, N_BODIES - 1):
        bodies = list(GOOD)
        bodies[r] = body
        check(bodies, {r})


def test_several_bad_bodies_and_all_of_them():
    pool = list(bad_bodies())
    for k in range(0, len(pool) - 1, 3):
        bodies = list(GOOD)
        bodies[1], bodies[4] = pool[k][1], pool[k + 1][1]
        check(bodies, {1, 4})
    check([b for _, b in pool[:N_BODIES]], set(range(N_BODIES)))
    check([b"", b"", b""], {0, 1, 2})
    pair, _ = gc.split_string_pair()
    check([GOOD[0]] + pair + [GOOD[1]], {1, 2})     # the first ends inside a string; the second does not close it
