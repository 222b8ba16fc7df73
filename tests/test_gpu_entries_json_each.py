"""-m gpu: ctmr_entries_json_each* (include/ctmr.h) — every get-entries body judged on its own, both
variants through the C ABI against the CPU twin (get_entries.parse_each).  The harness is that of
tests/test_gpu_entries_json.py: exact-size buffers between 0xEE guards, the device text at a chosen byte phase between
bytes that would parse as more entries; resp_bad is guarded too.  A failing call must leave every buffer as it was."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import get_entries as ge, _native as N  # noqa: E402
from tests import get_entries_corpus as gc  # noqa: E402
from tests.test_gpu_entries_json import framed, call as call_strict, PAD, NONE, GUARD64  # noqa: E402

N_BODIES, PER = 5, 5
ENTRIES = gc.small_entries(N_BODIES * PER, seed=21)
GOOD = ge.write(ENTRIES, PER)


@pytest.fixture(scope="module")
def eng():
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
    yield e
    e.close()


def bad_bodies():
    """(name, body) of every rejection of the corpus: the entry-level ones applied to the first, the middle and the last
    entry in turn"""
    out = [(rej["name"], gc.reject_body(rej, ENTRIES[:PER], (0, PER // 2, PER - 1)[k % 3])) for k, rej in enumerate(gc.REJECTIONS)]
    return out + list(gc.BAD_BODIES)


def call(eng, variant, buf, rb, blob_cap, entries_cap, with_bad=True):
    """One call between guards → (rc, info, blob with 16 guard bytes on both sides; bounds, resp_first and resp_bad with
    one guard word on both sides)."""
    R = len(rb) - 1
    info = N.EntriesJsonInfo()
    first = np.full(R + 3, GUARD64, np.uint64)
    bad = np.full(R + 2, GUARD64, np.uint64)
    p_bad = bad[1:].ctypes.data if with_bad else None
    lib, h = eng._lib, eng._h
    if variant == "device":
        d_text = torch.from_numpy(buf).to("cuda:0")
        d_blob = torch.full((blob_cap + 32,), 0xEE, dtype=torch.uint8, device="cuda:0")
        d_bounds = torch.full((2 * entries_cap + 3,), GUARD64 - 2**64, dtype=torch.int64, device="cuda:0")
        assert d_text.data_ptr() % 16 == 0 and d_blob.data_ptr() % 16 == 0
        rc = lib.ctmr_entries_json_each_device(h, C.c_void_p(d_text.data_ptr()), rb.ctypes.data, R, C.c_void_p(d_blob.data_ptr() + 16), blob_cap,
                                               C.c_void_p(d_bounds.data_ptr() + 8), entries_cap, first[1:].ctypes.data, p_bad, C.byref(info))
        torch.cuda.synchronize()
        return rc, info, d_blob.cpu().numpy(), d_bounds.cpu().numpy().view(np.uint64), first, bad
    blob = np.full(blob_cap + 32, 0xEE, np.uint8)
    bounds = np.full(2 * entries_cap + 3, GUARD64, np.uint64)
    rc = lib.ctmr_entries_json_each(h, buf.ctypes.data, rb.ctypes.data, R, blob[16:].ctypes.data, blob_cap, bounds[1:].ctypes.data, entries_cap,
                                    first[1:].ctypes.data, p_bad, C.byref(info))
    return rc, info, blob, bounds, first, bad


def untouched(blob, bounds, first, bad):
    return (blob == 0xEE).all() and (bounds == GUARD64).all() and (first == GUARD64).all() and (bad == GUARD64).all()


def check(eng, bodies, phase=0, want_bad=None):
    """both variants give the twin's result at buffers sized exactly for the good bodies; want_bad: the bad bodies"""
    blob_w, bounds_w, first_w, bad_w = ge.parse_each(bodies)
    if want_bad is not None:
        assert {r for r, b in enumerate(bad_w) if b is not None} == set(want_bad)
    R, n, bb = len(bodies), (len(bounds_w) - 1) // 2, len(blob_w)
    buf, rb = framed(bodies, phase)
    lowest = next((r for r in range(R) if bad_w[r] is not None), None)
    for variant in ("device", "host"):
        rc, info, blob, bounds, first, bad = call(eng, variant, buf, rb, bb + PAD, n)
        assert rc == 0, (variant, rc, eng._lib.ctmr_last_error(eng._h))
        assert (info.responses, info.entries, info.blob_bytes, info.text_bytes) == (R, n, bb, int(rb[-1] - rb[0]) if R else 0), variant
        assert (blob[:16] == 0xEE).all() and (blob[16 + bb + PAD:] == 0xEE).all() and (blob[16 + bb:16 + bb + PAD] == 0).all(), variant
        got = blob[16:16 + bb].tobytes()
        if got != blob_w:
            k = next(i for i in range(bb) if got[i] != blob_w[i])
            raise AssertionError("%s: blob differs at byte %d of %d" % (variant, k, bb))
        assert bounds[0] == GUARD64 and bounds[-1] == GUARD64 and (bounds[1:-1] == bounds_w).all(), variant
        assert first[0] == GUARD64 and first[-1] == GUARD64 and (first[1:-1] == first_w).all(), (variant, first[1:-1], first_w)
        assert bad[0] == GUARD64 and bad[-1] == GUARD64, variant
        for r in range(R):
            if bad_w[r] is None:
                assert bad[1 + r] == NONE, (variant, r, int(bad[1 + r]))
            else:
                assert int(rb[r]) <= int(bad[1 + r]) < max(int(rb[r + 1]), int(rb[r]) + 1), (variant, r, int(bad[1 + r]), int(rb[r]), int(rb[r + 1]))
        if lowest is None:
            assert info.bad_response == NONE and info.bad_offset == NONE, variant
        else:
            assert info.bad_response == lowest and info.bad_offset == bad[1 + lowest], variant


# ---------------------------------------------------------------------------------------------- the corpus' rejections
@pytest.mark.parametrize("k", range(len(bad_bodies())), ids=[n for n, _ in bad_bodies()])
def test_a_bad_body_first_middle_last_two_at_once_and_all_five(eng, k):
    pool = bad_bodies()
    body, other = pool[k][1], pool[(k + 7) % len(pool)][1]
    for r in (0, N_BODIES // 2, N_BODIES - 1):
        bodies = list(GOOD)
        bodies[r] = body
        check(eng, bodies, phase=(3 * k + r) % 16, want_bad=[r])
    bodies = list(GOOD)
    bodies[1], bodies[3] = body, other
    check(eng, bodies, phase=(5 * k + 1) % 16, want_bad=[1, 3])
    check(eng, [pool[(k + j) % len(pool)][1] for j in range(N_BODIES)], phase=k % 16, want_bad=range(N_BODIES))


# ---------------------------------------------------------------------------------------------- the wave case
def test_two_bad_bodies_of_one_mark_block_and_one_check_wave(eng):
    """Three bodies inside one mark block (one wave of k_ej_mark), the first and the third bad, the second good: a report
    reduced over the wave to its lowest response never hears of the third, whose entry would then be decoded.  First by a
    violation k_ej_mark finds, a stray byte outside a string; then by one k_ej_check finds, a key in another case, with
    the 60 tokens of the three bodies in the first 64-lane wave of the check."""
    e = gc.small_entries(3, seed=31, lo=6, hi=12)
    one = [ge.write_one([x]) for x in e]
    stray = [one[0] + b"x", one[1], one[2][:-2] + b"x]}"]
    key = [one[0].replace(b"leaf_input", b"leaf_inpuT"), one[1], one[2].replace(b"extra_data", b"Extra_data")]
    for bodies in (stray, key):
        assert sum(len(b) for b in bodies) + 15 <= gc.MARK_BLOCK
        assert sum(sum(b.count(c) for c in b'{}[]:,"') for b in key) <= 64
        for phase in (0, 9):
            check(eng, bodies, phase=phase, want_bad=[0, 2])
    check(eng, [stray[0], key[2], one[1], key[0], stray[2]], phase=4, want_bad=[0, 1, 3, 4])
    # bodies of a byte or two: several responses inside one lane's 16 bytes, each with a stray byte of its own
    check(eng, [b"x", b"y", one[1], b"zz", b"[]", b"\\"], phase=2, want_bad=[0, 1, 3, 4, 5])


def test_a_body_that_ends_inside_a_string_and_one_that_would_close_it(eng):
    pair, _ = gc.split_string_pair()
    check(eng, pair, phase=6, want_bad=[0, 1])
    check(eng, [GOOD[0]] + pair + [GOOD[1]], phase=1, want_bad=[1, 2])
    check(eng, [GOOD[0], GOOD[1]] + pair, phase=12, want_bad=[2, 3])
    check(eng, [pair[0], GOOD[2]], phase=3, want_bad=[0])    # the good body's string state starts afresh


@pytest.mark.parametrize("phase", range(16))
def test_a_bad_body_between_two_good_ones_at_all_text_phases(eng, phase):
    pool = bad_bodies()
    check(eng, [GOOD[0], pool[(5 * phase) % len(pool)][1], GOOD[1]], phase=phase, want_bad=[1])


# ---------------------------------------------------------------------------------------------- degenerate inputs
def test_no_body_one_bad_body_and_empty_bodies(eng):
    check(eng, [], phase=3, want_bad=[])
    check(eng, [b"{}"], phase=5, want_bad=[0])
    check(eng, [b""], phase=7, want_bad=[0])
    check(eng, [b"", b"", b""], phase=8, want_bad=[0, 1, 2])
    check(eng, [b""] + GOOD[:2], phase=9, want_bad=[0])
    check(eng, [GOOD[0], b"", GOOD[1]], phase=10, want_bad=[1])
    check(eng, [GOOD[0], b"", b"", GOOD[1]], phase=10, want_bad=[1, 2])
    check(eng, GOOD[:2] + [b""], phase=11, want_bad=[2])


# ---------------------------------------------------------------------------------------------- no bad body
def test_without_a_bad_body_every_output_is_that_of_the_strict_call(eng):
    entries = gc.small_entries(40, seed=6, lo=0, hi=300)
    entries[11] = (gc.content("random", 3 * gc.TILE_OUT + 5), gc.content("ramp1", 2 * gc.TILE_OUT))    # a string of 4 decode tiles
    for bodies, phase in ((ge.write(entries, 7, "alternate"), 13), (ge.write(entries, [0, 40, 0], "indent"), 2), ([], 0)):
        check(eng, bodies, phase=phase, want_bad=[])
        blob_w, bounds_w, _ = ge.parse(bodies)
        n, bb = (len(bounds_w) - 1) // 2, len(blob_w)
        buf, rb = framed(bodies, phase)
        for variant in ("device", "host"):
            a = call(eng, variant, buf, rb, bb + PAD, n)
            s = call_strict(eng, variant, buf, rb, bb + PAD, n)
            assert a[0] == s[0] == 0
            assert bytes(a[1]) == bytes(s[1])                      # info
            for x, y in zip(a[2:5], s[2:5]):                       # blob, bounds, resp_first: guards included
                assert (x == y).all(), variant
            assert (a[5][1:-1] == NONE).all()


# ---------------------------------------------------------------------------------------------- sizing, arguments
def test_buffers_one_short_of_the_good_bodies_need_give_range_and_nothing_written(eng):
    bodies = list(ge.write(gc.small_entries(50, seed=12), 7))
    bodies[2] = bodies[2].replace(b"leaf_input", b"leaf_inpuT", 1)
    bodies[5] = bodies[5] + b"x"
    blob_w, bounds_w, _, bad_w = ge.parse_each(bodies)
    n, bb = (len(bounds_w) - 1) // 2, len(blob_w)
    assert n == 50 - 14 and [r for r, b in enumerate(bad_w) if b is not None] == [2, 5]
    buf, rb = framed(bodies, 2)
    for variant in ("device", "host"):
        for blob_cap, entries_cap in ((bb + PAD - 1, n), (bb + PAD, n - 1), (0, 0)):
            rc, info, blob, bounds, first, bad = call(eng, variant, buf, rb, blob_cap, entries_cap)
            assert rc == N.E_RANGE, (variant, blob_cap, entries_cap, rc)
            assert (info.responses, info.entries, info.blob_bytes, info.text_bytes, info.bad_response) == (len(bodies), n, bb, int(rb[-1] - rb[0]), 2)
            assert untouched(blob, bounds, first, bad)
        assert call(eng, variant, buf, rb, bb + PAD, n)[0] == 0     # sized by the good bodies, not by all of them


def test_a_null_resp_bad_is_an_argument_error_and_nothing_is_written(eng):
    bodies = list(GOOD)
    blob_w, bounds_w, _ = ge.parse(bodies)
    buf, rb = framed(bodies, 3)
    for variant in ("device", "host"):
        rc, info, blob, bounds, first, bad = call(eng, variant, buf, rb, len(blob_w) + PAD, len(ENTRIES), with_bad=False)
        assert rc == N.E_INVAL and info.bad_response == NONE and info.bad_offset == NONE
        assert untouched(blob, bounds, first, bad)


# ---------------------------------------------------------------------------------------------- Python
def test_python_methods(eng):
    bodies = list(GOOD)
    bodies[3] = b"{}"
    blob_w, bounds_w, first_w, bad_w = ge.parse_each(bodies)
    raw = eng.entries_json_each(bodies)
    assert raw.blob.tobytes() == blob_w + bytes(PAD) and (raw.bounds == bounds_w).all() and (raw.resp_first == first_w).all()
    assert [b is None for b in raw.bad] == [b is None for b in bad_w] and raw.n == 20
    text, rb = ge.join(bodies)
    d_text = torch.from_numpy(np.frombuffer(b"x" + text, np.uint8).copy()).to("cuda:0")
    d_blob, d_bounds, first, bad, info = eng.entries_json_each_device(d_text, rb + np.uint64(1))
    assert d_blob.cpu().numpy().tobytes() == blob_w + bytes(PAD) and (d_bounds.cpu().numpy().view(np.uint64) == bounds_w).all()
    assert (first == first_w).all() and [b is None for b in bad] == [b is None for b in bad_w] and info.bad_response == 3
