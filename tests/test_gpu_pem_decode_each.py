"""-m gpu: ctmr_pem_decode_each* (include/ctmr.h) — every PEM file judged on its own — both variants through
the C ABI against the CPU twin (pem_text.parse_each) and, bit for bit, against ctmr_pem_decode_device over the good files
alone.  Every call runs at exact-size buffers between 0xEE guards with the device text at a chosen byte phase between bytes
that would parse as one more block, as in tests/test_gpu_pem_decode.py; a failing call must leave every buffer as it was."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import pem_text as pt, _native as N  # noqa: E402
from tests import pem_each_corpus as ec, pem_text_corpus as pc  # noqa: E402
from tests.test_gpu_pem_decode import GUARD64, NONE, PAD, call as strict_call, framed, untouched  # noqa: E402


@pytest.fixture(scope="module")
def eng():
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
    yield e
    e.close()


def call(eng, variant, buf, fb, payload_cap, certs_cap, with_bad=True):
    """One call between guards → (rc, info, payload with 16 guard bytes on both sides, offsets, file_first and file_bad
    with one guard word on both sides)."""
    F = len(fb) - 1
    info = N.PemDecodeInfo()
    first = np.full(F + 3, GUARD64, np.uint64)
    bad = np.full(F + 2, GUARD64, np.uint64)
    bad_p = bad[1:].ctypes.data if with_bad else None
    lib, h = eng._lib, eng._h
    if variant == "device":
        d_text = torch.from_numpy(buf).to("cuda:0")
        d_pay = torch.full((payload_cap + 32,), 0xEE, dtype=torch.uint8, device="cuda:0")
        d_off = torch.full((certs_cap + 3,), GUARD64 - 2**64, dtype=torch.int64, device="cuda:0")
        assert d_text.data_ptr() % 16 == 0 and d_pay.data_ptr() % 16 == 0
        torch.cuda.synchronize()        # the engine runs on a stream of its own: the guards are written before it starts
        rc = lib.ctmr_pem_decode_each_device(h, C.c_void_p(d_text.data_ptr()), fb.ctypes.data, F, C.c_void_p(d_pay.data_ptr() + 16), payload_cap,
                                             C.c_void_p(d_off.data_ptr() + 8), certs_cap, first[1:].ctypes.data, bad_p, C.byref(info))
        torch.cuda.synchronize()
        return rc, info, d_pay.cpu().numpy(), d_off.cpu().numpy().view(np.uint64), first, bad
    pay = np.full(payload_cap + 32, 0xEE, np.uint8)
    off = np.full(certs_cap + 3, GUARD64, np.uint64)
    rc = lib.ctmr_pem_decode_each(h, buf.ctypes.data, fb.ctypes.data, F, pay[16:].ctypes.data, payload_cap, off[1:].ctypes.data, certs_cap,
                                  first[1:].ctypes.data, bad_p, C.byref(info))
    return rc, info, pay, off, first, bad


def strict_over(eng, files, phase):
    """ctmr_pem_decode_device over `files` (all good) → (payload with pad, offsets, file_first, regular, irregular)"""
    pay_w, off_w, _ = pt.parse(files)
    n, pb = len(off_w) - 1, len(pay_w)
    buf, fb = framed(files, phase)
    rc, info, pay, off, first = strict_call(eng, "device", buf, fb, pb + PAD, n)
    assert rc == 0 and (info.certificates, info.payload_bytes) == (n, pb)
    return pay[16:16 + pb + PAD].copy(), off[1:-1].copy(), first[1:-1].copy(), info.regular, info.irregular


def check(eng, files, phase=0, want_bad=None, variants=("device", "host")):
    """both variants give the twin's verdicts and the strict call's outputs over the good files"""
    _, first_w, bad_w = pt.parse_each(files)
    if want_bad is not None:
        assert [f for f, b in enumerate(bad_w) if b is not None] == list(want_bad)
    good = [t for f, t in enumerate(files) if bad_w[f] is None]
    s_pay, s_off, _, s_reg, s_irr = strict_over(eng, good, phase)
    pay_w, off_w, _ = pt.parse(good)
    assert s_pay[:-PAD].tobytes() == pay_w and (s_off == off_w).all() and not s_pay[-PAD:].any()
    n, pb = len(off_w) - 1, len(pay_w)
    lowest = next((f for f, b in enumerate(bad_w) if b is not None), None)
    buf, fb = framed(files, phase)
    infos = []
    for variant in variants:
        rc, info, pay, off, first, bad = call(eng, variant, buf, fb, pb + PAD, n)
        assert rc == 0, (variant, eng._lib.ctmr_last_error(eng._h))
        assert (info.files, info.certificates, info.payload_bytes, info.text_bytes) == (len(files), n, pb, int(fb[-1] - fb[0])), variant
        assert (info.regular, info.irregular) == (s_reg, s_irr), (variant, info.regular, info.irregular, s_reg, s_irr)
        assert (pay[:16] == 0xEE).all() and (pay[16 + pb + PAD:] == 0xEE).all() and (pay[16:16 + pb + PAD] == s_pay).all(), variant
        assert off[0] == GUARD64 and off[-1] == GUARD64 and (off[1:-1] == s_off).all(), variant
        assert first[0] == GUARD64 and first[-1] == GUARD64 and (first[1:-1] == first_w).all(), variant
        assert bad[0] == GUARD64 and bad[-1] == GUARD64
        for f in range(len(files)):
            got = int(bad[1 + f])
            assert (got == NONE) == (bad_w[f] is None), (variant, f, got, bad_w[f])
            if got != NONE:
                assert int(fb[f]) <= got < int(fb[f + 1]), (variant, f, got)
        if lowest is None:
            assert info.bad_file == NONE and info.bad_offset == NONE
        else:
            assert info.bad_file == lowest and info.bad_offset == int(bad[1 + lowest]), variant
        infos.append(info)
    return infos


# ---------------------------------------------------------------------------------------------- no bad file
def test_with_no_bad_file_the_strict_call_is_reproduced(eng):
    fams = list(pc.regular_files().items()) + list(pc.irregular_files().items()) + [("mixed", [pc.mixed_file(), pc.mixed_file() * 3])]
    for k, (name, files) in enumerate(fams):
        buf, fb = framed(files, k % 16)
        _, off_w, _ = pt.parse(files)
        n, pb = len(off_w) - 1, int(off_w[-1])
        s = strict_call(eng, "device", buf, fb, pb + PAD, n)
        assert s[0] == 0, name
        for variant in ("device", "host"):
            rc, info, pay, off, first, bad = call(eng, variant, buf, fb, pb + PAD, n)
            assert rc == 0, (name, variant)
            assert bytes(info) == bytes(s[1]), (name, variant)
            assert (pay == s[2]).all() and (off == s[3]).all() and (first == s[4]).all(), (name, variant)
            assert bad[0] == GUARD64 and bad[-1] == GUARD64 and (bad[1:-1] == NONE).all(), (name, variant)


# ---------------------------------------------------------------------------------------------- one bad file
@pytest.mark.parametrize("name", sorted(pc.REJECTIONS))
def test_every_rejection_in_every_place(eng, name):
    for k, (file_at, block_at) in enumerate((fa, ba) for fa in pc.PLACES for ba in pc.PLACES):
        files, f = pc.place(pc.REJECTIONS[name][0], file_at, block_at)
        check(eng, files, (3 * k + len(name)) % 16, [f])


@pytest.mark.parametrize("name", sorted(pc.TRUNCATIONS))
def test_a_file_that_ends_inside_a_block(eng, name):
    for k, file_at in enumerate(pc.PLACES):
        files, f = pc.place(pc.TRUNCATIONS[name], file_at, "last", truncated=True)
        check(eng, files, 5 * k + 1, [f])
    check(eng, [pc.GOOD[:60], pc.GOOD[60:]], 7, [0, 1])      # the state starts afresh at the boundary: both halves are bad alone


# ---------------------------------------------------------------------------------------------- several bad files
@pytest.mark.parametrize("name", sorted(ec.several_bad()))
def test_several_bad_files_each_found_by_another_pass(eng, name):
    files, bad = ec.several_bad()[name]
    for phase in (0, 5, 11):
        infos = check(eng, files, phase, bad)
    if name == "all bad":
        assert all((i.certificates, i.payload_bytes, i.bad_file) == (0, 0, 0) for i in infos)


@pytest.mark.parametrize("at", list(range(16)) + [1022, 1023, 1024, 1025, 1026])
def test_one_lane_many_files(eng, at):
    """sixteen one-byte files in sixteen bytes, empty files among them, between two good files: a verdict each, the first
    at every residue of a lane and across the edge of a mark block"""
    files, bad = ec.one_lane(at)
    check(eng, files, 0, bad)
    check(eng, ec.one_lane(at, empties=False)[0], 0, variants=("device",))


def test_the_gate_is_a_snapshot(eng):
    """a file mark rejects, its armor lines paired and its blocks irregular, beside a good irregular and a good regular file:
    the counts are the good files', call after call"""
    files = [ec.GOOD_IRREGULAR, ec.BAD_MARK_PAIRED_IRREGULAR, ec.GOOD_REGULAR, ec.BAD_MARK_PAIRED_IRREGULAR * 40, ec.GOOD_IRREGULAR]
    seen = set()
    for _ in range(5):
        for info in check(eng, files, 3, [1, 3]):
            seen.add((info.regular, info.irregular))
    assert seen == {(1, 2)}


def test_the_gather_across_block_edges(eng):
    check(eng, ec.one_block_files(257, (0, 63, 64, 255, 256)), 2, [0, 63, 64, 255, 256])
    check(eng, [ec.GOOD_REGULAR, ec.many_blocks(65, 1, bad=True), ec.GOOD_IRREGULAR], 9, [1])
    check(eng, [ec.BAD_MARK, ec.many_blocks(300, 2), ec.GOOD_IRREGULAR], 14, [0])


# ---------------------------------------------------------------------------------------------- sizing and arguments
def test_buffers_one_short_and_arguments(eng):
    files = [pc.mixed_file(), ec.BAD_CHECK, pc.regular_files()["lengths L=64 e=1"][0], ec.BAD_MARK]
    good = [files[0], files[2]]
    pay_w, off_w, _ = pt.parse(good)
    n, pb = len(off_w) - 1, len(pay_w)
    buf, fb = framed(files, 4)
    for variant in ("device", "host"):
        for pcap, ccap in ((pb + PAD - 1, n), (pb + PAD, n - 1), (0, 0)):
            rc, info, pay, off, first, bad = call(eng, variant, buf, fb, pcap, ccap)
            assert rc == N.E_RANGE and (info.certificates, info.payload_bytes, info.files) == (n, pb, len(files)), (variant, pcap, ccap)
            assert (info.irregular, info.regular, info.bad_file) == (1, n - 1, 1)
            assert untouched(pay, off, first) and (bad == GUARD64).all()
        rc, info, pay, off, first, bad = call(eng, variant, buf, fb, pb + PAD, n, with_bad=False)
        assert rc == N.E_INVAL and untouched(pay, off, first)


def test_no_files_and_empty_files(eng):
    for files in ([], [b""], [b"", b"", b""]):
        buf, fb = framed(files, 6)
        for variant in ("device", "host"):
            rc, info, pay, off, first, bad = call(eng, variant, buf, fb, PAD, 0)
            assert rc == 0 and (info.files, info.certificates, info.payload_bytes, info.bad_file) == (len(files), 0, 0, NONE), variant
            assert (bad[1:-1] == NONE).all() and bad[0] == GUARD64 and bad[-1] == GUARD64
            assert off[1] == 0 and not first[1:-1].any() and not pay[16:16 + PAD].any() and (pay[16 + PAD:] == 0xEE).all()
    check(eng, [b" \n", b"", pc.GOOD, b"\t"], 1, [])


def test_the_python_calls(eng):
    files = [pc.mixed_file(), ec.BAD_FILES, b"", pt.write([b"abc"])]
    ders, first_w, bad_w = pt.parse_each(files)
    pay, off, first, info, bad = eng.pem_decode_each(files)
    assert pay[:-PAD].tobytes() == b"".join(ders) and not pay[-PAD:].any() and (first == first_w).all() and len(off) == len(ders) + 1
    assert [b is None for b in bad] == [b is None for b in bad_w] and info.bad_file == 1
    text, fb = pt.join(files)
    d_text = torch.from_numpy(np.frombuffer(b"x" + text, np.uint8).copy()).to("cuda:0")
    d_pay, d_off, first, info, bad = eng.pem_decode_each_device(d_text, fb + np.uint64(1))
    assert d_pay.cpu().numpy()[:-PAD].tobytes() == b"".join(ders) and (d_off.cpu().numpy().view(np.uint64) == off).all() and (first == first_w).all()
    assert (info.regular, info.irregular) == (3, 1) and bad[1] is not None and int(fb[1]) + 1 <= bad[1] < int(fb[2]) + 1
    assert eng.pem_decode_each([])[4] == []
