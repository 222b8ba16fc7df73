"""-m gpu: ctmr_pem_decode* (include/ctmr.h) — PEM certificate files as they lie → a packed batch, both
variants through the C ABI, byte for byte against the CPU twin (ct_mapreduce_amd.pem_text).  Every call runs at exact-size
buffers between 0xEE guards, with the device text at a chosen byte phase between bytes that would parse as one more
block; info.regular / info.irregular must be the twin's layout counts; a failing call must leave every buffer as it was."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import pem_text as pt, synth, _native as N  # noqa: E402
from ct_mapreduce_amd.engine import Batch, PemDecodeError  # noqa: E402
from tests import pem_text_corpus as pc  # noqa: E402

PAD = N.PAYLOAD_PAD
DECOY = pt.write_block(b"decoy")       # read, it is one more certificate
NONE = 2**64 - 1
GUARD64 = 0xEEEEEEEEEEEEEEEE
NOW = synth.BASE_TIME


@pytest.fixture(scope="module")
def eng():
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
    yield e
    e.close()


def framed(files, phase):
    """the text between decoys, its first byte at offset ≡ phase (mod 16): (buffer u8, file_bounds into it)"""
    text, fb = pt.join(files)
    front = b" " * ((phase - len(DECOY)) % 16) + DECOY
    assert len(front) % 16 == phase
    buf = np.frombuffer(front + text + DECOY, np.uint8).copy()
    return buf, fb + np.uint64(len(front))


def call(eng, variant, buf, fb, payload_cap, certs_cap):
    """One call between guards → (rc, info, payload with 16 guard bytes on both sides, offsets and file_first with one
    guard word on both sides)."""
    F = len(fb) - 1
    info = N.PemDecodeInfo()
    first = np.full(F + 3, GUARD64, np.uint64)
    lib, h = eng._lib, eng._h
    if variant == "device":
        d_text = torch.from_numpy(buf).to("cuda:0")
        d_pay = torch.full((payload_cap + 32,), 0xEE, dtype=torch.uint8, device="cuda:0")
        d_off = torch.full((certs_cap + 3,), GUARD64 - 2**64, dtype=torch.int64, device="cuda:0")
        assert d_text.data_ptr() % 16 == 0 and d_pay.data_ptr() % 16 == 0
        torch.cuda.synchronize()        # the engine runs on a stream of its own: the guards are written before it starts
        rc = lib.ctmr_pem_decode_device(h, C.c_void_p(d_text.data_ptr()), fb.ctypes.data, F, C.c_void_p(d_pay.data_ptr() + 16), payload_cap,
                                        C.c_void_p(d_off.data_ptr() + 8), certs_cap, first[1:].ctypes.data, C.byref(info))
        torch.cuda.synchronize()
        return rc, info, d_pay.cpu().numpy(), d_off.cpu().numpy().view(np.uint64), first
    pay = np.full(payload_cap + 32, 0xEE, np.uint8)
    off = np.full(certs_cap + 3, GUARD64, np.uint64)
    rc = lib.ctmr_pem_decode(h, buf.ctypes.data, fb.ctypes.data, F, pay[16:].ctypes.data, payload_cap, off[1:].ctypes.data, certs_cap,
                             first[1:].ctypes.data, C.byref(info))
    return rc, info, pay, off, first


def untouched(pay, off, first):
    return (pay == 0xEE).all() and (off == GUARD64).all() and (first == GUARD64).all()


def check_ok(eng, files, phase=0, want=None, variants=("device", "host")):
    """both variants give the twin's result (or `want`: the DERs) at exact-size buffers"""
    pay_w, off_w, first_w = pt.parse(files)
    lay = pt.layout(files)
    if want is not None:
        assert pay_w == b"".join(want) and [int(off_w[k + 1] - off_w[k]) for k in range(len(want))] == [len(d) for d in want]
    n, pb = len(off_w) - 1, len(pay_w)
    n_irr = sum(1 for x in lay if x == ("irregular",))
    buf, fb = framed(files, phase)
    for variant in variants:
        rc, info, pay, off, first = call(eng, variant, buf, fb, pb + PAD, n)
        assert rc == 0, (variant, eng._lib.ctmr_last_error(eng._h))
        assert (info.files, info.certificates, info.payload_bytes, info.text_bytes) == (len(files), n, pb, int(fb[-1] - fb[0]))
        assert (info.regular, info.irregular) == (n - n_irr, n_irr), (variant, info.regular, info.irregular, n_irr)
        assert info.bad_file == NONE and info.bad_offset == NONE
        assert (pay[:16] == 0xEE).all() and (pay[16 + pb + PAD:] == 0xEE).all() and (pay[16 + pb:16 + pb + PAD] == 0).all(), variant
        got = pay[16:16 + pb].tobytes()
        if got != pay_w:
            k = next(i for i in range(pb) if got[i] != pay_w[i])
            raise AssertionError("%s: payload differs at byte %d of %d (certificate %d)" % (variant, k, pb, int(np.searchsorted(off_w, k, "right")) - 1))
        assert off[0] == GUARD64 and off[-1] == GUARD64 and (off[1:-1] == off_w).all(), variant
        assert first[0] == GUARD64 and first[-1] == GUARD64 and (first[1:-1] == first_w).all(), variant
    return pay_w, off_w, lay


def check_bad(eng, files, bad, phase=0):
    """both variants fail with CTMR_E_INVAL, name file `bad` and an offset inside it, and write nothing"""
    buf, fb = framed(files, phase)
    text_bytes = int(fb[-1] - fb[0])
    for variant in ("device", "host"):
        rc, info, pay, off, first = call(eng, variant, buf, fb, text_bytes * 3 // 4 + PAD, (text_bytes + len(files)) // 54 + 1)
        assert rc == N.E_INVAL and info.bad_file == bad, (variant, rc, info.bad_file, bad)
        assert int(fb[bad]) <= info.bad_offset < max(int(fb[bad + 1]), int(fb[bad]) + 1), variant
        assert untouched(pay, off, first), variant


# ---------------------------------------------------------------------------------------------- lengths and contents
@pytest.mark.parametrize("eol", pc.EOLS, ids=["lf", "crlf"])
@pytest.mark.parametrize("line", pc.LINES)
def test_every_decoded_length_and_the_tile_edges(eng, line, eol):
    """DER lengths 0…200 (which pass 48 k − 1, 48 k, 48 k + 1) and 766…770, 1 534…1 538, every content in one file each:
    the payload positions pass through all 16 residues on the way"""
    files = [pt.write(pc.length_ders(kind), line, eol) for kind in pc.CONTENTS]
    _, off, lay = check_ok(eng, files, phase=(line or 1) % 16)
    assert {int(o) % 16 for o in off} == set(range(16)) and all(x[0] == "regular" for x in lay)


def test_every_sextet_at_every_position_and_spare_bits(eng):
    check_ok(eng, pc.regular_files()["sextets"], phase=5, want=pc.sextet_ders() * 2)
    check_ok(eng, [pc.SPARE_BITS_FILE], phase=9, want=pc.SPARE_BITS_DERS)


@pytest.mark.parametrize("name", sorted(pc.regular_files()))
def test_regular_families(eng, name):
    _, _, lay = check_ok(eng, pc.regular_files()[name], phase=len(name) % 16)
    assert all(x[0] == "regular" for x in lay)


# ---------------------------------------------------------------------------------------------- alignment
@pytest.mark.parametrize("phase", range(16))
def test_text_pointer_and_file_boundaries_at_all_residues(eng, phase):
    """file f is f bytes of ws longer than a multiple of 16 would be: the boundaries pass through every residue"""
    files = []
    for f in range(18):
        t = pt.write([pc.content("random", 30 + 5 * f + k, 100 * phase + 10 * f + k) for k in range(3)], (64, 76)[f % 2], pc.EOLS[f % 2])
        files.append(t + b"\n" * ((f + 1 - len(t)) % 16))
    _, fb = pt.join(files)
    assert {int(b) % 16 for b in fb} == set(range(16))
    check_ok(eng, files, phase=phase)


def test_the_first_begin_behind_every_amount_of_ws(eng):
    """0 … 1 026 bytes of ws in front of the first BEGIN: of a file each in one call, and of the text in calls of their own"""
    block = pt.write_block(b"behind ws")
    check_ok(eng, [pc.ws_run(k, k)[:-1] + b"\n" + block if k else block for k in range(0, 1027)], phase=3)
    for k in (1, 15, 16, 17, 1007, 1008, 1009, 1023, 1024, 1025, 1026):
        check_ok(eng, [pc.ws_run(k, k)[:-1] + b"\n" + block], phase=k % 16, variants=("device",))


def test_the_armor_lines_at_every_residue_of_the_mark_block(eng):
    """blocks of 59 bytes (59 is prime to 1 024): over 1 100 of them every byte of both armor lines meets every residue"""
    block = pt.write_block(b"ABC")
    assert len(block) == 59
    check_ok(eng, [block * 1100], phase=7)
    check_ok(eng, [pt.write_block(b"ABC", eol=b"\r\n") * 1100], phase=8)


# ---------------------------------------------------------------------------------------------- irregular blocks
@pytest.mark.parametrize("name", sorted(pc.irregular_files()))
def test_irregular_families(eng, name):
    _, _, lay = check_ok(eng, pc.irregular_files()[name], phase=len(name) % 16)
    assert all(x == ("irregular",) for x in lay)


def test_an_irregular_block_between_two_regular_ones(eng):
    _, _, lay = check_ok(eng, [pc.mixed_file(), pc.mixed_file() * 3], phase=11)
    assert [x[0] for x in lay[:3]] == ["regular", "irregular", "regular"]


# ---------------------------------------------------------------------------------------------- counts
@pytest.mark.parametrize("F", pc.COUNT_FILES)
def test_counts_of_files_and_blocks(eng, F):
    for per in pc.COUNT_BLOCKS:
        check_ok(eng, pc.count_files(F, per), phase=(F + per) % 16, variants=("device",) if F * per > 4000 else ("device", "host"))


def test_empty_and_ws_only_files(eng):
    good = pt.write([b"abc", b"de"], end_eol=b"")       # END at the end of its file with no eol
    for files in ([b""], [b"", b""], [b" \n\t\r"], [b"", good], [good, b""], [b"", good, b"\n\n", good, b""], [b"   ", good, b"", b"\t", good, b" "]):
        check_ok(eng, files, phase=len(files))
    check_ok(eng, [pc.tightest_file(n) for n in (1, 0, 3, 70)], phase=2)


# ---------------------------------------------------------------------------------------------- large
def test_one_certificate_of_a_megabyte_among_short_ones(eng):
    big = pc.content("random", (1 << 20) + 1, 5)
    ders = [b"ab", big, b"cde", big[:5000]]
    check_ok(eng, [pt.write(ders, 64)], phase=13, want=ders, variants=("device",))
    check_ok(eng, [pt.write(ders[:3], 76, b"\r\n")], phase=1, variants=("device",))
    _, _, lay = check_ok(eng, [pt.write([big[:300000]], 64).replace(b"\n", b" \n", 3)], phase=6, variants=("device",))
    assert lay == [("irregular",)]


def test_a_text_of_over_four_gigabytes(eng):
    """a file of a few KB tiled on the device to just over 2^32 bytes: every position is 64-bit, the passes run in turns"""
    unit = pt.write([pc.content("random", 700 + 31 * k, k) for k in range(6)], 64) + pt.write([pc.content("random", 900, 9)], 76, b"\r\n")
    pay_u, off_u, _ = pt.parse([unit])
    reps = (1 << 32) // len(unit) + 2
    total, nu, pu = reps * len(unit), len(off_u) - 1, len(pay_u)
    need = total + reps * pu + PAD + 8 * reps * nu + total // 16 + reps * nu * 8 * 12 + (1 << 30)
    free = torch.cuda.mem_get_info(0)[0]
    if free < need:
        pytest.skip("needs %.1f GB of device memory, %.1f GB are free" % (need / 1e9, free / 1e9))
    dev = "cuda:0"
    d_text = torch.from_numpy(np.frombuffer(unit, np.uint8).copy()).to(dev).repeat(reps)
    fb = np.asarray([0, total], np.uint64)
    torch.cuda.synchronize()            # the engine runs on a stream of its own: the text is whole before it starts
    d_pay, d_off, first, info = eng.pem_decode_device(d_text, fb)
    assert (info.certificates, info.payload_bytes, info.text_bytes, info.irregular) == (reps * nu, reps * pu, total, 0)
    assert first.tolist() == [0, reps * nu]
    want = torch.from_numpy(np.frombuffer(pay_u, np.uint8).copy()).to(dev)
    assert bool((d_pay[:reps * pu].view(reps, pu) == want).all()) and not bool(d_pay[reps * pu:].any())
    want_off = torch.from_numpy(off_u[:-1].astype(np.int64)).to(dev)
    assert bool((d_off[:-1].view(reps, nu) - torch.arange(reps, device=dev, dtype=torch.int64)[:, None] * pu == want_off).all())
    assert int(d_off[-1]) == reps * pu


# ---------------------------------------------------------------------------------------------- failures
@pytest.mark.parametrize("name", sorted(pc.REJECTIONS))
def test_every_rejection_in_every_place(eng, name):
    bad = pc.REJECTIONS[name][0]
    for k, (file_at, block_at) in enumerate((fa, ba) for fa in pc.PLACES for ba in pc.PLACES):
        files, f = pc.place(bad, file_at, block_at)
        check_bad(eng, files, f, phase=(3 * k + len(name)) % 16)


@pytest.mark.parametrize("name", sorted(pc.TRUNCATIONS))
def test_a_file_that_ends_inside_a_block(eng, name):
    for k, file_at in enumerate(pc.PLACES):
        files, f = pc.place(pc.TRUNCATIONS[name], file_at, "last", truncated=True)
        check_bad(eng, files, f, phase=5 * k)
    check_bad(eng, [pc.GOOD[:60], pc.GOOD[60:]], 0)      # the state starts afresh at the boundary


def test_the_lowest_bad_file_is_named(eng):
    files = [pc.GOOD] * 40
    for bads in ([39, 7, 22], [0, 39], [38]):
        fs = list(files)
        for b in bads:
            fs[b] = pc.REJECTIONS["a comment" if b % 2 else "three '='"][0]
        check_bad(eng, fs, min(bads))


def test_buffers_one_short(eng):
    files = pc.regular_files()["lengths L=64 e=1"] + [pc.mixed_file()]
    pay_w, off_w, _ = pt.parse(files)
    n, pb = len(off_w) - 1, len(pay_w)
    buf, fb = framed(files, 4)
    for variant in ("device", "host"):
        for pcap, ccap in ((pb + PAD - 1, n), (pb + PAD, n - 1), (0, 0)):
            rc, info, pay, off, first = call(eng, variant, buf, fb, pcap, ccap)
            assert rc == N.E_RANGE and (info.certificates, info.payload_bytes, info.files) == (n, pb, len(files)), (variant, pcap, ccap)
            assert info.irregular == 1 and info.regular == n - 1 and untouched(pay, off, first)
    # the bounds a caller may use without a first call hold
    assert pb <= int(fb[-1] - fb[0]) * 3 // 4 and n <= (int(fb[-1] - fb[0]) + len(files)) // 54


def test_the_python_calls(eng):
    files = [pc.mixed_file(), b"", pt.write([b"abc"])]
    pay_w, off_w, first_w = pt.parse(files)
    pay, off, first, info = eng.pem_decode(files)
    assert pay[:-PAD].tobytes() == pay_w and not pay[-PAD:].any() and (off == off_w).all() and (first == first_w).all()
    text, fb = pt.join(files)
    d_text = torch.from_numpy(np.frombuffer(b"x" + text, np.uint8).copy()).to("cuda:0")
    d_pay, d_off, first, info = eng.pem_decode_device(d_text, fb + np.uint64(1))
    assert d_pay.cpu().numpy()[:-PAD].tobytes() == pay_w and (d_off.cpu().numpy().view(np.uint64) == off_w).all() and (first == first_w).all()
    assert (info.regular, info.irregular) == (3, 1)
    with pytest.raises(PemDecodeError) as err:
        eng.pem_decode([files[0], pc.REJECTIONS["X509 CRL"][0]])
    assert err.value.bad_file == 1 and err.value.code == N.E_INVAL
    assert eng.pem_decode([])[3].certificates == 0 and eng.map_pem([], []).stats.n == 0


# ---------------------------------------------------------------------------------------------- round trip
def test_round_trip_through_the_encoder_and_the_map():
    """4 096 synthetic certificates → pem_encode_device → pem_decode_device gives back payload and offsets byte for byte;
    map_pem of that text gives the records, NEW list and sets of map_batch_device of the original batch"""
    n, dev = 4096, "cuda:0"
    cfg = synth.config(seed=20261019, n_issuers=1, dup_permille=100, ca_permille=20, expired_permille=20)
    batch = synth.host_batch(cfg, 0, n)
    issuers = synth.issuers(cfg)
    a = ctmr.Engine(device=0, table_slots=1 << 14, pair_slots=1 << 10)
    b = ctmr.Engine(device=0, table_slots=1 << 14, pair_slots=1 << 10)
    for e in (a, b):
        e.add_issuers(issuers)
        e.set_filter(b"", False, NOW)
    pb = int(batch.offsets[n])
    d_pay = torch.from_numpy(np.concatenate([batch.payload[:pb], np.zeros(PAD, np.uint8)])).to(dev)
    d_off = torch.from_numpy(batch.offsets.astype(np.int64)).to(dev)
    d_idx = torch.arange(n, dtype=torch.int64, device=dev)
    d_po = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()            # the engines run on streams of their own
    total = a.pem_encode_device(d_pay.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(), n, 0, 0, d_po.data_ptr())
    d_pem = torch.zeros(total, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    a.pem_encode_device(d_pay.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(), n, d_pem.data_ptr(), total, d_po.data_ptr())
    d_pay2, d_off2, first, info = a.pem_decode_device(d_pem, np.asarray([0, total], np.uint64))
    assert (info.certificates, info.payload_bytes, info.regular, info.irregular) == (n, pb, n, 0)
    assert bool((d_pay2 == d_pay).all()) and bool((d_off2 == d_off).all())
    # the map: the original batch on one engine, the text on the other
    d_iss = torch.from_numpy(batch.issuer_idx.view(np.int32).copy()).to(dev)
    d_et = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_rec = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    d_new = torch.zeros(n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    st = a.map_batch_device(d_pay.data_ptr(), d_off.data_ptr(), d_iss.data_ptr(), d_et.data_ptr(), n, d_rec.data_ptr(), d_new.data_ptr())
    assert (batch.issuer_idx == 0).all()
    res = b.map_pem([d_pem.cpu().numpy().tobytes()], [0])
    assert (res.records.view(np.uint8) == d_rec.cpu().numpy()).all()
    assert (res.new_idx == d_new.cpu().numpy().view(np.uint64)[:st.n_new]).all() and 0 < st.n_new < n
    assert list(res.stats.by_status) == list(st.by_status) and res.stats.n_new == st.n_new
    assert sorted(a.keys(b"serials::*")) == sorted(b.keys(b"serials::*")) and a.total_count() == b.total_count() > 0
    for key in a.keys(b"serials::*")[:20]:
        assert a.set_list(key) == b.set_list(key)
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- real certificates
@pytest.mark.parametrize("split", ["one file", "161 files"])
@pytest.mark.parametrize("profile", ["reference", "fast"])
def test_ca_roots_through_map_pem(profile, split):
    """tests/golden/ca_roots.pem through Engine.map_pem, the roots registered as their own issuers: records and sets ≡ the
    oracle over the same DER"""
    from oracle import oracle as orc
    from tests.gpu_common import assert_records_equal, assert_state_equal
    from tests.test_real_certs_cpu import CA_ROOTS
    text = open(CA_ROOTS, "rb").read()
    pay, off, _ = pt.parse([text])
    ders = [pay[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)]
    assert len(ders) == 161
    if split == "one file":
        files, file_iss = [text], [0]              # one file lies below one issuer: the first root
    else:       # a block per file, each below its own issuer
        cut = [0] + [k + len(pt.END) + 1 for k in range(len(text)) if text.startswith(pt.END, k)]
        files, file_iss = [text[cut[k]:cut[k + 1]] for k in range(161)], list(range(161))
        assert b"".join(files) == text[:cut[-1]]
    for log_expired, now in ((True, NOW), (False, NOW)):
        eng = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
        eng.set_profile(profile)
        eng.add_issuers(ders)
        eng.set_filter(b"", log_expired, now)
        res = eng.map_pem(files, file_iss)
        batch = Batch.from_certs(ders, [0] * 161 if split == "one file" else list(range(161)))
        batch.payload = np.concatenate([batch.payload, np.zeros(PAD, np.uint8)])
        o = orc.Engine(b"", log_expired, now)
        o.set_profile(profile)
        io = np.zeros(162, np.uint64)
        io[1:] = np.cumsum([len(d) for d in ders])
        st, unk, eh = o.batch(batch.payload, batch.offsets, batch.issuer_idx, np.frombuffer(b"".join(ders), np.uint8), io, entry_type=batch.entry_type)
        if profile == "reference":
            assert_records_equal(res, batch, st, unk, eh)
        else:
            assert (res.records["status"] == st).all() and (((res.records["flags"] & 2) != 0) == (unk != 0)).all()
            assert (res.new_idx == np.nonzero(unk)[0]).all()
        assert_state_equal(eng, o, 161)
        eng.close()
