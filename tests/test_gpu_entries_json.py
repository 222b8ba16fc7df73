"""-m gpu: ctmr_entries_json* (include/ctmr.h) — get-entries HTTP bodies as they lie → raw entries, both
variants through the C ABI, byte for byte against the CPU twin (ct_mapreduce_amd.get_entries) and Python's json + base64.
Every call runs at exact-size buffers between 0xEE guards, with the device text at a chosen byte phase between bytes that
would parse as more entries; a failing call must leave every buffer as it was."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import get_entries as ge, synth, _native as N  # noqa: E402
from ct_mapreduce_amd.engine import EntriesJsonError, RawEntries  # noqa: E402
from tests import get_entries_corpus as gc  # noqa: E402

PAD = N.PAYLOAD_PAD
DECOY = b'{"leaf_input":"QUJD","extra_data":"QUJD"},"'   # an entry and one more quote: read, it flips the string state
NONE = 2**64 - 1
GUARD64 = 0xEEEEEEEEEEEEEEEE


@pytest.fixture(scope="module")
def eng():
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
    yield e
    e.close()


def framed(bodies, phase):
    """the text between decoys, its first byte at offset ≡ phase (mod 16): (buffer u8, resp_bounds into it)"""
    text, rb = ge.join(bodies)
    front = b" " * ((phase - len(DECOY)) % 16) + DECOY
    assert len(front) % 16 == phase
    buf = np.frombuffer(front + text + b'",' + DECOY, np.uint8).copy()
    return buf, rb + np.uint64(len(front))


def call(eng, variant, buf, rb, blob_cap, entries_cap):
    """One call between guards → (rc, info, blob with 16 guard bytes on both sides, bounds and resp_first with one guard
    word on both sides)."""
    R = len(rb) - 1
    info = N.EntriesJsonInfo()
    first = np.full(R + 3, GUARD64, np.uint64)
    lib, h = eng._lib, eng._h
    if variant == "device":
        d_text = torch.from_numpy(buf).to("cuda:0")
        d_blob = torch.full((blob_cap + 32,), 0xEE, dtype=torch.uint8, device="cuda:0")
        d_bounds = torch.full((2 * entries_cap + 3,), GUARD64 - 2**64, dtype=torch.int64, device="cuda:0")
        assert d_text.data_ptr() % 16 == 0 and d_blob.data_ptr() % 16 == 0
        rc = lib.ctmr_entries_json_device(h, C.c_void_p(d_text.data_ptr()), rb.ctypes.data, R, C.c_void_p(d_blob.data_ptr() + 16), blob_cap,
                                          C.c_void_p(d_bounds.data_ptr() + 8), entries_cap, first[1:].ctypes.data, C.byref(info))
        torch.cuda.synchronize()
        return rc, info, d_blob.cpu().numpy(), d_bounds.cpu().numpy().view(np.uint64), first
    blob = np.full(blob_cap + 32, 0xEE, np.uint8)
    bounds = np.full(2 * entries_cap + 3, GUARD64, np.uint64)
    rc = lib.ctmr_entries_json(h, buf.ctypes.data, rb.ctypes.data, R, blob[16:].ctypes.data, blob_cap, bounds[1:].ctypes.data, entries_cap,
                               first[1:].ctypes.data, C.byref(info))
    return rc, info, blob, bounds, first


def untouched(blob, bounds, first):
    return (blob == 0xEE).all() and (bounds == GUARD64).all() and (first == GUARD64).all()


def check_ok(eng, bodies, phase=0, want=None):
    """both variants give the twin's result (or `want`: (blob bytes, bounds)) at exact-size buffers"""
    blob_w, bounds_w, first_w = ge.parse(bodies)
    if want is not None:
        assert blob_w == want[0] and (bounds_w == want[1]).all()
    n, bb = (len(bounds_w) - 1) // 2, len(blob_w)
    buf, rb = framed(bodies, phase)
    for variant in ("device", "host"):
        rc, info, blob, bounds, first = call(eng, variant, buf, rb, bb + PAD, n)
        assert rc == 0, (variant, eng._lib.ctmr_last_error(eng._h))
        assert (info.responses, info.entries, info.blob_bytes, info.text_bytes) == (len(bodies), n, bb, int(rb[-1] - rb[0]))
        assert info.bad_response == NONE
        assert (blob[:16] == 0xEE).all() and (blob[16 + bb + PAD:] == 0xEE).all() and (blob[16 + bb:16 + bb + PAD] == 0).all(), variant
        got = blob[16:16 + bb].tobytes()
        if got != blob_w:
            k = next(i for i in range(bb) if got[i] != blob_w[i])
            raise AssertionError("%s: blob differs at byte %d of %d" % (variant, k, bb))
        assert bounds[0] == GUARD64 and bounds[-1] == GUARD64 and (bounds[1:-1] == bounds_w).all(), variant
        assert first[0] == GUARD64 and first[-1] == GUARD64 and (first[1:-1] == first_w).all(), variant
    return blob_w, bounds_w


def check_bad(eng, bodies, bad, phase=0):
    """both variants fail with CTMR_E_INVAL, name response `bad` and an offset inside it, and write nothing"""
    buf, rb = framed(bodies, phase)
    text_bytes = int(rb[-1] - rb[0])
    for variant in ("device", "host"):
        rc, info, blob, bounds, first = call(eng, variant, buf, rb, text_bytes * 3 // 4 + PAD, text_bytes // 34 + 1)
        assert rc == N.E_INVAL and info.bad_response == bad, (variant, rc, info.bad_response, bad)
        assert int(rb[bad]) <= info.bad_offset < max(int(rb[bad + 1]), int(rb[bad]) + 1), variant
        assert untouched(blob, bounds, first), variant


# ---------------------------------------------------------------------------------------------- lengths and contents
@pytest.mark.parametrize("kind", gc.CONTENTS)
def test_every_decoded_length_and_the_tile_edges(eng, kind):
    """leaf and extra of every length 0…200 crossed, and TILE·3/4 − 2 … + 2, 2·TILE·3/4 − 2 … + 2 of the decode tile
    (768 bytes): the blob positions pass through all 16 residues on the way."""
    entries = gc.length_entries(kind) + gc.tile_entries(kind)
    _, bounds = check_ok(eng, ge.write(entries, 64), phase=gc.CONTENTS.index(kind) * 3)
    assert {int(b) % 16 for b in bounds} == set(range(16))
    check_ok(eng, ge.write(gc.tile_entries(kind), 4, "alternate"), phase=15)


def test_every_sextet_at_every_position_and_spare_bits(eng):
    check_ok(eng, ge.write(gc.sextet_entries(), 2, "alternate"), phase=5)
    check_ok(eng, [gc.spare_bits_body()], phase=9, want=(b"ABA\xff\xef\xfb", np.asarray([0, 2, 3, 5, 6], np.uint64)))


# ---------------------------------------------------------------------------------------------- phases
@pytest.mark.parametrize("phase", range(16))
def test_text_pointer_and_response_boundaries_at_all_residues(eng, phase):
    entries = gc.small_entries(34, seed=phase, lo=0, hi=90)
    bodies = []
    for k in range(17):   # every body 1 (mod 16) bytes long: the boundaries step through all residues
        b = ge.write_one(entries[2 * k:2 * k + 2], ge.STYLES[k % 4])
        bodies.append(b + b" " * ((1 - len(b)) % 16))
    _, rb = ge.join(bodies)
    assert {int(x) % 16 for x in rb} == set(range(16))
    check_ok(eng, bodies, phase)


def test_every_token_byte_across_a_mark_block_edge(eng):
    """One entry of about 110 bytes of text behind 0 … BLOCK + 2 bytes of white space.  Every shift is a response of its
    own, filled up to a multiple of the mark block, and the text starts on a block edge: shift w puts every byte of the
    entry w bytes further into its block."""
    e, body = gc.one_entry_110()
    B = gc.MARK_BLOCK
    bodies = []
    for w in range(B + 3):
        b = b" \t\r\n"[w & 3:(w & 3) + 1] * w + body
        bodies.append(b + b"\n" * (-len(b) % B))
    marks = [k for k, c in enumerate(body) if c in b'{}[]:,"']
    for k in marks:
        assert {(w + k) % B for w in range(B + 3)} == set(range(B))
    blob, bounds = check_ok(eng, bodies, phase=0)
    assert blob == (e[0][0] + e[0][1]) * (B + 3)


# ---------------------------------------------------------------------------------------------- styles
@pytest.mark.parametrize("style", ge.STYLES)
def test_styles(eng, style):
    entries = gc.small_entries(150, seed=11, lo=0, hi=300)
    check_ok(eng, ge.write(entries, 40, style), phase=3)


def test_white_space_between_every_pair_of_tokens(eng):
    """0 … 70 ws bytes in every gap in turn — in front of the first token and behind the last included; each a response"""
    e = gc.small_entries(2, seed=4)
    bodies = [b for _, _, b in gc.gap_bodies(e)]
    assert len(bodies) == (len(ge.tokens(e)) + 1) * 71
    blob, _ = check_ok(eng, bodies, phase=7)
    assert blob == b"".join(a + b for a, b in e) * len(bodies)


# ---------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("R", [0, 1, 2, 63, 64, 65, 257])
def test_shapes(eng, R):
    for per in (0, 1, 2, 64, 65):
        entries = gc.small_entries(R * per, seed=R + per, lo=0, hi=24)
        check_ok(eng, ge.write(entries, [per] * R), phase=(R + per) % 16)


def test_empty_responses_first_in_the_middle_and_last(eng):
    entries = gc.small_entries(9, seed=2)
    for counts in ([0, 4, 5], [4, 0, 0, 5], [4, 5, 0], [0, 0, 9, 0, 0], [0], [0, 0, 0]):
        bodies = ge.write(entries[:sum(counts)], counts, "indent")
        check_ok(eng, bodies, phase=11)
        assert (ge.parse(bodies)[2] == np.concatenate([[0], np.cumsum(counts)])).all()


# ---------------------------------------------------------------------------------------------- large
def test_one_string_of_a_thousand_tiles_among_short_ones(eng):
    entries = gc.small_entries(40, seed=6)
    entries[17] = (gc.content("random", 5), gc.content("random", (1 << 20) + 1))
    entries[18] = (gc.content("ramp1", (1 << 20) + 1), b"")
    check_ok(eng, ge.write(entries, 16), phase=13)


def test_a_text_of_just_over_4_gib(eng):
    """One response of about 1 MiB repeated on the device until the text passes 2^32 bytes: the smallest shape at which a
    32-bit position goes wrong.  The blob is compared on the device with the one response's blob, viewed as rows; the
    bounds with numpy's arithmetic."""
    entries = gc.small_entries(128, seed=9, lo=2000, hi=4200)
    body = ge.write_one(entries)
    blob_w, bounds_w, _ = ge.parse([body])
    reps = (1 << 32) // len(body) + 1
    assert 900_000 < len(body) < 1_300_000 and reps * len(body) > 1 << 32
    d_text = torch.from_numpy(np.frombuffer(body, np.uint8).copy()).to("cuda:0").repeat(reps)
    rb = np.arange(reps + 1, dtype=np.uint64) * np.uint64(len(body))
    d_blob, d_bounds, first, info = eng.entries_json_device(d_text, rb)
    del d_text
    n1, b1 = len(entries), len(blob_w)
    assert (info.entries, info.blob_bytes, info.text_bytes) == (n1 * reps, b1 * reps, len(body) * reps)
    assert (first == np.arange(reps + 1, dtype=np.uint64) * np.uint64(n1)).all()
    row = torch.from_numpy(np.frombuffer(blob_w, np.uint8).copy()).to("cuda:0")
    assert bool((d_blob[:b1 * reps].view(reps, b1) == row).all())
    assert bool((d_blob[b1 * reps:] == 0).all()) and d_blob.numel() == b1 * reps + PAD
    want = (np.arange(reps, dtype=np.uint64)[:, None] * np.uint64(b1) + bounds_w[None, :-1]).reshape(-1)
    got = d_bounds.cpu().numpy().view(np.uint64)
    assert (got[:-1] == want).all() and int(got[-1]) == b1 * reps


# ---------------------------------------------------------------------------------------------- rejections
@pytest.mark.parametrize("rej", gc.REJECTIONS, ids=lambda r: r["name"])
def test_rejections_in_the_first_a_middle_and_the_last_response_and_entry(eng, rej):
    for k, (bodies, bad) in enumerate(gc.rejection_cases(rej)):
        check_bad(eng, bodies, bad, phase=(5 * k + 2) % 16)


def test_bodies_outside_the_grammar_and_a_string_across_a_boundary(eng):
    good = ge.write(gc.small_entries(6, seed=8), 2)
    for name, body in gc.BAD_BODIES:
        for r in range(3):
            bodies = list(good)
            bodies[r] = body
            check_bad(eng, bodies, r, phase=4 + r)
    check_bad(eng, [b"", b""], 0)
    check_bad(eng, [good[0], b'{"entries":[', b']}'], 1)
    # the first of the pair ends inside a string; together they are one valid body
    pair, entries = gc.split_string_pair()
    check_ok(eng, [b"".join(pair)], phase=6, want=(b"".join(a + b for a, b in entries), ge.parse([b"".join(pair)])[1]))
    check_bad(eng, pair, 0, phase=6)
    check_bad(eng, [good[0]] + pair + [good[1]], 1, phase=1)
    check_bad(eng, [good[0], good[1]] + pair, 2, phase=12)


# ---------------------------------------------------------------------------------------------- sizing
def test_buffers_one_short_give_range_with_the_twin_s_sizes_and_nothing_written(eng):
    bodies = ge.write(gc.small_entries(50, seed=12), 7)
    blob_w, bounds_w, _ = ge.parse(bodies)
    n, bb = 50, len(blob_w)
    buf, rb = framed(bodies, 2)
    for variant in ("device", "host"):
        for blob_cap, entries_cap in ((bb + PAD - 1, n), (bb + PAD, n - 1), (0, 0)):
            rc, info, blob, bounds, first = call(eng, variant, buf, rb, blob_cap, entries_cap)
            assert rc == N.E_RANGE, (variant, blob_cap, entries_cap, rc)
            assert (info.responses, info.entries, info.blob_bytes, info.text_bytes, info.bad_response) == (len(bodies), n, bb, int(rb[-1] - rb[0]), NONE)
            assert untouched(blob, bounds, first)
        assert call(eng, variant, buf, rb, bb + PAD, n)[0] == 0
    # the bounds a caller may size by without a first call
    assert bb <= 3 * int(rb[-1] - rb[0]) // 4 and n <= int(rb[-1] - rb[0]) // 34
    assert len(ge.write_one([(b"", b"")])) == 14 + 33


def test_a_bad_argument_names_no_response(eng):
    """null resp_bounds, a null text, a blob off its 16-byte alignment: CTMR_E_INVAL with bad_response = UINT64_MAX in an
    info that was zero before, so that no caller takes it for "response 0 is outside the grammar"; nothing written"""
    buf, rb = framed(ge.write(gc.small_entries(4, seed=14), 2), 3)
    d_text = torch.from_numpy(buf).to("cuda:0")
    d_blob = torch.full((len(buf) + 64,), 0xEE, dtype=torch.uint8, device="cuda:0")
    d_bounds = torch.full((64,), GUARD64 - 2**64, dtype=torch.int64, device="cuda:0")
    blob, bounds = np.full(len(buf) + 64, 0xEE, np.uint8), np.full(64, GUARD64, np.uint64)
    lib, h, R = eng._lib, eng._h, len(rb) - 1
    dev = (lib.ctmr_entries_json_device, d_text.data_ptr(), d_blob.data_ptr(), d_bounds.data_ptr())
    host = (lib.ctmr_entries_json, buf.ctypes.data, blob.ctypes.data, bounds.ctypes.data)
    for fn, text, out, bnd in (dev, host):
        cases = [(text, None, out), (None, rb.ctypes.data, out)] + ([(text, rb.ctypes.data, out + 8)] if fn is dev[0] else [])
        for t, b, o in cases:
            info = N.EntriesJsonInfo()
            rc = fn(h, C.c_void_p(t) if t else None, b, R, C.c_void_p(o), len(buf), C.c_void_p(bnd), 16, None, C.byref(info))
            assert rc == N.E_INVAL and info.bad_response == NONE and info.bad_offset == NONE
    torch.cuda.synchronize()
    assert (d_blob.cpu().numpy() == 0xEE).all() and (d_bounds.cpu().numpy().view(np.uint64) == GUARD64).all()
    assert (blob == 0xEE).all() and (bounds == GUARD64).all()
    info = N.EntriesJsonInfo()   # descending bounds: a bad argument too
    down = np.asarray([5, 4], np.uint64)
    rc = lib.ctmr_entries_json_device(h, C.c_void_p(d_text.data_ptr()), down.ctypes.data, 1, C.c_void_p(d_blob.data_ptr()), len(buf),
                                      C.c_void_p(d_bounds.data_ptr()), 16, None, C.byref(info))
    assert rc == N.E_INVAL and info.bad_response == NONE
    with pytest.raises(ValueError):
        eng.entries_json_device(d_text, down)


# ---------------------------------------------------------------------------------------------- end to end
def test_python_methods_and_the_error_they_raise(eng):
    entries = gc.small_entries(30, seed=13)
    bodies = ge.write(entries, 8, "indent")
    raw = eng.entries_json(bodies)
    blob_w, bounds_w, first_w = ge.parse(bodies)
    assert isinstance(raw, RawEntries) and raw.blob.tobytes() == blob_w + bytes(PAD) and (raw.bounds == bounds_w).all() and (raw.resp_first == first_w).all()
    assert [(raw.leaf_input(i), raw.extra_data(i)) for i in range(raw.n)] == entries
    empty = eng.map_entries_json([b'{"entries":[]}', b'{"entries":[]}'])
    assert len(empty.records) == len(empty.new_idx) == len(empty.timestamp) == 0 and empty.stats.n == 0
    none = eng.entries_json([])
    assert none.n == 0 and none.blob.tobytes() == bytes(PAD) and (none.resp_first == [0]).all()
    bodies[2] = bodies[2].replace(b"leaf_input", b"leaf_inpuT", 1)
    with pytest.raises(EntriesJsonError) as x:
        eng.entries_json(bodies)
    assert x.value.bad_response == 2 and x.value.code == N.E_INVAL


def test_the_reference_certificates_through_map_entries_json():
    """tests/golden/entries_from_reference_pems.json as get-entries bodies → Engine.map_entries_json: the fixture's
    statuses and final keys, as the raw-entry test asks of map_entries."""
    from tests.test_oracle_golden import load_entry_fixture, STATUS_NAMES
    fx, pairs, raw = load_entry_fixture()
    for style, per in (("compact", len(pairs)), ("indent", 3), ("alternate", 1)):
        e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
        e.set_filter(fx["filter"].encode(), fx["log_expired"], fx["now"])
        res = e.map_entries_json(ge.write(pairs, per, style))
        for i, x in enumerate(fx["entries"]):
            r = res.records[i]
            assert int(r["status"]) == STATUS_NAMES[x["status"]] and bool(r["flags"] & 2) == x["was_unknown"], x["name"]
            assert int(res.timestamp[i]) == x["timestamp"]
            if x.get("serial_hex"):
                assert bytes(r["serial"][:int(r["serial_len"])]).hex() == x["serial_hex"]
        assert sorted(k.decode() for k in e.keys(b"serials::*")) == fx["final_keys"]
        assert e.total_count() == fx["final_total_count"]
        e.close()


def test_synthetic_entries_as_seven_responses(eng):
    """4 096 entries of synth_entries_device written as 7 responses decode to the synthetic blob and bounds byte for
    byte, and map_entries_json gives the records map_entries_device gives on the original."""
    n = 4096
    cfg = synth.config(seed=20261019, n_issuers=16, dup_permille=100)
    cap = n * 6144 + 64
    d_blob0 = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    d_bounds0 = torch.zeros(2 * n + 1, dtype=torch.int64, device="cuda:0")
    used = eng.synth_entries_device(cfg, 0, n, d_bounds0.data_ptr(), d_blob0.data_ptr(), cap)
    blob0, bounds0 = d_blob0[:used].cpu().numpy(), d_bounds0.cpu().numpy().view(np.uint64)
    raw0 = RawEntries(blob0, bounds0)
    bodies = ge.write([(raw0.leaf_input(i), raw0.extra_data(i)) for i in range(n)], [600, 600, 0, 600, 600, 600, 1096])
    assert len(bodies) == 7
    text, rb = ge.join(bodies)
    d_text = torch.from_numpy(np.frombuffer(b"x" + text, np.uint8).copy()).to("cuda:0")
    d_blob, d_bounds, first, info = eng.entries_json_device(d_text, rb + np.uint64(1))
    assert info.entries == n and info.blob_bytes == used
    assert torch.equal(d_blob[:used], d_blob0[:used]) and torch.equal(d_bounds, d_bounds0)
    assert (first == np.concatenate([[0], np.cumsum([600, 600, 0, 600, 600, 600, 1096])])).all()
    res = []
    for k in range(2):
        e = ctmr.Engine(device=0, table_slots=1 << 14, pair_slots=1 << 12)
        e.set_filter(b"", False, synth.BASE_TIME)
        if k == 0:
            res.append(e.map_entries_json(bodies))
        else:
            d_rec = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
            d_new = torch.zeros(n, dtype=torch.int64, device="cuda:0")
            st, ds = e.map_entries_device(d_blob0.data_ptr(), d_bounds0.data_ptr(), n, d_rec.data_ptr(), d_new.data_ptr())
            assert st.n_new == res[0].stats.n_new > 0
            assert d_rec.cpu().numpy().tobytes() == res[0].records.tobytes()
            assert (d_new.cpu().numpy().view(np.uint64)[:st.n_new] == res[0].new_idx).all()
        e.close()
