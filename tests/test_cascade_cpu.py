"""The CPU twin of the filter cascade (ct_mapreduce_amd/cascade.py) held to tests/cascade_corpus.py byte for byte, the
corpus held to its coverage, crlite_params held to integers worked out by hand (no GPU needed).  DESIGN.md §29."""
import struct

import numpy as np
import pytest

from ct_mapreduce_amd import cascade as CA
from ct_mapreduce_amd import known_image as KI

import cascade_corpus as CC
import find_corpus as FC

CASES = CC.all_cases()


def params_of(c):
    return CA.Params(*c.params)


@pytest.mark.parametrize("c", [c for c in CASES if c.cascade is not None], ids=lambda c: c.name)
def test_the_twin_builds_the_corpus_s_cascade_byte_for_byte(c):
    out, info = CA.build_info(c.revoked, c.known, c.now, params_of(c))
    assert out == c.cascade
    assert CA.build(c.revoked, c.known, c.now, params_of(c)) == out
    assert info["layer"] == c.layers and info["layers"] == len(c.layers) and info["bytes"] == len(out)
    assert (info["r_records"], info["s_records"]) == (len(c.r_keys), len(c.s_keys))
    assert (info["r_host_skipped"], info["s_host_skipped"]) == (c.r_host, c.s_host)
    parsed = CA.parse(out)
    assert parsed["layers"] == c.layers and parsed["salt"] == c.params[5]
    assert (parsed["r_records"], parsed["s_records"], parsed["bytes"]) == (len(c.r_keys), len(c.s_keys), len(out))
    assert CA.query_keys(out, c.r_keys) == b"\1" * len(c.r_keys)
    assert CA.query_keys(out, c.s_keys) == b"\0" * len(c.s_keys)


@pytest.mark.parametrize("c", [c for c in CASES if c.cascade is not None and not c.name.endswith("bad-record")], ids=lambda c: c.name)
def test_the_twin_s_query_of_an_image_answers_every_record_in_order(c):
    """All sets answer, kept or not: the answers are those of the corpus's own walk over the records' keys."""
    for image in (c.revoked, c.known):
        dev = KI._sections(image)[0]
        want = bytes(CC.answer(c.cascade, _digest(ident) + m) for _, ident, m in dev)
        assert CA.query(c.cascade, image) == want


def _digest(ident):
    import base64
    return base64.urlsafe_b64decode(ident)


@pytest.mark.parametrize("c", [c for c in CASES if c.cascade is None], ids=lambda c: c.name)
def test_the_twin_refuses_what_the_corpus_says_is_refused(c):
    if c.notes.get("bad_record"):
        with pytest.raises(KI.ImageError):
            CA.build(c.revoked, c.known, c.now, params_of(c))
        return
    with pytest.raises(CA.CascadeError) as err:
        CA.build(c.revoked, c.known, c.now, params_of(c))
    assert err.value.left == c.left
    assert (c.left > 0) == (not c.notes.get("bad_params"))


def test_the_twin_refuses_a_damaged_cascade():
    damaged, good = CC.damaged()
    assert CA.parse(good.cascade)["layers"] == good.layers
    for name, b in damaged:
        with pytest.raises(CA.CascadeError):
            CA.parse(b)
        with pytest.raises(CA.CascadeError):
            CA.query(b, good.revoked)


def test_the_corpus_covers_what_it_says():
    assert {c.family for c in CASES} == set(CC.FAMILIES) == {"sizes", "lengths", "bits", "sets", "refusals", "host"}
    seen = CC.MESSAGE_LENGTHS
    assert set(seen) == set(range(37, 94))
    assert all(seen[n] >= 10 for n in (55, 56, 63, 64, 65))
    sizes = {(len(c.r_keys), len(c.s_keys)) for c in CASES if c.family == "sizes"}
    assert {(0, 0), (1025, 3), (3, 1025)} <= sizes
    assert all({(0, n), (n, 0), (n, n)} <= sizes for n in CC.SIZES)
    first = {(c.notes["m"], c.params[0]) for c in CASES if c.family == "bits"}
    assert first == {(m, k) for m in CC.BITS for k in (1, 2, 7, 32)}
    assert all((c.cascade is None) == (c.notes["m"] == 1) for c in CASES if c.family == "bits")
    assert max(len(c.layers) for c in CASES) >= 3
    by = {c.name: c for c in CASES}
    assert by["sets-now-before-expiry"].layers[0][4] == 60 and by["sets-now-at-expiry"].layers[0][4] == 20
    assert by["host-long-members"].r_host == 4 and by["host-long-members"].s_host == 2
    assert by["refusal-shared-key"].left > 0
    with pytest.raises(KI.ImageError):     # the bad records of sets-not-kept-bad-record are bad for a reader of all sets
        KI.parse(by["sets-not-kept-bad-record"].revoked)
    with pytest.raises(KI.ImageError):
        KI.parse(by["sets-not-kept-bad-record"].known)


def test_the_layers_of_the_zero_and_one_sided_cases():
    by = {c.name: c for c in CASES}
    assert by["sizes-0-0"].layers == [] and len(by["sizes-0-0"].cascade) == 64
    assert by["sizes-0-257"].layers == [] and len(by["sizes-0-257"].cascade) == 64
    one = by["sizes-257-0"]
    assert len(one.layers) == 1 and one.layers[0] == (1, 2, (257 * 740 + 255) // 256, 128, 257)


def test_crlite_params_against_integers_worked_out_by_hand():
    # p = 1 / √2 > ½ → ½: one hash function, 370/256 bits
    assert CA.crlite_params(1, 1, b"s") == CA.Params(1, 370, 1, 370, 64, b"s")
    # p = 10^3 / (1.41421 · 10^6) = 7.0711e-4, 1 / p = 1414.2, log2 = 10.47 → 11 hash functions, 11 · 370 = 4 070
    assert CA.crlite_params(10 ** 3, 10 ** 6) == CA.Params(11, 4070, 1, 370, 64, b"")
    assert CA.crlite_params(5, 0) == CA.Params(1, 370, 1, 370, 64, b"")
    assert CA.crlite_params(10, 10) == CA.crlite_params(10 ** 6, 10) == CA.Params(1, 370, 1, 370, 64, b"")
    # p = 1 / (4 √2) = 0.1768, 1 / p = 5.657, log2 = 2.5 → 3
    assert CA.crlite_params(1, 4, max_layers=9) == CA.Params(3, 1110, 1, 370, 9, b"")
    assert CA.layer_bits(0, 370) == 1 and CA.layer_bits(1, 370) == 2 and CA.layer_bits(256, 370) == 370 and CA.layer_bits(3, 256) == 3


def test_a_drawn_20_000_200_000_case_answers_all_ones_and_all_zeros():
    rng = np.random.default_rng(20260921)
    raw = rng.integers(0, 256, size=(220_000, 12), dtype=np.uint8)
    raw[:, :4] = np.arange(220_000, dtype="<u4").view(np.uint8).reshape(-1, 4)     # distinct
    lens = rng.integers(4, 13, size=220_000)
    ser = [raw[i, :lens[i]].tobytes() for i in range(220_000)]
    r_sets = [(FC.H0 + h, FC.digest(h & 3), ser[5000 * h:5000 * (h + 1)]) for h in range(4)]
    s_sets = [(FC.H0 + h, FC.digest(h % 5), ser[20_000 + 20_000 * h:20_000 + 20_000 * (h + 1)]) for h in range(10)]
    revoked, known = FC.raw_image(r_sets)[0], FC.raw_image(s_sets)[0]
    p = CA.crlite_params(20_000, 200_000, b"fixed seed")
    out = CA.build(revoked, known, FC.INT64_MIN, p)
    assert struct.unpack_from("<QQ", out, 48) == (20_000, 200_000)
    assert CA.query(out, revoked) == b"\1" * 20_000
    assert CA.query(out, known) == b"\0" * 200_000


def test_a_layer_of_2_32_bits_is_refused_by_the_twin():
    """2^24 records at 65 536/256 bits each are 2^32 bits: the size step of build_info, alone — an image of 2^24 records
    is 805 MB — and one record fewer, one step of bpk_q8 fewer, on either kind of layer."""
    p = CA.Params(1, 65536, 1, 65536, 64, b"")
    for level in (1, 2):
        with pytest.raises(CA.CascadeError):
            CA.layer_shape(2 ** 24, level, p)
        assert CA.layer_shape(2 ** 24 - 1, level, p) == (1, 2 ** 32 - 256)
    assert CA.layer_shape(2 ** 24, 1, CA.Params(1, 65535, 1, 370, 64, b"")) == (1, 2 ** 32 - 2 ** 16)
    with pytest.raises(CA.CascadeError):
        CA.layer_shape(2 ** 31, 2, CA.Params(1, 370, 1, 512, 64, b""))
