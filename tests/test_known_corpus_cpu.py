"""The corpus builder of the every-length tests (tests/known_corpus.py) without a GPU: its image is the canonical one,
and each mix has the structure the GPU tests rely on.  Conditions on the input, not on the code under test: they keep
tests/test_gpu_known_lengths.py from passing on a corpus that no longer reaches the branch a test was written for."""
import hashlib

import numpy as np
import pytest

from ct_mapreduce_amd import known_image as KI
from tests import known_corpus as KC

HOUR0 = 491000
DIGESTS = [hashlib.sha256(b"corpus issuer %d" % i).digest() for i in range(5)]
HOURS = [HOUR0, HOUR0 + 1, HOUR0 + 30]
SIZES = {"uniform": [700, 1, 255, 256, 257], "tiny": [300, 1, 255, 256, 257, 2, 3], "interleaved": [600, 1, 255, 256, 257, 130],
         "runs": [900, 1, 255, 256, 257, 1500], "twins": 0}


def small(mix):
    return KC.make(mix, DIGESTS, HOURS, SIZES[mix], seed=11)


@pytest.mark.parametrize("mix", KC.MIXES)
def test_image_is_canonical_and_every_length_occurs(mix):
    c = small(mix)
    assert c.image == KI.build(c.sets)
    parsed = KI.parse(c.image)
    assert parsed.sets == c.sets and parsed.total == c.members
    assert len(c.sets) == len(DIGESTS) * len(HOURS)
    lens = KC.record_lens(c.image)
    assert len(lens) == parsed.n_members == len(KC.record_sets(c.image))
    want = set(KC.default_lengths(mix))
    if mix == "twins":
        want = {L + z for L in want for z in range(4)}
        assert parsed.n_host_members > 0
        assert {len(m) for v in c.sets.values() for m in v} == want
        want = {L for L in want if L <= 40}
    assert set(lens.tolist()) == want
    if mix != "twins":
        assert not c.capped
        sizes = SIZES[mix]
        assert [len(c.sets[k]) for k in sorted(c.sets)] == [sizes[i % len(sizes)] for i in range(len(c.sets))]


def test_uniform_first_octets_are_arbitrary():
    c = small("uniform")
    first = {m[0] for v in c.sets.values() for m in v if m}
    assert 0x00 in first and 0xff in first and len(first) > 200


def test_interleaved_has_both_classes_in_every_wave():
    long_ = KC.record_lens(small("interleaved").image) > 20
    assert (long_[0::2] == False).all() and (long_[1::2] == True).all()     # noqa: E712
    for w in range(0, len(long_) - 1, 64):
        g = long_[w:w + 64]
        assert g.any() and not g.all()


def test_runs_has_blocks_of_one_class_alone_and_mixed_ones():
    long_ = KC.record_lens(small("runs").image) > 20
    blocks = [long_[b:b + 256] for b in range(0, len(long_) - 255, 256)]
    assert sum(b.all() for b in blocks) >= 1 and sum(not b.any() for b in blocks) >= 1
    assert sum(b.any() and not b.all() for b in blocks) >= 1


def test_tiny_has_chunks_of_text_under_sixteen_bytes_and_is_capped():
    c = small("tiny")
    lens = KC.record_lens(c.image)
    assert lens.max() == 7
    # a chunk of the lists is a run of whole sets: the sets of 1..3 members write at most 3 × 15 bytes, some under 16
    text = {k: sum(2 * len(m) + 1 for m in v) for k, v in c.sets.items()}
    assert sum(t < 16 for t in text.values()) >= 2
    # ... and inside a large set whole 256-blocks stay far below 256 × 81
    assert max(text.values()) < 300 * 15
    # lengths 0..1 hold 257 distinct members: a larger set is capped, and the builder says so
    capped = KC.make("tiny", DIGESTS[:1], HOURS[:2], [257, 400], seed=3, lengths=(0, 1))
    assert [len(capped.sets[k]) for k in sorted(capped.sets)] == [257, 257] and capped.capped == sorted(capped.sets)[1:]
    assert capped.image == KI.build(capped.sets)


def test_twins_differ_in_length_alone_and_cross_both_boundaries():
    c = small("twins")
    meta, rec = KC.split(c.image)
    for key, ms in c.sets.items():
        assert b"" in ms and b"\x00" in ms and b"\x00\x00" in ms
        for L in (17, 18, 19, 20, 37, 38, 39, 40):
            base = [m for m in ms if len(m) == L and m[-1] != 0]
            assert base
            for b in base:
                assert all(b + b"\x00" * z in ms for z in range(4))
    # records that are equal in all 40 octets and differ in serial_len, on both sides of 20/21
    by_octets = {}
    for r in rec[KC.record_sets(c.image) == 0]:
        by_octets.setdefault(r["serial"].tobytes(), []).append(int(r["len"]))
    assert any(min(v) <= 20 < max(v) for v in by_octets.values())
    assert {0, 1, 2, 3, 4, 20, 21, 22, 23, 40} <= set(by_octets[bytes(40)])   # 00, 00 00, ...: one member per length
    assert max(len(m) for v in c.sets.values() for m in v) == 43


def test_fast_image_handles_host_only_keys_and_long_members():
    sets = dict(small("uniform").sets)
    sets[b"serials::2026-01-05-08::not-an-issuer-id"] = [b"\x07\x08", b"\x09" * 45]
    sets[b"serials::2026-01-05::" + KI.issuer_id(DIGESTS[0])] = [b"\x01"]
    key = sorted(sets)[3]
    sets[key] = sorted(sets[key] + [b"\x05" * 41, b"\x06" * 60])
    assert KC.image(sets) == KI.build(sets)
    assert KI.parse(KC.image(sets)).sets == {k: sorted(v) for k, v in sets.items()}


def test_large_corpus_is_built_quickly():
    import time
    t0 = time.perf_counter()
    c = KC.make("uniform", DIGESTS, HOURS, 14000, seed=5)
    dt = time.perf_counter() - t0
    assert c.members == 15 * 14000 and dt < 20
    lens = KC.record_lens(c.image)
    assert np.bincount(lens, minlength=41).min() > 0
