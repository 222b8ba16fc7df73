"""-m gpu: one image through every consumer of the image kernels' shared run walk (kernels/image.h known_run_set,
KnownSegs, KnownFlags; engine/image.inc known_cut_sets): lists from an image, the RESP writer, sort, union,
find, split, and the cascade build and query.  Each result equals its CPU twin's, byte for byte, with the call's chunk
override unset and at 1, 64 and 257 records per run.

K (tests/known_corpus.make, two issuers): in image order 70 sets of one record — a wave spans 64 sets —, then sets of 63,
64, 65, 255, 256, 257 and 1 records, and two host pairs.  A third of the sets, 26, have an hour that `NOW` makes expired.
An image's sets lie in key order, which for four-digit years is the order of (hour, Issuer.ID): the expired sets are
therefore the first 26 of the image, not every third one, and the layout is chosen so that what this allows still holds
where it can go wrong.
  - The calls that walk the kept sets in image order (find, split, cascade) read virtual record v at image record v + 26:
    their waves and blocks begin strictly inside the image's, and the last set that is not kept lies strictly inside
    wave 0 and block 0 of the image, next to kept records.
  - The lists walk the kept sets per issuer: there src − dst changes from segment to segment, inside a wave and in a
    segment that crosses a block edge.
P is half of K's kept records plus as many serials K does not hold.
"""
import functools
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import cascade as CA, known_image as KI, _native as N  # noqa: E402
from tests import find_corpus as FC, known_corpus as KC  # noqa: E402
from tests.test_gpu_cascade import build as cascade_build  # noqa: E402
from tests.test_gpu_known_find import call as find_call, damaged_record  # noqa: E402
from tests.test_gpu_known_split import call as split_call  # noqa: E402

DIGESTS = [FC.digest(3), FC.digest(4)]
HOURS = [FC.H0 + k for k in range(39)]                    # × two issuers: 78 keys, the last one dropped
SIZES = [1] * 70 + [63, 64, 65, 255, 256, 257, 1]
EXPIRED = 26                                              # the sets of the first 13 hours
NOW = (FC.H0 + 13) * 3600
PER = 100                                                 # members per SADD command: the larger sets take several
PARAMS = CA.Params(2, 740, 1, 370, 64, b"run walk")
CHUNKS = ("CTMR_KNOWN_LISTS_CHUNK", "CTMR_KNOWN_RESP_CHUNK", "CTMR_KNOWN_SORT_CHUNK", "CTMR_KNOWN_FIND_CHUNK", "CTMR_KNOWN_SPLIT_CHUNK",
          "CTMR_CASCADE_CHUNK")


@pytest.fixture(scope="module")
def eng():
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)   # no issuer registered: the calls need none
    yield e
    e.close()


def set_records(img):
    """(hour, issuer ordinal, first record, count) of every set record of an image."""
    h = KI._HEADER.unpack_from(img, 0)
    return [KI._SET.unpack_from(img, 64 + 32 * h[3] + 24 * s) for s in range(h[5])]


@functools.lru_cache(None)
def operands():
    """K, P, the other operands made of them, and every twin's result: computed once, never changed."""
    sets = dict(KC.make("uniform", DIGESTS, HOURS, SIZES + [1], seed=5, lengths=tuple(range(8, 40))).sets)
    keys = sorted(sets)
    del sets[keys[-1]]
    keys = keys[:-1]
    sets[keys[3]] = sets[keys[3]] + [b"\x51" * 41]        # two host pairs: under an expired key and under a kept one
    sets[keys[40]] = sets[keys[40]] + [b"\x52" * 45]
    known = KC.image(sets)
    assert [c for _, _, _, c in set_records(known)] == SIZES
    kept = [(key, m) for key, m in KI.records(known)[0] if FC.kept(KI.parse_key(key)[0], NOW)]
    last = kept[-1]
    drawn = [km for km in kept[::2] if km != last]        # K's last record stays a miss: the second test damages it there
    held = {(KI.parse_key(key)[1], m) for key, m in KI.records(known)[0]}
    by_digest = {d: [] for d in DIGESTS}
    for key, m in drawn:
        by_digest[KI.parse_key(key)[1]].append(m)
    for j in range(len(drawn)):
        stranger = (DIGESTS[j & 1], b"\xff\xfe" + j.to_bytes(4, "big") + b"\x07" * 14)
        assert stranger not in held
        by_digest[stranger[0]].append(stranger[1])
    probes = KI.probes(by_digest)
    meta, rec = KC.split(known)
    for _, _, first, count in set_records(known):         # every set backwards: something to sort
        rec[first:first + count] = rec[first:first + count][::-1].copy()
    unsorted = meta + rec.tobytes()
    half = KC.image({k: sets[k] for k in keys[::2]})
    hit, miss = KI.split(known, probes, NOW)
    cascade = CA.build(hit, miss, NOW, PARAMS)
    return types.SimpleNamespace(
        known=known, probes=probes, unsorted=unsorted, half=half, hit=hit, miss=miss, cascade=cascade,
        lists=KI.image_lists(known, NOW), resp=KI.image_resp(known, PER), sorted=KI.sort(unsorted), union=KI.union(known, half),
        find=KI.find(known, probes, NOW), answers=CA.query(cascade, known))


def test_the_image_has_the_shapes_the_walk_can_go_wrong_at():
    o = operands()
    recs = set_records(o.known)
    hours, ordinal, first, count = (np.asarray(x) for x in zip(*recs))
    kept = np.asarray([FC.kept(int(h), NOW) for h in hours])
    n = int(first[-1] + count[-1])
    assert n == sum(SIZES) and not kept[:EXPIRED].any() and kept[EXPIRED:].all()
    set_of = np.repeat(np.arange(len(recs)), count)
    # some wave holds at least 64 sets
    assert max(len(set(set_of[w:w + 64])) for w in range(0, n, 64)) >= 64
    # the last set that is not kept lies strictly inside a wave and inside a 256-record block of the image, and kept
    # records share both with it: the kept sets' virtual record v is image record v + shift
    s = EXPIRED - 1
    lo, hi = int(first[s]), int(first[s] + count[s] - 1)
    shift = int(first[EXPIRED])
    for width in (64, 256):
        assert lo // width == hi // width and lo % width != 0 and hi % width != width - 1
        assert kept[set_of[lo // width * width:(lo // width + 1) * width]].any()
        assert shift % width != 0
    # the lists' order, per issuer: src − dst changes between two segments inside a wave, and at a segment that crosses
    # a block edge
    ids = [KI.issuer_id(d) for d in sorted(DIGESTS)]         # (an image numbers its issuers in digest order)
    order = sorted((s for s in range(len(recs)) if kept[s]), key=lambda s: (ids[ordinal[s]], hours[s]))
    dst = np.concatenate([[0], np.cumsum(count[order])])
    delta = first[order] - dst[:-1]
    changes = [j for j in range(1, len(order)) if delta[j] != delta[j - 1]]
    assert any(dst[j] % 64 != 0 and dst[j] // 64 == (dst[j + 1] - 1) // 64 for j in changes)
    assert any(dst[j] // 256 != (dst[j + 1] - 1) // 256 for j in changes)
    # P: half of K's kept records and as many strangers
    p_found = int((o.find[0]["records"] > 0).sum())
    assert p_found == len(o.find[0]) // 2 and abs(p_found - int(count[kept].sum()) // 2) <= 1


@pytest.mark.parametrize("chunk", [None, 1, 64, 257])
def test_every_consumer_equals_its_twin(chunk, eng, monkeypatch):
    for name in CHUNKS:
        if chunk is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(chunk))
    o = operands()
    assert eng.known_image_lists(o.known, NOW) == o.lists
    assert eng.known_image_resp(o.known, PER) == o.resp
    assert eng.known_sort(o.unsorted) == o.sorted
    assert eng.known_merge(N.KNOWN_UNION, o.known, o.half) == o.union
    hits, host_hits, _ = eng.known_image_find(o.known, o.probes, NOW)
    assert hits.tobytes() == o.find[0].tobytes() and host_hits.tobytes() == o.find[1].tobytes()
    hit, miss, _ = eng.known_image_split(o.known, o.probes, NOW)
    assert (hit, miss) == (o.hit, o.miss)
    cascade, _ = eng.cascade_build(o.hit, o.miss, NOW, PARAMS)
    assert cascade == o.cascade
    answers, _ = eng.cascade_query(cascade, o.known)
    assert answers.tobytes() == o.answers


def test_a_bad_record_at_the_end_of_the_last_run_is_refused_and_nothing_written(eng, monkeypatch):
    """Padding that is not zero in the last record of the last kept run, at 64 records per run: find, split and the
    cascade build refuse it with the text they have, and none writes any output (the raw-call helpers hold every
    buffer to its fill)."""
    for name in CHUNKS:
        monkeypatch.setenv(name, "64")
    o = operands()
    text = b": a member record's padding octets are not zero"
    bad = damaged_record(o.known, KI._HEADER.unpack_from(o.known, 0)[6] - 1, "pad")
    for device in (False, True):
        assert find_call(eng, bad, o.probes, NOW, device)[0] == N.E_INVAL
        assert eng._lib.ctmr_last_error(eng._h) == b"known image find" + text
        caps = (len(o.known), KI._HEADER.unpack_from(o.known, 0)[6]) if device else len(o.known)
        assert split_call(eng, bad, o.probes, NOW, device, caps, caps)[0] == N.E_INVAL
        assert eng._lib.ctmr_last_error(eng._h) == b"known image split" + text
        n_miss = KI._HEADER.unpack_from(o.miss, 0)[6]
        assert o.miss[-48:] == o.known[-48:]                                  # K's last record is MISS's last
        case = types.SimpleNamespace(revoked=o.hit, known=damaged_record(o.miss, n_miss - 1, "pad"), now=NOW, cascade=o.cascade,
                                     params=(PARAMS.k_first, PARAMS.bpk_first_q8, PARAMS.k_rest, PARAMS.bpk_rest_q8, PARAMS.max_layers,
                                             PARAMS.salt))
        assert cascade_build(eng, case, device)[0] == N.E_INVAL
        assert eng._lib.ctmr_last_error(eng._h) == b"cascade build" + text
