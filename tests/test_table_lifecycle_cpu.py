"""No GPU: the model and the schedule builder of tests/table_lifecycle.py held to their properties, so that
tests/test_gpu_table_lifecycle.py cannot pass by being vacuous.  The coverage is found by replaying each schedule on a
fresh model (table_lifecycle.coverage), not read from the builder."""
import pytest

from ct_mapreduce_amd import known_image as KI, synth
from tests import known_corpus as KC, table_lifecycle as TL


@pytest.fixture(scope="module")
def schedules():
    cfg = TL.lifecycle_config()
    issuers, corpus, out = synth.issuers(cfg), None, {}
    for seed in TL.SEEDS:
        steps, corpus = TL.make_schedule(seed, TL.N_STEPS, issuers, cfg, corpus=corpus)
        out[seed] = (steps, TL.coverage(steps, corpus))
    return out, corpus


@pytest.mark.parametrize("seed", TL.SEEDS)
def test_every_schedule_has_every_step_kind_and_every_reinsert_pair(schedules, seed):
    steps, cov = schedules[0][seed]
    assert TL.N_STEPS <= len(steps) <= TL.N_STEPS + 10
    assert cov["kinds"] == set(TL.STEP_KINDS)
    assert cov["reinserts"] == {(i, r) for i in TL.INSERT_PATHS for r in TL.REMOVE_PATHS}
    assert cov["partial"] >= 1 and cov["early"] >= 1 and cov["late"] >= 1
    assert 50 <= min(cov["sizes"]["map"]) and max(cov["sizes"]["map"]) <= 1500
    assert 10 <= min(cov["sizes"]["image"]) and max(cov["sizes"]["image"]) <= 2000
    long_members = sum(len(m) > KI.MAX_SERIAL for s in steps if s["kind"] == "set_insert" for _, m in s["items"])
    before_epoch = sum(KI.parse_key(k)[0] < 0 for s in steps if s["kind"] == "set_insert" for k, _ in s["items"])
    assert long_members >= 3 and before_epoch >= 4


def test_schedules_are_reproducible(schedules):
    cfg = TL.lifecycle_config()
    again, _ = TL.make_schedule(TL.SEEDS[0], TL.N_STEPS, synth.issuers(cfg), cfg, corpus=schedules[1])
    assert again == schedules[0][TL.SEEDS[0]][0]


def test_model_sweep_follows_the_engine_rules():
    d = [bytes([k]) * 32 for k in (1, 2)]
    m = TL.Model(d[:1])
    k1, k2, kold = KI.set_key(1000, d[0]), KI.set_key(2000, d[0]), KI.set_key(-5, d[0])
    other = KI.set_key(1000, d[1])                               # an issuer that is not registered: never due by itself
    for k in (k1, k2, kold, other):
        assert m.insert(k, b"\x01") and m.insert(k, b"\x02" * 50) and not m.insert(k, b"\x01")
    assert m.total() == 6 and m.issuer_counts() == [6] and m.device_members() == 3
    assert m.lists(0) == [(KI.issuer_id(d[0]), (KI.line(b"\x01") + KI.line(b"\x02" * 50)) * 2),
                          (KI.issuer_id(d[1]), KI.line(b"\x01") + KI.line(b"\x02" * 50))]        # the expired set is not listed
    assert m.sweep(-6 * 3600) == 0 and m.sweep(-5 * 3600) == 2 and m.keys() == sorted([k1, k2, other])
    m.expire_at(k1, 5000 * 3600)                                 # later than natural: spared at its hour
    m.expire_at(k2, 1500 * 3600)                                 # earlier: taken before its hour
    m.expire_at(other, 1200 * 3600)
    assert m.sweep(1000 * 3600) == 0 and len(m.expiry) == 3
    assert m.sweep(1200 * 3600) == 2 and other not in m.sets and other not in m.expiry
    assert m.sweep(1500 * 3600) == 2 and m.keys() == [k1] and set(m.expiry) == {k1}
    assert m.sweep(1500 * 3600) == 0
    assert m.insert(k2, b"\x03") and m.sweep(1999 * 3600) == 0 and m.sweep(2000 * 3600) == 1   # the override is gone
    assert m.sweep(5000 * 3600) == 2 and not m.sets and not m.expiry


def test_model_image_calls_agree_with_known_image():
    d = [bytes([k]) * 32 for k in (3, 4, 5)]
    a = KC.make("uniform", d, (500000, 500001), (40, 7), seed=1).sets
    b = KC.make("uniform", d[:2], (500001, 500002), (25, 60), seed=2).sets
    k = sorted(set(a) & set(b))[0]
    a[k] = a[k] + [b"\x07" * 45]                                 # host-side members on both sides
    b[k] = b[k] + [b"\x07" * 45, b"\x09" * 41]
    for k in list(b)[:3]:
        if k in a:
            b[k] = sorted(set(b[k]) | set(a[k][::2]))
    m = TL.Model(d)
    st = m.import_image(KC.image(a))
    assert st["inserted"] == st["taken"] == KI.parse(KC.image(a)).n_members and st["host_inserted"] == 1
    assert m.image() == KI.sort(KC.image(a)) and m.sorted_sets() == {k: sorted(v) for k, v in a.items()}
    img_b = KC.image(b)
    fl, hf, st = m.query_image(img_b)
    want = KI.query(img_b, a)
    assert (fl == want[0]).all() and (hf == want[1]).all() and st["hits"] == int(want[0].sum()) > 0
    assert st["host_hits"] == int(want[1].sum()) == 1 and 0 in fl
    st = m.remove_image(img_b)
    assert m.sorted_sets() == KI.subtract(a, img_b) and st["hits"] == int(want[0].sum()) and st["host_hits"] == 1
    assert m.remove_image(img_b)["hits"] == 0
    st = m.import_image(img_b)
    assert st["known"] == 0 and st["host_inserted"] == 2
    union = {k: sorted(set(KI.subtract(a, img_b).get(k, [])) | set(b.get(k, []))) for k in set(a) | set(b)}
    assert m.image() == KI.sort(KI.build(union))


def test_model_map_flags_first_occurrence_only():
    m = TL.Model([b"\x01" * 32])
    k = KI.set_key(500000, b"\x01" * 32)
    keys = [(k, b"a"), None, (k, b"b"), (k, b"a"), (k, b"b"), (k, b"c")]
    assert m.map(keys).tolist() == [True, False, True, False, False, True]
    assert m.remove(k, b"a") and m.map(keys).tolist() == [True, False, False, False, False, False]
