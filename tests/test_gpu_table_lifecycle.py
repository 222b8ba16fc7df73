"""-m gpu: the known-certificate table through remove, expiry, rebuild and compaction, against the plain model of
tests/table_lifecycle.py.  Every comparison is exact equality with the model.

Randomised: for each seed of table_lifecycle.SEEDS a schedule of about 80 steps (map batches over overlapping ranges, point
and bulk inserts / removes / queries, ExpireAt overrides, partial sweeps, exports) on an engine that starts with 1 024
slots, 1 024 cells and 16 pair slots.  After EVERY step: the step's own answer, total and per-issuer counts, the whole
state as one sorted export (byte for byte the model's canonical image), and the host accounting — `occupied` is exactly
the model's device-resident members plus the members removed since the last rebuild.  At the end of a seed the table
must have been rebuilt at the same size (tombstones recovered) and at a larger one, compacted its arena while
tombstones were present, and grown it.

Directed: the re-insert matrix (3 insert paths x 4 remove paths at load 0.70, nothing rebuilt in between), a removed
key three times in one batch (both map variants), churn under max_table_slots, overrides on table keys, and an arena
compaction over tombstones."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401  (loaded first so that libctmr binds to the same HIP runtime)

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import known_image as KI, synth, _native as N  # noqa: E402
from ct_mapreduce_amd.engine import Batch  # noqa: E402
from tests import known_corpus as KC, table_lifecycle as TL  # noqa: E402

NOW = TL.NOW


@pytest.fixture(scope="module")
def corpus():
    cfg = TL.lifecycle_config()
    return TL.Corpus(cfg, synth.issuers(cfg), 9000)


def make_engine(cp, **kw):
    kw.setdefault("table_slots", 1 << 10)
    kw.setdefault("pair_slots", 1 << 4)
    eng = ctmr.Engine(device=0, **kw)
    eng.add_issuers(cp.issuers)
    eng.set_filter(b"", True, NOW)
    eng.set_known_order(N.KNOWN_ORDER_SORTED)
    return eng


def image_of(pairs):
    sets = {}
    for k, mem in pairs:
        sets.setdefault(k, []).append(mem)
    return KC.image(sets)


def check_map(eng, m, batch, cp):
    """One batch on the engine and on the model: status, WasUnknown, the NEW list, n_new."""
    res = eng.map_batch(batch)
    st, keys = TL.entry_keys(batch, cp.issuers, cp.digests)
    new = m.map(keys)
    assert (res.records["status"] == st).all()
    got = (res.records["flags"] & N.FL_WAS_UNKNOWN) != 0
    assert (got == new).all(), (np.nonzero(got != new)[0][:10], got.sum(), new.sum())
    assert (res.new_idx == np.nonzero(new)[0]).all() and res.stats.n_new == int(new.sum())
    return new


def check_step(eng, m, step, cp):
    kind = step["kind"]
    if kind == "map":
        check_map(eng, m, cp.batch(step["first"], step["n"]), cp)
        return
    want = TL.apply_step(m, step)
    if kind in ("set_insert", "set_remove", "set_contains"):
        f = getattr(eng, kind)
        assert [f(k, mem) for k, mem in step["items"]] == want
    elif kind == "known_import":
        assert eng.known_import(step["image"]) == want
    elif kind == "known_remove":
        assert eng.known_remove(step["image"]) == want
    elif kind == "known_query":
        fl, hf, st = eng.known_query(step["image"])
        assert (fl == want[0]).all() and (hf == want[1]).all() and st == want[2]
    elif kind == "expire_at":
        for k, t in step["items"]:
            eng.expire_at(k, t)
    elif kind == "sweep":
        assert eng.expire_sweep(step["now"]) == want


def check_state(eng, m, export=True):
    assert eng.total_count() == m.total()
    assert [int(c) for c in eng.issuer_counts()] == m.issuer_counts()
    if export:
        assert eng.known_export() == m.image()
    ti = eng.table_info()
    assert ti.occupied * 4 <= ti.slots * 3 and ti.arena_used <= ti.arena_cells and ti.occupied >= m.device_members()
    return ti


def check_views(eng, m, now, dead=()):
    keys = m.keys()
    assert sorted(eng.keys(b"serials::*")) == keys
    for k in keys:
        assert eng.set_cardinality(k) == len(m.sets[k]) and eng.exists(k)
        assert eng.set_list(k) == m.members(k)
    for k in dead:
        if k not in m.sets:
            assert eng.set_cardinality(k) == 0 and not eng.exists(k) and eng.set_list(k) == []
    assert eng.known_lists(now) == m.lists(now)


# ---------------------------------------------------------------------------------------------------- randomised
@pytest.mark.parametrize("seed", TL.SEEDS)
def test_random_schedule_against_the_model(corpus, seed):
    cp = corpus
    steps, _ = TL.make_schedule(seed, TL.N_STEPS, cp.issuers, cp.cfg, corpus=cp)
    eng, m = make_engine(cp), TL.Model(cp.digests)
    prev = eng.table_info()
    assert (prev.slots, prev.arena_cells) == (1024, 1024)
    tombs = 0                                         # the model's removed-but-not-rebuilt members
    same = grown = squeezed_over_tombs = 0
    ever_held, now = set(), NOW
    for j, step in enumerate(steps):
        held0, tombs0 = m.device_members(), tombs
        check_step(eng, m, step, cp)
        ti = check_state(eng, m, export=j < 30 or j % 4 == 0 or j == len(steps) - 1)
        if ti.rebuilds > prev.rebuilds:               # a rebuild drops every tombstone; only inserting steps rebuild
            same += ti.slots == prev.slots
            grown += ti.slots > prev.slots
            tombs = 0
        tombs += max(0, held0 - m.device_members())
        assert ti.occupied == m.device_members() + tombs, (j, step["kind"], ti.occupied, m.device_members(), tombs)
        squeezed_over_tombs += ti.arena_compactions > prev.arena_compactions and tombs0 > 0
        prev = ti
        ever_held.update(m.sets)
        if step["kind"] == "sweep":
            now = step["now"]
        if step["kind"] == "export":
            check_views(eng, m, now, sorted(ever_held - set(m.sets))[:20])
    check_views(eng, m, now, sorted(ever_held - set(m.sets))[:20])
    # the coverage condition: a condition on the inputs (the seeds were chosen to meet it), not a tolerance
    assert same >= 1 and grown >= 1, (same, grown)
    assert squeezed_over_tombs >= 1 and prev.arena_growths >= 1, (squeezed_over_tombs, prev.arena_growths)
    eng.close()


# ---------------------------------------------------------------------------------------------------- directed
def entries_batch(cp, idx):
    """The synthetic entries `idx` (any order, repeats allowed) as one batch."""
    src = cp.batch(0, max(idx) + 1)
    b = Batch.from_certs([src.cert(i) for i in idx], [int(src.issuer_idx[i]) for i in idx],
                         [int(src.entry_type[i]) for i in idx])
    b.payload = np.concatenate([b.payload, np.zeros(N.PAYLOAD_PAD, np.uint8)])
    return b


@pytest.mark.parametrize("remove_path", TL.REMOVE_PATHS)
@pytest.mark.parametrize("insert_path", TL.INSERT_PATHS)
def test_reinsert_matrix(corpus, insert_path, remove_path):
    """M (about 10 members) among 717 members in 1 024 slots (load 0.70: chains of several slots), removed by one path and
    re-inserted by another with NO rebuild in between — M, its tombstones and the last batch together stay under the 768
    slots at which the table would be rebuilt — so that a word re-inserted by a point insert or an import lies behind its
    own tombstone, and neighbours lie behind M's.  Then: contains, the export (M once), cardinalities, every neighbour,
    and one batch with M's certificates twice and as many neighbours' as still fit: all known."""
    FILL = 717                                        # the smallest count at load 0.70 of 1 024 slots
    cp = corpus
    eng, m = make_engine(cp), TL.Model(cp.digests)
    check_map(eng, m, cp.batch(0, 600), cp)
    fill = [p for p in image_pairs(KC.make("uniform", cp.digests[:3], (492000, 492001), 60, seed=5).sets)
            if len(p[1]) <= KI.MAX_SERIAL][:FILL - m.device_members()]
    assert eng.known_import(image_of(fill)) == m.import_image(image_of(fill))
    assert m.device_members() == FILL == eng.table_info().occupied
    first = {}
    for i in range(600):                              # the entry that carries each key first
        if cp.keys[i] is not None:
            first.setdefault(cp.keys[i], i)
    by_hour = sorted(first, key=lambda p: (m.natural(p[0]), p))
    if remove_path == "sweep":                        # everything at or before the 10th earliest member's hour
        cut = m.natural(by_hour[9][0])
        victims = [p for p in by_hour if m.natural(p[0]) <= cut]
        assert eng.expire_sweep(cut) == m.sweep(cut) == len(victims)
    elif remove_path == "override":                   # whole sets from the LATE end, made due by an override
        keys = sorted({p[0] for p in by_hour[-8:]})
        victims = [p for p in by_hour if p[0] in keys]
        for k in keys:
            eng.expire_at(k, 1000)
            m.expire_at(k, 1000)
        assert eng.expire_sweep(1000) == m.sweep(1000) == len(victims)
    else:
        victims = by_hour[100:400:30]
        if remove_path == "point":
            assert all(eng.set_remove(*p) and m.remove(*p) for p in victims)
        else:
            assert eng.known_remove(image_of(victims)) == m.remove_image(image_of(victims))
    assert 8 <= len(victims) <= 14 and not any(eng.set_contains(*p) for p in victims)
    check_state(eng, m)
    if insert_path == "point":
        assert all(eng.set_insert(*p) and m.insert(*p) for p in victims)
    elif insert_path == "import":
        st = eng.known_import(image_of(victims))
        assert st == m.import_image(image_of(victims)) and st["inserted"] == len(victims)
    else:
        new = check_map(eng, m, entries_batch(cp, [first[p] for p in victims]), cp)
        assert new.all()
    ti = check_state(eng, m)
    assert ti.rebuilds == 0 and ti.slots == 1024 and ti.occupied == FILL + len(victims)    # tombstones still in place
    assert all(eng.set_contains(*p) for p in victims)
    for k in sorted({p[0] for p in victims}):
        assert eng.set_cardinality(k) == len(m.sets[k]) and eng.set_list(k) == m.members(k)
    fl, hf, st = eng.known_query(m.image())
    assert fl.all() and st["hits"] == st["members"] == m.device_members() == FILL
    room = 768 - (FILL + len(victims)) - 2 * len(victims)       # entries the batch may add before 3/4 is crossed
    near = [first[p] for p in by_hour if p not in victims and m.contains(*p)][:room]
    assert len(near) >= 8
    twice = [first[p] for p in victims] * 2 + near
    new = check_map(eng, m, entries_batch(cp, twice), cp)
    assert not new.any() and eng.table_info().rebuilds == 0
    check_state(eng, m)
    eng.close()


def image_pairs(sets):
    return [(k, mem) for k in sorted(sets) for mem in sets[k]]


@pytest.mark.parametrize("variant", [13, 15], ids=["winc_separate_insert", "fused"])
def test_removed_key_three_times_in_one_batch(corpus, variant):
    """A key removed earlier comes back three times in one batch — twice inside one wave of 64 entries, once in another
    wave: exactly the lowest index is new, under both map variants."""
    cp = corpus
    eng, m = make_engine(cp, map_variant=variant), TL.Model(cp.digests)
    check_map(eng, m, cp.batch(0, 300), cp)
    count = {}
    for k in cp.keys[:600]:
        count[k] = count.get(k, 0) + 1
    e = next(i for i in range(50, 300) if cp.keys[i] is not None and count[cp.keys[i]] == 1)
    assert eng.set_remove(*cp.keys[e]) and m.remove(*cp.keys[e])
    idx = list(range(300, 500))
    for at in (5, 40, 130):                           # waves 0, 0 and 2
        idx[at] = e
    new = check_map(eng, m, entries_batch(cp, idx), cp)
    assert new[5] and not new[40] and not new[130]
    check_state(eng, m)
    assert eng.set_cardinality(cp.keys[e][0]) == len(m.sets[cp.keys[e][0]])
    eng.close()


def test_churn_under_a_cap_keeps_the_permanent_members(corpus):
    """max_table_slots = 1 024: 40 rounds of 500 members that come and go (bulk remove; on odd rounds 50 of them by point
    remove) around 100 permanent ones.  Every round's tombstones are recovered by a same-size rebuild: never
    CTMR_E_FULL, never more slots, the permanent members present after every round.  Then the same with the churn
    coming from map batches and a partial sweep: a cut among the mapped sets' own hours takes two thirds of them, so
    the survivors share chains with fresh tombstones round after round."""
    cp = corpus
    eng, m = make_engine(cp, max_table_slots=1 << 10), TL.Model(cp.digests)
    far = KC.make("uniform", cp.digests[:2], (600000,), 50, seed=9)           # expDates far beyond every sweep below
    perm = far.image
    assert eng.known_import(perm) == m.import_image(perm) and m.device_members() == 100
    rebuilds = 0
    for rnd in range(40):
        c = KC.make("uniform", cp.digests[2:4], (492100 + rnd,), 250, seed=100 + rnd)
        pairs = image_pairs(c.sets)
        st = eng.known_import(c.image)                # (CTMR_E_FULL would raise)
        assert st == m.import_image(c.image) and st["inserted"] == 500
        if rnd % 2:
            assert all(eng.set_remove(*p) and m.remove(*p) for p in pairs[100:150])
            pairs = pairs[:100] + pairs[150:]
        assert eng.known_remove(image_of(pairs)) == m.remove_image(image_of(pairs))
        ti = check_state(eng, m, export=rnd % 8 == 0)
        assert ti.slots == 1024 and ti.rebuilds >= rebuilds
        rebuilds = ti.rebuilds
        fl, _, _ = eng.known_query(perm)
        assert fl.all() and eng.total_count() == 100
    assert rebuilds >= 20                             # 600 claimed slots a round in a table that holds 768
    survived = 0
    for rnd in range(16):
        check_map(eng, m, cp.batch(250 * rnd, 250), cp)
        hours = sorted(m.natural(k) for k in m.sets if m.natural(k) < 600000 * 3600)
        now = hours[2 * len(hours) // 3]              # some mapped sets die, some survive; the permanent ones are far off
        before = m.total()
        assert eng.expire_sweep(now) == m.sweep(now) and 100 < m.total() < before
        survived += m.total() - 100
        ti = check_state(eng, m, export=rnd % 4 == 0)
        assert ti.slots == 1024 and eng.known_query(perm)[0].all()
    assert eng.table_info().rebuilds > rebuilds and survived > 16 * 30
    assert eng.known_export() == m.image()
    check_views(eng, m, NOW)
    eng.close()


def test_overrides_on_table_keys(corpus):
    """ExpireAt on keys that live in the device table: the sweep goes key by key (one k_sweep launch per pair)."""
    cp = corpus
    eng, m = make_engine(cp), TL.Model(cp.digests)
    h1, h2 = 495000, 495100
    k1, k2, k0 = (KI.set_key(h, cp.digests[1]) for h in (h1, h2, -7))
    long1, long2 = b"\x11" * 41, b"\x22" * 64
    pairs = [(k1, bytes([1, j])) for j in range(30)] + [(k2, bytes([2, j]) * 9) for j in range(30)] + \
            [(k1, long1), (k2, long2)] + [(k0, bytes([j])) for j in range(5)]

    def insert(key, member):
        got = eng.set_insert(key, member)
        assert got == m.insert(key, member)
        return got

    def expire_at(key, t):
        eng.expire_at(key, t)
        m.expire_at(key, t)

    def sweep(now):
        got = eng.expire_sweep(now)
        assert got == m.sweep(now)
        return got

    assert all(insert(*p) for p in pairs)
    assert eng.total_count() == 67
    # no override anywhere: one sweep over every key, expDates before the epoch included
    assert sweep(-8 * 3600) == 0 and sweep(-7 * 3600) == 5
    later, earlier = (h2 + 50) * 3600, (h2 - 500) * 3600
    expire_at(k1, later)
    assert sweep(h1 * 3600) == 0 and eng.set_cardinality(k1) == 31                          # nothing of k1 goes
    expire_at(k2, earlier)
    assert sweep(earlier) == 31 and not eng.exists(k2)                                      # its host member included
    check_state(eng, m)
    assert sweep(earlier) == 0
    assert insert(k2, b"\x05") and insert(k2, long2)
    assert sweep(h2 * 3600 - 1) == 0 and eng.set_cardinality(k2) == 2                       # natural again
    assert sweep(h2 * 3600) == 2 and eng.set_cardinality(k1) == 31                          # k1: spared past its hour
    assert sweep(later - 1) == 0 and sweep(later) == 31
    assert eng.total_count() == 0 == m.total() and eng.keys(b"serials::*") == []
    check_state(eng, m)
    eng.close()


def test_arena_compaction_over_tombstones(corpus):
    """The arrangement of test_the_arena_squeezes_out_the_cells_of_known_certificates with a third of the members removed
    (half of them in bulk, half by a sweep) before the round that compacts: survivors are known, removed members are
    new exactly once, and the arena holds the live cells plus the batch."""
    cp = corpus
    eng, m = make_engine(cp, table_slots=1 << 13, pair_slots=1 << 14), TL.Model(cp.digests)
    assert eng.table_info().arena_cells == 4096
    b = cp.batch(0, 1500)
    check_map(eng, m, b, cp)
    assert not check_map(eng, m, b, cp).any()         # 3 000 cells used, half of them garbage
    held = sorted({p for p in cp.keys[:1500] if p is not None}, key=lambda p: (m.natural(p[0]), p))
    cut = m.natural(held[len(held) // 6][0])
    swept = eng.expire_sweep(cut)
    assert swept == m.sweep(cut) > 150
    bulk = [p for p in held if m.contains(*p)][::5]
    assert eng.known_remove(image_of(bulk)) == m.remove_image(image_of(bulk))
    live = m.device_members()
    assert live <= len(held) * 0.75 and eng.table_info().arena_compactions == 0
    idx = list(range(0, 1000)) + list(range(5000, 5500))      # survivors, removed members (some twice), strangers
    new = check_map(eng, m, entries_batch(cp, idx), cp)
    assert 200 < int(new[:1000].sum()) < 500 and new[1000:].sum() > 300
    ti = check_state(eng, m)
    assert ti.arena_compactions == 1 and ti.arena_growths == 0 and ti.rebuilds == 0
    assert ti.arena_used == live + 1500 and ti.occupied == live + swept + len(bulk) + int(new.sum())
    check_views(eng, m, NOW)
    assert not check_map(eng, m, entries_batch(cp, idx), cp).any()
    eng.close()
