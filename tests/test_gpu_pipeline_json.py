"""-m gpu: the asynchronous JSON form of the ingestion pipeline (ctmr_submit_entries_json / ctmr_wait_entries_json,
include/ctmr.h).  get-entries bodies submitted as text without waiting coalesce into super-batches; every
body is judged alone, and each ticket answers as one synchronous map_entries call over its good bodies would, in
submission order.  The corpus is synth.host_entries written as bodies with get_entries.write; the yardstick is a second
engine that runs map_entries once per submit."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import get_entries as ge, synth, _native as N  # noqa: E402
from ct_mapreduce_amd.engine import RawEntries, RECORD_DTYPE  # noqa: E402

NOW = synth.BASE_TIME
FILT = b"Synth Issuer 0,Synth Issuer 1"
NONE = 2**64 - 1
EMPTY = b'{"entries":[]}'


def make(issuers=None, **kw):
    kw.setdefault("table_slots", 1 << 18)
    kw.setdefault("pair_slots", 1 << 12)
    e = ctmr.Engine(device=0, **kw)
    if issuers:
        e.add_issuers(issuers)
    e.set_filter(FILT, False, NOW)
    return e


def pairs_of(raw):
    return [(raw.leaf_input(i), raw.extra_data(i)) for i in range(raw.n)]


def same(got, want, where=""):
    """a ticket's answer against the synchronous call's"""
    assert got.records.tobytes() == want.records.tobytes(), where
    assert (got.new_idx == want.new_idx).all() and (got.timestamp == want.timestamp).all(), where
    for f in ("n", "n_new", "n_dup", "n_host_set", "payload_bytes"):
        assert getattr(got.stats, f) == getattr(want.stats, f), (where, f)
    assert list(got.stats.by_status) == list(want.stats.by_status), where
    for f in ("n", "n_x509", "n_precert", "n_decode_error", "n_no_chain", "blob_bytes"):
        assert getattr(got.decode, f) == getattr(want.decode, f), (where, f)


def same_sets(eng, ref):
    assert (eng.issuer_counts() == ref.issuer_counts()).all()
    assert sorted(eng.keys(b"serials::*")) == sorted(ref.keys(b"serials::*"))
    assert eng.total_count() == ref.total_count()


@pytest.mark.parametrize("per", [1, 7, 1001])
@pytest.mark.parametrize("submits", [1, 3, 9])
def test_tickets_answer_like_synchronous_calls(per, submits):
    """Two bodies a submit (one in every third); the generator's duplicates span bodies and submits, so WasUnknown
    depends on the order."""
    cfg = synth.config(seed=97, n_issuers=24, zipf=1, dup_permille=20, ca_permille=10, expired_permille=10)
    eng, ref = make(), make()
    groups, at = [], 0
    for k in range(submits):
        nb = 1 if k % 3 == 2 else 2
        raw = synth.host_entries(cfg, at, per * nb)
        at += per * nb
        groups.append((ge.write(pairs_of(raw), per), raw))
    tickets = [eng.submit_entries_json(bodies) for bodies, _ in groups]
    for k, ((bodies, raw), t) in enumerate(zip(groups, tickets)):
        res = eng.wait_entries_json(t)
        same(res, ref.map_entries(raw), k)
        assert res.bad == [None] * len(bodies)
        assert (res.resp_first == np.arange(len(bodies) + 1) * per).all()
    same_sets(eng, ref)
    eng.close()
    ref.close()


def test_one_bad_body_among_eight_submits_costs_no_other_ticket_anything():
    cfg = synth.config(seed=98, n_issuers=8, zipf=1, dup_permille=20)
    raws = [synth.host_entries(cfg, 40 * k, 40) for k in range(8)]
    bodies = [ge.write_one(pairs_of(r)) for r in raws]
    bad5 = bodies[5].replace(b"extra_data", b"extra_datA", 1)
    eng, ref = make(), make()
    tickets = [eng.submit_entries_json([bad5 if k == 5 else bodies[k]]) for k in range(8)]
    assert len({t >> 20 for t in tickets}) == 1                 # one super-batch
    got = {}
    for k in (7, 5, 0, 1, 2, 3, 4, 6):
        res = got[k] = eng.wait_entries_json(tickets[k])
        if k == 5:
            assert len(res.bad) == 1 and 0 <= res.bad[0] < len(bad5)
            assert len(res.records) == len(res.new_idx) == len(res.timestamp) == 0 and res.stats.n == 0
            assert (res.resp_first == [0, 0]).all()
        else:
            assert res.bad == [None]
    # the seven others, collected above out of order, and the sets: a run without the bad body
    eng2 = make()
    t2 = [eng2.submit_entries_json([bodies[k]]) for k in range(8) if k != 5]
    want = [ref.map_entries(raws[k]) for k in range(8) if k != 5]
    for k, t, w in zip([k for k in range(8) if k != 5], t2, want):
        same(eng2.wait_entries_json(t), w, k)
        same(got[k], w, k)
    same_sets(eng2, ref)
    same_sets(eng, ref)
    # three bodies in one ticket, the middle one bad, in front of text that is not part of the submit
    text = b"#" * 37 + bodies[0] + bad5 + bodies[1]
    rb = np.asarray([37, 37 + len(bodies[0]), 37 + len(bodies[0]) + len(bad5), len(text)], np.uint64)
    buf = np.frombuffer(text, np.uint8).copy()
    res = eng.wait_entries_json(eng.submit_entries_json((buf, rb)))
    assert res.bad[0] is None and res.bad[2] is None and int(rb[1]) <= res.bad[1] < int(rb[2])
    assert (res.resp_first == [0, 40, 40, 80]).all() and res.stats.n == 80 and res.stats.n_new == 0
    assert (res.timestamp == np.concatenate([want[0].timestamp, want[1].timestamp])).all()
    for e in (eng, eng2, ref):
        e.close()


def test_json_raw_and_packed_submits_interleaved():
    """Every change of form closes the open super-batch and the order of the stream is kept across forms."""
    cfg = synth.config(seed=99, n_issuers=16, zipf=1, dup_permille=300)
    issuers = synth.issuers(cfg)
    eng, ref = make(issuers), make(issuers)
    size, pending, keep, seqs = 300, [], [], []

    def collect(form, x, t):
        if form == "packed":
            got, want = eng.wait(t, x.n), ref.map_batch(x)
            assert got.records.tobytes() == want.records.tobytes() and (got.new_idx == want.new_idx).all()
        elif form == "raw":
            same(eng.wait_entries(t, x.n), ref.map_entries(x), form)
        else:
            same(eng.wait_entries_json(t), ref.map_entries(x), form)

    for k in range(12):
        form = ("json", "raw", "json", "packed")[k % 4]
        if form == "packed":
            x = synth.host_batch(cfg, k * size, size)
            a = (np.concatenate([x.payload, np.zeros(32, np.uint8)]), x.offsets.astype(np.uint64), x.issuer_idx.astype(np.uint32),
                 x.entry_type.astype(np.uint8))
            t = eng.submit_batch(a[0], a[1], a[2], a[3], x.n)
        elif form == "raw":
            x = synth.host_entries(cfg, k * size, size)
            a = (np.concatenate([x.blob, np.zeros(32, np.uint8)]), np.ascontiguousarray(x.bounds, np.uint64))
            t = eng.submit_entries(a[0], a[1], x.n)
        else:
            x = synth.host_entries(cfg, k * size, size)
            a = None
            t = eng.submit_entries_json(ge.write(pairs_of(x), 100))
        keep.append(a)
        seqs.append(t >> 20)
        pending.append((form, x, t))
        if len(pending) == 3:          # at most four super-batches may be unfinished or uncollected
            collect(*pending.pop(0))
    while pending:
        collect(*pending.pop(0))
    assert len(set(seqs)) == 12         # a super-batch each: the forms closed each other's
    same_sets(eng, ref)
    eng.close()
    ref.close()


def test_the_size_query_double_collection_and_the_calls_without_a_capacity():
    cfg = synth.config(seed=100, n_issuers=4)
    raw = synth.host_entries(cfg, 0, 50)
    eng, ref = make(), make()
    t = eng.submit_entries_json(ge.write(pairs_of(raw), 20))
    lib, h = eng._lib, eng._h
    rec = np.zeros(50, RECORD_DTYPE)
    st = N.BatchStats()
    assert lib.ctmr_wait(h, t, rec.ctypes.data, None, C.byref(st)) == N.E_INVAL          # no capacity argument: refused,
    assert lib.ctmr_wait_entries(h, t, rec.ctypes.data, None, None, None, C.byref(st)) == N.E_INVAL
    assert not rec.tobytes().strip(b"\0")
    info = N.EntriesJsonInfo()
    for cap in (0, 49):                                                                   # … and still collectable
        rc = lib.ctmr_wait_entries_json(h, t, cap, rec.ctypes.data, None, None, None, None, C.byref(info), None, None)
        assert rc == N.E_RANGE and (info.entries, info.responses, info.bad_response) == (50, 3, NONE)
        assert info.blob_bytes == int(raw.bounds[-1]) and not rec.tobytes().strip(b"\0")
    same(eng.wait_entries_json(t), ref.map_entries(raw))
    with pytest.raises(ctmr.CtmrError) as ei:
        eng.wait_entries_json(t)
    assert ei.value.code == N.E_NOTFOUND
    rc = lib.ctmr_wait_entries_json(h, t, 50, None, None, None, None, None, C.byref(info), None, None)
    assert rc == N.E_NOTFOUND
    # a raw ticket is not for ctmr_wait_entries_json, and stays collectable too
    a = (np.concatenate([raw.blob, np.zeros(32, np.uint8)]), np.ascontiguousarray(raw.bounds, np.uint64))
    t = eng.submit_entries(a[0], a[1], raw.n)
    assert lib.ctmr_wait_entries_json(h, t, 50, None, None, None, None, None, C.byref(info), None, None) == N.E_INVAL
    assert eng.wait_entries(t, raw.n).stats.n_new == 0
    # all outputs NULL
    t = eng.submit_entries_json([EMPTY])
    assert lib.ctmr_wait_entries_json(h, t, 0, None, None, None, None, None, None, None, None) == 0
    eng.close()
    ref.close()


def test_text_in_pinned_and_in_pageable_memory():
    cfg = synth.config(seed=101, n_issuers=8, dup_permille=100)
    eng, ref = make(), make()
    tickets, raws, keep = [], [], []
    for k in range(6):
        raw = synth.host_entries(cfg, 200 * k, 200)
        text, rb = ge.join(ge.write(pairs_of(raw), 64, ge.STYLES[k % 4]))
        if k % 2 == 0:
            buf = eng.pinned_array(len(text) + 5)
            buf[5:] = np.frombuffer(text, np.uint8)
            rb = rb + np.uint64(5)
        else:
            buf = np.frombuffer(text, np.uint8).copy()
        keep.append(buf)
        raws.append(raw)
        tickets.append(eng.submit_entries_json((buf, rb)))
    for raw, t in zip(raws, tickets):
        same(eng.wait_entries_json(t), ref.map_entries(raw))
    same_sets(eng, ref)
    eng.close()
    ref.close()


def test_four_threads_submit_and_wait():
    cfg = synth.config(seed=102, n_issuers=16, dup_permille=0)
    eng = make()
    per, rounds, T = 101, 12, 4
    news, errors = [0] * T, []
    texts = [[ge.write(pairs_of(synth.host_entries(cfg, (t * rounds + r) * per, per)), 50) for r in range(rounds)] for t in range(T)]

    def worker(t):
        try:
            for r in range(rounds):
                res = eng.wait_entries_json(eng.submit_entries_json(texts[t][r]))
                assert res.stats.n == per and res.bad == [None] * 3
                news[t] += res.stats.n_new
        except Exception as ex:                          # noqa: BLE001
            errors.append(ex)
    ths = [threading.Thread(target=worker, args=(t,), daemon=True) for t in range(T)]
    for th in ths:
        th.start()
    for th in ths:
        th.join(60)
    assert not any(th.is_alive() for th in ths), "a ticket never completed"
    assert not errors, errors
    ref = make()
    want = ref.map_entries(synth.host_entries(cfg, 0, per * rounds * T))
    assert sum(news) == want.stats.n_new == eng.total_count()    # disjoint keys: the interleaving does not matter
    assert sorted(eng.keys(b"serials::*")) == sorted(ref.keys(b"serials::*"))
    eng.close()
    ref.close()


def test_super_batches_close_by_body_count():
    eng = make()
    buf = np.frombuffer(EMPTY, np.uint8).copy()
    rb = np.asarray([0, len(EMPTY)], np.uint64)
    tickets = [eng.submit_entries_json((buf, rb)) for _ in range(4096 + 200)]
    seq = [t >> 20 for t in tickets]
    assert len(set(seq[:4096])) == 1 and seq[4096] != seq[4095] and len(set(seq[4096:])) == 1
    for t in tickets:
        res = eng.wait_entries_json(t)
        assert res.stats.n == 0 and len(res.records) == 0 and res.bad == [None] and (res.resp_first == [0, 0]).all()
    assert eng.total_count() == 0
    eng.close()


def test_autoregistration_off_reports_the_pending_issuers():
    cfg = synth.config(seed=95, n_issuers=5)
    raw = synth.host_entries(cfg, 0, 500)
    bodies = ge.write(pairs_of(raw), 200)
    eng = ctmr.Engine(device=0, table_slots=1 << 14, pair_slots=1 << 12)
    eng.set_filter(b"", True, NOW)
    eng.set_issuer_autoregister(False)
    t = eng.submit_entries_json(bodies)
    with pytest.raises(ctmr.CtmrError) as ei:
        eng.wait_entries_json(t)
    assert ei.value.code == N.E_NOTFOUND
    pend = eng.pending_issuers()
    assert sorted(pend) == sorted(set(synth.issuers(cfg)[int(i)] for i in synth.host_batch(cfg, 0, 500).issuer_idx))
    eng.add_issuers(sorted(pend))
    res = eng.wait_entries_json(eng.submit_entries_json(bodies))
    ref = ctmr.Engine(device=0, table_slots=1 << 14, pair_slots=1 << 12)
    ref.set_filter(b"", True, NOW)
    ref.add_issuers(sorted(pend))
    same(res, ref.map_entries(raw))
    eng.close()
    ref.close()
