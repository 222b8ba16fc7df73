"""-m gpu: a super-batch of the ingestion pipeline that FAILS, in each of its four forms (packed, raw, JSON, PEM; include/ctmr.h,
DESIGN.md §21-23).  The failure is the ordinary refusal of tests/test_gpu_errors.py: 3 000 distinct certificates do not fit a
table capped at 1 024 slots, CTMR_E_FULL before anything is applied.  Every ticket of the super-batch answers with the code
and the message of the synchronous call, the text forms' info names the ticket's bodies and nothing else, a ticket is
collected by that answer, the slot is free again behind the last one and the table is what it was."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import get_entries as ge, pem_text as pt, synth, _native as N  # noqa: E402
from ct_mapreduce_amd.engine import RECORD_DTYPE  # noqa: E402

NOW = synth.BASE_TIME
NONE = 2**64 - 1
FORMS = ["packed", "raw", "json", "pem"]
PER = 250          # entries a body, certificates a file: four bodies a ticket


def make(issuers):
    e = ctmr.Engine(device=0, table_slots=1 << 10, pair_slots=1 << 10, max_table_slots=1 << 10)
    e.add_issuers(issuers)
    e.set_filter(b"", True, NOW)
    return e


def pairs_of(raw):
    return [(raw.leaf_input(i), raw.extra_data(i)) for i in range(raw.n)]


def items(form, cfg, first, n):
    """certificates first … first + n of the stream in the form's own shape: what submit() and sync() take"""
    if form == "packed":
        b = synth.host_batch(cfg, first, n)
        return (np.concatenate([b.payload, np.zeros(32, np.uint8)]), b.offsets.astype(np.uint64), b.issuer_idx.astype(np.uint32),
                b.entry_type.astype(np.uint8), b)
    if form == "raw":
        return synth.host_entries(cfg, first, n)
    if form == "json":
        return ge.write(pairs_of(synth.host_entries(cfg, first, n)), PER)
    b = synth.host_batch(cfg, first, n)
    cuts = list(range(0, n, PER)) + [n]
    return ([pt.write([b.cert(i) for i in range(lo, hi)]) for lo, hi in zip(cuts[:-1], cuts[1:])], [int(b.issuer_idx[lo]) for lo in cuts[:-1]])


def bodies(form, x):
    return len(x) if form == "json" else len(x[0]) if form == "pem" else 0


def submit(eng, form, x):
    if form == "packed":
        return eng.submit_batch(x[0], x[1], x[2], x[3], x[4].n)
    if form == "raw":
        return eng.submit_entries(x.blob, np.ascontiguousarray(x.bounds, np.uint64), x.n)
    return eng.submit_entries_json(x) if form == "json" else eng.submit_pem(*x)


def sync(eng, form, x):
    if form == "packed":
        return eng.map_batch(x[4])
    if form == "raw":
        return eng.map_entries(x)
    return eng.map_entries_json(x) if form == "json" else eng.map_pem(*x)


def wait_c(eng, form, t, nbody):
    """the C entry point of the form, the text forms as the size query (cap = 0) → (code, info or None)"""
    lib, h = eng._lib, eng._h
    rec, new, ts = np.zeros(1000, RECORD_DTYPE), np.zeros(1000, np.uint64), np.zeros(1000, np.uint64)
    first, bad = np.zeros(nbody + 1, np.uint64), np.zeros(max(nbody, 1), np.uint64)
    st, ds = N.BatchStats(), N.DecodeStats()
    if form == "packed":
        return lib.ctmr_wait(h, t, rec.ctypes.data, new.ctypes.data, C.byref(st)), None
    if form == "raw":
        return lib.ctmr_wait_entries(h, t, rec.ctypes.data, new.ctypes.data, ts.ctypes.data, C.byref(ds), C.byref(st)), None
    if form == "json":
        info = N.EntriesJsonInfo()
        info.entries = info.bad_response = info.bad_offset = 77       # (overwritten, or the assertions below fail)
        return lib.ctmr_wait_entries_json(h, t, 0, None, None, None, first.ctypes.data, bad.ctypes.data, C.byref(info), C.byref(ds),
                                          C.byref(st)), info
    info = N.PemDecodeInfo()
    info.certificates = info.bad_file = info.bad_offset = 77
    return lib.ctmr_wait_pem(h, t, 0, None, None, first.ctypes.data, bad.ctypes.data, C.byref(info), C.byref(st)), info


def last_error(eng):
    return eng._lib.ctmr_last_error(eng._h)


def code(fn):
    with pytest.raises(ctmr.CtmrError) as ei:
        fn()
    return ei.value.code


@pytest.mark.parametrize("form", FORMS)
def test_every_ticket_of_a_failed_super_batch_answers_with_its_failure(form):
    cfg = synth.config(seed=1, n_issuers=2)
    issuers = synth.issuers(cfg)
    eng, ref = make(issuers), make(issuers)
    small = synth.host_batch(cfg, 0, 300)
    assert eng.map_batch(small).stats.n_new == ref.map_batch(small).stats.n_new == eng.total_count() > 0
    total = eng.total_count()
    # the synchronous call over the same 3 000: its code and its message
    assert code(lambda: sync(ref, form, items(form, cfg, 300, 3000))) == N.E_FULL
    message = last_error(ref)
    assert b"3000 incoming" in message
    # three tickets of 1 000 in one super-batch
    parts = [items(form, cfg, 300 + 1000 * k, 1000) for k in range(3)]
    tickets = [submit(eng, form, x) for x in parts]
    assert len({t >> 20 for t in tickets}) == 1
    for x, t in zip(parts, tickets):
        nbody = bodies(form, x)
        rc, info = wait_c(eng, form, t, nbody)
        assert rc == N.E_FULL and last_error(eng) == message           # (not E_RANGE: the failure wins over the size query)
        if form == "json":
            assert (info.responses, info.entries, info.bad_response, info.bad_offset) == (nbody, 0, NONE, NONE) and nbody == 4
            assert (info.text_bytes, info.blob_bytes) == (0, 0)
        if form == "pem":
            assert (info.files, info.certificates, info.bad_file, info.bad_offset) == (nbody, 0, NONE, NONE) and nbody == 4
            assert (info.text_bytes, info.payload_bytes, info.regular, info.irregular) == (0, 0, 0, 0)
        assert wait_c(eng, form, t, nbody)[0] == N.E_NOTFOUND          # collected by its failure
    assert eng.total_count() == total                                   # nothing of the failed super-batch is in the table
    # the slot is free again: four super-batches more, all open or uncollected at once, are all the pipeline holds
    good = [items(form, cfg, 5000 + 5 * k, 5) for k in range(4)]
    tickets = []
    for x in good:
        tickets.append(submit(eng, form, x))
        eng.flush()
    assert len({t >> 20 for t in tickets}) == 4
    for x, t in zip(good, tickets):
        res = {"packed": lambda: eng.wait(t, 5), "raw": lambda: eng.wait_entries(t, 5), "json": lambda: eng.wait_entries_json(t),
               "pem": lambda: eng.wait_pem(t)}[form]()
        want = sync(ref, form, x)
        assert res.records.tobytes() == want.records.tobytes() and (res.new_idx == want.new_idx).all() and res.stats.n == 5
    assert eng.total_count() == ref.total_count() > total
    eng.close()
    ref.close()


@pytest.mark.parametrize("form", ["json", "pem"])
def test_the_text_waits_raise_the_failure_once(form):
    cfg = synth.config(seed=1, n_issuers=2)
    eng = make(synth.issuers(cfg))
    wait = eng.wait_entries_json if form == "json" else eng.wait_pem
    tickets = [submit(eng, form, items(form, cfg, 300 + 1000 * k, 1000)) for k in range(3)]
    assert len({t >> 20 for t in tickets}) == 1
    for t in tickets:
        assert code(lambda: wait(t)) == N.E_FULL
        assert code(lambda: wait(t)) == N.E_NOTFOUND
    assert eng.total_count() == 0
    t = submit(eng, form, items(form, cfg, 0, 5))                       # … and the engine still works
    res = wait(t)
    assert res.stats.n == 5 and 0 < res.stats.n_new == eng.total_count()
    eng.close()
