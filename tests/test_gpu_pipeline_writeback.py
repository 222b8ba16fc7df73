"""-m gpu: write-back for the tickets of the ingestion pipeline (ctmr_set_pipeline_writeback / ctmr_ticket_writeback,
include/ctmr.h; csrc/engine/pipeline_writeback.inc, csrc/kernels/writeback.h).  What FilesystemDatabase.Store
does for a certificate that WasUnknown — its PEM block, and the first sightings IssuerMetadata.Accumulate would make — comes
back per ticket, for all four submit forms.  The oracle sees ONE stream: a ticket's PEM blocks are the oracle's encode of
exactly the entries in the new_idx its wait returns, and the items over all tickets are the first sightings of the stream,
each reported once.  ct_mapreduce_amd/writeback.py is the model of the slicing."""
import base64
import ctypes as C
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import get_entries as ge, pem_text as pt, synth, writeback, _native as N  # noqa: E402
from ct_mapreduce_amd.engine import Batch  # noqa: E402
from ct_mapreduce_amd.host_writeback import HostWriter  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import der as D  # noqa: E402
from tests.gpu_common import run_oracle  # noqa: E402
from tests.meta_corpus import dp, dp_ext, expected_first_sightings, got_first_sightings, uri  # noqa: E402

NOW = synth.BASE_TIME
NO_ISSUER = 0xFFFFFFFF


def make(issuers=None, profile=None, pem=True, meta=True, **kw):
    kw.setdefault("table_slots", 1 << 20)
    kw.setdefault("pair_slots", 1 << 14)
    kw.setdefault("collect_meta", True)
    e = ctmr.Engine(device=0, **kw)
    if profile:
        e.set_profile(profile)
    if issuers:
        e.add_issuers(issuers)
    e.set_filter(b"", True, NOW)
    e.set_pipeline_writeback(pem=pem, meta=meta)
    return e


def arrays(b):
    pay = np.concatenate([b.payload, np.zeros(32, np.uint8)])
    return pay, b.offsets.astype(np.uint64), b.issuer_idx.astype(np.uint32), b.entry_type.astype(np.uint8)


class Stream:
    """What the tickets of one engine brought, in submission order, to be held to the oracle at the end."""

    def __init__(self, eng):
        self.eng, self.certs, self.canon, self.hours, self.new, self.items = eng, [], [], [], [], []
        self._canon = {}

    def canon_of(self, idx):
        if idx not in self._canon:
            self._canon[idx] = self.eng.issuer_info(idx).canonical_idx if idx != NO_ISSUER else 0
        return self._canon[idx]

    def ticket(self, ticket, wait, certs):
        """ticket_writeback, then the wait; certs: the ticket's certificates (DER), one per entry."""
        eng = self.eng
        wb = eng.ticket_writeback(ticket)
        res = wait(ticket)
        assert len(res.records) == len(certs)
        new = [int(i) for i in res.new_idx]
        assert wb.info.n_new == len(new) and int(wb.pem_offsets[0]) == 0 and len(wb.pem_offsets) == len(new) + 1
        assert wb.pem_blocks() == [orc.pem_encode(certs[i]) for i in new]
        keys = []
        for (kind, entry, idx, hour, b), off in zip(wb.items, wb.offs):
            assert entry in new, (kind, entry)
            assert idx == res.records["issuer_idx"][entry] and hour == res.records["exp_hour"][entry]
            assert certs[entry][off:off + len(b)] == b
            assert b == b"" or kind in (N.MK_CRL, N.MK_DN)
            keys.append((entry, kind, off))
        assert keys == sorted(keys)
        base = len(self.certs)
        self.certs += certs
        self.canon += [self.canon_of(int(i)) for i in res.records["issuer_idx"]]
        self.hours += [int(h) for h in res.records["exp_hour"]]
        self.new += [base + i for i in new]
        self.items += [(kind, base + entry, idx, hour, b) for kind, entry, idx, hour, b in wb.items]
        return wb, res

    def check(self, already=()):
        """the items over all tickets are the stream's first sightings, none reported twice"""
        want = expected_first_sightings(self.certs, self.canon, self.new, self.hours) - set(already)
        got = got_first_sightings(self.eng, self.items)
        assert len(got) == len(self.items)
        assert got == want
        return got


def raw_cert(raw, i):
    leaf, extra = raw.leaf_input(i), raw.extra_data(i)
    e = orc.decode_entry(leaf, extra)
    assert e.ok
    return (extra if e.cert_in_extra else leaf)[e.cert_off:e.cert_off + e.cert_len]


# ------------------------------------------------------------------ the four forms
@pytest.mark.parametrize("size,count", [(257, 40), (1001, 20)])
def test_packed_tickets(size, count):
    cfg = synth.config(seed=141, n_issuers=48, zipf=1, dup_permille=200, ca_permille=10, expired_permille=10)
    issuers = synth.issuers(cfg)
    eng = make(issuers)
    batches = [synth.host_batch(cfg, k * size, size) for k in range(count)]
    keep = [arrays(b) for b in batches]
    tickets = [eng.submit_batch(a[0], a[1], a[2], a[3], b.n) for a, b in zip(keep, batches)]
    st = Stream(eng)
    for b, t in zip(batches, tickets):
        st.ticket(t, lambda t: eng.wait(t, b.n), [b.cert(i) for i in range(b.n)])
    whole = synth.host_batch(cfg, 0, size * count)
    _, _, unk, _ = run_oracle(whole, issuers, b"", True, NOW)
    assert st.new == [int(i) for i in np.nonzero(unk)[0]]
    got = st.check()
    assert {k[0] for k in got} == {N.MK_EXPDATE, N.MK_CRL, N.MK_DN}
    eng.close()


def test_raw_tickets():
    cfg = synth.config(seed=142, n_issuers=32, zipf=1, dup_permille=200, ca_permille=10, expired_permille=10)
    eng = make()
    size, count = 333, 12
    raws = [synth.host_entries(cfg, k * size, size) for k in range(count)]
    keep = [(np.concatenate([np.ascontiguousarray(r.blob, dtype=np.uint8), np.zeros(32, np.uint8)]), np.ascontiguousarray(r.bounds, dtype=np.uint64))
            for r in raws]
    tickets = [eng.submit_entries(a[0], a[1], r.n) for a, r in zip(keep, raws)]
    st = Stream(eng)
    o = orc.Engine(b"", True, NOW)
    for r, t in zip(raws, tickets):
        _, res = st.ticket(t, lambda t: eng.wait_entries(t, r.n), [raw_cert(r, i) for i in range(r.n)])
        _, unk, _, _ = o.raw_batch(r.blob, r.bounds)
        assert (res.new_idx == np.nonzero(unk)[0]).all()
    assert len(st.new) > 1000
    st.check()
    eng.close()


def test_json_tickets():
    cfg = synth.config(seed=143, n_issuers=12, zipf=1, dup_permille=150)
    eng = make()
    st = Stream(eng)
    groups, at = [], 0
    for k, per in enumerate((7, 1, 40, 7)):
        nb = 1 if k % 3 == 2 else 2
        raw = synth.host_entries(cfg, at, per * nb)
        at += per * nb
        bodies = ge.write([(raw.leaf_input(i), raw.extra_data(i)) for i in range(raw.n)], per)
        if k == 1:
            bodies.insert(1, b'{"entries":[]}')
        groups.append((bodies, raw))
    tickets = [eng.submit_entries_json(bodies) for bodies, _ in groups]
    assert len({t >> 20 for t in tickets}) == 1
    for (bodies, raw), t in zip(groups, tickets):
        st.ticket(t, eng.wait_entries_json, [raw_cert(raw, i) for i in range(raw.n)])
    assert len(st.new) > 50
    st.check()
    eng.close()


def test_pem_tickets():
    cfg = synth.config(seed=144, n_issuers=6, zipf=1, dup_permille=150, ca_permille=20, expired_permille=20)
    issuers = synth.issuers(cfg)
    eng = make(issuers)
    b = synth.host_batch(cfg, 0, 90)
    st = Stream(eng)
    groups = []
    for cuts in ([0, 1], list(range(1, 21)), [20, 50], [], [50, 55, 55, 90]):
        files = [pt.write([b.cert(i) for i in range(lo, hi)]) for lo, hi in zip(cuts[:-1], cuts[1:])]
        iss = [int(b.issuer_idx[lo]) if hi > lo else NO_ISSUER for lo, hi in zip(cuts[:-1], cuts[1:])]
        groups.append((files, iss, list(range(cuts[0], cuts[-1])) if cuts else []))
    tickets = [eng.submit_pem(f, i) for f, i, _ in groups]
    assert len({t >> 20 for t in tickets}) == 1
    for (f, i, which), t in zip(groups, tickets):
        st.ticket(t, eng.wait_pem, [b.cert(k) for k in which])
    assert len(st.new) > 30
    st.check()
    eng.close()


# ------------------------------------------------------------------ ticket edges
def test_ticket_edges_in_one_super_batch():
    """New counts 0, 1, 63, 64, 65, 255, 256, 257 and 0 again in one super-batch, duplicates placed by hand between the
    new certificates, an empty batch as the first and as the last ticket; then the same again: nothing new at all."""
    cfg = synth.config(seed=145, n_issuers=8, dup_permille=0, ca_permille=0, expired_permille=0)
    issuers = synth.issuers(cfg)
    eng = make(issuers)
    seeds = synth.host_batch(cfg, 0, 5)
    seed_res = eng.map_batch(seeds)                        # what the tickets without anything new repeat
    assert seed_res.stats.n_new == 5
    eng.meta_new()                                         # (the seeds' sightings go to the synchronous call)
    seed_hours = [int(h) for h in seed_res.records["exp_hour"]]
    fresh = synth.host_batch(cfg, 5, 1 + 63 + 64 + 65 + 255 + 256 + 257)
    seed_certs = [(seeds.cert(i), int(seeds.issuer_idx[i])) for i in range(5)]
    tickets_certs, at = [[]], 0
    for c in (0, 1, 63, 64, 65, 255, 256, 257, 0):
        mine = [seed_certs[0], seed_certs[3]] if c == 0 else []
        for k in range(c):
            mine.append((fresh.cert(at + k), int(fresh.issuer_idx[at + k])))
            if k % 50 == 7:
                mine.append(seed_certs[k % 5])             # a known certificate between two new ones
            if k % 64 == 63:
                mine.append(mine[-1])                      # a copy right behind its original: the lower index is the new one
        at += c
        tickets_certs.append(mine)
    tickets_certs.append([])
    batches = [Batch.from_certs([d for d, _ in m], [i for _, i in m]) for m in tickets_certs]
    for rnd in range(2):
        keep = [arrays(b) for b in batches]
        tickets = [eng.submit_batch(a[0], a[1], a[2], a[3], b.n) for a, b in zip(keep, batches)]
        eng.flush()
        assert len({t >> 20 for t in tickets}) == 1
        # the model: the super-batch's NEW list and PEM offsets from the oracle, cut by writeback.split
        first = np.concatenate([[0], np.cumsum([b.n for b in batches])])
        all_certs = [d for m in tickets_certs for d, _ in m]
        seen, new_idx = set(seeds.cert(i) for i in range(5)), []
        for i, d in enumerate(all_certs):
            if rnd == 0 and d not in seen:
                seen.add(d)
                new_idx.append(i)
        po = np.concatenate([[0], np.cumsum([len(orc.pem_encode(all_certs[i])) for i in new_idx])]).astype(np.uint64)
        model = writeback.split(new_idx, first, po, [])
        st = Stream(eng)
        counts = []
        for m, t, b, sl in zip(tickets_certs, tickets, batches, model):
            wb, res = st.ticket(t, lambda t: eng.wait(t, b.n), [d for d, _ in m])
            assert (res.new_idx == sl.new_idx).all() and (wb.pem_offsets == sl.pem_offsets).all()
            counts.append(len(res.new_idx))
        assert counts == ([0, 0, 1, 63, 64, 65, 255, 256, 257, 0, 0] if rnd == 0 else [0] * 11)
        if rnd == 0:
            seed_canon = [st.canon_of(i) for _, i in seed_certs]
            want = expected_first_sightings([d for d, _ in seed_certs] + st.certs, seed_canon + st.canon,
                                            list(range(5)) + [5 + i for i in st.new], seed_hours + st.hours)
            seed_items = expected_first_sightings([d for d, _ in seed_certs], seed_canon, list(range(5)), seed_hours)
            got = got_first_sightings(eng, st.items)
            assert len(got) == len(st.items) and got == want - seed_items
        else:
            assert st.items == [] and st.new == []
    eng.close()


# ------------------------------------------------------------------ items
URI_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 4096)


def item_corpus():
    """Hand-built certificates under one issuer: URIs of the edge lengths, one entry with all six items, host entries, and a
    run of certificates whose URI lengths step through 1..16 so that the Names behind them start at every phase of the
    packed bytes."""
    issuer = D.cert(serial=b"\x31", exts=[D.BC_CA], subject=D.name(D.rdn(3, b"Writeback CA")))
    certs, serial = [], [0]

    def add(nm, uris, **kw):
        serial[0] += 1
        exts = [D.BC_NOT_CA] + ([dp_ext(dp(*[uri(u) for u in uris]))] if uris is not None else [])
        certs.append(D.cert(serial=b"\x05" + serial[0].to_bytes(3, "big"), issuer=nm, exts=exts, **kw))

    base = D.name(D.rdn(3, b"Writeback CA"))
    for n in URI_LENGTHS:
        add(base, [(b"http://len.example/%04d/" % n + b"u" * n)[:n]])
    # all six: a fresh hour, a fresh Name, four fresh URIs
    add(D.name(D.rdn(10, b"Six"), D.rdn(3, b"Writeback CA")), [b"http://six.example/%d" % k for k in range(4)], not_after=D.utctime("280203040000Z"))
    # host: five URIs; a Name beyond 4 096 octets
    add(base, [b"http://five.example/%d" % k for k in range(5)])
    add(D.name(D.rdn(10, b"x" * 5000), D.rdn(3, b"Writeback CA")), [b"http://big-name.example/"])
    for k in range(1, 49):        # URI of 1..16 octets in front of a fresh Name: the Name's bytes start at every phase
        add(D.name(D.rdn(10, b"Phase %02d" % k), D.rdn(3, b"Writeback CA")), [(b"p%02d:" % k + b"/" * 16)[:4 + k % 16 + (1 if k % 16 == 0 else 0)]])
    return issuer, certs


@pytest.mark.parametrize("profile", ["reference", "fast"])
def test_items_at_every_length_and_phase(profile):
    issuer, certs = item_corpus()
    eng = make([issuer], profile)
    cut = 12
    parts = [certs[:cut], certs[cut:]]
    batches = [Batch.from_certs(p, [0] * len(p)) for p in parts]
    keep = [arrays(b) for b in batches]
    tickets = [eng.submit_batch(a[0], a[1], a[2], a[3], b.n) for a, b in zip(keep, batches)]
    assert len({t >> 20 for t in tickets}) == 1
    st = Stream(eng)
    wbs = [st.ticket(t, lambda t: eng.wait(t, b.n), p)[0] for t, b, p in zip(tickets, batches, parts)]
    assert st.new == list(range(len(certs)))
    got = st.check()
    lens = {len(k[3]) for k in got if k[0] == N.MK_CRL}
    assert set(URI_LENGTHS) <= lens
    six = [it for it in st.items if it[1] == len(URI_LENGTHS)]
    assert [it[0] for it in six] == [N.MK_EXPDATE] + [N.MK_CRL] * 4 + [N.MK_DN]
    assert sorted(it[1] for it in st.items if it[0] == N.MK_HOST) == [len(URI_LENGTHS) + 1, len(URI_LENGTHS) + 2]
    # where every item's bytes start in the super-batch's packed bytes: the second ticket's follow the first's
    phases, at = {N.MK_CRL: set(), N.MK_DN: set()}, 0
    for wb in wbs:
        for kind, _, _, _, b in wb.items:
            if b:
                phases[kind].add(at % 16)
            at += len(b)
    assert phases[N.MK_DN] == set(range(16)) and phases[N.MK_CRL] == set(range(16))
    eng.close()


def test_overflow_repeats_the_run_and_leaves_the_cold_memo():
    """400 certificates with a Name, four URIs and an hour of their own under one issuer: 2 400 items against the first run's
    3 · 400 + 1 024.  The worker's repeat delivers all of them once; the memo afterwards is the cold one — it holds this
    super-batch's items, and what an earlier super-batch had reported was reported again."""
    issuer = D.cert(serial=b"\x32", exts=[D.BC_CA], subject=D.name(D.rdn(3, b"Overflow CA")))

    def one(k, tag, n_uris=4):
        hour = "28%02d%02d%02d0000Z" % (1 + k // 672 % 12, 1 + k // 24 % 28, k % 24)
        us = [b"http://overflow.example/%04d/%d.crl" % (k, j) for j in range(n_uris)]
        return D.cert(serial=bytes([tag]) + k.to_bytes(3, "big"), issuer=D.name(D.rdn(3, b"Overflow CA %04d" % k)), not_after=D.utctime(hour),
                      exts=[D.BC_NOT_CA, dp_ext(dp(*[uri(u) for u in us]))])

    eng = make([issuer])
    small = [one(k, 1, 1) for k in range(20)]
    big = [one(k, 2) for k in range(400)]
    again = [one(k, 3) for k in range(0, 400, 7)]
    reports = []
    for part in (small, big, again):
        b = Batch.from_certs(part, [0] * len(part))
        a = arrays(b)
        t = eng.submit_batch(a[0], a[1], a[2], a[3], b.n)
        st = Stream(eng)
        st.ticket(t, lambda t: eng.wait(t, b.n), part)
        assert st.new == list(range(len(part)))
        reports.append((st, got_first_sightings(eng, st.items)))
        assert len(reports[-1][1]) == len(st.items)
    assert len(reports[0][1]) == 3 * 20
    st, got = reports[1]
    assert len(st.items) == 2400 and got == expected_first_sightings(st.certs, st.canon, st.new, st.hours)   # cold: the small one's again
    assert reports[0][1] <= got
    assert reports[2][0].items == []
    eng.close()


# ------------------------------------------------------------------ semantics
def _wb_raw(eng, ticket, pem_cap, off_n, items_cap, bytes_cap):
    info = N.WritebackInfo()
    pem = np.full(max(pem_cap, 1), 0xEE, np.uint8)
    offs = np.full(max(off_n, 1), 2**64 - 1, np.uint64)
    items = (N.MetaItem * max(items_cap, 1))()
    buf = np.full(max(bytes_cap, 1), 0xEE, np.uint8)
    rc = N.lib().ctmr_ticket_writeback(eng.handle, ticket, pem.ctypes.data if pem_cap else None, pem_cap, offs.ctypes.data if off_n else None,
                                       items if items_cap else None, items_cap, buf.ctypes.data if bytes_cap else None, bytes_cap, C.byref(info))
    return rc, info, pem, offs, buf


def test_flags_buffers_and_ticket_life():
    cfg = synth.config(seed=146, n_issuers=8, dup_permille=100)
    issuers = synth.issuers(cfg)
    plain = ctmr.Engine(device=0, table_slots=1 << 16, pair_slots=1 << 12)
    with pytest.raises(ctmr.CtmrError) as ei:              # META needs collect_meta
        plain.set_pipeline_writeback(meta=True)
    assert ei.value.code == N.E_INVAL
    assert N.lib().ctmr_set_pipeline_writeback(plain.handle, 4) == N.E_INVAL
    plain.close()
    eng = make(issuers, pem=False, meta=False)
    assert N.lib().ctmr_set_pipeline_writeback(eng.handle, 8 | 1) == N.E_INVAL
    batches = [synth.host_batch(cfg, 300 * k, 300) for k in range(4)]
    keep = [arrays(b) for b in batches]

    def submit(k):
        a, b = keep[k], batches[k]
        return eng.submit_batch(a[0], a[1], a[2], a[3], b.n)

    # flags 0: all zero, CTMR_OK, no buffers
    t0 = submit(0)
    rc, info, *_ = _wb_raw(eng, t0, 0, 0, 0, 0)
    assert rc == 0 and bytes(info) == bytes(C.sizeof(N.WritebackInfo))
    r0 = eng.wait(t0, 300)
    # PEM only; META only — each super-batch takes the flags as they stand when it is opened
    eng.set_pipeline_writeback(pem=True)
    t1 = submit(1)
    eng.flush()
    eng.set_pipeline_writeback(meta=True)
    t2 = submit(2)
    eng.flush()
    w1 = eng.ticket_writeback(t1)
    assert w1.info.flags == N.WB_PEM and w1.items == [] and w1.info.n_items == 0 and w1.info.pem_bytes > 0
    w2 = eng.ticket_writeback(t2)
    assert w2.info.flags == N.WB_META and w2.info.pem_bytes == 0 and len(w2.pem_buf) == 0 and len(w2.items) > 0
    eng.meta_reset()                                       # (the eight issuers' Names and URIs count as unseen again: items with bytes)
    eng.set_pipeline_writeback(pem=True, meta=True)
    t3 = submit(3)
    # too small → E_RANGE with info filled and nothing written; then success; repeated calls are identical
    w3 = eng.ticket_writeback(t3)
    inf = w3.info
    assert inf.flags == 3 and inf.n_new > 0 and inf.pem_bytes > 0 and inf.n_items > 0 and inf.item_bytes > 0
    for caps in ((0, 0, 0, 0), (inf.pem_bytes - 1, inf.n_new + 1, inf.n_items, inf.item_bytes), (inf.pem_bytes, 0, inf.n_items, inf.item_bytes),
                 (inf.pem_bytes, inf.n_new + 1, inf.n_items - 1, inf.item_bytes), (inf.pem_bytes, inf.n_new + 1, inf.n_items, inf.item_bytes - 1)):
        rc, info, pem, offs, buf = _wb_raw(eng, t3, *[int(c) for c in caps])
        assert rc == N.E_RANGE and bytes(info) == bytes(inf)
        assert (pem == 0xEE).all() and (buf == 0xEE).all() and (offs == 2**64 - 1).all()
    again = eng.ticket_writeback(t3)
    assert again.pem_buf.tobytes() == w3.pem_buf.tobytes() and (again.pem_offsets == w3.pem_offsets).all() and again.items == w3.items
    # collected out of order; after the wait the ticket is gone
    r3 = eng.wait(t3, 300)
    with pytest.raises(ctmr.CtmrError) as ei:
        eng.ticket_writeback(t3)
    assert ei.value.code == N.E_NOTFOUND
    r1, r2 = eng.wait(t1, 300), eng.wait(t2, 300)
    assert w1.pem_blocks() == [orc.pem_encode(batches[1].cert(int(i))) for i in r1.new_idx]
    assert w3.pem_blocks() == [orc.pem_encode(batches[3].cert(int(i))) for i in r3.new_idx]
    assert len(r0.new_idx) and len(r2.new_idx)
    eng.close()


def test_a_sighting_goes_to_the_earlier_super_batch_and_never_to_a_later_synchronous_call():
    issuer = D.cert(serial=b"\x33", exts=[D.BC_CA], subject=D.name(D.rdn(3, b"Carrier CA")))
    nm = D.name(D.rdn(3, b"Carrier CA"))

    def one(serial, u):
        return D.cert(serial=serial, issuer=nm, exts=[D.BC_NOT_CA, dp_ext(dp(uri(u)))])

    eng = make([issuer])
    first, second, third = [one(b"\x01", b"http://carrier.example/a")], [one(b"\x02", b"http://carrier.example/a")], \
        [one(b"\x03", b"http://carrier.example/a"), one(b"\x04", b"http://carrier.example/b")]
    bs = [Batch.from_certs(p, [0] * len(p)) for p in (first, second)]
    keep = [arrays(b) for b in bs]
    t1 = eng.submit_batch(*keep[0], 1)
    eng.flush()
    t2 = eng.submit_batch(*keep[1], 1)
    assert t1 >> 20 != t2 >> 20                            # consecutive super-batches
    w2, w1 = eng.ticket_writeback(t2), eng.ticket_writeback(t1)
    assert sorted(k for k, *_ in w1.items) == [N.MK_EXPDATE, N.MK_CRL, N.MK_DN] and w2.items == []
    assert len(w1.pem_blocks()) == len(w2.pem_blocks()) == 1
    eng.wait(t2, 1)
    eng.wait(t1, 1)
    res = eng.map_batch(Batch.from_certs(third, [0, 0]))   # the memo is the engine's: the synchronous call reports what is left
    assert res.stats.n_new == 2
    assert [(k, e, b) for k, e, _, _, b in eng.meta_new()] == [(N.MK_CRL, 1, b"http://carrier.example/b")]
    eng.close()


# ------------------------------------------------------------------ threads
def test_four_threads_fetch_their_own_tickets():
    cfg = synth.config(seed=147, n_issuers=16, dup_permille=0)
    issuers = synth.issuers(cfg)
    eng = make(issuers)
    per, rounds, T = 501, 6, 4
    pems, items, errors = [set() for _ in range(T)], [[] for _ in range(T)], []

    def worker(t):
        try:
            for r in range(rounds):
                b = synth.host_batch(cfg, (t * rounds + r) * per, per)
                a = arrays(b)
                tk = eng.submit_batch(a[0], a[1], a[2], a[3], b.n)
                wb = eng.ticket_writeback(tk)
                res = eng.wait(tk, b.n)
                blocks = wb.pem_blocks()
                assert len(blocks) == len(res.new_idx)
                pems[t].update(blocks)
                for kind, entry, idx, hour, by in wb.items:
                    assert entry in res.new_idx
                    items[t].append((kind, ((t * rounds + r) * per) + entry, idx, hour, by))
        except Exception as ex:                          # noqa: BLE001
            errors.append(ex)
    ths = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errors, errors
    whole = synth.host_batch(cfg, 0, per * rounds * T)
    _, _, unk, eh = run_oracle(whole, issuers, b"", True, NOW)
    new = [int(i) for i in np.nonzero(unk)[0]]
    assert set().union(*pems) == {orc.pem_encode(whole.cert(i)) for i in new}
    every = [it for part in items for it in part]
    got = got_first_sightings(eng, every)
    assert len(got) == len(every)
    assert got == expected_first_sightings([whole.cert(i) for i in range(whole.n)], [int(k) for k in whole.issuer_idx], new, eh)
    eng.close()


# ------------------------------------------------------------------ end to end
def test_host_writer_stores_the_new_set_from_tickets(tmp_path):
    cfg = synth.config(seed=148, n_issuers=6, zipf=1, dup_permille=200, ca_permille=10, expired_permille=10)
    issuers = synth.issuers(cfg)
    eng = make(issuers, meta=False)
    root = tmp_path / "certs"
    w = HostWriter(str(root), [eng.issuer_id(k) for k in range(len(issuers))], threads=4)
    size, count = 120, 4
    batches = [synth.host_batch(cfg, k * size, size) for k in range(count)]
    keep = [arrays(b) for b in batches]
    tickets = [eng.submit_batch(a[0], a[1], a[2], a[3], b.n) for a, b in zip(keep, batches)]
    jobs, alive = [], []
    for b, t in zip(batches, tickets):
        wb = eng.ticket_writeback(t)
        res = eng.wait(t, b.n)
        recs = np.ascontiguousarray(res.records[res.new_idx.astype(np.int64)])
        pem = wb.pem_buf if len(wb.pem_buf) else np.zeros(1, np.uint8)
        alive.append((wb, recs, pem))
        jobs.append((w.submit(pem.ctypes.data, wb.pem_offsets.ctypes.data, recs.ctypes.data, len(recs)), len(recs)))
    for job, n in jobs:
        files, _, skipped, _ = w.wait(job)
        assert files == n and skipped == 0
    w.close()
    whole = synth.host_batch(cfg, 0, size * count)
    _, _, unk, eh = run_oracle(whole, issuers, b"", True, NOW)
    want = {}
    for i in np.nonzero(unk)[0]:
        der = whole.cert(int(i))
        c = orc.parse_cert(der)
        serial = der[c.serial_off:c.serial_off + c.serial_len]
        path = os.path.join(orc.exp_date_id(int(eh[i])), eng.issuer_id(int(whole.issuer_idx[i])), base64.urlsafe_b64encode(serial).decode())
        want[path] = orc.pem_encode(der)
    have = {}
    for dp_, _, fs in os.walk(root):
        for f in fs:
            full = os.path.join(dp_, f)
            have[os.path.relpath(full, root)] = open(full, "rb").read()
    assert len(want) > 300 and have == want
    eng.close()
