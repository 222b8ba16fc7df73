"""ct_mapreduce_amd/writeback.py — the CPU twin of the ingestion pipeline's write-back — held to the oracle with no engine:
a synthetic stream cut into super-batches and those into tickets at arbitrary places (empty tickets among them); what
split() hands each ticket must be the PEM of the ticket's own new certificates, the first sightings of the whole stream
exactly once over all tickets, every item inside its ticket, on a new entry, in (entry, kind, off) order."""
import random

import numpy as np
import pytest

from ct_mapreduce_amd import synth, writeback, _native as N
from oracle import oracle as orc
from tests.gpu_common import run_oracle
from tests.meta_corpus import expected_first_sightings

NOW = synth.BASE_TIME


def super_batch_items(certs, issuer_idx, exp_hours, new_idx, seen, rng):
    """What a super-batch's k_meta_new reports against the memo `seen` (updated): one item per first sighting, on the
    certificate that claims it — any of the new certificates that bring it — in arrival order (shuffled)."""
    carriers = {}
    for i in new_idx:
        name, uris, m = orc.cert_meta(certs[i])
        c = int(issuer_idx[i])
        mine = [((N.MK_EXPDATE, c, int(exp_hours[i]), b""), 0), ((N.MK_DN, c, 0, name), m.issuer_off)]
        mine += [((N.MK_CRL, c, 0, u), m.crl_off[k]) for k, u in enumerate(uris)]
        for key, off in mine:
            if key not in seen:
                carriers.setdefault(key, []).append((i, off))
    items = []
    for key, where in carriers.items():
        seen.add(key)
        i, off = rng.choice(where)
        items.append((key[0], i, int(issuer_idx[i]), int(exp_hours[i]), key[3], off))
    rng.shuffle(items)
    return items


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_split_hands_every_ticket_its_own(seed):
    rng = random.Random(seed)
    cfg = synth.config(seed=4100 + seed, n_issuers=12, zipf=1, dup_permille=250, ca_permille=20, expired_permille=20)
    issuers = synth.issuers(cfg)
    total = 1500
    whole = synth.host_batch(cfg, 0, total)
    certs = [whole.cert(i) for i in range(total)]
    o, st, unk, eh = run_oracle(whole, issuers, b"", True, NOW)
    new_all = [int(i) for i in np.nonzero(unk)[0]]
    assert 0 < len(new_all) < total
    want = expected_first_sightings(certs, [int(k) for k in whole.issuer_idx], new_all, eh)
    # super-batches, then tickets: cuts anywhere, some of them equal (empty tickets, empty super-batches' worth of them)
    sb_cuts = sorted([0, total] + [rng.randrange(total + 1) for _ in range(3)])
    seen, got, got_count = set(), set(), 0
    for s0, s1 in zip(sb_cuts, sb_cuts[1:]):
        cuts = sorted([s0, s1] + [rng.randrange(s0, s1 + 1) for _ in range(9)] + [s0, s1])   # empty first and last tickets
        new_idx = np.asarray([i - s0 for i in new_all if s0 <= i < s1], np.uint64)
        pems = [orc.pem_encode(certs[s0 + int(i)]) for i in new_idx]
        po = np.concatenate([[0], np.cumsum([len(p) for p in pems])]).astype(np.uint64)
        items = [(k, e - s0, idx, h, b, off)
                 for k, e, idx, h, b, off in super_batch_items(certs, whole.issuer_idx, eh, [int(i) + s0 for i in new_idx], seen, rng)]
        slices = writeback.split(new_idx, [c - s0 for c in cuts], po, items)
        assert len(slices) == len(cuts) - 1
        for (t0, t1), sl in zip(zip(cuts, cuts[1:]), slices):
            own_new = [i for i in new_all if t0 <= i < t1]
            assert [int(i) + t0 for i in sl.new_idx] == own_new
            assert int(sl.pem_offsets[0]) == 0 and len(sl.pem_offsets) == len(own_new) + 1
            assert sl.pem_blocks(b"".join(pems)) == [orc.pem_encode(certs[i]) for i in own_new]
            keys = []
            for kind, entry, idx, hour, b in sl.items:
                assert 0 <= entry < t1 - t0 and entry + t0 in own_new
                der = certs[entry + t0]
                off = der.find(b) if b else 0
                assert off >= 0
                keys.append((entry, kind))
                key = (kind, int(idx), hour if kind == N.MK_EXPDATE else 0, b)
                assert key not in got                       # reported once in the stream's life
                got.add(key)
                got_count += 1
            assert keys == sorted(keys)
            if t0 == t1:
                assert len(sl.new_idx) == 0 and sl.items == []
    assert got == want and got_count == len(want)


def test_split_orders_by_entry_kind_and_offset_and_refuses_what_cannot_be():
    new_idx = [2, 5, 6]
    items = [(N.MK_CRL, 5, 0, 7, b"u2", 90), (N.MK_DN, 5, 0, 7, b"dn", 40), (N.MK_CRL, 5, 0, 7, b"u1", 80),
             (N.MK_EXPDATE, 5, 0, 7, b"", 0), (N.MK_HOST, 2, 1, 9, b"", 0), (N.MK_EXPDATE, 6, 0, 8, b"", 0)]
    a, b, c, d = writeback.split(new_idx, [0, 0, 6, 7, 7], [0, 10, 30, 60], items)
    assert a.items == [] and len(a.new_idx) == 0 and list(a.pem_offsets) == [0]
    assert list(b.new_idx) == [2, 5] and list(b.pem_offsets) == [0, 10, 30] and b.pem_at == 0
    assert b.items == [(N.MK_HOST, 2, 1, 9, b""), (N.MK_EXPDATE, 5, 0, 7, b""), (N.MK_CRL, 5, 0, 7, b"u1"),
                       (N.MK_CRL, 5, 0, 7, b"u2"), (N.MK_DN, 5, 0, 7, b"dn")]
    assert list(c.new_idx) == [0] and list(c.pem_offsets) == [0, 30] and c.pem_at == 30
    assert c.items == [(N.MK_EXPDATE, 0, 0, 8, b"")]
    assert d.items == [] and list(d.pem_offsets) == [0]
    with pytest.raises(ValueError):
        writeback.split(new_idx, [0, 7], None, [(N.MK_EXPDATE, 3, 0, 7, b"", 0)])       # an item of an entry that is not new
    with pytest.raises(ValueError):
        writeback.split(new_idx, [0, 6], None, [])                                      # a new entry outside every ticket
    with pytest.raises(ValueError):
        writeback.split([5, 2], [0, 7], None, [])
