"""-m gpu: the Chain[0] → issuer match (kernels/entries.h match_wave in k_decode_match and k_chain0_match, the registration
loop of engine/entries.inc, the certificate store and table of engine/issuers.inc) over tests/chain0_corpus.py: issuer
certificates of every length mod 16 and on both sides of the comparison's 1 KiB, 2 KiB and 3 KiB steps, twins that differ in
one bit at every octet that matters, twins in the chunk before the masked last one at every residue, junk of 1 … 47
octets, a probe run that wraps the table, more unknown certificates than the claim table and the overflow list hold, batches around a wave, a workgroup and DECODE_PER_BLOCK.

References, bit for bit, no tolerances: the corpus' MODEL — a dict from Chain[0] bytes to registration index
(expected_issuer_idx, expected_view, expected_pending, expected_self_registration) — for the decode alone, and the ORACLE
(check_against_oracle) through the map.  Out-of-range reads are looked for by VALUE: the pad behind the blob is 0xff where the
certificate store pads with zeros, the octet behind a Chain[0] that ends its extra_data is the next leaf's 0xff."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import _native as N  # noqa: E402
from ct_mapreduce_amd.engine import CtmrError, RawEntries  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import chain0_corpus as K  # noqa: E402
from tests.test_gpu_entries import check_against_oracle  # noqa: E402

DEV = torch.device("cuda:0")
NOW = 1_700_000_000
MODES = {"exact": N.CHAIN0_EXACT, "trusted": N.CHAIN0_TRUSTED_LOG}


def engine(mode="exact", registered=(), **kw):
    kw.setdefault("table_slots", 1 << 12)
    kw.setdefault("pair_slots", 1 << 10)
    e = ctmr.Engine(device=0, **kw)
    e.set_filter(b"", True, NOW)
    e.set_chain0_match(MODES[mode])
    if registered:
        assert e.add_issuers(list(registered)) == 0
    return e


def decode(eng, pairs):
    """ctmr_decode_entries_device over blob ‖ 32 octets of 0xff: the view's arrays on the host, and the decode counters."""
    raw = RawEntries.from_pairs(pairs)
    n = raw.n
    blob = np.concatenate([raw.blob, np.full(K.PAD, 0xff, np.uint8)])
    d_blob = torch.from_numpy(blob).to(DEV)
    d_bounds = torch.from_numpy(raw.bounds.astype(np.int64)).to(DEV)
    t = {"cert_start": torch.zeros(n, dtype=torch.int64, device=DEV), "cert_end": torch.zeros(n, dtype=torch.int64, device=DEV),
         "issuer_idx": torch.full((n,), 0x55555555, dtype=torch.int32, device=DEV),
         "entry_type": torch.full((n,), 0x55, dtype=torch.uint8, device=DEV),
         "chain0_start": torch.zeros(n, dtype=torch.int64, device=DEV), "chain0_len": torch.zeros(n, dtype=torch.int32, device=DEV)}
    view = N.EntryView(timestamp=None, **{k: v.data_ptr() for k, v in t.items()})
    ds = eng.decode_entries_device(d_blob.data_ptr(), d_bounds.data_ptr(), n, view)
    out = {k: v.cpu().numpy() for k, v in t.items()}
    for k in ("cert_start", "cert_end", "chain0_start"):
        out[k] = out[k].astype(np.uint64)
    out["issuer_idx"] = out["issuer_idx"].astype(np.uint32)
    out["chain0_len"] = out["chain0_len"].astype(np.uint32)
    return out, ds


def check_view(out, ds, pairs):
    want = K.expected_view(pairs)
    for f in ("entry_type", "cert_start", "cert_end", "chain0_start", "chain0_len"):
        assert (out[f] == want[f]).all(), (f, np.nonzero(out[f] != want[f])[0][:8])
    assert (ds.n_x509, ds.n_precert, ds.n_decode_error, ds.n_no_chain) == want["counters"] and ds.n == len(pairs)


def check_idx(out, pairs, registered):
    want = K.expected_issuer_idx(pairs, registered)
    want = np.where(want == K.UNDECODABLE, K.NO_ISSUER, want).astype(np.uint32)
    bad = np.nonzero(out["issuer_idx"] != want)[0]
    assert len(bad) == 0, [(int(i), int(out["issuer_idx"][i]), int(want[i])) for i in bad[:8]]


def check_partition(eng, out, pairs):
    """The classes of equal issuer_idx are exactly the classes of equal Chain[0] bytes; issuer_id(idx) is the SHA-256 of that
    certificate's SubjectPublicKeyInfo."""
    c0 = K.chain0_of(pairs)
    of_idx, of_cert = {}, {}
    count = eng.issuer_count()
    for i, c in enumerate(c0):
        k = int(out["issuer_idx"][i])
        if not isinstance(c, bytes):
            assert k == K.NO_ISSUER, i
            continue
        assert k < count, (i, k)
        assert of_idx.setdefault(k, c) == c and of_cert.setdefault(c, k) == k, i
    assert len(of_idx) == len(of_cert) == len(K.distinct(c0))
    for k, c in of_idx.items():
        info, pc = eng.issuer_info(k), orc.parse_cert(c)
        assert pc.ok or not info.valid, k
        if info.valid:
            assert info.issuer_id.decode() == orc.issuer_id(c[pc.spki_off:pc.spki_off + pc.spki_len]), k
    return of_idx


def seeded_order(certs, what):
    certs = list(certs)
    K._rng("order", what).shuffle(certs)
    return certs


def family_pairs(name):
    if name == "twins_shuffled":
        fam = K.twins()
        return fam, [fam.pairs[i] for i in fam.info["shuffled"]]
    fam = K.FAMILIES[name]()
    return fam, fam.pairs


# ------------------------------------------------------------------ 1. decode alone against the dict

@pytest.mark.parametrize("name,mode", [("lengths", "exact"), ("lengths", "trusted"), ("edges", "exact"), ("edges", "trusted"),
                                       ("short", "exact"), ("twins", "exact"), ("twins", "trusted"),
                                       ("twins_shuffled", "exact"), ("twins_shuffled", "trusted"),
                                       ("waves", "exact")])
def test_decode_with_every_issuer_registered_beforehand(name, mode):
    """The index is the model's, in a registration order that is not the order of appearance; the trusted-log mode gives the
    same arrays (every twin carries HT_TWIN, every other hash is one certificate's)."""
    fam, pairs = family_pairs(name)
    registered = seeded_order(fam.chain0, name)
    eng = engine(mode, registered)
    out, ds = decode(eng, pairs)
    check_view(out, ds, pairs)
    check_idx(out, pairs, registered)
    check_partition(eng, out, pairs)
    assert ds.n_issuers_added == 0 and eng.issuer_count() == len(registered) == len(fam.chain0)
    if name == "lengths":                      # Chain[0] as the LAST thing in the blob: 0xff right behind it
        for batch in fam.info["last"]:
            out, ds = decode(eng, batch)
            check_view(out, ds, batch)
            check_idx(out, batch, registered)
    if name == "waves":                        # batch by batch: sizes around a wave, a workgroup, DECODE_PER_BLOCK
        for batch in fam.info["batches"]:
            out, ds = decode(eng, batch)
            check_view(out, ds, batch)
            check_idx(out, batch, registered)
    eng.close()


@pytest.mark.parametrize("name,mode", [("lengths", "exact"), ("lengths", "trusted"), ("edges", "exact"), ("short", "exact"),
                                       ("twins", "exact"), ("twins_shuffled", "exact"), ("waves", "exact")])
def test_decode_self_registering(name, mode):
    """Nothing registered: the call registers what it meets.  The partition by issuer_idx is the partition by bytes, the
    count is the number of distinct Chain[0], issuer_id is the SHA-256 of the SPKI; a second fresh engine gives the identical
    array.  (Trusted and self-registering only where hashes are distinct: lengths.)"""
    fam, pairs = family_pairs(name)
    runs = []
    for _ in range(2):
        eng = engine(mode)
        out, ds = decode(eng, pairs)
        check_view(out, ds, pairs)
        check_partition(eng, out, pairs)
        assert ds.n_issuers_added == eng.issuer_count() == len(fam.chain0)
        runs.append(out["issuer_idx"])
        if name == "lengths" and not runs[1:]:
            for batch in fam.info["last"]:     # … and these register nothing more
                o2, d2 = decode(eng, batch)
                check_view(o2, d2, batch)
                check_partition(eng, o2, batch)
                assert d2.n_issuers_added == 0
        if name == "waves" and not runs[1:]:
            for batch in fam.info["batches"]:  # a cold engine per size is the point: round 0 AND the retry rounds at every size
                e3 = engine(mode, fam.info["registered"])
                o3, d3 = decode(e3, batch)
                check_view(o3, d3, batch)
                check_partition(e3, o3, batch)
                reg, _ = K.expected_self_registration(batch, fam.info["registered"])
                check_idx(o3, batch, reg)
                assert d3.n_issuers_added == len(reg) - len(fam.info["registered"])
                e3.close()
        eng.close()
    assert (runs[0] == runs[1]).all()


def test_twins_register_one_per_hash_in_two_rounds_then_all_the_rest():
    """The documented order of a self-registering call (engine/entries.inc): rounds 0 and 1 register one certificate per
    candidate hash — the lowest log index — then report_all lists every entry that is left; indices follow log order within
    a round.  expected_self_registration restates it; the twins are what needs the third round."""
    for name in ("twins", "twins_shuffled"):
        fam, pairs = family_pairs(name)
        reg, rounds = K.expected_self_registration(pairs)
        assert len(rounds) == 3 and len(rounds[2]) > 1000 and len(reg) == len(fam.chain0)
        eng = engine("exact")
        out, ds = decode(eng, pairs)
        check_idx(out, pairs, reg)
        assert ds.n_issuers_added == len(reg)
        eng.close()


# ------------------------------------------------------------------ 2. through the map against the oracle

@pytest.mark.parametrize("profile", ["reference", "fast"])
@pytest.mark.parametrize("name", ["lengths", "edges", "short", "twins", "twins_shuffled", "waves"])
def test_through_the_map_against_the_oracle(name, profile):
    """Status, flags, expiry hour, the new list, by_status and the serials:: keys — a twin inside the modulus lands under its
    own issuer ID, one that no longer parses is an issuer parse error."""
    fam, pairs = family_pairs(name)
    eng = ctmr.Engine(device=0, table_slots=1 << 14, pair_slots=1 << 12)
    eng.set_profile(profile)
    eng.set_filter(b"", True, NOW)
    o = orc.Engine(b"", True, NOW)
    o.set_profile(profile)
    batches = fam.info["batches"] if name == "waves" else [pairs] + (fam.info["last"][::8] if name == "lengths" else [])
    for batch in batches:
        raw = RawEntries.from_pairs(batch)
        raw.blob = np.concatenate([raw.blob, np.full(N.PAYLOAD_PAD, 0xff, np.uint8)])
        res = eng.map_entries(raw)
        st, _ = check_against_oracle(eng, raw, o, res)
        idx = K.expected_issuer_idx(batch, K.distinct(K.chain0_of(batch)))
        assert ((st == orc.ST_ENTRY_DECODE_ERROR) == (idx == K.UNDECODABLE)).all()
        assert ((st == orc.ST_NO_ISSUER) == (idx == K.NO_ISSUER)).all()
    assert eng.issuer_count() == len(fam.chain0)
    if name.startswith("twins"):
        ids = {k.split(b"::")[2] for k in eng.keys(b"serials::*")}
        assert len(ids) > 2
    eng.close()
    o.close()


# ------------------------------------------------------------------ 3. registration reports

def failing_decode(eng, pairs):
    with pytest.raises(CtmrError) as err:
        decode(eng, pairs)
    assert err.value.code == N.E_NOTFOUND
    return eng.pending_issuers()


@pytest.mark.parametrize("name", ["lengths", "waves"])
def test_pending_issuers_and_the_number_of_calls(name):
    """Auto-registration off: the failed call reports, per distinct hash, the Chain[0] of the lowest log index; register
    them, call again, until the call succeeds — in as many calls as the model says."""
    fam = K.FAMILIES[name]()
    pairs = fam.pairs if name == "lengths" else fam.info["batches"][K.WAVE_SIZES.index(2049)]
    registered = list(fam.info["registered"]) if name == "waves" else [fam.chain0[5], fam.chain0[77]]
    eng = engine("exact", registered)
    eng.set_issuer_autoregister(False)
    calls = model_calls = 1
    reg = list(registered)
    while K.expected_pending(pairs, reg):
        reg += K.expected_pending(pairs, reg)
        model_calls += 1
    assert model_calls == 2                                     # distinct hashes: one report settles it
    reg = list(registered)
    while True:
        want = K.expected_pending(pairs, reg)
        if not want:
            break
        assert failing_decode(eng, pairs) == want
        eng.add_issuers(want)
        reg += want
        calls += 1
    out, ds = decode(eng, pairs)
    assert calls == model_calls and ds.n_issuers_added == 0
    check_view(out, ds, pairs)
    check_idx(out, pairs, reg)
    eng.close()


def test_pending_issuers_of_the_twins():
    """Every call with auto-registration off is a round 0: one certificate per hash, the lowest log index that carries an
    unregistered one.  Two reports are checked against the model (the second names each hash's SECOND certificate); the
    hundreds that would follow one by one are registered at once and the third call succeeds."""
    fam = K.twins()
    pairs = [fam.pairs[i] for i in fam.info["shuffled"]]
    eng = engine("exact")
    eng.set_issuer_autoregister(False)
    reg = []
    for n_want in (66, 2):                                      # 2 x 32 twins in the hashed head and tail, the two bases' hashes
        want = K.expected_pending(pairs, reg)
        assert len(want) == len({K.quick_hash(c) for c in want}) == n_want
        assert failing_decode(eng, pairs) == want
        eng.add_issuers(want)
        reg += want
    rest = [c for c in K.distinct(K.chain0_of(pairs)) if c not in set(reg)]
    assert len(rest) > 1000 and len({K.quick_hash(c) for c in rest}) == 2
    eng.add_issuers(rest)
    reg += rest
    out, ds = decode(eng, pairs)
    check_idx(out, pairs, reg)
    eng.close()


# ------------------------------------------------------------------ 4. claims

def test_more_unknown_certificates_than_the_claim_table_and_the_overflow_list_hold():
    """26 000 distinct hashes in one call: PEND_SLOTS claims, the 64-probe overflow onto unreg_list, more than UNREG_CAP
    entries on it.  Self-registration converges; the dict is the reference (decode only)."""
    fam = K.claims()
    eng = engine("exact")
    out, ds = decode(eng, fam.pairs)
    check_view(out, ds, fam.pairs)
    assert eng.issuer_count() == K.N_CLAIMS == ds.n_issuers_added
    idx, order = out["issuer_idx"], np.asarray(fam.info["order"])
    _, first = np.unique(order, return_index=True)              # first[k]: the first entry that carries certificate k
    assert (idx < K.N_CLAIMS).all() and len(np.unique(idx[first])) == K.N_CLAIMS
    assert (idx == idx[first][order]).all()                     # the repeats carry the index of their first occurrence
    for i in range(0, len(order), 1111):                        # … and the index names those bytes' certificate
        c = fam.chain0[order[i]]
        pc = orc.parse_cert(c)
        assert eng.issuer_id(int(idx[i])) == orc.issuer_id(c[pc.spki_off:pc.spki_off + pc.spki_len])
    out2, ds2 = decode(eng, fam.pairs[::-1][:5000])             # everything is registered now
    assert ds2.n_issuers_added == 0 and (out2["issuer_idx"] == idx[::-1][:5000]).all()
    eng.close()


# ------------------------------------------------------------------ 5. the host table's probe run wraps

@pytest.mark.parametrize("mode", ["exact", "trusted"])
def test_probe_run_that_wraps_the_table_and_a_same_hash_stranger(mode):
    fam = K.table()
    reg = fam.info["register"]
    eng = engine(mode, reg, max_issuers=K.TABLE_MAX_ISSUERS)
    out, ds = decode(eng, fam.pairs)
    check_view(out, ds, fam.pairs)
    check_idx(out, fam.pairs, reg + [fam.info["stranger"]])     # the stranger is the one new certificate: the next index
    assert ds.n_issuers_added == 1 and eng.issuer_count() == len(reg) + 1
    a, b = fam.info["cross"]                                    # equal upper halves and slots, different lengths
    both = [K.entry(k, c, "x509") for k, c in enumerate([b, a, b, b, a])]
    out, ds = decode(eng, both)
    check_idx(out, both, reg)
    eng.close()


# ------------------------------------------------------------------ 6. the certificate store grows with contents

def test_store_growth_keeps_the_certificates_registered_before():
    certs = K.length_certs()
    first = [certs[n] for n in K.LENGTHS[::3]]
    second, third = K.claims().chain0[:2200], K.claims().chain0[2200:5600]
    assert sum(len(c) + 32 for c in first) < (1 << 20) < sum(len(c) for c in second) and \
        2 * sum(len(c) + 32 for c in first + second) < sum(len(c) for c in first + second + third)
    eng = engine("exact")
    pairs = [K.entry(k, c, K.FORMS[k % 3]) for k, c in enumerate(first + second[::100] + third[::100] + first[::-1])]
    for part in (first, second, third):
        eng.add_issuers(part)
    out, ds = decode(eng, pairs)
    check_view(out, ds, pairs)
    check_idx(out, pairs, first + second + third)
    assert ds.n_issuers_added == 0
    eng.close()
