"""-m gpu: the dates the device reads (rd_time inside the map kernels), floors (k_map*), compares with `now` (the expired
filter, k_sweep, the lists), keeps (the IssuerMetadata memo's 2^20-hour bitmap) and writes back (resp_put_key / resp_rec,
rp_set_key) — on the cases of tests/calendar_corpus.py, whose expected values come from Python's datetime
(tests/test_calendar_corpus_cpu.py holds that reference to the oracle and to the host build of the walk without a GPU).

Records, stats and state are compared with the oracle in the same mode, as the other parity tests do; exp_hour of every
accepted case, the status of every rejected one and the text of every set name are ALSO compared with the Python reference
directly, so that a mistake the oracle and a kernel share still fails.  Nothing here reads anything outside the repository."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401

import ct_mapreduce_amd as ctmr  # noqa: E402
from ct_mapreduce_amd import _native as N, known_image as KI  # noqa: E402
from ct_mapreduce_amd.engine import Batch, RawEntries  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import calendar_corpus as K  # noqa: E402
from tests.gpu_common import run_oracle, assert_records_equal, assert_state_equal  # noqa: E402
from tests.test_entry_decode_cpu import x509_leaf, precert_leaf, chain, asn1cert  # noqa: E402
from tests.test_gpu_entries import check_against_oracle  # noqa: E402
from tests.test_walk_cpu import tbs_of  # noqa: E402

VARIANTS = {"winc_separate_insert": 13, "fused": 15}          # the two of tests/test_gpu_reduce_corpus.py
PROFILES = ("reference", "fast")
IN_RANGE = ("grid", "instants", "zones", "shapes", "name_values", "not_before")
SLOTS = dict(table_slots=1 << 16, pair_slots=1 << 15)


def engine(variant="fused", profile="reference", **kw):
    eng = ctmr.Engine(device=0, map_variant=VARIANTS[variant], **dict(SLOTS, **kw))
    eng.set_profile(profile)
    eng.add_issuers(K.ISSUERS)
    assert [eng.issuer_id(k) for k in range(2)] == K.ISSUER_IDS
    return eng


def packed(cs):
    """The cases as one packed batch, entry types 0 and 1 alternating."""
    b = Batch.from_certs([c.der for c in cs], [c.iss for c in cs], [i & 1 for i in range(len(cs))])
    b.payload = np.concatenate([b.payload, np.zeros(N.PAYLOAD_PAD, np.uint8)])
    return b


def model_of(cs):
    """set name → sorted serials, by the Python reference alone (accepted cases whose hour some name spells)."""
    sets = {}
    for c in cs:
        if c.ok and K.in_range(c.hour):
            sets.setdefault(K.set_name(c.hour, c.iss), set()).add(c.serial)
    return {k: sorted(v) for k, v in sets.items()}


def assert_reference_records(records, cs, rejected=orc.ST_PARSE_ERROR):
    """exp_hour of every accepted case and the status of every case, by the Python reference.  rejected: the status of a
    case that does not parse (one for all, or one per case)."""
    want_ok = np.array([c.ok for c in cs])
    st = records["status"]
    want_st = np.where(want_ok, orc.ST_PASS, rejected)
    assert (st == want_st).all(), [(cs[i].label, int(st[i]), int(want_st[i])) for i in np.nonzero(st != want_st)[0][:10]]
    want = np.array([c.hour if c.ok else 0 for c in cs], np.int64)
    got = records["exp_hour"].astype(np.int64)
    assert (got[want_ok] == want[want_ok]).all(), [(cs[i].label, int(got[i]), int(want[i])) for i in np.nonzero(want_ok & (got != want))[0][:10]]


def assert_reference_state(eng, cs):
    """Every set name, and every set's members, by the Python reference."""
    sets = model_of(cs)
    assert sorted(eng.keys(b"serials::*")) == sorted(sets)
    assert eng.total_count() == sum(len(v) for v in sets.values())
    for name, members in sets.items():
        assert eng.set_list(name) == members, name


# ------------------------------------------------------------------------------------------------ the map, packed batches
_oracle = {}


def oracle_batches(profile, names):
    """The oracle's verdicts on the families, one batch each on ONE oracle engine, computed once per profile and shared."""
    key = (profile, names)
    if key not in _oracle:
        o = orc.Engine(b"", True, 0)
        o.set_profile(profile)
        out = []
        for k, name in enumerate(names):
            cs = K.shuffled(K.cases(name), k)
            b = packed(cs)
            o, st, unk, eh = run_oracle(b, K.ISSUERS, b"", True, 0, engine=o)
            out.append((name, cs, b, st, unk, eh))
        _oracle[key] = (o, out)
    return _oracle[key]


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_map_reads_and_floors_every_family(variant, profile):
    """Every family in a seeded shuffle, nothing filtered (log_expired): records, stats and state against the oracle in
    the same mode, exp_hour / status / set names and members against datetime.  The failing families are all named."""
    t0 = time.perf_counter()
    strict = profile == "reference"
    failed, n = [], 0
    for names in (IN_RANGE, ("out_of_range",)):
        o, batches = oracle_batches(profile, names)
        eng = engine(variant, profile)
        try:
            eng.set_filter(b"", True, 0)
            done = []
            for name, cs, b, st, unk, eh in batches:
                res = eng.map_batch(b)
                n += len(cs)
                done += cs
                try:
                    assert_records_equal(res, b, st, unk, eh, strict_strings=strict, strict_ext=strict)
                    assert_reference_records(res.records, cs)
                    assert int(unk.sum()) == sum(c.ok for c in cs) == res.stats.n_new       # no serial comes twice
                except AssertionError as ex:
                    failed.append("%s: %s" % (name, str(ex).splitlines()[0] if str(ex) else "assertion"))
            try:
                if names == IN_RANGE:
                    assert_state_equal(eng, o, len(K.ISSUERS))
                    assert_reference_state(eng, done)
                else:       # no name spells these hours: the oracle's keys (its own spelling) and the counts
                    assert sorted(eng.keys(b"serials::*")) == [k for k in o.keys() if k.startswith(b"serials::")]
                    assert eng.total_count() == o.total_count() == sum(c.ok for c in done)
            except AssertionError as ex:
                failed.append("state of %s: %s" % ("+".join(names), str(ex).splitlines()[0] if str(ex) else "assertion"))
        finally:
            eng.close()
    print("%s, %s: %d families, %d certificates, %.2f s" % (variant, profile, len(IN_RANGE) + 1, n, time.perf_counter() - t0))
    assert not failed, "\n".join(failed)


# ------------------------------------------------------------------------------------------------ the raw path
def raw_cases():
    return K.shuffled(K.cases("grid")[::7] + K.cases("instants") + K.cases("zones"), 11)


@pytest.mark.parametrize("profile", PROFILES)
def test_the_raw_path_reads_the_same_dates(profile):
    """get-entries leaf_input / extra_data pairs, X509 and precertificate entries alternating, the issuers registered from
    Chain[0] by the device."""
    t0 = time.perf_counter()
    cs = raw_cases()
    pairs = []
    for k, c in enumerate(cs):
        ch = chain([K.ISSUERS[c.iss]])
        pairs.append((precert_leaf(tbs_of(c.der), ts=k), asn1cert(c.der) + ch) if k & 1 else (x509_leaf(c.der, ts=k), ch))
    raw = RawEntries.from_pairs(pairs)
    raw.blob = np.concatenate([raw.blob, np.zeros(N.PAYLOAD_PAD, np.uint8)])
    eng = ctmr.Engine(device=0, **SLOTS)
    try:
        eng.set_profile(profile)
        eng.set_filter(b"", True, 0)
        res = eng.map_entries(raw)
        o = orc.Engine(b"", True, 0)
        o.set_profile(profile)
        check_against_oracle(eng, raw, o, res)
        # a precertificate entry whose TBSCertificate does not parse fails as an ENTRY under strict_leaf (the reference profile)
        leaf_fails = orc.ST_ENTRY_DECODE_ERROR if profile == "reference" else orc.ST_PARSE_ERROR
        assert_reference_records(res.records, cs, np.where(np.arange(len(cs)) & 1, leaf_fails, orc.ST_PARSE_ERROR))
        assert sorted(eng.issuer_id(k) for k in range(eng.issuer_count())) == sorted(K.ISSUER_IDS)
        assert_reference_state(eng, cs)
    finally:
        eng.close()
    print("%s: %d entries, %d accepted, %.2f s" % (profile, len(cs), sum(c.ok for c in cs), time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------ the filter's edge
def edge_instants():
    """A dozen accepted instants of both signs (one case each)."""
    want = [-1, 0, 1, (1 << 31) - 1, 1 << 31, 1 << 32, 1048576 * 3600, 277778 * 3600 - 1, -27778 * 3600, -2777778 * 3600,
            K.FIRST_SECOND, K.LAST_SECOND]
    by = {c.not_after: c for c in K.cases("instants")}
    return [by[t] for t in want]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_a_certificate_is_expired_only_when_not_after_lies_before_now(variant):
    t0 = time.perf_counter()
    cs = edge_instants()
    assert sum(c.not_after < 0 for c in cs) >= 4 and sum(c.not_after > 0 for c in cs) >= 6
    eng = engine(variant)
    try:
        for c in cs:
            b = packed([c])
            for now in (c.not_after - 1, c.not_after, c.not_after + 1):
                eng.set_filter(b"", False, now)
                res = eng.map_batch(b)
                want = orc.ST_FILTERED_EXPIRED if c.not_after < now else orc.ST_PASS
                assert res.records["status"][0] == want, (c.label, now)
                assert run_oracle(b, K.ISSUERS, b"", False, now)[1][0] == want, (c.label, now)
                assert res.records["exp_hour"][0] == c.hour, (c.label, now)
    finally:
        eng.close()
    print("%s: %d instants × 3 clocks, %.2f s" % (variant, len(cs), time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------ sweep and lists at `now`
def test_the_sweep_and_the_lists_at_the_edges_of_an_hour():
    """An engine with one set (or two: both issuers) at every hour of the instants.  expire_sweep(now) drops a set exactly
    when hour · 3600 <= now; known_lists(now) keeps it exactly while now < (hour + 1) · 3600 — against a dict model of the
    reference's hours, on a fresh engine per clock."""
    t0 = time.perf_counter()
    cs = K.cases("instants")
    b = packed(cs)
    hours = sorted({c.hour for c in cs})
    clocks = [t for h in (-277778, 0, 277778) for t in (h * 3600 - 1, h * 3600, (h + 1) * 3600 - 1, (h + 1) * 3600)]
    assert all(h in hours for h in (-277778, 0, 277778)) and hours[0] == K.HOUR_MIN and hours[-1] == K.HOUR_MAX
    for now in clocks:
        eng = engine()
        try:
            eng.set_filter(b"", True, 0)
            assert eng.map_batch(b).stats.n_new == len(cs)
            listed = {}
            for ident, text in eng.known_lists(now):
                assert text.endswith(b"\n")
                listed[ident.decode()] = sorted(text.split(b"\n")[:-1])
            want = {}
            for c in cs:
                if now < (c.hour + 1) * 3600:
                    want.setdefault(K.ISSUER_IDS[c.iss], []).append(c.serial.hex().encode())
            assert listed == {k: sorted(v) for k, v in want.items()}, now
            gone = [c for c in cs if c.hour * 3600 <= now]
            assert eng.expire_sweep(now) == len(gone), now
            assert_reference_state(eng, [c for c in cs if c.hour * 3600 > now])
        finally:
            eng.close()
    print("%d certificates in %d hours, %d clocks, %.2f s" % (len(cs), len(hours), len(clocks), time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------ the memo's bitmap edge
MEMO_HOURS = (-1, 0, 1048575, 1048576)             # the bitmap holds hours 0 .. 2^20 − 1; the others go to the hash set
_memo = []


def memo_batches():
    """Two certificates per (issuer, hour), the second of each pair in the later batch."""
    if not _memo:
        K.families()                                # (the corpus takes its serials first)
        for second in (1800, 3599):
            cs = []
            for h in MEMO_HOURS:
                for iss in (0, 1):
                    c = K.make("memo", "hour %d issuer %d +%d s" % (h, iss, second), 0x18, K.fmt(0x18, *K.civil_of(h * 3600 + second)), iss=iss)
                    assert c.ok and c.hour == h
                    cs.append(c)
            _memo.append(cs)
    return _memo


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_memo_reports_each_issuer_and_hour_once_on_both_sides_of_the_bitmap(variant):
    t0 = time.perf_counter()
    first, second = memo_batches()
    eng = engine(variant, collect_meta=True)
    try:
        eng.set_filter(b"", True, 0)
        res = eng.map_batch(packed(first))
        assert res.stats.n_new == len(first)
        assert_reference_records(res.records, first)
        got = [(it[2], it[3]) for it in eng.meta_new() if it[0] == N.MK_EXPDATE]
        assert sorted(got) == sorted((c.iss, c.hour) for c in first)             # each once …
        res = eng.map_batch(packed(second))
        assert res.stats.n_new == len(second)
        assert_reference_records(res.records, second)
        assert [it for it in eng.meta_new() if it[0] == N.MK_EXPDATE] == []       # … and only once
    finally:
        eng.close()
    print("%s: %d + %d certificates, %.2f s" % (variant, len(first), len(second), time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------ key text on the device and back
def resp_commands(stream):
    """A strict reader of RESP arrays of bulk strings, written out here: → [[argument, …], …].  Every length must be the
    canonical decimal of what follows, every part must end in CR LF."""
    out, p, n = [], 0, len(stream)

    def number(mark):
        nonlocal p
        assert stream[p:p + 1] == mark, (p, stream[p:p + 16])
        e = stream.index(b"\r\n", p)
        txt = stream[p + 1:e]
        v = int(txt)
        assert txt == str(v).encode() and v >= 0, (p, txt)
        p = e + 2
        return v

    while p < n:
        args = []
        for _ in range(number(b"*")):
            ln = number(b"$")
            assert stream[p + ln:p + ln + 2] == b"\r\n", (p, ln)
            args.append(stream[p:p + ln])
            p += ln + 2
        out.append(args)
    assert p == n
    return out


def test_key_text_and_expireat_on_the_device_and_back():
    """known_resp() of the engine that mapped grid + instants + zones: every key is date_id(hour) of the reference, every
    EXPIREAT str(hour · 3600) (nine to twelve characters, both signs), every bulk-string length right; known_resp_image of
    that stream is the image known_export gives.  With an hour outside 0000..9999 in the engine known_resp refuses (DESIGN.md
    §18 "Rejected": no four year digits spell its key), as the CPU twin does, and nothing else changes."""
    t0 = time.perf_counter()
    cs = K.shuffled(K.cases("grid", "instants", "zones"), 21)
    sets = model_of(cs)
    eng = engine()
    try:
        eng.set_filter(b"", True, 0)
        assert eng.map_batch(packed(cs)).stats.n_new == sum(c.ok for c in cs)
        stream = eng.known_resp()
        sadd, expire = {}, {}
        for args in resp_commands(stream):
            if args[0] == b"SADD":
                assert len(args) >= 3
                sadd.setdefault(args[1], []).extend(args[2:])
            else:
                assert args[0] == b"EXPIREAT" and len(args) == 3 and args[1] not in expire and args[1] in sadd
                expire[args[1]] = args[2]
        assert {k: sorted(v) for k, v in sadd.items()} == sets
        hour_of_name = {K.set_name(c.hour, c.iss): c.hour for c in cs if c.ok}
        assert expire == {k: str(h * 3600).encode() for k, h in hour_of_name.items()}
        assert {len(v) for v in expire.values()} >= {1, 5, 9, 10, 11, 12} and any(v.startswith(b"-") for v in expire.values())
        image = eng.known_resp_image(stream)
        back, export = KI.parse(image), KI.parse(eng.known_export())
        assert back.sets == export.sets == sets and back.n_members == export.n_members == sum(len(v) for v in sets.values())
        # an hour no name spells
        oor = [c for c in K.cases("out_of_range") if c.ok]
        assert eng.map_batch(packed(oor)).stats.n_new == len(oor)
        with pytest.raises(ctmr.CtmrError) as ex:
            eng.known_resp()
        assert ex.value.code == N.E_INVAL
        with pytest.raises(KI.ImageError):
            KI.image_resp(eng.known_export())
        assert eng.total_count() == sum(len(v) for v in sets.values()) + len(oor)
    finally:
        eng.close()
    print("%d certificates, %d sets, %d bytes of stream, %.2f s" % (len(cs), len(sets), len(stream), time.perf_counter() - t0))
