"""The corpus builders of the memo's every-length tests (tests/meta_corpus.py) without a GPU: every certificate is one the
oracle passes under both profiles, and each corpus has the structure the GPU tests rely on.  Conditions on the input, not
on the code under test: they keep tests/test_gpu_meta_lengths.py from passing on a corpus that no longer reaches the
length, the address or the path a test was written for."""
import functools

import numpy as np
import pytest

from ct_mapreduce_amd import _native as N
from ct_mapreduce_amd.engine import Batch
from oracle import oracle as orc
from tests import meta_corpus as MC
from tests.gpu_common import run_oracle

CORPORA = ("name_lengths", "uri_lengths", "addresses", "crowd", "overflow")


@functools.lru_cache(maxsize=None)
def corpus(which):
    return MC.crowd(2000) if which == "crowd" else getattr(MC, which)()


@functools.lru_cache(maxsize=None)
def metas(which):
    return [orc.cert_meta(der) for der, _ in corpus(which).certs]


def triples(c):
    groups = {}
    for i, r in enumerate(c.rows):
        if r.get("group") is not None:
            groups.setdefault(r["group"], {}).setdefault(r["role"], []).append(i)
    return groups


def item(c, ms, i):
    """(bytes, bytes behind them) of the item a row is about: the Name, or the URI of the claimed length."""
    der, row = c.certs[i][0], c.rows[i]
    m = ms[i][2]
    if row["kind"] in ("name", "address"):
        off, ln = m.issuer_off, m.issuer_len
    else:
        k = 1 if row.get("form") == "second" else 0
        off, ln = m.crl_off[k], m.crl_len[k]
    return der[off:off + ln], der[off + ln:off + ln + 15]


@pytest.mark.parametrize("which", CORPORA)
@pytest.mark.parametrize("profile", ["reference", "fast"])
def test_the_oracle_passes_every_certificate_under_both_profiles(which, profile):
    c = corpus(which)
    ders, idx, _ = c.part()
    o = orc.Engine(b"", True, 0)
    o.set_profile(profile)
    _, st, unk, _ = run_oracle(Batch.from_certs(ders, idx), c.issuers, engine=o)
    assert (st == orc.ST_PASS).all(), np.nonzero(st != orc.ST_PASS)[0][:10]
    assert unk.all()                                  # … and every one is a certificate of its own
    assert all(m is not None for m in metas(which))


@pytest.mark.parametrize("which", CORPORA)
def test_claimed_lengths_are_the_lengths_the_oracle_extracts(which):
    c = corpus(which)
    for i, (row, (name, uris, m)) in enumerate(zip(c.rows, metas(which))):
        assert m.n_crl_ext <= 1 and not m.bad_crl
        if "uris" in row:
            assert uris == row["uris"], i
        if row.get("kind") in ("name", "address"):
            assert len(name) == row["length"], i
        if row.get("kind") in ("uri", "address"):
            assert len(item(c, metas(which), i)[0]) == row["length"], i
        if row.get("kind") == "count":
            assert m.n_crl == row["length"]


@pytest.mark.parametrize("which", ["name_lengths", "uri_lengths"])
def test_triples_are_equal_equal_and_different_in_the_last_byte(which):
    c, ms = corpus(which), metas(which)
    n = 0
    for group, roles in triples(c).items():
        if group[0] not in ("name", "uri"):
            continue
        (a,), (again,) = roles["A"], roles["again"]
        ia, ib = item(c, ms, a), item(c, ms, again)
        assert ia[0] == ib[0] and c.certs[a][1] == c.certs[again][1]
        assert ia[1] != ib[1], group                   # the 15 bytes behind the item
        if c.rows[a]["length"] == 0:
            assert "prime" not in roles
            continue
        (p,) = roles["prime"]
        ip = item(c, ms, p)[0]
        assert len(ip) == len(ia[0]) and ip[:-1] == ia[0][:-1] and ip[-1] != ia[0][-1] and c.certs[p][1] == c.certs[a][1]
        n += 1
    assert n >= {"name_lengths": 150, "uri_lengths": 4 * 171}[which]


def test_name_lengths_reach_every_switch():
    c = corpus("name_lengths")
    got = {r["length"] for r in c.rows}
    lo = min(got)
    assert lo <= 15
    small = [n for n in c.unreachable if n <= MC.NAME_TOP]
    assert len(small) < 5 and got | set(c.unreachable) >= set(range(lo, MC.NAME_TOP + 1)) | set(MC.NAME_BIG)
    assert not set(c.unreachable) & {15, 16, 17, 127, 128, 129, 4095, 4096, 4097}
    assert set(range(4090, 4101)) <= got
    for n in got:                                     # every length mod 16 on either side of the LDS staging limit
        assert {r["role"] for r in c.rows if r["length"] == n} == {"A", "again", "prime"}
    assert {n % 16 for n in got if n <= MC.META_LDS_DN} == {n % 16 for n in got if MC.META_LDS_DN < n <= 160} == set(range(16))


def test_uri_lengths_reach_every_switch():
    c, ms = corpus("uri_lengths"), metas("uri_lengths")
    values = {f: {} for f in MC.URI_FORMS}            # form → extension value length → URI lengths
    for i, row in enumerate(c.rows):
        if row["kind"] == "uri":
            s, e = MC.crl_value_range(c.certs[i][0])
            values[row["form"]].setdefault(e - s, set()).add(row["length"])
    for form in MC.URI_FORMS:
        assert {r["length"] for r in c.rows if r["kind"] == "uri" and r["form"] == form} == set(MC.URI_SMALL + MC.URI_BIG)
        assert set(range(62, 67)) <= set(values[form])              # the value on either side of META_LDS_CRL
    # a value of 62..66 bytes: with the URI filling it but for the headers, and with a short URI in front of another
    at64 = {f: set().union(*(values[f][v] for v in range(62, 67))) for f in MC.URI_FORMS}
    assert min(at64["alone"]) >= 50 and max(at64["pair"]) < 40 and max(at64["second"]) < 30
    # the URI itself on either side of 64 and of 4096, in every form
    assert {r["length"] for r in c.rows if r["kind"] == "count"} == {4, 5}
    # the same item lies at another offset in its staged value from form to form
    where = {}
    for i, row in enumerate(c.rows):
        if row["kind"] == "uri" and row["role"] == "A" and row["length"] == 24:
            s, _ = MC.crl_value_range(c.certs[i][0])
            where[row["form"]] = ms[i][2].crl_off[1 if row["form"] == "second" else 0] - s
    assert len(set(where.values())) >= 2


@pytest.mark.parametrize("which", [None, "first", "second"])
def test_the_sweep_ends_inside_and_beyond_the_window(which):
    c = corpus("uri_lengths")
    wb = MC.window_bytes()
    assert wb == {"fast": 216, "reference": 224}      # WinGeo<13>, WinGeo<14> (kernels/readers.h)
    for profile, margins in MC.sweep_margins(c, which).items():
        got = set(margins.values())
        assert set(range(-24, 40)) <= got, profile    # less than 8 bytes before the window's end: 0..7; crossing it: < 0


def test_the_second_part_brings_nothing_the_first_did_not():
    for which in ("name_lengths", "uri_lengths", "addresses"):
        c = corpus(which)
        seen = {}
        for part in ("first", "second"):
            ders, idx, _ = c.part(part)
            hours = [orc.exp_hour(orc.parse_cert(d).not_after) for d in ders]
            seen[part] = {k for k in MC.expected_first_sightings(ders, idx, range(len(ders)), hours) if k[0] != N.MK_HOST}
        assert seen["second"] and seen["second"] <= seen["first"], which


def test_addresses_reach_all_sixteen_residues():
    c = corpus("addresses")
    assert {r["length"] for r in c.rows if r["kind"] == "address"} == set(MC.ADDRESS_LENGTHS)
    serial_lens = set()
    for der, _ in c.certs:
        serial_lens.add(orc.parse_cert(der).serial_len)
    assert set(range(1, 17)) <= serial_lens
    assert any(r["kind"] == "filler" for r in c.rows)
    for part in (None, "first", "second"):
        res = MC.item_residues(c, part)
        assert set(res) == {(k, n) for k in ("name", "uri") for n in MC.ADDRESS_LENGTHS}
        for key, got in res.items():
            assert got == set(range(16)), (part, key)
    # an item and its prime, 16 sightings each per segment
    ms = metas("addresses")
    for group, roles in triples(c).items():
        if group[0] != "address":
            continue
        idx = [i for v in roles.values() for i in v]
        assert len(idx) == 32 and len({item(c, ms, i)[0] for i in idx}) == 1


def test_crowd_items_are_pairwise_distinct():
    c = corpus("crowd")
    us = [u for _, uris, _ in metas("crowd") for u in uris]
    assert len(us) == 2000 == len(set(us)) and len(c.certs) == 1000
    assert len({MC.crowd_uri(k) for k in range(60000)}) == 60000
    assert len({len(u) for u in us}) >= 3 and {i for _, i in c.certs} == set(range(MC.CROWD_ISSUERS))
    # one Name and one hour per issuer: two items per certificate, under the first buffer of 3·n + 1024
    assert len({(i, m[0]) for (_, i), m in zip(c.certs, metas("crowd"))}) == MC.CROWD_ISSUERS
    more = MC.crowd(100, start=2000, tag=1)
    assert not {u for r in more.rows for u in r["uris"]} & set(us)
    assert not {d for d, _ in more.certs} & {d for d, _ in c.certs}


OVERFLOW_MUCH_SHARED = dict(n_big=1000, n_small=200, small_uris=4)


@pytest.mark.parametrize("much_shared", [False, True])
def test_overflow_brings_more_items_than_the_first_buffer_holds(much_shared):
    c = MC.overflow(**OVERFLOW_MUCH_SHARED) if much_shared else corpus("overflow")
    small, big = c.part("first"), c.part("second")
    n = len(big[0])
    assert n >= 400 and 0 < len(small[0]) < n
    hours = lambda ders: [orc.exp_hour(orc.parse_cert(d).not_after) for d in ders]
    exp_small = MC.expected_first_sightings(small[0], small[1], range(len(small[0])), hours(small[0]))
    exp_big = MC.expected_first_sightings(big[0], big[1], range(n), hours(big[0]))
    assert len(exp_big) > 3 * n + 1024
    shared = exp_small & exp_big
    assert {k[0] for k in shared} == {N.MK_EXPDATE, N.MK_DN, N.MK_CRL}
    # with the small batch's items in the memo the first run still overflows, and the cold run fits the second buffer
    # … or, with more shared items than the second buffer's slack of 1024, does not: a third run has to
    assert len(exp_big - exp_small) > 3 * n + 1024 and (len(exp_big) > len(exp_big - exp_small) + 1024) == much_shared
    assert len(exp_small) <= 3 * len(small[0]) + 1024             # the small batch itself fits
    assert sum(r["kind"] == "seen" for r in big[2]) >= 10
    assert not any(k[0] == N.MK_HOST for k in exp_big | exp_small)
