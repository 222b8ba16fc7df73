"""tests/calendar_corpus.py held to what it promises, and its plain-Python reference (datetime) held against the oracle,
the host build of the walk (csrc/der_walk.h rd_time) and known_image's key text — without a GPU.  The lists of years,
instants and zones are written out again here, so that a case dropped from the corpus fails a test."""
import itertools
import time
from datetime import datetime, timezone

from ct_mapreduce_amd import known_image as KI
from oracle import oracle as orc
from tests import calendar_corpus as K, harness

YEARS = (0, 1, 4, 100, 400, 1599, 1600, 1899, 1900, 1901, 1938, 1949, 1950, 1966, 1969, 1970, 1999, 2000, 2001, 2023, 2024,
         2038, 2049, 2050, 2089, 2099, 2100, 2106, 2286, 2400, 9999)
ZONES = ("+0001", "-0001", "+0059", "+0100", "-0100", "+0530", "-0800", "+1400", "+2359", "+9900", "-9900")
EDGE_HOURS = (1048575, 1048576, 277777, 277778, 2777777, 2777778, -27777, -27778, -277777, -277778, -2777777, -2777778)


def unix(y, mo, d, h=0, mi=0, s=0):
    return int(datetime(y, mo, d, h, mi, s, tzinfo=timezone.utc).timestamp())


def fields(c):
    """(year, month, day, H, M, S) as a grid case's content spells them."""
    t = c.content.decode()
    if c.tag == 0x18:
        y, t = int(t[:4]), t[4:]
    else:
        y, t = (2000 if int(t[:2]) < 50 else 1900) + int(t[:2]), t[2:]
    return (y,) + tuple(int(t[i:i + 2]) for i in range(0, 10, 2))


# ------------------------------------------------------------------------------------------------ the reference itself
def test_the_reference_is_datetime():
    assert K.parse_time(0x17, b"270101000000Z") == (True, unix(2027, 1, 1))
    assert K.parse_time(0x18, b"20380119031408Z") == (True, 1 << 31) and K.parse_time(0x18, b"21060207062816Z") == (True, 1 << 32)
    assert K.parse_time(0x17, b"491231235959-0100") == (True, unix(2050, 1, 1, 0, 59, 59))
    assert K.parse_time(0x17, b"500101000000+0100") == (True, unix(1949, 12, 31, 23))
    assert K.parse_time(0x18, b"00010101000000Z") == (True, unix(1, 1, 1))
    assert K.parse_time(0x18, b"00000101000000Z") == (True, unix(1, 1, 1) - 366 * 86400)      # year 0000 is a leap year
    assert K.parse_time(0x18, b"00000229000000Z")[0] and not K.parse_time(0x18, b"01000229000000Z")[0]
    assert K.hour_of(-1) == -1 and K.hour_of(-3600) == -1 and K.hour_of(-3601) == -2 and K.hour_of(3599) == 0
    assert K.date_id(0) == "1970-01-01-00" and K.date_id(-1) == "1969-12-31-23"
    assert K.date_id(1048575) == "2089-08-14-15" and K.date_id(1048576) == "2089-08-14-16"
    assert K.date_id(277778)[:10] == "2001-09-09" and K.date_id(2777778)[:10] == "2286-11-20"
    assert K.date_id(-27778)[:4] == "1966" and K.date_id(-277778)[:10] == "1938-04-24" and K.date_id(-2777778)[:10] == "1653-02-10"
    assert K.date_id(K.HOUR_MIN) == "0000-01-01-00" and K.date_id(K.HOUR_MAX) == "9999-12-31-23"
    assert K.date_id(K.hour_of(unix(1, 1, 1)) - 1) == "0000-12-31-23"
    for h in (K.HOUR_MIN - 1, K.HOUR_MAX + 1):
        try:
            K.date_id(h)
            assert False, h
        except ValueError:
            pass


# ------------------------------------------------------------------------------------------------ coverage
def test_the_grid_holds_every_valid_cell_and_every_cell_one_step_outside():
    grid = K.families()["grid"]
    assert len(grid) < 15000
    seen = {(c.tag,) + fields(c): c for c in grid}
    assert len(seen) == len(grid)
    assert {(k[1], k[2]) for k in seen if k[0] == 0x18} == set(itertools.product(YEARS, range(14)))
    days, tods = (0, 1, 28, 29, 30, 31, 32), ((0, 0, 0), (23, 59, 59), (24, 0, 0), (0, 60, 0), (0, 0, 60))
    assert {k[3] for k in seen} == set(days) and {k[4:] for k in seen} == set(tods)
    n_valid = n_step = 0
    for y in YEARS:
        tags = (0x18, 0x17) if 1950 <= y <= 2049 else (0x18,)
        assert {k[0] for k in seen if k[1] == y} == set(tags), y
        for m in range(1, 13):
            dim = K.days_in_month(y, m)
            nxt = min(d for d in days if d > dim)
            for tag in tags:
                for d in days:
                    for tod in tods:
                        good_day, good_tod = 1 <= d <= dim, tod in tods[:2]
                        if good_day and good_tod:
                            assert seen[(tag, y, m, d) + tod].ok, (y, m, d, tod)
                            n_valid += 1
                        elif (good_day and not good_tod) or (d in (0, nxt) and good_tod):   # one of the two out, by one step
                            assert not seen[(tag, y, m, d) + tod].ok, (y, m, d, tod)
                            n_step += 1
        for m in (0, 13):                               # the month alone out of range: every day that some month has
            for tag in tags:
                for d in (1, 28, 29, 30, 31):
                    for tod in tods[:2]:
                        assert not seen[(tag, y, m, d) + tod].ok, (y, m, d, tod)
                        n_step += 1
    assert n_valid == sum(c.ok for c in grid)
    assert sum(k[0] == 0x17 and seen[k].ok for k in seen) > 1000
    print("grid: %d cases, %d valid, %d one step outside, %d further out" % (len(grid), n_valid, n_step, len(grid) - n_valid - n_step))


def test_the_instants_are_all_there():
    inst = K.families()["instants"]
    assert all(c.ok for c in inst)
    have = {c.not_after for c in inst}
    first, last = unix(1, 1, 1) - 366 * 86400, unix(9999, 12, 31, 23, 59, 59)
    named = [0, 1 << 31, 1 << 32, first, last] + [h * 3600 for h in EDGE_HOURS]
    for t in named:
        h = t // 3600
        for s in (t - 1, t, t + 1, h * 3600 - 1, h * 3600, h * 3600 + 3599, (h + 1) * 3600):
            assert (s in have) == (first <= s <= last), (t, s)
    hours = {c.hour for c in inst}
    assert set(EDGE_HOURS) <= hours and {h - 1 for h in EDGE_HOURS} <= hours and {-1, 0, 1, K.HOUR_MIN, K.HOUR_MAX} <= hours
    assert {c.tag for c in inst} == {0x17, 0x18}
    by = {(c.tag, c.not_after) for c in inst}
    assert (0x17, 0) in by and (0x17, -1) in by and (0x17, 1 << 31) in by and (0x17, 277778 * 3600) in by and (0x17, -27778 * 3600) in by


def test_the_zones_carry_where_they_say():
    zones = K.families()["zones"]
    ok = [c for c in zones if c.ok]
    for z in ZONES:
        for tag, secs in ((0x18, 14), (0x17, 12), (0x17, 10)):
            assert any(c.tag == tag and c.content[secs:] == z.encode() for c in ok), (z, tag, secs)
    assert any(c.tag == 0x17 and c.content[10:] == b"Z" for c in ok)
    local = lambda c: K.parse_time(c.tag, c.content[:-5] + b"Z")[1] if c.content[-5:-4] in b"+-" else c.not_after
    carried = {"hour": 3600, "day": 86400}
    for name, unit in carried.items():
        assert any(local(c) // unit > c.not_after // unit for c in ok) and any(local(c) // unit < c.not_after // unit for c in ok), name
    ids = {(K.date_id(local(c) // 3600)[:10], K.date_id(c.hour)[:10]) for c in ok}
    for a, b in (("2024-02-29", "2024-03-01"), ("2024-03-01", "2024-02-29"), ("2024-02-29", "2024-02-28"), ("2024-02-28", "2024-02-29"),
                 ("2023-02-28", "2023-03-01"), ("2023-03-01", "2023-02-28"), ("1900-02-28", "1900-03-01"), ("1900-03-01", "1900-02-28"),
                 ("2000-02-29", "2000-03-01"), ("2000-03-01", "2000-02-29"), ("2027-04-30", "2027-05-01"), ("2027-05-01", "2027-04-30"),
                 ("2026-12-31", "2027-01-01"), ("2027-01-01", "2026-12-31"), ("1969-12-31", "1970-01-01"), ("1970-01-01", "1969-12-31")):
        assert (a, b) in ids, (a, b)
    # the pivot is read in the local zone: a UTCTime of local year 49 that lies in 2050, one of local year 50 that lies in 1949
    assert any(c.tag == 0x17 and c.content[:2] == b"49" and K.date_id(c.hour)[:4] == "2050" for c in ok)
    assert any(c.tag == 0x17 and c.content[:2] == b"50" and K.date_id(c.hour)[:4] == "1949" for c in ok)
    assert any(c.hour < 0 for c in ok) and any(c.hour > 0 for c in ok) and any(c.not_after < 0 <= local(c) for c in ok)
    rejected = {c.content.decode() for c in zones if not c.ok}
    assert {"270101000000+0000", "270101000000-0000", "270101000000+0060", "270101000000+01", "270101000000+010",
            "270101000000+01000", "270101000000 0100", "270101000000+0a00", "270101000000z", "2701010000Z0", "27010100000Z",
            "270101000000.5Z", "270101000000+01:00", "20270101000000+0000", "202701010000Z", "202701010000+0100",
            "20270101000000+0160", "20270101000000", "20270101000000.0Z"} <= rejected
    oor = K.families()["out_of_range"]
    assert {c.content[14:].decode() for c in oor if c.ok} == set(ZONES)
    assert all(not K.in_range(c.hour) for c in oor if c.ok)
    assert any(c.hour < K.HOUR_MIN for c in oor if c.ok) and any(c.hour > K.HOUR_MAX for c in oor if c.ok)
    assert {K.HOUR_MIN - 1, K.HOUR_MAX + 1} <= {c.hour for c in oor if c.ok}              # ±0001: the first hour outside


def test_the_shapes_and_name_values_are_all_there():
    shapes = K.families()["shapes"]
    by = {(c.tag, c.content): c for c in shapes}
    for tag, base, nd in ((0x17, b"2701010000Z", 10), (0x17, b"270101000000Z", 12), (0x18, b"20270101000000Z", 14)):
        assert by[(tag, base)].ok
        for p in range(nd):
            for x in (0x2f, 0x3a, 0x00, base[p] | 0x80):
                assert not by[(tag, base[:p] + bytes([x]) + base[p + 1:])].ok, (base, p, x)
        assert not by[(tag, base[:nd - 1] + b"Z")].ok and not by[(tag, base[:nd] + b"0Z")].ok
        for other in {0x16, 0x17, 0x18} - {tag}:
            assert not by[(other, base)].ok
    nv = K.families()["name_values"]
    assert 50 <= len(nv) <= 80
    for where in ("subject", "issuer"):
        mine = [c for c in nv if c.where == where]
        assert {(c.tag, c.ok) for c in mine} == {(0x17, True), (0x17, False), (0x18, True), (0x18, False)}
        assert all(c.not_after == unix(2027, 1, 1) for c in mine if c.ok)
    nb = K.families()["not_before"]
    assert len(nb) * 10 >= len(K.cases("grid", "zones")) and all(c.where == "not_before" for c in nb)
    assert len({c.not_before for c in nb if c.ok}) > 300 and all(c.not_after == unix(2027, 1, 1) for c in nb if c.ok)


def test_every_family_accepts_and_rejects_and_no_certificate_comes_twice():
    fam = K.families()
    assert tuple(fam) == ("grid", "instants", "zones", "out_of_range", "shapes", "name_values", "not_before")
    for name, cs in fam.items():
        assert all(c.family == name for c in cs)
        assert any(c.ok for c in cs), name
        assert name == "instants" or any(not c.ok for c in cs), name          # an instant is a time that exists
        assert {c.iss for c in cs} == {0, 1}, name
    every = K.cases()
    assert len({c.der for c in every}) == len(every) and len({c.der[:40] for c in every}) == len(every)   # (the serial lies in front)
    ok = [c for c in every if c.ok]
    assert {c.tag for c in ok} == {0x17, 0x18} and any(c.hour < 0 for c in ok) and any(c.hour > 0 for c in ok) and any(c.hour == 0 for c in ok)
    assert all(len(c.der) < 400 for c in every)
    print("corpus: " + ", ".join("%s %d" % (n, len(cs)) for n, cs in fam.items()) + "; %d certificates, %d bytes" %
          (len(every), sum(len(c.der) for c in every)))


# ------------------------------------------------------------------------------------------------ against the project
def test_the_oracle_and_the_host_build_of_the_walk_agree_with_datetime():
    t0 = time.perf_counter()
    diffs = []
    for c in K.cases():
        for who, got in (("oracle", orc.parse_cert(c.der)), ("walk", harness.product_walk(c.der))):
            if bool(got.ok) != c.ok:
                diffs.append("%s: %s %s: ok %d, the reference says %d" % (who, c.family, c.label, got.ok, c.ok))
            elif c.ok and (got.not_after, got.not_before) != (c.not_after, c.not_before):
                diffs.append("%s: %s %s: (%d, %d), the reference says (%d, %d)" % (who, c.family, c.label, got.not_after, got.not_before,
                                                                                c.not_after, c.not_before))
    print("%d cases through the oracle and the walk, %.2f s" % (len(K.cases()), time.perf_counter() - t0))
    assert not diffs, "%d differences\n" % len(diffs) + "\n".join(diffs[:40])


def test_hours_and_key_text_agree_with_datetime_both_ways_round():
    ok = [c for c in K.cases() if c.ok]
    for c in ok:
        assert orc.exp_hour(c.not_after) == c.hour == K.hour_of(c.not_after), c.label
    hours = sorted({c.hour for c in ok} | {K.hour_of(c.not_before) for c in ok})
    inside = [h for h in hours if K.in_range(h)]
    assert len(inside) > 2000 and len(hours) - len(inside) >= 8           # (+0001, +0059 and +0100 share the last hour of year −1)
    digest = bytes(range(32))
    for h in inside:
        want = K.date_id(h)
        assert orc.exp_date_id(h) == want, h
        assert KI.exp_date_id(h) == want.encode(), h
        key = b"serials::" + want.encode() + b"::" + KI.issuer_id(digest)
        assert KI.set_key(h, digest) == key and KI.parse_key(key) == (h, digest), h
    print("%d accepted cases, %d distinct hours, %d of them in 0000..9999" % (len(ok), len(hours), len(inside)))
