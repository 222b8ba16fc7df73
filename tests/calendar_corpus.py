"""The dates the engine reads, keeps and writes, held to Python's datetime.  No GPU, no torch, nothing of the project but the
DER encoder (tests/der.py): the reference below calls neither the oracle nor known_image nor the package.

The reference restates the rules written above rd_time (csrc/der_walk.h) — Go's asn1.parseUTCTime / parseGeneralizedTime —
in plain Python and takes the calendar itself from datetime:

  parse_time(tag, content) → (ok, unix seconds)   tag 0x17 "YYMMDDHHMM[SS]" + zone, tag 0x18 "YYYYMMDDHHMMSS" + zone; zone "Z" or
                                                  ±hhmm with mm <= 59 and not ±0000, hh any two digits; digits only, no fraction;
                                                  a UTCTime year yy < 50 is 20yy, else 19yy, read in the time's own zone
  hour_of(seconds)                                seconds // 3600, Python's floor
  date_id(hour)                                   ExpDate.ID "YYYY-MM-DD-HH"; defined for the hours of the years 0000..9999 only

datetime has no year 0000: that year is read as year 0400 (the Gregorian calendar repeats every 400 years = 146 097 days,
and both are leap years) and 146 097 days are taken off.

A case carries its DER (a distinct serial each, one of two issuers) and the reference's verdict.  Families:

  grid          31 years × months 00..13 × days 00 01 28 29 30 31 32 × five times of day, as GeneralizedTime and, for 1950..2049,
                as UTCTime.  Every valid cell; every cell with exactly ONE field out of range (month 00 / 13, day 00 / last + 1 …
                32, 24:00:00, 00:60:00, 00:00:60); of the cells with two or more fields out of range every THIN-th.  The
                valid cells are 4 470 and the cells one step outside 9 561, so the family has 14 256 certificates (4 MB):
                keeping all of both was chosen over a smaller family, and the device tests still take under a second each
  instants      the second before, at and behind the epoch, 2^31 s, 2^32 s, the IssuerMetadata bitmap's last hour and the first
                beyond it, the hours at which EXPIREAT gains a character, the first second of 0000 and the last of 9999 — and
                mm:ss 59:59 / 00:00 on both sides of each of those hours
  zones         eleven numeric offsets on local times from which the offset carries over an hour, a day, a month end, Feb 28 /
                29 of 2024, 2023, 1900 and 2000, a year end, the UTCTime pivot and the epoch; the layout without seconds; the
                rejected forms of tests/test_der_edge_cpu.py::test_time_zone_offsets
  out_of_range  accepted times whose hour lies outside 0000..9999 (year 0000 with a positive offset, 9999 with a negative
                one): no ExpDate.ID spells them
  shapes        a non-digit (0x2f, 0x3a, 0x00, a digit with bit 7 set) at each digit position of the three layouts, lengths
                one short and one long, the tags 0x16 / 0x17 / 0x18 over a content of another kind
  name_values   times (valid and not, both tags) as the value of a subject and of an issuer attribute: the Name, and with it
                the certificate, parses only when the time does; notAfter stays ordinary
  not_before    a tenth of grid and zones on notBefore, with an ordinary notAfter

tests/test_calendar_corpus_cpu.py holds the corpus to these promises and the reference to the oracle and to the host
build of the walk; tests/test_gpu_calendar.py runs the cases on the device."""
import base64
import hashlib
import random
from collections import namedtuple
from datetime import datetime, timedelta

from tests import der as D

SEED = 20261020
EPOCH = datetime(1970, 1, 1)
ERA_DAYS = 146097                                  # 400 Gregorian years


# ------------------------------------------------------------------------------------------------ the reference
def is_leap(y):
    return y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)


def days_in_month(y, m):
    return 29 if m == 2 and is_leap(y) else (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)[m - 1]


def civil_seconds(y, m, d, H, M, S):
    """Seconds from the epoch to y-m-d H:M:S of the proleptic Gregorian calendar, by datetime (0 <= y <= 9999)."""
    shift = 0
    if y == 0:
        y, shift = 400, ERA_DAYS
    t = datetime(y, m, d, H, M, S) - EPOCH
    return (t.days - shift) * 86400 + t.seconds


def _digits(b):
    return all(0x30 <= x <= 0x39 for x in b)


def _zone(z):
    """b"Z" or ±hhmm → (ok, offset in seconds east of UTC)."""
    if z == b"Z":
        return True, 0
    if len(z) != 5 or z[0:1] not in (b"+", b"-") or not _digits(z[1:]):
        return False, 0
    hh, mm = int(z[1:3]), int(z[3:5])
    if mm > 59 or (hh == 0 and mm == 0):
        return False, 0
    off = hh * 3600 + mm * 60
    return True, -off if z[0:1] == b"-" else off


def parse_time(tag, content):
    """(ok, unix seconds) of a UTCTime (0x17) or GeneralizedTime (0x18) value; (False, None) for anything else."""
    content = bytes(content)
    layouts = {0x17: (10, 12), 0x18: (14,)}.get(tag, ())
    for nd in layouts:                              # the layout without seconds is tried first; at most one can fit
        body, zone = content[:nd], content[nd:]
        if len(body) != nd or not _digits(body):
            continue
        zok, off = _zone(zone)
        if not zok:
            continue
        f = [int(body[i:i + 2]) for i in range(0, nd, 2)]
        if tag == 0x18:
            year, f = f[0] * 100 + f[1], f[2:]
        else:
            year, f = (2000 + f[0] if f[0] < 50 else 1900 + f[0]), f[1:]
        mon, day, H, M = f[0], f[1], f[2], f[3]
        S = f[4] if len(f) > 4 else 0
        if not (1 <= mon <= 12 and 1 <= day <= days_in_month(year, mon) and H <= 23 and M <= 59 and S <= 59):
            return False, None
        return True, civil_seconds(year, mon, day, H, M, S) - off
    return False, None


def hour_of(seconds):
    return seconds // 3600


HOUR_MIN = hour_of(civil_seconds(0, 1, 1, 0, 0, 0))          # 0000-01-01-00
HOUR_MAX = hour_of(civil_seconds(9999, 12, 31, 23, 0, 0))    # 9999-12-31-23


def in_range(hour):
    return HOUR_MIN <= hour <= HOUR_MAX


def civil_of(seconds):
    """(y, m, d, H, M, S) of an instant of the years 0000..9999, by datetime."""
    shift = 0
    if seconds < civil_seconds(1, 1, 1, 0, 0, 0):
        seconds, shift = seconds + ERA_DAYS * 86400, 400
    t = EPOCH + timedelta(seconds=seconds)
    return t.year - shift, t.month, t.day, t.hour, t.minute, t.second


def date_id(hour):
    if not in_range(hour):
        raise ValueError("hour %d lies outside the years 0000..9999" % hour)
    y, m, d, H, _, _ = civil_of(hour * 3600)
    return "%04d-%02d-%02d-%02d" % (y, m, d, H)


# ------------------------------------------------------------------------------------------------ issuers, certificates
ISSUER_NAMES = [D.name(D.rdn(3, b"Calendar CA A")), D.name(D.rdn(3, b"Calendar CA B"))]
ISSUERS = [D.cert(serial=b"\x01", subject=ISSUER_NAMES[0], issuer=ISSUER_NAMES[0], spki=D.rsa_spki(n=b"\x00" + b"\xc3" * 256), exts=[D.BC_CA]),
           D.cert(serial=b"\x02", subject=ISSUER_NAMES[1], issuer=ISSUER_NAMES[1], spki=D.rsa_spki(n=b"\x00" + b"\xc5" * 256), exts=[D.BC_CA])]
ISSUER_SPKIS = [D.rsa_spki(n=b"\x00" + b"\xc3" * 256), D.rsa_spki(n=b"\x00" + b"\xc5" * 256)]
# Issuer.ID: the padded base64url of the SHA-256 of the SubjectPublicKeyInfo
ISSUER_IDS = [base64.urlsafe_b64encode(hashlib.sha256(s).digest()).decode() for s in ISSUER_SPKIS]


def set_name(hour, iss):
    """The key of the set a certificate of that expiry hour and issuer belongs to, by the reference."""
    return ("serials::%s::%s" % (date_id(hour), ISSUER_IDS[iss])).encode()


ORDINARY = (0x17, b"270101000000Z")              # the notAfter of the cases whose subject lies elsewhere
ORDINARY_BEFORE = (0x17, b"250101000000Z")

# where: the field that carries the time (not_after | not_before | subject | issuer); ok: the reference's verdict on the
# CERTIFICATE; not_after / not_before / hour: the reference's values when ok (hour = hour_of(not_after))
Case = namedtuple("Case", "family label der iss serial where tag content ok not_after not_before hour")
_serial = [0]


def make(family, label, tag, content, where="not_after", iss=None):
    _serial[0] += 1
    k = _serial[0]
    iss = k & 1 if iss is None else iss
    serial = b"\x4c" + k.to_bytes(3, "big")
    content = bytes(content)
    kw = {"issuer": ISSUER_NAMES[iss]}
    na, nb = ORDINARY, ORDINARY_BEFORE
    if where == "not_after":
        na = (tag, content)
    elif where == "not_before":
        nb = (tag, content)
    elif where == "subject":
        kw["subject"] = D.name(D.rdn(3, b"leaf"), D.rdn(10, content, tag))
    else:
        kw["issuer"] = D.name(D.rdn(10, content, tag), D.rdn(3, b"Calendar CA " + b"AB"[iss:iss + 1]))
    der = D.cert(serial=serial, not_before=D.tlv(*nb), not_after=D.tlv(*na), **kw)
    ok_v, _ = parse_time(tag, content)
    ok_a, t_a = parse_time(*na)
    ok_b, t_b = parse_time(*nb)
    ok = ok_v and ok_a and ok_b
    return Case(family, label, der, iss, serial, where, tag, content, ok, t_a if ok else None, t_b if ok else None,
                hour_of(t_a) if ok else None)


def fmt(tag, y, m, d, H, M, S, zone=b"Z", seconds=True):
    """The fields as text, in range or not (two digits each, four for a GeneralizedTime's year)."""
    s = ("%04d" % y if tag == 0x18 else "%02d" % (y % 100)) + "%02d%02d%02d%02d" % (m, d, H, M) + ("%02d" % S if seconds else "")
    return s.encode() + zone


def utc_year(y):
    return 1950 <= y <= 2049


# ------------------------------------------------------------------------------------------------ grid
GRID_YEARS = (0, 1, 4, 100, 400, 1599, 1600, 1899, 1900, 1901, 1938, 1949, 1950, 1966, 1969, 1970, 1999, 2000, 2001, 2023,
              2024, 2038, 2049, 2050, 2089, 2099, 2100, 2106, 2286, 2400, 9999)
GRID_MONTHS = tuple(range(14))
GRID_DAYS = (0, 1, 28, 29, 30, 31, 32)
GRID_TIMES = ((0, 0, 0), (23, 59, 59), (24, 0, 0), (0, 60, 0), (0, 0, 60))
THIN = 29                                          # of the cells with two or more fields out of range: every 29th


def grid_wrong_fields(y, m, d, tod):
    """How many of (month, day, time of day) are out of range, and whether each is the nearest listed step outside: a day
    behind the month's last counts as one step only when it is the first listed day behind it."""
    wrong = 0
    if not 1 <= m <= 12:
        wrong += 1
        if not 1 <= d <= 31:                        # no month to judge the day by: 00 and 32 are out for every month
            wrong += 1
    else:
        dim = days_in_month(y, m)
        if d == 0 or d == min(x for x in GRID_DAYS if x > dim):
            wrong += 1
        elif d > dim:
            wrong += 2                              # further out than the first step
    if tod[0] > 23 or tod[1] > 59 or tod[2] > 59:
        wrong += 1
    return wrong


def grid_cells():
    """(year, month, day, time of day, fields out of range) of every cell that is kept."""
    k = 0
    for y in GRID_YEARS:
        for m in GRID_MONTHS:
            for d in GRID_DAYS:
                for tod in GRID_TIMES:
                    w = grid_wrong_fields(y, m, d, tod)
                    if w >= 2:
                        k += 1
                        if k % THIN:
                            continue
                    yield y, m, d, tod, w


def family_grid():
    out = []
    for y, m, d, tod, w in grid_cells():
        for tag in (0x18, 0x17):
            if tag == 0x17 and not utc_year(y):
                continue
            out.append(make("grid", "%04d-%02d-%02d %02d:%02d:%02d %s" % ((y, m, d) + tod + ("gt" if tag == 0x18 else "utc",)),
                            tag, fmt(tag, y, m, d, *tod)))
    return out


# ------------------------------------------------------------------------------------------------ instants
BITMAP_HOURS = (1048575, 1048576)                  # META_HOUR_BITS = 2^20: the last hour of the bitmap and the first behind it
DIGIT_HOURS = (277777, 277778, 2777777, 2777778, -27777, -27778, -277777, -277778, -2777777, -2777778)
INSTANTS = {"epoch": 0, "2^31": 1 << 31, "2^32": 1 << 32, "year_0000_first": civil_seconds(0, 1, 1, 0, 0, 0),
            "year_9999_last": civil_seconds(9999, 12, 31, 23, 59, 59)}
INSTANTS.update({"hour_%d" % h: h * 3600 for h in BITMAP_HOURS + DIGIT_HOURS})
FIRST_SECOND, LAST_SECOND = INSTANTS["year_0000_first"], INSTANTS["year_9999_last"]


def instant_seconds():
    """name → the seconds asked of it: T − 1, T, T + 1, and 59:59 / 00:00 on both sides of T's hour."""
    out = {}
    for name, t in INSTANTS.items():
        h = t // 3600
        want = [t - 1, t, t + 1, h * 3600 - 1, h * 3600, h * 3600 + 3599, (h + 1) * 3600]
        out[name] = sorted({s for s in want if FIRST_SECOND <= s <= LAST_SECOND})
    return out


def family_instants():
    out, seen = [], set()
    for name, secs in instant_seconds().items():
        for s in secs:
            if s in seen:
                continue
            seen.add(s)
            f = civil_of(s)
            for tag in (0x18, 0x17):
                if tag == 0x17 and not utc_year(f[0]):
                    continue
                c = make("instants", "%s %+d" % (name, s - INSTANTS[name]), tag, fmt(tag, *f))
                assert c.ok and c.not_after == s, (name, s)
                out.append(c)
    return out


# ------------------------------------------------------------------------------------------------ zones
ZONES = ("+0001", "-0001", "+0059", "+0100", "-0100", "+0530", "-0800", "+1400", "+2359", "+9900", "-9900")
# local midnights (and the hour of an ordinary day): one second before and at each, every offset, carries the instant over
# an hour, a day, a month end, the end of February in leap and common years, a year end, the UTCTime pivot and the epoch
ZONE_EDGES = {"hour": (2027, 3, 10, 12), "day": (2027, 3, 10, 0), "month": (2027, 5, 1, 0), "feb_2024": (2024, 3, 1, 0),
              "feb_2023": (2023, 3, 1, 0), "feb_1900": (1900, 3, 1, 0), "feb_2000": (2000, 3, 1, 0), "feb29_2024": (2024, 2, 29, 0),
              "year": (2027, 1, 1, 0), "pivot_2050": (2050, 1, 1, 0), "pivot_1950": (1950, 1, 1, 0), "epoch": (1970, 1, 1, 0)}
ZONE_REJECTED_UTC = ("270101000000+0000", "270101000000-0000", "270101000000+0060", "270101000000+01", "270101000000+010",
                     "270101000000+01000", "270101000000 0100", "270101000000+0a00", "270101000000z", "2701010000Z0",
                     "27010100000Z", "270101000000.5Z", "270101000000+01:00", "2701010000+0000", "2701010000+0160")
ZONE_REJECTED_GT = ("20270101000000+0000", "202701010000Z", "202701010000+0100", "20270101000000+0160", "20270101000000",
                    "20270101000000.0Z", "20270101000000-0000", "20270101000000+0099")


def family_zones():
    out = []
    for name, (y, m, d, H) in ZONE_EDGES.items():
        at = civil_seconds(y, m, d, H, 0, 0)
        for local in (at - 1, at):
            f = civil_of(local)
            for z in ZONES + ("Z",):
                forms = [(0x18, True)]
                if utc_year(f[0]):
                    forms += [(0x17, True), (0x17, False)]
                for tag, secs in forms:
                    c = make("zones", "%s %+d %s %s%s" % (name, local - at, z, "gt" if tag == 0x18 else "utc", "" if secs else " no seconds"),
                             tag, fmt(tag, *f, zone=z.encode(), seconds=secs))
                    assert c.ok, c.label
                    out.append(c)
    for s in ZONE_REJECTED_UTC:
        out.append(make("zones", "rejected utc " + s, 0x17, s.encode()))
    for s in ZONE_REJECTED_GT:
        out.append(make("zones", "rejected gt " + s, 0x18, s.encode()))
    assert not any(c.ok for c in out[-len(ZONE_REJECTED_UTC) - len(ZONE_REJECTED_GT):])
    return out


def family_out_of_range():
    out = []
    for z in ZONES:
        f = (0, 1, 1, 0, 0, 0) if z[0] == "+" else (9999, 12, 31, 23, 59, 59)
        c = make("out_of_range", "%04d %s" % (f[0], z), 0x18, fmt(0x18, *f, zone=z.encode()))
        assert c.ok and not in_range(c.hour), c.label
        out.append(c)
    # … and their neighbours that no parser may let through to such an hour: minute 60 in the zone, second 60 in the time
    out.append(make("out_of_range", "0000 +0060", 0x18, b"00000101000000+0060"))
    out.append(make("out_of_range", "9999 :60 -0001", 0x18, b"99991231235960-0001"))
    assert not out[-1].ok and not out[-2].ok
    return out


# ------------------------------------------------------------------------------------------------ shapes
SHAPE_BASES = ((0x17, b"2701010000Z", 10), (0x17, b"270101000000Z", 12), (0x18, b"20270101000000Z", 14),
               (0x17, b"270101000000+0100", 12), (0x18, b"20270101000000-0100", 14))
NON_DIGITS = (0x2f, 0x3a, 0x00, None)              # None: the digit itself with bit 7 set


def family_shapes():
    out = []
    for tag, base, nd in SHAPE_BASES:
        out.append(make("shapes", "base %s" % base.decode(), tag, base))
        assert out[-1].ok
        if base[nd:] != b"Z":
            continue
        for p in range(nd):
            for x in NON_DIGITS:
                b = bytearray(base)
                b[p] = x if x is not None else b[p] | 0x80
                out.append(make("shapes", "%s octet %d = %02x" % (base.decode(), p, b[p]), tag, b))
        for label, b in (("a digit short", base[:nd - 1] + base[nd:]), ("a digit long", base[:nd] + b"0" + base[nd:]),
                         ("no zone", base[:nd]), ("an octet long", base + b"Z"), ("empty", b"")):
            out.append(make("shapes", "%s %s" % (base.decode(), label), tag, b))
        for other in (0x16, 0x17, 0x18):
            if other != tag:
                out.append(make("shapes", "%s under tag %02x" % (base.decode(), other), other, base))
    assert sum(c.ok for c in out) == len(SHAPE_BASES), [c.label for c in out if c.ok]
    return out


# ------------------------------------------------------------------------------------------------ name_values
NAME_VALUES = ((0x17, b"270101000000Z"), (0x17, b"2701010000Z"), (0x18, b"20270101000000Z"), (0x18, b"00000101000000Z"),
               (0x18, b"99991231235959Z"), (0x18, b"20240229235959Z"), (0x17, b"240229235959Z"), (0x18, b"19000228000000Z"),
               (0x17, b"491231235959-0100"), (0x17, b"500101000000+0100"), (0x18, b"20270101000000+9900"), (0x17, b"2701010530+0530"),
               (0x18, b"19691231235959Z"), (0x18, b"20890814150000Z"), (0x18, b"00000101000000+1400"),
               (0x18, b"20230229000000Z"), (0x17, b"230229000000Z"), (0x18, b"19000229000000Z"), (0x18, b"21000229000000Z"),
               (0x18, b"20270431000000Z"), (0x18, b"20270100000000Z"), (0x18, b"20271301000000Z"), (0x18, b"20270101240000Z"),
               (0x17, b"270101006000Z"), (0x17, b"270101000060Z"), (0x17, b"270101000000+0000"), (0x18, b"20270101000000+0060"),
               (0x18, b"202701010000Z"), (0x17, b"27010100000/Z"), (0x18, b"2027010100000:Z"), (0x17, b"20270101000000Z"),
               (0x18, b"270101000000Z"), (0x17, b""), (0x18, b"20270101000000.0Z"))


def family_name_values():
    out = []
    for where in ("subject", "issuer"):
        for tag, content in NAME_VALUES:
            out.append(make("name_values", "%s %02x %s" % (where, tag, content.decode()), tag, content, where))
    return out


# ------------------------------------------------------------------------------------------------ everything
FAMILIES = ("grid", "instants", "zones", "out_of_range", "shapes", "name_values", "not_before")
_all = {}


def families():
    """family → its cases, built once (the tests share them and leave them unchanged)."""
    if not _all:
        _all["grid"] = family_grid()
        _all["instants"] = family_instants()
        _all["zones"] = family_zones()
        _all["out_of_range"] = family_out_of_range()
        _all["shapes"] = family_shapes()
        _all["name_values"] = family_name_values()
        _all["not_before"] = [make("not_before", c.label, c.tag, c.content, "not_before")
                              for c in (_all["grid"] + _all["zones"])[::10]]
        assert tuple(_all) == FAMILIES
    return _all


def cases(*names):
    fam = families()
    return [c for n in (names or FAMILIES) for c in fam[n]]


def shuffled(cs, salt=0):
    """The cases in a seeded shuffle (a list of its own)."""
    cs = list(cs)
    random.Random(SEED + salt).shuffle(cs)
    return cs
