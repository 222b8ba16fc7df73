"""Cases for the lookup of serials in a known image whatever their expiration date (test helper, no test): a known image
K, a probe image P, a `now`, and the hits expected for every probe — include/ctmr.h ctmr_known_image_find, DESIGN.md §25.

The expectation is worked out here from the Python lists the images are written from, with dicts and integers only: it
never goes through known_image.find (the twin under test in tests/test_find_corpus_cpu.py) nor through the images'
bytes.  Host keys get their date strings from `datetime`, so the calendar is not the twin's either.

`raw_image` writes an image exactly as given — members in the order given, repeats kept, pairs of the host section
that the member section could carry left where they are — because the call neither sorts nor deduplicates.

Families (`FAMILIES`: name → function returning [Case]):
  counts      0, 1, 63, 64, 65, 255, 256, 257 and 1 025 probes against 257 records, the same counts of records
              against 65 probes, and 1 025 × 1 025: one set of K spans several blocks, the rest are one-member sets
  hours       one issuer's serial under 1, 2 and 300 hours, hours before 1970 among them
  misses      another serial, one octet shorter, one longer ending in 00, "", 00 and 00 00, the same serial under
              another issuer, two issuers of P against one of K and the reverse
  lengths     every serial length 0..40 on both sides, in the mixes of tests/known_corpus.py
  now         the second before a set expires and the second it does, hours outside the years 0000..9999, INT64_MIN
  repeats     a record twice in an unsorted K, probes repeated in P, an issuer K does not name
  host        serials of 41..45 octets on both sides, a pair of K's host section the member section could carry met by a
              member record of P and the reverse, a day-resolution key, a date that does not parse
"""
import base64
import datetime
import struct
from dataclasses import dataclass, field

import numpy as np

from ct_mapreduce_amd import known_image as KI

import known_corpus as KC

INT64_MIN = -2 ** 63
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1025)
HOUR_LO = (datetime.date(1, 1, 1).toordinal() - 366 - datetime.date(1970, 1, 1).toordinal()) * 24   # 0000-01-01-00
HOUR_HI = (datetime.date(9999, 12, 31).toordinal() + 1 - datetime.date(1970, 1, 1).toordinal()) * 24  # 10000-01-01-00
H0 = 482136   # 2025-01-01-00


def digest(k):
    return bytes([(37 * k + 11) & 255]) + struct.pack("<I", k) * 7 + bytes([k & 255, 0x5A, 0xA5])


def ident(dg):
    return base64.urlsafe_b64encode(dg)


def hour_date(hour):
    """"2006-01-02-15" of an hour count inside the years 0001..9999, by datetime."""
    t = datetime.datetime(1970, 1, 1) + datetime.timedelta(hours=hour)
    return b"%04d-%02d-%02d-%02d" % (t.year, t.month, t.day, t.hour)


def host_key(hour, dg, day=False):
    """A host-section key of hour resolution, or of day resolution for the day `hour` lies in."""
    d = hour_date(hour)
    return b"serials::" + (d[:10] if day else d) + b"::" + ident(dg)


@dataclass
class Case:
    name: str
    known: bytes
    probes: bytes
    now: int
    hits: list          # (records, first_hour, last_hour) per member record of P
    host_hits: list     # … per host-section member of P
    notes: dict = field(default_factory=dict)


def raw_image(sets, host=()):
    """An image written as given.  sets: [(hour, digest, [members])], at most one per (hour, digest), written in key
    order with the members in the order given; host: [(key, member)], written sorted.
    → (bytes, [(digest, member)] per member record in image order, [(key, member)] per host member in section order)."""
    sets = sorted(sets, key=lambda s: KI.set_key(s[0], s[1]))
    host = sorted(set(host))
    digests = sorted({s[1] for s in sets})
    ordinal = {d: i for i, d in enumerate(digests)}
    set_part, first, order = [], 0, []
    for hour, dg, ms in sets:
        assert ms and all(len(m) <= KI.MAX_SERIAL for m in ms)
        set_part.append(KI._SET.pack(hour, ordinal[dg], first, len(ms)))
        first += len(ms)
        order += [(dg, bytes(m)) for m in ms]
    host_part = b"".join(struct.pack("<I", len(k)) + k + struct.pack("<I", len(m)) + m for k, m in host)
    meta = KI._HEADER.pack(KI.MAGIC, KI.VERSION, KI.HEADER_BYTES, len(digests), 0, len(sets), first, len(host_part),
                           len(host), 0) + b"".join(digests) + b"".join(set_part) + host_part
    meta += b"\0" * (-len(meta) % 64)
    rec = np.zeros(first, KI.MEMBER_DTYPE)
    if first:
        rec["len"] = np.fromiter((len(m) for _, m in order), np.uint64, first)
        rec["serial"] = np.frombuffer(b"".join(m.ljust(KI.MAX_SERIAL, b"\0") for _, m in order), np.uint8).reshape(first, KI.MAX_SERIAL)
    return meta + rec.tobytes(), order, host


def kept(hour, now):
    return HOUR_LO <= hour < HOUR_HI and now < (hour + 1) * 3600


def case(name, k_sets, p_sets, now, k_host=(), p_host=(), **notes):
    """k_host: [(key, member, hour or None, hours the key lasts)] — the hour the key's date spells, None when it does not
    parse; p_host: [(key, member, Issuer.ID)]."""
    held = {}
    for hour, dg, ms in k_sets:
        if kept(hour, now):
            for m in ms:
                held.setdefault((ident(dg), bytes(m)), []).append(hour)
    for key, m, hour, span in set(k_host):
        if hour is not None and now < (hour + span) * 3600:
            held.setdefault((key.split(b"::")[2], bytes(m)), []).append(hour)
    known, _, _ = raw_image(k_sets, [(k, m) for k, m, _, _ in k_host])
    probes, order, horder = raw_image(p_sets, [(k, m) for k, m, _ in p_host])
    id_of = {(k, m): i for k, m, i in p_host}

    def hit(i, m):
        hours = held.get((i, m), ())
        return (len(hours), min(hours), max(hours)) if hours else (0, 0, 0)
    return Case(name, known, probes, now, [hit(ident(dg), m) for dg, m in order], [hit(id_of[km], km[1]) for km in horder], notes)


def as_array(hits):
    out = np.zeros(len(hits), KI.HIT_DTYPE)
    for i, (n, lo, hi) in enumerate(hits):
        out[i] = (n, lo, hi, 0)
    return out


def _serials(rng, n, lo=1, hi=20):
    out = set()
    while len(out) < n:
        out.add(bytes(rng.integers(0, 256, size=int(rng.integers(lo, hi + 1)), dtype=np.uint8).tolist()))
    return sorted(out)


def _counts_case(n_probes, n_known, seed):
    """K: issuer 0 holds one set of three quarters of the records (three blocks of 256 at 1 025), issuer 1 the rest in
    one-member sets of consecutive hours; members in drawn (unsorted) order.  P: half its probes are members of K, under
    the right issuer, the rest are not; two issuers, sets of uneven size."""
    rng = np.random.default_rng(seed)
    ser = _serials(rng, n_known + n_probes)
    rng.shuffle(ser)
    big = n_known * 3 // 4
    k_sets = ([(H0, digest(0), ser[:big])] if big else []) + [(H0 + 1 + i, digest(1), [ser[big + i]]) for i in range(n_known - big)]
    owner = {m: 0 for m in ser[:big]}
    owner.update({m: 1 for m in ser[big:n_known]})
    present = [ser[i] for i in rng.permutation(n_known)[:n_probes // 2]] if n_known else []
    absent = ser[n_known:n_known + n_probes - len(present)]
    by = {0: [], 1: []}
    for m in present:
        by[owner[m]].append(m)
    for i, m in enumerate(absent):
        by[i & 1].append(m)
    p_sets = [(0, digest(d), ms) for d, ms in by.items() if ms]
    return case("counts-%d-%d" % (n_probes, n_known), k_sets, p_sets, INT64_MIN, n_probes=n_probes, n_known=n_known,
                largest_set=big, one_member_sets=n_known - big)


def counts():
    out = [_counts_case(n, 257, 100 + n) for n in COUNTS] + [_counts_case(65, n, 200 + n) for n in COUNTS if n != 257]
    return out + [_counts_case(1025, 1025, 300)]


def hours():
    out = []
    s, other = b"\x01\x02\x03\x04\x05\x06\x07\x08", b"\x01\x02\x03\x04\x05\x06\x07\x09"
    for n in (1, 2, 300):
        # hours before 1970 (negative) and after, not in order of the set keys' issuer
        hs = [-5 - 7 * i for i in range(n // 2)] + [H0 + 11 * i for i in range(n - n // 2)]
        k_sets = [(h, digest(0), [other, s] if i % 3 else [s]) for i, h in enumerate(hs)] + [(h, digest(1), [other]) for h in hs[:3]]
        out.append(case("hours-%d" % n, k_sets, [(0, digest(0), [s, other]), (0, digest(1), [s])], INT64_MIN, hours=n,
                        negative=sum(h < 0 for h in hs)))
    return out


def misses():
    s = bytes(range(1, 18))
    k_sets = [(H0, digest(0), [s, b"\x00"]), (H0 + 1, digest(1), [s[:5]]), (H0 + 2, digest(0), [b"\x00"])]
    near = [s, s[:-1] + b"\xff", s[:-1], s + b"\x00", b"", b"\x00", b"\x00\x00", s[:5]]
    p_sets = [(0, digest(0), near), (0, digest(1), near), (0, digest(2), near)]
    out = [case("misses", k_sets, p_sets, INT64_MIN)]
    # the empty serial held, 00 and 00 00 not
    out.append(case("misses-empty", [(H0, digest(0), [b"", b"\x00\x00\x00"])], [(0, digest(0), [b"", b"\x00", b"\x00\x00", b"\x00\x00\x00"])],
                    INT64_MIN))
    # two issuers of P against one of K; two of K against one of P
    out.append(case("misses-2p-1k", [(H0, digest(0), [s])], [(0, digest(0), [s]), (0, digest(1), [s])], INT64_MIN))
    out.append(case("misses-1p-2k", [(H0, digest(0), [s]), (H0, digest(1), [s]), (H0 + 9, digest(1), [s])], [(0, digest(1), [s])], INT64_MIN))
    return out


def lengths():
    out = []
    for mix in KC.MIXES:
        c = KC.make(mix, [digest(0), digest(1)], [H0, H0 + 30], [130, 70, 41, 90], seed=7)
        k_sets, k_host = [], []
        for key, ms in c.sets.items():
            hour, dg = KI.parse_key(key)
            dev = [m for m in ms if len(m) <= KI.MAX_SERIAL]
            if dev:
                k_sets.append((hour, dg, dev))
            k_host += [(key, m, hour, 1) for m in ms if len(m) > KI.MAX_SERIAL]
        # probes: every third member of K under its own issuer and under the other one, and for each a twin one octet
        # shorter and one longer
        by = {0: set(), 1: set()}
        for j, (hour, dg, ms) in enumerate(k_sets):
            d = 0 if dg == digest(0) else 1
            for m in ms[j % 3::3]:
                by[d].add(m)
                by[1 - d].add(m[:-1])
                if len(m) < KI.MAX_SERIAL:
                    by[d].add(m + b"\x00")
        p_sets = [(0, digest(d), sorted(ms)) for d, ms in by.items()]
        cs = case("lengths-" + mix, k_sets, p_sets, INT64_MIN, k_host=k_host)
        cs.notes["k_lengths"] = sorted({len(m) for _, _, ms in k_sets for m in ms})
        cs.notes["p_lengths"] = sorted({len(m) for _, _, ms in p_sets for m in ms})
        out.append(cs)
    return out


def now_edges():
    s, t = b"\x0a\x0b\x0c", b"\x0d\x0e"
    h = H0 + 5
    base = [(h, digest(0), [s]), (h - 1, digest(0), [s, t]), (h + 1, digest(0), [t])]
    p_sets = [(0, digest(0), [s, t])]
    out = [case("now-kept", base, p_sets, (h + 1) * 3600 - 1), case("now-dropped", base, p_sets, (h + 1) * 3600),
           case("now-all-gone", base, p_sets, (h + 2) * 3600), case("now-early", base, p_sets, 0)]
    wide = base + [(HOUR_LO, digest(0), [s]), (HOUR_LO - 1, digest(0), [s]), (HOUR_HI - 1, digest(0), [t]), (HOUR_HI, digest(0), [t]),
                   (-2 ** 31, digest(0), [s]), (2 ** 31 - 1, digest(0), [t])]
    out.append(case("now-min-years", wide, p_sets, INT64_MIN))
    out.append(case("now-years-late", wide, p_sets, (h + 2) * 3600))
    return out


def repeats():
    s, t, u = b"\x21\x22\x23\x24", b"\x21\x22\x23", b"\x99"
    k_sets = [(H0, digest(0), [s, t, s, u, s]), (H0 + 4, digest(0), [t, t]), (H0 + 4, digest(1), [u])]
    p_sets = [(0, digest(0), [s, t, s, s, u, t]), (0, digest(3), [s, t]), (0, digest(1), [u, u])]
    return [case("repeats", k_sets, p_sets, INT64_MIN)]


def host():
    longs = [bytes([40 + n]) * n for n in range(41, 46)]
    s, t = b"\x31\x32\x33", b"\x34" * 40
    k_sets = [(H0, digest(0), [s]), (H0 + 1, digest(1), [t])]
    k_host = [(host_key(H0, digest(0)), m, H0, 1) for m in longs[:3]] + \
             [(host_key(H0 + 2, digest(0)), m, H0 + 2, 1) for m in longs[:2]] + \
             [(host_key(H0 + 3, digest(0)), s, H0 + 3, 1),                               # … the member section could carry
              (host_key(H0 + 3, digest(1)), t, H0 + 3, 1),
              (host_key(H0 + 30, digest(0), day=True), s, (H0 + 30) // 24 * 24, 24),     # a day key: the day's first hour
              (host_key(H0 + 30, digest(0), day=True), longs[4], (H0 + 30) // 24 * 24, 24),
              (b"serials::2025-02-30-00::" + ident(digest(0)), s, None, 0),                # no such day: skipped
              (b"serials::soon::" + ident(digest(0)), longs[0], None, 0),
              (b"serials::2025-01-01-07::not-a-digest", s, H0 + 7, 1)]                      # an ID of its own
    p_sets = [(0, digest(0), [s, t]), (0, digest(1), [t, s])]
    p_host = [(host_key(0, digest(0)), m, ident(digest(0))) for m in longs] + \
             [(host_key(77, digest(0)), s, ident(digest(0))),                            # a host pair of P met by K's records
              (host_key(77, digest(1)), t, ident(digest(1))),
              (b"serials::whenever::" + ident(digest(0)), longs[1], ident(digest(0))),   # P's dates are not parsed
              (b"serials::whenever::not-a-digest", s, b"not-a-digest"),
              (b"serials::whenever::nobody", s, b"nobody")]
    day_end = ((H0 + 30) // 24 * 24 + 24) * 3600
    return [case("host", k_sets, p_sets, INT64_MIN, k_host, p_host), case("host-now", k_sets, p_sets, (H0 + 3) * 3600, k_host, p_host),
            case("host-day-last", k_sets, p_sets, day_end - 1, k_host, p_host), case("host-day-gone", k_sets, p_sets, day_end, k_host, p_host),
            case("host-only", [], [], INT64_MIN, k_host, p_host), case("host-k-only", [], p_sets, INT64_MIN, k_host, ()),
            case("host-p-only", k_sets, [], INT64_MIN, (), p_host)]


FAMILIES = {"counts": counts, "hours": hours, "misses": misses, "lengths": lengths, "now": now_edges, "repeats": repeats,
            "host": host}


def all_cases():
    return [c for f in FAMILIES.values() for c in f()]
