"""Cases for the filter cascade of a revoked / not-revoked image pair (test helper, no test): a revoked image R, a
not-revoked image S, a `now`, the parameters and the cascade expected — include/ctmr.h ctmr_cascade_build, DESIGN.md §29.

The expectation is worked out here from the Python lists the images are written from, with struct.pack and hashlib
directly, from the format text of the header: it never goes through ct_mapreduce_amd.cascade (the twin under test in
tests/test_cascade_cpu.py).  The images are written with tests/find_corpus.py's `raw_image`.  For every case that has a
cascade the defining property is checked here with a query written here: every kept record of R answers 1, every kept
record of S answers 0.  Every such case converges within its max_layers under this builder, or building the corpus fails.

Params are tuples (k_first, bpk_first_q8, k_rest, bpk_rest_q8, max_layers, salt).

Families (`FAMILIES`: name → function returning [Case]):
  sizes     0/0, 0/n, n/0 and n/n records for n in 1, 63, 64, 65, 255, 256, 257, 1 025; R ≫ S and S ≫ R
  lengths   serial lengths 0..40 on both sides under every salt length 0..16: every message length 37..93
  bits      a first layer of 1, 7, 8, 9, 31, 32, 33, 63, 64, 65 and 65 537 bits with 1, 2, 7 and 32 hash functions
            (1 bit: refused by max_layers)
  sets      257 one-member sets, one 1 025-record set, sets that are not kept (one with a bad record), `now` one second
            before and at an expiry, one digest under two ordinals, one serial under two issuers and under two hours
  refusals  a key in R and S, a bad record in a kept set of R and of S, parameters out of range
  host      members of 41..45 octets in both host sections: counted, absent from the filter
`damaged()` gives the cascades the query refuses.
"""
import hashlib
import struct
from collections import Counter
from dataclasses import dataclass, field

import numpy as np

from ct_mapreduce_amd import known_image as KI

import find_corpus as FC

INT64_MIN = FC.INT64_MIN
H0 = FC.H0
SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)
REST = (1, 370)
MESSAGE_LENGTHS = Counter()    # of every message this builder hashed, by length


@dataclass
class Case:
    name: str
    revoked: bytes
    known: bytes
    now: int
    params: tuple
    cascade: bytes = None       # None: refused with CTMR_E_INVAL
    layers: list = field(default_factory=list)   # (level, k, m_bits, offset, n_held)
    left: int = 0               # refused by max_layers: the false positives of the last layer
    r_keys: list = field(default_factory=list)
    s_keys: list = field(default_factory=list)
    r_host: int = 0
    s_host: int = 0
    family: str = ""
    notes: dict = field(default_factory=dict)


def bit_of(salt, i, level, key, m):
    msg = salt + struct.pack("<I", i) + bytes([level]) + key
    MESSAGE_LENGTHS[len(msg)] += 1
    return struct.unpack("<I", hashlib.sha256(msg).digest()[:4])[0] % m


def expected(r_keys, s_keys, params):
    """→ (cascade bytes, layer table), or (None, how many records max_layers layers left)"""
    k1, b1, k2, b2, max_layers, salt = params
    hold, test, layers = r_keys, s_keys, []
    while hold:
        level = len(layers) + 1
        k, bpk = (k1, b1) if level == 1 else (k2, b2)
        m = max(1, -(-len(hold) * bpk // 256))
        bits = bytearray(-(-((m + 7) // 8) // 64) * 64)
        for key in hold:
            for i in range(k):
                b = bit_of(salt, i, level, key, m)
                bits[b >> 3] |= 1 << (b & 7)
        layers.append((level, k, m, len(hold), bits))
        passed = []
        for key in test:
            for i in range(k):
                b = bit_of(salt, i, level, key, m)
                if not bits[b >> 3] & (1 << (b & 7)):
                    break
            else:
                passed.append(key)
        if not passed:
            break
        if level == max_layers:
            return None, len(passed)
        hold, test = passed, hold
    head = -(-(64 + 32 * len(layers)) // 64) * 64
    table, at = [], head
    for level, k, m, held, bits in layers:
        table.append((level, k, m, at, held))
        at += len(bits)
    out = struct.pack("<8sIIII16sQQQ", b"CTMRCASC", 1, 2, len(layers), len(salt), salt + b"\0" * (16 - len(salt)), at, len(r_keys), len(s_keys))
    out += b"".join(struct.pack("<IIQQQ", *t) for t in table)
    out += b"\0" * (head - len(out)) + b"".join(bytes(l[4]) for l in layers)
    assert len(out) == at and at % 64 == 0
    return out, table


def answer(cascade, key):
    """The walk of the header's text over the cascade's own bytes: 1 = revoked."""
    n, salt_len, salt = struct.unpack_from("<II16s", cascade, 16)
    salt, passed = salt[:salt_len], 0
    for j in range(n):
        level, k, m, off, _ = struct.unpack_from("<IIQQQ", cascade, 64 + 32 * j)
        for i in range(k):
            b = struct.unpack("<I", hashlib.sha256(salt + struct.pack("<I", i) + bytes([level]) + key).digest()[:4])[0] % m
            if not cascade[off + (b >> 3)] & (1 << (b & 7)):
                return passed & 1
        passed += 1
    return passed & 1


def keys_of(sets, now):
    """digest ‖ serial of every record of a kept set, in image order"""
    out = []
    for hour, dg, ms in sorted(sets, key=lambda s: KI.set_key(s[0], s[1])):
        if FC.kept(hour, now):
            out += [dg + bytes(m) for m in ms]
    return out


def case(name, r_sets, s_sets, now, params, r_host=(), s_host=(), r_kept_host=0, s_kept_host=0, **notes):
    """r_host / s_host: [(key, member)] of the host sections; *_kept_host: how many of them lie under keys kept at now."""
    r_keys, s_keys = keys_of(r_sets, now), keys_of(s_sets, now)
    revoked, known = FC.raw_image(r_sets, r_host)[0], FC.raw_image(s_sets, s_host)[0]
    cascade, more = expected(r_keys, s_keys, params)
    c = Case(name, revoked, known, now, params, r_keys=r_keys, s_keys=s_keys, r_host=r_kept_host, s_host=s_kept_host, notes=notes)
    if cascade is None:
        c.left = more
        return c
    c.cascade, c.layers = cascade, more
    assert all(answer(cascade, k) == 1 for k in r_keys), name
    assert all(answer(cascade, k) == 0 for k in s_keys), name
    for level, k, m, off, held in more:     # the bits at and above m, and the padding, are zero
        bits = np.unpackbits(np.frombuffer(cascade, np.uint8, -(-((m + 7) // 8) // 64) * 64, off), bitorder="little")
        assert not bits[m:].any(), name
    return c


def _two_sides(n_r, n_s, seed):
    """n_r + n_s distinct serials: R under two issuers (one large set, one-member sets behind it), S the same way"""
    rng = np.random.default_rng(seed)
    ser = FC._serials(rng, n_r + n_s)
    rng.shuffle(ser)

    def sets(ms, d):
        big = len(ms) * 3 // 4
        return ([(H0, FC.digest(d), ms[:big])] if big else []) + [(H0 + 1 + i, FC.digest(d + 1), [m]) for i, m in enumerate(ms[big:])]
    return sets(ser[:n_r], 0), sets(ser[n_r:], 1)


def sizes():
    p = (2, 740) + REST + (64, b"salt")
    out = [case("sizes-0-0", [], [], INT64_MIN, p)]
    for n in SIZES:
        for n_r, n_s in ((0, n), (n, 0), (n, n)):
            r, s = _two_sides(n_r, n_s, 900 + n)
            out.append(case("sizes-%d-%d" % (n_r, n_s), r, s, INT64_MIN, p, n=n))
    for n_r, n_s in ((1025, 3), (3, 1025)):
        r, s = _two_sides(n_r, n_s, 77)
        out.append(case("sizes-%d-%d" % (n_r, n_s), r, s, INT64_MIN, p, n=1025))
    return out


def lengths():
    """Under every salt length 0..16: serials of every length 0..40 on both sides, two per length and side (the empty
    serial once per issuer)."""
    out = []
    for sl in range(17):
        rng = np.random.default_rng(1000 + sl)
        r_ms, s_ms = [b""], []
        for n in range(1, 41):
            four = set()
            while len(four) < 4:
                four.add(bytes(rng.integers(0, 256, size=n, dtype=np.uint8).tolist()))
            four = sorted(four)
            r_ms += four[:2]
            s_ms += four[2:]
        salt = bytes(range(0xA0, 0xA0 + sl))
        out.append(case("lengths-salt-%d" % sl, [(H0, FC.digest(3), r_ms)], [(H0, FC.digest(3), s_ms), (H0, FC.digest(4), [b""])],
                        INT64_MIN, (3, 1110) + REST + (64, salt)))
    return out


BITS = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 65537)


def _records_for_bits(m):
    """(n, bpk_q8) with max(1, ceil(n · bpk_q8 / 256)) == m: one bit per record while m is small"""
    if m <= 256:
        return m, 256
    for n in range(300, 5000):
        bpk = (m * 256) // n
        if bpk <= 65536 and -(-n * bpk // 256) == m:
            return n, bpk
    raise AssertionError(m)


def bits():
    out = []
    for m in BITS:
        n, bpk = _records_for_bits(m)
        r, s = _two_sides(n, 2 * n, 3000 + m)
        for k in (1, 2, 7, 32):
            # (one bit: every record passes every layer of the first kind; the rest are one bit wide too)
            p = (k, bpk) + ((1, 1) if m == 1 else REST) + (4 if m == 1 else 64, b"\x01\x02")
            out.append(case("bits-%d-k%d" % (m, k), r, s, INT64_MIN, p, m=m))
            assert out[-1].cascade is None if m == 1 else out[-1].layers[0][2] == m
    return out


def _patched(image, record, how):
    """the image with member record `record` made bad: a serial_len of 41, or a padding octet that is not zero"""
    b = bytearray(image)
    n = struct.unpack_from("<Q", b, 32)[0]
    at = len(b) - 48 * (n - record)
    if how == "len":
        struct.pack_into("<Q", b, at, 41)
    else:
        b[at + 47] = 1
    return bytes(b)


def listed_twice():
    """An R whose issuer table names digest(0) twice (ordinals 0 and 1): both ordinals give the same key bytes."""
    a, b = FC.digest(0), FC.digest(1)
    s, t, u = b"\x41\x42", b"\x43", b"\x44\x45\x46"
    table = [a, a, b]
    sets = [(H0, 0, [s, t]), (H0 + 1, 1, [u]), (H0 + 1, 2, [s])]
    set_part, first = [], 0
    for hour, ordinal, ms in sets:
        set_part.append(struct.pack("<iIQQ", hour, ordinal, first, len(ms)))
        first += len(ms)
    meta = struct.pack("<8sIIIIQQQQQ", b"CTMRKNWN", 1, 64, len(table), 0, len(sets), first, 0, 0, 0) + b"".join(table) + b"".join(set_part)
    meta += b"\0" * (-len(meta) % 64)
    revoked = meta + b"".join(struct.pack("<Q", len(m)) + m.ljust(40, b"\0") for _, _, ms in sets for m in ms)
    p = (2, 740) + REST + (64, b"")
    c = case("sets-digest-twice", [(H0, a, [s, t]), (H0 + 1, a, [u]), (H0 + 1, b, [s])], [(H0, a, [u + b"\x00"]), (H0, b, [t, u])], INT64_MIN, p)
    c.revoked = revoked
    return c


def sets():
    p = (2, 740) + REST + (64, b"\xff" * 16)
    rng = np.random.default_rng(4242)
    ser = FC._serials(rng, 2 * 257 + 2 * 1025 + 8)
    rng.shuffle(ser)
    a, b, big_r, big_s, rest = ser[:257], ser[257:514], ser[514:1539], ser[1539:2564], ser[2564:]
    out = [case("sets-257-one-member", [(H0 + i, FC.digest(1), [m]) for i, m in enumerate(a)],
                [(H0 + i, FC.digest(1), [m]) for i, m in enumerate(b)], INT64_MIN, p),
           case("sets-1025-in-one", [(H0, FC.digest(0), big_r)], [(H0, FC.digest(0), big_s)], INT64_MIN, p)]
    # sets that are not kept on both sides, between kept ones; in a second case a bad record lies in such a set
    now = (H0 + 5) * 3600
    r_sets = [(H0 + 2, FC.digest(0), rest[:2]), (H0 + 5, FC.digest(0), a[:70]), (H0 + 6, FC.digest(1), a[70:80])]
    s_sets = [(H0 + 5, FC.digest(0), b[:90]), (H0 + 4, FC.digest(1), rest[2:5]), (H0 + 9, FC.digest(1), b[90:130])]
    out.append(case("sets-not-kept", r_sets, s_sets, now, p))
    c = case("sets-not-kept-bad-record", r_sets, s_sets, now, p)
    c.revoked, c.known = _patched(c.revoked, 1, "len"), _patched(c.known, 1, "pad")   # (in key order both begin with the set that is not kept)
    out.append(c)
    # `now` one second before a set expires and the second it does
    r_sets = [(H0, FC.digest(0), a[:40]), (H0 + 1, FC.digest(0), a[40:60])]
    s_sets = [(H0, FC.digest(0), b[:40]), (H0 + 1, FC.digest(2), b[40:90])]
    out.append(case("sets-now-before-expiry", r_sets, s_sets, (H0 + 1) * 3600 - 1, p))
    out.append(case("sets-now-at-expiry", r_sets, s_sets, (H0 + 1) * 3600, p))
    out.append(listed_twice())
    # one serial under two issuers — two keys, one on each side — and under two hours of one issuer: one key twice in R
    s1, s2 = rest[5], rest[6]
    out.append(case("sets-serial-two-issuers", [(H0, FC.digest(0), [s1, s2])], [(H0, FC.digest(1), [s1, s2])], INT64_MIN, p))
    c = case("sets-serial-two-hours", [(H0, FC.digest(0), [s1]), (H0 + 1, FC.digest(0), [s1, s2])], [(H0, FC.digest(0), a[:5])], INT64_MIN, p)
    assert c.layers[0][4] == 3
    out.append(c)
    return out


def refusals():
    p = (2, 740) + REST + (6, b"s")
    rng = np.random.default_rng(99)
    ser = FC._serials(rng, 140)
    r_sets, s_sets = [(H0, FC.digest(0), ser[:60])], [(H0, FC.digest(0), ser[60:])]
    out = [case("refusal-shared-key", r_sets, [(H0 + 3, FC.digest(0), ser[55:])], INT64_MIN, p)]
    assert out[0].cascade is None and out[0].left > 0
    for side, how in (("R", "len"), ("R", "pad"), ("S", "len"), ("S", "pad")):
        c = case("refusal-bad-record-%s-%s" % (side, how), r_sets, s_sets, INT64_MIN, p[:4] + (64, b"s"), bad_record=True)
        assert c.cascade is not None      # (refused for the record alone)
        if side == "R":
            c.revoked = _patched(c.revoked, 17, how)
        else:
            c.known = _patched(c.known, 79, how)
        c.cascade, c.layers = None, []
        out.append(c)
    for name, q in (("k-0", (0, 740, 1, 370, 6, b"")), ("k-33", (33, 740, 1, 370, 6, b"")), ("k-rest-0", (2, 740, 0, 370, 6, b"")),
                    ("bpk-0", (2, 0, 1, 370, 6, b"")), ("bpk-rest-0", (2, 740, 1, 0, 6, b"")), ("bpk-65537", (2, 65537, 1, 370, 6, b"")),
                    ("layers-0", (2, 740, 1, 370, 0, b"")), ("layers-256", (2, 740, 1, 370, 256, b"")), ("salt-17", (2, 740, 1, 370, 6, b"x" * 17))):
        c = Case("refusal-" + name, FC.raw_image(r_sets)[0], FC.raw_image(s_sets)[0], INT64_MIN, q, notes=dict(bad_params=True))
        out.append(c)
    return out


def host():
    """Members of 41..45 octets under a kept key and under an expired one, on both sides, and a pair the member section
    could carry: none is in the filter, the kept ones are counted."""
    p = (2, 740) + REST + (64, b"")
    rng = np.random.default_rng(5)
    ser = FC._serials(rng, 40)
    a = FC.digest(0)
    longs = [bytes([90 + n]) * n for n in range(41, 46)]
    now = (H0 + 2) * 3600
    kept_key, gone_key = FC.host_key(H0 + 3, a), FC.host_key(H0 + 1, a)
    r_host = [(kept_key, m) for m in longs[:3]] + [(gone_key, longs[3])] + [(kept_key, ser[0])]
    s_host = [(kept_key, m) for m in longs[3:]] + [(gone_key, longs[0])]
    return [case("host-long-members", [(H0 + 3, a, ser[1:20])], [(H0 + 3, a, ser[20:])], now, p, r_host, s_host, 4, 2)]


FAMILIES = {"sizes": sizes, "lengths": lengths, "bits": bits, "sets": sets, "refusals": refusals, "host": host}
_CASES = []


def all_cases():
    """Every case, built once."""
    if not _CASES:
        for family, f in FAMILIES.items():
            for c in f():
                c.family = family
                _CASES.append(c)
    return _CASES


def damaged():
    """[(name, bytes)]: a good cascade of two or more layers damaged in one place each — what the query refuses."""
    good = next(c for c in all_cases() if c.cascade and len(c.layers) >= 2 and c.family == "sizes")
    g = good.cascade

    def patch(fmt, at, *v):
        b = bytearray(g)
        struct.pack_into(fmt, b, at, *v)
        return bytes(b)
    second = struct.unpack_from("<IIQQQ", g, 64 + 32)
    return [("magic", b"CTMRCASK" + g[8:]), ("version", patch("<I", 8, 2)), ("hash-algorithm", patch("<I", 12, 1)),
            ("offset-outside", patch("<Q", 64 + 16, len(g))), ("offset-unaligned", patch("<Q", 64 + 16, second[3] + 4)),
            ("offset-in-table", patch("<Q", 64 + 16, 64)), ("m-0", patch("<Q", 64 + 8, 0)), ("m-2-32", patch("<Q", 64 + 8, 2 ** 32)),
            ("k-0", patch("<I", 64 + 4, 0)), ("k-33", patch("<I", 64 + 4, 33)),
            ("levels-descending", patch("<I", 64 + 32, 1)), ("level-0", patch("<I", 64, 0)),
            ("truncated", g[:-64]), ("truncated-into-header", g[:32]), ("longer", g + b"\0" * 64), ("salt-17", patch("<I", 20, 17)),
            ("layers-256", patch("<I", 16, 256))], good
