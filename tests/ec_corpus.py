"""The values at which multi-limb field arithmetic goes wrong, as EC public keys on the five curves the walk knows — built
from Python integers only (no product code, no oracle): coordinates next to 0 and to p, around every 32-bit limb boundary,
with saturated / zero / one-bit limbs, unreduced coordinates x + m·p that still fit into the key's octets, and uniform
ones; every x with both square roots of x³ − 3x + b when it has one.  The expected verdict of a case is elliptic.Unmarshal's
test, recomputed from the integers: 0 ≤ x < p ∧ 0 ≤ y < p ∧ y² ≡ x³ − 3x + b (mod p)  (csrc/spki_key.h ec_equation).

tests/test_ec_corpus_cpu.py pins the corpus (floors per curve), the host build and the oracle to that verdict;
tests/test_gpu_ec_corpus.py runs the same cases through the device's three sites of the equation."""
import random
from collections import namedtuple

from tests import der as D
from tests.test_spki_cpu import BS, CURVES, PRIMES, cert, ec_spki

CURVE_ID = {"P256": 1, "P384": 2, "P521": 3, "P224": 4, "P192": 5}      # spki_key.h ec_key_check
SEED = 20261018

# kind: "root" (x, ±y) · "y+1" · "flip_y" · "flip_x" · "x+mp" / "y+mp" (m in .m) · "noroot" (x, random y), (x, 0) ·
# "top_bit" (P-521: a bit above the 521st set) · "edge" (p, y), (x, p), (0, 0).  src: where x came from — "end", "limb", "pattern", "random", "small_y" (y + p fits), "carry33" (P256_CARRY33), "edge".
Case = namedtuple("Case", "curve x y ok kind src m")


def byte_len(curve):
    return CURVES[curve][1]


def n_limbs(curve):
    return (byte_len(curve) + 3) // 4


def on_curve(curve, x, y):
    p = PRIMES[curve]
    return 0 <= x < p and 0 <= y < p and (y * y - (x * x * x - 3 * x + BS[curve])) % p == 0


def sqrt_mod(a, p):
    """A square root of a mod p (p an odd prime), or None.  p ≡ 3 (mod 4): a^((p+1)/4); else Tonelli–Shanks (P-224)."""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    if p % 4 == 3:
        return pow(a, (p + 1) // 4, p)
    q, s = p - 1, 0
    while q % 2 == 0:
        q //= 2
        s += 1
    z = next(z for z in range(2, 1000) if pow(z, (p - 1) // 2, p) == p - 1)
    m, c, t, r = s, pow(z, q, p), pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2 = t2 * t2 % p
            i += 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c = i, b * b % p
        t, r = t * c % p, r * b % p
    return r


def x_values(curve):
    """[(x, src)] in a fixed order, x < p, no x twice."""
    p, nl = PRIMES[curve], n_limbs(curve)
    rng = random.Random("%d x %s" % (SEED, curve))
    xs = [(k, "end") for k in range(64)] + [(p - 1 - k, "end") for k in range(64)]
    for j in range(1, nl):
        xs += [((1 << 32 * j) + d, "limb") for d in range(-8, 9)]
        xs += [(p - (1 << 32 * j) - d, "limb") for d in range(8)]
    limb = (0, 1, 0x80000000, 0xfffffffe, 0xffffffff, None)
    for _ in range(64):
        v = 0
        for j in range(nl):
            w = rng.choice(limb)
            v |= (rng.getrandbits(32) if w is None else w) << 32 * j
        xs.append((v % p, "pattern"))
    xs += [(rng.randrange(p), "random") for _ in range(200)]
    seen, out = set(), []
    for x, src in xs:
        assert 0 <= x < p, (curve, x)
        if x not in seen:
            seen.add(x)
            out.append((x, src))
    return out


def _pmul(f, g, p):
    out = [0] * (len(f) + len(g) - 1)
    for i, a in enumerate(f):
        for j, b in enumerate(g):
            out[i + j] = (out[i + j] + a * b) % p
    return out


def _pmod(f, g, p):
    """f mod g over GF(p); coefficient lists, lowest first, g's leading coefficient non-zero."""
    f, inv = list(f), pow(g[-1], -1, p)
    while len(f) >= len(g):
        q = f[-1] * inv % p
        for i in range(len(g)):
            f[len(f) - len(g) + i] = (f[len(f) - len(g) + i] - q * g[i]) % p
        f.pop()
    while f and f[-1] == 0:
        f.pop()
    return f


def x_of_y(curve, y):
    """The x with x³ − 3x + b = y² (mod p) when there is exactly one (half of all y), else None: gcd(x^p − x, cubic)."""
    p = PRIMES[curve]
    f = [(BS[curve] - y * y) % p, p - 3, 0, 1]
    h, sq, e = [1], [0, 1], p
    while e:
        if e & 1:
            h = _pmod(_pmul(h, sq, p), f, p)
        sq = _pmod(_pmul(sq, sq, p), f, p)
        e >>= 1
    g = h + [0] * (2 - len(h))
    g[1] = (g[1] - 1) % p
    while g and g[-1] == 0:
        g.pop()
    a, b = f, g
    while b:
        a, b = b, _pmod(a, b, p)
    return (-a[0] * pow(a[1], -1, p)) % p if len(a) == 2 else None


def small_y_points(curve, n=8):
    """Points whose y + p still fits into the coordinate's octets, on the curves where a uniform y never does (p lies
    within 2^(8·BYTES − 32) of the top there): y counted up from 1 and down from the largest that fits, in turn."""
    p, room = PRIMES[curve], (1 << 8 * byte_len(curve)) - PRIMES[curve]
    out, k = [], 0
    while len(out) < n:
        k += 1
        y = (k + 1) // 2 if k & 1 else room - k // 2
        x = x_of_y(curve, y)
        if x is not None:
            out.append((x, y))
    return out


# P-256 field elements whose SQUARING drives the ninth accumulator limb of mont_mul to 2^32 — the carry p256_redc_step's
# `top` must keep (spki_key.h; ADVICE r05: it was once cut to 32 bits, and nothing that is not built for it gets there: the
# row sum t + b_i·a reaches 2^288 only when a lies within 2^160 of p, b_i = 2^32 − 1, and the two rows before it had
# b_i = m = 2^32 − 1 exactly).  In a squaring that leaves a = 2^256 − 2^224 + 2^192 − e, 1 ≤ e ≤ 2^96 (limbs 3, 4, 5
# saturated), and the rows 3 and 4 reduce with m = 2^32 − 1 exactly when e² mod (2^96 − 1) ≡ −1 (mod 2^64): e is a square
# root of 2^64·k − 1 modulo the twelve prime powers of 2^96 − 1, put together by the Chinese remainder theorem.
# (scripts/find_p256_carry33.py is the search.)  p256_row_tops() below recomputes the row sums: the property is checked.
P256_CARRY33 = (0xffffffff00000000ffffffffffffffffffffffffffffff7fff800080007fff80,      # as x: the curve has both y
                0xffffffff00000000ffffffffffffffffffffffffffffffd554d5562aab2aaa80,      # as y: one x belongs to it
                0xffffffff00000000fffffffffffffffffffffffffffe36870bad98a56f3c24c7,      # these three: as x and as y
                0xffffffff00000000ffffffffffffffffffffffffffff7218bdd11d966734f65d,
                0xffffffff00000000fffffffffffffffffffffffffffcd6fac03ac15e5bc4e4aa)


def p256_row_tops(a, b):
    """Limb 8 of the accumulator (`top`) in every row of mont_mul<CurveP256>(a, b), from Python integers."""
    p, t, tops = PRIMES["P256"], 0, []
    for i in range(8):
        s = t + ((b >> 32 * i) & 0xffffffff) * a
        tops.append(s >> 256)
        t = (s + (s & 0xffffffff) * p) >> 32          # −p⁻¹ ≡ 1 (mod 2^32): m = t[0]
    return tops


def multiples_that_fit(curve, v):
    """The m ≥ 1 with v + m·p still inside the coordinate's octets: at most one on four of the curves; P-521's 66 octets
    leave room for 127 — the first two, a middle one and the last."""
    p, top = PRIMES[curve], 1 << 8 * byte_len(curve)
    ms = (1, 2, 64, 127) if curve == "P521" else (1,)
    return [m for m in ms if v + m * p < top]


def flip_bit(curve, v, rng):
    """v with one bit flipped in a randomly chosen limb (a bit the coordinate's octets hold)."""
    j = rng.randrange(n_limbs(curve))
    width = min(32, 8 * byte_len(curve) - 32 * j)
    return v ^ (1 << (32 * j + rng.randrange(width)))


_cache = {}


def cases(curve):
    """Every case of the curve, in a fixed order (memoised: the tests share one corpus and leave it unchanged)."""
    if curve in _cache:
        return _cache[curve]
    p, b = PRIMES[curve], BS[curve]
    rng = random.Random("%d cases %s" % (SEED, curve))
    out = []

    def emit(x, y, kind, src, m=0):
        out.append(Case(curve, x, y, on_curve(curve, x, y), kind, src, m))

    first = None
    for x, src in x_values(curve):
        rhs = (x * x * x - 3 * x + b) % p
        y = sqrt_mod(rhs, p)
        if y is None:
            emit(x, rng.randrange(p), "noroot", src)
            emit(x, 0, "noroot", src)
            continue
        assert y * y % p == rhs
        first = first or (x, y)
        emit(x, y, "root", src)
        emit(x, (p - y) % p, "root", src)
        emit(x, (y + 1) % p, "y+1", src)
        emit(x, flip_bit(curve, y, rng), "flip_y", src)
        emit(flip_bit(curve, x, rng), y, "flip_x", src)
        for m in multiples_that_fit(curve, x):
            emit(x + m * p, y, "x+mp", src, m)
        for m in multiples_that_fit(curve, y):
            emit(x, y + m * p, "y+mp", src, m)
    if curve == "P256":
        for a in P256_CARRY33:
            y, x = sqrt_mod((a * a * a - 3 * a + b) % p, p), x_of_y(curve, a)
            for px, py in ([(a, y)] if y is not None else []) + ([(x, a)] if x is not None else []):
                emit(px, py, "root", "carry33")
                emit(px, p - py, "root", "carry33")
                emit(px, (py + 1) % p, "y+1", "carry33")
                emit((px + 1) % p, py, "flip_x", "carry33")
    if curve == "P521":                          # a bit above the 521st: the top limb's 16 bits are range-checked, not masked
        roots = [c for c in out if c.kind == "root"][:16:2]
        for c in roots:
            for bit in range(521, 528):
                emit(c.x | 1 << bit, c.y, "top_bit", c.src)
                emit(c.x, c.y | 1 << bit, "top_bit", c.src)
    if curve != "P521":
        for x, y in small_y_points(curve):
            emit(x, y, "root", "small_y")
            emit(x, p - y, "root", "small_y")
            emit(x, y + p, "y+mp", "small_y", 1)
    emit(p, first[1], "edge", "edge")
    emit(first[0], p, "edge", "edge")
    emit(0, 0, "edge", "edge")
    for c in out:      # what the construction promises, from the integers
        assert c.ok == (c.kind == "root") or c.kind in ("y+1", "flip_y", "flip_x", "noroot"), c
        assert c.x < 1 << 8 * byte_len(curve) and c.y < 1 << 8 * byte_len(curve), c
    _cache[curve] = out
    return out


def all_cases():
    return [c for curve in CURVES for c in cases(curve)]


def xy(c):
    """X ‖ Y octets of a case."""
    bl = byte_len(c.curve)
    return c.x.to_bytes(bl, "big") + c.y.to_bytes(bl, "big")


def case_spki(c):
    return ec_spki(c.curve, xy(c))


def case_cert(c, serial=b"\x01", **kw):
    return cert(case_spki(c), serial=serial, **kw)


def edge_distance(c):
    """How far the case's x lies from the nearest end (0, p − 1) or limb boundary (2^(32j), p − 2^(32j))."""
    p = PRIMES[c.curve]
    x = c.x % p
    anchors = [0, p - 1] + [a for j in range(1, n_limbs(c.curve)) for a in (1 << 32 * j, p - (1 << 32 * j))]
    return min(abs(x - a) for a in anchors)


def closest_to_the_edges(curve, n=24):
    """(n accepted, n refused) cases of the curve whose x lies closest to an end or a limb boundary; the refused ones taken
    in turn from every kind of refusal, so that unreduced coordinates and near misses are both among them."""
    cs = [c for c in cases(curve) if c.src in ("end", "limb", "edge")]
    good = sorted((c for c in cs if c.ok), key=lambda c: (edge_distance(c), c.x, c.y))[:n]
    by_kind = {}
    for c in sorted((c for c in cs if not c.ok), key=lambda c: (edge_distance(c), c.x, c.y)):
        by_kind.setdefault(c.kind, []).append(c)
    bad, kinds = [], sorted(by_kind)
    while len(bad) < n:
        for k in kinds:
            if by_kind[k] and len(bad) < n:
                bad.append(by_kind[k].pop(0))
    assert len(good) == n and len(bad) == n
    return good, bad


# ------------------------------------------------------------------ placement: pad counts and byte phases
def right_align(bits, pad):
    """encoding/asn1 BitString.RightAlign: the octets shifted right by the pad count."""
    return (int.from_bytes(bits, "big") >> pad).to_bytes(len(bits), "big") if bits else b""


def unmarshal_ok(curve, bits, pad):
    """parsePublicKey's verdict on an EC key's BIT STRING octets, from the integers: length, the 04, the point."""
    bl = byte_len(curve)
    a = right_align(bits, pad)
    if len(a) != 1 + 2 * bl or a[0] != 4:
        return False
    return on_curve(curve, int.from_bytes(a[1:1 + bl], "big"), int.from_bytes(a[1 + bl:], "big"))


def shifted_key(c, pad):
    """The BIT STRING octets whose right-aligned form is 04 ‖ X ‖ Y (the last `pad` bits zero) — as far as that exists:
    04 << 6 does not fit into the first octet, so at pad counts 6 and 7 what is left is a key that does not begin with 04."""
    body = b"\x04" + xy(c)
    return ((int.from_bytes(body, "big") << pad) & ((1 << 8 * len(body)) - 1)).to_bytes(len(body), "big")


Placed = namedtuple("Placed", "curve pad phase ok der keypos")     # keypos: offset of the BIT STRING's key octets in der


def placement_points(curve):
    """Three accepted and three refused points of the curve: an end, a limb boundary and a patterned x each; the refused
    ones a near miss, an unreduced x and a flipped bit."""
    cs = cases(curve)
    good = [next(c for c in cs if c.ok and c.src == s) for s in ("end", "limb", "pattern")]
    bad = [next(c for c in cs if not c.ok and c.kind == k) for k in ("y+1", "x+mp", "flip_x")]
    return good + bad


def placement_cases(start=0):
    """Every curve × six points × pad count 0 … 7 × the four byte phases of the point in a payload that holds the
    certificates back to back from byte `start` on: the serial's length (3 … 6 octets) is chosen per certificate so that
    the key octets begin at the phase wanted.  Distinct serials."""
    out, at, k = [], start, 0
    subject = D.name(D.rdn(3, b"placement"))
    for curve in CURVES:
        params = D.tlv(0x06, bytes.fromhex(CURVES[curve][0]))
        for c in placement_points(curve):
            for pad in range(8):
                bits = shifted_key(c, pad)
                sp = D.spki(D.OID_EC, params, bits, pad)
                for phase in range(4):
                    for sl in range(3, 7):
                        serial = (b"\x31" + k.to_bytes(2, "big") + b"\x55" * 3)[:sl]
                        der = cert(sp, serial=serial, subject=subject)
                        keypos = der.index(sp) + sp.index(bits)
                        if (at + keypos) % 4 == phase:
                            break
                    else:
                        raise AssertionError((curve, pad, phase))
                    out.append(Placed(curve, pad, phase, unmarshal_ok(curve, bits, pad), der, keypos))
                    at += len(der)
                    k += 1
    return out


# ------------------------------------------------------------------ the batches the device tests map
# (built here, without the engine, so that tests/test_ec_corpus_cpu.py can hold what they expect to the oracle first)
RSA_ISSUER = D.cert(serial=b"\x01", spki=D.rsa_spki(), exts=[D.BC_CA])
Entries = namedtuple("Entries", "certs ets ok stored")
# ok[i]: the integer verdict on entry i's key (None: an RSA key, always fine); stored: how many distinct certificates the
# table holds once the batch is mapped under one good issuer — an accepted key, except that secp192r1 is a finding, which
# costs a precertificate entry (ets[i] == 1) its place (csrc/spki_key.h)


def serial_of(tag, k):
    return bytes([tag]) + k.to_bytes(2, "big")


def _entries(items, ets):
    p192 = bytes.fromhex(CURVES["P192"][0])
    stored = len({c for i, (c, v) in enumerate(items) if v is not False and not (ets[i] == 1 and p192 in c)})
    return Entries([c for c, _ in items], list(ets), [v for _, v in items], stored)


def leaf_entries():
    """The whole corpus, one certificate per case with a serial of its own, X509 and precertificate entries in turn,
    shuffled: P-256 and the other curves share their 1 024-entry blocks.  Returns (Entries, the case of every entry)."""
    cs = all_cases()
    order = list(range(len(cs)))
    random.Random(SEED).shuffle(order)
    items = [(case_cert(cs[k], serial=serial_of(0x41, k)), cs[k].ok) for k in order]
    return _entries(items, [n & 1 for n in range(len(items))]), [cs[k] for k in order]


def edge_cases():
    """What the in-walk equation (issuer registration, the strict_leaf TBS check) is run at: per curve the 24 accepted and
    24 refused cases closest to the edges, in turn, and P-256's carry cases."""
    out = []
    for curve in CURVES:
        good, bad = closest_to_the_edges(curve)
        out += [c for pair in zip(good, bad) for c in pair]
    return out + [c for c in cases("P256") if c.src == "carry33"]


def picks(curve, ok, n, skip=0):
    """n cases of the curve with that verdict, from the corpus in its order (every kind of refusal among the refused)."""
    out = [c for c in cases(curve) if c.ok == ok][skip:skip + n]
    assert len(out) == n, (curve, ok, n)
    return out


def block_entries(first_block):
    """2 051 entries for k_ec_resolve's block structure (kernels/reduce.h: a block compacts the pending entries of 1 024
    consecutive entries into list[1024] and walks them 256 at a time; two instantiations pick their own curves).
    Block 0: 1 024 EC keys, on and off the curve — "p256_and_p384": the two in turn (the list is full between the two
    instantiations: 512 each, two rounds), "p384_only": list[1024] full in one (four rounds).  Block 1: RSA keys but for
    exactly 257 P-521 / P-224 / P-192 keys at fixed-seed places (two full rounds and one lane).  Block 2: RSA, RSA, an
    off-curve P-256 key — the batch ends inside a group of four ent[] words with a pending entry last.  Some accepted keys
    occur twice (DEFER in pass 1 of the insert)."""
    rng = random.Random("%d blocks" % SEED)
    items, n_ser = [], [0]

    def ec(c):
        n_ser[0] += 1
        return case_cert(c, serial=serial_of(0x71, n_ser[0])), c.ok

    def rsa():
        n_ser[0] += 1
        return D.cert(serial=serial_of(0x72, n_ser[0]), spki=D.rsa_spki(), exts=[D.BC_NOT_CA]), None

    if first_block == "p256_and_p384":
        src = {(cv, ok): iter(picks(cv, ok, 256)) for cv in ("P256", "P384") for ok in (True, False)}
        for i in range(1024):
            items.append(ec(next(src["P256" if i % 2 == 0 else "P384", (i // 2) % 2 == 0])))
    else:
        assert first_block == "p384_only"
        src = {ok: iter(picks("P384", ok, 512)) for ok in (True, False)}
        for i in range(1024):
            items.append(ec(next(src[i % 2 == 0])))
    for i in range(8, 1024, 61):                 # in-batch duplicates: entry i − 4 has the same curve and the same verdict
        if items[i][1]:
            items[i] = items[i - 4]
    rare = [ec(picks(("P521", "P224", "P192")[j % 3], j % 2 == 0, 1, skip=7 * (j // 6))[0]) for j in range(257)]
    for j in range(6, 257, 30):                  # (even: accepted; j − 6: the same curve)
        rare[j] = rare[j - 6]
    at, rare = set(rng.sample(range(1024, 2048), 257)), iter(rare)
    for i in range(1024, 2048):
        items.append(next(rare) if i in at else rsa())
    items += [rsa(), rsa(), ec(picks("P256", False, 1, skip=300)[0])]
    assert len(items) == 2051 and sum(v is not None for _, v in items[1024:2048]) == 257
    assert all(v is not None for _, v in items[:1024]) and items[-1][1] is False
    assert len({c for c, _ in items}) <= len(items) - 12
    return _entries(items, [1 if i % 5 == 3 else 0 for i in range(len(items))])


def issuer_entries():
    """The cases closest to the edges as Chain[0] issuers, one RSA leaf each: (issuer certificates, Entries, cases)."""
    cs = edge_cases()
    issuers = [D.cert(serial=serial_of(0x51, k), spki=case_spki(c), exts=[D.BC_CA]) for k, c in enumerate(cs)]
    items = [(D.cert(serial=serial_of(0x52, k), spki=D.rsa_spki(), exts=[D.BC_NOT_CA]), None) for k in range(len(cs))]
    return issuers, _entries(items, [k & 1 for k in range(len(cs))]), cs


def raw_precert_pairs():
    """The same cases as raw precertificate entries (leaf_input, extra_data): the leaf's TBSCertificate carries the key."""
    from tests.test_entry_decode_cpu import asn1cert, chain, precert_leaf
    from tests.test_walk_cpu import tbs_of
    cs = edge_cases()
    pairs = []
    for k, c in enumerate(cs):
        der = case_cert(c, serial=serial_of(0x61, k))
        pairs.append((precert_leaf(tbs_of(der), ts=1000 + k), asn1cert(der) + chain([RSA_ISSUER])))
    return pairs, cs


def raw_precert_status(c):
    """What becomes of the raw precertificate entry of a case under strict_leaf: a key that does not parse drops the entry
    in the decode; an accepted secp192r1 key is a finding — the entry is decoded, and the precertificate then loses its
    place in the map; any other accepted key passes."""
    from oracle import oracle as orc
    return orc.ST_ENTRY_DECODE_ERROR if not c.ok else orc.ST_PARSE_ERROR if c.curve == "P192" else orc.ST_PASS
