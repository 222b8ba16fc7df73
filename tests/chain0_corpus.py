"""Constructed corpus for the Chain[0] → issuer match of the raw get-entries path (kernels/entries.h match_wave, called from
k_decode_match and k_chain0_match; registration in engine/entries.inc, the certificate store and its table in
engine/issuers.inc), and the reference model the tests hold it to.

Pure Python over tests/der.py and the RFC 6962 encoders of tests/test_entry_decode_cpu.py; deterministic from SEED.  The only
product code it touches is the candidate hash compiled for the host (tests/harness: harness_quick_hash), to search for hash
geometries and to be checked against.

What the match reads and how: the candidate hash covers the length and the first and last 16 octets (every octet below 32);
the comparison streams Chain[0] sixteen octets per lane, lane·16 in the first KiB, lane·16 + 1024 in the second, a loop from
2 KiB on, the last chunk cut by a mask (eq16_prefix).  The families put certificate lengths, differing octets, table slots
and batch sizes at the edges of exactly that.

The reference model is a dict from Chain[0] bytes to registration index: expected_issuer_idx, expected_pending,
expected_self_registration below.  decode_pair restates the RFC 6962 framing for the model; tests/test_chain0_corpus_cpu.py
holds it to the oracle's decoder on every entry of the corpus."""
import dataclasses
import functools
import random
import struct

import numpy as np

from tests import der
from tests.test_entry_decode_cpu import asn1cert, chain, precert_leaf, x509_leaf

SEED = 20261019
NO_ISSUER = 0xFFFFFFFF
UNDECODABLE = -1            # expected_issuer_idx: the entry does not decode (the product writes NO_ISSUER and ENTRY_INVALID)
ENTRY_INVALID = 0xFF
PAD = 32                    # octets a caller keeps readable behind the blob (CTMR_PAYLOAD_PAD)
PEND_SLOTS = 8192           # kernels/entries.h
UNREG_CAP = 16384           # ctmr_engine.hip
M64 = (1 << 64) - 1
U = np.uint64


# ------------------------------------------------------------------ the candidate hash (entry_decode.h cert_quick_hash)

def qh_mix(z):
    """numpy uint64 (arrays or scalars), wrapping."""
    z = (z ^ (z >> U(30))) * U(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> U(27))) * U(0x94d049bb133111eb)
    return z ^ (z >> U(31))


def quick_hash_tails(length, head16, tails):
    """cert_quick_hash of n certificates of `length` >= 32 octets that share their first sixteen octets `head16`;
    tails: uint64[n, 4], the last sixteen octets as four little-endian dwords.  uint64[n]."""
    assert length >= 32 and len(head16) == 16
    with np.errstate(over="ignore"):
        h = qh_mix(U(0x9e3779b97f4a7c15) + U(length))
        hd = np.frombuffer(head16, "<u4").astype(np.uint64)
        for k in range(4):
            h = qh_mix(h ^ (hd[k] << U(1) | U(1)))
        h = np.full(len(tails), h, np.uint64)
        for k in range(4):
            h = qh_mix(h ^ (tails[:, k] << U(1)))
    return np.where(h == 0, U(1), h)


def _mix(z):
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def quick_hash(c):
    """cert_quick_hash of one byte string of any length (the len < 32 branch included), in Python integers."""
    n = len(c)
    h = _mix((0x9e3779b97f4a7c15 + n) & M64)
    if n >= 32:
        for w in struct.unpack("<4I", c[:16]):
            h = _mix(h ^ (w << 1 | 1))
        for w in struct.unpack("<4I", c[-16:]):
            h = _mix(h ^ (w << 1))
    else:
        for b in c:
            h = _mix(h ^ b)
    return h or 1


def harness_quick_hash(c):
    """The product's cert_quick_hash, host build."""
    from tests import harness
    harness.product_decode_entry(b"\0" * 16, b"\0" * 4)              # (builds and binds the harness library)
    return int(harness._entry.harness_quick_hash(bytes(c), len(c)))


# ------------------------------------------------------------------ certificates

def _rng(*what):
    return random.Random("/".join(str(w) for w in (SEED,) + what))


def modulus(ident):
    """A 2048-bit modulus of its own per identity: positive, minimally encoded, odd."""
    return b"\x00\xc3" + _rng("n", ident).randbytes(254) + b"\x01"


def ca_cert(length, ident, n=None):
    """A CA certificate that parses as an issuer, `length` octets to the byte: the signature BIT STRING is unconstrained,
    its filler (seeded noise: a comparison that shifts or skips octets sees it) sets the length; where a DER length field
    grows on the way, a longer subject steps over the gap."""
    n = n if n is not None else modulus(ident)
    spki = der.rsa_spki(n=n)
    noise = _rng("sig", ident).randbytes(max(length, 64))
    for cn_pad in range(6):
        kw = dict(serial=b"\x01" + _rng("serial", ident).randbytes(7), issuer=der.name(der.rdn(3, b"Chain0 Root")),
                  subject=der.name(der.rdn(3, b"Chain0 CA " + str(ident).encode() + b"." * cn_pad)),
                  exts=[der.BC_CA], spki=spki)
        f = length - len(der.cert(sig=b"\x00", **kw))
        for fill in range(max(f - 6, 0), max(f, 0) + 1):
            c = der.cert(sig=b"\x00" + noise[:fill], **kw)
            if len(c) == length:
                return c
    raise ValueError(f"no CA certificate of {length} octets")


def spki_of(c, n):
    """(offset, length) of the SubjectPublicKeyInfo with modulus n inside c."""
    s = der.rsa_spki(n=n)
    at = c.index(s)
    return at, len(s)


@functools.lru_cache(maxsize=None)
def leaves():
    """A few leaf certificates every family wraps again and again: (certificate, its TBSCertificate)."""
    out = []
    for k in range(6):
        c = der.cert(serial=b"\x02" + _rng("leaf", k).randbytes(3 + k), subject=der.name(der.rdn(3, b"leaf %d" % k)),
                     not_after=der.utctime("2%d0%d01000000Z" % (7 + k % 2, 1 + k)))
        out.append((c, _tbs_of(c)))
    return out


def _tbs_of(c):
    def hdr(p):
        ln = c[p + 1]
        if ln < 0x80:
            return p + 2, p + 2 + ln
        k = ln & 0x7f
        return p + 2 + k, p + 2 + k + int.from_bytes(c[p + 2:p + 2 + k], "big")
    c0, _ = hdr(0)
    _, t1 = hdr(c0)
    return c[c0:t1]


FF_ELEMENT = b"\xff" * 40   # a second chain element: 0xff right behind Chain[0]'s last octet, no 0x00 in reach of a 16-octet read


def entry(k, chain0, form):
    """One get-entries pair around leaf k.  form: "x509" — Chain[0] ends extra_data, the next entry's leaf (or the blob's
    end) lies behind it; "x509ff" — a chain element of 0xff octets follows; "precert" — a precertificate entry, Chain[0]
    ends extra_data; chain0 None = an empty chain."""
    cert, tbs = leaves()[k % len(leaves())]
    ts = 1_700_000_000_000 + k
    certs = [] if chain0 is None else [chain0] + ([FF_ELEMENT] if form == "x509ff" else [])
    if form == "precert":
        return _v(precert_leaf(tbs, ikh=bytes([k & 0xff]) * 32, ts=ts)), asn1cert(cert) + chain(certs)
    return _v(x509_leaf(cert, ts=ts)), chain(certs)


def _v(leaf):
    """Version octet 0xff (CT-go bounds the enum by its maximum only): the octet right behind a Chain[0] that ends its
    extra_data is the next leaf's first, and the certificate store pads with zeros."""
    return b"\xff" + leaf[1:]


def undecodable(k):
    """An entry LogEntryFromLeaf rejects, with a Chain[0]-shaped run of octets where a decoder gone wrong would look."""
    cert, _ = leaves()[k % len(leaves())]
    c0 = b"\x30\x82" + bytes([k & 0xff]) * 70
    return [(x509_leaf(cert, entry_type=3), chain([c0])),               # unknown entry type
            (x509_leaf(cert), chain([c0]) + b"\x00"),                   # CertificateChain: trailing data
            (x509_leaf(cert), chain([c0])[:-1]),                        # chain cut short
            (x509_leaf(cert)[:-1], chain([c0])),                        # leaf cut short
            (b"", b""),
            (x509_leaf(cert, leaf_type=1), chain([c0]))][k % 6]


# ------------------------------------------------------------------ RFC 6962 framing, restated for the model

@dataclasses.dataclass
class Dec:
    entry_type: int
    cert_in_extra: bool
    cert_off: int
    cert_len: int
    chain0_off: int     # into extra_data
    chain0_len: int
    n_chain: int


def decode_pair(leaf, extra):
    """ct.LogEntryFromLeaf's framing (RFC 6962 §3.4, §4.6): None = rejected."""
    if len(leaf) < 12 or leaf[1] != 0:
        return None
    et = int.from_bytes(leaf[10:12], "big")
    p = 12
    if et == 1:
        p += 32
    elif et != 0:
        return None
    if len(leaf) < p + 3:
        return None
    n1 = int.from_bytes(leaf[p:p + 3], "big")
    body = p + 3
    p = body + n1
    if n1 < 1 or len(leaf) < p + 2:
        return None
    if p + 2 + int.from_bytes(leaf[p:p + 2], "big") != len(leaf):
        return None
    q = 0
    cert_off, cert_len = body, n1
    if et == 1:
        if len(extra) < 3:
            return None
        cert_len = int.from_bytes(extra[:3], "big")
        cert_off = 3
        q = 3 + cert_len
        if cert_len < 1 or q > len(extra):
            return None
    if len(extra) < q + 3 or q + 3 + int.from_bytes(extra[q:q + 3], "big") != len(extra):
        return None
    q += 3
    c0_off = c0_len = n = 0
    while q < len(extra):
        if len(extra) - q < 3:
            return None
        k = int.from_bytes(extra[q:q + 3], "big")
        q += 3
        if k < 1 or len(extra) - q < k:
            return None
        if n == 0:
            c0_off, c0_len = q, k
        n += 1
        q += k
    return Dec(et, et == 1, cert_off, cert_len, c0_off, c0_len, n)


def chain0_of(pairs):
    """Per entry: Chain[0]'s octets, None for an empty chain, UNDECODABLE."""
    out = []
    for leaf, extra in pairs:
        d = decode_pair(leaf, extra)
        out.append(UNDECODABLE if d is None else (extra[d.chain0_off:d.chain0_off + d.chain0_len] if d.n_chain else None))
    return out


def distinct(chain0s):
    """The distinct Chain[0] byte strings in order of first appearance."""
    return list(dict.fromkeys(c for c in chain0s if isinstance(c, bytes)))


def expected_view(pairs):
    """What the decode must write for blob = leaf_0 ‖ extra_0 ‖ leaf_1 ‖ …: a dict of arrays (entry_type, cert_start,
    cert_end, chain0_start, chain0_len) and the counters (n_x509, n_precert, n_decode_error, n_no_chain)."""
    n = len(pairs)
    v = {"entry_type": np.full(n, ENTRY_INVALID, np.uint8), "cert_start": np.zeros(n, np.uint64), "cert_end": np.zeros(n, np.uint64),
         "chain0_start": np.zeros(n, np.uint64), "chain0_len": np.zeros(n, np.uint32)}
    cnt = [0, 0, 0, 0]
    at = 0
    for i, (leaf, extra) in enumerate(pairs):
        d = decode_pair(leaf, extra)
        if d is None:
            cnt[2] += 1
        else:
            cnt[d.entry_type] += 1
            cnt[3] += d.n_chain == 0
            base = at + (len(leaf) if d.cert_in_extra else 0)
            v["entry_type"][i] = d.entry_type
            v["cert_start"][i] = base + d.cert_off
            v["cert_end"][i] = base + d.cert_off + d.cert_len
            if d.n_chain:
                v["chain0_start"][i] = at + len(leaf) + d.chain0_off
                v["chain0_len"][i] = d.chain0_len
        at += len(leaf) + len(extra)
    v["counters"] = tuple(cnt)
    return v


def expected_issuer_idx(pairs, registered):
    """THE MODEL.  Per entry: the index of its Chain[0] in registration order, NO_ISSUER (empty chain), UNDECODABLE; a
    Chain[0] that is not registered raises KeyError.  int64[n]."""
    index = {}
    for k, c in enumerate(registered):
        index.setdefault(c, k)
    return np.asarray([c if c == UNDECODABLE else NO_ISSUER if c is None else index[c] for c in chain0_of(pairs)], np.int64)


def expected_pending(pairs, registered, quick_hash=quick_hash):
    """What round 0 must report with auto-registration off: per distinct candidate hash among the entries whose Chain[0] is
    not registered, the Chain[0] of the lowest log index carrying it; deduplicated by content, in log order."""
    known = set(registered)
    first = {}
    for c in chain0_of(pairs):
        if isinstance(c, bytes) and c not in known:
            first.setdefault(quick_hash(c), c)
    return list(dict.fromkeys(first.values()))


def expected_self_registration(pairs, registered=(), quick_hash=quick_hash):
    """The registration order of one self-registering call (engine/entries.inc): the first two rounds register one
    certificate per candidate hash — the lowest log index carrying it — in log order, the third every one that is left, in log
    order.  Holds while a round's distinct hashes fit the claim table.  Returns (registered afterwards, certificates per
    round)."""
    reg, rounds = list(registered), []
    for r in range(3):
        if r < 2:
            new = expected_pending(pairs, reg, quick_hash)
            assert len(new) < PEND_SLOTS // 8
        else:
            known = set(reg)
            new = [c for c in distinct(chain0_of(pairs)) if c not in known]
        if not new:
            break
        rounds.append(new)
        reg += new
    return reg, rounds


# ------------------------------------------------------------------ the families

@dataclasses.dataclass
class Family:
    name: str
    pairs: list            # [(leaf_input, extra_data)]
    chain0: list           # the distinct Chain[0] byte strings, in order of first appearance
    info: dict


def _family(name, pairs, **info):
    return Family(name, pairs, distinct(chain0_of(pairs)), info)


LENGTHS = (list(range(530, 611)) + list(range(1008, 1042)) + list(range(2032, 2066)) + list(range(3056, 3090)) + [5003])
# Chain[0] as the last thing in the blob (nothing but the caller's pad behind it): every residue mod 16 twice around 1 KiB,
# the 2 KiB and 3 KiB edges, the longest one
LAST_IN_BLOB = list(range(1008, 1040)) + [545, 2047, 2048, 2049, 3071, 3072, 3073, 5003]
FORMS = ("x509ff", "x509", "precert")


@functools.lru_cache(maxsize=None)
def length_certs():
    return {n: ca_cert(n, "len%d" % n) for n in LENGTHS}


@functools.lru_cache(maxsize=None)
def lengths():
    """One valid CA certificate at every length of LENGTHS, each Chain[0] of three entries (FORMS) at different lanes.
    info["last"]: small batches that END with Chain[0] of the lengths of LAST_IN_BLOB."""
    certs = length_certs()
    pairs = []
    for rep, form in enumerate(FORMS):
        order = LENGTHS if rep != 1 else LENGTHS[::-1]
        for k, n in enumerate(order):
            pairs.append(entry(7 * rep + k, certs[n], form))
    last = []
    for k, n in enumerate(LAST_IN_BLOB):
        other = certs[LENGTHS[(5 * k) % len(LENGTHS)]]
        last.append([entry(k, other, "precert"), entry(k + 1, certs[n], "x509ff"), entry(k + 2, certs[n], "x509")])
    return _family("lengths", pairs, by_length=certs, last=last)


@functools.lru_cache(maxsize=None)
def short():
    """Chain[0] of every length 1 … 47, junk that does not parse; pairs that differ in the LAST octet at 31, 32 and 33 (all
    hashed there) and pairs that differ only in octet 16 at 32 … 47 (inside the hashed tail at 32, outside head and tail from
    33 up: info["same_hash"] says which pairs share a hash)."""
    rng = _rng("short")
    junk = []
    for n in range(1, 48):
        junk.append(b"\xa5" + rng.randbytes(n - 1))
    pairs16 = []
    for n in (31, 32, 33):
        a = b"\xa5" + rng.randbytes(n - 1)
        junk += [a, a[:-1] + bytes([a[-1] ^ 0x10])]
    for n in range(32, 48):
        a = b"\xa5" + rng.randbytes(n - 1)
        b = a[:16] + bytes([a[16] ^ (1 << (n % 8))]) + a[17:]
        junk += [a, b]
        pairs16.append((a, b))
    same = {}
    for a, b in pairs16:
        same[len(a)] = quick_hash(a) == quick_hash(b)
        assert same[len(a)] == (len(a) >= 33), len(a)
    pairs = []
    for rep, form in enumerate(("x509", "x509ff", "precert")):
        for k, j in enumerate(junk if rep != 1 else junk[::-1]):
            pairs.append(entry(3 * rep + k, j, form))
    return _family("short", pairs, same_hash=same, pairs16=pairs16)


def twin_positions(n):
    """The octet positions of a base of n octets at which a twin differs: (mandatory ones, all).  The rest is a stride, 17
    through the certificate's structure and 3 through the signature's filler from FILLER_FROM on (both coprime to 16 and
    64: every residue mod 16 and every lane (p // 16) mod 64 occurs).  Every octet of the filler parses, which is what keeps
    the share of twins that the oracle takes for issuers above 95 %: about fifty of the structure's do not."""
    must = set(range(64)) | set(range(n - 64, n))
    must |= {p for p in range(n) if p % 16 in (0, 15)}
    for edge in (1024, 2048, 3072):
        if edge + 16 < n:
            must |= set(range(edge - 16, edge + 17))
    stride = set(range(64, FILLER_FROM, 17)) | set(range(FILLER_FROM, n - 64, 3))
    return sorted(must), sorted(must | stride)


TWIN_BASES = (2131, 3203)
FILLER_FROM = 480          # both bases: tbsCertificate, signatureAlgorithm and the BIT STRING's header end before it


@functools.lru_cache(maxsize=None)
def twins():
    """Per base certificate (TWIN_BASES octets): one twin per position of twin_positions, base ^ (1 << b) there with b
    cycling over 0 … 7; every twin Chain[0] of two entries at different lanes and log indices, the base before, between and
    after.  info: bases, twins[(base index, position, bit, twin bytes)], in_spki (twin numbers whose octet lies in the
    SubjectPublicKeyInfo: another issuer ID, where it still parses), shuffled (a seeded permutation of the entries)."""
    pairs, bases, tw, in_spki = [], [], [], set()
    k = 0
    for bi, n in enumerate(TWIN_BASES):
        mod = modulus("twin%d" % n)
        base = ca_cert(n, "twin%d" % n, n=mod)
        s_off, s_len = spki_of(base, mod)
        bases.append(base)
        mine = []
        for t, p in enumerate(twin_positions(n)[1]):
            c = bytearray(base)
            c[p] ^= 1 << (t % 8)
            if s_off <= p < s_off + s_len:
                in_spki.add(len(tw))
            tw.append((bi, p, t % 8, bytes(c)))
            mine.append(bytes(c))
        pairs.append(entry(k, base, "x509ff"))
        first = len(pairs)
        for rep, form in enumerate(("x509", "precert")):
            for t, c in enumerate(mine):
                pairs.append(entry(k + t, c, form))
            k += len(mine)
            pairs.append(entry(k, base, "x509" if rep else "precert"))
            if rep == 0 and (len(pairs) - first) % 64 == 0:           # (the second carrier of a twin sits at another lane)
                pairs.append(entry(k + 1, base, "x509ff"))
    perm = list(range(len(pairs)))
    _rng("twins", "shuffle").shuffle(perm)
    return _family("twins", pairs, bases=bases, twins=tw, in_spki=in_spki, shuffled=perm)


EDGE_LENGTHS = (list(range(530, 546)) + list(range(1041, 1057)) + list(range(1500, 1516)) + list(range(2065, 2081)) +
                list(range(3089, 3105)))


@functools.lru_cache(maxsize=None)
def edges():
    """The last octets that only the comparison sees.  The hash covers the last sixteen octets, so the masked last chunk
    never decides a match on its own; the chunk in front of it does.  Per length of EDGE_LENGTHS (every residue mod 16 with
    that chunk in the first row, the second row — right behind 1 KiB and in its middle — and the first two turns of the
    loop): a certificate and two twins of it, one differing in octet len - 17 (the last one outside the hashed tail), one in
    octet 16 (the first one outside the hashed head).  info["triples"]: (base, twin at len - 17, twin at 16)."""
    triples, pairs = [], []
    for n in EDGE_LENGTHS:
        base = ca_cert(n, "edge%d" % n)
        hi = base[:n - 17] + bytes([base[n - 17] ^ (1 << (n % 8))]) + base[n - 16:]
        lo = base[:16] + bytes([base[16] ^ (0x80 >> (n % 8))]) + base[17:]
        triples.append((base, hi, lo))
    k = 0
    for rep, form in enumerate(("x509", "precert", "x509ff")):
        for t in triples:
            for c in (t[rep:] + t[:rep]):                                 # (a certificate's three carriers sit at three lanes)
                pairs.append(entry(k, c, form))
                k += 1
    return _family("edges", pairs, triples=triples)


TABLE_SLOTS = 1024          # the issuer table of an engine with max_issuers <= 256 (engine/lifecycle.inc)
TABLE_MAX_ISSUERS = 256
TABLE_HOMES = (1021, 1021, 1021, 1022, 1022, 1023, 1023)


@functools.lru_cache(maxsize=None)
def table():
    """For an engine with max_issuers = 256: certificates whose home slots are TABLE_HOMES — registered in that order their
    probe run wraps from the last slot to slot 0 — found by search over the signature's last sixteen octets; two certificates
    of DIFFERENT lengths with equal upper hash halves and equal home slots (the candidate loop steps over the first); a twin
    of the first certificate, registered (both then carry HT_TWIN: the bytes decide in both modes), and a second twin of it
    that is NOT registered.  info: register (the order), homes, cross (the two lengths' pair), stranger."""
    rng = np.random.default_rng(SEED)
    la, lb = 598, 1030
    a, b = ca_cert(la, "tableA"), ca_cert(lb, "tableB")
    n = 1 << 22
    ta = rng.integers(0, 1 << 32, (n, 4), dtype=np.uint64)
    tb = rng.integers(0, 1 << 32, (n, 4), dtype=np.uint64)
    ha, hb = quick_hash_tails(la, a[:16], ta), quick_hash_tails(lb, b[:16], tb)
    mask = U(TABLE_SLOTS - 1)

    def with_tail(c, t):
        return c[:-16] + t.astype("<u4").tobytes()
    wrap = []
    for k, home in enumerate(TABLE_HOMES):
        at = np.nonzero((ha[:1 << 16] & mask) == U(home))[0]
        wrap.append(with_tail(a, ta[at[k]]))                           # (the k-th hit: distinct tails within one home)
    sa, sb = ((ha >> U(32)) << U(10)) | (ha & mask), ((hb >> U(32)) << U(10)) | (hb & mask)
    common = np.intersect1d(sa, sb)
    assert len(common) >= 1, "search space too small"
    ia, ib = int(np.nonzero(sa == common[0])[0][0]), int(np.nonzero(sb == common[0])[0][0])
    cross = (with_tail(a, ta[ia]), with_tail(b, tb[ib]))
    assert int(ha[ia]) != int(hb[ib]) and int(ha[ia]) >> 32 == int(hb[ib]) >> 32
    mid = la // 2
    twin = wrap[0][:mid] + bytes([wrap[0][mid] ^ 0x04]) + wrap[0][mid + 1:]
    stranger = wrap[0][:mid + 7] + bytes([wrap[0][mid + 7] ^ 0x80]) + wrap[0][mid + 8:]
    register = wrap + [twin] + list(cross)
    homes = [quick_hash(c) & (TABLE_SLOTS - 1) for c in register]
    pairs = []
    for rep, form in enumerate(FORMS):
        for k, c in enumerate(register + [stranger]):
            pairs.append(entry(11 * rep + k, c, form))
    return _family("table", pairs, register=register, homes=homes, cross=cross, stranger=stranger,
                   hashes=[int(ha[ia]), int(hb[ib])])


N_CLAIMS = 26000
N_CLAIM_REPEATS = 2000


@functools.lru_cache(maxsize=None)
def claims():
    """N_CLAIMS distinct small valid CA certificates (one template, distinct in the signature's last sixteen octets, so
    distinct hashes: more than PEND_SLOTS + UNREG_CAP), each Chain[0] of one entry; N_CLAIM_REPEATS of them come once more,
    half of those in the middle of the batch and half at its end."""
    assert N_CLAIMS > PEND_SLOTS + UNREG_CAP
    tmpl = ca_cert(561, "claims")
    rng = _rng("claims")
    certs = [tmpl[:-16] + rng.randbytes(10) + k.to_bytes(6, "little") for k in range(N_CLAIMS)]
    half = N_CLAIMS // 2
    rep_a = rng.sample(range(half), N_CLAIM_REPEATS // 2)
    rep_b = rng.sample(range(N_CLAIMS), N_CLAIM_REPEATS // 2)
    order = list(range(half)) + rep_a + list(range(half, N_CLAIMS)) + rep_b
    pairs = [entry(i, certs[k], "x509") for i, k in enumerate(order)]
    return Family("claims", pairs, certs, {"order": order})


WAVE_SIZES = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097)
CLASSES = ("registered", "unregistered", "empty", "undecodable", "precert")
WAVE_REGISTERED = (533, 540, 1030, 2050)      # lengths of `lengths` certificates
WAVE_UNREGISTERED = (531, 547, 1023, 3060)


def wave_class(batch, i):
    """Lane class of entry i of batch number `batch`: (lane + row + batch) mod 5 — five consecutive rows put every class at
    every lane — except that every eighth row of 64 is ONE class throughout (waves whose lanes all skip the match, or all
    enter it)."""
    row = i // 64
    if row % 8 == 7:
        return CLASSES[(row // 8 + batch) % 5]
    return CLASSES[(i + 2 * row + batch) % 5]


@functools.lru_cache(maxsize=None)
def waves():
    """Batches of WAVE_SIZES entries around a wave (64), a workgroup (256) and DECODE_PER_BLOCK (2048).  info["batches"]:
    the pairs per batch; info["registered"]: what a test registers beforehand; .pairs is all batches in a row."""
    certs = length_certs()
    reg, unreg = [certs[n] for n in WAVE_REGISTERED], [certs[n] for n in WAVE_UNREGISTERED]
    batches, classes = [], []
    for bi, n in enumerate(WAVE_SIZES):
        pairs, cls = [], []
        for i in range(n):
            c = wave_class(bi, i)
            cls.append(c)
            if c == "registered":
                pairs.append(entry(i, reg[(i // 5) % 4], "x509ff" if i % 2 else "x509"))
            elif c == "unregistered":
                pairs.append(entry(i, unreg[(i // 5) % 4], "x509" if i % 2 else "x509ff"))
            elif c == "empty":
                pairs.append(entry(i, None, "precert" if i % 3 == 0 else "x509"))
            elif c == "undecodable":
                pairs.append(undecodable(i // 5))
            else:
                pairs.append(entry(i, (reg + unreg)[(i // 5) % 8], "precert"))
        batches.append(pairs)
        classes.append(cls)
    return _family("waves", [p for b in batches for p in b], batches=batches, classes=classes, registered=reg)


FAMILIES = {"lengths": lengths, "edges": edges, "short": short, "twins": twins, "table": table, "claims": claims, "waves": waves}
