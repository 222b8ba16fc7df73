"""Certificates that put the Names' string rules (strict_strings) to every octet, length and window position (test helper,
no test; pure tests/der.py, no GPU, seeded and deterministic).  der_walk.h checks the character set of each string value
where the walk meets it: value_strings_ok reads sixteen octets per step through the map kernels' window, masks what lies
behind the value, judges PrintableString and NumericString four octets at a time (string_word_ok), carries a UTF-8
automaton across 4-octet words (utf8_exact_ok) and asks for the window every 64 octets of a value.  Wrong, each of these is
silent: a precertificate keeps or loses its place, an issuer registers as valid or not, and nothing else shows.

THE RULES, stated here once more and independently of the oracle and of the product (finding()): Go's encoding/asn1 over an
AttributeTypeAndValue's value —
  PrintableString 0x13   A-Z a-z 0-9 space ' ( ) + , - . / : = ? * &
  NumericString   0x12   0-9 and space
  IA5String       0x16   every octet below 0x80
  UTF8String      0x0c   bytes.decode("utf-8") succeeds (Python's strict decoder rejects what utf8.Valid rejects: overlong
                         forms, surrogates, values above U+10FFFF, truncated sequences)
  every other tag        no finding (T61String 0x14, BMPString 0x1e, OCTET STRING 0x04 are swept as such)
Every certificate carries the verdict these rules give over the values the builder put into it (Family.expect: the OR of
SF_* bits, the oracle's numbering); tests/test_strings_corpus_cpu.py holds the oracle and the host build of the walk to it.

LAYOUT.  Every case is built twice, as an X509 entry and as a precertificate entry (entry types 0 and 1, interleaved, each
with a serial of its own): neighbouring lanes of a wave differ in whether they run the check at all, and the X509 copy
must be kept whatever its strings hold.  TWINS (Family.pairs: (i, j, kind)) have equal length, share their serial and differ
in a few octets at the place under test; the first is the clean one.  Fillers are octets of the type's own set: "1" for a
NumericString, "a" otherwise.  Keys are RSA (the window simulation evaluates EC points through the window).

Families (each at most 8000 certificates):
  alphabet        the seven tags x every octet 0..255 x the four byte lanes of a word (value indices 0..3 of an 8-octet
                  value).  An octet outside its type's set has a certificate of its own per lane; the octets INSIDE the set
                  share one certificate per octet (four RDNs, one per lane: no lane may object), the unchecked tags one per
                  two octets — 256 x 4 x 7 single certificates would be 14 336 with both entry types.  Then the boundary
                  octets of the two SWAR sets and their neighbours outside, each with the lanes next to it holding 0x20 and
                  0xff (0x7f once masked: the carry argument of string_word_ok; the twin of an in-set octet between 0xff is
                  the same between 0x20).  Octets >= 0x80 whose 7-bit image is in the set (0xc1 -> A, 0xb1 -> 1) are marked
                  "masked": only the `ascii` verdict catches them.
  lengths         the four checked tags x value lengths 0..80, 127, 128, 129, 255, 256, 257, 300: clean, one bad octet at
                  the first, the last, the 15th, 16th, 63rd, 64th index; a clean value with ff 5f 80 bf behind it inside
                  the AttributeTypeAndValue, in the 12-octet fast form of walk_name and behind a 9-octet OID (not the fast
                  form); UTF8String: a value that ends in a complete 2-, 3-, 4-octet sequence, and the same cut by one octet
                  with the missing octet behind the value (a finding: the value ends inside a sequence)
  utf8_edges      the boundary table (UTF8_VALID, UTF8_INVALID, the invalid leads, lone continuations, every continuation
                  octet of a valid sequence replaced by 7f and by c0) behind 0..19 ASCII octets and followed by 0..4 — each
                  entry at EVERY offset 0..19, its tail cycling through 0..4 on the way (every tail four times; the full
                  cross product would be 18 200 certificates); a replaced continuation is the twin of its valid sequence at
                  the same place; and 2000 seeded random strings of 0..40 octets over RANDOM_ALPHABET (built of valid
                  sequences, half of them then hurt in one octet)
  positions       values of 300 octets, each checked tag, in the subject and in the issuer, the bad octet at every index
                  (UTF8String: a 3-octet sequence whose middle octet is no continuation); values of 700 octets with the bad
                  octet within 2 of every multiple of 64 and at the last index; the 300-octet value inside a multi-valued
                  RDN and behind a 9-octet OID (every 11th index); five 64-octet RDNs in the fast form with the bad octet at
                  every index of every value
  positions_edge  issuer values of 260 octets behind serials of 1..20 octets, the bad octet at every certificate offset
                  180..280 (both geometries' first windows end at 224; from serial to serial the bad octet's index takes
                  every residue mod 16); subject values of 260 octets with the bad octet at every offset 200..250 from the
                  subject Name's contents (where the subject's refilled window begins, give or take 3)
                  — a family of its own only to keep positions under 8000 certificates
  positions_end   values of 33..48 octets whose END lies at every certificate offset 216..232 (issuer) and at every offset
                  200..228 from the subject Name's contents, clean and with the LAST octet bad: the last word of a value is
                  read four octets wide, so within three octets of the window's end that read reaches across it — clamped
                  by WinReaderS::ld4, which must raise `miss` (served silently, the bad octet would be a filler)
  rel_name        the lengths table (lengths 0..40) as the value of an attribute inside a distribution point's
                  nameRelativeToCRLIssuer (walk_rdns: counts under strict_extensions and strict_strings together; the
                  verdict is the oracle's ext_string_findings)
issuers()         CA certificates whose own subject or issuer Name carries the alphabet cases of PrintableString and
                  UTF8String and the utf8_edges table at every offset 0..19 (tail cycling), each with a key of its own and
                  one ordinary leaf under it
"""
import functools
from dataclasses import dataclass, field

import numpy as np

from ct_mapreduce_amd import synth
from ct_mapreduce_amd.engine import Batch
from tests import der as D
from tests import geometry_corpus as G
from tests.meta_corpus import dp_ext

FILT = b"Str"                        # the CN filter: every issuer Name here ends in CN = "Str CA"
NOW = synth.BASE_TIME
N_ISSUERS = 3
MAX_CERTS = 8000
SF_PRINTABLE, SF_NUMERIC, SF_IA5, SF_UTF8 = 1, 2, 4, 8        # the oracle's numbering (oracle/oracle.py)
CHECKED = (0x13, 0x12, 0x16, 0x0c)
UNCHECKED = (0x14, 0x1e, 0x04)
TAGS = CHECKED + UNCHECKED
SF_OF = {0x13: SF_PRINTABLE, 0x12: SF_NUMERIC, 0x16: SF_IA5, 0x0c: SF_UTF8}
PRINTABLE = frozenset(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789 '()+,-./:=?*&")
NUMERIC = frozenset(b"0123456789 ")
BAD = {0x13: 0x5f, 0x12: 0x61, 0x16: 0xe1, 0x0c: 0xff}         # one octet outside each set
HOSTILE = bytes.fromhex("ff5f80bf")                            # behind a value: outside every set, and two continuation octets
LONG_OID = bytes.fromhex("2a864886f70d010901")                 # emailAddress, nine octets: never walk_name's fast form
IDS = dict(alphabet=0x41, lengths=0x42, utf8_edges=0x43, positions=0x44, positions_edge=0x45, rel_name=0x46, issuers=0x47,
           positions_end=0x48)

PRINTABLE_EDGES = (0x20, 0x26, 0x3a, 0x3d, 0x3f, 0x41, 0x5a, 0x61, 0x7a)
NUMERIC_EDGES = (0x20, 0x30, 0x39)
LENGTHS = tuple(range(81)) + (127, 128, 129, 255, 256, 257, 300)
BAD_AT = (15, 16, 63, 64)
END_SEQ = {2: bytes.fromhex("c3a9"), 3: bytes.fromhex("e282ac"), 4: bytes.fromhex("f09f9880")}
UTF8_VALID = tuple(bytes.fromhex(h) for h in ("c280", "dfbf", "e0a080", "ed9fbf", "ee8080", "efbfbf", "f0908080", "f48fbfbf"))
UTF8_INVALID = tuple(bytes.fromhex(h) for h in ("e09fbf", "eda080", "f08fbfbf", "f4908080"))
UTF8_LONE = tuple(bytes([b]) for b in (0xc0, 0xc1) + tuple(range(0xf5, 0x100)) + (0x80, 0xbf))
RANDOM_ALPHABET = (0x00, 0x41, 0x7f, 0x80, 0x8f, 0x90, 0x9f, 0xa0, 0xbf, 0xc0, 0xc1, 0xc2, 0xdf, 0xe0, 0xe1, 0xec, 0xed, 0xee, 0xef,
                   0xf0, 0xf1, 0xf3, 0xf4, 0xf5, 0xff)      # the alphabet of tests/test_strings_cpu.py
N_RANDOM = 2000


def finding(tag, value):
    """The SF_* bit a value of this tag earns under the Go stdlib rules, 0 = none."""
    if tag == 0x13:
        return 0 if all(b in PRINTABLE for b in value) else SF_PRINTABLE
    if tag == 0x12:
        return 0 if all(b in NUMERIC for b in value) else SF_NUMERIC
    if tag == 0x16:
        return 0 if all(b < 0x80 for b in value) else SF_IA5
    if tag == 0x0c:
        try:
            bytes(value).decode("utf-8")
            return 0
        except UnicodeDecodeError:
            return SF_UTF8
    return 0


def filler(tag):
    return b"1" if tag == 0x12 else b"a"


def put(value, at, octets):
    """value with `octets` written from index `at` (cut at the value's end)."""
    octets = bytes(octets)[:len(value) - at]
    return value[:at] + octets + value[at + len(octets):]


@dataclass(frozen=True)
class Atv:
    """One AttributeTypeAndValue: the value under test, what lies behind it inside the SEQUENCE, and the type's OID."""
    tag: int
    value: bytes
    trail: bytes = b""
    long_oid: bool = False
    attr: int = 10

    def der(self):
        oid = D.tlv(0x06, LONG_OID) if self.long_oid else D.oid(0x55, 0x04, self.attr)
        return D.seq(oid, D.tlv(self.tag, self.value), self.trail)

    def finding(self):
        return finding(self.tag, self.value)


def rdn_of(*atvs):
    return D.tlv(0x31, b"".join(a.der() for a in atvs))


@dataclass(frozen=True)
class Spec:
    """What a certificate carries: RDNs (each a tuple of Atv: more than one is a multi-valued RDN) in front of the Name's
    CN, in the subject, the issuer, or a distribution point's nameRelativeToCRLIssuer."""
    rdns: tuple
    where: str = "subject"

    def expect(self):
        e = 0
        for r in self.rdns:
            for a in r:
                e |= a.finding()
        return e

    def names(self):
        """(issuer Name, subject Name, extensions or None)"""
        body = [rdn_of(*r) for r in self.rdns]
        issuer, subject, exts = D.name(D.rdn(3, b"Str CA")), D.name(D.rdn(3, b"leaf")), None
        if self.where == "issuer":
            issuer = D.name(*body, D.rdn(3, b"Str CA"))
        elif self.where == "subject":
            subject = D.name(*body, D.rdn(3, b"leaf"))
        else:
            exts = [dp_ext(D.seq(D.tlv(0xa0, D.tlv(0xa1, b"".join(body)))))]
        return issuer, subject, exts

    def cert(self, serial, step=0):
        issuer, subject, exts = self.names()
        return G.make(serial, issuer, D.utctime(G.when(step)), subject, D.rsa_spki(), exts=exts)


def one(tag, value, where="subject", **kw):
    return Spec(((Atv(tag, value, **kw),),), where)


def serial_of(fam_id, k, ln=8):
    """The k-th serial of a family, ln octets, every octet in 01..7f (positive, minimal).  From five octets on they are
    distinct; shorter ones repeat (a repeated key is a known certificate, for the oracle and the engine alike)."""
    digits = bytes(1 + (k // 126 ** j) % 126 for j in (3, 2, 1, 0))
    return (bytes([fam_id]) + b"\x11" * max(0, ln - 5) + digits)[-ln:] if ln >= 5 else digits[-ln:]


@dataclass
class Family:
    name: str
    certs: list = field(default_factory=list)      # (der, issuer_idx, entry_type)
    expect: list = field(default_factory=list)     # per certificate: the SF_* bits the rules give
    pairs: list = field(default_factory=list)      # (i, j, kind): twins, i the clean one
    marks: list = field(default_factory=list)      # per certificate: the builder's bookkeeping (dict)
    cuts = None                                    # (no sequence families here: geometry_corpus.shuffled looks for it)
    _count: int = 0

    def group(self, specs, ln=8, twins=None, **mark):
        """One case: the specs (dicts of their own marks ride along as (spec, dict)) as X509 and as precertificate entries,
        interleaved; the two entry types have a serial each, which the specs of the group share.  twins = kind: specs[0] is
        the clean twin of every other one."""
        serials = [serial_of(IDS[self.name], self._count + et, ln) for et in (0, 1)]
        step = self._count // 2
        self._count += 2
        first = None
        for s in specs:
            spec, own = s if isinstance(s, tuple) else (s, {})
            at = []
            for et in (0, 1):
                at.append(len(self.certs))
                self.certs.append((spec.cert(serials[et], step), step % N_ISSUERS, et))
                self.expect.append(spec.expect())
                self.marks.append(dict(mark, where=spec.where, et=et, **own))
            if twins:
                if first is None:
                    first = at
                else:
                    self.pairs += [(first[et], at[et], twins) for et in (0, 1)]

    def batch(self, order=None):
        idx = range(len(self.certs)) if order is None else order
        return Batch.from_certs([self.certs[i][0] for i in idx], [self.certs[i][1] for i in idx], [self.certs[i][2] for i in idx])


def where_of(k):
    return "subject" if k % 2 == 0 else "issuer"


def lane_value(tag, octet, lane, left=None, right=None):
    """The 8-octet value with `octet` at index `lane` (0..3) and, where given, the lanes next to it inside the word."""
    v = bytearray(filler(tag) * 8)
    v[lane] = octet
    if left is not None and lane > 0:
        v[lane - 1] = left
    if right is not None and lane < 3:
        v[lane + 1] = right
    return bytes(v)


def alphabet_specs(tags=TAGS):
    """[(Spec, mark)] or, for twins, [((clean Spec, mark), (bad Spec, mark))]: what the alphabet family and the issuers
    table are built of.  mark["cover"] lists the (tag, octet, lane) a certificate answers for."""
    out, k = [], 0
    for tag in tags:
        inside = [b for b in range(256) if not finding(tag, lane_value(tag, b, 0))]
        if tag in CHECKED:
            for b in range(256):
                if b in inside:
                    continue
                for lane in range(4):
                    masked = b >= 0x80 and not finding(tag, lane_value(tag, b & 0x7f, lane)) and tag in (0x13, 0x12)
                    out.append((one(tag, lane_value(tag, b, lane), where_of(k)),
                                dict(kind="masked" if masked else "outside", cover=[(tag, b, lane)])))
                    k += 1
            per = 1
        else:
            per = 2
        for i in range(0, len(inside), per):
            octets = inside[i:i + per]
            rdns = tuple((Atv(tag, lane_value(tag, b, lane)),) for b in octets for lane in range(4))
            out.append((Spec(rdns, where_of(k)), dict(kind="inside", cover=[(tag, b, lane) for b in octets for lane in range(4)])))
            k += 1
    for tag, edges, inset in ((0x13, PRINTABLE_EDGES, PRINTABLE), (0x12, NUMERIC_EDGES, NUMERIC)):
        if tag not in tags:
            continue
        octets = sorted(set(edges) | {b + d for b in edges for d in (-1, 1) if b + d not in inset})
        for b in octets:
            for lane in range(4):
                calm = one(tag, lane_value(tag, b, lane, 0x20, 0x20), where_of(k))
                loud = one(tag, lane_value(tag, b, lane, 0xff, 0xff), where_of(k))
                mark = dict(edge=(tag, b, lane), cover=[])
                if b in inset:
                    out.append(((calm, dict(mark, kind="edge_20")), (loud, dict(mark, kind="edge_ff"))))
                else:
                    out += [(calm, dict(mark, kind="edge_20")), (loud, dict(mark, kind="edge_ff"))]
                k += 1
    return out


@functools.lru_cache(maxsize=None)
def alphabet():
    fam = Family("alphabet")
    for item in alphabet_specs():
        if isinstance(item[0], tuple):
            fam.group(list(item), twins="neighbour")
        else:
            fam.group([item])
    return fam


def length_specs(lengths, where_salt=0):
    """The lengths table: [(kind for twins or None, [(Spec, mark)…])] — one group each."""
    out = []
    for t, tag in enumerate(CHECKED):
        f, bad = filler(tag), BAD[tag]
        for n in lengths:
            where = where_of(n + t + where_salt)
            clean = f * n
            at = sorted({i for i in (0, n - 1) + BAD_AT if 0 <= i < n})
            group = [(one(tag, clean, where), dict(kind="clean", tag=tag, n=n))]
            group += [(one(tag, put(clean, i, [bad]), where), dict(kind="bad", tag=tag, n=n, at=i)) for i in at]
            out.append(("octet" if at else None, group))
            for long_oid in (False, True):
                out.append((None, [(one(tag, clean, where, trail=HOSTILE, long_oid=long_oid),
                                    dict(kind="trail", tag=tag, n=n, long_oid=long_oid))]))
            if tag == 0x0c:
                for q, seq in END_SEQ.items():
                    if n < q:
                        continue
                    whole = f * (n - q) + seq
                    out.append((None, [(one(tag, whole, where), dict(kind="utf8_end", tag=tag, n=n, seq=q))]))
                    out.append((None, [(one(tag, whole[:-1], where, trail=seq[-1:]), dict(kind="utf8_cut", tag=tag, n=n, seq=q))]))
    return out


@functools.lru_cache(maxsize=None)
def lengths():
    fam = Family("lengths")
    for kind, group in length_specs(LENGTHS):
        fam.group(group, twins=kind)
    return fam


def utf8_table():
    """[(name, octets, valid, twin: the valid sequence it was made of, or None)]"""
    out = [("valid", s, True, None) for s in UTF8_VALID] + [("invalid", s, False, None) for s in UTF8_INVALID]
    out += [("lone", s, False, None) for s in UTF8_LONE]
    for s in UTF8_VALID:
        for i in range(1, len(s)):
            for r in (0x7f, 0xc0):
                out.append(("replaced", put(s, i, [r]), False, s))
    return out


def utf8_places():
    """(entry index, octets in front, octets behind): every entry at every offset 0..19; over the twenty its tail takes
    every length 0..4 four times."""
    return [(e, pre, (pre + e) % 5) for e in range(len(utf8_table())) for pre in range(20)]


def random_utf8(rng):
    """A string of 0..40 octets over RANDOM_ALPHABET: valid sequences of its octets; every second one hurt in one octet."""
    cont = (0x80, 0x8f, 0x90, 0x9f, 0xa0, 0xbf)
    units = [(0x00,), (0x41,), (0x7f,)] + [(a, c) for a in (0xc2, 0xdf) for c in cont]
    units += [(0xe0, c, d) for c in (0xa0, 0xbf) for d in cont] + [(a, c, d) for a in (0xe1, 0xec, 0xee, 0xef) for c in cont for d in cont]
    units += [(0xed, c, d) for c in (0x80, 0x8f, 0x90, 0x9f) for d in cont]
    units += [(0xf0, c, d, d) for c in (0x90, 0x9f, 0xa0, 0xbf) for d in cont] + [(a, c, d, c) for a in (0xf1, 0xf3) for c in cont for d in cont]
    units += [(0xf4, c, d, d) for c in (0x80, 0x8f) for d in cont]
    n, v = int(rng.integers(0, 41)), b""
    while len(v) < n:
        u = units[int(rng.integers(0, 3))] if rng.random() < 0.5 else units[int(rng.integers(0, len(units)))]
        if len(v) + len(u) <= n:
            v += bytes(u)
        elif rng.random() < 0.5:
            v += b"A" * (n - len(v))
    if v and rng.random() < 0.5:
        v = put(v, int(rng.integers(0, len(v))), [RANDOM_ALPHABET[int(rng.integers(0, len(RANDOM_ALPHABET)))]])
    assert set(v) <= set(RANDOM_ALPHABET)
    return v


def random_strings():
    rng = np.random.default_rng(20261020)
    return [random_utf8(rng) for _ in range(N_RANDOM)]


def utf8_specs():
    """[(twin kind or None, [(Spec, mark)…])] of the utf8_edges table at its places."""
    table, out = utf8_table(), []
    for k, (e, pre, post) in enumerate(utf8_places()):
        name, s, valid, twin = table[e]
        where = where_of(k)
        mark = dict(kind=name, entry=e, pre=pre, post=post)
        spec = one(0x0c, b"a" * pre + s + b"a" * post, where)
        if twin is None:
            out.append((None, [(spec, mark)]))
        else:
            out.append(("continuation", [(one(0x0c, b"a" * pre + twin + b"a" * post, where), dict(mark, kind="twin")), (spec, mark)]))
    return out


@functools.lru_cache(maxsize=None)
def utf8_edges():
    fam = Family("utf8_edges")
    for kind, group in utf8_specs():
        fam.group(group, twins=kind)
    for k, v in enumerate(random_strings()):
        fam.group([(one(0x0c, v, where_of(k)), dict(kind="random", k=k))])
    return fam


BROKEN3 = bytes([0xe2, 0x61, 0xac])        # a 3-octet sequence whose middle octet is no continuation


def hurt(tag, value, at):
    return put(value, at, BROKEN3 if tag == 0x0c else [BAD[tag]])


def sweep(fam, tag, n, where, indices, shape="plain", ln=8, **mark):
    """One group: the clean value of n octets and the value hurt at each of `indices`."""
    clean = filler(tag) * n

    def spec(v):
        if shape == "multi":        # a multi-valued RDN: the value behind a first attribute of the same SET
            return Spec(((Atv(0x13, b"multi", attr=11), Atv(tag, v)),), where)
        return one(tag, v, where, long_oid=shape == "long_oid")
    group = [(spec(clean), dict(mark, kind="clean", tag=tag, n=n, shape=shape))]
    group += [(spec(hurt(tag, clean, i)), dict(mark, kind="bad", tag=tag, n=n, shape=shape, at=i)) for i in indices]
    fam.group(group, ln=ln, twins="position")


def near_64(n):
    return sorted({m + d for m in range(0, n, 64) for d in range(-2, 3) if 0 <= m + d < n} | {n - 1})


FAST_CHAIN = 5                             # RDNs of 64 octets each, every one in walk_name's 12-octet fast form


@functools.lru_cache(maxsize=None)
def positions():
    fam = Family("positions")
    for tag in CHECKED:
        for where in ("subject", "issuer"):
            sweep(fam, tag, 300, where, range(300))
            sweep(fam, tag, 700, where, near_64(700))
            for shape in ("multi", "long_oid"):
                sweep(fam, tag, 300, where, sorted(set(range(0, 300, 11)) | {299}), shape)
    for k, where in enumerate(("subject", "issuer")):
        tags = [CHECKED[(r + k) % 4] for r in range(FAST_CHAIN)]
        clean = [filler(t) * 53 for t in tags]
        chain = lambda vals: Spec(tuple((Atv(t, v),) for t, v in zip(tags, vals)), where)
        assert all(len(rdn_of(Atv(t, v))) == 64 for t, v in zip(tags, clean))
        group = [(chain(clean), dict(kind="clean", shape="fast_chain"))]
        for r in range(FAST_CHAIN):
            for i in range(53):
                vals = list(clean)
                vals[r] = hurt(tags[r], clean[r], i)
                group.append((chain(vals), dict(kind="bad", shape="fast_chain", rdn=r, at=i, tag=tags[r])))
        fam.group(group, twins="position")
    return fam


EDGE_N = 260
ISSUER_OFFSETS = range(180, 281)           # certificate offsets of the bad octet in the issuer sweep
SUBJECT_OFFSETS = range(200, 251)          # offsets from the subject Name's contents


def value_start(der, tag, n):
    """Certificate offset of the (only) value of n filler octets' first octet."""
    head = D.tlv(tag, filler(tag) * n)[:-n]
    at = der.index(head + filler(tag) * 8)
    assert der.count(head + filler(tag) * 8) == 1
    return at + len(head)


@functools.lru_cache(maxsize=None)
def positions_edge():
    fam = Family("positions_edge")
    for ln in range(1, 21):
        tag = CHECKED[ln % 4]
        probe = one(tag, filler(tag) * EDGE_N, "issuer").cert(serial_of(0x45, 0, ln))
        cv = value_start(probe, tag, EDGE_N)
        sweep(fam, tag, EDGE_N, "issuer", [o - cv for o in ISSUER_OFFSETS], ln=ln, cv=cv, serial_len=ln)
    for ln in range(1, 21):
        tag = CHECKED[(ln + 2) % 4]
        probe = one(tag, filler(tag) * EDGE_N, "subject").cert(serial_of(0x45, 0, ln))
        cv = value_start(probe, tag, EDGE_N)
        cs = cv - 17                       # 31 82 .. .. 30 82 .. .. 06 03 55 04 0a tt 82 .. ..: seventeen octets of headers
        assert probe[cs - 4] == 0x30 and probe[cs] == 0x31
        sweep(fam, tag, EDGE_N, "subject", [o - 17 for o in SUBJECT_OFFSETS], ln=ln, cv=cv, cs=cs, serial_len=ln)
    return fam


END_LENGTHS = range(33, 49)                # sixteen value lengths: every residue mod 16, longer than touch(a, 32) covers
ISSUER_ENDS = range(216, 233)              # certificate offsets of the value's END in the issuer sweep
SUBJECT_ENDS = range(200, 229)             # … from the subject Name's contents


def padded(n, where, tag, fill, bad):
    """A value of n octets behind `fill` octets of two O= RDNs in short form, its last octet bad or not."""
    v = filler(tag) * n
    v = put(v, n - 1, [BAD[tag]]) if bad else v
    front = tuple((Atv(0x0c, b"o" * k, attr=11),) for k in (fill // 2, fill - fill // 2))
    return Spec(front + ((Atv(tag, v),),), where)


@functools.lru_cache(maxsize=None)
def positions_end():
    """The value's END at every offset around the end of the window that holds it, the bad octet its last one: the last
    word of a value is read four octets wide, so a value that ends within three octets of the window's end has a read that
    reaches across it — clamped by WinReaderS::ld4, which must raise `miss`: served silently, the bad octet is a filler."""
    fam = Family("positions_end")
    for n in END_LENGTHS:
        tag = CHECKED[n % 4]
        found = {}
        for ln in (8, 9, 10):                                   # (a header that grows on the way skips an offset: the serial gives it back)
            for fill in range(60, 160):
                end = value_start(padded(n, "issuer", tag, fill, False).cert(serial_of(0x48, 0, ln)), tag, n) + n
                found.setdefault(end, (ln, fill))
        for end in ISSUER_ENDS:
            ln, fill = found[end]
            fam.group([(padded(n, "issuer", tag, fill, False), dict(kind="clean", tag=tag, n=n, end=end)),
                       (padded(n, "issuer", tag, fill, True), dict(kind="bad", tag=tag, n=n, end=end))], ln=ln, twins="end")
    for n in END_LENGTHS:
        tag = CHECKED[(n + 1) % 4]
        for end in SUBJECT_ENDS:
            fill = end - n - 33                                 # three RDN headers of eleven octets in front of the value
            fam.group([(padded(n, "subject", tag, fill, False), dict(kind="clean", tag=tag, n=n, end=end)),
                       (padded(n, "subject", tag, fill, True), dict(kind="bad", tag=tag, n=n, end=end))], twins="end")
    return fam


REL_LENGTHS = tuple(range(41))


@functools.lru_cache(maxsize=None)
def rel_name():
    fam = Family("rel_name")
    for kind, group in length_specs(REL_LENGTHS):
        fam.group([(Spec(s.rdns, "rel"), m) for s, m in group], twins=kind)
    return fam


FAMILIES = dict(alphabet=alphabet, lengths=lengths, utf8_edges=utf8_edges, positions=positions, positions_edge=positions_edge,
                positions_end=positions_end, rel_name=rel_name)


def registered_issuers():
    return G.registered_issuers()


def shuffled(fam, seed=20261020):
    rng = np.random.default_rng([seed, IDS[fam.name]])
    return [int(i) for i in rng.permutation(len(fam.certs))]


@dataclass
class IssuerTable:
    cas: list          # CA certificates, each with a key of its own
    valid: list        # per CA: the rules find nothing in its two Names
    leaves: list       # per CA: (der, entry type) of one ordinary leaf under it
    marks: list


def ca_key(k):
    return D.rsa_spki(n=b"\x00" + b"\xc3" * 253 + k.to_bytes(2, "big") + b"\xc3")


@functools.lru_cache(maxsize=None)
def issuers():
    specs = []
    for item in alphabet_specs((0x13, 0x0c)):
        specs += list(item) if isinstance(item[0], tuple) else [item]
    table = utf8_table()
    for e, (name, s, valid, twin) in enumerate(table):
        for pre in range(20):
            post = (pre + e) % 5
            specs.append((one(0x0c, b"a" * pre + s + b"a" * post), dict(kind=name, entry=e, pre=pre, post=post)))
    out = IssuerTable([], [], [], [])
    for k, (spec, mark) in enumerate(specs):
        body = [rdn_of(*r) for r in spec.rdns]
        own = D.name(*body, D.rdn(3, b"Str CA")) if k % 2 == 0 else D.name(D.rdn(3, b"Str CA"))
        above = D.name(*body, D.rdn(3, b"Str Root")) if k % 2 == 1 else D.name(D.rdn(3, b"Str Root"))
        out.cas.append(D.cert(serial=serial_of(IDS["issuers"], k), subject=own, issuer=above, exts=[D.BC_CA], spki=ca_key(k)))
        out.valid.append(spec.expect() == 0)
        leaf = G.make(serial_of(IDS["issuers"], 100000 + k), D.name(D.rdn(3, b"Str CA")), D.utctime(G.when(k)), D.name(D.rdn(3, b"leaf")),
                      D.rsa_spki())
        out.leaves.append((leaf, k % 2))
        out.marks.append(dict(mark, where="subject" if k % 2 == 0 else "issuer"))
    return out
