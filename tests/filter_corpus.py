"""Certificates and filter strings that put the issuer CN filter (certIsFilteredOut filter 3, cmd/ct-fetch/ct-fetch.go:57-69)
to every piece length, Name shape and window edge (test helper, no test; pure tests/der.py, no GPU, seeded and deterministic).
The product restates the filter in three parts: ctmr_set_filter (engine/map.inc) cuts the string into at most 64 pieces,
zero padded to words, 1024 words in all; walk_name<CN> (der_walk.h) picks the CommonName through a 12-octet fast form and a
general form; cn_prefix_match compares word by word with a mask on the last word, through whichever reader the kernel uses
— and calls no touch() of its own: walk_name asks for 32 octets per RDN step, a longer piece reads past that.  A read
served from the wrong bytes WITHOUT a miss is silent: the record says PASS or FILTERED_CN.

THE MODEL, written from the reference's text and from nothing else (never from the device, the oracle or the host walk):

    skip = len(filt) != 0 and not any((cn or b"").startswith(p) for p in filt.split(b","))

over the EFFECTIVE issuer CN every certificate records by construction (Cert.cn: bytes, or None when the Name has none),
and status() — the if-chain of insertCTWorker: CA, expired, CN, then no issuer, then issuer parse error.
tests/test_filter_corpus_cpu.py holds the oracle and the host build of the walk to it.

A family is a list of certificates and a SEQUENCE of cases: a case is one setting (filter, log_expired, now) and the
certificates mapped under it as one batch.  A case whose setting ctmr_set_filter must REFUSE (Setting.refused) is mapped
under the setting in force before it.  Families, each the smallest that still reaches its edge:
  prefix   CN = P[:c], c = 0..72, 126..130, 254..257 (P: 257 seeded octets without ','; T61String, the one string type in
           which strict_strings accepts 0x00 and octets >= 0x80 — P has both) under the one-piece filters P[:p], p = 0..72,
           127, 128, 129, 255, 256, 257; for each p >= 1 the near-miss pieces — one octet changed at 0, p − 1, p − 2 and at
           the first octet of the last word — joined into one filter, and twin CNs of length p that carry the same change:
           each near-miss piece matches exactly one certificate of the family
  address  a 23-octet CN, and the same with octet j = 0..22 changed, behind serials of 1..20 octets (the CN's certificate
           offset takes every residue mod 4 and mod 16) under the pieces A[:p], p = 1..23; views lead the payload by
           5p mod 16 octets: the payload starts at every address mod 16
  window   geometry_corpus's `front` method: an O= filler in front of the CN moves it octet by octet; piece lengths 1, 3, 4,
           5, 8, 16, 17, 33, 40, 64; equal-length twins whose CNs differ only at octet p − 1 (the piece's last) or only at
           octet 0; the filler is swept so that the differing octet, and the CN's first octet, each lie at every
           certificate offset 213 .. 232 — both geometries' first windows (224 octets from the certificate; 216 from 8
           octets in) end at 224 minus the payload address mod 4; views lead by 0, 5 and 12.  Filler and CN are
           T61Strings and the pairs are X509 and precertificate entries in turn: the map kernels check the Names' strings
           for precertificates only, and a checked string type would move the window in front of the compare
  names    which CommonName is used: none, empty, two in two RDNs (twins: the filter matches only the first / only the
           last), two in one multi-valued RDN, a string CN followed and preceded by a 2.5.4.3 value of tag 04, 1e, 1c, 02,
           a CN only in the subject, the attribute OIDs 55 04 03 01, 55 04 2a and 55 04 with a matching value, each of the
           five string tags, CNs of 127 and 128 octets, a short CN beside a second attribute of 200 octets (long-form SET)
           and in front of 200 octets inside its AttributeTypeAndValue (long-form SEQUENCE).
           The rule for the non-string 2.5.4.3 values is the PROJECT's stated one (der_walk.h string_tag: only UTF8String,
           NumericString, PrintableString, T61String and IA5String values count): it cannot be checked against Go here.
  lists    strings.Split semantics: "", ",", ",x", "x,", "x,,y", " x", "x ", a piece equal to the whole CN, duplicate
           pieces, 64 pieces with the only match at index 0, 31, 63 and with none, 64 pieces of 61..64 octets (exactly 1024
           words) matching in the last, one word more and 65 pieces (refused), a piece with 0x00 and 0xff
  order    CA x expired x CN match x issuer {registered, out of range, does not parse} x {X509, precertificate} under
           log_expired off and on; a certificate that does not parse; CTMR_ENTRY_INVALID
  switch   settings applied in turn to one engine: filters, log_expired, now; a refused one; a return to the first
"""
import datetime
import functools
from dataclasses import dataclass, field

import numpy as np

from ct_mapreduce_amd import synth, _native as N
from ct_mapreduce_amd.engine import Batch
from tests import der as D
from tests.geometry_corpus import bc, make, subj
from tests.meta_corpus import issuers

NOW = synth.BASE_TIME
ST_PASS, ST_PARSE_ERROR, ST_FILTERED_CA, ST_FILTERED_EXPIRED, ST_FILTERED_CN, ST_NO_ISSUER, ST_ISSUER_PARSE_ERROR, \
    ST_ENTRY_DECODE_ERROR = range(8)
IDS = dict(prefix=0x31, address=0x32, window=0x33, names=0x34, lists=0x35, order=0x36, switch=0x37)
T61 = 0x14
# the registered issuers: three that parse and one that does not (cut short: its outer length overruns it)
N_GOOD_ISSUERS = 3
BAD_ISSUER, OUT_OF_RANGE = 3, 9
ISSUER_KINDS = ("registered", "range", "bad")
FINE, GONE = "270615120000Z", "200615120000Z"          # notAfter: not expired / expired at NOW


def registered_issuers():
    return issuers(N_GOOD_ISSUERS) + [D.cert(serial=b"\x2f", exts=[D.BC_CA])[:-3]]


def unix(utc):
    return int(datetime.datetime.strptime(utc, "%y%m%d%H%M%SZ").replace(tzinfo=datetime.timezone.utc).timestamp())


# ------------------------------------------------------------------ the model
def cn_skips(filt, cn):
    """ct-fetch.go:57-69: skip unless the filter is empty or strings.HasPrefix(Issuer.CommonName, piece) for some piece of
    strings.Split(filter, ",") — a Name without CommonName has the empty string there."""
    return len(filt) != 0 and not any((cn or b"").startswith(p) for p in filt.split(b","))


@dataclass(frozen=True)
class Setting:
    filt: bytes = b""
    log_expired: bool = False
    now: int = NOW
    refused: bool = False          # ctmr_set_filter must answer CTMR_E_INVAL and leave the earlier setting in force


@dataclass
class Cert:
    der: bytes
    issuer_idx: int
    et: int
    cn: object                     # the effective issuer CN: bytes, or None
    ca: bool = False
    not_after: int = unix(FINE)
    parses: bool = True
    issuer: str = "registered"     # ISSUER_KINDS
    mark: dict = field(default_factory=dict)


def status(c, s):
    """insertCTWorker's order (ct-fetch.go:198-225) with certIsFilteredOut's (:44-70) inside: an entry that never decoded,
    a certificate that does not parse, CA, expired, CN, no issuer, issuer parse error."""
    if c.et == N.ENTRY_INVALID:
        return ST_ENTRY_DECODE_ERROR
    if not c.parses:
        return ST_PARSE_ERROR
    if c.ca:
        return ST_FILTERED_CA
    if c.not_after < s.now and not s.log_expired:
        return ST_FILTERED_EXPIRED
    if cn_skips(s.filt, c.cn):
        return ST_FILTERED_CN
    if c.issuer == "range":
        return ST_NO_ISSUER
    if c.issuer == "bad":
        return ST_ISSUER_PARSE_ERROR
    return ST_PASS


@dataclass
class Case:
    setting: Setting
    idx: list                      # the certificates of the batch, in entry order
    lead: int = 0                  # views: octets in front of the first certificate
    mark: dict = field(default_factory=dict)


@dataclass
class Family:
    name: str
    certs: list = field(default_factory=list)
    cases: list = field(default_factory=list)
    views: bool = False            # the GPU test also maps the cases as entry views, ascending and reversed
    _count: int = 0

    def serial(self, ln=4):
        """ln octets: the family's number, then a counter (ln >= 4; shorter serials are the caller's)."""
        self._count += 1
        return (bytes([IDS[self.name]]) + self._count.to_bytes(3, "big") + b"\x55" * 16)[:ln]

    def add(self, issuer_name, cn, *, serial=None, et=0, ca=False, not_after=FINE, issuer="registered", subject=None, der=None,
            parses=True, **mark):
        k = len(self.certs)
        idx = {"registered": k % N_GOOD_ISSUERS, "range": (OUT_OF_RANGE, N.NO_ISSUER)[k % 2], "bad": BAD_ISSUER}[issuer]
        if der is None:
            der = make(serial or self.serial(), issuer_name, D.utctime(not_after), subject or subj(), D.rsa_spki(),
                       exts=[bc(ca)])
        self.certs.append(Cert(der, idx, et, cn, ca, unix(not_after), parses, issuer, mark))
        return k

    def case(self, setting, idx=None, lead=0, **mark):
        self.cases.append(Case(setting, list(range(len(self.certs))) if idx is None else list(idx), lead, mark))

    def batch(self, case):
        cs = [self.certs[i] for i in case.idx]
        return Batch.from_certs([c.der for c in cs], [c.issuer_idx for c in cs], [c.et for c in cs])

    def in_force(self):
        """[(case, the setting in force when its batch is mapped)]: a refused setting changes nothing."""
        out, cur = [], Setting()
        for case in self.cases:
            cur = cur if case.setting.refused else case.setting
            out.append((case, cur))
        return out

    def expected(self, case, setting):
        return np.array([status(self.certs[i], setting) for i in case.idx], np.uint8)


def cn_name(cn, tag=0x0c):
    return D.name(D.rdn(3, cn, tag))


# ------------------------------------------------------------------ prefix
CN_LENGTHS = tuple(range(73)) + tuple(range(126, 131)) + tuple(range(254, 258))
PIECE_LENGTHS = tuple(range(73)) + (127, 128, 129, 255, 256, 257)


def pattern():
    """P: 257 seeded octets without ',' — 0x00, 0xff and 0x80 among the first nine, so that short pieces hold them too."""
    rng = np.random.default_rng(20261021)
    p = bytearray(int(x) for x in rng.integers(0, 256, size=257))
    p[5:9] = b"\x00\xff\x80\x00"
    for k in range(257):
        if p[k] == 0x2c:
            p[k] = 0x2d
    return bytes(p)


P = pattern()


def changed(b, p):
    """Another octet than b, never ',': b + 1 + (the index of piece length p) — every piece length changes an octet its own way."""
    v = (b + 1 + PIECE_LENGTHS.index(p)) % 256
    return v if v != 0x2c else (b + 253) % 256


def near_miss_positions(p):
    return sorted({0, p - 1, max(p - 2, 0), 4 * ((p - 1) // 4)})


def near_miss(p, k):
    return P[:k] + bytes([changed(P[k], p)]) + P[k + 1:p]


@functools.lru_cache(maxsize=None)
def prefix():
    fam = Family("prefix")
    for c in CN_LENGTHS:
        fam.add(cn_name(P[:c], T61), P[:c], kind="base", c=c)
    for p in PIECE_LENGTHS[1:]:
        for k in near_miss_positions(p):
            fam.add(cn_name(near_miss(p, k), T61), near_miss(p, k), kind="twin", p=p, k=k)
    for p in PIECE_LENGTHS:
        fam.case(Setting(P[:p]), kind="piece", p=p)
    for p in PIECE_LENGTHS[1:]:
        fam.case(Setting(b",".join(near_miss(p, k) for k in near_miss_positions(p))), kind="near", p=p)
    return fam


# ------------------------------------------------------------------ address
ADDRESS_CN = b"Address CA 0123456789ab"
SERIAL_LENGTHS = tuple(range(1, 21))


@functools.lru_cache(maxsize=None)
def address():
    assert len(ADDRESS_CN) == 23
    fam = Family("address", views=True)
    for s in SERIAL_LENGTHS:
        for j in range(-1, 23):
            cn = ADDRESS_CN if j < 0 else ADDRESS_CN[:j] + bytes([ADDRESS_CN[j] ^ 0x40]) + ADDRESS_CN[j + 1:]
            # (a subject filler of its own length moves the NEXT certificate: each variant's CN meets every address mod 16)
            fam.add(cn_name(cn), cn, serial=bytes([0x10 + j + 1]) + b"\x55" * (s - 1), subject=subj((3 * s + 5 * j) % 16), s=s, j=j)
    for p in range(1, 24):
        fam.case(Setting(ADDRESS_CN[:p]), lead=5 * p % 16, p=p)
    return fam


# ------------------------------------------------------------------ window
WINDOW_PIECES = (1, 3, 4, 5, 8, 16, 17, 33, 40, 64)
WINDOW_END = 224                   # both geometries: 224 octets from the certificate, 216 from 8 octets in
EDGE = (WINDOW_END - 11, WINDOW_END + 8)           # 8 octets inside (and 3 more: the window begins on a dword of the payload) .. 8 beyond
WINDOW_LEADS = (0, 5, 12)
Q = bytes(0x41 + (7 * i + i // 26) % 26 for i in range(70))        # the pieces are Q[:p]; a CN is Q[:p + 2]


def front_issuer(filler, cn):
    """Filler and CN as T61Strings: strict_strings checks no octet of those and so asks for no window of its own
    (value_strings_ok touches every 64 octets of a UTF8String or a 7-bit string: with such values a precertificate's walk
    under the reference profile moves the window over the filler and pulls the CN in before the compare runs)."""
    return D.name(D.rdn(10, b"o" * filler, T61), D.rdn(3, cn, T61))


def cn_offset(filler, n, serial_len):
    """Certificate offset of the first octet of a CN of n octets under `front`: found by building one."""
    mark = b"\x7f" * n
    return make(b"\x33" * serial_len, front_issuer(filler, mark), D.utctime(FINE), subj(), D.rsa_spki(), exts=[bc(False)]).index(mark)


@functools.lru_cache(maxsize=None)
def window():
    fam = Family("window", views=True)
    for p in WINDOW_PIECES:
        cn = Q[:p + 2]
        at = {}
        for f in range(261):                         # (where a header takes its long form the filler skips an offset: a serial
            for sl in (4, 5):                        #  one octet longer reaches it)
                at.setdefault(cn_offset(f, len(cn), sl), (f, sl))
        first = len(fam.certs)
        for off in range(EDGE[0] - (p - 1), EDGE[1] + 1):     # the CN's first octet at `off`: octet p − 1 reaches the edge first
            if off not in at:
                continue
            for kind, d in (("last", p - 1), ("first", 0)):
                if not EDGE[0] <= off + d <= EDGE[1]:
                    continue
                twin = cn[:d] + bytes([cn[d] ^ 0x20]) + cn[d + 1:]
                s = fam.serial(at[off][1])
                et = (off + (kind == "first")) % 2   # X509 and precertificate entries in turn, for either kind: strict_strings runs per lane
                for value in (cn, twin):             # equal length, one serial: the twins differ in ONE octet
                    fam.add(front_issuer(at[off][0], value), value, serial=s, et=et, p=p, kind=kind, cn_off=off, at=off + d)
                fam.certs[-1].issuer_idx = fam.certs[-2].issuer_idx
        for lead in WINDOW_LEADS:
            fam.case(Setting(Q[:p]), range(first, len(fam.certs)), lead=lead, p=p)
    return fam


# ------------------------------------------------------------------ names
def atv(oid, value, tag=0x0c, behind=b""):
    return D.seq(D.tlv(0x06, oid), D.tlv(tag, value), behind)


def rdn_of(*atvs):
    return D.tlv(0x31, b"".join(atvs))


CN_OID = b"\x55\x04\x03"
ALPHA, BETA = b"Alpha Root", b"Beta Root"
NON_STRING = {0x04: BETA, 0x1e: BETA.decode().encode("utf-16-be"), 0x1c: BETA.decode().encode("utf-32-be"), 0x02: b"\x42\x65"}
STRING_VALUES = {0x0c: ALPHA, 0x12: b"12 345", 0x13: ALPHA, 0x14: ALPHA, 0x16: ALPHA}
NAMES_FILTERS = (b"", b"Alpha", b"Beta", b"Alpha,Beta", b"Gamma", b"Alpha Root", b"Alpha Rootx", b"A", b",", b"12", b"Org",
                 b"Gamma,\x00B", b"B,\x42\x65", b"Alpha Root" + b"x" * 117, b"Alpha Root" + b"x" * 118, b"Alpha Root" + b"x" * 119)


@functools.lru_cache(maxsize=None)
def names():
    fam = Family("names")
    org = D.rdn(10, b"Org")
    fam.add(D.name(org), None, shape="no_cn")
    fam.add(D.name(org, D.rdn(3, b"")), b"", shape="empty_cn")
    fam.add(D.name(D.rdn(3, ALPHA), D.rdn(3, BETA)), BETA, shape="two_rdns")
    fam.add(D.name(D.rdn(3, BETA), D.rdn(3, ALPHA)), ALPHA, shape="two_rdns")
    fam.add(D.name(rdn_of(atv(CN_OID, ALPHA), atv(CN_OID, BETA))), BETA, shape="multi_valued")
    fam.add(D.name(rdn_of(atv(CN_OID, BETA), atv(CN_OID, ALPHA))), ALPHA, shape="multi_valued")
    for tag, value in NON_STRING.items():           # the project's rule (string_tag): not checkable against Go here
        fam.add(D.name(D.rdn(3, ALPHA), D.rdn(3, value, tag)), ALPHA, shape="non_string_behind", tag=tag)
        fam.add(D.name(D.rdn(3, value, tag), D.rdn(3, ALPHA)), ALPHA, shape="non_string_in_front", tag=tag)
        fam.add(D.name(rdn_of(atv(CN_OID, ALPHA), atv(CN_OID, value, tag))), ALPHA, shape="non_string_behind", tag=tag)
        fam.add(D.name(org, D.rdn(3, value, tag)), None, shape="non_string_alone", tag=tag)
    fam.add(D.name(org), None, subject=D.name(D.rdn(3, ALPHA)), shape="subject_only")
    for oid in (b"\x55\x04\x03\x01", b"\x55\x04\x2a", b"\x55\x04"):
        fam.add(D.name(org, rdn_of(atv(oid, ALPHA))), None, shape="other_oid", oid=oid)
        fam.add(D.name(D.rdn(3, BETA), rdn_of(atv(oid, ALPHA))), BETA, shape="other_oid", oid=oid)
    for tag, value in STRING_VALUES.items():
        fam.add(D.name(org, D.rdn(3, value, tag)), value, shape="string_tag", tag=tag)
    for n in (127, 128):                            # 128: the value's length takes two octets — not the 12-octet fast form
        fam.add(cn_name(ALPHA + b"x" * (n - len(ALPHA))), ALPHA + b"x" * (n - len(ALPHA)), shape="long_cn", n=n)
    big = b"o" * 200
    fam.add(D.name(rdn_of(atv(b"\x55\x04\x0a", big), atv(CN_OID, ALPHA))), ALPHA, shape="long_set")
    fam.add(D.name(rdn_of(atv(CN_OID, ALPHA), atv(b"\x55\x04\x0a", big))), ALPHA, shape="long_set")
    fam.add(D.name(D.rdn(3, BETA), rdn_of(atv(CN_OID, ALPHA, behind=D.tlv(0x04, big)))), ALPHA, shape="long_sequence")
    for f in NAMES_FILTERS:
        fam.case(Setting(f))
    return fam


# ------------------------------------------------------------------ lists
def pieces64(fmt):
    return [fmt % k for k in range(64)]


LONG_PIECES = [bytes([0x61 + k % 26]) * (61 + k % 4) for k in range(63)] + [b"L" * 64]          # 64 x 16 words = 1024
ONE_WORD_MORE = LONG_PIECES[:62] + [b"z" * 65, LONG_PIECES[63]]
LISTS_FILTERS = (b"", b",", b",x", b"x,", b"x,,y", b" x", b"x ", b"xy", b"x,x", b"q,q", b"y,x,y", b"a\x00\xff", b"a\x00,a\xff",
                 b",".join(pieces64(b"p%02d")), b",".join(pieces64(b"q%02d")), b",".join(LONG_PIECES))
LISTS_REFUSED = (b",".join(ONE_WORD_MORE), b",".join(pieces64(b"p%02d") + [b"p64"]))


@functools.lru_cache(maxsize=None)
def lists():
    assert sum((len(p) + 3) // 4 for p in LONG_PIECES) == 1024 and {len(p) for p in LONG_PIECES} == {61, 62, 63, 64}
    assert sum((len(p) + 3) // 4 for p in ONE_WORD_MORE) == 1025 and len(ONE_WORD_MORE) == 64
    fam = Family("lists")
    fam.add(D.name(D.rdn(10, b"Org")), None, what="no_cn")
    for cn in (b"", b"x", b"xy", b"y", b"yx", b" x", b"x ", b"p00-first", b"p31-middle", b"p63-last", b"p64", b"p6", b"L" * 70,
               b"L" * 63, b"z" * 70, b"a" * 70):
        fam.add(cn_name(cn), cn, what="cn")
    for cn in (b"a\x00\xffb", b"a\x00", b"a\xff\x00"):
        fam.add(cn_name(cn, T61), cn, what="octets")
    for f in LISTS_FILTERS:
        fam.case(Setting(f))
    fam.case(Setting(LISTS_REFUSED[0], refused=True))             # … the batch follows the 1024-word filter set before
    fam.case(Setting(b"x"))
    fam.case(Setting(LISTS_REFUSED[1], refused=True))
    return fam


# ------------------------------------------------------------------ order
ORDER_FILT = b"Ord"


def order_certs(fam):
    for ca in (False, True):
        for gone in (False, True):
            for match in (True, False):
                for issuer in ISSUER_KINDS:
                    for et in (0, 1):
                        cn = b"Ord CA" if match else b"Xrd CA"
                        fam.add(cn_name(cn), cn, et=et, ca=ca, not_after=GONE if gone else FINE, issuer=issuer, ca_=ca, gone=gone,
                                match=match)
    good = fam.certs[0].der
    fam.add(None, b"Ord CA", der=good[:-1], parses=False, what="cut short")
    fam.add(None, b"Ord CA", der=make(fam.serial(), cn_name(b"Ord CA"), D.utctime(FINE), subj(), D.rsa_spki(), exts=[bc(False)]),
            et=N.ENTRY_INVALID, what="entry invalid")


@functools.lru_cache(maxsize=None)
def order():
    fam = Family("order")
    order_certs(fam)
    for log_expired in (False, True):
        fam.case(Setting(ORDER_FILT, log_expired))
    return fam


# ------------------------------------------------------------------ switch
@functools.lru_cache(maxsize=None)
def switch():
    fam = Family("switch")
    order_certs(fam)
    for cn in (b"Alt CA", b"", b"Ord"):
        fam.add(cn_name(cn), cn)
    fam.add(D.name(D.rdn(10, b"Org")), None)
    first = Setting(ORDER_FILT, False, NOW)
    for s in (first, Setting(b""), Setting(ORDER_FILT, True), Setting(LISTS_REFUSED[0], refused=True),
              Setting(b"Xyz,Alt", False, NOW + 10 * 365 * 86400), Setting(b"Alt,Ord", False, unix(GONE) - 86400),
              Setting(b"", True, NOW + 10 * 365 * 86400), Setting(LISTS_REFUSED[1], True, 0, refused=True), Setting(b","), first):
        fam.case(s)
    return fam


FAMILIES = dict(prefix=prefix, address=address, window=window, names=names, lists=lists, order=order, switch=switch)
