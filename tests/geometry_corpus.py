"""Certificates that put every verdict-bearing field at every position of the map kernels' windows (test helper, no test;
pure tests/der.py, no GPU, seeded and deterministic).  kernels/readers.h serves the walk from a per-lane LDS window of 224
(STRICT) or 216 octets (fast, beginning 8 octets in), refilled where the walk's hints say, from two register prefetches
(the 32 octets behind the TBSCertificate, the 16 around the key's end) and, for a subjectAltName, in rounds that begin on a
32-octet sector.  A read served wrongly WITHOUT a miss is silent: the record carries the wrong bytes' verdict.

TWINS.  Every geometry appears as a pair of certificates of EQUAL LENGTH that differ only in a few octets at the position
under test (Family.pairs: (i, j, kind); the position is where the two differ) and whose oracle records differ — in status,
exp_hour, or the drop of a precertificate entry over a finding.  A read that returns neighbouring or stale bytes cannot
be right for both.  The twins of a pair share their serial (they are byte-identical elsewhere); serials differ from pair
to pair, are 1..20 octets long and begin with the family's number.  A few certificates have no twin (Family.singles: a
9-octet RSA exponent, a TBSCertificate that overruns its certificate: refused whatever else they hold).
tests/test_geometry_corpus_cpu.py holds every claim made here against the oracle and the positions it reports.

Families (each steps ONE octet at a time; two thirds RSA keys, one third P-256 points, where the family is not about the key):
  front        issuer O= filler 0..260 in front of the CN: CN, validity, subject, SPKI head cross the first window's end
               twins: CN first letter (the filter) / notAfter hour / notAfter tag 17 | 18
  front_rdn    the filler as 1..5 RDNs of 64 octets: walk_name's 64-octet hint fires 1..5 times (+ the CN's)
  subject      subject filler 0..300: SPKI head, key end, extension block move; moduli 128 / 256 / 384 / 512 octets and 250
               (30 82 … 02 81 …: not the shortcut's shape); exponents 03, 010001, 01000001, 8 octets; 9 octets as singles
               twins: exponent 00 | 01 / modulus 00 c3 | 80 c3 (negative: a finding) / modulus 00 c3 | 00 43 (not minimal:
               the shortcut's shape against the general parse, a finding) / notAfter hour (EC keys) — findings as precertificates
  tail         what lies behind the TBSCertificate: ecdsa-with-SHA256 (12), sha256WithRSA (15), RSASSA-PSS (67), a 30-octet
               AlgorithmIdentifier (unknown OID + OCTET STRING) at subject fillers 0..63, and AlgorithmIdentifiers of 10..40 octets
               twins: signatureValue pad 0 | 8 / tag 03 | 04 / the outer AlgorithmIdentifier's length one too large
  tail_last    the same four as the LAST certificate of a small payload, and TBSCertificates that overrun theirs by 1..40
  ext          subjectKeyIdentifier of 0..250 octets in front of basicConstraints (critical present / absent), and behind it
               twins: cA ff | 00 / critical ff | 01 (no DER BOOLEAN)
  ext_unknown  1..24 small unknown extensions in front of basicConstraints
  ext_crl      the subjectKeyIdentifier filler, basicConstraints, then cRLDistributionPoints (the memo pre-check's window)
  san          subjectAltName of 2..700 octets of dNSNames, basicConstraints behind it
               twins: cA ff | 00 (X509 entries) / the last elements 82 03 … 87 04 … | 82 02 … 87 05 … (precertificates: the
               bad iPAddress length is a finding)
  san_long     one long-form element (82 81 80 …) at each of the first 40 positions
  small        unknown key algorithm, key of 1..40 octets, total length 90..215 and 250..262 (30 7x / 30 81 / 30 82 headers;
               130 and 259 are lengths no DER element has): the neighbour's bytes lie in the window, and under the fast
               geometry the short headers put the version in FRONT of it — the hand-over to the exact reader
  large        one certificate of 70 000 octets (30 83) in lane 0, 17 and 63 of a wave of small ones; its basicConstraints
               lies behind 69 kB of an unknown extension (a window the lane fetches for itself)
  waves        small payloads of n = 1, 3, 4, 5, 15, 16, 17, 61, 64, 65 from front and subject; one long subject among 63
               short ones and the reverse
Families with `cuts` are SEQUENCES of small payloads (tail_last, waves): each slice is mapped as a batch of its own.
"""
import datetime
import functools
from dataclasses import dataclass, field

import numpy as np

from ct_mapreduce_amd import synth, _native as N
from ct_mapreduce_amd.engine import Batch
from tests import der as D
from tests.meta_corpus import ECDSA_SIGALG, dp, dp_ext, issuers, uri

FILT = b"Geo"                       # the CN filter: "Geo CA …" passes, "Xeo CA …" does not
NOW = synth.BASE_TIME
N_ISSUERS = 3
IDS = dict(front=1, front_rdn=2, subject=3, tail=4, tail_last=5, ext=6, ext_unknown=7, ext_crl=8, san=9, san_long=10,
           small=11, large=12, waves=13)
PSS_SIGALG = D.seq(D.tlv(0x06, bytes.fromhex("2a864886f70d01010a")), D.seq(
    D.tlv(0xa0, D.seq(D.tlv(0x06, bytes.fromhex("608648016503040201")), D.NULL)),
    D.tlv(0xa1, D.seq(D.tlv(0x06, bytes.fromhex("2a864886f70d010108")),
                      D.seq(D.tlv(0x06, bytes.fromhex("608648016503040201")), D.NULL))),
    D.tlv(0xa2, D.tlv(0x02, b"\x20"))))
_OID11 = bytes.fromhex("2a864886f70d010163050711")


def algid_of_len(t):
    """An AlgorithmIdentifier of exactly t octets (10..): an unknown OID, from 16 octets on with an OCTET STRING parameter."""
    a = D.seq(D.tlv(0x06, _OID11[:t - 4])) if t <= 15 else D.seq(D.tlv(0x06, _OID11[:10]), D.tlv(0x04, bytes(range(1, t - 15))))
    assert len(a) == t
    return a


TAIL_ALGS = (ECDSA_SIGALG, D.SIGALG, PSS_SIGALG, algid_of_len(30))
UNKNOWN_KEY_OID = bytes.fromhex("2b0663")
SHORT_ALG = D.seq(D.oid(0x2b, 0x06, 0x63))      # 7 octets, an OID nobody knows: parsing does not look it up


@dataclass
class Family:
    name: str
    certs: list = field(default_factory=list)      # (der, issuer_idx, entry_type)
    pairs: list = field(default_factory=list)      # (i, j, kind): twins
    singles: list = field(default_factory=list)    # (i, kind): refused whatever else they hold
    marks: list = field(default_factory=list)      # per certificate: the builder's own bookkeeping (dict)
    cuts: list = None                              # sequence families: slice k is certs[cuts[k]:cuts[k + 1]]
    _count: int = 0

    def serial(self, ln=None):
        """A serial of this family's next step: 1, 2, then 3..20 octets (ln: that many — a sweep that moves a field octet by
        octet keeps the serial's length); the first octet is the family's number, the next two count the steps."""
        k, fam = self._count, IDS[self.name]
        self._count += 1
        if k == 0:
            return bytes([fam])
        if k == 1:
            return bytes([fam, 0x5a])
        ln = ln or 3 + k % 18
        return (bytes([fam]) + k.to_bytes(2, "big") + bytes(((k * 7 + i) & 0x7f) | 1 for i in range(17)))[:ln]

    def add(self, der, et=0, **mark):
        i = len(self.certs)
        self.certs.append((der, i % N_ISSUERS, et))
        self.marks.append(mark)
        return i

    def twins(self, kind, a, b, et=0, **mark):
        i = self.add(a, et, kind=kind, **mark)
        j = self.add(b, et, kind=kind, **mark)
        self.certs[j] = (b, self.certs[i][1], et)              # the twins share their issuer
        self.pairs.append((i, j, kind))

    def single(self, kind, der, et=0, **mark):
        self.singles.append((self.add(der, et, kind=kind, **mark), kind))

    def batch(self, order=None):
        idx = range(len(self.certs)) if order is None else order
        return Batch.from_certs([self.certs[i][0] for i in idx], [self.certs[i][1] for i in idx], [self.certs[i][2] for i in idx])


def when(step, odd=0):
    """notAfter of a step: a day and an EVEN hour of its own (+ odd: the twin's hour differs in one digit), never expired."""
    t = datetime.datetime(2027, 1, 1) + datetime.timedelta(days=step % 331, hours=2 * (step % 12) + odd)
    return t.strftime("%y%m%d%H0000Z")


def key_of(step):
    """Two thirds RSA (the default 2048-bit shape), one third points on P-256."""
    return D.rsa_spki() if step % 3 != 2 else (D.EC_SPKI, D.EC_SPKI_2)[step // 3 % 2]


def make(serial, issuer, not_after, subject, spki, exts=None, tbs_sigalg=D.SIGALG, outer_sigalg=None, sig_tag=0x03,
         sig=b"\x00" + b"\x5a" * 64, version=True, tbs_over=0):
    """D.cert with the pieces behind the TBSCertificate open: the signatureValue's tag, a TBSCertificate header whose length
    reaches tbs_over octets past the Certificate's end (the Certificate keeps its own)."""
    tbs = (D.tlv(0xa0, D.tlv(0x02, b"\x02")) if version else b"") + D.tlv(0x02, serial) + tbs_sigalg + issuer + \
        D.seq(D.utctime("250101000000Z"), not_after) + subject + spki
    if exts is not None:
        tbs += D.tlv(0xa3, D.seq(*exts))
    t = D.tlv(0x30, tbs)
    rest = (tbs_sigalg if outer_sigalg is None else outer_sigalg) + D.tlv(sig_tag, sig)
    if tbs_over:                                    # the TBSCertificate claims to end tbs_over octets behind the certificate
        claimed = len(tbs) + len(rest) + tbs_over
        t = D.tlv(0x30, bytes(claimed))[:-claimed] + tbs
    return D.seq(t + rest)


def cn(step, first=b"G"):
    return first + b"eo CA %d" % (step % 7)


def subj(filler=None, letter=b"s"):
    return D.name(*([D.rdn(10, letter * filler)] if filler is not None else []), D.rdn(3, b"leaf"))


ISS = D.name(D.rdn(3, cn(0)))


def bc(ca, critical=True, crit_octet=0xff):
    e = D.ext(0x13, D.seq(D.tlv(0x01, b"\xff" if ca else b"\x00")), critical=critical if critical else None)
    if critical and crit_octet != 0xff:
        at = e.index(b"\x01\x01\xff") + 2
        e = e[:at] + bytes([crit_octet]) + e[at + 1:]
    return e


def ski(n):
    return D.ext(0x0e, D.tlv(0x04, bytes((7 * k + n) & 0xff for k in range(n))))


def three_front_twins(fam, step, issuer_of, subject, spki, ln=None, **mark):
    """The front family's three pairs for one geometry: CN first letter, notAfter hour, notAfter tag."""
    s = fam.serial(ln)
    fam.twins("cn", make(s, issuer_of(b"G"), D.utctime(when(step)), subject, spki),
              make(s, issuer_of(b"X"), D.utctime(when(step)), subject, spki), **mark)
    s = fam.serial(ln)
    fam.twins("hour", make(s, issuer_of(b"G"), D.utctime(when(step)), subject, spki),
              make(s, issuer_of(b"G"), D.utctime(when(step, 1)), subject, spki), **mark)
    s = fam.serial(ln)
    fam.twins("tag", make(s, issuer_of(b"G"), D.utctime(when(step)), subject, spki),
              make(s, issuer_of(b"G"), D.tlv(0x18, when(step).encode()), subject, spki), **mark)


@functools.lru_cache(maxsize=None)
def front():
    fam = Family("front")
    for f in range(261):
        three_front_twins(fam, f, lambda g, f=f: D.name(D.rdn(10, b"o" * f), D.rdn(3, cn(f, g))), subj(), key_of(f), ln=4, filler=f)
    return fam


@functools.lru_cache(maxsize=None)
def front_rdn():
    fam = Family("front_rdn")
    for k in range(1, 6):
        for j in range(12):
            # an RDN with an O= of 53 octets is 64 octets long: every one of them begins on a multiple of 64 of the Name
            rdns = [D.rdn(10, bytes([0x61 + (j + r) % 26]) * 53) for r in range(k)]
            assert all(len(r) == 64 for r in rdns)
            step = 12 * k + j
            three_front_twins(fam, step, lambda g, rdns=rdns, step=step: D.name(*rdns, D.rdn(3, cn(step, g))), subj(),
                              key_of(step), ln=3 + step % 18, hints=k)
    return fam


EXPONENTS = (b"\x03", b"\x01\x00\x01", b"\x01\x00\x00\x01", b"\x01" + bytes(6) + b"\x01")
MODULI = (128, 384, 512, 250, 256)
RSA_TWINS = ("exp0", "neg", "shape")


def modulus(m, b0=0x00, b1=0xc3):
    return bytes([b0, b1]) + b"\xc3" * (m - 1)


@functools.lru_cache(maxsize=None)
def subject():
    """Step f = 3t + r.  r = 2: a P-256 point (the key's position, k_ec_resolve's keypos, is swept too).  r = 1: a modulus of
    256 octets, the exponent form changing every 16 steps.  r = 0: the five moduli in turn, each with one exponent form —
    so that for every modulus the key's END moves octet by octet (15 is odd) over all 16 residues."""
    fam = Family("subject")
    for f in range(301):
        s, su, na, t = fam.serial(9), subj(f), D.utctime(when(f)), f // 3
        if f % 3 == 2:
            key = (D.EC_SPKI, D.EC_SPKI_2)[t % 2]
            fam.twins("hour", make(s, ISS, na, su, key), make(s, ISS, D.utctime(when(f, 1)), su, key), filler=f, m=0)
            continue
        m, e = (256, EXPONENTS[t // 16 % 4]) if f % 3 == 1 else (MODULI[t % 5], EXPONENTS[t % 5 % 4])
        kind = RSA_TWINS[t % 3]
        if kind == "exp0":
            a, b, et = D.rsa_spki(modulus(m), b"\x01"), D.rsa_spki(modulus(m), b"\x00"), 0
        elif kind == "neg":                         # findings: what a precertificate entry loses its place over
            a, b, et = D.rsa_spki(modulus(m), e), D.rsa_spki(modulus(m, 0x80), e), 1
        else:
            a, b, et = D.rsa_spki(modulus(m), e), D.rsa_spki(modulus(m, 0x00, 0x43), e), 1
        fam.twins(kind, make(s, ISS, na, su, a), make(s, ISS, na, su, b), et, filler=f, m=m)
        if f % 30 == 1:                             # 9 octets do not fit an int: refused
            fam.single("exp9", make(fam.serial(9), ISS, na, su, D.rsa_spki(modulus(m), b"\x01" + bytes(7) + b"\x01")), filler=f, m=m)
    # … and each modulus once more at sixteen CONSECUTIVE fillers (no length header changes form on the way: every residue
    # of the key's end for certain), with the P-256 points that keep the family's one third
    for mi, m in enumerate(MODULI):
        for f in range(16, 32):
            s, su, na, e = fam.serial(9), subj(f), D.utctime(when(400 + 16 * mi + f)), EXPONENTS[(mi + 1) % 4]
            kind = RSA_TWINS[mi % 3]                 # (one kind, one exponent length per modulus: the end moves by the filler alone)
            b = dict(exp0=D.rsa_spki(modulus(m), b"\x00"), neg=D.rsa_spki(modulus(m, 0x80), e), shape=D.rsa_spki(modulus(m, 0x00, 0x43), e))[kind]
            a = D.rsa_spki(modulus(m), b"\x01" if kind == "exp0" else e)
            fam.twins(kind, make(s, ISS, na, su, a), make(s, ISS, na, su, b), int(kind != "exp0"), filler=f, m=m)
    for f in range(16, 56):
        s, su, key = fam.serial(9), subj(f), (D.EC_SPKI, D.EC_SPKI_2)[f % 2]
        fam.twins("hour", make(s, ISS, D.utctime(when(500 + f)), su, key), make(s, ISS, D.utctime(when(500 + f, 1)), su, key), filler=f, m=0)
    return fam


def tail_twins(fam, step, alg, su, key, **mark):
    over = alg[:1] + bytes([alg[1] + 1]) + alg[2:]
    s, na = fam.serial(16), D.utctime(when(step))
    fam.twins("pad", make(s, ISS, na, su, key, tbs_sigalg=alg), make(s, ISS, na, su, key, tbs_sigalg=alg, sig=b"\x08" + b"\x5a" * 64), **mark)
    s = fam.serial(16)
    fam.twins("sigtag", make(s, ISS, na, su, key, tbs_sigalg=alg), make(s, ISS, na, su, key, tbs_sigalg=alg, sig_tag=0x04), **mark)
    s = fam.serial(16)
    fam.twins("algover", make(s, ISS, na, su, key, tbs_sigalg=alg), make(s, ISS, na, su, key, tbs_sigalg=alg, outer_sigalg=over), **mark)


@functools.lru_cache(maxsize=None)
def tail():
    fam = Family("tail")
    for v, alg in enumerate(TAIL_ALGS):
        for g in range(64):
            tail_twins(fam, 64 * v + g, alg, subj(g, b"t"), key_of(g), variant=v, alg_len=len(alg))
    for t in range(10, 41):
        tail_twins(fam, 300 + t, algid_of_len(t), subj((5 * t) % 64, b"t"), key_of(t), variant=4, alg_len=t)
    return fam


def plain(fam, step, filler=3):
    """An ordinary certificate with a serial of its own (fills the small payloads of the sequence families)."""
    return make(fam.serial(), ISS, D.utctime(when(step)), subj(filler, b"p"), key_of(step), exts=[bc(False)])


@functools.lru_cache(maxsize=None)
def tail_last():
    fam = Family("tail_last", cuts=[0])
    step = 0
    for v, alg in enumerate(TAIL_ALGS):
        over = alg[:1] + bytes([alg[1] + 1]) + alg[2:]
        for kind, kw in (("pad", dict(sig=b"\x08" + b"\x5a" * 64)), ("sigtag", dict(sig_tag=0x04)), ("algover", dict(outer_sigalg=over))):
            s, na, su, key = fam.serial(), D.utctime(when(step)), subj(step % 17, b"t"), key_of(step)
            ab = [make(s, ISS, na, su, key, tbs_sigalg=alg), make(s, ISS, na, su, key, tbs_sigalg=alg, **kw)]
            at = []
            for der in ab:                          # the certificate under test ends the payload
                for k in range(3):
                    fam.add(plain(fam, step + k, k), kind="plain")
                at.append(fam.add(der, kind=kind, variant=v, last=True))
                fam.cuts.append(len(fam.certs))
            fam.certs[at[1]] = (ab[1], fam.certs[at[0]][1], 0)
            fam.pairs.append((at[0], at[1], kind))
            step += 1
    for over in range(1, 41):                       # a TBSCertificate that overruns the certificate (and the payload's pad)
        alg = TAIL_ALGS[over % 4]
        for k in range(over % 4):
            fam.add(plain(fam, step + k, k), kind="plain")
        fam.single("tbs_over", make(fam.serial(), ISS, D.utctime(when(step)), subj(over % 9, b"t"), key_of(over), tbs_sigalg=alg,
                                    tbs_over=over), variant=over % 4, last=True, over=over)
        fam.cuts.append(len(fam.certs))
        step += 1
    return fam


@functools.lru_cache(maxsize=None)
def ext():
    fam = Family("ext")
    for n in range(251):
        na, key = D.utctime(when(n)), key_of(n)
        for critical in (True, False):              # the 12-octet and the 9-octet fast form of the header
            s = fam.serial(20)
            fam.twins("ca", make(s, ISS, na, subj(), key, exts=[ski(n), bc(True, critical)]),
                      make(s, ISS, na, subj(), key, exts=[ski(n), bc(False, critical)]), ski=n, critical=critical, first=False)
        if n % 4 == 0:                              # basicConstraints first: the filler lies behind it
            s = fam.serial()
            fam.twins("ca", make(s, ISS, na, subj(n % 50), key, exts=[bc(True), ski(n)]),
                      make(s, ISS, na, subj(n % 50), key, exts=[bc(False), ski(n)]), ski=n, critical=True, first=True)
        if n % 4 == 2:
            s = fam.serial()
            fam.twins("critical", make(s, ISS, na, subj(), key, exts=[ski(n), bc(False)]),
                      make(s, ISS, na, subj(), key, exts=[ski(n), bc(False, True, 0x01)]), ski=n, critical=True, first=False)
    return fam


def unknown_ext(k, size):
    return D.seq(D.oid(0x55, 0x1d, 0x63), D.tlv(0x04, bytes((k + i) & 0xff for i in range(size))))


@functools.lru_cache(maxsize=None)
def ext_unknown():
    fam = Family("ext_unknown")
    for count in range(1, 25):
        for k, size in enumerate((0, 3, 9)):
            step = 3 * count + k
            s, na, key = fam.serial(), D.utctime(when(step)), key_of(step)
            front_exts = [unknown_ext(k, size + k % 2) for k in range(count)]
            fam.twins("ca", make(s, ISS, na, subj(), key, exts=front_exts + [bc(True)]),
                      make(s, ISS, na, subj(), key, exts=front_exts + [bc(False)]), count=count)
    return fam


@functools.lru_cache(maxsize=None)
def ext_crl():
    fam = Family("ext_crl")
    for n in range(251):
        s, na, key = fam.serial(12), D.utctime(when(n % 47)), key_of(n)
        crl = dp_ext(dp(uri(b"http://crl.example/geo/%02d.crl" % (n % 13))))
        issuer = D.name(D.rdn(10, b"Geometry %d" % (n % 5)), D.rdn(3, cn(n)))
        fam.twins("ca", make(s, issuer, na, subj(), key, exts=[ski(n), bc(True), crl]),
                  make(s, issuer, na, subj(), key, exts=[ski(n), bc(False), crl]), ski=n)
    return fam


def dns_names(total, salt=0):
    """dNSName elements of exactly `total` octets, headers included (2: one empty name)."""
    out, rem = [], total
    while rem:
        take = min(rem, 35)
        if rem - take in (1, 2):
            take -= 3
        assert take >= 2
        out.append(D.tlv(0x82, bytes(0x61 + (salt + len(out) + i) % 26 for i in range(take - 2))))
        rem -= take
    return out


def san_ext(elements):
    return D.ext(0x11, D.seq(*elements))


@functools.lru_cache(maxsize=None)
def san():
    fam = Family("san")
    for s_len in range(2, 701):
        s, na, key = fam.serial(7), D.utctime(when(s_len)), key_of(s_len)
        if s_len % 2 == 0 or s_len < 14:
            names = dns_names(s_len, s_len)
            fam.twins("ca", make(s, ISS, na, subj(), key, exts=[san_ext(names), bc(True)]),
                      make(s, ISS, na, subj(), key, exts=[san_ext(names), bc(False)]), 0, san=s_len)
        else:                                       # … 82 03 abc 87 04 ….  |  … 82 02 ab 87 05 …..: the same length
            names = dns_names(s_len - 11, s_len)
            good = names + [D.tlv(0x82, b"abc"), D.tlv(0x87, bytes([10, 1, 2, 3]))]
            bad = names + [D.tlv(0x82, b"ab"), D.tlv(0x87, bytes([10, 1, 2, 3, 4]))]
            fam.twins("ip", make(s, ISS, na, subj(), key, exts=[san_ext(good), bc(False)]),
                      make(s, ISS, na, subj(), key, exts=[san_ext(bad), bc(False)]), 1, san=s_len)
    return fam


@functools.lru_cache(maxsize=None)
def san_long():
    fam = Family("san_long")
    long_el = D.tlv(0x82, b"l" * 128)
    assert long_el[:3] == b"\x82\x81\x80"
    for k in range(40):
        s, na, key = fam.serial(), D.utctime(when(k)), key_of(k)
        names = [D.tlv(0x82, bytes([0x61 + i % 26])) for i in range(k)] + [long_el] + dns_names(90 + k % 7, k)
        fam.twins("ca", make(s, ISS, na, subj(), key, exts=[san_ext(names), bc(True)]),
                  make(s, ISS, na, subj(), key, exts=[san_ext(names), bc(False)]), k % 2, at=k)
    return fam


def sized(total, serial, first, na, key_len):
    """A certificate of exactly `total` octets with an unknown key algorithm and a key of key_len octets (one to three more,
    or fewer, where the header forms or the serial leave no such length), an empty subject, no version, no extensions:
    the shortest is 88 octets.  None: no DER element has that length."""
    for kl in list(range(key_len, key_len + 4)) + list(range(key_len - 1, 0, -1)):
        key = D.spki(UNKNOWN_KEY_OID, b"", bytes(0x30 + i % 10 for i in range(kl)))
        for sig_len in range(1, total):
            der = make(serial, D.name(D.rdn(3, first + b"eo")), na, D.name(), key, tbs_sigalg=SHORT_ALG,
                       sig=b"\x00" + b"\x5a" * sig_len, version=False)
            if len(der) >= total:
                break
        if len(der) == total:
            return der
    return None


SMALL_LENGTHS = tuple(range(90, 216)) + tuple(range(250, 263))
UNREACHABLE = (130, 259)


@functools.lru_cache(maxsize=None)
def small():
    fam = Family("small")
    for total in SMALL_LENGTHS:
        s, key_len = fam.serial()[:6], 1 + (total - 90) % 40 if total >= 130 else 1 + (total - 90)
        na = D.utctime(when(total))
        kind = "cn" if total % 2 == 0 else "hour"
        a = sized(total, s, b"G", na, key_len)
        b = sized(total, s, b"X", na, key_len) if kind == "cn" else sized(total, s, b"G", D.utctime(when(total, 1)), key_len)
        if total in UNREACHABLE:                    # no DER element has these lengths: 2 + 127 = 129, 3 + 128 = 131, …
            assert a is None and b is None
            continue
        fam.twins(kind, a, b, total=total)
    return fam


BIG = 70000


def big_cert(serial, na, ca):
    lo = make(serial, ISS, na, subj(), D.rsa_spki(), exts=[unknown_ext(0, 0), bc(ca)])
    der = make(serial, ISS, na, subj(), D.rsa_spki(), exts=[unknown_ext(0, BIG - len(lo) - 12), bc(ca)])
    der = make(serial, ISS, na, subj(), D.rsa_spki(), exts=[unknown_ext(0, BIG - len(lo) - 12 + BIG - len(der)), bc(ca)])
    assert len(der) == BIG and der[:2] == b"\x30\x83"
    return der


@functools.lru_cache(maxsize=None)
def large():
    fam = Family("large")
    s, na = fam.serial(), D.utctime(when(5))
    at = {}
    for ca in (True, False):                        # three waves per twin: the big one in lane 0, 17, 63
        for w, lane in enumerate((0, 17, 63)):
            for k in range(64):
                if k == lane:
                    at[ca, lane] = fam.add(big_cert(s + bytes([lane + 1]), na, ca), kind="ca", lane=lane, big=True)
                else:
                    fam.add(sized(150 + k, fam.serial()[:6], b"G", D.utctime(when(k)), 1 + k % 40), kind="plain", big=False)
    for lane in (0, 17, 63):
        i, j = at[True, lane], at[False, lane]
        fam.certs[j] = (fam.certs[j][0], fam.certs[i][1], 0)
        fam.pairs.append((i, j, "ca"))
    return fam


WAVE_SIZES = (1, 3, 4, 5, 15, 16, 17, 61, 64, 65)


@functools.lru_cache(maxsize=None)
def waves():
    """Small payloads: twins of the front and subject families, A's payload then B's (the two payloads are byte-identical
    except in ONE certificate), and the long subject among short ones."""
    fam = Family("waves", cuts=[0])
    fr, sb = front(), subject()
    rng = np.random.default_rng(20261018)

    def payload(members, target, where):
        for twin in (0, 1):
            here = []
            for k, m in enumerate(members):
                if k == where:
                    here.append(fam.add(target[twin][0], target[twin][2], kind=target[2], n=len(members)))
                else:
                    fam.add(m[0], m[2], kind="plain", n=len(members))
            at.append(here[0])
            fam.cuts.append(len(fam.certs))

    for n in WAVE_SIZES:
        for src in (fr, sb):
            at = []
            i, j, kind = src.pairs[int(rng.integers(0, len(src.pairs)))]
            others = [src.certs[src.pairs[int(p)][0]] for p in rng.integers(0, len(src.pairs), size=n)]
            payload(others, (src.certs[i], src.certs[j], kind), int(rng.integers(0, n)))
            fam.certs[at[1]] = (fam.certs[at[1]][0], fam.certs[at[0]][1], fam.certs[at[1]][2])
            fam.pairs.append((at[0], at[1], kind))
    short = [fr.certs[fr.pairs[3 * f][0]] for f in range(64)]                       # issuer fillers 0..63
    long_ = [sb.certs[sb.pairs[f][0]] for f in range(237, 301)]                     # subject fillers 237..300
    for others, src, lane in ((short, sb, 40), (long_, fr, 23)):
        at = []
        i, j, kind = src.pairs[-2] if src is sb else src.pairs[0]
        payload(others, (src.certs[i], src.certs[j], kind), lane)
        fam.certs[at[1]] = (fam.certs[at[1]][0], fam.certs[at[0]][1], fam.certs[at[1]][2])
        fam.pairs.append((at[0], at[1], kind))
    return fam


FAMILIES = dict(front=front, front_rdn=front_rdn, subject=subject, tail=tail, tail_last=tail_last, ext=ext,
                ext_unknown=ext_unknown, ext_crl=ext_crl, san=san, san_long=san_long, small=small, large=large, waves=waves)


def registered_issuers():
    return issuers(N_ISSUERS)


def shuffled(fam, seed=20261018):
    """A seeded permutation of a family's certificates (sequence families: within each payload)."""
    rng = np.random.default_rng([seed, IDS[fam.name]])
    if fam.cuts is None:
        return [int(i) for i in rng.permutation(len(fam.certs))]
    out = []
    for lo, hi in zip(fam.cuts, fam.cuts[1:]):
        out += [lo + int(i) for i in rng.permutation(hi - lo)]
    return out


def line_view(batch, fill=1):
    """(blob, cert_start, cert_end): an ASCENDING entry view in which certificate k starts at residue 37·k mod 128 of a
    128-octet line (37 is odd: 128 consecutive certificates take every residue); non-zero noise between the certificates
    and in the CTMR_PAYLOAD_PAD octets behind the last one, as tests/view_corpus.py lays its views out."""
    rng = np.random.default_rng([int(fill), 37])
    n = batch.n
    start, end = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    at = 0
    for k in range(n):
        at += (37 * k - at) % 128
        ln = int(batch.offsets[k + 1] - batch.offsets[k])
        start[k], end[k] = at, at + ln
        at += ln
    blob = rng.integers(1, 256, size=at + N.PAYLOAD_PAD, dtype=np.uint8)
    for k in range(n):
        blob[int(start[k]):int(end[k])] = batch.payload[int(batch.offsets[k]):int(batch.offsets[k + 1])]
    return blob, start, end
