"""Corpora for the IssuerMetadata memo at every item length, address and path (test helper, no test): hand-built
certificates over tests/der.py for the directed tests of k_meta_new, the map kernel's memo pre-check and ctmr_meta_new
(tests/test_gpu_meta_lengths.py).  The synthetic corpus shows one Name and one URI length per issuer; here the length, the
address and what lies BEHIND an item are the parameters.  tests/test_meta_corpus_cpu.py holds every claim a builder makes
against the oracle, without a GPU.

A corpus is a list of (der, issuer_idx) plus one row of claims per certificate.  Items come in triples:
  A       the item (an issuer Name, a CRL distribution point URI);
  again   the same item in another certificate whose bytes behind the item differ within the first 15 — what an unaligned
          16-byte read of the item's last chunk also sees;
  prime   the item with its last byte changed: another item.
`part("first")` is every certificate but the `again` ones, `part("second")` the `again` ones: a memo that saw the first
part holds everything the second brings.

  name_lengths()  issuer Names of every DER length from the shortest through 160 and of 4090..4100 (beyond 4096: host);
  uri_lengths()   URIs of 0..160 and 4090..4100 octets, each alone in its DistributionPoint, followed by a second URI,
                  behind a first URI, and as the last bytes of the extension block; certificates of exactly 4 and 5 URIs; a
                  sweep that moves a distribution point across the end of the map kernel's extension window;
  addresses()     Names and first URIs of 15..129 octets at all 16 residues mod 16 of their payload address;
  crowd(n)        n distinct URIs for one memo, two per certificate;
  overflow()      a batch that brings more first sightings than ctmr_meta_new's first item buffer holds, and a small one
                  before it that shares items with it.

expected_first_sightings / got_first_sightings state the reference's memo semantics (storage/issuermetadata.go:92-138) over
the oracle's field extraction; every expectation of the memo's tests is made by them.
"""
import functools
import os
import re
from dataclasses import dataclass, field

import numpy as np

from ct_mapreduce_amd import _native as N
from oracle import oracle as orc
from tests import der as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
ECDSA_SIGALG = bytes.fromhex("300a06082a8648ce3d040302")       # ecdsa-with-SHA256: 12 octets, sha256WithRSA has 15
META_LDS_DN, META_LDS_CRL, META_MAX_BYTES, META_MAX_URIS = 128, 64, 4096, 4   # kernels/meta_core.h
NAME_TOP, NAME_BIG = 160, tuple(range(4090, 4101))
URI_SMALL, URI_BIG = tuple(range(0, 161)), tuple(range(4090, 4101))
ADDRESS_LENGTHS = (15, 16, 17, 63, 64, 65, 127, 128, 129)
URI_FORMS = ("alone", "pair", "second", "last")


def dp_ext(*points, critical=None):
    return D.ext(0x1f, D.seq(*points), critical)


def dp(*general_names, reasons=None, crl_issuer=None):
    parts = []
    if general_names:
        parts.append(D.tlv(0xa0, D.tlv(0xa0, b"".join(general_names))))
    if reasons:
        parts.append(D.tlv(0x81, reasons))
    if crl_issuer:
        parts.append(D.tlv(0xa2, crl_issuer))
    return D.seq(*parts)


def uri(s):
    return D.tlv(0x86, s)


def expected_first_sightings(certs, issuer_canon, new_idx, exp_hours):
    """The reference's memo semantics over the new certificates, in log order."""
    seen, out = set(), set()
    for i in new_idx:
        meta = orc.cert_meta(certs[i])
        assert meta is not None
        name, uris, m = meta
        c = issuer_canon[i]
        host = (m.n_crl_ext > 1 or len(name) > 4096 or any(len(u) > 4096 for u in uris) or m.n_crl > 4
                or len(certs[i]) > 0xfffe)
        items = [(N.MK_EXPDATE, c, int(exp_hours[i]), b"")]
        if host:
            out.add((N.MK_HOST, i))
        else:
            items += [(N.MK_DN, c, 0, name)] + [(N.MK_CRL, c, 0, u) for u in uris]
        for it in items:
            if it not in seen:
                seen.add(it)
                out.add(it)
    return out


def got_first_sightings(eng, items):
    out = set()
    for kind, entry, idx, exp_hour, b in items:
        c = eng.issuer_info(idx).canonical_idx
        if kind == N.MK_HOST:
            out.add((kind, entry))
        elif kind == N.MK_EXPDATE:
            out.add((kind, c, exp_hour, b""))
        else:
            out.add((kind, c, 0, b))
    return out


def window_bytes():
    """{profile: bytes of the map kernel's per-lane window}, from kernels/readers.h (WinGeo::WBYTES)."""
    text = open(os.path.join(ROOT, "ct_mapreduce_amd", "csrc", "kernels", "readers.h"), encoding="utf-8").read()
    ch = {k: int(re.search(r"#define CTMR_WIN_CH_%s (\d+)" % k, text).group(1)) for k in ("FAST", "STRICT")}
    xdw14 = int(re.search(r"#define CTMR_WIN_XDW14 (\d+)u", text).group(1))
    assert "XDW = WCH == 13 ? 2u : WCH == 14 ? CTMR_WIN_XDW14 : 0u" in text and "WBYTES = (uint32_t)WCH * 16u + XDW * 4u" in text
    return {p: 16 * c + 4 * (2 if c == 13 else xdw14 if c == 14 else 0)
            for p, c in (("fast", ch["FAST"]), ("reference", ch["STRICT"]))}


@dataclass
class Corpus:
    issuers: list                                  # issuer certificates (DER), registered in this order
    certs: list = field(default_factory=list)      # (der, issuer_idx)
    rows: list = field(default_factory=list)       # per certificate: what the builder claims about it
    unreachable: list = field(default_factory=list)
    _serial: int = 0

    def add(self, issuer_idx, role, **kw):
        """One certificate with a serial of its own (four octets unless the caller brings one)."""
        claims = {k: kw.pop(k) for k in list(kw) if k in ("kind", "length", "form", "group", "uris", "name", "sweep")}
        if "serial" not in kw:
            self._serial += 1
            kw["serial"] = b"\x01" + self._serial.to_bytes(3, "big")
        der = D.cert(**kw)
        self.certs.append((der, issuer_idx))
        self.rows.append(dict(claims, role=role))
        return der

    def part(self, which=None):
        """→ (ders, issuer indices, rows) of the whole corpus, of its "first" part or of its "second" one."""
        keep = [i for i, r in enumerate(self.rows)
                if which is None or (r["role"] == "again") == (which == "second")]
        return [self.certs[i][0] for i in keep], [self.certs[i][1] for i in keep], [self.rows[i] for i in keep]

    def offsets(self, which=None):
        """Payload offset of every certificate of a part in its packed batch."""
        ders = self.part(which)[0]
        return np.concatenate([[0], np.cumsum([len(d) for d in ders])]).astype(np.int64)


def issuers(n):
    """n issuer certificates with keys of their own: two points on P-256, then RSA moduli."""
    out = []
    for k in range(n):
        key = D.EC_SPKI if k == 0 else D.EC_SPKI_2 if k == 1 else D.rsa_spki(n=b"\x00" + b"\xc3" * 254 + bytes([0xc1 + 2 * k, 0xc3]))
        out.append(D.cert(serial=bytes([0x20 + k]), exts=[D.BC_CA], subject=D.name(D.rdn(3, b"Memo CA %d" % k)), spki=key))
    return out


def letters(n, salt):
    """n ASCII letters that differ from salt to salt."""
    reps = n // len(LETTERS) + 2
    return (LETTERS * reps)[salt % len(LETTERS):][:n]


def other_last(b):
    """b with its last byte replaced by another letter."""
    return b[:-1] + (b"q" if b[-1:] != b"q" else b"r")


# ------------------------------------------------------------------ Names
def _name(cn, org=None):
    return D.name(*([D.rdn(10, org)] if org is not None else []), D.rdn(3, cn))


@functools.lru_cache(maxsize=None)
def name_shapes():
    """DER length → (organization octets or None, commonName octets).  One RDN where it reaches the length; two where a
    length header's step from one octet to two (at 128) makes the one-RDN Name skip it."""
    table = {}
    for c in list(range(1, 200)) + list(range(4040, 4100)):
        table.setdefault(len(_name(b"x" * c)), (None, c))
    for o in range(1, 24):
        for c in range(1, 160):
            table.setdefault(len(_name(b"x" * c, b"o" * o)), (o, c))
    return table


def name_of(length, salt=0):
    o, c = name_shapes()[length]
    nm = _name(letters(c, salt + length), None if o is None else letters(o, salt + 7))
    assert len(nm) == length
    return nm


def name_lengths():
    c = Corpus(issuers(2))
    shapes = name_shapes()
    lo = min(shapes)
    c.unreachable = [n for n in list(range(lo, NAME_TOP + 1)) + list(NAME_BIG) if n not in shapes]
    shared = [b"http://crl.example/names-%d.crl" % k for k in range(2)]
    for n in [n for n in range(lo, NAME_TOP + 1) if n in shapes] + [n for n in NAME_BIG if n in shapes]:
        iss = n & 1
        a = name_of(n)
        exts = [D.BC_NOT_CA, dp_ext(dp(uri(shared[iss])))]
        claims = dict(kind="name", length=n, group=("name", n))
        c.add(iss, "A", issuer=a, exts=exts, **claims)
        c.add(iss, "again", issuer=a, exts=exts, not_before=D.utctime("240202030405Z"), **claims)
        c.add(iss, "prime", issuer=other_last(a), exts=exts, **claims)
    return c


# ------------------------------------------------------------------ URIs
def uri_of(length, form, salt=0):
    head = b"http://" + form.encode() + b"."
    return (head + letters(length, salt + length))[:length]


def _san(dns):
    return D.ext(0x11, D.seq(D.tlv(0x82, dns)))


def _uri_cert(c, iss, role, u, form, group, behind, name, **kw):
    """`behind` picks what follows the URI: 0 for A and prime, 1 for again."""
    first = b"http://crl.example/first-of-issuer-%d.crl" % iss
    seconds = (b"ldap://second.example/one", b"http://second.example/number/two")
    tails = (_san(b"tail.example"), _san(b"another-tail.example.org"))
    if form == "alone":
        exts, us = [D.BC_NOT_CA, dp_ext(dp(uri(u))), tails[behind]], [u]
    elif form == "pair":       # the second URI of `again` is the one `prime` brought: the first part holds both
        s = seconds[1 if role != "A" else 0]
        exts, us = [D.BC_NOT_CA, dp_ext(dp(uri(u), uri(s)))], [u, s]
    elif form == "second":
        exts, us = [D.BC_NOT_CA, dp_ext(dp(uri(first), uri(u))), tails[behind]], [first, u]
    else:                      # "last": the URI ends the extension block; the signature algorithm follows
        exts, us = [D.BC_NOT_CA, dp_ext(dp(uri(u)))], [u]
        if behind:
            kw.update(tbs_sigalg=ECDSA_SIGALG, outer_sigalg=ECDSA_SIGALG)
    c.add(iss, role, issuer=name, exts=exts, kind="uri", length=len(u), form=form, group=group, uris=us, **kw)


def uri_lengths():
    c = Corpus(issuers(2))
    names = [_name(b"URI lengths %d" % k) for k in range(2)]
    for fi, form in enumerate(URI_FORMS):
        for n in URI_SMALL + URI_BIG:
            iss = (n + fi) & 1
            a = uri_of(n, form)
            group = ("uri", form, n)
            _uri_cert(c, iss, "A", a, form, group, 0, names[iss])
            _uri_cert(c, iss, "again", a, form, group, 1, names[iss])
            if n:
                _uri_cert(c, iss, "prime", other_last(a), form, group, 0, names[iss])
    # exactly META_MAX_URIS URIs stay on the device, one more goes to the host; twice each: the second is a repeat
    for count in (META_MAX_URIS, META_MAX_URIS + 1):
        us = [b"http://many.example/%d-of-%d" % (k, count) for k in range(count)]
        for role in ("A", "again"):
            c.add(0, role, issuer=names[0], exts=[D.BC_NOT_CA, dp_ext(dp(*[uri(u) for u in us]))], kind="count",
                  length=count, group=("count", count), uris=us)
    # a distribution point behind a subjectAltName that grows octet by octet: the extension value moves across the end of
    # the window the map kernel's pre-check reads it from (sweep_margins)
    for s in range(60, 230):
        u = b"http://sweep.example/%03d.crl" % (s % 7)
        exts = [D.BC_NOT_CA, _san(letters(s, s)), dp_ext(dp(uri(u)))]
        claims = dict(kind="sweep", length=len(u), group=("sweep", s), uris=[u], sweep=s)
        for k in range(8):    # serials of 4..7 octets: every dword alignment of the window, in either part
            c._serial += 1
            c.add(1, "A" if k < 4 else "again", issuer=names[1], exts=exts,
                  serial=b"\x02" + c._serial.to_bytes(3, "big") + bytes(k & 3), **claims)
    return c


def crl_value_range(der):
    """(start, end) of the cRLDistributionPoints extension value of a hand-built certificate that has one distribution
    point whose last element is its last URI: the value ends where that URI ends."""
    m = orc.cert_meta(der)[2]
    k = m.n_crl - 1
    end = m.crl_off[k] + m.crl_len[k]
    at = der.rfind(bytes.fromhex("0603551d1f"), 0, end)
    hdr = at + 5                                    # OCTET STRING header
    assert der[hdr] == 0x04
    start = hdr + 2 + (der[hdr + 1] & 0x7f if der[hdr + 1] & 0x80 else 0)
    return start, end


def sweep_margins(c, which=None):
    """Per profile, for every sweep certificate of a part: octets between the end of its cRLDistributionPoints value and
    the end of the extension window — of the window the map kernel fills at the [3] Extensions element when the wave is
    whole (it begins there, give or take the 3 octets of dword alignment in the payload) and keeps as long as every
    extension header lies 16 octets inside it.  Negative: the value crosses the window's end."""
    ders, _, rows = c.part(which)
    offs = c.offsets(which)
    out = {p: {} for p in window_bytes()}
    for i, (der, row) in enumerate(zip(ders, rows)):
        if row.get("kind") != "sweep":
            continue
        q = orc.parse_cert(der).exts_off
        start, end = crl_value_range(der)
        begin = q - ((int(offs[i]) + q) & 3)
        for p, wb in window_bytes().items():
            out[p][i] = wb - (end - begin)
    return out


# ------------------------------------------------------------------ addresses
def _filler(c, pad, role):
    c.add(0, role, issuer=_name(b"filler"), subject=_name(letters(1 + pad, pad)), kind="filler")


def addresses():
    """Names and first URIs of ADDRESS_LENGTHS octets at every residue mod 16 of the payload address.  The serial's length
    (1..16 octets) moves both by one octet at a time; filler certificates in front move the certificate itself.  Two
    segments, the second a whole number of 16 octets behind the first one's start: the residues are those of the whole
    batch and of either part alone.  In each segment an item appears 16 times and its `prime` 16 times."""
    c = Corpus(issuers(2))
    for seg, role_of in ((0, lambda prime: "prime" if prime else "A"), (1, lambda prime: "again")):
        at0 = sum(len(d) for d, _ in c.certs)
        assert at0 % 16 == 0
        for li, n in enumerate(ADDRESS_LENGTHS):
            nm, u = name_of(n, salt=3), uri_of(n, "address")
            for r in range(16):
                for prime in (False, True):
                    if (r + li) % 5 == 0 and not prime:
                        _filler(c, (r * 7 + li) % 23, role_of(False))
                    total = sum(len(d) for d, _ in c.certs)
                    # Name offset in the certificate: outer and TBS headers (4 + 4), version (5), serial TLV, signature (15)
                    slen = (r - (total + 8 + 5 + 2 + 15)) % 16 or 16
                    c._serial += 1
                    serial = (b"\x01" + c._serial.to_bytes(3, "big") + bytes(12))[:max(slen, 4)] if slen >= 4 else None
                    if serial is None:      # 1..3 octets: the counter does not fit — the hour makes the certificate unique
                        serial = bytes([1 + seg * 2 + prime, r + 1, li + 1][:slen])
                    c.add(li & 1, role_of(prime), serial=serial, issuer=other_last(nm) if prime else nm,
                          exts=[D.BC_NOT_CA, dp_ext(dp(uri(other_last(u) if prime else u)))],
                          not_after=D.utctime("27%02d%02d000000Z" % (1 + li, 1 + r)),
                          kind="address", length=n, group=("address", n, prime))
        tail = -sum(len(d) for d, _ in c.certs) % 16      # close the segment on a multiple of 16
        base = len(D.cert(issuer=_name(b"filler"), subject=_name(b"x"), serial=b"\x7e\x01" + bytes([seg])))
        pad = (tail - base) % 16
        c.add(0, "A" if seg == 0 else "again", issuer=_name(b"filler"), subject=_name(b"x" * (1 + pad)),
              serial=b"\x7e\x01" + bytes([seg]), kind="filler")
        assert sum(len(d) for d, _ in c.certs) % 16 == 0
    return c


def item_residues(c, which=None):
    """{("name" | "uri", length): set of payload-address residues mod 16} of the address certificates of a part, from the
    oracle's offsets."""
    ders, _, rows = c.part(which)
    offs = c.offsets(which)
    out = {}
    for i, (der, row) in enumerate(zip(ders, rows)):
        if row.get("kind") != "address":
            continue
        m = orc.cert_meta(der)[2]
        out.setdefault(("name", row["length"]), set()).add(int(offs[i] + m.issuer_off) % 16)
        out.setdefault(("uri", row["length"]), set()).add(int(offs[i] + m.crl_off[0]) % 16)
    return out


# ------------------------------------------------------------------ crowd
CROWD_ISSUERS = 3


def crowd_uri(k):
    """The k-th URI of the crowd: 24, 24, 41 or 71 octets."""
    return b"http://crowd.example/%07d" % k + (b"", b"", b"/a-longer-path.crl", b"/" + b"p" * 42 + b".crl")[k & 3]


def crowd_certs(pairs, tag):
    """One certificate per (k1, k2) or (k1, k2, k): URIs crowd_uri(k1), crowd_uri(k2); `tag` keeps the serials of separate
    batches apart.  The issuer follows k (k1 when absent); each issuer shows one Name and one hour."""
    names = [_name(b"Crowd CA %d" % k) for k in range(CROWD_ISSUERS)]
    certs = []
    for j, (k1, k2, *k) in enumerate(pairs):
        iss = (k[0] if k else k1) % CROWD_ISSUERS
        der = D.cert(serial=bytes([1 + tag]) + j.to_bytes(3, "big"), issuer=names[iss],
                     exts=[D.BC_NOT_CA, dp_ext(dp(uri(crowd_uri(k1)), uri(crowd_uri(k2))))])
        certs.append((der, iss))
    return certs


def crowd(n, start=0, tag=0):
    """n distinct URIs start .. start + n − 1, two per certificate, both under the certificate's issuer."""
    assert n % 2 == 0
    c = Corpus(issuers(CROWD_ISSUERS))
    pairs = [(start + 2 * j, start + 2 * j + 1) for j in range(n // 2)]
    c.certs = crowd_certs(pairs, tag)
    c.rows = [dict(kind="crowd", role="A", uris=[crowd_uri(a), crowd_uri(b)]) for a, b in pairs]
    return c


# ------------------------------------------------------------------ overflow
def overflow(n_big=500, n_small=20, n_seen=20, small_uris=1):
    """Two batches: `small` (role A) and `big` (role again, so that part("second") is the big one).  Every one of the big
    batch's first n_big certificates brings a fresh Name, a fresh hour and four fresh URIs — six first sightings, more than
    the 3·n + 1024 items ctmr_meta_new's first buffer holds.  The small batch shows the Name, the hour and the first URI of
    the big batch's certificates 0 .. n_small − 1 before (small_uris = 4: all four URIs); the big batch ends with n_seen
    certificates that show exactly those again — certificates the map kernel's pre-check finds wholly seen in the memo the small batch left."""
    c = Corpus(issuers(2))

    def parts(k):
        hour = "28%02d%02d%02d0000Z" % (1 + k // 672 % 12, 1 + k // 24 % 28, k % 24)
        return _name(b"Overflow CA %04d" % k), D.utctime(hour), [b"http://overflow.example/%04d/%d.crl" % (k, j) for j in range(4)]

    for k in range(n_small):
        nm, na, us = parts(k)
        c.add(k & 1, "A", issuer=nm, not_after=na, exts=[D.BC_NOT_CA, dp_ext(dp(*[uri(u) for u in us[:small_uris]]))],
              kind="small", uris=us[:small_uris])
    for k in range(n_big):
        nm, na, us = parts(k)
        c.add(k & 1, "again", issuer=nm, not_after=na, exts=[D.BC_NOT_CA, dp_ext(dp(*[uri(u) for u in us]))], kind="big", uris=us)
    for k in range(n_seen):
        nm, na, us = parts(k % max(n_small, 1))
        c.add(k & 1, "again", issuer=nm, not_after=na, exts=[D.BC_NOT_CA, dp_ext(dp(uri(us[0])))], kind="seen", uris=us[:1])
    return c
