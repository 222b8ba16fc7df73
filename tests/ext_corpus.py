"""Certificates that put the extension-body rules (strict_extensions) to every window position of the map kernels (test
helper, no test; pure tests/der.py, no GPU, seeded and deterministic).  der_walk.h checks the bodies Go's parseCertificate
unmarshals: ext_body_check (keyUsage, subjectKeyIdentifier, extKeyUsage, authorityKeyIdentifier, certificatePolicies, the two
InfoAccess lists), ext_san_check / ext_san_coop with san_uri_ok, crl_dps with rel_name, ext_nc_check, ext_sct_ok,
ext_ipaddr_ok and ext_asnum_ok.  On the device the same code runs behind kernels/readers.h: a 224-octet LDS window whose
reads outside are clamped and only remembered (miss), content parsers that are reached through defer_exact() alone, and a
wave-collective walk of the subjectAltName.  Wrong, each of these is silent: a certificate keeps or loses its place.

THE RULES, stated once: TABLES holds, extension by extension, the hand-built bodies that tests/test_ext_cpu.py pins one by
one between the oracle and the host build of the walk — each row (Extension octets, verdict):
  clean            nothing to say
  fatal            the certificate does not parse under strict_extensions
  finding          what CT-go files as non-fatal inside the body (WALK_NF_EXT)
  string_finding   a character set inside a distribution point's nameRelativeToCRLIssuer (WALK_NF_STRING: under
                   strict_strings as well)
and every certificate of a family carries such a verdict, from which its status follows without asking the oracle
(expected_status): fatal — PARSE_ERROR; a finding — PARSE_ERROR for a precertificate entry, PASS for an X509 entry; clean —
PASS.  tests/test_ext_corpus_cpu.py holds the oracle and the host build to every verdict.

LAYOUT.  Every certificate has a serial of its own (eight octets: the family's number, 11 11 11, a counter in four octets
01..7e), an RSA key, the issuer Name of tests/geometry_corpus.py and basicConstraints behind the extension under test.
Every case is built as an X509 entry and as a precertificate entry (et 0, 1), interleaved.  TWINS (Family.pairs: (i, j,
kind)) have equal length and differ, outside their serials, only in the `span` octets their kind states — the last octets
the rule reads; the first is the clean one.  No family's size is a multiple of 64: the last wave is partial.

Families:
  rules          every row of TABLES as the only extension next to basicConstraints
  slide          per kind (SLIDE_KINDS: ext_body_check's kinds 1..6 and the second InfoAccess list, subjectAltName iPAddress
                 and URI, a distribution point's reasons and its nameRelativeToCRLIssuer — fatal, finding and string
                 finding —, nameConstraints dNS, rfc822, URI and IP mask, the SCT list, ipAddrBlock, autonomousSysNum) one
                 twin pair behind ONE filler extension of every length the encoding has from 0 (none) to 255 — there is no
                 Extension of 1..6 octets, and no DER element of 130: two of 65 —, so that the deciding octet lies at every
                 offset from the extension block's start (d0 + 7 .. d0 + 255, d0 = its offset without a filler: at least
                 every offset 64..255) — through one window (224) and two 16-octet refill steps
  san_elements   a subjectAltName of k = 0, 2..300 octets of dNSNames (no element has one octet), one SPECIAL element, a
                 dNSName tail; with the three forms of the SEQUENCE's header the special element's header lies at every
                 offset 2..300 of the value (0 and 1 are that header's).  Then: a subjectAltName behind a filler extension
                 whose own three headers (13 octets) begin at every offset 200..223 of the extension block; two
                 subjectAltNames, the good or the bad one first; an empty value; a bad subjectAltName behind an extension
                 that is fatal already
  chain0()       CA certificates (each with a key of its own, one ordinary leaf under it): every row of `rules` and every
                 kind of `slide` at 16 filler lengths — registered through add_issuers or met as Chain[0] of raw entries,
                 they run through k_issuer_ids with the exact reader; any finding drops the issuer
"""
import functools
from dataclasses import dataclass, field

import numpy as np

from ct_mapreduce_amd import synth
from ct_mapreduce_amd.engine import Batch
from oracle import oracle as orc
from tests import der as D
from tests import geometry_corpus as G

FILT = G.FILT
NOW = synth.BASE_TIME
N_ISSUERS = G.N_ISSUERS
CLEAN, FATAL, FINDING, STRING_FINDING = "clean", "fatal", "finding", "string_finding"
VERDICTS = (CLEAN, FATAL, FINDING, STRING_FINDING)
IDS = dict(rules=0x51, slide=0x52, san_elements=0x53, chain0=0x54)

AIA_OID = D.tlv(0x06, bytes.fromhex("2b06010505070101"))
SIA_OID = D.tlv(0x06, bytes.fromhex("2b0601050507010b"))
IPADDR_OID = D.tlv(0x06, bytes.fromhex("2b06010505070107"))
ASNUM_OID = D.tlv(0x06, bytes.fromhex("2b06010505070108"))
SCT_OID = D.tlv(0x06, bytes.fromhex("2b06010401d679020402"))
OCSP = D.tlv(0x06, bytes.fromhex("2b06010505073001"))
CA_REPO = D.tlv(0x06, bytes.fromhex("2b06010505073005"))
POL = D.tlv(0x06, bytes.fromhex("6086480186f8420101"))
EKU_SRV = D.tlv(0x06, bytes.fromhex("2b06010505070301"))
EKU_CLI = D.tlv(0x06, bytes.fromhex("2b06010505070302"))
NULL = b"\x05\x00"


# ------------------------------------------------------------------ the builders of one Extension
def x(oid_last, value):
    return D.ext(oid_last, value)


def aia(value):
    return D.seq(AIA_OID, D.tlv(0x04, value))


def sia(value):
    return D.seq(SIA_OID, D.tlv(0x04, value))


def ipaddr(value, critical=True):
    return D.seq(IPADDR_OID, *([D.tlv(0x01, b"\xff")] if critical else []), D.tlv(0x04, value))


def asnum(value):
    return D.seq(ASNUM_OID, D.tlv(0x01, b"\xff"), D.tlv(0x04, value))


def bits(b, pad=0):
    return D.tlv(0x03, bytes([pad]) + b)


def san(*names):
    return x(17, D.seq(*names))


def uri(u):
    return D.tlv(0x86, u if isinstance(u, bytes) else u.encode())


def dps(*points):
    return x(31, D.seq(*points))


def fullname(*names):
    return D.tlv(0xa0, D.tlv(0xa0, b"".join(names)))


def rel(val, attr=5):
    """cRLDistributionPoints with one nameRelativeToCRLIssuer of one attribute."""
    return dps(D.seq(D.tlv(0xa0, D.tlv(0xa1, D.tlv(0x31, D.seq(D.oid(0x55, 4, attr), val))))))


def nc(permitted=None, excluded=None, raw=None):
    body = b""
    if permitted is not None:
        body += D.tlv(0xa0, b"".join(D.seq(c) for c in permitted))
    if excluded is not None:
        body += D.tlv(0xa1, b"".join(D.seq(c) for c in excluded))
    return x(30, D.seq(body) if raw is None else raw)


def sct_ext(value):
    return D.seq(SCT_OID, D.tlv(0x04, value))


def sct_list(*s):
    return D.tlv(0x04, len(b"".join(s)).to_bytes(2, "big") + b"".join(s))


def dns(b):
    return D.tlv(0x82, b)


def rows(verdict, exts):
    return [(e, verdict) for e in exts]


# ------------------------------------------------------------------ 1. the rule tables
def _key_usage():
    return rows(CLEAN, [x(15, D.tlv(0x03, b"\x05\xa0")),
                        x(15, D.tlv(0x03, b"\x00")),                                # no bits at all
                        x(15, D.tlv(0x03, b"\x07\x80"))]) + \
        rows(FATAL, [x(15, v) for v in (
            D.tlv(0x03, b""), D.tlv(0x03, b"\x08\x00"), D.tlv(0x03, b"\x01"), D.tlv(0x03, b"\x05\xa1"),   # parseBitString
            D.tlv(0x04, b"\x05\xa0"), D.tlv(0x23, D.tlv(0x03, b"\x05\xa0")),                             # wrong / constructed tag
            D.tlv(0x03, b"\x05\xa0") + b"\x00", b"", b"\x03\x05\x05\xa0")])                               # trailing; empty; truncated


def _subject_key_identifier():
    return rows(CLEAN, [x(14, D.tlv(0x04, b"\x11" * 20)), x(14, D.tlv(0x04, b""))]) + \
        rows(FATAL, [x(14, v) for v in (D.tlv(0x03, b"\x00\x11"), D.tlv(0x24, D.tlv(0x04, b"\x11")), D.tlv(0x04, b"\x11") + b"\x05\x00", b"",
                                        b"\x04\x81\x01\x11")])                     # … and a length that is not minimal


def _ext_key_usage():
    return rows(CLEAN, [x(37, D.seq(EKU_SRV, EKU_CLI)), x(37, D.seq())]) + \
        rows(FATAL, [x(37, v) for v in (
            D.seq(EKU_SRV, D.tlv(0x0c, b"x")),                                      # sequence tag mismatch
            D.seq(D.tlv(0x06, b"")), D.seq(D.tlv(0x06, b"\x2a\x81")), D.seq(D.tlv(0x06, b"\x2a\x88\x80\x80\x80\x00")),
            D.tlv(0x31, EKU_SRV), D.seq(EKU_SRV) + b"\x00\x00", D.seq(EKU_SRV)[:-1] + b"", EKU_SRV)])


def _authority_key_identifier():
    kid = D.tlv(0x80, b"\x22" * 20)
    return rows(CLEAN, [x(35, D.seq(kid)), x(35, D.seq()),
                        x(35, D.seq(kid, D.tlv(0xa1, b"\xff\xff"), D.tlv(0x82, b"\x01"))),    # whatever follows the first field is ignored
                        x(35, D.seq(D.tlv(0xa1, D.tlv(0x86, b"u")), D.tlv(0x82, b"\x01"))),    # no keyIdentifier: the field is skipped
                        x(35, D.seq(D.tlv(0xa0, b"\x01"))),                                    # [0] but constructed: does not match, skipped
                        x(35, D.seq(b"\x81\x7f"))]) + \
        rows(FATAL, [x(35, v) for v in (                                                      # (above: a skipped element need not even fit)
            D.seq(b"\x80\x7f\x01"),                                                           # the keyIdentifier itself must fit
            D.seq(b"\x9f"), D.seq(b"\x80\x81\x01\x00"),                                       # its header must parse (truncated tag; length not minimal)
            D.tlv(0x31, kid), D.seq(kid) + b"\x00", b"")])


def _certificate_policies():
    q = D.seq(D.tlv(0x06, bytes.fromhex("2b06010505070201")), D.tlv(0x16, b"http://cps"))
    return rows(CLEAN, [x(32, D.seq(D.seq(POL), D.seq(POL, D.seq(q)))),
                        x(32, D.seq(D.seq(POL, b"\xff\xff"))),                      # what follows the OID is not looked at
                        x(32, D.seq())]) + \
        rows(FATAL, [x(32, v) for v in (D.seq(POL), D.seq(D.seq()), D.seq(D.seq(D.tlv(0x0c, b"x"))), D.seq(D.seq(D.tlv(0x06, b"\x2a\x81"))),
                                        D.seq(D.seq(POL), D.tlv(0x31, POL)), D.seq(D.seq(POL)) + b"\x05\x00", D.tlv(0x30, b"\x30"))])


def _authority_info_access():
    loc = D.tlv(0x86, b"http://ocsp.example")
    return rows(CLEAN, [aia(D.seq(D.seq(OCSP, loc), D.seq(OCSP, D.tlv(0x0c, b"anything")))),
                        aia(D.seq(D.seq(OCSP, loc, b"\xff")))]) + \
        rows(FATAL, [aia(v) for v in (
            D.seq(D.seq(OCSP)),                                                     # Location is not optional: "sequence truncated"
            D.seq(D.seq(loc, OCSP)), D.seq(D.seq(OCSP, b"\x86\x05ab")), D.seq(OCSP, loc),
            D.seq(D.seq(OCSP, loc)) + b"\x00", D.tlv(0x31, D.seq(OCSP, loc)),
            D.seq())])                                                              # CT-go (recalled): "x509: empty AuthorityInfoAccess extension"


def _subject_info_access():
    """CT-go's fork knows 1.3.6.1.5.5.7.1.11 (the standard library does not): []accessDescription filling the value, failure
    and trailing data fatal, an empty list an error (recalled — go.mod:10; round 6)."""
    loc = D.tlv(0x86, b"rsync://repo.example/ca/")
    # the neighbouring id-pe numbers are not this extension: an unknown extension's value is not looked at
    neighbours = [D.seq(D.tlv(0x06, bytes.fromhex("2b06010505070100")[:-1] + bytes([last])), D.tlv(0x04, b"\xff\xff")) for last in (0x02, 0x0a, 0x0c)]
    return rows(CLEAN, [sia(D.seq(D.seq(CA_REPO, loc), D.seq(CA_REPO, D.tlv(0xa4, b"\x31\x00")))),
                        sia(D.seq(D.seq(CA_REPO, loc, b"\xff")))]) + \
        rows(FATAL, [sia(v) for v in (
            D.seq(), D.seq(D.seq(CA_REPO)), D.seq(D.seq(loc, CA_REPO)), D.seq(D.seq(CA_REPO, b"\x86\x05ab")), D.seq(CA_REPO, loc),
            D.seq(D.seq(CA_REPO, loc)) + b"\x00", D.tlv(0x31, D.seq(CA_REPO, loc)), b"", D.seq(D.seq(D.tlv(0x06, b"\x2a\x81"), loc)))]) + \
        rows(CLEAN, neighbours)


def ipaddr_bodies():
    """(clean bodies, bodies with a finding) of sbgp-ipAddrBlock as CT-go's x509/rpki.go decodes it (recalled; go.mod:10): strict
    asn1.Unmarshal calls, every failure an nfe.AddError — the certificate parses, a precertificate and a Chain[0] issuer
    are dropped over the finding."""
    v4, v6 = D.tlv(0x04, b"\x00\x01"), D.tlv(0x04, b"\x00\x02\x01")
    fam = lambda af, choice, *more: D.seq(af, choice, *more)
    ok = [D.seq(), D.seq(fam(v4, NULL)), D.seq(fam(v4, D.seq(bits(b"\x0a"), bits(b"\xc0\xa8\x80", 7)))),
          D.seq(fam(v4, D.seq(D.seq(bits(b"\x0a\x00"), bits(b"\x0a\xff"))), b"\xff\xff"), fam(v6, NULL)),   # behind the last field: ignored
          D.seq(fam(v6, D.seq())), D.seq(fam(v4, D.seq(D.seq(bits(b"\x0a"), bits(b"\x0b"), b"\x00"))))]
    findings = [b"", D.tlv(0x31, fam(v4, NULL)), D.seq(fam(v4, NULL)) + b"\x00",            # not one SEQUENCE filling the value
                D.seq(D.tlv(0x31, v4 + NULL)), D.seq(fam(D.tlv(0x24, v4), NULL)), D.seq(fam(D.tlv(0x03, b"\x00\x01"), NULL)),
                D.seq(D.seq(v4)), D.seq(D.seq(v4, b"\x30\x05\x00")),                     # Choice missing / does not fit
                D.seq(fam(D.tlv(0x04, b"\x01"), NULL)), D.seq(fam(D.tlv(0x04, b"\x00\x01\x01\x01"), NULL)),   # AFI of 1 or 4 octets
                D.seq(fam(v4, b"\x05\x81\x00")), D.seq(fam(v4, D.tlv(0x04, b""))), D.seq(fam(v4, D.tlv(0x31, bits(b"\x0a")))),
                D.seq(fam(v4, D.seq(b"\x03\x05\x00"))),                                   # an element that does not fit
                D.seq(fam(v4, D.seq(D.tlv(0x03, b"")))), D.seq(fam(v4, D.seq(bits(b"\x0a", 8)))), D.seq(fam(v4, D.seq(bits(b"\x0b", 1)))),
                D.seq(fam(v4, D.seq(D.tlv(0x83, b"\x00\x0a")))), D.seq(fam(v4, D.seq(D.tlv(0x23, bits(b"\x0a"))))),   # number 3, not universal primitive
                D.seq(fam(v4, D.seq(D.seq(bits(b"\x0a"))))), D.seq(fam(v4, D.seq(D.seq(bits(b"\x0a"), D.tlv(0x04, b"\x00"))))),
                D.seq(fam(v4, D.seq(D.tlv(0xb0, bits(b"\x0a") + bits(b"\x0b"))))),       # number 16 of another class
                D.seq(fam(v4, D.seq(D.tlv(0x04, b"\x0a")))), D.seq(fam(v4, D.seq(b"\x9f\x21\x00"))),
                D.seq(fam(v4, NULL), fam(v4, D.seq(D.tlv(0x02, b"\x01"))))]
    return ok, findings


def _ip_addr_block():
    ok, findings = ipaddr_bodies()
    return rows(CLEAN, [ipaddr(v) for v in ok]) + rows(FINDING, [ipaddr(v) for v in findings]) + \
        rows(FINDING, [ipaddr(findings[5], critical=False)])


def asnum_bodies():
    """sbgp-autonomousSysNum: struct { ASNum RawValue `optional,tag:0`; RDI RawValue `optional,tag:1` } filling the value; a
    choice's contents are NULL or one []RawValue of INTEGERs (`int`: minimal, at most 8 octets) and ASIDRange pairs."""
    i = lambda b: D.tlv(0x02, b)
    ok = [D.seq(), D.seq(D.tlv(0xa0, NULL)), D.seq(D.tlv(0xa0, D.seq(i(b"\x01"), D.seq(i(b"\x02"), i(b"\x00\xff\xff"))))),
          D.seq(D.tlv(0xa0, NULL), D.tlv(0xa1, D.seq(i(b"\x7f" + b"\xff" * 7)))), D.seq(D.tlv(0xa1, D.seq())),
          D.seq(D.tlv(0x80, NULL)),                                  # `tag:0` on a RawValue: the class and the number, either form
          D.seq(D.tlv(0xa0, D.seq(i(b"\x01"))), b"\xff\xff\xff"[:0] + D.tlv(0xa2, b"\x01")),   # what follows the two fields: ignored
          D.seq(D.tlv(0xa1, NULL), D.tlv(0xa0, b"\x02")),            # [0] behind [1]: never reached
          D.seq(D.tlv(0xa0, D.seq(D.seq(i(b"\x01"), i(b"\x02"), b"\x05\x00"))))]
    findings = [b"", D.tlv(0x31, D.tlv(0xa0, NULL)), D.seq(D.tlv(0xa0, NULL)) + b"\x00",
                D.seq(b"\xa0\x05\x05\x00"), D.seq(b"\x9f"),                            # a matching field must fit; a header must parse
                D.seq(D.tlv(0xa0, b"")), D.seq(D.tlv(0xa0, b"\x05\x81\x00")), D.seq(D.tlv(0xa0, NULL + b"\x00")),
                D.seq(D.tlv(0xa0, D.tlv(0x31, i(b"\x01")))), D.seq(D.tlv(0xa0, D.seq(i(b"\x01")) + b"\x00")),
                D.seq(D.tlv(0xa0, D.seq(b"\x02\x05\x01"))), D.seq(D.tlv(0xa0, D.seq(i(b"")))), D.seq(D.tlv(0xa0, D.seq(i(b"\x00\x01")))),
                D.seq(D.tlv(0xa0, D.seq(i(b"\x01" * 9)))), D.seq(D.tlv(0xa0, D.seq(D.tlv(0x82, b"\x01")))),
                D.seq(D.tlv(0xa0, D.seq(D.seq(i(b"\x01"))))), D.seq(D.tlv(0xa0, D.seq(D.seq(i(b"\x01"), D.tlv(0x04, b"\x02"))))),
                D.seq(D.tlv(0xa0, D.seq(D.tlv(0x04, b"\x01")))), D.seq(D.tlv(0xa0, NULL), D.tlv(0xa1, D.seq(i(b"\xff\xff"))))]
    return ok, findings


def _as_identifiers():
    ok, findings = asnum_bodies()
    return rows(CLEAN, [asnum(v) for v in ok]) + rows(FINDING, [asnum(v) for v in findings])


def long_san(*last):
    """A subjectAltName of some 450 octets — two windows — that ends in `last`."""
    return san(*[dns(b"host-%02d.a-rather-long-name.example" % k) for k in range(12)], *last)


def _subject_alt_name():
    """forEachSAN: one universal constructed SEQUENCE filling the value, every element a TLV that fits, dispatched on the
    tag NUMBER alone."""
    return rows(CLEAN, [san(dns(b"a.example"), D.tlv(0x81, b"x@a.example"), D.tlv(0x87, bytes(4)), D.tlv(0x87, bytes(16)),
                            uri("https://a.example/x")),
                        san(),                                                      # empty: parses (only "unhandled" when critical)
                        san(dns(b"\xff\x00 not IA5")),                              # no character set is checked on the parse side
                        san(D.tlv(0xa0, b"\xff\xff"), D.tlv(0xa4, b"\x05"), D.tlv(0x88, b""), D.tlv(0x05, b"")),   # other names: not looked into
                        san(b"\x9f\x21\x01\x00")]) + \
        rows(FATAL, [x(17, v) for v in (                                            # (above: a high-tag-number element, number 33 — no case)
            b"", D.tlv(0x31, dns(b"a")), D.tlv(0x10, dns(b"a")),                    # not 0x30
            D.seq(dns(b"a")) + b"\x00", D.seq(b"\x82\x05ab"), D.seq(b"\x82"), D.seq(b"\x82\x81\x01a"),
            D.seq(b"\x9f\x1e\x00"))]) + \
        rows(FINDING,                                                               # (above: the high-tag-number form for a number below 31)
             # iPAddress of another length: CT-go files it as NON-fatal (the stdlib fails); any class with number 7 counts
             [san(D.tlv(0x87, bytes(n))) for n in (0, 3, 5, 8, 15, 17, 32)] +
             [san(D.tlv(0x07, b"abc")), san(D.tlv(0xa7, D.tlv(0x04, b"abc"))),
              san(dns(b"ok"), D.tlv(0x87, bytes(4)), D.tlv(0x87, bytes(5)))]) + \
        [(long_san(D.tlv(0x87, bytes(4)), uri("https://u@a.example:8443/x%20y?q#f")), CLEAN),   # longer than the window that holds it
         (long_san(uri("http://a b/")), FATAL), (long_san(D.tlv(0x87, bytes(5)), dns(b"tail.example")), FINDING),
         (long_san(b"\x82\x05ab"), FATAL)]


URI_OK = ["https://a.example/x", "http://a.example:8080/p?q#f", "urn:isbn:0451450523", "mailto:u@h", "", "*", "/just/a/path",
          "relative/path", "?q=1", "#frag", "http://", "http:///path", "///three", "//host.example/x", "http://[::1]:80/",
          "http://[fe80::1%25en0]/", "http://u:p@h.example/", "http://u%41@h.example",
          "http://h.example/%41", "http://h.example/a%20b", "http://a.b/c?%zz", "HTTP://A.EXAMPLE", "a+b-c.d:rest",
          "http://h.example:/x", "http://h!$&'()*+,;=.example", "http://h.example/\x80\xff",
          "http://a.example/#%41", "http://a_b.example", "x://h<>\"/", "http://h/a:b", "./a:b", "http://h/?\x01"[:9], "*#f",
          "http://@h/", "http://:@h/", "http://h.example:80", "x:", "x:%zz", "http://a@b@c/",
          # ONE leading dot passes domainToReverseLabels in the release the reference builds with: labels are cut off the END and
          # the empty one in front is never recorded (later releases append it: "domain is prefixed with an empty label")
          "http://.example/", "//.h/", "http://.a.b:80/"]
URI_BAD = [":", ":x", "a b"[0:0] + "\x7f", "http://a\x01", "\x00", "http://h/\x1f", "a b:c",   # control characters; a colon in the first segment
           "//h:port/", "http://h:80x/", "http://h:-1", "http://[::1", "http://[::1]x", "http://[::1]:x", "http://a:b:c/",
           "http://h%20x/", "http://h%41/", "http://%zz/", "http://h/%", "http://h/%4", "http://h/%zz", "http://h/#%", "http://h/#%g1",
           "http://h x/", "http://h\\x/", "http://h^x/", "http://h`x/", "http://h{x/", "http://h|x/", "http://h}x/",
           "http://u ser@h/", "http://us\x80er@h/", "http://u%zz@h/", "http://u:p%@h/", "http://a@b@c d/",
           "http://..example/", "http://./", "http://example./", "http://a..b/", "http://h\x80/", "http://h%c3%a9/", "http://[::1%25\x80]/",
           "http://[fe80::1%25e%7fn]/", "//..h/", "*\x01", "http://h/%41%zz",
           "1http://x/y",                                            # no scheme (a digit first): a colon in the first path segment
           "http://[fe80::1%25e%20n]/"]                              # url.Parse takes the space in the zone, domainToReverseLabels does not


def _subject_alt_name_uri():
    """A subjectAltName URI goes through url.Parse."""
    return rows(CLEAN, [san(uri(u.encode("latin-1"))) for u in URI_OK]) + \
        rows(FATAL, [san(uri(u.encode("latin-1"))) for u in URI_BAD if u]) + \
        rows(FATAL, [san(D.tlv(0x06, b":x")),                                       # any class with number 6; the URI among other names
                     san(dns(b"fine"), uri("http://ok.example"), D.tlv(0xa6, b"\x7f"))])


def _crl_distribution_points():
    u = D.tlv(0x86, b"http://crl.example/a.crl")
    many = [D.tlv(0x86, b"http://crl-%02d.a-rather-long-name.example/a.crl" % k) for k in range(6)]
    return rows(CLEAN, [
        dps(D.seq(fullname(u))),
        dps(),                                                       # an empty SEQUENCE OF
        dps(D.seq()),                                                # every field optional
        dps(D.seq(fullname(u), D.tlv(0x81, b"\x01\x06"), D.tlv(0xa2, D.tlv(0xa4, b"")))),
        dps(D.seq(fullname(u, dns(b"x"), D.tlv(0x05, b"")), b"\x05\x00\xff")),   # names of any kind; behind the fields only the next header must parse
        dps(D.seq(D.tlv(0x81, b"\x00"), fullname(b"\xff"))),                      # fields out of order: [0] behind reasons is never parsed
        dps(D.seq(D.tlv(0x82, b"anything"))),                        # cRLIssuer primitive
        dps(D.seq(D.tlv(0x80, b"\xff"))),                            # [0] primitive: no field matches, skipped
        dps(D.seq(D.tlv(0xa0, b""))),                                # an empty distributionPointName
        dps(D.seq(D.tlv(0xa0, D.tlv(0xa1, D.tlv(0x31, D.seq(D.oid(0x55, 4, 3), D.tlv(0x0c, b"rel"))))))),   # nameRelativeToCRLIssuer
        dps(D.seq(D.tlv(0xa0, D.tlv(0xa0, b"") + D.tlv(0xa1, b"")))),              # both, empty
        dps(D.seq(D.tlv(0xa0, D.tlv(0xa2, b"\xff") + b"\x00\x00"))),              # inside [0]: another tag skipped, the rest ignored
        dps(D.seq(fullname(*many)), D.seq(D.tlv(0x81, b"\x01\x06")))]) + \
        rows(FATAL, [x(31, v) for v in (                                          # (above: longer than the 200 octets its hint asks for)
            b"", D.tlv(0x31, b""), D.seq() + b"\x00", D.seq(D.tlv(0x31, b"")), D.seq(D.tlv(0x04, b"")),      # outer, elements
            D.seq(D.seq(b"\xa0")), D.seq(D.seq(b"\xa0\x05ab")), D.seq(D.seq(b"\x9f")),                      # a field header that does not parse / fit
            D.seq(D.seq(D.tlv(0xa0, b"\xa0"))), D.seq(D.seq(D.tlv(0xa0, b"\xa0\x03ab"))),                   # … inside the name
            D.seq(D.seq(fullname(b"\x86\x05ab"))), D.seq(D.seq(fullname(u, b"\x86"))),                     # FullName elements must fit
            D.seq(D.seq(D.tlv(0x81, b""))), D.seq(D.seq(D.tlv(0x81, b"\x08\x00"))), D.seq(D.seq(D.tlv(0x81, b"\x01\x01"))),   # reasons: parseBitString
            D.seq(D.seq(D.tlv(0x81, b"\x00"), b"\x82\x05ab")), D.seq(D.seq(b"\xa2\x05ab")),               # cRLIssuer must fit
            D.seq(D.seq(fullname(u), b"\x9f")), D.seq(D.seq(D.tlv(0x81, b"\x00"), b"\x81")),               # the header behind a field
            D.seq(D.seq(D.tlv(0xa0, D.tlv(0xa1, D.tlv(0x30, b""))))),                                        # RelativeName: SET elements
            D.seq(D.seq(D.tlv(0xa0, D.tlv(0xa1, D.tlv(0x31, D.seq(D.oid(0x55, 4, 3))))))),                   # … the value is not optional
            D.seq(D.seq(D.tlv(0xa0, D.tlv(0xa1, D.tlv(0x31, D.seq(D.tlv(0x06, b"\x55\x84"), D.tlv(0x0c, b"x"))))))),
            D.seq(D.seq(D.tlv(0xa0, D.tlv(0xa1, D.tlv(0x31, D.seq(D.oid(0x55, 4, 3), D.tlv(0x02, b""))))))),
            D.seq(D.seq(D.tlv(0xa0, D.tlv(0xa0, b"") + D.tlv(0xa1, b"\x31")))),
            D.seq(D.seq(fullname(*many)), D.seq(D.tlv(0x81, b"\x01\x07"))))]) + \
        [(rel(D.tlv(0x02, b"\x00\x01")), FINDING),                   # findings inside nameRelativeToCRLIssuer: an INTEGER only the lax parser
         (rel(D.tlv(0x13, b"a@b")), STRING_FINDING)]                 # takes; a PrintableString with '@'


NC_BAD = (dns(b"exa mple.com"), dns(b"example..com"), dns(b"example.com."), dns(b"...example.com"), dns(b".."), dns(b"\x80"), dns(b"a\x7fb"),
          D.tlv(0x87, bytes(7)), D.tlv(0x87, bytes(9)), D.tlv(0x87, bytes(4) + b"\xff\x00\xff\x00"), D.tlv(0x87, bytes(4) + b"\xfd\x00\x00\x00"),
          D.tlv(0x87, bytes(16) + b"\x00" * 15 + b"\x01"),
          D.tlv(0x81, b"@example.com"), D.tlv(0x81, b".user@example.com"), D.tlv(0x81, b"us..er@example.com"), D.tlv(0x81, b"user.@x"),
          D.tlv(0x81, b'"unterminated@example.com'), D.tlv(0x81, b'"a"b@example.com'), D.tlv(0x81, b"a b@example.com"),
          D.tlv(0x81, b"user@exa mple"), D.tlv(0x81, b"user@..example"), D.tlv(0x81, b"user@example."), D.tlv(0x81, b"u\\@x"), D.tlv(0x81, b'"\\\n"@x'), D.tlv(0x81, b"ex ample.com"),
          D.tlv(0x81, b"\xe9@example.com"),
          D.tlv(0x86, b"1.2.3.4"), D.tlv(0x86, b"01.02.03.004"), D.tlv(0x86, b"::1"), D.tlv(0x86, b"::"), D.tlv(0x86, b"2001:db8::1"),
          D.tlv(0x86, b"1:2:3:4:5:6:7:8"), D.tlv(0x86, b"::ffff:1.2.3.4"), D.tlv(0x86, b"1:2:3:4:5:6:1.2.3.4"),
          D.tlv(0x86, b"exa mple"), D.tlv(0x86, b"a..b"), D.tlv(0x86, b"\xff"))
# not addresses → judged as domains (all fine: ':' is a printable label octet)
NC_NOT_ADDRESSES = (b"1:2:3:4:5:6:7", b"1:2:3:4:5:6:7:8:9", b"::1::", b"1::2::3", b"12345::", b":1", b"1:", b"::1.2.3", b"1.2.3.4.5",
                    b"1:2:3:4:5:1.2.3.4", b"g::1", b"1:2:3:4:5:6:7:1.2.3.4", b"ffffff::")


def _name_constraints():
    """nameConstraints as cryptobyte reads them."""
    good = [nc([dns(b"example.com")], [dns(b".example.org")]),
            # one leading dot is trimmed by the caller, a second one passes domainToReverseLabels (see the URI cases); a third does not
            nc([dns(b"..example.com"), D.tlv(0x81, b"user@.example"), D.tlv(0x81, b"..example.com"), D.tlv(0x86, b"..example.com"),
                dns(b"."), dns(b"")]),                                                     # (trimmed to nothing: no labels, no complaint)
            nc([dns(b"")]),                                              # an empty domain has no labels: fine
            nc(None, [D.tlv(0x87, bytes(4) + b"\xff\xff\xf0\x00")]),
            nc([D.tlv(0x87, bytes(16) + b"\xff" * 8 + bytes(8))]),
            nc([D.tlv(0x81, b"user@example.com"), D.tlv(0x81, b"example.com"), D.tlv(0x81, b".example.com"),
                D.tlv(0x81, b'"quoted string"@example.com'), D.tlv(0x81, b"a\\@b@example.com"), D.tlv(0x81, b"u@")]),
            nc([D.tlv(0x86, b"example.com"), D.tlv(0x86, b".example.com"), D.tlv(0x86, b"1.2.3"), D.tlv(0x86, b"1.2.3.256")]),
            nc([D.tlv(0xa4, b"\xff"), D.tlv(0x88, b"\x2a"), D.tlv(0x02, b"")]),        # other name forms: unhandled, not an error
            nc([dns(b"a") + D.tlv(0x80, b"\x00") + b"\xff\xff"])]                     # minimum / maximum are never read
    fatal = [nc(raw=b""), nc(raw=D.seq()), nc([], []), nc(raw=D.tlv(0x31, D.tlv(0xa0, D.seq(dns(b"a"))))),
             nc(raw=D.seq(D.tlv(0xa0, D.seq(dns(b"a")))) + b"\x00"),
             nc(raw=D.seq(D.tlv(0xa1, D.seq(dns(b"a"))) + D.tlv(0xa0, D.seq(dns(b"a"))))),   # [1] before [0]: toplevel not empty
             nc(raw=D.seq(D.tlv(0xa0, D.seq(dns(b"a"))) + b"\x05\x00")),
             nc(raw=D.seq(b"\xa0\x05ab")), nc(raw=D.seq(D.tlv(0xa0, D.tlv(0x31, dns(b"a"))))),
             nc(raw=D.seq(D.tlv(0xa0, D.seq()))), nc(raw=D.seq(D.tlv(0xa0, D.seq(b"\x82")))),
             nc(raw=D.seq(D.tlv(0xa0, D.seq(b"\x9f\x21\x00")))),                     # cryptobyte refuses the high-tag-number form
             nc(raw=D.seq(D.tlv(0x80, b"")))]                                        # [0] primitive: not the optional element
    for c in NC_BAD:
        fatal += [nc([c]), nc(None, [c])]
    return rows(CLEAN, good) + rows(FATAL, fatal) + rows(CLEAN, [nc([D.tlv(0x86, c)]) for c in NC_NOT_ADDRESSES])


def _sct_list():
    """The embedded SCT list: findings are non-fatal."""
    one = b"\x00\x03abc"
    return rows(CLEAN, [sct_ext(sct_list(one)), sct_ext(sct_list(one, b"\x00\x01x"))]) + \
        rows(FINDING, [sct_ext(v) for v in (
            b"", D.tlv(0x04, b""), D.tlv(0x04, b"\x00"), D.tlv(0x04, b"\x00\x00"), sct_list(), sct_list(b"\x00\x00"), sct_list(one) + b"\x00",
            D.tlv(0x04, b"\x00\x06" + one), D.tlv(0x04, b"\x00\x04" + one), sct_list(b"\x00\x05abc"), sct_list(one, b"\x00"),
            D.tlv(0x03, b"\x00\x05" + one), D.tlv(0x24, sct_list(one)))]) + \
        rows(CLEAN,      # the neighbouring OID …2.4.3 (the precertificate poison) is not an SCT list
             [D.seq(D.tlv(0x06, bytes.fromhex("2b06010401d679020403")), D.tlv(0x01, b"\xff"), D.tlv(0x04, b"\x05\x00"))])


TABLES = dict(key_usage=_key_usage(), subject_key_identifier=_subject_key_identifier(), ext_key_usage=_ext_key_usage(),
              authority_key_identifier=_authority_key_identifier(), certificate_policies=_certificate_policies(),
              authority_info_access=_authority_info_access(), subject_info_access=_subject_info_access(),
              subject_alt_name=_subject_alt_name(), subject_alt_name_uri=_subject_alt_name_uri(),
              crl_distribution_points=_crl_distribution_points(), name_constraints=_name_constraints(), sct_list=_sct_list(),
              ip_addr_block=_ip_addr_block(), as_identifiers=_as_identifiers())


# ------------------------------------------------------------------ 2. the families
def expected_status(verdict, et, strict_ext=True, strict_strings=True):
    """What the verdict of the rules makes of an entry (kernels/map.h map_one): a fatal body is a parse error; a finding
    costs a precertificate entry its place and an X509 entry nothing."""
    if not strict_ext or verdict == CLEAN:
        return orc.ST_PASS
    if verdict == FATAL:
        return orc.ST_PARSE_ERROR
    if verdict == STRING_FINDING and not strict_strings:
        return orc.ST_PASS
    return orc.ST_PARSE_ERROR if et == 1 else orc.ST_PASS


def serial_of(fam_id, k):
    """The k-th serial of a family: eight octets, every one in 01..7e (positive, minimal), distinct for k < 126^4."""
    return bytes([fam_id]) + b"\x11" * 3 + bytes(1 + (k // 126 ** j) % 126 for j in (3, 2, 1, 0))


@dataclass
class Family:
    name: str
    certs: list = field(default_factory=list)      # (der, issuer_idx, entry_type)
    verdict: list = field(default_factory=list)    # per certificate: one of VERDICTS
    pairs: list = field(default_factory=list)      # (i, j, kind): twins, i the clean one
    marks: list = field(default_factory=list)      # per certificate: the builder's bookkeeping (dict)
    cuts = None                                    # (no sequence families here: geometry_corpus.shuffled looks for it)

    def cert(self, exts, verdict, et, step=None, **mark):
        k = len(self.certs)
        step = k // 2 if step is None else step    # (notAfter and the issuer: twins share them)
        der = G.make(serial_of(IDS[self.name], k), G.ISS, D.utctime(G.when(step)), G.subj(), D.rsa_spki(), exts=list(exts) + [G.bc(False)])
        self.certs.append((der, step % N_ISSUERS, et))
        self.verdict.append(verdict)
        self.marks.append(dict(mark, et=et))
        return k

    def case(self, exts, verdict, step=None, **mark):
        """One case as an X509 entry and as a precertificate entry."""
        return [self.cert(exts, verdict, et, step, **mark) for et in (0, 1)]

    def twins(self, kind, good, bad, verdict, **mark):
        """The same, twice: the clean twin and the other one (lists of extensions of equal length)."""
        step = len(self.certs) // 2
        a = self.case(good, CLEAN, step, kind=kind, twin=0, **mark)
        b = self.case(bad, verdict, step, kind=kind, twin=1, **mark)
        self.pairs += [(a[et], b[et], kind) for et in (0, 1)]

    def finish(self):
        """No family's size is a multiple of 64: the last wave is partial."""
        if len(self.certs) % 64 == 0:
            self.case([], CLEAN, kind="plain")
        return self

    def batch(self, order=None):
        idx = range(len(self.certs)) if order is None else order
        return Batch.from_certs([self.certs[i][0] for i in idx], [self.certs[i][1] for i in idx], [self.certs[i][2] for i in idx])

    def expect(self, strict_ext=True, strict_strings=True):
        return np.array([expected_status(v, c[2], strict_ext, strict_strings) for v, c in zip(self.verdict, self.certs)], np.uint8)


@functools.lru_cache(maxsize=None)
def rules():
    fam = Family("rules")
    for table, body in TABLES.items():
        for row, (e, verdict) in enumerate(body):
            fam.case([e], verdict, kind=table, row=row)
    return fam.finish()


@functools.lru_cache(maxsize=None)
def fillers():
    """{length: one filler extension of that length} for every length an Extension can have up to 255 (none has 1..6; 0: no
    filler): the subjectKeyIdentifier of geometry_corpus.ski where it reaches the length (its body is checked: kind 2), an
    unknown extension where it does not — geometry_corpus.unknown_ext, or the same with an OID of one octet."""
    out = {}
    for n in range(250):
        for e in (G.unknown_ext(n, n), D.seq(D.tlv(0x06, b"\x2a"), D.tlv(0x04, bytes((n + i) & 0xff for i in range(n))))):
            out.setdefault(len(e), e)
    for n in range(250):
        if n % 2:
            out[len(G.ski(n))] = G.ski(n)
    return {0: None, **{n: e for n, e in out.items() if n <= 255}}


FILLER_LENGTHS = (0,) + tuple(range(7, 256))


def filler(n):
    """The filler in front: nothing, one extension of n octets, or — no DER element has 130 octets — two of 65."""
    if n == 130:
        return filler(65) * 2
    e = fillers()[n]
    return [] if e is None else [e]


def slide_kinds():
    """{kind: (clean Extension, the other one, its verdict, span)}: equal length, differing in the last `span` octets the rule
    reads."""
    kid = b"\x22" * 20
    loc = b"http://ocsp.example"
    v4 = D.tlv(0x04, b"\x00\x01")
    i = lambda b: D.tlv(0x02, b)
    tail = [dns(b"tail.example")]
    many = [dns(b"a.example")]
    return {
        "key_usage": (x(15, D.tlv(0x03, b"\x05\xa0")), x(15, D.tlv(0x03, b"\x05\xa1")), FATAL, 1),           # pad 5, a bit set below it
        "subject_key_identifier": (x(14, b"\x04\x14" + kid), x(14, b"\x04\x13" + kid), FATAL, 1),          # trailing data
        "ext_key_usage": (x(37, D.seq(EKU_SRV, EKU_CLI)), x(37, D.seq(EKU_SRV, EKU_CLI[:-1] + b"\x82")), FATAL, 1),   # an arc that never ends
        "authority_key_identifier": (x(35, D.seq(b"\x80\x14" + kid)), x(35, D.seq(b"\x80\x15" + kid)), FATAL, 1),   # must fit
        "certificate_policies": (x(32, D.seq(D.seq(POL))), x(32, D.seq(D.seq(POL[:-1] + b"\x81"))), FATAL, 1),
        "authority_info_access": (aia(D.seq(D.seq(OCSP, b"\x86\x13" + loc))), aia(D.seq(D.seq(OCSP, b"\x86\x14" + loc))), FATAL, 1),
        "subject_info_access": (sia(D.seq(D.seq(CA_REPO, b"\x86\x13" + loc))), sia(D.seq(D.seq(CA_REPO, b"\x86\x14" + loc))), FATAL, 1),
        "san_ip": (san(*many, dns(b"abc"), D.tlv(0x87, bytes([10, 1, 2, 3])), *tail),
                   san(*many, dns(b"ab"), D.tlv(0x87, bytes([10, 1, 2, 3, 4])), *tail), FINDING, 11),
        "san_uri": (san(*many, uri("http://h.example/%41")), san(*many, uri("http://h.example/%4z")), FATAL, 1),
        "dp_reasons": (dps(D.seq(D.tlv(0x81, b"\x01\x06"))), dps(D.seq(D.tlv(0x81, b"\x01\x07"))), FATAL, 1),
        "dp_rel_name": (rel(D.tlv(0x0c, b"rel"), 3), rel(D.tlv(0x0c, b"rel"), 0x83), FATAL, 1),            # the attribute's OID never ends
        "dp_rel_integer": (rel(D.tlv(0x02, b"\x00\xff")), rel(D.tlv(0x02, b"\x00\x7f")), FINDING, 1),     # not minimal: the lax parser's
        "dp_rel_string": (rel(D.tlv(0x13, b"a.b")), rel(D.tlv(0x13, b"a.@")), STRING_FINDING, 1),
        "nc_dns": (nc([dns(b"example.com")]), nc([dns(b"example.co\x80")]), FATAL, 1),
        "nc_rfc822": (nc(None, [D.tlv(0x81, b"user@example")]), nc(None, [D.tlv(0x81, b"user@exampl ")]), FATAL, 1),
        "nc_uri": (nc([D.tlv(0x86, b".example.com")]), nc([D.tlv(0x86, b".example.co\xff")]), FATAL, 1),
        "nc_ip_mask": (nc([D.tlv(0x87, bytes(4) + b"\xff\xff\x00\x00")]), nc([D.tlv(0x87, bytes(4) + b"\xff\x00\xff\x00")]), FATAL, 2),
        "sct_list": (sct_ext(sct_list(b"\x00\x03abc", b"\x00\x01x")), sct_ext(sct_list(b"\x00\x03abc", b"\x00\x02x")), FINDING, 1),
        "ip_addr_block": (ipaddr(D.seq(D.seq(v4, D.seq(bits(b"\x0a", 1))))), ipaddr(D.seq(D.seq(v4, D.seq(bits(b"\x0b", 1))))), FINDING, 1),
        "as_identifiers": (asnum(D.seq(D.tlv(0xa0, D.seq(i(b"\x01"), i(b"\x00\xff"))))), asnum(D.seq(D.tlv(0xa0, D.seq(i(b"\x01"), i(b"\x00\x7f"))))),
                           FINDING, 1),
    }


SLIDE_KINDS = tuple(slide_kinds())


@functools.lru_cache(maxsize=None)
def slide():
    fam = Family("slide")
    for kind, (good, bad, verdict, span) in slide_kinds().items():
        assert len(good) == len(bad)
        for n in FILLER_LENGTHS:
            fam.twins(kind, filler(n) + [good], filler(n) + [bad], verdict, filler=n, span=span)
    return fam.finish()


LONG_ELEMENT = dns(b"l" * 128)                      # 82 81 80 …
SPECIALS = {                                        # name: (the element, its verdict, placed last)
    "uri_good": (uri("http://h.example/%41"), CLEAN, False),
    "uri_bad": (uri("http://h.example/%4z"), FATAL, False),
    "ip4": (D.tlv(0x87, bytes([10, 1, 2, 3])), CLEAN, False),
    "ip5": (D.tlv(0x87, bytes([10, 1, 2, 3, 4])), FINDING, False),
    "ip16": (D.tlv(0x87, bytes(range(16))), CLEAN, False),
    "high_tag": (b"\x9f\x21\x01\x00", CLEAN, False),
    "high_tag_illegal": (b"\x9f\x1e\x00", FATAL, False),
    "long_form": (LONG_ELEMENT, CLEAN, False),
    "other_name": (D.tlv(0xa0, D.tlv(0x06, b"\x2b\x06\x01") + D.tlv(0xa0, D.tlv(0x0c, b"other"))), CLEAN, False),
    "truncated": (b"\x82\x05abcd", FATAL, True),    # its length runs one octet past the value: "data truncated"
}
SAN_FILL = (0,) + tuple(range(2, 301))              # octets of dNSNames in front (no element has one octet)
SAN_TAIL = 260                                      # … behind: the SEQUENCE's header is 30 82 ll ll whatever lies in front
STRADDLE = range(200, 224)                          # where in the extension block the subjectAltName's own headers begin


def san_with(k, name, tail, el=None):
    verdict, last = SPECIALS[name][1:]
    el = SPECIALS[name][0] if el is None else el
    return san(*G.dns_names(k, k), el, *([] if last else G.dns_names(tail, k + 1))), verdict


@functools.lru_cache(maxsize=None)
def san_elements():
    fam = Family("san_elements")
    for name in SPECIALS:
        for k in SAN_FILL:
            e, verdict = san_with(k, name, SAN_TAIL)
            fam.case([e], verdict, kind=name, fill=k, special=SPECIALS[name][0])
        # the shorter forms of the SEQUENCE's header: 30 ll (the element at offset 2) and 30 81 ll (at 3 and 5)
        # (the element of 131 octets never lies behind 30 ll: offset 3 is its first)
        for k, tail in ((0, 0), (0, 40), (2, 40)) if SPECIALS[name][0] is LONG_ELEMENT else ((0, 20), (0, 140), (2, 140)):
            e, verdict = san_with(k, name, tail)
            fam.case([e], verdict, kind=name, fill=k, special=SPECIALS[name][0])
    # placed last, the element's offset and the SEQUENCE's header move together: three offsets need a longer element
    for k, el in ((0, b"\x82\x7f" + b"t" * 126), (121, b"\x82\x06abcde"), (249, b"\x82\x06abcde")):
        e, verdict = san_with(k, "truncated", 0, el)
        fam.case([e], verdict, kind="truncated", fill=k, special=el)
    good = G.dns_names(300, 1) + [D.tlv(0x87, bytes([10, 1, 2, 3])), dns(b"abc")]
    bad = G.dns_names(300, 1) + [D.tlv(0x87, bytes([10, 1, 2, 3, 4])), dns(b"ab")]
    for at in STRADDLE:                             # 30 82 ll ll 06 03 55 1d 11 04 82 ll ll across the extension window's end
        fam.twins("straddle", filler(at) + [san(*good)], filler(at) + [san(*bad)], FINDING, filler=at, span=10)
    ok, ip5, bad_uri = san(dns(b"good.example")), san(dns(b"b.example"), D.tlv(0x87, bytes(5))), san(dns(b"b.example"), uri("http://a b/"))
    for n in (0, 60, 190):
        for other, verdict in ((ip5, FINDING), (bad_uri, FATAL)):
            fam.case(filler(n) + [ok, other], verdict, kind="two", filler=n)          # a second subjectAltName is walked where it is met
            fam.case(filler(n) + [other, ok], verdict, kind="two", filler=n)
            fam.case(filler(n) + [long_san(), other], verdict, kind="two", filler=n)
            fam.case(filler(n) + [other, long_san()], verdict, kind="two", filler=n)
        fam.case(filler(n) + [x(17, b"")], FATAL, kind="empty", filler=n)
        fam.case(filler(n) + [x(17, b""), ok], FATAL, kind="empty", filler=n)
        for other in (ip5, bad_uri, long_san(uri("http://a b/"))):                   # fatal already: the subjectAltName changes nothing
            fam.case(filler(n) + [x(15, D.tlv(0x03, b"")), other], FATAL, kind="fatal_before", filler=n)
            fam.case(filler(n) + [other, x(15, D.tlv(0x03, b""))], FATAL, kind="fatal_behind", filler=n)
    return fam.finish()


FAMILIES = dict(rules=rules, slide=slide, san_elements=san_elements)


def registered_issuers():
    return G.registered_issuers()


def shuffled(fam, seed=20261021):
    rng = np.random.default_rng([seed, IDS[fam.name]])
    return [int(i) for i in rng.permutation(len(fam.certs))]


CHAIN0_FILLERS = (0, 7, 23, 40, 57, 74, 91, 108, 125, 142, 159, 176, 193, 210, 227, 244)


@dataclass
class IssuerTable:
    cas: list          # CA certificates, each with a key of its own
    valid: list        # per CA: the rules find nothing in its extensions
    verdict: list
    leaves: list       # per CA: (der, entry type) of one ordinary leaf under it
    marks: list


def ca_key(k):
    return D.rsa_spki(n=b"\x00" + b"\xc3" * 253 + k.to_bytes(2, "big") + b"\xc3")


@functools.lru_cache(maxsize=None)
def chain0():
    cases = [([e], verdict, dict(kind=table, row=row)) for table, body in TABLES.items() for row, (e, verdict) in enumerate(body)]
    for kind, (good, bad, verdict, span) in slide_kinds().items():
        for n in CHAIN0_FILLERS:
            cases.append((filler(n) + [good], CLEAN, dict(kind=kind, filler=n, twin=0)))
            cases.append((filler(n) + [bad], verdict, dict(kind=kind, filler=n, twin=1)))
    out = IssuerTable([], [], [], [], [])
    for k, (exts, verdict, mark) in enumerate(cases):
        out.cas.append(D.cert(serial=serial_of(IDS["chain0"], k), subject=G.ISS, issuer=D.name(D.rdn(3, b"Geo Root")),
                              exts=list(exts) + [D.BC_CA], spki=ca_key(k)))
        out.valid.append(verdict == CLEAN)
        out.verdict.append(verdict)
        leaf = G.make(serial_of(IDS["chain0"], 100000 + k), G.ISS, D.utctime(G.when(k)), G.subj(), D.rsa_spki(), exts=[G.bc(False)])
        out.leaves.append((leaf, k % 2))
        out.marks.append(mark)
    return out
