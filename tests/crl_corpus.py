"""Hand-built DER CRLs for the probe-image tests (include/ctmr.h ctmr_crl_probes*), made with tests/der.py.
Every case carries the serials it holds as a plain Python list, and every rejection the offset at which the grammar is
left, both worked out from how the bytes were put together — never by the twin ct_mapreduce_amd/crl.py, which
tests/test_crl_corpus_cpu.py holds to these lists and tests/test_gpu_crl_probes.py then uses as the expectation."""
import functools

import numpy as np

from tests.der import SIGALG, name, oid, rdn, seq, tlv

DIGESTS = [bytes(np.random.default_rng(2600 + k).integers(0, 256, size=32, dtype=np.uint8).tolist()) for k in range(8)]
UTC = b"250101000000Z"
GEN = b"20250101000000Z"
ISSUER = name(rdn(3, b"Test CA"))
SIG = b"\x00" + b"\x5a" * 32
REASON = seq(seq(oid(0x55, 0x1d, 0x15), tlv(0x04, tlv(0x0a, b"\x01"))))          # crlEntryExtensions { reasonCode keyCompromise }
CRL_NUMBER = seq(seq(oid(0x55, 0x1d, 0x14), tlv(0x04, tlv(0x02, b"\x07"))))      # crlExtensions { cRLNumber 7 }


def length(n, form=None):
    """The length octets of n: minimal, or in a chosen form — 1..4: that many octets behind 8x whatever n needs; "80":
    indefinite; "85": five octets; ("delta", d): the minimal form of n + d."""
    if isinstance(form, tuple):
        return length(n + form[1])
    if form == "80":
        return b"\x80"
    if form == "85":
        return b"\x85" + n.to_bytes(5, "big")
    if form is not None:
        return bytes([0x80 | form]) + n.to_bytes(form, "big")
    return tlv(0, b"\0" * n)[1:len(tlv(0, b"\0" * n)) - n]


def non_minimal_forms(n):
    """Every length form the grammar refuses for contents of n octets."""
    return [nb for nb, least in ((1, 0x80), (2, 1 << 8), (3, 1 << 16), (4, 1 << 24)) if n < least] + ["80", "85"]


def enc(node):
    """node = (name, tag, bytes or [nodes / bytes], length form) → (its bytes, [(name, offset)] of it and every node in it)."""
    nm, tag, kids, form = node
    marks, content = [], b""
    if isinstance(kids, bytes):
        content = kids
    else:
        for k in kids:
            if isinstance(k, bytes):
                content += k
                continue
            b, m = enc(k)
            marks += [(n, o + len(content)) for n, o in m]
            content += b
    head = bytes([tag]) + length(len(content), form)
    return head + content, [(nm, 0)] + [(n, o + len(head)) for n, o in marks]


def entry(serial, date=UTC, date_tag=0x17, ext=None):
    """One revokedCertificates entry; ext: the crlEntryExtensions TLV, or None."""
    return tlv(0x30, tlv(0x02, serial) + tlv(date_tag, date) + (ext or b""))


def ext_of(n):
    """A crlEntryExtensions TLV of exactly n octets in all (n >= 2, and no length that has no encoding)."""
    for body in range(max(n - 6, 0), n - 1):
        t = tlv(0x30, bytes([0xc5]) * body)
        if len(t) == n:
            return t
    raise ValueError(n)


def crl(entries=(), version=True, next_update=True, crl_exts=CRL_NUMBER, sig=SIG, issuer=ISSUER, this_tag=0x17, tbs_pad=0):
    """A CRL.  entries: a list of entry bytes, or None for a CRL without revokedCertificates; tbs_pad: octets added to the
    issuer so that the tbsCertList grows.  → bytes."""
    return crl_at(entries, version, next_update, crl_exts, sig, issuer, this_tag, tbs_pad)[0]


def crl_at(entries=(), version=True, next_update=True, crl_exts=CRL_NUMBER, sig=SIG, issuer=ISSUER, this_tag=0x17, tbs_pad=0):
    """→ (the CRL, the offset of its revokedCertificates value or None)"""
    if tbs_pad:
        issuer = name(rdn(3, b"Test CA"), rdn(10, b"p" * tbs_pad))
    pre = (tlv(0x02, b"\x01") if version else b"") + SIGALG + issuer + tlv(this_tag, UTC if this_tag == 0x17 else GEN)
    pre += tlv(0x17, UTC) if next_update else b""
    value = None if entries is None else b"".join(entries)
    rev = b"" if value is None else tlv(0x30, value)
    tbs_content = pre + rev + (tlv(0xa0, crl_exts) if crl_exts is not None else b"")
    tbs = tlv(0x30, tbs_content)
    outer_content = tbs + SIGALG + tlv(0x03, sig)
    out = tlv(0x30, outer_content)
    lo = None if value is None else (len(out) - len(outer_content)) + (len(tbs) - len(tbs_content)) + len(pre) + (len(rev) - len(value))
    assert lo is None or out[lo:lo + len(value)] == value
    return out, lo


def serial_of(k, n):
    """A serial of n octets that says which it is; never a well-formed entry."""
    return bytes(((k * 7 + j * 13) % 200) + 0x38 for j in range(n))


def big_extension(k):
    """crlExtensions { cRLNumber 7, an extension of a private arc that carries k octets }"""
    return seq(CRL_NUMBER[2:], seq(tlv(0x06, bytes.fromhex("2b0601040182e91a01")), tlv(0x04, b"\xa5" * k)))


def tbs_octets(c):
    """The contents' length of the tbsCertList of the CRL c."""
    at = 2 + (c[1] & 0x7f if c[1] >= 0x80 else 0) + 1
    return c[at] if c[at] < 0x80 else int.from_bytes(c[at + 1:at + 1 + (c[at] & 0x7f)], "big")


# ---- good cases: [(name, [CRL bytes], [digest of each], [[serials of each]])]

@functools.lru_cache(maxsize=None)
def good_cases():
    D = DIGESTS
    out = []

    def one(nm, entries, serials, **kw):
        out.append((nm, [crl(entries, **kw)], [D[0]], [serials]))

    one("no revokedCertificates", None, [])
    one("no revokedCertificates, no extensions, no nextUpdate, no version", None, [], version=False, next_update=False, crl_exts=None)
    one("an empty value", [], [])
    one("an empty value and nothing behind it", [], [], crl_exts=None)
    for n in (1, 63, 64, 65, 255, 256, 257, 1025):
        ss = [serial_of(k, 16 + k % 2) for k in range(n)]
        one("%d entries" % n, [entry(s, ext=REASON if k % 8 == 0 else None) for k, s in enumerate(ss)], ss)
    ss = [serial_of(L, L) for L in range(46)] * 2
    one("serial lengths 0 to 45 cycling", [entry(s) for s in ss], ss)
    ss = [b"\x41" * 40, b"\x42" * 41, b"\x43" * 40, b"\x42" * 41, b"\x44" * 41, b"", b"\x00", b"\x00\x80", b"\xff" * 20]
    one("40 next to 41, a repeat above 40, a leading 00, a negative", [entry(s) for s in ss], ss)
    ss = [serial_of(k, 9) for k in range(12)]
    one("GeneralizedTime and UTCTime, with and without extensions",
        [entry(s, GEN if k % 2 else UTC, 0x18 if k % 2 else 0x17, REASON if k % 3 == 0 else None) for k, s in enumerate(ss)], ss,
        this_tag=0x18)
    for total in (126, 127, 128, 129, 254, 255, 256, 257, 258, 259, 260):          # the entry's contents cross 127/128 and 255/256
        ss = [serial_of(1, 3), serial_of(2, 3), serial_of(3, 3)]
        es = [entry(ss[0]), tlv(0x30, tlv(0x02, ss[1]) + tlv(0x17, UTC) + ext_of(total - 5 - 15)), entry(ss[2])]
        assert len(es[1]) - {True: 2, False: 3 if total < 256 else 4}[total < 128] == total
        one("an entry of %d content octets" % total, es, ss)
    for pad in range(0, 200):                                                      # the tbsCertList at its length-form boundaries
        c = crl([entry(b"\x05")], tbs_pad=pad)
        if tbs_octets(c) in (126, 127, 128, 129, 254, 255, 256, 257):
            one("a tbsCertList of %d octets" % tbs_octets(c), [entry(b"\x05")], [b"\x05"], tbs_pad=pad)
    ss = [serial_of(k, 16 + k % 2) for k in range(9)]
    for n in (65535, 65536, (1 << 24) - 1, 1 << 24):                               # … 82 ff ff / 83 01 00 00, 83 ff ff ff / 84 01 00 00 00:
        es = [entry(s, ext=REASON if k % 4 == 0 else None) for k, s in enumerate(ss)]   # grown through an extension of the CRL, which is not read
        fill = n - tbs_octets(crl(es, crl_exts=big_extension(0)))
        for k in range(fill, fill - 16, -1):
            if tbs_octets(crl(es, crl_exts=big_extension(k))) == n:
                break
        else:
            raise AssertionError(n)
        one("a tbsCertList of %d octets" % n, es, ss, crl_exts=big_extension(k))
    a = [serial_of(k, 16) for k in range(7)]
    b = [serial_of(50 + k, 17) for k in range(5)]
    c = [serial_of(90 + k, 20) for k in range(4)]
    out.append(("three shards of one issuer interleaved with another's",
                [crl([entry(s) for s in a[:3]]), crl([entry(s) for s in b[:2]]), crl([entry(s) for s in a[3:4]]), crl([entry(s) for s in b[2:]]),
                 crl([entry(s) for s in a[4:]]), crl(None), crl([entry(s) for s in c])],
                [D[1], D[2], D[1], D[2], D[1], D[3], D[4]], [a[:3], b[:2], a[3:4], b[2:], a[4:], [], c]))
    return out


def reversed_pair():
    """Two digests whose Issuer.ID order is the reverse of their digest order: the ID of the first starts with 'A', that
    of the second with '0', which base64 counts later and ASCII sorts earlier."""
    return b"\x00" * 32, b"\xd0" + b"\x00" * 31


# ---- fake entries: a well-formed entry where none starts

SMALLEST = bytes.fromhex("300402001700")           # SEQUENCE { INTEGER of no octets, UTCTime of none }


def spec_entry(serial, ext_body=None):
    return tlv(0x30, tlv(0x02, serial) + tlv(0x17, UTC) + (tlv(0x30, ext_body) if ext_body is not None else b""))


def with_fake(spec, h, j, in_ext=False, pre=b"\x59", post=b"\x55", delta=0):
    """spec: [[serial, extension body or None]].  The serial (in_ext: the extension body) of entry h becomes pre + the four
    to eight header octets 30 L 02 S of a fake entry + post, with L and S such that the fake's INTEGER runs up to the date
    of entry j >= h (h itself only with the fake in its serial), that date is the fake's Time, and the fake ends where
    entry j ends (delta: L is that much larger).  → (the new spec, where the fake starts in the value, where it ends)"""
    for nl in (1, 2, 3):
        for ns in (1, 2, 3):
            ph = b"\0" * (2 + nl + ns)
            s = [list(x) for x in spec]
            s[h][1 if in_ext else 0] = pre + ph + post
            es = [spec_entry(*x) for x in s]
            start = sum(len(e) for e in es[:h]) + es[h].index(pre + ph + post) + len(pre)
            ej = sum(len(e) for e in es[:j])
            date = ej + (len(es[j]) - len(tlv(0x02, s[j][0]) + tlv(0x17, UTC)) - (len(tlv(0x30, s[j][1])) if s[j][1] is not None else 0)) + len(tlv(0x02, s[j][0]))
            end = ej + len(es[j])
            S, L = date - (start + len(ph)), end - (start + 1 + nl)
            if S < 0:
                continue
            hdr = b"\x30" + length(L + delta) + b"\x02" + length(S)
            if len(hdr) == len(ph) and len(length(L)) == nl:
                s[h][1 if in_ext else 0] = pre + hdr + post
                v = b"".join(spec_entry(*x) for x in s)
                assert v[date] == 0x17 and v[start] == 0x30
                return s, start, end + delta
    raise AssertionError("no header fits")


def fake_cases():
    """[(name, spec, where the fake starts in the value, where it ends or None when it is no candidate)]; the serials of
    a spec are [x[0] for x in spec]."""
    base = [[serial_of(k, 5 + k % 3), (REASON[2:] if k % 4 == 1 else None)] for k in range(8)]
    long = [[serial_of(k, 16 + k % 2), None] for k in range(60)]                     # > 1024 octets: a region over tile edges
    out = []

    def add(nm, got, candidate=True):
        s, start, end = got
        out.append((nm, s, start, end if candidate else None))

    def whole(nm, h, in_ext, pre, post):
        s = [list(x) for x in base]
        s[h][1 if in_ext else 0] = pre + SMALLEST + post
        v = [spec_entry(*x) for x in s]
        start = sum(len(e) for e in v[:h]) + v[h].index(pre + SMALLEST + post) + len(pre)
        out.append((nm, s, start, start + 6))

    whole("in a serial, ends inside the true entry", 2, False, b"\x59\x58", b"\x97")
    whole("in an extension body, ends inside the true entry", 1, True, b"\xc5", b"\xc5\xc5")
    whole("in an extension body, ends at the true entry's end", 1, True, b"\xc5\xc5", b"")
    whole("the first bytes of a serial", 3, False, b"", b"\x97")
    whole("the first bytes of an extension body", 5, True, b"", b"\xc5")
    add("in a serial, ends at the true entry's end", with_fake(base, 2, 2))
    add("in a serial, ends at the end of an entry with an extension", with_fake(base, 1, 1))
    add("in a serial, ends entries later", with_fake(base, 2, 5))
    add("in an extension body, ends entries later", with_fake(base, 1, 4, in_ext=True))
    add("in a serial, ends at hi", with_fake(base, 3, 7))
    add("in an extension body, ends at hi", with_fake(base, 5, 7, in_ext=True))
    add("in a serial, ends one past hi", with_fake(base, 3, 7, delta=1), candidate=False)
    add("in the first serial of the value, its first bytes", with_fake(base, 0, 3, pre=b""))
    two, _, _ = with_fake(base, 4, 6)
    add("overlaps another fake entry", with_fake(two, 2, 5))
    add("a region over tile edges", with_fake(long, 1, 58))
    both, _, _ = with_fake(long, 30, 59, pre=b"\x58\x97\x96")
    add("two regions over tile edges, overlapping", with_fake(both, 2, 40))
    return out


def fake_crl_inside():
    """A whole CRL inside crlExtensions and inside the signature: those bytes are not read.  → [(name, CRL, serials)]"""
    ss = [serial_of(k, 12) for k in range(5)]
    inner = crl([entry(serial_of(70 + k, 8)) for k in range(9)])
    return [("a whole CRL inside crlExtensions", crl([entry(s) for s in ss], crl_exts=inner), ss),
            ("a whole CRL inside the signature", crl([entry(s) for s in ss], sig=b"\x00" + inner), ss),
            ("entries inside the issuer", crl([entry(s) for s in ss], issuer=tlv(0x30, b"".join(entry(serial_of(k, 4)) for k in range(3)))), ss)]


# ---- rejections: [(name, CRL bytes, the offset in it at which the grammar is left)]

HEAD_NODES = ("crl", "tbs", "version", "signature", "issuer", "this", "next", "revoked", "exts", "sigalg", "sig")
ENTRY_NODES = ("entry1", "serial1", "date1", "ext1")


def tree(bad=None, tags=None, extra=None, more=None, drop=None):
    """A small CRL as a tree of named nodes.  bad = (node, length form); tags = {node: tag}; extra = (node, bytes): bytes
    appended to that node's contents; more = (node, [nodes]): nodes appended to it; drop: a node left out."""
    tags = tags or {}

    def N(nm, tag, kids):
        kids = [k for k in kids if k[0] != drop] if not isinstance(kids, bytes) else kids
        if extra and extra[0] == nm:
            kids = kids + extra[1] if isinstance(kids, bytes) else kids + [extra[1]]
        if more and more[0] == nm:
            kids = kids + list(more[1])
        return (nm, tags.get(nm, tag), kids, bad[1] if bad and bad[0] == nm else None)

    ents = []
    for i in range(3):
        kids = [N("serial%d" % i, 0x02, serial_of(i, 4)), N("date%d" % i, 0x17, UTC)]
        if i == 1:
            kids.append(N("ext%d" % i, 0x30, REASON[2:]))
        ents.append(N("entry%d" % i, 0x30, kids))
    tbs = N("tbs", 0x30, [N("version", 0x02, b"\x01"), N("signature", 0x30, SIGALG[2:]), N("issuer", 0x30, ISSUER[2:]), N("this", 0x17, UTC),
                          N("next", 0x17, UTC), N("revoked", 0x30, ents), N("exts", 0xa0, CRL_NUMBER)])
    return N("crl", 0x30, [tbs, N("sigalg", 0x30, SIGALG[2:]), N("sig", 0x03, SIG)])


def small_crl():
    return enc(tree())[0]


SMALL_SERIALS = [serial_of(i, 4) for i in range(3)]


def rejections():
    out = []
    good, marks = enc(tree())
    at = dict(marks)
    sizes = {}

    def blame(nm, marks):
        return dict(marks)["entry1" if nm in ENTRY_NODES else nm]

    for nm in HEAD_NODES + ENTRY_NODES:
        # its contents' length: from a build with the five-octet form, which states it
        b85, m85 = enc(tree(bad=(nm, "85")))
        n = int.from_bytes(b85[dict(m85)[nm] + 2:dict(m85)[nm] + 7], "big")
        sizes[nm] = n
        for form in non_minimal_forms(n):
            b, m = enc(tree(bad=(nm, form)))
            out.append(("length of %s in the form %s" % (nm, form), b, blame(nm, m)))
        wrong = {"crl": 0x31, "tbs": 0x31, "version": 0x04, "signature": 0x31, "issuer": 0x31, "this": 0x16, "next": 0x04, "revoked": 0x31,
                 "exts": 0xa1, "sigalg": 0x31, "sig": 0x04, "entry1": 0x31, "serial1": 0x0a, "date1": 0x19, "ext1": 0x31}[nm]
        b, m = enc(tree(tags={nm: wrong}))
        out.append(("tag %02x for %s" % (wrong, nm), b, blame(nm, m)))
    assert sizes["crl"] >= 128 and sizes["serial1"] == 4
    out.append(("a byte behind the CertificateList", good + b"\x00", len(good)))
    b, m = enc(tree(more=("crl", [("extra", 0x05, b"", None)])))
    out.append(("a TLV behind the signatureValue", b, dict(m)["extra"]))
    b, m = enc(tree(more=("tbs", [("extra", 0x05, b"", None)])))
    out.append(("a TLV behind crlExtensions", b, dict(m)["extra"]))
    b, m = enc(tree(extra=("tbs", b"\x00")))
    out.append(("a byte behind crlExtensions", b, dict(m)["sigalg"] - 1))
    b, m = enc(tree(extra=("revoked", b"\x00")))
    out.append(("a byte behind the last entry", b, dict(m)["exts"] - 1))
    b, m = enc(tree(more=("entry1", [("extra", 0x05, b"", None)])))
    out.append(("a fourth TLV in an entry", b, dict(m)["entry1"]))
    b, m = enc(tree(more=("entry2", [("x", 0x30, b"", None), ("y", 0x30, b"", None)])))
    out.append(("two SEQUENCEs behind the date", b, dict(m)["entry2"]))
    for d in (-1, 1):
        for nm in ("entry0", "entry1", "entry2"):
            b, m = enc(tree(bad=(nm, ("delta", d))))
            out.append(("%s one byte %s" % (nm, "short" if d < 0 else "long"), b, dict(m)[nm]))
    b, m = enc(tree(bad=("serial1", ("delta", 200))))
    out.append(("a serial that runs past its entry", b, dict(m)["entry1"]))
    b, m = enc(tree(bad=("revoked", ("delta", 1))))
    out.append(("revokedCertificates one byte long", b, dict(m)["exts"] + 1))     # the TLV behind it starts inside crlExtensions
    b, m = enc(tree(bad=("revoked", ("delta", -1))))                 # the TLV behind it starts with the last entry's last octet
    out.append(("revokedCertificates one byte short", b, dict(m)["exts"] - 1))
    b, m = enc(tree(bad=("tbs", ("delta", 1))))
    out.append(("tbsCertList one byte long", b, dict(m)["sigalg"]))
    # a required one missing: the TLV behind it is taken for it where the tag allows, and the next one is blamed
    for nm, blamed in (("signature", "this"), ("issuer", "this"), ("sigalg", "sig")):
        b, m = enc(tree(drop=nm))
        out.append(("no %s" % nm, b, dict(m)[blamed]))
    b, m = enc(tree(drop="sig"))
    out.append(("no signatureValue", b, len(b)))
    b, m = enc(tree(drop="this"))                                    # nextUpdate is taken for thisUpdate: inside the grammar
    assert b != good
    out.append(("a time for the issuer", enc(tree(tags={"issuer": 0x17}))[0], at["issuer"]))
    b, m = enc(_third_time())
    out.append(("a third Time", b, dict(m)["third"]))
    return out


def _third_time():
    t = tree()
    nm, tag, kids, form = t
    tbs = list(kids[0][2])
    tbs.insert(5, ("third", 0x17, UTC, None))
    return (nm, tag, [(kids[0][0], kids[0][1], tbs, None)] + list(kids[1:]), form)
