"""DER CertificateLists → a probe image without a GPU (include/ctmr.h ctmr_crl_probes): the CPU twin of
`Engine.crl_probes`, written from the grammar in the header and independent of the device code.

`entries(crl)` is the sequential parse of one CRL — the revoked serials in order, raw octets — and raises `CrlError`
with the byte offset for anything outside the grammar.  `probes_image(crls, digests)` is the image the library writes
for the same CRLs, byte for byte: one set per issuer digest under exp hour 0, its member records in input order, the
serials above 40 octets as sorted host-section pairs.  `known_image.find(known, probes_image(...), now)` then says under
which expDates the revoked serials are known.  `probes_each(crls, digests)` is the twin of `Engine.crl_probes_each`
(DESIGN.md §27): every CRL judged on its own, a verdict per CRL, the image of the good ones.  Pure Python + numpy.
"""
import struct

import numpy as np

from . import known_image as KI

MAX_LEN = (1 << 32) - 64
NONE = (1 << 64) - 1
TIME_TAGS = (0x17, 0x18)
INFO_FIELDS = ("crls", "entries", "records", "host_members", "empty_crls", "bad_crl", "bad_offset")


class CrlError(ValueError):
    """A CRL is outside the grammar: the library refuses the call with CTMR_E_INVAL.  `crl` is the CRL's index in the
    call (0 for `entries`), `offset` the byte offset — in the CRL for `entries` and `head`, in the blob for the rest."""

    def __init__(self, offset, what, crl=0):
        super().__init__("CRL %d, offset %d: %s" % (crl, offset, what))
        self.crl, self.offset, self.what = crl, offset, what


def _length(b, p, end):
    """The length octets at b[p] inside [.., end) → (where the contents start, where they end), or None: definite,
    minimal, the contents inside `end`."""
    if p >= end:
        return None
    first = b[p]
    if first < 0x80:
        body, v = p + 1, first
    else:
        nb = first - 0x80
        if not 1 <= nb <= 4 or p + nb >= end:
            return None
        v = int.from_bytes(b[p + 1:p + 1 + nb], "big")
        if v < (0x80 if nb == 1 else 1 << 8 * (nb - 1)):
            return None
        body = p + 1 + nb
    return (body, body + v) if body + v <= end else None


def _tlv(b, p, end):
    """→ (tag, contents start, end of the TLV) of the TLV at b[p] inside [.., end), or None."""
    if p >= end:
        return None
    ln = _length(b, p + 1, end)
    return None if ln is None else (b[p], ln[0], ln[1])


def head(crl):
    """The outer TLVs of one CRL → (lo, hi): the bounds of the revokedCertificates value; lo == hi when it is absent or
    empty.  Raises CrlError at the first TLV that is not what the grammar wants there."""
    b, e = bytes(crl), len(crl)

    def want(p, end, tags, what):
        t = _tlv(b, p, end)
        if t is None or t[0] not in tags:
            raise CrlError(p, what)
        return t

    _, body, nxt = want(0, e, (0x30,), "no CertificateList SEQUENCE with a definite minimal length inside the slice")
    if nxt != e:
        raise CrlError(nxt, "bytes behind the CertificateList")
    _, p, tbs = want(body, e, (0x30,), "no tbsCertList SEQUENCE")
    t = _tlv(b, p, tbs)
    if t is not None and t[0] == 0x02:                                     # version
        p = t[2]
    p = want(p, tbs, (0x30,), "no signature AlgorithmIdentifier")[2]
    p = want(p, tbs, (0x30,), "no issuer Name")[2]
    p = want(p, tbs, TIME_TAGS, "no thisUpdate Time")[2]
    lo = hi = p
    if p < tbs:
        t = want(p, tbs, range(256), "no TLV inside tbsCertList")
        if t[0] in TIME_TAGS:                                              # nextUpdate
            lo = hi = p = t[2]
            t = want(p, tbs, range(256), "no TLV inside tbsCertList") if p < tbs else None
        if t is not None and t[0] == 0x30:                                 # revokedCertificates
            lo, hi, p = t[1], t[2], t[2]
            t = want(p, tbs, range(256), "no TLV inside tbsCertList") if p < tbs else None
        if t is not None and t[0] == 0xA0:                                 # crlExtensions
            p = t[2]
        if p != tbs:
            raise CrlError(p, "not what tbsCertList holds here")
    p = want(tbs, e, (0x30,), "no signatureAlgorithm")[2]
    p = want(p, e, (0x03,), "no signatureValue BIT STRING")[2]
    if p != e:
        raise CrlError(p, "bytes behind the signatureValue")
    return lo, hi


def entry(b, i, hi):
    """The entry at b[i] inside a value that ends at hi → (its end, its serial), or None when there is none."""
    if b[i] != 0x30:
        return None
    ln = _length(b, i + 1, hi)
    if ln is None:
        return None
    p, end = ln
    serial = _tlv(b, p, end)
    if serial is None or serial[0] != 0x02:
        return None
    date = _tlv(b, serial[2], end)
    if date is None or date[0] not in TIME_TAGS:
        return None
    if date[2] != end:
        ext = _tlv(b, date[2], end)
        if ext is None or ext[0] != 0x30 or ext[2] != end:
            return None
    return end, b[serial[1]:serial[2]]


def entries(crl):
    """The revoked serials of one CRL, in order, as raw content octets (a leading 00 stays)."""
    b = bytes(crl)
    if not b:
        raise CrlError(0, "a CRL of 0 bytes")
    lo, hi = head(b)
    out, p = [], lo
    while p < hi:
        got = entry(b, p, hi)
        if got is None:
            raise CrlError(p, "not SEQUENCE { INTEGER, Time, optional SEQUENCE } filled exactly inside revokedCertificates")
        out.append(got[1])
        p = got[0]
    return out


def check_offsets(offsets, n_crls, length):
    """What the library says of the offsets before it reads a byte: None, or (bad_crl, bad_offset)."""
    if offsets[0] != 0:
        return 0, 0
    for k in range(n_crls):
        if offsets[k + 1] < offsets[k]:
            return k, offsets[k]
    if offsets[n_crls] != length:
        return n_crls, length
    return None


def probes_parts(crls, digests):
    """→ (image bytes, info dict as ctmr_crl_info has it) of the CRLs `crls` (a list of bytes) whose issuers' SPKI
    digests are `digests` (32 bytes each).  Raises CrlError naming the lowest CRL outside the grammar and the offset in
    the concatenation of the CRLs."""
    crls, digests = [bytes(c) for c in crls], [bytes(d) for d in digests]
    if len(crls) != len(digests) or any(len(d) != 32 for d in digests):
        raise ValueError("one 32-byte digest per CRL")
    if sum(len(c) for c in crls) >= MAX_LEN:
        raise ValueError("2^32 - 64 bytes or more")
    by_digest, pairs, at, n_entries, empty = {}, set(), 0, 0, 0
    for k, (c, d) in enumerate(zip(crls, digests)):
        try:
            serials = entries(c)
        except CrlError as x:
            raise CrlError(at + x.offset, x.what, k) from None
        at += len(c)
        n_entries += len(serials)
        empty += not serials
        for s in serials:
            if len(s) <= KI.MAX_SERIAL:
                by_digest.setdefault(d, []).append(s)
            else:
                pairs.add((KI.set_key(0, d), s))
    issuers = sorted(by_digest)
    ordinal = {d: i for i, d in enumerate(issuers)}
    set_part, members, first = [], [], 0
    for d in sorted(issuers, key=KI.issuer_id):
        set_part.append(KI._SET.pack(0, ordinal[d], first, len(by_digest[d])))
        members += by_digest[d]
        first += len(by_digest[d])
    host = sorted(pairs)
    host_part = b"".join(struct.pack("<I", len(k)) + k + struct.pack("<I", len(m)) + m for k, m in host)
    meta = KI._HEADER.pack(KI.MAGIC, KI.VERSION, KI.HEADER_BYTES, len(issuers), 0, len(issuers), first, len(host_part), len(host), 0)
    meta += b"".join(issuers) + b"".join(set_part) + host_part
    meta += b"\0" * (-len(meta) % 64)
    rec = np.zeros(first, KI.MEMBER_DTYPE)
    for i, m in enumerate(members):
        rec["len"][i] = len(m)
        rec["serial"][i, :len(m)] = np.frombuffer(m, np.uint8)
    info = dict(crls=len(crls), entries=n_entries, records=first, host_members=len(host), empty_crls=empty, bad_crl=NONE, bad_offset=NONE)
    return meta + rec.tobytes(), info


def probes_image(crls, digests) -> bytes:
    """The probe image of the CRLs: what Engine.crl_probes writes, byte for byte."""
    return probes_parts(crls, digests)[0]


def probes_each(crls, digests):
    """Every CRL judged on its own (include/ctmr.h ctmr_crl_probes_each) → (image bytes, info dict,
    verdicts): verdicts[k] = (bad_offset, records, long_entries) as ctmr_crl_verdict has them — bad_offset NONE for a CRL
    inside the grammar, else the offset in the concatenation of the CRLs at which `entries` leaves it.  The image is
    probes_parts of the good CRLs with their digests; the info counts those, `crls` all, and bad_crl / bad_offset name
    the lowest bad CRL.  Nothing raises for a CRL's contents."""
    crls, digests = [bytes(c) for c in crls], [bytes(d) for d in digests]
    if len(crls) != len(digests) or any(len(d) != 32 for d in digests):
        raise ValueError("one 32-byte digest per CRL")
    if sum(len(c) for c in crls) >= MAX_LEN:
        raise ValueError("2^32 - 64 bytes or more")
    verdicts, good, at = [], [], 0
    for k, c in enumerate(crls):
        try:
            serials = entries(c)
            short = sum(len(s) <= KI.MAX_SERIAL for s in serials)
            verdicts.append((NONE, short, len(serials) - short))
            good.append(k)
        except CrlError as x:
            verdicts.append((at + x.offset, 0, 0))
        at += len(c)
    image, info = probes_parts([crls[k] for k in good], [digests[k] for k in good])
    info["crls"] = len(crls)
    bad = [k for k, v in enumerate(verdicts) if v[0] != NONE]
    if bad:
        info["bad_crl"], info["bad_offset"] = bad[0], verdicts[bad[0]][0]
    return image, info, verdicts
