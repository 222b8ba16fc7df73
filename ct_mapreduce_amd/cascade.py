"""The CRLite filter cascade of a revoked / not-revoked image pair without a GPU (include/ctmr.h ctmr_cascade_*, DESIGN.md
§29): the CPU twin of Engine.cascade_build / cascade_query, byte for byte, in plain code over known_image's section
layout and hashlib.

A cascade is a stack of Bloom filter layers.  Layer 1 holds every member record of the sets of R kept at `now`; the kept
records of S that pass it are its false positives, which layer 2 holds; the records of R that pass layer 2 go to layer
3, and so on until a layer has no false positive.  The key of a record is its issuer's 32-byte digest followed by its
serial octets; hash function i of layer `level` of m bits is u32le(SHA-256(salt ‖ u32le(i) ‖ u8(level) ‖ key)[0:4]) mod m.
Compatibility with filtercascade / rust-cascade is unpinned (neither is available to this project).

Format CTMRCASC v1 (little-endian): a 64-byte header, one 32-byte layer record per layer, then each layer's bits at the
next multiple of 64 bytes; bit b is byte b >> 3, mask 1 << (b & 7).
"""
import math
import struct
from dataclasses import dataclass
from hashlib import sha256

import numpy as np

from . import known_image as KI

MAGIC = b"CTMRCASC"
VERSION = 1
HASH_SHA256_32 = 2
HEADER_BYTES = 64
LAYER_BYTES = 32
MAX_LAYERS = 255
_HEADER = struct.Struct("<8sIIII16sQQQ")
_LAYER = struct.Struct("<IIQQQ")


class CascadeError(ValueError):
    """What the library refuses with CTMR_E_INVAL: parameters out of range, a layer of 2^32 bits or more, a build that
    max_layers layers do not finish (`left`: the false positives of the last layer), a damaged cascade."""

    def __init__(self, msg, left=0):
        super().__init__(msg)
        self.left = left


@dataclass
class Params:
    k_first: int
    bpk_first_q8: int
    k_rest: int
    bpk_rest_q8: int
    max_layers: int
    salt: bytes = b""

    def check(self):
        ks, bs = (self.k_first, self.k_rest), (self.bpk_first_q8, self.bpk_rest_q8)
        if not (all(1 <= k <= 32 for k in ks) and all(1 <= b <= 65536 for b in bs) and 1 <= self.max_layers <= MAX_LAYERS
                and len(self.salt) <= 16):
            raise CascadeError("k in 1..32, bpk_q8 in 1..65536, max_layers in 1..255, salt_len in 0..16")


def crlite_params(n_revoked, n_known, salt=b"", max_layers=64) -> Params:
    """CRLite's usual choice for n_revoked records in R and n_known in S: a first layer with a false-positive rate of
    p = n_revoked / (√2 · n_known), at most ½, so k = ceil(log2(1 / p)) hash functions (at most 32) and 370/256 ≈ 1 / ln 2
    bits per record and hash function; one hash function and 370/256 bits per record in every other layer.  The only
    float arithmetic of the cascade: what it hands over are integers."""
    p = 0.5 if n_known <= 0 or n_revoked <= 0 else min(0.5, n_revoked / (math.sqrt(2.0) * n_known))
    k = min(32, max(1, math.ceil(math.log2(1.0 / p))))
    return Params(k, 370 * k, 1, 370, max_layers, bytes(salt))


def layer_bits(n, bpk_q8):
    """The bits of a layer that holds n records: integer arithmetic only."""
    return max(1, (n * bpk_q8 + 255) // 256)


def layer_shape(n, level, params):
    """(k, m) of layer `level` when it holds n records; raises CascadeError for a layer of 2^32 bits or more."""
    k, bpk = (params.k_first, params.bpk_first_q8) if level == 1 else (params.k_rest, params.bpk_rest_q8)
    m = layer_bits(n, bpk)
    if m >= 2 ** 32:
        raise CascadeError("layer %d would have %d bits, at most 2^32 - 1" % (level, m))
    return k, m


def _hash(prefix, key, m):
    return int.from_bytes(sha256(prefix + key).digest()[:4], "little") % m


def _prefixes(salt, level, k):
    return [salt + struct.pack("<IB", i, level) for i in range(k)]


def _keys(image, now):
    """→ (the keys of the member records of the sets of `image` kept at `now` in image order — now None: of all sets —,
    the host-section pairs under keys kept at `now`, all host-section pairs).  The meta part is held to the checks of
    the library; of the member records only those of kept sets are read and validated."""
    b = bytes(image)
    if len(b) < KI.HEADER_BYTES:
        raise KI.ImageError("shorter than its header")
    magic, version, hdr, n_iss, flags, n_sets, n_mem, host_bytes, n_host, reserved = KI._HEADER.unpack_from(b, 0)
    if magic != KI.MAGIC or version != KI.VERSION or hdr != KI.HEADER_BYTES or flags or reserved:
        raise KI.ImageError("bad magic, version, header size, flags or reserved field")
    content = KI.HEADER_BYTES + 32 * n_iss + KI.SET_BYTES * n_sets + host_bytes
    meta = (content + 63) & ~63
    if meta + n_mem * KI.MEMBER_BYTES != len(b) or any(b[content:meta]):
        raise KI.ImageError("%d bytes, the header says %d, or padding that is not zero" % (len(b), meta + n_mem * KI.MEMBER_BYTES))
    rec = np.frombuffer(b, KI.MEMBER_DTYPE, count=n_mem, offset=meta)
    so = KI.HEADER_BYTES + 32 * n_iss
    keys, at = [], 0
    for s in range(n_sets):
        eh, ordinal, first, count = KI._SET.unpack_from(b, so + KI.SET_BYTES * s)
        if ordinal >= n_iss or first != at or count == 0 or count > n_mem - at:
            raise KI.ImageError("set %d names an issuer the image lacks or does not follow its predecessor" % s)
        at += count
        if now is not None and not (KI._HOUR_LO <= eh < KI._HOUR_HI and now < (eh + 1) * 3600):
            continue
        r = rec[first:first + count]
        lens = r["len"]
        if (lens > KI.MAX_SERIAL).any():
            raise KI.ImageError("a member record's serial_len is above %d" % KI.MAX_SERIAL)
        if r["serial"][np.arange(KI.MAX_SERIAL)[None, :] >= lens[:, None].astype(np.int64)].any():
            raise KI.ImageError("a member record's padding octets are not zero")
        dg = b[KI.HEADER_BYTES + 32 * ordinal:KI.HEADER_BYTES + 32 * (ordinal + 1)]
        raw = r["serial"].tobytes()
        keys += [dg + raw[40 * i:40 * i + int(n)] for i, n in enumerate(lens)]
    if at != n_mem:
        raise KI.ImageError("the sets cover %d of %d members" % (at, n_mem))
    h, q, kept, pairs = so + KI.SET_BYTES * n_sets, 0, 0, 0
    while q < host_bytes:
        if host_bytes - q < 8:
            raise KI.ImageError("host section truncated")
        (kl,) = struct.unpack_from("<I", b, h + q)
        key = b[h + q + 4:h + q + 4 + kl]
        q += 4 + kl
        if host_bytes - q < 4:
            raise KI.ImageError("host section truncated")
        (ml,) = struct.unpack_from("<I", b, h + q)
        q += 4 + ml
        if q > host_bytes:
            raise KI.ImageError("host section truncated")
        pairs += 1
        if now is not None:
            parts = key.split(b"::")
            if len(parts) != 3:
                raise KI.ListsError("unexpected key format: %r" % key)
            span = KI.exp_date_span(parts[1])
            kept += span is not None and now < span[1]
    if pairs != n_host:
        raise KI.ImageError("host section holds %d members, the header says %d" % (pairs, n_host))
    return keys, kept, pairs


def build_info(revoked, known, now, params):
    """→ (the cascade, info): info as Engine.cascade_build gives it, without `syncs`."""
    params.check()
    salt = bytes(params.salt)
    r_keys, r_host, _ = _keys(revoked, now)
    s_keys, s_host, _ = _keys(known, now)
    hold, test = r_keys, s_keys
    layers = []   # (level, k, m, n_held, bits)
    while hold:
        level = len(layers) + 1
        k, m = layer_shape(len(hold), level, params)
        bits = bytearray(((m + 7) // 8 + 63) & ~63)
        pre = _prefixes(salt, level, k)
        for key in hold:
            for p in pre:
                bit = _hash(p, key, m)
                bits[bit >> 3] |= 1 << (bit & 7)
        layers.append((level, k, m, len(hold), bits))
        passed = []
        for key in test:
            for p in pre:
                bit = _hash(p, key, m)
                if not bits[bit >> 3] >> (bit & 7) & 1:
                    break
            else:
                passed.append(key)
        if not passed:
            break
        if level == params.max_layers:
            raise CascadeError("%d records left after %d layers" % (len(passed), level), left=len(passed))
        hold, test = passed, hold
    at = head = (HEADER_BYTES + LAYER_BYTES * len(layers) + 63) & ~63
    table = []
    for level, k, m, n_held, bits in layers:
        table.append((level, k, m, at, n_held))
        at += len(bits)
    out = _HEADER.pack(MAGIC, VERSION, HASH_SHA256_32, len(layers), len(salt), salt.ljust(16, b"\0"), at, len(r_keys), len(s_keys))
    out += b"".join(_LAYER.pack(*t) for t in table)
    out = out.ljust(head, b"\0") + b"".join(bytes(l[4]) for l in layers)
    info = dict(bytes=at, layers=len(layers), r_records=len(r_keys), s_records=len(s_keys), r_host_skipped=r_host,
                s_host_skipped=s_host, left=0, layer=table)
    return out, info


def build(revoked, known, now, params) -> bytes:
    """Engine.cascade_build(revoked, known, now, params) without a GPU → the cascade.  Raises CascadeError for what the
    library refuses with CTMR_E_INVAL of its own, known_image.ImageError / ListsError for a bad image."""
    return build_info(revoked, known, now, params)[0]


def parse(cascade) -> dict:
    """Validates a cascade as the query does before it launches anything → {salt, r_records, s_records, bytes, layers:
    [(level, k, m_bits, offset, n_held)]}.  Raises CascadeError."""
    b = bytes(cascade)
    if len(b) < HEADER_BYTES:
        raise CascadeError("a cascade shorter than its header")
    magic, version, alg, n, salt_len, salt, total, n_r, n_s = _HEADER.unpack_from(b, 0)
    if magic != MAGIC:
        raise CascadeError("bad magic")
    if version != VERSION:
        raise CascadeError("version %d, expected 1" % version)
    if alg != HASH_SHA256_32:
        raise CascadeError("hash algorithm %d, expected 2" % alg)
    if n > MAX_LAYERS or salt_len > 16:
        raise CascadeError("%d layers, a salt of %d octets" % (n, salt_len))
    if total != len(b):
        raise CascadeError("%d bytes, the header says %d" % (len(b), total))
    head = HEADER_BYTES + LAYER_BYTES * n
    if head > len(b):
        raise CascadeError("the layer table reaches beyond the cascade")
    layers, prev = [], 0
    for i in range(n):
        level, k, m, off, held = _LAYER.unpack_from(b, HEADER_BYTES + LAYER_BYTES * i)
        if level <= prev or level > 255:
            raise CascadeError("layer %d has level %d behind level %d" % (i, level, prev))
        if not 1 <= k <= 32 or not 1 <= m < 2 ** 32:
            raise CascadeError("layer %d has k = %d, m = %d" % (i, k, m))
        if off & 63 or off < head or off > len(b) or (m + 31) // 32 * 4 > len(b) - off:
            raise CascadeError("the bits of layer %d lie outside the cascade" % i)
        prev = level
        layers.append((level, k, m, off, held))
    return dict(salt=salt[:salt_len], r_records=n_r, s_records=n_s, bytes=total, layers=layers)


def query_keys(cascade, keys) -> bytes:
    """One byte per key (issuer digest ‖ serial): 1 = the cascade says revoked.  A key that fails layer j + 1 after
    passing j layers is revoked iff j is odd; one that passes every layer iff the layer count is odd."""
    c = parse(cascade)
    b = bytes(cascade)
    pre = [_prefixes(c["salt"], level, k) for level, k, _, _, _ in c["layers"]]
    out = bytearray(len(keys))
    for at, key in enumerate(keys):
        passed = 0
        for (_, _, m, off, _), ps in zip(c["layers"], pre):
            for p in ps:
                bit = _hash(p, key, m)
                if not b[off + (bit >> 3)] >> (bit & 7) & 1:
                    break
            else:
                passed += 1
                continue
            break
        out[at] = passed & 1
    return bytes(out)


def query(cascade, probes) -> bytes:
    """Engine.cascade_query(cascade, probes) without a GPU: one byte per member record of the image `probes`, all sets,
    in record order.  Its host section is not answered."""
    parse(cascade)
    return query_keys(cascade, _keys(probes, None)[0])
