"""The known-certificate image (include/ctmr.h) without a GPU: parse, write, and convert to and from the
Redis protocol stream of remote_cache.redis_dump.

An image is what `Engine.known_export` writes and `Engine.known_import` reads: every serials::<expDate>::<issuerID> set
of the engine — what a restarted reference deployment still finds in its Redis.  `parse` checks exactly what the library
checks before it applies an image; `build` is the canonical writer; `sort` is the twin of `Engine.known_sort`
(every set's member records in ascending order, repeats kept); `query` / `subtract` are the twins of
`Engine.known_query` / `Engine.known_remove` over a dict of sets; `union` / `minus` / `intersect` are the twins of
`Engine.known_merge` (set algebra on images, key by key); `image_lists` is the twin of `Engine.known_image_lists`
(per-issuer lists straight from an image, in the image's order); `find` is the twin of `Engine.known_image_find`
(serials looked up whatever their expiration date) and `probes` builds its probe image; `split` is the twin of
`Engine.known_image_split` (an image partitioned by a probe image: the records that equal a probe, and the others); `image_resp` is the twin of `Engine.known_image_resp`
(the SADD + EXPIREAT stream of an image as it lies, key by key) and `resp_image` its inverse, the twin of
`Engine.known_resp_image` (a SADD / EXPIREAT stream as it lies → an image, members in stream order); `to_resp` /
`from_resp` turn an image into the SADD + EXPIREAT stream `redis_dump` writes for the same sets and back (a warm start
from a reference deployment's Redis contents).  Pure Python + numpy.
"""
import base64
import io
import struct
from dataclasses import dataclass, field

import numpy as np

MAGIC = b"CTMRKNWN"
VERSION = 1
HEADER_BYTES = 64
SET_BYTES = 24
MEMBER_BYTES = 48
MAX_SERIAL = 40
PREFIX = b"serials::"
_HEADER = struct.Struct("<8sIIIIQQQQQ")
_SET = struct.Struct("<iIQQ")
MEMBER_DTYPE = np.dtype([("len", "<u8"), ("serial", "u1", (MAX_SERIAL,))])
assert _HEADER.size == HEADER_BYTES and _SET.size == SET_BYTES and MEMBER_DTYPE.itemsize == MEMBER_BYTES


class ImageError(ValueError):
    """The image is malformed: the library refuses it with CTMR_E_INVAL."""


@dataclass
class KnownImage:
    sets: dict = field(default_factory=dict)   # key bytes → sorted list of member bytes (both sections)
    issuers: list = field(default_factory=list)  # 32-byte SPKI digests, by ordinal
    n_sets: int = 0                            # sets of the members section
    n_members: int = 0                         # member records
    n_host_members: int = 0                    # host-section members

    @property
    def total(self):
        return self.n_members + self.n_host_members


# ExpDate.ID() "2006-01-02-15" of an hour count (storage/types.go:339-384), as the library formats it
def _civil_from_days(z):
    z += 719468
    era = z // 146097          # (// floors: no adjustment for negative z, unlike C)
    doe = z - era * 146097
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
    mp = (5 * doy + 2) // 153
    d = doy - (153 * mp + 2) // 5 + 1
    m = mp + 3 if mp < 10 else mp - 9
    return yoe + era * 400 + (m <= 2), m, d


def exp_date_id(exp_hour: int) -> bytes:
    days, hh = divmod(exp_hour, 24)
    y, m, d = _civil_from_days(days)
    return b"%04d-%02d-%02d-%02d" % (y, m, d, hh)


def issuer_id(digest: bytes) -> bytes:
    """Issuer.ID: the padded base64url of the SPKI digest (storage/types.go:155-159)."""
    return base64.urlsafe_b64encode(digest)


def set_key(exp_hour: int, digest: bytes) -> bytes:
    return PREFIX + exp_date_id(exp_hour) + b"::" + issuer_id(digest)


def _days_from_civil(y, m, d):
    y -= m <= 2
    era = y // 400
    yoe = y - era * 400
    doy = (153 * (m - 3 if m > 2 else m + 9) + 2) // 5 + d - 1
    doe = yoe * 365 + yoe // 4 - yoe // 100 + doy
    return era * 146097 + doe - 719468


def parse_key(key: bytes):
    """serials::<expDate>::<Issuer.ID> → (exp_hour, digest), or None when the key is not one the members section can
    carry (then its members belong to the host section)."""
    if not key.startswith(PREFIX) or len(key) < len(PREFIX) + 13 + 2 + 1 or key[22:24] != b"::":
        return None
    date, ident = key[9:22], key[24:]
    try:
        y, mo, d, h = (int(x) for x in date.split(b"-"))
        digest = base64.urlsafe_b64decode(ident)
    except Exception:
        return None
    if len(digest) != 32 or not (1 <= mo <= 12 and 1 <= d <= 31 and 0 <= h <= 23):
        return None
    hour = _days_from_civil(y, mo, d) * 24 + h
    if not -2 ** 31 <= hour < 2 ** 31 or set_key(hour, digest) != key:
        return None
    return hour, digest


def parse(image) -> KnownImage:
    """Validates and reads an image (bytes-like): the checks the library makes before it applies one."""
    b = memoryview(bytes(image))
    if len(b) < HEADER_BYTES:
        raise ImageError("shorter than its header")
    magic, version, hdr, n_iss, flags, n_sets, n_mem, host_bytes, n_host, reserved = _HEADER.unpack_from(b, 0)
    if magic != MAGIC:
        raise ImageError("bad magic")
    if version != VERSION:
        raise ImageError("version %d, expected 1" % version)
    if hdr != HEADER_BYTES or flags or reserved:
        raise ImageError("header size, flags or reserved field")
    content = HEADER_BYTES + n_iss * 32 + n_sets * SET_BYTES + host_bytes
    meta = (content + 63) & ~63
    if meta + n_mem * MEMBER_BYTES != len(b):
        raise ImageError("%d bytes, the header says %d" % (len(b), meta + n_mem * MEMBER_BYTES))
    if any(b[content:meta]):
        raise ImageError("padding before the members is not zero")
    issuers = [bytes(b[HEADER_BYTES + 32 * k:HEADER_BYTES + 32 * (k + 1)]) for k in range(n_iss)]
    so = HEADER_BYTES + 32 * n_iss
    rec = np.frombuffer(b[meta:], MEMBER_DTYPE, count=n_mem) if n_mem else np.zeros(0, MEMBER_DTYPE)
    if n_mem:
        lens = rec["len"]
        if (lens > MAX_SERIAL).any():
            raise ImageError("a member record's serial_len is above %d" % MAX_SERIAL)
        pad = np.arange(MAX_SERIAL)[None, :] >= lens[:, None].astype(np.int64)
        if rec["serial"][pad].any():
            raise ImageError("a member record's padding octets are not zero")
    out = KnownImage(issuers=issuers, n_sets=n_sets, n_members=n_mem, n_host_members=n_host)
    at, prev = 0, None
    for s in range(n_sets):
        eh, ordinal, first, count = _SET.unpack_from(b, so + SET_BYTES * s)
        if ordinal >= n_iss:
            raise ImageError("set %d names issuer %d of %d" % (s, ordinal, n_iss))
        if first != at or count == 0 or count > n_mem - at:
            raise ImageError("set %d does not follow its predecessor (gap, overlap or empty)" % s)
        key = set_key(eh, issuers[ordinal])
        if prev is not None and not prev < key:
            raise ImageError("sets out of key order")
        prev = key
        r = rec[first:first + count]
        out.sets[key] = [bytes(m[:int(l)]) for l, m in zip(r["len"], r["serial"])]
        at += count
    if at != n_mem:
        raise ImageError("the sets cover %d of %d members" % (at, n_mem))
    h, q, hosts = so + SET_BYTES * n_sets, 0, []
    while q < host_bytes:
        if host_bytes - q < 4:
            raise ImageError("host section truncated")
        (kl,) = struct.unpack_from("<I", b, h + q)
        if host_bytes - q - 4 < kl + 4:
            raise ImageError("host section truncated")
        key = bytes(b[h + q + 4:h + q + 4 + kl])
        q += 4 + kl
        (ml,) = struct.unpack_from("<I", b, h + q)
        if host_bytes - q - 4 < ml:
            raise ImageError("host section truncated")
        mem = bytes(b[h + q + 4:h + q + 4 + ml])
        q += 4 + ml
        if not key.startswith(PREFIX):
            raise ImageError("a host-section key outside serials::")
        if hosts and not hosts[-1] < (key, mem):
            raise ImageError("host section out of (key, member) order")
        hosts.append((key, mem))
    if len(hosts) != n_host:
        raise ImageError("host section holds %d members, the header says %d" % (len(hosts), n_host))
    for key, mem in hosts:
        out.sets.setdefault(key, []).append(mem)
    for key in out.sets:
        out.sets[key] = sorted(set(out.sets[key]))
    return out


def build(sets) -> bytes:
    """The canonical image of {key: members}: members of at most 40 octets under keys that name an expDate and an issuer
    digest go to the members section (sorted), everything else to the host section; issuers in digest order."""
    dev, host = {}, []
    for key, members in sets.items():
        key = bytes(key)
        if not key.startswith(PREFIX):
            raise ValueError("not a known-certificate set: %r" % key)
        members = sorted(set(bytes(m) for m in members))
        pk = parse_key(key)
        for m in members:
            if pk is not None and len(m) <= MAX_SERIAL:
                dev.setdefault(key, (pk, []))[1].append(m)
            else:
                host.append((key, m))
    host.sort()
    keys = sorted(dev)
    digests = sorted({dev[k][0][1] for k in keys})
    ordinal = {d: i for i, d in enumerate(digests)}
    set_part, members, first = [], [], 0
    for k in keys:
        (eh, dg), ms = dev[k]
        set_part.append(_SET.pack(eh, ordinal[dg], first, len(ms)))
        members += ms
        first += len(ms)
    host_part = b"".join(struct.pack("<I", len(k)) + k + struct.pack("<I", len(m)) + m for k, m in host)
    body = b"".join(digests) + b"".join(set_part) + host_part
    head = _HEADER.pack(MAGIC, VERSION, HEADER_BYTES, len(digests), 0, len(keys), first, len(host_part), len(host), 0)
    meta = head + body
    meta += b"\0" * (-len(meta) % 64)
    rec = np.zeros(first, MEMBER_DTYPE)
    for i, m in enumerate(members):
        rec["len"][i] = len(m)
        rec["serial"][i, :len(m)] = np.frombuffer(m, np.uint8)
    return meta + rec.tobytes()


def sort(image) -> bytes:
    """The image with the member records of every set in ascending order of their serials as byte strings (a proper
    prefix first) — Engine.known_sort without a GPU (include/ctmr.h).  Repeated records stay, the meta
    part stays byte for byte; raises ImageError for what `parse` rejects."""
    parse(image)
    b = bytes(image)
    _, _, _, n_iss, _, n_sets, n_mem, _, _, _ = _HEADER.unpack_from(b, 0)
    at = len(b) - n_mem * MEMBER_BYTES
    if n_mem < 2:
        return b
    rec = np.frombuffer(b, MEMBER_DTYPE, count=n_mem, offset=at)
    so = HEADER_BYTES + 32 * n_iss
    counts = [_SET.unpack_from(b, so + SET_BYTES * s)[3] for s in range(n_sets)]
    set_of = np.repeat(np.arange(n_sets), counts)
    # the 40 padded octets as five big-endian words, then serial_len: numpy compares them as unsigned integers
    words = np.ascontiguousarray(rec["serial"]).view(">u8").astype(np.uint64)
    order = np.lexsort((rec["len"],) + tuple(words[:, k] for k in (4, 3, 2, 1, 0)) + (set_of,))
    return b[:at] + rec[order].tobytes()


# ---- bulk SetContains / SetRemove with an image as the batch (include/ctmr.h ctmr_known_query / ctmr_known_remove;
# DESIGN.md §14), without a GPU.  world = 1: which records another rank owns depends on the engine's issuer numbering.

def records(image):
    """→ ([(key, member)] per member record in image order, [(key, member)] per host-section member in section order) of
    a valid image.  `parse` merges the two sections and drops repeats; this keeps every record where it is."""
    parse(image)
    b = bytes(image)
    _, _, _, n_iss, _, n_sets, n_mem, host_bytes, n_host, _ = _HEADER.unpack_from(b, 0)
    so = HEADER_BYTES + 32 * n_iss
    rec = np.frombuffer(b, MEMBER_DTYPE, count=n_mem, offset=len(b) - n_mem * MEMBER_BYTES)
    dev = []
    for s in range(n_sets):
        eh, ordinal, first, count = _SET.unpack_from(b, so + SET_BYTES * s)
        key = set_key(eh, b[HEADER_BYTES + 32 * ordinal:HEADER_BYTES + 32 * (ordinal + 1)])
        r = rec[first:first + count]
        dev += [(key, bytes(m[:int(l)])) for l, m in zip(r["len"], r["serial"])]
    h, q, host = so + SET_BYTES * n_sets, 0, []
    while q < host_bytes:
        (kl,) = struct.unpack_from("<I", b, h + q)
        key = b[h + q + 4:h + q + 4 + kl]
        q += 4 + kl
        (ml,) = struct.unpack_from("<I", b, h + q)
        host.append((key, b[h + q + 4:h + q + 4 + ml]))
        q += 4 + ml
    return dev, host


def query(image, sets):
    """Engine.known_query(image) of an engine holding exactly `sets` ({key: members}) → (flags, host_flags): numpy uint8,
    1 where sets[key] holds the member, else 0."""
    dev, host = records(image)
    held = {bytes(k): set(bytes(m) for m in v) for k, v in sets.items()}
    return tuple(np.fromiter((m in held.get(k, ()) for k, m in part), np.uint8, len(part)) for part in (dev, host))


def subtract(sets, image) -> dict:
    """The sets an engine holding `sets` is left with by Engine.known_remove(image): members sorted, empty sets gone."""
    dev, host = records(image)
    gone = {}
    for k, m in dev + host:
        gone.setdefault(k, set()).add(m)
    out = {}
    for k, v in sets.items():
        left = sorted(set(bytes(m) for m in v) - gone.get(bytes(k), set()))
        if left:
            out[bytes(k)] = left
    return out


# ---- set algebra on images (include/ctmr.h ctmr_known_merge*), without a GPU: `build` over the algebra
# of the sets `parse` reads, key by key.  None stands for the empty image.

KNOWN_UNION, KNOWN_MINUS, KNOWN_INTERSECT = 0, 1, 2


def _sets_of(image) -> dict:
    return {} if image is None else {k: set(v) for k, v in parse(image).sets.items()}


def union(*images) -> bytes:
    """The canonical image of the union of the images' sets; union(a) normalises a (members sorted, each once, the
    host-section pairs the member section can carry moved there)."""
    out = {}
    for image in images:
        for k, v in _sets_of(image).items():
            out.setdefault(k, set()).update(v)
    return build(out)


def minus(a, b) -> bytes:
    """The canonical image of a's sets without the members b's set of the same key holds."""
    sb = _sets_of(b)
    return build({k: v - sb.get(k, set()) for k, v in _sets_of(a).items()})


def intersect(a, b) -> bytes:
    """The canonical image of the members both images hold under the same key."""
    sb = _sets_of(b)
    return build({k: v & sb.get(k, set()) for k, v in _sets_of(a).items()})


def merge(op, a, b=None) -> bytes:
    """Engine.known_merge(op, a, b) without a GPU."""
    if op not in (KNOWN_UNION, KNOWN_MINUS, KNOWN_INTERSECT):
        raise ValueError("unknown op %r" % (op,))
    return (union, minus, intersect)[op](a, b)


class _SetsCache:
    """The two RemoteCache methods redis_dump / redis_load use, over a dict of sets."""

    def __init__(self, sets=None):
        self.sets = sets if sets is not None else {}

    def KeysToChan(self, pattern):
        return iter(sorted(self.sets))        # an image holds serials:: keys only; redis_dump asks for serials::*

    def SetToChan(self, key):
        return iter(self.sets.get(bytes(key), ()))

    def SetInsert(self, key, member):
        s = self.sets.setdefault(bytes(key), set())
        new = bytes(member) not in s
        s.add(bytes(member))
        return new

    def ExpireAt(self, key, unix_seconds):
        pass                                  # the image carries the expDate of every key: EXPIREAT is implied


def to_resp(image, out) -> dict:
    """Writes the bytes redis_dump(cache, out, patterns=("serials::*",)) writes for a cache holding the image's sets."""
    from .remote_cache import redis_dump
    return redis_dump(_SetsCache(parse(image).sets), out, patterns=("serials::*",))


def from_resp(stream) -> bytes:
    """An image of the serials:: sets of a redis_dump / redis-cli style stream of SADD (and EXPIREAT) commands.  Other
    keys are skipped.  One member at a time through redis_load; `resp_image` is the strict twin of the GPU path
    (Engine.known_resp_image / known_import_resp), and union(resp_image(s)) == from_resp(s) for every stream both
    accept."""
    from .remote_cache import redis_load
    if isinstance(stream, (bytes, bytearray, memoryview)):
        stream = io.BytesIO(bytes(stream))
    c = _SetsCache()
    redis_load(c, stream)
    return build({k: v for k, v in c.sets.items() if k.startswith(PREFIX)})


# ---- per-issuer known-serial lists (include/ctmr.h ctmr_known_lists), without a GPU

class ListsError(ValueError):
    """A serials:: key that does not split into three "::" parts: the library fails with CTMR_E_INVAL."""


def exp_date_span(date: bytes):
    """NewExpDate(date) (storage/types.go): → (first second, first second at which IsExpiredAt is true), or None when it
    does not parse.  "2006-01-02-15" (one or two hour digits, as time.Parse takes them) or "2006-01-02"; four-digit
    years."""
    d = bytes(date)
    if len(d) not in (10, 12, 13) or d[4:5] != b"-" or d[7:8] != b"-":
        return None
    if not (d[0:4] + d[5:7] + d[8:10]).isdigit():
        return None
    h = None
    if len(d) > 10:
        if d[10:11] != b"-" or not d[11:].isdigit():
            return None
        h = int(d[11:])
    y, m, day = int(d[0:4]), int(d[5:7]), int(d[8:10])
    if not (1 <= m <= 12 and 1 <= day <= 31) or (h is not None and h > 23):
        return None
    days = _days_from_civil(y, m, day)
    if _civil_from_days(days) != (y, m, day):
        return None
    start = days * 86400 + (h or 0) * 3600
    return start, start + (86400 if h is None else 3600)


def list_blocks(sets, now) -> list:
    """[(Issuer.ID, [(expDate, [members])])]: the sets of {key: members} kept at `now`, grouped per Issuer.ID (bytewise
    ascending) and expDate (ascending: first second, then the date string) — GetIssuerAndDatesFromCache and
    IsExpiredAt as the library applies them.  Members keep the order they have in `sets`."""
    by_id = {}
    for key, members in sets.items():
        key = bytes(key)
        if not key.startswith(PREFIX):
            continue
        parts = key.split(b"::")
        if len(parts) != 3:
            raise ListsError("unexpected key format: %r" % key)
        span = exp_date_span(parts[1])
        if span is None or now >= span[1]:
            continue
        by_id.setdefault(parts[2], {})[(span[0], parts[1])] = list(members)
    return [(i, [(k[1], by_id[i][k]) for k in sorted(by_id[i])]) for i in sorted(by_id)]


def line(serial: bytes) -> bytes:
    """One line of a list: hex.EncodeToString(serial) + "\\n" (Serial.HexString, lowercase)."""
    return bytes(serial).hex().encode() + b"\n"


def lists_of_sets(sets, now) -> list:
    """[(Issuer.ID, text)] of {key: members}: what Engine.known_lists returns for an engine holding those sets (the
    order inside an expDate is the order of `sets`; the library's is unspecified)."""
    return [(i, b"".join(line(m) for _, ms in blocks for m in ms)) for i, blocks in list_blocks(sets, now)]


def known_lists(image, now) -> list:
    """The per-issuer known-serial lists of an image at `now`: Engine.known_lists of the engine that exported it."""
    return lists_of_sets(parse(image).sets, now)


# the hours whose ExpDate.ID has four year digits: the library lists no set record of another hour
_HOUR_LO, _HOUR_HI = _days_from_civil(0, 1, 1) * 24, _days_from_civil(10000, 1, 1) * 24


def image_lists(image, now) -> list:
    """[(Issuer.ID, text)] of an image at `now` as Engine.known_image_lists writes it (include/ctmr.h
    ctmr_known_image_lists): one line per member record in the image's order inside its set, repeats
    kept; the host-section members of a key behind the member records of the same key; expiry, grouping and order as
    in `list_blocks`.  Raises ImageError for what `parse` rejects and ListsError for a host key that does not split
    into three "::" parts."""
    parse(image)
    b = bytes(image)
    _, _, _, n_iss, _, n_sets, n_mem, _, _, _ = _HEADER.unpack_from(b, 0)
    so = HEADER_BYTES + 32 * n_iss
    rec = np.frombuffer(b, MEMBER_DTYPE, count=n_mem, offset=len(b) - n_mem * MEMBER_BYTES)
    by_id = {}
    for s in range(n_sets):
        eh, ordinal, first, count = _SET.unpack_from(b, so + SET_BYTES * s)
        if not _HOUR_LO <= eh < _HOUR_HI or now >= (eh + 1) * 3600:
            continue
        ident = issuer_id(b[HEADER_BYTES + 32 * ordinal:HEADER_BYTES + 32 * (ordinal + 1)])
        r = rec[first:first + count]
        by_id.setdefault(ident, {})[(eh * 3600, exp_date_id(eh))] = [bytes(m[:int(l)]) for l, m in zip(r["len"], r["serial"])]
    for key, member in records(image)[1]:
        parts = key.split(b"::")
        if len(parts) != 3:
            raise ListsError("unexpected key format: %r" % key)
        span = exp_date_span(parts[1])
        if span is None or now >= span[1]:
            continue
        by_id.setdefault(parts[2], {}).setdefault((span[0], parts[1]), []).append(member)
    return [(i, b"".join(line(m) for k in sorted(by_id[i]) for m in by_id[i][k])) for i in sorted(by_id)]


# ---- serials looked up in an image whatever their expiration date (include/ctmr.h ctmr_known_image_find),
# without a GPU

HIT_DTYPE = np.dtype([("records", "<u4"), ("first_hour", "<i4"), ("last_hour", "<i4"), ("reserved", "<u4")])


def probes(serials_by_digest) -> bytes:
    """The probe image of {32-byte issuer digest: [serials]}: canonical, every set under hour 0 (the hour of a probe is
    ignored), serials above 40 octets in the host section."""
    return build({set_key(0, bytes(d)): ms for d, ms in serials_by_digest.items()})


def _sections(image):
    """→ ([(exp hour or None, Issuer.ID, serial)] per member record in image order, the same per host-section member in
    section order; the hour of a host key is that of its date's first second, None when the date does not parse, with
    the second at which the key expires beside it): the two sections as `find` reads them."""
    parse(image)
    b = bytes(image)
    _, _, _, n_iss, _, n_sets, n_mem, _, _, _ = _HEADER.unpack_from(b, 0)
    so = HEADER_BYTES + 32 * n_iss
    rec = np.frombuffer(b, MEMBER_DTYPE, count=n_mem, offset=len(b) - n_mem * MEMBER_BYTES)
    dev = []
    for s in range(n_sets):
        eh, ordinal, first, count = _SET.unpack_from(b, so + SET_BYTES * s)
        ident = issuer_id(b[HEADER_BYTES + 32 * ordinal:HEADER_BYTES + 32 * (ordinal + 1)])
        r = rec[first:first + count]
        dev += [(eh, ident, bytes(m[:int(l)])) for l, m in zip(r["len"], r["serial"])]
    host = []
    for key, member in records(image)[1]:
        parts = key.split(b"::")
        if len(parts) != 3:
            raise ListsError("unexpected key format: %r" % key)
        host.append((exp_date_span(parts[1]), parts[2], member))
    return dev, host


def find(known, probes, now):
    """Engine.known_image_find(known, probes, now) without a GPU → (hits, host_hits): numpy HIT_DTYPE, one per member
    record of `probes` in image order and one per member of its host section in section order.  A probe is (Issuer.ID,
    serial); its answer counts the member records and host-section members of the sets of `known` kept at `now` under
    the same ID with the same serial, and gives the lowest and highest exp hour among them (zeros when there are none).
    Raises ImageError for what `parse` rejects and ListsError for a host key that does not split into three "::" parts,
    in either operand."""
    k_dev, k_host = _sections(known)
    p_dev, p_host = _sections(probes)
    held = {}
    for eh, ident, m in k_dev:
        if _HOUR_LO <= eh < _HOUR_HI and now < (eh + 1) * 3600:
            held.setdefault((ident, m), []).append(eh)
    for span, ident, m in k_host:
        if span is not None and now < span[1]:
            held.setdefault((ident, m), []).append(span[0] // 3600)
    out = []
    for part in (p_dev, p_host):
        h = np.zeros(len(part), HIT_DTYPE)
        for i, (_, ident, m) in enumerate(part):
            hours = held.get((ident, m))
            if hours:
                h[i] = (len(hours) % 2 ** 32, min(hours), max(hours), 0)
        out.append(h)
    return tuple(out)


# ---- an image partitioned by a probe image, the hour as wildcard (include/ctmr.h ctmr_known_image_split),
# without a GPU

def _image_as_given(sets, rec, host) -> bytes:
    """The image of sets [(exp hour, digest, [indices into rec])] in the order given and host pairs [(key, member)] in
    the order given: the issuer table is the distinct digests ascending, nothing else is sorted or dropped."""
    digests = sorted({dg for _, dg, _ in sets})
    ordinal = {dg: i for i, dg in enumerate(digests)}
    set_part, first, take = [], 0, []
    for eh, dg, idx in sets:
        set_part.append(_SET.pack(eh, ordinal[dg], first, len(idx)))
        first += len(idx)
        take += idx
    host_part = b"".join(struct.pack("<I", len(k)) + k + struct.pack("<I", len(m)) + m for k, m in host)
    meta = _HEADER.pack(MAGIC, VERSION, HEADER_BYTES, len(digests), 0, len(sets), first, len(host_part), len(host), 0)
    meta += b"".join(digests) + b"".join(set_part) + host_part
    meta += b"\0" * (-len(meta) % 64)
    return meta + rec[np.asarray(take, np.int64)].tobytes()


def split(known, probes, now):
    """Engine.known_image_split(known, probes, now) without a GPU → (hit, miss): two images.  A probe is (Issuer.ID,
    serial) — the member records and host-section members of `probes`, their hours ignored.  hit holds every member
    record and host pair of a set of `known` kept at `now` that equals a probe, miss every other one of a kept set; sets
    that are not kept are in neither.  Both keep the order of `known`: the set records with their hour, those left
    empty dropped, the records of a set and the host pairs as they lie, repeats carried, nothing moved between the
    sections; the issuer table is the distinct digests the surviving set records name, ascending.  A canonical `known`
    gives canonical results.  Raises ImageError / ListsError where `find` does."""
    _, k_host = _sections(known)
    p_dev, p_host = _sections(probes)
    wanted = {(ident, m) for _, ident, m in p_dev + p_host}
    b = bytes(known)
    _, _, _, n_iss, _, n_sets, n_mem, _, _, _ = _HEADER.unpack_from(b, 0)
    so = HEADER_BYTES + 32 * n_iss
    rec = np.frombuffer(b, MEMBER_DTYPE, count=n_mem, offset=len(b) - n_mem * MEMBER_BYTES)
    sets, host = ([], []), ([], [])
    for s in range(n_sets):
        eh, ordinal, first, count = _SET.unpack_from(b, so + SET_BYTES * s)
        if not _HOUR_LO <= eh < _HOUR_HI or now >= (eh + 1) * 3600:
            continue
        dg = b[HEADER_BYTES + 32 * ordinal:HEADER_BYTES + 32 * (ordinal + 1)]
        ident = issuer_id(dg)
        r = rec[first:first + count]
        idx = ([], [])
        for i, (l, m) in enumerate(zip(r["len"], r["serial"])):
            idx[(ident, bytes(m[:int(l)])) not in wanted].append(first + i)
        for side in (0, 1):
            if idx[side]:
                sets[side].append((eh, dg, idx[side]))
    for (key, member), (span, ident, _) in zip(records(known)[1], k_host):
        if span is not None and now < span[1]:
            host[(ident, member) not in wanted].append((key, member))
    return _image_as_given(sets[0], rec, host[0]), _image_as_given(sets[1], rec, host[1])


def merge_hits(per_rank):
    """The hits of several ranks for the same probes (each a HIT_DTYPE array) as one: the records added, first_hour the
    minimum and last_hour the maximum over the ranks with records > 0.  The ranks of a group hold each key once."""
    per_rank = [np.asarray(h) for h in per_rank]
    out = np.zeros(len(per_rank[0]), HIT_DTYPE)
    first = np.full(len(out), 2 ** 31 - 1, np.int64)
    last = np.full(len(out), -2 ** 31, np.int64)
    total = np.zeros(len(out), np.uint64)
    for h in per_rank:
        got = h["records"] > 0
        total += h["records"]
        first = np.where(got, np.minimum(first, h["first_hour"]), first)
        last = np.where(got, np.maximum(last, h["last_hour"]), last)
    any_ = total > 0
    out["records"] = (total % np.uint64(2 ** 32)).astype(np.uint32)
    out["first_hour"] = np.where(any_, first, 0)
    out["last_hour"] = np.where(any_, last, 0)
    return out


def merge_lists(per_rank) -> list:
    """The lists of several ranks (each [(Issuer.ID, text)]) concatenated per Issuer.ID in rank order, IDs ascending.
    The ranks of a group hold each key once (owner or Bloom mode), so this is the group's list up to the order inside
    an expDate block.  Gathering the ranks' lists between processes is left to the caller."""
    out = {}
    for lists in per_rank:
        for i, text in lists:
            out.setdefault(bytes(i), []).append(bytes(text))
    return [(i, b"".join(out[i])) for i in sorted(out)]


# ---- the Redis protocol stream of an image as it lies (include/ctmr.h ctmr_known_image_resp), without a GPU

RESP_MAX_PER_COMMAND = 1 << 20


def image_resp(image, members_per_command=512) -> bytes:
    """The SADD + EXPIREAT stream of an image as Engine.known_image_resp writes it: the keys of the set records and of
    the host section in ascending bytewise order, a key of both sections once.  Per key: its member records in image
    order in SADD commands of at most `members_per_command` members, its host-section members in section order in SADD
    commands of their own, then one EXPIREAT key <first second of its expDate> (none for a host key without a second
    "::" or with a date `exp_date_span` cannot parse).  Neither sorts nor deduplicates.  Raises ImageError for what
    `parse` rejects and for a set record whose hour lies outside the years 0000..9999."""
    from .remote_cache import _resp
    per = int(members_per_command)
    if not 1 <= per <= RESP_MAX_PER_COMMAND:
        raise ValueError("members_per_command %r outside 1..2^20" % (members_per_command,))
    parse(image)
    b = bytes(image)
    _, _, _, n_iss, _, n_sets, n_mem, _, _, _ = _HEADER.unpack_from(b, 0)
    so = HEADER_BYTES + 32 * n_iss
    rec = np.frombuffer(b, MEMBER_DTYPE, count=n_mem, offset=len(b) - n_mem * MEMBER_BYTES)
    dev, expire = {}, {}
    for s in range(n_sets):
        eh, ordinal, first, count = _SET.unpack_from(b, so + SET_BYTES * s)
        if not _HOUR_LO <= eh < _HOUR_HI:
            raise ImageError("set %d: hour %d lies outside the years 0000..9999" % (s, eh))
        key = set_key(eh, b[HEADER_BYTES + 32 * ordinal:HEADER_BYTES + 32 * (ordinal + 1)])
        r = rec[first:first + count]
        dev[key] = [bytes(m[:int(l)]) for l, m in zip(r["len"], r["serial"])]
        expire[key] = eh * 3600
    host = {}
    for key, member in records(image)[1]:
        host.setdefault(key, []).append(member)
    for key in host:
        if key not in expire:
            date, sep, _ = key[len(PREFIX):].partition(b"::")
            span = exp_date_span(date) if sep else None
            expire[key] = None if span is None else span[0]
    out = []
    for key in sorted(expire):
        for members in (dev.get(key, ()), host.get(key, ())):
            for i in range(0, len(members), per):
                out.append(_resp(b"SADD", key, *members[i:i + per]))
        if expire[key] is not None:
            out.append(_resp(b"EXPIREAT", key, b"%d" % expire[key]))
    return b"".join(out)


def _digits(v):
    return len(b"%d" % v)


def resp_record_bytes(p, c, serial_len, hour, per, host_members=False) -> int:
    """The stream bytes of the member record at position p of a set of c records: its bulk string, the
    SADD header in front of it when it opens a command, and the EXPIREAT behind it when it is the set's last and the key
    has no host-section members.  The key of a set record is always 68 octets."""
    n = 5 + _digits(serial_len) + serial_len
    if p % per == 0:
        n += 13 + _digits(min(per, c - p) + 2) + 75
    if p == c - 1 and not host_members:
        t = _digits(hour * 3600)
        n += 98 + _digits(t) + t
    return n


def resp_bound(n_members, n_sets, host_bytes, n_host_members, per) -> int:
    """The size a caller can give the text buffer without a first call (include/ctmr.h ctmr_known_image_resp)."""
    return 47 * n_members + 95 * (n_members // per + n_sets) + 112 * n_sets + 2 * host_bytes + 208 * n_host_members


# ---- a Redis protocol stream as it lies → an image (include/ctmr.h ctmr_known_resp_image), without a GPU

class RespError(ValueError):
    """The stream is not a sequence of the commands ctmr_known_resp_image takes: the library fails with CTMR_E_INVAL."""


def resp_commands(stream) -> list:
    """The commands of a stream, each a list of its arguments.  Grammar: zero or more `*<N>\r\n` (N >= 1) followed by N
    bulk strings `$<L>\r\n<L octets>\r\n`; N and L are 1..10 decimal digits without sign or leading zero ("0" itself
    is allowed); nothing else — no inline commands, no null bulk strings, no trailing bytes."""
    b = bytes(stream)
    n, p, out = len(b), 0, []

    def number(p, lead):
        if p >= n or b[p] != lead:
            raise RespError("offset %d: %r expected" % (p, chr(lead)))
        q = p + 1
        while q < n and q - p <= 10 and 0x30 <= b[q] <= 0x39:
            q += 1
        d = b[p + 1:q]
        if not d or (len(d) > 1 and d[0] == 0x30) or b[q:q + 2] != b"\r\n":
            raise RespError("offset %d: 1..10 digits without a leading zero and CRLF expected" % p)
        return int(d), q + 2

    while p < n:
        at = p
        argc, p = number(p, 0x2a)
        if argc < 1:
            raise RespError("offset %d: a command of no arguments" % at)
        args = []
        for _ in range(argc):
            ln, q = number(p, 0x24)
            if q + ln + 2 > n or b[q + ln:q + ln + 2] != b"\r\n":
                raise RespError("offset %d: a bulk string of %d octets does not end in CRLF inside the stream" % (p, ln))
            args.append(b[q:q + ln])
            p = q + ln + 2
        out.append(args)
    return out


def resp_image_parts(stream):
    """→ (image, info dict) of a stream: `resp_image` and the counts ctmr_known_resp_image_info carries besides the
    image's own (commands; skipped_members: members of SADD commands under keys outside serials::)."""
    dev, host, commands, skipped = {}, set(), 0, 0
    for args in resp_commands(stream):
        commands += 1
        name = args[0].upper()
        if name == b"SADD":
            if len(args) < 3:
                raise RespError("SADD with %d arguments" % len(args))
            key = args[1]
            if not key.startswith(PREFIX):
                skipped += len(args) - 2
                continue
            pk = parse_key(key)
            for m in args[2:]:
                if pk is not None and len(m) <= MAX_SERIAL:
                    dev.setdefault(key, (pk, []))[1].append(m)
                else:
                    host.add((key, m))
        elif name in (b"EXPIREAT", b"PEXPIREAT"):
            if len(args) != 3:
                raise RespError("%s with %d arguments" % (name.decode(), len(args)))
        elif name == b"SELECT":
            if len(args) != 2:
                raise RespError("SELECT with %d arguments" % len(args))
        else:
            raise RespError("command %r" % args[0][:32])
    host = sorted(host)
    keys = sorted(dev)
    digests = sorted({dev[k][0][1] for k in keys})
    ordinal = {d: i for i, d in enumerate(digests)}
    set_part, members, first = [], [], 0
    for k in keys:
        (eh, dg), ms = dev[k]
        set_part.append(_SET.pack(eh, ordinal[dg], first, len(ms)))
        members += ms
        first += len(ms)
    host_part = b"".join(struct.pack("<I", len(k)) + k + struct.pack("<I", len(m)) + m for k, m in host)
    meta = _HEADER.pack(MAGIC, VERSION, HEADER_BYTES, len(digests), 0, len(keys), first, len(host_part), len(host), 0)
    meta += b"".join(digests) + b"".join(set_part) + host_part
    meta += b"\0" * (-len(meta) % 64)
    rec = np.zeros(first, MEMBER_DTYPE)
    if first:
        rec["len"] = np.fromiter((len(m) for m in members), np.uint64, first)
        rec["serial"] = np.frombuffer(b"".join(m.ljust(MAX_SERIAL, b"\0") for m in members), np.uint8).reshape(first, MAX_SERIAL)
    info = dict(members=first, sets=len(keys), host_members=len(host), meta_bytes=len(meta),
                image_bytes=len(meta) + MEMBER_BYTES * first, issuers=len(digests), commands=commands, skipped_members=skipped)
    return meta + rec.tobytes(), info


def resp_image(stream) -> bytes:
    """The image of a SADD / EXPIREAT stream as Engine.known_resp_image writes it — the inverse of `image_resp`.  The
    commands: SADD key member… (at least one member), EXPIREAT / PEXPIREAT key time and SELECT db (accepted and ignored:
    the image implies the expiry), names in any case; anything else raises RespError, as does every violation of the
    grammar of `resp_commands`.  A SADD under a key outside serials:: is skipped.  Under a serials:: key a member of at
    most 40 octets whose key `parse_key` takes becomes a member record, every other (key, member) pair goes to the host
    section.  The image is valid for `parse` but not necessarily canonical: issuers in digest order, one set per key
    with member records in key order, the records of a set in stream order across all its commands with repeats kept,
    the host pairs sorted and each once.  resp_image(image_resp(build(sets), per)) == build(sets), and
    union(resp_image(s)) == from_resp(s)."""
    return resp_image_parts(stream)[0]
