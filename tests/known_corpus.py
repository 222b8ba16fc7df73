"""Corpora of known-certificate sets with serials of every length (test helper, no test): {key: [members]} dicts and their
canonical image, for the directed tests of the image and list kernels (tests/test_gpu_known_lengths.py).  The synthetic
corpus has serials of 16 or 17 octets only; here the length mix is the parameter.

`make(mix, digests, hours, sizes)` builds the sets, `image(sets)` is known_image.build with the member records filled
by numpy (byte-identical, fast enough for a million members), `record_lens(image)` the serial_len column of an image.
tests/test_known_corpus_cpu.py checks all of it, and the structural claims of each mix, without a GPU.

Mixes (the record positions meant are those of the canonical image: sets in key order, members sorted):
  uniform      every length of `lengths` (default 0..40) equally likely, random octets (first octet arbitrary);
  tiny         uniform over 0..7: blocks of list text under 16 bytes;
  interleaved  record p is of 3..20 octets when p is even, of 21..40 when odd: both record classes in every wave of 64;
  runs         768 records of one class, then 768 of the other (shifted by 100): aligned 256-blocks of one class alone,
               and blocks where the class changes;
  twins        for each base string the base and the base followed by one, two and three 00 octets; the default bases
               cross the 20/21 boundary (17..20 octets) and the 40 limit (37..40: the longer twins are host members).
interleaved and runs start every member with its index in the set as three big-endian octets, which makes the sorted
order the generation order (so the class of a position is chosen, not drawn) and every member distinct; their lengths
therefore start at 3.  A set cannot hold more distinct members than its lengths allow (tiny: 1 + 256 + ... ): `make`
caps such a set at what it could draw and lists the key in Corpus.capped.
"""
import struct
from dataclasses import dataclass, field

import numpy as np

from ct_mapreduce_amd import known_image as KI

MIXES = ("uniform", "tiny", "interleaved", "runs", "twins")
SHORT, LONG = tuple(range(3, 21)), tuple(range(21, 41))
RUN, RUN_SHIFT = 768, 100


@dataclass
class Corpus:
    sets: dict                                  # key → sorted members (both sections)
    image: bytes
    capped: list = field(default_factory=list)  # keys whose set is smaller than asked for

    @property
    def members(self):
        return sum(len(v) for v in self.sets.values())


def default_lengths(mix):
    return {"uniform": tuple(range(41)), "tiny": tuple(range(8)), "interleaved": SHORT + LONG, "runs": SHORT + LONG,
            "twins": (0, 1, 17, 18, 19, 20, 37, 38, 39, 40)}[mix]


def class_at(mix, p):
    """Record class (0: at most 20 octets, 1: 21..40) of image position p in the positional mixes."""
    return p & 1 if mix == "interleaved" else ((p + RUN_SHIFT) // RUN) & 1


def _random_members(rng, size, lengths):
    """`size` distinct members with lengths drawn uniformly from `lengths` (fewer when the lengths do not hold as many)."""
    room = sum(256 ** L for L in lengths)
    size = min(size, room)
    got, lengths = set(), np.asarray(lengths)
    if room <= 1 << 17:  # lengths 0..2 only: take from all there are (drawing would not find the last ones)
        got = {v.to_bytes(L, "big") for L in lengths.tolist() for v in range(256 ** L)}
    for _ in range(6):
        if len(got) >= size:
            break
        m = 2 * (size - len(got)) + 64
        lens = rng.choice(lengths, m)
        raw = rng.integers(0, 256, size=(m, KI.MAX_SERIAL), dtype=np.uint8).tobytes()
        got.update(raw[40 * i:40 * i + L] for i, L in enumerate(lens.tolist()))
    got = sorted(got)
    if len(got) > size:
        got = [got[i] for i in np.sort(rng.choice(len(got), size, replace=False))]
    return got


def _positional_members(rng, mix, first, size, lengths):
    short = np.asarray([L for L in lengths if L <= 20]), np.asarray([L for L in lengths if L > 20])
    assert size < 1 << 24 and min(lengths) >= 3 and len(short[0]) and len(short[1])
    p = first + np.arange(size)
    cls = class_at(mix, p)
    # the lengths of a class in turn (every one occurs after a few dozen records), at a random phase per set
    turn = p // 2 + int(rng.integers(0, 64))
    lens = np.where(cls == 0, short[0][turn % len(short[0])], short[1][turn % len(short[1])])
    ser = rng.integers(0, 256, size=(size, KI.MAX_SERIAL), dtype=np.uint8)
    j = np.arange(size)
    ser[:, 0], ser[:, 1], ser[:, 2] = j >> 16, (j >> 8) & 255, j & 255
    raw = ser.tobytes()
    return [raw[40 * i:40 * i + L] for i, L in enumerate(lens.tolist())]


def twin_bases(rng, lengths):
    """Per length: random octets, the same ending in 00 already, and all zero; the empty string once."""
    out = []
    for L in lengths:
        if L == 0:
            out.append(b"")
            continue
        r = bytes(rng.integers(1, 256, size=L, dtype=np.uint8).tolist())
        out += [r, r[:-1] + b"\x00", b"\x00" * L]
    return out


def make(mix, digests, hours, sizes, seed=0, lengths=None, bases=None) -> Corpus:
    """Sets under serials::<expDate of hour>::<Issuer.ID of digest> for every hour and digest; `sizes`: members per set,
    one number or a list taken in key order (cycled)."""
    assert mix in MIXES
    rng = np.random.default_rng(seed)
    lengths = tuple(lengths) if lengths is not None else default_lengths(mix)
    keys = sorted(KI.set_key(h, d) for h in hours for d in digests)
    sizes = [sizes] if isinstance(sizes, int) else list(sizes)
    sets, capped, first = {}, [], 0
    for k, key in enumerate(keys):
        size = sizes[k % len(sizes)]
        if mix in ("uniform", "tiny"):
            ms = _random_members(rng, size, lengths)
        elif mix == "twins":
            bs = bases if bases is not None else twin_bases(rng, lengths)
            ms = sorted({b + b"\x00" * z for b in bs for z in range(4)})
        else:
            ms = _positional_members(rng, mix, first, size, lengths)
        if mix != "twins" and len(ms) < size:
            capped.append(key)
        sets[key] = ms
        first += sum(len(m) <= KI.MAX_SERIAL for m in ms)
    return Corpus(sets, image(sets), capped)


def image(sets) -> bytes:
    """known_image.build(sets), with the member records written by numpy instead of one by one."""
    dev, host = [], []
    for key in sorted(sets):
        pk = KI.parse_key(key)
        ms = sorted(set(sets[key]))
        if pk is None:
            host += [(key, m) for m in ms]
            continue
        host += [(key, m) for m in ms if len(m) > KI.MAX_SERIAL]
        ms = [m for m in ms if len(m) <= KI.MAX_SERIAL]
        if ms:
            dev.append((pk, ms))
    host.sort()
    digests = sorted({pk[1] for pk, _ in dev})
    ordinal = {d: i for i, d in enumerate(digests)}
    set_part, first = [], 0
    for (eh, dg), ms in dev:
        set_part.append(KI._SET.pack(eh, ordinal[dg], first, len(ms)))
        first += len(ms)
    host_part = b"".join(struct.pack("<I", len(k)) + k + struct.pack("<I", len(m)) + m for k, m in host)
    meta = KI._HEADER.pack(KI.MAGIC, KI.VERSION, KI.HEADER_BYTES, len(digests), 0, len(dev), first, len(host_part),
                           len(host), 0) + b"".join(digests) + b"".join(set_part) + host_part
    meta += b"\0" * (-len(meta) % 64)
    rec = np.zeros(first, KI.MEMBER_DTYPE)
    if first:
        rec["len"] = np.fromiter((len(m) for _, ms in dev for m in ms), np.uint64, first)
        padded = b"".join(m.ljust(KI.MAX_SERIAL, b"\0") for _, ms in dev for m in ms)
        rec["serial"] = np.frombuffer(padded, np.uint8).reshape(first, KI.MAX_SERIAL)
    return meta + rec.tobytes()


def split(img):
    """→ (meta bytes, member records as a writable MEMBER_DTYPE array) of an image."""
    n_mem = KI._HEADER.unpack_from(img, 0)[6]
    at = len(img) - n_mem * KI.MEMBER_BYTES
    return bytes(img[:at]), np.frombuffer(bytes(img[at:]), KI.MEMBER_DTYPE).copy()


def record_lens(img):
    return split(img)[1]["len"].astype(np.int64)


def record_sets(img):
    """The set index of every member record of an image."""
    _, _, _, n_iss, _, n_sets, n_mem, _, _, _ = KI._HEADER.unpack_from(img, 0)
    so = KI.HEADER_BYTES + 32 * n_iss
    counts = [KI._SET.unpack_from(img, so + KI.SET_BYTES * s)[3] for s in range(n_sets)]
    return np.repeat(np.arange(n_sets), counts)
