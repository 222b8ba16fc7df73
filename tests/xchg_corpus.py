"""Constructed key patterns for the cross-rank dedup (kernels/exchange.h, the XM_OWNER / XM_BLOOM tails of k_map_fused,
engine/exchange.inc, engine/group.inc) at up to MAX_WORLD = 16 ranks.  No GPU, no torch.

Three parts:
  * a PORT of the key hashing to plain Python integers (key_meta, mixk, key_hash, key_tag of ctmr_dev.h; key_owner_h,
    bloom_pos of kernels/keyrec.h; serial octets → s[0..4] as record_key of kernels/reduce.h lays them out), for serials
    of 0..40 octets, with numpy forms of the 8-octet case for the searches;
  * the MODEL: a dict over (exp_hour, canonical issuer, serial octets) fed the whole stream in log order — an entry was
    unknown if and only if its key has not been seen before.  It knows nothing of owners, tags or filters;
  * BUILDERS of rounds (holders, edges, twins, collisions, saturating): per-rank lists of certificates with their
    order_bases, ascending with the rank, whose keys were picked WITH the port so that named situations occur by
    construction — which rank owns a key, who presents it first, where in a wave a record sits, which keys share a tag.
tests/test_xchg_corpus_cpu.py holds the corpus to those conditions; tests/test_gpu_xchg_corpus.py runs it on the device.
"""
import calendar
import random
from collections import namedtuple

import numpy as np

from tests import der as D

M64 = (1 << 64) - 1
MAX_WORLD = 16
MAX_SERIAL = 40                                   # CTMR_MAX_SERIAL: longer serials live in host-side sets
NOT_AFTER = "270101000000Z"
EXP_HOUR = calendar.timegm((2027, 1, 1, 0, 0, 0)) // 3600
ISSUER_NAME = D.name(D.rdn(3, b"Synth Issuer 000"))   # the Name of synth.issuer(synth.config(n_issuers=1), 0)
CANON = 0                                         # one issuer: canonical index 0


# ------------------------------------------------------------------------------------------------ the hash port
def key_meta(exp_hour, canon, serial_len):
    return (1 << 63) | ((serial_len & 0x7f) << 56) | ((canon & 0xffffff) << 32) | (exp_hour & 0xffffffff)


def mixk(z):
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def rotl64(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def serial_words(serial):
    """Serial octets → s[0..4]: little-endian 64-bit words, zero padded to 40 octets."""
    assert len(serial) <= MAX_SERIAL
    p = bytes(serial) + bytes(MAX_SERIAL - len(serial))
    return [int.from_bytes(p[8 * k:8 * k + 8], "little") for k in range(5)]


def key_hash(meta, s):
    h = mixk((meta + 0x9e3779b97f4a7c15) & M64)
    h = mixk(h ^ s[0] ^ rotl64(s[1], 29) ^ 0x3c6ef372fe94f82b)
    h = mixk(h ^ s[2] ^ rotl64(s[3], 29) ^ rotl64(s[4], 47))
    return h


def key_tag(h):
    t = h >> 40
    if t == 0:
        t = 1
    if t == 0xffffff:
        t = 0xfffffe
    return t


def key_owner_h(h, world):
    return ((mixk(h ^ 0x5bd1e995) >> 32) * world) >> 32


def bloom_pos(h, wmask):
    """→ (word, bits) of a key in a blocked Bloom filter of wmask + 1 words."""
    g = mixk(h ^ 0xa0761d6478bd642f)
    bits = (1 << ((g >> 40) & 63)) | (1 << ((g >> 46) & 63)) | (1 << ((g >> 52) & 63)) | (1 << ((g >> 58) & 63))
    return g & wmask, bits


def serial_meta(serial, exp_hour=EXP_HOUR, canon=CANON):
    return key_meta(exp_hour, canon, len(serial))


def serial_hash(serial, exp_hour=EXP_HOUR, canon=CANON):
    return key_hash(serial_meta(serial, exp_hour, canon), serial_words(serial))


def serial_owner(serial, world):
    return key_owner_h(serial_hash(serial), world)


# numpy forms (uint64 arrays; the multiplications wrap)
U = np.uint64


def np_mixk(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U(30))) * U(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> U(27))) * U(0x94d049bb133111eb)
        return z ^ (z >> U(31))


def np_key_hash8(s0, exp_hour=EXP_HOUR, canon=CANON):
    """key_hash of 8-octet serials held little-endian in the uint64 array s0 (s[1..4] = 0)."""
    with np.errstate(over="ignore"):
        h = np_mixk(np.full(1, key_meta(exp_hour, canon, 8), U) + U(0x9e3779b97f4a7c15))
        h = np_mixk(h ^ s0 ^ U(0x3c6ef372fe94f82b))
        return np_mixk(h)


def np_key_tag(h):
    t = h >> U(40)
    t = np.where(t == U(0), U(1), t)
    return np.where(t == U(0xffffff), U(0xfffffe), t)


def np_key_owner_h(h, world):
    with np.errstate(over="ignore"):
        return ((np_mixk(h ^ U(0x5bd1e995)) >> U(32)) * U(world)) >> U(32)


def np_bloom_pos(h, wmask):
    g = np_mixk(h ^ U(0xa0761d6478bd642f))
    one = U(1)
    bits = (one << ((g >> U(40)) & U(63))) | (one << ((g >> U(46)) & U(63))) | (one << ((g >> U(52)) & U(63))) | \
        (one << ((g >> U(58)) & U(63)))
    return g & U(wmask), bits


def np_serials8(seed, n):
    """n distinct 8-octet serials as uint64 (little-endian: the low byte is the first octet, kept in 1..0x7e so that the
    INTEGER is minimal and positive)."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 1 << 63, n, dtype=np.int64).astype(U)
    first = rng.integers(1, 0x7f, n, dtype=np.int64).astype(U)
    s = np.unique((s & ~U(0xff)) | first)
    rng.shuffle(s)
    return s


def s8(v):
    return int(v).to_bytes(8, "little")


# ------------------------------------------------------------------------------------------------ certificates
Entry = namedtuple("Entry", "serial der")          # serial None: the certificate does not parse (it has no key)
Shard = namedtuple("Shard", "order_base entries")  # one rank's part of a round

_certs = {}


def cert(serial):
    c = _certs.get(serial)
    if c is None:
        c = _certs[serial] = D.cert(serial=serial, issuer=ISSUER_NAME, not_after=D.utctime(NOT_AFTER))
    return c


def entry(serial):
    return Entry(serial, cert(serial))


def bad_entry():
    """A certificate whose TBSCertificate is no SEQUENCE: a parse error, no key."""
    good = cert(b"\x01\x02\x03")
    assert good[0] == 0x30 and good[1] == 0x82 and good[4] == 0x30
    return Entry(None, good[:4] + b"\x31" + good[5:])


def rand_serial(rng, ln):
    return bytes([rng.randrange(1, 0x7f)] + [rng.randrange(256) for _ in range(ln - 1)])


def make_rounds(rounds_of_serials):
    """[[serials or Entries of rank 0, of rank 1, …], …] → [[Shard, …], …] with order_bases in log order over everything."""
    out, base = [], 0
    for per_rank in rounds_of_serials:
        shards = []
        for lst in per_rank:
            ents = [x if isinstance(x, Entry) else entry(x) for x in lst]
            shards.append(Shard(base, ents))
            base += len(ents)
        out.append(shards)
    return out


def stream(rounds):
    """Every entry in log order: round after round, rank after rank."""
    return [e for shards in rounds for sh in shards for e in sh.entries]


# ------------------------------------------------------------------------------------------------ the model
def entry_key(e, exp_hour=EXP_HOUR, canon=CANON):
    return None if e.serial is None else (exp_hour, canon, bytes(e.serial))


class Model:
    """WasUnknown of a single stream: unknown if and only if the key has not been seen before."""

    def __init__(self, key=entry_key):
        self.seen = {}
        self.key = key

    def feed(self, entries):
        out = []
        for e in entries:
            k = self.key(e)
            new = k is not None and k not in self.seen
            if new:
                self.seen[k] = True
            out.append(new)
        return out


def model_verdicts(rounds, model=None):
    """→ [[per-entry WasUnknown of rank 0's shard, of rank 1's, …], …] for the rounds in log order."""
    m = model or Model()
    return [[m.feed(sh.entries) for sh in shards] for shards in rounds]


# ------------------------------------------------------------------------------------------------ partitions by the port
Rec32 = namedtuple("Rec32", "meta s0 s1 s2 ord")
Rec64 = namedtuple("Rec64", "meta s src owner ord")


def partitions(entries, world, rank, ord_base, owner_of=key_owner_h):
    """What ctmr_xchg_map_device + ctmr_xchg_keys_device must deliver for one shard: per owner the 32-byte records
    (serials of at most 20 octets, ascending log order) and the 64-byte records (21..40 octets), nothing for `rank`."""
    p32 = [[] for _ in range(world)]
    p64 = [[] for _ in range(world)]
    for i, e in enumerate(entries):
        if e.serial is None or len(e.serial) > MAX_SERIAL:
            continue
        meta, s = serial_meta(e.serial), serial_words(e.serial)
        o = owner_of(key_hash(meta, s), world)
        if o == rank:
            continue
        if len(e.serial) <= 20:
            p32[o].append(Rec32(meta, s[0], s[1], s[2] & 0xffffffff, (ord_base + i) & 0xffffffff))
        else:
            p64[o].append(Rec64(meta, tuple(s), i, o, ord_base + i))
    return p32, p64


# ------------------------------------------------------------------------------------------------ key pools
class Pool:
    """Fresh 8-octet keys by owner under `world` (bucketed with the numpy port); no key is handed out twice."""

    def __init__(self, world, seed, n=1 << 16):
        self.world = world
        s = np_serials8(seed, n)
        own = np_key_owner_h(np_key_hash8(s), world)
        self.by_owner = [list(s[own == U(o)]) for o in range(world)]
        self.turn = 0

    def take(self, owner):
        return s8(self.by_owner[owner].pop())

    def any(self):
        self.turn += 1
        return self.take(self.turn % self.world)


# ------------------------------------------------------------------------------------------------ holders
HOLDER_WORLDS = (2, 3, 4, 5, 8, 16)
# where a key sits twice inside one shard: one wave, two waves of one 1 024-entry block, two blocks
PLACEMENTS = {"wave": (5, 41), "block": (64 + 7, 640 + 9), "blocks": (200, 1024 + 30)}


def presenter_triples(world):
    """(f1, f2, owner) with f1 < f2: every triple for world <= 5; beyond, every pair with the owner classes o = f1,
    o = f2 and a third rank taking turns."""
    out = []
    pairs = [(a, b) for a in range(world) for b in range(a + 1, world)]
    if world <= 5:
        return [(a, b, o) for a, b in pairs for o in range(world)]
    for k, (a, b) in enumerate(pairs):
        third = (a + b + k) % world
        while third in (a, b):
            third = (third + 1) % world
        out.append((a, b, (a, b, third)[k % 3]))
    return out


def holders(world, seed=0x686f6c64):
    """Two rounds in which every (owner, presenter, later presenter, held-before) situation occurs by construction."""
    assert world in HOLDER_WORLDS
    W = world
    pool = Pool(W, seed + W)
    r1 = [[] for _ in range(W)]
    r2 = [[] for _ in range(W)]
    for o in range(W):
        for f in range(W):
            r1[f].append(pool.take(o))                              # fresh, one presenter, into empty tables
            k = pool.take(o)
            g = (f + 1 + o % (W - 1)) % W                           # another rank presents it in round 1 …
            r1[g].append(k)
            r2[f].append(k)                                         # … f in round 2: known, wherever it lives
            r2[f].append(pool.take(o))                              # fresh, one presenter, into filled tables
    for f1, f2, o in presenter_triples(W):
        k = pool.take(o)
        r2[f1].append(k)
        r2[f2].append(k)
    k = pool.take(W // 2)                                           # one key from everybody
    for f in range(W):
        r2[f].append(k)
    k = pool.take(W - 1)                                            # the lowest rank and the owner itself (the highest)
    r2[0].append(k)
    r2[W - 1].append(k)
    # a key twice inside ONE shard: rank W − 1's, for keys of three other owners; rank 0's, for keys it owns itself
    def place(lst, owners):
        fixed = {}
        for (name, (p, q)), o in zip(PLACEMENTS.items(), owners):
            k = pool.take(o)
            fixed[p] = fixed[q] = k
        n = max(max(fixed) + 1, len(lst) + len(fixed))
        rest = iter(lst)
        out = []
        for i in range(n):
            out.append(fixed[i] if i in fixed else next(rest, None) or pool.any())
        return out
    r2[W - 1] = place(r2[W - 1], [0, (W - 1) // 2, max(W - 2, 0)])
    r2[0] = place(r2[0], [0, 0, 0])
    return make_rounds([r1, r2])


# ------------------------------------------------------------------------------------------------ edges
EDGE_WORLDS = (5, 8, 16)
EDGE_LENGTHS = (1, 63, 64, 65, 1023, 1024, 1025, 2049)


def edge_ranks(world):
    return (1, world // 2, world - 1)


def edges(world, rank, seed=0x65646765):
    """One sender's shard of 2 049 entries, wave by wave (64 entries each); every EDGE_LENGTHS prefix is a shard too.
    Block 0 (entries 0..1023): a wave full of records for the lowest remote owner, one for the highest, one for an owner
    in each dword of the 16-byte count row, a wave whose only remote record is lane 0, an empty one, one with lane 63
    only, an empty one, one with a record for every remote owner, one with a parse error and a 41-octet serial among 62
    remote records, then waves of serials of every length 1..40.  Block 1 (1024..2047): sixteen waves full of records for
    ONE owner.  Entry 2048: one more remote record."""
    assert world in EDGE_WORLDS and 0 <= rank < world
    pool = Pool(world, seed + 31 * world + rank)
    rng = random.Random(seed + 31 * world + rank)
    remote = [o for o in range(world) if o != rank]
    lo, hi = remote[0], remote[-1]
    full = lambda o: [pool.take(o) for _ in range(64)]
    own = lambda n: [pool.take(rank) for _ in range(n)]
    waves = [full(lo), full(hi)]
    for d in range(4):
        cand = [o for o in range(4 * d, min(4 * d + 4, world)) if o != rank]
        if cand:
            waves.append(full(cand[len(cand) // 2]))
    waves.append([pool.take(hi)] + own(63))
    waves.append(own(64))
    waves.append(own(63) + [pool.take(lo)])
    waves.append(own(64))
    waves.append([pool.take(remote[i % len(remote)]) for i in range(64)])
    w = [pool.take(remote[(3 * i) % len(remote)]) for i in range(64)]
    w[17] = bad_entry()
    w[40] = rand_serial(rng, 41)
    waves.append(w)
    ln = 0
    while len(waves) < 16:
        w = []
        for _ in range(64):
            ln = ln % 40 + 1
            w.append(rand_serial(rng, ln))
        waves.append(w)
    waves += [full(hi) for _ in range(16)]
    flat = [x for w in waves for x in w] + [pool.take(lo)]
    assert len(flat) == 2049
    return [x if isinstance(x, Entry) else entry(x) for x in flat]


# ------------------------------------------------------------------------------------------------ twins
TWIN_PREFIXES = (8, 16, 20)
TWIN_LENGTHS = (1, 7, 8, 15, 16, 19, 20, 21, 39, 40)


def twin_pairs(rng):
    """Pairs of serials that must stay two keys: equal in their first 8 / 16 / 20 octets and different behind, and
    X against X ‖ 00 (equal zero-padded words; only the length — or, at 40 → 41, the host-set boundary — differs)."""
    pairs = []
    for p in TWIN_PREFIXES:
        for total in sorted({p + 1, p + 4, min(p + 12, 40), 40}):
            head = rand_serial(rng, p)
            a = head + bytes(rng.randrange(256) for _ in range(total - p))
            b = bytearray(a)
            b[rng.randrange(p, total)] ^= 1 << rng.randrange(8)
            pairs.append((a, bytes(b)))
    for ln in TWIN_LENGTHS:
        x = rand_serial(rng, ln)
        pairs.append((x, x + b"\x00"))
    return pairs


def twins(world, seed=0x7477696e):
    """Three rounds.  Round 1: the partners of one set of pairs on different ranks; the first partners of a second set.
    Round 2: the second set's other partners, on other ranks.  Round 3: everything again, one rank further: all known.
    → (rounds, pairs)."""
    rng = random.Random(seed + world)
    same, apart = twin_pairs(rng), twin_pairs(rng)
    r1 = [[] for _ in range(world)]
    r2 = [[] for _ in range(world)]
    r3 = [[] for _ in range(world)]
    for k, (a, b) in enumerate(same):
        r1[k % world].append(a)
        r1[(k + 1 + (k // world) % (world - 1)) % world].append(b)
    for k, (a, b) in enumerate(apart):
        r1[(3 * k) % world].append(a)
        r2[(3 * k + 1) % world].append(b)
    for k, (a, b) in enumerate(same + apart):
        r3[(k + 2) % world].append(b)
        r3[(k + 3) % world].append(a)
    return make_rounds([r1, r2, r3]), same + apart


# ------------------------------------------------------------------------------------------------ tag collisions
COLLISION_WORLDS = (4, 8, 16)
COLLISION_SEARCH = 1 << 22
COLLISION_BLOOM_BITS = 1 << 16
Pair = namedtuple("Pair", "a b owner fillers")     # fillers: keys whose filter bits cover b's, in b's filter word

_searches = {}


def collisions(world, slots, seed=20261019, limit=12):
    """Pairs of 8-octet serials with the same 24-bit tag, the same home slot in a table of `slots` slots and the same
    owner under `world` — a seeded search over 2^22 serials with the numpy port.  Every pair comes with up to four filler
    keys that, added to a Bloom filter of COLLISION_BLOOM_BITS bits, make it report b."""
    got = _searches.get((world, slots, seed, limit))
    if got is not None:
        return got
    s = np_serials8(seed, COLLISION_SEARCH)
    h = np_key_hash8(s)
    owner = np_key_owner_h(h, world)
    sig = (np_key_tag(h) << U(40)) | ((h & U(slots - 1)) << U(8)) | owner
    order = np.argsort(sig, kind="stable")
    eq = np.nonzero(sig[order][1:] == sig[order][:-1])[0]
    word, bits = np_bloom_pos(h, COLLISION_BLOOM_BITS // 64 - 1)
    pairs, used, last = [], set(), -2
    for k in eq:
        if k == last + 1:                                           # three of a kind: the pairs must not overlap
            continue
        last = k
        ia, ib = int(order[k]), int(order[k + 1])
        fillers = []
        need = int(bits[ib])
        cand = np.nonzero(word == word[ib])[0]
        for c in cand:
            c = int(c)
            if c in (ia, ib) or c in used or not (int(bits[c]) & need):
                continue
            fillers.append(s8(s[c]))
            used.add(c)
            need &= ~int(bits[c])
            if not need:
                break
        if need:
            continue
        pairs.append(Pair(s8(s[ia]), s8(s[ib]), int(owner[ia]), tuple(fillers)))
        if len(pairs) == limit:
            break
    _searches[(world, slots, seed, limit)] = (pairs, len(eq))
    return pairs, len(eq)


def collision_senders(world, pair, k):
    """Three different ranks other than the pair's owner."""
    others = [r for r in range(world) if r != pair.owner]
    return others[k % len(others)], others[(k + 1) % len(others)], others[(k + 2) % len(others)]


def collision_rounds(world, pairs, placement, bloom=False):
    """(a) both partners received by the owner from two senders in one round; (b) one in the owner's own shard, the other
    received in the same round; (c) one held since an earlier round, the other received; (d) as (c), then real duplicates
    of both from a third rank.  bloom: a's first presenter also presents the fillers, so that its filter reports b and b
    is looked up in the table that holds a.  → (rounds, holder): holder[serial] = the rank that keeps the key — its
    owner, or in Bloom mode its first presenter."""
    assert placement in "abcd" and not (bloom and placement in "ab")
    r = [[[] for _ in range(world)] for _ in range({"a": 1, "b": 1, "c": 2, "d": 3}[placement])]
    holder = {}
    for k, p in enumerate(pairs):
        s1, s2, s3 = collision_senders(world, p, k)
        if placement == "a":
            r[0][s1].append(p.a)
            r[0][s2].append(p.b)
        elif placement == "b":
            own, sent = (p.a, p.b) if k % 2 == 0 else (p.b, p.a)
            r[0][p.owner].append(own)
            r[0][s2].append(sent)
        else:
            if bloom:
                r[0][s1] += list(p.fillers)
            r[0][s1].append(p.a)
            r[1][s2].append(p.b)
            if placement == "d":
                r[2][s3] += [p.a, p.b]
        holder[p.a] = s1 if bloom else p.owner
        holder[p.b] = s2 if bloom else p.owner
    return make_rounds(r), holder


# ------------------------------------------------------------------------------------------------ a saturated filter
SATURATED_BITS = 1 << 12


SATURATED_PER_RANK = 1600


def saturating(world=16, per=SATURATED_PER_RANK, seed=0x73617475):
    """Two rounds of `per` fresh keys per rank.  Every rank keeps a filter of its OWN keys: SATURATED_BITS bits = 64 words
    under 2 × 1 600 = 3 200 keys of 4 bits each are all but full (1 − e^(−3 200 · 4 / 4 096) = 0.96 of the bits), so in
    round 2 a key hits each of its 15 peers with probability ≈ 0.96^4 = 0.83 and goes to about 12 of them.  (200 keys per
    rank and round would leave the filters a third full — 0.32^4 = 0.01 per peer: a filter holds what ONE rank presented,
    not what the world did.)"""
    s = np_serials8(seed, 2 * world * per + 64)
    it = iter(s)
    return make_rounds([[[s8(next(it)) for _ in range(per)] for _ in range(world)] for _ in range(2)])


def bloom_traffic(rounds, bits):
    """Per round, the key records a Bloom round sends when every key is locally new where it is presented (fresh keys,
    each presented once): a key goes to every peer whose cumulative filter — the keys that peer found new up to and
    including this round — holds all of its bits."""
    world = len(rounds[0])
    wmask = bits // 64 - 1
    filt = [dict() for _ in range(world)]
    out = []
    for shards in rounds:
        pos = [[bloom_pos(serial_hash(e.serial), wmask) for e in sh.entries] for sh in shards]
        for r in range(world):
            for w, b in pos[r]:
                filt[r][w] = filt[r].get(w, 0) | b
        sent = 0
        for r in range(world):
            for w, b in pos[r]:
                sent += sum(1 for p in range(world) if p != r and (filt[p].get(w, 0) & b) == b)
        out.append(sent)
    return out
