"""The known-certificate table through remove, expiry, rebuild and compaction (test helper, no test): a plain model of the
known sets and a builder of operation schedules.  tests/test_gpu_table_lifecycle.py replays a schedule on an engine and
on a model and compares every answer; tests/test_table_lifecycle_cpu.py holds both to their properties without a GPU.

Model: {key: set of members} plus {key: unix seconds} of ExpireAt overrides, with the RemoteCache set methods, the three
image calls and the sweep as engine/sets.inc applies it.  It knows the registered issuers' SPKI digests (a serials:: key
of a registered issuer is a table key: it expires at its expDate hour) and nothing else of the engine.  (What it takes
from tests/gpu_common.py, run_oracle, drives the CPU oracle: no GPU and no engine is involved.)

Schedule: a list of steps, each a dict with "kind" (one of STEP_KINDS) and its arguments:
  map            first, n            the synthetic entries [first, first + n) as one batch (overlaps: known entries)
  set_insert / set_remove / set_contains    items: [(key, member)]
  known_import / known_remove / known_query image: bytes (cut from the model's content at that point, plus strangers)
  expire_at      items: [(key, unix seconds)], live table keys
  sweep          now
  export         (nothing: the full comparison of every view)
The builder works through the twelve (insert path x remove path) pairs in a shuffled order — remove some members by
point remove / bulk remove / a sweep at their natural hour / a sweep that an earlier override makes due, then bring the
same members back by point insert / a map batch / an import — with other steps in between, so that tombstones, members
re-inserted behind them and live neighbours share probe chains while batches keep arriving.  `coverage(schedule, …)`
finds those pairs again by replaying the schedule on a fresh model: it does not trust the builder's bookkeeping.
"""
import base64
import random

import numpy as np

from ct_mapreduce_amd import known_image as KI, synth
from oracle import oracle as orc
from tests import known_corpus as KC
from tests.gpu_common import run_oracle

NOW = synth.BASE_TIME
STEP_KINDS = ("map", "set_insert", "set_remove", "set_contains", "known_import", "known_remove", "known_query",
              "expire_at", "sweep", "export")
INSERT_PATHS = ("point", "map", "import")
REMOVE_PATHS = ("point", "bulk", "sweep", "override")
INSERT_KIND = {"point": "set_insert", "map": "map", "import": "known_import"}
MAX_SERIAL = KI.MAX_SERIAL
# the randomised GPU test's inputs, fixed once every seed met its coverage condition on the GPU (same-size and growing
# rebuilds, a compaction over tombstones, an arena growth)
SEEDS = (1, 2, 4, 6)
N_STEPS = 80


def lifecycle_config():
    return synth.config(seed=77, n_issuers=6, dup_permille=150)


def issuer_digests(issuers):
    """SHA-256(SPKI) of each issuer certificate, through the oracle's Issuer.ID."""
    out = []
    for der in issuers:
        c = orc.parse_cert(der)
        out.append(base64.urlsafe_b64decode(orc.issuer_id(der[c.spki_off:c.spki_off + c.spki_len])))
    return out


def entry_keys(batch, issuers, digests):
    """(status per entry, [(set key, serial) of a PASS entry, else None]): the batch through a fresh oracle engine for
    status and expDate hour, the serial from the oracle's parse."""
    _, st, _, eh = run_oracle(batch, issuers, b"", True, NOW)
    keys = [None] * batch.n
    for i in np.nonzero(st == orc.ST_PASS)[0].tolist():
        der = batch.cert(i)
        c = orc.parse_cert(der)
        keys[i] = (KI.set_key(int(eh[i]), digests[int(batch.issuer_idx[i])]), der[c.serial_off:c.serial_off + c.serial_len])
    return st, keys


class Model:
    def __init__(self, digests):
        self.digests = [bytes(d) for d in digests]      # registered issuers, by issuer index
        self._registered = set(self.digests)
        self.sets = {}                                  # key → set of members
        self.expiry = {}                                # key → unix seconds (ExpireAt overrides)
        self._parsed = {}                               # key → table_key(key), kept: parsing a key is the slow part

    # ---- keys
    def table_key(self, key):
        """(exp_hour, digest) of a serials:: key of a registered issuer, else None."""
        if key not in self._parsed:
            pk = KI.parse_key(key)
            self._parsed[key] = pk if pk is not None and pk[1] in self._registered else None
        return self._parsed[key]

    def natural(self, key):
        pk = self.table_key(key)
        return None if pk is None else pk[0] * 3600

    def due(self, key):
        """When the key expires: its override, else its expDate hour (a table key), else never (None)."""
        return self.expiry[key] if key in self.expiry else self.natural(key)

    # ---- RemoteCache set methods
    def insert(self, key, member) -> bool:
        s = self.sets.setdefault(bytes(key), set())
        new = bytes(member) not in s
        s.add(bytes(member))
        return new

    def remove(self, key, member) -> bool:
        s = self.sets.get(bytes(key))
        if s is None or bytes(member) not in s:
            return False
        s.discard(bytes(member))
        if not s:
            del self.sets[bytes(key)]
        return True

    def contains(self, key, member) -> bool:
        return bytes(member) in self.sets.get(bytes(key), ())

    def expire_at(self, key, t):
        self.expiry[bytes(key)] = int(t)

    def sweep(self, now) -> int:
        gone = 0
        for key in list(self.sets):
            t = self.due(key)
            if t is not None and t <= now:
                gone += len(self.sets.pop(key))
        self.expiry = {k: t for k, t in self.expiry.items() if t > now}
        return gone

    # ---- a map batch: keys = [(key, serial) or None per entry]
    def map(self, keys):
        """→ WasUnknown per entry: the first PASS occurrence of a key the sets do not hold."""
        return np.fromiter((k is not None and self.insert(*k) for k in keys), bool, len(keys))

    # ---- the image calls (world = 1): the statistics include/ctmr.h defines
    def import_image(self, image) -> dict:
        dev, host = KI.records(image)
        ins = sum(self.insert(k, m) for k, m in dev)
        hins = sum(self.insert(k, m) for k, m in host)
        return {"members": len(dev), "taken": len(dev), "inserted": ins, "known": len(dev) - ins,
                "host_members": len(host), "host_inserted": hins}

    def remove_image(self, image) -> dict:
        dev, host = KI.records(image)
        hits = sum(self.remove(k, m) for k, m in dev)
        hhits = sum(self.remove(k, m) for k, m in host)
        return {"members": len(dev), "taken": len(dev), "hits": hits, "host_members": len(host), "host_hits": hhits}

    def query_image(self, image):
        dev, host = KI.records(image)
        fl = np.fromiter((self.contains(k, m) for k, m in dev), np.uint8, len(dev))
        hf = np.fromiter((self.contains(k, m) for k, m in host), np.uint8, len(host))
        return fl, hf, {"members": len(dev), "taken": len(dev), "hits": int(fl.sum()), "host_members": len(host),
                        "host_hits": int(hf.sum())}

    # ---- derived views
    def total(self):
        return sum(len(v) for k, v in self.sets.items() if self.table_key(k))

    def issuer_counts(self):
        at = {d: i for i, d in enumerate(self.digests)}
        out = [0] * len(self.digests)
        for k, v in self.sets.items():
            pk = self.table_key(k)
            if pk is not None:
                out[at[pk[1]]] += len(v)
        return out

    def device_members(self):
        """Members that live in the device table: at most 40 octets, under a table key."""
        return sum(sum(len(m) <= MAX_SERIAL for m in v) for k, v in self.sets.items() if self.table_key(k))

    def keys(self):
        return sorted(self.sets)

    def members(self, key):
        return sorted(self.sets.get(bytes(key), ()))

    def sorted_sets(self):
        return {k: sorted(self.sets[k]) for k in sorted(self.sets)}

    def lists(self, now):
        """[(Issuer.ID, text)]: known_image.lists_of_sets with, inside an expDate, the order a CTMR_KNOWN_ORDER_SORTED engine
        writes: the members its table holds, ascending, then those of the host-side store, ascending."""
        def order(key, members):
            dev = self.table_key(key) is not None
            return sorted(m for m in members if dev and len(m) <= MAX_SERIAL) + \
                sorted(m for m in members if not (dev and len(m) <= MAX_SERIAL))
        return KI.lists_of_sets({k: order(k, v) for k, v in self.sets.items()}, now)

    def image(self) -> bytes:
        """The canonical image: what an engine holding these sets exports in CTMR_KNOWN_ORDER_SORTED.  Members longer than
        40 octets are in it, in the host section (include/ctmr.h).  known_corpus.image writes what
        known_image.build writes, with numpy; its members are in known_image.sort's order already (both are checked in
        tests/test_table_lifecycle_cpu.py and tests/test_known_corpus_cpu.py)."""
        return KC.image(self.sets)


def apply_step(model, step, keys=None):
    """Applies one step to the model → what the engine must answer (kind by kind: see test_gpu_table_lifecycle.py).
    keys: the (key, serial) list of a map step's batch."""
    kind = step["kind"]
    if kind == "map":
        return model.map(keys)
    if kind in ("set_insert", "set_remove", "set_contains"):
        f = {"set_insert": model.insert, "set_remove": model.remove, "set_contains": model.contains}[kind]
        return [f(k, m) for k, m in step["items"]]
    if kind == "known_import":
        return model.import_image(step["image"])
    if kind == "known_remove":
        return model.remove_image(step["image"])
    if kind == "known_query":
        return model.query_image(step["image"])
    if kind == "expire_at":
        return [model.expire_at(k, t) for k, t in step["items"]]
    if kind == "sweep":
        return model.sweep(step["now"])
    assert kind == "export", kind
    return None


class Corpus:
    """The synthetic entries [0, span) a schedule maps from: status and (key, serial) of each."""
    def __init__(self, cfg, issuers, span):
        self.cfg, self.issuers, self.span = cfg, issuers, span
        self.digests = issuer_digests(issuers)
        self.status, self.keys = entry_keys(synth.host_batch(cfg, 0, span), issuers, self.digests)

    def batch(self, first, n):
        return synth.host_batch(self.cfg, first, n)


def _serial(rng, lo, hi):
    return bytes(rng.getrandbits(8) for _ in range(rng.randint(lo, hi)))


def make_schedule(seed, n_steps, issuers, cfg, span=9000, batch=(50, 1500), image=(10, 2000), point_run=50, corpus=None):
    """→ (steps, corpus).  See the module docstring; sizes: map batches of batch[0]..batch[1] entries, images of
    image[0]..image[1] records, point runs of at most point_run members."""
    rng = random.Random(seed)
    cp = corpus or Corpus(cfg, issuers, span)
    m = Model(cp.digests)
    steps, seen = [], set()                           # seen: entries presented so far

    def emit(**step):
        steps.append(step)
        if step["kind"] == "map":
            lo, n = step["first"], step["n"]
            seen.update(range(lo, lo + n))
            apply_step(m, step, cp.keys[lo:lo + n])
        else:
            apply_step(m, step)

    def emit_map(first, n):
        n = max(batch[0], min(n, batch[1], span))
        first = max(0, min(first, span - n))
        emit(kind="map", first=first, n=n)

    def live_entries():
        """Entries presented so far whose key is held now, in entry order, one per key."""
        out, had = [], set()
        for i in sorted(seen):
            k = cp.keys[i]
            if k is not None and k not in had and m.contains(*k) and m.table_key(k[0]):
                had.add(k)
                out.append(i)
        return out

    def fresh_map():
        hi = max(seen) + 1 if seen else 0
        if hi >= span - batch[0]:
            hi = rng.randrange(0, span - batch[1])
        emit_map(max(0, hi - rng.randint(0, 300)), rng.randint(400, batch[1]))   # overlaps what came before

    def strangers(n, long_too=True):
        """n (key, member) pairs nobody holds yet: random serials of 0..40 octets (a few above 40: host-side members)
        under keys the model holds, or under an expDate of their own."""
        keys = [k for k in m.keys() if m.table_key(k)]
        own = KI.set_key(rng.randint(491000, 493000), rng.choice(cp.digests))
        out = []
        while len(out) < n:
            key = rng.choice(keys) if keys and rng.random() < 0.5 else own
            mem = _serial(rng, 41, 60) if long_too and rng.random() < 0.03 else _serial(rng, 0, MAX_SERIAL)
            if not m.contains(key, mem) and (key, mem) not in out:
                out.append((key, mem))
        return out

    def image_of(pairs):
        sets = {}
        for k, mem in pairs:
            sets.setdefault(k, []).append(mem)
        return KC.image(sets)

    def held(n):
        """Up to n (key, member) pairs the model holds, long members included."""
        pairs = [(k, mem) for k in m.keys() for mem in m.members(k)]
        return rng.sample(pairs, min(n, len(pairs)))

    def clip(pairs):
        return pairs[:image[1]]

    def partial_now():
        """A `now` among the due times of the live sets at which some of them die and some survive."""
        times = sorted({m.due(k) for k in m.keys() if m.due(k) is not None})
        assert len(times) >= 2, "nothing to sweep partially"
        return times[rng.randint(len(times) // 4, len(times) // 2)] if len(times) > 6 else times[0]

    def remove(path):
        """Removes members of presented entries by `path` → their entry indices."""
        live = live_entries()
        while len(live) < 400:
            fresh_map()
            live = live_entries()
        if path == "point":
            a = rng.randrange(0, len(live) - point_run)
            victims = live[a:a + rng.randint(point_run // 2, point_run)]
            items = [cp.keys[i] for i in victims] + strangers(3)             # the strangers: nothing to remove
            rng.shuffle(items)
            emit(kind="set_remove", items=items)
        elif path == "bulk":
            n = rng.randint(150, 700)
            a = rng.randrange(0, max(1, len(live) - n))
            victims = live[a:a + n]
            extra = [p for p in held(60) if len(p[1]) > MAX_SERIAL or rng.random() < 0.3]   # host-side members leave too
            emit(kind="known_remove", image=image_of(clip([cp.keys[i] for i in victims] + extra + strangers(40))))
        elif path == "sweep":
            now = partial_now()
            victims = [i for i in live if m.due(cp.keys[i][0]) <= now and cp.keys[i][0] not in m.expiry]
            emit(kind="sweep", now=now)
        else:
            # an override EARLIER than the natural hour on a late key that holds presented entries, one LATER than it on a
            # key the sweep would take, then the sweep that crosses both
            now = partial_now()
            late = [i for i in live if m.natural(cp.keys[i][0]) > now and cp.keys[i][0] not in m.expiry]
            early = [k for k in m.keys() if m.natural(k) is not None and m.natural(k) <= now and k not in m.expiry]
            assert late and early
            emit(kind="expire_at", items=[(cp.keys[i][0], now - rng.randint(0, 5) * 3600)
                                          for i in rng.sample(late, min(40, len(late)))])
            emit(kind="expire_at", items=[(k, m.natural(k) + rng.randint(2000, 4000) * 3600)
                                          for k in rng.sample(early, min(10, len(early)))])
            victims = [i for i in live if cp.keys[i][0] in m.expiry and m.expiry[cp.keys[i][0]] <= now]
            filler(rng.choice(("set_contains", "known_query")))
            emit(kind="sweep", now=now)
        assert victims and not any(m.contains(*cp.keys[i]) for i in victims)
        return victims

    def reinsert(path, victims):
        if path == "point":
            items = [cp.keys[i] for i in rng.sample(victims, min(len(victims), point_run))] + held(2)
            rng.shuffle(items)
            emit(kind="set_insert", items=items)
        elif path == "import":
            emit(kind="known_import", image=image_of(clip([cp.keys[i] for i in victims]) + held(50) + strangers(50)))
        else:
            a = rng.choice(victims)
            emit_map(a - rng.randint(0, 200), rng.randint(300, batch[1]))

    def filler(kind):
        if kind == "map":
            if rng.random() < 0.7 and seen:             # a replay: known entries, cells that hold nothing afterwards
                emit_map(rng.randrange(0, max(seen)), rng.randint(batch[0], batch[1]))
            else:
                fresh_map()
        elif kind == "set_insert":
            pre1970 = KI.set_key(-rng.randint(1, 2000), rng.choice(cp.digests))       # an expDate before the epoch
            items = strangers(rng.randint(5, 30)) + [(pre1970, _serial(rng, 1, 20)) for _ in range(4)]
            if m.keys():
                items.append((rng.choice([k for k in m.keys() if m.table_key(k)]), _serial(rng, 41, 70)))
            emit(kind="set_insert", items=items)
        elif kind == "set_remove":
            emit(kind="set_remove", items=held(rng.randint(5, 30)) + strangers(3))
        elif kind == "set_contains":
            items = held(rng.randint(10, 40)) + strangers(10)
            rng.shuffle(items)
            emit(kind="set_contains", items=items)
        elif kind == "known_import":
            old = KI.set_key(-rng.randint(1, 2000), rng.choice(cp.digests))
            emit(kind="known_import", image=image_of(strangers(rng.randint(image[0], 600)) + held(30) +
                                                     [(old, _serial(rng, 0, MAX_SERIAL)) for _ in range(20)]))
        elif kind == "known_remove":
            emit(kind="known_remove", image=image_of(held(rng.randint(image[0], 300)) + strangers(20)))
        elif kind == "known_query":
            emit(kind="known_query", image=image_of(held(rng.randint(image[0], image[1] - 100)) + strangers(60)))
        elif kind == "expire_at":
            ks = [k for k in m.keys() if m.table_key(k)]
            emit(kind="expire_at", items=[(k, m.natural(k) + rng.randint(-48, 48) * 3600)
                                          for k in rng.sample(ks, min(5, len(ks)))])
        elif kind == "sweep":
            emit(kind="sweep", now=partial_now())
        else:
            emit(kind="export")

    fresh_map()
    fresh_map()
    filler("set_insert")
    filler("known_import")
    pairs = [(i, r) for i in INSERT_PATHS for r in REMOVE_PATHS]
    rng.shuffle(pairs)
    kinds = []
    for j, (ins, rem) in enumerate(pairs):
        victims = remove(rem)
        if rng.random() < 0.5:
            filler(rng.choice(("set_contains", "known_query", "export")))
        reinsert(ins, victims)
        while len(steps) < n_steps * (j + 1) // len(pairs):
            if not kinds:
                kinds = [k for k in STEP_KINDS if k != "sweep"] + ["map", "map"]
                rng.shuffle(kinds)
            filler(kinds.pop())
    emit(kind="export")
    return steps, cp


def coverage(steps, corpus):
    """What a schedule exercises, found by replaying it on a fresh model:
      kinds         the step kinds that occur
      reinserts     {(insert path, remove path)}: a member removed by the one and, absent since, inserted again by the other
      partial       sweeps that removed some sets and left others
      early, late   overrides that made a sweep take a live key before its natural hour / spare one past it
      sizes         {"map": [entries], "image": [member records]}"""
    m = Model(corpus.digests)
    removed_by = {}                                   # (key, member) → the path that removed it last
    out = {"kinds": set(), "reinserts": set(), "partial": 0, "early": 0, "late": 0, "sizes": {"map": [], "image": []}}

    def inserted(path, pairs):
        for p in pairs:
            if p in removed_by:
                out["reinserts"].add((path, removed_by.pop(p)))

    for step in steps:
        kind = step["kind"]
        out["kinds"].add(kind)
        if kind == "map":
            keys = corpus.keys[step["first"]:step["first"] + step["n"]]
            out["sizes"]["map"].append(len(keys))
            new = m.map(keys)
            inserted("map", [k for k, w in zip(keys, new) if w])
        elif kind == "set_insert":
            inserted("point", [p for p in step["items"] if m.insert(*p)])
        elif kind == "set_remove":
            for p in step["items"]:
                if m.remove(*p):
                    removed_by[tuple(p)] = "point"
        elif kind in ("known_import", "known_remove", "known_query"):
            dev, host = KI.records(step["image"])
            out["sizes"]["image"].append(len(dev))
            if kind == "known_import":
                inserted("import", [p for p in dev + host if m.insert(*p)])
            elif kind == "known_remove":
                for p in dev + host:
                    if m.remove(*p):
                        removed_by[p] = "bulk"
        elif kind == "sweep":
            now, before = step["now"], {k: set(v) for k, v in m.sets.items()}
            overridden = {k for k in before if k in m.expiry}
            out["early"] += any(m.expiry[k] <= now < m.natural(k) for k in overridden if m.natural(k) is not None)
            out["late"] += any(m.natural(k) <= now < m.expiry[k] for k in overridden if m.natural(k) is not None)
            m.sweep(now)
            dead = [k for k in before if k not in m.sets]
            out["partial"] += bool(dead) and bool(m.sets)
            for k in dead:
                for mem in before[k]:
                    removed_by[(k, mem)] = "override" if k in overridden else "sweep"
        elif kind == "expire_at":
            for k, t in step["items"]:
                m.expire_at(k, t)
    return out
