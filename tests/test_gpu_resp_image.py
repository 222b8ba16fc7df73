"""-m gpu: a Redis protocol stream → an image (include/ctmr.h ctmr_known_resp_image*; kernels/resp_parse.h).

Expected bytes come from the CPU twin known_image.resp_image (tests/test_resp_image_cpu.py holds it to build, image_resp,
union and from_resp), never from the code under test; every comparison is exact bytes and runs through both variants at
exact-size buffers, with guard bytes round every buffer.  The device variant's stream lies at a chosen byte phase and is
followed by guard bytes that would parse — a read past len changes the result instead of faulting.  A call that fails
must leave every buffer as it was."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr
from ct_mapreduce_amd import known_image as KI, synth, _native as N
from ct_mapreduce_amd.remote_cache import _resp
from tests import known_corpus as KC
from tests.test_gpu_exchange import DEV
from tests.test_gpu_image_lists import CFG
from tests.test_gpu_known_image import engine, state
from tests.test_gpu_known_sort import shuffled, table
from tests.test_image_lists_cpu import raw_image
from tests.test_known_merge_cpu import with_host_pairs
from tests.test_resp_image_cpu import (DAY_KEY, GOOD, candidates, expireat, fragment_stream, key_cases, prefix_stream, rejections, sadd,
                                       sequential_tokens)

HOURS = [491000, 491003, 491027]
DIGESTS = [bytes(np.random.default_rng(2000 + k).integers(0, 256, size=32, dtype=np.uint8).tolist()) for k in range(72)]
GUARD = 64
TILE = 1024           # the bytes of a mark block (kernels/resp_parse.h RP_TILE); its waves take 64 in turn
TEMPT = b"\r\n$5\r\nhello\r\n*3\r\n$4\r\nSADD\r\n$68\r\n" + GOOD + b"\r\n$1\r\nZ\r\n" + sadd(GOOD, b"tempt") * 2
INFO = [f for f, _ in N.KnownRespImageInfo._fields_ if f != "reserved"]


@pytest.fixture(scope="module")
def eng():
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)   # no issuer registered: the call needs none
    yield e
    e.close()


def fields(info):
    return {f: getattr(info, f) for f in INFO}


def call_host(e, stream, cap, n=None):
    """→ (rc, info, image or None): the host variant with guards round the image buffer."""
    info = N.KnownRespImageInfo()
    buf = np.full(cap + 2 * GUARD, 0xEE, np.uint8)
    n = len(stream) if n is None else n
    rc = e._lib.ctmr_known_resp_image(e._h, bytes(stream), n, buf.ctypes.data + GUARD, cap, C.byref(info))
    assert (buf[:GUARD] == 0xEE).all() and (buf[GUARD + cap:] == 0xEE).all(), "image guards"
    if rc:
        assert (buf == 0xEE).all(), "written on failure"
        return rc, info, None
    assert (buf[GUARD + info.image_bytes:] == 0xEE).all()
    return rc, info, buf[GUARD:GUARD + info.image_bytes].tobytes()


def call_device(e, stream, meta_cap, members_cap, phase=0, n=None):
    """→ (rc, info, image or None): the device variant.  The first n bytes of `stream` (all by default) are the
    operand; it lies `phase` bytes behind a 16-byte boundary, behind a CRLF, and what follows its n bytes — the rest of
    `stream`, then TEMPT — would parse."""
    info = N.KnownRespImageInfo()
    n = len(stream) if n is None else n
    lead = b"\xee" * (14 + phase) + b"\r\n"
    raw = np.frombuffer(lead + bytes(stream) + TEMPT, np.uint8)
    d_s = torch.from_numpy(raw.copy()).to(DEV)
    meta = np.full(meta_cap + 2 * GUARD, 0xEE, np.uint8)
    d_out = torch.full((48 * members_cap + 2 * GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
    assert d_s.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    rc = e._lib.ctmr_known_resp_image_device(e._h, C.c_void_p(d_s.data_ptr() + len(lead)), n, meta.ctypes.data + GUARD, meta_cap,
                                             C.c_void_p(d_out.data_ptr() + GUARD), members_cap, C.byref(info))
    assert (d_s.cpu().numpy() == raw).all(), "the stream changed"
    rec = d_out.cpu().numpy()
    assert (meta[:GUARD] == 0xEE).all() and (meta[GUARD + meta_cap:] == 0xEE).all(), "meta guards"
    assert (rec[:GUARD] == 0xEE).all() and (rec[GUARD + 48 * members_cap:] == 0xEE).all(), "record guards"
    if rc:
        assert (meta == 0xEE).all() and (rec == 0xEE).all(), "written on failure"
        return rc, info, None
    assert (meta[GUARD + info.meta_bytes:] == 0xEE).all() and (rec[GUARD + 48 * info.members:] == 0xEE).all()
    return rc, info, meta[GUARD:GUARD + info.meta_bytes].tobytes() + rec[GUARD:GUARD + 48 * info.members].tobytes()


def differ(got, want):
    if got != want:
        assert len(got) == len(want), (len(got), len(want))
        bad = np.nonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[0]
        raise AssertionError("%d bytes differ, first at %d of %d: %r, expected %r" % (
            len(bad), bad[0], len(want), got[max(bad[0] - 20, 0):bad[0] + 28], want[max(bad[0] - 20, 0):bad[0] + 28]))


def check(e, stream, phases=(0,), host=True):
    """Both variants at exact-size buffers against the twin → the twin's image."""
    want, winfo = KI.resp_image_parts(stream)
    if host:
        rc, info, got = call_host(e, stream, len(want))
        assert rc == 0, (rc, e._lib.ctmr_last_error(e._h), fields(info), winfo)
        differ(got, want)
        assert fields(info) == winfo
    for phase in phases:
        rc, info, got = call_device(e, stream, winfo["meta_bytes"], winfo["members"], phase)
        assert rc == 0, (rc, e._lib.ctmr_last_error(e._h), fields(info), winfo)
        differ(got, want)
        assert fields(info) == winfo
    return want


def rejected(e, stream, phases=(0,), n=None):
    cap = 64 * len(stream) + 4096
    rc, _, got = call_host(e, stream, cap, n)
    assert rc == N.E_INVAL and got is None
    for phase in phases:
        rc, _, got = call_device(e, stream, cap, len(stream) // 6 + 1, phase, n)
        assert rc == N.E_INVAL and got is None


def ms(rng, n, lo=0, hi=41):
    return [bytes(rng.integers(0, 256, size=int(L), dtype=np.uint8).tolist()) for L in rng.integers(lo, hi, size=n)]


def test_the_struct():
    assert C.sizeof(N.KnownRespImageInfo) == 64 and N.KnownRespImageInfo.commands.offset == 48
    assert N.KnownRespImageInfo.skipped_members.offset == 56 and N.KnownRespImageInfo.issuers.offset == 40


# ---- 1. small streams, whole images

def test_the_smallest_streams(eng):
    assert check(eng, b"", phases=range(16)) == KI.build({})
    assert check(eng, sadd(GOOD, b"\x01\x02\x03"), phases=range(16)) == KI.build({GOOD: [b"\x01\x02\x03"]})
    check(eng, sadd(GOOD, b""), phases=(0, 7))
    only_host = sadd(DAY_KEY, b"\x01", b"") + sadd(b"serials::y", b"\x02" * 50) + sadd(GOOD, b"\x03" * 41) + expireat(GOOD)
    img = check(eng, only_host, phases=(0, 3))
    assert KI._HEADER.unpack_from(img, 0)[3:7] == (0, 0, 0, 0) and KI.parse(img).n_host_members == 4
    skipped = sadd(b"crl::x", b"a", b"b") + _resp(b"SELECT", b"0") + sadd(b"issuer::y", b"c") + expireat(b"crl::x")
    assert check(eng, skipped, phases=(0, 9)) == KI.build({})
    assert KI.resp_image_parts(skipped)[1]["skipped_members"] == 3
    assert eng.known_resp_image(only_host + skipped) == KI.resp_image(only_host)


@pytest.mark.parametrize("mix", KC.MIXES)
def test_every_mix_comes_back_byte_for_byte(mix, eng):
    c = KC.make(mix, DIGESTS, HOURS, [1, 63, 64, 65, 2, 255, 256, 257, 1, 7, 3, 127, 128, 129], seed=3)
    for per in (1, 2, 3, 512, 1 << 20):
        stream = KI.image_resp(c.image, per)
        assert check(eng, stream, phases=(per % 16,)) == c.image
    assert eng.known_merge(N.KNOWN_UNION, eng.known_resp_image(stream)) == KI.from_resp(stream) == c.image
    sh = shuffled(c.image, 4)
    stream = KI.image_resp(sh, 64)
    assert check(eng, stream, phases=(5,)) == sh
    # the Python surface
    assert eng.known_resp_image(stream) == sh
    meta, d_rec = eng.known_resp_image_device(torch.from_numpy(np.frombuffer(b"\0" * 3 + stream, np.uint8).copy()).to(DEV)[3:])
    assert meta + d_rec.cpu().numpy().tobytes() == sh
    assert eng.known_merge(N.KNOWN_UNION, sh) == KI.from_resp(stream)


def test_two_dumps_and_keys_that_come_back(eng):
    c = KC.make("uniform", DIGESTS[:6], HOURS, [5, 9, 70], seed=2)
    two = KI.image_resp(c.image, 2) + _resp(b"select", b"3") + KI.image_resp(shuffled(c.image), 3)
    img = check(eng, two, phases=(0, 11))
    assert eng.known_merge(N.KNOWN_UNION, img) == c.image == KI.from_resp(two.replace(_resp(b"select", b"3"), b""))
    k2 = KI.set_key(HOURS[1], DIGESTS[1])
    s = sadd(GOOD, b"\x03", b"\x01") + sadd(k2, b"\x09") + sadd(GOOD, b"\x02", b"\x03") + expireat(GOOD) + sadd(GOOD, b"") + sadd(k2, b"\x09")
    img = check(eng, s, phases=(0, 1))
    assert KI.records(img)[0] == [(GOOD, m) for m in (b"\x03", b"\x01", b"\x02", b"\x03", b"")] + [(k2, b"\x09")] * 2
    img = with_host_pairs({GOOD: [b"\x05"]}, [(GOOD, b"\x01" * 41), (DAY_KEY, b"\x07"), (b"serials::zzz", b"\x05")])
    for per in (1, 512):
        assert check(eng, KI.image_resp(img, per), phases=(0, 13)) == img


# ---- 2. tile edges

def cycle_stream(n=40):
    """Member lengths cycling 0..40 under three keys: more than three mark tiles."""
    out = []
    for k in range(n):
        out.append(sadd(KI.set_key(HOURS[k % 3], DIGESTS[k % 5]), *[bytes([(k + L) % 251 + 1]) * ((k + L) % 41) for L in range(3)]))
    s = b"".join(out)
    assert len(s) > 3 * TILE + 64
    return s


def shift(pad):
    """A skipped command that grows by one byte per pad"""
    s = sadd(b"crl::" + b"x" * (pad + 10), b"y")
    return s


def test_every_residue_of_the_tile(eng):
    s = cycle_stream()
    base = len(shift(0))
    for pad in range(64):
        lead = shift(pad)
        assert len(lead) == base + pad                                       # (the key's length keeps its two digits)
        check(eng, lead + s, phases=(pad % 16,), host=pad % 8 == 0)


@pytest.mark.parametrize("which", ["$", "1", "6", "\\r", "\\n", "\\r|\\n"])
def test_the_last_byte_of_a_tile(which, eng):
    j = ["$", "1", "6", "\\r", "\\n", "\\r|\\n"].index(which)
    member = bytes(range(1, 17))
    head = b"*3\r\n$4\r\nSADD\r\n$68\r\n" + GOOD + b"\r\n"
    for tile_end in (TILE - 1, 2 * TILE - 1, 255, 63):
        for pad in range(2300):
            lead = sadd(b"crl::" + b"x" * pad, b"y")
            at = len(lead) + len(head) + (j if j < 5 else 5 + 16)
            if at % TILE == tile_end % TILE and at >= tile_end:
                break
        else:
            raise AssertionError("no pad")
        s = lead + sadd(GOOD, member) + cycle_stream(30)
        assert s[at:at + 1] == {0: b"$", 1: b"1", 2: b"6", 3: b"\r", 4: b"\n", 5: b"\r"}[j] and s[len(lead) + len(head):][:5] == b"$16\r\n"
        check(eng, s, phases=(0, 15), host=tile_end == TILE - 1)


# ---- 3. fake headers

def aim(make, nd_max=5):
    """make(K as digits) → (stream, the position of the fake header, where its span shall end): the K that does it."""
    for nd in range(1, nd_max + 1):
        s, p, end = make(b"1" * nd)
        k = end - (p + 1 + nd + 2) - 2
        if k >= 0 and len(b"%d" % k) == nd:
            s, p, end = make(b"%d" % k)
            return s, p, end
    raise AssertionError("no K")


def fake_cases():
    """[(name, stream, the position of a fake header, where its span ends or None when it is no candidate)]"""
    out = []
    k2 = KI.set_key(HOURS[1], DIGESTS[1])
    tail = sadd(k2, b"\x01\x02", b"", b"\x03" * 40) + expireat(k2) + sadd(GOOD, b"\x07")

    def one(name, member, end_of, key=GOOD, pre=b"", post=tail, star=False, where=None):
        def make(kd):
            m = member.replace(b"K", kd)
            s = pre + sadd(key, b"\x09", m, b"\x0a") + post
            p = s.index(where or m) + (where or m).index(b"*" if star else b"$")
            return s, p, end_of(s, p)
        s, p, end = aim(make) if b"K" in member else make(b"")
        out.append((name, s, p, end))

    one("ends inside the same member", b"ab\r\n$3\r\nxyz\r\nrest", lambda s, p: p + 4 + 3 + 2)
    one("ends at the member's end", b"ab\r\n$3\r\nxyz", lambda s, p: p + 4 + 3 + 2)
    one("ends several true tokens later", b"ab\r\n$K\r\nxyz", lambda s, p: s.index(b"\x03" * 40) + 42)
    one("ends at the end of the command", b"ab\r\n$K\r\nxyz", lambda s, p: s.index(b"\x0a\r\n") + 3)
    one("ends exactly at len", b"ab\r\n$K\r\nxyz", lambda s, p: len(s))
    one("a fake * inside a member", b"ab\r\n*3\r\nxyz", lambda s, p: p + 4, star=True)
    one("a fake * and a bulk string behind it", b"ab\r\n*1\r\n$1\r\nq\r\nxyz", lambda s, p: p + 4, star=True)
    one("inside a host key", b"m", lambda s, p: p + 4 + 5 + 2, key=b"serials::\r\n$5\r\nhello\r\nx", where=b"\r\n$5\r\nhello")
    one("inside a skipped key", b"m", lambda s, p: p + 4 + 5 + 2, key=b"crl::\r\n$5\r\nhello\r\nx", where=b"\r\n$5\r\nhello")
    one("the first bytes of a member", b"$3\r\nabc", lambda s, p: p + 4 + 3 + 2)
    one("the first bytes of a member, ending later", b"$K\r\nabc", lambda s, p: s.index(b"\x03" * 40) + 42)
    one("a whole fake command in a member", sadd(GOOD, b"fake"), lambda s, p: p + 4, star=True)
    # no candidate: the landing bytes are not CRLF
    name, s, p, end = out[2]
    k = int(s[p + 1:s.index(b"\r\n", p)])
    out.append(("lands one short of a CRLF", s.replace(b"$%d\r\nxyz" % k, b"$%d\r\nxyz" % (k - 1)), p, None))
    out.append(("lands one behind a CRLF", s.replace(b"$%d\r\nxyz" % k, b"$%d\r\nxyz" % (k + 1)), p, None))
    out.append(("lands beyond len", s.replace(b"$%d\r\nxyz" % k, b"$%d\r\nxyz" % (len(s) + 7)), p, None))
    # two overlapping fakes in one region: the first ends inside the second's span, the second several tokens on
    def two(kd):
        m = b"a\r\n$40\r\n" + b"b" * 30 + b"\r\n$" + kd + b"\r\n" + b"c" * (5 - len(kd)) + b"\r\nddd"
        s = sadd(GOOD, b"\x09", m, b"\x0a") + tail
        return s, s.index(b"b\r\n$") + 3, s.index(b"\x03" * 40) + 42
    s, p, end = aim(two)
    assert (s.index(b"$40"), s.index(b"$40") + 5 + 40 + 2) in candidates(s)
    out.append(("two overlapping fakes", s, p, end))
    # a region that spans a tile edge (and several tiles)
    long = sadd(k2, *[bytes([k]) * 37 for k in range(1, 90)])
    one("a region over tile edges", b"ab\r\n$K\r\nxyz", lambda s, p: len(s) - len(tail), pre=sadd(b"crl::" + b"x" * 900, b"y"), post=long + tail)
    return out


@pytest.mark.parametrize("case", fake_cases(), ids=[c[0] for c in fake_cases()])
def test_fake_headers(case, eng):
    name, s, p, end = case
    cand = dict(candidates(s))
    if end is None:
        assert p not in cand
    else:
        assert cand[p] == end and p not in sequential_tokens(s), name
    check(eng, s, phases=(0, 6))
    check(eng, s + s, phases=(3,), host=False)


def test_streams_of_fragments(eng):
    rng = np.random.default_rng(11)
    fooled = 0
    for k in range(300):
        s = fragment_stream(rng, keys=(GOOD, DAY_KEY, b"crl::x", KI.set_key(HOURS[2], DIGESTS[2])))
        fooled += len(candidates(s)) > len(sequential_tokens(s))
        check(eng, s, phases=(k % 16,), host=k % 4 == 0)
    assert fooled > 150
    big = b"".join(fragment_stream(rng) for _ in range(400))                 # regions in every tile of a longer stream
    assert len(big) > 20 * TILE
    check(eng, big, phases=(0, 9))


# ---- 4. scan depth

def depth_commands():
    rng = np.random.default_rng(21)
    keys = [KI.set_key(h, d) for h in HOURS for d in DIGESTS[:40]] + [DAY_KEY]
    out = []
    for k in range(1200):
        n = int(rng.integers(1, 120))
        out.append((keys[int(rng.integers(0, len(keys)))], ms(rng, n, 0, 46)))
    return out


def test_more_tokens_than_a_scan_tile(eng):
    cmds = depth_commands()
    s = b"".join(sadd(k, *m) for k, m in cmds)
    assert sum(len(m) + 3 for _, m in cmds) >= 70000                          # tokens
    img = check(eng, s, phases=(0, 5))
    assert eng.known_merge(N.KNOWN_UNION, img) == KI.union(img)
    one = b"".join(sadd(k, x) for k, m in cmds for x in m)                    # per = 1: every command a run of its own
    check(eng, one, phases=(2,))
    by_key = sorted(cmds, key=lambda c: c[0])                                 # … and key by key: few runs, long ones
    check(eng, b"".join(sadd(k, *m) for k, m in by_key), phases=(4,), host=False)


def test_a_million_tokens(eng):
    """More than 2^20 candidates and more than 4096 mark tiles: every level of the scans and of the prefix maximum."""
    a, b = KI.set_key(HOURS[0], DIGESTS[0]), KI.set_key(HOURS[1], DIGESTS[1])
    few = [b"", b"\x01", b"\x02\x03", b""]
    s = (sadd(a, *(few * 140000)) + sadd(b, *(few * 125000)) + expireat(b) + sadd(a, b"\xff" * 40))
    assert len(s) > 4096 * TILE
    want, winfo = KI.resp_image_parts(s)
    assert winfo["members"] == 4 * 265000 + 1 > 1 << 20
    rc, info, got = call_device(eng, s, winfo["meta_bytes"], winfo["members"], phase=7)
    assert rc == 0 and fields(info) == winfo
    differ(got, want)


# ---- 5. members and keys

def test_member_lengths_alone_and_mixed(eng):
    for L in range(46):
        s = sadd(GOOD, *([bytes([L + 1]) * L] * 3)) + sadd(KI.set_key(HOURS[1], DIGESTS[0]), bytes([L]) * L)
        check(eng, s, phases=(L % 16,), host=L in (0, 40, 41, 45))
    mixed = [bytes([L ^ 0x5a]) * L for L in range(46)]
    check(eng, sadd(GOOD, *(mixed + mixed[::-1])) + sadd(GOOD, *mixed[::3]) + sadd(GOOD, b"\x01" * 40, b"\x02" * 41, b"\x03" * 40, b"\x02" * 41),
          phases=(0, 1))


def test_sets_of_one_and_of_65537_records(eng):
    rng = np.random.default_rng(31)
    big = [bytes(x) for x in rng.integers(0, 256, size=(65537, 16), dtype=np.uint8)]
    k2 = KI.set_key(HOURS[1], DIGESTS[1])
    s = sadd(k2, b"\x01") + b"".join(sadd(GOOD, *big[i:i + 512]) for i in range(0, len(big), 512)) + expireat(GOOD)
    img = check(eng, s, phases=(0, 10))
    assert [c for c in (KI._SET.unpack_from(img, 64 + 64 + 24 * k)[3] for k in range(2))] == [65537, 1]


@pytest.mark.parametrize("name,key,taken", key_cases(), ids=[c[0] for c in key_cases()])
def test_key_cases(name, key, taken, eng):
    other = KI.set_key(HOURS[2], DIGESTS[3])
    s = sadd(other, b"\x01") + sadd(key, b"\x05", b"\x04") + sadd(other, b"\x02") + sadd(key, b"\x06")
    img = check(eng, s, phases=(0, 12))
    dev, host = KI.records(img)
    assert ((key, b"\x05") in dev) == taken and ((key, b"\x05") in host) == (not taken)


# ---- 6. rejection and sizing

@pytest.mark.parametrize("name,stream", rejections(), ids=[c[0] for c in rejections()])
def test_rejections(name, stream, eng):
    with pytest.raises(KI.RespError):
        KI.resp_image(stream)
    rejected(eng, stream, phases=(0, 5))
    # … the damage in the last tile of a three-tile stream
    lead = b"".join(sadd(GOOD, bytes([k + 1]) * 30) for k in range(20))
    assert 2 * TILE + 100 < len(lead) < 3 * TILE - 300
    rejected(eng, lead + stream)


def test_every_prefix(eng):
    s = prefix_stream()
    ends, at = {0}, 0
    for args in KI.resp_commands(s):
        at += len(_resp(*args))
        ends.add(at)
    for n in range(len(s) + 1):
        if n in ends:
            want, winfo = KI.resp_image_parts(s[:n])
            rc, info, got = call_device(eng, s, winfo["meta_bytes"], winfo["members"], phase=n % 16, n=n)
            assert rc == 0 and got == want and fields(info) == winfo
        else:
            rejected(eng, s, phases=(n % 16,), n=n)        # the bytes behind n are the rest of the stream, then TEMPT
    # the final CRLF in the guard alone
    one = sadd(GOOD, b"\x01")
    assert TEMPT.startswith(b"\r\n")
    rc, _, got = call_device(eng, one[:-2], 4096, 8)
    assert rc == N.E_INVAL and got is None
    rc, _, got = call_device(eng, one + TEMPT[:13], 4096, 8, n=len(one))
    assert rc == 0 and got == KI.resp_image(one)


def test_a_length_of_4_gib_is_refused_without_a_read(eng):
    info = N.KnownRespImageInfo()
    small = sadd(GOOD, b"\x01")
    d = torch.from_numpy(np.frombuffer(small, np.uint8).copy()).to(DEV)
    out = np.full(4096, 0xEE, np.uint8)
    d_out = torch.full((4096,), 0xEE, dtype=torch.uint8, device=DEV)
    for n in (1 << 32, (1 << 32) - 64, 1 << 40):
        assert eng._lib.ctmr_known_resp_image(eng._h, small, n, out.ctypes.data, 4096, C.byref(info)) == N.E_INVAL
        assert eng._lib.ctmr_known_resp_image_device(eng._h, C.c_void_p(d.data_ptr()), n, out.ctypes.data, 4096, C.c_void_p(d_out.data_ptr()),
                                                     64, C.byref(info)) == N.E_INVAL
    assert (out == 0xEE).all() and (d_out.cpu().numpy() == 0xEE).all()


def test_short_buffers(eng):
    c = KC.make("twins", DIGESTS[:4], HOURS, 0, seed=11)                      # member records and host members
    s = KI.image_resp(c.image, 3)
    want, winfo = KI.resp_image_parts(s)
    assert winfo["host_members"] > 0 and winfo["members"] > 0
    for cap in (len(want) - 1, len(want) - 48, winfo["meta_bytes"], 0):
        rc, info, got = call_host(eng, s, cap)
        assert rc == N.E_RANGE and got is None and fields(info) == winfo
    for mc, nc in ((winfo["meta_bytes"] - 1, winfo["members"]), (winfo["meta_bytes"], winfo["members"] - 1), (0, 0)):
        rc, info, got = call_device(eng, s, mc, nc, phase=4)
        assert rc == N.E_RANGE and got is None and fields(info) == winfo
    rc, info, got = call_device(eng, s, winfo["meta_bytes"] + 100, len(s) // 6, phase=4)     # sized by the bound
    assert rc == 0 and got == want


# ---- 7. engines

def source_engine():
    issuers = synth.issuers(CFG)
    e = engine(issuers, table_slots=1 << 13)
    e.map_batch(synth.host_batch(CFG, 0, 2500))
    for k in range(2):                                                        # host-section members: above 40 octets
        for L in (41, 50, 60):
            e.set_insert("serials::%s::%s" % (KI.exp_date_id(491000).decode(), e.issuer_id(k)), bytes([k + 1]) * L)
    return issuers, e


def sorted_export(e):
    e.set_known_order(N.KNOWN_ORDER_SORTED)
    try:
        return e.known_export()
    finally:
        e.set_known_order(N.KNOWN_ORDER_ANY)


def test_the_warm_start(eng):
    issuers, e = source_engine()
    stream = e.known_resp(100)
    twin = KI.resp_image(stream)
    before = (state(e), table(e), e.issuer_counts().tobytes())
    assert e.known_resp_image(stream) == twin
    meta, d_rec = e.known_resp_image_device(torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).to(DEV))
    assert meta + d_rec.cpu().numpy().tobytes() == twin
    assert (state(e), table(e), e.issuer_counts().tobytes()) == before       # read-only
    fresh = engine(issuers, order=[5, 3, 1, 0, 2, 4], table_slots=1 << 13)
    st = fresh.known_import_resp(stream)
    assert st["inserted"] + st["host_inserted"] == KI.parse(twin).total
    assert sorted_export(fresh) == KI.union(twin) == sorted_export(e)
    assert state(fresh) == state(e)
    again = fresh.known_import_resp(stream + stream)                         # repeats: nothing new
    assert again["inserted"] == 0 and state(fresh) == state(e)
    ranks = [engine(issuers, table_slots=1 << 13) for _ in range(2)]
    for r, x in enumerate(ranks):
        x.known_import_resp(stream, world=2, rank=r)
    parts = [sorted_export(x) for x in ranks]
    assert all(KI.parse(p).total for p in parts) and KI.union(*parts) == KI.union(twin)
    for x in ranks + [fresh, e]:
        x.close()
