"""A Redis protocol stream → an image without a GPU (include/ctmr.h ctmr_known_resp_image): the CPU twin
known_image.resp_image against the functions that were there before it — `build`, `image_resp`, `union`, `from_resp` —,
its grammar, its key and member cases and every rejection; and a Python model of the parallel token search the kernels
run (candidates, cuts, conflict regions, the chain check) against the sequential parse on streams made to fool it.
tests/test_gpu_resp_image.py takes its streams and cases from here."""
import numpy as np
import pytest

from ct_mapreduce_amd import known_image as KI
from ct_mapreduce_amd.remote_cache import _resp
from tests import known_corpus as KC
from tests.test_image_lists_cpu import raw_image
from tests.test_known_merge_cpu import with_host_pairs
from tests.test_known_sort_cpu import shuffled, with_repeats

DIGESTS = [bytes([k]) * 31 + bytes([255 - k]) for k in range(1, 6)]
HOURS = [491000, 491003, 491027]
H = HOURS[0]
PERS = (1, 2, 3, 512)
GOOD = KI.set_key(H, DIGESTS[0])
DAY_KEY = b"serials::" + KI.exp_date_id(H)[:10] + b"::" + KI.issuer_id(DIGESTS[1])


def sadd(key, *members):
    return _resp(b"SADD", key, *members)


def expireat(key, t=1767600000):
    return _resp(b"EXPIREAT", key, b"%d" % t)


def both_identities(img, per, exact=True):
    """resp_image(image_resp(img)) == img (exact: an image whose host pairs all belong there) and
    union(resp_image(s)) == from_resp(s) → the stream."""
    s = KI.image_resp(img, per)
    back = KI.resp_image(s)
    KI.parse(back)
    if exact:
        assert back == img
    assert KI.union(back) == KI.from_resp(s) == KI.union(img)
    return s


# ---- 1. the two identities

@pytest.mark.parametrize("mix", KC.MIXES)
def test_the_inverse_of_image_resp_over_every_mix(mix):
    c = KC.make(mix, DIGESTS, HOURS, [1, 2, 65, 130], seed=5)
    assert c.image == KI.build(c.sets)
    for per in PERS:
        both_identities(c.image, per)
        both_identities(shuffled(c.image, per), per)
    both_identities(with_repeats(shuffled(c.image)), 3)


def test_raw_images_and_host_pairs():
    rng = np.random.default_rng(1)
    ms = [bytes(rng.integers(0, 256, size=int(L), dtype=np.uint8).tolist()) for L in rng.integers(0, 41, size=90)]
    raw = raw_image([(HOURS[0], DIGESTS[0], ms + ms[:7]), (HOURS[1], DIGESTS[1], [b""] * 3), (-5, DIGESTS[0], ms[::-1])])
    pairs = [(GOOD, b"\x01" * 41), (GOOD, b"\x02" * 45), (DAY_KEY, b"\x07"), (DAY_KEY, b""), (b"serials::zzz", b"\x05")]
    for per in PERS:
        both_identities(raw, per)
        both_identities(with_host_pairs({GOOD: ms}, pairs), per)
        # a host pair the member section can carry moves there: the image changes, its sets do not
        both_identities(with_host_pairs({GOOD: ms[:5]}, pairs + [(KI.set_key(H + 1, DIGESTS[2]), b"\x09")]), per, exact=False)


def test_two_hundred_random_images():
    rng = np.random.default_rng(7)
    for n in range(200):
        sets = {}
        for _ in range(int(rng.integers(0, 5))):
            key = KI.set_key(int(rng.integers(-30, 30)) * 1000, DIGESTS[int(rng.integers(0, 5))])
            sets[key] = [bytes(rng.integers(0, 256, size=int(L), dtype=np.uint8).tolist()) for L in rng.integers(0, 46, size=int(rng.integers(1, 9)))]
        if n % 3 == 0:
            sets[DAY_KEY] = [b"\x01", b"\x02" * 44]
        img = KI.build(sets)
        for per in PERS:
            s = both_identities(img, per)
        twice = s + _resp(b"SELECT", b"0") + KI.image_resp(img, 2)
        assert KI.union(KI.resp_image(twice)) == KI.from_resp(s + KI.image_resp(img, 2)) == KI.union(img)


def test_the_same_key_in_commands_that_are_not_adjacent_and_in_two_dumps():
    k2 = KI.set_key(H + 1, DIGESTS[1])
    s = sadd(GOOD, b"\x03", b"\x01") + sadd(k2, b"\x09") + sadd(GOOD, b"\x02", b"\x03") + expireat(GOOD) + sadd(GOOD, b"")
    img = KI.resp_image(s)
    assert img == raw_image([(H, DIGESTS[0], [b"\x03", b"\x01", b"\x02", b"\x03", b""]), (H + 1, DIGESTS[1], [b"\x09"])])
    assert KI.union(img) == KI.from_resp(s)
    c = KC.make("uniform", DIGESTS[:3], HOURS, [5, 9], seed=2)
    two = KI.image_resp(c.image, 2) + _resp(b"select", b"3") + KI.image_resp(shuffled(c.image), 3)
    img = KI.resp_image(two)
    assert KI.union(img) == c.image and KI.parse(img).n_members == 2 * KI.parse(c.image).n_members
    info = KI.resp_image_parts(two)[1]
    assert info["members"] == 2 * c.members and info["sets"] == 9 and info["skipped_members"] == 0 and info["issuers"] == 3
    assert KI.resp_image(b"") == KI.build({}) and KI.resp_image_parts(b"")[1]["commands"] == 0


# ---- 2. keys, members, commands

def key_cases():
    """[(name, key, whether parse_key takes it)]"""
    ident = KI.issuer_id(DIGESTS[0])
    spare = KI.issuer_id(DIGESTS[0][:31] + b"\x00")          # ends in "A=": the 43rd character carries four bits + 00

    def dated(date, i=ident):
        return b"serials::" + date + b"::" + i
    plus = KI.issuer_id(b"\xfb\xef\xbe" * 10 + b"\xfb\xef")   # an ID full of '-' …
    under = KI.issuer_id(b"\xff" * 32)                        # … and one full of '_'
    assert b"-" in plus and b"_" in under
    out = [("good", GOOD, True),
           ("67 octets", GOOD[:-1], False), ("69 octets", GOOD + b"=", False), ("69 octets, a longer date", dated(b"2026-01-05-010"), False),
           ("Feb 29 of a leap year", dated(b"2024-02-29-00"), True), ("Feb 29 of another", dated(b"2023-02-29-00"), False),
           ("Feb 29 of 1900", dated(b"1900-02-29-00"), False), ("Feb 29 of 2000", dated(b"2000-02-29-23"), True),
           ("Feb 30", dated(b"2024-02-30-00"), False), ("Apr 31", dated(b"2024-04-31-00"), False), ("month 00", dated(b"2024-00-10-00"), False),
           ("month 13", dated(b"2024-13-10-00"), False), ("day 00", dated(b"2024-01-00-00"), False), ("hour 24", dated(b"2024-01-10-24"), False),
           ("year 0000", dated(b"0000-01-01-00"), True), ("year 0000, Feb 29", dated(b"0000-02-29-05"), True),
           ("year 9999", dated(b"9999-12-31-23"), True), ("a sign for a digit", dated(b"+024-01-10-00"), False),
           ("a space for a digit", dated(b" 024-01-10-00"), False), ("a dot for a dash", dated(b"2024.01-10-00"), False),
           ("a spare bit set", dated(b"2024-01-10-00", spare[:42] + b"B="), False), ("spare bits zero", dated(b"2024-01-10-00", spare), True),
           ("- in the ID", dated(b"2024-01-10-00", plus), True), ("+ for -", dated(b"2024-01-10-00", plus.replace(b"-", b"+")), False),
           ("_ in the ID", dated(b"2024-01-10-00", under), True), ("/ for _", dated(b"2024-01-10-00", under.replace(b"_", b"/")), False),
           ("no =", dated(b"2024-01-10-00", ident[:43] + b"A"), False), ("= too early", dated(b"2024-01-10-00", ident[:42] + b"=="), False),
           ("a day-resolution key", DAY_KEY, False), ("no second ::", b"serials::zzz", False), ("the prefix alone", b"serials::", False),
           ("one : for ::", GOOD[:22] + b":-" + GOOD[24:], False)]
    assert spare.endswith(b"A=") and len({k for _, k, _ in out}) == len(out)
    return out


@pytest.mark.parametrize("name,key,taken", key_cases(), ids=[c[0] for c in key_cases()])
def test_key_cases(name, key, taken):
    assert (KI.parse_key(key) is not None) == taken
    other = KI.set_key(H + 2, DIGESTS[3])
    s = sadd(other, b"\x01") + sadd(key, b"\x05", b"\x04") + sadd(other, b"\x02")
    img, info = KI.resp_image_parts(s)
    assert KI.union(img) == KI.from_resp(s)
    dev, host = KI.records(img)
    if taken:
        assert sorted(dev) == sorted([(other, b"\x01"), (other, b"\x02"), (key, b"\x05"), (key, b"\x04")]) and not host
        assert [m for k, m in dev if k == key] == [b"\x05", b"\x04"]            # stream order
    else:
        assert dev == [(other, b"\x01"), (other, b"\x02")] and host == [(key, b"\x04"), (key, b"\x05")]
    assert (info["members"], info["host_members"], info["commands"]) == (len(dev), len(host), 3)


def test_member_lengths_0_40_and_41():
    s = sadd(GOOD, b"", b"\x01" * 40, b"\x02" * 41, b"\x03" * 40, b"") + sadd(GOOD, b"\x02" * 41, b"\x04" * 300)
    dev, host = KI.records(KI.resp_image(s))
    assert dev == [(GOOD, m) for m in (b"", b"\x01" * 40, b"\x03" * 40, b"")]
    assert host == [(GOOD, b"\x02" * 41), (GOOD, b"\x04" * 300)]
    assert KI.union(KI.resp_image(s)) == KI.from_resp(s)


def test_names_in_any_case_and_the_ignored_and_skipped_commands():
    s = (_resp(b"sAdD", GOOD, b"\x01") + _resp(b"ExpireAt", GOOD, b"1") + _resp(b"PEXPIREAT", GOOD, b"1000") + _resp(b"pexpireat", GOOD, b"x")
         + _resp(b"SELECT", b"0") + _resp(b"select", b"15") + sadd(b"crl::x", b"a", b"b", b"c") + sadd(b"serials:", b"d") + sadd(b"", b"e"))
    img, info = KI.resp_image_parts(s)
    assert img == KI.build({GOOD: [b"\x01"]})
    assert info["commands"] == 9 and info["skipped_members"] == 5 and info["members"] == 1
    assert KI.union(img) == KI.from_resp(sadd(GOOD, b"\x01") + sadd(b"crl::x", b"a"))


def rejections():
    """[(name, stream)]: every one raises RespError / gives CTMR_E_INVAL."""
    ok = sadd(GOOD, b"\x01")
    return [("N = 0", ok + b"*0\r\n"), ("SADD with N = 2", ok + _resp(b"SADD", GOOD)), ("SADD with N = 1", _resp(b"SADD") + ok),
            ("EXPIREAT with N = 2", ok + _resp(b"EXPIREAT", GOOD)), ("EXPIREAT with N = 4", _resp(b"EXPIREAT", GOOD, b"1", b"2") + ok),
            ("PEXPIREAT with N = 2", _resp(b"PEXPIREAT", GOOD)), ("SELECT with N = 1", _resp(b"SELECT")), ("SELECT with N = 3", _resp(b"SELECT", b"0", b"1")),
            ("an unknown command", ok + _resp(b"SREM", GOOD, b"\x01")), ("a name one longer", _resp(b"SADDX", GOOD, b"\x01")),
            ("a name one shorter", _resp(b"SAD", GOOD, b"\x01")), ("an empty name", _resp(b"", GOOD, b"\x01")),
            ("a name with a high bit", _resp(b"\xd3ADD", GOOD, b"\x01")), ("a name with a digit bit", _resp(b"SADd"[:3] + b"\x04", GOOD, b"\x01")),
            ("$-1", b"*3\r\n$4\r\nSADD\r\n$-1\r\n$1\r\nx\r\n"), ("*-1", b"*-1\r\n"),
            ("a leading zero in L", ok + b"*3\r\n$04\r\nSADD\r\n$1\r\nk\r\n$1\r\nx\r\n"), ("a leading zero in N", b"*03\r\n" + ok[4:]),
            ("11 digits", b"*3\r\n$4\r\nSADD\r\n$00000000001\r\nk\r\n$1\r\nx\r\n"), ("11 digits of N", b"*10000000000\r\n"),
            ("10 digits of L", b"*3\r\n$4\r\nSADD\r\n$4294967295\r\nk\r\n$1\r\nx\r\n"), ("10 digits of N", b"*4294967296\r\n" + ok[4:]),
            ("+5", b"*3\r\n$4\r\nSADD\r\n$+5\r\nabcde\r\n$1\r\nx\r\n"), ("no digits", b"*3\r\n$4\r\nSADD\r\n$\r\n\r\n$1\r\nx\r\n"),
            ("LF without CR in a header", ok + b"*3\n$4\r\nSADD\r\n$1\r\nk\r\n$1\r\nx\r\n"), ("LF without CR behind a member", ok[:-2] + b"\n"),
            ("CR without LF behind a member", ok[:-1] + b"\r"), ("an inline command", b"PING\r\n"), ("an inline command behind a good one", ok + b"PING\r\n"),
            ("a trailing byte", ok + b"\n"), ("a trailing CRLF", ok + b"\r\n"), ("a leading byte", b" " + ok), ("a bulk string first", b"$4\r\nSADD\r\n"),
            ("a member one octet longer than its length", sadd(GOOD, b"ab").replace(b"$2\r\nab", b"$1\r\nab")),
            ("a member one octet shorter", sadd(GOOD, b"ab").replace(b"$2\r\nab", b"$3\r\nab")),
            ("one argument too few", b"*4" + ok[2:]), ("one argument too many", b"*2" + ok[2:]),
            ("one argument too few, then a command", b"*4" + ok[2:] + ok), ("a simple string", b"+OK\r\n"), ("an integer", b":1\r\n")]


@pytest.mark.parametrize("name,stream", rejections(), ids=[c[0] for c in rejections()])
def test_rejections(name, stream):
    with pytest.raises(KI.RespError):
        KI.resp_image(stream)


def prefix_stream():
    """~200 bytes: three commands, a member that looks like a header, an empty member."""
    s = sadd(GOOD, b"\x01\x02", b"", b"\r\n$1\r\nx") + expireat(GOOD) + sadd(b"crl::x", b"y")
    assert 190 <= len(s) <= 260
    return s


def test_every_proper_prefix_is_rejected_unless_it_ends_a_command():
    s = prefix_stream()
    ends, at = {0}, 0
    for args in KI.resp_commands(s):
        at += len(_resp(*args))
        ends.add(at)
    assert at == len(s) and len(ends) == 4
    for n in range(len(s)):
        if n in ends:
            assert KI.union(KI.resp_image(s[:n])) == KI.from_resp(s[:n])
        else:
            with pytest.raises(KI.RespError):
                KI.resp_image(s[:n])


# ---- 3. the parallel token search (kernels/resp_parse.h), modelled: it finds the sequential parse's tokens or fails

def number(b, i):
    """rp_number: → (value, header bytes) of the number behind b[i], or None"""
    q = i + 1
    while q < len(b) and q - i <= 10 and 0x30 <= b[q] <= 0x39:
        q += 1
    d = b[i + 1:q]
    if not d or (len(d) > 1 and d[0] == 0x30) or b[q:q + 2] != b"\r\n":
        return None
    return int(d), q + 2 - i


def candidates(b):
    """[(position, next)] of every candidate token start, ascending."""
    out = []
    for i in range(len(b)):
        if b[i] not in b"*$" or (i != 0 and b[max(i - 2, 0):i] != b"\r\n"):
            continue
        num = number(b, i)
        if num is None:
            continue
        nx = i + num[1]
        if b[i] == 0x24:
            nx += num[0] + 2
            if nx > len(b) or b[nx - 2:nx] != b"\r\n":
                continue
        out.append((i, nx))
    return out


def parallel_tokens(b):
    """The kept candidates after cuts and conflict regions, or None when the chain check fails."""
    cand = candidates(b)
    pos = [c for c, _ in cand]
    nxt = [n for _, n in cand]
    at = {p: k for k, p in enumerate(pos)}
    cut, m = [], 0
    for k in range(len(cand)):
        cut.append(m <= pos[k])
        m = max(m, nxt[k])
    keep = list(cut)
    for k in range(len(cand) - 1):
        if cut[k] and not cut[k + 1]:
            p = nxt[k]
            while p in at and not cut[at[p]]:
                keep[at[p]] = True
                p = nxt[at[p]]
    toks = [k for k in range(len(cand)) if keep[k]]
    if not toks or pos[toks[0]] != 0 or b[0] != 0x2a:
        return None
    for a, c in zip(toks, toks[1:] + [None]):
        if nxt[a] != (len(b) if c is None else pos[c]):
            return None
    return [pos[k] for k in toks], sum(not c for c in cut)


def sequential_tokens(b):
    out, p = [], 0
    while p < len(b):
        if b[p] not in b"*$":
            return None
        num = number(b, p)
        if num is None:
            return None
        out.append(p)
        p += num[1] + (num[0] + 2 if b[p] == 0x24 else 0)
        if p > len(b) or (b[out[-1]] == 0x24 and b[p - 2:p] != b"\r\n"):
            return None
    return out


FRAGMENTS = [b"\r\n", b"\r", b"\n", b"$", b"*", b"0", b"1", b"2", b"3", b"7", b"10", b"\r\n$1\r\n", b"\r\n$0\r\n\r\n", b"\r\n$2\r\n", b"\r\n$3\r\n",
             b"\r\n$5\r\n", b"\r\n$12\r\n", b"\r\n$40\r\n", b"\r\n*1\r\n", b"\r\n*3\r\n", b"$4\r\nSADD\r\n", b"\r\n*3\r\n$4\r\nSADD\r\n", b"x", b"\x00", b"\xff"]


def fragment_stream(rng, keys=(GOOD, DAY_KEY, b"crl::x")):
    """A valid stream whose members are assembled from the fragments: many of them hold well-formed headers, some of
    which land on a CRLF further on."""
    out = []
    for _ in range(int(rng.integers(1, 6))):
        members = [b"".join(FRAGMENTS[int(k)] for k in rng.integers(0, len(FRAGMENTS), size=int(rng.integers(0, 9))))
                   for _ in range(int(rng.integers(1, 5)))]
        key = keys[int(rng.integers(0, len(keys)))]
        out.append(sadd(key, *members))
        if rng.integers(0, 3) == 0:
            out.append(expireat(key))
    return b"".join(out)


def test_the_parallel_search_finds_the_sequential_parse_on_streams_made_to_fool_it():
    rng = np.random.default_rng(11)
    fooled = 0
    for _ in range(3000):
        s = fragment_stream(rng)
        want = sequential_tokens(s)
        assert want is not None
        got, not_cut = parallel_tokens(s)
        assert got == want
        fooled += len(candidates(s)) > len(want)
        # … and damaged: whatever passes the chain check is the sequential parse
        cut = s[:int(rng.integers(1, len(s)))]                    # (the empty stream never reaches the search)
        got, want = parallel_tokens(cut), sequential_tokens(cut)
        assert (got is None) == (want is None) and (got is None or got[0] == want)
    assert fooled > 1500
