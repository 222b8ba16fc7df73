"""Builders shared by tests/test_get_entries_cpu.py and tests/test_gpu_entries_json.py: the accepted texts and the
rejections of ctmr_entries_json* (include/ctmr.h).  Expected bytes never come from the code under test:
the entries a builder starts from are the expectation, Python's json + base64 the second opinion."""
import base64
import json
import random

from ct_mapreduce_amd import get_entries as ge

MARK_BLOCK = 1024    # the bytes of a mark block (kernels/text_scan.h TX_TILE): one wave, 16 bytes a lane
DECODE_TILE = 1024   # the characters of a decode tile (TX_DTILE) → 768 bytes
TILE_OUT = DECODE_TILE * 3 // 4


def content(kind, n, rng=None):
    if kind == "zero":
        return bytes(n)
    if kind == "ff":
        return b"\xff" * n
    if kind.startswith("ramp"):
        p = int(kind[4:])
        return bytes((p + i) & 255 for i in range(n))
    return (rng or random.Random(n)).randbytes(n)


CONTENTS = ("zero", "ff", "ramp0", "ramp1", "ramp2", "random")


def length_entries(kind, top=200):
    """leaf and extra of every decoded length 0…top, crossed: (i, top − i) pairs pad 0 with 2, 1 with 1, 2 with 0 (top
    = 200), (i, i + 1 mod …) the rest — both '=' and '==' occur in both members."""
    rng = random.Random(7)
    out = [(content(kind, i, rng), content(kind, top - i, rng)) for i in range(top + 1)]
    out += [(content(kind, i, rng), content(kind, (i + 1) % (top + 1), rng)) for i in range(top + 1)]
    return out


def tile_entries(kind):
    """lengths TILE·3/4 − 2 … + 2 and 2·TILE·3/4 − 2 … + 2 of the decode tile, in both members"""
    rng = random.Random(8)
    ls = [m * TILE_OUT + d for m in (1, 2) for d in (-2, -1, 0, 1, 2)]
    return [(content(kind, a, rng), content(kind, b, rng)) for a, b in zip(ls, reversed(ls))]


def sextet_entries():
    """every sextet value at each of the four positions of a quantum: the value strings are built as text"""
    out = []
    for p in range(4):
        s = b"".join(bytes(ge.ALPHABET[v] if k == p else ge.ALPHABET[(v * 5 + k) & 63] for k in range(4)) for v in range(64))
        out.append((base64.b64decode(s), base64.b64decode(s[::-1][:128])))
    return out


def spare_bits_body():
    """padded quanta whose spare bits are not zero ("QUJ=" for "QUI=", "QR==" for "QQ=="): accepted, the bits dropped"""
    return b'{"entries":[{"leaf_input":"QUJ=","extra_data":"QR=="},{"leaf_input":"/+/=","extra_data":"+/=="}]}'


def small_entries(n, seed=1, lo=6, hi=40):
    rng = random.Random(seed)
    return [(rng.randbytes(rng.randrange(lo, hi)), rng.randbytes(rng.randrange(lo, hi))) for _ in range(n)]


def one_entry_110():
    """one entry of about 110 bytes of text"""
    e = [(bytes(range(30)), bytes(range(100, 124)))]
    body = ge.write_one(e)
    assert 100 <= len(body) <= 120
    return e, body


def gap_bodies(entries, widths=range(0, 71)):
    """0…70 ws bytes between every pair of neighbouring tokens in turn (gap g in front of token g; the last behind the
    closing brace): (g, w, body)"""
    nt = len(ge.tokens(entries))
    ws = b" \t\n\r"
    for g in range(nt + 1):
        for w in widths:
            yield g, w, ge.write_one(entries, gaps={g: bytes(ws[(g + k) & 3] for k in range(w))})


def lenient_host_accepts(body):
    """Would Python's json plus a lenient host (keys in any letter case, unknown keys ignored, escapes resolved — what
    encoding/json does for ct.GetEntriesResponse) take this body?"""
    try:
        doc = json.loads(bytes(body).decode("utf-8"))
        low = {k.lower(): v for k, v in doc.items()}
        if not isinstance(low["entries"], list):
            return False
        for e in low["entries"]:
            e = {k.lower(): v for k, v in e.items()}
            for k in ("leaf_input", "extra_data"):
                if not isinstance(e[k], str):
                    return False
                base64.b64decode(e[k], validate=True)
        return True
    except Exception:
        return False


def _at(i):
    return 4 + 10 * i   # the first token of entry i (ge.tokens: 4 of frame, 9 per entry, a comma between)


def _val(t, k, f):
    """token k is a value string: f(its characters) → the new characters"""
    t[k] = b'"' + f(t[k][1:-1]) + b'"'


def _rej(name, host, fn, whole=False):
    return {"name": name, "host_accepts": host, "fn": fn, "whole": whole}


def _sub(pos, what):
    return lambda t, i: _val(t, _at(i) + 3, lambda s: s[:pos] + what + s[pos + 1:])


def _tok(off, what):
    def f(t, i):
        t[_at(i) + off] = what
    return f


def _cut(lo, hi):
    def f(t, i):
        del t[_at(i) + lo:_at(i) + hi]
    return f


def _third_key(t, i):
    t[_at(i) + 8:_at(i) + 8] = [b",", b'"sct"', b":", b'"AAAA"']


def _trailing_comma(t, i):
    t.insert(_at(i) + 8, b",")


# entry-level rejections: fn(tokens of the body, index of the entry).  Values are at least 8 characters long.
REJECTIONS = [
    _rej("backslash in a value", False, _sub(2, b"\\")),
    _rej("escaped solidus", True, _sub(2, b"\\/")),
    _rej("minus in a value", False, _sub(3, b"-")),
    _rej("underscore in a value", False, _sub(3, b"_")),
    _rej("space in a value", False, _sub(3, b" ")),
    _rej("0x00 in a value", False, _sub(3, b"\x00")),
    _rej("0x80 in a value", False, _sub(3, b"\x80")),
    _rej("= in the middle", False, _sub(1, b"=")),
    _rej("===", False, lambda t, i: _val(t, _at(i) + 3, lambda s: s[:-3] + b"===")),
    _rej("length 1 mod 4", False, lambda t, i: _val(t, _at(i) + 3, lambda s: s[:4] + b"A")),
    _rej("length 2 mod 4", False, lambda t, i: _val(t, _at(i) + 3, lambda s: s[:4] + b"AA")),
    _rej("length 3 mod 4", False, lambda t, i: _val(t, _at(i) + 3, lambda s: s[:4] + b"AAA")),
    _rej("missing padding", False, lambda t, i: _val(t, _at(i) + 3, lambda s: b"QUJDRA")),
    _rej("url-safe alphabet", False, lambda t, i: _val(t, _at(i) + 3, lambda s: b"QUJD-_8A")),
    _rej("unknown third key", True, _third_key),
    _rej("leaf_input twice", False, _tok(5, b'"leaf_input"')),
    _rej("one key missing", False, _cut(4, 8)),
    _rej("key in another case", True, _tok(1, b'"Leaf_Input"')),
    _rej("trailing comma in an entry", False, _trailing_comma),
    _rej("missing comma", False, _cut(4, 5)),
    _rej("missing colon", False, _cut(2, 3)),
    _rej("missing closing brace of an entry", False, _cut(8, 9)),
    _rej("a number as value", False, _tok(3, b"1")),
    _rej("null as value", False, _tok(3, b"null")),
    _rej("an object as value", False, _tok(3, b"{}")),
    _rej("an array as value", False, _tok(3, b"[]")),
    # whole-body rejections: fn(tokens, index) ignores the index
    _rej("trailing comma in the array", False, lambda t, i: t.insert(len(t) - 2, b","), True),
    _rej("missing ]", False, lambda t, i: t.pop(len(t) - 2), True),
    _rej("missing }", False, lambda t, i: t.pop(), True),
    _rej("a byte behind }", False, lambda t, i: t.append(b"x"), True),
    _rej("a second object behind }", False, lambda t, i: t.extend([b"{", b"}"]), True),
    _rej("byte-order mark", False, lambda t, i: t.insert(0, b"\xef\xbb\xbf"), True),
    _rej("first key in another case", True, lambda t, i: t.__setitem__(1, b'"Entries"'), True),
]
assert len({r["name"] for r in REJECTIONS}) == len(REJECTIONS)

# bodies that are rejected as they stand
BAD_BODIES = [("empty body", b""), ("all-ws body", b" \n\t\r  "), ("a bare array", b"[]"), ("no entries key", b"{}"),
              ("entries is an object", b'{"entries":{}}'), ("a lone quote", b'"'), ("a backslash outside a string", b'{"entries":[]}\\')]


def reject_body(rej, entries, i):
    """the body of `entries` with rejection rej applied at entry i"""
    t = ge.tokens(entries)
    rej["fn"](t, i)
    return b"".join(t)


def rejection_cases(rej, n_resp=5, per=5, seed=3):
    """rej in the first, a middle and the last response and the first, a middle and the last entry: (bodies,
    bad_response).  The other bodies are valid; behind the bad one stands a second bad body in one case of three, so the
    LOWEST is what is asked for."""
    entries = small_entries(n_resp * per, seed)
    good = ge.write(entries, per)
    for r in (0, n_resp // 2, n_resp - 1):
        for i in ((0,) if rej["whole"] else (0, per // 2, per - 1)):
            bodies = list(good)
            bodies[r] = reject_body(rej, entries[r * per:(r + 1) * per], i)
            if r + 1 < n_resp and i == 0:
                bodies[-1] = b"{}"
            yield bodies, r


def split_string_pair():
    """two bodies whose concatenation is one valid body: the first ends inside a string"""
    entries = small_entries(3, 5)
    body = ge.write_one(entries)
    cut = body.index(b'"leaf_input":"') + 18
    return [body[:cut], body[cut:]], entries
