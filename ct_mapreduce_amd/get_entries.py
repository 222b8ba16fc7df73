"""get-entries HTTP bodies ↔ raw entries on the CPU: the twin of ctmr_entries_json* (include/ctmr.h).

`parse` is a sequential restatement of the header's grammar, byte by byte; it shares nothing with the device code and
asks neither `json` nor `base64` for a verdict.  `write` is the writer the tests and scripts/bench_entries_json.py use.
No GPU is needed for either.
"""
import binascii

import numpy as np

WS = b" \t\n\r"
ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
_LUT = np.full(256, 255, np.uint8)
_LUT[list(ALPHABET)] = np.arange(64)
KEYS = (b"leaf_input", b"extra_data")
STYLES = ("compact", "indent", "swapped", "alternate")


class GetEntriesError(ValueError):
    """A response outside the grammar: bad_response is its number, offset a byte offset inside it."""

    def __init__(self, bad_response, offset, what):
        super().__init__("response %d, offset %d: %s" % (bad_response, offset, what))
        self.bad_response = bad_response
        self.offset = offset


class _Bad(Exception):
    def __init__(self, at, what):
        self.at, self.what = at, what


def _ws(t, i):
    while i < len(t) and t[i] in WS:
        i += 1
    return i


def _expect(t, i, byte):
    if i >= len(t) or t[i] != byte:
        raise _Bad(min(i, len(t) - 1), "expected %r" % chr(byte))
    return i + 1


def _string(t, i):
    """The string that opens at t[i]: (its octets, the index behind its closing quote).  No quote lies inside a string
    of the grammar, so it ends at the next quote whatever stands in front of that."""
    i = _expect(t, i, 0x22)
    j = t.find(b'"', i)
    if j < 0:
        raise _Bad(len(t) - 1, "a string without its closing quote")
    return t[i:j], j + 1


def b64_decode(s, at=0):
    """Standard alphabet, length a multiple of 4, '=' or '==' at the very end only; the spare bits of a padded quantum
    may hold anything.  (Sextets by table, four to three by shifts: numpy does the arithmetic, not the judging.)"""
    if len(s) % 4:
        raise _Bad(at, "a value of %d characters" % len(s))
    pad = 2 if s.endswith(b"==") else 1 if s.endswith(b"=") else 0
    v = _LUT[np.frombuffer(s, np.uint8)[:len(s) - pad]]
    bad = np.nonzero(v == 255)[0]
    if bad.size:
        raise _Bad(at + int(bad[0]), "byte 0x%02x inside a value" % s[int(bad[0])])
    v = np.concatenate([v, np.zeros(pad, np.uint8)]).reshape(-1, 4).astype(np.uint32)
    x = v[:, 0] << 18 | v[:, 1] << 12 | v[:, 2] << 6 | v[:, 3]
    out = np.stack([x >> 16, x >> 8 & 255, x & 255], 1).astype(np.uint8).tobytes()
    return out[:len(out) - pad] if pad else out


def _value(t, i):
    s, j = _string(t, i)
    return b64_decode(s, i + 1), j


def _entry(t, i):
    i = _ws(t, _expect(t, i, 0x7B))
    got = {}
    for k in range(2):
        at = i
        key, i = _string(t, i)
        if key not in KEYS or key in got:
            raise _Bad(at, "key %r" % key)
        i = _ws(t, _expect(t, _ws(t, i), 0x3A))
        got[key], i = _value(t, i)
        i = _ws(t, i)
        if k == 0:
            i = _ws(t, _expect(t, i, 0x2C))
    return (got[KEYS[0]], got[KEYS[1]]), _expect(t, i, 0x7D)


def parse_one(t):
    """One body → [(leaf_input, extra_data)]; raises _Bad."""
    t = bytes(t)
    if not t:
        raise _Bad(0, "an empty body")
    i = _ws(t, _expect(t, _ws(t, 0), 0x7B))
    at = i
    key, i = _string(t, i)
    if key != b"entries":
        raise _Bad(at, "key %r" % key)
    i = _ws(t, _expect(t, _ws(t, i), 0x3A))
    i = _ws(t, _expect(t, i, 0x5B))
    out = []
    if i < len(t) and t[i] != 0x5D:
        while True:
            e, i = _entry(t, i)
            out.append(e)
            i = _ws(t, i)
            if i < len(t) and t[i] == 0x2C:
                i = _ws(t, i + 1)
                continue
            break
    i = _ws(t, _expect(t, i, 0x5D))
    i = _ws(t, _expect(t, i, 0x7D))
    if i != len(t):
        raise _Bad(i, "byte 0x%02x behind the closing brace" % t[i])
    return out


def parse(bodies):
    """bodies: the HTTP bodies in order → (blob bytes, bounds u64[2n+1], resp_first u64[R+1]).  Raises GetEntriesError
    with the number of the first body outside the grammar."""
    parts, bounds, resp_first, at, base = [], [0], [0], 0, 0
    for r, body in enumerate(bodies):
        try:
            entries = parse_one(body)
        except _Bad as b:
            raise GetEntriesError(r, base + max(b.at, 0), b.what) from None
        for pair in entries:
            for x in pair:
                parts.append(x)
                at += len(x)
                bounds.append(at)
        resp_first.append((len(bounds) - 1) // 2)
        base += len(body)
    return b"".join(parts), np.asarray(bounds, np.uint64), np.asarray(resp_first, np.uint64)


def parse_each(bodies):
    """Every body judged on its own, the twin of ctmr_entries_json_each* (DESIGN.md §22): (blob bytes, bounds u64[2n+1],
    resp_first u64[R+1], bad).  bad[r] is None, or an offset inside body r (counted from the first body's first byte) when
    that body is outside the grammar: it contributes no entries, resp_first[r + 1] == resp_first[r], and blob and
    bounds are those of `parse` over the other bodies."""
    parts, bounds, resp_first, bad, at, base = [], [0], [0], [], 0, 0
    for body in bodies:
        try:
            entries = parse_one(body)
            bad.append(None)
        except _Bad as b:
            entries = []
            bad.append(base + max(b.at, 0))
        for pair in entries:
            for x in pair:
                parts.append(x)
                at += len(x)
                bounds.append(at)
        resp_first.append((len(bounds) - 1) // 2)
        base += len(body)
    return b"".join(parts), np.asarray(bounds, np.uint64), np.asarray(resp_first, np.uint64), bad


def b64_encode(b):
    """The writer's encoder: nothing is judged here, so the standard library serves."""
    return binascii.b2a_base64(bytes(b), newline=False)


def tokens(entries, swap=lambda i: False):
    """The tokens of one body (a string is one token): 4 of frame, 9 per entry, a comma between entries, 2 to close."""
    t = [b"{", b'"entries"', b":", b"["]
    for i, (leaf, extra) in enumerate(entries):
        if i:
            t.append(b",")
        pair = [(KEYS[0], leaf), (KEYS[1], extra)]
        if swap(i):
            pair.reverse()
        t += [b"{", b'"%s"' % pair[0][0], b":", b'"%s"' % b64_encode(pair[0][1]), b",",
              b'"%s"' % pair[1][0], b":", b'"%s"' % b64_encode(pair[1][1]), b"}"]
    return t + [b"]", b"}"]


def _indent_gaps(t):
    """json.MarshalIndent(v, "", "  "): gap g stands in front of token g."""
    gaps, depth = [b""] * (len(t) + 1), 0
    for g in range(1, len(t)):
        prev, cur = t[g - 1], t[g]
        if prev in (b"{", b"["):
            depth += 1
        if cur in (b"}", b"]"):
            depth -= 1
        if prev in (b"{", b"[") and cur in (b"}", b"]"):
            gaps[g] = b""
        elif prev in (b"{", b"[", b",") or cur in (b"}", b"]"):
            gaps[g] = b"\n" + b"  " * depth
        elif prev == b":":
            gaps[g] = b" "
    return gaps


def write_one(entries, style="compact", gaps=None):
    """One body.  gaps: {g: white space in front of token g} (g = the token count: behind the last), over the style's."""
    if style not in STYLES:
        raise ValueError("style %r" % (style,))
    t = tokens(entries, {"swapped": lambda i: True, "alternate": lambda i: i % 2 == 1}.get(style, lambda i: False))
    gp = _indent_gaps(t) if style == "indent" else [b""] * (len(t) + 1)
    for g, w in (gaps or {}).items():
        if bytes(w).strip(WS):
            raise ValueError("gap %r is not white space" % (w,))
        gp[g if g >= 0 else len(t) + 1 + g] = bytes(w)
    return b"".join(gp[g] + t[g] for g in range(len(t))) + gp[len(t)]


def write(entries, per_response, style="compact", gaps=None):
    """entries: [(leaf_input, extra_data)]; per_response: entries per body (an int: that many, the last body the rest; a
    list: exactly those counts, zeros allowed) → the bodies.  style: compact (what log servers send), indent
    (MarshalIndent-like), swapped (extra_data first), alternate (every other entry swapped)."""
    entries = list(entries)
    if isinstance(per_response, int):
        counts = [per_response] * (len(entries) // per_response) + ([len(entries) % per_response] if len(entries) % per_response else [])
        counts = counts or [0]
    else:
        counts = list(per_response)
    if sum(counts) != len(entries):
        raise ValueError("per_response sums to %d, %d entries" % (sum(counts), len(entries)))
    out, at = [], 0
    for c in counts:
        out.append(write_one(entries[at:at + c], style, gaps))
        at += c
    return out


def join(bodies):
    """The bodies back to back and their bounds: (text bytes, resp_bounds u64[R+1])."""
    rb = np.zeros(len(bodies) + 1, np.uint64)
    if bodies:
        rb[1:] = np.cumsum([len(b) for b in bodies], dtype=np.uint64)
    return b"".join(bytes(b) for b in bodies), rb
