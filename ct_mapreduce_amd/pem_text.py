"""PEM certificate files ↔ a packed batch on the CPU: the twin of ctmr_pem_decode* (include/ctmr.h).

`parse` is a sequential restatement of the header's grammar, byte by byte; it shares nothing with the device code.  It
judges every byte itself and leaves only the arithmetic of four characters to three bytes to `base64`.  `parse_each`
judges every file on its own, the twin of ctmr_pem_decode_each* (DESIGN.md §23).  `layout` says which blocks the device
decodes where they lie.  `write` is the writer the tests and scripts/bench_pem_decode.py use.  No GPU is needed for any
of it.
"""
import base64

import numpy as np

WS = b" \t\r\n"
BLANK = b" \t\r"
ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
BEGIN = b"-----BEGIN CERTIFICATE-----"
END = b"-----END CERTIFICATE-----"
LINE_MAX = 1024     # a regular block of two lines and more has lines of at most this; so has the blank run behind BEGIN
_BODY = frozenset(ALPHABET + b"=" + WS)
_WS = frozenset(WS)


class PemTextError(ValueError):
    """A file outside the grammar: bad_file is its number, bad_offset a byte offset inside it (counted over the files
    back to back, as file_bounds counts)."""

    def __init__(self, bad_file, bad_offset, what):
        super().__init__("file %d, offset %d: %s" % (bad_file, bad_offset, what))
        self.bad_file = bad_file
        self.bad_offset = bad_offset


class _Bad(Exception):
    def __init__(self, at, what):
        self.at, self.what = at, what


def _skip(t, i, among):
    while i < len(t) and t[i] in among:
        i += 1
    return i


def _armor(t, i, literal, may_end_the_file):
    """The armor line whose first dash is t[i] → the index behind its eol."""
    if not (i == 0 or t[i - 1] == 0x0A):
        raise _Bad(i, "an armor line that does not start a line")
    if t[i:i + len(literal)] != literal:
        raise _Bad(i, "dashes that do not spell %r" % literal.decode())
    j = _skip(t, i + len(literal), BLANK)
    if j == len(t):
        if may_end_the_file:
            return j
        raise _Bad(len(t) - 1, "the file ends behind BEGIN")
    if t[j] != 0x0A:
        raise _Bad(j, "byte 0x%02x behind the closing dashes" % t[j])
    return j + 1


def _decode(chars, at):
    """The base64 text of a body (ws removed) → bytes.  Standard alphabet, a multiple of 4 characters, '=' only as the
    last one or two; spare bits may hold anything."""
    if len(chars) % 4:
        raise _Bad(at, "a body of %d characters" % len(chars))
    pad = len(chars) - len(chars.rstrip(b"="))
    if pad > 2 or b"=" in chars[:len(chars) - pad]:
        raise _Bad(at, "'=' elsewhere than at the end, or more than two")
    return base64.b64decode(chars)      # (every character has been judged: nothing is discarded here)


def _layout(t, begin, body, end, chars):
    """The layout of the block whose BEGIN starts at t[begin], whose body is t[body:end] and holds `chars`."""
    C = len(chars)
    if not C:
        return ("regular", 0, 0)
    if body - 1 - (begin + len(BEGIN)) > LINE_MAX:
        return ("irregular",)
    region = t[body:end]
    L = next(k for k, c in enumerate(region) if c in _WS)       # (an LF stands in front of END)
    eol = b"\n" if region[L] == 0x0A else b"\r\n" if region[L:L + 2] == b"\r\n" else None
    if eol is None:
        return ("irregular",)
    if L == C:                                                   # one line
        return ("regular", C, len(eol)) if region[L:] == eol else ("irregular",)
    if L == 0 or L > LINE_MAX or L % 4:
        return ("irregular",)
    want = b"".join(chars[k:k + L] + eol for k in range(0, C, L))
    return ("regular", L, len(eol)) if region == want else ("irregular",)


def parse_one(t):
    """One file → [(DER bytes, layout)]; raises _Bad."""
    t = bytes(t)
    out, i = [], 0
    while True:
        i = _skip(t, i, WS)
        if i == len(t):
            return out
        if t[i] != 0x2D:
            raise _Bad(i, "byte 0x%02x outside a block" % t[i])
        begin = i
        body = i = _armor(t, i, BEGIN, False)
        while i < len(t) and t[i] != 0x2D:
            if t[i] not in _BODY:
                raise _Bad(i, "byte 0x%02x inside a body" % t[i])
            i += 1
        if i == len(t):
            raise _Bad(len(t) - 1, "a BEGIN without its END")
        end = i
        i = _armor(t, i, END, True)
        chars = bytes(c for c in t[body:end] if c not in _WS)
        out.append((_decode(chars, body), _layout(t, begin, body, end, chars)))


def _walk(files):
    base = 0
    for f, t in enumerate(files):
        try:
            yield parse_one(t)
        except _Bad as b:
            raise PemTextError(f, base + max(b.at, 0), b.what) from None
        base += len(t)


def parse(files):
    """files: the texts in order → (payload bytes, offsets u64[n+1], file_first u64[F+1]).  Raises PemTextError with the
    number of the first file outside the grammar."""
    parts, offsets, file_first, at = [], [0], [0], 0
    for blocks in _walk(files):
        for der, _ in blocks:
            parts.append(der)
            at += len(der)
            offsets.append(at)
        file_first.append(len(offsets) - 1)
    return b"".join(parts), np.asarray(offsets, np.uint64), np.asarray(file_first, np.uint64)


def parse_each(files):
    """Every file judged on its own, the twin of ctmr_pem_decode_each* (DESIGN.md §23): (ders — the certificates of the
    good files in order, file_first u64[F+1], bad — per file None, or the offset that puts it outside the grammar, counted
    as in parse).  parse_one per file with the error caught: a bad file has no certificates and fails nothing."""
    ders, file_first, bad, base = [], [0], [], 0
    for t in files:
        try:
            ders += [der for der, _ in parse_one(t)]
            bad.append(None)
        except _Bad as b:
            bad.append(base + max(b.at, 0))
        file_first.append(len(ders))
        base += len(t)
    return ders, np.asarray(file_first, np.uint64), bad


def layout(files):
    """Per block, in text order: ("regular", L, e) — lines of L characters (the last may be shorter; L = the character
    count when there is one line, 0 with e = 0 for a body of none), each ended by the same eol of e bytes, no other ws in
    the body — or ("irregular",).  What include/ctmr.h says of info.regular / info.irregular."""
    return [lay for blocks in _walk(files) for _, lay in blocks]


def write_block(der, line=64, eol=b"\n", begin_blank=b"", end_eol=None):
    """One block.  line: characters per line (None: all in one); end_eol: what stands behind END's dashes (None: eol;
    b"": nothing, for a block that ends its file)."""
    chars = base64.b64encode(bytes(der))
    step = line or max(len(chars), 1)
    body = b"".join(chars[k:k + step] + eol for k in range(0, len(chars), step))
    return BEGIN + begin_blank + eol + body + END + (eol if end_eol is None else end_eol)


def write(ders, line=64, eol=b"\n", gap=b"", begin_blank=b"", end_eol=None):
    """One file: a block per DER, `gap` (ws) between blocks.  pem.EncodeToMemory writes line=64, eol=b"\\n"."""
    if bytes(gap).strip(WS) or bytes(begin_blank).strip(BLANK):
        raise ValueError("gap and begin_blank are white space")
    ders = list(ders)
    return bytes(gap).join(write_block(d, line, eol, begin_blank, end_eol if k + 1 == len(ders) else None)
                           for k, d in enumerate(ders))


def join(files):
    """The files back to back and their bounds: (text bytes, file_bounds u64[F+1])."""
    fb = np.zeros(len(files) + 1, np.uint64)
    if files:
        fb[1:] = np.cumsum([len(f) for f in files], dtype=np.uint64)
    return b"".join(bytes(f) for f in files), fb
