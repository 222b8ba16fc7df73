"""PEM texts for ctmr_pem_decode* (include/ctmr.h): the builders tests/test_pem_text_cpu.py holds to their
coverage and tests/test_gpu_pem_decode.py runs on the device.  "DER" here is any byte string: the decoder does not care
that it is no certificate.  No GPU."""
import base64

import numpy as np

from ct_mapreduce_amd import pem_text as pt

CONTENTS = ("zero", "ff", "ramp0", "ramp1", "ramp2", "random")
LINES = (4, 64, 76, None)          # None: the whole body in one line
EOLS = (b"\n", b"\r\n")
TILE_OUT = 768                     # the decode tile, in decoded bytes


def content(kind, n, seed=0):
    if kind == "zero":
        return bytes(n)
    if kind == "ff":
        return b"\xff" * n
    if kind.startswith("ramp"):
        return bytes((int(kind[4:]) + k) & 255 for k in range(n))
    return np.random.default_rng(1000 + seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def length_ders(kind):
    """every length 0…200 — which passes 48 k − 1, 48 k, 48 k + 1 (L = 64: last line one quantum short, full, a new line
    of one quantum) and the like for 57 k (L = 76) — and the decode tile's edges"""
    lens = list(range(0, 201)) + list(range(TILE_OUT - 2, TILE_OUT + 3)) + list(range(2 * TILE_OUT - 2, 2 * TILE_OUT + 3))
    return [content(kind, n, seed=n) for n in lens]


def sextet_ders():
    """every sextet value at every position of a quantum: DER p holds the 64 quanta whose character p runs through the
    alphabet while the other three hold the complement pattern"""
    out = []
    for p in range(4):
        b = bytearray()
        for v in range(64):
            s = [(63 - v) & 63] * 4
            s[p] = v
            x = s[0] << 18 | s[1] << 12 | s[2] << 6 | s[3]
            b += bytes([x >> 16, x >> 8 & 255, x & 255])
        out.append(bytes(b))
    return out


# spare bits set: "QR==" is 'A' with four spare bits 0001, "QUL=" is "AB" with two spare bits 11
SPARE_BITS_FILE = (pt.BEGIN + b"\nQR==\n" + pt.END + b"\n" + pt.BEGIN + b"\nQUL=\n" + pt.END + b"\n" +
                   pt.BEGIN + b"\nQUJDQf==\n" + pt.END + b"\n")
SPARE_BITS_DERS = [b"A", b"AB", b"ABCA"]


def ws_run(n, seed=0, among=pt.WS):
    """n bytes of mixed ws"""
    x, out = 12345 + 977 * seed, bytearray()
    for _ in range(n):
        x = (1103515245 * x + 12345) & 0x7fffffff
        out.append(among[(x >> 16) % len(among)])
    return bytes(out)


# ---------------------------------------------------------------------------------------------- regular families
def regular_files():
    """name → [file]: every block regular"""
    fam = {}
    for line in LINES:
        for eol in EOLS:
            fam["lengths L=%s e=%d" % (line, len(eol))] = [pt.write(length_ders("random"), line, eol)]
    fam["begin blank"] = [b"".join(pt.write_block(content("random", 100 + n, n), 64, b"\n", ws_run(n, n, pt.BLANK)) for n in range(0, 71))]
    fam["end of file"] = [pt.write([b"abc", b"defg"], end_eol=b""), pt.write([b"x" * 100], 76, b"\r\n", end_eol=b"")]
    fam["sextets"] = [pt.write(sextet_ders(), 64), pt.write(sextet_ders(), 4, b"\r\n")]
    fam["spare bits"] = [SPARE_BITS_FILE]
    fam["gaps between blocks"] = [b"\n \t\r\n" + pt.write([b"abc", b"", b"defgh"], gap=b"\r\n\t \n") + b"  \n\n"]
    return fam


# ---------------------------------------------------------------------------------------------- irregular families
GAP_KINDS = ("between lines", "after 1st", "after 2nd", "after 3rd", "before pads", "between pads", "before END")


def with_gap(der, kind, gap):
    """the LF / 64 block of `der` (its length ≡ 1 mod 3, at least 52: two pads, two lines and more) with ws at one place"""
    assert len(der) % 3 == 1 and len(der) >= 52
    chars = base64.b64encode(der)
    lines = [chars[k:k + 64] for k in range(0, len(chars), 64)]
    body = b"".join(l + b"\n" for l in lines)
    at = {"between lines": 65, "after 1st": 1, "after 2nd": 66 + 2, "after 3rd": 3, "before pads": len(body) - 3,
          "between pads": len(body) - 2, "before END": len(body)}[kind]
    if kind == "before END":
        gap = gap + b"\n"              # END's first dash follows an LF
    return pt.BEGIN + b"\n" + body[:at] + gap + body[at:] + pt.END + b"\n"


def irregular_files():
    """name → [file]: every block irregular"""
    fam = {}
    for kind in GAP_KINDS:
        fam["gap " + kind] = [b"".join(with_gap(content("random", 52 + 3 * (n % 40), n), kind, ws_run(n, n)) for n in range(1, 71))]
    fam["long ws runs"] = [with_gap(content("random", 100, 1), "after 2nd", ws_run(1100, 1)) + with_gap(content("random", 1000, 2), "between lines", ws_run(2100, 2)),
                           with_gap(content("random", 58, 3), "between pads", ws_run(1100, 3)) + with_gap(content("random", 61, 4), "before END", ws_run(2100, 4))]
    d = content("random", 400, 9)
    chars = base64.b64encode(d)

    def lines(lens, eols=(b"\n",), tail=()):
        out, at, k = [], 0, 0
        while at < len(chars):
            n = lens[k % len(lens)]
            out.append(chars[at:at + n] + (tail[k % len(tail)] if tail else b"") + eols[k % len(eols)])
            at += n
            k += 1
        return pt.BEGIN + b"\n" + b"".join(out) + pt.END + b"\n"
    fam["alternating lengths"] = [lines([64, 60])]
    fam["first line shorter"] = [lines([60] + [64] * 20)]
    fam["L = 62"] = [lines([62])]
    fam["eols mixed"] = [lines([64], (b"\r\n", b"\n")), lines([64], (b"\n", b"\n", b"\r\n"))]
    fam["blank behind one line"] = [lines([64], tail=(b"", b"", b" ", b"", b"", b"", b"", b"", b"", b"", b""))]
    fam["lines over the limit"] = [pt.write_block(content("random", 3 * 780, 5), pt.LINE_MAX + 4)]
    fam["blanks behind BEGIN over the limit"] = [pt.write_block(b"abcd", begin_blank=b" " * (pt.LINE_MAX + 1))]
    return fam


def mixed_file():
    """an irregular block between two regular ones"""
    return pt.write_block(content("random", 300, 1)) + with_gap(content("random", 100, 2), "after 1st", b" ") + pt.write_block(content("random", 301, 3), 76, b"\r\n")


# ---------------------------------------------------------------------------------------------- counts
COUNT_FILES = (0, 1, 2, 63, 64, 65, 257)
COUNT_BLOCKS = (0, 1, 2, 64, 65)


def count_files(F, per):
    return [pt.write([content("random", (7 * f + 3 * k) % 90, f * 131 + k) for k in range(per)], (64, 76, 4, None)[f % 4], EOLS[f % 2]) for f in range(F)]


def tightest_file(n):
    """n blocks of 54 bytes but for the last, which ends with the file: 54 n − 1 bytes"""
    return (pt.BEGIN + b"\n" + pt.END + b"\n") * (n - 1) + pt.BEGIN + b"\n" + pt.END if n else b""


# ---------------------------------------------------------------------------------------------- rejections
GOOD = pt.write_block(content("random", 100, 77))
_B64 = base64.b64encode(content("random", 100, 78))        # 136 characters, two pads


def _block(body, begin=pt.BEGIN, end=pt.END, after_begin=b"\n", after_end=b"\n"):
    return begin + after_begin + body + end + after_end


_BODY = b"".join(_B64[k:k + 64] + b"\n" for k in range(0, len(_B64), 64))
# name → (what stands in the place of one good block, what Go's  for { block, rest = pem.Decode(rest) }  — recalled, not
# pinned — would have done with it)
REJECTIONS = {
    "four dashes": (_block(_BODY, begin=b"----BEGIN CERTIFICATE-----"), "skipped the junk"),
    "six dashes": (_block(_BODY, begin=b"------BEGIN CERTIFICATE-----"), "skipped the junk"),
    "six closing dashes": (_block(_BODY, begin=b"-----BEGIN CERTIFICATE------"), "skipped the junk"),
    "four closing dashes of END": (_block(_BODY, end=b"-----END CERTIFICATE----"), "skipped the junk"),
    "a dash inside the body": (_block(_BODY[:10] + b"-" + _BODY[10:]), "failed the block"),
    "the URL-safe alphabet": (_block(b"QUJD_-8=\n"), "failed the block"),
    "X509 CRL": (_block(_BODY, b"-----BEGIN X509 CRL-----", b"-----END X509 CRL-----"), "taken the block, another type"),
    "TRUSTED CERTIFICATE": (_block(_BODY, b"-----BEGIN TRUSTED CERTIFICATE-----", b"-----END TRUSTED CERTIFICATE-----"), "taken the block, another type"),
    "another letter case": (_block(_BODY, b"-----Begin Certificate-----", b"-----End Certificate-----"), "taken the block, another type"),
    "a header line": (_block(b"Proc-Type: 4,ENCRYPTED\n\n" + _BODY), "taken the header"),
    "a header line without dashes": (_block(b"Label: x\n\n" + _BODY), "taken the header"),
    "a comment": (b"# Label: \"Some Root\"\n" + GOOD, "skipped the junk"),
    "subject= lines": (b"subject=CN = Some Root\nissuer=CN = Some Root\n" + GOOD, "skipped the junk"),
    "a byte-order mark": (b"\xef\xbb\xbf" + GOOD, "skipped the junk"),
    "NUL": (GOOD + b"\x00\n", "skipped the junk"),
    "a byte over 0x7f in the body": (_block(_BODY[:5] + b"\x80" + _BODY[5:]), "failed the block"),
    "BEGIN without END": (pt.BEGIN + b"\n" + _BODY, "skipped the junk"),
    "END without BEGIN": (_BODY + pt.END + b"\n", "skipped the junk"),
    "two BEGINs": (pt.BEGIN + b"\n" + GOOD, "taken the inner block"),
    "two ENDs": (GOOD + pt.END + b"\n", "skipped the junk"),
    "END before BEGIN": (pt.END + b"\n" + pt.BEGIN + b"\n", "skipped the junk"),
    "a byte behind BEGIN's dashes": (_block(_BODY, after_begin=b"x\n"), "skipped the junk"),
    "a byte behind BEGIN's dashes and a blank": (_block(_BODY, after_begin=b" \tQUJD\n"), "skipped the junk"),
    "a byte behind END's dashes": (_block(_BODY, after_end=b"x\n"), "skipped the junk"),
    "a byte behind END's dashes and a blank": (_block(_BODY, after_end=b" \r x\n"), "taken the block, skipped the junk"),
    "BEGIN not at a line start": (b" " + GOOD, "taken the block"),
    "BEGIN behind a lone CR": (b"\r" + GOOD, "taken the block"),
    "END not at a line start": (_block(_BODY[:-1]), "failed the block"),
    "BEGIN and END on one line": (pt.BEGIN + b" " + pt.END + b"\n", "failed the block"),
    "one character short": (_block(_BODY[:3] + _BODY[4:]), "failed the block"),
    "'=' followed by a character": (_block(b"QUJDQQ=A\n"), "failed the block"),
    "'=' followed by a character on the next line": (_block(b"QUJDQQ=\nA\n"), "failed the block"),
    "three '='": (_block(b"QUJDQ===\n"), "failed the block"),
    "four '='": (_block(b"QUJD====\n"), "failed the block"),
    "'=' only, a mark block full": (_block(b"=" * 2048 + b"\n"), "failed the block"),
    "an unpadded last quantum": (_block(b"QUJDQUI\n"), "failed the block"),
    "a character before the block": (b"QUJD\n" + GOOD, "skipped the junk"),
    "a character behind the block": (GOOD + b"QUJD\n", "skipped the junk"),
    "'=' at the start of a body": (_block(b"=UJD\n"), "failed the block"),
    "the literal repeated": (_block(_BODY, begin=b"-----BEGIN CERTIFICATE-----BEGIN CERTIFICATE-----"), "skipped the junk"),
    "BEGIN spelled short": (_block(_BODY, begin=b"-----BEGIN CERTIFICAT-----"), "skipped the junk"),
}
# cut short, a file ends inside its last block: nothing may stand behind it in that file
TRUNCATIONS = {
    "inside a body": GOOD[:60],
    "inside BEGIN": GOOD[:20],
    "behind BEGIN's dashes": GOOD[:27],
    "inside END": GOOD[:-10],
}
PLACES = ("first", "middle", "last")


def place(bad, file_at, block_at, truncated=False):
    """three files of three blocks, `bad` in the place of one block → (files, the number of its file)"""
    f = PLACES.index(file_at)
    k = 2 if truncated else PLACES.index(block_at)
    files = []
    for i in range(3):
        blocks = [pt.write_block(content("random", 40 + 10 * i + j, 10 * i + j), (64, 76, 4)[j]) for j in range(3)]
        if i == f:
            blocks[k] = bad
        files.append(b"".join(blocks))
    return files, f
