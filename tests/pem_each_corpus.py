"""PEM texts with several files outside the grammar, for ctmr_pem_decode_each* (include/ctmr.h): the builders
tests/test_pem_text_each_cpu.py holds to what they claim and tests/test_gpu_pem_decode_each.py runs on the device.  Each
bad file is one that a different pass of the device code finds: mark (a byte of no class), files (an odd number of armor
lines) or check (what lies between paired armor lines).  No GPU."""
from ct_mapreduce_amd import pem_text as pt
from tests import pem_text_corpus as pc

CLASSES = frozenset(pt.ALPHABET + b"=-" + pt.WS)       # every byte of a file the mark pass lets through has one of these

GOOD_REGULAR = pc.GOOD
GOOD_IRREGULAR = pc.with_gap(pc.content("random", 100, 31), "after 2nd", b" \t")
BAD_MARK = pc.REJECTIONS["a comment"][0]               # '#' and '"' have no class
BAD_FILES = pc.REJECTIONS["BEGIN without END"][0]      # one armor line
BAD_CHECK = pc.REJECTIONS["one character short"][0]    # paired armor lines, 135 characters between them
# what mark rejects although its armor lines are paired, and whose blocks would be irregular if the check looked at them
_IRR = pc.with_gap(pc.content("random", 103, 32), "after 1st", b"  ")
BAD_MARK_PAIRED_IRREGULAR = (_IRR[:40] + b"#" + _IRR[40:]) * 3
BADS = {"mark": BAD_MARK, "files": BAD_FILES, "check": BAD_CHECK}


def armor_lines(t):
    """the lines of t that begin with a dash"""
    return [ln for ln in bytes(t).split(b"\n") if ln.startswith(b"-")]


def found_by(t):
    """the first pass of the device code whose rule file t breaks, or None: "mark" — a byte of no class; "files" — an
    odd number of armor lines, each spelled right; "check" — armor lines spelled right and paired, and parse_one rejects it"""
    t = bytes(t)
    if any(c not in CLASSES for c in t):
        return "mark"
    lines = armor_lines(t)
    if any(ln.rstrip(pt.BLANK) not in (pt.BEGIN, pt.END) for ln in lines):
        return "mark"       # (a dash that is not of an armor line: the mark pass's as well)
    if len(lines) % 2:
        return "files"
    try:
        pt.parse_one(t)
    except Exception:
        return "check"
    return None


def several_bad():
    """name → (files, the numbers of the bad ones)"""
    g = [pt.write([pc.content("random", 50 + 7 * k, 40 + k) for k in range(2)], (64, 76, 4)[k % 3]) for k in range(6)]
    m, f, c = BAD_MARK, BAD_FILES, BAD_CHECK
    return {
        "adjacent": ([g[0], m, f, c, g[1]], [1, 2, 3]),
        "first and last": ([c, g[0], g[1], g[2], m], [0, 4]),
        "alternating": ([f, g[0], c, g[1], m, g[2], f, g[3]], [0, 2, 4, 6]),
        "all bad": ([m, f, c], [0, 1, 2]),
    }


def one_lane(boundary_at, xs=16, empties=True):
    """sixteen one-byte files b"x" back to back — with empty files between them — between two good files; the first good
    file is padded with ws so that the first x lies at text offset ≡ boundary_at (mod 1024) → (files, the bad ones)"""
    head = pc.GOOD
    head += b"\n" * ((boundary_at - len(head)) % 1024)
    files, bad = [head], []
    for k in range(xs):
        if empties and k % 3 == 1:
            files.append(b"")
        bad.append(len(files))
        files.append(b"x")
    files.append(pt.write_block(pc.content("random", 77, 5), 76, b"\r\n"))
    return files, bad


def one_block_files(F, bad_at):
    """F files of one block each, those in bad_at one character short"""
    return [BAD_CHECK if f in bad_at else pt.write_block(pc.content("random", 30 + f % 50, f), (64, 76)[f % 2], pc.EOLS[f % 2]) for f in range(F)]


def many_blocks(n, seed, bad=False):
    """a file of n blocks; bad: its last block is one character short"""
    t = pt.write([pc.content("random", 20 + (k * 7) % 40, seed + k) for k in range(n - 1 if bad else n)], 64)
    return t + BAD_CHECK if bad else t
