"""Every CRL judged on its own, without a GPU (include/ctmr.h ctmr_crl_probes_each): the CPU twin
ct_mapreduce_amd/crl.py probes_each against the strict twin over the good CRLs and against the offsets tests/crl_corpus.py
worked out from how it put the bytes together; and the pass model of tests/test_crl_corpus_cpu.py with a finding per CRL
— candidates with their frames, cuts, conflict regions, then the chain check blaming the CRL of the token that does not
reach the next one — against the sequential parse of each CRL, over generated and damaged CRLs laid several to a blob.
tests/test_gpu_crl_each.py holds the library to this twin."""
import ctypes as C

import numpy as np
import pytest

from ct_mapreduce_amd import crl as CRL, known_image as KI, _native as N
from tests import crl_corpus as CC
from tests import test_crl_corpus_cpu as MODEL

DG = CC.DIGESTS
NONE = CRL.NONE
REJ = {nm: (c, off) for nm, c, off in CC.rejections()}


def good_four():
    """Four good CRLs and their digests: two shards of one digest (the second with a serial above 40 octets), a CRL
    without entries, and one of another issuer."""
    a = [CC.serial_of(k, 12) for k in range(3)]
    b = [CC.serial_of(20 + k, 9) for k in range(2)] + [b"\x42" * 41]
    return ([CC.crl([CC.entry(s) for s in a]), CC.crl(None), CC.crl([CC.entry(s) for s in b]), CC.small_crl()],
            [DG[1], DG[2], DG[1], DG[3]])


def five(c, k, digest=DG[1]):
    """The good four with c as CRL k → (crls, digests)"""
    crls, digests = good_four()
    return crls[:k] + [c] + crls[k:], digests[:k] + [digest] + digests[k:]


def long_then_broken():
    """A CRL with a 41-octet serial, a short one, and then the start of an entry that says 3 octets and has 2 → (the CRL,
    the offset of that start)"""
    es = [CC.entry(b"\x42" * 41), CC.entry(b"\x07"), b"\x30\x03\x02\x01"]
    c, lo = CC.crl_at(es)
    return c, lo + len(es[0]) + len(es[1])


def starts(crls):
    return [sum(len(c) for c in crls[:k]) for k in range(len(crls))]


def identities(crls, image, info, verdicts):
    """What the header promises of the counts, whatever the CRLs hold."""
    im = KI._HEADER.unpack_from(image, 0)
    assert len(verdicts) == len(crls) == info["crls"]
    assert sum(v[1] for v in verdicts) == im[6] == info["records"]
    assert sum(v[1] + v[2] for v in verdicts) == info["entries"]
    bad = [k for k, v in enumerate(verdicts) if v[0] != NONE]
    assert all(verdicts[k][1:] == (0, 0) for k in bad)
    assert (info["bad_crl"], info["bad_offset"]) == ((bad[0], verdicts[bad[0]][0]) if bad else (NONE, NONE))
    at = starts(crls)
    assert all(at[k] <= verdicts[k][0] <= at[k] + len(crls[k]) for k in bad)


def judged(crls, digests, bad):
    """probes_each of the CRLs, of which `bad` = {index: offset inside that CRL} are outside the grammar: the image is the
    strict twin's over the others, the verdicts name the offsets → (image, info, verdicts)"""
    image, info, verdicts = CRL.probes_each(crls, digests)
    keep = [k for k in range(len(crls)) if k not in bad]
    want, winfo = CRL.probes_parts([crls[k] for k in keep], [digests[k] for k in keep])
    assert image == want
    at = starts(crls)
    assert [v[0] for v in verdicts] == [at[k] + bad[k] if k in bad else NONE for k in range(len(crls))]
    for f in ("entries", "records", "host_members", "empty_crls"):
        assert info[f] == winfo[f], f
    identities(crls, image, info, verdicts)
    return image, info, verdicts


def test_the_struct():
    assert C.sizeof(N.CrlVerdict) == 16
    assert (N.CrlVerdict.bad_offset.offset, N.CrlVerdict.records.offset, N.CrlVerdict.long_entries.offset) == (0, 8, 12)


@pytest.mark.parametrize("case", CC.good_cases(), ids=[c[0] for c in CC.good_cases()])
def test_with_nothing_bad_it_is_the_strict_twin(case):
    nm, crls, digests, serials = case
    image, info, verdicts = CRL.probes_each(crls, digests)
    assert (image, info) == CRL.probes_parts(crls, digests)
    assert verdicts == [(NONE, sum(len(s) <= 40 for s in ss), sum(len(s) > 40 for s in ss)) for ss in serials]
    identities(crls, image, info, verdicts)


def test_no_crls():
    assert CRL.probes_each([], []) == CRL.probes_parts([], []) + ([],)


@pytest.mark.parametrize("case", CC.rejections(), ids=[c[0] for c in CC.rejections()])
def test_a_rejection_as_the_first_a_middle_and_the_last_of_five(case):
    nm, c, offset = case
    four = CRL.probes_image(*good_four())
    for k in (0, 2, 4):
        crls, digests = five(c, k)
        image, info, verdicts = judged(crls, digests, {k: offset})
        assert image == four and info["bad_crl"] == k


def test_two_bad_and_all_five_bad():
    head, ent, short = REJ["tag 31 for signature"], REJ["a fourth TLV in an entry"], REJ["entry2 one byte short"]
    crls, digests = good_four()
    crls, digests = [crls[0], head[0], crls[1], ent[0], crls[2]], [DG[1], DG[4], DG[2], DG[1], DG[1]]
    _, info, verdicts = judged(crls, digests, {1: head[1], 3: ent[1]})
    assert info["bad_crl"] == 1 and verdicts[4][1:] == (2, 1)
    _, info, _ = judged([ent[0], crls[0], head[0]], DG[:3], {0: ent[1], 2: head[1]})
    assert info["bad_crl"] == 0
    bad = [head, ent, short, (b"", 0), REJ["a byte behind the CertificateList"]]
    image, info, verdicts = judged([c for c, _ in bad], DG[:5], {k: off for k, (_, off) in enumerate(bad)})
    assert image == KI.build({}) and info["entries"] == 0 and info["empty_crls"] == 0


def test_a_digest_whose_every_crl_is_bad_is_no_issuer_and_a_bad_shard_leaves_the_others_in_order():
    a, b = CC.reversed_pair()
    ent = REJ["entry1 one byte long"]
    sa = [CC.serial_of(k, 12) for k in range(4)]
    crls = [CC.crl([CC.entry(s) for s in sa[:2]]), ent[0], CC.crl([CC.entry(s) for s in sa[2:]]), ent[0]]
    image, _, _ = judged(crls, [a, a, a, b], {1: ent[1], 3: ent[1]})
    assert KI.parse(image).issuers == [a] and [m for _, m in KI.records(image)[0]] == sa
    # a long serial of a bad CRL is not in the host section: the CRL is broken behind it
    long, at = long_then_broken()
    image, info, _ = judged([crls[0], long], [a, b], {1: at})
    assert KI.records(image)[1] == [] and info["host_members"] == 0


ZERO_SHAPES = {"first": [0], "in the middle": [2], "last": [4], "two adjacent": [1, 2], "two adjacent at the end": [4, 5], "alone": None}


@pytest.mark.parametrize("shape", list(ZERO_SHAPES), ids=list(ZERO_SHAPES))
def test_crls_of_0_bytes(shape):
    if ZERO_SHAPES[shape] is None:
        for n in (1, 3):
            image, info, verdicts = judged([b""] * n, DG[:n], {k: 0 for k in range(n)})
            assert image == KI.build({}) and verdicts == [(0, 0, 0)] * n
        return
    crls, digests = good_four()
    for k in ZERO_SHAPES[shape]:
        crls, digests = crls[:k] + [b""] + crls[k:], digests[:k] + [DG[1]] + digests[k:]
    image, _, verdicts = judged(crls, digests, {k: 0 for k in ZERO_SHAPES[shape]})
    assert image == CRL.probes_image(*good_four())
    at = starts(crls)
    assert all(verdicts[k][0] == at[k] for k in ZERO_SHAPES[shape])


# ---- the passes, modelled with a finding per CRL (kernels/crl.h k_crl_head<true>, k_crl_chain)

def layout_each(crls):
    """→ (blob, [(start, lo, hi, end)] per CRL, {CRL: the head's finding}): a CRL the head refuses is one frame over
    all its bytes (lo == hi == end); a CRL of 0 bytes holds no byte."""
    blob, out, bad, at = b"".join(crls), [], {}, 0
    for k, c in enumerate(crls):
        try:
            lo, hi = CRL.head(c)
        except CRL.CrlError as x:
            lo = hi = len(c)
            bad[k] = at + x.offset
        out.append((at, at + lo, at + hi, at + len(c)))
        at += len(c)
    return blob, out, bad


def candidates_each(blob, spans):
    """MODEL.candidates with the head-refused and the empty CRLs: a frame is a candidate where it has a byte to start
    at (k_crl_candidate: front = i == s0, behind = i == hi < e)."""
    out = []
    for s, lo, hi, e in spans:
        if s == e:
            continue
        out.append((s, lo))
        for i in range(lo, hi):
            got = CRL.entry(blob, i, hi)
            if got:
                out.append((i, got[0]))
        if hi < e:
            out.append((hi, e))
    return out


def kept(cand):
    """The candidates the cuts and the conflict regions keep (MODEL.parallel_tokens, up to the chain check)."""
    pos, nxt = [c for c, _ in cand], [n for _, n in cand]
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
    return [cand[k] for k in range(len(cand)) if keep[k]]


def crl_of(spans, i):
    """The last CRL that starts at or before byte i (kernels/crl.h crl_of)."""
    return max(k for k, sp in enumerate(spans) if sp[0] <= i)


def parallel_findings(blob, spans, head_bad):
    """→ {CRL: offset}: the head's findings, and per CRL the smallest nxt that is not the next kept position."""
    toks = kept(candidates_each(blob, spans))
    assert toks and toks[0][0] == 0
    bad = dict(head_bad)
    for (p, n), after in zip(toks, [t[0] for t in toks[1:]] + [len(blob)]):
        if n != after:
            k = crl_of(spans, p)
            assert k not in head_bad                                             # a refused CRL is one frame: it cannot break
            bad[k] = min(bad.get(k, n), n)
    return bad


def sequential_findings(crls):
    out, at = {}, 0
    for k, c in enumerate(crls):
        try:
            CRL.entries(c)
        except CRL.CrlError as x:
            out[k] = at + x.offset
        at += len(c)
    return out


def test_the_model_on_every_rejection_between_good_crls_and_next_to_0_bytes():
    for nm, c, offset in CC.rejections():
        for k in (0, 2, 4):
            crls, _ = five(c, k)
            crls = crls + [b""] if k == 2 else [b""] + crls if k == 4 else crls
            blob, spans, head_bad = layout_each(crls)
            want = sequential_findings(crls)
            assert parallel_findings(blob, spans, head_bad) == want, nm
            j = k + (k == 4)
            assert want[j] == starts(crls)[j] + offset and len(want) == 1 + (k != 0), nm


def test_the_model_finds_each_crls_sequential_failure_on_crls_made_to_fool_it():
    rng = np.random.default_rng(27)
    rejected = [c for _, c, _ in CC.rejections()]
    two_bad = broken = 0
    for n in range(500):                                                         # 2 000 generated CRLs, four to a blob, …
        crls = [MODEL.fooling_crl(rng)[0] for _ in range(4)]
        if n % 3 == 0:                                                           # … a head-refused or an empty one among them
            crls.insert(int(rng.integers(0, 5)), rejected[int(rng.integers(0, len(rejected)))] if n % 2 else b"")
        blob, spans, head_bad = layout_each(crls)
        # damaged inside two values: the heads stay what they were
        values = [(lo, hi) for _, lo, hi, _ in spans if hi > lo]
        hurt = bytearray(blob)
        for j in rng.choice(len(values), size=2, replace=False):
            lo, hi = values[int(j)]
            i = int(rng.integers(lo, hi))
            hurt[i] = (hurt[i] + int(rng.integers(1, 256))) % 256 if n % 2 else int(rng.choice([0x30, 0x02, 0x17, 0x00, 0x04]))
        hurt = bytes(hurt)
        parts = [hurt[sp[0]:sp[3]] for sp in spans]
        want = sequential_findings(parts)
        assert parallel_findings(hurt, spans, head_bad) == want
        image, info, verdicts = CRL.probes_each(parts, [DG[k % 3] for k in range(len(parts))])
        assert {k: v[0] for k, v in enumerate(verdicts) if v[0] != NONE} == want
        identities(parts, image, info, verdicts)
        inside = [k for k in want if k not in head_bad]
        broken += len(inside) > 0
        two_bad += len(inside) > 1
    assert broken > 150 and two_bad > 20                                         # (the generator does its job)
