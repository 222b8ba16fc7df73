"""DER CRLs → a probe image without a GPU (include/ctmr.h ctmr_crl_probes): the CPU twin
ct_mapreduce_amd/crl.py against the plain lists and offsets of tests/crl_corpus.py, against the functions that were there
before it — known_image.probes, union, parse, records —, against OpenSSL where OpenSSL can be a judge, and on a CRL that
`openssl ca -gencrl` made; and a Python model of the parallel entry search the kernels run (candidates with their frames,
cuts, conflict regions, the chain check) against the sequential parse on CRLs made to fool it.
tests/test_gpu_crl_probes.py takes its cases from the same corpus."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from ct_mapreduce_amd import crl as CRL, known_image as KI
from tests import crl_corpus as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DG = CC.DIGESTS


def fake_crls():
    return [(nm, CC.crl([CC.spec_entry(*x) for x in spec]), [x[0] for x in spec]) for nm, spec, _, _ in CC.fake_cases()]


# ---- 1. the twin against the corpus's lists

@pytest.mark.parametrize("case", CC.good_cases(), ids=[c[0] for c in CC.good_cases()])
def test_the_twin_reads_what_the_corpus_wrote(case):
    nm, crls, digests, serials = case
    assert [CRL.entries(c) for c in crls] == serials
    img, info = CRL.probes_parts(crls, digests)
    im = KI.parse(img)
    by = {}
    for d, ss in zip(digests, serials):
        by.setdefault(d, []).extend(ss)
    assert KI.union(img) == KI.probes({d: ss for d, ss in by.items()})
    dev, host = KI.records(img)
    for d, ss in by.items():                                                      # input order, repeats kept; above 40: sorted, each once
        assert [m for k, m in dev if k == KI.set_key(0, d)] == [s for s in ss if len(s) <= 40]
        assert [m for k, m in host if k == KI.set_key(0, d)] == sorted({s for s in ss if len(s) > 40})
    assert [KI.parse_key(k)[1] for k in dict.fromkeys(k for k, _ in dev)] == sorted({d for d, ss in by.items() if any(len(s) <= 40 for s in ss)},
                                                                                   key=KI.issuer_id)
    assert im.issuers == sorted(d for d, ss in by.items() if any(len(s) <= 40 for s in ss))
    n = sum(len(ss) for ss in serials)
    assert info == dict(crls=len(crls), entries=n, records=len(dev), host_members=len(host), empty_crls=sum(not ss for ss in serials),
                        bad_crl=CRL.NONE, bad_offset=CRL.NONE)


def test_fake_entries_are_candidates_and_are_not_read():
    for (nm, spec, start, end), (_, c, serials) in zip(CC.fake_cases(), fake_crls()):
        es = [CC.spec_entry(*x) for x in spec]
        _, lo = CC.crl_at(es)
        got = CRL.entry(c, lo + start, lo + sum(map(len, es)))
        assert (got[0] - lo if got else None) == end, nm
        assert CRL.entries(c) == serials, nm
        assert KI.union(CRL.probes_image([c, c], [DG[0], DG[0]])) == KI.probes({DG[0]: serials})
    for nm, c, serials in CC.fake_crl_inside():
        assert CRL.entries(c) == serials, nm


def test_digests_whose_ids_sort_the_other_way_and_shards():
    a, b = CC.reversed_pair()
    assert a < b and KI.issuer_id(a) > KI.issuer_id(b)
    crls = [CC.crl([CC.entry(b"\x01"), CC.entry(b"\x02" * 41)]), CC.crl([CC.entry(b"\x03")]), CC.crl([CC.entry(b"\x01"), CC.entry(b"\x02" * 41)])]
    img = CRL.probes_image(crls, [a, b, a])
    assert KI.parse(img).issuers == [a, b]
    assert KI.records(img) == ([(KI.set_key(0, b), b"\x03"), (KI.set_key(0, a), b"\x01"), (KI.set_key(0, a), b"\x01")],
                               [(KI.set_key(0, a), b"\x02" * 41)])
    assert CRL.probes_image([], []) == KI.build({})
    hits, host_hits = KI.find(KI.build({KI.set_key(500000, a): [b"\x01", b"\x02" * 41], KI.set_key(500001, b): [b"\x04"]}), img, 0)
    assert hits["records"].tolist() == [0, 1, 1] and host_hits["records"].tolist() == [1]


# ---- 2. rejections: the CRL and the offset

@pytest.mark.parametrize("case", CC.rejections(), ids=[c[0] for c in CC.rejections()])
def test_rejections(case):
    nm, c, offset = case
    with pytest.raises(CRL.CrlError) as x:
        CRL.entries(c)
    assert x.value.offset == offset
    lead = [CC.small_crl(), CC.crl(None)]
    with pytest.raises(CRL.CrlError) as x:
        CRL.probes_image(lead + [c], DG[:3])
    assert (x.value.crl, x.value.offset) == (2, len(lead[0]) + len(lead[1]) + offset)
    with pytest.raises(CRL.CrlError) as x:                                       # the lowest CRL is named
        CRL.probes_image([c] + lead + [c], DG[:4])
    assert (x.value.crl, x.value.offset) == (0, offset)


def test_every_proper_prefix_a_slice_of_no_bytes_and_the_offsets():
    c = CC.small_crl()
    assert CRL.entries(c) == CC.SMALL_SERIALS
    for n in range(len(c)):
        with pytest.raises(CRL.CrlError) as x:
            CRL.entries(c[:n])
        assert x.value.offset == 0
    with pytest.raises(CRL.CrlError) as x:
        CRL.probes_image([c, b"", c], DG[:3])
    assert (x.value.crl, x.value.offset) == (1, len(c))
    A = len(c)
    assert CRL.check_offsets([0, A, 2 * A], 2, 2 * A) is None and CRL.check_offsets([0], 0, 0) is None
    assert CRL.check_offsets([1, A, 2 * A], 2, 2 * A) == (0, 0)
    assert CRL.check_offsets([0, A + 1, A], 2, A) == (1, A + 1)
    assert CRL.check_offsets([0, A, 2 * A - 1], 2, 2 * A) == (2, 2 * A) and CRL.check_offsets([0], 0, 5) == (0, 5)


# ---- 3. the parallel entry search (kernels/crl.h + kernels/resp_parse.h), modelled: it finds the sequential parse or
# fails where the sequential parse fails

def layout(crls):
    """→ (blob, [(start, lo, hi, end)] per CRL): the heads walked (the model is about what lies inside the values)."""
    blob, out, at = b"".join(crls), [], 0
    for c in crls:
        lo, hi = CRL.head(c)
        out.append((at, at + lo, at + hi, at + len(c)))
        at += len(c)
    return blob, out


def candidates(blob, spans):
    """[(position, next)] of every candidate, ascending: the two frames of each CRL and every well-formed entry inside
    its value that ends inside it."""
    out = []
    for s, lo, hi, e in spans:
        out.append((s, lo))
        for i in range(lo, hi):
            got = CRL.entry(blob, i, hi)
            if got:
                out.append((i, got[0]))
        out.append((hi, e))
    return out


def parallel_tokens(cand, length):
    """→ (the kept positions, None) after cuts and conflict regions, or (None, the smallest offset the chain check
    reports)."""
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
    assert toks and pos[toks[0]] == 0
    bad = [nxt[a] for a, c in zip(toks, toks[1:] + [None]) if nxt[a] != (length if c is None else pos[c])]
    return (None, min(bad)) if bad else ([pos[k] for k in toks], None)


def sequential_tokens(blob, spans):
    out = []
    for s, lo, hi, e in spans:
        out.append(s)
        p = lo
        while p < hi:
            got = CRL.entry(blob, p, hi)
            if not got:
                return None, p
            out.append(p)
            p = got[0]
        out.append(hi)
    return out, None


FRAGMENTS = [CC.SMALLEST, CC.SMALLEST, b"\x30", b"\x30\x04", b"\x02\x00", b"\x17\x00", b"\x18\x00", b"\x30\x06\x02\x02", b"\x30\x08\x02\x01\x41\x17\x03abc",
             b"\x30\x06\x02\x00\x17\x00\x30\x00", b"\x30\x0a\x02\x00\x18\x00\x30\x04", b"\x30\x05\x02\x00\x17\x01", b"\x30\x81\x80", b"\x30\x80",
             b"\x00", b"\xff", b"A", b"\x30\x0c\x02\x02", b"\x30\x14\x02\x0a", CC.entry(b"\x07\x08"), CC.entry(b"", ext=CC.REASON)]


def fooling_crl(rng):
    """A valid CRL whose serials and extension bodies are assembled from the fragments — many hold well-formed entries —,
    and in two of three with a fake header aimed at the end of a later entry."""
    def junk(n):
        return b"".join(FRAGMENTS[int(k)] for k in rng.integers(0, len(FRAGMENTS), size=n))
    spec = [[junk(int(rng.integers(0, 5))), junk(int(rng.integers(0, 4))) if rng.integers(0, 3) == 0 else None] for _ in range(int(rng.integers(1, 9)))]
    for _ in range(int(rng.integers(0, 3))):
        h = int(rng.integers(0, len(spec)))
        j = int(rng.integers(h, len(spec)))
        in_ext = spec[h][1] is not None and j > h and bool(rng.integers(0, 2))
        spec, _, _ = CC.with_fake(spec, h, j, in_ext=in_ext, pre=junk(int(rng.integers(0, 3))), post=junk(int(rng.integers(0, 3))))
    return CC.crl([CC.spec_entry(*x) for x in spec], next_update=bool(rng.integers(0, 2))), [x[0] for x in spec]


def test_the_parallel_search_finds_the_sequential_parse_on_crls_made_to_fool_it():
    rng = np.random.default_rng(26)
    fooled = broken = 0
    for n in range(1100):                                                        # 3 300 CRLs, three to a call
        made = [fooling_crl(rng) for _ in range(3)]
        crls = [c for c, _ in made]
        assert [CRL.entries(c) for c in crls] == [ss for _, ss in made]
        blob, spans = layout(crls)
        cand = candidates(blob, spans)
        want, _ = sequential_tokens(blob, spans)
        assert want is not None and len(want) == sum(len(ss) for _, ss in made) + 6
        got, _ = parallel_tokens(cand, len(blob))
        assert got == want
        fooled += len(cand) > len(want)
        # … and damaged inside a value: what passes the chain check is the sequential parse, what fails fails where it does
        values = [(lo, hi) for _, lo, hi, _ in spans if hi > lo]
        lo, hi = values[int(rng.integers(0, len(values)))]
        i = int(rng.integers(lo, hi))
        hurt = blob[:i] + bytes([(blob[i] + int(rng.integers(1, 256))) % 256 if n % 2 else rng.choice([0x30, 0x02, 0x17, 0x00, 0x04])]) + blob[i + 1:]
        got, want = parallel_tokens(candidates(hurt, spans), len(hurt)), sequential_tokens(hurt, spans)
        assert got == want
        broken += want[0] is None
    assert fooled > 800 and broken > 150                                         # (the generator does its job)


def test_a_twin_that_trusts_patterns_would_be_caught():
    """The corpus holds CRLs on which taking every well-formed entry for an entry gives other serials."""
    wrong = 0
    for nm, c, serials in fake_crls():
        lo, hi = CRL.head(c)
        by_pattern = [CRL.entry(c, i, hi)[1] for i in range(lo, hi) if CRL.entry(c, i, hi)]
        wrong += by_pattern != serials
    assert wrong >= 12


# ---- 4. OpenSSL as the judge, where it can be one

READER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <openssl/bn.h>
#include <openssl/x509.h>
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  unsigned char len4[4];
  if (!f) return 2;
  while (fread(len4, 1, 4, f) == 4) {
    long n = len4[0] | len4[1] << 8 | len4[2] << 16 | (long)len4[3] << 24;
    unsigned char* buf = malloc(n ? n : 1);
    if (fread(buf, 1, n, f) != (size_t)n) return 3;
    const unsigned char* p = buf;
    X509_CRL* crl = d2i_X509_CRL(NULL, &p, n);
    if (!crl || p != buf + n) { printf("fail\n"); free(buf); continue; }
    STACK_OF(X509_REVOKED)* rev = X509_CRL_get_REVOKED(crl);
    printf("crl %d\n", rev ? sk_X509_REVOKED_num(rev) : 0);
    for (int i = 0; rev && i < sk_X509_REVOKED_num(rev); i++) {
      BIGNUM* bn = ASN1_INTEGER_to_BN(X509_REVOKED_get0_serialNumber(sk_X509_REVOKED_value(rev, i)), NULL);
      char* hex = BN_bn2hex(bn);
      printf("%s\n", hex);
      OPENSSL_free(hex);
      BN_free(bn);
    }
    X509_CRL_free(crl);
    free(buf);
  }
  return 0;
}
"""


def minimal_and_positive(serials):
    return all(len(s) >= 1 and s[0] < 0x80 and not (len(s) > 1 and s[0] == 0 and s[1] < 0x80) for s in serials)


def openssl_cases():
    """The corpus CRLs OpenSSL reads as they are: serials minimal and positive, every extension a real one."""
    out = []
    for nm, crls, _, serials in CC.good_cases():
        if not nm.startswith("an entry of"):                                     # (those carry filler for an extension)
            out += [(nm, c, ss) for c, ss in zip(crls, serials) if minimal_and_positive(ss)]
    out += [(nm, c, ss) for nm, c, ss in fake_crls() if "extension body" not in nm and minimal_and_positive(ss)]
    return out


def test_openssl_reads_the_same_serials(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    src, exe, data = tmp_path / "crl_reader.c", tmp_path / "crl_reader", tmp_path / "crls.bin"
    src.write_text(READER)
    built = subprocess.run([cc, "-O1", "-o", str(exe), str(src), "-lcrypto"], capture_output=True, text=True)
    if built.returncode:
        pytest.skip("libcrypto cannot be linked: " + built.stderr.strip().splitlines()[-1][:200])
    cases = openssl_cases()
    real = open(os.path.join(ROOT, "tests", "golden", "crl", "openssl_ca_gencrl.der"), "rb").read()
    cases.append(("the fixture", real, CRL.entries(real)))
    assert len(cases) >= 25 and sum("in a serial" in nm or "region" in nm for nm, _, _ in cases) >= 6
    data.write_bytes(b"".join(struct.pack("<I", len(c)) + c for _, c, _ in cases))
    lines = subprocess.run([str(exe), str(data)], capture_output=True, text=True, check=True).stdout.split()
    at = 0
    for nm, c, serials in cases:
        assert lines[at] == "crl", (nm, lines[at])
        n = int(lines[at + 1])
        got = [int(x, 16) for x in lines[at + 2:at + 2 + n]]
        assert got == [int.from_bytes(s, "big") for s in serials], nm
        at += 2 + n
    assert at == len(lines)


# ---- 5. a CRL OpenSSL made

def test_the_crl_openssl_ca_gencrl_made():
    """tests/golden/crl/openssl_ca_gencrl.der: `openssl ca -gencrl` over an index of six revoked certificates and a valid
    one; two entries carry a reason code, one serial is itself a well-formed entry, two have a leading 00."""
    c = open(os.path.join(ROOT, "tests", "golden", "crl", "openssl_ca_gencrl.der"), "rb").read()
    want = [bytes.fromhex(x) for x in ("01", "7f", "0080", "300402001700", "3a5b7c9d1e2f30410203040506070809", "00fedcba9876543210fedcba9876543210fedc")]
    assert CRL.entries(c) == want
    lo, hi = CRL.head(c)
    assert sum(1 for i in range(lo, hi) if CRL.entry(c, i, hi)) == len(want) + 1       # the serial that is an entry
    assert KI.union(CRL.probes_image([c], [DG[0]])) == KI.probes({DG[0]: want})
