"""pem_text, the CPU twin of ctmr_pem_decode* (include/ctmr.h), against base64 and ssl; the corpus of
tests/pem_text_corpus.py held to its coverage.  No GPU."""
import base64
import os
import ssl

import numpy as np
import pytest

from ct_mapreduce_amd import pem_text as pt
from tests import pem_text_corpus as pc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def independent(files):
    """the DERs of accepted files by other means: split at the armor, ws stripped, base64.b64decode(validate=True)"""
    out = []
    for t in files:
        for part in bytes(t).split(pt.BEGIN)[1:]:
            body = part.split(pt.END)[0]
            out.append(base64.b64decode(b"".join(body.split()), validate=True))
    return out


def check_accepted(files):
    payload, offsets, file_first = pt.parse(files)
    ders = independent(files)
    assert payload == b"".join(ders)
    assert offsets.tolist() == [0] + np.cumsum([len(d) for d in ders]).tolist() if ders else offsets.tolist() == [0]
    assert file_first.tolist() == [0] + np.cumsum([bytes(t).count(pt.BEGIN) for t in files]).tolist()
    return ders


def all_accepted():
    fams = dict(pc.regular_files())
    fams.update(pc.irregular_files())
    fams["mixed"] = [pc.mixed_file()]
    return fams


@pytest.mark.parametrize("name", sorted(all_accepted()))
def test_the_twin_against_base64_and_ssl(name):
    files = all_accepted()[name]
    ders = check_accepted(files)
    assert ders
    for t in files:       # ssl reads one block: a file's first
        first = bytes(t)[:bytes(t).index(pt.END) + len(pt.END)].lstrip()
        if b"\r" not in first and name != "spare bits":   # (ssl wants its own armor lines exactly and no spare bits)
            assert ssl.PEM_cert_to_DER_cert(first.decode()) == independent([first])[0]


def test_layout_of_each_family():
    """regular families are all regular, irregular ones all irregular: both device paths are exercised"""
    for name, files in pc.regular_files().items():
        lay = pt.layout(files)
        assert lay and all(x[0] == "regular" for x in lay), name
    for name, files in pc.irregular_files().items():
        lay = pt.layout(files)
        assert lay and all(x == ("irregular",) for x in lay), name
    assert [x[0] for x in pt.layout([pc.mixed_file()])] == ["regular", "irregular", "regular"]
    assert pt.layout([pt.write([b"x" * 100, b"", b"y" * 10], 76, b"\r\n")]) == [("regular", 76, 2), ("regular", 0, 0), ("regular", 16, 2)]
    assert len(pc.irregular_files()) >= 7 + 8 and {"gap " + k for k in pc.GAP_KINDS} <= set(pc.irregular_files())


def test_the_corpus_covers_what_it_says():
    lens = {len(d) for d in pc.length_ders("zero")}
    assert set(range(201)) <= lens and {766, 767, 768, 769, 770, 1534, 1535, 1536, 1537, 1538} <= lens
    for p, d in enumerate(pc.sextet_ders()):
        chars = base64.b64encode(d)
        assert {chars[4 * q + p] for q in range(64)} == set(pt.ALPHABET)
    assert pt.parse([pc.SPARE_BITS_FILE])[0] == b"".join(pc.SPARE_BITS_DERS)
    for n in (0, 1, 5, 70):
        assert len(pc.ws_run(n, n)) == n and not pc.ws_run(n, n).strip(pt.WS)
    assert set(pc.ws_run(70, 1)) == set(pt.WS)


def test_ca_roots():
    from tests.test_real_certs_cpu import bundle_ders, CA_ROOTS
    text = open(CA_ROOTS, "rb").read()
    payload, offsets, first = pt.parse([text])
    assert len(offsets) - 1 == 161 and first.tolist() == [0, 161]
    ders = [payload[int(offsets[k]):int(offsets[k + 1])] for k in range(161)]
    assert list(dict.fromkeys(ders)) == bundle_ders()
    assert pt.layout([text]) == [("regular", 64, 1) if len(base64.b64encode(d)) > 64 else ("regular", len(base64.b64encode(d)), 1) for d in ders]
    assert sum(len(base64.b64encode(d)) % 64 != 0 for d in ders) == 149       # short last lines


def test_the_reference_pems(golden_certs):
    for name in ("kEmptySPKI", "kLeadingZeroes", "kRealSPKI"):
        text = open(os.path.join(GOLDEN, name + ".pem"), "rb").read()
        payload, offsets, _ = pt.parse([text])
        assert len(offsets) == 2 and payload == golden_certs[name], name


@pytest.mark.parametrize("eol", pc.EOLS)
@pytest.mark.parametrize("line", (4, 60, 64, 76, None))
def test_write_then_parse_is_the_identity(line, eol):
    ders = pc.length_ders("random")[:120] + pc.sextet_ders()
    files = [pt.write(ders[:50], line, eol), pt.write(ders[50:], line, eol, end_eol=b"")]
    payload, offsets, first = pt.parse(files)
    assert payload == b"".join(ders) and first.tolist() == [0, 50, len(ders)]
    assert [int(offsets[k + 1] - offsets[k]) for k in range(len(ders))] == [len(d) for d in ders]
    assert all(x[0] == "regular" and x[2] == (len(eol) if d else 0) for x, d in zip(pt.layout(files), ders))


def test_the_bound_on_certificates_at_its_equality_case():
    """certificates <= (text_bytes + F) / 54: blocks of no characters, each file's last one ending with the file"""
    for counts in ([1], [3], [2, 0, 5], [1, 1, 1, 1]):
        files = [pc.tightest_file(n) for n in counts]
        text, fb = pt.join(files)
        n = len(pt.parse(files)[1]) - 1
        F = sum(1 for c in counts if c)           # (a file of no bytes neither holds a block nor saves an LF)
        assert n == sum(counts) == (len(text) + F) // 54 and (len(text) + F) % 54 == 0
    for files in all_accepted().values():
        text, _ = pt.join(files)
        n = len(pt.parse(files)[1]) - 1
        assert n <= (len(text) + len(files)) // 54 and len(pt.parse(files)[0]) <= len(text) * 3 // 4


@pytest.mark.parametrize("name", sorted(pc.REJECTIONS))
def test_every_rejection_in_every_place(name):
    bad, go = pc.REJECTIONS[name]
    assert go.split(",")[0] in ("skipped the junk", "taken the header", "failed the block", "taken the block", "taken the inner block")
    for file_at in pc.PLACES:
        for block_at in pc.PLACES:
            files, f = pc.place(bad, file_at, block_at)
            with pytest.raises(pt.PemTextError) as err:
                pt.parse(files)
            _, fb = pt.join(files)
            assert err.value.bad_file == f and int(fb[f]) <= err.value.bad_offset < int(fb[f + 1]), (file_at, block_at)


@pytest.mark.parametrize("name", sorted(pc.TRUNCATIONS))
def test_a_file_that_ends_inside_a_block(name):
    for file_at in pc.PLACES:
        files, f = pc.place(pc.TRUNCATIONS[name], file_at, "last", truncated=True)
        with pytest.raises(pt.PemTextError) as err:
            pt.parse(files)
        assert err.value.bad_file == f
    # the files back to back would parse: the state starts afresh at every boundary
    whole = pc.GOOD
    assert len(pt.parse([whole])[1]) == 2
    with pytest.raises(pt.PemTextError):
        pt.parse([whole[:60], whole[60:]])


def test_empty_and_ws_only_files():
    good = pt.write([b"abc", b"de"])
    for files in ([], [b""], [b"", b" \n\t\r"], [b"", good, b"\n\n", good, b""], [good, b"   "]):
        payload, offsets, first = pt.parse(files)
        assert len(first) == len(files) + 1 and int(first[-1]) == len(offsets) - 1 == 2 * sum(1 for t in files if t == good)
