"""ct_mapreduce_amd.get_entries, the CPU twin of ctmr_entries_json* (include/ctmr.h): against Python's
json + base64 on every accepted text, on the committed raw-entry fixture in every style, on every rejection — and the
builders of tests/get_entries_corpus.py held to the coverage the GPU tests rely on.  No GPU."""
import base64
import hashlib
import json
import os

import numpy as np
import pytest

from ct_mapreduce_amd import get_entries as ge
from ct_mapreduce_amd._entry_host import certificate_of
from tests import get_entries_corpus as gc

HERE = os.path.dirname(os.path.abspath(__file__))


def python_parse(bodies):
    parts, bounds, first = [], [0], [0]
    for b in bodies:
        for e in json.loads(b)["entries"]:
            for k in ("leaf_input", "extra_data"):
                parts.append(base64.b64decode(e[k]))
                bounds.append(bounds[-1] + len(parts[-1]))
        first.append((len(bounds) - 1) // 2)
    return b"".join(parts), np.asarray(bounds, np.uint64), np.asarray(first, np.uint64)


def same(a, b):
    return a[0] == b[0] and (a[1] == b[1]).all() and (a[2] == b[2]).all()


def accepted_texts():
    for kind in gc.CONTENTS:
        for style in ge.STYLES:
            yield ge.write(gc.length_entries(kind), 64, style)
        yield ge.write(gc.tile_entries(kind), 3)
    yield ge.write(gc.sextet_entries(), 2, "alternate")
    yield [gc.spare_bits_body()]
    yield [b'{"entries":[]}', b' {\n"entries" : [ ] } \r\n', ge.write_one(gc.small_entries(2)), b'{"entries":[]}']
    yield []
    e, _ = gc.one_entry_110()
    for g, w, body in gc.gap_bodies(e, widths=(0, 1, 5, 70)):
        yield [body]


def test_twin_against_python_on_every_accepted_text():
    n = 0
    for bodies in accepted_texts():
        assert same(ge.parse(bodies), python_parse(bodies)), bodies[:1]
        n += 1
    assert n > 90
    assert ge.parse([gc.spare_bits_body()])[0] == b"ABA\xff\xef\xfb"


def test_writer_styles_are_what_they_say():
    es = gc.small_entries(5)
    doc = {"entries": [{"leaf_input": base64.b64encode(a).decode(), "extra_data": base64.b64encode(b).decode()} for a, b in es]}
    assert ge.write_one(es).decode() == json.dumps(doc, separators=(",", ":"))
    assert ge.write_one(es, "indent").decode() == json.dumps(doc, indent=2)
    assert ge.write_one([], "indent") == b'{\n  "entries": []\n}'
    assert ge.write_one(es, "swapped").count(b'{"extra_data"') == 5 and ge.write_one(es, "alternate").count(b'{"extra_data"') == 2
    assert [len(json.loads(b)["entries"]) for b in ge.write(es, [0, 2, 0, 3, 0])] == [0, 2, 0, 3, 0]
    assert ge.b64_encode(b"\xfb\xff\xfe") == b"+//+" and all(ge.b64_encode(bytes(k)) == base64.b64encode(bytes(k)) for k in range(9))


def test_golden_fixture_in_every_style():
    fx = json.load(open(os.path.join(HERE, "golden", "entries_from_reference_pems.json")))
    pairs = [(base64.b64decode(e["leaf_input"]), base64.b64decode(e["extra_data"])) for e in fx["entries"]]
    want = b"".join(a + b for a, b in pairs)
    for style in ge.STYLES:
        for per in (1, 3, len(pairs)):
            blob, bounds, first = ge.parse(ge.write(pairs, per, style))
            assert blob == want and len(bounds) == 2 * len(pairs) + 1
            for i, e in enumerate(fx["entries"]):
                leaf = blob[int(bounds[2 * i]):int(bounds[2 * i + 1])]
                extra = blob[int(bounds[2 * i + 1]):int(bounds[2 * i + 2])]
                assert (leaf, extra) == pairs[i]
                if e.get("cert_sha256"):
                    assert hashlib.sha256(certificate_of(leaf, extra)).hexdigest() == e["cert_sha256"], e["name"]
    assert any(e.get("cert_sha256") for e in fx["entries"])


@pytest.mark.parametrize("rej", gc.REJECTIONS, ids=lambda r: r["name"])
def test_every_rejection_names_the_lowest_bad_response(rej):
    for bodies, bad in gc.rejection_cases(rej):
        with pytest.raises(ge.GetEntriesError) as x:
            ge.parse(bodies)
        assert x.value.bad_response == bad
        lo = sum(len(b) for b in bodies[:bad])
        assert lo <= x.value.offset < lo + len(bodies[bad])
        # the documented host-fallback class: what Python's json and a lenient host would have taken
        assert gc.lenient_host_accepts(bodies[bad]) == rej["host_accepts"], rej["name"]
        ge.parse(bodies[:bad])   # the bodies in front are inside the grammar


def test_bodies_rejected_as_they_stand_and_a_string_across_a_boundary():
    good = ge.write_one(gc.small_entries(2))
    for name, body in gc.BAD_BODIES:
        for r in (0, 1, 2):
            bodies = [good, good, good]
            bodies[r] = body
            with pytest.raises(ge.GetEntriesError) as x:
                ge.parse(bodies)
            assert x.value.bad_response == r, name
            assert not gc.lenient_host_accepts(body), name
    pair, entries = gc.split_string_pair()
    assert ge.parse([b"".join(pair)])[0] == b"".join(a + b for a, b in entries)
    with pytest.raises(ge.GetEntriesError) as x:
        ge.parse([good] + pair)
    assert x.value.bad_response == 1
    assert sorted(r["name"] for r in gc.REJECTIONS if r["host_accepts"]) == ["escaped solidus", "first key in another case", "key in another case",
                                                                             "unknown third key"]


def test_the_builders_cover_what_the_gpu_tests_rely_on():
    # every decoded length mod 3, in both members, with both pads
    for kind in ("random",):
        es = gc.length_entries(kind)
        assert {(len(a) % 3, len(b) % 3) for a, b in es} >= {(0, 2), (1, 1), (2, 0), (0, 1), (1, 2), (2, 0)}
        assert {len(a) for a, _ in es} == set(range(201)) == {len(b) for _, b in es}
        text = ge.write_one(es)
        assert text.count(b'=="') > 100 and text.count(b'="') - text.count(b'=="') > 100
    ls = {len(a) for a, _ in gc.tile_entries("zero")}
    assert ls == {m * 768 + d for m in (1, 2) for d in range(-2, 3)} and gc.TILE_OUT == 768
    # every sextet value at each of the four positions of a quantum
    seen = set()
    for a, b in gc.sextet_entries():
        for s in (ge.b64_encode(a), ge.b64_encode(b)):
            seen |= {(k & 3, c) for k, c in enumerate(s)}
    assert seen >= {(p, c) for p in range(4) for c in ge.ALPHABET}
    # every token byte of the 110-byte entry at every residue of the mark block, once leading ws of 0…BLOCK + 2 is put
    # in front: the body is shorter than the block, so the shifts move each of its bytes over every residue
    e, body = gc.one_entry_110()
    assert len(body) < gc.MARK_BLOCK
    marks = [k for k, c in enumerate(body) if c in b'{}[]:,"']
    assert len(marks) == 7 + 13   # quotes counted one by one: 5 + 2 of frame, 13 of the entry
    for k in marks:
        assert {(k + w) % gc.MARK_BLOCK for w in range(gc.MARK_BLOCK + 3)} == set(range(gc.MARK_BLOCK))
    # the gap builder reaches every gap, the one behind the closing brace included
    gaps = {g for g, w, _ in gc.gap_bodies(e, widths=(1,))}
    assert gaps == set(range(len(ge.tokens(e)) + 1))
