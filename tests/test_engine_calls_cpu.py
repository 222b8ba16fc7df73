"""What the host-memory wrappers of engine.py ask of the library, call by call, with a recording stand-in in the library's
place: the first guess of every wrapper that sizes, the one exact second call after CTMR_E_RANGE, no third call, the typed
errors, the warm state, the `bad` lists and the ticket book of the text waits.  No GPU and no built library: the
stand-in plays a script of (rc, what the call writes into the structs and arrays behind its arguments)."""
import ctypes as C
import struct

import numpy as np
import pytest

from ct_mapreduce_amd import _native as N
from ct_mapreduce_amd import crl, engine, known_image

NONE = 2**64 - 1
PAD = N.PAYLOAD_PAD


class Lib:
    """Every ctmr_* attribute is a callable that appends (name, args) to .log — a pointer argument as None (NULL) or
    "ptr", or the byte size of a ctypes array; a struct behind a byref as "&Name"; everything else as an int — and
    plays the next step scripted for its name: (rc, {struct class name, or argument position: {field: value}, a value
    for a plain byref, or bytes to lay down at that pointer}).  A call without a step returns 0 and writes nothing."""

    def __init__(self):
        self.log, self.steps = [], {}

    def script(self, name, *steps):
        self.steps.setdefault(name, []).extend(steps)

    def calls(self, name):
        return [args for n, args in self.log if n == name]

    def __getattr__(self, name):
        if not name.startswith("ctmr_"):
            raise AttributeError(name)
        argtypes = N.SIGNATURES[name][1]

        def fn(*args):
            assert len(args) == len(argtypes), (name, len(args))
            if name == "ctmr_last_error":
                return b"scripted"
            seen = []
            for a, t in zip(args, argtypes):
                if hasattr(a, "_obj"):
                    seen.append("&" + type(a._obj).__name__)
                elif t is C.c_void_p:
                    null = a is None or (isinstance(a, C.c_void_p) and not a.value) or (isinstance(a, int) and a == 0)
                    seen.append(None if null else C.sizeof(a) if isinstance(a, C.Array) else "ptr")
                elif t is C.c_char_p:
                    seen.append(None if a is None else "ptr")
                else:
                    seen.append(int(a))
            self.log.append((name, tuple(seen)))
            queue = self.steps.get(name)
            rc, writes = queue.pop(0) if queue else (0, {})
            for key, what in writes.items():
                if isinstance(key, str):
                    objs = [a._obj for a in args if hasattr(a, "_obj") and type(a._obj).__name__ == key]
                    assert len(objs) == 1, (name, key)
                    for f, v in what.items():
                        setattr(objs[0], f, v)
                elif isinstance(what, bytes):
                    a = args[key]
                    C.memmove(a if isinstance(a, int) else C.addressof(a), what, len(what))
                else:
                    args[key]._obj.value = what
            return rc
        return fn


@pytest.fixture
def rig(monkeypatch):
    lib = Lib()
    monkeypatch.setattr(N, "lib", lambda: lib)
    e = engine.Engine()
    assert lib.log.pop(0)[0] == "ctmr_create"
    return e, lib


def occupied(lib, n, times=1):
    lib.script("ctmr_table_info_get", *[(0, {"TableInfo": {"occupied": n}})] * times)


def image_header(sets=0, members=0, host_bytes=0, host_members=0, tail=0):
    """An image as far as the wrappers read it: the 64-byte header with these counts, `tail` bytes behind it."""
    return known_image._HEADER.pack(b"CTMRKNWN", 0, 0, 0, 0, sets, members, host_bytes, host_members, 0) + bytes(tail)


def u64s(*values):
    return struct.pack("<%dQ" % len(values), *values)


RANGE = N.E_RANGE


# ---- the wrappers that guess first and ask a second time only after CTMR_E_RANGE.  Each case: (the call, the library
# function, the positions of its caps, the first caps, the struct the sizes come back in, what a short first call reports,
# the caps of the second call, what the final info says, a check of the result)

IMAGE = image_header(sets=3, members=5, host_bytes=40, host_members=2, tail=500)
CRLS = [b"\x30" * 40, b"\x30" * 33, b""]
DIGESTS = [bytes([k]) * 32 for k in range(3)]


def guess_cases():
    def known_export(e, lib):
        occupied(lib, 7)
        return e.known_export()

    def known_lists_raw(e, lib):
        occupied(lib, 7)
        return e.known_lists_raw(1234)
    yield ("known_export", known_export, "ctmr_known_export", (2,), (65536 + 48 * 7,), "KnownImageInfo",
           {"meta_bytes": 70000, "members": 9}, (70000 + 48 * 9,), {"image_bytes": 300}, lambda r: len(r) == 300)
    yield ("known_export_floors", known_export, "ctmr_known_export", (2,), (65536 + 48 * 7,), "KnownImageInfo",
           {"meta_bytes": 10, "members": 0}, (64 + 48,), {"image_bytes": 64}, lambda r: len(r) == 64)
    yield ("known_lists_raw", known_lists_raw, "ctmr_known_lists", (3, 5, 7), (81 * 7 + 4096, 4096, 256), "KnownListsInfo",
           {"text_bytes": 9000, "ids_bytes": 5000, "issuers": 200}, (9000, 5000, 402),
           {"text_bytes": 100, "ids_bytes": 88, "issuers": 2, "members": 1},
           lambda r: (len(r[0]), len(r[1]), len(r[2]), len(r[3])) == (100, 88, 3, 3))
    yield ("known_image_lists_raw", lambda e, lib: e.known_image_lists_raw(IMAGE, 99), "ctmr_known_image_lists", (5, 7, 9),
           (81 * 5 + 2 * 40 + 1, 4096, 256), "KnownListsInfo", {"text_bytes": 300, "ids_bytes": 6000, "issuers": 150},
           (300, 6000, 302), {"text_bytes": 120, "ids_bytes": 44, "issuers": 1},
           lambda r: (len(r[0]), len(r[1]), len(r[2]), len(r[3])) == (120, 44, 2, 2))
    yield ("known_image_lists_raw_short_image", lambda e, lib: e.known_image_lists_raw(b"x" * 63, 99), "ctmr_known_image_lists",
           (5, 7, 9), (1, 4096, 256), "KnownListsInfo", {"text_bytes": 0, "ids_bytes": 0, "issuers": 0}, (0, 0, 2),
           {"text_bytes": 0, "ids_bytes": 0, "issuers": 0}, lambda r: (len(r[0]), len(r[1]), len(r[2])) == (0, 0, 1))
    yield ("known_merge", lambda e, lib: e.known_merge(N.KNOWN_UNION, b"a" * 100, b"b" * 30), "ctmr_known_merge", (7,),
           (100 + 30 + 64,), "KnownImageInfo", {"image_bytes": 777}, (777,), {"image_bytes": 150}, lambda r: len(r) == 150)
    yield ("known_merge_b_none", lambda e, lib: e.known_merge(N.KNOWN_MINUS, b"a" * 100), "ctmr_known_merge", (5, 7),
           (0, 100 + 64,), "KnownImageInfo", {"image_bytes": 200}, (0, 200), {"image_bytes": 164}, lambda r: len(r) == 164)
    yield ("known_image_resp", lambda e, lib: e.known_image_resp(IMAGE, 2), "ctmr_known_image_resp", (3, 5),
           (2, known_image.resp_bound(5, 3, 40, 2, 2)), "KnownRespInfo", {"text_bytes": 5000}, (2, 5000), {"text_bytes": 1234},
           lambda r: len(r) == 1234)
    yield ("known_image_resp_per_0", lambda e, lib: e.known_image_resp(IMAGE, 0), "ctmr_known_image_resp", (3, 5),
           (0, known_image.resp_bound(5, 3, 40, 2, 1)), "KnownRespInfo", {"text_bytes": 5000}, (0, 5000), {"text_bytes": 0},
           lambda r: r == b"")
    yield ("known_resp_image", lambda e, lib: e.known_resp_image(b"*1\r\n" * 3), "ctmr_known_resp_image", (2, 4), (12, 65536),
           "KnownRespImageInfo", {"image_bytes": 70000}, (12, 70000), {"image_bytes": 64}, lambda r: len(r) == 64)
    for each in (False, True):
        name = "crl_probes_each" if each else "crl_probes"
        yield (name, lambda e, lib, name=name: getattr(e, name)(CRLS, DIGESTS), "ctmr_" + name, (2, 4, 7),
               (73, 3, 64 + 56 * 3 + 48 * (73 // 6)), "KnownImageInfo", {"image_bytes": 900}, (73, 3, 900), {"image_bytes": 256},
               lambda r, each=each: len(r[0]) == 256 and len(r) == (3 if each else 2))
        yield (name + "_floors", lambda e, lib, name=name: getattr(e, name)([], []), "ctmr_" + name, (2, 4, 7), (0, 0, 64),
               "KnownImageInfo", {"image_bytes": 8}, (0, 0, 64), {"image_bytes": 64}, lambda r: len(r[0]) == 64)


GUESS = list(guess_cases())
IDS = [c[0] for c in GUESS]


def caps_of(args, at):
    return tuple(args[k] for k in at)


@pytest.mark.parametrize("case", GUESS, ids=IDS)
def test_first_guess_fits_one_call(rig, case):
    e, lib = rig
    _, call, fn, at, first, info, _, _, final, good = case
    lib.script(fn, (0, {info: final}))
    assert good(call(e, lib))
    assert [caps_of(a, at) for a in lib.calls(fn)] == [first]


@pytest.mark.parametrize("case", GUESS, ids=IDS)
def test_short_guess_second_call_with_what_info_says(rig, case):
    e, lib = rig
    _, call, fn, at, first, info, short, second, final, good = case
    lib.script(fn, (RANGE, {info: short}), (0, {info: final}))
    assert good(call(e, lib))
    assert [caps_of(a, at) for a in lib.calls(fn)] == [first, second]


@pytest.mark.parametrize("case", GUESS, ids=IDS)
def test_short_twice_raises_without_a_third_call(rig, case):
    e, lib = rig
    _, call, fn, at, first, info, short, second, _, _ = case
    lib.script(fn, (RANGE, {info: short}), (RANGE, {info: short}), (0, {}))
    with pytest.raises(engine.CtmrError) as x:
        call(e, lib)
    assert x.value.code == RANGE and len(lib.calls(fn)) == 2


@pytest.mark.parametrize("case", GUESS, ids=IDS)
def test_another_failure_is_raised_after_one_call(rig, case):
    e, lib = rig
    _, call, fn, at, first, info, short, _, _, _ = case
    lib.script(fn, (N.E_NOMEM, {info: short}))
    with pytest.raises(engine.CtmrError) as x:
        call(e, lib)
    assert x.value.code == N.E_NOMEM and type(x.value) is engine.CtmrError and len(lib.calls(fn)) == 1


def test_what_the_pointers_of_a_guess_call_are(rig):
    e, lib = rig
    occupied(lib, 0)
    e.known_export()
    e.known_merge(N.KNOWN_UNION, b"a" * 64)
    e.crl_probes_each([b"\x30\x00"], [bytes(32)])
    e.crl_probes([b"\x30\x00"], [bytes(32)])
    assert lib.calls("ctmr_known_export") == [(None, "ptr", 65536 + 48, "&KnownImageInfo")]
    assert lib.calls("ctmr_known_merge") == [(None, N.KNOWN_UNION, "ptr", 64, None, 0, "ptr", 128, "&KnownImageInfo")]
    assert lib.calls("ctmr_crl_probes_each") == [(None, "ptr", 2, "ptr", 1, "ptr", "ptr", 120, "&KnownImageInfo", "&CrlInfo",
                                                  "&CrlVerdict_Array_1")]
    assert lib.calls("ctmr_crl_probes") == [(None, "ptr", 2, "ptr", 1, "ptr", "ptr", 120, "&KnownImageInfo", "&CrlInfo")]


# ---- warm state

def test_known_export_starts_from_the_larger_of_last_cap_and_info(rig):
    e, lib = rig
    occupied(lib, 2, times=4)
    sizes = lambda: [a[2] for a in lib.calls("ctmr_known_export")]
    lib.script("ctmr_known_export", (0, {"KnownImageInfo": {"meta_bytes": 100, "image_bytes": 196}}))
    e.known_export()                                     # the first guess stays: it was the larger
    lib.script("ctmr_known_export", (RANGE, {"KnownImageInfo": {"meta_bytes": 90000, "members": 2}}),
               (0, {"KnownImageInfo": {"meta_bytes": 90000, "image_bytes": 90096}}))
    e.known_export()
    lib.script("ctmr_known_export", (0, {"KnownImageInfo": {"meta_bytes": 95000, "image_bytes": 95096}}))
    e.known_export()                                     # (a call that fitted although info says more: info wins)
    e.known_export()
    assert sizes() == [65536 + 96, 65536 + 96, 90000 + 96, 90000 + 96, 95000 + 96]
    assert e._known_meta_cap == 95000


def test_known_lists_raw_starts_from_the_larger_of_last_caps_and_info(rig):
    e, lib = rig
    occupied(lib, 10, times=3)
    caps = lambda: [caps_of(a, (3, 5, 7)) for a in lib.calls("ctmr_known_lists")]
    lib.script("ctmr_known_lists", (RANGE, {"KnownListsInfo": {"text_bytes": 9000, "ids_bytes": 5000, "issuers": 200, "members": 10}}),
               (0, {"KnownListsInfo": {"text_bytes": 9000, "ids_bytes": 5000, "issuers": 200, "members": 10}}))
    e.known_lists_raw(0)
    lib.script("ctmr_known_lists", (0, {"KnownListsInfo": {"text_bytes": 700, "ids_bytes": 6000, "issuers": 3, "members": 8}}))
    e.known_lists_raw(0)
    e.known_lists_raw(0)
    host = 9000 - 81 * 10
    assert caps() == [(810 + 4096, 4096, 256), (9000, 5000, 402), (810 + host, 5000, 402), (810 + 4096, 6000, 402)]
    assert (e._known_lists_host, e._known_lists_ids, e._known_lists_offs) == (4096, 6000, 402)


def test_known_lists_raw_slices_ids_and_both_offset_halves(rig):
    e, lib = rig
    occupied(lib, 1)
    lib.script("ctmr_known_lists", (0, {"KnownListsInfo": {"text_bytes": 6, "ids_bytes": 4, "issuers": 2, "members": 1},
                                        2: b"abcdefgh", 4: b"IDidXX", 6: u64s(0, 2, 6, 0, 2, 4, 77)}))
    text, ids, toff, ioff, info = e.known_lists_raw(5)
    assert (text.tobytes(), ids, list(toff), list(ioff), info.issuers) == (b"abcdef", b"IDid", [0, 2, 6], [0, 2, 4], 2)
    assert lib.calls("ctmr_known_lists")[0][:2] == (None, 5)
    occupied(lib, 1)
    lib.script("ctmr_known_lists", (0, {"KnownListsInfo": {"text_bytes": 6, "ids_bytes": 4, "issuers": 2, "members": 1},
                                        2: b"abcdefgh", 4: b"IDidXX", 6: u64s(0, 2, 6, 0, 2, 4, 77)}))
    assert e.known_lists(5) == [(b"ID", b"ab"), (b"id", b"cdef")]
    lib.script("ctmr_known_image_lists", (0, {"KnownListsInfo": {"text_bytes": 6, "ids_bytes": 4, "issuers": 2},
                                              4: b"abcdefgh", 6: b"IDidXX", 8: u64s(0, 2, 6, 0, 2, 4, 77)}))
    assert e.known_image_lists(IMAGE, 5) == [(b"ID", b"ab"), (b"id", b"cdef")]


# ---- the typed errors: E_INVAL with the index set; a plain CtmrError with the index NONE

BODIES = [b"a" * 40, b"b" * 31, b""]
TEXT = 71


def test_crl_error_carries_index_and_offset(rig):
    e, lib = rig
    for each, fn in ((False, "ctmr_crl_probes"), (True, "ctmr_crl_probes_each")):
        call = e.crl_probes_each if each else e.crl_probes
        lib.script(fn, (N.E_INVAL, {"CrlInfo": {"bad_crl": 1, "bad_offset": 17}}))
        with pytest.raises(crl.CrlError) as x:
            call(CRLS, DIGESTS)
        assert (x.value.crl, x.value.offset, x.value.what) == (1, 17, "scripted")
        assert str(x.value) == "CRL 1, offset 17: scripted"
        lib.script(fn, (N.E_INVAL, {"CrlInfo": {"bad_crl": NONE, "bad_offset": 17}}))
        with pytest.raises(engine.CtmrError) as x:
            call(CRLS, DIGESTS)
        assert x.value.code == N.E_INVAL and str(x.value) == "ctmr error -1: scripted"
        lib.script(fn, (RANGE, {"KnownImageInfo": {"image_bytes": 2000}}), (N.E_INVAL, {"CrlInfo": {"bad_crl": 0, "bad_offset": 3}}))
        with pytest.raises(crl.CrlError) as x:
            call(CRLS, DIGESTS)
        assert (x.value.crl, x.value.offset) == (0, 3) and len(lib.calls(fn)) == 4


def test_entries_json_error_carries_index_and_offset(rig):
    e, lib = rig
    lib.script("ctmr_entries_json", (N.E_INVAL, {"EntriesJsonInfo": {"bad_response": 2, "bad_offset": 71}}))
    with pytest.raises(engine.EntriesJsonError) as x:
        e.entries_json(BODIES)
    assert (x.value.code, x.value.bad_response, x.value.bad_offset) == (N.E_INVAL, 2, 71)
    assert str(x.value) == "ctmr error -1: scripted"
    lib.script("ctmr_entries_json", (N.E_INVAL, {"EntriesJsonInfo": {"bad_response": NONE}}))
    with pytest.raises(engine.CtmrError) as x:
        e.entries_json(BODIES)
    assert type(x.value) is engine.CtmrError and x.value.code == N.E_INVAL
    lib.script("ctmr_entries_json", (N.E_NOMEM, {"EntriesJsonInfo": {"bad_response": 1}}))     # (the index alone makes no typed error)
    with pytest.raises(engine.CtmrError) as x:
        e.entries_json(BODIES)
    assert type(x.value) is engine.CtmrError and x.value.code == N.E_NOMEM
    lib.script("ctmr_entries_json_each", (N.E_INVAL, {"EntriesJsonInfo": {"bad_response": 2, "bad_offset": 71}}))
    with pytest.raises(engine.CtmrError) as x:
        e.entries_json_each(BODIES)                      # every body is judged alone: the call has no typed error
    assert type(x.value) is engine.CtmrError


def test_pem_decode_error_carries_index_and_offset(rig):
    e, lib = rig
    for fn, call in (("ctmr_pem_decode", e.pem_decode), ("ctmr_pem_decode_each", e.pem_decode_each)):
        lib.script(fn, (N.E_INVAL, {"PemDecodeInfo": {"bad_file": 1, "bad_offset": 44}}))
        with pytest.raises(engine.PemDecodeError) as x:
            call(BODIES)
        assert (x.value.code, x.value.bad_file, x.value.bad_offset) == (N.E_INVAL, 1, 44) and len(lib.calls(fn)) == 1
        lib.script(fn, (RANGE, {"PemDecodeInfo": {"files": 3, "certificates": 2, "payload_bytes": 50, "bad_file": NONE}}),
                   (N.E_INVAL, {"PemDecodeInfo": {"bad_file": 0, "bad_offset": 9}}))
        with pytest.raises(engine.PemDecodeError) as x:
            call(BODIES)
        assert (x.value.bad_file, x.value.bad_offset) == (0, 9) and len(lib.calls(fn)) == 3
        lib.script(fn, (N.E_INVAL, {"PemDecodeInfo": {"bad_file": NONE}}))
        with pytest.raises(engine.CtmrError) as x:
            call(BODIES)
        assert type(x.value) is engine.CtmrError and x.value.code == N.E_INVAL


# ---- the text decoders

@pytest.mark.parametrize("each", [False, True])
@pytest.mark.parametrize("bodies", [BODIES, [], [b"x" * 33]], ids=["three", "none", "one"])
def test_entries_json_is_one_call_sized_by_the_bounds(rig, each, bodies):
    """3/4 of the text + PAYLOAD_PAD bytes of blob, text / 34 entries: no second call, CTMR_E_RANGE is a failure."""
    e, lib = rig
    fn = "ctmr_entries_json_each" if each else "ctmr_entries_json"
    call = e.entries_json_each if each else e.entries_json
    text, R = sum(len(b) for b in bodies), len(bodies)
    n = 1 if text >= 34 else 0
    lib.script(fn, (0, {"EntriesJsonInfo": {"entries": n, "blob_bytes": 5 * n}, 8: u64s(*range(R + 1)),
                        **({9: u64s(*([NONE, 7, NONE][:R]))} if each else {})}))
    raw = call(bodies)
    want = (None, "ptr", "ptr", R, "ptr", text * 3 // 4 + PAD, "ptr", text // 34, "ptr") + (("ptr",) if each else ()) + ("&EntriesJsonInfo",)
    assert lib.calls(fn) == [want]
    assert (len(raw.blob), len(raw.bounds), list(raw.resp_first)) == (5 * n + PAD, 2 * n + 1, list(range(R + 1)))
    assert raw.bad == ([None, 7, None][:R] if each else None)
    lib.script(fn, (RANGE, {}))
    with pytest.raises(engine.CtmrError) as x:
        call(bodies)
    assert x.value.code == RANGE and len(lib.calls(fn)) == 2


@pytest.mark.parametrize("each", [False, True])
@pytest.mark.parametrize("files", [BODIES, [], [b"x" * 33]], ids=["three", "none", "one"])
def test_pem_decode_asks_for_the_sizes_then_collects(rig, each, files):
    e, lib = rig
    fn = "ctmr_pem_decode_each" if each else "ctmr_pem_decode"
    call = e.pem_decode_each if each else e.pem_decode
    F = len(files)
    bad = {9: u64s(*([3, NONE, NONE][:F]))} if each else {}
    sizes = {"files": F, "certificates": 2, "payload_bytes": 50, "bad_file": NONE}
    lib.script(fn, (RANGE, {"PemDecodeInfo": sizes}),
               (0, {"PemDecodeInfo": sizes, 4: b"\x07" * (50 + PAD), 6: u64s(0, 20, 50), 8: u64s(*range(F + 1)), **bad}))
    out = call(files)
    tail = (("ptr",) if each else ()) + ("&PemDecodeInfo",)
    assert lib.calls(fn) == [(None, "ptr", "ptr", F, None, 0, None, 0, None) + tail,
                             (None, "ptr", "ptr", F, "ptr", 50 + PAD, "ptr", 2, "ptr") + tail]
    payload, offsets, first, info = out[:4]
    assert (payload.tobytes(), list(offsets), list(first), info.certificates) == (b"\x07" * (50 + PAD), [0, 20, 50], list(range(F + 1)), 2)
    assert len(out) == (5 if each else 4) and (not each or out[4] == [3, None, None][:F])
    lib.script(fn, (RANGE, {"PemDecodeInfo": sizes}), (RANGE, {"PemDecodeInfo": sizes}), (0, {}))
    with pytest.raises(engine.CtmrError) as x:
        call(files)
    assert x.value.code == RANGE and len(lib.calls(fn)) == 4


# ---- write-back and the text waits: the sizes first, then the exact call

def test_ticket_writeback_without_anything_is_one_call(rig):
    e, lib = rig
    lib.script("ctmr_ticket_writeback", (0, {"WritebackInfo": {"flags": N.WB_PEM}}))
    wb = e.ticket_writeback(5)
    assert lib.calls("ctmr_ticket_writeback") == [(None, 5, None, 0, None, None, 0, None, 0, "&WritebackInfo")]
    assert (len(wb.pem_buf), list(wb.pem_offsets), wb.items, wb.offs) == (0, [0], [], [])


def test_ticket_writeback_collects_with_the_sizes_of_the_first_call(rig):
    e, lib = rig
    sizes = {"n_new": 2, "pem_bytes": 30, "n_items": 2, "item_bytes": 5, "flags": N.WB_PEM | N.WB_META}
    items = (N.MetaItem * 2)(N.MetaItem(entry=0, kind=N.MK_CRL, issuer_idx=4, exp_hour=9, off=11, len=3),
                             N.MetaItem(entry=1, kind=N.MK_DN, issuer_idx=5, exp_hour=8, off=12, len=2))
    lib.script("ctmr_ticket_writeback", (RANGE, {"WritebackInfo": sizes}),
               (0, {"WritebackInfo": sizes, 2: b"p" * 30, 4: u64s(0, 10, 30), 5: bytes(items), 7: b"abcde"}))
    wb = e.ticket_writeback(5)
    assert lib.calls("ctmr_ticket_writeback") == [(None, 5, None, 0, None, None, 0, None, 0, "&WritebackInfo"),
                                                  (None, 5, "ptr", 30, "ptr", 2 * C.sizeof(N.MetaItem), 2, "ptr", 5, "&WritebackInfo")]
    assert (wb.pem_buf.tobytes(), list(wb.pem_offsets)) == (b"p" * 30, [0, 10, 30])
    assert (wb.items, wb.offs) == ([(N.MK_CRL, 0, 4, 9, b"abc"), (N.MK_DN, 1, 5, 8, b"de")], [11, 12])
    sizes = {"n_new": 2, "pem_bytes": 0, "n_items": 0, "item_bytes": 0, "flags": N.WB_META}       # (the floors of empty parts)
    lib.script("ctmr_ticket_writeback", (RANGE, {"WritebackInfo": sizes}), (0, {"WritebackInfo": sizes}))
    wb = e.ticket_writeback(6)
    assert lib.calls("ctmr_ticket_writeback")[3] == (None, 6, "ptr", 1, "ptr", C.sizeof(N.MetaItem), 0, "ptr", 1, "&WritebackInfo")
    assert (len(wb.pem_buf), list(wb.pem_offsets), wb.items) == (0, [0], [])


def test_ticket_writeback_failures(rig):
    e, lib = rig
    lib.script("ctmr_ticket_writeback", (N.E_NOTFOUND, {}))
    with pytest.raises(engine.CtmrError) as x:
        e.ticket_writeback(5)
    assert x.value.code == N.E_NOTFOUND and len(lib.calls("ctmr_ticket_writeback")) == 1
    lib.script("ctmr_ticket_writeback", (RANGE, {"WritebackInfo": {"n_new": 1}}), (RANGE, {}), (0, {}))
    with pytest.raises(engine.CtmrError) as x:
        e.ticket_writeback(5)
    assert x.value.code == RANGE and len(lib.calls("ctmr_ticket_writeback")) == 3


def submit(e, lib, which, bodies, ticket):
    if which == "json":
        lib.script("ctmr_submit_entries_json", (0, {4: ticket}))
        assert e.submit_entries_json(bodies) == ticket
    else:
        lib.script("ctmr_submit_pem", (0, {5: ticket}))
        assert e.submit_pem(bodies, [N.NO_ISSUER] * len(bodies)) == ticket


WAITS = {"json": ("ctmr_wait_entries_json", "EntriesJsonInfo", "entries", "wait_entries_json",
                  lambda cap, p: (None, 21, cap, p, p, p, "ptr", "ptr", "&EntriesJsonInfo", "&DecodeStats", "&BatchStats")),
         "pem": ("ctmr_wait_pem", "PemDecodeInfo", "certificates", "wait_pem",
                 lambda cap, p: (None, 21, cap, p, p, "ptr", "ptr", "&PemDecodeInfo", "&BatchStats"))}


@pytest.mark.parametrize("which", ["json", "pem"])
def test_wait_of_a_ticket_without_items_is_one_call(rig, which):
    e, lib = rig
    fn, info, _, wait, args = WAITS[which]
    first_at, bad_at = (6, 7) if which == "json" else (5, 6)
    submit(e, lib, which, BODIES, 21)
    lib.script(fn, (0, {first_at: u64s(0, 0, 0, 0), bad_at: u64s(4, NONE, 70)}))
    r = getattr(e, wait)(21)
    assert lib.calls(fn) == [args(0, None)]
    assert (len(r.records), len(r.new_idx), r.bad) == (0, 0, [4, None, 70])
    assert list(r.resp_first if which == "json" else r.file_first) == [0, 0, 0, 0]


@pytest.mark.parametrize("which", ["json", "pem"])
def test_wait_collects_with_the_size_of_the_first_call(rig, which):
    e, lib = rig
    fn, info, field, wait, args = WAITS[which]
    first_at, bad_at = (6, 7) if which == "json" else (5, 6)
    submit(e, lib, which, BODIES, 21)
    lib.script(fn, (RANGE, {info: {field: 3}}),
               (0, {info: {field: 3}, "BatchStats": {"n_new": 2}, 4: u64s(0, 2, 99), first_at: u64s(0, 2, 2, 3), bad_at: u64s(NONE, 0, NONE)}))
    r = getattr(e, wait)(21)
    assert lib.calls(fn) == [args(0, None), args(3, "ptr")]
    assert (len(r.records), list(r.new_idx), r.bad) == (3, [0, 2], [None, 0, None])
    assert list(r.resp_first if which == "json" else r.file_first) == [0, 2, 2, 3]
    if which == "json":
        assert len(r.timestamp) == 3
    else:
        assert r.info.certificates == 3


@pytest.mark.parametrize("which", ["json", "pem"])
def test_wait_short_twice_raises_and_the_ticket_is_gone(rig, which):
    e, lib = rig
    fn, info, field, wait, args = WAITS[which]
    submit(e, lib, which, BODIES, 21)
    lib.script(fn, (RANGE, {info: {field: 3}}), (RANGE, {info: {field: 4}}))
    with pytest.raises(engine.CtmrError) as x:
        getattr(e, wait)(21)
    assert x.value.code == RANGE and len(lib.calls(fn)) == 2 and 21 not in e._text_tickets
    submit(e, lib, which, BODIES, 22)
    lib.script(fn, (N.E_HIP, {}))                        # failed with its super-batch: raised after the one call, and gone
    with pytest.raises(engine.CtmrError) as x:
        getattr(e, wait)(22)
    assert x.value.code == N.E_HIP and len(lib.calls(fn)) == 3 and e._text_tickets == {}


def test_text_tickets_are_waited_for_once_and_by_their_own_kind(rig):
    e, lib = rig
    submit(e, lib, "json", BODIES, 21)
    submit(e, lib, "pem", BODIES, 22)
    assert e._text_tickets == {21: ("submit_entries_json", 3), 22: ("submit_pem", 3)}
    for wait, ticket in ((e.wait_pem, 21), (e.wait_entries_json, 22), (e.wait_pem, 23), (e.wait_entries_json, 23)):
        with pytest.raises(engine.CtmrError) as x:
            wait(ticket)
        assert x.value.code == N.E_NOTFOUND
    assert lib.calls("ctmr_wait_pem") == [] and lib.calls("ctmr_wait_entries_json") == []
    e.wait_entries_json(21)
    e.wait_pem(22)
    for wait, ticket in ((e.wait_entries_json, 21), (e.wait_pem, 22)):
        with pytest.raises(engine.CtmrError) as x:
            wait(ticket)
        assert x.value.code == N.E_NOTFOUND and "already collected" in str(x.value)
    assert len(lib.calls("ctmr_wait_pem")) == 1 and len(lib.calls("ctmr_wait_entries_json")) == 1
