"""-m gpu: what the four parse entry points — ctmr_known_resp_image(_device), ctmr_crl_probes(_device) — answer at their
edges, to the letter: the return code, the text of ctmr_last_error, and what `info` / `cinfo` hold afterwards.

tests/test_gpu_resp_image.py and tests/test_gpu_crl_probes.py pin codes, offsets and images; this file pins the texts and
the order of the checks, on inputs of tens of bytes.  Every expected string and figure is written out here.  Before each
call the engine's error text is set to PRIMED by a call of another family, and `info` / `cinfo` are filled with 0xA5: a
call that sets no text leaves PRIMED, a structure the call does not write stays UNTOUCHED."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import ct_mapreduce_amd as ctmr
from ct_mapreduce_amd import _native as N
from tests import crl_corpus as CC
from tests.test_gpu_exchange import DEV
from tests.test_resp_image_cpu import GOOD, sadd

UNTOUCHED = "untouched"
PRIMED = "known image: bad magic"
NONE = (1 << 64) - 1
HUGE = (1 << 32) - 64

ONE = sadd(GOOD, b"\x01\x02\x03")                       # 98 bytes: one command, one member record
CRL_ONE, CRL_ONE_LO = CC.crl_at([CC.entry(CC.serial_of(0, 4))])
CRL_NONE = CC.crl([])
CRL_CUT = CRL_ONE[:77] + b"\x04" + CRL_ONE[78:]         # the entry's serial is no INTEGER: nothing fills the value
DG = CC.DIGESTS[0]

RESP = "known resp image: "
CRLP = "crl probes: "
T_RESP_NEED = RESP + "128 meta bytes and 1 member records needed"
T_RESP_BYTES = RESP + "176 bytes needed"
T_CRL_NEED = CRLP + "128 meta bytes and 1 member records needed"
T_CRL_BYTES = CRLP + "176 bytes needed"
T_HEAD = CRLP + "CRL 0, offset 0: not the TLV a CertificateList has here, or not a definite minimal length inside its structure"
T_ENTRY = CRLP + "CRL 0, offset 75: not SEQUENCE { INTEGER, Time, optional SEQUENCE } filled exactly inside revokedCertificates"

I_ONE = dict(members=1, sets=1, host_members=0, meta_bytes=128, image_bytes=176, issuers=1)
I_RESP_ONE = dict(I_ONE, commands=1, skipped_members=0)
I_NONE = dict(members=0, sets=0, host_members=0, meta_bytes=64, image_bytes=64, issuers=0)


def cinfo_of(entries=0, records=0, empty_crls=0, candidates=0, bad_crl=NONE, bad_offset=NONE):
    return dict(crls=1, entries=entries, records=records, host_members=0, empty_crls=empty_crls, candidates=candidates,
                bad_crl=bad_crl, bad_offset=bad_offset)


C_ARGS = cinfo_of()                                     # what the argument checks leave: the count, nothing bad named
C_ONE = cinfo_of(entries=1, records=1, candidates=3)    # the entry and the CRL's two frames
C_NONE = cinfo_of(empty_crls=1, candidates=2)


def test_the_inputs_are_what_the_figures_assume():
    assert len(ONE) == 98 and ONE[89:93] == b"$3\r\n"
    assert (len(CRL_ONE), CRL_ONE_LO, len(CRL_NONE)) == (164, 75, 141) and CRL_ONE[75:79] == b"\x30\x15\x02\x04"


@pytest.fixture(scope="module")
def eng():
    e = ctmr.Engine(device=0, table_slots=1 << 12, pair_slots=1 << 10)
    yield e
    e.close()


def prime(e):
    with pytest.raises(ctmr.CtmrError):
        e.known_import(b"\0" * 64)
    assert e._lib.ctmr_last_error(e._h).decode() == PRIMED


def filled(cls):
    x = cls()
    C.memset(C.byref(x), 0xA5, C.sizeof(x))
    return x


def seen(x):
    if bytes(x) == b"\xa5" * C.sizeof(x):
        return UNTOUCHED
    return {f: getattr(x, f) for f, _ in x._fields_ if f != "reserved"}


def on_device(data):
    return torch.from_numpy(np.frombuffer(bytes(data) or b"\0", np.uint8).copy()).to(DEV)


def resp_call(e, device, stream, n=None, meta_cap=128, members_cap=1, null_out=False, null_info=False):
    """stream None: a null pointer.  The host variant's buffer is meta_cap + 48 members_cap bytes."""
    prime(e)
    info = filled(N.KnownRespImageInfo)
    p_info = None if null_info else C.byref(info)
    n = len(stream) if n is None else n
    if device:
        d_s = on_device(stream or b"")
        d_out = torch.empty(48 * max(members_cap, 1), dtype=torch.uint8, device=DEV)
        meta = np.empty(max(meta_cap, 1), np.uint8)
        rc = e._lib.ctmr_known_resp_image_device(e._h, None if stream is None else C.c_void_p(d_s.data_ptr()), n, meta.ctypes.data, meta_cap,
                                                 None if null_out else C.c_void_p(d_out.data_ptr()), members_cap, p_info)
    else:
        cap = meta_cap + 48 * members_cap
        out = np.empty(max(cap, 1), np.uint8)
        rc = e._lib.ctmr_known_resp_image(e._h, stream, n, None if null_out else out.ctypes.data, cap, p_info)
    return rc, e._lib.ctmr_last_error(e._h).decode(), seen(info)


def crl_call(e, device, blob, n=None, offsets=None, meta_cap=128, members_cap=1, null_out=False, null_info=False, null_cinfo=False):
    prime(e)
    info, cinfo = filled(N.KnownImageInfo), filled(N.CrlInfo)
    p_info = None if null_info else C.byref(info)
    p_cinfo = None if null_cinfo else C.byref(cinfo)
    n = len(blob) if n is None else n
    offs = np.asarray([0, n] if offsets is None else offsets, np.uint64)
    if device:
        d_s = on_device(blob or b"")
        d_out = torch.empty(48 * max(members_cap, 1), dtype=torch.uint8, device=DEV)
        meta = np.empty(max(meta_cap, 1), np.uint8)
        rc = e._lib.ctmr_crl_probes_device(e._h, None if blob is None else C.c_void_p(d_s.data_ptr()), n, offs.ctypes.data, 1, DG,
                                           meta.ctypes.data, meta_cap, None if null_out else C.c_void_p(d_out.data_ptr()), members_cap,
                                           p_info, p_cinfo)
    else:
        cap = meta_cap + 48 * members_cap
        out = np.empty(max(cap, 1), np.uint8)
        rc = e._lib.ctmr_crl_probes(e._h, blob, n, offs.ctypes.data, 1, DG, None if null_out else out.ctypes.data, cap, p_info, p_cinfo)
    return rc, e._lib.ctmr_last_error(e._h).decode(), seen(info), seen(cinfo)


# (case, arguments of resp_call, → rc, text, info); the same for both variants unless a variant is named
RESP_CASES = [
    ("null input with a length", dict(stream=None, n=5), N.E_INVAL, RESP + "null stream", UNTOUCHED),
    ("2^32 - 64 bytes", dict(stream=ONE, n=HUGE), N.E_INVAL,
     RESP + "4294967232 bytes: a stream of 2^32 - 64 bytes or more is split at a command start", UNTOUCHED),
    ("2^32 - 64 bytes of a null input: the length is looked at first", dict(stream=None, n=HUGE), N.E_INVAL,
     RESP + "4294967232 bytes: a stream of 2^32 - 64 bytes or more is split at a command start", UNTOUCHED),
    ("null info", dict(stream=ONE, null_info=True), N.E_INVAL, PRIMED, UNTOUCHED),
    ("null info before a null input", dict(stream=None, n=5, null_info=True), N.E_INVAL, PRIMED, UNTOUCHED),
    ("one well-formed command", dict(stream=ONE), 0, PRIMED, I_RESP_ONE),
    ("no byte at all", dict(stream=b""), 0, PRIMED, dict(I_NONE, commands=0, skipped_members=0)),
    ("one byte of garbage", dict(stream=b"x"), N.E_INVAL, RESP + "offset 0: no command starts here", UNTOUCHED),
    ("a command cut short", dict(stream=ONE[:-2]), N.E_INVAL,
     RESP + "offset 89: not the start of a command or of a bulk string that ends in CRLF inside the stream", UNTOUCHED),
    ("a command that is none of the four", dict(stream=b"*1\r\n$4\r\nPING\r\n"), N.E_INVAL,
     RESP + "offset 0: not SADD key member..., EXPIREAT / PEXPIREAT key time or SELECT db with exactly its arguments", UNTOUCHED),
    ("meta one byte short", dict(stream=ONE, meta_cap=127), N.E_RANGE, {True: T_RESP_NEED, False: T_RESP_BYTES}, I_RESP_ONE),
    ("records one short", dict(stream=ONE, members_cap=0), N.E_RANGE, {True: T_RESP_NEED, False: T_RESP_BYTES}, I_RESP_ONE),
    ("records null with records needed", dict(stream=ONE, null_out=True), N.E_RANGE, {True: T_RESP_NEED, False: T_RESP_BYTES}, I_RESP_ONE),
    ("garbage before a short buffer", dict(stream=b"x", meta_cap=0, members_cap=0), N.E_INVAL, RESP + "offset 0: no command starts here",
     UNTOUCHED),
]

# (case, arguments of crl_call, → rc, text, info, cinfo)
CRL_CASES = [
    ("null input with a length", dict(blob=None, n=5), N.E_INVAL, CRLP + "null blob, offsets or digests", UNTOUCHED, C_ARGS),
    ("2^32 - 64 bytes", dict(blob=CRL_ONE, n=HUGE), N.E_INVAL,
     CRLP + "4294967232 bytes: a blob of 2^32 - 64 bytes or more is split between two CRLs", UNTOUCHED, C_ARGS),
    ("2^32 - 64 bytes of a null input: the length is looked at first", dict(blob=None, n=HUGE), N.E_INVAL,
     CRLP + "4294967232 bytes: a blob of 2^32 - 64 bytes or more is split between two CRLs", UNTOUCHED, C_ARGS),
    ("null info", dict(blob=CRL_ONE, null_info=True), N.E_INVAL, PRIMED, UNTOUCHED, UNTOUCHED),
    ("null cinfo", dict(blob=CRL_ONE, null_cinfo=True), N.E_INVAL, PRIMED, UNTOUCHED, UNTOUCHED),
    ("offsets[0] is not 0", dict(blob=CRL_ONE, offsets=[1, 164]), N.E_INVAL, CRLP + "CRL 0, offset 0: offsets[0] is not 0", UNTOUCHED,
     cinfo_of(bad_crl=0, bad_offset=0)),
    ("a null input before offsets[0]", dict(blob=None, n=5, offsets=[1, 5]), N.E_INVAL, CRLP + "null blob, offsets or digests", UNTOUCHED,
     C_ARGS),
    ("the last offset is not the length", dict(blob=CRL_ONE, offsets=[0, 163]), N.E_INVAL,
     CRLP + "CRL 1, offset 164: the last offset is not the blob's length", UNTOUCHED, cinfo_of(bad_crl=1, bad_offset=164)),
    ("one byte of garbage", dict(blob=b"\0"), N.E_INVAL, T_HEAD, UNTOUCHED, cinfo_of(bad_crl=0, bad_offset=0)),
    ("a CRL of no bytes", dict(blob=b"", offsets=[0, 0]), N.E_INVAL, CRLP + "CRL 0, offset 0: a CRL of 0 bytes", UNTOUCHED,
     cinfo_of(bad_crl=0, bad_offset=0)),
    ("one CRL with one entry", dict(blob=CRL_ONE), 0, PRIMED, I_ONE, C_ONE),
    ("one CRL with none", dict(blob=CRL_NONE, meta_cap=64, members_cap=0), 0, PRIMED, I_NONE, C_NONE),
    ("one CRL with none and null records", dict(blob=CRL_NONE, meta_cap=64, members_cap=0, null_out={True: True, False: False}), 0, PRIMED,
     I_NONE, C_NONE),
    ("an entry that is none", dict(blob=CRL_CUT), N.E_INVAL, T_ENTRY, UNTOUCHED, cinfo_of(bad_crl=0, bad_offset=75)),
    ("meta one byte short", dict(blob=CRL_ONE, meta_cap=127), N.E_RANGE, {True: T_CRL_NEED, False: T_CRL_BYTES}, I_ONE, C_ONE),
    ("records one short", dict(blob=CRL_ONE, members_cap=0), N.E_RANGE, {True: T_CRL_NEED, False: T_CRL_BYTES}, I_ONE, C_ONE),
    ("records null with records needed", dict(blob=CRL_ONE, null_out=True), N.E_RANGE, {True: T_CRL_NEED, False: T_CRL_BYTES}, I_ONE, C_ONE),
    ("garbage before a short buffer", dict(blob=b"\0", meta_cap=0, members_cap=0), N.E_INVAL, T_HEAD, UNTOUCHED,
     cinfo_of(bad_crl=0, bad_offset=0)),
]


def per_variant(x, device):
    return x[device] if isinstance(x, dict) and set(x) == {True, False} else x


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", RESP_CASES, ids=[c[0] for c in RESP_CASES])
def test_known_resp_image_answers(eng, case, device):
    _, kw, rc, text, info = case
    got = resp_call(eng, device, **{k: per_variant(v, device) for k, v in kw.items()})
    print(got)
    assert got == (rc, per_variant(text, device), info)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", CRL_CASES, ids=[c[0] for c in CRL_CASES])
def test_crl_probes_answers(eng, case, device):
    _, kw, rc, text, info, cinfo = case
    got = crl_call(eng, device, **{k: per_variant(v, device) for k, v in kw.items()})
    print(got)
    assert got == (rc, per_variant(text, device), info, cinfo)
