"""Builds and binds the test-only helpers (host build of the product walk, OpenSSL extractor)."""
import ctypes as C
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "..", "ct_mapreduce_amd", "csrc")
WALK_DEPS = [os.path.join(CSRC, h) for h in ("der_walk.h", "spki_key.h", "ec_curves.h", "entry_decode.h")]


def _build(src, out, cmd, deps=(), libs=()):
    """The library `out` built from `src` (+ `deps`): next to its source, where __graft_entry__.build() leaves it, or
    rebuilt there when a source is newer.  A checkout that was built and is then only read (not writable) rebuilds a
    stale library in this user's private cache directory (_cache_dir) instead of failing."""
    srcp = os.path.join(HERE, src)
    inputs = [srcp] + list(deps)

    def fresh(p):
        return os.path.exists(p) and all(os.path.getmtime(p) >= os.path.getmtime(d) for d in inputs)
    outp = os.path.join(HERE, out)
    if fresh(outp):
        return outp
    if not os.access(HERE, os.W_OK):
        outp = os.path.join(_cache_dir(), out)
        if fresh(outp):
            return outp
    subprocess.check_call(list(cmd) + [srcp, "-o", outp] + list(libs))
    return outp


def _cache_dir():
    """This user's private cache for harness libraries that cannot be rebuilt in place: $XDG_CACHE_HOME or ~/.cache, else
    a fresh private temporary directory.  A directory another user owns or may write is refused: a library is loaded from it."""
    base = os.environ.get("XDG_CACHE_HOME") or os.path.join(os.path.expanduser("~"), ".cache")
    d = os.path.join(base, "ctmr_harness")
    try:
        os.makedirs(d, mode=0o700, exist_ok=True)
    except OSError:
        d = tempfile.mkdtemp(prefix="ctmr_harness_")
    st = os.stat(d)
    if st.st_uid != os.getuid() or st.st_mode & 0o022:
        raise PermissionError(f"{d}: not a private directory of this user; refusing to build or load a library there")
    return d


def _lib(name):
    src, out, cmd, kw = LIBS[name]
    return _build(src, out, cmd, **kw)


def build_all():
    """Every harness library (what __graft_entry__.build() compiles, so that tests and bench.py need no compiler)."""
    return [_lib(name) for name in LIBS]


class HarnessOut(C.Structure):
    _fields_ = [("ok", C.c_int32), ("serial_off", C.c_uint32), ("serial_len", C.c_uint32),
                ("not_before", C.c_int64), ("not_after", C.c_int64), ("cn_off", C.c_uint32),
                ("cn_len", C.c_uint32), ("bc_valid", C.c_int32), ("is_ca", C.c_int32),
                ("spki_off", C.c_uint32), ("spki_len", C.c_uint32), ("serial_w", C.c_uint32 * 5),
                ("cn_match", C.c_int32), ("nonfatal", C.c_int32)]


class OsslOut(C.Structure):
    _fields_ = [("ok", C.c_int), ("not_before", C.c_longlong), ("not_after", C.c_longlong),
                ("is_ca", C.c_int), ("has_bc", C.c_int), ("serial_len", C.c_int),
                ("serial", C.c_ubyte * 64), ("serial_neg", C.c_int), ("cn_len", C.c_int),
                ("cn", C.c_ubyte * 256), ("spki_len", C.c_int), ("spki", C.c_ubyte * 1024)]


class EntryOut(C.Structure):
    _fields_ = [("ok", C.c_int32), ("entry_type", C.c_int32), ("timestamp", C.c_uint64), ("cert_lo", C.c_uint64),
                ("cert_hi", C.c_uint64), ("chain0_lo", C.c_uint64), ("chain0_len", C.c_uint32),
                ("n_chain", C.c_uint32), ("tbs_lo", C.c_uint64), ("tbs_len", C.c_uint32)]


_walk = None
_ossl = None
_entry = None


def product_decode_entry(leaf_input: bytes, extra_data: bytes, fill=0xA5, prefix=b"") -> EntryOut:
    """The product's decode_entry (host build) on blob = prefix ‖ leaf_input ‖ extra_data."""
    global _entry
    if _entry is None:
        p = _lib("entry")
        _entry = C.CDLL(p)
        _entry.harness_decode_entry.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint8,
                                                C.POINTER(EntryOut)]
        _entry.harness_quick_hash.argtypes = [C.c_char_p, C.c_uint32]
        _entry.harness_quick_hash.restype = C.c_uint64
    blob = prefix + leaf_input + extra_data
    o = EntryOut()
    l0 = len(prefix)
    _entry.harness_decode_entry(blob, len(blob), l0, l0 + len(leaf_input), len(blob), fill, C.byref(o))
    return o


def product_walk(der: bytes, fill=0xA5, cn_filter=None) -> HarnessOut:
    """cn_filter=None: no issuerCNFilter (cn_match is True); bytes: the raw filter string."""
    global _walk
    if _walk is None:
        p = _lib("walk")
        _walk = C.CDLL(p)
        _walk.harness_walk_f.argtypes = [C.c_char_p, C.c_uint32, C.c_uint8, C.c_char_p, C.c_uint32,
                                         C.c_int, C.POINTER(HarnessOut)]
    o = HarnessOut()
    _walk.harness_walk_f(der, len(der), fill, *_filter_args(cn_filter), C.byref(o))
    return o


def product_set_spki(on: bool):
    """The host build's strict_spki switch (default on): parse the public key as CT-go's parsePublicKey does."""
    product_walk(b"\x30\x00")
    _walk.harness_set_spki(int(bool(on)))


def product_set_ext(on: bool):
    """The host build's strict_extensions switch (default off): the bodies of the extensions Go unmarshals."""
    product_walk(b"\x30\x00")
    _walk.harness_set_ext(int(bool(on)))


def product_set_strings(on: bool):
    """The host build's strict_strings switch (default off): findings arrive as WALK_NF_STRING (4) in .nonfatal."""
    product_walk(b"\x30\x00")
    _walk.harness_set_strings(int(bool(on)))


def product_crl_uris(der: bytes, cv: int, ev: int):
    """der_walk.h crl_dps<COLLECT> over the cRLDistributionPoints value der[cv:ev]: None = malformed, else the URIs."""
    product_walk(b"\x30\x00")
    out = (C.c_uint32 * 16)()
    _walk.harness_crl_uris.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32]
    n = _walk.harness_crl_uris(der, len(der), cv, ev, out, 8)
    if n < 0:
        return None
    return [bytes(der[out[2 * k]:out[2 * k] + out[2 * k + 1]]) for k in range(min(n, 8))]


def product_ec_point_bits(buf: bytes, xbit: int, curve: int) -> bool:
    """k_ec_resolve's loader + curve equation (host build): X starts at BIT xbit of buf; curve 1..5 = P-256, P-384, P-521,
    P-224, secp192r1."""
    product_walk(b"\x30\x00")
    _walk.harness_ec_point_bits.argtypes = [C.c_char_p, C.c_uint32, C.c_uint64, C.c_int]
    return bool(_walk.harness_ec_point_bits(buf, len(buf), xbit, curve))


def product_walk_tbs(tbs: bytes, fill=0xA5) -> HarnessOut:
    """The product's walk over a bare TBSCertificate (strict_leaf)."""
    product_walk(b"\x30\x00")          # builds and binds the library
    _walk.harness_walk_tbs.argtypes = [C.c_char_p, C.c_uint32, C.c_uint8, C.POINTER(HarnessOut)]
    o = HarnessOut()
    _walk.harness_walk_tbs(tbs, len(tbs), fill, C.byref(o))
    return o


def product_name_strings(der: bytes, fill=0xA5) -> int:
    """strict_strings: 1 = the Names' string values keep to their types' character sets, 0 = a finding, -1 = no parse."""
    product_walk(b"\x30\x00")
    _walk.harness_name_strings.argtypes = [C.c_char_p, C.c_uint32, C.c_uint8]
    return _walk.harness_name_strings(der, len(der), fill)


def walk_touched(der: bytes, phase: int = 0, cn_filter: bytes = b"", reference_profile: bool = False):
    """(accepted, bytes the walk's reads cover, distinct 128-byte lines they lie in when the certificate starts at
    byte `phase` of a line) — bench.py's needed_bytes accounting.  reference_profile: the walk with strict_strings and
    strict_extensions (the subjectAltName's headers and the extension bodies are read)."""
    product_walk(b"\x30\x00")          # builds / loads the library
    _walk.harness_touched_profile(int(reference_profile))
    fn = _walk.harness_walk_touched
    fn.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32),
                   C.POINTER(C.c_uint32)]
    nb, nl = C.c_uint32(0), C.c_uint32(0)
    ok = fn(der, len(der), phase & 127, cn_filter, len(cn_filter), C.byref(nb), C.byref(nl))
    return bool(ok), nb.value, nl.value


def _filter_args(cn_filter):
    f = cn_filter if cn_filter is not None else b""
    return f, len(f), int(cn_filter is not None)


def walk_window(der: bytes, phase: int = 0, wbytes: int = 224, strings: bool = False, ext: bool = False, skip: int = 0,
                cn_filter=None):
    """The walk through a SIMULATED per-lane window of `wbytes` bytes (kernels/readers.h geometry) for a certificate that
    starts at byte `phase` of its 128-byte line: (accepted, per-lane refills the hints asked for, reads that missed the
    window, position of the first refill, position of the first miss, cooperative refills of the subjectAltName walk,
    defer_exact calls).  cn_filter (bytes: the raw issuerCNFilter): three more — cn_match as THIS walk saw it, and how many
    reads of cn_prefix_match lay inside and outside the window."""
    product_walk(b"\x30\x00")
    out = (C.c_uint32 * 9)()
    if skip:    # the first window begins `skip` octets in, the outer headers come from sixteen octets held apart (WinGeo::SKIP)
        fn = _walk.harness_walk_window_skip
        fn.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_char_p, C.c_uint32, C.c_int,
                       C.POINTER(C.c_uint32)]
        ok = fn(der, len(der), phase, wbytes, skip, int(strings), int(ext), *_filter_args(cn_filter), out)
    else:
        fn = _walk.harness_walk_window
        fn.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_char_p, C.c_uint32, C.c_int,
                       C.POINTER(C.c_uint32)]
        ok = fn(der, len(der), phase, wbytes, int(strings), int(ext), *_filter_args(cn_filter), out)
    return (bool(ok),) + tuple(out)[:6 if cn_filter is None else 9]


class DidNotTerminate(Exception):
    """The simulated out-of-reach lane passed its round cap: on the device that wave never ends."""


def walk_window_noreach(der: bytes, phase: int = 0, wbytes: int = 224, flavour: str = "C", strings: bool = True, ext: bool = True,
                        cap: int = 10_000, fill: int = 0xA5, cn_filter=None):
    """The walk as a lane OUT OF REACH of its wave's buffer descriptor runs it (kernels/readers.h lrel == REL_NONE: an entry
    view in no order): cooperative refills do nothing, the lane's own refills work; flavour "C" = WinReaderC (reads outside
    the window are global reads), "S" = WinReaderS (clamped and counted; the exact reader then decides).  Returns
    (HarnessOut, stats) with stats = (per-lane refills, misses, cooperative refills asked for in vain, defer_exact calls,
    exact rerun, window reads outside the window); raises DidNotTerminate past `cap` calls of holds / coop_refill_lines_to.
    cn_filter (bytes): the walk runs under that issuerCNFilter, and stats gains the reads of cn_prefix_match inside and
    outside the window (flavour "S": of the clamped walk)."""
    product_walk(b"\x30\x00")
    fn = _walk.harness_walk_window_noreach
    fn.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint8,
                   C.c_char_p, C.c_uint32, C.c_int, C.POINTER(HarnessOut), C.POINTER(C.c_uint32)]
    o, st = HarnessOut(), (C.c_uint32 * 8)()
    if not fn(der, len(der), phase, wbytes, {"C": 0, "S": 1}[flavour], int(strings), int(ext), cap, fill, *_filter_args(cn_filter),
              C.byref(o), st):
        raise DidNotTerminate(f"phase {phase}, window {wbytes}, flavour {flavour}: more than {cap} rounds")
    return o, tuple(st)[:6 if cn_filter is None else 8]


def walk_window_stale(der: bytes, phase: int = 0, wbytes: int = 224, slack: int = 4, strings: bool = True, ext: bool = True,
                      fill: int = 0xA5, cn_filter=None, skip: int = 0):
    """The walk through a simulated window with CONTENTS of its own: refills copy the payload's octets, a partial cooperative
    refill (kernels/readers.h coop_refill_lines_to: up to the value's end + `slack`) leaves the rows behind its chunks as they
    were, reads are clamped into the window and counted as WinReaderS does, ld2 is not; after a miss or a deferral the exact
    reader decides.  Returns (HarnessOut, stats) with stats = (per-lane refills, misses, cooperative refills, defer_exact
    calls, partial cooperative refills, unclamped reads outside the window).  cn_filter (bytes): the walk runs under that
    issuerCNFilter, and stats gains the reads of cn_prefix_match inside and outside the window.  skip: the first window begins
    that many octets into the certificate, the outer headers come from sixteen octets held apart (WinGeo::SKIP)."""
    product_walk(b"\x30\x00")
    fn = _walk.harness_walk_window_stale
    fn.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_int, C.c_int, C.c_uint8, C.c_char_p,
                   C.c_uint32, C.c_int, C.POINTER(HarnessOut), C.POINTER(C.c_uint32)]
    o, st = HarnessOut(), (C.c_uint32 * 8)()
    fn(der, len(der), phase, wbytes, skip, slack, int(strings), int(ext), fill, *_filter_args(cn_filter), C.byref(o), st)
    return o, tuple(st)[:6 if cn_filter is None else 8]


def ossl_extract(der: bytes):
    global _ossl
    if _ossl is None:
        _ossl = C.CDLL(_lib("ossl"))
        _ossl.ossl_extract.argtypes = [C.c_char_p, C.c_long, C.POINTER(OsslOut)]
        _ossl.ossl_pubkey_ok.argtypes = [C.c_char_p, C.c_long]
    o = OsslOut()
    if not _ossl.ossl_extract(der, len(der), C.byref(o)):
        return None
    return o


class OsslVerdict(C.Structure):
    _fields_ = [("stage", C.c_int), ("ext_nid", C.c_int), ("n_ext", C.c_int), ("reason", C.c_char * 96)]


def ossl_verdict(der: bytes) -> OsslVerdict:
    """OpenSSL's accept/reject opinion by stage: 0 everything decodes, 1 d2i_X509, 2 trailing bytes, 3 the public key,
    4 a validity time, 5 the body of an extension it has a decoder for (ext_nid)."""
    ossl_extract(b"\x30\x00")
    _ossl.ossl_verdict.argtypes = [C.c_char_p, C.c_long, C.POINTER(OsslVerdict)]
    v = OsslVerdict()
    _ossl.ossl_verdict(der, len(der), C.byref(v))
    return v


def ossl_pubkey_ok(der: bytes) -> int:
    """OpenSSL's opinion on the public key: 1 = certificate and key decode (X509_get_pubkey), 0 = the key does not,
    -1 = the certificate does not."""
    ossl_extract(b"\x30\x00")
    return _ossl.ossl_pubkey_ok(der, len(der))


_hk = None


def host_keys_lib():
    """Host build of csrc/host_keys.h: the wire form and the verdict of a group round's long-serial settlement."""
    global _hk
    if _hk is None:
        _hk = C.CDLL(_lib("host_keys"))
        _hk.harness_host_keys_verdict.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint64),
                                                  C.POINTER(C.c_uint8), C.c_uint32]
        _hk.harness_host_keys_append.argtypes = [C.c_uint64, C.c_int32, C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint64),
                                                 C.c_uint32]
        _hk.harness_host_keys_append.restype = C.c_uint32
    return _hk


_hash = None


def hash_lib():
    """Host build of the key hashing (csrc/ctmr_dev.h key_meta / mixk / key_hash / key_tag, csrc/kernels/keyrec.h
    key_owner_h / bloom_pos): what the port in tests/xchg_corpus.py is held against."""
    global _hash
    if _hash is None:
        _hash = C.CDLL(_lib("hash"))
        _hash.harness_key_meta.argtypes = [C.c_int32, C.c_uint32, C.c_uint32]
        _hash.harness_mixk.argtypes = [C.c_uint64]
        _hash.harness_key_hash.argtypes = [C.c_uint64, C.POINTER(C.c_uint64)]
        _hash.harness_key_tag.argtypes = [C.c_uint64]
        _hash.harness_key_owner_h.argtypes = [C.c_uint64, C.c_uint32]
        _hash.harness_bloom_pos.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        for f in (_hash.harness_key_meta, _hash.harness_mixk, _hash.harness_key_hash):
            f.restype = C.c_uint64
        _hash.harness_key_tag.restype = _hash.harness_key_owner_h.restype = C.c_uint32
        _hash.harness_bloom_pos.restype = None
    return _hash


def build_fake_rccl() -> str:
    """The stand-in for librccl (fake_rccl.cpp: ranks as threads or processes on ONE GPU, bytes through POSIX shared
    memory), built on demand; hand the path to the library through CTMR_RCCL_LIB."""
    return _lib("fake_rccl")


# name → (source, library, compiler command, {deps, libs})
LIBS = {
    "walk": ("walk_harness.cpp", "libwalk_harness.so", ["g++", "-O2", "-std=c++17", "-shared", "-fPIC"],
             {"deps": WALK_DEPS}),
    "entry": ("entry_harness.cpp", "libentry_harness.so", ["g++", "-O2", "-std=c++17", "-shared", "-fPIC"],
              {"deps": WALK_DEPS}),
    "ossl": ("ossl_extract.c", "libossl_extract.so", ["gcc", "-O2", "-shared", "-fPIC"], {"libs": ["-lcrypto"]}),
    "host_keys": ("host_keys_harness.cpp", "libhost_keys_harness.so", ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall"],
                  {"deps": [os.path.join(CSRC, "host_keys.h")]}),
    # (the device headers as the host sees them: the flags of fake_rccl)
    "hash": ("hash_harness.cpp", "libhash_harness.so",
             ["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"],
             {"deps": WALK_DEPS + [os.path.join(CSRC, "ctmr_dev.h"), os.path.join(CSRC, "kernels", "keyrec.h")]}),
    "fake_rccl": ("fake_rccl.cpp", "libfake_rccl.so",
                  ["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"],
                  {"libs": ["-L/opt/rocm/lib", "-lamdhip64", "-pthread", "-lrt"]}),
}
