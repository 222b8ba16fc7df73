"""The walk of a lane OUT OF REACH of its wave's buffer descriptor, on the CPU (no GPU).

An entry view may address its certificates in any order (include/ctmr.h ctmr_map_view_device).  The map kernels read through
one descriptor per wave whose base is the certificate of the wave's first lane; a lane whose certificate lies below that
base, or REL_SPAN or more beyond it, has lrel == REL_NONE: the cooperative refills do nothing for it.  der_walk.h's
ext_san_coop used to wait for such a refill to move the window — a wave that never ends.  tests/harness simulates that lane
(walk_window_noreach: flavour C = WinReaderC / k_map_winc, flavour S = WinReaderS / k_map_fused) with a cap on the rounds, so
that a walk that would spin the GPU raises DidNotTerminate here instead of spinning this process.

For every certificate below — the synthetic corpus (profile 0 and the mixed profile 1), the public CA roots of
tests/golden/ca_roots.pem, hand-built certificates with a subjectAltName (the shapes of tests/test_ext_cpu.py and
tests/test_der_edge_cpu.py) and the fifteen damage kinds of tests/damage.py — at window sizes 224 and 256, at every phase
0..127 for a handful of certificates and a few phases for the rest, with strict_strings and strict_extensions on: the
out-of-reach walk TERMINATES, and its verdict and every HarnessOut field equal product_walk's (which tests/test_walk_cpu.py
and tests/test_ext_cpu.py pin to the oracle).  The field comparison has teeth for flavour C, whose own walk decides; flavour S
starts without a window as on the device, always misses and is decided by the exact rerun — what S checks is that the walk
over clamped, wrong bytes ENDS.  The model does not see the stale window of WinReaderC::touch_tail (kernels/readers.h, a
defect of the reader, not of the walk): tests/test_gpu_view_order.py does.

The cap: the in-reach walk of the same certificate (harness.walk_window) tells how many cooperative refills a terminating walk
takes; the cap is 100 x the largest such count over the corpus, at least 10 000."""
import pytest

from ct_mapreduce_amd import synth
from oracle import oracle as orc
from tests import der as D
from tests import harness
from tests.damage import hurt, KINDS_FATAL, KINDS_FINDING
from tests.test_ext_cpu import san, uri
from tests.test_real_certs_cpu import bundle_ders

FIELDS = [f for f, _ in harness.HarnessOut._fields_ if f != "serial_w"]
WINDOWS = (224, 256)
FEW_PHASES = (0, 3, 17, 64, 101, 127)


def dns(k, n=24):
    return D.tlv(0x82, (b"host-%04d." % k + b"x" * n)[:n])


def hand_built():
    """Certificates with a subjectAltName that sit on the rules of ext_san_check / ext_san_coop: short and long values, URIs,
    iPAddresses, high tag numbers, long-form lengths, elements that straddle a window's end, truncated and mislabelled ones."""
    many = [dns(k) for k in range(40)]                                    # ≈ 1 KB: four windows
    vals = [
        san(D.tlv(0x82, b"a.example"), D.tlv(0x81, b"x@a.example"), D.tlv(0x87, bytes(4)), D.tlv(0x87, bytes(16)), uri("https://a.example/x")),
        san(), san(D.tlv(0x82, b"\xff\x00 not IA5")), san(D.tlv(0xa0, b"\xff\xff"), D.tlv(0xa4, b"\x05"), D.tlv(0x88, b""), D.tlv(0x05, b"")),
        san(b"\x9f\x21\x01\x00"), san(D.tlv(0x87, bytes(5))), san(D.tlv(0x82, b"ok"), D.tlv(0x87, bytes(4)), D.tlv(0x87, bytes(5))),
        san(uri("http://a b/")), san(D.tlv(0x82, b"fine"), uri("http://ok.example"), D.tlv(0xa6, b"\x7f")),
        D.ext(17, b""), D.ext(17, D.tlv(0x31, D.tlv(0x82, b"a"))), D.ext(17, D.seq(D.tlv(0x82, b"a")) + b"\x00"),
        D.ext(17, D.seq(b"\x82\x05ab")), D.ext(17, D.seq(b"\x82")), D.ext(17, D.seq(b"\x82\x81\x01a")), D.ext(17, D.seq(b"\x9f\x1e\x00")),
        san(*many), san(*many, uri("https://deep.example/x")), san(*many, uri("http://h x/")), san(*many[:20], D.tlv(0x87, bytes(7)), *many[20:]),
        san(*many[:9], b"\x9f\x21\x01\x00", *many[9:]), san(*many[:30], D.tlv(0x82, b"y" * 200), *many[30:]),
        san(*many[:7], D.tlv(0x82, b"z" * 300), uri("urn:x:y"), *many[7:]), san(D.tlv(0x82, b"a" * 70000)),
        D.ext(17, D.seq(*many)[:-1] + b""), D.ext(17, D.seq(*many[:-1], b"\x82\x30" + b"q" * 24)),   # the last element does not fit
        san(*[D.tlv(0x82, b"") for _ in range(300)]), san(*[D.tlv(0x82, b"ab") for _ in range(200)], uri(":")),
    ]
    out = [D.cert(exts=[D.BC_NOT_CA, v]) for v in vals]
    out.append(D.cert(exts=[vals[16], vals[0]]))                          # a second subjectAltName: walked lane by lane
    out.append(D.cert(exts=[vals[16], D.BC_CA], subject=D.name(D.rdn(10, b"o" * 180), D.rdn(3, b"long subject"))))
    return out


def damaged():
    cfg = synth.config(seed=20261016, n_issuers=8, dup_permille=0)
    out = []
    for j, kind in enumerate(KINDS_FATAL + KINDS_FINDING):
        for i in (2 * j, 2 * j + 1):
            der = synth.leaf(cfg, i)[0]
            bad = hurt(der, kind, orc.parse_cert(der))
            assert len(bad) == len(der) and bad != der
            out.append(bad)
    return out


def corpora():
    c0, c1 = synth.config(seed=31, n_issuers=16, ca_permille=50, expired_permille=50), synth.config(seed=32, n_issuers=9, profile=1)
    return {"synthetic": [synth.leaf(c0, i)[0] for i in range(120)], "mixed": [synth.leaf(c1, i)[0] for i in range(120)],
            "roots": bundle_ders(), "hand_built": hand_built(), "damaged": damaged()}


@pytest.fixture(scope="module")
def corpus():
    return corpora()


@pytest.fixture(scope="module")
def cap(corpus):
    """100 x the most cooperative refills any in-reach walk of the corpus takes, at least 10 000."""
    most = 0
    for ders in corpus.values():
        for der in ders:
            for w in WINDOWS:
                most = max(most, harness.walk_window(der, 5, w, True, True)[5])
    assert most >= 3                                                      # the synthetic subjectAltName: several windows
    return max(10_000, 100 * most)


@pytest.fixture()
def reference_walk():
    harness.product_set_strings(True)
    harness.product_set_ext(True)
    yield
    harness.product_set_strings(False)
    harness.product_set_ext(False)


def check(der, phases, cap, counts):
    want = harness.product_walk(der, 0xA5)
    for w in WINDOWS:
        for flavour in ("C", "S"):
            for ph in phases:
                for fill in (0xA5, 0x30):
                    try:
                        got, st = harness.walk_window_noreach(der, ph, w, flavour, True, True, cap, fill)
                    except harness.DidNotTerminate:
                        counts["did_not_terminate", flavour] = counts.get(("did_not_terminate", flavour), 0) + 1
                        counts.setdefault("first", (len(der), ph, w, flavour))
                        counts.setdefault("stuck_certificates", set()).add(der)
                        continue
                    assert bool(got.ok) == bool(want.ok), (der[:16].hex(), len(der), ph, w, flavour)
                    for f in FIELDS:
                        assert getattr(got, f) == getattr(want, f), (f, len(der), ph, w, flavour)
                    assert list(got.serial_w) == list(want.serial_w)
                    assert st[5] == 0, "a window read outside the window"
                    counts["asked_in_vain"] = counts.get("asked_in_vain", 0) + st[2]
                    counts["rerun"] = counts.get("rerun", 0) + st[4]
    counts["accepted"] = counts.get("accepted", 0) + bool(want.ok)


@pytest.mark.parametrize("name", ["synthetic", "mixed", "roots", "hand_built", "damaged"])
def test_an_out_of_reach_lane_terminates_with_the_plain_walks_verdict(name, corpus, cap, reference_walk):
    ders, counts = corpus[name], {}
    for k, der in enumerate(ders):
        every = k < 4 or (name in ("hand_built", "damaged") and k % 6 == 0)
        check(der, range(128) if every else FEW_PHASES, cap, counts)
    stuck = {f: counts.get(("did_not_terminate", f), 0) for f in "CS"}
    assert stuck == {"C": 0, "S": 0}, "did not terminate: walks per flavour %r, %d of %d certificates, first case %r" % (
        stuck, len(counts.get("stuck_certificates", ())), len(ders), counts.get("first"))
    if name in ("synthetic", "mixed", "damaged"):
        # the case the model exists for was met: walks asked for a cooperative refill that does nothing, and went on alone
        assert counts["asked_in_vain"] > len(ders)
    if name != "damaged":
        assert counts["accepted"] > len(ders) // 3
    if name in ("hand_built", "damaged"):
        assert counts["accepted"] < len(ders)                             # both verdicts occur
    assert counts["rerun"] > 0                                            # flavour S hands a certificate without a window to the exact reader


def test_the_round_cap_stops_a_reader_that_never_holds(cap):
    """The model's own safety: a cap of a few rounds ends any walk that looks at its window more often than that — the
    certificate whose in-reach walk takes the most rounds — with DidNotTerminate, not a spin."""
    cfg = synth.config(seed=31, n_issuers=16)
    with pytest.raises(harness.DidNotTerminate):
        harness.walk_window_noreach(synth.leaf(cfg, 0)[0], 0, 224, "C", True, True, 1)
    assert cap >= 10_000
