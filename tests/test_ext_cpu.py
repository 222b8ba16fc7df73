"""strict_extensions (opt-in): the bodies of the extensions Go's parseCertificate unmarshals by plain struct rules — one
hand-built certificate per rule, oracle vs the product walk (host build), OpenSSL as a third opinion where it has one.
CPU only."""
import random

from oracle import oracle as orc
from tests import der as D
from tests import harness
from tests.ext_corpus import (CLEAN, FATAL, FINDING, STRING_FINDING, TABLES, AIA_OID, OCSP, POL, EKU_SRV, EKU_CLI,  # noqa: F401
                               SIA_OID, CA_REPO, IPADDR_OID, ASNUM_OID, NULL, SCT_OID, x, aia, sia, ipaddr, asnum, bits, san, uri, dps,
                               fullname, nc, sct_ext, ipaddr_bodies, asnum_bodies)      # (tests/test_gpu_ext.py takes them from here)


NF_STRING, NF_EXT = 4, 16


def verdicts(c, findings=None):
    """(structure parses, strict_extensions accepts) — asserted equal between the oracle and the product, and with them
    the NON-fatal findings of an accepted certificate: what CT-go files as non-fatal inside an extension body
    (WALK_NF_EXT ⇔ orc_cert.ext_findings) and, with strict_strings on as well, the character sets inside a distribution
    point's nameRelativeToCRLIssuer (WALK_NF_STRING ⇔ string_findings | ext_string_findings).  findings: a list that
    receives (ext finding, string finding) of an accepted certificate."""
    o = orc.parse_cert(c)
    harness.product_set_ext(False)
    p0 = harness.product_walk(c)
    harness.product_set_ext(True)
    p1 = harness.product_walk(c)
    harness.product_set_strings(True)
    p2 = harness.product_walk(c)
    harness.product_set_strings(False)
    harness.product_set_ext(False)
    assert bool(o.ok) == bool(p0.ok), (o.ok, o.err_site, p0.ok)
    strict_ok = bool(o.ok) and not o.ext_fatal
    assert strict_ok == bool(p1.ok) == bool(p2.ok), (o.ok, o.ext_fatal, p1.ok, p2.ok)
    if strict_ok:
        assert bool(p1.nonfatal & NF_EXT) == bool(o.ext_findings) == bool(p2.nonfatal & NF_EXT), (o.ext_findings, p1.nonfatal)
        assert not (p1.nonfatal & NF_STRING)
        assert bool(p2.nonfatal & NF_STRING) == bool(o.string_findings or o.ext_string_findings), \
            (o.string_findings, o.ext_string_findings, p2.nonfatal)
        if findings is not None:
            findings.append((bool(o.ext_findings), bool(o.ext_string_findings)))
    return bool(o.ok), strict_ok


def good(e):
    assert verdicts(D.cert(exts=[e])) == (True, True), e.hex()


def bad(e):
    assert verdicts(D.cert(exts=[e])) == (True, False), e.hex()      # only the switch rejects it


def nonfatal(e, ext=True, strings=False):
    f = []
    assert verdicts(D.cert(exts=[e]), f) == (True, True), e.hex()
    assert f == [(ext, strings)], (f, e.hex())


def check_table(name, clean=0, fatal=0, finding=0, string_finding=0):
    """Every row of one table of tests/ext_corpus.py, where the bodies are stated: a clean row passes the switch (and files
    nothing), a fatal one is rejected by the switch alone, a finding is filed and the certificate accepted.  The counts are
    the rows each verdict has at the least: the cases this module held before the tables moved."""
    seen = {CLEAN: 0, FATAL: 0, FINDING: 0, STRING_FINDING: 0}
    for e, verdict in TABLES[name]:
        seen[verdict] += 1
        if verdict == CLEAN:
            good(e)
            nonfatal(e, ext=False)
        elif verdict == FATAL:
            bad(e)
        else:
            nonfatal(e, ext=verdict == FINDING, strings=verdict == STRING_FINDING)
    assert seen[CLEAN] >= clean and seen[FATAL] >= fatal and seen[FINDING] >= finding and seen[STRING_FINDING] >= string_finding, seen


def test_key_usage_is_one_bit_string():
    check_table("key_usage", clean=3, fatal=9)


def test_subject_key_identifier_is_one_octet_string():
    check_table("subject_key_identifier", clean=2, fatal=5)


def test_ext_key_usage_is_a_sequence_of_oids():
    check_table("ext_key_usage", clean=2, fatal=8)


def test_authority_key_identifier_optional_first_field():
    check_table("authority_key_identifier", clean=6, fatal=6)


def test_certificate_policies_is_a_sequence_of_sequences_led_by_an_oid():
    check_table("certificate_policies", clean=3, fatal=7)


def test_authority_info_access_elements_carry_an_oid_and_a_location():
    check_table("authority_info_access", clean=2, fatal=7)


def test_subject_info_access_is_parsed_like_authority_info_access():
    """CT-go's fork knows 1.3.6.1.5.5.7.1.11 (the standard library does not): []accessDescription filling the value, failure
    and trailing data fatal, an empty list an error (recalled — go.mod:10; round 6); the neighbouring id-pe
    numbers are not this extension."""
    check_table("subject_info_access", clean=2 + 3, fatal=9)


def test_rfc3779_address_blocks_findings_are_non_fatal():
    """sbgp-ipAddrBlock as CT-go's x509/rpki.go decodes it (recalled; go.mod:10): strict asn1.Unmarshal calls, every failure
    an nfe.AddError — the certificate parses, a precertificate and a Chain[0] issuer are dropped over the finding."""
    check_table("ip_addr_block", clean=6, finding=25 + 1)
    ok, findings = ipaddr_bodies()
    for v in ok:
        f = []
        assert verdicts(D.cert(exts=[ipaddr(v)]), f) == (True, True), v.hex()
        assert f == [(False, False)], (f, v.hex())
    for v in findings:
        nonfatal(ipaddr(v))
    nonfatal(ipaddr(findings[5], critical=False))
    # a finding next to a fatal body elsewhere stays fatal; the switch off: nothing is looked at
    bad_and = D.cert(exts=[ipaddr(findings[0]), x(15, D.tlv(0x03, b""))])
    assert verdicts(bad_and) == (True, False)


def test_rfc3779_as_identifiers_findings_are_non_fatal():
    """sbgp-autonomousSysNum: struct { ASNum RawValue `optional,tag:0`; RDI RawValue `optional,tag:1` } filling the value; a
    choice's contents are NULL or one []RawValue of INTEGERs (`int`: minimal, at most 8 octets) and ASIDRange pairs."""
    check_table("as_identifiers", clean=9, finding=19)
    ok, findings = asnum_bodies()
    for v in ok:
        f = []
        assert verdicts(D.cert(exts=[asnum(v)]), f) == (True, True), v.hex()
        assert f == [(False, False)], (f, v.hex())
    for v in findings:
        nonfatal(asnum(v))


def test_subject_alt_name_is_a_sequence_of_general_names():
    """forEachSAN: one universal constructed SEQUENCE filling the value, every element a TLV that fits, dispatched on the
    tag NUMBER alone; an iPAddress of another length than 4 or 16 is a NON-fatal finding (the stdlib fails)."""
    check_table("subject_alt_name", clean=5, fatal=8, finding=10)


def test_subject_alt_name_uri_goes_through_url_parse():
    check_table("subject_alt_name_uri", clean=42, fatal=45 + 2)


def test_crl_distribution_points_follow_the_struct_rules():
    check_table("crl_distribution_points", clean=12, fatal=24, finding=1, string_finding=1)
    u = D.tlv(0x86, b"http://crl.example/a.crl")
    # where the URIs lie (kernels/meta*.h, orc_cert_meta): FullName elements with tag NUMBER 6, positional fields
    def uris(value):
        c = D.cert(exts=[x(31, value)])
        _, ulist, m = orc.cert_meta(c)
        o = orc.parse_cert(c)
        at = c.index(value)
        got = harness.product_crl_uris(c, at, at + len(value))
        want = None if m.bad_crl else ulist[:8]
        assert got == want and o.ok, (got, want)
        return got
    assert uris(D.seq(D.seq(fullname(u, D.tlv(0x06, b"oid-as-uri"), D.tlv(0x82, b"dns"), D.tlv(0xa6, b"cons"))))) == \
        [b"http://crl.example/a.crl", b"oid-as-uri", b"cons"]
    assert uris(D.seq(D.seq(D.tlv(0x81, b"\x00"), fullname(u)))) == []                # out of order: not reached
    assert uris(D.seq(D.seq(fullname(u)), D.seq(fullname(D.tlv(0x86, b"second"))))) == [b"http://crl.example/a.crl", b"second"]
    assert uris(D.seq(D.seq(fullname(u), b"\x9f"))) is None
    assert uris(D.seq(D.seq(D.tlv(0xa0, D.tlv(0xa0, u) + D.tlv(0xa1, D.tlv(0x30, b"")))))) == [b"http://crl.example/a.crl"]   # RelativeName contents: not the metadata's business


def test_name_constraints_as_cryptobyte_reads_them():
    check_table("name_constraints", clean=9 + 13, fatal=13 + 2 * 37)


def test_embedded_sct_list_findings_are_non_fatal():
    check_table("sct_list", clean=2 + 1, finding=13)


def test_other_extensions_and_the_switch_off():
    # unknown extensions are not looked into
    for e in (x(18, b"\xff\xff"), x(9, b""), D.seq(D.tlv(0x06, b"\x2a\x03\x04"), D.tlv(0x04, b"\xff"))):
        good(e)
    # a repeated extension: every occurrence is checked
    c = D.cert(exts=[x(15, D.tlv(0x03, b"\x05\xa0")), x(15, D.tlv(0x03, b"\x08\x00"))])
    assert verdicts(c) == (True, False)
    # the critical flag and long-form headers in front of the value do not matter
    c = D.cert(exts=[D.ext(15, D.tlv(0x03, b"\x08\x00"), critical=True)])
    assert verdicts(c) == (True, False)
    long_form = D.seq(D.oid(0x55, 0x1d, 14), b"\x04\x81\x03" + D.tlv(0x04, b"\x11") )
    assert verdicts(D.cert(exts=[long_form]))[0] is False              # the extnValue length itself is not minimal: structure
    # the TBSCertificate walk (strict_leaf) applies the same rule
    c = D.cert(exts=[x(14, D.tlv(0x03, b"\x00\x11"))])
    o = orc.parse_cert(c)
    tbs = c[o.tbs_off:o.tbs_off + o.tbs_len]
    harness.product_set_ext(True)
    assert harness.product_walk_tbs(tbs).ok == 0
    harness.product_set_ext(False)
    assert harness.product_walk_tbs(tbs).ok == 1 and orc.parse_tbs(tbs).ext_fatal != 0


def test_real_world_certificates_pass_the_switch(golden_certs=None):
    """Every certificate of the reference's goldens and of the system CA bundle that parses also passes strict_extensions."""
    import glob
    import ssl
    ders = []
    for p in glob.glob("tests/golden/*.pem"):
        for blk in open(p).read().split("-----BEGIN CERTIFICATE-----")[1:]:
            ders.append(ssl.PEM_cert_to_DER_cert("-----BEGIN CERTIFICATE-----" + blk.split("-----END CERTIFICATE-----")[0] + "-----END CERTIFICATE-----\n"))
    for path in ("/etc/ssl/certs/ca-certificates.crt",):
        try:
            txt = open(path).read()
        except OSError:
            continue
        for blk in txt.split("-----BEGIN CERTIFICATE-----")[1:]:
            ders.append(ssl.PEM_cert_to_DER_cert("-----BEGIN CERTIFICATE-----" + blk.split("-----END CERTIFICATE-----")[0] + "-----END CERTIFICATE-----\n"))
    assert len(ders) >= 3
    n_ok = 0
    for d in ders:
        a, b = verdicts(d)
        if a:
            assert b, "a real certificate fails strict_extensions"
            n_ok += 1
    assert n_ok >= 3


def rich_seeds():
    """Certificates that carry every extension body strict_extensions looks into (the fuzz campaigns' seeds)."""
    old = [x(15, D.tlv(0x03, b"\x05\xa0")), x(14, D.tlv(0x04, b"\x11" * 20)), x(37, D.seq(EKU_SRV, EKU_CLI)),
           x(35, D.seq(D.tlv(0x80, b"\x22" * 20))), x(32, D.seq(D.seq(POL))),
           aia(D.seq(D.seq(OCSP, D.tlv(0x86, b"http://o.example")))), D.BC_NOT_CA]
    u = D.tlv(0x86, b"http://crl.example/a.crl")
    rel = D.tlv(0xa1, D.tlv(0x31, D.seq(D.oid(0x55, 4, 3), D.tlv(0x13, b"rel name"))))
    lst = lambda *q: D.tlv(0x04, len(b"".join(q)).to_bytes(2, "big") + b"".join(q))
    web = [san(D.tlv(0x82, b"a.example"), D.tlv(0x82, b"*.b.example"), D.tlv(0x87, bytes(4)), D.tlv(0x87, bytes(16)),
               uri("https://u:p@a.example:8443/x%20y?q#f"), D.tlv(0x81, b"m@a.example"), uri("http://[fe80::1%25en0]:80/")),
           dps(D.seq(fullname(u)), D.seq(D.tlv(0xa0, rel), D.tlv(0x81, b"\x01\x06"), D.tlv(0xa2, D.tlv(0xa4, b"")))),
           sct_ext(lst(b"\x00\x03abc", b"\x00\x02xy")), D.BC_NOT_CA]
    ca = [nc([D.tlv(0x82, b".example.com"), D.tlv(0x87, bytes(4) + b"\xff\xff\x00\x00"), D.tlv(0x81, b"user@example.com"),
              D.tlv(0x81, b'"q s"@example.com'), D.tlv(0x86, b".example.com")],
             [D.tlv(0x87, bytes(16) + b"\xff" * 6 + bytes(10)), D.tlv(0x82, b"x.y"), D.tlv(0x86, b"1:2:3:4:5:6:7")]),
          D.BC_CA]
    # round 6: CT-go's own extensions — subjectInfoAccess, RFC 3779 address blocks and AS identifiers
    i = lambda v: D.tlv(0x02, v)
    rpki = [sia(D.seq(D.seq(CA_REPO, D.tlv(0x86, b"rsync://repo.example/ca/")))),
            ipaddr(D.seq(D.seq(D.tlv(0x04, b"\x00\x01"), D.seq(bits(b"\x0a"), D.seq(bits(b"\xc0\xa8"), bits(b"\xc0\xa9\x80", 7)))),
                         D.seq(D.tlv(0x04, b"\x00\x02\x01"), NULL))),
            asnum(D.seq(D.tlv(0xa0, D.seq(i(b"\x00\xfd\xe8"), D.seq(i(b"\x01"), i(b"\x02")))), D.tlv(0xa1, NULL))), D.BC_CA]
    return [D.cert(exts=old), D.cert(exts=web), D.cert(exts=ca), D.cert(exts=web[:2] + old), D.cert(exts=rpki)]


def mutate_exts(rng, der, lo, hi):
    c = bytearray(der)
    for _k in range(rng.choice((1, 1, 2, 3))):
        p = rng.randrange(lo, hi)
        c[p] = rng.choice((c[p] ^ (1 << rng.randrange(8)), rng.randrange(256), 0x00, 0x80, 0x30, 0x06, 0x04, 0x03, 0x25, 0x2e, 0x3a,
                           0x40, 0x5b, 0x5d, 0x2f, 0x23, 0x3f, 0x5c, 0x22, 0xa0, 0xa1, 0x86, 0x87, 0x82, 0x81, 0x31))
    return bytes(c)


def test_product_equals_oracle_on_mutated_extension_bodies():
    rng = random.Random(20261012)
    seeds = rich_seeds()
    rng_ranges = []
    for sd in seeds:
        o = orc.parse_cert(sd)
        assert o.ok and not o.ext_fatal and not o.ext_findings
        rng_ranges.append((o.exts_off, o.exts_end))
    n = rejected = nf = 0
    for _ in range(40000):
        k = rng.randrange(len(seeds))
        f = []
        a, b = verdicts(mutate_exts(rng, seeds[k], *rng_ranges[k]), f)
        n += 1
        rejected += a and not b
        nf += bool(f and (f[0][0] or f[0][1]))
    assert rejected > 1000 and nf > 20                                 # the switch had something to say, both ways


def test_product_equals_oracle_on_random_uris_and_constraints():
    """Strings made for the content parsers (url.Parse, parseRFC2821Mailbox, net.ParseIP, domainToReverseLabels, the IP mask):
    product (host build) ≡ oracle on each, as a subjectAltName URI and as each kind of name constraint."""
    rng = random.Random(20261013)
    alpha_u = "ab1:/@[]%25.?#-+~! \\\"<>_*|\x01\x7f\x80é"
    alpha_m = "ab1.@\\\" -!#\x0b\x7f"
    alpha_i = "0123456789abcdefg:.:."
    seen = set()
    for t in range(12000):
        a = (alpha_u, alpha_m, alpha_i)[t % 3]
        sx = "".join(rng.choice(a) for _ in range(rng.randrange(0, 14)))
        if t % 7 == 0:
            sx = rng.choice(("http://", "//", "http://[", "x:", "http://u@", "")) + sx
        b = sx.encode("latin-1")
        e = [san(uri(b)), nc([D.tlv(0x86, b)]), nc(None, [D.tlv(0x81, b)]), nc([D.tlv(0x82, b)])][rng.randrange(4)]
        seen.add(verdicts(D.cert(exts=[e]))[1])
        if t % 5 == 0:
            m = bytes(rng.choice((0, 0xff, 0x80, 0xfe, 0xf0, 0x01)) for _ in range(rng.choice((4, 4, 16, 3))))
            seen.add(verdicts(D.cert(exts=[nc([D.tlv(0x87, bytes(len(m)) + m)])]))[1])
    assert seen == {True, False}
