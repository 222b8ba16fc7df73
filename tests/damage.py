"""In-place, length-preserving injuries to a synthetic leaf, one per family of reference-profile rules (subjectAltName
elements, the bodies of five more extensions, Name strings).  What each one must cost is the ORACLE's call; the tests that use
them assert the counts.  Shared by the GPU tests (tests/test_gpu_scale.py, tests/test_gpu_view_order.py) and the CPU model of
an out-of-reach lane (tests/test_view_order_cpu.py)."""


def ext_list(der, c):
    """(oid content, value offset, value end) of every extension of a synthetic leaf (short and two-octet lengths only)."""
    def hdr(p):
        ln = der[p + 1]
        if ln < 0x80:
            return p + 2, p + 2 + ln
        k = ln & 0x7f
        return p + 2 + k, p + 2 + k + int.from_bytes(der[p + 2:p + 2 + k], "big")
    out, e = [], c.exts_off
    while e < c.exts_end:
        x, x_end = hdr(e)
        o, o_end = hdr(x)
        v = o_end
        if der[v] == 0x01:
            v = hdr(v)[1]
        out.append((bytes(der[o:o_end]), *hdr(v)))
        e = x_end
    return out


def hurt(der, kind, c):
    """One in-place, length-preserving injury per rule family; returns the damaged bytes.  What each one must cost is the
    ORACLE's call — the comments say what is expected, the test asserts the counts."""
    b = bytearray(der)
    exts = {oid: (v, ve) for oid, v, ve in ext_list(der, c)}
    san_v, san_e = exts[b"\x55\x1d\x11"]
    first = san_v + (2 if b[san_v + 1] < 0x80 else 2 + (b[san_v + 1] & 0x7f))     # the first GeneralName
    if kind == "san_uri_ctl":          # a URI with a control character: url.Parse fails — fatal
        b[first] = 0x86; b[first + 3] = 0x01
    elif kind == "san_uri_space_host":  # "//a b…": invalid character in host name — fatal
        b[first] = 0x86; b[first + 2] = 0x2f; b[first + 3] = 0x2f; b[first + 5] = 0x20
    elif kind == "san_ip_length":      # an iPAddress of 22..49 octets: CT-go's NON-fatal finding — precertificates only
        b[first] = 0x87
    elif kind == "san_truncated":      # the last dNSName claims one octet too many: "data truncated" — fatal
        p = first
        while p + 2 + b[p + 1] < san_e:
            p += 2 + b[p + 1]
        b[p + 1] += 1
    elif kind == "san_not_a_sequence":  # "bad SAN sequence" — fatal
        b[san_v] = 0x31
    elif kind == "san_uri_deep":       # a bad URI far into the subjectAltName (beyond the walk's second window) — fatal
        p, k = first, 0
        while p + 2 + b[p + 1] < san_e and k < 9:
            p += 2 + b[p + 1]; k += 1
        b[p] = 0x86; b[p + 4] = 0x7f
    elif kind == "key_usage_pad":      # parseBitString: pad count 8 — fatal
        v, _ = exts[b"\x55\x1d\x0f"]; b[v + 2] = 0x08
    elif kind == "eku_element":        # SEQUENCE OF OBJECT IDENTIFIER with a UTF8String in it — fatal
        v, _ = exts[b"\x55\x1d\x25"]; b[v + 2] = 0x0c
    elif kind == "ski_tag":            # not an OCTET STRING — fatal
        v, _ = exts[b"\x55\x1d\x0e"]; b[v] = 0x03
    elif kind == "aki_fit":            # the keyIdentifier does not fit — fatal
        v, _ = exts[b"\x55\x1d\x23"]; b[v + 3] = 0x7f
    elif kind == "crl_relative_name":  # fullName → nameRelativeToCRLIssuer holding a URI where a SET belongs — fatal
        v, _ = exts[b"\x55\x1d\x1f"]; b[v + 6] = 0xa1
    elif kind == "crl_reasons":        # distributionPoint → reasons [1] with pad count 0x30 — fatal
        v, _ = exts[b"\x55\x1d\x1f"]; b[v + 4] = 0x81
    elif kind == "name_constraints":   # subjectKeyIdentifier relabelled nameConstraints: its value is no SEQUENCE — fatal
        v, _ = exts[b"\x55\x1d\x0e"]; b[v - 3] = 0x1e
    elif kind == "issuer_utf8":        # the issuer's O (UTF8String) is not UTF-8: a string finding — precertificates only
        at = der.index(b"Synth CA Org", c.issuer_off); b[at + 3] = 0xff
    elif kind == "subject_utf8":       # … and the subject's CN
        at = der.index(b"host-", c.issuer_off + c.issuer_len); b[at + 2] = 0xc0
    else:
        raise KeyError(kind)
    return bytes(b)


KINDS_FATAL = ["san_uri_ctl", "san_uri_space_host", "san_truncated", "san_not_a_sequence", "san_uri_deep", "key_usage_pad",
               "eku_element", "ski_tag", "aki_fit", "crl_relative_name", "crl_reasons", "name_constraints"]
KINDS_FINDING = ["san_ip_length", "issuer_utf8", "subject_utf8"]
