"""The numbers DESIGN.md §21 and README.md quote for profiles/bench_pem_decode.json are that file's numbers
(scripts/bench_pem_decode.py writes it), as tests/test_docs_cpu.py holds the earlier sections to their files.  No GPU."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_numbers_quoted_for_the_pem_decode_measurement_are_the_files():
    d = json.loads(open(os.path.join(ROOT, "profiles", "bench_pem_decode.json")).read().splitlines()[-1])
    assert d["metric"] == "pem_decode" and d["regular"] == d["certs"] and d["irregular"]["regular"] == 0
    dec, enc, cp, irr = d["decode"], d["encode"], d["copy"], d["irregular"]
    quotes = ["%.2f M certificates" % (d["certs"] / 1e6), "%.2f GB of text" % (d["text_bytes"] / 1e9),
              "%.2f GB of payload" % (d["payload_bytes"] / 1e9), "takes %.1f ms" % dec["ms_median"],
              "%.1f M certificates/s" % (dec["certs_per_s"] / 1e6), "%.0f GB/s of text" % d["decode_text_GB_per_s"],
              "`encode` %.2f ms" % enc["ms_median"], "`copy` of the text %.2f ms" % cp["ms_median"],
              "%.1f × the encode" % d["ratio_decode_over_encode"], "%.1f × one pass over its text" % d["ratio_decode_over_copy"],
              "irregular leg takes %.1f ms" % irr["ms_median"], "%.2f × the regular leg per certificate" % d["ratio_irregular_over_regular_per_cert"]]
    flat = " ".join(open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read().split())
    assert "profiles/bench_pem_decode.json" in flat
    for q in quotes:
        assert q in flat, q
    # the split over the kernels: four calls of the decode leg under a kernel trace, total / 4
    import csv
    ms = {}
    for row in csv.DictReader(open(os.path.join(ROOT, "profiles", "pem_decode_kernel_stats_4m.csv"))):
        for k in ("k_pd_mark<false>", "k_pd_mark<true>", "k_pd_decode", "k_pd_check"):
            if k in row["Name"]:
                assert int(row["Calls"]) % 4 == 0
                ms[k] = float(row["TotalDurationNs"]) / 4e6
    assert "pem_decode_kernel_stats_4m.csv" in flat
    for k, v in ms.items():
        assert "`%s` %.1f ms" % (k, v) in flat, k
    assert len(ms) == 4 and 0.55 < (ms["k_pd_mark<false>"] + ms["k_pd_mark<true>"]) / d["decode"]["ms_median"] < 0.65      # "three fifths"
    readme = " ".join(open(os.path.join(ROOT, "README.md"), encoding="utf-8").read().split())
    for q in (quotes[3], quotes[4], quotes[5], quotes[9]):
        assert q in readme, q
