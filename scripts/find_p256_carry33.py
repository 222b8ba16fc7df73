"""How tests/ec_corpus.py P256_CARRY33 was found: P-256 field elements a whose squaring a·a drives limb 8 of mont_mul's
accumulator to 2^32 (csrc/spki_key.h p256_redc_step `top`), and the curve points that carry one as x or as y.

The row sum t + b_i·a reaches 2^288 only if a lies within 2^160 of p, b_i = 2^32 − 1, and the two rows before had
b_i = m = 2^32 − 1 exactly (any shortfall of b or m costs ≈ 2^224 of t two rows later).  In a squaring b = a, so three
saturated limbs in a row leave a = 2^256 − 2^224 + 2^192 − e with 1 ≤ e ≤ 2^96 (limbs 3, 4, 5 = ffffffff).  With L = 2^96 − e
the accumulator after rows 0 … 2 is ≡ Q + M − L (mod 2^64), L² = 2^96·Q + M, and rows 3 and 4 take m = 2^32 − 1 exactly when
Q + M − 2L + 1 ≡ 0 (mod 2^64), which in e reads  e² mod (2^96 − 1) ≡ −1 (mod 2^64):  e² ≡ 2^64·k − 1 (mod 2^96 − 1) for
some k.  2^96 − 1 = 3²·5·7·13·17·97·193·241·257·673·65537·22253377: for the k whose right-hand side is a square modulo all
twelve, the roots per prime power are combined by the Chinese remainder theorem; p256_row_tops() is the judge of each.

    python scripts/find_p256_carry33.py [how many]      (a minute or two for the first forty)"""
import itertools
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import ec_corpus as E  # noqa: E402

N = 2 ** 96 - 1
FACTORS = ((3, 2), (5, 1), (7, 1), (13, 1), (17, 1), (97, 1), (193, 1), (241, 1), (257, 1), (673, 1), (65537, 1), (22253377, 1))
MODS = [q ** e for q, e in FACTORS]
assert math.prod(MODS) == N


def roots_mod(c, q, e):
    m = q ** e
    if m < 1000:
        return [r for r in range(m) if (r * r - c) % m == 0]
    r = E.sqrt_mod(c % q, q)
    return [] if r is None else sorted({r, (q - r) % q})


def crt(rs):
    x, m = 0, 1
    for r, q in zip(rs, MODS):
        x += m * (((r - x) * pow(m, -1, q)) % q)
        m *= q
    return x


def main(want):
    p, b = E.PRIMES["P256"], E.BS["P256"]
    top = 2 ** 256 - 2 ** 224 + 2 ** 192
    found, k = 0, 0
    while found < want:
        k += 1
        c = (k << 64) - 1
        per = [roots_mod(c % m, q, e) for (q, e), m in zip(FACTORS, MODS)]
        if not all(per):
            continue
        for combo in itertools.product(*per):
            r = crt(combo)
            for e in (r, r + N):
                a = top - e
                if 1 <= e <= 2 ** 96 and max(E.p256_row_tops(a, a)) >> 32:
                    found += 1
                    y, x = E.sqrt_mod((a ** 3 - 3 * a + b) % p, p), E.x_of_y("P256", a)
                    print("%#x  as x: %s  as y: %s" % (a, "y = %#x" % y if y is not None else "-", "x = %#x" % x if x is not None else "-"),
                          flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 8)
