"""Cases for the scaled Horner chain of pf::exp256_split (csrc/u256.h, exp_sched), shared by
tests/test_exp_scale_host.py and tests/test_gpu_exp_scale.py.

The chain keeps its values scaled by 2^c and its factor shifted once, and shifts only at the
levels where the scale no longer fits the level's limbs (the un-scaling levels).  ``schedule``
mirrors the header's compile-time schedule in Python integers; ``pairs`` puts n = (e >> M) at
and around every un-scaling level (the binomials C(n, j) vanish above level n, so that level is
the last that matters), under bases whose t = ((b^(2^M) - 1) >> (M + 2)) mod 2^(254 - M) is all
ones (every carry of the products and of the factor's step), 1 (the factor is n - i + 1 itself)
and random."""
import random

MOD = 1 << 256
MASK = MOD - 1


def _v2(i):
    return (i & -i).bit_length() - 1


def _v2fact(j):
    return sum(_v2(k) for k in range(2, j + 1))


def terms(m):
    j = 1
    while (j + 1) * (m + 2) - _v2fact(j + 1) < 256:
        j += 1
    return j


def _literal_ok(k, limbs):
    """tmul_add takes the addend's limbs 2 .. L-1 as literals next to the column's carries."""
    return limbs >= 8 or all((k >> (32 * c)) & 0xFFFFFFFF <= 0xFFFFFFFF - (c - 1) for c in range(2, limbs))


def schedule(m):
    """{level: (c, un-scales the inner value, shifts the factor)} as exp_sched(m) derives it."""
    j = terms(m)
    inv = 1
    for k in range(1, j + 1):
        inv *= k >> _v2(k)
    inv = pow(inv, -1, MOD)
    out, e, cin = {}, 1, 0
    for i in range(j, 0, -1):
        e *= i >> _v2(i)
        p = 256 - ((i - 1) * (m + 2) - _v2fact(i - 1))
        limbs = (p + 31) // 32
        k = e * inv % (1 << (32 * limbs))
        v = _v2(i)

        def fits(c):
            return p + c <= 32 * limbs and _literal_ok((k << c) % (1 << (32 * limbs)), limbs)

        if fits(cin + v):
            out[i] = (cin + v, False, False)
        elif fits(v):
            out[i] = (v, cin != 0, False)
        else:
            out[i] = (0, cin != 0, v != 0)
        cin = out[i][0]
    return out


def unscaling_levels(m):
    return sorted(i for i, (_, un, sh) in schedule(m).items() if un or sh)


def base_with_t(m, t):
    """The b = 1 mod 4 with b^(2^m) = 1 + 2^(m+2) t mod 2^256, one bit at a time:
    adding 2^k to b flips bit k + m of b^(2^m) and nothing below it (k >= 2)."""
    target = (1 + (t << (m + 2))) % MOD
    b = 1
    for k in range(2, 256 - m):
        if ((pow(b, 1 << m, MOD) - target) >> (k + m)) & 1:
            b += 1 << k
    assert pow(b, 1 << m, MOD) == target
    return b


def bases(m, rng, nrandom):
    """(t all ones, t = 1, random odd bases)."""
    return [base_with_t(m, (1 << (254 - m)) - 1), base_with_t(m, 1)] + \
           [rng.getrandbits(256) | 1 for _ in range(nrandom)]


def pairs(m, nrandom_bases, seed=0x5CA1E):
    """(base, exponent) with n at and around every un-scaling level and n = 2^246 - 1 (cut to
    the exponent's 256 bits), e0 in {0, 255}."""
    rng = random.Random(seed + m)
    ns = sorted({n for lv in unscaling_levels(m) for n in (lv - 1, lv, lv + 1)} | {(1 << 246) - 1})
    return [(b, (e0 + (n << m)) & MASK) for b in bases(m, rng, nrandom_bases) for n in ns for e0 in (0, 255)]


def mixed_wave(w, m=8):
    """One wave of 64 (base, exponent) lanes at width w: odd and even bases alternate, n walks
    over the un-scaling levels and their neighbours (and 0 and 2^246 - 1), t all ones / 1 /
    random rotate."""
    import numpy as np

    rng = np.random.default_rng(0x5CA1E + w)
    Mw = (1 << w) - 1
    ones, tiny = bases(m, None, 0)
    ns = sorted({n for lv in unscaling_levels(m) for n in (lv - 1, lv, lv + 1)} | {(1 << 246) - 1})
    assert ns[0] == 0
    lanes = []
    for lane in range(64):
        b = (ones, tiny, int.from_bytes(rng.bytes(32), "little") | 1)[lane % 3]
        if lane % 4 == 3:
            b &= ~1
        n = ns[lane % len(ns)]
        lanes.append((b & Mw, ((0, 255)[(lane >> 2) & 1] + (n << m)) & Mw))
    return lanes


def is_mixed_wave(lanes):
    """Odd and even bases, each with exponents below and from 256 on."""
    return {(b & 1, e >= 256) for b, e in lanes} == {(0, False), (0, True), (1, False), (1, True)}
