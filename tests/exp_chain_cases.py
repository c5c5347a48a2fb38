"""Cases for the fused powering chain of pf::exp256_split (csrc/u256.h), shared by
tests/test_exp_chain_host.py and tests/test_gpu_exp_chain.py.

Where the series runs, b^e0 (e0 = e mod 2^M) is the product of the squarings b^(2^k) that
climb to the series' step b^(2^M) - 1, one factor per set bit of e0.  What can go wrong there
is a bit of e0 taken from the wrong place, a factor taken one squaring early or late, the first
factor (bit 0, the base itself) or the last (bit M - 1, the last value before the step), and
the lanes that sit in a wave that runs the series without needing it (n = 0, even bases).  So:
every e0 of the configured split's eight bits, the single-bit and alternating patterns, n = 0,
1 and all ones, bases 0, 1, 2, 2^32 and 2^w - 1, and the even bases' edges at e = 255 / 256.
Everything is checked against pow(b, e, 1 << w)."""
import random

import exp_scale_cases as S

SPLIT = 8            # PF_EXP_SPLIT as configured in csrc/u256.h
N_BIG = (1 << 246) - 1
PATTERNS = (0x01, 0x80, 0x55, 0xAA, 0xFF)
PATTERN_NS = (0, 1, N_BIG)


def e0_patterns(m):
    """The single-bit and alternating patterns; a wider split adds its own top bit, its all
    ones and the alternating patterns over all of its bits."""
    out = list(PATTERNS)
    if m > 8:
        full = (1 << m) - 1
        out += [1 << (m - 1), full, 0x55555555 & full, 0xAAAAAAAA & full]
    return out


def three_bases(m, seed=0xC4A1):
    """(odd random, t all ones, even random) at split m."""
    rng = random.Random(seed + m)
    return [rng.getrandbits(256) | 1, S.base_with_t(m, (1 << (254 - m)) - 1), rng.getrandbits(256) & ~1]


def _e(e0, n, m):
    return (e0 + (n << m)) & S.MASK


def every_e0(m, seed=0xE0):
    """Every e0 in 0..255 with n != 0 (1, all ones and random in turn) under the three bases;
    the even base also with n = 0, where its power is not simply 0."""
    rng = random.Random(seed + m)
    odd, ones, even = three_bases(m)
    out = []
    for e0 in range(256):
        n = (1, N_BIG, rng.getrandbits(246) | 1)[e0 % 3]
        out += [(odd, _e(e0, n, m)), (ones, _e(e0, n, m)), (even, _e(e0, n, m)), (even, e0)]
    return out


def pattern_pairs(m):
    return [(b, _e(e0, n, m)) for b in three_bases(m) for e0 in e0_patterns(m) for n in PATTERN_NS]


def special_bases(m, w=256):
    es = [_e(0xFF, 1, m), 0x55, _e(0xAA, N_BIG, m), 0, 1]
    return [(b, e) for b in (0, 1, 2, 1 << 32, (1 << w) - 1) for e in es]


def even_edges(m, seed=0xEE):
    rng = random.Random(seed + m)
    even = rng.getrandbits(256) & ~1
    odd = rng.getrandbits(256) | 1
    return [(2, 255), (2, 256), (2, 254), (2, 1 << 254), (2, (1 << 255) | 5), (even, (1 << 254) + 3),
            (even, (3 << 254) | 0xAA), (6, 255), (6, 99),
            # odd bases: the unit group has exponent 2^254, bits >= 254 change nothing
            (odd, (1 << 254) | 0x55), (odd, (3 << 254) | _e(0xFF, 12345, m))]


def host_pairs(m):
    return every_e0(m) + pattern_pairs(m) + special_bases(m) + even_edges(m)


def gpu_pairs(w):
    """About a hundred of the host's rows at the configured split, cut to width w."""
    m = SPLIT
    pairs = pattern_pairs(m) + special_bases(m, w) + even_edges(m)
    rest = every_e0(m)
    step = len(rest) // (100 - len(pairs))
    pairs += rest[3::step][:100 - len(pairs)]
    mask = (1 << w) - 1
    return [(b & mask, e & mask) for b, e in pairs]


# ---- mixed 64-lane waves: (base, exponent) per lane -------------------------------------

def split_e(e, m=SPLIT):
    """(e0, n) as the kernel splits the exponent."""
    return e & ((1 << m) - 1), (e >> m) & ((1 << (254 - m)) - 1)


def runs_series(lanes, m=SPLIT):
    return any((b & 1) and split_e(e, m)[1] for b, e in lanes)


def wave_mixed(w, seed=0xA):
    """(a) odd and even bases alternate, e0 walks the patterns, n = 0 in a third of the odd
    lanes: the series runs for the wave while those lanes need (1 + X)^0 = 1."""
    rng = random.Random(seed + w)
    pats = (0x00,) + PATTERNS
    lanes = []
    for lane in range(64):
        b = rng.getrandbits(256) | 1
        if lane & 1:
            b &= ~1
        n = 0 if (lane >> 1) % 3 == 0 else (1, N_BIG, rng.getrandbits(246))[(lane >> 1) % 3 - 1 + (lane >> 5)]
        pair = lane >> 1  # the patterns shift by one every round, so each meets n = 0 and n != 0
        lanes.append((b, _e(pats[(pair + pair // len(pats)) % len(pats)], n, SPLIT)))
    return _cut(lanes, w)


def wave_bits_clear(w, seed=0xB):
    """(b) bits 3 and 6 of e0 clear in every lane (every other bit set in some lane): the
    chain's products of steps 3 and 6 have no lane to serve."""
    rng = random.Random(seed + w)
    lanes = []
    for lane in range(64):
        b = rng.getrandbits(256) | 1
        if lane % 8 == 5:
            b &= ~1
        e0 = (rng.getrandbits(8) | (1 << (lane % 8))) & ~0x48
        lanes.append((b, _e(e0, rng.getrandbits(246) | 1, SPLIT)))
    return _cut(lanes, w)


def wave_short_e0(w, seed=0xC):
    """(c) every e0 < 8 with n != 0: three bits of e0 is all the wave has."""
    rng = random.Random(seed + w)
    lanes = [(rng.getrandbits(256) | 1, _e(lane % 8, rng.getrandbits(246) | 1, SPLIT)) for lane in range(64)]
    return _cut(lanes, w)


def wave_all_even(w, seed=0xD):
    """(d) no series: every base even (e below and above 256)."""
    rng = random.Random(seed + w)
    lanes = []
    for lane in range(64):
        b = rng.getrandbits(256) & ~1
        if lane % 4 == 0:
            b = (2, 6, 1 << 32, 0)[(lane >> 2) % 4]
        e = rng.getrandbits(8) if lane % 3 else _e(rng.getrandbits(8), rng.getrandbits(246), SPLIT)
        lanes.append((b, e))
    lanes[1] = (2, 255)
    lanes[2] = (2, 256)
    return _cut(lanes, w)


def wave_all_n0(w, seed=0xE):
    """(d) no series: every n = 0 (odd and even bases, every length of e0 from 0 to 8 bits)."""
    rng = random.Random(seed + w)
    lanes = []
    for lane in range(64):
        b = rng.getrandbits(256) | 1
        if lane % 4 == 1:
            b &= ~1
        e0 = rng.getrandbits(8) >> (lane % 9)
        lanes.append((b, PATTERNS[lane % 5] if lane % 7 == 0 else e0))
    lanes[0] = (lanes[0][0], 0xFF)
    lanes[63] = (lanes[63][0], 0)
    return _cut(lanes, w)


def _cut(lanes, w):
    mask = (1 << w) - 1
    return [(b & mask, e & mask) for b, e in lanes]


# ---- what each wave is there for: predicates over 64 (base, exponent) lanes ----------------

def _e0s(lanes):
    return [split_e(e)[0] for _, e in lanes]


def is_mixed(lanes):
    odd_n0 = [b & 1 and split_e(e)[1] == 0 for b, e in lanes]
    n_odd = sum(b & 1 for b, _ in lanes)
    return (runs_series(lanes) and n_odd == 32 and 3 * sum(odd_n0) >= n_odd
            and {e0 for (b, _), e0 in zip(lanes, _e0s(lanes)) if b & 1} >= set(PATTERNS))


def has_bits_clear(lanes):
    e0s = _e0s(lanes)
    seen = 0
    for e0 in e0s:
        seen |= e0
    return runs_series(lanes) and seen == 0xFF & ~0x48 and all(split_e(e)[1] for _, e in lanes)


def is_short(lanes):
    return (runs_series(lanes) and max(e0.bit_length() for e0 in _e0s(lanes)) == 3
            and set(_e0s(lanes)) == set(range(8)) and all(split_e(e)[1] for _, e in lanes))


def all_even(lanes):
    return (not runs_series(lanes) and not any(b & 1 for b, _ in lanes)
            and {e >= 256 for _, e in lanes} == {False, True})


def all_n0(lanes):
    return (not runs_series(lanes) and all(e < 256 for _, e in lanes)
            and {b & 1 for b, _ in lanes} == {0, 1}
            and {e.bit_length() for _, e in lanes} >= {0, 1, 8})


WAVES = {
    "mixed": (wave_mixed, is_mixed),
    "bits_3_6_clear": (wave_bits_clear, has_bits_clear),
    "short_e0": (wave_short_e0, is_short),
    "no_series_even": (wave_all_even, all_even),
    "no_series_n0": (wave_all_n0, all_n0),
}
