"""Operands for the product routines of csrc/u256.h (mul256, sqr256, the truncated multiply-adds
of EXP's series, exp256_split), shared by tests/test_products_host.py (the C mirror, CPU) and
tests/test_gpu_products.py (the inline-asm columns, GPU).

A model of the column scan in Python integers says which columns of a product carry out of the
64-bit accumulator, so that the operands can be asserted to do what they are for."""

M256 = (1 << 256) - 1
F = 0xFFFFFFFF
SPLIT = 8            # PF_EXP_SPLIT as configured in csrc/u256.h


def limbs(v):
    return [(v >> (32 * i)) & F for i in range(8)]


def carrying_columns(a, b):
    """Columns of mul256(a, b) in which some v_mad_u64_u32 carries out of bit 63."""
    x, y = limbs(a), limbs(b)
    acc, out = 0, set()
    for c in range(8):
        hi = 0
        for t in range(c + 1):
            acc += x[t] * y[c - t]
            if acc >> 64:
                hi += 1
                acc &= (1 << 64) - 1
                out.add(c)
        acc = (acc >> 32) | (hi << 32)
    return out


def mul_rows():
    """(a, b) pairs: see the module docstrings of the two tests."""
    rows = [(M256, M256)]
    # every carry add fires: each mad of columns 1..5 carries (column 0 has one product)
    assert carrying_columns(M256, M256) >= {1, 2, 3, 4, 5}
    for c in range(1, 6):
        v = F | (F << (32 * c))
        assert carrying_columns(v, v) & {1, 2, 3, 4, 5} == {c}, c
        rows.append((v, v))
    for i in range(8):
        for j in range(8):
            rows.append((0xFFFFFFFF << (32 * i), 0x87654321 << (32 * j)))
    for k in (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192, 193,
              223, 224, 225, 254, 255):
        for j in (31, 32, 33, 255 - k if k < 255 else 1):
            rows.append((1 << k, 1 << j))
            rows.append(((1 << k) - 1, (1 << j) + 1))
            rows.append(((1 << k) + 1, M256 >> (j % 64)))
    return rows


# exponent classes that exp256_split separates: does the series run (odd base and e >> SPLIT
# non-zero in some lane), and the wave's bit length nb0 of e mod 2^SPLIT
N = 5
EXP_EXPS = [0, 1, 2, 3, 255, 256, 256 * N, 256 * N + 1, 256 * N + 2, 256 * N + 3, 1 << 84, 1 << 254, M256]
EXP_BASES = [1, 3, 0xDEADBEEF | 1, M256, (1 << 255) + 1, (0x9E3779B97F4A7C15F39CC0605CEDC834 << 128) | 0x1234567,
             0, 2, 6, 1 << 31, 1 << 255, M256 - 1, 0xA5A5A5A5 << 200]


def exp_class(b, e):
    """(series, nb0) of a wave whose lanes all hold (b, e)."""
    series = bool(b & 1) and ((e >> SPLIT) & ((1 << (254 - SPLIT)) - 1)) != 0
    return series, (e & ((1 << SPLIT) - 1)).bit_length()


def exp_rows():
    rows = [(b, e) for b in EXP_BASES for e in EXP_EXPS]
    seen = {(s, min(n, 2) if s else n) for s, n in (exp_class(b, e) for b, e in rows)}
    assert seen >= {(True, 0), (True, 1), (True, 2), (False, 0), (False, 1), (False, 2), (False, 8)}, seen
    return rows


# Mixed waves: 63 lanes of one class and one lane of another.  Each entry: (name, the 63 lanes'
# (b, e) as a function of the lane, the odd lane's (b, e)).
def _b(i, odd=True):
    v = (0x9E3779B97F4A7C15F39CC0605CEDC834 * (2 * i + 3) ** 7) & M256
    return v | 1 if odd else v & ~1


WAVES = {
    # no series anywhere: the window's table is needed by one lane only / by all but one
    "nb0_0_one_lane_1": (lambda i: (_b(i), 0), (_b(99), 1)),
    "nb0_1_one_lane_0": (lambda i: (_b(i), 1), (_b(99), 0)),
    "nb0_1_one_lane_2": (lambda i: (_b(i), i & 1), (_b(99), 2)),
    "nb0_0_one_lane_8": (lambda i: (_b(i, i & 1), 0), (_b(99), 255)),
    # the series runs for one lane: base^2 without a table (nb0 0, 1) and with one
    "nb0_0_one_lane_series": (lambda i: (_b(i), 0), (_b(99), 256 * N)),
    "nb0_1_one_lane_series": (lambda i: (_b(i), i & 1), (_b(99), 256 * (N + 1) + 1)),
    "nb0_2_one_lane_series": (lambda i: (_b(i), 2 + (i & 1)), (_b(99), (1 << 254) - 256)),
    # the series runs for all lanes but one: an even base, n = 0, and a lane that raises nb0
    "series_nb0_0_one_lane_even": (lambda i: (_b(i), 256 * (i + 1)), (_b(99, False), 256 * N)),
    "series_nb0_0_one_lane_n0": (lambda i: (_b(i), 256 * (i + 1)), (_b(99), 0)),
    "series_nb0_0_one_lane_1": (lambda i: (_b(i), 256 * (i + 1)), (_b(99), 256 * N + 1)),
    "series_nb0_1_one_lane_2": (lambda i: (_b(i), 256 * (i + 1) + (i & 1)), (_b(99), 3)),
    "series_nb0_8_one_lane_0": (lambda i: (_b(i), M256 - i), (_b(99), 1 << 84)),
}
POSITIONS = (0, 31, 32, 63)


def wave(name, pos):
    """64 (b, e) pairs; asserts that the odd lane's class differs from the others'."""
    rest, odd = WAVES[name]
    lanes = [rest(i) for i in range(64)]
    classes = {exp_class(*p) for i, p in enumerate(lanes) if i != pos}
    lanes[pos] = odd
    assert exp_class(*odd) not in classes, (name, exp_class(*odd), classes)
    return lanes
