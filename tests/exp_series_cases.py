"""The mixed wave of EXP's division-free series (pf::exp256_split, csrc/u256.h), shared by
tests/test_gpu_exp_series.py and tests/lane_table_cases.py (no GPU needed to import)."""

import numpy as np


def mixed_wave(w):
    """One wave of 64 (base, exponent) lanes at width w: odd / even bases alternate, and so do
    n = 0 and n != 0, so every combination sits next to the others while the series runs for the
    lanes that need it."""
    rng = np.random.default_rng(0x3A7E + w)
    Mw = (1 << w) - 1
    lanes = []
    for lane in range(64):
        b = int.from_bytes(rng.bytes(32), "little")
        b = (b | 1) if lane & 1 else (b & ~1)
        if lane % 8 == 7:
            b = ((1 << (8 + lane)) + 1) & Mw           # t tiny
        e0 = int(rng.integers(0, 256))
        n = 0 if lane & 2 else [1, 2, lane, 1 << lane, int.from_bytes(rng.bytes(31), "little")][lane % 5]
        lanes.append((b & Mw, (e0 + 256 * n) & Mw))
    return lanes
