"""GPU parity of EXP's division-free series (pf::exp256_split, csrc/u256.h) through the kernels a
search runs, against oracle/pyoracle.py, bit-exact: the base x exponent grid of
tests/test_exp_series_host.py reduced to a few hundred rows.

* e = e0 + 256 n for n = 0..30 (the binomials vanish above level n, so every level's constant is
  the last that matters once), n a single bit, n all ones, and exponent bits 254 / 255;
* odd bases 1, 3, 5, 7, 2^k +- 1, 2^256 - 1 and random ones; even bases below and above e = 256.

Rows reach the search kernels by the candidate-0 protocol of op_programs.py, as the EXP grid of
test_gpu_narrow_ops.py does: both register files, the full sweep and the early-exit kernels,
widths 256 and 200, every row as a set that holds and as one whose expectation is wrong in one
bit.  One mixed wave (exp_series_cases.mixed_wave) goes through ``eval_assignments`` (the SoA
kernel): 64 lanes with odd and even bases and n = 0 and n != 0 side by side, so the series runs
under a wave-uniform branch that only some lanes need; the other kernels get it in
tests/test_gpu_mixed_waves.py."""

import functools

import exp_series_cases as X
import numpy as np
import op_programs as P
import pyoracle as O
import pytest
from test_gpu_narrow_ops import _row, _run, kernels
from test_gpu_parity import _op_program

from mythril_amd import ir

pytestmark = pytest.mark.gpu

_M = ir.mask(256)


def _pairs():
    rng = np.random.default_rng(0x5E71E5)

    def rnd():
        return int.from_bytes(rng.bytes(32), "little")

    odd = [1, 3, 5, 7, _M, (1 << 3) - 1, (1 << 3) + 1, (1 << 32) - 1, (1 << 32) + 1, (1 << 33) + 1,
           (1 << 128) - 1, (1 << 255) - 1, (1 << 255) + 1] + [rnd() | 1 for _ in range(5)]
    pairs = []
    # every level alone: n = 0..30, the base and the low part rotating
    for n in range(31):
        for k in range(4):
            pairs.append((odd[(4 * n + k) % len(odd)], (0, 1, 255)[(n + k) % 3] + 256 * n))
    # n a single bit, all ones, and the bits that do not matter
    for k in (0, 1, 2, 7, 8, 23, 24, 31, 32, 63, 64, 127, 128, 200, 244, 245):
        for b in (3, odd[13 + k % 5], (1 << 32) + 1):
            pairs.append((b, (255 if k & 1 else 0) + 256 * (1 << k)))
    for b in (3, 7, _M, odd[14], odd[15]):
        pairs.append((b, 256 * ((1 << 246) - 1) + 255))
        pairs.append((b, (1 << 254) + 256 * 5 + 1))
        pairs.append((b, (1 << 255) + 256 * 28))
        pairs.append((b, _M))
    # every odd base shape under exponents that run the whole chain
    for b in odd:
        pairs.append((b, 256 * 28 + 255))
        pairs.append((b, rnd()))
    # even bases: e < 256 and e >= 256
    for b in (0, 2, 6, 1 << 31, 1 << 255, _M - 1, rnd() & ~1, rnd() & ~1):
        for e in (0, 1, 7, 85, 255, 256, 257, 256 * 3, (1 << 254) + 1, _M):
            pairs.append((b, e))
    return pairs


@functools.lru_cache(maxsize=None)
def _rows(w):
    rows = []
    for b, e in _pairs():
        b_, e_ = b & ir.mask(w), e & ir.mask(w)
        r = O.bvexp(b_, e_, w)
        assert r == pow(b_, e_, 1 << w)
        rows.append(_row(P.binop_set, (ir.W_EXP, w, b_, e_), r, w, bit=len(rows) * 7))
    return rows


@kernels
@pytest.mark.parametrize("w", [256, 200])
def test_exp_series_grid_through_search(engine, w, base, flags):
    rows = _rows(w)
    assert 300 <= len(rows) <= 400
    _run(engine, rows, base, flags)


@pytest.mark.parametrize("w", [256, 200])
def test_exp_series_mixed_wave(engine, w):
    """One wave of 64 lanes: odd / even bases alternate, and so do n = 0 and n != 0, so every
    combination sits next to the others while the series runs for the lanes that need it."""
    prog = _op_program("exp", w)
    db = engine.upload([prog])
    cands, wrong = [], []
    for lane, (b, e) in enumerate(X.mixed_wave(w)):
        r = O.bvexp(b, e, w)
        assert r == pow(b, e, 1 << w)
        cands.append([b, e, r])
        wrong.append([b, e, P.corrupt(r, w, 3 * lane)])
    assert {(c[0] & 1, c[1] >= 256) for c in cands} == {(0, False), (0, True), (1, False), (1, True)}
    got = engine.eval_assignments(db, 0, ir.pack_assignments(prog, cands))
    assert got.all(), (w, [[hex(v) for v in cands[i]] for i in np.nonzero(~got)[0][:3]])
    got = engine.eval_assignments(db, 0, ir.pack_assignments(prog, wrong))
    assert not got.any(), (w, [[hex(v) for v in wrong[i]] for i in np.nonzero(got)[0][:3]])
