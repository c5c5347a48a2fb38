"""GPU parity of EXP's scaled Horner chain (pf::exp256_split, csrc/u256.h: the factor shifted
once, the values kept scaled, shifts only at the un-scaling levels) through the kernels a search
runs, against oracle/pyoracle.py, bit-exact: about a hundred of the rows of
tests/test_exp_scale_host.py at the configured split.

n = (e >> 8) sits at and around every un-scaling level (the binomials vanish above level n, so
that level is the last that matters) and at 2^246 - 1, under bases whose t is all ones, 1 and
random, e0 in {0, 255}; a few random pairs follow.  Rows reach the search kernels by the
candidate-0 protocol of op_programs.py: both register files, the full sweep and the early-exit
kernels, widths 256 and 200, every row as a set that holds and as one whose expectation is wrong
in one bit.  One mixed wave (exp_scale_cases.mixed_wave) goes through ``eval_assignments`` (the
SoA kernel): odd and even bases side by side, n at and around the un-scaling levels; the other
kernels get it in tests/test_gpu_mixed_waves.py."""

import functools

import exp_scale_cases as S
import numpy as np
import op_programs as P
import pyoracle as O
import pytest
from test_gpu_narrow_ops import _row, _run, kernels
from test_gpu_parity import _op_program

from mythril_amd import ir

pytestmark = pytest.mark.gpu

SPLIT = 8


@functools.lru_cache(maxsize=None)
def _pairs():
    rng = np.random.default_rng(0x5CA1E)
    pairs = S.pairs(SPLIT, nrandom_bases=1)
    pairs += [(int.from_bytes(rng.bytes(32), "little") | 1, int.from_bytes(rng.bytes(32), "little"))
              for _ in range(100 - len(pairs))]
    return pairs


@functools.lru_cache(maxsize=None)
def _rows(w):
    rows = []
    for b, e in _pairs():
        b_, e_ = b & ir.mask(w), e & ir.mask(w)
        r = O.bvexp(b_, e_, w)
        assert r == pow(b_, e_, 1 << w)
        rows.append(_row(P.binop_set, (ir.W_EXP, w, b_, e_), r, w, bit=len(rows) * 5))
    return rows


@kernels
@pytest.mark.parametrize("w", [256, 200])
def test_exp_scale_rows_through_search(engine, w, base, flags):
    rows = _rows(w)
    assert len(rows) == 100
    _run(engine, rows, base, flags)


@pytest.mark.parametrize("w", [256, 200])
def test_exp_scale_mixed_wave(engine, w):
    """One wave of 64 lanes: odd and even bases alternate, n walks over the un-scaling levels
    and their neighbours (and 0 and 2^246 - 1), t all ones / 1 / random rotate."""
    prog = _op_program("exp", w)
    db = engine.upload([prog])
    cands, wrong = [], []
    for lane, (b, e) in enumerate(S.mixed_wave(w, SPLIT)):
        r = O.bvexp(b, e, w)
        assert r == pow(b, e, 1 << w)
        cands.append([b, e, r])
        wrong.append([b, e, P.corrupt(r, w, 3 * lane)])
    assert {(c[0] & 1, c[1] >= 256) for c in cands} == {(0, False), (0, True), (1, False), (1, True)}
    got = engine.eval_assignments(db, 0, ir.pack_assignments(prog, cands))
    assert got.all(), (w, [[hex(v) for v in cands[i]] for i in np.nonzero(~got)[0][:3]])
    got = engine.eval_assignments(db, 0, ir.pack_assignments(prog, wrong))
    assert not got.any(), (w, [[hex(v) for v in wrong[i]] for i in np.nonzero(got)[0][:3]])
