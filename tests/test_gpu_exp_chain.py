"""GPU parity of EXP's fused powering chain (pf::exp256_split, csrc/u256.h: where the series runs,
b^e0 is the product of the squarings that climb to the series' step) through the kernels a
search runs, against oracle/pyoracle.py, bit-exact.

About a hundred of the rows of tests/test_exp_chain_host.py at the configured split (the
single-bit and alternating patterns of e0 under n in {0, 1, 2^246 - 1}, bases 0, 1, 2, 2^32 and
2^w - 1, the even bases' edges, a walk over every e0) reach the search kernels by the candidate-0
protocol of op_programs.py: both register files, the full sweep and the early-exit kernels,
widths 256 and 200, every row as a set that holds and as one whose expectation is wrong in one
bit.  A candidate-0 wave is uniform, so the waves in which lanes differ go through
``eval_assignments`` (the SoA kernel), 64 lanes each:
 (a) odd and even bases alternate, e0 walks the patterns, n = 0 in a third of the odd lanes —
     the series runs for the wave while those lanes need (1 + X)^0 = 1;
 (b) bits 3 and 6 of e0 clear in every lane — the products of those steps are skipped;
 (c) every e0 < 8 with n != 0 — the wave's longest e0 has three bits;
 (d) no lane runs the series (all bases even; all n = 0) — the kept windowed path.
Each wave is checked to have the property it is named for."""

import functools

import exp_chain_cases as C
import numpy as np
import op_programs as P
import pyoracle as O
import pytest
from test_gpu_narrow_ops import _row, _run, kernels
from test_gpu_parity import _op_program

from mythril_amd import ir

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _rows(w):
    rows = []
    for b, e in C.gpu_pairs(w):
        r = O.bvexp(b, e, w)
        assert r == pow(b, e, 1 << w)
        rows.append(_row(P.binop_set, (ir.W_EXP, w, b, e), r, w, bit=len(rows) * 5))
    return rows


@kernels
@pytest.mark.parametrize("w", [256, 200])
def test_exp_chain_rows_through_search(engine, w, base, flags):
    rows = _rows(w)
    assert len(rows) == 100
    _run(engine, rows, base, flags)


def _e0s(lanes):
    return [C.split_e(e)[0] for _, e in lanes]


def _is_mixed(lanes):
    odd_n0 = [b & 1 and C.split_e(e)[1] == 0 for b, e in lanes]
    n_odd = sum(b & 1 for b, _ in lanes)
    return (C.runs_series(lanes) and n_odd == 32 and 3 * sum(odd_n0) >= n_odd
            and {e0 for (b, _), e0 in zip(lanes, _e0s(lanes)) if b & 1} >= set(C.PATTERNS))


def _has_bits_clear(lanes):
    e0s = _e0s(lanes)
    seen = 0
    for e0 in e0s:
        seen |= e0
    return C.runs_series(lanes) and seen == 0xFF & ~0x48 and all(C.split_e(e)[1] for _, e in lanes)


def _is_short(lanes):
    return (C.runs_series(lanes) and max(e0.bit_length() for e0 in _e0s(lanes)) == 3
            and set(_e0s(lanes)) == set(range(8)) and all(C.split_e(e)[1] for _, e in lanes))


def _all_even(lanes):
    return (not C.runs_series(lanes) and not any(b & 1 for b, _ in lanes)
            and {e >= 256 for _, e in lanes} == {False, True})


def _all_n0(lanes):
    return (not C.runs_series(lanes) and all(e < 256 for _, e in lanes)
            and {b & 1 for b, _ in lanes} == {0, 1}
            and {e.bit_length() for _, e in lanes} >= {0, 1, 8})


WAVES = {
    "mixed": (C.wave_mixed, _is_mixed),
    "bits_3_6_clear": (C.wave_bits_clear, _has_bits_clear),
    "short_e0": (C.wave_short_e0, _is_short),
    "no_series_even": (C.wave_all_even, _all_even),
    "no_series_n0": (C.wave_all_n0, _all_n0),
}


@pytest.mark.parametrize("w", [256, 200])
@pytest.mark.parametrize("name", sorted(WAVES))
def test_exp_chain_wave(engine, name, w):
    make, has_property = WAVES[name]
    lanes = make(w)
    assert len(lanes) == 64 and has_property(lanes), name
    prog = _op_program("exp", w)
    db = engine.upload([prog])
    cands, wrong = [], []
    for lane, (b, e) in enumerate(lanes):
        r = O.bvexp(b, e, w)
        assert r == pow(b, e, 1 << w)
        cands.append([b, e, r])
        wrong.append([b, e, P.corrupt(r, w, 3 * lane)])
    got = engine.eval_assignments(db, 0, ir.pack_assignments(prog, cands))
    assert got.all(), (name, w, [[hex(v) for v in cands[i]] for i in np.nonzero(~got)[0][:3]])
    got = engine.eval_assignments(db, 0, ir.pack_assignments(prog, wrong))
    assert not got.any(), (name, w, [[hex(v) for v in wrong[i]] for i in np.nonzero(got)[0][:3]])
