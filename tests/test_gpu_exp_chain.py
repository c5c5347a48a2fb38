"""GPU parity of EXP's fused powering chain (pf::exp256_split, csrc/u256.h: where the series runs,
b^e0 is the product of the squarings that climb to the series' step) through the kernels a
search runs, against oracle/pyoracle.py, bit-exact.

About a hundred of the rows of tests/test_exp_chain_host.py at the configured split (the
single-bit and alternating patterns of e0 under n in {0, 1, 2^246 - 1}, bases 0, 1, 2, 2^32 and
2^w - 1, the even bases' edges, a walk over every e0) reach the search kernels by the candidate-0
protocol of op_programs.py: both register files, the full sweep and the early-exit kernels,
widths 256 and 200, every row as a set that holds and as one whose expectation is wrong in one
bit.  A candidate-0 wave is uniform, so the waves in which lanes differ go through
``eval_assignments`` (the SoA kernel) here, 64 lanes each, and through the search, stream, census
and climb kernels in tests/test_gpu_mixed_waves.py (the lane-table protocol of
lane_table_cases.py):
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


WAVES = C.WAVES      # the waves and the predicates that say what each is there for


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
