"""GPU parity of the product routines (csrc/u256_cols.h: the generated inline-asm columns, whose
carry word is created by each column's first carry add; the series' multiply-adds with the addend's
limbs as literals; csrc/u256.h: exp256_w32 building only the table entries it reads) against
Python integers and oracle/pyoracle.py, bit-exact.

* Rows through the kernels a search runs, by the candidate-0 protocol of op_programs.py: MUL and
  EXP at widths 256 and 200, both register files, the full sweep and the early-exit kernels.
  MUL: every limb 0xFFFFFFFF on both sides (every carry add of every column fires), a carry in
  exactly one of the columns 1..5, one-limb operands, 2^k at and around limb boundaries.  EXP:
  odd and even bases under exponents 0, 1, 2, 3, 255, 256, 256 n (+ 1, 2, 3), 2^84, 2^254,
  2^256 - 1: the series with nb0 = 0, 1, >= 2 and no series with nb0 = 0, 1, 2, 8.
* Mixed waves of 64 lanes through ``eval_assignments`` (the SoA kernel): 63 lanes of one of
  those classes and one lane of another, at lane 0, 31, 32 or 63.  The same waves, and a MUL wave
  of carrying and non-carrying columns, reach the search, stream, census and climb kernels in
  tests/test_gpu_mixed_waves.py (the lane-table protocol of lane_table_cases.py).

products_cases.py builds the operands and asserts what they are for; tests/test_products_host.py
runs the same rows through the host mirrors."""

import functools

import numpy as np
import op_programs as P
import products_cases as C
import pyoracle as O
import pytest
from test_gpu_narrow_ops import _row, _run, kernels
from test_gpu_parity import _op_program

from mythril_amd import ir

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _rows(op, w):
    fn, pairs = ((O.bvmul, C.mul_rows()) if op == ir.W_MUL else (O.bvexp, C.exp_rows()))
    rows = []
    for a, b in pairs:
        a, b = a & ir.mask(w), b & ir.mask(w)
        r = fn(a, b, w)
        assert r == (a * b if op == ir.W_MUL else pow(a, b, 1 << w)) & ir.mask(w)
        rows.append(_row(P.binop_set, (op, w, a, b), r, w, bit=len(rows) * 11))
    return rows


@kernels
@pytest.mark.parametrize("w", [256, 200])
@pytest.mark.parametrize("op", [ir.W_MUL, ir.W_EXP], ids=["mul", "exp"])
def test_products_rows_through_search(engine, op, w, base, flags):
    rows = _rows(op, w)
    assert len(rows) == (6 + 64 + 25 * 4 * 3 if op == ir.W_MUL else 13 * 13)
    _run(engine, rows, base, flags)


@functools.lru_cache(maxsize=None)
def _program():
    return _op_program("exp", 256)


@pytest.mark.parametrize("pos", C.POSITIONS)
@pytest.mark.parametrize("name", sorted(C.WAVES))
def test_exp_mixed_wave(engine, name, pos):
    lanes = C.wave(name, pos)                     # asserts the odd lane's class
    prog = _program()
    db = engine.upload([prog])
    good = [[b, e, O.bvexp(b, e, 256)] for b, e in lanes]
    for b, e, r in good:
        assert r == pow(b, e, 1 << 256)
    wrong = [[b, e, P.corrupt(r, 256, 5 * i + 1)] for i, (b, e, r) in enumerate(good)]
    got = engine.eval_assignments(db, 0, ir.pack_assignments(prog, good))
    assert got.all(), (name, pos, [(i, [hex(v) for v in good[i]]) for i in np.nonzero(~got)[0][:3]])
    got = engine.eval_assignments(db, 0, ir.pack_assignments(prog, wrong))
    assert not got.any(), (name, pos, [(i, [hex(v) for v in wrong[i]]) for i in np.nonzero(got)[0][:3]])
