"""GPU parity of the divider's wave-uniform tests and saturating digit conversion
(pf::udivrem256, csrc/u256.h: lane masks combined in scalar code, one v_cvt_u32_f64 per digit)
against oracle/pyoracle.py, bit-exact.

* Rows through the kernels a search runs, by the candidate-0 protocol of op_programs.py: UDIV,
  UREM, SDIV, SREM and SMOD at widths 256 and 200, both register files, the full sweep and the
  early-exit kernels.  The operands are uniform over the wave, so each row takes the fast path
  it qualifies for: zero, short (with and without saturating digits), one-digit (with and
  without the add-back), general (divisor lengths, digits 0xFFFFFFFF under an estimate of 2^32
  and digits 0 under an estimate of 1, at the highest and lowest executed digit).
* Mixed waves of 64 lanes through ``eval_assignments`` (the SoA kernel), where the scalar mask
  combinations can go wrong: one lane differs from the other 63 in the one condition a test is
  about, and sits at lane 0, 31, 32 or 63 — both halves of the 64-bit mask.  The same waves
  reach the search, stream, census and climb kernels, under all five ops, in
  tests/test_gpu_mixed_waves.py (the lane-table protocol of lane_table_cases.py).

div_trim_cases.py builds the operands and asserts, with a model of the divider in Python
integers, that each reaches its path and digits; tests/test_div_trim_cases.py runs the same
assertions without a GPU."""

import functools

import div_trim_cases as C
import numpy as np
import op_programs as P
import pyoracle as O
import pytest
from test_gpu_narrow_ops import _row, _run, kernels
from test_gpu_parity import _op_program

from mythril_amd import ir

pytestmark = pytest.mark.gpu

_UNSIGNED = ((ir.W_UDIV, O.bvudiv), (ir.W_UREM, O.bvurem))
_SIGNED = ((ir.W_SDIV, O.bvsdiv), (ir.W_SREM, O.bvsrem), (ir.W_SMOD, O.bvsmod))


@functools.lru_cache(maxsize=None)
def _rows(w):
    """Width 256: the 8-limb cases for the unsigned ops; the cases below 2^192 for all five
    (non-negative at both widths, so SDIV / SREM / SMOD hand the divider |a| and |b| as built,
    under every combination of signs).  Width 200: the cases below 2^192."""
    rows = []

    def add(op, fn, a, b):
        a, b = a & ir.mask(w), b & ir.mask(w)
        rows.append(_row(P.binop_set, (op, w, a, b), fn(a, b, w), w, bit=len(rows) * 11))

    if w == 256:
        for _, a, b in C.all_rows(8):
            for op, fn in _UNSIGNED:
                add(op, fn, a, b)
    for k, (_, a, b) in enumerate(C.all_rows(6)):
        assert a < 1 << 192 and b < 1 << 192
        for op, fn in _UNSIGNED:
            add(op, fn, a, b)
        for n, (op, fn) in enumerate(_SIGNED):
            s = (k + n) % 4                       # signs of (a, b): the divider sees (a, b)
            add(op, fn, -a if s & 1 else a, -b if s & 2 else b)
    return rows


@kernels
@pytest.mark.parametrize("w", [256, 200])
def test_div_trim_rows_through_search(engine, w, base, flags):
    rows = _rows(w)
    assert len(rows) == (2 * 83 if w == 256 else 0) + 5 * 83
    _run(engine, rows, base, flags)


@functools.lru_cache(maxsize=None)
def _programs():
    return {name: _op_program(name, 256) for name in ("udiv", "urem")}


@pytest.mark.parametrize("pos", C.POSITIONS)
@pytest.mark.parametrize("name", C.WAVES)
def test_div_trim_mixed_wave(engine, name, pos):
    lanes = C.wave(name, pos)                     # asserts the wave's path and its special lane
    for op, fn in (("udiv", O.bvudiv), ("urem", O.bvurem)):
        prog = _programs()[op]
        db = engine.upload([prog])
        good = [[a, b, fn(a, b, 256)] for a, b in lanes]
        for a, b, r in good:
            assert r == ((a // b if op == "udiv" else a % b) if b else (ir.mask(256) if op == "udiv" else a))
        wrong = [[a, b, P.corrupt(r, 256, 5 * i + 1)] for i, (a, b, r) in enumerate(good)]
        got = engine.eval_assignments(db, 0, ir.pack_assignments(prog, good))
        assert got.all(), (name, pos, op, [(i, [hex(v) for v in good[i]]) for i in np.nonzero(~got)[0][:3]])
        got = engine.eval_assignments(db, 0, ir.pack_assignments(prog, wrong))
        assert not got.any(), (name, pos, op, [(i, [hex(v) for v in wrong[i]]) for i in np.nonzero(got)[0][:3]])
