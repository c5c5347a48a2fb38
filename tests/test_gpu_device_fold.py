"""GPU: searches over folded device programs (mythril_amd/csrc/pf_fold.h) report what the
oracle finds in the programs as lowered — ``found`` and the counters of search_counters.py.

One batch of 48 sets at a budget of 4,096: config-3 ids 0..39 (the benchmark's programs, a
quarter of whose instructions the pass removes) and eight sets built around what the pass
leaves behind — a bare END, a constant-false B_CONST with its assert, a zero written as
W_XOR r, r that feeds a live division and a live EXP, and two rules at four widths.  The
kernel runs the folded programs; coracle evaluates the lowered ones."""

import functools

import numpy as np
import pytest
import search_counters as SC

from mythril_amd import ir, synth
from mythril_amd.lower import Dag, lower

pytestmark = pytest.mark.gpu

COUNT_OPS, SHORT, EARLY = ir.FLAG_COUNT_OPS, ir.FLAG_SHORTCIRCUIT, ir.FLAG_EARLY_EXIT
SEED, BUDGET, SHORT_BUDGET = 0xF01D_5EED, 4096, 128


def _b(dag, op, w, *args):
    return dag.add(op, w, args, 0, True)


def _special_sets():
    out = []
    dag = Dag()                                   # folds to a bare END: every candidate holds
    x = dag.var("x", 256)
    dag.assert_(_b(dag, ir.B_EQ, 256, dag.add(ir.W_XOR, 256, (x, x)), dag.const(0, 256)))
    out.append(lower(dag, seed=1))
    dag = Dag()                                   # constant false
    x = dag.var("x", 64)
    dag.assert_(_b(dag, ir.B_ULT, 64, x, x))
    out.append(lower(dag, seed=2))
    dag = Dag()                                   # a dropped assert, then B_CONST + ASSERT alone
    x, y = dag.var("x", 160), dag.var("y", 160)
    dag.assert_(_b(dag, ir.B_ULE, 160, x, x))
    dag.assert_(_b(dag, ir.B_XOR, 1, _b(dag, ir.B_SLT, 160, x, x), _b(dag, ir.B_ULT, 160, y, y)))
    out.append(lower(dag, seed=3))
    dag = Dag()                                   # 0 / y + 0 ** y == t, the 0 from x - x
    x, y, t = dag.var("x", 256), dag.var("y", 256), dag.var("t", 256)
    z = dag.add(ir.W_SUB, 256, (x, x))
    s = dag.add(ir.W_ADD, 256, (dag.add(ir.W_UDIV, 256, (z, y)), dag.add(ir.W_EXP, 256, (z, y))))
    dag.assert_(_b(dag, ir.B_EQ, 256, s, t))
    out.append(lower(dag, seed=4))
    for w in (8, 64, 160, 256):                   # (x smod x) + y * 1 <u 2^(w-2), and x | M(w) == ~0
        dag = Dag()
        x, y = dag.var("x", w), dag.var("y", w)
        r = dag.add(ir.W_ADD, w, (dag.add(ir.W_SMOD, w, (x, x)), dag.add(ir.W_MUL, w, (y, dag.const(1, w)))))
        dag.assert_(_b(dag, ir.B_ULT, w, r, dag.const(1 << (w - 2), w)))
        ones = dag.const((1 << w) - 1, w)
        dag.assert_(_b(dag, ir.B_EQ, w, dag.add(ir.W_OR, w, (x, ones)), dag.add(ir.W_NOT, w, (dag.const(0, w),))))
        out.append(lower(dag, seed=10 + w))
    return out


@functools.lru_cache(maxsize=None)
def sets():
    progs = [synth.random_dag_set(i, plant=False)[0] for i in range(40)] + _special_sets()
    assert len(progs) == 48
    batch = ir.Batch(progs)
    return progs, batch, SC.sat_masks(batch, SEED, BUDGET), SC.aux1_totals(batch)


@pytest.fixture(scope="module")
def db(engine):
    d = engine.upload(sets()[0])
    yield d
    d.free()


def test_the_batch_is_what_it_says():
    """The device forms the cases rest on (host only), and witnesses of every kind."""
    _, batch, masks, aux1 = sets()
    rows = SC.device_rows(batch)
    ops = [[r[0] & 0xFF for r in rs] for rs in rows]
    assert ops[40] == [ir.END] and rows[40][0][3] == aux1[40]
    assert ops[41] == [ir.B_CONST, ir.END] and ops[42] == [ir.B_CONST, ir.END]
    assert ir.W_SUB not in ops[43] and ir.W_UDIV in ops[43] and ir.W_EXP in ops[43]
    zero = [r for r in rows[43] if r[0] & 0xFF == ir.W_XOR]
    assert len(zero) == 1 and (zero[0][1] >> 8) & 0xFF == (zero[0][1] >> 16) & 0xFF
    for s in range(44, 48):
        assert not {ir.W_SMOD, ir.W_MUL, ir.W_OR, ir.W_NOT} & set(ops[s]), s
    assert [sum(r[3] for r in rs) for rs in rows] == aux1
    assert sum(len(rs) for rs in rows) < 0.85 * len(batch.code)
    fs = [SC.first_witness(m, BUDGET) for m in masks]
    assert fs[40] == 0 and fs[41] is None and fs[42] is None and fs[43] is not None
    assert sum(f is None for f in fs[:40]) >= 3 and sum(f is not None and f >= 64 for f in fs) >= 3


def test_full_sweep_counts_every_candidate_and_the_lowered_ops(engine, db):
    _, _, masks, aux1 = sets()
    res = engine.check(db, budget=BUDGET, seed=SEED, flags=COUNT_OPS)
    assert np.array_equal(res.found, SC.found(masks, BUDGET))
    assert not res.timed_out
    assert (res.cands_decided, res.evals_full, res.ops) == SC.full_sweep(masks, BUDGET, aux1)
    assert res.evals_full == 48 * 4096


def test_shortcircuit_sweep_leaves_where_the_device_program_says(engine, db):
    """SHORTCIRCUIT | COUNT_OPS: a wave leaves at the assert where its last lane falls, and
    has counted the aux1 of the device instructions up to it — the dropped ones' included."""
    _, batch, masks, _ = sets()
    res = engine.check(db, budget=SHORT_BUDGET, seed=SEED, flags=SHORT | COUNT_OPS)
    assert np.array_equal(res.found, SC.found(masks, SHORT_BUDGET))
    assert res.cands_decided == 48 * SHORT_BUDGET
    assert res.evals_full == SC.shortcircuit_evals_full(masks, SHORT_BUDGET)
    assert res.ops == SC.shortcircuit_ops(batch, SEED, SHORT_BUDGET)


@pytest.mark.parametrize("flags", [EARLY | COUNT_OPS, EARLY | SHORT | COUNT_OPS], ids=["early", "early_shortcircuit"])
def test_early_exit_search_finds_the_first_witness(engine, db, flags):
    _, _, masks, aux1 = sets()
    res = engine.check(db, budget=BUDGET, seed=SEED, flags=flags)
    assert np.array_equal(res.found, SC.found(masks, BUDGET))
    assert not res.timed_out
    floor, total = SC.early_exit_floor(masks, BUDGET), 48 * BUDGET
    assert floor <= res.cands_decided <= total
    if flags & SHORT:
        assert res.evals_full <= res.cands_decided
    else:
        # every decided candidate ran its program to END: per set between the floor and the budget
        assert res.evals_full == res.cands_decided
        lo = sum(a * SC.early_exit_floor(masks[s:s + 1], BUDGET) for s, a in enumerate(aux1))
        assert lo <= res.ops <= BUDGET * sum(aux1)
