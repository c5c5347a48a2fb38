"""CPU: the fold pass of the device program (mythril_amd/csrc/pf_fold.h, the first rewrite of
pf_batch_create, exported host-only through pf_device_program).

The pass replaces results that are the same for every candidate — constant operands, x-op-x
identities, absorbing and neutral constants — and drops what only they needed.  The oracle
evaluates the program as lowered (SetView.evaluate); ``eval_device`` of test_device_program is
the kernel's reading of the rewritten one.  Every rule is run at widths 1, 8, 32, 64, 160 and
256 with the boundary values of each width, the near misses must keep their instruction, and
config 3 (the benchmark's programs) must lose at least a fifth of its weighted cost.

``PF_DEVICE_FOLD`` is read by pf_device_program on every call: 0 switches the pass off, 2 runs
the pass alone (no peephole after it), whose output is still a lowered program and can be fed
back in — the fixed-point check below."""

import random
import types

import numpy as np
import pytest

import pyoracle as O
from mythril_amd import ir, synth
from mythril_amd.lower import K_CONST, Dag, lower
from op_programs import Asm
from test_device_program import _programs, device_program, eval_device

WIDTHS = (1, 8, 32, 64, 160, 256)
DIV_OPS = (ir.W_UDIV, ir.W_UREM, ir.W_SDIV, ir.W_SREM, ir.W_SMOD)
HEAVY = DIV_OPS + (ir.W_EXP, ir.W_MUL, ir.B_UMUL_NOOVF)


def M(w):
    return (1 << w) - 1


def boundary_values(w, rng):
    vals = [0, 1, 2, M(w), 1 << (w - 1), (1 << (w - 1)) - 1] + [rng.getrandbits(w) for _ in range(3)]
    return sorted({v & M(w) for v in vals})


def rows_of(code, descs, s=0):
    d = descs[s]
    return [tuple(int(x) for x in r) for r in code[int(d[0]):int(d[0]) + int(d[1])]]


def opcodes(rows):
    return [r[0] & 0xFF for r in rows]


def is_zero_idiom(row):
    """W_XOR d, r, r: how the pass writes a constant 0 that is not in the set's pool."""
    w0, w1 = row[0], row[1]
    return w0 & 0xFF == ir.W_XOR and (w1 >> 8) & 0xFF == (w1 >> 16) & 0xFF


def has_op(rows, op):
    return any(r[0] & 0xFF == op and not is_zero_idiom(r) for r in rows)


def assert_same_verdicts(prog, w, seed=1):
    """The device program against the lowered one over the boundary values of every variable;
    returns the device rows."""
    batch = ir.Batch([prog])
    code, descs = device_program(batch)
    rows = rows_of(code, descs)
    assert rows[-1][0] & 0xFF == ir.END and len(rows) <= len(batch.code)
    sv = O.SetView.from_batch(batch, 0)
    vals = boundary_values(w, random.Random(seed))
    n = len(sv.schema)
    assert 1 <= n <= 2
    for x in vals:
        for y in (vals if n == 2 else [0]):
            v = [x, y][:n]
            assert eval_device(sv, rows, v) == sv.evaluate(v), (prog.name, w, v)
    return rows


# ---- one program per rule ------------------------------------------------------------------
# A rule is (name, folded opcode, build): build(dag, w, x) -> the node the rule folds; x is a
# width-w variable.  Nodes go in through Dag.add, which hash-conses but does not simplify.

def W(op):
    return lambda dag, w, *args: dag.add(op, w, args)


def Bc(op):
    return lambda dag, w, *args: dag.add(op, w, args, 0, True)


def same(op, boolean=False):
    mk = Bc(op) if boolean else W(op)
    return lambda dag, w, x: mk(dag, w, x, x)


def k_right(op, value):
    return lambda dag, w, x: W(op)(dag, w, x, dag.const(value(w), w))


def k_left(op, value):
    return lambda dag, w, x: W(op)(dag, w, dag.const(value(w), w), x)


ZERO, ONE, ONES, WIDTH = (lambda w: 0), (lambda w: 1), M, (lambda w: w)

W_RULES = (
    [(f"same:{ir.OPNAMES[op]}", op, same(op)) for op in
     (ir.W_SUB, ir.W_XOR, ir.W_UREM, ir.W_SREM, ir.W_SMOD, ir.W_AND, ir.W_OR)] +
    [(f"{ir.OPNAMES[op]}(x,{tag})", op, k_right(op, val)) for op, tag, val in (
        (ir.W_MUL, "0", ZERO), (ir.W_MUL, "1", ONE), (ir.W_AND, "0", ZERO), (ir.W_AND, "M", ONES),
        (ir.W_OR, "M", ONES), (ir.W_OR, "0", ZERO), (ir.W_XOR, "0", ZERO), (ir.W_ADD, "0", ZERO),
        (ir.W_SUB, "0", ZERO), (ir.W_SHL, "w", WIDTH), (ir.W_LSHR, "w", WIDTH), (ir.W_SHL, "M", ONES),
        (ir.W_LSHR, "M", ONES), (ir.W_SHL, "0", ZERO), (ir.W_LSHR, "0", ZERO), (ir.W_ASHR, "0", ZERO),
        (ir.W_UREM, "1", ONE), (ir.W_SREM, "1", ONE), (ir.W_SMOD, "1", ONE),
        (ir.W_UREM, "0", ZERO), (ir.W_SREM, "0", ZERO), (ir.W_SMOD, "0", ZERO),
        (ir.W_UDIV, "0", ZERO), (ir.W_UDIV, "1", ONE), (ir.W_SDIV, "1", ONE),
        (ir.W_EXP, "0", ZERO), (ir.W_EXP, "1", ONE))] +
    [(f"{ir.OPNAMES[op]}({tag},x)", op, k_left(op, val)) for op, tag, val in (
        (ir.W_MUL, "0", ZERO), (ir.W_MUL, "1", ONE), (ir.W_AND, "0", ZERO), (ir.W_AND, "M", ONES),
        (ir.W_OR, "M", ONES), (ir.W_OR, "0", ZERO), (ir.W_XOR, "0", ZERO), (ir.W_ADD, "0", ZERO),
        (ir.W_SHL, "0", ZERO), (ir.W_LSHR, "0", ZERO), (ir.W_ASHR, "0", ZERO),
        (ir.W_UREM, "0", ZERO), (ir.W_SREM, "0", ZERO), (ir.W_SMOD, "0", ZERO), (ir.W_EXP, "1", ONE))]
)
B_RULES = [(f"same:{ir.OPNAMES[op]}", op, same(op, True)) for op in
           (ir.B_EQ, ir.B_ULE, ir.B_SLE, ir.B_ULT, ir.B_SLT)]


def rule_program(build, w, boolean, pooled_zero):
    dag = Dag()
    # a constant result can only be named through the pool: x / 0 = M(w) and x ** 0 = 1 need
    # theirs there; a 0 outside the pool is written W_XOR d, r, r
    dag.force_consts([M(w), 1] + ([0] if pooled_zero else []))
    x, y = dag.var("x", w), dag.var("y", w)
    r = build(dag, w, x)
    if boolean:   # the root needs the folded bool and the second variable
        dag.assert_(dag.add(ir.B_XOR, 1, (r, dag.add(ir.B_UADD_NOOVF, w, (y, x), 0, True)), 0, True))
    else:
        dag.assert_(dag.add(ir.B_EQ, w, (r, y), 0, True))
    return lower(dag)


@pytest.mark.parametrize("pooled_zero", (False, True), ids=("xor_zero", "pooled_zero"))
@pytest.mark.parametrize("w", WIDTHS)
def test_every_rule_folds_at_every_width(w, pooled_zero):
    for boolean, rules in ((False, W_RULES), (True, B_RULES)):
        for name, op, build in rules:
            prog = rule_program(build, w, boolean, pooled_zero)
            prog.name = name
            assert op in [i.op for i in prog.code], (name, w)       # the lowering kept it
            rows = assert_same_verdicts(prog, w)
            assert not has_op(rows, op), (name, w, rows)
            if pooled_zero:
                assert not any(is_zero_idiom(r) for r in rows), (name, w)


CONST_PAIRS = ((0xA5A5_5A5A_DEAD_BEEF_0123_4567_89AB_CDEF_F00D, 3), (5, 0), (0, 7), (M(256), M(256) - 1),
               (1 << 255 | 12345, 1 << 200 | 77))


@pytest.mark.parametrize("w", WIDTHS)
def test_constant_operands_are_evaluated_on_the_host(w):
    """op(c1, c2) and NOT / NEG of a constant, with the result in the pool (a result outside
    it leaves the instruction in place: the device program has no immediates)."""
    for op in sorted(ir.W_BINARY):
        for c1, c2 in CONST_PAIRS:
            c1, c2 = c1 & M(w), c2 & M(w)
            want = O._WBIN[op](c1, c2, w) & M(w)
            dag = Dag()
            dag.force_consts([want])
            y = dag.var("y", w)
            r = dag.add(op, w, (dag.const(c1, w), dag.const(c2, w)))
            dag.assert_(dag.add(ir.B_EQ, w, (r, y), 0, True))
            prog = lower(dag)
            prog.name = f"{ir.OPNAMES[op]}({c1:#x},{c2:#x})"
            assert op in [i.op for i in prog.code]
            rows = assert_same_verdicts(prog, w)
            assert not has_op(rows, op), (prog.name, w)
            sv = O.SetView.from_batch(ir.Batch([prog]), 0)
            assert eval_device(sv, rows, [want]) and not eval_device(sv, rows, [want ^ 1])
    for op, fn in ((ir.W_NOT, O.bvnot), (ir.W_NEG, O.bvneg)):
        for c1, _ in CONST_PAIRS:
            c1 &= M(w)
            dag = Dag()
            dag.force_consts([fn(c1, w)])
            y = dag.var("y", w)
            dag.assert_(dag.add(ir.B_EQ, w, (dag.add(op, w, (dag.const(c1, w),)), y), 0, True))
            prog = lower(dag)
            assert op in [i.op for i in prog.code]
            assert not has_op(assert_same_verdicts(prog, w), op), (ir.OPNAMES[op], w, c1)


@pytest.mark.parametrize("w", WIDTHS)
def test_constant_compares_ite_and_bool_logic(w):
    """Compares of constants, W_ITE / B_ITE on a constant condition or with identical arms, and
    B_AND / B_OR / B_XOR / B_NOT with the constant operand that decides them."""
    def prog_of(make, op):
        dag = Dag()
        x, y = dag.var("x", w), dag.var("y", w)
        # a bool that depends on both variables (not through the opcode under test)
        p = dag.add(ir.B_SLT if op == ir.B_ULT else ir.B_ULT, w, (x, y), 0, True)
        dag.assert_(make(dag, x, y, p))
        return lower(dag)

    def b(op, *args):
        return lambda dag: dag.add(op, 1, args, 0, True)

    c5, c9 = 5 & M(w), 9 & M(w)
    cases = []
    for op in (ir.B_EQ, ir.B_ULT, ir.B_ULE, ir.B_SLT, ir.B_SLE, ir.B_UADD_NOOVF):
        for p, q in ((c5, c9), (c9, c5), (M(w), 1), (c5, c5)):
            cases.append((op, lambda dag, x, y, p_, op=op, p=p, q=q: dag.add(
                ir.B_XOR, 1, (dag.add(op, w, (dag.const(p, w), dag.const(q, w)), 0, True), p_), 0, True)))
    for cond in (True, False):
        cases.append((ir.W_ITE, lambda dag, x, y, p_, cond=cond: dag.add(
            ir.B_EQ, w, (dag.add(ir.W_ITE, w, (dag.bconst(cond), x, dag.add(ir.W_NOT, w, (y,)))), y), 0, True)))
        # a constant condition picking a constant arm (an arm that is a register stays a
        # B_ITE: the device program has no bool move)
        cases.append((ir.B_ITE, lambda dag, x, y, p_, cond=cond: dag.add(ir.B_XOR, 1, (dag.add(
            ir.B_ITE, 1, (dag.bconst(cond), dag.bconst(cond), dag.add(ir.B_EQ, w, (x, y), 0, True))
            if cond else (dag.bconst(cond), dag.add(ir.B_EQ, w, (x, y), 0, True), dag.bconst(cond)), 0, True), p_),
            0, True)))
    cases.append((ir.W_ITE, lambda dag, x, y, p_: dag.add(
        ir.B_EQ, w, (dag.add(ir.W_ITE, w, (p_, x, x)), y), 0, True)))
    cases.append((ir.B_AND, lambda dag, x, y, p_: dag.add(
        ir.B_OR, 1, (dag.add(ir.B_AND, 1, (p_, dag.bconst(False)), 0, True), dag.add(ir.B_EQ, w, (x, y), 0, True)),
        0, True)))
    cases.append((ir.B_NOT, lambda dag, x, y, p_: dag.add(
        ir.B_XOR, 1, (dag.add(ir.B_NOT, 1, (dag.bconst(False),), 0, True), p_), 0, True)))
    cases.append((ir.B_OR, lambda dag, x, y, p_: dag.add(
        ir.B_XOR, 1, (dag.add(ir.B_OR, 1, (dag.bconst(True), p_), 0, True), dag.add(ir.B_EQ, w, (x, y), 0, True)),
        0, True)))
    for op, make in cases:
        prog = prog_of(make, op)
        prog.name = ir.OPNAMES[op]
        assert op in [i.op for i in prog.code], (ir.OPNAMES[op], w, prog.code)
        rows = assert_same_verdicts(prog, w)
        assert not has_op(rows, op), (ir.OPNAMES[op], w, rows)


def test_constant_asserts():
    """ASSERT of a constant true goes (x ^ x == 0 folds to a bare END, every candidate holds);
    a constant false stays (x < x: B_CONST 0 with the assert, no candidate holds)."""
    for w in WIDTHS:
        dag = Dag()
        x = dag.var("x", w)
        dag.assert_(dag.add(ir.B_EQ, w, (dag.add(ir.W_XOR, w, (x, x)), dag.const(0, w)), 0, True))
        batch = ir.Batch([lower(dag)])
        code, descs = device_program(batch)
        rows = rows_of(code, descs)
        assert opcodes(rows) == [ir.END]
        assert rows[0][3] == int(np.asarray(batch.code, dtype=np.uint64)[:, 3].sum())   # ops stay
        dag = Dag()
        x = dag.var("x", w)
        dag.assert_(dag.add(ir.B_ULT, w, (x, x), 0, True))
        batch = ir.Batch([lower(dag)])
        code, descs = device_program(batch)
        rows = rows_of(code, descs)
        assert opcodes(rows) == [ir.B_CONST, ir.END] and rows[0][2] == 0 and rows[0][0] & (1 << 24)
        sv = O.SetView.from_batch(batch, 0)
        for v in boundary_values(w, random.Random(2)):
            assert eval_device(sv, rows, [v]) is False and sv.evaluate([v]) is False


# ---- near misses: these must stay ----------------------------------------------------------

@pytest.mark.parametrize("w", WIDTHS[1:])
def test_shift_by_width_minus_one_stays(w):
    for op in (ir.W_SHL, ir.W_LSHR, ir.W_ASHR):
        prog = rule_program(k_right(op, lambda w: w - 1), w, False, False)
        assert has_op(assert_same_verdicts(prog, w), op), (ir.OPNAMES[op], w)


@pytest.mark.parametrize("w", WIDTHS[:-1])
def test_all_ones_of_256_bits_is_not_all_ones_of_the_width(w):
    """M(w) in the rules is the instruction's width's: x | (2^256 - 1) and x & (2^256 - 1) at
    width w < 256, the constant held at 256 bits, are not M(w) and x to the oracle (which does
    not mask OR and AND), so both stay; and a constant M(256) masked to w by its W_CONST is M(w)
    and folds."""
    for op in (ir.W_OR, ir.W_AND):
        s = Asm(f"m256:{ir.OPNAMES[op]}/w{w}", parents=False)
        s.wvar(0, w, None)
        s.wvar(1, 256, None)
        s.wconst(2, 256, M(256))
        s.w(op, w, 3, 0, 2)
        s.cmp(ir.B_EQ, 256, 0, 3, 1)
        s.p.emit(ir.ASSERT, 1, a=0)
        prog = s.done()
        batch = ir.Batch([prog])
        code, descs = device_program(batch)
        rows = rows_of(code, descs)
        assert has_op(rows, op), (ir.OPNAMES[op], w, rows)
        sv = O.SetView.from_batch(batch, 0)
        rng = random.Random(w)
        for x in boundary_values(w, rng):
            for y in (x, M(256), M(w), 0):
                assert eval_device(sv, rows, [x, y]) == sv.evaluate([x, y])
    dag = Dag()
    x, y = dag.var("x", w), dag.var("y", w)
    ones = dag.add(K_CONST, w, (), M(256))          # pool entry 2^256 - 1, loaded at width w
    dag.assert_(dag.add(ir.B_EQ, w, (dag.add(ir.W_AND, w, (x, ones)), y), 0, True))
    assert not has_op(assert_same_verdicts(lower(dag), w), ir.W_AND)


@pytest.mark.parametrize("w", WIDTHS)
def test_a_reused_register_number_is_not_the_same_value(w):
    """r2 = x + y is copied to r3, then r2 is rewritten with x * y: r2 % r3 reads two values
    that shared register 2 at different times.  It stays; and r3 % r3' with r3' a copy of the
    first sum folds."""
    for op in (ir.W_UREM, ir.W_SREM, ir.W_SMOD, ir.W_SUB, ir.W_XOR):
        for stale in (True, False):
            s = Asm(f"reuse:{ir.OPNAMES[op]}/w{w}", parents=False)
            s.wvar(0, w, None)
            s.wvar(1, w, None)
            s.w(ir.W_ADD, w, 2, 0, 1)
            s.w(ir.W_MOV, w, 3, 2)
            if stale:
                s.w(ir.W_MUL, w, 2, 0, 1)
            s.w(op, w, 4, 2, 3)
            s.cmp(ir.B_EQ, w, 0, 4, 1)
            s.p.emit(ir.ASSERT, 1, a=0)
            prog = s.done()
            rows = assert_same_verdicts(prog, w)
            assert has_op(rows, op) == stale, (ir.OPNAMES[op], w, stale, rows)


# ---- the benchmark's programs and the corpus buckets ---------------------------------------

def _aux1(code, d):
    return int(np.asarray(code[int(d[0]):int(d[0]) + int(d[1]), 3], dtype=np.uint64).sum())


def _heavy_counts(code, d):
    ops = code[int(d[0]):int(d[0]) + int(d[1]), 0] & 0xFF
    return {op: int((ops == op).sum()) for op in HEAVY}


def _check_sets(progs, monkeypatch, seed):
    batch = ir.Batch(progs)
    lowered = np.asarray(batch.code, dtype=np.uint32).reshape(-1, 4)
    code, descs = device_program(batch)
    monkeypatch.setenv("PF_DEVICE_FOLD", "0")
    code_off, descs_off = device_program(batch)
    monkeypatch.setenv("PF_DEVICE_FOLD", "2")
    code_f, descs_f = device_program(batch)
    monkeypatch.delenv("PF_DEVICE_FOLD")
    rng = random.Random(seed)
    for s, prog in enumerate(progs):
        sv = O.SetView.from_batch(batch, s)
        d, lo = descs[s], batch.descs[s]
        rows = rows_of(code, descs, s)
        assert rows[-1][0] & 0xFF == ir.END and ir.END not in opcodes(rows[:-1]), s
        assert int(d[1]) <= int(lo[1]), s
        assert _aux1(code, d) == _aux1(lowered, lo) == _aux1(code_off, descs_off[s]), s
        cands = sv.gen_assignments(np.arange(24, dtype=np.uint64), 5)
        for vals in cands + [[rng.getrandbits(sv.var_width(v)) for v in range(len(sv.schema))]]:
            assert eval_device(sv, rows, vals) == sv.evaluate(vals), s
        assert _heavy_counts(code_off, descs_off[s]) == _heavy_counts(lowered, lo), s
        # the pass alone: still a lowered program (no device flag), with the same verdicts
        f = descs_f[s]
        words = code_f[int(f[0]):int(f[0]) + int(f[1])]
        assert not (words[:, 0] >> 24).any(), s
        frows = rows_of(code_f, descs_f, s)
        for vals in cands[:8]:
            assert eval_device(sv, frows, vals) == sv.evaluate(vals), s
    # fixed point: the folded programs (the arrays as they are: ir.Batch would recompute aux1)
    # go through unchanged, and their device programs are the device programs of the lowered ones
    again = types.SimpleNamespace(code=code_f, descs=descs_f, consts=batch.consts)
    code2, descs2 = device_program(again)
    monkeypatch.setenv("PF_DEVICE_FOLD", "2")
    code_f2, descs_f2 = device_program(again)
    monkeypatch.delenv("PF_DEVICE_FOLD")
    for s in range(len(progs)):
        for (ca, da), (cb, db) in (((code_f, descs_f), (code_f2, descs_f2)), ((code, descs), (code2, descs2))):
            a = ca[int(da[s][0]):int(da[s][0]) + int(da[s][1])]
            b = cb[int(db[s][0]):int(db[s][0]) + int(db[s][1])]
            assert a.shape == b.shape and (a == b).all(), s


@pytest.mark.parametrize("plant", (False, True), ids=("plain", "planted"))
def test_config3_sets_keep_their_verdicts(monkeypatch, plant):
    _check_sets([synth.random_dag_set(i, plant=plant)[0] for i in range(200)], monkeypatch, 3)


def test_corpus_buckets_keep_their_verdicts(monkeypatch):
    _check_sets(_programs(monkeypatch), monkeypatch, 4)


def _weighted_cost(code):
    ops = code[:, 0] & 0xFF
    cost = np.full(len(ops), 10, dtype=np.int64)
    cost[ops == ir.W_MUL] = 12
    cost[np.isin(ops, DIV_OPS + (ir.B_UMUL_NOOVF,))] = 40
    cost[ops == ir.W_EXP] = 110
    return int(cost.sum())


def test_effect_floor_on_the_benchmark_programs(monkeypatch):
    """Config-3 ids 0..399, the wave-order weights of pf_batch_create (EXP 110, division 40,
    MUL 12, other 10): the folded programs cost at most 0.80 of the unfolded ones (the rule
    set gives 0.75 before the zeros that have to keep an operand's writer)."""
    batch = ir.Batch([synth.random_dag_set(i, plant=False)[0] for i in range(400)])
    code, _ = device_program(batch)
    monkeypatch.setenv("PF_DEVICE_FOLD", "0")
    code_off, _ = device_program(batch)
    ratio = _weighted_cost(code) / _weighted_cost(code_off)
    print(f"weighted cost {_weighted_cost(code)} / {_weighted_cost(code_off)} = {ratio:.4f}; "
          f"instructions {len(code)} / {len(code_off)}")
    assert ratio <= 0.80, ratio
