"""CPU: the range rules of the device program's fold pass and the constants of its own
(mythril_amd/csrc/pf_fold.h).

Every value the pass tracks carries a bound (the value is below 2^bound): a constant's bit
length, an unknown result's from its operands.  The bound decides compares against constants,
turns ``x / c``, ``x % c``, ``x & c`` and ``x >> c`` into 0 or x, and a result with bound 0 is
0.  As in test_device_fold, every rule is run at widths 1, 8, 32, 64, 160 and 256 against the
oracle over the boundary values of each variable, and the near misses must keep their
instruction.

``pf_device_program`` gets the range rules but stays readable against the caller's pool.
``pf_device_batch`` (``_lib.device_batch``) returns what pf_batch_create uploads: there a W
result known to be a constant that is neither 0 nor in the set's pool becomes a W_CONST of a
constant appended behind the set's own in the device pool."""

import copy
import random

import numpy as np
import pytest

import pyoracle as O
from mythril_amd import _lib, ir, synth
from op_programs import Asm
from test_device_fold import (M, WIDTHS, _aux1, _check_sets, _weighted_cost, assert_same_verdicts,
                              boundary_values, has_op, is_zero_idiom, opcodes, rows_of)
from test_device_program import I_KA, I_KB, device_program, eval_device

X, Y = 0, 1                      # W registers of the two variables
T0, T1, T2, T3, R = 2, 3, 4, 5, 6


def bits(w):
    """A bound p with 2 <= p <= w - 2 (widths >= 8)."""
    return max(2, w // 2)


# ---- a value with a known bound, through each propagating op ---------------------------------
# emit(s, w, p) leaves a value below 2^p (and reaching 2^p - 1 or close) in register R.

def _and(s, w, p, dst=R, src=X, tmp=T0):
    s.wconst(tmp, w, M(p))
    s.w(ir.W_AND, w, dst, src, tmp)


def via_and(s, w, p):
    _and(s, w, p)


def via_or(s, w, p):
    _and(s, w, p, dst=T1)
    _and(s, w, p - 1, dst=T2, src=Y)
    s.w(ir.W_OR, w, R, T1, T2)


def via_xor(s, w, p):
    _and(s, w, p - 1, dst=T1)
    _and(s, w, p, dst=T2, src=Y)
    s.w(ir.W_XOR, w, R, T1, T2)


def via_add(s, w, p):
    _and(s, w, p - 1, dst=T1)
    _and(s, w, p - 1, dst=T2, src=Y)
    s.w(ir.W_ADD, w, R, T1, T2)


def via_mul(s, w, p):
    _and(s, w, p - 1, dst=T1)
    _and(s, w, 1, dst=T2, src=Y)
    s.w(ir.W_MUL, w, R, T1, T2)


def via_urem_const(s, w, p):
    s.wconst(T0, w, (1 << (p - 1)) | 1)          # bit length p: x % c < c < 2^p
    s.w(ir.W_UREM, w, R, X, T0)


def via_urem_dividend(s, w, p):
    _and(s, w, p, dst=T1)
    s.w(ir.W_UREM, w, R, T1, Y)                   # x % y <= x, also for y = 0


def via_udiv_const(s, w, p):
    s.wconst(T0, w, 1 << (w - p))                # bit length w - p + 1
    s.w(ir.W_UDIV, w, R, X, T0)


def via_lshr(s, w, p):
    s.wconst(T0, w, w - p)
    s.w(ir.W_LSHR, w, R, X, T0)


def via_shl(s, w, p):
    _and(s, w, p - 1, dst=T1)
    s.wconst(T0, w, 1)
    s.w(ir.W_SHL, w, R, T1, T0)


def via_ite(s, w, p):
    _and(s, w, p, dst=T1)
    _and(s, w, p - 1, dst=T2, src=Y)
    s.cmp(ir.B_UMUL_NOOVF, w, 7, X, Y)
    s.w(ir.W_ITE, w, R, T1, T2, c=7)


def via_extract(s, w, p):
    _and(s, w, p + 1, dst=T1)
    s.w(ir.W_EXTRACT, w, R, T1, aux0=1)


def via_mov(s, w, p):
    _and(s, w, p, dst=T1)
    s.w(ir.W_MOV, w, R, T1)


def via_fill(s, w, p):
    _and(s, w, p, dst=T1)
    s.p.emit(ir.W_SPILL, w, a=T1, aux0=3)
    s.w(ir.W_NOT, w, T1, Y)                       # the register moves on; the slot keeps the value
    s.p.emit(ir.W_FILL, w, dst=R, aux0=3)


PROPAGATORS = (via_and, via_or, via_xor, via_add, via_mul, via_urem_const, via_urem_dividend, via_udiv_const,
               via_lshr, via_shl, via_ite, via_extract, via_mov, via_fill)


def plain(s, w, p):
    """The variable itself: bound w."""
    s.w(ir.W_OR, w, R, X, X)


# ---- one program per rule --------------------------------------------------------------------

def cmp_program(name, w, p, op, const, x_left, bound=via_and):
    """ASSERT (R op const) xor q, or (const op R) xor q: R below 2^p, q a bool of both variables
    through an opcode other than ``op``."""
    s = Asm(f"{name}/w{w}", parents=False)
    s.wvar(X, w, None)
    s.wvar(Y, w, None)
    bound(s, w, p)
    s.wconst(T3, w, const)
    s.cmp(op, w, 0, *((R, T3) if x_left else (T3, R)))
    s.cmp(ir.B_EQ if op != ir.B_EQ else ir.B_ULT, w, 1, Y, X)
    s.b(ir.B_XOR, 2, 0, 1)
    s.assert_(2)
    return s.done()


def w_program(name, w, p, op, const, bound=via_and, aux0=0):
    """ASSERT op(R, const) == y (EXTRACT: op(R) with lo = aux0)."""
    s = Asm(f"{name}/w{w}", parents=False)
    s.wvar(X, w, None)
    s.wvar(Y, w, None)
    bound(s, w, p)
    if op == ir.W_EXTRACT:
        s.w(op, w, T3, R, aux0=aux0)
    else:
        s.wconst(T3, w, const)
        s.w(op, w, T3, R, T3)
    s.cmp(ir.B_EQ, w, 0, T3, Y)
    s.assert_(0)
    return s.done()


def uadd_program(name, w, pa, pb, const=None):
    s = Asm(f"{name}/w{w}", parents=False)
    s.wvar(X, w, None)
    s.wvar(Y, w, None)
    _and(s, w, pa, dst=T1) if pa < w else s.w(ir.W_OR, w, T1, X, X)
    if const is None:
        _and(s, w, pb, dst=T2, src=Y)
    else:
        s.wconst(T2, w, const)
    s.cmp(ir.B_UADD_NOOVF, w, 0, T1, T2)
    s.cmp(ir.B_EQ, w, 1, Y, X)
    s.b(ir.B_XOR, 2, 0, 1)
    s.assert_(2)
    return s.done()


def folding_programs(w):
    """(program, the opcode that must be gone)."""
    out = []

    def c(name, p, op, const, x_left, bound=via_and):
        out.append((cmp_program(name, w, p, op, const, x_left, bound), op))

    c("0<=x", w, ir.B_ULE, 0, False, plain)
    c("x<=M", w, ir.B_ULE, M(w), True, plain)
    c("x<0", w, ir.B_ULT, 0, True, plain)
    c("M<x", w, ir.B_ULT, M(w), False, plain)
    if w == 1:
        return out
    p = bits(w)
    c("x<=2^p-1", p, ir.B_ULE, M(p), True)
    for cv, tag in ((1 << p, "2^p"), (M(w), "M")):
        c(f"x<{tag}", p, ir.B_ULT, cv, True)
        c(f"x<={tag}", p, ir.B_ULE, cv, True)
        c(f"x=={tag}", p, ir.B_EQ, cv, True)
        c(f"{tag}<x", p, ir.B_ULT, cv, False)
        c(f"{tag}<=x", p, ir.B_ULE, cv, False)
        c(f"{tag}==x", p, ir.B_EQ, cv, False)
    # signed: both sides below 2^(w-1)
    c("0<=s x", p, ir.B_SLE, 0, False)
    c("x<s 0", p, ir.B_SLT, 0, True)
    c("x<=s 2^p-1", p, ir.B_SLE, M(p), True)
    for op, left in ((ir.B_SLT, True), (ir.B_SLE, True), (ir.B_SLT, False), (ir.B_SLE, False)):
        c(f"signed {ir.OPNAMES[op]} 2^p {'right' if left else 'left'}", p, op, 1 << p, left)
    out.append((uadd_program("noovf(x,y)", w, w - 1, w - 1), ir.B_UADD_NOOVF))
    out.append((uadd_program("noovf(x,c)", w, p, 0, const=M(w - 1)), ir.B_UADD_NOOVF))
    for cv in (1 << p, M(w)):
        out.append((w_program("x/c", w, p, ir.W_UDIV, cv), ir.W_UDIV))
        out.append((w_program("x%c", w, p, ir.W_UREM, cv), ir.W_UREM))
    out.append((w_program("x&c", w, p, ir.W_AND, M(p) | (1 << (w - 1)), bound=via_lshr), ir.W_AND))
    out.append((w_program("x>>p", w, p, ir.W_LSHR, p), ir.W_LSHR))
    out.append((w_program("x>>w-1", w, p, ir.W_LSHR, w - 1), ir.W_LSHR))
    out.append((w_program("extract above the bound", w, p, ir.W_EXTRACT, 0, aux0=p), ir.W_EXTRACT))
    return out


def staying_programs(w):
    """Near misses: (program, the opcode that must stay)."""
    p = bits(w)
    out = [
        (cmp_program("x<=M-1", w, w, ir.B_ULE, M(w) - 1, True, plain), ir.B_ULE),
        (cmp_program("1<=x", w, w, ir.B_ULE, 1, False, plain), ir.B_ULE),
        (cmp_program("x<1", w, w, ir.B_ULT, 1, True, plain), ir.B_ULT),
        (cmp_program("M-1<x", w, w, ir.B_ULT, M(w) - 1, False, plain), ir.B_ULT),
        # c = 2^p - 1 on the left is decided too, but the rule set stops at c >= 2^p
        (cmp_program("2^p-1<x", w, p, ir.B_ULT, M(p), False), ir.B_ULT),
        (cmp_program("x<2^p-1", w, p, ir.B_ULT, M(p), True), ir.B_ULT),
        (cmp_program("x<=2^p-2", w, p, ir.B_ULE, M(p) - 1, True), ir.B_ULE),
        (cmp_program("x==2^p-1", w, p, ir.B_EQ, M(p), True), ir.B_EQ),
        # a signed compare whose constant has the sign bit set, or whose value may have it
        (cmp_program("x<s -1", w, p, ir.B_SLT, M(w), True), ir.B_SLT),
        (cmp_program("x<=s min", w, p, ir.B_SLE, 1 << (w - 1), True), ir.B_SLE),
        (cmp_program("0<=s x", w, w, ir.B_SLE, 0, False, plain), ir.B_SLE),
        # a bound that only holds at a wider width: w bits, not w - 1
        (uadd_program("noovf(x,y)", w, w, w - 1), ir.B_UADD_NOOVF),
        (uadd_program("noovf(x,2^(w-1))", w, p, 0, const=1 << (w - 1)), ir.B_UADD_NOOVF),
        (w_program("x/(2^p-1)", w, p, ir.W_UDIV, M(p)), ir.W_UDIV),
        (w_program("x%(2^p-1)", w, p, ir.W_UREM, M(p)), ir.W_UREM),
        (w_program("x&(2^(p-1)-1)", w, p, ir.W_AND, M(p - 1) | (1 << (w - 1)), bound=via_lshr), ir.W_AND),
        (w_program("x>>p-1", w, p, ir.W_LSHR, p - 1), ir.W_LSHR),
        (w_program("extract below the bound", w, p, ir.W_EXTRACT, 0, aux0=p - 1), ir.W_EXTRACT),
        # bounds that would be one bit too low
        (cmp_program("x+y<2^p", w, p, ir.B_ULT, 1 << p, True, lambda s, w, p: via_add(s, w, p + 1)), ir.B_ULT),
        (cmp_program("x*y<2^p", w, p, ir.B_ULT, 1 << p, True,
                     lambda s, w, p: (_and(s, w, p, dst=T1), _and(s, w, 1, dst=T2, src=Y),
                                      s.w(ir.W_MUL, w, R, T1, T2))), ir.B_ULT),
    ]
    # x / y says nothing: y = 0 gives M(w)
    s = Asm(f"x/y<2^p/w{w}", parents=False)
    s.wvar(X, w, None)
    s.wvar(Y, w, None)
    _and(s, w, p, dst=T1)
    s.w(ir.W_UDIV, w, R, T1, Y)
    s.wconst(T3, w, 1 << p)
    s.cmp(ir.B_ULT, w, 0, R, T3)
    s.assert_(0)
    out.append((s.done(), ir.B_ULT))
    return out


@pytest.mark.parametrize("w", WIDTHS)
def test_every_range_rule_folds_at_every_width(w):
    for prog, op in folding_programs(w):
        assert op in [i.op for i in prog.code], (prog.name, w)
        rows = assert_same_verdicts(prog, w)
        assert not has_op(rows, op), (prog.name, rows)


@pytest.mark.parametrize("w", WIDTHS[1:])
def test_a_bound_arrives_through_each_propagating_op(w):
    """R < 2^p with R built by each op that hands a bound on — (x & 0xff) < 256,
    (x >> 200) <= 2^56 - 1, (x % c) < c among them."""
    p = bits(w)
    for bound in PROPAGATORS:
        for op, cv in ((ir.B_ULT, 1 << p), (ir.B_ULE, M(p))):
            prog = cmp_program(f"{bound.__name__}:{ir.OPNAMES[op]}", w, p, op, cv, True, bound)
            rows = assert_same_verdicts(prog, w)
            assert not has_op(rows, op), (prog.name, rows)
            # one bit less is a near miss for the propagators that reach 2^p - 1
            if bound in (via_and, via_or, via_xor, via_lshr, via_udiv_const, via_mov, via_fill, via_urem_dividend):
                prog = cmp_program(f"{bound.__name__}:near", w, p, ir.B_ULT, 1 << (p - 1), True, bound)
                assert has_op(assert_same_verdicts(prog, w), ir.B_ULT), prog.name
    # the three of the issue, as written
    if w >= 32:
        s = cmp_program("(x&0xff)<256", w, 8, ir.B_ULT, 256, True)
        assert not has_op(assert_same_verdicts(s, w), ir.B_ULT)
    if w == 256:
        s = cmp_program("(x>>200)<=2^56-1", w, 56, ir.B_ULE, M(56), True, via_lshr)
        assert not has_op(assert_same_verdicts(s, w), ir.B_ULE)
    s = Asm(f"(x%c)<c/w{w}", parents=False)
    s.wvar(X, w, None)
    s.wvar(Y, w, None)
    s.wconst(T0, w, 1 << (p - 1))                # a power of two: x % c < c = 2^(p-1) needs the
    s.w(ir.W_UREM, w, R, X, T0)                  # divisor's bit length, not the value
    s.wconst(T3, w, 1 << p)
    s.cmp(ir.B_ULT, w, 0, R, T3)
    s.cmp(ir.B_EQ, w, 1, Y, X)
    s.b(ir.B_XOR, 2, 0, 1)
    s.assert_(2)
    assert not has_op(assert_same_verdicts(s.done(), w), ir.B_ULT)


@pytest.mark.parametrize("w", WIDTHS[1:])
def test_near_misses_keep_their_instruction(w):
    for prog, op in staying_programs(w):
        rows = assert_same_verdicts(prog, w)
        assert has_op(rows, op), (prog.name, rows)


def test_a_dropped_root_takes_its_chain_along():
    """0 <= ((x / y) ** y): the assert goes, and with it the division and the EXP."""
    s = Asm("dropped-root", parents=False)
    s.wvar(X, 256, None)
    s.wvar(Y, 256, None)
    s.w(ir.W_UDIV, 256, T1, X, Y)
    s.w(ir.W_EXP, 256, T2, T1, Y)
    s.wconst(T3, 256, 0)
    s.cmp(ir.B_ULE, 256, 0, T3, T2)
    s.assert_(0)
    s.cmp(ir.B_ULT, 256, 1, X, Y)
    s.assert_(1)
    prog = s.done()
    batch = ir.Batch([prog])
    rows = assert_same_verdicts(prog, 256)
    assert [o for o in opcodes(rows) if o in (ir.W_UDIV, ir.W_EXP, ir.B_ULE)] == []
    code, descs = device_program(batch)
    assert _aux1(code, descs[0]) == _aux1(np.asarray(batch.code, dtype=np.uint32).reshape(-1, 4), batch.descs[0])


def test_rule_programs_are_a_fixed_point_of_the_pass(monkeypatch):
    """test_device_fold's checks (same verdicts, same aux1 totals, PF_DEVICE_FOLD=2 output fed
    back in unchanged and to the same device program) over the programs of the rules above."""
    progs = []
    for w in (8, 160, 256):
        progs += [p for p, _ in folding_programs(w)] + [p for p, _ in staying_programs(w)]
    _check_sets(progs, monkeypatch, 6)


# ---- constants of the device program's own ---------------------------------------------------

FILLERS = 15     # pf_batch_create folds batches of 16 sets or more, and so does pf_device_batch


def device_batch(progs):
    """The programs (padded past the fold gate with config-3 sets) as pf_batch_create would
    upload them: (batch, code, descs, pool)."""
    batch = ir.Batch(list(progs) + [synth.random_dag_set(700 + i, plant=False)[0] for i in range(FILLERS)])
    code, descs, pool = _lib.device_batch(batch.code, batch.consts, batch.descs)
    return batch, code, descs, pool


def pool_view(batch, descs, pool, s):
    """SetView of set s whose constants are the device pool's from the device descriptor's
    const_off on (the set's own, then the program's) — what the kernel indexes."""
    sv = copy.copy(O.SetView.from_batch(batch, s))
    sv.consts = [O.limbs_to_int(row) for row in pool[int(descs[s][2]):]]
    return sv


def check_against_pool(batch, code, descs, pool, s, w, seed=1):
    lowered = O.SetView.from_batch(batch, s)
    dev = pool_view(batch, descs, pool, s)
    rows = rows_of(code, descs, s)
    vals = boundary_values(w, random.Random(seed))
    n = len(lowered.schema)
    for x in vals:
        for y in (vals if n >= 2 else [0]):
            v = [x, y][:n]
            assert eval_device(dev, rows, v) == lowered.evaluate(v), (s, v)
    return rows


def const_result_program(w, consumer, rel=ir.B_EQ):
    """t = (c1 * c2 + c1) — a constant the pool does not hold, computed by a MUL and an ADD —
    consumed as a divisor, as an EXP base or by a compare (``rel``: how the first two results
    are compared with y)."""
    c1, c2 = 0x1234_5677 & M(w) | 1, 0x0BAD_CAFD & M(w) | 1
    s = Asm(f"own:{consumer}/w{w}", parents=False)
    s.wvar(X, w, None)
    s.wvar(Y, w, None)
    s.wconst(T0, w, c1)
    s.wconst(T1, w, c2)
    s.w(ir.W_MUL, w, T2, T0, T1)
    s.w(ir.W_ADD, w, T2, T2, T0)
    value = (c1 * c2 + c1) & M(w)
    if consumer == "divisor":
        s.w(ir.W_UREM, w, T3, X, T2)
        s.cmp(rel, w, 0, T3, Y)
    elif consumer == "exp_base":
        s.w(ir.W_EXP, w, T3, T2, X)
        s.cmp(rel, w, 0, T3, Y)
    else:
        s.w(ir.W_XOR, w, T3, X, Y)
        s.cmp(ir.B_ULT, w, 0, T3, T2)
    s.assert_(0)
    return s.done(), value


@pytest.mark.parametrize("w", WIDTHS[1:])
def test_a_constant_result_outside_the_pool_becomes_a_constant_of_the_program(w):
    built = [const_result_program(w, c) for c in ("divisor", "exp_base", "compare")]
    progs = [p for p, _ in built]
    batch, code, descs, pool = device_batch(progs)
    lowered = np.asarray(batch.code, dtype=np.uint32).reshape(-1, 4)
    consts = np.asarray(batch.consts, dtype=np.uint32).reshape(-1, 8)
    assert (pool[:len(consts)] == consts).all()                 # the caller's part, byte for byte
    for s, (prog, value) in enumerate(built):
        assert value not in prog.consts and value != 0
        rows = check_against_pool(batch, code, descs, pool, s, w)
        assert not has_op(rows, ir.W_MUL) and not has_op(rows, ir.W_ADD), (prog.name, rows)   # the feeders
        d, lo = descs[s], batch.descs[s]
        assert int(d[3]) == int(lo[3]) and list(d[4:]) == list(lo[4:])       # n_const and the schema stay
        own = pool[int(d[2]) + int(d[3])]
        assert O.limbs_to_int(own) == value
        assert (pool[int(d[2]):int(d[2]) + int(d[3])] == consts[int(lo[2]):int(lo[2]) + int(lo[3])]).all()
        k = int(d[3])                                           # the constant's index: an immediate operand
        imm = [r for r in rows if (r[0] & I_KA and (r[1] >> 8) & 0xFF == k) or (r[0] & I_KB and (r[1] >> 16) & 0xFF == k)]
        assert len(imm) == 1 and ir.W_CONST not in opcodes(rows), (prog.name, rows)
        assert _aux1(code, d) == _aux1(lowered, lo)
        # pf_device_program: the same program against the caller's pool keeps the computation
        code1, descs1 = device_program(batch)
        rows1 = rows_of(code1, descs1, s)
        assert has_op(rows1, ir.W_MUL) and has_op(rows1, ir.W_ADD)
        assert int(descs1[s][2]) == int(lo[2])
    # the fillers, with or without constants of their own, compute what they computed
    for s in range(len(progs), len(batch.descs)):
        sv, dev = O.SetView.from_batch(batch, s), pool_view(batch, descs, pool, s)
        assert _aux1(code, descs[s]) == _aux1(lowered, batch.descs[s])
        for vals in sv.gen_assignments(np.arange(16, dtype=np.uint64), 5):
            assert eval_device(dev, rows_of(code, descs, s), vals) == sv.evaluate(vals), s


def no_const_program(w=256):
    """~(x ^ x) = M(w) in a set without constants."""
    s = Asm(f"own:no-pool/w{w}", parents=False)
    s.wvar(X, w, None)
    s.wvar(Y, w, None)
    s.w(ir.W_XOR, w, T0, X, X)
    s.w(ir.W_NOT, w, T1, T0)
    s.w(ir.W_UDIV, w, T2, T1, Y)
    s.cmp(ir.B_ULT, w, 0, X, T2)
    s.assert_(0)
    return s.done()


@pytest.mark.parametrize("w", (8, 256))
def test_a_set_without_constants_gains_one(w):
    prog = no_const_program(w)
    assert prog.consts == []
    batch, code, descs, pool = device_batch([prog])
    rows = check_against_pool(batch, code, descs, pool, 0, w)
    assert int(descs[0][3]) == 0 and O.limbs_to_int(pool[int(descs[0][2])]) == M(w)
    assert not has_op(rows, ir.W_NOT) and not any(is_zero_idiom(r) for r in rows), rows
    assert [r for r in rows if r[0] & I_KA and r[0] & 0xFF == ir.W_UDIV], rows


def test_a_constant_index_past_255_stays_a_w_const():
    """PF_I_KA / PF_I_KB carry eight bits: 300 distinct constant results, the later ones stay
    W_CONSTs of their own."""
    w, n = 256, 300
    s = Asm("own:many", parents=False)
    s.wvar(X, w, None)
    s.wvar(Y, w, None)
    s.wconst(T0, w, 0x10001)
    s.wconst(T1, w, 3)
    s.w(ir.W_OR, w, T2, T1, T1)
    for i in range(n):
        s.w(ir.W_MUL, w, T2, T2, T0)              # 3 * 0x10001^(i+1): a new constant each time
        s.w(ir.W_XOR, w, X, X, T2)
    s.cmp(ir.B_EQ, w, 0, X, Y)
    s.assert_(0)
    prog = s.done()
    batch, code, descs, pool = device_batch([prog])
    rows = check_against_pool(batch, code, descs, pool, 0, w)
    d = descs[0]
    assert int(d[3]) == 2 and not has_op(rows, ir.W_MUL)
    kept = [r for r in rows if r[0] & 0xFF == ir.W_CONST]
    imm = [r for r in rows if r[0] & (I_KA | I_KB)]
    assert kept and all(r[2] > 255 for r in kept) and len(kept) + len(imm) == n, (len(kept), len(imm))
    assert all(((r[1] >> 16) & 0xFF if r[0] & I_KB else (r[1] >> 8) & 0xFF) >= 2 for r in imm)
    # one entry per value
    own = [O.limbs_to_int(r) for r in pool[int(d[2]) + 2:int(d[2]) + 2 + n]]
    assert len(set(own)) == n


def test_equal_constants_share_one_entry():
    w = 64
    s = Asm("own:dedup", parents=False)
    s.wvar(X, w, None)
    s.wvar(Y, w, None)
    s.wconst(T0, w, 5)
    s.wconst(T1, w, 7)
    s.w(ir.W_MUL, w, T2, T0, T1)
    s.w(ir.W_XOR, w, T3, X, T2)
    s.w(ir.W_MUL, w, T2, T1, T0)
    s.w(ir.W_ADD, w, T3, T3, T2)
    s.cmp(ir.B_EQ, w, 0, T3, Y)
    s.assert_(0)
    batch, code, descs, pool = device_batch([s.done()])
    rows = check_against_pool(batch, code, descs, pool, 0, w)
    assert not has_op(rows, ir.W_MUL)
    d = descs[0]
    n_own = (len(pool) if all(int(e[2]) <= int(d[2]) for e in descs) else
             min(int(e[2]) for e in descs if int(e[2]) > int(d[2]))) - int(d[2]) - int(d[3])
    assert n_own == 1 and O.limbs_to_int(pool[int(d[2]) + int(d[3])]) == 35


def test_below_the_gate_and_with_the_pass_off_the_pool_is_the_callers(monkeypatch):
    prog, _ = const_result_program(64, "divisor")
    batch = ir.Batch([prog] * 15)
    code, descs, pool = _lib.device_batch(batch.code, batch.consts, batch.descs)
    assert (pool == np.asarray(batch.consts, dtype=np.uint32).reshape(-1, 8)).all()
    assert has_op(rows_of(code, descs), ir.W_MUL)
    monkeypatch.setenv("PF_DEVICE_FOLD", "0")
    batch, code, descs, pool = device_batch([prog])
    assert (pool == np.asarray(batch.consts, dtype=np.uint32).reshape(-1, 8)).all()
    assert (descs[:, 2] == np.asarray(batch.descs)[:, 2]).all() and has_op(rows_of(code, descs), ir.W_MUL)


# ---- the benchmark's programs ----------------------------------------------------------------

FOLD_ON_BEFORE = 746_736 / 1_026_186     # config-3 ids 0..1023 before the range rules: fold on / fold off


def test_effect_floor_on_the_benchmark_batch(monkeypatch):
    """Config-3 ids 0..1023 (the benchmark's first batch), the wave-order weights, relative to
    PF_DEVICE_FOLD=0 of the same build: pf_device_program costs at most 0.94 of what it cost
    before the range rules, pf_device_batch at most 0.92; aux1 totals per set are unchanged."""
    batch = ir.Batch([synth.random_dag_set(i, plant=False)[0] for i in range(1024)])
    lowered = np.asarray(batch.code, dtype=np.uint32).reshape(-1, 4)
    code, descs = device_program(batch)
    code_b, descs_b, pool = _lib.device_batch(batch.code, batch.consts, batch.descs)
    monkeypatch.setenv("PF_DEVICE_FOLD", "0")
    code_off, _ = device_program(batch)
    off = _weighted_cost(code_off)
    r_prog, r_batch = _weighted_cost(code) / off, _weighted_cost(code_b) / off
    print(f"fold off {off}; pf_device_program {r_prog:.4f} ({r_prog / FOLD_ON_BEFORE:.4f} of {FOLD_ON_BEFORE:.4f}); "
          f"pf_device_batch {r_batch:.4f} ({r_batch / FOLD_ON_BEFORE:.4f}); pool {len(batch.consts)} -> {len(pool)}")
    assert r_prog <= 0.94 * FOLD_ON_BEFORE, r_prog
    assert r_batch <= 0.92 * FOLD_ON_BEFORE, r_batch
    consts = np.asarray(batch.consts, dtype=np.uint32).reshape(-1, 8)
    assert (pool[:len(consts)] == consts).all()
    for s in range(len(batch.descs)):
        lo = batch.descs[s]
        assert _aux1(code, descs[s]) == _aux1(code_b, descs_b[s]) == _aux1(lowered, lo), s
        assert int(descs_b[s][3]) == int(lo[3]) and list(descs_b[s][4:]) == list(lo[4:]), s
    rng = random.Random(8)
    for s in rng.sample(range(len(batch.descs)), 120):
        sv, dev = O.SetView.from_batch(batch, s), pool_view(batch, descs_b, pool, s)
        rows = rows_of(code_b, descs_b, s)
        for vals in sv.gen_assignments(np.arange(12, dtype=np.uint64), 5):
            assert eval_device(dev, rows, vals) == sv.evaluate(vals), s
