"""Test tooling (not a test): the hand-made sets of the tree-score tests, shared by the CPU
checks of the model (test_climb_tree_model.py) and the device comparison
(test_gpu_climb_tree.py).

* ``compare_row`` / ``logic_row`` — one row of the header's table each, for explicit values;
* ``table_sets`` — every row under the generator's candidates, at either register base;
* ``saturation_set`` — AND / OR of three order compares that fail by more than 128 bits;
* ``family`` — the pinned sets the tree climb witnesses and the sites climb leaves."""

from mythril_amd import ir
from op_programs import Asm

K1 = 0x8F3A6C21D4E7B5909A1C3E5F7B2D4F6081A3C5E7092B4D6F8E0C2A4B6D8F1E37
K2 = 0x5DEECE66D1234567F00DFACE0BADC0DE13579BDF02468ACE1122334455667788
K3 = 0xC2B2AE3D27D4EB4F165667B19E3779B97F4A7C15F39CC0605CEDC8341082276B


def compare_row(op, w, a, b, base=0, bd=0, fused=True):
    """B[bd] <- op(a, b) at width w over two variables, asserted: by the compare itself (the
    device program fuses the ASSERT into it) or, ``fused=False``, through two B_NOTs."""
    s = Asm(f"row:{ir.OPNAMES[op]}/w{w}/bd{bd}/base{base}/{'fused' if fused else 'plain'}", base)
    s.wvar(0, w, a)
    s.wvar(1, w, b)
    s.cmp(op, w, bd, 0, 1)
    if not fused:
        s.b(ir.B_NOT, (bd + 1) % 32, a=bd)
        s.b(ir.B_NOT, (bd + 2) % 32, a=(bd + 1) % 32)
        bd = (bd + 2) % 32
    s.p.emit(ir.ASSERT, 1, a=bd)
    return s.done(None)


# the inputs of a logic row: x = EQ(v0, v1), y = ULT(v2, v3) at 256 bits, c = a Bool variable
def logic_row(op, values, regs=(3, 0, 31, 7), base=0):
    """B[d] <- op(B[a], B[b] (, B[c])) asserted, with regs = (d, a, b, c); ``values`` =
    (v0, v1, v2, v3, c)."""
    d, ra, rb, rc = regs
    s = Asm(f"row:{ir.OPNAMES[op]}/{d}.{ra}.{rb}.{rc}/base{base}", base)
    for r, v in enumerate(values[:4]):
        s.wvar(r, 256, v)
    s.cmp(ir.B_EQ, 256, ra, 0, 1)
    s.cmp(ir.B_ULT, 256, rb, 2, 3)
    s.bvar(rc, values[4])
    s.b(op, d, a=ra, b=rb, c=rc)
    s.p.emit(ir.ASSERT, 1, a=d)
    return s.done(None)


def table_sets(base=0):
    """Every writer of the table under generated candidates.  None of them can hold (each ends
    in 5 == 6 through a NOT NOT), so every round runs."""
    out = []

    def never(s, bd):
        s.wconst(4, 256, 5)
        s.wconst(5, 256, 6)
        s.cmp(ir.B_EQ, 256, bd, 4, 5)
        s.b(ir.B_NOT, bd, a=bd)
        s.b(ir.B_NOT, bd, a=bd)
        s.p.emit(ir.ASSERT, 1, a=bd)

    # compares at 256 and 64 bits, each asserted as written (fused) and negated (a B_NOT site)
    s = Asm(f"table:compares/base{base}", base)
    s.wvar(0, 256, K1)
    s.wvar(1, 256, K1 ^ (1 << 77) ^ (1 << 3))
    s.wvar(2, 64, K2 & ir.mask(64))
    s.wvar(3, 64, (K2 >> 7) & ir.mask(64))
    k = 0
    for w, (ra, rb) in ((256, (0, 1)), (64, (2, 3))):
        for op in (ir.B_EQ, ir.B_ULT, ir.B_ULE, ir.B_SLT, ir.B_SLE):
            s.cmp(op, w, k, ra, rb)
            s.p.emit(ir.ASSERT, 1, a=k)
            s.cmp(op, w, k + 1, rb, ra)
            s.b(ir.B_NOT, k + 2, a=k + 1)
            s.p.emit(ir.ASSERT, 1, a=k + 2)
            k += 3
    never(s, 31)
    out.append(s.done(False))

    # leaves without a gradient, Bool variables, and the two-input ops over B0 and B31
    s = Asm(f"table:logic/base{base}", base)
    s.wvar(0, 256, K1)
    s.wvar(1, 256, K3)
    s.wvar(2, 64, 0xFFFF_FFFF)
    s.wvar(3, 64, 0x1_0000_0001)
    s.cmp(ir.B_EQ, 256, 0, 0, 1)
    s.cmp(ir.B_ULT, 256, 31, 1, 0)
    s.cmp(ir.B_UADD_NOOVF, 256, 1, 0, 1)
    s.cmp(ir.B_UMUL_NOOVF, 64, 2, 2, 3)
    s.b(ir.B_CONST, 3, aux0=0)
    s.b(ir.B_CONST, 4, aux0=1)
    s.bvar(5, 1)
    s.bvar(6, 0)
    k = 7
    for op in (ir.B_AND, ir.B_OR, ir.B_XOR):
        for ra, rb in ((0, 31), (31, 1), (2, 0), (3, 31), (4, 0), (5, 31), (6, 0), (5, 6)):
            s.b(op, k, a=ra, b=rb)
            s.p.emit(ir.ASSERT, 1, a=k)
            k = 7 + (k - 6) % 20
    for rc, ra, rb in ((5, 0, 31), (6, 31, 0), (0, 5, 31), (31, 2, 1), (1, 31, 31)):
        s.b(ir.B_ITE, k, a=ra, b=rb, c=rc)
        s.p.emit(ir.ASSERT, 1, a=k)
        k = 7 + (k - 6) % 20
    s.b(ir.B_NOT, 30, a=0)
    s.b(ir.B_NOT, 0, a=30)                 # NOT NOT x back in x's own register
    s.p.emit(ir.ASSERT, 1, a=0)
    never(s, 29)
    out.append(s.done(False))
    return out


def saturation_set(kind, values=(None, None, None), base=0):
    """ULT(v_i, 5) for three 256-bit variables, joined by ``kind`` (B_AND / B_OR), asserted."""
    s = Asm(f"sat:{ir.OPNAMES[kind]}/base{base}", base, parents=values[0] is not None)
    s.wconst(3, 256, 5)
    for i, v in enumerate(values):
        s.wvar(i, 256, v)
        s.cmp(ir.B_ULT, 256, i, i, 3)
    s.b(kind, 3, a=0, b=1)
    s.b(kind, 4, a=3, b=2)
    s.p.emit(ir.ASSERT, 1, a=4)
    return s.done(None)


# ---- the pinned family ---------------------------------------------------------------------
# Three 6-bit fields s0, s1, s2 (VK_SMALL variables, uniform in 0..63, no parents) placed at
# 256-bit constants' positions: t = s0 * M0 + s1 * M1 + s2 * M2 + C.  One assignment of 2^18
# satisfies each set, so 8 rounds of 256 candidates meet it by chance in under 1 % of the
# seeds; under the sites score every candidate of these sets scores 0 (their only site is a
# B_NOT, B_OR or B_AND).  The tree score follows the order compares' bitlen and the
# equalities' popcount.
FIELD = 63
M = (1 << 250, 1 << 244, 1 << 238)
C0 = K2 & ir.mask(200)
ROUNDS, PER_ROUND, SEED = 8, 256, 0x54524545
SHAPES = ("not-ult", "or-eq", "and-ule-noteq")


def _fields(s):
    """W0 <- s0 * M0 + s1 * M1 + s2 * M2 + C0 (registers 0..3 used)."""
    s.wconst(0, 256, C0)
    for i in range(3):
        s.wvar(1, 256, None, kind=ir.VK_SMALL, hint0=FIELD)
        s.wconst(2, 256, M[i])
        s.w(ir.W_MUL, 256, 3, 1, 2)
        s.w(ir.W_ADD, 256, 0, 0, 3)


def field_value(f):
    return (sum(v * m for v, m in zip(f, M)) + C0) & ir.mask(256)


def family_set(shape, base=0, seed=0):
    assert shape in SHAPES
    s = Asm(f"family:{shape}/base{base}", base, parents=False)
    _fields(s)
    if shape == "not-ult":
        # NOT(t < K): K = the largest t, so s0 = s1 = s2 = 63
        s.wconst(1, 256, field_value((63, 63, 63)))
        s.cmp(ir.B_ULT, 256, 0, 0, 1)
        s.b(ir.B_NOT, 1, a=0)
        s.p.emit(ir.ASSERT, 1, a=1)
        s.p.solution = [(63, 63, 63)]
    elif shape == "or-eq":
        # t == Ka or t ^ K3 == Kb ^ K3: two isolated solutions
        s.wconst(1, 256, field_value((45, 19, 33)))
        s.cmp(ir.B_EQ, 256, 0, 0, 1)
        s.wconst(2, 256, K3)
        s.w(ir.W_XOR, 256, 3, 0, 2)
        s.wconst(1, 256, field_value((10, 52, 7)) ^ K3)
        s.cmp(ir.B_EQ, 256, 1, 3, 1)
        s.b(ir.B_OR, 2, a=0, b=1)
        s.p.emit(ir.ASSERT, 1, a=2)
        s.p.solution = [(45, 19, 33), (10, 52, 7)]
    else:
        # (t < K or t == K) and not (t == C0 + M2): K = C0 + M2, so t is C0 (all fields 0)
        s.wconst(1, 256, field_value((0, 0, 1)))
        s.cmp(ir.B_ULT, 256, 0, 0, 1)
        s.cmp(ir.B_EQ, 256, 1, 0, 1)
        s.b(ir.B_OR, 2, a=0, b=1)
        s.b(ir.B_NOT, 3, a=1)
        s.b(ir.B_AND, 4, a=2, b=3)
        s.p.emit(ir.ASSERT, 1, a=4)
        s.p.solution = [(0, 0, 0)]
    p = s.done(None)
    p.seed = seed
    return p


# per set: the candidate seed (pf_set_desc.seed) under which the tree climb of ROUNDS x PER_ROUND
# with global seed SEED ends on a witness and the sites climb does not; test_climb_tree_model.py
# asserts both with the two models
FAMILY = (("not-ult", 0), ("or-eq", 0), ("and-ule-noteq", 0), ("not-ult", 8), ("or-eq", 8))
FAMILY_SEEDS = {"family:not-ult/base0": 1, "family:or-eq/base0": 4, "family:and-ule-noteq/base0": 14,
                "family:not-ult/base8": 1, "family:or-eq/base8": 4}


def family():
    return [family_set(shape, base, FAMILY_SEEDS[f"family:{shape}/base{base}"]) for shape, base in FAMILY]
