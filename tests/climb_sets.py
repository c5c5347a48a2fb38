"""Test tooling (not a test): the hand-made sets of the climb tests, shared by the CPU checks
of the model (test_climb_model.py) and the device comparison (test_gpu_climb.py).

Every "near" set carries a parent model a few bits away from its only solutions, so a climb
of a few rounds of <= 1,024 candidates can reach them, while the plain search cannot: its
candidates mutate the parent one bit at a time and draw everything else at random or from the
constants, and the solutions are neither.  NEAR_SEEDS below are candidate seeds for which both
facts hold; test_climb_model.py asserts them on the CPU (C oracle / model) before the GPU test
relies on them."""

from mythril_amd import ir
from op_programs import Asm

X = 0x8F3A6C21D4E7B5909A1C3E5F7B2D4F6081A3C5E7092B4D6F8E0C2A4B6D8F1E37
K = 0x5DEECE66D1234567F00DFACE0BADC0DE13579BDF02468ACE1122334455667788

# three bytes of X, by bit position of their least significant bit
BYTES = (16, 104, 200)


def _byte(v, lo):
    return (v >> lo) & 0xFF


def bytes3(flips=(19, 107), base=0, name="bytes3", unfused=False, spill=False):
    """One 256-bit variable x; asserts: byte(x, lo) == byte(X, lo) for the three BYTES.  The
    parent is X with the bits ``flips`` inverted (inside the compared bytes).  ``unfused``: every
    compare goes through two B_NOTs, so the assert site is a bool op and scores 0 or 512;
    ``spill``: x goes through spill slots, one kept in scratch (a W_EXP between spill and fill),
    one free to live in LDS."""
    a = Asm(name, base=base)
    parent = X
    for f in flips:
        parent ^= 1 << f
    a.wvar(0, 256, parent)
    src = 0
    if spill:
        a.p.emit(ir.W_SPILL, 256, a=0 + base, aux0=5)
        a.wconst(1, 256, 3)
        a.w(ir.W_EXP, 256, 2, 1, 1)                 # rewrites LDS entries 1..3: slot 5 stays in scratch
        a.p.emit(ir.W_FILL, 256, dst=3 + base, aux0=5)
        a.p.emit(ir.W_SPILL, 256, a=3 + base, aux0=9)
        a.p.emit(ir.W_FILL, 256, dst=4 + base, aux0=9)
        a.assert_eq(256, 2, 27, 1, bd=3)            # 3 ** 3, so the EXP stays live
        src = 4
    for i, lo in enumerate(BYTES):
        a.w(ir.W_EXTRACT, 8, 5, src, aux0=lo)
        a.wconst(6, 8, _byte(X, lo))
        a.cmp(ir.B_EQ, 8, i, 5, 6)
        if unfused:
            a.b(ir.B_NOT, 8 + i, a=i)
            a.b(ir.B_NOT, 16 + i, a=8 + i)
            a.p.emit(ir.ASSERT, 1, a=16 + i)
        else:
            a.p.emit(ir.ASSERT, 1, a=i)
    return a.done()


def orderings(flips=(70, 130), base=0, name="orderings"):
    """t = x ^ K must lie in (L, H]: ULT(L, t), SLE(t, H) and SLT(L, t) with H - L = 64 — the
    solutions are x = K ^ (L + 1 .. H), none of them a constant of the set or its neighbour.
    The parent's t is a solution plus two powers of two (the first bits at or above ``flips``
    that are clear in it), so clearing the higher one, then the lower one, each shortens
    |t - H|; clearing the lower one first changes no score."""
    a = Asm(name, base=base)
    low = (X >> 1) & ~0xFFFF               # positive as a signed 256-bit value
    sol = (low + 17) ^ K
    parent = sol
    for f in flips:
        while (low + 17) >> f & 1:
            f += 1
        parent ^= 1 << f
    a.wvar(0, 256, parent)
    a.wconst(1, 256, K)
    a.w(ir.W_XOR, 256, 2, 0, 1)
    a.wconst(3, 256, low)
    a.cmp(ir.B_ULT, 256, 0, 3, 2)
    a.p.emit(ir.ASSERT, 1, a=0)
    a.wconst(4, 256, low + 64)
    a.cmp(ir.B_SLE, 256, 1, 2, 4)
    a.p.emit(ir.ASSERT, 1, a=1)
    a.cmp(ir.B_SLT, 256, 2, 3, 2)          # ... also as signed values: t is not negative
    a.p.emit(ir.ASSERT, 1, a=2)
    return a.done()


def bare_end():
    a = Asm("bare-end")
    return a.done()


def no_vars(holds=True):
    """A variable-free program: 5 == 5 (a witness in round 0) or 5 == 6 (never)."""
    a = Asm("no-vars" if holds else "no-vars-false")
    a.wconst(0, 256, 5)
    a.assert_eq(256, 0, 5 if holds else 6, 1)
    return a.done()


def flat():
    """Every candidate scores the same (the only site, 5 == 6, fails for all of them), while a
    256-bit variable is free: round 0's best is index 0, every later round's is index 1 (the
    smallest that may move), and each is adopted as a sideways move — the returned assignment is
    candidate 1 of the last round."""
    a = Asm("flat", parents=False)
    a.wvar(2, 256, None)
    a.wconst(0, 256, 5)
    a.assert_eq(256, 0, 6, 1)
    return a.done()


def kinds():
    """One variable of every schema kind (and a plain one), none with a parent of its own; the
    asserts cannot all hold (the last is 5 == 6), so the set runs every round."""
    a = Asm("kinds", parents=False)
    p = a.p
    actors = [p.const_index(0xDEADBEEFDEADBEEFDEADBEEFDEADBEEFDEADBEEF),
              p.const_index(0xAFFEAFFEAFFEAFFEAFFEAFFEAFFEAFFEAFFEAFFE)]
    kbase = p.const_index(0x6B65636361 << 200)
    word = p.const_index(0xA9059CBB << 224)
    a.wvar(0, 160, None, kind=ir.VK_ACTOR, hint0=actors[0], hint1=2)
    a.wvar(1, 256, None, kind=ir.VK_KECCAK, hint0=kbase)
    a.wvar(2, 32, None, kind=ir.VK_SMALL, hint0=100)
    a.bvar(0, None)
    a.wvar(3, 8, None, kind=ir.VK_CDBYTE, hint0=24 | (1 << 8) | (word << 20), hint1=0xFFFFFFFF)
    a.wvar(4, 256, None, kind=ir.VK_VALUE)
    a.wvar(5, 256, None)
    # one compare per variable against a value the generator does not draw, so every score is
    # a sum of distance terms that the variables move
    for i, (reg, w) in enumerate(((0, 160), (1, 256), (2, 32), (3, 8), (4, 256), (5, 256))):
        a.wconst(6, w, (X >> (5 * i)) & ir.mask(w))
        a.cmp(ir.B_EQ if i % 2 == 0 else ir.B_ULT, w, 1 + i, reg, 6)
        a.p.emit(ir.ASSERT, 1, a=1 + i)
    a.p.emit(ir.ASSERT, 1, a=0)
    a.wconst(0, 256, 5)
    a.assert_eq(256, 0, 6, 1, bd=9)
    return a.done()


def long_exp(n=200):
    """A long program for the deadline test: a chain of n W_EXP over a variable, then 5 == 6."""
    a = Asm("long-exp", parents=False)
    a.wvar(0, 256, None)
    a.wconst(1, 256, 0x10001)
    for _ in range(n):
        a.w(ir.W_EXP, 256, 0, 0, 1)
    a.wconst(2, 256, 5)
    a.cmp(ir.B_EQ, 256, 0, 0, 2)
    a.p.emit(ir.ASSERT, 1, a=0)
    a.assert_eq(256, 2, 6, 1, bd=1)
    return a.done()


# The climb of the near sets: global seed, rounds, candidates per round
SEED, ROUNDS, PER_ROUND = 0x4D595448, 16, 1024
# per-set candidate seeds (pf_set_desc.seed) for which the plain search of 65,536 candidates
# under SEED finds nothing and the climb above ends on a witness; test_climb_model.py asserts
# both on the CPU
NEAR_SEEDS = {"bytes3": 6, "orderings": 2, "bytes3-unfused": 6, "orderings-r16": 2, "bytes3-spill": 6}


def near_sets(seeds=None):
    """The sets the plain search misses and the climb reaches: fused byte equalities,
    orderings, unfused sites, a 16-register set, spills."""
    sets = [bytes3(), orderings(), bytes3(name="bytes3-unfused", unfused=True),
            orderings(base=8, name="orderings-r16"), bytes3(name="bytes3-spill", spill=True)]
    for p in sets:
        p.seed = (seeds or NEAR_SEEDS)[p.name]
    return sets
