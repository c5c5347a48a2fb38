"""Test tooling (not a test): the hand-made sets of the census tests, shared by the CPU checks of
the model (test_census_model.py) and the device comparison (test_gpu_census.py).

Small programs whose assert sites hold for some candidates and fail for others, so every census
output is non-trivial: a set with witnesses, sets without one, sites that are the only failing
one, plain PF_ASSERT sites next to fused ones, more than 32 sites, a B value that crosses two
sites through a spill slot, a set for the 16-register kernel.  test_census_model.py asserts on
the CPU that they are not degenerate before the GPU test relies on them."""

from mythril_amd import ir
from op_programs import Asm

X = 0x8F3A6C21D4E7B5909A1C3E5F7B2D4F6081A3C5E7092B4D6F8E0C2A4B6D8F1E37

SEED, SEED2 = 0x43454E53, 0x5355534E
BUDGETS = (209, 64, 1)     # three full groups and a 17-lane tail; one group; one lane


def one_site(base=0, name="one-site"):
    """x (8 bits, no parent) == 0x5A: one fused site, and a constant the generator harvests, so
    a few candidates of every hundred are witnesses."""
    a = Asm(name, base=base, parents=False)
    a.wvar(0, 8, None)
    a.assert_eq(8, 0, 0x5A, 1)
    return a.done()


def bare_end():
    return Asm("bare-end").done()


def folded_away():
    """x ^ x == 0: the fold pass proves the only assert, so a folded batch runs a bare END for
    it; an unfolded one keeps the site, which every candidate passes."""
    a = Asm("folded-away", parents=False)
    a.wvar(0, 8, None)
    a.w(ir.W_XOR, 8, 1, 0, 0)
    a.assert_eq(8, 1, 0, 2)
    return a.done()


def ground(holds=True):
    """5 == 5 / 5 == 6 without a variable (the fold pass leaves such programs as lowered): one
    fused site that every candidate passes, or none does."""
    a = Asm("ground-true" if holds else "ground-false")
    a.wconst(0, 256, 5)
    a.assert_eq(256, 0, 5 if holds else 6, 1)
    return a.done()


def contra():
    """x == 5, x == 6, x == 7: no witness, and every candidate fails at least two sites."""
    a = Asm("contra", parents=False)
    a.wvar(0, 8, None)
    for i, v in enumerate((5, 6, 7)):
        a.assert_eq(8, 0, v, 1, bd=i)
    return a.done()


def two_bounds(base=0, name="two-bounds"):
    """x < 128 and 64 <= x on a byte: below 64 the second site alone fails, from 128 on the
    first alone, so both have sole > 0; in between lie the witnesses."""
    a = Asm(name, base=base, parents=False)
    a.wvar(0, 8, None)
    a.wconst(1, 8, 128)
    a.cmp(ir.B_ULT, 8, 0, 0, 1)
    a.p.emit(ir.ASSERT, 1, a=0)
    a.wconst(2, 8, 64)
    a.cmp(ir.B_ULE, 8, 1, 2, 0)
    a.p.emit(ir.ASSERT, 1, a=1)
    return a.done()


def plain_sites():
    """Sites that stay plain PF_ASSERTs on the device: a Bool variable asserted (B_VAR is no
    compare or bool op), and one B register asserted twice (its writer carries one assert
    only) — next to a fused bool op."""
    a = Asm("plain-sites", parents=False)
    a.bvar(0, None)
    a.p.emit(ir.ASSERT, 1, a=0)
    a.bvar(1, None)
    a.wvar(0, 8, None)
    a.wconst(1, 8, 200)
    a.cmp(ir.B_ULT, 8, 2, 0, 1)
    a.p.emit(ir.ASSERT, 1, a=2)
    a.p.emit(ir.ASSERT, 1, a=2)
    a.b(ir.B_OR, 3, a=1, b=2)
    a.p.emit(ir.ASSERT, 1, a=3)
    a.p.emit(ir.ASSERT, 1, a=1)
    return a.done()


def many_sites(n=40):
    """One 256-bit variable, n > 32 sites: byte i of x below a bound that grows with i (sites of
    every holding rate), every fifth one through two B_NOTs (the site is then a bool op)."""
    a = Asm("many-sites", parents=False)
    a.wvar(0, 256, None)
    for i in range(n):
        a.w(ir.W_EXTRACT, 8, 1, 0, aux0=(6 * i) % 248)
        a.wconst(2, 8, 96 + 4 * i)
        a.cmp(ir.B_ULT, 8, i % 8, 1, 2)
        if i % 5 == 4:
            a.b(ir.B_NOT, 8 + i % 8, a=i % 8)
            a.b(ir.B_NOT, 16 + i % 8, a=8 + i % 8)
            a.p.emit(ir.ASSERT, 1, a=16 + i % 8)
        else:
            a.p.emit(ir.ASSERT, 1, a=i % 8)
    return a.done()


def spilled_bool(exp_between=False, base=0):
    """B0 = (x < 160) is asserted, spilled, overwritten, filled into B2 after a second site and
    asserted again through an XOR with a Bool variable.  ``exp_between``: a W_EXP between spill
    and fill keeps the slot in scratch (else it may live in LDS)."""
    a = Asm("spilled-bool" + ("-exp" if exp_between else "") + (f"-b{base}" if base else ""), base=base,
            parents=False)
    a.wvar(0, 8, None)
    a.wconst(1, 8, 160)
    a.cmp(ir.B_ULT, 8, 0, 0, 1)
    a.p.emit(ir.ASSERT, 1, a=0)
    a.b(ir.B_SPILL, 0, a=0, aux0=3)
    a.bvar(0, None)
    a.p.emit(ir.ASSERT, 1, a=0)
    if exp_between:
        a.wconst(2, 256, 3)
        a.w(ir.W_EXP, 256, 3, 2, 2)
        a.assert_eq(256, 3, 27, 4, bd=5)
    a.b(ir.B_FILL, 2, aux0=3)
    a.b(ir.B_XOR, 3, a=2, b=0)
    a.p.emit(ir.ASSERT, 1, a=3)
    return a.done()


def parented():
    """A 256-bit variable with a parent one bit away from the only solutions of its first site;
    candidate 0 (the parent itself) fails that site alone."""
    a = Asm("parented")
    a.wvar(0, 256, X ^ (1 << 9))
    a.w(ir.W_EXTRACT, 16, 1, 0, aux0=0)
    a.assert_eq(16, 1, X & 0xFFFF, 2, bd=0)
    a.w(ir.W_EXTRACT, 8, 3, 0, aux0=248)
    a.assert_eq(8, 3, X >> 248, 2, bd=1)
    return a.done()


def folded_first():
    """Its first assert (7 == 7) folds away in a folded batch; the second does not."""
    a = Asm("folded-first", parents=False)
    a.wconst(0, 256, 7)
    a.assert_eq(256, 0, 7, 1, bd=0)
    a.wvar(2, 8, None)
    a.assert_eq(8, 2, 0x11, 1, bd=1)
    a.wconst(3, 256, 9)
    a.assert_eq(256, 3, 9, 1, bd=2)
    a.wvar(4, 8, None)
    a.wconst(1, 8, 99)
    a.cmp(ir.B_ULT, 8, 3, 4, 1)
    a.p.emit(ir.ASSERT, 1, a=3)
    return a.done()


def small_batch():
    """3 sets: below the fold gate."""
    sets = [two_bounds(), folded_away(), spilled_bool(base=8)]
    for i, p in enumerate(sets):
        p.seed = 11 + i
    return sets


def big_batch():
    """18 sets: folded, with device constants of their own; narrow sets next to 16-register ones."""
    sets = [one_site(), bare_end(), ground(True), ground(False), contra(), two_bounds(), plain_sites(),
            many_sites(), spilled_bool(), spilled_bool(True), parented(), folded_first(),
            folded_away(), one_site(base=8, name="one-site-r16"), two_bounds(base=8, name="two-bounds-r16"),
            spilled_bool(True, base=8), many_sites(33), contra()]
    for i, p in enumerate(sets):
        p.seed = 3 + 7 * i
    return sets
