"""Test tooling (not a test): hand-made link groups, shared by the CPU checks of the link model
(test_link_cases.py) and the device comparison (test_gpu_linked.py).

A group is built from a list of roots — small self-contained pieces of code that end in an
ASSERT — over one fixed schema and one fixed constant pool.  ``unsplit`` runs every root in one
program; the members run disjoint subsets of them and carry the same variables, constants and
seed, as lower_parts makes them.  Programs have at most about 100 instructions.

``target`` groups have their smallest witness at a chosen candidate: the K members each pin 32
bits of a 256-bit variable to what the generator draws for it at that candidate.  The pool has to
hold those 32-bit pieces and the generator may draw from the pool, so the pieces are found by
iterating to a fixed point; test_link_cases.py asserts on the CPU model that every target group's
verdict is the candidate it was built for."""

import numpy as np

import pyoracle as O
from mythril_amd import ir
from op_programs import Asm

GSEED = 0x4C494E4B            # the global seed of every call of these tests
BUDGETS = (1, 63, 64, 65, 197, 4096)
TARGETS = (0, 62, 63, 64, 196, 4095, 4096)   # every budget's last candidate, and one past the largest
KS = (1, 2, 3, 7)
P16 = 0xBEEF

# the schema of every group: (width, parent value or None, kind)
SCHEMA = ((256, None, ir.VK_GENERIC), (8, None, ir.VK_GENERIC), (16, P16, ir.VK_GENERIC), (1, None, ir.VK_BOOL))
W, S, P, B = 0, 1, 2, 3


class Group:
    def __init__(self, name, unsplit, members):
        self.name, self.unsplit, self.members = name, unsplit, members


def _asm(name, base, seed, consts, parents=True):
    a = Asm(name, base=base)
    for width, parent, kind in SCHEMA:
        a.var(width, parent if parents else None, kind)
    a.p.consts = list(consts)
    a.p.seed = seed
    return a


def _done(a, n_const):
    p = a.done()
    assert len(p.consts) == n_const, f"{p.name}: a root added a constant to the fixed pool"
    return p


# ---- roots: f(a) emits code on Asm a, W registers 0..5 (+ base), B registers 0..3 --------------
def piece_eq(i, value):
    """bits [32 i, 32 i + 32) of w == value"""
    def f(a):
        a.p.emit(ir.W_VAR, 256, dst=a.base, aux0=W)
        a.w(ir.W_EXTRACT, 32, 1, 0, aux0=32 * i)
        a.assert_eq(32, 1, value, 2)
    return f


def s_below(bound):
    def f(a):
        a.p.emit(ir.W_VAR, 8, dst=a.base, aux0=S)
        a.wconst(1, 8, bound)
        a.cmp(ir.B_ULT, 8, 0, 0, 1)
        a.p.emit(ir.ASSERT, 1, a=0)
    return f


def s_from(bound):
    def f(a):
        a.p.emit(ir.W_VAR, 8, dst=a.base, aux0=S)
        a.wconst(1, 8, bound)
        a.cmp(ir.B_ULE, 8, 1, 1, 0)
        a.p.emit(ir.ASSERT, 1, a=1)
    return f


def s_bit(k, want):
    """bit k of s == want, through a plain ASSERT of a NOT where want is 0"""
    def f(a):
        a.p.emit(ir.W_VAR, 8, dst=a.base, aux0=S)
        a.w(ir.W_EXTRACT, 1, 1, 0, aux0=k)
        a.wconst(2, 1, 1)
        a.cmp(ir.B_EQ, 1, 2, 1, 2)
        a.assert_(2, bool(want))
    return f


def b_is(want):
    def f(a):
        a.p.emit(ir.B_VAR, 1, dst=3, aux0=B)
        a.assert_(3, bool(want))
    return f


def p_is_parent():
    """p == its parent value: candidate 0 and most odd candidates"""
    def f(a):
        a.p.emit(ir.W_VAR, 16, dst=a.base, aux0=P)
        a.assert_eq(16, 0, P16, 1)
    return f


def mul_low(value):
    """(s * s + s) mod 256 < value: a few more instructions, a product"""
    def f(a):
        a.p.emit(ir.W_VAR, 8, dst=a.base, aux0=S)
        a.w(ir.W_MUL, 8, 1, 0, 0)
        a.w(ir.W_ADD, 8, 2, 1, 0)
        a.wconst(3, 8, value)
        a.cmp(ir.B_ULT, 8, 0, 2, 3)
        a.p.emit(ir.ASSERT, 1, a=0)
    return f


def folds_away():
    """s ^ s == 0: the fold pass proves it, a folded batch runs a bare END for a member of it"""
    def f(a):
        a.p.emit(ir.W_VAR, 8, dst=a.base, aux0=S)
        a.w(ir.W_XOR, 8, 1, 0, 0)
        a.assert_eq(8, 1, 0, 2)
    return f


def nowhere():
    """s == 5 and s == 6"""
    def f(a):
        a.p.emit(ir.W_VAR, 8, dst=a.base, aux0=S)
        a.assert_eq(8, 0, 5, 1, bd=0)
        a.assert_eq(8, 0, 6, 1, bd=1)
    return f


POOL = (0, 1, 5, 6, 50, 64, 128, 200, 240, P16)


def make_group(name, roots, split, seed, pool=POOL, wide=(), parents=True):
    """``split``: per member the indices of its roots (a partition of range(len(roots)), or with
    an empty list for a member that is a bare END); ``wide``: the members lowered over W registers
    8.. (the 16-register kernels)."""
    assert sorted(i for m in split for i in m) == list(range(len(roots))), name
    a = _asm(name + "/unsplit", 0, seed, pool, parents)
    for f in roots:
        f(a)
    unsplit = _done(a, len(pool))
    members = []
    for k, idx in enumerate(split):
        a = _asm(f"{name}/{k}of{len(split)}", 8 if k in wide else 0, seed, pool, parents)
        for i in idx:
            roots[i](a)
        members.append(_done(a, len(pool)))
    return Group(name, unsplit, members)


def _w_at(cand, seed, pool):
    """The generator's value of w at candidate ``cand`` for a group with this seed and pool."""
    a = _asm("probe", 0, seed, pool)
    b = ir.Batch([a.done()])
    vals = O.SetView.from_batch(b, 0).gen_assignments(np.array([cand], dtype=np.uint64), GSEED)[0]
    return int(vals[W])


def target_group(cand, k, seed, wide=()):
    """K members pinning pieces 0 .. 6 of w to its value at ``cand`` (7 roots dealt round robin),
    so ``cand`` is a witness; the pool holds the pieces."""
    for seed in range(seed, seed + 0x400000, 0x10000):   # a seed at which w is not drawn from the pool
        pieces = [0x1000 + i for i in range(7)]
        for _ in range(3):
            pool = POOL + tuple(pieces)
            w = _w_at(cand, seed, pool)
            new = [(w >> (32 * i)) & 0xFFFFFFFF for i in range(7)]
            if new == pieces:
                break
            pieces = new
        if new == pieces and all(8 <= bin(x).count("1") <= 24 for x in pieces):   # no boundary value
            break
    else:
        raise AssertionError(f"target {cand} seed {seed}: the pieces do not settle")
    roots = [piece_eq(i, pieces[i]) for i in range(7)]
    split = [[i for i in range(7) if i % k == m] for m in range(k)]
    return make_group(f"target{cand}/k{k}", roots, split, seed, pool, wide)


def band_group(i):
    """Members that each hold at many candidates and together at few: bands of s, bits of s, the
    Bool, the parented variable; K and the register files vary with i."""
    roots = [s_below(200 - 8 * (i % 5)), s_from(50 + 3 * (i % 7)), s_bit(i % 6, i & 1), b_is(i % 3 == 0),
             mul_low(240 - 16 * (i % 4)), s_bit((i + 3) % 6, (i >> 1) & 1), p_is_parent() if i % 4 == 0 else s_below(240)]
    k = (2, 3, 7, 2, 4)[i % 5]
    split = [[r for r in range(7) if r % k == m] for m in range(k)]
    pool = POOL + (192, 184, 176, 168, 53, 56, 59, 62, 65, 68, 224, 208)
    return make_group(f"band{i}", roots, split, 0x600 + i, pool, wide={m for m in range(k) if (m + i) % 3 == 0})


def special_groups():
    out = []
    # a member that holds nowhere, next to members that hold often
    out.append(make_group("nowhere", [s_below(200), nowhere(), b_is(True)], [[0], [1], [2]], 0x701))
    # a member with no root at all: a bare END as lowered
    out.append(make_group("bare", [s_below(128), s_bit(0, 1)], [[0], [], [1]], 0x702))
    # a member the fold pass reduces to a bare END (batches of 16 sets or more are folded)
    out.append(make_group("folded", [s_from(64), folds_away(), s_bit(1, 0)], [[0], [1], [2]], 0x703))
    # every member a bare END: every candidate is a witness
    out.append(make_group("all-bare", [], [[], []], 0x704))
    # the two register files in one group, either way round
    out.append(make_group("wide-first", [s_below(200), s_from(50), s_bit(2, 1)], [[0], [1], [2]], 0x705, wide={0}))
    out.append(make_group("wide-last", [s_below(200), s_from(50), s_bit(2, 1)], [[0, 1], [2]], 0x706, wide={1}))
    out.append(make_group("all-wide", [s_below(200), s_from(50)], [[0], [1]], 0x707, wide={0, 1}))
    return out


def target_groups():
    out = []
    for k in KS:
        for t in TARGETS:
            out.append(target_group(t, k, 0x100 * k + 0x11 + TARGETS.index(t), wide={1} if k == 3 else ()))
    return out


class Layout:
    """Groups laid out as one batch: every group's unsplit program (a group of one) and its
    members, the sets dealt out so that the members of a group are not adjacent."""

    def __init__(self, groups, interleave=True):
        self.groups = groups
        entries = []                      # (program, group id)
        self.unsplit_gid, self.parts_gid = [], []
        gid = 0
        for g in groups:
            self.unsplit_gid.append(gid)
            entries.append((g.unsplit, gid))
            gid += 1
            self.parts_gid.append(gid)
            entries += [(m, gid) for m in g.members]
            gid += 1
        if interleave:
            n = len(entries)
            stride = next(s for s in range(max(2, n // 3), n + 2) if np.gcd(s, n) == 1)
            entries = [entries[(i * stride) % n] for i in range(n)]
        self.programs = [p for p, _ in entries]
        self.group_of = [g for _, g in entries]
        self.n_groups = gid
        self.unsplit_set = [self.programs.index(g.unsplit) for g in groups]

    def sets_of(self, gid):
        return [s for s, g in enumerate(self.group_of) if g == gid]


def big_layout():
    """72 groups of K = 1, 2, 3, 4 and 7 (36 hand-made groups and their unsplit programs)."""
    return Layout(target_groups() + special_groups() + [band_group(0)])


def bands_layout():
    """64 link groups of mixed K: 32 band groups and their unsplit programs."""
    return Layout([band_group(i) for i in range(32)])


def small_layout():
    """Below the fold gate and small enough for the probe launch (2 .. 64 sets, every set with a
    parent model): two groups whose members keep their programs as lowered."""
    return Layout([make_group("small-a", [p_is_parent(), s_below(200), folds_away()], [[0], [1], [2]], 0x801),
                   make_group("small-b", [s_from(50), mul_low(200), b_is(True)], [[0, 1], [2]], 0x802, wide={1})],
                  interleave=False)
