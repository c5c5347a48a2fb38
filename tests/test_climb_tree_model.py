"""CPU: the model of the climb's tree score (tests/climb_tree_model.py) against the table of
include/pf_bytecode.h, row by row on hand-emitted programs; saturation; witnesses; Bool spills;
and the premise of the pinned family (tests/climb_tree_sets.py): the tree climb witnesses every
set of it and the sites climb none, by the two models alone."""

import random

import pytest

import bool_file_cases as C
import climb_model as CM
import climb_sets as CS
import climb_tree_model as TM
import climb_tree_sets as TS
from mythril_amd import ir

M256 = ir.mask(256)


def dev_of(prog):
    return CM.device_sets(ir.Batch([prog]))[0]


def pair_of(prog, reg, values=None):
    """The (dt, df) last written to B[reg], and the score, under the program's own values."""
    trace = []
    dev = dev_of(prog)
    root, score = TM.tree_run(dev, prog.assignment if values is None else values, trace)
    pairs = [p for (_, r, _, p) in trace if r == reg]
    assert pairs, f"B{reg} is never written"
    return pairs[-1], root, score, dev


# (op, width, a, b) -> (dt, df): every compare row, holding and failing, the bitlen edges
_NEG1_64, _MIN_64 = ir.mask(64), 1 << 63
COMPARE_ROWS = [
    (ir.B_EQ, 256, 0b1011, 0b0001, (2, 0)),
    (ir.B_EQ, 256, TS.K1, TS.K1, (0, 1)),
    (ir.B_EQ, 256, 0, M256, (256, 0)),
    (ir.B_ULT, 256, 11, 1, (4, 0)),
    (ir.B_ULT, 256, 1, 11, (0, 4)),
    (ir.B_ULT, 256, 7, 7, (1, 0)),                       # D = 0: max(1, D)
    (ir.B_ULT, 256, M256, 0, (256, 0)),
    (ir.B_ULT, 256, 0, M256, (0, 256)),
    (ir.B_ULE, 256, 7, 7, (0, 1)),
    (ir.B_ULE, 256, 1 << 200, 0, (201, 0)),
    (ir.B_ULE, 256, 0, 1 << 200, (0, 201)),
    (ir.B_SLT, 256, M256, 0, (0, 1)),                    # -1 < 0: one apart
    (ir.B_SLT, 256, 0, M256, (1, 0)),
    (ir.B_SLT, 256, 5, 5, (1, 0)),
    (ir.B_SLT, 64, _NEG1_64, 0, (0, 1)),                 # at width 64 the register holds 2^64 - 1
    (ir.B_SLT, 64, 0, _NEG1_64, (1, 0)),
    (ir.B_SLT, 64, _MIN_64 - 1, _MIN_64, (64, 0)),       # max against min: 2^64 - 1 apart
    (ir.B_SLE, 64, _MIN_64, _MIN_64 - 1, (0, 64)),
    (ir.B_SLE, 256, 9, 9, (0, 1)),
    (ir.B_SLE, 256, 1 << 254, (1 << 255) | 1, (256, 0)),
    (ir.B_UADD_NOOVF, 256, M256, 1, (256, 0)),
    (ir.B_UADD_NOOVF, 256, 1, 1, (0, 256)),
    (ir.B_UMUL_NOOVF, 64, 1 << 40, 1 << 40, (256, 0)),
    (ir.B_UMUL_NOOVF, 64, 3, 4, (0, 256)),
]


@pytest.mark.parametrize("op,w,a,b,want", COMPARE_ROWS,
                         ids=[f"{ir.OPNAMES[r[0]]}/w{r[1]}/{i}" for i, r in enumerate(COMPARE_ROWS)])
def test_compare_rows(op, w, a, b, want):
    for fused, bd in ((True, 0), (False, 31), (True, 31)):
        prog = TS.compare_row(op, w, a, b, bd=bd, fused=fused)
        pair, root, score, dev = pair_of(prog, bd)
        assert pair == want and root == (want[0] == 0) and dev.sites == 1
        assert score == (512 if want[0] == 0 else 256 - want[0])
        # the site is the compare itself (B_UMUL_NOOVF is never fused: a plain ASSERT) or the
        # second B_NOT above it: it adds the same either way
        sites = [w0 & 0xFF for (w0, _, _, _) in dev.code if w0 & CM.I_ASSERT or (w0 & 0xFF) == ir.ASSERT]
        assert sites == [ir.B_NOT if not fused else ir.ASSERT if op == ir.B_UMUL_NOOVF else op]


# x = EQ(v0, v1), y = ULT(v2, v3), c = Bool; (values) -> pairs of x, y, c
X_F3, X_T = (0b111, 0, (3, 0)), (6, 6, (0, 1))
Y_T5, Y_F9 = (0, 16, (0, 5)), (256, 0, (9, 0))
C_T, C_F = (1, (0, 1)), (0, (1, 0))
LOGIC_ROWS = [
    (ir.B_AND, X_F3, Y_T5, C_T, (3, 0)),
    (ir.B_AND, X_F3, Y_F9, C_T, (12, 0)),
    (ir.B_AND, X_T, Y_T5, C_T, (0, 1)),
    (ir.B_OR, X_F3, Y_T5, C_T, (0, 5)),
    (ir.B_OR, X_F3, Y_F9, C_T, (3, 0)),
    (ir.B_OR, X_T, Y_T5, C_T, (0, 6)),
    (ir.B_XOR, X_F3, Y_T5, C_T, (0, 3)),
    (ir.B_XOR, X_F3, Y_F9, C_T, (3, 0)),
    (ir.B_XOR, X_T, Y_T5, C_T, (1, 0)),
    (ir.B_NOT, X_F3, Y_T5, C_T, (0, 3)),
    (ir.B_NOT, X_T, Y_T5, C_T, (1, 0)),
    (ir.B_ITE, X_F3, Y_T5, C_T, (1, 0)),     # c ? x : y — flipping c costs 1 and gives y
    (ir.B_ITE, X_F3, Y_T5, C_F, (0, 1)),
    (ir.B_ITE, X_F3, Y_F9, C_T, (3, 0)),
    (ir.B_ITE, X_T, Y_F9, C_F, (1, 0)),
    (ir.B_ITE, X_T, Y_T5, C_T, (0, 1)),
]


@pytest.mark.parametrize("op,x,y,c,want", LOGIC_ROWS,
                         ids=[f"{ir.OPNAMES[r[0]]}/{i}" for i, r in enumerate(LOGIC_ROWS)])
def test_logic_rows(op, x, y, c, want):
    values = (x[0], x[1], y[0], y[1], c[0])
    for regs in ((3, 0, 31, 7), (31, 0, 1, 2), (0, 0, 31, 30), (31, 30, 31, 0)):
        prog = TS.logic_row(op, values, regs)
        d, ra, rb, rc = regs
        trace = []
        dev = dev_of(prog)
        root, score = TM.tree_run(dev, prog.assignment, trace)
        first = {}
        for (_, r, _, p) in trace:
            first.setdefault(r, p)
        assert (first[ra], first[rb], first[rc]) == (x[2], y[2], c[1])
        assert trace[-1][1] == d and trace[-1][3] == want, regs
        assert score == (512 if want[0] == 0 else 256 - want[0]) and root == (want[0] == 0)


def test_constants_and_bool_variables():
    for bit in (0, 1):
        s = TS.Asm(f"const{bit}")
        s.b(ir.B_CONST, 4, aux0=bit)
        s.bvar(9, bit)
        s.p.emit(ir.ASSERT, 1, a=4)
        s.p.emit(ir.ASSERT, 1, a=9)
        prog = s.done(None)
        (pc, _, score, _), (pv, _, _, _) = pair_of(prog, 4), pair_of(prog, 9)
        assert pc == ((0, 256) if bit else (256, 0)) and pv == ((0, 1) if bit else (1, 0))
        assert score == (1024 if bit else 0 + 255)


def test_saturation():
    """Three compares failing with D > 128 each: their AND is 256 from true and its site adds 0;
    their OR takes the smallest."""
    values = [1 << 200, 1 << 130, 1 << 255]
    pair, _, score, _ = pair_of(TS.saturation_set(ir.B_AND, values), 4)
    assert pair == (256, 0) and score == 0
    pair, _, score, _ = pair_of(TS.saturation_set(ir.B_OR, values), 4)
    assert pair == (130, 0) and score == 256 - 130        # bitlen(2^130 - 5)
    # holding, the sums saturate on the other side
    values = [0, 1, 2]
    assert pair_of(TS.saturation_set(ir.B_AND, values), 4)[0] == (0, 2)
    assert pair_of(TS.saturation_set(ir.B_OR, values), 4)[0] == (0, 3 + 3 + 2)
    s = TS.Asm("sat-or-holds")
    for i in range(3):
        s.wvar(i, 256, 0)
        s.wconst(3, 256, M256 >> i)
        s.cmp(ir.B_ULT, 256, i, i, 3)
    s.b(ir.B_OR, 3, a=0, b=1)
    s.b(ir.B_OR, 4, a=3, b=2)
    s.p.emit(ir.ASSERT, 1, a=4)
    assert pair_of(s.done(None), 4)[0] == (0, 256)


def test_not_not_is_the_identity():
    rng = random.Random(5)
    dev = dev_of(TS.table_sets()[1])
    for _ in range(50):
        trace = []
        TM.tree_run(dev, [rng.getrandbits(256), rng.getrandbits(256), rng.getrandbits(64), rng.getrandbits(64),
                          rng.getrandbits(1), rng.getrandbits(1)], trace)
        writes0 = [p for (_, r, _, p) in trace if r == 0]
        assert len(writes0) == 2 and writes0[0] == writes0[1]       # B_EQ, then NOT NOT of it


def _eight_programs():
    progs = CS.near_sets() + TS.family()[:3]
    assert len(progs) == 8
    return progs


def test_a_witness_scores_512_x_sites_and_nothing_else_does():
    rng = random.Random(2024)
    progs = _eight_programs()
    devs = CM.device_sets(ir.Batch(progs))
    n_holds = 0
    for prog, dev in zip(progs, devs):
        widths = [v.width for v in prog.vars]
        sols = [[f[i] for i in range(3)] for f in getattr(prog, "solution", [])]
        sols += [[CS.X] * len(widths)] if prog.name.startswith("bytes3") else []
        for k in range(250):
            if k < 8 and sols:
                values = list(sols[k % len(sols)])
                if k >= len(sols):                                # a solution with one bit flipped
                    values[k % len(values)] ^= 1 << rng.randrange(6)
            else:
                values = [rng.getrandbits(w) if k % 3 else rng.getrandbits(min(w, 6)) for w in widths]
            root, score = TM.tree_run(dev, values)
            sroot, _ = dev.run(values)
            assert root == sroot
            assert (score == dev.target) == root, (prog.name, values)
            assert score <= dev.target
            n_holds += root
    assert n_holds >= 8


def test_a_failing_fused_eq_adds_what_the_sites_score_adds():
    rng = random.Random(7)
    for w in (8, 64, 256):
        for _ in range(40):
            a, b = rng.getrandbits(w), rng.getrandbits(w)
            if rng.getrandbits(1):
                b = a ^ (1 << rng.randrange(w))
            dev = dev_of(TS.compare_row(ir.B_EQ, w, a, b))
            assert TM.tree_score(dev, [a, b]) == dev.score([a, b]) == 256 - bin(a ^ b).count("1")
    # the order compares: the same but for a strict compare of equal operands
    for op in (ir.B_ULT, ir.B_ULE):
        for a, b in ((5, 3), (1 << 255, 0), (9, 9), (0, 7)):
            dev = dev_of(TS.compare_row(op, 256, a, b))
            t, s = TM.tree_score(dev, [a, b]), dev.score([a, b])
            assert t == (255 if (op == ir.B_ULT and a == b) else s)
    dev = dev_of(TS.compare_row(ir.B_ULT, 256, 9, 9))
    assert (TM.tree_score(dev, [9, 9]), dev.score([9, 9])) == (255, 256)


def test_sites_mode_of_the_round_loop_is_the_sites_model():
    progs = CS.near_sets()[:3] + [CS.flat(), CS.kinds()]
    batch = ir.Batch(progs)
    ids = list(range(len(progs)))
    assert TM.climb(batch, ids, 5, 128, 9, "sites") == CM.climb(batch, ids, 5, 128, 9)
    with pytest.raises(ValueError):
        TM.climb(batch, [0], 1, 8, 0, "bogus")


def check_spills(dev, values):
    """Every B_FILL writes exactly the pair its slot's B_SPILL read; -> (the pairs filled, the
    slots' aux words)."""
    trace = []
    root, score = TM.tree_run(dev, values, trace)
    assert root == dev.run(values)[0] and (score == dev.target) == root
    by_pc = {pc: p for (pc, _, _, p) in trace}
    live, stored, filled = {}, {}, []
    for pc, (w0, w1, aux0, _) in enumerate(dev.code):
        op = w0 & 0xFF
        if pc in by_pc:
            live[w1 & 31] = by_pc[pc]
        if op == ir.B_SPILL:
            stored[aux0] = live[(w1 >> 8) & 31]
        elif op == ir.B_FILL:
            assert by_pc[pc] == stored[aux0]
            filled.append(by_pc[pc])
    return filled, list(stored)


@pytest.mark.parametrize("name", ["p40/free/narrow", "p64x/free/r16"])
def test_bool_spills_keep_their_pair_in_the_pressure_dags(name):
    """More than 32 live Bools through lower(): compares' pairs (not just 0 / 1) go through the
    slots."""
    _, prog, cands = C.pressure_explicit(name, 6)
    dev = dev_of(prog)
    wide = 0
    for values in cands:
        filled, slots = check_spills(dev, values)
        assert filled and slots
        wide += sum(max(p) > 1 for p in filled)
    assert wide


def test_bool_spills_keep_their_pair_in_the_hand_emitted_sets():
    """Scratch slots 0 and 63, LDS entries, a W_EXP or a B_UMUL_NOOVF between spill and fill."""
    aux = set()
    for variant in C.SPILL_VARIANTS:
        for rot in (0, 1, 3):
            prog = C.bspill_set(variant, 0x5A5AC33C ^ rot, rot=rot)
            filled, slots = check_spills(dev_of(prog), prog.assignment)
            assert len(filled) == len(C.SPILL_REGS) and set(filled) <= {(0, 1), (1, 0)}     # Bool variables
            aux |= set(slots)
    assert {0, 63} <= aux and any(a & 0x100 for a in aux)


def test_the_family_is_witnessed_by_the_tree_climb_and_left_by_the_sites_climb():
    progs = TS.family()
    assert {p.name.split(":")[1].split("/")[0] for p in progs} == set(TS.SHAPES)
    batch = ir.Batch(progs)
    ids = list(range(len(progs)))
    devs = CM.device_sets(batch)
    assert TS.ROUNDS <= 8 and TS.PER_ROUND <= 256
    tree = TM.climb(batch, ids, TS.ROUNDS, TS.PER_ROUND, TS.SEED, "tree", devs)
    sites = TM.climb(batch, ids, TS.ROUNDS, TS.PER_ROUND, TS.SEED, "sites", devs)
    for p, t, s in zip(progs, tree, sites):
        assert t.status == ir.CLIMB_WITNESS and t.round >= 1, p.name      # not round 0's luck
        assert tuple(t.values) in [tuple(f) for f in p.solution]
        assert s.status == ir.CLIMB_NONE and s.score == 0, p.name         # flat: a Bool-op site
    # 256-bit constants
    assert all(max(d.consts).bit_length() > 200 for d in devs)
