"""CPU: the width catalogue of tests/width_cases.py — its own conditions, its expectations
against oracle/pyoracle.py, and its programs against the oracle's evaluator, the C oracle and
the device programs pf_batch_create would upload (fold on, off and alone), at every width
1..256 of every key.

The conditions and the expectations are checked on all rows.  The program legs take, per key
and width, the row and the twin at position w mod 8 of the 8-row list (every key, every width,
every position), as one batch through pf_device_batch: far past the fold gate of 16 sets."""

import functools
import types

import coracle_py
import numpy as np
import pyoracle as O
import pytest
import width_cases as C
from test_device_program import eval_device

from mythril_amd import _lib, ir

_OFN = {"add": O.bvadd, "sub": O.bvsub, "mul": O.bvmul, "udiv": O.bvudiv, "urem": O.bvurem, "sdiv": O.bvsdiv,
        "srem": O.bvsrem, "smod": O.bvsmod, "and": lambda a, b, w: a & b, "or": lambda a, b, w: a | b,
        "xor": lambda a, b, w: a ^ b, "shl": O.bvshl, "lshr": O.bvlshr, "ashr": O.bvashr, "exp": O.bvexp,
        "eq": lambda a, b, w: a == b, "ult": O.ult, "ule": O.ule, "slt": O.slt, "sle": O.sle,
        "uadd_noovf": O.uadd_noovf, "umul_noovf": O.umul_noovf}


def _oracle(key, w, args):
    s = C.spec(key, w)
    if key in _OFN:
        return _OFN[key](*args, w)
    if key == "not":
        return O.bvnot(args[0], w)
    if key == "neg":
        return O.bvneg(args[0], w)
    if key in ("mov", "mov_narrow"):
        return args[0] & O.M(w)
    if key == "ite":
        return args[1] if args[0] else args[2]
    if key in C.HASHES:
        return O.uf_hash(args[0], s.aux0) & O.M(w)
    if key in C.SEXTS:
        return O.sign_extend(args[0], s.wa, w)
    if key in C.EXTRACTS:
        return O.extract(args[0], s.aux0, w)
    return O.concat(args[0], args[1], s.wb)


def test_the_catalogue_names_every_op_and_width():
    assert len(C.KEYS) == len(set(C.KEYS)) == 15 + 3 + 2 + 3 + 7 + 4 + 5 + 3
    for key in C.KEYS:
        ws = C.widths_of(key)
        if key in C.CONCATS or key == "sext:w-1":
            assert ws == C.WIDTHS[1:], key
        elif key == "mov_narrow":
            assert ws == C.WIDTHS[:-1], key
        elif key in ("extract:1", "extract:31", "extract:32"):
            assert ws == tuple(range(1, 257 - C.spec(key, 1).aux0)), key
        else:
            assert ws == C.WIDTHS, key
        for w in ws:
            assert len(C.rows(key, w, 8)) == 8 and len(C.rows(key, w, 40)) == 40
            assert C.rows(key, w, 40)[:8] == C.rows(key, w, 8)
    assert C.rows("add", 77) is C.rows("add", 77)          # drawn once, shared


@pytest.mark.parametrize("key", C.KEYS)
def test_expectations_are_the_oracles(key):
    n = 0
    for w in C.widths_of(key):
        s = C.spec(key, w)
        for r in C.rows(key, w, 40):
            ops = r.args[1:] if key == "ite" else r.args
            assert 0 <= ops[0] < 1 << s.wa and (len(ops) < 2 or 0 <= ops[1] < 1 << s.wb), (key, w, r)
            want = _oracle(key, w, r.args)
            assert r.expect == want and type(r.expect) is type(want), (key, w, r, want)
            n += 1
    assert n == 40 * len(C.widths_of(key))


def test_conditions_on_the_rows():
    """What the catalogue promises, on the 8-row lists of every width."""
    for w in C.WIDTHS:
        m, top = C.M(w), 1 << (w - 1)
        neg = lambda x: bool(x >> (w - 1))
        for key in C.SIGNED:
            pairs = [r.args for r in C.rows(key, w, 8)]
            if w >= 2:
                assert {(neg(a), neg(b)) for a, b in pairs if b} == {(False, False), (False, True), (True, False),
                                                                      (True, True)}, (key, w)
            assert any(b == 0 for _, b in pairs) and (top, m) in pairs, (key, w)
        for key in ("slt", "sle"):
            pairs = [r.args for r in C.rows(key, w, 8)]
            assert len({(neg(a), neg(b)) for a, b in pairs}) == 4, (key, w)
        for key in C.SHIFTS:
            amts = {r.args[1] for r in C.rows(key, w, 8)}
            assert amts >= {v & m for v in (0, 1, w - 1, w, w + 1)}, (key, w)
            assert w <= 32 or any(b >> 32 for b in amts), (key, w)
            if key == "ashr":      # the sign bit set under an amount below, at and above w
                assert any(neg(r.args[0]) for r in C.rows(key, w, 8)), w
        ex = [r.args for r in C.rows("exp", w, 8)]
        assert {a & 1 for a, _ in ex} == {0, 1} and {b for _, b in ex} >= {0, 1 & m, 2 & m, m}, w
        for key in C.CMP:
            verdicts = {r.expect for r in C.rows(key, w, 8)}
            both = not (key == "umul_noovf" and w == 1)      # 1 * 1 fits in one bit
            assert verdicts == ({False, True} if both else {True}), (key, w)
        for key in C.SEXTS:
            if C.spec(key, w) is not None:
                ws = C.spec(key, w).wa
                assert {r.args[0] >> (ws - 1) for r in C.rows(key, w, 8)} == {0, 1}, (key, w)
        for key in C.KEYS:
            for n in (8, 40):
                rs = C.rows(key, w, n)
                if not rs:
                    continue
                ew = 1 if key in C.CMP else w
                for r in rs:
                    diff = int(C.corrupted(r)) ^ int(r.expect)
                    assert diff == 1 << r.bit and r.bit < ew, (key, w, r)
                assert 4 * sum(r.bit == ew - 1 for r in rs) >= len(rs), (key, w, n)


def test_near_rows_cover_the_distances():
    for key in C.NEAR_KEYS:
        for w in C.WIDTHS:
            near = C.near_rows(key, w)
            assert all(not C.expectation(key, w, (a, b)) and abs(a - b).bit_length() == d for a, b, d in near)
            want = {1, (w + 1) // 2, w} | ({0} if key in ("ult", "slt") else set())
            assert {d for _, _, d in near} == want, (key, w)
            if key in ("slt", "sle") and w >= 2:
                assert any((a >> (w - 1)) != (b >> (w - 1)) for a, b, _ in near), (key, w)


# ---- the programs -----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sample():
    """Per key and width the row at position w mod 8, held and corrupted, variable operands;
    for the ground keys the same row with constant operands too."""
    progs = []
    for key in C.KEYS:
        for w in C.widths_of(key):
            r = C.rows(key, w, 8)[w % 8]
            for twin in (False, True):
                progs.append(C.search_set(r, base=8 * (w & 1), twin=twin))
            if key in C.GROUND_KEYS:
                for twin in (False, True):
                    progs.append(C.ground_set(r, base=8 * (w & 1), twin=twin))
    return progs, ir.Batch(progs)


def test_the_sample_holds_every_key_width_and_row_position():
    progs, _ = _sample()
    seen = {(p.row.key, p.row.w) for p in progs}
    assert seen == {(k, w) for k in C.KEYS for w in C.widths_of(k)}
    assert {C.rows(p.row.key, p.row.w, 8).index(p.row) for p in progs} == set(range(8))
    assert {p.row.w for p in progs if p.name.startswith("ground")} == set(C.WIDTHS)
    assert len(progs) > 16


@pytest.mark.parametrize("key", C.KEYS)
def test_the_oracles_give_every_programs_verdict(key):
    """All 8 rows and twins of every width, as the search legs upload them (and the rows with
    constant operands): the Python oracle on the assignment, the C oracle on candidate 0."""
    progs = []
    for w in C.widths_of(key):
        for i, r in enumerate(C.rows(key, w, C.N_SEARCH)):
            progs += [C.search_set(r, 8 * (w & 1)), C.search_set(r, 8 * (w & 1), twin=True)]
            if key in C.GROUND_KEYS and i == w % 8:          # the row the GPU's constant leg takes
                progs += [C.ground_set(r), C.ground_set(r, twin=True)]
    assert len(progs) == (18 if key in C.GROUND_KEYS else 16) * len(C.widths_of(key))
    batch = ir.Batch(progs)
    packed = coracle_py.Packed(batch)
    for s, p in enumerate(progs):
        assert O.SetView.from_batch(batch, s).evaluate(p.assignment) is p.verdict, C.describe(p)
        assert (packed.first_sat(s, 0x5EED, 1) == 0) is p.verdict, C.describe(p)


@pytest.mark.parametrize("fold", ["default", "0", "2"])
def test_device_programs_give_every_programs_verdict(monkeypatch, fold):
    """The whole sample as one batch through pf_device_batch: every set's device program, read
    against the device pool, gives the verdict — with the fold pass on, off and alone."""
    if fold != "default":
        monkeypatch.setenv("PF_DEVICE_FOLD", fold)
    progs, batch = _sample()
    code, descs, pool = _lib.device_batch(batch.code, batch.consts, batch.descs)
    consts = [O.limbs_to_int(r) for r in pool]
    for s, p in enumerate(progs):
        d = [int(x) for x in descs[s]]
        rows = [tuple(int(x) for x in r) for r in code[d[0]:d[0] + d[1]]]
        view = types.SimpleNamespace(consts=consts[d[2]:])
        assert eval_device(view, rows, p.assignment) is p.verdict, (fold, C.describe(p), rows)
    if fold == "default":      # constant operands are evaluated on the host past the gate
        ground = [s for s, p in enumerate(progs) if p.name.startswith("ground:W_")]
        kept = sum(int(descs[s][1]) for s in ground)
        assert kept < sum(int(batch.descs[s][1]) for s in ground)


def test_explicit_sets_hold_exactly_their_rows():
    """One program per (key, width, base); 80 candidates, held and corrupted interleaved."""
    for key in C.KEYS:
        for w in C.widths_of(key):
            p = C.explicit_set(key, w, base=8 * (w & 1))
            cands, want = C.explicit_candidates(key, w)
            assert len(cands) == 80 and want == [True, False] * 40
            # all 80 at every eighth width of the key (and 1, 2, 256), the first 16 at the others
            n = 80 if w % 8 == C.KEYS.index(key) % 8 or w in (1, 2, 256) else 16
            sv = O.SetView.from_batch(ir.Batch([p]), 0)
            got = [sv.evaluate(c) for c in cands[:n]]
            assert got == want[:n], (key, w, [i for i in range(n) if got[i] != want[i]][:4])
    regs = {(i.op, i.dst) for key in C.KEYS for w in (7, 8) if C.spec(key, w) for i in C.explicit_set(key, w).code}
    assert {d for op, d in regs if op == ir.W_VAR} >= {5, 6}


# ---- the generator ----------------------------------------------------------------------------

@pytest.mark.parametrize("layout", C.GEN_LAYOUTS)
def test_generator_set_values_vary(layout):
    p = C.generator_set(layout, seed=0x51ED)
    assert [(v.width, v.kind) for v in p.vars] == [(w, k) for w in C.WIDTHS for k in (ir.VK_GENERIC, ir.VK_VALUE)]
    assert bool(p.consts) == layout.startswith("consts")
    assert any(v.parent is not None for v in p.vars) == layout.endswith("alternate")
    batch = ir.Batch([p])
    _lib.device_batch(batch.code, batch.consts, batch.descs)       # the host accepts 512 variables
    vals = O.SetView.from_batch(batch, 0).gen_assignments(np.array(C.GEN_CANDS, dtype=np.uint64), C.GEN_SEEDS[0])
    assert len(vals) == 260
    for v, var in enumerate(p.vars):
        col = {a[v] for a in vals}
        assert all(x >> var.width == 0 for x in col) and len(col) > 1, (v, var.width)


def test_every_pin_set_has_a_witness_within_the_budget():
    progs = [C.width_pin_set_at(w, base=8 * (w & 1)) for w in C.WIDTHS]
    assert {p.cand for p in progs} == set(C.PIN_CANDS)
    packed = coracle_py.Packed(ir.Batch(progs))
    for s, p in enumerate(progs):
        first = packed.first_sat(s, C.PIN_SEED, C.PIN_BUDGET)
        assert first is not None and first <= p.cand < C.PIN_BUDGET, (p.name, first)
