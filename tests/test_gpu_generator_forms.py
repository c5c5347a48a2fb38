"""GPU: the candidate generator's forms and the 256-bit selects against the oracle, bit-exact.

The generator (pf_eval.hip gen_var) runs its Philox blocks interleaved, in a three-block form
for w > 128 and a two-block form below, and merges its strategy arms with lane masks; sel256
(u256.h) selects per limb by a lane mask, whichever instruction that is.  Three copies of the
generator exist: the materialise kernel's, the search kernels' (8- and 16-register) and the
climb kernels'.

* materialise: every variable kind, the widths around the w > 128 branch and the top-limb
  masks, 0 / 1 / 3 constants, with and without parents, candidates around the group edges,
  two seeds, limb for limb against pyoracle.gen_values;
* search: one- and two-variable sets ``x == K`` whose K is the oracle's value of one candidate
  (only a search kernel whose generator is the oracle's finds it where the oracle does), full
  sweep and early exit, budgets 128 and 4096, one set over the 16-register kernel; found and
  the counters against search_counters.py;
* selects: W_ITE with the condition mixed within a wave, W_SDIV / W_SREM / W_SMOD over all four
  sign combinations, divisor 0 and the most negative value, one pinned set per candidate.

Small sets only; the oracle masks are computed once per module."""

import functools

import numpy as np
import pyoracle as O
import pytest
import search_counters as SC
from test_gpu_search_schedule import COUNT_OPS, EARLY, SHORT, _max_w_written, assert_row

from mythril_amd import ir
from mythril_amd.lower import Dag, lower

pytestmark = pytest.mark.gpu

M256 = (1 << 256) - 1
MIN256 = 1 << 255
WIDTHS = (1, 8, 32, 33, 128, 129, 160, 256)
CANDS = (0, 1, 2, 3, 63, 64, 65, 4095, 65535)
SEEDS = (0x5EED_0014, 0x1234_5678_9ABC_DEF0)
POOL = (0xDEAD_BEEF_0000_0000_0000_0000_0000_0000_0000_0001,      # a 160-bit address
        M256,                                                     # + 1 wraps to 0
        0x8000_0000_0000_0000_FFFF_FFFF_FFFF_FFFF << 128)         # carries across the limbs


def _rnd(k, w):
    """A fixed w-bit value (parents)."""
    return O.uf_hash(k + 1, 0x9E37) & ir.mask(w)


def _generator_set(n_const, parented):
    """Every kind of variable over ``n_const`` pool constants; with ``parented`` all but
    every fourth variable carry a parent value."""
    dag = Dag()
    if n_const:
        dag.force_consts(POOL[:n_const])
    specs = [("g%d" % w, w, ir.VK_GENERIC, 0, 0) for w in WIDTHS]
    specs += [("s%d" % i, w, ir.VK_SMALL, h, 0)
              for i, (w, h) in enumerate([(32, 0xFFFFFFFF), (8, 3), (32, 4), (256, 100), (129, 0xFFFFFFFF)])]
    specs += [("b", 1, ir.VK_BOOL, 0, 0)]
    specs += [("a0", 160, ir.VK_ACTOR, 0, 0), ("v", 256, ir.VK_VALUE, 0, 0), ("v128", 128, ir.VK_VALUE, 0, 0)]
    if n_const >= 3:
        specs += [("a3", 160, ir.VK_ACTOR, 0, 3), ("a3w", 256, ir.VK_ACTOR, 0, 3)]
    if n_const:
        specs += [("k", 256, ir.VK_KECCAK, n_const - 1, 0)]
    # calldata bytes: byte 0 and byte 13 of word 5 over the whole pool (wk = 0), byte 31 of
    # word 6 over const[1 .. 3)
    specs += [("cd0", 8, ir.VK_CDBYTE, 0, 5), ("cd13", 8, ir.VK_CDBYTE, 8 * 13, 5)]
    if n_const >= 3:
        specs += [("cd31", 8, ir.VK_CDBYTE, 8 * 31 | 2 << 8 | 1 << 20, 6)]
    nodes = {}
    for i, (name, w, kind, h0, h1) in enumerate(specs):
        par = _rnd(i, w) if parented and i % 4 != 3 else None
        nodes[name] = dag.var(name, w, kind, h0, h1, par)
    dag.assert_(nodes["b"])
    return lower(dag, seed=0xC0FFEE + n_const)


@functools.lru_cache(maxsize=None)
def generator_sets():
    progs = [_generator_set(n, par) for n in (0, 1, 3) for par in (False, True)]
    batch = ir.Batch(progs)
    for s, n in enumerate((0, 0, 1, 1, 3, 3)):
        assert int(batch.descs[s][3]) == n, (s, batch.descs[s])
    assert int(batch.descs[0][5]) >= 19
    return progs, batch


def test_materialize_matches_oracle(engine):
    progs, batch = generator_sets()
    db = engine.upload(progs)
    set_ids = [s for s in range(len(progs)) for _ in CANDS]
    cand_ids = [c for _ in range(len(progs)) for c in CANDS]
    for seed in SEEDS:
        got = engine.materialize_limbs(db, set_ids, cand_ids, seed=seed)
        want = []
        for s in range(len(progs)):
            want += [v for row in O.SetView.from_batch(batch, s).gen_assignments(np.array(CANDS, dtype=np.uint64), seed)
                     for v in row]
        want = ir.limbs_array(want)
        assert got.shape == want.shape
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (hex(seed), [(int(r), got[r].tolist(), want[r].tolist()) for r in bad[:4]])
    db.free()


# ---- search path ---------------------------------------------------------------------------

SEED_S, N_CAND_S = 0x5EED_0A_6E4E, 4096


def _value_at(prog, cand, seed):
    return O.SetView.from_batch(ir.Batch([prog]), 0).gen_assignments(np.array([cand], dtype=np.uint64), seed)[0]


def _pin(build, node_values, cands, **kw):
    """build(ks) with ks = node_values(the oracle's variable values of a candidate): the first
    of ``cands`` at which that holds for the finished program too.  The pinned constants join
    the set's pool, which the generator's constant arm reads, so a candidate whose variables
    take that arm can move under its own pin; the next candidate is taken then."""
    probe = lower(build(None), **kw)
    for c in cands:
        ks = node_values(_value_at(probe, c, SEED_S))
        if ks is None:
            continue
        prog = lower(build(ks), **kw)
        if node_values(_value_at(prog, c, SEED_S)) == ks:
            return prog
    raise AssertionError("no stable candidate among %r" % (list(cands),))


def _pinned(specs, cand, parent_of=None):
    """ASSERT(v == K_v) for every variable, K the oracle's values of candidate ``cand``."""
    def build(ks):
        dag = Dag()
        for i, (name, w, kind, h0, h1) in enumerate(specs):
            x = dag.var(name, w, kind, h0, h1, parent_of(i, w) if parent_of else None)
            dag.assert_(dag.op(ir.B_EQ, w, x, dag.const(ks[i] if ks else i + 2, w)))
        return dag
    return _pin(build, list, range(cand, cand + 32), seed=77)


def _wide_pinned(cand, n_live=10):
    """Ten products alive at once (the 16-register kernel), each pinned to the oracle's value."""
    def build(ks):
        dag = Dag()
        x, y = dag.var("x", 256), dag.var("y", 256)
        prods = [dag.op(ir.W_MUL, 256, x, dag.op(ir.W_ADD, 256, y, dag.const(k + 1, 256))) for k in range(n_live)]
        acc = prods[0]
        for p in prods[1:]:
            acc = dag.op(ir.W_XOR, 256, acc, p)
        for k, p in enumerate(prods):
            dag.assert_(dag.op(ir.B_EQ, 256, dag.op(ir.W_XOR, 256, p, acc), dag.const(ks[k] if ks else 100 + k, 256)))
        return dag

    def node_values(vals):
        if min(vals) >> 128 == 0:   # x = 0 or a small y would hold in many candidates
            return None
        prods = [vals[0] * (vals[1] + k + 1) & M256 for k in range(n_live)]
        acc = functools.reduce(lambda a, b: a ^ b, prods)
        return [p ^ acc for p in prods]
    prog = _pin(build, node_values, range(cand, cand + 32), seed=78, nw=ir.NW)
    assert _max_w_written(prog) >= ir.NW_NARROW
    return prog


@functools.lru_cache(maxsize=None)
def search_sets():
    G = ir.VK_GENERIC
    progs = []
    # (a one-variable set's K is its pool's only constant, so the constant arm finds it early
    # as well: about one candidate in 16)
    for w, cand in [(256, 5), (256, 77), (129, 100), (128, 101), (8, 90), (160, 63)]:
        progs.append(_pinned([("x", w, G, 0, 0)], cand))
    for ws, cand in [((256, 256), 64), ((256, 64), 3001), ((32, 256), 127), ((160, 129), 1),
                     ((256, 256, 256), 2500), ((33, 256, 129), 4000), ((128, 8, 256), 191)]:
        progs.append(_pinned([("x%d" % i, w, G, 0, 0) for i, w in enumerate(ws)], cand))
    # a parent that is no witness: candidate 0 and the parent's neighbourhood fall
    progs.append(_pinned([("x", 256, G, 0, 0), ("y", 128, G, 0, 0)], 66, parent_of=lambda i, w: _rnd(40 + i, w)))
    progs.append(_pinned([("n", 32, ir.VK_SMALL, 100, 0), ("v", 256, ir.VK_VALUE, 0, 0)], 70))
    progs.append(_wide_pinned(75))
    progs.append(_wide_pinned(3500))
    batch = ir.Batch(progs)
    masks = np.array([O.SetView.from_batch(batch, s).check(N_CAND_S, SEED_S)[1] for s in range(len(progs))], dtype=bool)
    # every set has a witness, and some sets' first witness lies past 128
    firsts = [SC.first_witness(m, N_CAND_S) for m in masks]
    assert all(f is not None for f in firsts) and sum(f >= 128 for f in firsts) >= 3
    return progs, masks, SC.aux1_totals(batch)


@pytest.fixture(scope="module")
def db_search(engine):
    db = engine.upload(search_sets()[0])
    yield db
    db.free()


@pytest.mark.parametrize("flags", [pytest.param(COUNT_OPS, id="full"), pytest.param(SHORT, id="shortcircuit"),
                                   pytest.param(EARLY, id="early"), pytest.param(EARLY | SHORT, id="early_shortcircuit")])
@pytest.mark.parametrize("budget", [128, 4096])
def test_search_generator_matches_oracle(engine, db_search, budget, flags):
    progs, masks, aux1 = search_sets()
    res = engine.check(db_search, budget=budget, seed=SEED_S, flags=flags)
    assert_row(res, masks, budget, flags, aux1, "generator")


# ---- selects -------------------------------------------------------------------------------

SEED_D, N_CAND_D = 0x5EED_0D17, 128
NEG = M256 - 6            # -7
_SIGNED = {ir.W_SDIV: O.bvsdiv, ir.W_SREM: O.bvsrem, ir.W_SMOD: O.bvsmod}


def _select_dag(op, k):
    """a = b0 ? MIN : (b1 ? -7 : x), b = b2 ? 0 : (b3 ? -1 : y): W_ITE with the condition mixed
    within a wave; ASSERT(op(a, b) == k), or ASSERT(a + b == k) for W_ITE itself."""
    dag = Dag()
    b = [dag.var("b%d" % i, 1, ir.VK_BOOL) for i in range(4)]
    x, y = dag.var("x", 256), dag.var("y", 256)
    a_ = dag.op(ir.W_ITE, 256, b[0], dag.const(MIN256, 256), dag.op(ir.W_ITE, 256, b[1], dag.const(NEG, 256), x))
    b_ = dag.op(ir.W_ITE, 256, b[2], dag.const(0, 256), dag.op(ir.W_ITE, 256, b[3], dag.const(M256, 256), y))
    node = dag.op(ir.W_ADD if op == ir.W_ITE else op, 256, a_, b_)
    dag.assert_(dag.op(ir.B_EQ, 256, node, dag.const(k, 256)))
    return dag


def _select_operands(vals):
    b0, b1, b2, b3, x, y = vals
    return (MIN256 if b0 else (NEG if b1 else x)), (0 if b2 else (M256 if b3 else y))


_CLASSES = [  # (a negative, b negative, b == 0, a == MIN, MIN / -1)
    (0, 0, False, False, False), (0, 1, False, False, False), (1, 0, False, False, False),
    (1, 1, False, False, False), (0, 0, True, False, False), (1, 0, True, False, False),
    (1, 1, False, True, True), (1, 0, True, True, False), (1, 0, False, True, False)]


def _class_of(a, b):
    return (a >> 255, b >> 255, b == 0, a == MIN256, a == MIN256 and b == M256)


@functools.lru_cache(maxsize=None)
def select_sets():
    """Per op, one set per operand class, pinned at a candidate of that class (the first at
    which the pin holds under its own constant, _pin)."""
    probe = lower(_select_dag(ir.W_ITE, 0), seed=79)
    vals = O.SetView.from_batch(ir.Batch([probe]), 0).gen_assignments(np.arange(N_CAND_D, dtype=np.uint64), SEED_D)
    assert len({v[0] for v in vals[:64]}) == 2 and len({v[2] for v in vals[:64]}) == 2  # mixed in one wave
    by_class = {}
    for c, v in enumerate(vals):
        by_class.setdefault(_class_of(*_select_operands(v)), []).append(c)
    progs = []
    for op in (ir.W_ITE, ir.W_SDIV, ir.W_SREM, ir.W_SMOD):
        def value(v, op=op):
            a, b = _select_operands(v)
            return (a + b) & M256 if op == ir.W_ITE else _SIGNED[op](a, b, 256)
        for key in _CLASSES:
            prog = None
            for c in by_class[key]:
                k = value(vals[c])
                cand = lower(_select_dag(op, k), seed=79)
                v = O.SetView.from_batch(ir.Batch([cand]), 0).gen_assignments(np.array([c], dtype=np.uint64), SEED_D)[0]
                if _class_of(*_select_operands(v)) == key and value(v) == k:
                    prog = cand
                    break
            assert prog is not None, (op, key)
            ops = ir.Batch([prog]).code.reshape(-1, 4)[:, 0] & 0xFF
            assert (ops == ir.W_ITE).any() and (op == ir.W_ITE or (ops == op).any()), (op, key)
            progs.append(prog)
    batch = ir.Batch(progs)
    masks = np.array([O.SetView.from_batch(batch, s).check(N_CAND_D, SEED_D)[1] for s in range(len(progs))], dtype=bool)
    assert masks.any(axis=1).all()
    return progs, masks, SC.aux1_totals(batch)


@pytest.mark.parametrize("flags", [pytest.param(COUNT_OPS, id="full"), pytest.param(SHORT, id="shortcircuit"),
                                   pytest.param(EARLY | SHORT, id="early_shortcircuit")])
def test_selects_match_oracle(engine, flags):
    progs, masks, aux1 = select_sets()
    db = engine.upload(progs)
    res = engine.check(db, budget=N_CAND_D, seed=SEED_D, flags=flags)
    db.free()
    assert_row(res, masks, N_CAND_D, flags, aux1, "selects")
