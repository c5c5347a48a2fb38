"""GPU: searches over device programs folded by the range rules, with constants of their own
in the device pool (mythril_amd/csrc/pf_fold.h, pf_batch_create's device pool), report what
the oracle finds in the programs as lowered — ``found`` and the counters of search_counters.py.

One batch of 48 sets (above pf_batch_create's 16-set fold gate) at a budget of 4,096:
config-3 ids 0..39 and eight sets built around the new rewrites — a dropped ``0 <= x`` root
whose chain held a division and an EXP, a bound-decided compare at widths 8 and 160, a constant
of the program's own consumed as a divisor, as an EXP base and by a compare, a set without
constants that gains one, and a set whose variables draw from the pool (harvested constants,
the actor table), where a shifted pool would change the candidates.  The kernel runs the
device programs; coracle evaluates the lowered ones.  A last case sends the special sets
through pf_materialize, pf_eval_assignments and pf_eval_programs, the other readers of the
device pool."""

import functools

import numpy as np
import pytest
import search_counters as SC

import pyoracle as O
from mythril_amd import _lib, ir, synth
from op_programs import Asm
from test_device_range import (M, R, T0, T1, T2, T3, X, Y, _and, cmp_program, const_result_program,
                               no_const_program, pool_view)

pytestmark = pytest.mark.gpu

COUNT_OPS, SHORT, EARLY = ir.FLAG_COUNT_OPS, ir.FLAG_SHORTCIRCUIT, ir.FLAG_EARLY_EXIT
SEED, BUDGET, SHORT_BUDGET = 0x4A9E_5EED, 4096, 128
N_CONFIG3 = 40
ACTORS = [0xA11CE << 140 | 1, 0xB0B << 148 | 2, 0xCA401 << 120 | 3]
HARVESTED = 0x5EED_0000_0000_0000_1234 << 96


def _dropped_root_set():
    s = Asm("range:dropped-root", parents=False)
    s.p.seed = 21
    s.wvar(X, 256, None)
    s.wvar(Y, 256, None)
    s.w(ir.W_UDIV, 256, T1, X, Y)
    s.w(ir.W_EXP, 256, T2, T1, Y)
    s.wconst(T3, 256, 0)
    s.cmp(ir.B_ULE, 256, 0, T3, T2)
    s.assert_(0)
    s.cmp(ir.B_ULT, 256, 1, X, Y)
    s.assert_(1)
    return s.done(verdict=None)


def _pool_reader_set():
    """a: an actor (table = constants 0..2), g: a generic variable whose constant arm draws
    from the pool.  a == ACTORS[1] and g == HARVESTED + 1 are reached through the pool alone;
    y != c (c = ACTORS[0] * 3, a constant of the program's own) keeps a new constant live."""
    s = Asm("range:pool-readers", parents=False)
    s.p.seed = 22
    s.p.consts.extend(ACTORS + [HARVESTED])
    a = s.var(160, None, ir.VK_ACTOR, 0, 3)
    g = s.var(256, None)
    y = s.var(256, None)
    s.p.emit(ir.W_VAR, 160, dst=X, aux0=a)
    s.p.emit(ir.W_VAR, 256, dst=Y, aux0=g)
    s.p.emit(ir.W_VAR, 256, dst=R, aux0=y)
    s.wconst(T0, 160, ACTORS[1])
    s.cmp(ir.B_EQ, 160, 0, X, T0)
    s.assert_(0)
    s.wconst(T0, 256, HARVESTED + 1)
    s.cmp(ir.B_EQ, 256, 1, Y, T0)
    s.assert_(1)
    s.wconst(T0, 256, ACTORS[0])
    s.wconst(T1, 256, 3)
    s.w(ir.W_MUL, 256, T2, T0, T1)
    s.cmp(ir.B_EQ, 256, 2, R, T2)
    s.assert_(2, expect=False)
    return s.done(verdict=None)


def _special_sets():
    out = [_dropped_root_set()]
    for w, p in ((8, 4), (160, 80)):              # ((x & M(p)) < 2^p) xor (y == x)
        out.append(cmp_program("range:bound", w, p, ir.B_ULT, 1 << p, True))
    out.append(const_result_program(256, "divisor", ir.B_ULE)[0])
    out.append(const_result_program(256, "exp_base", ir.B_ULE)[0])
    out.append(const_result_program(64, "compare")[0])
    out.append(no_const_program(256))
    out.append(_pool_reader_set())
    for k, p in enumerate(out):
        p.seed = 31 + k
    return out


@functools.lru_cache(maxsize=None)
def sets():
    progs = [synth.random_dag_set(i, plant=False)[0] for i in range(N_CONFIG3)] + _special_sets()
    assert len(progs) == 48
    batch = ir.Batch(progs)
    code, descs, pool = _lib.device_batch(batch.code, batch.consts, batch.descs)
    rows = [[tuple(int(x) for x in r) for r in code[int(d[0]):int(d[0]) + int(d[1])]] for d in descs]
    return progs, batch, SC.sat_masks(batch, SEED, BUDGET), SC.aux1_totals(batch), (rows, descs, pool)


def shortcircuit_ops(batch, dev, seed, budget):
    """search_counters.shortcircuit_ops over the program pf_batch_create uploads, read against
    the device pool."""
    rows_all, descs, pool = dev
    total = 0
    for s, rows in enumerate(rows_all):
        view = pool_view(batch, descs, pool, s)
        vals = O.SetView.from_batch(batch, s).gen_assignments(np.arange(budget, dtype=np.uint64), seed)
        tr = [SC.device_trace(view, rows, v) for v in vals]
        prefix = np.cumsum([r[3] for r in rows], dtype=np.uint64)
        for g, size in enumerate(SC.group_sizes(budget)):
            lanes = tr[64 * g:64 * g + size]
            if any(root for root, _ in lanes):
                total += size * int(prefix[-1])
            else:
                total += size * int(prefix[max(fell for _, fell in lanes)])
    return total


@pytest.fixture(scope="module")
def db(engine):
    d = engine.upload(sets()[0])
    yield d
    d.free()


def test_the_batch_is_what_it_says():
    """The device forms the cases rest on (host only), and witnesses of every kind."""
    _, batch, masks, aux1, (rows, descs, pool) = sets()
    ops = [[r[0] & 0xFF for r in rs] for rs in rows]
    s0 = N_CONFIG3
    assert not {ir.W_UDIV, ir.W_EXP, ir.B_ULE} & set(ops[s0]) and ir.B_ULT in ops[s0]
    for s in (s0 + 1, s0 + 2):
        assert ir.B_ULT not in ops[s] and ir.W_AND not in ops[s], s
    consts = np.asarray(batch.consts, dtype=np.uint32).reshape(-1, 8)
    assert (pool[:len(consts)] == consts).all() and len(pool) > len(consts)
    for s, unit in ((s0 + 3, ir.W_UREM), (s0 + 4, ir.W_EXP), (s0 + 5, ir.B_ULT), (s0 + 6, ir.W_UDIV),
                    (s0 + 7, ir.B_EQ)):
        d, lo = descs[s], batch.descs[s]
        assert int(d[2]) >= len(consts) and int(d[3]) == int(lo[3]), s      # moved behind the caller's pool
        assert (pool[int(d[2]):int(d[2]) + int(d[3])] == consts[int(lo[2]):int(lo[2]) + int(lo[3])]).all(), s
        k = int(d[3])                                                        # the new constant's index
        user = [r for r in rows[s] if r[0] & 0xFF == unit and
                ((r[0] & SC.I_KA and (r[1] >> 8) & 0xFF == k) or (r[0] & SC.I_KB and (r[1] >> 16) & 0xFF == k))]
        assert user and ir.W_MUL not in ops[s] and ir.W_NOT not in ops[s], (s, rows[s])
    assert int(descs[s0 + 6][3]) == 0
    assert [sum(r[3] for r in rs) for rs in rows] == aux1
    assert int((descs[:N_CONFIG3, 2] != np.asarray(batch.descs)[:N_CONFIG3, 2]).sum()) >= 3   # config 3 gains some too
    fs = [SC.first_witness(m, BUDGET) for m in masks]
    assert all(f is not None for f in fs[s0:]), fs[s0:]
    assert sum(f is not None and f >= 64 for f in fs[s0:]) >= 1
    assert sum(f is None for f in fs[:s0]) >= 3


def test_full_sweep_counts_every_candidate_and_the_lowered_ops(engine, db):
    _, _, masks, aux1, _ = sets()
    res = engine.check(db, budget=BUDGET, seed=SEED, flags=COUNT_OPS)
    assert np.array_equal(res.found, SC.found(masks, BUDGET))
    assert not res.timed_out
    assert (res.cands_decided, res.evals_full, res.ops) == SC.full_sweep(masks, BUDGET, aux1)
    assert res.evals_full == 48 * 4096


def test_shortcircuit_sweep_leaves_where_the_device_program_says(engine, db):
    _, batch, masks, _, dev = sets()
    res = engine.check(db, budget=SHORT_BUDGET, seed=SEED, flags=SHORT | COUNT_OPS)
    assert np.array_equal(res.found, SC.found(masks, SHORT_BUDGET))
    assert res.cands_decided == 48 * SHORT_BUDGET
    assert res.evals_full == SC.shortcircuit_evals_full(masks, SHORT_BUDGET)
    assert res.ops == shortcircuit_ops(batch, dev, SEED, SHORT_BUDGET)
    # the program readable against the caller's pool exits at the same asserts
    assert res.ops == SC.shortcircuit_ops(batch, SEED, SHORT_BUDGET)


@pytest.mark.parametrize("flags", [EARLY | COUNT_OPS, EARLY | SHORT | COUNT_OPS], ids=["early", "early_shortcircuit"])
def test_early_exit_search_finds_the_first_witness(engine, db, flags):
    _, _, masks, aux1, _ = sets()
    res = engine.check(db, budget=BUDGET, seed=SEED, flags=flags)
    assert np.array_equal(res.found, SC.found(masks, BUDGET))
    assert not res.timed_out
    floor, total = SC.early_exit_floor(masks, BUDGET), 48 * BUDGET
    assert floor <= res.cands_decided <= total
    if flags & SHORT:
        assert res.evals_full <= res.cands_decided
    else:
        assert res.evals_full == res.cands_decided
        lo = sum(a * SC.early_exit_floor(masks[s:s + 1], BUDGET) for s, a in enumerate(aux1))
        assert lo <= res.ops <= BUDGET * sum(aux1)


def test_a_program_folded_to_a_bare_end_is_decided_by_its_first_group(engine):
    """Sixteen sets whose roots the range rules decide (0 <= x * y): every program is a bare
    END, candidate 0 is the witness, and an early-exit search evaluates exactly the first
    group of each — the later slices stop without waiting to see the post in found[], so the
    counters are the same in every run."""
    progs = []
    for k in range(16):
        s = Asm(f"range:bare-end/{k}", parents=False)
        s.p.seed = 60 + k
        s.wvar(X, 256, None)
        s.wvar(Y, 256, None)
        s.w(ir.W_MUL, 256, T1, X, Y)
        s.wconst(T3, 256, 0)
        s.cmp(ir.B_ULE, 256, 0, T3, T1)
        s.assert_(0)
        progs.append(s.done(verdict=None))
    batch = ir.Batch(progs)
    code, descs, _ = _lib.device_batch(batch.code, batch.consts, batch.descs)
    assert [int(d[1]) for d in descs] == [1] * 16
    aux1 = SC.aux1_totals(batch)
    d = engine.upload(progs)
    try:
        for flags in (EARLY | COUNT_OPS, EARLY | SHORT | COUNT_OPS):
            for _ in range(2):
                res = engine.check(d, budget=BUDGET, seed=SEED, flags=flags)
                assert not res.found.any()
                assert (res.cands_decided, res.evals_full, res.ops) == (16 * 64, 16 * 64, 64 * sum(aux1))
    finally:
        d.free()


def test_the_other_readers_of_the_device_pool(engine, db):
    """pf_materialize regenerates the oracle's candidates of the special sets (their const_off
    moved, their n_const did not), and pf_eval_assignments (the batch's pool) and
    pf_eval_programs (a pool of its own call) give the oracle's verdicts on them."""
    _, batch, masks, _, _ = sets()
    n_cand = 64
    cands = np.arange(n_cand, dtype=np.uint64)
    special = range(N_CONFIG3, 48)
    views = {s: O.SetView.from_batch(batch, s) for s in special}
    vals = {s: views[s].gen_assignments(cands, SEED) for s in special}
    set_ids = [s for s in special for _ in range(n_cand)]
    cand_ids = [c for _ in special for c in range(n_cand)]
    got = engine.materialize(db, set_ids, cand_ids, seed=SEED)
    want = [vals[s][c] for s in special for c in range(n_cand)]
    assert got == want
    n_vars = int(np.asarray(batch.descs)[:, 5].sum())
    soa_all = np.zeros((max(n_vars, 1), 8, n_cand), dtype=np.uint32)
    for s in range(48):
        sv = views.get(s) or O.SetView.from_batch(batch, s)
        vs = vals.get(s) or sv.gen_assignments(cands, SEED)
        off = int(batch.descs[s][4])
        for c, row in enumerate(vs):
            for v, x in enumerate(row):
                soa_all[off + v, :, c] = ir.to_limbs(x)
    for s in special:
        off, nv = int(batch.descs[s][4]), int(batch.descs[s][5])
        sat = engine.eval_assignments(db, s, soa_all[off:off + nv])
        assert np.array_equal(sat, masks[s][:n_cand]), s
    pack = tuple(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
                 for a in (batch.code, batch.consts, batch.schema, batch.descs))
    sat = engine.eval_programs(pack, soa_all)
    assert np.array_equal(sat, masks[:, :n_cand])
