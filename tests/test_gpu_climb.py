"""GPU: pf_climb_batch (Engine.climb) returns what the climb contract's CPU model
(tests/climb_model.py) returns — status, score, round and values, exactly — on the hand-made
sets of tests/climb_sets.py, whose premises (the plain search misses them, the model reaches
them) tests/test_climb_model.py asserts on the CPU.  Each call is at most 8 sets, 16 rounds
of 1,024 candidates."""

from dataclasses import replace

import numpy as np
import pytest

import climb_model as CM
import climb_sets as CS
from mythril_amd import _lib, ir
from mythril_amd.smt import gpu_check

pytestmark = pytest.mark.gpu


def ints(rows):
    return [ir.from_limbs(r) for r in np.asarray(rows, dtype=np.uint32).reshape(-1, 8)]


def both(engine, progs, set_ids, rounds, per_round, seed, timeout_ms=0):
    """(device result, model result) of one climb call over a fresh upload of ``progs``."""
    db = engine.upload(progs)
    try:
        got = engine.climb(db, set_ids, rounds, per_round, seed=seed, timeout_ms=timeout_ms)
    finally:
        db.free()
    return got, CM.climb(db.batch, set_ids, rounds, per_round, seed)


def assert_same(got, want, names):
    assert len(got.status) == len(want)
    for i, (w, name) in enumerate(zip(want, names)):
        dev = (int(got.status[i]), int(got.score[i]), int(got.round[i]), ints(got.values[i]))
        assert dev == (w.status, w.score, w.round, w.values), name
    assert got.evals == sum(w.evals for w in want)      # finished sets are no longer evaluated
    assert not got.timed_out


@pytest.fixture(scope="module")
def near(engine):
    progs = CS.near_sets()
    ids = list(range(len(progs)))
    got, want = both(engine, progs, ids, CS.ROUNDS, CS.PER_ROUND, CS.SEED)
    return progs, got, want


def test_plain_search_misses_what_the_climb_reaches(engine, near):
    """Fused byte equalities reached by bit flips, ULT / SLE / SLT bounds, sites that are not
    fused compares, a 7-register and a 16-register set in one call, W_SPILL / W_FILL."""
    progs, got, want = near
    db = engine.upload(progs)
    res = engine.check(db, budget=65536, seed=CS.SEED, flags=ir.FLAG_EARLY_EXIT)
    db.free()
    assert (res.found == 0xFFFFFFFF).all()
    assert_same(got, want, [p.name for p in progs])
    assert got.sat.all() and all(1 <= int(r) < CS.ROUNDS for r in got.round)
    assert {p.name for p in progs} >= {"bytes3", "orderings", "bytes3-unfused", "orderings-r16", "bytes3-spill"}


def test_unfused_sites_move_in_steps_of_512(engine, near):
    progs, got, _ = near
    i = [p.name for p in progs].index("bytes3-unfused")
    assert int(got.score[i]) == 3 * 512
    # a climb cut short of the witness: still a multiple of 512, and the model's
    g, w = both(engine, [progs[i]], [0], 1, CS.PER_ROUND, CS.SEED)
    assert_same(g, w, ["bytes3-unfused"])
    assert int(g.score[0]) % 512 == 0 and int(g.status[0]) == ir.CLIMB_NONE


def test_trivial_programs_are_witnesses_in_round_0(engine):
    progs = [CS.bare_end(), CS.no_vars(), CS.no_vars(False)]
    got, want = both(engine, progs, [0, 1, 2], 4, 100, 3)
    assert_same(got, want, [p.name for p in progs])
    assert [int(s) for s in got.status] == [ir.CLIMB_WITNESS, ir.CLIMB_WITNESS, ir.CLIMB_NONE]
    assert [int(r) for r in got.round[:2]] == [0, 0] and [int(s) for s in got.score] == [0, 512, 254]


@pytest.mark.parametrize("per_round", [100, 1, 64, 65])
def test_last_group_with_inactive_lanes(engine, per_round):
    """per_round = 100 is not a multiple of 64: the lanes past it count for nothing."""
    progs = CS.near_sets()[:2] + [CS.kinds()]
    got, want = both(engine, progs, [0, 1, 2], 6, per_round, 77)
    assert_same(got, want, [p.name for p in progs])


def test_ties_go_to_the_smaller_index_and_sideways_moves_are_adopted(engine):
    """Every candidate of `flat` scores 254: round 0 takes index 0; every later round's best
    equals the current score and is index 1 — adopted, so the values are candidate 1 of the last
    round under the assignment before it."""
    got, want = both(engine, [CS.flat()], [0], 5, 256, 11)
    assert_same(got, want, ["flat"])
    assert (want[0].score, want[0].round, want[0].index) == (254, 4, 1)
    prev, _ = both(engine, [CS.flat()], [0], 4, 256, 11)
    assert ints(prev.values[0]) != ints(got.values[0])


def test_subset_in_reversed_order_with_different_variable_counts(engine):
    progs = [CS.bytes3(), CS.kinds(), CS.flat(), CS.no_vars(), CS.orderings(base=8, name="orderings-r16"),
             CS.no_vars(False)]
    for p in progs:
        p.seed = CS.NEAR_SEEDS.get(p.name, 21)
    assert len({len(p.vars) for p in progs}) >= 3
    ids = [4, 3, 1, 0]
    got, want = both(engine, progs, ids, 5, 200, CS.SEED)
    assert_same(got, want, [progs[i].name for i in ids])
    assert [len(v) for v in got.values] == [len(progs[i].vars) for i in ids]
    # the same sets asked for one by one give the same answers
    for k, i in enumerate(ids):
        g, _ = both(engine, progs, [i], 5, 200, CS.SEED)
        assert (int(g.status[0]), int(g.score[0]), int(g.round[0]), ints(g.values[0])) == \
            (int(got.status[k]), int(got.score[k]), int(got.round[k]), ints(got.values[k]))


def test_a_set_that_finishes_early_next_to_one_that_runs_all_rounds(engine, near):
    progs, _, nwant = near
    early = min(range(len(progs)), key=lambda i: nwant[i].round)
    pair = [progs[early], CS.kinds()]
    got, want = both(engine, pair, [0, 1], CS.ROUNDS, CS.PER_ROUND, CS.SEED)
    assert_same(got, want, [p.name for p in pair])
    assert int(got.status[0]) == ir.CLIMB_WITNESS and int(got.round[0]) < CS.ROUNDS - 1
    assert int(got.status[1]) == ir.CLIMB_NONE
    assert got.evals == (int(got.round[0]) + 1) * CS.PER_ROUND + CS.ROUNDS * CS.PER_ROUND


def test_every_variable_kind_keeps_its_parent_first(engine):
    """ACTOR, KECCAK, SMALL, BOOL, CDBYTE, VALUE and a plain variable, all parented from round
    1 on: the model applies the "parent first" rule to each."""
    prog = CS.kinds()
    assert {v.kind for v in prog.vars} == {ir.VK_ACTOR, ir.VK_KECCAK, ir.VK_SMALL, ir.VK_BOOL, ir.VK_CDBYTE,
                                           ir.VK_VALUE, ir.VK_GENERIC}
    for seed in (5, 6):
        got, want = both(engine, [prog], [0], 8, 512, seed)
        assert_same(got, want, ["kinds"])
    # with one candidate per round only candidate 0 exists: after round 0 nothing moves, and
    # what is returned is round 0's candidate 0 of every kind
    got, want = both(engine, [prog], [0], 3, 1, 5)
    assert_same(got, want, ["kinds"])
    assert int(got.round[0]) == 0


def test_deadline_cuts_or_gives_the_models_verdict(engine):
    db = engine.upload([CS.long_exp()])
    try:
        got = engine.climb(db, [0], 16, 64, seed=1, timeout_ms=1)
    finally:
        db.free()
    assert int(got.status[0]) != ir.CLIMB_WITNESS          # 5 == 6 is part of it
    if int(got.status[0]) == ir.CLIMB_CUT:
        # cut: the deadline is reported, the score is no witness's, and only whole rounds count
        assert got.timed_out
        assert int(got.score[0]) < CM.device_sets(db.batch)[0].target
        assert int(got.round[0]) < 16 and got.evals % 64 == 0 and got.evals < 16 * 64
        assert len(got.values[0]) == 1
    else:
        assert_same(got, CM.climb(db.batch, [0], 16, 64, 1), ["long-exp"])


def test_errors_launch_nothing(engine):
    db = engine.upload([CS.flat(), CS.no_vars()])
    try:
        # every one of these is pf_climb_batch's own error (Engine.climb passes a single
        # batch's ids through unchecked)
        for kw, text in ((dict(set_ids=[0], rounds=0, per_round=8), "pf_climb_batch: rounds"),
                         (dict(set_ids=[0], rounds=2, per_round=0), "pf_climb_batch: per_round"),
                         (dict(set_ids=[0, 2], rounds=2, per_round=8), "pf_climb_batch: set 2 out of range"),
                         (dict(set_ids=[1, 1], rounds=2, per_round=8), "pf_climb_batch: set 1 requested twice")):
            with pytest.raises(_lib.PathFeasError, match=text):
                engine.climb(db, **kw)
        # over several batches the routing has to know where an id belongs
        with pytest.raises(_lib.PathFeasError, match="out of range"):
            engine.climb([db, db], [4], 2, 8)
        empty = engine.climb(db, [], 2, 8)
        assert len(empty.status) == 0 and empty.evals == 0
        # the batch is still good, for the search and for a climb
        assert int(engine.check(db, budget=64, seed=0).found[1]) == 0
        assert int(engine.climb(db, [1], 2, 8).status[0]) == ir.CLIMB_WITNESS
    finally:
        db.free()


def test_climbing_twice_and_searching_in_between_changes_nothing(engine):
    progs = CS.near_sets()[:2]
    db = engine.upload(progs)
    try:
        a = engine.climb(db, [0, 1], 6, 128, seed=9)
        found = engine.check(db, budget=4096, seed=CS.SEED).found.copy()
        b = engine.climb(db, [1, 0], 6, 128, seed=9)
        assert (engine.check(db, budget=4096, seed=CS.SEED).found == found).all()
    finally:
        db.free()
    for i, j in ((0, 1), (1, 0)):
        assert (int(a.status[i]), int(a.score[i]), int(a.round[i]), ints(a.values[i])) == \
            (int(b.status[j]), int(b.score[j]), int(b.round[j]), ints(b.values[j]))


def test_sharded_upload_routes_every_set_to_its_batch(engine):
    """Engine.climb over a list of batches: set ids index their concatenation."""
    progs = CS.near_sets()[:2] + [CS.flat(), CS.no_vars()]
    dbs = [engine.upload(progs[:3]), engine.upload(progs[3:])]
    try:
        got = engine.climb(dbs, [3, 0, 2], 4, 96, seed=4)
    finally:
        for d in dbs:
            d.free()
    want = CM.climb(dbs[0].batch, [0, 2], 4, 96, 4) + CM.climb(dbs[1].batch, [0], 4, 96, 4)
    assert_same(got, [want[2], want[0], want[1]], ["no-vars", "bytes3", "flat"])


def test_check_sets_with_climb_on_the_device(engine):
    """tests/test_climb_wiring.py's checks on the real engine, over the whole wiring corpus."""
    import test_climb_wiring as W

    cfg_off = replace(gpu_check.CONFIG, budget=W.BUDGET, hints=False, climb_rounds=0)
    cfg_on = replace(cfg_off, climb_rounds=W.ROUNDS, climb_candidates=W.CANDIDATES)
    c, unsat = W.wiring_corpus(n_unsat=48)
    off, on, climbed, climb_sat = W.check_wiring(c, unsat, cfg_off, cfg_on, engine)
    # ... and the whole corpus' figures are the oracle-backed engine's (the model's)
    gained = [i for i, (m0, m1) in enumerate(zip(off, on)) if m0 is None and m1 is not None]
    got = dict(queries=len(on), off=sum(m is not None for m in off), on=sum(m is not None for m in on),
               climbed=climbed, climb_sat=climb_sat, gained=gained)
    assert got == W.WHOLE
