"""GPU: pf_census_batch (Engine.census) returns what the census contract's CPU model
(tests/census_model.py) returns — every count, the nearest miss and the status, exactly — on the
hand-made sets of tests/census_sets.py, whose premises (witnesses, misses, sole sites, more than
32 sites, plain and fused sites, a spilled Bool) tests/test_census_model.py asserts on the CPU.
The parity calls are at most 18 small sets and 209 candidates; the deadline and the explain_sets
cases take 4,096."""

import pytest

import census_model as M
import census_sets as CS
import climb_sets
from mythril_amd import _lib, ir

pytestmark = pytest.mark.gpu


def rows(res, i):
    return (res.holds[i].tolist(), res.alive[i].tolist(), res.sole[i].tolist(), int(res.best_fails[i]),
            int(res.best_cand[i]), int(res.status[i]))


def assert_same(got, want, names, budget):
    assert len(got.status) == len(want) == len(names)
    for i, (w, name) in enumerate(zip(want, names)):
        assert rows(got, i) == (w.holds, w.alive, w.sole, w.best_fails, w.best_cand, ir.CENSUS_DONE), name
    assert got.evals == budget * len(want) and not got.timed_out


@pytest.fixture(scope="module")
def big(engine):
    progs = CS.big_batch()
    db = engine.upload(progs)
    yield progs, db
    db.free()


@pytest.fixture(scope="module")
def small(engine):
    progs = CS.small_batch()
    db = engine.upload(progs)
    yield progs, db
    db.free()


@pytest.mark.parametrize("budget", CS.BUDGETS)
def test_folded_batch_equals_the_model(engine, big, budget):
    """18 sets, folded, constants of their own; 8-register sets next to 16-register ones, one
    site, no site, 40 sites, plain and fused sites, Bool spills in scratch and LDS."""
    progs, db = big
    ids = list(range(len(progs)))
    got = engine.census(db, ids, budget=budget, seed=CS.SEED)
    assert_same(got, M.census(db.batch, ids, budget, CS.SEED), [p.name for p in progs], budget)
    assert [len(h) for h in got.holds] == engine.site_counts(db, ids).tolist()
    # best_fails == 0 exactly where the plain search finds a witness, best_cand its index
    found = engine.check(db, budget=budget, seed=CS.SEED, flags=ir.FLAG_EARLY_EXIT).found
    for i, p in enumerate(progs):
        assert (int(got.best_fails[i]) == 0) == (int(found[i]) != 0xFFFFFFFF), p.name
        if int(got.best_fails[i]) == 0:
            assert int(got.best_cand[i]) == int(found[i]), p.name


@pytest.mark.parametrize("budget", CS.BUDGETS)
def test_unfolded_batch_equals_the_model(engine, small, budget):
    progs, db = small
    got = engine.census(db, [0, 1, 2], budget=budget, seed=CS.SEED)
    assert_same(got, M.census(db.batch, [0, 1, 2], budget, CS.SEED), [p.name for p in progs], budget)


def test_subset_in_another_order_and_a_second_seed(engine, big):
    """Output offsets (sets of 40, 0, 3, 1 and 5 sites, not ascending) and the accumulator
    reset: the second call's counts are its own, not the sum."""
    progs, db = big
    names = [p.name for p in progs]
    ids = [7, 1, 17, 13, 6, 0]
    assert len({len(M.site_indices(d)) for d in M.CM.device_sets(db.batch)}) >= 4
    a = engine.census(db, ids, budget=209, seed=CS.SEED)
    assert_same(a, M.census(db.batch, ids, 209, CS.SEED), [names[i] for i in ids], 209)
    b = engine.census(db, ids, budget=209, seed=CS.SEED2)
    assert_same(b, M.census(db.batch, ids, 209, CS.SEED2), [names[i] for i in ids], 209)
    assert rows(a, 0) != rows(b, 0)
    c = engine.census(db, list(reversed(ids)), budget=209, seed=CS.SEED)
    for k in range(len(ids)):
        assert rows(c, len(ids) - 1 - k) == rows(a, k)


def test_search_after_a_census_gives_what_it_gave_before(engine, big, small):
    for progs, db in (big, small):
        before = engine.check(db, budget=4096, seed=CS.SEED, flags=ir.FLAG_EARLY_EXIT)
        engine.census(db, list(range(len(progs))), budget=209, seed=CS.SEED)
        after = engine.check(db, budget=4096, seed=CS.SEED, flags=ir.FLAG_EARLY_EXIT)
        assert (before.found == after.found).all()
        full0 = engine.check(db, budget=256, seed=CS.SEED, flags=0)
        engine.census(db, [0], budget=64, seed=1)
        full1 = engine.check(db, budget=256, seed=CS.SEED, flags=0)
        assert (full0.found == full1.found).all() and full0.evals_full == full1.evals_full


def test_deadline_is_reported_consistently(engine):
    """timeout_ms = 1 over a long program: the call may or may not be cut; what it reports must
    agree with itself."""
    budget = 4096
    progs = [climb_sets.long_exp(), CS.two_bounds()]
    db = engine.upload(progs)
    try:
        got = engine.census(db, [0, 1], budget=budget, seed=1, timeout_ms=1)
    finally:
        db.free()
    cut = [int(s) == ir.CENSUS_CUT for s in got.status]
    assert any(cut) == got.timed_out
    for i, c in enumerate(cut):
        if c:
            assert not got.holds[i].any() and not got.alive[i].any() and not got.sole[i].any()
            assert int(got.best_fails[i]) == int(got.best_cand[i]) == ir.CENSUS_UNKNOWN
        else:
            assert int(got.status[i]) == ir.CENSUS_DONE
            assert int(got.alive[i][-1]) <= budget and (got.holds[i] >= got.alive[i]).all()
    if not any(cut):
        assert got.evals == 2 * budget


def test_errors_launch_nothing(engine, small):
    progs, db = small
    for kw, text in ((dict(set_ids=[0], budget=0), "pf_census_batch: budget"),
                     (dict(set_ids=[0, 3], budget=8), "pf_census_batch: set 3 out of range"),
                     (dict(set_ids=[1, 1], budget=8), "pf_census_batch: set 1 requested twice")):
        with pytest.raises(_lib.PathFeasError, match=text):
            engine.census(db, **kw)
    with pytest.raises(_lib.PathFeasError, match="out of range"):
        engine.site_counts(db, [9])
    empty = engine.census(db, [], budget=8)
    assert len(empty.status) == 0 and empty.evals == 0
    assert _lib.lib().pf_version() >= 4
    # the batch is still good
    got = engine.census(db, [2], budget=64, seed=CS.SEED)
    assert_same(got, M.census(db.batch, [2], 64, CS.SEED), ["spilled-bool-b8"], 64)


def test_explain_sets_on_the_device(engine):
    """tests/test_explain_wiring.py's two queries through gpu_check.explain_sets on the real
    engine: the satisfiable one is a witness, the other is a miss whose second pinning equality
    no candidate is alive at, and a later check_sets answers as before."""
    from dataclasses import replace

    import test_explain_wiring as W
    from mythril_amd.smt import gpu_check

    cfg = replace(gpu_check.CONFIG, budget=4096, climb_rounds=0, timeout_ms=0)
    qs = [W.sat_query(), W.blocked_query()]
    gpu_check.reset_cache()
    try:
        first = gpu_check.check_sets(qs, config=cfg)
        before = W.snapshot()
        ex = gpu_check.explain_sets(qs, cfg=cfg)
        assert W.snapshot() == before
        assert [e.outcome for e in ex] == ["witness", "miss"]
        b = next(b for b in ex[1].buckets if b.outcome == "miss" and len(b.constraints) >= 2)
        last = b.rows[len(b.constraints) - 1]
        assert not last.folded and last.alive == 0 and b.budget == 4096 and b.best_fails >= 1
        assert "y_blk" in b.nearest
        again = gpu_check.check_sets(qs, config=cfg)
        assert [m is not None for m in again] == [m is not None for m in first] == [True, False]
    finally:
        gpu_check.reset_cache()
