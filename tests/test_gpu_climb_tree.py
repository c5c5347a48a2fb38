"""GPU: pf_climb_batch_scored with PF_CLIMB_SCORE_TREE (Engine.climb(score="tree")) returns
what the tree score's CPU model (tests/climb_tree_model.py) returns — status, score, round and
values, exactly (the values are the chosen candidate's, so its index is compared with them) —
on the hand-made sets of tests/climb_tree_sets.py and tests/bool_file_cases.py, whose premises
tests/test_climb_tree_model.py asserts on the CPU, and on the buckets a small corpus' search
leaves.  Each call is at most 8 rounds of 256 candidates."""

from dataclasses import replace

import pytest

import bool_file_cases as C
import climb_model as CM
import climb_tree_model as TM
import climb_tree_sets as TS
from mythril_amd import _lib, corpus, ir
from mythril_amd.smt import gpu_check
from test_climb_tree_model import COMPARE_ROWS, LOGIC_ROWS
from test_gpu_climb import ints

pytestmark = pytest.mark.gpu


def both(engine, progs, set_ids, rounds, per_round, seed, score="tree"):
    db = engine.upload(progs)
    try:
        got = engine.climb(db, set_ids, rounds, per_round, seed=seed, score=score)
    finally:
        db.free()
    return got, TM.climb(db.batch, set_ids, rounds, per_round, seed, score)


def assert_same(got, want, names):
    assert len(got.status) == len(want)
    for i, (w, name) in enumerate(zip(want, names)):
        dev = (int(got.status[i]), int(got.score[i]), int(got.round[i]), ints(got.values[i]))
        assert dev == (w.status, w.score, w.round, w.values), name
    assert got.evals == sum(w.evals for w in want)
    assert not got.timed_out


def table_progs():
    """The table programs on the 8-register kernel and (base 8: W registers 8 and above) on the
    16-register one, with the saturating AND / OR."""
    progs = []
    for base in (0, 8):
        progs += TS.table_sets(base) + [TS.saturation_set(ir.B_AND, base=base), TS.saturation_set(ir.B_OR, base=base)]
    for k, p in enumerate(progs):
        p.seed = 3 + k
    return progs


@pytest.mark.parametrize("rounds", [1, 3])
@pytest.mark.parametrize("per_round", [64, 100, 192])
def test_table_programs(engine, per_round, rounds):
    """per_round 100: the lanes past it post nothing; 192: three waves, ties to the smallest
    index.  One call of 8 sets mixing both register files."""
    progs = table_progs()
    ids = list(range(len(progs)))
    got, want = both(engine, progs, ids, rounds, per_round, 0x7EE5 + per_round)
    assert_same(got, want, [p.name for p in progs])
    assert all(int(s) == ir.CLIMB_NONE for s, p in zip(got.status, progs) if p.name.startswith("table:"))


def test_every_row_for_explicit_values(engine):
    """The CPU test's rows as candidate 0 (the parent model) of one-round, one-candidate climbs:
    the device's score of exactly those operands; B registers 0 and 31."""
    progs = []
    for k, (op, w, a, b, _) in enumerate(COMPARE_ROWS):
        progs.append(TS.compare_row(op, w, a, b, base=8 * (k % 2), bd=31 * (k % 2), fused=k % 3 != 0))
    regs = ((3, 0, 31, 7), (31, 0, 1, 2), (0, 0, 31, 30), (31, 30, 31, 0))
    for k, (op, x, y, c, _) in enumerate(LOGIC_ROWS):
        progs.append(TS.logic_row(op, (x[0], x[1], y[0], y[1], c[0]), regs[k % 4], base=8 * (k % 2)))
    for lo in range(0, len(progs), 12):          # uploads below PF_FOLD_MIN_SETS: nothing is folded away
        chunk = progs[lo:lo + 12]
        ids = list(range(len(chunk)))
        got, want = both(engine, chunk, ids, 1, 1, 5)
        assert_same(got, want, [p.name for p in chunk])
        devs = CM.device_sets(ir.Batch(chunk))
        for i, p in enumerate(chunk):
            assert ints(got.values[i]) == p.assignment                 # candidate 0 is the parent model
            assert int(got.score[i]) == TM.tree_score(devs[i], p.assignment)


def test_batches_of_one_and_nine(engine):
    progs = table_progs()
    got, want = both(engine, progs[:1], [0], 3, 128, 41)
    assert_same(got, want, [progs[0].name])
    nine = progs + [TS.family()[0]]
    assert len(nine) == 9
    ids = [8, 3, 0, 7, 5, 1, 6, 2, 4]
    got, want = both(engine, nine, ids, 3, 128, 41)
    assert_same(got, want, [nine[i].name for i in ids])


@pytest.mark.parametrize("per_round", [64, 100])
def test_bool_spills_keep_their_pair(engine, per_round):
    """Scratch slots 0 and 63 and LDS entries, a W_EXP or a B_UMUL_NOOVF between spill and
    fill, a slot a W_SPILL wrote before, both register files; lower()'s own spills under more
    than 32 live Bools."""
    progs = [C.bspill_set(v, 0x5A5AC33C ^ rot, base=base, rot=rot)
             for v in C.SPILL_VARIANTS for base, rot in ((0, 0), (8, 1), (0, 3))]
    progs += [C.fused_all(0), C.fused_all(8)]
    progs += [C.pressure_program(n)[1] for n in ("p40/free/narrow", "p64x/free/r16", "p90x/free/narrow")]
    for lo in range(0, len(progs), 7):
        chunk = progs[lo:lo + 7]
        got, want = both(engine, chunk, list(range(len(chunk))), 3, per_round, 0xB5)
        assert_same(got, want, [p.name for p in chunk])


def test_the_family_is_witnessed_under_the_tree_score_only(engine):
    progs = TS.family()
    ids = list(range(len(progs)))
    got, want = both(engine, progs, ids, TS.ROUNDS, TS.PER_ROUND, TS.SEED)
    assert_same(got, want, [p.name for p in progs])
    assert got.sat.all() and all(int(r) >= 1 for r in got.round)
    for p, v in zip(progs, got.values):
        assert tuple(ints(v)) in [tuple(f) for f in p.solution]
    sites, swant = both(engine, progs, ids, TS.ROUNDS, TS.PER_ROUND, TS.SEED, score="sites")
    assert_same(sites, swant, [p.name for p in progs])
    assert not sites.sat.any() and not sites.score.any()


def test_the_buckets_a_small_search_leaves(engine, monkeypatch):
    """corpus.build(6, 2, seed=2024), budget 1,024, hints off: every climb call check_sets
    makes with climb_score="tree" at 4 x 128 returns the model's climb of the same batch."""
    calls = []
    real = engine.climb

    def checking(db, set_ids, rounds, per_round, seed=0, timeout_ms=0, score="sites"):
        got = real(db, set_ids, rounds, per_round, seed=seed, timeout_ms=timeout_ms, score=score)
        dbs = list(db) if isinstance(db, (list, tuple)) else [db]
        assert len(dbs) == 1 and (rounds, per_round, score) == (4, 128, "tree")
        want = TM.climb(dbs[0].batch, set_ids, rounds, per_round, seed, score)
        assert_same(got, want, [f"bucket {s}" for s in set_ids])
        calls.append(len(set_ids))
        return got

    monkeypatch.setattr(engine, "climb", checking, raising=False)
    cfg = replace(gpu_check.CONFIG, budget=1024, hints=False, climb_rounds=4, climb_candidates=128,
                  climb_score="tree")
    c = corpus.build(6, 2, seed=2024)
    gpu_check.reset_cache()
    before = replace(gpu_check.STATS)
    try:
        models = gpu_check.check_sets([q.constraints for q in c.queries], registry=c.kfm.registry, config=cfg)
    finally:
        gpu_check.reset_cache()
    assert calls and sum(calls) == gpu_check.STATS.climbed - before.climbed
    assert gpu_check.STATS.recheck_failures == before.recheck_failures
    assert all(m is None or m.origin in ("climb", "search", "hint", "parent", "first", "cache") for m in models)


def test_an_unknown_score_is_refused(engine):
    db = engine.upload([TS.family()[0]])
    try:
        with pytest.raises(_lib.PathFeasError, match="pf_climb_batch: unknown score 7"):
            engine.climb(db, [0], 2, 64, score=7)
        # nothing was launched and the batch is still good, under either score
        assert int(engine.climb(db, [0], 1, 64, score=ir.CLIMB_SCORE_TREE).status[0]) == ir.CLIMB_NONE
        assert int(engine.climb(db, [0], 1, 64).status[0]) == ir.CLIMB_NONE
    finally:
        db.free()
