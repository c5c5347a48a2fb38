"""CPU: GpuConfig.climb_score from check_sets down to Engine.climb, on the oracle-backed engine
whose ``climb`` honours ``score`` (tests/climb_tree_model.py).  The default configuration makes
the calls it makes today; "tree" reaches the engine, keys its own negative entries, and its
witnesses pass the host re-check and carry the origin "climb"."""

from dataclasses import replace

import pytest

import climb_model as CM
import climb_tree_model as TM
from mythril_amd import ir
from mythril_amd.smt import gpu_check
from mythril_amd.smt import terms as T
from test_climb_wiring import BUDGET, CANDIDATES, QUERIES, ROUNDS, host_keccak, wiring_corpus


@pytest.fixture
def eng(monkeypatch):
    host_keccak(monkeypatch)
    e = TM.TreeOracleEngine()
    import mythril_amd.engine as E

    monkeypatch.setattr(E, "get_engine", lambda device=None: e)
    monkeypatch.setattr(gpu_check.CONFIG, "workers", 1)
    gpu_check.reset_cache()
    yield e
    gpu_check.reset_cache()


def test_the_default_configuration_makes_the_calls_it_makes_today(monkeypatch, eng):
    """climb_score defaults to "sites", and then Engine.climb is called without ``score`` — an
    engine whose climb does not know the argument (the sites model's) still serves."""
    monkeypatch.delenv("PF_CLIMB_SCORE", raising=False)
    assert gpu_check.GpuConfig().climb_score == "sites" and gpu_check.GpuConfig().climb_rounds == 0
    seen = []

    def old_climb(db, set_ids, rounds, per_round, seed=0, timeout_ms=0):      # no ``score``
        seen.append((len(set_ids), rounds, per_round, seed, timeout_ms))
        return CM.ClimbOracleEngine.climb(eng, db, set_ids, rounds, per_round, seed, timeout_ms)

    eng.climb = old_climb
    c, _ = wiring_corpus()
    qs = [q.constraints for q in c.queries[QUERIES]]
    cfg_off = replace(gpu_check.CONFIG, budget=BUDGET, hints=False, climb_rounds=0, climb_score="sites")
    gpu_check.check_sets(qs, registry=c.kfm.registry, config=cfg_off)
    assert seen == []
    # climb off: the score changes nothing, not even the negative key
    assert gpu_check._neg_key(("k",), cfg_off) == gpu_check._neg_key(("k",), replace(cfg_off, climb_score="tree"))
    gpu_check.reset_cache()
    cfg_on = replace(cfg_off, climb_rounds=ROUNDS, climb_candidates=CANDIDATES)
    gpu_check.check_sets(qs, registry=c.kfm.registry, config=cfg_on)
    assert seen and all(s[1:4] == (ROUNDS, CANDIDATES, cfg_on.seed) for s in seen)
    sites_calls = [x[:5] for x in eng.climb_calls]
    assert sites_calls == seen


def test_tree_reaches_the_engine_and_its_witnesses_are_rechecked(eng):
    c, _ = wiring_corpus()
    queries = c.queries[QUERIES]
    qs = [q.constraints for q in queries]
    cfg_off = replace(gpu_check.CONFIG, budget=BUDGET, hints=False, climb_rounds=0)
    off = gpu_check.check_sets(qs, registry=c.kfm.registry, config=cfg_off)
    gpu_check.reset_cache()
    cfg = replace(cfg_off, climb_rounds=ROUNDS, climb_candidates=CANDIDATES, climb_score="tree")
    before = replace(gpu_check.STATS)
    on = gpu_check.check_sets(qs, registry=c.kfm.registry, config=cfg)
    assert eng.climb_calls and all(call[1:] == (ROUNDS, CANDIDATES, cfg.seed, 0, "tree") for call in eng.climb_calls)
    climb_sat = gpu_check.STATS.climb_sat - before.climb_sat
    assert gpu_check.STATS.recheck_failures == before.recheck_failures
    assert sum(n for n, *_ in eng.climb_calls) == gpu_check.STATS.climbed - before.climbed
    gained = [i for i, (m0, m1) in enumerate(zip(off, on)) if m0 is None and m1 is not None]
    assert climb_sat > 0 and gained
    for i, (q, m0, m1) in enumerate(zip(queries, off, on)):
        assert m0 is None or m1 is not None
        if m1 is not None:
            assert all(m1.w.ev(t) for t in q.constraints if t is not T.TRUE), q.origin
    assert all(on[i].origin == "climb" for i in gained)


def test_the_negative_key_separates_the_two_scores(eng):
    cfg_sites = replace(gpu_check.CONFIG, budget=64, hints=False, climb_rounds=1, climb_candidates=8,
                        climb_score="sites")
    cfg_tree = replace(cfg_sites, climb_score="tree")
    assert gpu_check._neg_key(("k",), cfg_sites) != gpu_check._neg_key(("k",), cfg_tree)
    c, _ = wiring_corpus()
    qs = [q.constraints for q in c.queries][:6]
    gpu_check.check_sets(qs, registry=c.kfm.registry, config=cfg_sites)
    n0 = eng.launches
    assert [x[5] for x in eng.climb_calls] == ["sites"]
    gpu_check.check_sets(qs, registry=c.kfm.registry, config=cfg_sites)
    assert eng.launches == n0 and len(eng.climb_calls) == 1            # negative under "sites"
    gpu_check.check_sets(qs, registry=c.kfm.registry, config=cfg_tree)
    assert eng.launches == n0 + 1 and [x[5] for x in eng.climb_calls] == ["sites", "tree"]
    gpu_check.check_sets(qs, registry=c.kfm.registry, config=cfg_tree)
    assert eng.launches == n0 + 1 and len(eng.climb_calls) == 2        # and now under "tree" too
    gpu_check.check_sets(qs, registry=c.kfm.registry, config=cfg_sites)
    assert eng.launches == n0 + 1 and len(eng.climb_calls) == 2


def test_engine_climb_rejects_an_unknown_score_name():
    with pytest.raises(ValueError, match="climb score"):
        ir.climb_score_id("forest")
    assert ir.climb_score_id("sites") == ir.CLIMB_SCORE_SITES == 0
    assert ir.climb_score_id("tree") == ir.CLIMB_SCORE_TREE == 1


def test_the_tools_take_the_score(monkeypatch, tmp_path, capsys):
    from mythril_amd import replay

    seen = []

    def fake(path, config=None, models_dir=None, workers=None):
        seen.append(config)
        return replay.ReplayReport()

    monkeypatch.setattr(replay, "replay_dir", fake)
    assert replay.main([str(tmp_path), "--climb", "4:64", "--climb-score", "tree"]) == 0
    assert (seen[-1].climb_rounds, seen[-1].climb_candidates, seen[-1].climb_score) == (4, 64, "tree")
    assert replay.main([str(tmp_path), "--climb", "4:64"]) == 0
    assert seen[-1].climb_score == gpu_check.CONFIG.climb_score
    with pytest.raises(SystemExit):
        replay.main([str(tmp_path), "--climb-score", "forest"])
    capsys.readouterr()


def test_the_census_counts_sites_by_their_writer():
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        import assert_site_census as A
    finally:
        sys.path.pop(0)
    import climb_tree_sets as TS

    progs = [TS.family_set("not-ult"), TS.family_set("or-eq"), TS.compare_row(ir.B_ULT, 256, 9, 3)]
    batch = ir.Batch(progs)
    devs = CM.device_sets(batch)
    assert [ir.OPNAMES[op] for _, op in A.site_writers(devs[0])] == ["B_NOT"]
    assert [ir.OPNAMES[op] for _, op in A.site_writers(devs[2])] == ["B_ULT"]
    all_sites, failing, buckets, flat, evals = A.census([batch], n_cand=16)
    assert dict(all_sites) == {"B_NOT": 1, "B_OR": 1, "B_ULT": 1} and buckets == 3 and evals == 48
    assert failing["B_NOT"] == 16 and failing["B_OR"] == 16 and flat == 2
    text = A.table(all_sites, failing, buckets, flat, evals, 16, "three sets")
    assert "| `B_OR` | 1 |" in text and "2 of 3" in text
