"""CPU: gpu_check.explain_sets and ``replay --explain``, end to end on the oracle-backed engine
whose ``census`` is the contract's model (tests/census_model.py), as ClimbOracleEngine's
``climb`` is the climb's."""

import copy
import os
from dataclasses import replace

import pytest

import test_climb_wiring as W
from census_model import CensusOracleEngine
from mythril_amd import replay, smtlib
from mythril_amd.smt import gpu_check
from mythril_amd.smt import terms as T

BUDGET = 128


@pytest.fixture
def eng(monkeypatch):
    W.host_keccak(monkeypatch)
    e = CensusOracleEngine()
    import mythril_amd.engine as E

    monkeypatch.setattr(E, "get_engine", lambda device=None: e)
    monkeypatch.setattr(gpu_check.CONFIG, "workers", 1)
    gpu_check.reset_cache()
    yield e
    gpu_check.reset_cache()


def cfg():
    return replace(gpu_check.CONFIG, budget=BUDGET, climb_rounds=0, timeout_ms=0)


def sat_query():
    x = T.var("x_sat", 256)
    return [T.eq(x, T.const(5, 256))]


def blocked_query():
    """No witness: y is pinned to two values; a third conjunct that most candidates pass."""
    y, z = T.var("y_blk", 256), T.var("z_blk", 8)
    return [T.cmp("bvult", z, T.const(200, 8)), T.eq(T.binop("bvadd", y, T.const(1, 256)), T.const(78, 256)),
            T.eq(y, T.const(99, 256))]


def snapshot():
    s = gpu_check.STATS
    return (copy.deepcopy({k: v for k, v in vars(s).items()}), list(gpu_check._CACHE.items()),
            list(gpu_check._NEG.items()), list(gpu_check._RECENT_VARS.items()),
            [(k, list(v.items())) for k, v in gpu_check._RECENT_READS.items()])


def test_planted_contradiction_names_a_pinning_equality(eng):
    c, unsat = W.wiring_corpus()
    two = [(cs, o, r) for cs, o, r in unsat if o.startswith("contra:two-values")]
    assert two
    cs, origin, reg = min(two, key=lambda t: len(smtlib.write_query(t[0])))
    pins = set(cs[-2:])                     # labelled_unsat appends the two pinning equalities
    ex = gpu_check.explain_sets([cs], registry=reg, cfg=cfg())[0]
    assert ex.outcome == "miss", (origin, [b.outcome for b in ex.buckets])
    missed = [b for b in ex.buckets if b.outcome == "miss"]
    assert len(eng.census_calls) == 1 and len(eng.census_calls[0][0]) == len(missed)
    assert eng.census_calls[0][1:] == (BUDGET, cfg().seed, 0)
    named = [r for b in missed for r in b.blocking() if r.term in pins and r.alive == 0]
    assert named, origin
    for b in missed:
        assert b.budget == BUDGET and b.best_fails >= 1 and 0 <= b.best_cand < BUDGET
        assert len(b.rows) >= len(b.constraints)           # the conjuncts, then the side constraints
        assert [r.term for r in b.rows[:len(b.constraints)]] == list(b.constraints)
        assert all(r.term is None for r in b.rows[len(b.constraints):])
        for r in b.rows:
            assert r.folded or (0 <= r.alive <= r.holds <= BUDGET and r.sole <= BUDGET)
        # the nearest miss shows values of symbols its failing conjuncts read, and only those
        assert b.nearest
    pinned = [b for b in missed if pins & set(b.constraints)]
    assert pinned and all(any(t.op in ("var", "bvar") and t.val in b.nearest
                              for p in pins & set(b.constraints) for t in gpu_check._subterms(p))
                          for b in pinned)


def test_a_sat_query_reports_witness_and_no_census(eng):
    ex = gpu_check.explain_sets([sat_query(), blocked_query()], cfg=cfg())
    assert ex[0].outcome == "witness" and [b.outcome for b in ex[0].buckets] == ["witness"]
    assert ex[0].buckets[0].rows == []
    assert ex[1].outcome == "miss"
    # one census call, over the missed buckets only
    assert len(eng.census_calls) == 1
    n_missed = sum(b.outcome == "miss" for b in ex[1].buckets)
    assert len(eng.census_calls[0][0]) == n_missed >= 1
    b = next(b for b in ex[1].buckets if b.outcome == "miss" and len(b.constraints) >= 2)   # y's bucket
    last = b.rows[len(b.constraints) - 1]
    assert not last.folded and last.alive == 0
    eng.census_calls.clear()
    assert gpu_check.explain_sets([sat_query()], cfg=cfg())[0].outcome == "witness"
    assert eng.census_calls == []


def test_explaining_changes_no_cache_and_no_later_answer(eng):
    qs = [sat_query(), blocked_query()]
    first = gpu_check.check_sets(qs, config=cfg())
    assert first[0] is not None and first[1] is None
    before = snapshot()
    launches = eng.launches
    gpu_check.explain_sets(qs, cfg=cfg())
    assert eng.launches > launches                  # it did search
    assert snapshot() == before
    again = gpu_check.check_sets(qs, config=cfg())
    assert (again[0] is not None, again[1]) == (True, None)
    assert again[0].w.vars == first[0].w.vars
    # ... and from cold caches: explaining first leaves nothing behind that answers for the search
    gpu_check.reset_cache()
    cold = snapshot()
    gpu_check.explain_sets(qs, cfg=cfg())
    assert snapshot()[1:] == cold[1:]
    fresh = gpu_check.check_sets(qs, config=cfg())
    assert fresh[0] is not None and fresh[1] is None and fresh[0].w.vars == first[0].w.vars


def test_replay_explain_writes_reports_for_undischarged_dumps_only(eng, tmp_path):
    d = tmp_path / "dumps"
    os.makedirs(d)
    for name, cs in (("q000", sat_query()), ("q001", blocked_query())):
        (d / f"{name}.smt2").write_text(smtlib.write_query(cs))
    out = tmp_path / "why"
    plain = replay.replay_dir(str(d), config=cfg(), workers=1)
    assert not out.exists() and eng.census_calls == []          # without the flag: as before
    rc = replay.main([str(d), "--budget", str(BUDGET), "--workers", "1", "--explain", str(out),
                      "--out", str(tmp_path / "report.jsonl")])
    assert rc == 0
    assert sorted(os.listdir(out)) == ["q001.explain.txt"]
    text = (out / "q001.explain.txt").read_text()
    assert text.startswith("q001.smt2: miss") and "alive        0" in text and "y_blk" in text
    assert "nearest y_blk = 0x" in text
    assert all(len(line) < 2 * replay.EXPLAIN_TERM_CHARS for line in text.splitlines())
    rows = [line for line in text.splitlines() if line.startswith("  alive")]
    keys = [(int(r.split()[1]), int(r.split()[3])) for r in rows]
    assert rows and keys == sorted(keys)                          # by alive, then sole
    # the answers are the plain replay's
    import json

    lines = [json.loads(x) for x in (tmp_path / "report.jsonl").read_text().splitlines()]
    assert [(x["file"], x["class"]) for x in lines[:-1]] == [(f.name, f.cls) for f in plain.files]
    assert [f.cls for f in plain.files] == ["sat", "unknown"]
