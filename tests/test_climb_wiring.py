"""CPU: check_sets with the climb switched on, end to end on the oracle-backed engine whose
``climb`` is the contract's model (tests/climb_model.py).  The GPU run of the same checks on
the real engine is tests/test_gpu_climb.py::test_check_sets_with_climb_on_the_device."""

from dataclasses import replace

import pytest

import pyoracle as O
from climb_model import ClimbOracleEngine
from mythril_amd import corpus
from mythril_amd import keccak_manager as KM
from mythril_amd.smt import gpu_check, symbol_factory
from mythril_amd.smt import terms as T

# the wiring corpus and its climb: small, so that the model (pure Python; its time goes into
# pyoracle's Philox, once per variable and round) stays quick.  The CPU test runs QUERIES of the
# corpus — a stretch of the queries this search budget leaves unanswered, one of which the
# climb answers — and N_UNSAT labelled-UNSAT queries.  The GPU test runs all 142 queries and 48
# labelled-UNSAT ones through the same checks and asserts WHOLE, what the oracle-backed engine
# gives for the whole corpus (the device is bit-exact with the model, so the figures are the same).
BUDGET, ROUNDS, CANDIDATES = 1024, 4, 64
QUERIES, N_UNSAT = slice(17, 21), 10
# whole corpus: queries, answered with the climb off / on, buckets climbed, climb witnesses, and
# the queries only the climb answers
WHOLE = dict(queries=142, off=99, on=100, climbed=28, climb_sat=1, gained=[19])


def host_keccak(monkeypatch):
    monkeypatch.setattr(KM.KeccakFunctionManager, "find_concrete_keccak", staticmethod(
        lambda data: symbol_factory.BitVecVal(
            int.from_bytes(O.keccak256(data.value.to_bytes(data.size() // 8, "big")), "big"), 256)))


def wiring_corpus(n_unsat=N_UNSAT):
    c = corpus.build(6, 2, seed=11)
    return c, corpus.labelled_unsat(c, n=n_unsat, seed=5)


def run_unsat(unsat, cfg):
    """Origins of the UNSAT-labelled queries that were answered (must be none)."""
    fps = []
    for reg in {id(r): r for _, _, r in unsat}.values():
        group = [(cs, o) for cs, o, r in unsat if r is reg]
        ms = gpu_check.check_sets([cs for cs, _ in group], registry=reg, config=cfg)
        fps += [o for (cs, o), m in zip(group, ms) if m is not None]
    return fps


def check_wiring(c, unsat, cfg_off, cfg_on, eng, queries=slice(None)):
    """What both the CPU and the GPU wiring test assert, on engine ``eng`` (the one
    check_sets uses); returns (answers off, answers on, buckets climbed, buckets the climb
    answered)."""
    calls = []
    real = eng.climb

    def recording(db, set_ids, rounds, per_round, seed=0, timeout_ms=0):
        calls.append((len(set_ids), rounds, per_round, seed, timeout_ms))
        return real(db, set_ids, rounds, per_round, seed=seed, timeout_ms=timeout_ms)

    eng.climb = recording
    try:
        return _check_wiring(c, unsat, cfg_off, cfg_on, calls, queries)
    finally:
        del eng.climb


def _check_wiring(c, unsat, cfg_off, cfg_on, calls, queries):
    qs = [q.constraints for q in c.queries[queries]]
    gpu_check.reset_cache()
    off = gpu_check.check_sets(qs, registry=c.kfm.registry, config=cfg_off)
    assert calls == []                                      # climb off: nothing calls climb
    gpu_check.reset_cache()
    before = replace(gpu_check.STATS)
    on = gpu_check.check_sets(qs, registry=c.kfm.registry, config=cfg_on)
    main_calls = list(calls)
    climbed = gpu_check.STATS.climbed - before.climbed
    climb_sat = gpu_check.STATS.climb_sat - before.climb_sat
    assert gpu_check.STATS.recheck_failures == before.recheck_failures
    # a superset of the answers, and every answer a model of its query
    for q, m0, m1 in zip(c.queries[queries], off, on):
        assert m0 is None or m1 is not None, q.origin
        if m1 is not None:
            assert all(m1.w.ev(t) for t in q.constraints if t is not T.TRUE), q.origin
    # the queries only the climb answered say so, and nothing else does
    gained = [i for i, (m0, m1) in enumerate(zip(off, on)) if m0 is None and m1 is not None]
    assert all(on[i].origin == "climb" for i in gained)
    assert all(m.origin != "climb" for m in off if m is not None)
    # the climb was run over the buckets the search left, answered some of them, and those
    # answers reached the queries: more are answered than with the climb off
    assert climbed > 0 and climb_sat > 0 and gained
    assert sum(m is not None for m in on) > sum(m is not None for m in off)
    assert gpu_check.STATS.bucket_origin.get("climb", 0) >= climb_sat
    assert main_calls and sum(n for n, *_ in main_calls) == climbed
    # soundness: the UNSAT-labelled queries stay unanswered with the climb on
    gpu_check.reset_cache()
    assert run_unsat(unsat, cfg_on) == []
    gpu_check.reset_cache()
    # every climb call, of the queries and of the UNSAT-labelled ones, carried the configuration
    assert all((r, n, seed) == (cfg_on.climb_rounds, cfg_on.climb_candidates, cfg_on.seed)
               for _, r, n, seed, _ in calls)
    return off, on, climbed, climb_sat


def test_check_sets_with_climb_answers_a_superset(monkeypatch):
    host_keccak(monkeypatch)
    eng = ClimbOracleEngine()
    import mythril_amd.engine as E

    monkeypatch.setattr(E, "get_engine", lambda device=None: eng)
    monkeypatch.setattr(gpu_check.CONFIG, "workers", 1)
    cfg_off = replace(gpu_check.CONFIG, budget=BUDGET, hints=False, climb_rounds=0)
    cfg_on = replace(cfg_off, climb_rounds=ROUNDS, climb_candidates=CANDIDATES)
    c, unsat = wiring_corpus()
    check_wiring(c, unsat, cfg_off, cfg_on, eng, QUERIES)
    assert all(t == 0 for *_, t in eng.climb_calls)           # no deadline configured: none passed on


def test_the_climb_gets_what_the_search_left_of_the_deadline(monkeypatch):
    """timeout_ms bounds the call's device work as a whole: the climb's deadline is the rest of
    it, and with none left there is no climb and no negative entry."""
    host_keccak(monkeypatch)
    eng = ClimbOracleEngine()
    import mythril_amd.engine as E

    monkeypatch.setattr(E, "get_engine", lambda device=None: eng)
    monkeypatch.setattr(gpu_check.CONFIG, "workers", 1)
    c, _ = wiring_corpus()
    qs = [q.constraints for q in c.queries[:6]]
    cfg = replace(gpu_check.CONFIG, budget=64, hints=False, climb_rounds=1, climb_candidates=8,
                  timeout_ms=3_600_000)
    gpu_check.reset_cache()
    gpu_check.check_sets(qs, registry=c.kfm.registry, config=cfg)
    assert len(eng.climb_calls) == 1 and 0 < eng.climb_calls[0][4] < cfg.timeout_ms
    # a search that used the deadline up (here: a clock that jumps an hour per reading)
    import time as _time

    now = [0.0]

    def jumping():
        now[0] += 3600.0
        return now[0]

    gpu_check.reset_cache()
    with monkeypatch.context() as m:
        m.setattr(_time, "perf_counter", jumping)
        gpu_check.check_sets(qs, registry=c.kfm.registry, config=cfg)
    assert len(eng.climb_calls) == 1 and not gpu_check._NEG
    gpu_check.reset_cache()


def test_climb_off_never_calls_climb(monkeypatch):
    host_keccak(monkeypatch)
    eng = ClimbOracleEngine()
    import mythril_amd.engine as E

    monkeypatch.setattr(E, "get_engine", lambda device=None: eng)
    monkeypatch.setattr(gpu_check.CONFIG, "workers", 1)
    assert gpu_check.GpuConfig().climb_rounds == 0          # the default is off
    cfg = replace(gpu_check.CONFIG, budget=BUDGET, hints=False, climb_rounds=0, climb_candidates=CANDIDATES)
    c, _ = wiring_corpus()
    gpu_check.reset_cache()
    before = gpu_check.STATS.climbed
    ms = gpu_check.check_sets([q.constraints for q in c.queries[QUERIES]], registry=c.kfm.registry, config=cfg)
    assert eng.climb_calls == [] and gpu_check.STATS.climbed == before
    assert any(m is None for m in ms)                      # there was something to climb
    gpu_check.reset_cache()


def test_an_unanswered_bucket_is_negative_only_for_the_same_climb(monkeypatch):
    """_NEG keys carry the climb parameters: a bucket the plain search (or a shorter climb) left
    unanswered is searched again when a climb is asked for, and not again for the same one."""
    host_keccak(monkeypatch)
    eng = ClimbOracleEngine()
    import mythril_amd.engine as E

    monkeypatch.setattr(E, "get_engine", lambda device=None: eng)
    monkeypatch.setattr(gpu_check.CONFIG, "workers", 1)
    cfg_off = replace(gpu_check.CONFIG, budget=64, hints=False, climb_rounds=0)
    cfg_on = replace(cfg_off, climb_rounds=1, climb_candidates=8)
    c, _ = wiring_corpus()
    qs = [q.constraints for q in c.queries][:6]
    gpu_check.reset_cache()
    gpu_check.check_sets(qs, registry=c.kfm.registry, config=cfg_off)
    n0 = eng.launches
    gpu_check.check_sets(qs, registry=c.kfm.registry, config=cfg_off)
    assert eng.launches == n0 and eng.climb_calls == []       # negative: not searched again
    gpu_check.check_sets(qs, registry=c.kfm.registry, config=cfg_on)
    assert eng.launches == n0 + 1 and len(eng.climb_calls) == 1
    gpu_check.check_sets(qs, registry=c.kfm.registry, config=cfg_on)
    assert eng.launches == n0 + 1 and len(eng.climb_calls) == 1
    gpu_check.reset_cache()


def test_replay_climb_option(monkeypatch, tmp_path, capsys):
    """``python -m mythril_amd.replay DIR --climb ROUNDS[:CANDIDATES]`` sets the two fields."""
    from mythril_amd import replay

    seen = []

    def fake(path, config=None, models_dir=None, workers=None):
        seen.append(config)
        return replay.ReplayReport()

    monkeypatch.setattr(replay, "replay_dir", fake)
    assert replay.main([str(tmp_path), "--climb", "12:300"]) == 0
    assert (seen[-1].climb_rounds, seen[-1].climb_candidates) == (12, 300)
    assert replay.main([str(tmp_path), "--climb", "7"]) == 0
    assert (seen[-1].climb_rounds, seen[-1].climb_candidates) == (7, gpu_check.CONFIG.climb_candidates)
    assert replay.main([str(tmp_path)]) == 0
    assert seen[-1].climb_rounds == gpu_check.CONFIG.climb_rounds == 0
    for bad in ("x", "3:0", "-1"):
        with pytest.raises(SystemExit):
            replay.main([str(tmp_path), "--climb", bad])
    capsys.readouterr()
