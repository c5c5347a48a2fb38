"""GPU: array reads with 257-512-bit indices on the MI355X — the programs of
tests/wide_index_cases.py (tens of instructions, today's opcodes only) against the oracles,
bit-exact: the smallest witness index of every search, the materialised witnesses, check_sets
and the funnel on the real engine, and the .smt2 texts through replay.
tests/test_wide_index.py proves on the CPU which cases the search answers."""

from dataclasses import replace

import coracle_py
import numpy as np
import pyoracle as O
import pytest

import oracle_engine
import wide_index_cases as W
from test_gpu_replay import _replay
from test_wide_index import CASES, NOT_FOUND_AT_DEFAULT, check_funnel

from mythril_amd import ir, seed, smtlib
from mythril_amd.engine import NOT_FOUND
from mythril_amd.lower import lower
from mythril_amd.smt import gpu_check
from mythril_amd.smt.to_dag import TermLowering, UFRegistry

pytestmark = pytest.mark.gpu

GSEED = 0x51DE_1153
FLAGS = (ir.FLAG_SHORTCIRCUIT, ir.FLAG_SHORTCIRCUIT | ir.FLAG_EARLY_EXIT)


@pytest.fixture(scope="module")
def programs():
    """One program per case, hints applied, over the register file the lowering picks."""
    out = []
    for k, (name, cs, _) in enumerate(CASES):
        lo = TermLowering(UFRegistry()).lower(cs)
        seed.apply_hints(lo.dag)
        out.append(lower(lo.dag, seed=gpu_check._set_seed(cs), name=name))
    return out


def _top_w(prog):
    return max([i.dst for i in prog.code if i.op < ir.B_CONST and i.op not in (ir.W_SPILL, ir.END)], default=0)


def test_register_files(programs):
    """Every case but one runs the 8-register kernels; the free-key journal the r16 pair."""
    by = {p.name: _top_w(p) for p in programs}
    assert by.pop("free_key_journal") >= ir.NW_NARROW
    assert all(t < ir.NW_NARROW for t in by.values()), by


@pytest.mark.parametrize("flags", FLAGS, ids=["late", "early"])
@pytest.mark.parametrize("budget", [4096, 100])
def test_first_witness_equals_the_oracle(engine, programs, budget, flags):
    """One upload of all cases (the free-key journal among them: its batch runs the r16
    kernels) and one of the narrow programs alone (the 8-register kernels): ``found`` is the C
    oracle's first witness index, and pf_materialize gives the oracle's values for it."""
    for progs in (programs, [p for p in programs if _top_w(p) < ir.NW_NARROW]):
        batch = ir.Batch(progs)
        packed = coracle_py.Packed(batch)
        want = [packed.first_sat(s, GSEED, budget) for s in range(len(progs))]
        db = engine.upload(batch)
        try:
            res = engine.check(db, budget=budget, seed=GSEED, flags=flags)
            got = [None if f == NOT_FOUND else int(f) for f in res.found]
            assert got == want, [(p.name, g, w) for p, g, w in zip(progs, got, want) if g != w]
            hit = [s for s, f in enumerate(got) if f is not None]
            vals = engine.materialize(db, hit, [got[s] for s in hit], GSEED)
        finally:
            db.free()
        for s, v in zip(hit, vals):
            sv = O.SetView.from_batch(batch, s)
            ref = [int(x) for x in sv.gen_assignments(np.array([got[s]], dtype=np.uint64), GSEED)[0]]
            assert v == ref and sv.evaluate(ref), progs[s].name
        label = {c[0]: c[2] for c in CASES}
        assert not [progs[s].name for s in hit if label[progs[s].name] == "unsat"]
        if budget == 4096:
            assert len(hit) >= 10


def _answers(cfg):
    gpu_check.reset_cache()
    before = gpu_check.STATS.recheck_failures
    ms = gpu_check.check_sets([cs for _, cs, _ in CASES], registry=UFRegistry(), config=cfg)
    assert gpu_check.STATS.recheck_failures == before
    gpu_check.reset_cache()
    return [None if m is None else (m.origin, dict(m.w.vars), dict(m.w.bools), dict(m.w.reads)) for m in ms]


def test_check_sets_equals_the_oracle_engine(engine, monkeypatch):
    cfg = replace(gpu_check.CONFIG, recheck_union=True, workers=1)
    gpu = _answers(cfg)
    oracle_engine.install(monkeypatch)
    ora = _answers(cfg)
    assert gpu == ora
    for (name, cs, label), a in zip(CASES, gpu):
        assert (a is not None) == (label == "sat" and name not in NOT_FOUND_AT_DEFAULT), name


def test_replay_of_the_smt2_texts(engine, tmp_path, monkeypatch):
    import mythril_amd.engine as E

    for name, cs, _ in CASES:
        (tmp_path / f"{name}.smt2").write_text(smtlib.write_query(cs))
    gpu, gpu_launches = _replay(engine, str(tmp_path))
    ora_eng = oracle_engine.OracleEngine()
    monkeypatch.setattr(E, "get_engine", lambda device=None: ora_eng)
    ora, ora_launches = _replay(ora_eng, str(tmp_path))
    assert gpu == ora and gpu_launches == ora_launches and gpu_launches
    cls = {r["file"][:-5]: r["class"] for r in gpu[:-1]}
    label = {c[0]: c[2] for c in CASES}
    assert set(cls.values()) == {"sat", "unknown"} and len(cls) == len(CASES)
    assert not [n for n, c in cls.items() if c == "sat" and label[n] == "unsat"]
    assert sum(c == "sat" for c in cls.values()) >= 10


def test_funnel_on_the_device(engine, monkeypatch):
    import fake_z3 as z3
    import mythril_standin
    from mythril_amd import integration

    ns = mythril_standin.install(monkeypatch, z3)
    gpu_check.reset_cache()
    integration._BATCH_CACHE.clear()
    check_funnel(ns, z3)
    gpu_check.reset_cache()
