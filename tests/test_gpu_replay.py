"""GPU: solver-log dumps from files on the MI355X (mythril_amd/replay.py) — the reader's terms
feed the device.  Parity form: the same directories on the C oracle engine
(tests/oracle_engine.py) give the same classes, witness values and smallest witness indices in
every launch; the command line, as a fresh process, gives the same JSON lines."""

import json
import os
import shutil
import subprocess
import sys

import pytest

import oracle_engine
from conftest import ROOT
from mythril_amd import corpus, replay
from test_replay import GOLDEN_SMT2, config, keccak_sat_queries, write_dir

pytestmark = pytest.mark.gpu


def _replay(eng, d):
    """replay_dir on ``eng``: (comparable JSON records, per-launch smallest witness indices)."""
    launches = []
    orig = eng.check

    def check(db, *a, **k):
        r = orig(db, *a, **k)
        launches.append(r.found.tolist())
        return r

    eng.check = check
    try:
        rep = replay.replay_dir(d, config=config(), workers=1)
    finally:
        eng.check = orig
    assert rep.recheck_failures == 0
    return [_comparable(json.loads(ln)) for ln in rep.json_lines()], launches


def _comparable(rec):
    if "totals" in rec:
        return {k: rec["totals"][k] for k in ("files", "sat", "unknown", "objective", "error", "groups")}
    rec.pop("ms")
    return rec


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """The directory of tests/test_replay.py's test 3 plus the committed z3-style files."""
    c = corpus.build(n_scenarios=8)
    d = write_dir(tmp_path_factory.mktemp("dumps"), [q.constraints for q in keccak_sat_queries(c)])
    for n in os.listdir(GOLDEN_SMT2):
        shutil.copy(os.path.join(GOLDEN_SMT2, n), d)
    return d


@pytest.fixture(scope="module")
def on_device(engine, dumps):
    return _replay(engine, dumps)


def test_replay_on_device_equals_oracle(engine, dumps, on_device, monkeypatch):
    import mythril_amd.engine as E

    gpu, gpu_launches = on_device
    ora_eng = oracle_engine.OracleEngine()
    monkeypatch.setattr(E, "get_engine", lambda device=None: ora_eng)
    ora, ora_launches = _replay(ora_eng, dumps)
    assert gpu == ora
    assert gpu_launches == ora_launches and len(gpu_launches) >= 2
    cls = {r["file"]: r["class"] for r in gpu[:-1]}
    assert len(cls) == 37 and cls["minimize.smt2"] == "objective"
    assert sum(c == "sat" for c in cls.values()) >= 30 and not any(c.startswith("error") for c in cls.values())


def test_command_line_as_a_fresh_process(dumps, on_device, tmp_path):
    out = tmp_path / "answers.jsonl"
    env = dict(os.environ, PF_TORCH="0")
    p = subprocess.run([sys.executable, "-m", "mythril_amd.replay", dumps, "--out", str(out), "--budget", "4096",
                        "--timeout-ms", "0", "--workers", "2", "--models", str(tmp_path / "models")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [_comparable(json.loads(ln)) for ln in out.read_text().splitlines()]
    assert lines == on_device[0]
    assert json.loads(p.stdout.splitlines()[-1])["totals"]["sat"] == lines[-1]["sat"]
    sat = [r["file"] for r in lines[:-1] if r["class"] == "sat"]
    assert sorted(os.listdir(tmp_path / "models")) == sorted(n[:-5] + ".model.smt2" for n in sat)
