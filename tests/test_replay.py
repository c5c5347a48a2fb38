"""CPU: solver-log dumps from files to the engine and back (mythril_amd/replay.py,
smtlib.write_query / recover_registry).  The device is the C oracle (tests/oracle_engine.py);
tests/test_gpu_replay.py runs the same directories on the MI355X."""

import os
import shutil
from dataclasses import replace

import pytest

import oracle_engine
from conftest import GOLDEN
from mythril_amd import corpus, replay, smtlib
from mythril_amd.keccak_manager import PART, KeccakFunctionManager
from mythril_amd.smt import ULT, symbol_factory
from mythril_amd.smt import gpu_check
from mythril_amd.smt import terms as T
from mythril_amd.smt.to_dag import ACTORS, UFRegistry

BVV = symbol_factory.BitVecVal
BV = symbol_factory.BitVecSym
BUDGET = 4096
GOLDEN_SMT2 = os.path.join(GOLDEN, "smt2")


def config():
    return replace(gpu_check.CONFIG, budget=BUDGET, timeout_ms=0)


def keccak_sat_queries(c, n=32):
    """The first ``n`` sat-labelled corpus queries that apply a keccak function."""
    return [q for q in c.queries if q.label == "sat" and "keccak256_" in smtlib.write_query(q.constraints)][:n]


def write_dir(path, sets, stem="q"):
    os.makedirs(path, exist_ok=True)
    for i, cs in enumerate(sets):
        with open(os.path.join(path, f"{stem}{i:03d}.smt2"), "w") as f:
            f.write(smtlib.write_query(cs))
    return str(path)


@pytest.fixture(scope="module")
def corp():
    """corpus.build(n_scenarios=8) (its concrete hashes by the oracle's Keccak-256), built once."""
    mp = pytest.MonkeyPatch()
    oracle_engine.install(mp)
    try:
        c = corpus.build(n_scenarios=8)
    finally:
        mp.undo()
    return c


# ---- 1. recovery ---------------------------------------------------------------------------
def _manager_query():
    kfm = KeccakFunctionManager(UFRegistry())
    a, b = BV("a", 256), BV("b", 256)
    s, t = BV("s", 512), BV("t", 512)
    hs = [kfm.create_keccak(BVV(7, 256)), kfm.create_keccak(BVV(1 << 200, 256)),
          kfm.create_keccak(BVV((0xAFFE << 256) | 2, 512))]
    fa, fb, fs, ft = (kfm.create_keccak(x) for x in (a, b, s, t))
    cs = [ULT(a, BVV(100, 256)).raw, (fa != fb).raw, (fs != ft).raw, (fa != hs[0]).raw,
          kfm.create_conditions().raw]
    return kfm, cs


def test_recovery_is_exact(monkeypatch):
    oracle_engine.install(monkeypatch)
    kfm, cs = _manager_query()
    q = smtlib.read_query(smtlib.write_query(cs))
    assert all(x is y for x, y in zip(q.assertions, cs))
    reg = smtlib.recover_registry(q.assertions)
    assert set(reg.keccak) == set(kfm.registry.keccak) == {256, 512}
    for n, spec in kfm.registry.keccak.items():
        assert reg.keccak[n].lo == spec.lo and spec.lo is not None
        assert reg.keccak[n].concrete == spec.concrete and spec.concrete
    assert sum(len(s.concrete) for s in reg.keccak.values()) == 3
    assert reg.actors == ACTORS
    assert reg.recovery.symbolic == {256: 2, 512: 2}
    assert not reg.recovery.ambiguous and not reg.recovery.dropped and not reg.recovery.problems(reg)


def test_recovery_drops_a_wrong_hash_and_an_ambiguous_width(monkeypatch):
    oracle_engine.install(monkeypatch)
    kfm, cs = _manager_query()
    f = lambda x: T.apply("keccak256_256", 256, x)  # noqa: E731
    wrong = T.eq(f(T.const(9, 256)), T.const(12345, 256))           # not the Keccak-256 of 9
    reg = smtlib.recover_registry(cs + [wrong])
    assert reg.keccak[256].concrete == kfm.registry.keccak[256].concrete
    assert reg.recovery.dropped == [(256, 9, 12345)]
    # a second interval for width 256 on another input: the width stays unrecovered, 512 does not
    c = T.var("c", 256)
    lo2 = kfm.registry.keccak[256].lo - 5 * PART
    other = T.and_(T.cmp("bvule", T.const(lo2, 256), f(c)), T.cmp("bvult", f(c), T.const(lo2 + PART, 256)))
    reg = smtlib.recover_registry(cs + [other])
    assert 256 not in reg.keccak and reg.keccak[512].lo == kfm.registry.keccak[512].lo
    assert reg.recovery.ambiguous == {256: sorted([lo2, kfm.registry.keccak[256].lo])}
    assert any("ambiguous" in p for p in reg.recovery.problems(reg))
    # an upper bound that is not lo + PART is no interval
    off = T.and_(T.cmp("bvule", T.const(lo2, 256), f(c)), T.cmp("bvult", f(c), T.const(lo2 + PART + 1, 256)))
    assert smtlib.recover_registry(cs + [off]).keccak[256].lo == kfm.registry.keccak[256].lo
    # only the inverse function, or nothing: no entry
    inv = T.eq(T.apply("keccak256_64-1", 64, T.var("h", 256)), T.const(3, 64))
    assert smtlib.recover_registry([inv, ULT(BV("a", 256), BVV(5, 256)).raw]).keccak == {}


# ---- 2. round trip ---------------------------------------------------------------------------
def test_round_trip_gives_identical_terms(corp):
    total = 0
    for q in corp.queries:
        text = smtlib.write_query(q.constraints)
        total += len(text)
        back = smtlib.read_query(text).assertions
        assert len(back) == len(q.constraints)
        assert all(x is y for x, y in zip(back, q.constraints)), q.origin
    print(f"write_query: {total / len(corp.queries):.0f} bytes per dump over {len(corp.queries)} queries")
    x, y = T.var("a!1", 8), T.var("1 odd/name", 8)   # a let-like name and one that needs quotes
    sh = T.binop("bvadd", x, y)
    c = T.eq(T.binop("bvmul", sh, sh), T.const(5, 8))
    text = smtlib.write_query([c], minimize=[x], maximize=[sh])
    q = smtlib.read_query(text)
    assert q.assertions[0] is c and q.minimize == [x] and q.maximize == [sh]
    assert "(let ((a!!1 " in text and text.endswith("(check-sat)\n")
    assert "(_ bv5 7)" in smtlib.write_query([T.eq(T.var("z", 7), T.const(5, 7))])


# ---- 3 / 4. from files equals in memory; soundness ---------------------------------------------
@pytest.fixture(scope="module")
def replayed(corp, tmp_path_factory):
    """The directory of test 3, replayed once on the oracle engine (certificates included)."""
    mp = pytest.MonkeyPatch()
    oracle_engine.install(mp)
    try:
        qs = keccak_sat_queries(corp)
        d = write_dir(tmp_path_factory.mktemp("dumps"), [q.constraints for q in qs])
        rep = replay.replay_dir(d, config=config(), models_dir=os.path.join(d, "models"), workers=1)
    finally:
        mp.undo()
    return qs, d, rep


def test_from_files_equals_in_memory(corp, replayed, monkeypatch):
    oracle_engine.install(monkeypatch)
    qs, d, rep = replayed
    assert len(qs) == 32 and [f.name for f in rep.files] == sorted(n for n in os.listdir(d) if n.endswith(".smt2"))
    sat_files = {i for i, f in enumerate(rep.files) if f.cls == "sat"}
    mem = {}
    for i, q in enumerate(qs):     # in memory, each under its own file's recovered registry
        gpu_check.reset_cache()
        m = gpu_check.check_sets([q.constraints], registry=rep.files[i].registry, config=config())[0]
        if m is not None:
            mem[i] = (dict(m.w.vars), dict(m.w.bools))
    assert sat_files == set(mem)
    for i in sat_files:
        w = rep.files[i].model.w
        assert (dict(w.vars), dict(w.bools)) == mem[i]
    gpu_check.reset_cache()
    empty = gpu_check.check_sets([q.constraints for q in qs], registry=UFRegistry(), config=config())
    gpu_check.reset_cache()
    final = gpu_check.check_sets([q.constraints for q in qs], registry=corp.kfm.registry, config=config())
    gpu_check.reset_cache()
    n_empty, n_final = sum(m is not None for m in empty), sum(m is not None for m in final)
    print(f"sat of 32: from files {len(sat_files)}, empty registry {n_empty}, the corpus' final registry {n_final}")
    assert len(sat_files) > n_empty
    assert rep.recheck_failures == 0 and rep.count("error") == 0
    assert rep.discharged_share == len(sat_files) / 32 and rep.files_per_s > 0
    assert set(rep.phase_s) == set(replay.PHASES)


def test_soundness(corp, replayed, tmp_path, monkeypatch):
    oracle_engine.install(monkeypatch)
    qs, d, rep = replayed
    for f in rep.files:
        if f.cls == "sat":         # under the assertions read from the file (= the query's own terms)
            assert all(f.model.w.ev(c) for c in f.query.assertions)
    unsat = corpus.labelled_unsat(corp, n=32)[:32]
    rep2 = replay.replay_dir(write_dir(tmp_path, [cs for cs, _, _ in unsat]), config=config(), workers=1)
    assert len(rep2.files) == 32 and rep2.count("sat") == 0, [f.name for f in rep2.files if f.cls == "sat"]


# ---- 5. classification -------------------------------------------------------------------------
def test_classification(corp, replayed, tmp_path, monkeypatch):
    eng = oracle_engine.install(monkeypatch)
    qs, d, rep = replayed
    only = tmp_path / "only"
    write_dir(only, [])
    shutil.copy(os.path.join(GOLDEN_SMT2, "minimize.smt2"), only)
    r = replay.replay_dir(str(only), config=config(), workers=1)
    assert [f.cls for f in r.files] == ["objective"] and eng.launches == 0 and r.discharged_share == 0.0

    mixed = tmp_path / "mixed"
    names = sorted(n for n in os.listdir(d) if n.endswith(".smt2"))[:6]
    write_dir(mixed, [])
    for n in names:
        shutil.copy(os.path.join(d, n), mixed)
    text = open(os.path.join(d, names[0])).read()
    (mixed / "broken.smt2").write_text(text[:len(text) // 2])
    (mixed / "objective.smt2").write_text(text.replace("(check-sat)", "(minimize call_value1)\n(check-sat)"))
    r = replay.replay_dir(str(mixed), config=config(), workers=2)     # read in worker processes
    by = {f.name: f for f in r.files}
    assert by["broken.smt2"].cls.startswith("error:") and by["objective.smt2"].cls == "objective"
    want = {f.name: (f.cls, f.values()) for f in rep.files}
    assert all((by[n].cls, by[n].values()) == want[n] for n in names)
    assert any(by[n].cls == "sat" for n in names)

    renamed = tmp_path / "renamed"
    write_dir(renamed, [])
    new = {n: f"{(7 * i + 3) % len(names):02d}_{n[:-5][::-1]}.smt2" for i, n in enumerate(names)}
    for n in names:
        shutil.copy(os.path.join(d, n), renamed / new[n])
    r = replay.replay_dir(str(renamed), config=config(), workers=1)
    by = {f.name: f for f in r.files}
    assert all((by[new[n]].cls, by[new[n]].values()) == want[n] for n in names)


def test_missing_interval_is_an_error(tmp_path, monkeypatch):
    """A width with symbolic inputs and no (or no single) recovered interval: error, no search."""
    eng = oracle_engine.install(monkeypatch)
    f = T.apply("keccak256_256", 256, T.var("x", 256))
    write_dir(tmp_path, [[T.cmp("bvult", f, T.const(1 << 255, 256))]])
    r = replay.replay_dir(str(tmp_path), config=config(), workers=1)
    assert r.files[0].cls.startswith("error: keccak256_256: no interval") and eng.launches == 0


# ---- 6. certificates -----------------------------------------------------------------------------
class _Pinned(corpus._PlantedEval):
    """Evaluation under a certificate's pins alone: symbols, array tables, UF points."""

    def __init__(self, vars_, arrays, points, registry):
        super().__init__(corpus.Planted(vars_, arrays), registry)
        self.points = points

    def _apply(self, t):
        key = (t.val[0], tuple(int(self._evr(a)) for a in t.args))
        return self.points[key] if key in self.points else super()._apply(t)


def _pins(extra):
    vars_, bools, arrays, points = {}, {}, {}, {}
    for e in extra:
        assert e.op in ("=", "iff"), e
        a, b = e.args
        if a.op == "var":
            vars_[a.val] = b.val
        elif a.op == "bvar":
            bools[a.val] = b is T.TRUE
        elif a.op == "select":
            assert a.args[0].op == "array" and a.args[1].op == "bv"
            arrays.setdefault(a.args[0].val, {})[a.args[1].val] = b.val
        else:
            assert a.op == "apply" and all(x.op == "bv" for x in a.args) and b.op == "bv", e
            points[(a.val[0], tuple(x.val for x in a.args))] = b.val
    return vars_, bools, arrays, points


def test_certificates(replayed):
    qs, d, rep = replayed
    n = 0
    for f in rep.files:
        if f.cls != "sat":
            assert f.certificate is None
            continue
        assert f.certificate == os.path.join(d, "models", f.name[:-5] + ".model.smt2")
        text = open(f.certificate).read()
        assert text.startswith(open(os.path.join(d, f.name)).read().replace("(check-sat)\n", ""))
        assert text.count("(check-sat)") == 1 and text.endswith("(check-sat)\n")
        q = smtlib.read_query(text)
        k = len(f.query.assertions)
        assert all(x is y for x, y in zip(q.assertions[:k], f.query.assertions))
        vars_, bools, arrays, points = _pins(q.assertions[k:])
        w = f.model.w
        assert {x: v for x, v in w.vars.items() if x in vars_} == {x: v for x, v in vars_.items() if x in w.vars}
        assert set(w.vars) <= set(vars_) and set(vars_) == {x for x, (dm, r) in q.decls.items() if not dm and r[0] == "bv"}
        assert arrays == {a: t for a, t in w.tables().items() if t}
        assert points and all(int(w.ev(app)) == points[(fn, tuple(int(w.ev(a)) for a in args))]
                              for fn, args, app in w.uf_apps)
        ev = _Pinned(vars_, arrays, points, f.registry)
        ev.bools = bools
        assert all(ev.ev(c) for c in f.query.assertions), f.name
        n += 1
    assert n > 0


# ---- the committed z3-style files ----------------------------------------------------------------
def test_golden_files(monkeypatch):
    oracle_engine.install(monkeypatch)
    names = sorted(os.listdir(GOLDEN_SMT2))
    assert 4 <= len(names) <= 6 and all(os.path.getsize(os.path.join(GOLDEN_SMT2, n)) < 8192 for n in names)
    rep = replay.replay_dir(GOLDEN_SMT2, config=config(), workers=1)
    cls = {f.name: f.cls for f in rep.files}
    assert cls == {"calldata_let.smt2": "sat", "concrete_or.smt2": "sat", "interval_let.smt2": "sat",
                   "minimize.smt2": "objective", "two_widths.smt2": "sat"}
    regs = {f.name: f.registry for f in rep.files if f.registry is not None}
    assert regs["calldata_let.smt2"].keccak == {}
    assert regs["interval_let.smt2"].keccak[256].lo == regs["concrete_or.smt2"].keccak[256].lo
    assert sorted(regs["concrete_or.smt2"].keccak[256].concrete) == [1, 0xDEADBEEF]
    two = regs["two_widths.smt2"].keccak
    assert two[512].lo == regs["interval_let.smt2"].keccak[256].lo and two[256].lo not in (None, two[512].lo)
    assert rep.groups == 4
