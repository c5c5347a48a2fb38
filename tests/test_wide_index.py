"""CPU: array reads with 257-512-bit indices (EIP-1153 transient storage reads) through both
lowerings, the search on the C oracle engine (tests/oracle_engine.py), the explicit-model
programs, the .smt2 reader and replay, the witness views and the funnel.  The cases are those
of tests/wide_index_cases.py; tests/test_gpu_wide_index.py runs them on the MI355X.

Before array indices were carried as chunks every case here raised LoweringError ("array
index wider than 256 bits")."""

import os
import random
from dataclasses import replace

import numpy as np
import pytest

import oracle_engine
import pyoracle as O
import wide_index_cases as W
from test_native_terms import _compare_dag, _compare_program

from mythril_amd import ir, model_cache, replay, smtlib
from mythril_amd.lower import lower
from mythril_amd.smt import gpu_check
from mythril_amd.smt import native_terms as NT
from mythril_amd.smt import terms as T
from mythril_amd.smt.interp import Witness
from mythril_amd.smt.to_dag import ExplicitLowering, TermLowering, UFRegistry

CASES = W.cases() + [("free_key_journal", W.free_key_journal(), "sat")]
IDS = [c[0] for c in CASES]
# SAT, but the search does not reach it at the default budget (the stored slot has to equal
# the read one for a value deep in the chain to show): lowering and evaluation checks only
NOT_FOUND_AT_DEFAULT = {"base_over_journal"}
native = pytest.mark.skipif(NT.store() is None, reason="libpflower.so not built")


def searched(label):
    return [c for c in CASES if c[2] == label and c[0] not in NOT_FOUND_AT_DEFAULT]


# ---- the lowerings ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,cs,label", CASES, ids=IDS)
def test_lowers(name, cs, label):
    """The feature's own test: every case lowers (no LoweringError), to a program whose
    variables are generic (no calldata-byte or actor hints from a wide-index read)."""
    lo = TermLowering(UFRegistry()).lower(cs)
    for v in lo.dag.vars:
        assert v.kind in (ir.VK_GENERIC, ir.VK_BOOL) and v.hint0 == 0 and v.hint1 == 0, v
    lower(lo.dag, seed=1).validate()


@native
@pytest.mark.parametrize("name,cs,label", CASES, ids=IDS)
def test_native_lowering_is_identical(name, cs, label):
    reg = UFRegistry()
    assert _compare_dag(cs, reg) is not None
    _compare_program(cs, reg, hints=True)
    _compare_program(cs, reg, hints=False)


@native
def test_native_lowering_with_parents():
    """Parents by symbol name (a 512-bit symbol's chunks) and by the read's own select term."""
    name, cs, _ = next(c for c in CASES if c[0] == "base_const_index")
    lo = TermLowering(UFRegistry()).lower(cs)
    parent = {"X": (0xAFFE << 256) | 9}
    parent.update({t: 77 + k for k, t in enumerate(lo.var_terms) if t.op == "select"})
    assert len(parent) == 3
    assert _compare_dag(cs, UFRegistry(), parent) is not None
    _compare_program(cs, UFRegistry(), parent, hints=True)


def test_structural_shortcuts():
    """Concats that differ in a constant part are never compared; a chunk both keys share is
    left out of the compare; the generic chunked ``=`` is what is left."""
    def n_eq(cs):
        lo = TermLowering(UFRegistry()).lower(cs)
        return sum(n.kind == ir.B_EQ for n in lo.dag.nodes), lo
    by = {c[0]: c[1] for c in CASES}
    # another contract's store / another constant slot: no index compare at all (the one B_EQ
    # is the constraint's own, on the read value)
    assert n_eq(by["chunks_addr_const"])[0] == 1 and n_eq(by["chunks_slot_const"])[0] == 1
    # Concat(A1, i) against Concat(A1, j): the address chunk is one node, the slots compare
    k, lo = n_eq(by["one_store_hit"])
    assert k == 3 and not any(n.kind == ir.B_AND for n in lo.dag.nodes)
    # Concat(a, i) against Concat(b, i): the slot chunk is one node, the addresses compare
    k, lo = n_eq(by["chunks_addr_sym"])
    assert k == 3 and not any(n.kind == ir.B_AND for n in lo.dag.nodes)
    # free 512-bit keys: both chunks under B_AND
    lo = TermLowering(UFRegistry()).lower(by["journal3_free_key"])
    assert any(n.kind == ir.B_AND for n in lo.dag.nodes)
    # indices of 256 bits and fewer lower as before: offsets of one base never alias
    x = T.var("x", 256)
    arr = T.store(T.const_array(256, W.ZERO), T.binop("bvadd", x, T.const(1, 256)), W.v)
    lo = TermLowering(UFRegistry()).lower([W.ne(T.select(arr, T.binop("bvadd", x, T.const(2, 256))), W.ZERO)])
    assert not lo.dag.vars


def test_array_values_past_256_bits_still_refuse():
    from mythril_amd.lower import LoweringError

    arr = T.store(T.const_array(512, T.const(0, 512)), W.X, T.var("Y", 512))
    c = T.eq(T.select(arr, W.key(W.A1, W.i)), T.const(0, 512))
    with pytest.raises(LoweringError):
        TermLowering(UFRegistry()).lower([c])
    if NT.store() is not None:
        assert _compare_dag([c], UFRegistry()) is None      # the same refusal natively
    # one array name declared at two index widths: refused, not compared chunk against node
    two = [T.eq(T.select(T.array("ts", 512, 256), W.X), W.v), T.eq(T.select(T.array("ts", 256, 256), W.i), W.w)]
    with pytest.raises(LoweringError, match="two index widths"):
        TermLowering(UFRegistry()).lower(two)
    if NT.store() is not None:
        assert _compare_dag(two, UFRegistry()) is None


# ---- the search on the C oracle engine -------------------------------------------------------
@pytest.fixture
def oracle(monkeypatch):
    eng = oracle_engine.install(monkeypatch)
    yield eng
    gpu_check.reset_cache()


def _check(cs_list, **kw):
    gpu_check.reset_cache()
    before = gpu_check.STATS.recheck_failures
    ms = gpu_check.check_sets(cs_list, registry=UFRegistry(), config=replace(gpu_check.CONFIG, **kw))
    assert gpu_check.STATS.recheck_failures == before
    return ms


def test_sat_cases_get_a_rechecked_witness(oracle):
    sat = searched("sat")
    assert len(sat) >= 14
    ms = _check([cs for _, cs, _ in sat], recheck_union=True)
    for (name, cs, _), m in zip(sat, ms):
        assert m is not None, name
        assert all(m.w.ev(c) for c in cs), name


def test_unsat_cases_get_no_witness(oracle):
    unsat = [c for c in CASES if c[2] == "unsat"]
    assert len(unsat) >= 11
    sets = [cs for _, cs, _ in unsat]
    assert _check(sets) == [None] * len(sets)
    for sd in (1, 2, 3):
        assert _check(sets, budget=4096, seed=sd) == [None] * len(sets), sd


def test_witness_entries_are_named_by_the_512_bit_index(oracle):
    name, cs, _ = next(c for c in CASES if c[0] == "base_const_index")
    lo = TermLowering(UFRegistry()).lower(cs)
    k = (5 << 256) | 7
    assert [v.name for v in lo.dag.vars][:1] == [f"ts[{k}]"] and "ts@1" in [v.name for v in lo.dag.vars]
    m = _check([cs])[0]
    tab = m.w.tables()["ts"]
    assert tab[k] == 3 and tab[m.w.vars["X"]] == 4 and m.w.vars["X"] != k


# ---- the lowering against the term evaluator ---------------------------------------------------
_SMALL = (0, 1, 2, 3, 5, 6, 7)
_ADDR = (W.A1.val, W.A2.val, 9)


def _assignment(lo, rng, forced):
    """One value per program variable.  ``forced``: the index symbols are equal (i = j, a = b,
    every free key the key most cases store at) and the stored values come from a small pool."""
    slot, addr = rng.choice(_SMALL), rng.choice(_ADDR)
    out = []
    for v, t in zip(lo.dag.vars, lo.var_terms):
        if not forced:
            out.append(rng.choice(_SMALL) if rng.random() < 0.25 else rng.getrandbits(v.width))
        elif v.name in ("i", "j"):
            out.append(slot)
        elif v.name in ("a", "b"):
            out.append(addr)
        elif v.name.endswith("#0"):
            out.append(rng.choice((slot, 1, 2)))
        elif v.name.endswith("#1"):
            out.append(rng.choice((addr, W.A1.val, W.A1.val + 1)))
        else:
            out.append(rng.choice(_SMALL) & ir.mask(v.width))
    return out


@pytest.mark.parametrize("name,cs,label", CASES, ids=IDS)
def test_program_equals_the_term_evaluator(name, cs, label):
    """256 assignments, half random and half with the index variables forced equal: the
    lowered program (pyoracle) and smt/interp.py on the terms give one verdict — a dropped
    chunk or a wrong store order shows here."""
    reg = UFRegistry()
    lo = TermLowering(reg).lower(cs)
    sv = O.SetView.from_batch(ir.Batch([lower(lo.dag, seed=3)]), 0)
    rng = random.Random(zlib_seed(name))
    conj = T.and_(*cs)
    holds = 0
    for n in range(256):
        vals = _assignment(lo, rng, forced=n % 2 == 1)
        want = bool(Witness(lo, vals, reg).ev(conj))
        assert bool(sv.evaluate(vals)) == want, (name, n, [hex(x) for x in vals])
        holds += want
    if label == "unsat":
        assert holds == 0, (name, holds)


def zlib_seed(name):
    import zlib

    return zlib.crc32(name.encode())


# ---- explicit-model programs (model_cache / pf_eval_programs) -----------------------------------
@pytest.mark.parametrize("name,cs,label", CASES, ids=IDS)
def test_explicit_programs_equal_the_conjunction(name, cs, label):
    eng = oracle_engine.OracleEngine()
    reg = UFRegistry()
    conj = T.and_(*cs)
    leaves_py, prog_py = model_cache.lower_explicit_py(cs)
    leaves, prog = model_cache._lower_explicit(cs)
    assert list(leaves) == list(leaves_py)
    b1, b2 = ir.Batch([prog_py]), ir.Batch([prog])
    for part in ("code", "consts", "schema", "descs"):
        assert np.array_equal(getattr(b1, part), getattr(b2, part)), part
    # a read of the base array is a leaf: the select term itself, whatever the index width
    for t in leaves:
        assert t.op in ("var", "extract") or (t.op == "select" and t.args[0].op == "array"), t
    lo = TermLowering(reg).lower(cs)
    rng = random.Random(zlib_seed(name) + 1)
    ws = [Witness(lo, _assignment(lo, rng, forced=n % 2 == 1), reg) for n in range(64)]
    rows = model_cache.rows_of_ints([[int(w.ev(t)) for t in leaves] for w in ws])
    want = [bool(w.ev(conj)) for w in ws]
    assert model_cache.eval_rows(prog, rows, eng).tolist() == want
    # the same through pf_eval_programs' packing (several programs of one call)
    pack = tuple(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1) for a in (b2.code, b2.consts, b2.schema, b2.descs))
    soa = model_cache.soa_of(rows, max(1, len(leaves))) if leaves else model_cache.soa_of(rows, 0)
    assert eng.eval_programs(pack, soa)[0].tolist() == want


def test_explicit_leaf_of_a_wide_read():
    ts = T.array("ts", 512, 256)
    r = T.select(T.store(ts, W.key(W.A1, W.i), W.v), W.key(W.A1, W.j))
    lo = ExplicitLowering().lower([T.eq(r, W.ZERO)])
    assert T.select(ts, W.key(W.A1, W.j)) in lo.var_terms


# ---- .smt2 texts and replay ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def smt2_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("wide_smt2")
    for name, cs, _ in CASES:
        (d / f"{name}.smt2").write_text(smtlib.write_query(cs))
    return str(d)


def test_smt2_texts_read_back(smt2_dir):
    text = open(os.path.join(smt2_dir, "journal8_offset_key.smt2")).read()
    assert "(declare-fun X () (_ BitVec 512))" in text and "(let (" in text
    assert "((as const (Array (_ BitVec 512) (_ BitVec 256)))" in text
    assert "(declare-fun ts () (Array (_ BitVec 512) (_ BitVec 256)))" in open(
        os.path.join(smt2_dir, "base_equal_unsat.smt2")).read()
    for name, cs, _ in CASES:
        q = smtlib.read_query(open(os.path.join(smt2_dir, name + ".smt2")).read())
        assert len(q.assertions) == len(cs) and all(x is y for x, y in zip(q.assertions, cs)), name


def test_replay_answers_the_smt2_texts(smt2_dir, oracle, tmp_path):
    models = str(tmp_path / "models")
    rep = replay.replay_dir(smt2_dir, config=replace(gpu_check.CONFIG, timeout_ms=0), models_dir=models, workers=1)
    cls = {f.name[:-5]: f.cls for f in rep.files}
    want = {name: ("sat" if label == "sat" and name not in NOT_FOUND_AT_DEFAULT else "unknown")
            for name, _, label in CASES}
    assert cls == want and rep.recheck_failures == 0
    # the certificate of a base-array witness pins its reads at 512-bit indices
    text = open(os.path.join(models, "base_const_index.model.smt2")).read()
    q = smtlib.read_query(text)
    pins = [c for c in q.assertions[2:] if c.op == "=" and c.args[0].op == "select"]
    assert len(pins) == 2 and all(p.args[0].args[1].op == "bv" and p.args[0].args[1].width == 512 for p in pins)
    assert {p.args[0].args[1].val: p.args[1].val for p in pins}[(5 << 256) | 7] == 3
    reg = smtlib.recover_registry(q.assertions)
    assert reg.keccak == {} and not reg.recovery.problems(reg)


# ---- the facade ------------------------------------------------------------------------------------
def test_facade_arrays_with_concat_keys(oracle):
    from mythril_amd.smt import Array, Concat, K, Solver, sat, symbol_factory

    BVV, BV = symbol_factory.BitVecVal, symbol_factory.BitVecSym
    addr, slot, val = BVV(W.A1.val, 256), BV("slot", 256), BV("val", 256)
    ts = K(512, 256, 0)
    assert ts.raw is W.K0
    ts[Concat(addr, slot)] = val
    assert ts.raw is T.store(W.K0, T.concat(W.A1, slot.raw), val.raw)
    read = ts[Concat(addr, BVV(3, 256))]
    assert read.raw.width == 256 and read.raw.op == "select"
    s = Solver()
    s.add(read == BVV(8, 256))
    assert s.check() == sat
    m = s.model()
    assert m.eval(slot.raw).as_long() == 3 and m.eval(val.raw).as_long() == 8 and m.eval(read.raw).as_long() == 8
    base = Array("ts", 512, 256)
    assert base.raw is T.array("ts", 512, 256) and base[Concat(addr, slot)].raw.args[1].width == 512
    s = Solver()
    s.add(base[Concat(addr, slot)] == BVV(5, 256))
    assert s.check() == sat and s.model().eval(base[Concat(addr, slot)].raw).as_long() == 5


# ---- the funnel ---------------------------------------------------------------------------------------
def funnel_fork(ns, z3):
    """``TLOAD; ISZERO; JUMPI`` over a two-store journal, in z3 expressions as LASER builds
    them: (the lock word, the two successors' constraint lists)."""
    bv = lambda n: z3.BitVec(n, 256)            # noqa: E731
    A1 = z3.BitVecVal(W.A1.val, 256)
    ts = z3.K(z3.BitVecSort(512), z3.BitVecVal(0, 256))
    ts = z3.Store(ts, z3.Concat(A1, z3.BitVecVal(0, 256)), bv("v"))
    ts = z3.Store(ts, z3.Concat(A1, bv("i")), bv("w"))
    lock = z3.Select(ts, z3.Concat(A1, z3.BitVecVal(0, 256)))
    pre = ns.Bool(z3.ULT(z3.BitVecVal(0, 256), bv("i")))
    zero = z3.BitVecVal(0, 256)
    return lock, [ns.Constraints([pre, ns.Bool(lock == zero)]), ns.Constraints([pre, ns.Bool(lock != zero)])]


def check_funnel(ns, z3):
    """Both successors answered by the engine, counted by gpu_sat, and the returned Models
    evaluate the read as the branch says."""
    from mythril_amd import integration
    from mythril_amd.smt.solver import SolverStatistics

    integration.install()
    st = SolverStatistics()
    before = st.gpu_sat
    lock, (taken, fallen) = funnel_fork(ns, z3)
    m0 = ns.funnel.get_model(taken)
    m1 = ns.funnel.get_model(fallen)
    assert st.gpu_sat - before == 2
    assert m0.eval(lock, model_completion=True).as_long() == 0
    assert m1.eval(lock, model_completion=True).as_long() != 0
    assert m1.eval(z3.BitVec("i", 256), model_completion=True).as_long() > 0


def test_funnel_answers_both_successors(monkeypatch):
    import fake_z3 as z3
    import mythril_standin
    from mythril_amd import integration
    from mythril_amd.smt.solver import SolverStatistics

    ns = mythril_standin.install(monkeypatch, z3)
    oracle_engine.install(monkeypatch)
    monkeypatch.setattr(gpu_check.CONFIG, "budget", 4096)
    integration._BATCH_CACHE.clear()
    st = SolverStatistics()
    st.gpu_sat = st.gpu_attempts = 0
    check_funnel(ns, z3)
    gpu_check.reset_cache()
