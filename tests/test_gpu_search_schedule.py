"""GPU: the layer around the interpreter — which candidates a search evaluates and what it
reports about them — against the oracle, bit-exact (no tolerance anywhere).

``geometry()`` / ``check_enqueue()`` (pathfeas.hip) cut ``[0, budget)`` into per-wave slices,
chunks and the probe's first group; ``search_item`` / ``check_body`` (pf_eval.hip) mask the
ragged tail and count.  The tests run budgets that are no multiple of 64, budgets at and
around a set's first witness, the probe hand-off at candidate 64, both register files in one
batch, and hold ``found`` and the three counters of ``pf_stats`` to search_counters.py (the
contract of DESIGN.md §5).  The last section calls the C-ABI entry points nothing else does.

The oracle masks are computed once per module (coracle_py, about two seconds per 96 sets)."""

import copy
import ctypes
import functools

import numpy as np
import pytest
import search_counters as SC
from test_gpu_parity import _pressure_program

from mythril_amd import _lib, ir, synth
from mythril_amd.lower import lower

pytestmark = pytest.mark.gpu

COUNT_OPS, SHORT, EARLY, NO_PROBE = ir.FLAG_COUNT_OPS, ir.FLAG_SHORTCIRCUIT, ir.FLAG_EARLY_EXIT, ir.FLAG_NO_PROBE
ROWS = [pytest.param(COUNT_OPS, id="count_ops"), pytest.param(SHORT, id="shortcircuit"),
        pytest.param(EARLY, id="early"), pytest.param(EARLY | SHORT, id="early_shortcircuit")]
EARLY_ROWS = ROWS[2:]

SEED_A, N_CAND_A = 0x5EED_0F_5CA1E, 4160
SEED_B, BUDGET_B = 0x5EED_0042, 2048
FIXED_BUDGETS = (0, 1, 2, 63, 64, 65, 66, 100, 127, 128, 129, 191, 1000, 4095, 4097)


def assert_row(res, masks, budget, flags, aux1, what):
    """found, timed_out and the counter row of ``flags`` (search_counters.py)."""
    n, total = len(masks), len(masks) * budget
    want = SC.found(masks, budget)
    bad = np.flatnonzero(res.found != want)
    assert bad.size == 0, (what, budget, flags, [(int(s), int(res.found[s]), int(want[s])) for s in bad[:6]])
    assert not res.timed_out, (what, budget, flags)
    got = (res.cands_decided, res.evals_full, res.ops)
    if not flags & EARLY:
        assert res.cands_decided == total, (what, budget, flags, got)
        full = SC.shortcircuit_evals_full(masks, budget) if flags & SHORT else total
        assert res.evals_full == full, (what, budget, flags, got, full)
        if flags & COUNT_OPS and not flags & SHORT:
            assert res.ops == budget * sum(aux1), (what, budget, flags, got, budget * sum(aux1))
    else:
        floor = SC.early_exit_floor(masks, budget)
        assert floor <= res.cands_decided <= total, (what, budget, flags, got, floor, total)
        if flags & SHORT:
            assert res.evals_full <= res.cands_decided, (what, budget, flags, got)
        else:
            assert res.evals_full == res.cands_decided, (what, budget, flags, got)
        unwitnessed = bool((want == SC.NOT_FOUND).all())
        if budget <= 64 or unwitnessed:
            assert res.cands_decided == total, (what, budget, flags, got)
        if unwitnessed and flags & SHORT:
            assert res.evals_full == 0, (what, budget, flags, got)
    if not flags & COUNT_OPS:
        assert res.ops == 0, (what, budget, flags, got)
    return n


# ---- A. config-3 sets, not parented -------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sets_a():
    progs = [synth.random_dag_set(20_000 + 7 * i, plant=False)[0] for i in range(96)]
    batch = ir.Batch(progs)
    masks = SC.sat_masks(batch, SEED_A, N_CAND_A)
    return progs, masks, SC.aux1_totals(batch)


@functools.lru_cache(maxsize=None)
def witness_budgets_a():
    """f and f + 1 for five sets whose first witness f is at or above 64 (the smallest, the
    largest and three between, from the oracle)."""
    fs = sorted({f for f in (SC.first_witness(m, N_CAND_A) for m in sets_a()[1]) if f is not None and f >= 64})
    assert len(fs) >= 5, fs
    pick = [fs[round(k * (len(fs) - 1) / 4)] for k in range(5)]
    return sorted({b for f in pick for b in (f, f + 1)})


@pytest.fixture(scope="module")
def db_a(engine):
    db = engine.upload(sets_a()[0])
    yield db
    db.free()


def test_oracle_first_witnesses_cover_every_kind():
    """The selection the cases below rest on: sets without a witness, with one at candidate
    0, inside the first group, and beyond it (so a budget cuts through them)."""
    fs = [SC.first_witness(m, N_CAND_A) for m in sets_a()[1]]
    assert sum(f is None for f in fs) >= 8 and sum(f == 0 for f in fs) >= 8
    assert sum(f is not None and 0 < f < 64 for f in fs) >= 8
    assert sum(f is not None and f >= 64 for f in fs) >= 5


@pytest.mark.parametrize("flags", ROWS)
@pytest.mark.parametrize("budget", FIXED_BUDGETS)
def test_ragged_budgets(engine, db_a, budget, flags):
    """Budgets around the group size, the per-wave slice and the chunk: no witness at or past
    the budget, none missed below it, and every counter of the row."""
    _, masks, aux1 = sets_a()
    assert_row(engine.check(db_a, budget=budget, seed=SEED_A, flags=flags), masks, budget, flags, aux1, "A")


@pytest.mark.parametrize("flags", ROWS)
def test_budget_at_and_past_a_witness(engine, db_a, flags):
    """budget = f hides the witness at f, budget = f + 1 shows it: the last candidate of a
    search is evaluated, the one after it is not."""
    _, masks, aux1 = sets_a()
    res = {}
    for budget in witness_budgets_a():
        res[budget] = engine.check(db_a, budget=budget, seed=SEED_A, flags=flags)
        assert_row(res[budget], masks, budget, flags, aux1, "A witness")
    n_edges = 0
    for s, m in enumerate(masks):       # the edge itself, spelled out
        f = SC.first_witness(m, N_CAND_A)
        if f is not None and f >= 64 and f in res and f + 1 in res:
            assert res[f].found[s] == SC.NOT_FOUND and res[f + 1].found[s] == f, (s, f)
            n_edges += 1
    assert n_edges >= 5


@pytest.mark.parametrize("budget", [100, 1000])
def test_ops_stay_zero_without_count_ops(engine, db_a, budget):
    _, masks, aux1 = sets_a()
    res = engine.check(db_a, budget=budget, seed=SEED_A, flags=0)
    assert_row(res, masks, budget, 0, aux1, "A plain")
    assert res.ops == 0 and res.evals_full == res.cands_decided == 96 * budget


# ---- B. parented batches that take the probe ----------------------------------------------

def _shifted(p):
    p = copy.deepcopy(p)
    for v in p.vars:
        if v.parent is not None:
            v.parent = (v.parent + 1) & ((1 << v.width) - 1)
    return p


@functools.lru_cache(maxsize=None)
def sets_b():
    """96 planted sets with every parent value shifted by one (candidate 0 no longer the
    planted witness) and 49 untouched ones, each with its oracle mask over the budget."""
    planted = [synth.random_dag_set(500 + i, plant=True)[0] for i in range(96)]
    shifted = [_shifted(p) for p in planted]
    assert all(p.has_parent for p in planted + shifted)
    ms = SC.sat_masks(ir.Batch(shifted), SEED_B, BUDGET_B)
    mp = SC.sat_masks(ir.Batch(planted[:49]), SEED_B, BUDGET_B)
    assert mp[:, 0].all()                                   # the planted witness is candidate 0
    return shifted, ms, planted[:49], mp


def _run_b(engine, progs, masks, budgets, flags, what):
    db = engine.upload(progs)
    aux1 = SC.aux1_totals(db.batch)
    out = []
    for budget in budgets:
        res = engine.check(db, budget=budget, seed=SEED_B, flags=flags)
        assert_row(res, masks, budget, flags, aux1, what)
        out.append(res)
    db.free()
    return out


@pytest.mark.parametrize("flags", EARLY_ROWS)
def test_probe_batch_without_witnesses_counts_every_candidate_once(engine, flags):
    """16..64 parented sets, none with a witness in budget: the probe evaluates candidates
    0..63, the search behind it 64..budget - 1 — n * budget decided in all, none twice, and
    with SHORTCIRCUIT no group runs to END."""
    shifted, ms, _, _ = sets_b()
    keep = [s for s, m in enumerate(ms) if SC.first_witness(m, BUDGET_B) is None][:64]
    assert len(keep) >= 16, len(keep)
    (res,) = _run_b(engine, [shifted[s] for s in keep], ms[keep], [BUDGET_B], flags, "B none")
    assert res.cands_decided == len(keep) * BUDGET_B
    assert res.evals_full == (0 if flags & SHORT else len(keep) * BUDGET_B)


@pytest.mark.parametrize("flags", EARLY_ROWS)
def test_probe_hand_off_at_candidate_64(engine, flags):
    """Up to 64 parented sets: those whose first witness is at or above 64 (the search behind
    the probe finds it) padded with untouched planted sets (the probe decides them).  Budgets
    one past the probe's group, at and past three witnesses in 64..127, and 2047; the same
    answers with PF_FLAG_NO_PROBE."""
    shifted, ms, planted, mp = sets_b()
    late = [s for s, m in enumerate(ms) if (SC.first_witness(m, BUDGET_B) or 0) >= 64]
    assert len(late) >= 8, late
    n_pad = 64 - len(late)
    progs = [shifted[s] for s in late] + planted[:n_pad]
    masks = np.concatenate([ms[late], mp[:n_pad]])
    fs = sorted({SC.first_witness(ms[s], BUDGET_B) for s in late} & set(range(64, 128)))
    assert len(fs) >= 3, fs
    near = [fs[0], fs[len(fs) // 2], fs[-1]]
    budgets = sorted({65, 2047} | {b for f in near for b in (f, f + 1)})
    with_probe = _run_b(engine, progs, masks, budgets, flags, "B hand-off")
    without = _run_b(engine, progs, masks, budgets, flags | NO_PROBE, "B hand-off, no probe")
    for budget, r0, r1 in zip(budgets, with_probe, without):
        assert np.array_equal(r0.found, r1.found), budget


@pytest.mark.parametrize("flags", EARLY_ROWS)
def test_probe_decides_a_planted_batch_in_one_group_per_set(engine, flags):
    _, _, planted, mp = sets_b()
    (res,) = _run_b(engine, planted[:32], mp[:32], [1000], flags, "B planted")
    assert (res.found == 0).all()
    assert res.cands_decided == 64 * 32, res.cands_decided


# ---- C. both register files in one batch ---------------------------------------------------

def _dag_of(dag_id):
    got = {}
    orig = synth.lower
    synth.lower = lambda dag, **k: got.setdefault("dag", dag) and orig(dag, **k)
    try:
        synth.random_dag_set(dag_id, plant=False)
    finally:
        synth.lower = orig
    return got["dag"]


def _max_w_written(prog):
    code = ir.Batch([prog]).code.reshape(-1, 4)
    ops = code[:, 0] & 0xFF
    w_res = (ops < ir.B_CONST) & (ops != ir.END) & (ops != ir.W_SPILL)
    return int((code[w_res, 1] & 0xFF).max())


@functools.lru_cache(maxsize=None)
def sets_c():
    """40 narrow sets of A with 8 sets lowered over 15 registers at positions 1, 3, .. 15:
    seven config-3 DAGs and the pressure program."""
    narrow = list(sets_a()[0][:40])
    wide = [lower(_dag_of(20_000 + 7 * i), nw=ir.NW) for i in range(40, 47)] + [_pressure_program()]
    progs = []
    for k in range(8):
        progs += [narrow[k], wide[k]]
    progs += narrow[8:]
    n_wide = sum(_max_w_written(p) >= ir.NW_NARROW for p in progs)
    assert 1 <= n_wide <= 8 and _max_w_written(wide[-1]) >= ir.NW_NARROW
    assert all(_max_w_written(p) < ir.NW_NARROW for p in narrow)
    batch = ir.Batch(progs)
    return progs, SC.sat_masks(batch, SEED_A, 1000), SC.aux1_totals(batch)


@pytest.fixture(scope="module")
def db_c(engine):
    db = engine.upload(sets_c()[0])
    yield db
    db.free()


@pytest.mark.parametrize("flags", ROWS)
@pytest.mark.parametrize("budget", [100, 1000])
def test_both_register_files_in_one_batch(engine, db_c, budget, flags):
    """The 8-register and the 16-register launch of one search share found[] and the counter
    lines: the answers are the oracle's and the counters are the sum over both."""
    progs, masks, aux1 = sets_c()
    assert_row(engine.check(db_c, budget=budget, seed=SEED_A, flags=flags), masks, budget, flags, aux1, "C")


# ---- D. ops under SHORTCIRCUIT -------------------------------------------------------------

def test_shortcircuit_ops_stop_at_the_last_falling_assert(engine):
    """12 sets at budget 150 (groups of 64, 64 and 22): a group whose lanes all end false is
    charged the instructions up to the assert where its last root fell, any other group the
    whole program — times its size, not times 64."""
    progs, masks, _ = sets_a()
    fs = [SC.first_witness(m, N_CAND_A) for m in masks]
    pick = list(range(8)) + [s for s, f in enumerate(fs) if f is not None and 64 <= f < 150 and s >= 8][:4]
    assert len(pick) == 12, pick
    budget, flags = 150, SHORT | COUNT_OPS
    sub = [progs[s] for s in pick]
    db = engine.upload(sub)
    res = engine.check(db, budget=budget, seed=SEED_A, flags=flags)
    db.free()
    assert_row(res, masks[pick], budget, flags, None, "D")
    want = SC.shortcircuit_ops(ir.Batch(sub), SEED_A, budget)
    whole = budget * sum(SC.aux1_totals(ir.Batch(sub)))
    assert 0 < want < whole                                 # some group does leave early
    assert res.ops == want, (res.ops, want, whole)


# ---- E. entry points no other test calls ---------------------------------------------------

SENTINEL = 0x5A5A5A5A


def _check_host(db, budget, flags, seed=SEED_A, bitmap=None):
    found = np.full(len(db), 0x12345678, dtype=np.uint32)
    st = _lib.pf_stats()
    _lib.check(_lib.lib().pf_check_batch(db.handle, seed, budget, flags, 0, _lib.ptr_u32(found),
                                         _lib.ptr_u8(bitmap) if bitmap is not None else None, ctypes.byref(st)),
               "pf_check_batch")
    return found, st


def _counters(st):
    return (st.evals_full, st.cands_decided, st.ops, st.timed_out)


@pytest.mark.parametrize("budget", [100, 1000])
@pytest.mark.parametrize("side", [False, True], ids=["current_stream", "side_stream"])
def test_check_batch_dev(engine, db_a, side, budget):
    """pf_check_batch_dev leaves pf_check_batch's verdicts in the caller's device buffer (and
    nothing past them), with and without a stats block, on the current stream and on a side
    stream; the counters equal pf_check_batch's, whose own result is the same afterwards."""
    import torch

    _, masks, aux1 = sets_a()
    n, flags = len(db_a), COUNT_OPS
    found0, st0 = _check_host(db_a, budget, flags)
    assert np.array_equal(found0, SC.found(masks, budget))
    stream = torch.cuda.Stream() if side else torch.cuda.current_stream()
    for with_stats in (True, False):
        buf = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()                            # the fill, before another stream writes
        st = _lib.pf_stats()
        _lib.check(_lib.lib().pf_check_batch_dev(db_a.handle, SEED_A, budget, flags, 0, buf.data_ptr(),
                                                 ctypes.byref(st) if with_stats else None, stream.cuda_stream),
                   "pf_check_batch_dev")
        torch.cuda.synchronize()
        got = buf.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:n], found0), (with_stats, np.flatnonzero(got[:n] != found0)[:6])
        assert got[n] == SENTINEL
        if with_stats:
            assert _counters(st) == _counters(st0) == (n * budget, n * budget, budget * sum(aux1), 0)
    found1, st1 = _check_host(db_a, budget, flags)
    assert np.array_equal(found1, found0) and _counters(st1) == _counters(st0)


@functools.lru_cache(maxsize=None)
def _mixed_set():
    """The set of A whose first 300 verdicts are the most evenly split, its generated
    assignments as explicit candidates, and the oracle's verdicts on them."""
    import pyoracle as O

    progs, masks, _ = sets_a()
    s = int(np.argmax([min(m[:300].sum(), 300 - m[:300].sum()) for m in masks]))
    assert 0 < masks[s][:300].sum() < 300
    sv = O.SetView.from_batch(ir.Batch([progs[s]]), 0)
    cands = sv.gen_assignments(np.arange(300, dtype=np.uint64), SEED_A)
    return s, progs[s], cands, masks[s][:300]


@pytest.mark.parametrize("n_cand", [1, 63, 64, 65, 300])
def test_eval_assignments_dev(engine, db_a, n_cand):
    """pf_eval_assignments_dev on device-resident assignments: the verdicts of
    pf_eval_assignments and of the oracle, on the current and on a side stream, and no byte
    past n_cand."""
    import torch

    s, prog, cands, want = _mixed_set()
    soa = ir.pack_assignments(prog, cands[:n_cand])
    host = engine.eval_assignments(db_a, s, soa)
    assert np.array_equal(host, want[:n_cand])
    d_soa = torch.from_numpy(soa.view(np.int32)).to("cuda")
    for stream in (torch.cuda.current_stream(), torch.cuda.Stream()):
        out = torch.full((n_cand + 1,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        _lib.check(_lib.lib().pf_eval_assignments_dev(db_a.handle, s, d_soa.data_ptr(), n_cand, out.data_ptr(),
                                                      stream.cuda_stream), "pf_eval_assignments_dev")
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        bad = np.flatnonzero(got[:n_cand].astype(bool) != want[:n_cand])
        assert bad.size == 0, bad[:6]
        assert set(got[:n_cand].tolist()) <= {0, 1} and got[n_cand] == 0xA5


@pytest.mark.parametrize("n_sets", [96, 9])
def test_sat_bitmap(engine, n_sets):
    """sat_bitmap_out: bit s is found[s] != NOT_FOUND, the bytes past (n + 7) // 8 are the
    caller's; n_sat counts the same sets."""
    progs, masks, _ = sets_a()
    db = engine.upload(progs[:n_sets])
    nb = (n_sets + 7) // 8
    for budget in (100, 1000):
        bitmap = np.full(nb + 8, 0xA5, dtype=np.uint8)
        found, st = _check_host(db, budget, EARLY | SHORT, bitmap=bitmap)
        assert np.array_equal(found, SC.found(masks[:n_sets], budget))
        sat = found != SC.NOT_FOUND
        assert 0 < sat.sum() < n_sets
        assert np.array_equal(np.unpackbits(bitmap[:nb], bitorder="little")[:n_sets].astype(bool), sat)
        assert (bitmap[nb:] == 0xA5).all()
        assert st.n_sat == int(sat.sum())
    db.free()


def test_check_each_reports_every_batch_as_check_does(engine):
    """check_each (pf_check_batches: all enqueued before any result is read) over three
    batches: each entry's found and counters are that batch's own check()."""
    progs, masks, _ = sets_a()
    cuts = [(0, 40), (40, 57), (57, 96)]
    dbs = [engine.upload(progs[lo:hi]) for lo, hi in cuts]
    budget, flags = 100, COUNT_OPS
    each = engine.check_each(dbs, budget=budget, seed=SEED_A, flags=flags)
    assert len(each) == 3
    for (lo, hi), db, r in zip(cuts, dbs, each):
        one = engine.check(db, budget=budget, seed=SEED_A, flags=flags)
        aux1 = SC.aux1_totals(db.batch)
        assert_row(r, masks[lo:hi], budget, flags, aux1, ("each", lo))
        assert np.array_equal(r.found, one.found)
        assert (r.evals_full, r.cands_decided, r.ops) == (one.evals_full, one.cands_decided, one.ops)
        assert r.ops == budget * sum(aux1) > 0
    for db in dbs:
        db.free()
