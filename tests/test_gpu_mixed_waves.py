"""GPU: the mixed 64-lane waves of the divider, EXP, MUL and UMUL_NOOVF on every kernel that
evaluates programs, against oracle/pyoracle.py (and Python's integers: tests/
test_lane_table_cases.py), bit-exact.

The wave-wide decisions of pf::udivrem256 and exp256_split (csrc/u256.h) can only go wrong where
the lanes of a wave disagree.  The designed waves of div_trim_cases, products_cases,
exp_chain_cases and the exp_scale / exp_series mixed waves reach the SoA kernel through
``eval_assignments`` in their own test files; here they reach the others:

* the search kernels (pf_check_kernel / pf_check_early_kernel and the r16 pair) by the
  lane-table protocol of lane_table_cases.py: the wave is selected inside the program from the
  generated index k, a generated tag makes lane j the only witness of set j, so ``found[j] == j``
  for every set and NOT_FOUND for every twin with one bit of its expectation flipped.  One upload
  per family, register placement and register file; the full sweep, the early-exit kernels, and
  the early-exit kernels without the candidate-0 probe (candidate 0's group then goes through the
  search phase too);
* the stream kernels (pf_eval_batch, both register files) with the 64 realised pairs as explicit
  candidates of op_set programs, operands and results in registers 5 and 6: right expectations,
  lane i corrupted in bit 5 i + 1, and both side by side;
* the census kernels and the climb kernels (both scores) on the lane-table sets of positions 0
  and 63 of every divider and products wave and on the exp_chain waves.

A failure names the wave, the position, the lane, k_j and the operands, and says whether the set
fails on its own and under which register placements."""

import functools

import coracle_py
import lane_table_cases as L
import numpy as np
import op_programs as P
import pytest
import stream_model as M
from test_gpu_eval_batch import REGS, _same, op_set

from mythril_amd import ir

pytestmark = pytest.mark.gpu

BASES = (0, 8)
FLAGS = {"full": 0, "early": ir.FLAG_EARLY_EXIT | ir.FLAG_SHORTCIRCUIT,
         "early_noprobe": ir.FLAG_EARLY_EXIT | ir.FLAG_SHORTCIRCUIT | ir.FLAG_NO_PROBE}
ENTRIES = L.catalogue()
IDS = [e.id for e in ENTRIES]
SAMPLE_FAMILIES = sorted({e.family for e in L.sample()})
_FOUND = {}     # (family, base) -> {(placement, flags name): found}


def _lines(report):
    """A failure report as text, one finding per line (a tuple's repr is cut short)."""
    return "\n".join(" | ".join(str(x) for x in row) for row in report)


# ---- the search kernels ---------------------------------------------------------------------

def _family_found(engine, family, base):
    """One upload per placement of all the family's sets; one search per flag set."""
    key = (family, base)
    if key not in _FOUND:
        out = {}
        for placement in L.PLACEMENTS:
            batch = L.LaneBatch(L.family(family), placement, base)
            db = engine.upload(batch)
            try:
                for name, flags in FLAGS.items():
                    out[placement, name] = engine.check(db, budget=L.LANES, seed=L.G, flags=flags).found.copy()
            finally:
                db.free()
        _FOUND[key] = out
    return _FOUND[key]


def _alone(engine, entry, j, twin, base, flags):
    """The narrowing of a failure: the single set, under every register placement."""
    out = {}
    for placement in L.PLACEMENTS:
        db = engine.upload(L.LaneBatch([entry], placement, base, only={(j, twin)}))
        try:
            f = int(engine.check(db, budget=L.LANES, seed=L.G, flags=flags).found[0])
        finally:
            db.free()
        out[placement] = "NOT_FOUND" if f == L.NOT_FOUND else f
    return out


@functools.lru_cache(maxsize=None)
def _oracle_list(family):
    """The C oracle's first witness of every set of the family (the verdict does not depend on
    the register numbers: one placement, one register file)."""
    batch = L.LaneBatch(L.family(family), "lds", 0)
    packed = coracle_py.Packed(batch)
    got = [packed.first_sat(s, L.G, L.LANES) for s in range(len(batch))]
    want = np.array([L.NOT_FOUND if x is None else x for x in got], dtype=np.uint32)
    assert np.array_equal(want, batch.want), family          # lane j, and nothing for the twins
    return want


@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("entry", ENTRIES, ids=IDS)
def test_search_kernels(engine, entry, base, flags):
    found = _family_found(engine, entry.family, base)
    at = 128 * L.family(entry.family).index(entry)
    want = _oracle_list(entry.family)[at:at + 128]
    report = []
    for placement in L.PLACEMENTS:
        got = found[placement, flags][at:at + 128]
        for s in np.flatnonzero(got != want)[:3]:
            j, twin = int(s) // 2, bool(s & 1)
            report.append((placement, f"base{base}", flags, ("corrupted " if twin else "") + entry.describe(j),
                           f"found {int(got[s]):#x}, want {int(want[s]):#x}",
                           "alone:", _alone(engine, entry, j, twin, base, FLAGS[flags])))
    assert not report, _lines(report)


def test_the_search_runs_both_register_files(engine):
    """base 0 stays within the 8-register file and base 8 leaves it, under every placement."""
    e = L.family("udiv")[0]
    for placement in L.PLACEMENTS:
        for base in BASES:
            p = L.program(e, placement, base, e.expectations()[0])
            assert M.is_wide(p) == (base == 8), (placement, base)


# ---- the stream kernels -----------------------------------------------------------------------

@pytest.mark.parametrize("entry", ENTRIES, ids=IDS)
def test_stream_kernels(engine, entry):
    """The realised pairs as explicit candidates: three waves of 64 — right expectations, lane i
    corrupted in bit 5 i + 1, and right and corrupted lanes alternating — through both stream
    kernels, with short-circuit on and off."""
    op, w = entry.op, entry.w
    is_bool = op == ir.B_UMUL_NOOVF
    pairs, res = entry.realised(), entry.results()
    good, wrong = [], []
    for i, ((a, b), r) in enumerate(zip(pairs, res)):
        g = P.GUARDS[i % len(P.GUARDS)]
        r = int(r)
        good.append([a, b, g, r, g])
        wrong.append([a, b, g, r ^ 1 if is_bool else r ^ 1 << entry.twin_bit(i), g])
    cands = good + wrong + [wrong[i] if i & 1 else good[i] for i in range(L.LANES)]
    want = [True] * 64 + [False] * 64 + [not i & 1 for i in range(L.LANES)]
    progs = [op_set(op, w, regs, base) for base in BASES for regs in REGS]
    assert [M.is_wide(p) for p in progs] == [False] * len(REGS) + [True] * len(REGS)
    batch = ir.Batch(progs)
    rows = M.verdicts(batch, [cands] * len(progs))
    assert all(r == want for r in rows), entry.id         # the oracle agrees with the construction
    soa = ir.pack_soa(batch, [cands] * len(progs))
    db = engine.upload(batch)
    try:
        for sc in (True, False):
            got = engine.eval_batch(db, soa, shortcircuit=sc)
            v = got.verdicts()
            bad = [(progs[s].name, f"shortcircuit {sc}", "wave %d" % (c // 64), entry.describe(c % 64),
                    f"got {bool(v[s][c])}") for s in range(len(progs))
                   for c in np.flatnonzero(v[s] != np.array(want))[:3]]
            assert not bad, _lines(bad[:6])
            _same(got, rows, f"{entry.id} sc {sc}")
            assert got.first.tolist() == [0] * len(progs) and got.count.tolist() == [96] * len(progs)
    finally:
        db.free()


# ---- the census and the climb kernels -----------------------------------------------------------

def _sample_batches(family, base):
    entries = [e for e in L.sample() if e.family == family]
    assert entries
    for placement in ("low", "lds"):
        yield placement, L.LaneBatch(entries, placement, base)


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("family", SAMPLE_FAMILIES)
def test_census_kernels(engine, family, base):
    """One assert site per set: exactly one of the 64 candidates holds there, candidate j; under
    the twin none does."""
    for placement, batch in _sample_batches(family, base):
        db = engine.upload(batch)
        try:
            ids = list(range(len(batch)))
            assert (engine.site_counts(db, ids) == 1).all()
            res = engine.census(db, ids, budget=L.LANES, seed=L.G)
        finally:
            db.free()
        assert (res.status == ir.CENSUS_DONE).all() and not res.timed_out
        bad = []
        for s, (e, j, twin) in enumerate(batch.index):
            holds, alive = int(res.holds[s][-1]), int(res.alive[s][-1])
            fails, cand = int(res.best_fails[s]), int(res.best_cand[s])
            ok = (holds == 0 and alive == 0 and fails >= 1) if twin else \
                (holds == 1 and alive == 1 and fails == 0 and cand == j)
            if not ok:
                bad.append((placement, f"base{base}", batch.describe(s),
                            dict(holds=holds, alive=alive, best_fails=fails, best_cand=cand)))
        assert not bad, f"{len(bad)} sets\n" + _lines(bad[:4])


@pytest.mark.parametrize("score", ["sites", "tree"])
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("family", SAMPLE_FAMILIES)
def test_climb_kernels(engine, family, base, score):
    """One round of 64 candidates under the search's own seed: the witness is lane j's
    assignment (k_j, t_j); the twins end without one."""
    seed = (L.G - ir.CLIMB_SEED_MUL) & 0xFFFFFFFFFFFFFFFF
    assert ir.climb_round_seed(seed, 0) == L.G
    for placement, batch in _sample_batches(family, base):
        db = engine.upload(batch)
        try:
            res = engine.climb(db, list(range(len(batch))), rounds=1, per_round=L.LANES, seed=seed, score=score)
        finally:
            db.free()
        assert not res.timed_out
        bad = []
        for s, (e, j, twin) in enumerate(batch.index):
            status = int(res.status[s])
            if twin:
                ok = status == ir.CLIMB_NONE
            else:
                vals = [ir.from_limbs(r) for r in res.values[s]]
                ok = status == ir.CLIMB_WITNESS and vals == [e.ks()[j], e.tags()[j]] and int(res.round[s]) == 0
            if not ok:
                bad.append((placement, f"base{base}", score, batch.describe(s), f"status {status}",
                            [hex(ir.from_limbs(r)) for r in res.values[s]]))
        assert not bad, f"{len(bad)} sets\n" + _lines(bad[:4])
