"""GPU: every op, compare and generator arm at every width 1..256, on every kernel, bit-exact
against the width catalogue of tests/width_cases.py (whose expectations are Python integers and
whose premises tests/test_width_cases.py asserts on the CPU).

The width-dependent device code is written limb by limb (maskw's switch over the top limb,
limb_mask, sextw, ge_width, the generator's per-width arms); the other GPU tests reach it at
about ten widths.  Here, per catalogue key:

* search kernels (pf_check_kernel, pf_check_early_kernel, the r16 pair): 256 widths x 8 rows,
  each with its corrupted twin, by the candidate-0 protocol — 4,096 one-candidate sets per
  upload, both register files, full sweep and early exit;
* census and climb kernels on two of those rows and twins per width, plus directly asserted
  compares that fail at operand distances of bit length 0, 1, ceil(w / 2) and w: the census'
  counts against the verdict, the climb's score against climb_model ("sites") and
  climb_tree_model ("tree");
* constant operands (PF_I_KA / PF_I_KB): uploads of at most 15 sets stay below the fold gate,
  so the constants reach the device — one row and twin at the widths 0, 1, 31 (mod 32) and one
  more per top limb;
* stream kernels (Engine.eval_batch) and SoA kernels (eval_programs, eval_assignments): one
  program per width and register file, 80 explicit candidates (40 rows held and corrupted,
  interleaved: one full group and a partial one), the SoA legs with garbage above every
  variable's width;
* the generator: a GENERIC and a VALUE variable of every width through the materialise kernel,
  limb for limb against the oracle, and per width a set pinned to the oracle's value at a chosen
  candidate through the search kernels' inlined generator, census and climb."""

import functools

import census_model
import climb_model as CM
import climb_tree_model as TM
import coracle_py
import numpy as np
import pyoracle as O
import pytest
import stream_model as M
import width_cases as C

from mythril_amd import ir
from mythril_amd.engine import NOT_FOUND

pytestmark = pytest.mark.gpu

FLAGS = (0, ir.FLAG_EARLY_EXIT | ir.FLAG_SHORTCIRCUIT)
BASES = (0, 8)
SEED = 0x0C0DE_5EED


def _report(progs, bad, got=None):
    return (len(bad), [C.describe(progs[i]) + (() if got is None else (str(got[i]),)) for i in list(bad)[:4]])


def _found(engine, db, progs, flags, what, failures):
    res = engine.check(db, budget=1, seed=SEED, flags=flags)
    want = np.array([0 if p.verdict else NOT_FOUND for p in progs], dtype=np.uint32)
    bad = np.nonzero(res.found != want)[0]
    if bad.size:
        failures.append((what,) + _report(progs, bad, res.found))


# ---- search, census and climb kernels: the candidate-0 protocol -----------------------------------

def _census_climb(engine, db, progs, ids, what, failures):
    """One candidate (the parents) per set: the census' counts against the verdict, the climb's
    score and status against the models."""
    sub = [progs[i] for i in ids]
    got = engine.census(db, ids, budget=1, seed=SEED)
    bad = []
    for k, p in enumerate(sub):
        v = int(p.verdict)
        row = (got.holds[k].tolist(), got.alive[k].tolist(), int(got.best_fails[k]), int(got.status[k]))
        if row != ([v], [v], 1 - v, ir.CENSUS_DONE) or (v and int(got.best_cand[k]) != 0):
            bad.append(k)
    if bad or got.evals != len(ids):
        failures.append((what + " census",) + _report(sub, bad))
    devs = CM.device_sets(db.batch)
    for score, model in (("sites", lambda: CM.climb(db.batch, ids, 1, 1, SEED, devs)),
                         ("tree", lambda: TM.climb(db.batch, ids, 1, 1, SEED, "tree", devs))):
        res = engine.climb(db, ids, 1, 1, seed=SEED, score=score)
        want = model()
        bad = [k for k, m in enumerate(want)
               if (int(res.status[k]), int(res.score[k]), int(res.round[k])) != (m.status, m.score, m.round)
               or [ir.from_limbs(r) for r in res.values[k]] != m.values
               or (m.status == ir.CLIMB_WITNESS) != sub[k].verdict]
        if bad:
            failures.append((what + " climb " + score,) +
                            _report(sub, bad, [(int(res.score[k]), want[k].score) for k in range(len(sub))]))


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("key", C.KEYS)
def test_search_census_and_climb_kernels(engine, key, base):
    progs, picked = [], []
    widths = C.widths_of(key)
    for w in widths:
        for i, r in enumerate(C.rows(key, w, C.N_SEARCH)):
            if i in (w % 8, (w + 4) % 8):
                picked += [len(progs), len(progs) + 1]
            progs += [C.search_set(r, base), C.search_set(r, base, twin=True)]
    assert len(progs) == 2 * C.N_SEARCH * len(widths) and len(picked) == 4 * len(widths)
    near = [C.near_set(key, w, a, b, base) for w in C.WIDTHS for a, b, _ in C.near_rows(key, w)] \
        if key in C.NEAR_KEYS else []
    picked += range(len(progs), len(progs) + len(near))
    progs += near
    assert {progs[i].row.w for i in picked} == set(widths)
    failures = []
    db = engine.upload(progs)
    try:
        for flags in FLAGS:
            _found(engine, db, progs, flags, f"search flags {flags}", failures)
        _census_climb(engine, db, progs, picked, f"base {base}", failures)
    finally:
        db.free()
    assert not failures, failures


# ---- constant operands, below the fold gate ---------------------------------------------------------

@pytest.mark.parametrize("key", C.GROUND_KEYS)
def test_constant_operands_reach_the_device(engine, key):
    widths = C.gate_sample_widths()
    assert len(widths) == 32 and {(w - 1) >> 5 for w in widths} == set(range(8))
    failures = []
    for base in BASES:
        progs = []
        for w in widths:
            r = C.rows(key, w, C.N_SEARCH)[w % 8]
            progs += [C.ground_set(r, base), C.ground_set(r, base, twin=True)]
        for k in range(0, len(progs), 14):
            part = progs[k:k + 14]
            assert len(part) < 16                  # PF_FOLD_MIN_SETS: the fold pass stays off
            db = engine.upload(part)
            try:
                _found(engine, db, part, 0, f"ground base {base}", failures)
            finally:
                db.free()
    assert not failures, failures


# ---- stream and SoA kernels: explicit candidates ------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _explicit(key):
    """(programs, batch, SoA of the candidates, verdict rows): per width, base 0 then base 8."""
    progs, cands, rows = [], [], []
    for w in C.widths_of(key):
        c, want = C.explicit_candidates(key, w)
        for base in BASES:
            p = C.explicit_set(key, w, base)
            p.w = w
            progs.append(p)
            cands.append(c)
            rows.append(want)
    batch = ir.Batch(progs)
    assert [M.is_wide(p) for p in progs[:2]] == [False, True]
    return progs, batch, ir.pack_soa(batch, cands), rows


def _garbage(batch, soa, seed):
    """The SoA with random bits ORed in above every variable's width."""
    rng = np.random.default_rng(seed)
    out = soa.copy()
    n = soa.shape[2]
    for v, row in enumerate(batch.schema):
        vw = (int(row[0]) >> 8) & 0x3FF
        for limb in range(vw // 32, 8):
            keep = ir.mask(vw - 32 * limb) if vw > 32 * limb else 0
            noise = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
            out[v, limb] |= noise & np.uint32(~keep & 0xFFFFFFFF)
    return out


def _rows_differ(key, progs, got, rows):
    bad = [(key, f"w{p.w}", p.name, np.flatnonzero(got[s] != np.array(rows[s]))[:6].tolist())
           for s, p in enumerate(progs) if got[s].tolist() != rows[s]]
    return (len(bad), bad[:4])


@pytest.mark.parametrize("key", C.KEYS)
def test_stream_kernels(engine, key):
    progs, batch, soa, rows = _explicit(key)
    assert len(progs) == 2 * len(C.widths_of(key)) and soa.shape[2] == 80
    bits, first, count = M.summarize(rows)
    assert first.tolist() == [0] * len(progs) and count.tolist() == [40] * len(progs)
    db = engine.upload(batch)
    try:
        for sc in (True, False):
            res = engine.eval_batch(db, soa, shortcircuit=sc)
            got = res.verdicts()
            assert all(got[s].tolist() == rows[s] for s in range(len(progs))), (sc, _rows_differ(key, progs, got, rows))
            assert np.array_equal(res.bits, bits) and M.tail_is_zero(res.bits, 80), sc
            assert res.first.tolist() == first.tolist() and res.count.tolist() == count.tolist(), sc
            assert res.cands_decided == 80 * len(progs) and res.n_sat == len(progs)
    finally:
        db.free()


@pytest.mark.parametrize("key", C.KEYS)
def test_soa_kernels_with_garbage_above_the_width(engine, key):
    progs, batch, soa, rows = _explicit(key)
    dirty = _garbage(batch, soa, 0x6A7 + C.KEYS.index(key))
    assert dirty.shape == soa.shape and (dirty != soa).any()
    flat = lambda a: np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
    pack = (flat(batch.code), flat(batch.consts), flat(batch.schema), flat(batch.descs))
    got = engine.eval_programs(pack, dirty)
    assert all(got[s].tolist() == rows[s] for s in range(len(progs))), _rows_differ(key, progs, got, rows)
    sample = [s for s, p in enumerate(progs) if p.w in C.gate_sample_widths()]
    db = engine.upload(batch)
    try:
        for s in sample:
            off, nv = int(batch.descs[s][4]), int(batch.descs[s][5])
            one = engine.eval_assignments(db, s, dirty[off:off + nv])
            assert one.tolist() == rows[s], (key, progs[s].name, np.flatnonzero(one != np.array(rows[s]))[:6].tolist())
    finally:
        db.free()


# ---- the generator ------------------------------------------------------------------------------------

@pytest.mark.parametrize("gseed", C.GEN_SEEDS, ids=hex)
@pytest.mark.parametrize("layout", C.GEN_LAYOUTS)
def test_materialize_every_width(engine, layout, gseed):
    p = C.generator_set(layout, seed=0x51ED)
    batch = ir.Batch([p])
    cands = list(C.GEN_CANDS)
    want = O.SetView.from_batch(batch, 0).gen_assignments(np.array(cands, dtype=np.uint64), gseed)
    want = ir.limbs_array([x for a in want for x in a]).reshape(len(cands) * len(p.vars), 8)
    db = engine.upload(batch)
    try:
        got = engine.materialize_limbs(db, [0] * len(cands), cands, seed=gseed)
    finally:
        db.free()
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (len(bad), [(cands[i // 512], f"w{p.vars[i % 512].width}", p.vars[i % 512].kind,
                                       hex(ir.from_limbs(got[i])), hex(ir.from_limbs(want[i]))) for i in bad[:6]])


@functools.lru_cache(maxsize=2)
def _pins(base):
    progs = [C.width_pin_set_at(w, base) for w in C.WIDTHS]
    packed = coracle_py.Packed(ir.Batch(progs))
    want = [packed.first_sat(s, C.PIN_SEED, C.PIN_BUDGET) for s in range(len(progs))]
    assert all(x is not None and x <= p.cand for x, p in zip(want, progs))
    return progs, want


@pytest.mark.parametrize("base", BASES)
def test_inlined_generator_at_every_width(engine, base):
    progs, want = _pins(base)
    db = engine.upload(progs)
    try:
        for flags in FLAGS:
            res = engine.check(db, budget=C.PIN_BUDGET, seed=C.PIN_SEED, flags=flags)
            got = [None if f == NOT_FOUND else int(f) for f in res.found]
            assert got == want, (flags, [(p.name, p.cand, g, x) for p, g, x in zip(progs, got, want) if g != x][:8])
        ids = [w - 1 for w in C.gate_sample_widths()]
        cen = engine.census(db, ids, budget=C.PIN_BUDGET, seed=C.PIN_SEED)
        model = census_model.census(db.batch, ids, C.PIN_BUDGET, C.PIN_SEED)
        for k, m in enumerate(model):
            row = (cen.holds[k].tolist(), cen.alive[k].tolist(), cen.sole[k].tolist(), int(cen.best_fails[k]),
                   int(cen.best_cand[k]), int(cen.status[k]))
            assert row == (m.holds, m.alive, m.sole, m.best_fails, m.best_cand, ir.CENSUS_DONE), progs[ids[k]].name
            assert m.best_fails == 0 and m.best_cand == want[ids[k]]
        for score, model in (("sites", CM.climb(db.batch, ids, 2, 64, C.PIN_SEED)),
                             ("tree", TM.climb(db.batch, ids, 2, 64, C.PIN_SEED, "tree"))):
            res = engine.climb(db, ids, 2, 64, seed=C.PIN_SEED, score=score)
            for k, m in enumerate(model):
                dev = (int(res.status[k]), int(res.score[k]), int(res.round[k]),
                       [ir.from_limbs(r) for r in res.values[k]])
                assert dev == (m.status, m.score, m.round, m.values), (score, progs[ids[k]].name)
    finally:
        db.free()
