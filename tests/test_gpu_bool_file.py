"""GPU: the Bool register file — the 32 B registers as the bits of one VGPR, B_SPILL / B_FILL
to private scratch and to the LDS window-table entries, ASSERTs fused into B-unit ops — on every
kernel instantiation, against the oracles, bit-exact.  The programs are those of
tests/bool_file_cases.py; tests/test_bool_file_cases.py proves on the CPU that they hold B
spills of both kinds and fused asserts, and that every fill and every register decides some
candidate's verdict.

* SoA kernels (pf_eval_assignments, pf_eval_programs): 65 and 192 explicit candidates, every
  lane with a B file of its own, about half of them with a corrupted expected word — correct
  and corrupted candidates sit in the same wave, and the last wave is partial.  The identity
  pressure programs hold for no assignment, so they run on generated candidates only.
* search kernels (``base`` 0: the narrow pair, 8: the r16 pair; both EARLY settings): the
  candidate-0 protocol of test_gpu_narrow_ops.py, each program next to corrupted copies that
  must come out NOT_FOUND, and the pressure programs over 1,024 generated candidates, where
  ``found`` is the C oracle's first witness or none.
* the slot and spill sets go up twice: in one upload, which pf_batch_create folds, and in
  uploads below PF_FOLD_MIN_SETS sets, which it does not — only there do B_CONST and
  B_XOR r, r write their register on the device.
* climb: a pressure program and the fused-assert sets through test_gpu_climb.py's comparison
  with the climb model."""

import functools

import coracle_py
import numpy as np
import pytest
from test_bool_file_cases import c_eval_explicit
from test_gpu_climb import assert_same, both
from test_gpu_narrow_ops import _search, kernels

import bool_file_cases as C
from mythril_amd import ir
from mythril_amd.engine import NOT_FOUND

pytestmark = pytest.mark.gpu

N_CANDS = (65, 192)
BUDGET, GSEED = C.BUDGET, C.GSEED


@functools.lru_cache(maxsize=None)
def _explicit_sets(n):
    """The soa cases and the free pressure programs: (name, program, assignments, the C
    oracle's verdicts); for the hand-emitted sets those are the builder's verdicts too."""
    out = []
    names = [name for name, _ in C.soa_cases()]
    if n != N_CANDS[0]:      # three full waves: every spill set, a third of the slot sets
        names = [nm for nm in names if nm.startswith("bfile")][::3] + [nm for nm in names if not nm.startswith("bfile")]
    for name in names:
        prog, cands, verdicts = C.explicit_case(name, n)
        assert c_eval_explicit(ir.Batch([prog]), 0, cands) == verdicts, name
        out.append((name, prog, cands, verdicts))
    for name in C.PRESSURE:
        if "/free/" in name:
            _, prog, cands = C.pressure_explicit(name, n)
            out.append((name, prog, cands, c_eval_explicit(ir.Batch([prog]), 0, cands)))
    return out


def _soa(prog, cands):
    """ir.pack_assignments, by numpy: [var][limb][candidate]."""
    flat = ir.limbs_array([x for a in cands for x in a])
    return ir.pack_assignments_np(flat.reshape(len(cands), len(prog.vars), 8))


def _balanced(want):
    return len(want) / 4 <= sum(want) <= 3 * len(want) / 4


# ---- SoA kernels ------------------------------------------------------------------------------

@pytest.mark.parametrize("upload", ["folded", "unfolded"])
@pytest.mark.parametrize("n", N_CANDS)
def test_explicit_candidates_with_a_b_file_per_lane(engine, n, upload):
    """``folded``: all sets in one upload, which pf_batch_create folds (PF_FOLD_MIN_SETS sets or
    more) — a B_CONST and a B_XOR r, r are then constants of the device program.  ``unfolded``:
    uploads of C.CHUNK sets, which it leaves alone: there B_CONST itself writes rd."""
    sets = _explicit_sets(n)
    assert len(sets) >= C.FOLD_MIN_SETS > C.CHUNK
    bad = []
    for part in [sets] if upload == "folded" else C.chunks(sets):
        db = engine.upload([prog for _, prog, _, _ in part])
        try:
            for s, (name, prog, cands, want) in enumerate(part):
                assert _balanced(want) and len(cands) == n, name
                got = engine.eval_assignments(db, s, _soa(prog, cands))
                lanes = [i for i in range(n) if bool(got[i]) != want[i]]
                if lanes:
                    bad.append((name, lanes[:8], [hex(cands[i][-1]) for i in lanes[:3]]))
        finally:
            db.free()
    assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("n", N_CANDS)
def test_spill_sets_as_several_programs_of_one_call(engine, n):
    """pf_eval_programs: a wave per program and 64 candidates, the LDS sized for one wave."""
    sets = [x for x in _explicit_sets(n) if x[0].startswith(("bspill", "fused:fill", "p40"))]
    assert len(sets) == 12 + 2 + 2
    batch = ir.Batch([prog for _, prog, _, _ in sets])
    soa = np.zeros((int(batch.descs[:, 5].sum()), 8, n), dtype=np.uint32)
    for s, (_, prog, cands, _) in enumerate(sets):
        off = int(batch.descs[s][4])
        soa[off:off + len(prog.vars)] = _soa(prog, cands)
    pack = tuple(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
                 for a in (batch.code, batch.consts, batch.schema, batch.descs))
    got = engine.eval_programs(pack, soa)
    bad = [(name, [i for i in range(n) if bool(got[s][i]) != want[i]][:8])
           for s, (name, _, _, want) in enumerate(sets) if [bool(x) for x in got[s]] != want]
    assert not bad, bad


# ---- search kernels: one explicit assignment, candidate 0 -------------------------------------

@kernels
@pytest.mark.parametrize("op", C.BFILE_OPS, ids=lambda op: ir.OPNAMES[op])
def test_b_file_slots(engine, op, base, flags):
    """One B op between full B files: every rd of 0..31, rd equal to a source, the condition
    of a B_ITE over the whole file (a sample on the r16 kernels), under a file in which the
    op changes B[rd].  The copies expect the old bit in rd, or a flipped bit elsewhere.  Once
    as one upload and once in uploads too small for the fold pass, which turns a B_CONST and a
    B_XOR r, r into constants (tests/test_bool_file_cases.py::test_small_uploads_are_not_folded)."""
    groups = C.bfile_rows(op, base)
    progs = [p for g in groups for p in g]
    assert len(progs) >= 3 * (7 if base else 37) >= C.FOLD_MIN_SETS
    _search(engine, progs, flags)                 # one upload: folded
    for part in C.chunks(groups, C.CHUNK // 3):   # uploads the fold pass leaves alone
        _search(engine, [p for g in part for p in g], flags)


@kernels
def test_b_spill_slots(engine, base, flags):
    """B spills to slots 0, 63, a slot a W_SPILL wrote before and two more — in scratch and in
    LDS entries 1..3, across nothing, a W_EXP or a B_UMUL_NOOVF — next to the guards in W
    registers 5 and 6 (8 + 5, 8 + 6); every rotation of registers over slots."""
    groups = C.bspill_rows(base)
    _search(engine, [p for g in groups for p in g], flags)
    for part in C.chunks(groups, C.CHUNK // 3):
        _search(engine, [p for g in part for p in g], flags)


@kernels
def test_fused_and_plain_asserts(engine, base, flags):
    progs = [p for kind in C.FUSED_KINDS for p in C.fused_rows(kind, base)]
    assert len(progs) == 12
    _search(engine, progs, flags)


# ---- search kernels: generated candidates, every lane ------------------------------------------

@kernels
def test_pressure_programs_over_generated_candidates(engine, base, flags):
    """More than 32 live Bools through lower(): the free variants' first witness is the C
    oracle's, the identity variants (f ^ r, false unless a bit is wrong) have none."""
    names = [nm for nm in C.PRESSURE if nm.endswith("narrow" if base == 0 else "r16")]
    progs = [C.pressure_program(nm)[1] for nm in names]
    top = [max(i.dst for i in p.code if i.op < ir.B_CONST and i.op != ir.W_SPILL) for p in progs]
    # narrow: W registers 5 and 6, the LDS ones, are in use; else a register of the r16 kernels
    assert all(t >= ir.NW_NARROW for t in top) if base else top == [ir.NW_NARROW - 1] * 4
    packed = coracle_py.Packed(ir.Batch(progs))
    want = [packed.first_sat(s, GSEED, BUDGET) for s in range(len(progs))]
    assert [x is None for x in want] == ["/identity/" in nm for nm in names]
    db = engine.upload(progs)
    try:
        res = engine.check(db, budget=BUDGET, seed=GSEED, flags=flags)
    finally:
        db.free()
    got = [None if f == NOT_FOUND else int(f) for f in res.found]
    assert got == want, list(zip(names, got, want))


# ---- climb ------------------------------------------------------------------------------------

@pytest.mark.parametrize("per_round", [64, 65])
def test_climb_scores_b_unit_sites(engine, per_round):
    """MODE_CLIMB: BGET(d) * PF_CLIMB_HOLDS on the fused B_XOR, B_ITE and B_FILL, the plain
    ASSERTs after a B_VAR and a B_UMUL_NOOVF, and a pressure program's spills."""
    progs = [C.pressure_program("p40/free/narrow")[1], C.fused_all(0), C.fused_all(8),
             C.pressure_program("p64x/free/r16")[1]]
    got, want = both(engine, progs, [0, 1, 2, 3], 3, per_round, 0xC11B)
    assert_same(got, want, [p.name for p in progs])
    assert {int(s) % ir.CLIMB_HOLDS for s in got.score[1:3]} == {0}
