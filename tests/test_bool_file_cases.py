"""CPU: the Bool-register-file programs of tests/bool_file_cases.py are what they claim to be,
before tests/test_gpu_bool_file.py runs them on the device.

* the three oracles (pyoracle's SetView.evaluate, the C restatement, dag_eval on the DAG) agree
  on them, and with the builders' own bookkeeping;
* lower() and lower_py() emit the same code for the pressure DAGs, with B_SPILL / B_FILL in it;
* their device programs hold B spills in private scratch and in LDS, no LDS segment across a
  W_EXP and no entry-1 segment across a B_UMUL_NOOVF, ASSERTs fused into writers further back
  and into B_FILLs — and the Python device evaluator (test_device_program.eval_device) gives
  the oracle's verdict on every candidate — on the device program as uploaded
  (pf_device_batch), in a small upload that pf_batch_create does not fold, in a folded one and
  under PF_DEVICE_FOLD=0 (LEGS below);
* the fold pass turns a B_CONST and a B_XOR r, r into constants, so their BSET runs on the
  device only in the small uploads: the unfolded program still holds them;
* sensitivity: complementing any single B_FILL of any device program the GPU tests upload, or
  any single B register of a slot set, changes the verdict of at least one candidate of the
  set the GPU test uses;
* balance: between 1/4 and 3/4 of every explicit set hold."""

import copy
import ctypes
import functools
import numpy as np
import pytest

import bool_file_cases as C
import coracle_py
import pyoracle as O
from dag_eval import eval_dag
from mythril_amd import _lib, ir
from mythril_amd.lower import LoweringError, lower, lower_py
from test_device_program import I_ASSERT, SPILL_LDS, eval_device

N_EXPLICIT = 65          # the smaller of the GPU test's candidate counts
# The device program of a set as pf_batch_create uploads it (pf_device_batch: the same gate,
# the device constant pool), in the three forms the GPU tests meet:
#   "small"  a batch below PF_FOLD_MIN_SETS sets, which the fold pass leaves alone: the pressure
#            (4 sets), fused (12) and climb (4) uploads and the chunked uploads of the slot sets;
#   "batch"  a batch of PF_FOLD_MIN_SETS sets or more, folded: the whole-op uploads of the slot
#            and spill sets, the explicit-candidate uploads and pf_eval_programs' 16 sets;
#   "fold0"  such a batch under PF_DEVICE_FOLD=0.
LEGS = ("small", "batch", "fold0")


def c_eval_explicit(batch, s, assignments):
    """The C oracle's verdicts of explicit assignments of set s."""
    pk = coracle_py.Packed(batch)
    vals = np.ascontiguousarray(ir.limbs_array([x for a in assignments for x in a]).reshape(-1))
    out = np.zeros(len(assignments), dtype=np.uint8)
    rc = coracle_py.lib().co_eval_explicit(*pk.ptrs(), s, vals.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                           len(assignments), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    assert rc == 0
    return [bool(x) for x in out]


def rows_of(code, descs, s=0):
    d = descs[s]
    return [tuple(int(x) for x in r) for r in code[d[0]:d[0] + d[1]]]


def uploaded(monkeypatch, prog, leg, sv):
    """(rows, view) of the device program of ``prog`` in an upload of form ``leg``; the view is
    ``sv`` with the device pool's constants, which the rows index."""
    if leg == "fold0":
        monkeypatch.setenv("PF_DEVICE_FOLD", "0")
    else:
        monkeypatch.delenv("PF_DEVICE_FOLD", raising=False)
    batch = ir.Batch([prog] * (1 if leg == "small" else C.FOLD_MIN_SETS))
    code, descs, pool = _lib.device_batch(batch.code, batch.consts, batch.descs)
    dev = copy.copy(sv)
    dev.consts = [O.limbs_to_int(r) for r in pool[int(descs[0][2]):]]
    assert dev.consts[:len(sv.consts)] == sv.consts
    return rows_of(code, descs), dev


@functools.lru_cache(maxsize=None)
def hand_case(name):
    """(program, assignments, builder's verdicts, SetView, oracle verdicts) of a soa case."""
    prog, cands, verdicts = C.explicit_case(name, N_EXPLICIT)
    sv = O.SetView.from_batch(ir.Batch([prog]), 0)
    return prog, cands, verdicts, sv, [sv.evaluate(v) for v in cands]


@functools.lru_cache(maxsize=None)
def pressure_case(name):
    """(dag, program, assignments, SetView, oracle verdicts) of a pressure program's explicit
    form."""
    dag, prog, cands = C.pressure_explicit(name, N_EXPLICIT)
    sv = O.SetView.from_batch(ir.Batch([prog]), 0)
    return dag, prog, cands, sv, [sv.evaluate(v) for v in cands]


HAND = [name for name, _ in C.soa_cases()]
FREE = [name for name in C.PRESSURE if "/free/" in name]


# ---- oracles --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(C.PRESSURE))
def test_oracles_agree_on_the_pressure_dags(name):
    dag, prog, cands, sv, want = pressure_case(name)
    assert [eval_dag(dag, v) for v in cands] == want
    assert c_eval_explicit(ir.Batch([prog]), 0, cands) == want
    if "/identity/" in name:
        assert not any(want)
    # ... and on generated candidates, the form the search runs (rare as named)
    _, gen = C.pressure_program(name)
    batch = ir.Batch([gen])
    gv = O.SetView.from_batch(batch, 0)
    assign = gv.gen_assignments(np.arange(48, dtype=np.uint64), 11)
    assert list(coracle_py.Packed(batch).eval_generated(0, 11, 0, 48)) == [gv.evaluate(v) for v in assign]


def test_oracles_agree_with_the_hand_emitted_sets():
    assert len(HAND) == len(set(HAND)) and len(HAND) >= 50
    for name in HAND:
        prog, cands, verdicts, sv, want = hand_case(name)
        assert want == verdicts, name
        assert c_eval_explicit(ir.Batch([prog]), 0, cands) == want, name


def test_candidate_0_forms_hold_and_their_corrupted_copies_do_not():
    """The programs of the search tests (parents on every variable): the builder's verdict is
    the oracle's at the parent values."""
    progs = []
    for op in C.BFILE_OPS:
        for k, t in enumerate(C.bfile_tuples(op)):
            word = C.bfile_word(op, *t, seed=k)
            assert C.bfile_result_differs(op, *t, word), (op, t)     # a lost write would show
            progs += [C.bfile_set(op, *t, word, wrong=None), C.bfile_set(op, *t, word, base=8, wrong=t[3])]
    for variant in C.SPILL_VARIANTS:
        for rot in range(5):
            progs += [C.bspill_set(variant, 0xA5C3_0F96 ^ rot, base=8 * (rot & 1), rot=rot, wrong=w) for w in (None, 31)]
    assert {p.verdict for p in progs} == {True, False}
    batch = ir.Batch(progs)
    for s, p in enumerate(progs):
        sv = O.SetView.from_batch(batch, s)
        assert sv.evaluate(sv.parents) == p.verdict and sv.parents == p.assignment, p.name


# ---- lowering --------------------------------------------------------------------------------

@pytest.mark.parametrize("nw", [15, 7])
@pytest.mark.parametrize("n", [34, 40, 64, 90])
@pytest.mark.parametrize("clobber", [False, True])
def test_native_and_python_lowering_agree_and_spill_bools(n, clobber, nw):
    dag = C.bool_pressure_dag(n, clobber, "free", rare=2)
    native, py = lower(dag, seed=3, nw=nw), lower_py(dag, seed=3, nw=nw)
    assert isinstance(native, ir.PackedProgram)              # the native library did lower it
    assert [i.words()[:3] for i in native.code] == [i.words()[:3] for i in py.code]
    assert native.consts == py.consts
    ops = [i.op for i in py.code]
    assert ops.count(ir.B_SPILL) >= n - 32 and ops.count(ir.B_FILL) >= n - 32
    assert max(i.dst for i in py.code if i.op < ir.B_CONST and i.op != ir.W_SPILL) < nw


@pytest.mark.parametrize("nw", [15, 7])
def test_both_lowerings_reject_more_bools_than_spill_slots_can_hold(nw):
    dag = C.bool_pressure_dag(100)
    with pytest.raises(LoweringError) as e_native:
        lower(dag, nw=nw)
    with pytest.raises(LoweringError) as e_py:
        lower_py(dag, nw=nw)
    assert str(e_native.value) == str(e_py.value) == "more than 32 live B values"


# ---- device programs ---------------------------------------------------------------------------

def segments(rows):
    """(spill row, fill rows, slot word) of every spill segment of a device program."""
    open_, out = {}, []
    for i, (w0, _, aux0, _) in enumerate(rows):
        op = w0 & 0xFF
        if op in (ir.W_SPILL, ir.B_SPILL):
            open_[aux0] = len(out)
            out.append((i, [], aux0))
        elif op in (ir.W_FILL, ir.B_FILL):
            out[open_[aux0]][1].append(i)
    return out


def check_slots(rows):
    """No LDS segment spans a W_EXP, no entry-1 segment a B_UMUL_NOOVF, and no two segments
    of one LDS entry overlap.  -> (B spills in LDS, B spills in scratch)."""
    ops = [w0 & 0xFF for (w0, _, _, _) in rows]
    busy = {}
    n_lds = n_scratch = 0
    for spill, fills, aux0 in segments(rows):
        is_b = ops[spill] == ir.B_SPILL
        if not aux0 & SPILL_LDS:
            assert aux0 < ir.MAX_SPILL
            n_scratch += is_b
            continue
        e = aux0 & 0xFF
        assert e in (1, 2, 3) and fills
        inside = ops[spill:fills[-1]]
        assert ir.W_EXP not in inside
        assert e != 1 or ir.B_UMUL_NOOVF not in inside
        assert busy.get(e, -1) < spill
        busy[e] = fills[-1]
        n_lds += is_b
    return n_lds, n_scratch


@pytest.mark.parametrize("leg", LEGS)
def test_device_programs_of_the_pressure_dags(monkeypatch, leg):
    lds = scratch = 0
    for name in sorted(C.PRESSURE):
        _, prog, cands, sv, want = pressure_case(name)
        rows, dev = uploaded(monkeypatch, prog, leg, sv)
        a, b = check_slots(rows)
        assert a + b >= C.PRESSURE[name][0] - 32, name
        lds, scratch = lds + a, scratch + b
        if "x/" in name:       # the EXP and both overflow tests are still there to cross
            ops = [w0 & 0xFF for (w0, _, _, _) in rows]
            assert ops.count(ir.W_EXP) == 1 and ops.count(ir.B_UMUL_NOOVF) == 2, name
        assert [eval_device(dev, rows, v) for v in cands] == want, name
    assert lds >= 8 and scratch >= 8


@pytest.mark.parametrize("leg", LEGS)
def test_device_programs_of_the_hand_emitted_sets(monkeypatch, leg):
    lds = scratch = far = on_fill = plain = 0
    for name in HAND:
        prog, cands, _, sv, want = hand_case(name)
        rows, dev = uploaded(monkeypatch, prog, leg, sv)
        assert [eval_device(dev, rows, v) for v in cands] == want, name
        a, b = check_slots(rows)
        if name.startswith("bspill"):
            assert a + b == len(C.SPILL_REGS), name
            # crossed by an EXP: all in scratch; by an overflow test: not entry 1
            assert a == {"exp": 0, "umul": 2, "plain": 3}[name.split(":")[1].split("/")[0]], name
        lds, scratch = lds + a, scratch + b
        if name.startswith("fused"):
            src = [i.op for i in prog.code]
            ops = [w0 & 0xFF for (w0, _, _, _) in rows]
            fused = [i for i, (w0, _, _, _) in enumerate(rows) if w0 & I_ASSERT]
            kind = name.split(":")[1].split("/")[0]
            # the first ASSERT's writer: a B_XOR or B_FILL several instructions back takes it;
            # a B_VAR or B_UMUL_NOOVF does not, and the plain ASSERT stays
            if kind in ("far", "fill"):
                writer = {"far": ir.B_XOR, "fill": ir.B_FILL}[kind]
                at = [i for i in fused if ops[i] == writer]
                assert len(at) == 1 and ops.count(ir.ASSERT) == 0, name
                assert src.index(ir.ASSERT) - max(i for i, o in enumerate(src) if o == writer) >= 4
                far += kind == "far"
                on_fill += kind == "fill"
            else:
                assert ops.count(ir.ASSERT) == 1 and len(fused) == 1, name
                plain += 1
    assert lds > 0 and scratch > 0 and far >= 2 and on_fill >= 2 and plain >= 4


def test_small_uploads_are_not_folded(monkeypatch):
    """The gate, as the tests rely on it: below PF_FOLD_MIN_SETS sets the device program is the
    PF_DEVICE_FOLD=0 one, and a B_CONST or B_XOR r, r still writes its register there (the fold
    pass knows their value and deletes them: B_CONST's BSET runs in the small uploads only)."""
    kept = 0
    for op in (ir.B_CONST, ir.B_XOR):
        for group in C.bfile_rows(op, 0) + C.bfile_rows(op, 8):
            p = group[0]
            ins = next(i for i in p.code if i.op == op)
            if op == ir.B_XOR and ins.a != ins.b:
                continue
            sv = O.SetView.from_batch(ir.Batch([p]), 0)
            small, _ = uploaded(monkeypatch, p, "small", sv)
            assert small == uploaded(monkeypatch, p, "fold0", sv)[0]
            writes = [(w0 & 0xFF, w1 & 0xFF) for (w0, w1, _, _) in small]
            assert (op, ins.dst) in writes, p.name
            folded, _ = uploaded(monkeypatch, p, "batch", sv)
            assert op not in [w0 & 0xFF for (w0, _, _, _) in folded], p.name
            kept += 1
    assert kept >= 37 + 5            # every rd of B_CONST at base 0, the five B_XOR r, r


@pytest.mark.parametrize("leg", LEGS[:2])
def test_the_climb_sets_fuse_and_keep_asserts(monkeypatch, leg):
    p = C.fused_all()
    rows, _ = uploaded(monkeypatch, p, leg, O.SetView.from_batch(ir.Batch([p]), 0))
    fused = sorted(w0 & 0xFF for (w0, _, _, _) in rows if w0 & I_ASSERT)
    assert fused == sorted([ir.B_XOR, ir.B_FILL, ir.B_ITE])
    assert [w0 & 0xFF for (w0, _, _, _) in rows].count(ir.ASSERT) == 2


# ---- sensitivity and balance --------------------------------------------------------------------

def flips_verdict(sv, rows, cands, want, row, reg):
    """Does complementing B[reg] right after ``row`` change some candidate's verdict?  None
    when the device program has not written B[reg] by then."""
    seen = []

    def hook(i, B):
        if i == row:
            seen.append(reg in B)
            if reg in B:
                B[reg] = not B[reg]
    got = any(eval_device(sv, rows, v, hook) != w for v, w in zip(cands, want))
    return got if all(seen) else None


def fills_of(rows):
    return [(i, w1 & 0xFF) for i, (w0, w1, _, _) in enumerate(rows) if w0 & 0xFF == ir.B_FILL]


@functools.lru_cache(maxsize=None)
def searched_cases():
    """(name, program, candidates, SetView, oracle verdicts) of what the search and climb
    tests upload beyond the explicit sets: every spill rotation with its corrupted copies as
    the candidates, the pressure programs as searched (with their q_j) under the generated
    candidates whose q_j all hold, and the climb's fused set under generated candidates."""
    out = []
    for base in (0, 8):
        for group in C.bspill_rows(base):
            out.append((group[0].name, group[0], [p.assignment for p in group]))
    cand_ids = np.arange(C.BUDGET, dtype=np.uint64)
    for name in sorted(C.PRESSURE):
        _, prog = C.pressure_program(name)
        gen = O.SetView.from_batch(ir.Batch([prog]), 0).gen_assignments(cand_ids, C.GSEED)
        out.append((name + "/searched", prog, [v for v in gen if all(v[8:])][:48]))
    for base in (0, 8):
        p = C.fused_all(base)
        out.append((p.name, p, O.SetView.from_batch(ir.Batch([p]), 0).gen_assignments(cand_ids[:64], C.GSEED)))
    done = []
    for name, prog, cands in out:
        sv = O.SetView.from_batch(ir.Batch([prog]), 0)
        done.append((name, prog, cands, sv, [sv.evaluate(v) for v in cands]))
    return done


@pytest.mark.parametrize("leg", LEGS)
def test_every_fill_decides_some_verdict(monkeypatch, leg):
    n = 0
    cases = [(name,) + hand_case(name)[0:1] + hand_case(name)[1:2] + hand_case(name)[3:] for name in HAND]
    cases += [(name,) + pressure_case(name)[1:] for name in sorted(C.PRESSURE)]
    cases += searched_cases()
    for name, prog, cands, sv, want in cases:
        assert len(cands) >= 3, name
        rows, dev = uploaded(monkeypatch, prog, leg, sv)
        for row, reg in fills_of(rows):
            assert flips_verdict(dev, rows, cands, want, row, reg), (name, row, reg)
            n += 1
    assert n > 400


@pytest.mark.parametrize("leg", LEGS)
def test_every_register_of_the_slot_sets_decides_some_verdict(monkeypatch, leg):
    unwritten = set()
    for name in HAND:
        if not name.startswith(("bfile", "bspill")):
            continue
        prog, cands, _, sv, want = hand_case(name)
        rows, dev = uploaded(monkeypatch, prog, leg, sv)
        # the readout begins at the first W_ITE: every register is complemented right before it
        first = next(i for i, (w0, _, _, _) in enumerate(rows) if w0 & 0xFF == ir.W_ITE)
        for reg in range(ir.NB):
            got = flips_verdict(dev, rows, cands[:8], want[:8], first - 1, reg)
            if got is None:
                unwritten.add((name, reg))
            else:
                assert got, (name, reg)
    # In a folded upload the destination of a B_CONST or B_XOR r, r is no register any more
    # (test_small_uploads_are_not_folded); nothing else may be missing, and unfolded nothing is.
    # The GPU tests run these sets in small uploads too, where the leg "small" has checked them.
    if leg == "batch":
        assert unwritten and all(nm.startswith(("bfile:B_CONST", "bfile:B_XOR/31.31.")) for nm, _ in unwritten)
        assert all(f"d{reg}/" in hand_case(nm)[0].name for nm, reg in unwritten), unwritten
    else:
        assert not unwritten


def test_between_a_quarter_and_three_quarters_of_every_explicit_set_hold():
    for name in HAND:
        want = hand_case(name)[4]
        assert len(want) / 4 <= sum(want) <= 3 * len(want) / 4, (name, sum(want))
    for name in FREE:
        want = pressure_case(name)[4]
        assert len(want) / 4 <= sum(want) <= 3 * len(want) / 4, (name, sum(want))
