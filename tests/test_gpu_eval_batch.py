"""GPU: pf_eval_batch / pf_eval_batch_dev (include/pf_bytecode.h, stream contract) — explicit
candidates streamed through every requested set of a resident batch by pf_eval_stream_kernel
(the 8-register file, W registers 5 and 6 in LDS) and pf_eval_stream_r16_kernel, against the
oracle model of tests/stream_model.py, bit for bit.

* a batch of 24 config-3 sets, narrow and wide, 200 candidates — the generator's values under the
  oracle, the planted witness at index 137: bits, first, count, the counters, and
  pf_eval_assignments set by set; the sizes 1, 64 and 65 and partial, reversed, single and empty
  requests; PF_FLAG_SHORTCIRCUIT on and off; absent outputs; the device entry point on a side
  stream into buffers pre-filled with 0xFF;
* operations through the new kernels: the Bool-file programs of bool_file_cases.py (B ops, B
  spills to scratch and LDS, fused asserts), EXP over rows of exp_scale_cases.py and the divider
  and UMUL_NOOVF over rows of div_trim_cases.py, with operands, results and a guard value in
  registers 5 and 6 (narrow) and 13 and 14 (wide);
* the errors, each with a message and no output touched."""

import ctypes
import functools

import bool_file_cases as C
import div_trim_cases as D
import exp_scale_cases as S
import numpy as np
import op_programs as P
import pyoracle as O
import pytest
import stream_model as M
from test_gpu_search_schedule import _dag_of

from mythril_amd import _lib, ir, synth
from mythril_amd.lower import lower

pytestmark = pytest.mark.gpu

N_SETS, N_CAND, PLANT, SEED = 24, 200, 137, 0x57AE


# ---- the config-3 batch ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def main_case():
    """(programs, batch, per-set candidates, the oracle's verdict rows, which sets are wide):
    every third set lowered over 15 registers, the rest as synth lowers them."""
    progs, wits = [], []
    for i in range(N_SETS):
        dag_id = 31_000 + 5 * i
        prog, wit = synth.random_dag_set(dag_id, plant=False)
        if i % 3 == 1:
            prog = lower(_dag_of(dag_id), seed=prog.seed, name=f"dag{dag_id}/r16", nw=ir.NW)
        progs.append(prog)
        wits.append(list(wit))
    wide = [M.is_wide(p) for p in progs]
    assert any(wide) and not all(wide), wide           # both kernels run
    batch = ir.Batch(progs)
    cands = []
    for s in range(N_SETS):
        a = O.SetView.from_batch(batch, s).gen_assignments(np.arange(N_CAND, dtype=np.uint64), SEED)
        a[PLANT] = wits[s]
        cands.append(a)
    rows = M.verdicts(batch, cands)
    assert all(r[PLANT] for r in rows)
    return progs, batch, cands, rows, wide


def sized(n_cand, plant):
    """The first n_cand candidates of the main case with the witness moved to ``plant``: the
    reference rows are the main case's, not evaluated again."""
    _, batch, cands, rows, _ = main_case()
    wit = [c[PLANT] for c in cands]
    cs = [c[:n_cand] for c in cands]
    rs = [list(r[:n_cand]) for r in rows]
    for s in range(N_SETS):
        cs[s][plant] = wit[s]
        rs[s][plant] = True
    return ir.pack_soa(batch, cs), rs


@pytest.fixture(scope="module")
def db(engine):
    d = engine.upload(main_case()[1])
    yield d
    d.free()


def _same(res, rows, what=""):
    bits, first, count = M.summarize(rows)
    n_cand = len(rows[0]) if rows else res.n_cand
    print(what, "first", res.first.tolist(), "count", res.count.tolist())
    assert res.bits.shape == bits.shape and res.bits.dtype == np.uint64
    bad = [(i, c) for i, c in zip(*np.nonzero(M.unpack_bits(res.bits, n_cand) != np.array(rows, dtype=bool)))] \
        if rows else []
    assert not bad, (what, bad[:8])
    assert np.array_equal(res.bits, bits), what        # the tail bits too
    assert M.tail_is_zero(res.bits, n_cand)
    assert res.first.tolist() == first.tolist(), what
    assert res.count.tolist() == count.tolist(), what
    assert np.array_equal(res.verdicts(), np.array(rows, dtype=bool).reshape(len(rows), n_cand))


def test_batch_against_the_model_and_eval_assignments(engine, db):
    _, batch, cands, rows, _ = main_case()
    soa = ir.pack_soa(batch, cands)
    res = engine.eval_batch(db, soa)
    _same(res, rows, "all sets")
    assert res.first.tolist() == [min(PLANT, r.index(True)) for r in rows]
    assert res.cands_decided == N_SETS * N_CAND and res.n_sat == N_SETS and res.kernel_ms > 0
    assert 0 < res.evals_full <= res.cands_decided
    full = engine.eval_batch(db, soa, shortcircuit=False)
    _same(full, rows, "no short-circuit")
    assert full.evals_full == full.cands_decided == N_SETS * N_CAND and full.n_sat == N_SETS
    got = res.verdicts()
    for s in range(N_SETS):
        off, nv = int(batch.descs[s][4]), int(batch.descs[s][5])
        one = engine.eval_assignments(db, s, soa[off:off + nv])
        assert np.array_equal(one, got[s]), s


@pytest.mark.parametrize("n_cand", [1, 64, 65])
def test_sizes(engine, db, n_cand):
    """One lane, one full wave, one wave and a lane: the witness in the last candidate."""
    soa, rows = sized(n_cand, n_cand - 1)
    for sc in (True, False):
        res = engine.eval_batch(db, soa, shortcircuit=sc)
        _same(res, rows, f"n_cand {n_cand} sc {sc}")
        assert res.cands_decided == N_SETS * n_cand and res.n_sat == N_SETS


@pytest.mark.parametrize("chunk", [1, 2, 3, 64])
def test_items_of_several_groups(engine, db, monkeypatch, chunk):
    """A large call hands a wave runs of consecutive groups (one atomicMin and one atomicAdd per
    run); PF_STREAM_CHUNK_GROUPS forces that at 200 candidates — 4 groups: runs of 2 + 2, of
    3 + 1 and one run of all 4 — where the smallest witness is in the run's second or third
    group and other groups of the run hold witnesses too."""
    monkeypatch.setenv("PF_STREAM_CHUNK_GROUPS", str(chunk))
    _, batch, cands, rows, _ = main_case()
    wit = [c[PLANT] for c in cands]
    cs = [list(c) for c in cands]
    rs = [list(r) for r in rows]
    for s in range(N_SETS):
        for c in (70 + s, 199):                 # witnesses in groups 1, 2 (137) and 3
            cs[s][c] = wit[s]
            rs[s][c] = True
    soa = ir.pack_soa(batch, cs)
    for ids in (None, [5, 4, 22]):
        res = engine.eval_batch(db, soa, set_ids=ids)
        pick = range(N_SETS) if ids is None else ids
        _same(res, [rs[s] for s in pick], f"chunk {chunk}")
        assert all(res.count[i] >= 3 for i in range(len(res.count))) and res.n_sat == len(res.count)
        assert res.cands_decided == len(res.count) * N_CAND


def _requests():
    wide = main_case()[4]
    return {"wide": [s for s in range(N_SETS) if wide[s]], "narrow": [s for s in range(N_SETS) if not wide[s]],
            "reverse": list(range(N_SETS))[::-1], "single": [7], "single_wide": [4], "empty": []}


@pytest.mark.parametrize("name", ["wide", "narrow", "reverse", "single", "single_wide", "empty"])
def test_requests(engine, db, name):
    _, batch, cands, rows, wide = main_case()
    ids = _requests()[name]
    assert name != "single_wide" or wide[ids[0]]
    soa = ir.pack_soa(batch, cands)
    # rows of sets that are not requested are never read: poison them
    keep = np.zeros(soa.shape[0], dtype=bool)
    for s in ids:
        keep[int(batch.descs[s][4]):int(batch.descs[s][4]) + int(batch.descs[s][5])] = True
    soa[~keep] = 0xDEADBEEF
    res = engine.eval_batch(db, soa, set_ids=ids)
    if not ids:
        assert res.bits.shape == (0, 4) and res.first.size == 0 and res.count.size == 0
        assert (res.cands_decided, res.n_sat, res.evals_full) == (0, 0, 0)
        return
    _same(res, [rows[s] for s in ids], name)
    assert res.cands_decided == len(ids) * N_CAND and res.n_sat == len(ids)
    # the same request again (its tables are resident), then another one
    _same(engine.eval_batch(db, soa, set_ids=ids), [rows[s] for s in ids], name + " again")
    other = [ids[0]]
    _same(engine.eval_batch(db, soa, set_ids=other), [rows[s] for s in other], name + " then one")


def test_no_candidates(engine, db):
    soa = np.zeros((main_case()[1].schema.shape[0], 8, 0), dtype=np.uint32)
    res = engine.eval_batch(db, soa)
    assert res.bits.shape == (N_SETS, 0) and (res.first == M.NONE).all() and not res.count.any()
    assert res.cands_decided == 0 and res.n_sat == 0


def _raw(db, ids, soa, flags, bits, first, count):
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    st = _lib.pf_stats()
    rc = _lib.lib().pf_eval_batch(db.handle, _lib.ptr_u32(ids) if len(ids) else None, len(ids),
                                  _lib.ptr_u32(soa.reshape(-1)), soa.shape[2], flags,
                                  _lib.ptr_u64(bits.reshape(-1)) if bits is not None else None,
                                  _lib.ptr_u32(first) if first is not None else None,
                                  _lib.ptr_u32(count) if count is not None else None, ctypes.byref(st))
    return rc, _lib.lib().pf_last_error().decode(), st


def test_absent_outputs(engine, db):
    """bits absent with first given, first and count absent with bits given, count alone."""
    _, batch, cands, rows, _ = main_case()
    soa = ir.pack_soa(batch, cands)
    want_bits, want_first, want_count = M.summarize(rows)
    ids = list(range(N_SETS))
    first = np.full(N_SETS, 0x55555555, dtype=np.uint32)
    rc, msg, st = _raw(db, ids, soa, ir.FLAG_SHORTCIRCUIT, None, first, None)
    assert rc == 0, msg
    assert first.tolist() == want_first.tolist() and st.n_sat == N_SETS
    bits = np.full(want_bits.shape, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    rc, msg, st = _raw(db, ids, soa, 0, bits, None, None)
    assert rc == 0, msg
    assert np.array_equal(bits, want_bits) and st.n_sat == N_SETS
    count = np.full(N_SETS, 0x55555555, dtype=np.uint32)
    rc, msg, st = _raw(db, ids, soa, 0, None, None, count)
    assert rc == 0, msg
    assert count.tolist() == want_count.tolist() and st.n_sat == N_SETS


# ---- the device entry point -------------------------------------------------------------------

@pytest.mark.parametrize("n_cand", [65, N_CAND])
def test_device_path_on_a_side_stream(engine, db, n_cand):
    """Torch tensors in, torch tensors out, on a stream that is not the current one; the output
    buffers start as 0xFF bytes, so a word or a tail bit left unwritten shows."""
    import torch

    soa, rows = sized(n_cand, n_cand - 1) if n_cand != N_CAND else (ir.pack_soa(main_case()[1], main_case()[2]),
                                                                     main_case()[3])
    host = engine.eval_batch(db, soa)
    _same(host, rows, "host")
    d_soa = torch.from_numpy(soa.view(np.int32)).to("cuda")
    words = (n_cand + 63) // 64
    side = torch.cuda.Stream()
    for ids in (None, list(range(N_SETS))[::-2]):
        n = N_SETS if ids is None else len(ids)
        out = (torch.full((n, words), -1, dtype=torch.int64, device="cuda"),
               torch.full((n,), -1, dtype=torch.int32, device="cuda"),
               torch.full((n,), -1, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        res = engine.eval_stream(db, d_soa, set_ids=ids, out=out, stream=side)
        side.synchronize()
        assert res.bits is out[0] and res.first is out[1] and res.count is out[2]
        pick = list(range(N_SETS)) if ids is None else ids
        assert np.array_equal(res.bits.cpu().numpy().view(np.uint64), host.bits[pick])
        assert np.array_equal(res.first.cpu().numpy().view(np.uint32), host.first[pick])
        assert np.array_equal(res.count.cpu().numpy().view(np.uint32), host.count[pick])
        assert np.array_equal(res.verdicts(), host.verdicts()[pick])
    # absent outputs, new tensors, the current stream
    res = engine.eval_stream(db, d_soa, out=(None, torch.full((N_SETS,), -1, dtype=torch.int32, device="cuda"), None))
    torch.cuda.synchronize()
    assert res.bits is None and np.array_equal(res.first.cpu().numpy().view(np.uint32), host.first)
    res = engine.eval_stream(db, d_soa, out=(torch.full((N_SETS, words), -1, dtype=torch.int64, device="cuda"),
                                             None, None))
    torch.cuda.synchronize()
    assert res.first is None and res.count is None
    assert np.array_equal(res.bits.cpu().numpy().view(np.uint64), host.bits)
    res = engine.eval_stream(db, d_soa, shortcircuit=False)
    torch.cuda.synchronize()
    assert np.array_equal(res.bits.cpu().numpy().view(np.uint64), host.bits)
    assert np.array_equal(res.count.cpu().numpy().view(np.uint32), host.count)
    with pytest.raises(_lib.PathFeasError, match="variable rows"):
        engine.eval_stream(db, d_soa[1:])
    with pytest.raises(_lib.PathFeasError, match="shape"):
        engine.eval_stream(db, d_soa, out=(torch.zeros((N_SETS, words + 1), dtype=torch.int64, device="cuda"),
                                           None, None))


# ---- errors -----------------------------------------------------------------------------------

def test_errors_launch_nothing(engine, db):
    _, batch, cands, _, _ = main_case()
    soa = ir.pack_soa(batch, [c[:65] for c in cands])
    cases = {"out of range": ([0, N_SETS], ir.FLAG_SHORTCIRCUIT, True, "out of range"),
             "repeated": ([3, 5, 3], 0, True, "twice"),
             "unknown flag": ([0, 1], ir.FLAG_SHORTCIRCUIT | ir.FLAG_EARLY_EXIT, True, "flag"),
             "no output": ([0, 1], 0, False, "output")}
    for name, (ids, flags, outs, word) in cases.items():
        bits = np.full((len(ids), 2), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64) if outs else None
        first = np.full(len(ids), 0xA5A5A5A5, dtype=np.uint32) if outs else None
        count = np.full(len(ids), 0xA5A5A5A5, dtype=np.uint32) if outs else None
        rc, msg, _ = _raw(db, ids, soa, flags, bits, first, count)
        assert rc < 0 and word in msg and "pf_eval_batch" in msg, (name, rc, msg)
        if outs:
            assert (bits == 0xA5A5A5A5A5A5A5A5).all() and (first == 0xA5A5A5A5).all() and (count == 0xA5A5A5A5).all()
    with pytest.raises(_lib.PathFeasError, match="out of range"):
        engine.eval_batch(db, soa, set_ids=[N_SETS])
    # the device entry point makes the same checks
    import torch

    d_soa = torch.from_numpy(soa.view(np.int32)).to("cuda")
    with pytest.raises(_lib.PathFeasError, match="twice"):
        engine.eval_stream(db, d_soa, set_ids=[1, 1])
    with pytest.raises(_lib.PathFeasError, match="output"):
        engine.eval_stream(db, d_soa, out=(None, None, None))
    # and the batch still answers
    res = engine.eval_batch(db, soa, set_ids=[2])
    assert res.cands_decided == 65


# ---- operations through the new kernels ---------------------------------------------------------

def _run_sets(engine, sets, what):
    """sets: (name, program, candidates, expected verdicts), every set with the same number of
    candidates.  One upload, one call per short-circuit setting."""
    batch = ir.Batch([p for _, p, _, _ in sets])
    soa = ir.pack_soa(batch, [c for _, _, c, _ in sets])
    rows = M.verdicts(batch, [c for _, _, c, _ in sets])
    for (name, _, _, want), r in zip(sets, rows):
        assert want is None or r == [bool(x) for x in want], name
    d = engine.upload(batch)
    try:
        for sc in (True, False):
            res = engine.eval_batch(d, soa, shortcircuit=sc)
            got = res.verdicts()
            bad = [(name, np.flatnonzero(got[s] != np.array(rows[s]))[:8].tolist())
                   for s, (name, _, _, _) in enumerate(sets) if got[s].tolist() != rows[s]]
            assert not bad, (what, sc, len(bad), bad[:6])
            _same(res, rows, what)
    finally:
        d.free()
    return rows


@pytest.mark.parametrize("upload", ["folded", "unfolded"])
def test_bool_file_programs(engine, upload):
    """The Bool register file, B spills to scratch and to LDS entries, fused asserts, the pressure
    programs lowered for both register files: 65 candidates, a B file of its own per lane."""
    from test_gpu_bool_file import _explicit_sets

    sets = list(_explicit_sets(65))
    kinds = {M.is_wide(p) for _, p, _, _ in sets}
    assert kinds == {False, True} and len(sets) >= C.FOLD_MIN_SETS > C.CHUNK
    for part in [sets] if upload == "folded" else C.chunks(sets):
        rows = _run_sets(engine, part, f"bool file ({upload})")
        assert any(any(r) and not all(r) for r in rows)


OPS = {"exp": (ir.W_EXP, O.bvexp), "udiv": (ir.W_UDIV, O.bvudiv), "urem": (ir.W_UREM, O.bvurem),
       "sdiv": (ir.W_SDIV, O.bvsdiv), "smod": (ir.W_SMOD, O.bvsmod), "umul_noovf": (ir.B_UMUL_NOOVF, O.umul_noovf)}
# (ra, rb, rd, guard, scratch for the expectation, scratch for the guard's twin): the result and the
# guard in registers 5 and 6 — LDS in the narrow kernel, next to EXP's window table and the entry
# UMUL_NOOVF parks its operand in — or both operands there
REGS = ((0, 1, 5, 6, 2, 3), (5, 6, 2, 4, 0, 1), (6, 0, 6, 5, 1, 2))


def op_set(op, w, regs, base):
    """vars a, b, g, e, g2: rd <- op(ra, rb) with g waiting in another register; ASSERT rd == e
    (UMUL_NOOVF: its bit == the Bool e) and ASSERT g == g2."""
    ra, rb, rd, rg, se, sg = regs
    s = P.Asm(f"op:{ir.OPNAMES[op]}/w{w}/{ra}.{rb}.{rd}.{rg}/base{base}", base, parents=False)
    s.wvar(ra, w, None)
    s.wvar(rb, w, None)
    s.wvar(rg, 256, None)
    if op == ir.B_UMUL_NOOVF:
        s.cmp(op, w, 2, ra, rb)
        s.bvar(3, None)
        s.b(ir.B_XOR, 4, a=2, b=3)
        s.b(ir.B_NOT, 5, a=4)
        s.p.emit(ir.ASSERT, 1, a=5)
    else:
        s.w(op, w, rd, ra, rb)
        s.wvar(se, w, None)
        s.cmp(ir.B_EQ, w, 0, rd, se)
        s.p.emit(ir.ASSERT, 1, a=0)
    s.wvar(sg, 256, None)
    s.cmp(ir.B_EQ, 256, 1, rg, sg)
    s.p.emit(ir.ASSERT, 1, a=1)
    return s.done(verdict=None)


@functools.lru_cache(maxsize=None)
def op_pairs(name):
    if name == "exp":
        pairs = S.pairs(8, nrandom_bases=1)
        return pairs[::max(1, len(pairs) // 20)][:20]
    if name in ("udiv", "urem"):
        return [(a, b) for _, a, b in D.all_rows(8)]
    if name in ("sdiv", "smod"):
        return [((-a if k & 1 else a) & ir.mask(256), (-b if k & 2 else b) & ir.mask(256))
                for k, (_, a, b) in enumerate(D.all_rows(6))]
    rows = [(a, b) for _, a, b in D.all_rows(6)]
    small = [(a >> 140, b >> 150) for a, b in rows[::2]]
    edge = [(1 << 128, 1 << 128), ((1 << 128) - 1, (1 << 128) + 1), (ir.mask(256), 1), (ir.mask(256), 2), (0, 5), (7, 0)]
    return rows[::3] + small + edge


@pytest.mark.parametrize("name", list(OPS))
def test_ops_with_registers_5_and_6_in_lds(engine, name):
    """Every row as a candidate that holds and as two that do not (a wrong expectation, a wrong
    guard), interleaved in one wave; three register placements at both bases."""
    op, fn = OPS[name]
    pairs = op_pairs(name)
    assert len(pairs) >= 20
    cands, want = [], []
    for k, (a, b) in enumerate(pairs):
        r = int(fn(a, b, 256))
        g = P.GUARDS[k % len(P.GUARDS)]
        bad_r = (r ^ 1) if op == ir.B_UMUL_NOOVF else P.corrupt(r, 256, 7 * k)
        cands += [[a, b, g, r, g], [a, b, g, bad_r, g], [a, b, g, r, g ^ (1 << (k % 256))]]
        want += [True, False, False]
    if name == "umul_noovf":
        assert {bool(fn(a, b, 256)) for a, b in pairs} == {False, True}
    sets = [(f"{name}/{regs}/base{base}", op_set(op, 256, regs, base), cands, want)
            for base in (0, 8) for regs in REGS]
    assert [M.is_wide(p) for _, p, _, _ in sets] == [False] * 3 + [True] * 3
    _run_sets(engine, sets, name)


def test_values_are_masked_to_the_variables_width(engine):
    """Garbage above a variable's width changes nothing: the kernels mask as pf_eval_assignments
    does (ir.pack_soa passes all 256 bits through)."""
    progs = [P.cmp_set(ir.B_ULT, 8, 0, 0, True, regs=(5, 6), parents=False),
             P.cmp_set(ir.B_EQ, 200, 0, 0, True, regs=(5, 6), base=8, parents=False),
             P.bool_set(ir.B_AND, (1, 1), True, parents=False)]
    rng = np.random.default_rng(8)
    top = lambda: int.from_bytes(rng.bytes(32), "little") & ~ir.mask(200)
    c8 = [[(k % 7) | top(), (k % 5) | top()] for k in range(65)]
    c200 = [[(k * k) | top(), (k * k + k % 2) | top()] for k in range(65)]
    cb = [[(k & 1) | (top() << 1) & ir.mask(256), ((k >> 1) & 1) | 2] for k in range(65)]
    sets = [("ult/w8", progs[0], c8, [k % 7 < k % 5 for k in range(65)]),
            ("eq/w200", progs[1], c200, [k % 2 == 0 for k in range(65)]),
            ("and/bool", progs[2], cb, [(k & 3) == 3 for k in range(65)])]
    _run_sets(engine, sets, "masking")
