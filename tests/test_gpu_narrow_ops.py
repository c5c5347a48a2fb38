"""GPU parity, op by op, of the kernels a search runs: ``run_program<MODE_GEN, 8>``
(pf_check_kernel / pf_check_early_kernel: the 8-register file, registers 5 and 6 in LDS, the
inlined candidate generator) and ``<MODE_GEN, 16>`` (the r16 pair) — against oracle/pyoracle.py,
bit-exact.  test_gpu_parity.py's per-op tests call ``engine.eval_assignments``, which is
``run_program<MODE_SOA, 16>``: another instantiation.

An explicit assignment reaches a search kernel by the candidate-0 protocol (op_programs.py):
parents on every variable, ``budget=1``, ``found == 0`` iff the program holds.  ``base`` chooses
the register file (0: registers 0..6, the narrow kernels; 8: registers 8..14, the r16 kernels),
``flags`` the EARLY template constant.  Every row is also uploaded with its expectation
corrupted in one bit, and that copy must come out NOT_FOUND.

test_bool_ops here runs the B ops in five B registers of lane 0; test_gpu_bool_file.py covers the
whole B file, every lane, B spills and fused asserts."""

import functools

import coracle_py
import numpy as np
import op_programs as P
import pyoracle as O
import pytest
from conftest import load_golden
from test_gpu_parity import _CMPS, _OPS, _WIDTHS, _rand_operand

from mythril_amd import ir
from mythril_amd.engine import NOT_FOUND

pytestmark = pytest.mark.gpu

FLAGS = (0, ir.FLAG_EARLY_EXIT | ir.FLAG_SHORTCIRCUIT)
BASES = (0, 8)
both_kernels = [pytest.mark.parametrize("base", BASES), pytest.mark.parametrize("flags", FLAGS)]
SEED = 0x0C0DE_5EED

_FN = {"add": O.bvadd, "sub": O.bvsub, "mul": O.bvmul, "udiv": O.bvudiv, "urem": O.bvurem,
       "sdiv": O.bvsdiv, "srem": O.bvsrem, "smod": O.bvsmod, "shl": O.bvshl, "lshr": O.bvlshr,
       "ashr": O.bvashr, "exp": O.bvexp}
_CFN = {"ult": O.ult, "ule": O.ule, "slt": O.slt, "sle": O.sle, "uadd_noovf": O.uadd_noovf,
        "umul_noovf": O.umul_noovf}


def kernels(fn):
    for m in both_kernels:
        fn = m(fn)
    return fn


# A row is (builder, args before the expectation, expectation, width of the expectation,
# bit to corrupt, keyword arguments); rows do not depend on the kernel, programs do.
def _row(fn, args, expect, w, bit=0, **kw):
    return (fn, tuple(args), expect, w, bit, kw)


def _build(rows, base, **more):
    """Every row as a set that holds and as one whose expectation is wrong in one bit."""
    out = []
    for fn, args, expect, w, bit, kw in rows:
        wrong = (not expect) if isinstance(expect, bool) else P.corrupt(expect, w, bit)
        out.append(fn(*args, expect, base=base, verdict=True, **kw, **more))
        out.append(fn(*args, wrong, base=base, verdict=False, **kw, **more))
    return out


def _describe(progs, bad, got):
    return [(progs[i].name, "holds" if progs[i].verdict else "corrupted", str(got[i]),
             [hex(v) for v in progs[i].assignment], [hex(c) for c in progs[i].consts]) for i in bad[:4]]


def _search(engine, progs, flags, batch=None):
    """The candidate-0 protocol: one search of one candidate per set."""
    res = engine.check(engine.upload(batch if batch is not None else progs), budget=1, seed=SEED, flags=flags)
    want = np.array([0 if p.verdict else NOT_FOUND for p in progs], dtype=np.uint32)
    bad = np.nonzero(res.found != want)[0]
    assert bad.size == 0, (len(bad), _describe(progs, bad, res.found))
    return len(progs)


def _soa(engine, progs, garbage=None):
    """The same programs without parents, their assignment as one explicit candidate each
    (pf_eval_assignments: the SoA kernel)."""
    db = engine.upload(progs)
    got = []
    for s, p in enumerate(progs):
        soa = ir.pack_assignments(p, [p.assignment])
        if garbage is not None:
            for v, var in enumerate(p.vars):
                soa[v, :, 0] |= np.array(ir.to_limbs(garbage(var.width)), dtype=np.uint32)
        got.append(bool(engine.eval_assignments(db, s, soa)[0]))
    bad = [i for i, p in enumerate(progs) if got[i] != p.verdict]
    assert not bad, (len(bad), _describe(progs, bad, got))


def _run(engine, rows, base, flags):
    _search(engine, _build(rows, base), flags)
    return 2 * len(rows)


def _run_both(engine, rows, base, flags):
    """Search kernels, and (once per register file) the SoA kernel on the same programs."""
    _search(engine, _build(rows, base), flags)
    if flags == 0:
        _soa(engine, _build(rows, base, parents=False))


# ---- a. reference vectors ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _golden_rows(name):
    rows = []
    for v in load_golden("ops.json"):
        if v["op"] != name:
            continue
        a, b, w = int(v["a"], 16), int(v["b"], 16), v["w"]
        r = v["r"] if isinstance(v["r"], int) else int(v["r"], 16)
        if name in _OPS:
            rows.append(_row(P.binop_set, (_OPS[name], w, a, b), r, w))
        else:
            rows.append(_row(P.cmp_set, (_CMPS[name], w, a, b), bool(r), 1))
    return rows


@kernels
@pytest.mark.parametrize("name", sorted(_OPS) + sorted(_CMPS))
def test_golden_vectors_through_search(engine, name, base, flags):
    rows = _golden_rows(name)
    assert len(rows) == 564
    _run(engine, rows, base, flags)


@kernels
def test_eip145_through_search(engine, base, flags):
    rows = []
    for case in load_golden("eip145.json"):
        op = {"shl": ir.W_SHL, "shr": ir.W_LSHR, "sar": ir.W_ASHR}[case["op"]]
        # (value, shift) are the op's (a, b)
        rows.append(_row(P.binop_set, (op, 256, int(case["value"], 16), int(case["shift"], 16)),
                         int(case["expected"], 16), 256, bit=len(rows)))
    assert len(rows) == 38
    _run(engine, rows, base, flags)


# ---- b. edge families ---------------------------------------------------------------------

# the base x exponent grid of test_gpu_parity.test_exp_split_edges (locals there)
_M = ir.mask(256)
_EXP_EXPS = [0, 1, 2, 255, 256, 257, (1 << 84) - 1, 1 << 84, (1 << 84) + 1, (1 << 85) + 3,
             (1 << 126) + 5, (1 << 254) - 1, 1 << 254, (1 << 254) + 1, (1 << 255) + 7, _M, _M - 1]
_EXP_BASES = [0, 1, 2, 3, 5, 7, _M, _M - 1, 1 << 255, (1 << 255) + 1, 3 << 100, (1 << 84) + 1]


@functools.lru_cache(maxsize=None)
def _exp_rows(w, ground):
    rows = []
    for b in _EXP_BASES:
        for e in _EXP_EXPS:
            b_, e_ = b & ir.mask(w), e & ir.mask(w)
            r = O.bvexp(b_, e_, w)
            assert r == pow(b_, e_, 1 << w)
            rows.append(_row(P.ground_set if ground else P.binop_set, (ir.W_EXP, w, b_, e_), r, w,
                             bit=len(rows) * 7))
    return rows


@kernels
@pytest.mark.parametrize("ground", [False, True], ids=["var", "ground"])
@pytest.mark.parametrize("w", [256, 200, 64])
def test_exp_split_grid_through_search(engine, w, ground, base, flags):
    rows = _exp_rows(w, ground)
    assert len(rows) == len(_EXP_BASES) * len(_EXP_EXPS)
    _run(engine, rows, base, flags)


_DIV = {"udiv": ir.W_UDIV, "urem": ir.W_UREM, "sdiv": ir.W_SDIV, "srem": ir.W_SREM, "smod": ir.W_SMOD}


@functools.lru_cache(maxsize=None)
def _division_rows(name, family, ground):
    """256 operand pairs of test_division_one_limb_divisor_waves' / _one_digit_quotient_waves'
    generators."""
    rng = np.random.default_rng(0xD1 + len(name) + (0 if family == "one_limb" else 0x0D00))
    w, rows = 256, []
    for i in range(256):
        if family == "one_limb":
            a = _rand_operand(rng, w)
            b = [0, 1, 2, 3, 0xFFFFFFFF, 0x80000000, int(rng.integers(0, 1 << 32))][i % 7]
        else:
            lb = int(rng.integers(33, 255))
            b = int.from_bytes(rng.bytes(32), "little") % (1 << lb) | (1 << (lb - 1))
            k = int(rng.integers(0, 1 << 31))
            a = [b * k, b * k + b - 1, b * k + 1,
                 int.from_bytes(rng.bytes(32), "little") % (1 << min(255, lb + 30))][i % 4] % (1 << 255)
        rows.append(_row(P.ground_set if ground else P.binop_set, (_DIV[name], w, a, b), _FN[name](a, b, w), w,
                         bit=int(rng.integers(0, w))))
    return rows


@kernels
@pytest.mark.parametrize("ground", [False, True], ids=["var", "ground"])
@pytest.mark.parametrize("family", ["one_limb", "one_digit"])
@pytest.mark.parametrize("name", sorted(_DIV))
def test_division_paths_through_search(engine, name, family, ground, base, flags):
    rows = _division_rows(name, family, ground)
    assert len(rows) == 256
    _run(engine, rows, base, flags)


@functools.lru_cache(maxsize=None)
def _width_rows(w):
    """64 operand pairs of every arithmetic op and compare at width w (the generator of
    test_every_op_at_laser_widths)."""
    rng = np.random.default_rng(0xB175 + w)
    rows = []
    for name in sorted(_FN) + sorted(_CFN):
        for _ in range(64):
            a, b = _rand_operand(rng, w), _rand_operand(rng, w)
            if name in ("shl", "lshr", "ashr") and rng.random() < 0.6:
                b = int(rng.integers(0, w + 2)) & ir.mask(w)
            if name in _FN:
                rows.append(_row(P.binop_set, (_OPS[name], w, a, b), _FN[name](a, b, w), w,
                                 bit=int(rng.integers(0, w))))
            else:
                rows.append(_row(P.cmp_set, (_CMPS[name], w, a, b), bool(_CFN[name](a, b, w)), 1))
    return rows


@kernels
@pytest.mark.parametrize("w", _WIDTHS + (173,))
def test_every_op_at_every_width_through_search(engine, w, base, flags):
    rows = _width_rows(w)
    assert len(rows) == 18 * 64
    _run(engine, rows, base, flags)


# ---- c. the vocabulary without a direct comparison -----------------------------------------

_VOCAB_WIDTHS = (1, 8, 33, 160, 173, 256)


@functools.lru_cache(maxsize=None)
def _logic_rows(op):
    rng = np.random.default_rng(0x10C1C + op)
    rows = []
    for w in _VOCAB_WIDTHS:
        Mw = ir.mask(w)
        for _ in range(64):
            a, b, bit = _rand_operand(rng, w), _rand_operand(rng, w), int(rng.integers(0, w))
            if op in (ir.W_AND, ir.W_OR, ir.W_XOR):
                r = {ir.W_AND: a & b, ir.W_OR: a | b, ir.W_XOR: a ^ b}[op]
                rows.append(_row(P.binop_set, (op, w, a, b), r, w, bit))
            elif op == ir.W_MOV:
                rows.append(_row(P.unop_set, (op, w, a), a, w, bit))
                if w < 256:                       # narrowing: the source is wider than the move
                    wide = _rand_operand(rng, 256) | (1 << w)
                    rows.append(_row(P.unop_set, (op, w, wide), wide & Mw, w, bit, wa=256))
            else:
                r = O.bvnot(a, w) if op == ir.W_NOT else O.bvneg(a, w)
                rows.append(_row(P.unop_set, (op, w, a), r, w, bit))
    return rows


@kernels
@pytest.mark.parametrize("op", [ir.W_AND, ir.W_OR, ir.W_XOR, ir.W_NOT, ir.W_NEG, ir.W_MOV],
                         ids=lambda op: ir.OPNAMES[op])
def test_logic_and_moves(engine, op, base, flags):
    rows = _logic_rows(op)
    assert len(rows) == (64 * 11 if op == ir.W_MOV else 64 * 6)
    _run_both(engine, rows, base, flags)


_EXTRACTS = ((0, 1), (0, 8), (31, 2), (32, 32), (63, 130), (248, 8), (255, 1), (0, 256), (96, 160))
_CONCATS = ((1, 1), (8, 248), (128, 128), (255, 1), (1, 255), (96, 160), (3, 29))
_SEXTS = tuple((f, t) for f in (1, 8, 31, 32, 33, 255) for t in (32, 64, 256) if t > f)


@functools.lru_cache(maxsize=None)
def _structural_rows(kind):
    rng = np.random.default_rng(0x57C7 + len(kind))
    rows = []
    if kind == "extract":
        for lo, w in _EXTRACTS:
            for _ in range(64):
                a = _rand_operand(rng, 256)
                rows.append(_row(P.unop_set, (ir.W_EXTRACT, w, a), O.extract(a, lo, w), w,
                                 int(rng.integers(0, w)), wa=256, aux0=lo))
    elif kind == "concat":
        for wa, wb in _CONCATS:
            for _ in range(64):
                a, b = _rand_operand(rng, wa), _rand_operand(rng, wb)
                rows.append(_row(P.binop_set, (ir.W_CONCAT, wa + wb, a, b), O.concat(a, b, wb), wa + wb,
                                 int(rng.integers(0, wa + wb)), wa=wa, wb=wb, aux0=wb))
    elif kind == "sext":
        for f, t in _SEXTS:
            for i in range(64):
                a = _rand_operand(rng, f) & ir.mask(f - 1) if f > 1 else 0
                a |= (i & 1) << (f - 1)           # the sign bit set in every other tuple
                rows.append(_row(P.unop_set, (ir.W_SEXT, t, a), O.sign_extend(a, f, t), t,
                                 int(rng.integers(0, t)), wa=f, aux0=f))
    elif kind == "ite":
        for w in _VOCAB_WIDTHS:
            for i in range(64):
                a = _rand_operand(rng, w)
                b = a if i % 8 == 7 else _rand_operand(rng, w)
                sel = (i >> 1) & 1
                rows.append(_row(P.ite_set, (w, sel, a, b), a if sel else b, w, int(rng.integers(0, w))))
    elif kind == "hash":
        for w in (256, 160, 8):
            for salt in (0, 0x5A17, 0xFFFFFFFF):
                for _ in range(64):
                    a = _rand_operand(rng, 256)
                    rows.append(_row(P.unop_set, (ir.W_HASH, w, a), O.uf_hash(a, salt) & ir.mask(w), w,
                                     int(rng.integers(0, w)), wa=256, aux0=salt))
    return rows


@kernels
@pytest.mark.parametrize("kind", ["extract", "concat", "sext", "ite", "hash"])
def test_structural_ops(engine, kind, base, flags):
    rows = _structural_rows(kind)
    assert len(rows) == 64 * {"extract": len(_EXTRACTS), "concat": len(_CONCATS), "sext": 14, "ite": 6,
                              "hash": 9}[kind]
    _run_both(engine, rows, base, flags)


def _bool_rows():
    rows = []
    for v in (0, 1):
        rows.append(_row(P.bool_set, (ir.B_CONST, (v,)), bool(v), 1))
        rows.append(_row(P.bool_set, (ir.B_NOT, (v,)), not v, 1))
    for x in (0, 1):
        for y in (0, 1):
            rows.append(_row(P.bool_set, (ir.B_AND, (x, y)), bool(x & y), 1))
            rows.append(_row(P.bool_set, (ir.B_OR, (x, y)), bool(x | y), 1))
            rows.append(_row(P.bool_set, (ir.B_XOR, (x, y)), bool(x ^ y), 1))
            for c in (0, 1):
                rows.append(_row(P.bool_set, (ir.B_ITE, (x, y, c)), bool(x if c else y), 1))
    return rows


@kernels
def test_bool_ops(engine, base, flags):
    rows = _bool_rows()
    assert len(rows) == 4 + 12 + 8
    _run_both(engine, rows, base, flags)


@functools.lru_cache(maxsize=None)
def _eq_rows(w):
    rng = np.random.default_rng(0xE9 + w)
    rows = []
    for i in range(64):
        a = _rand_operand(rng, w)
        b = a if i % 2 == 0 else a ^ (1 << int(rng.integers(0, w)))
        rows.append(_row(P.cmp_set, (ir.B_EQ, w, a, b), a == b, 1))
    return rows


def _high_bits(rng):
    """width -> a value whose bits are all at or above it (bit ``width`` always set)."""
    def g(w):
        if w >= 256:
            return 0
        return ((int.from_bytes(rng.bytes(32), "little") | 1) << w) & ir.mask(256)
    return g


@kernels
@pytest.mark.parametrize("w", _WIDTHS)
def test_eq_remasks_its_sources(engine, w, base, flags):
    """B_EQ on values that agree below bit w: the parent rows as uploaded, and the explicit
    candidates, carry different bits above the variables' width, which the generator
    (maskw) and the SoA load's write-back must clear — the values as packed by ir.Batch are
    masked on the host, so the rows here are patched after packing."""
    rows = _eq_rows(w)
    progs = _build(rows, base)
    batch = ir.Batch(progs)
    g = _high_bits(np.random.default_rng(w))
    for s0, _, _, slot in batch.schema:
        vw = (int(s0) >> 8) & 0x3FF
        batch.parents[slot] |= np.array(ir.to_limbs(g(vw)), dtype=np.uint32)
    _search(engine, progs, flags, batch=batch)
    if flags == 0:
        _soa(engine, _build(rows, base, parents=False), garbage=g)


# ---- d. the register file and the LDS registers -----------------------------------------------

_A = 0xF123456789ABCDEF_0011223344556677_8899AABBCCDDEEFF_0F1E2D3C4B5A6979
_SLOT = {   # one fixed operand pair per op
    ir.W_ADD: (_A, 0x8FEDCBA987654321_1122334455667788_99AABBCCDDEEFF00_123456789ABCDEF1),
    ir.W_MUL: (_A, 0x8FEDCBA987654321_1122334455667788_99AABBCCDDEEFF00_123456789ABCDEF1),
    ir.W_EXP: (_A, 0x8FEDCBA987654321_1122334455667788_99AABBCCDDEEFF00_123456789ABCDEF1),
    ir.W_UDIV: (_A, 0x3_1122334455667788_99AABBCCDDEEFF00),
    ir.W_SDIV: (_A, 0x3_1122334455667788_99AABBCCDDEEFF00),
    ir.W_SHL: (_A, 77),
    ir.B_UMUL_NOOVF: (_A >> 130, 0x3_1122334455667788_99AABBCCDDEEFF00),
}
_SLOT_FN = {ir.W_ADD: O.bvadd, ir.W_MUL: O.bvmul, ir.W_EXP: O.bvexp, ir.W_UDIV: O.bvudiv,
            ir.W_SDIV: O.bvsdiv, ir.W_SHL: O.bvshl, ir.B_UMUL_NOOVF: O.umul_noovf}
_SLOT_SAMPLE = ((0, 5, 6), (5, 6, 0), (6, 0, 5), (6, 5, 6), (5, 0, 5), (0, 6, 3), (3, 5, 6), (6, 3, 0),
                (5, 6, 5), (0, 1, 2), (2, 6, 6), (5, 2, 1))     # offsets of registers 8, 13, 14 and others


def _slot_tuples(base):
    if base:
        return _SLOT_SAMPLE
    return [(ra, rb, rd) for ra in range(7) for rb in range(7) if ra != rb for rd in range(7)]


@kernels
@pytest.mark.parametrize("op", sorted(_SLOT), ids=lambda op: ir.OPNAMES[op])
def test_register_file_slots(engine, op, base, flags):
    """The op between full register files, every (ra, rb, rd) and both compare orders: the
    result reaches its register (or is forwarded) and no other register changes — registers
    5 and 6 of the narrow kernels live in LDS, next to EXP's window table."""
    a, b = _SLOT[op]
    expect = _SLOT_FN[op](a, b, 256)
    is_cmp = op in ir.B_CMP
    if is_cmp:
        expect = bool(expect)
        assert expect                      # no overflow: the division behind it runs in full
    else:
        assert expect not in (a, b) + P.GUARDS and len({a, b} | set(P.GUARDS)) == 9
    wrong = (not expect) if is_cmp else P.corrupt(expect, 256, 131)
    tuples = _slot_tuples(base)
    assert len(tuples) == (len(_SLOT_SAMPLE) if base else 294)
    progs, keys = [], []
    for ra, rb, rd in tuples:
        for order in ("guards_first", "result_first"):
            progs.append(P.slot_set(op, ra, rb, rd, order, a, b, expect, base=base, verdict=True))
            progs.append(P.slot_set(op, ra, rb, rd, order, a, b, wrong, base=base, verdict=False))
            keys += [(ra, rb, rd, order)] * 2
    found = engine.check(engine.upload(progs), budget=1, seed=SEED, flags=flags).found
    want = np.array([0 if p.verdict else NOT_FOUND for p in progs], dtype=np.uint32)
    bad = np.nonzero(found != want)[0]
    if bad.size == 0:
        return
    report = []
    for i in bad[:6]:
        ra, rb, rd, order = keys[i]
        if not progs[i].verdict:
            report.append((ir.OPNAMES[op], ra, rb, rd, order, "a corrupted result expectation was accepted"))
            continue
        names = P.slot_checks(op, ra, rb, rd)
        singles = [P.slot_set(op, ra, rb, rd, order, a, b, expect, base=base, only=nm) for nm in names]
        f1 = engine.check(engine.upload(singles), budget=1, seed=SEED, flags=flags).found
        wrong_at = [nm for nm, f in zip(names, f1) if f != 0]
        report.append((ir.OPNAMES[op], ra, rb, rd, order, wrong_at or "only the whole set fails"))
    raise AssertionError((len(bad), report))


# ---- e. all 64 lanes, generated values ------------------------------------------------------

@kernels
@pytest.mark.parametrize("w", [256, 64])
def test_identities_over_generated_candidates(engine, w, base, flags):
    """Sets asserting the violation of an identity between ops, over 4,096 generated
    candidates (every lane of every group active, values on the edges by the pool): no
    witness, as the C oracle says; the false variants return the oracle's first witness."""
    budget, gseed = 4096, 0x1DE7_717E
    progs = [P.identity_set(name, w, base, fv) for name in P.IDENTITIES for fv in (False, True)]
    packed = coracle_py.Packed(ir.Batch(progs))
    want = [packed.first_sat(s, gseed, budget) for s in range(len(progs))]
    assert all((x is None) == p.name.endswith("/true") for x, p in zip(want, progs))
    res = engine.check(engine.upload(progs), budget=budget, seed=gseed, flags=flags)
    got = [None if f == NOT_FOUND else int(f) for f in res.found]
    assert got == want, [(p.name, g, x) for p, g, x in zip(progs, got, want) if g != x]


# ---- f. the generator, every kind -----------------------------------------------------------

_GEN_CANDS = list(range(512)) + [65535, 65536, 1 << 31, (1 << 32) - 1]


@pytest.mark.parametrize("gseed", [7, 0xDEADBEEF_00C0FFEE], ids=hex)
@pytest.mark.parametrize("layout", P.GEN_LAYOUTS)
def test_materialize_every_kind(engine, layout, gseed):
    p = P.generator_set(layout, seed=0x51ED)
    batch = ir.Batch([p])
    db = engine.upload(batch)
    got = engine.materialize(db, [0] * len(_GEN_CANDS), _GEN_CANDS, seed=gseed)
    want = O.SetView.from_batch(batch, 0).gen_assignments(np.array(_GEN_CANDS, dtype=np.uint64), gseed)
    bad = [(c, v) for k, c in enumerate(_GEN_CANDS) for v in range(len(p.vars)) if got[k][v] != want[k][v]]
    assert not bad, (len(bad), [(c, v, p.vars[v].kind, p.vars[v].width, hex(p.vars[v].hint0), p.vars[v].hint1,
                                 hex(got[_GEN_CANDS.index(c)][v]), hex(want[_GEN_CANDS.index(c)][v]))
                                for c, v in bad[:6]])


@kernels
def test_inlined_generator_at_chosen_candidates(engine, base, flags):
    """gen_var as compiled into the search kernels: a set asserts that a high-entropy variable
    equals the oracle's value of it at candidate k; the first witness is the oracle's."""
    budget, gseed = 4096, 0xDEADBEEF_00C0FFEE
    progs, ks = [], []
    for v in range(len(P.PIN_VARS)):
        for k in P.PIN_CANDS:
            progs.append(P.pin_set_at(v, k, gseed, base=base, seed=0x9E37 + v))
            ks.append(k)
    packed = coracle_py.Packed(ir.Batch(progs))
    want = [packed.first_sat(s, gseed, budget) for s in range(len(progs))]
    assert all(x is not None and x <= k for x, k in zip(want, ks))
    res = engine.check(engine.upload(progs), budget=budget, seed=gseed, flags=flags)
    got = [None if f == NOT_FOUND else int(f) for f in res.found]
    assert got == want, [(p.name, k, g, x) for p, k, g, x in zip(progs, ks, got, want) if g != x]
