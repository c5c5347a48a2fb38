"""CPU: the hand-emitted programs of op_programs.py are what test_gpu_narrow_ops.py takes them
for — valid, on the intended side of the 8 / 16-register split, with the oracle's verdict equal
to the builder's stated one, and with the device form (pf_batch_create's peepholes) the GPU
tests rely on: constant operands folded, forwarding taken or not by the compare order."""

import coracle_py
import numpy as np
import op_programs as P
import pyoracle as O
import pytest
from test_device_program import I_FA, I_FB, I_KA, I_KB, TR_WW, device_program, eval_device

from mythril_amd import ir

A, B_ = 0xF123456789ABCDEF_0011223344556677_8899AABBCCDDEEFF_0F1E2D3C4B5A6978, \
    0x00000000000000000000000000000003_00000000000000000000000000010001


def _samples(base):
    """One or two sets of every builder: (program, kind)."""
    out = []
    for v in (True, False):
        c = 0 if v else 1          # a wrong expectation: the stated verdict is then False
        out += [
            P.binop_set(ir.W_ADD, 256, A, B_, O.bvadd(A, B_, 256) ^ c, base=base, verdict=v),
            P.binop_set(ir.W_SDIV, 173, A, B_, O.bvsdiv(A & ir.mask(173), B_, 173) ^ c, regs=(6, 5, 6),
                        base=base, verdict=v),
            P.binop_set(ir.W_CONCAT, 256, 0x5, B_, O.concat(0x5, B_, 253) ^ c, wa=3, wb=253, aux0=253,
                        base=base, verdict=v),
            P.unop_set(ir.W_SEXT, 64, 0x80, 0xFFFFFFFFFFFFFF80 ^ c, wa=8, aux0=8, base=base, verdict=v),
            P.unop_set(ir.W_EXTRACT, 130, A, O.extract(A, 63, 130) ^ c, wa=256, aux0=63, base=base, verdict=v),
            P.unop_set(ir.W_HASH, 160, A, (O.uf_hash(A, 9) & ir.mask(160)) ^ c, wa=256, aux0=9, base=base,
                       verdict=v),
            P.ite_set(33, 1, 7, 9, 7 ^ c, base=base, verdict=v),
            P.cmp_set(ir.B_SLT, 173, 1 << 172, 5, v, base=base, verdict=v),
            P.cmp_set(ir.B_UMUL_NOOVF, 256, A, B_, v, base=base, verdict=not v),
            P.bool_set(ir.B_ITE, (1, 0, 0), not v, base=base, verdict=v),
            P.bool_set(ir.B_CONST, (1,), v, base=base, verdict=v),
            P.ground_set(ir.W_UDIV, 256, A, 3, (A // 3) ^ c, base=base, verdict=v),
            P.ground_set(ir.B_ULE, 64, 3, 3, v, base=base, verdict=v),
        ]
        for order in ("guards_first", "result_first"):
            out.append(P.slot_set(ir.W_MUL, 5, 2, 6, order, A, B_, O.bvmul(A, B_, 256) ^ c, base=base, verdict=v))
            out.append(P.slot_set(ir.W_EXP, 0, 6, 0, order, A, B_, O.bvexp(A, B_, 256) ^ c, base=base, verdict=v))
            out.append(P.slot_set(ir.B_UMUL_NOOVF, 3, 4, 5, order, A, B_, not v, base=base, verdict=v))
    return out


def _max_wdst(p):
    return max(i.dst for i in p.code if i.op < ir.B_CONST and i.op not in (ir.END, ir.W_SPILL))


@pytest.mark.parametrize("base", [0, 8])
def test_builders_state_the_oracles_verdict(base):
    progs = _samples(base)
    batch = ir.Batch(progs)
    for s, p in enumerate(progs):
        p.validate()
        if base:
            assert ir.NW_NARROW <= _max_wdst(p) < ir.NW, p.name
        else:
            assert _max_wdst(p) < ir.NW_NARROW, p.name
        sv = O.SetView.from_batch(batch, s)
        assert all(par is not None for par in sv.parents), p.name
        assert sv.evaluate(sv.parents) == p.verdict, p.name
        assert sv.evaluate(p.assignment) == p.verdict, p.name
        first, _ = sv.check(1, 0xC0FFEE)
        assert first == (0 if p.verdict else None), p.name


def test_parentless_sets_carry_their_assignment():
    p = P.binop_set(ir.W_XOR, 160, A, B_, (A ^ B_) & ir.mask(160), parents=False)
    assert not p.has_parent and p.assignment == [A & ir.mask(160), B_]
    assert O.SetView.from_batch(ir.Batch([p]), 0).evaluate(p.assignment)


def _rows(p):
    code, descs = device_program(ir.Batch([p]))
    return code[descs[0][0]:descs[0][0] + descs[0][1]]


def _row_of(rows, op):
    return int(rows[[int(x) & 0xFF for x in rows[:, 0]].index(op), 0])


@pytest.mark.parametrize("base", [0, 8])
def test_device_form_of_ground_and_slot_sets(base):
    for op in (ir.W_UDIV, ir.W_EXP, ir.B_UMUL_NOOVF):
        rows = _rows(P.ground_set(op, 256, A, 3, 0, base=base, verdict=None))
        w0 = _row_of(rows, op)
        assert w0 & I_KA and w0 & I_KB and not w0 & (I_FA | I_FB), ir.OPNAMES[op]
    for op in (ir.W_ADD, ir.W_EXP, ir.W_UDIV):
        for ra, rb, rd in ((0, 1, 2), (5, 6, 5), (6, 0, 6), (3, 5, 6)):
            rows = _rows(P.slot_set(op, ra, rb, rd, "guards_first", A, B_, 0, base=base, verdict=None))
            w0 = _row_of(rows, op)
            assert w0 & TR_WW and not w0 & (I_FA | I_FB | I_KA | I_KB), (ir.OPNAMES[op], ra, rb, rd)
            ops = [int(x) & 0xFF for x in rows[:, 0]]
            last_eq = int(rows[len(ops) - 1 - ops[::-1].index(ir.B_EQ), 0])
            assert last_eq & I_KB and not last_eq & I_FA            # the result, from its register
            rows = _rows(P.slot_set(op, ra, rb, rd, "result_first", A, B_, 0, base=base, verdict=None))
            ops = [int(x) & 0xFF for x in rows[:, 0]]
            k = ops.index(op)
            assert ops[k + 1] == ir.B_EQ and int(rows[k + 1, 0]) & I_FA and int(rows[k + 1, 0]) & I_KB
            assert not int(rows[k, 0]) & TR_WW                      # forwarded only: never written


def test_device_form_computes_the_stated_verdict():
    progs = _samples(0) + _samples(8)
    batch = ir.Batch(progs)
    code, descs = device_program(batch)
    for s, p in enumerate(progs):
        sv = O.SetView.from_batch(batch, s)
        d = descs[s]
        rows = [tuple(int(x) for x in r) for r in code[d[0]:d[0] + d[1]]]
        assert eval_device(sv, rows, sv.parents) == p.verdict, p.name


def test_single_compare_slot_sets_partition_the_full_one():
    for op, rd in ((ir.W_SHL, 4), (ir.B_UMUL_NOOVF, 0)):
        names = P.slot_checks(op, 2, 4, rd)
        assert names[-1] == "result" and len(names) == (6 if op == ir.W_SHL else 7)
        full = P.slot_set(op, 2, 4, rd, "guards_first", A, 9, 0)
        n_full = sum(i.op == ir.ASSERT for i in full.code)
        assert n_full == len(names)
        for nm in names:
            one = P.slot_set(op, 2, 4, rd, "guards_first", A, 9, 0, only=nm)
            assert sum(i.op == ir.ASSERT for i in one.code) == 1


@pytest.mark.parametrize("w", [256, 64])
def test_identities_have_no_witness_and_their_false_variants_one(w):
    budget, gseed = 4096, 0x1DE7_717E
    progs = []
    for name in P.IDENTITIES:
        for base in (0, 8):
            progs.append(P.identity_set(name, w, base, False))
            progs.append(P.identity_set(name, w, base, True))
    for p in progs:
        assert [c & ir.mask(256) for c in P.edge_pool(w)] == p.consts[:6], p.name
        assert all(v.parent is None for v in p.vars)
    packed = coracle_py.Packed(ir.Batch(progs))
    for s, p in enumerate(progs):
        first = packed.first_sat(s, gseed, budget)
        if p.name.endswith("/true"):
            assert first is None, (p.name, first)
        else:
            assert first is not None, p.name
    # the C restatement and the Python one agree on the first groups of every set
    b = ir.Batch(progs)
    for s in range(0, len(progs), 5):
        want = O.SetView.from_batch(b, s).check(64, gseed)[1]
        assert list(packed.eval_generated(s, gseed, 0, 64)) == want


def test_generator_sets_stay_inside_the_schema_checks():
    for layout in P.GEN_LAYOUTS:
        p = P.generator_set(layout)
        n = len(p.consts)
        assert n == (0 if layout == "bare" else 8)
        kinds = {v.kind for v in p.vars}
        assert (ir.VK_KECCAK in kinds) == (n > 0)
        for v in p.vars:
            if v.kind == ir.VK_KECCAK:
                assert v.hint0 < n
            if v.kind == ir.VK_ACTOR:
                assert v.hint1 <= 4 and v.hint0 + v.hint1 <= n
            if v.kind == ir.VK_CDBYTE:
                assert v.hint0 & 0xFF <= 248 and not v.hint0 & 7
                assert (v.hint0 >> 20) + ((v.hint0 >> 8) & 0xFFF) <= n
        par = [v.parent is not None for v in p.vars]
        assert {"bare": not any(par), "consts": not any(par), "parented": all(par),
                "alternate": par == [k % 2 == 0 for k in range(len(par))]}[layout]
        # every candidate holds (the code compares variable 0 with itself)
        assert O.SetView.from_batch(ir.Batch([p]), 0).check(4, 1)[0] == 0


def test_pin_sets_first_witness_is_at_or_before_their_candidate():
    gseed = 0xDEAD_BEEF_00C0_FFEE
    progs, ks = [], []
    for v in range(len(P.PIN_VARS)):
        for k in P.PIN_CANDS:
            progs.append(P.pin_set_at(v, k, gseed))
            ks.append(k)
    b = ir.Batch(progs)
    packed = coracle_py.Packed(b)
    for s, (p, k) in enumerate(zip(progs, ks)):
        first = packed.first_sat(s, gseed, 4096)
        assert first is not None and first <= k, (p.name, k, first)
        sv = O.SetView.from_batch(b, s)
        vals = sv.gen_assignments(np.array([first, k], dtype=np.uint64), gseed)
        assert sv.evaluate(vals[0]) and sv.evaluate(vals[1])
