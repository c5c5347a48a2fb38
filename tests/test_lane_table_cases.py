"""CPU: the lane-table harness of tests/lane_table_cases.py is checked before any GPU sees it.

For every catalogue entry (a mixed wave of div_trim_cases, products_cases, exp_chain_cases, the
exp_scale and exp_series mixed waves, a MUL and a UMUL_NOOVF wave — under the committed set seed):

* the 64 realised lanes T[k_j] have the property the wave is named for, by the case module's own
  assertion, with the special lane in exactly one lane, at its position;
* the 64 tags are distinct;
* every expectation equals Python's own integers (pow, //, %, z3's conventions for a zero
  divisor), next to the oracle's;
* by the C oracle, candidate j is the first and the only witness of set j among the 64, and the
  twin of set j (one bit of E_j flipped) has none — so the reference alone stays within "every
  lane is its set's only witness";
* the table's compares survive the device program's fold pass, and the batches assembled from
  arrays are what ir.Batch packs from the validated programs."""

import coracle_py
import div_trim_cases as D
import exp_chain_cases as XC
import lane_table_cases as L
import numpy as np
import products_cases as PC
import pytest

from mythril_amd import ir

ENTRIES = L.catalogue()
IDS = [e.id for e in ENTRIES]


def test_the_catalogue_is_complete():
    assert len(set(IDS)) == len(IDS) and set(L.SEEDS) == set(IDS)
    assert {e.family for e in ENTRIES} == set(L.FAMILIES)
    have = {(e.family, e.wave, e.pos, e.w) for e in ENTRIES}
    for op in ("udiv", "urem", "sdiv", "srem", "smod"):
        assert {(op, n, p, 256) for n in D.WAVES for p in D.POSITIONS} <= have
    assert {("exp_products", n, p, 256) for n in PC.WAVES for p in PC.POSITIONS} <= have
    assert {("exp_chain", n, None, w) for n in XC.WAVES for w in (256, 200)} <= have
    assert {(f, "mixed", None, w) for f in ("exp_scale", "exp_series") for w in (256, 200)} <= have
    assert ("mul", "carry_alternating", None, 256) in have
    assert {("umul_noovf", "lone_zero_operand", p, 256) for p in D.POSITIONS} <= have
    assert len(ENTRIES) == 5 * 32 + 48 + 10 + 4 + 1 + 4
    # the signed entries hand the divider magnitudes below 2^192 under all four sign patterns
    for e in L.family("sdiv") + L.family("srem") + L.family("smod"):
        assert all(a < 1 << 192 and b < 1 << 192 for a, b in e.model)
        signs = {(a >> 255, b >> 255) for (a, b), (x, y) in zip(e.table, e.model) if x and y}
        assert signs == {(0, 0), (0, 1), (1, 0), (1, 1)}
        for (a, b), (x, y) in zip(e.table, e.model):
            assert {a, (-a) & L.M256} >= {x} and {b, (-b) & L.M256} >= {y}
    sample = L.sample()
    assert len(sample) == 5 * 16 + 24 + 10 and {e.pos for e in sample} == {0, 63, None}


@pytest.mark.parametrize("entry", ENTRIES, ids=IDS)
def test_the_realised_wave_has_its_property(entry):
    ks, ts = entry.ks(), entry.tags()
    assert len(ks) == 64 and all(0 <= k < entry.K for k in ks)
    assert len(set(ts)) == 64 and all(0 < t < 1 << 124 for t in ts)
    if entry.pos is not None:
        assert [j for j, k in enumerate(ks) if k == 0] == [entry.pos]
        assert entry.pos in D.POSITIONS
    ok = entry.check(entry.seen(), entry.pos)      # the case module's assertion
    assert ok is None or ok, entry.id
    assert len(set(entry.realised())) >= 8         # a wave, not a few rows repeated
    assert entry.holds_property()


@pytest.mark.parametrize("entry", ENTRIES, ids=IDS)
def test_expectations_equal_pythons_integers(entry):
    oracle, python = entry.results(1), entry.results(2)
    assert [int(x) for x in oracle] == [int(x) for x in python], entry.id
    w = entry.w
    for (a, b), r in zip(entry.realised(), python):
        assert a < 1 << w and b < 1 << w
        if entry.opname == "exp":
            assert r == pow(a, b, 1 << w)
        elif entry.opname == "udiv":
            assert r == (a // b if b else (1 << w) - 1)
        elif entry.opname == "urem":
            assert r == (a % b if b else a)
    Es = entry.expectations()
    assert len(set(Es)) == 64
    assert all(0 <= entry.twin_bit(j) < 256 for j in range(64))


def _check_family(entries, placement, base):
    batch = L.LaneBatch(entries, placement, base)
    assert len(batch) == 128 * len(entries)
    packed = coracle_py.Packed(batch)
    bad = []
    for s in range(len(batch)):
        sat = packed.eval_generated(s, L.G, 0, 64)
        e, j, twin = batch.index[s]
        want = [] if twin else [j]
        if np.flatnonzero(sat).tolist() != want:
            bad.append((batch.describe(s), np.flatnonzero(sat).tolist()))
    assert not bad, (len(bad), bad[:4])
    first = [packed.first_sat(s, L.G, 64) for s in range(0, len(batch), 37)]
    assert first == [None if x == L.NOT_FOUND else int(x) for x in batch.want[::37]]
    return batch


@pytest.mark.parametrize("family", L.FAMILIES)
def test_every_lane_is_its_sets_only_witness(family):
    """coracle: first_sat == j for set j and None for its twin — and no second witness."""
    _check_family(L.family(family), "lds", 0)


@pytest.mark.parametrize("base", [0, 8])
@pytest.mark.parametrize("placement", sorted(L.PLACEMENTS))
def test_every_placement_and_base(placement, base):
    """The first and the last entry of every family under every register placement."""
    entries = [e for f in L.FAMILIES for e in (L.family(f)[0], L.family(f)[-1])]
    batch = _check_family(entries, placement, base)
    regs = set()
    for w0, w1 in batch.code[:int(batch.descs[0][1]), :2].tolist():
        if (w0 & 0xFF) in (ir.W_CONST, ir.W_VAR, ir.W_ITE, ir.W_XOR, ir.W_NOT) or (w0 & 0xFF) in ir.W_BINARY:
            regs.add(w1 & 0xFF)
    assert regs and all(base <= r <= base + 6 for r in regs), regs
    if placement != "low":
        assert {base + 5, base + 6} <= regs


@pytest.mark.parametrize("placement", sorted(L.PLACEMENTS))
def test_assembled_batches_are_what_ir_batch_packs(placement):
    for e in (L.family("udiv")[5], L.family("exp_chain")[7], L.family("umul_noovf")[1]):
        for base in (0, 8):
            lb = L.LaneBatch([e], placement, base)
            Es = e.expectations()
            progs = []
            for j in (0, 63):
                progs += [L.program(e, placement, base, Es[j]),
                          L.program(e, placement, base, Es[j] ^ 1 << e.twin_bit(j))]
            b = ir.Batch(progs)
            n, c = len(progs[0].words), len(progs[0].consts)
            pick = [0, 1, 126, 127]
            assert np.array_equal(b.code, np.concatenate([lb.code[s * n:(s + 1) * n] for s in pick]))
            assert np.array_equal(b.consts, np.concatenate([lb.consts[s * c:(s + 1) * c] for s in pick]))
            assert np.array_equal(b.schema, lb.schema[:8]) and b.parents.size == 0 == lb.parents.size
            assert np.array_equal(b.descs[:, [1, 3, 5, 6, 7]], lb.descs[pick][:, [1, 3, 5, 6, 7]])
            assert lb.descs[:, 0].tolist() == [s * n for s in range(128)]
            assert lb.descs[:, 2].tolist() == [s * c for s in range(128)]
            assert lb.descs[:, 4].tolist() == [2 * s for s in range(128)]


@pytest.mark.parametrize("base", [0, 8])
def test_the_tables_compares_survive_the_fold(base):
    """k's range [0, K - 1] covers every index, so the device program's range rules decide none
    of the K - 1 compares (a decided one would take its row out of the wave)."""
    for placement in sorted(L.PLACEMENTS):
        entries = [L.family(f)[0] for f in L.FAMILIES]
        batch = L.LaneBatch(entries, placement, base)
        for i, e in enumerate(entries):
            for s in (128 * i, 128 * i + 127):
                assert L.surviving_compares(batch, s) == e.K - 1, (e.id, placement, s)
