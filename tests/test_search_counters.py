"""CPU: the counter formulas of search_counters.py (what tests/test_gpu_search_schedule.py
holds the search kernels to) against direct counts over pyoracle's SetView.check, the aux1
total the device program must keep, and the device trace against SetView.evaluate."""

import numpy as np
import pyoracle as O
import search_counters as SC

from mythril_amd import ir, synth

SEED = 0x5EED_0F_5CA1E


def _sets(n):
    return [synth.random_dag_set(20_000 + 7 * i, plant=False)[0] for i in range(n)]


def test_formulas_match_a_direct_count():
    """Six sets at budget 150 (groups of 64, 64 and 22): first witness, cands_decided,
    evals_full with and without SHORTCIRCUIT and the early-exit floor, counted candidate by
    candidate from pyoracle's masks."""
    budget = 150
    batch = ir.Batch(_sets(6))
    masks = SC.sat_masks(batch, SEED, budget)
    assert SC.group_sizes(budget) == [64, 64, 22] and SC.group_sizes(128) == [64, 64] and SC.group_sizes(0) == []
    decided = sc_full = floor = 0
    firsts = []
    for s in range(len(batch)):
        first, sat = O.SetView.from_batch(batch, s).check(budget, SEED)
        assert list(masks[s]) == sat, s                      # the C restatement agrees
        firsts.append(first)
        assert SC.first_witness(masks[s], budget) == first
        stop = budget if first is None else first
        for c in range(budget):
            decided += 1
            lo = c - c % 64
            if any(sat[lo:min(lo + 64, budget)]):
                sc_full += 1
            if lo <= stop:
                floor += 1
    assert None in firsts and 0 in firsts and any(f for f in firsts)    # every kind of set
    want = np.array([SC.NOT_FOUND if f is None else f for f in firsts], dtype=np.uint32)
    assert np.array_equal(SC.found(masks, budget), want)
    aux1 = SC.aux1_totals(batch)
    assert SC.full_sweep(masks, budget) == (decided, decided, 0)
    assert SC.full_sweep(masks, budget, aux1) == (decided, decided, budget * sum(aux1))
    assert SC.shortcircuit_evals_full(masks, budget) == sc_full
    assert SC.early_exit_floor(masks, budget) == floor
    assert floor <= decided and sc_full <= decided
    # a budget below a witness hides it; one above shows it
    for s, f in enumerate(firsts):
        if f:
            assert SC.first_witness(masks[s], f) is None and SC.first_witness(masks[s], f + 1) == f


def test_device_program_keeps_every_sets_aux1_total():
    """pf_device_program deletes instructions (folded ASSERTs, W_MOVs, W_CONSTs) but no cost:
    ops == budget * sum(aux1) holds for the program as packed and as run."""
    progs = _sets(96) + [synth.mythril_like_set(i) for i in range(24)]
    batch = ir.Batch(progs)
    code, descs = SC.device_program(batch)
    assert len(code) < len(batch.code)                       # the peepholes did delete
    dev = [int(code[int(d[0]):int(d[0]) + int(d[1]), 3].astype(np.uint64).sum()) for d in descs]
    assert dev == SC.aux1_totals(batch)
    assert all(a > 0 for a in dev)


def test_device_trace_root_matches_the_oracle():
    """The trace's root equals SetView.evaluate for every candidate, and the instruction it
    names for a false root is an assert (the only place a root can fall)."""
    budget = 150
    batch = ir.Batch(_sets(6))
    rows = SC.device_rows(batch)
    n_false = 0
    for s, tr in enumerate(SC.traces(batch, SEED, budget)):
        sv = O.SetView.from_batch(batch, s)
        vals = sv.gen_assignments(np.arange(budget, dtype=np.uint64), SEED)
        for c, (root, fell) in enumerate(tr):
            assert root == bool(sv.evaluate(vals[c])), (s, c)
            assert (fell is None) == root
            if fell is not None:
                n_false += 1
                w0 = rows[s][fell][0]
                assert (w0 & 0xFF) == ir.ASSERT or (w0 & SC.I_ASSERT), (s, c, fell)
    assert n_false > 0
