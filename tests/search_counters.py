"""What a search must report, stated from the oracle (no GPU here; DESIGN.md §5, "The
counter contract").

``pf_stats`` after ``pf_check_batch`` carries three counters that bench.py, tools/full_pass.py
and gpu_check.STATS sum: ``cands_decided`` (active lanes of every evaluated 64-candidate
group), ``evals_full`` (the active lanes of the groups that ran their program to END) and
``ops`` (aux1 of every executed instruction times the group's active lanes, with
PF_FLAG_COUNT_OPS).  Given the oracle's SAT mask of every set over ``[0, budget)`` they are
exact for the full sweep and bounded for the early-exit search; the functions below are those
formulas.  A *group* is candidates ``64g .. min(64g + 63, budget - 1)``.

``device_trace`` is test_device_program.eval_device extended to say where a candidate's root
fell, which the PF_FLAG_SHORTCIRCUIT ``ops`` figure needs: a wave leaves the program at the
assert where its last active lane's root falls."""

import coracle_py
import numpy as np
import pyoracle as O
from test_device_program import I_ASSERT, I_FA, I_FB, I_KA, I_KB, TR_WW, _step, device_program

NOT_FOUND = 0xFFFFFFFF


def sat_masks(batch, seed, n_cand):
    """[set][candidate] bool over candidates 0 .. n_cand - 1, from the C restatement."""
    P = coracle_py.Packed(batch)
    return np.stack([P.eval_generated(s, seed, 0, n_cand) for s in range(len(batch))])


def first_witness(mask, budget):
    """The smallest witness of one set below ``budget``, or None."""
    idx = np.flatnonzero(mask[:budget])
    return int(idx[0]) if idx.size else None


def found(masks, budget):
    """found[] as the C ABI reports it."""
    out = np.full(len(masks), NOT_FOUND, dtype=np.uint32)
    for s, m in enumerate(masks):
        f = first_witness(m, budget)
        if f is not None:
            out[s] = f
    return out


def group_sizes(budget):
    full, rest = divmod(budget, 64)
    return [64] * full + ([rest] if rest else [])


def aux1_totals(batch):
    """A_s: the sum of aux1 over each set's instructions (code and descs as packed; the device
    program of pf_device_program keeps it, tests/test_search_counters.py)."""
    code = np.asarray(batch.code, dtype=np.uint64).reshape(-1, 4)
    return [int(code[int(d[0]):int(d[0]) + int(d[1]), 3].sum()) for d in batch.descs]


def full_sweep(masks, budget, aux1=None):
    """(cands_decided, evals_full, ops) without EARLY_EXIT and without SHORTCIRCUIT; ``aux1``
    (the A_s) with PF_FLAG_COUNT_OPS, else ops is 0."""
    n = len(masks) * budget
    return n, n, (budget * sum(aux1) if aux1 is not None else 0)


def shortcircuit_evals_full(masks, budget):
    """Full sweep with SHORTCIRCUIT: a group runs to END exactly when one of its lanes holds
    (roots only fall, and the wave leaves only where every active lane's root is false)."""
    total = 0
    for m in masks:
        for g, size in enumerate(group_sizes(budget)):
            if m[64 * g:64 * g + size].any():
                total += size
    return total


def early_exit_floor(masks, budget):
    """L: what an early-exit search evaluates at the least.  The chunks below the witness's
    run whole, the witness's chunk up to the witness's group; a set without a witness runs
    its whole budget."""
    total = 0
    for m in masks:
        f = first_witness(m, budget)
        total += budget if f is None else min(budget, 64 * (f // 64 + 1))
    return total


def device_trace(sv, code_rows, values):
    """(root, index of the device instruction at which the root first became false or None):
    eval_device's reading of the device flags, one instruction at a time."""
    W, B, S = {}, {}, {}
    root, fell, last = True, None, None
    for i, (w0, w1, aux0, aux1) in enumerate(code_rows):
        op = w0 & 0xFF
        if op == O.OP["END"]:
            break
        if w0 & I_KA:
            W[0xFE] = sv.consts[(w1 >> 8) & 0xFF]
            w1 = (w1 & ~0xFF00) | (0xFE << 8)
        if w0 & I_KB:
            W[0xFD] = sv.consts[(w1 >> 16) & 0xFF]
            w1 = (w1 & ~0xFF0000) | (0xFD << 16)
        if w0 & I_FA:
            W[0xFC] = last
            w1 = (w1 & ~0xFF00) | (0xFC << 8)
        if w0 & I_FB:
            W[0xFB] = last
            w1 = (w1 & ~0xFF0000) | (0xFB << 16)
        w_result = op < O.OP["B_CONST"] and op != O.OP["W_SPILL"]
        d = w1 & 0xFF
        old = W.get(d)
        root = _step((w0 & ~(I_ASSERT | I_KA | I_KB | I_FA | I_FB), w1, aux0, aux1), sv.consts, W, B, S, values,
                     root)
        if w_result:
            last = W[d]
            if not (w0 & TR_WW):
                if old is None:
                    del W[d]
                else:
                    W[d] = old
        if w0 & I_ASSERT:
            root = root and B[w1 & 0xFF]
        if not root and fell is None:
            fell = i
    return bool(root), fell


def device_rows(batch):
    """Per set, the device program's instructions as tuples of ints."""
    code, descs = device_program(batch)
    return [[tuple(int(x) for x in r) for r in code[int(d[0]):int(d[0]) + int(d[1])]] for d in descs]


def traces(batch, seed, budget):
    """Per set, device_trace of every candidate below ``budget``."""
    out = []
    for s, rows in enumerate(device_rows(batch)):
        sv = O.SetView.from_batch(batch, s)
        vals = sv.gen_assignments(np.arange(budget, dtype=np.uint64), seed)
        out.append([device_trace(sv, rows, v) for v in vals])
    return out


def shortcircuit_ops(batch, seed, budget):
    """ops of a full sweep with SHORTCIRCUIT | COUNT_OPS: per group its size times the aux1 of
    the device instructions it executes — all of them if a lane holds, else those up to and
    including the assert at which the last lane's root fell."""
    total = 0
    for rows, tr in zip(device_rows(batch), traces(batch, seed, budget)):
        prefix = np.cumsum([r[3] for r in rows], dtype=np.uint64)
        for g, size in enumerate(group_sizes(budget)):
            lanes = tr[64 * g:64 * g + size]
            if any(root for root, _ in lanes):
                total += size * int(prefix[-1])
            else:
                total += size * int(prefix[max(fell for _, fell in lanes)])
    return total
