"""Test tooling (not a test; no GPU needed to import): the stream contract of
include/pf_bytecode.h in Python — what pf_eval_batch must return for explicit candidates.

``expected(batch, assignments, set_ids)`` evaluates every candidate of every requested set with
``pyoracle.SetView.evaluate`` and packs the verdicts the way the contract lays them out: ``bits``
(uint64 [n, ceil(n_cand / 64)], bit c & 63 of word c >> 6, the tail bits 0), ``first`` (the
smallest satisfying candidate or 0xFFFFFFFF) and ``count``, all in request order.
``assignments[s]`` is set s's candidate list (each a list of its variables' values), as
``ir.pack_soa`` takes it."""

import numpy as np
import pyoracle as O

from mythril_amd import ir

NONE = 0xFFFFFFFF


def pack_bits(verdicts) -> np.ndarray:
    """bool [n, n_cand] -> uint64 [n, ceil(n_cand / 64)], by the contract's own words: bit
    c & 63 of word c >> 6 is candidate c, the bits past n_cand are 0."""
    verdicts = [list(v) for v in verdicts]
    n_cand = len(verdicts[0]) if verdicts else 0
    words = (n_cand + 63) // 64
    out = np.zeros((len(verdicts), words), dtype=np.uint64)
    for i, row in enumerate(verdicts):
        assert len(row) == n_cand
        acc = [0] * words
        for c, v in enumerate(row):
            if v:
                acc[c >> 6] |= 1 << (c & 63)
        out[i] = np.array(acc, dtype=np.uint64)
    return out


def unpack_bits(bits, n_cand) -> np.ndarray:
    """uint64 [n, words] -> bool [n, n_cand], bit by bit (the inverse of pack_bits)."""
    bits = np.asarray(bits, dtype=np.uint64)
    out = np.zeros((len(bits), n_cand), dtype=bool)
    for i, row in enumerate(bits):
        for c in range(n_cand):
            out[i, c] = (int(row[c >> 6]) >> (c & 63)) & 1
    return out


def tail_is_zero(bits, n_cand) -> bool:
    """The bits past n_cand of every row's last word are 0."""
    bits = np.asarray(bits, dtype=np.uint64)
    if n_cand % 64 == 0 or bits.size == 0:
        return True
    return not any(int(row[-1]) >> (n_cand % 64) for row in bits)


def verdicts(batch: ir.Batch, assignments, set_ids=None):
    """bool rows [n][n_cand] of the requested sets, by the oracle."""
    ids = range(len(batch)) if set_ids is None else set_ids
    out = []
    for s in ids:
        sv = O.SetView.from_batch(batch, s)
        out.append([bool(sv.evaluate(a)) for a in assignments[s]])
    return out


def summarize(rows):
    """(bits, first, count) of verdict rows."""
    first = np.array([next((c for c, v in enumerate(r) if v), NONE) for r in rows], dtype=np.uint32)
    count = np.array([sum(map(bool, r)) for r in rows], dtype=np.uint32)
    return pack_bits(rows), first, count


def expected(batch: ir.Batch, assignments, set_ids=None):
    """(bits, first, count) the stream contract asks for, in request order."""
    return summarize(verdicts(batch, assignments, set_ids))


def max_w_written(prog) -> int:
    """The highest W register a program writes: >= ir.NW_NARROW runs the 16-register kernels."""
    code = ir.Batch([prog]).code.reshape(-1, 4)
    ops = code[:, 0] & 0xFF
    w_res = (ops < ir.B_CONST) & (ops != ir.END) & (ops != ir.W_SPILL)
    return int((code[w_res, 1] & 0xFF).max()) if w_res.any() else -1


def is_wide(prog) -> bool:
    return max_w_written(prog) >= ir.NW_NARROW
