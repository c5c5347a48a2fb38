"""Test tooling (not a test): the CPU model of the climb's tree score (include/pf_bytecode.h,
PF_CLIMB_SCORE_TREE).

* ``tree_run`` — a Python interpreter of the header's table on a set's *device program*
  (``climb_model.DeviceSet``): every B value carries (dt, df) beside its bit, a site adds
  CLIMB_HOLDS where it holds, else CLIMB_NEAR - dt.
* ``climb_set`` / ``climb`` — the round loop of the climb contract with a choice of score.  It is
  a loop of its own: ``climb_model.climb_set(score_fn=...)`` never stops at a witness.  With
  ``score="sites"`` it is ``climb_model.climb`` (tests/test_climb_tree_model.py checks that).
* ``TreeOracleEngine`` — the tests' oracle-backed engine whose ``climb`` honours ``score``.

The GPU tests compare pf_climb_batch_scored with this bit for bit.  Never imported by
mythril_amd/."""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

import climb_model as CM
import pyoracle as O
from mythril_amd import ir
from mythril_amd.engine import ClimbResult

NEAR, HOLDS = ir.CLIMB_NEAR, ir.CLIMB_HOLDS
I_ASSERT, I_KA, I_KB, I_FA, I_FB, TR_WW = CM.I_ASSERT, CM.I_KA, CM.I_KB, CM.I_FA, CM.I_FB, CM.TR_WW
_UNSIGNED = (O.OP["B_ULT"], O.OP["B_ULE"])
_SIGNED = (O.OP["B_SLT"], O.OP["B_SLE"])
_NOOVF = (O.OP["B_UADD_NOOVF"], O.OP["B_UMUL_NOOVF"])
TOP = 1 << 255


def sat(x: int) -> int:
    return min(x, NEAR)


def leaf(bit: bool, m: int):
    """A value m away from flipping: (0, m) where it holds, (m, 0) where it fails."""
    return (0, m) if bit else (m, 0)


def ordered(a: int, w: int) -> int:
    """What the kernel compares for SLT / SLE: a sign-extended from w bits to 256, top bit
    flipped — unsigned order of the results is signed order of the operands."""
    return O.sign_extend(a, w, 256) ^ TOP


def compare_pair(op: int, a: int, b: int, w: int, bit: bool):
    if op == O.OP["B_EQ"]:
        return (0, 1) if bit else (bin(a ^ b).count("1"), 0)
    if op in _UNSIGNED:
        return leaf(bit, max(1, abs(a - b).bit_length()))
    if op in _SIGNED:
        return leaf(bit, max(1, abs(ordered(a, w) - ordered(b, w)).bit_length()))
    if op in _NOOVF:
        return leaf(bit, NEAR)
    raise ValueError(f"tree model: compare {op}")


def p_not(x):
    return (x[1], x[0])


def p_and(x, y):
    return (sat(x[0] + y[0]), min(x[1], y[1]))


def p_or(x, y):
    return (min(x[0], y[0]), sat(x[1] + y[1]))


def p_xor(x, y):
    return (min(sat(x[0] + y[1]), sat(x[1] + y[0])), min(sat(x[0] + y[0]), sat(x[1] + y[1])))


def p_ite(c, x, y):
    return (min(sat(c[0] + x[0]), sat(c[1] + y[0])), min(sat(c[0] + x[1]), sat(c[1] + y[1])))


def site_term(pair) -> int:
    return HOLDS if pair[0] == 0 else NEAR - pair[0]


def tree_run(dev: CM.DeviceSet, values: Sequence[int], trace: Optional[list] = None,
             sites: Optional[list] = None):
    """(root, score) of one assignment under the tree score.  ``trace`` collects
    (instruction index, B register, bit, (dt, df)) of every B write, ``sites`` (instruction
    index, holds) of every assert site."""
    W: List[Optional[int]] = [None] * 256
    B: List[Optional[tuple]] = [None] * 32            # (dt, df); the bit is dt == 0
    S: Dict[int, object] = {}
    root, score, last = True, 0, None
    C = dev.consts
    OP = O.OP
    for pc, (cls, fn, w, d, ra, rb, rc, aux0, w0, op) in enumerate(dev._decoded()):
        a = C[ra] if w0 & I_KA else (last if w0 & I_FA else W[ra])
        b = C[rb] if w0 & I_KB else (last if w0 & I_FB else W[rb])
        m = (1 << w) - 1
        z = None
        pair = None
        if cls == 0:
            z = fn(a, b, w) & m
        elif cls == 1:
            pair = compare_pair(op, a, b, w, bool(fn(a, b, w)))
        elif op == OP["W_CONST"]:
            z = C[aux0] & m
        elif op == OP["W_VAR"]:
            z = int(values[aux0]) & m
        elif op == OP["W_MOV"]:
            z = a & m
        elif op == OP["W_EXTRACT"]:
            z = (a >> aux0) & m
        elif op == OP["W_CONCAT"]:
            z = ((a << aux0) | b) & m
        elif op == OP["W_NOT"]:
            z = O.bvnot(a, w)
        elif op == OP["W_NEG"]:
            z = O.bvneg(a, w)
        elif op == OP["W_SEXT"]:
            z = O.sign_extend(a, aux0, w)
        elif op == OP["W_ITE"]:
            z = (a if B[rc & 31][0] == 0 else b) & m
        elif op == OP["W_HASH"]:
            z = O.uf_hash(a, aux0) & m
        elif op == OP["W_SPILL"]:
            S[aux0] = a
        elif op == OP["W_FILL"]:
            z = S[aux0] & m
        elif op == OP["B_SPILL"]:
            S[aux0] = B[ra & 31]
        elif op == OP["B_FILL"]:
            pair = S[aux0]
        elif op == OP["B_CONST"]:
            pair = leaf(bool(aux0 & 1), NEAR)
        elif op == OP["B_VAR"]:
            pair = leaf(bool(int(values[aux0]) & 1), 1)
        elif op == OP["B_AND"]:
            pair = p_and(B[ra & 31], B[rb & 31])
        elif op == OP["B_OR"]:
            pair = p_or(B[ra & 31], B[rb & 31])
        elif op == OP["B_XOR"]:
            pair = p_xor(B[ra & 31], B[rb & 31])
        elif op == OP["B_NOT"]:
            pair = p_not(B[ra & 31])
        elif op == OP["B_ITE"]:
            pair = p_ite(B[rc & 31], B[ra & 31], B[rb & 31])
        elif op == OP["ASSERT"]:
            p = B[ra & 31]
            root = root and p[0] == 0
            score += site_term(p)
            if sites is not None:
                sites.append((pc, p[0] == 0))
        else:
            raise ValueError(f"tree model: unknown opcode {op}")
        if z is not None:
            last = z
            if w0 & TR_WW:
                W[d] = z
        elif pair is not None:
            assert 0 <= pair[0] <= NEAR and 0 <= pair[1] <= NEAR and (pair[0] == 0) != (pair[1] == 0), pair
            B[d & 31] = pair
            if trace is not None:
                trace.append((pc, d & 31, pair[0] == 0, pair))
            if w0 & I_ASSERT:
                root = root and pair[0] == 0
                score += site_term(pair)
                if sites is not None:
                    sites.append((pc, pair[0] == 0))
    return root, score & 0xFFFFFFFF


def tree_score(dev: CM.DeviceSet, values: Sequence[int]) -> int:
    return tree_run(dev, values)[1]


def score_fn(dev: CM.DeviceSet, score):
    sid = ir.climb_score_id(score)
    if sid == ir.CLIMB_SCORE_SITES:
        return dev.score
    if sid == ir.CLIMB_SCORE_TREE:
        return lambda values: tree_score(dev, values)
    raise ValueError(f"climb model: unknown score {score!r}")


def climb_set(sv: O.SetView, dev: CM.DeviceSet, rounds: int, per_round: int, seed: int,
              score="tree") -> CM.SetClimb:
    """The climb of one set under ``score``: climb_model.climb_set's rounds, adoption and ties,
    stopping at a witness."""
    score_of = score_fn(dev, score)
    target = dev.target
    own = list(sv.parents)
    memo: Dict[tuple, int] = {}
    cur, cur_round, cur_index, A = 0, 0, 0, None
    status, evals = ir.CLIMB_NONE, 0
    cands = np.arange(per_round, dtype=np.uint64)
    try:
        for r in range(rounds):
            sv.parents = own if r == 0 else list(A)
            assigns = sv.gen_assignments(cands, ir.climb_round_seed(seed, r))
            scores = []
            for a in assigns:
                k = tuple(a)
                if k not in memo:
                    memo[k] = score_of(a)
                scores.append(memo[k])
            evals += per_round
            best = CM.pick_best(scores, 1 if r else 0)
            if best is not None and scores[best] >= cur:
                cur, cur_round, cur_index, A = scores[best], r, best, [int(x) for x in assigns[best]]
            if cur == target:
                status = ir.CLIMB_WITNESS
                break
    finally:
        sv.parents = own
    return CM.SetClimb(status, cur, cur_round, A if A is not None else [], cur_index, evals)


def climb(batch: ir.Batch, set_ids: Sequence[int], rounds: int, per_round: int, seed: int = 0,
          score="tree", devs: Optional[List[CM.DeviceSet]] = None) -> List[CM.SetClimb]:
    """pf_climb_batch_scored on the CPU: one SetClimb per requested set, in request order."""
    devs = devs if devs is not None else CM.device_sets(batch)
    return [climb_set(O.SetView.from_batch(batch, int(s)), devs[int(s)], rounds, per_round, seed, score)
            for s in set_ids]


class TreeOracleEngine(CM.ClimbOracleEngine):
    """ClimbOracleEngine whose climb takes ``score``; ``climb_calls`` keeps (sets, rounds,
    per_round, seed, timeout_ms, score) of every call."""

    def climb(self, db, set_ids, rounds, per_round, seed=0, timeout_ms=0, score="sites"):
        ids = [int(s) for s in set_ids]
        self.climb_calls.append((len(ids), rounds, per_round, seed, timeout_ms, score))
        got = climb(db.batch, ids, rounds, per_round, seed, score)
        values = [ir.limbs_array(r.values) if r.values else np.zeros((0, 8), dtype=np.uint32) for r in got]
        return ClimbResult(np.array([r.status for r in got], dtype=np.uint32),
                           np.array([r.score for r in got], dtype=np.uint32),
                           np.array([r.round for r in got], dtype=np.uint32), values,
                           sum(r.evals for r in got), 0.0, False)
