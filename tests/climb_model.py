"""Test tooling (not a test): the CPU model of the climb contract (include/pf_bytecode.h).

* ``score`` — a candidate's score on a set's *device program* (``pf_device_batch``: what
  pf_batch_create uploads), by an interpreter of its own for the device-only instruction bits
  (PF_I_ASSERT, PF_I_KA / KB, PF_I_FA / FB, a cleared PF_TR_WW, LDS spill slots).
* ``climb`` — the round loop over ``pyoracle.SetView`` and ``gen_values``: every round is an
  ordinary generation under the unchanged contract, with the round's seed and the parents
  replaced by the current assignment.

The GPU tests compare pf_climb_batch with this bit for bit; tests/test_climb_model.py checks the
model itself.  ``ClimbOracleEngine`` is the tests' oracle-backed engine with ``climb`` by way of
the model.  Never imported by mythril_amd/.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

import oracle_engine
import pyoracle as O
from mythril_amd import _lib, ir
from mythril_amd.engine import ClimbResult

I_ASSERT, I_KA, I_KB, I_FA, I_FB = 1 << 24, 1 << 25, 1 << 26, 1 << 27, 1 << 28
TR_WW = 4 << 18
_ORDER = (O.OP["B_ULT"], O.OP["B_ULE"], O.OP["B_SLT"], O.OP["B_SLE"])


def near_term(op: int, a: int, b: int) -> int:
    """What a failing fused compare adds: a, b are the zero-extended register values."""
    if op == O.OP["B_EQ"]:
        return ir.CLIMB_NEAR - bin(a ^ b).count("1")
    if op in _ORDER:
        return ir.CLIMB_NEAR - abs(a - b).bit_length()
    return 0


@dataclass
class DeviceSet:
    """One set's device program: instruction rows and the constants they index (the set's
    range of the device pool: its own n_const constants, then the device program's)."""

    code: List[tuple]
    consts: List[int]

    @property
    def sites(self) -> int:
        return sum(1 for (w0, _, _, _) in self.code
                   if (w0 & 0xFF) == O.OP["ASSERT"] or (w0 & I_ASSERT))

    @property
    def target(self) -> int:
        return ir.CLIMB_HOLDS * self.sites

    def _decoded(self):
        """The program decoded once: (class, fn, w, d, ra, rb, rc, aux0, w0, op) per instruction
        up to END.  Classes: 0 W(a, b, w) 1 compare 2 the rest (by opcode)."""
        rows = self.__dict__.get("_rows")
        if rows is None:
            rows = []
            for (w0, w1, aux0, _aux1) in self.code:
                op, w = w0 & 0xFF, (w0 >> 8) & 0x3FF
                if op == O.OP["END"]:
                    break
                cls, fn = (0, O._WBIN[op]) if op in O._WBIN else (1, O._BCMP[op]) if op in O._BCMP else (2, None)
                rows.append((cls, fn, w, w1 & 0xFF, (w1 >> 8) & 0xFF, (w1 >> 16) & 0xFF, (w1 >> 24) & 0xFF,
                             aux0, w0, op))
            self.__dict__["_rows"] = rows
        return rows

    def run(self, values: Sequence[int]):
        """(root, score) of one assignment — the kernel's scored mode: no short-circuit."""
        W: List[Optional[int]] = [None] * 256
        B = [False] * 32
        S: Dict[int, int] = {}
        root, score, last = True, 0, None
        C = self.consts
        OP = O.OP
        HOLDS = ir.CLIMB_HOLDS
        for (cls, fn, w, d, ra, rb, rc, aux0, w0, op) in self._decoded():
            a = C[ra] if w0 & I_KA else (last if w0 & I_FA else W[ra])
            b = C[rb] if w0 & I_KB else (last if w0 & I_FB else W[rb])
            m = (1 << w) - 1
            z = None          # W result
            bres = None       # B result
            if cls == 0:
                z = fn(a, b, w) & m
            elif cls == 1:
                bres = bool(fn(a, b, w))
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
                z = (a if B[rc & 31] else b) & m
            elif op == OP["W_HASH"]:
                z = O.uf_hash(a, aux0) & m
            elif op == OP["W_SPILL"]:
                S[aux0] = a
            elif op == OP["W_FILL"]:
                z = S[aux0] & m
            elif op == OP["B_SPILL"]:
                S[aux0] = int(B[ra & 31])
            elif op == OP["B_FILL"]:
                bres = bool(S[aux0] & 1)
            elif op == OP["B_CONST"]:
                bres = bool(aux0 & 1)
            elif op == OP["B_VAR"]:
                bres = bool(int(values[aux0]) & 1)
            elif op == OP["B_AND"]:
                bres = B[ra & 31] and B[rb & 31]
            elif op == OP["B_OR"]:
                bres = B[ra & 31] or B[rb & 31]
            elif op == OP["B_XOR"]:
                bres = B[ra & 31] != B[rb & 31]
            elif op == OP["B_NOT"]:
                bres = not B[ra & 31]
            elif op == OP["B_ITE"]:
                bres = B[ra & 31] if B[rc & 31] else B[rb & 31]
            elif op == OP["ASSERT"]:
                holds = B[ra & 31]
                root = root and holds
                score += HOLDS if holds else 0
            else:
                raise ValueError(f"climb model: unknown opcode {op}")
            if z is not None:
                last = z
                if w0 & TR_WW:
                    W[d] = z
            elif bres is not None:
                B[d & 31] = bres
                if w0 & I_ASSERT:
                    root = root and bres
                    if bres:
                        score += HOLDS
                    elif cls == 1:
                        score += near_term(op, a, b)
        return root, score & 0xFFFFFFFF

    def score(self, values: Sequence[int]) -> int:
        return self.run(values)[1]


def device_sets(batch: ir.Batch) -> List[DeviceSet]:
    """The device programs of a batch, one DeviceSet per set (pf_device_batch, host only)."""
    if len(batch) == 0:
        return []
    code, descs, pool = _lib.device_batch(batch.code, batch.consts, batch.descs)
    out = []
    for d in descs.tolist():
        rows = [tuple(int(x) for x in r) for r in code[d[0]:d[0] + d[1]]]
        top = d[3]
        for (w0, w1, aux0, _) in rows:
            if (w0 & 0xFF) == O.OP["W_CONST"]:
                top = max(top, aux0 + 1)
            if w0 & I_KA:
                top = max(top, ((w1 >> 8) & 0xFF) + 1)
            if w0 & I_KB:
                top = max(top, ((w1 >> 16) & 0xFF) + 1)
        out.append(DeviceSet(rows, [O.limbs_to_int(r) for r in pool[d[2]:d[2] + top]]))
    return out


def pick_best(scores: Sequence[int], first: int) -> Optional[int]:
    """The best index among [first, len): highest score, ties to the smallest index."""
    best = None
    for i in range(first, len(scores)):
        if best is None or scores[i] > scores[best]:
            best = i
    return best


@dataclass
class SetClimb:
    status: int
    score: int
    round: int
    values: List[int]
    index: int = 0
    evals: int = 0


def climb_set(sv: O.SetView, dev: DeviceSet, rounds: int, per_round: int, seed: int,
              score_fn=None) -> SetClimb:
    """The climb of one set.  ``score_fn`` (values -> score) replaces the device score in the
    model's own tests."""
    score_of = score_fn or dev.score
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
            best = pick_best(scores, 1 if r else 0)   # candidate 0 is A_r itself from round 1 on
            if best is not None and scores[best] >= cur:   # sideways moves are taken
                cur, cur_round, cur_index, A = scores[best], r, best, [int(x) for x in assigns[best]]
            if score_fn is None and cur == target:
                status = ir.CLIMB_WITNESS
                break
    finally:
        sv.parents = own
    return SetClimb(status, cur, cur_round, A if A is not None else [], cur_index, evals)


def climb(batch: ir.Batch, set_ids: Sequence[int], rounds: int, per_round: int, seed: int = 0,
          devs: Optional[List[DeviceSet]] = None) -> List[SetClimb]:
    """pf_climb_batch on the CPU: one SetClimb per requested set, in request order."""
    devs = devs if devs is not None else device_sets(batch)
    return [climb_set(O.SetView.from_batch(batch, int(s)), devs[int(s)], rounds, per_round, seed)
            for s in set_ids]


class ClimbOracleEngine(oracle_engine.OracleEngine):
    """OracleEngine plus Engine.climb, by way of the model; ``climb_calls`` keeps
    (sets, rounds, per_round, seed, timeout_ms) of every call."""

    def __init__(self):
        super().__init__()
        self.climb_calls = []

    def climb(self, db, set_ids, rounds, per_round, seed=0, timeout_ms=0):
        ids = [int(s) for s in set_ids]
        self.climb_calls.append((len(ids), rounds, per_round, seed, timeout_ms))
        got = climb(db.batch, ids, rounds, per_round, seed)
        values = [ir.limbs_array(r.values) if r.values else np.zeros((0, 8), dtype=np.uint32) for r in got]
        return ClimbResult(np.array([r.status for r in got], dtype=np.uint32),
                           np.array([r.score for r in got], dtype=np.uint32),
                           np.array([r.round for r in got], dtype=np.uint32), values,
                           sum(r.evals for r in got), 0.0, False)
