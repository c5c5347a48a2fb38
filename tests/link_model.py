"""Test tooling (not a test): the CPU model of the link contract (include/pf_bytecode.h).

A link group's verdict is the smallest candidate at which every member's verdict on the committed
C oracle (oracle/coracle.c, by way of coracle_py.Packed.eval_generated) holds.  The GPU test
compares pf_check_linked with this exactly; ``LinkOracleEngine`` is the tests' oracle-backed
engine with ``check_linked`` by way of the model.  Never imported by mythril_amd/.
"""

from __future__ import annotations

from typing import List, Sequence

import numpy as np

import coracle_py
import oracle_engine
from mythril_amd import ir
from mythril_amd.engine import NOT_FOUND, CheckResult


def shared_error(batch: ir.Batch, members: Sequence[int]) -> str:
    """What the members of one group fail to share under the contract, or ''."""
    a = int(members[0])
    da = batch.descs[a]
    for s in members[1:]:
        d = batch.descs[int(s)]
        if int(d[5]) != int(da[5]):
            return f"set {s}: n_vars"
        if int(d[3]) != int(da[3]):
            return f"set {s}: n_const"
        if int(d[6]) != int(da[6]):
            return f"set {s}: seed"
        nc = int(da[3])
        if nc and not np.array_equal(batch.consts[int(d[2]):int(d[2]) + nc], batch.consts[int(da[2]):int(da[2]) + nc]):
            return f"set {s}: constants"
        for v in range(int(da[5])):
            sa, sb = batch.schema[int(da[4]) + v], batch.schema[int(d[4]) + v]
            if not np.array_equal(sa[:3], sb[:3]):
                return f"set {s}: schema entry {v}"
            pa, pb = int(sa[3]), int(sb[3])
            if (pa == ir.NO_PARENT) != (pb == ir.NO_PARENT):
                return f"set {s}: parent of {v}"
            if pa != ir.NO_PARENT and not np.array_equal(batch.parents[pa], batch.parents[pb]):
                return f"set {s}: parent of {v}"
    return ""


def members_of(group_of: Sequence[int]) -> List[List[int]]:
    n = (max(int(g) for g in group_of) + 1) if len(group_of) else 0
    out: List[List[int]] = [[] for _ in range(n)]
    for s, g in enumerate(group_of):
        out[int(g)].append(s)
    return out


def group_masks(packed: coracle_py.Packed, members: Sequence[int], budget: int, seed: int) -> np.ndarray:
    """bool [budget]: candidate c is a witness of the group."""
    m = np.ones(budget, dtype=bool)
    for s in members:
        m &= packed.eval_generated(int(s), seed, 0, budget)
    return m


def check_linked(batch: ir.Batch, group_of: Sequence[int], budget: int, seed: int = 0,
                 packed: coracle_py.Packed = None) -> np.ndarray:
    """pf_check_linked on the CPU: uint32 [n_groups] verdicts."""
    if budget == 0:
        raise ValueError("link model: budget must be at least 1")
    if len(group_of) != len(batch):
        raise ValueError("link model: one group id per set")
    packed = packed if packed is not None else coracle_py.Packed(batch)
    groups = members_of(group_of)
    found = np.full(len(groups), NOT_FOUND, dtype=np.uint32)
    for g, mem in enumerate(groups):
        if not mem:
            raise ValueError(f"link model: group {g} is empty")
        if len(mem) > ir.LINK_MAX_PARTS:
            raise ValueError(f"link model: group {g} has {len(mem)} members")
        err = shared_error(batch, mem)
        if err:
            raise ValueError(f"link model: group {g}: {err}")
        idx = np.nonzero(group_masks(packed, mem, budget, seed))[0]
        if idx.size:
            found[g] = int(idx[0])
    return found


class LinkOracleEngine(oracle_engine.OracleEngine):
    """OracleEngine plus Engine.check_linked, by way of the model; ``linked_calls`` keeps
    (group_of, budget, seed, flags, timeout_ms) of every call."""

    def __init__(self):
        super().__init__()
        self.linked_calls = []

    def check_linked(self, db, group_of, budget=65536, seed=0, flags=0, timeout_ms=0):
        ids = [int(g) for g in group_of]
        self.linked_calls.append((ids, budget, seed, flags, timeout_ms))
        self.launches += 1
        self.last_budget = budget
        found = check_linked(db.batch, ids, budget, seed, db.packed)
        return CheckResult(found, budget * len(db), budget * len(db), 0, 0.0)
