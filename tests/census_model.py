"""Test tooling (not a test): the CPU model of the census contract (include/pf_bytecode.h).

Built on tests/climb_model.DeviceSet, the interpreter of device programs, and pyoracle's
candidate generator: the sites of a set are the PF_ASSERTs and PF_I_ASSERT-flagged B ops of its
device program, and what site j sees of an assignment is read off the program cut after site j —
its root is "sites 0..j all hold" (alive), and its sites score grows by CLIMB_HOLDS over the
prefix before it exactly when site j holds (a failing site adds at most CLIMB_NEAR).

The GPU test compares pf_census_batch with this exactly; tests/test_census_model.py checks the
model itself against the C oracle.  ``CensusOracleEngine`` is the tests' oracle-backed engine
with ``census`` by way of the model.  Never imported by mythril_amd/.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

import climb_model as CM
import pyoracle as O
from mythril_amd import ir
from mythril_amd.engine import CensusResult


def site_indices(dev: CM.DeviceSet) -> List[int]:
    """Instruction indices of the set's assert sites, in program order."""
    out = []
    for i, (w0, _, _, _) in enumerate(dev.code):
        if (w0 & 0xFF) == O.OP["END"]:
            break
        if (w0 & 0xFF) == O.OP["ASSERT"] or (w0 & CM.I_ASSERT):
            out.append(i)
    return out


def _prefixes(dev: CM.DeviceSet) -> List[CM.DeviceSet]:
    pre = dev.__dict__.get("_census_prefixes")
    if pre is None:
        pre = [CM.DeviceSet(dev.code[:i + 1], dev.consts) for i in site_indices(dev)]
        dev.__dict__["_census_prefixes"] = pre
    return pre


def site_values(dev: CM.DeviceSet, values: Sequence[int]) -> List[bool]:
    """The value of every assert site under one assignment (nothing short-circuits)."""
    out, before = [], 0
    for p in _prefixes(dev):
        _root, score = p.run(values)
        out.append(score - before == ir.CLIMB_HOLDS)
        before = score
    return out


@dataclass
class SetCensus:
    holds: List[int]
    alive: List[int]
    sole: List[int]
    best_fails: int
    best_cand: int
    status: int = ir.CENSUS_DONE
    evals: int = 0


def census_set(sv: O.SetView, dev: CM.DeviceSet, budget: int, seed: int) -> SetCensus:
    n = len(site_indices(dev))
    holds, alive, sole = [0] * n, [0] * n, [0] * n
    best = None
    memo: Dict[tuple, List[bool]] = {}
    assigns = sv.gen_assignments(np.arange(budget, dtype=np.uint64), seed)
    for c, a in enumerate(assigns):
        k = tuple(int(x) for x in a)
        if k not in memo:
            memo[k] = site_values(dev, k)
        vals = memo[k]
        ok = True
        for j, v in enumerate(vals):
            holds[j] += v
            ok = ok and v
            alive[j] += ok
        fails = [j for j, v in enumerate(vals) if not v]
        if len(fails) == 1:
            sole[fails[0]] += 1
        if best is None or len(fails) < best[0]:
            best = (len(fails), c)
    return SetCensus(holds, alive, sole, best[0], best[1], ir.CENSUS_DONE, budget)


def census(batch: ir.Batch, set_ids: Sequence[int], budget: int, seed: int = 0,
           devs: Optional[List[CM.DeviceSet]] = None) -> List[SetCensus]:
    """pf_census_batch on the CPU: one SetCensus per requested set, in request order."""
    devs = devs if devs is not None else CM.device_sets(batch)
    return [census_set(O.SetView.from_batch(batch, int(s)), devs[int(s)], budget, seed) for s in set_ids]


def as_result(got: List[SetCensus]) -> CensusResult:
    u = lambda xs: np.array(xs, dtype=np.uint32)
    return CensusResult([u(r.holds) for r in got], [u(r.alive) for r in got], [u(r.sole) for r in got],
                        u([r.best_fails for r in got]), u([r.best_cand for r in got]),
                        u([r.status for r in got]), sum(r.evals for r in got), 0.0, False)


class CensusOracleEngine(CM.ClimbOracleEngine):
    """ClimbOracleEngine plus Engine.census and Engine.site_counts, by way of the model;
    ``census_calls`` keeps (set ids, budget, seed, timeout_ms) of every call."""

    def __init__(self):
        super().__init__()
        self.census_calls = []

    def site_counts(self, db, set_ids):
        devs = CM.device_sets(db.batch)
        return np.array([devs[int(s)].sites for s in set_ids], dtype=np.uint32)

    def census(self, db, set_ids, budget=65536, seed=0, timeout_ms=0):
        ids = [int(s) for s in set_ids]
        self.census_calls.append((ids, budget, seed, timeout_ms))
        return as_result(census(db.batch, ids, budget, seed))
