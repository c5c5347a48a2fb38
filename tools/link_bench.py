"""Linked search against the unsplit early-exit search on the bench corpus's long buckets.

Population: the buckets of corpus.build(48, 2, seed=2024) whose lowered program has at least
--min-ins instructions (default 400), lowered with hints off, so the search walks the budget (the
case the single-query tail is made of).  Arms: the unsplit search (Engine.check) and
Engine.check_linked at K = 2, 4, 8, 16 parts (lower_parts).  Shapes: every bucket as a batch of
its own (the single query), and all of them as one batch.  The arms alternate within one process,
--reps rounds (at least five), after a warm-up round of every shape; per arm the median and the
min .. max of kernel time (HIP events, pf_stats.kernel_ms) and of wall time per call.  Verdicts of
every arm are compared with the unsplit search's.  Also: the duplication factor (sum of the
parts' instructions over the unsplit program's) per K, and, with --discharge, the discharge pass
(check_sets over the whole corpus) with the knob off and on, which must answer the same queries.

    python tools/link_bench.py [--reps 7] [--budget 65536] [--discharge] > profiles/...
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from mythril_amd import corpus, ir  # noqa: E402
from mythril_amd.engine import get_engine  # noqa: E402
from mythril_amd.lower import LoweringError, _spill_code  # noqa: E402
from mythril_amd.smt import gpu_check  # noqa: E402
from mythril_amd.smt.independence import buckets  # noqa: E402

KS = (2, 4, 8, 16)
FLAGS = ir.FLAG_EARLY_EXIT | ir.FLAG_SHORTCIRCUIT


def long_buckets(c, min_ins, hints):
    reg = c.kfm.registry
    seen, out = set(), []
    for q in c.queries:
        for b in buckets(q.constraints):
            if tuple(b) in seen:
                continue
            seen.add(tuple(b))
            try:
                _, prog = gpu_check._lower_bucket(list(b), reg, None, hints)
            except (LoweringError, ValueError, OverflowError):
                continue
            if _spill_code(prog)[0] >= min_ins:
                out.append((list(b), prog))
    return out, len(seen)


def parts_of(b, reg, hints, min_ins, k):
    _, prog = gpu_check._lower_bucket(b, reg, None, hints, (min_ins, k))
    return getattr(prog, "link_parts", None) or [prog]


def stat(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def run_arms(eng, arms, budget, seed, reps):
    """arms: name -> (db, group_of or None).  One warm-up round, then ``reps`` alternations."""
    kms = {a: [] for a in arms}
    wall = {a: [] for a in arms}
    found = {}
    for r in range(reps + 1):
        for name, (db, group_of) in arms.items():
            t = time.perf_counter()
            if group_of is None:
                res = eng.check(db, budget=budget, seed=seed, flags=FLAGS)
            else:
                res = eng.check_linked(db, group_of, budget=budget, seed=seed, flags=FLAGS)
            w = 1e3 * (time.perf_counter() - t)
            if r:
                kms[name].append(res.kernel_ms)
                wall[name].append(w)
            found[name] = res.found.copy()
    return kms, wall, found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--budget", type=int, default=65536)
    ap.add_argument("--min-ins", type=int, default=400)
    ap.add_argument("--scenarios", type=int, default=48)
    ap.add_argument("--discharge", action="store_true")
    a = ap.parse_args()
    eng = get_engine(0)
    c = corpus.build(a.scenarios, 2, seed=2024)
    reg = c.kfm.registry
    seed = gpu_check.CONFIG.seed
    pop, n_buckets = long_buckets(c, a.min_ins, hints=False)
    print(f"# link_bench: {len(pop)} of {n_buckets} distinct buckets have >= {a.min_ins} instructions "
          f"(hints off), budget {a.budget}, {a.reps} alternations after one warm-up round")
    sizes = [_spill_code(p)[0] for _, p in pop]
    print("sizes:", sorted(sizes))
    parts = {k: [parts_of(b, reg, False, a.min_ins, k) for b, _ in pop] for k in KS}
    print("\n## duplication factor (sum of part instructions / unsplit instructions), parts made")
    for k in KS:
        tot = sum(_spill_code(p)[0] for ps in parts[k] for p in ps)
        print(f"K={k}: {tot / max(1, sum(sizes)):.3f}  parts per bucket: {sorted(len(ps) for ps in parts[k])}")

    print("\n## every bucket as a batch of its own: ms, median (min .. max) over the alternations")
    print("| bucket ins | arm | kernel ms | wall ms per call | verdict |")
    print("|---|---|---|---|---|")
    tail = {name: [] for name in ["unsplit"] + [f"K={k}" for k in KS]}
    for i, (b, prog) in enumerate(pop):
        arms = {"unsplit": (eng.upload([prog]), None)}
        for k in KS:
            arms[f"K={k}"] = (eng.upload(parts[k][i]), [0] * len(parts[k][i]))
        kms, wall, found = run_arms(eng, arms, a.budget, seed, a.reps)
        for name in arms:
            same = int(found[name][0]) == int(found["unsplit"][0])
            print(f"| {sizes[i]} | {name} | {stat(kms[name])} | {stat(wall[name])} | "
                  f"{int(found[name][0])}{'' if same else ' DIFFERS'} |")
            tail[name].append((statistics.median(kms[name]), statistics.median(wall[name])))
        for db, _ in arms.values():
            db.free()
    print("\n## single-bucket summary over the population: median of medians, max of medians (ms)")
    for name, xs in tail.items():
        if xs:
            ks_, ws = [x[0] for x in xs], [x[1] for x in xs]
            print(f"{name}: kernel {statistics.median(ks_):.3f} / {max(ks_):.3f}   wall {statistics.median(ws):.3f} / {max(ws):.3f}")

    print("\n## all of them as one batch")
    if pop:
        arms = {"unsplit": (eng.upload([p for _, p in pop]), None)}
        for k in KS:
            progs, gof = [], []
            for g, ps in enumerate(parts[k]):
                progs += ps
                gof += [g] * len(ps)
            arms[f"K={k}"] = (eng.upload(progs), gof)
        kms, wall, found = run_arms(eng, arms, a.budget, seed, a.reps)
        for name in arms:
            same = bool((found[name] == found["unsplit"]).all())
            print(f"{name}: kernel {stat(kms[name])}  wall {stat(wall[name])}  verdicts {'same' if same else 'DIFFER'}")
        for db, _ in arms.values():
            db.free()

    if a.discharge:
        print("\n## discharge pass over the whole corpus (check_sets, 64 queries per call)")
        sets = [q.constraints for q in c.queries]
        answers = {}
        for name, (mi, k) in {"knob off": (0, 8), "knob on": (a.min_ins, 8)}.items():
            gpu_check.reset_cache()
            gpu_check.CONFIG.link_min_ins, gpu_check.CONFIG.link_parts = mi, k
            t = time.perf_counter()
            got = []
            for i in range(0, len(sets), 64):
                got += [m is not None for m in gpu_check.check_sets(sets[i:i + 64], reg)]
            answers[name] = got
            print(f"{name} (PF_LINK_MIN_INS={mi}, PF_LINK_PARTS={k}): {sum(got)} of {len(got)} queries answered, "
                  f"{time.perf_counter() - t:.2f} s")
        gpu_check.CONFIG.link_min_ins = 0
        print("same queries answered:", answers["knob off"] == answers["knob on"])
    print(json.dumps({"population": len(pop), "sizes": sorted(sizes)}))


if __name__ == "__main__":
    main()
