"""Discharge with and without the climb, on the bench's corpus (bench.py's corpus leg:
``corpus.build(48, 2, seed=2024)`` and ``labelled_unsat(c, n=256)``).

    python tools/climb_discharge.py                     # the four-way table at 16 x 2,048
    python tools/climb_discharge.py --climb 24:512
    python tools/climb_discharge.py --score tree        # the same with the tree score
    python tools/climb_discharge.py --sweep 8:256,16:512,24:512,32:1024,16:2048
    python tools/climb_discharge.py --oracle --scenarios 6 --budget 1024 --climb 4:64

For hints off and hints on, each with the climb off and on: queries and buckets answered, climbs
run, the rounds that found the climb's witnesses, kernel and wall milliseconds per climbed
bucket beside the plain search's per bucket, and the SAT answers on the UNSAT-labelled queries
(must be 0).  One JSON line per configuration, then a markdown table.  ``--oracle`` runs it on
the oracle-backed engine of the tests (no GPU; slow: the climb is the Python model there).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
from collections import Counter
from dataclasses import replace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _pairs(text):
    """ROUNDS[:CANDIDATES],... — CANDIDATES defaults to GpuConfig's, as for ``replay --climb``."""
    from mythril_amd.smt import gpu_check

    out = []
    for part in text.split(","):
        r, _, n = part.partition(":")
        out.append((int(r), int(n) if n else gpu_check.CONFIG.climb_candidates))
    return out


class Recorder:
    """Wraps an engine's ``climb`` and ``check`` / ``check_many`` to keep what check_sets does
    not report: the round of every climb witness, and the wall time of each call."""

    def __init__(self, eng):
        self.eng = eng
        self.rounds = Counter()
        self.climb_wall = self.search_wall = 0.0
        self.climb_ms = self.search_ms = 0.0
        self.searched = 0
        for name in ("climb", "check", "check_many"):
            if hasattr(eng, name):
                setattr(self, "_" + name, getattr(eng, name))
                setattr(eng, name, getattr(self, "wrap_" + name))

    def restore(self):
        for name in ("climb", "check", "check_many"):
            if hasattr(self, "_" + name):
                setattr(self.eng, name, getattr(self, "_" + name))

    def wrap_climb(self, db, set_ids, rounds, per_round, seed=0, timeout_ms=0, **how):
        from mythril_amd import ir

        t = time.perf_counter()
        r = self._climb(db, set_ids, rounds, per_round, seed=seed, timeout_ms=timeout_ms, **how)
        self.climb_wall += time.perf_counter() - t
        self.climb_ms += r.kernel_ms
        for s, rd in zip(r.status, r.round):
            if int(s) == ir.CLIMB_WITNESS:
                self.rounds[int(rd)] += 1
        return r

    def _timed(self, fn, dbs, *a, **kw):
        t = time.perf_counter()
        r = fn(dbs, *a, **kw)
        self.search_wall += time.perf_counter() - t
        self.search_ms += r.kernel_ms
        self.searched += len(r.found)
        return r

    def wrap_check(self, db, *a, **kw):
        return self._timed(self._check, db, *a, **kw)

    def wrap_check_many(self, dbs, *a, **kw):
        return self._timed(self._check_many, dbs, *a, **kw)


def run_config(c, unsat, cfg, eng):
    from mythril_amd.smt import gpu_check

    gpu_check.reset_cache()
    gpu_check.STATS.bucket_origin.clear()
    s0 = replace(gpu_check.STATS)
    rec = Recorder(eng)
    try:
        t = time.perf_counter()
        models = gpu_check.check_sets([q.constraints for q in c.queries], registry=c.kfm.registry, config=cfg)
        wall = time.perf_counter() - t
        main = (rec.climb_wall, rec.climb_ms, rec.search_wall, rec.search_ms, rec.searched, dict(rec.rounds))
        origins = dict(gpu_check.STATS.bucket_origin)
        buckets = gpu_check.STATS.buckets - s0.buckets
        climbed = gpu_check.STATS.climbed - s0.climbed
        climb_sat = gpu_check.STATS.climb_sat - s0.climb_sat
        fps = []
        for reg in {id(r): r for _, _, r in unsat}.values():
            group = [(cs, o) for cs, o, r in unsat if r is reg]
            ms = gpu_check.check_sets([cs for cs, _ in group], registry=reg, config=cfg)
            fps += [o for (cs, o), m in zip(group, ms) if m is not None]
    finally:
        rec.restore()
        gpu_check.reset_cache()
    climb_wall, climb_ms, search_wall, search_ms, searched, rounds = main
    n = len(models)
    answered = sum(m is not None for m in models)
    return {
        "hints": cfg.hints, "climb": [cfg.climb_rounds, cfg.climb_candidates] if cfg.climb_rounds else None,
        "score": cfg.climb_score if cfg.climb_rounds else None,
        "queries": n, "answered": answered, "pct": round(100.0 * answered / max(n, 1), 2),
        "buckets_searched": buckets, "buckets_answered": sum(origins.values()),
        "bucket_origin": origins, "climbed": climbed, "climb_sat": climb_sat,
        "witness_round_histogram": {str(k): v for k, v in sorted(rounds.items())},
        "climb_kernel_ms_per_bucket": round(climb_ms / climbed, 4) if climbed else None,
        "climb_wall_ms_per_bucket": round(1e3 * climb_wall / climbed, 4) if climbed else None,
        "search_kernel_ms_per_bucket": round(search_ms / searched, 4) if searched else None,
        "search_wall_ms_per_bucket": round(1e3 * search_wall / searched, 4) if searched else None,
        "check_sets_wall_s": round(wall, 3),
        "recheck_failures": gpu_check.STATS.recheck_failures - s0.recheck_failures,
        "unsat_labelled": len(unsat), "unsat_labelled_sat_answers": len(fps),
    }


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scenarios", type=int, default=48, help="corpus.build's scenario count (bench.py: 48)")
    ap.add_argument("--unsat", type=int, default=256, help="labelled-UNSAT queries (bench.py: 256)")
    ap.add_argument("--budget", type=int, default=None, help="candidates per bucket of the plain search")
    ap.add_argument("--climb", default="16", metavar="ROUNDS[:CANDIDATES]",
                    help="default: the recommended 16 rounds of GpuConfig.climb_candidates (2,048)")
    ap.add_argument("--sweep", default=None, metavar="R:N,R:N,...",
                    help="hints off only: climb off, then each pair")
    ap.add_argument("--score", choices=("sites", "tree"), default="sites",
                    help="how the climb scores a candidate (GpuConfig.climb_score)")
    ap.add_argument("--oracle", action="store_true", help="the tests' oracle-backed engine instead of the GPU")
    args = ap.parse_args(argv)

    import mythril_amd.engine as E
    from mythril_amd import corpus
    from mythril_amd.smt import gpu_check

    if args.oracle:
        import pyoracle as O
        from mythril_amd import keccak_manager as KM
        from mythril_amd.smt import symbol_factory
        from climb_tree_model import TreeOracleEngine

        KM.KeccakFunctionManager.find_concrete_keccak = staticmethod(
            lambda data: symbol_factory.BitVecVal(
                int.from_bytes(O.keccak256(data.value.to_bytes(data.size() // 8, "big")), "big"), 256))
        eng = TreeOracleEngine()
        E.get_engine = lambda device=None: eng
        gpu_check.CONFIG.workers = 1
    else:
        eng = E.get_engine()
    base = replace(gpu_check.CONFIG, climb_rounds=0, climb_score=args.score)
    if args.budget:
        base = replace(base, budget=args.budget)
    c = corpus.build(args.scenarios, 2, seed=2024)
    unsat = corpus.labelled_unsat(c, n=args.unsat)
    if args.sweep:
        configs = [replace(base, hints=False)] + [replace(base, hints=False, climb_rounds=r, climb_candidates=n)
                                                  for r, n in _pairs(args.sweep)]
    else:
        (r, n), = _pairs(args.climb)
        configs = [replace(base, hints=h, climb_rounds=cr, climb_candidates=n) for h in (False, True)
                   for cr in (0, r)]
    rows = []
    for cfg in configs:
        rows.append(run_config(c, unsat, cfg, eng))
        print(json.dumps(rows[-1], sort_keys=True), flush=True)
    print()
    print(f"score: {args.score}")
    print()
    print("| hints | climb | queries answered | % | buckets answered / searched | climbed | climb witnesses | "
          "witness rounds | climb kernel / wall ms per climbed bucket | search kernel / wall ms per bucket | "
          "SAT on UNSAT-labelled |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        climb = "off" if r["climb"] is None else f"{r['climb'][0]} x {r['climb'][1]}"
        hist = " ".join(f"{k}:{v}" for k, v in r["witness_round_histogram"].items()) or "-"
        print(f"| {'on' if r['hints'] else 'off'} | {climb} | {r['answered']} / {r['queries']} | {r['pct']} | "
              f"{r['buckets_answered']} / {r['buckets_searched']} | {r['climbed']} | {r['climb_sat']} | {hist} | "
              f"{r['climb_kernel_ms_per_bucket']} / {r['climb_wall_ms_per_bucket']} | "
              f"{r['search_kernel_ms_per_bucket']} / {r['search_wall_ms_per_bucket']} | "
              f"{r['unsat_labelled_sat_answers']} of {r['unsat_labelled']} |")
    return 0 if all(r["unsat_labelled_sat_answers"] == 0 and r["recheck_failures"] == 0 for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
