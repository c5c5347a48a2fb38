"""Census of the buckets the search leaves on the bench's corpus (bench.py's corpus leg:
``corpus.build(48, 2, seed=2024)``), with hints on and with hints off.

    python tools/miss_census.py                          # prints the note
    python tools/miss_census.py --out profiles/r12_miss_census.md
    python tools/miss_census.py --oracle --scenarios 6 --budget 256      # no GPU (slow: the model)

For each configuration: every distinct bucket of the corpus is lowered as check_sets lowers it and
searched once (early exit); the buckets left without a witness are uploaded as a batch of their
own, on which a census (pf_census_batch) and the plain full sweep (pf_check_batch without early
exit, with and without short-circuit) are timed by their HIP events, the median of ``--repeat``
runs each.  One row per left-over bucket: the opcode that writes its most-blocking site (the site
the fewest candidates pass), holds / budget there, and the fewest failing sites of any candidate.
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys
from collections import Counter
from dataclasses import replace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

I_ASSERT = 1 << 24


def site_writers(code, descs):
    """Per set of a device batch (pf_device_batch's code and descriptors): for every assert site
    the opcode that writes the asserted B value — the fused op itself, or for a plain PF_ASSERT
    the last writer of its B register."""
    from mythril_amd import ir

    out = []
    for d in descs.tolist():
        last = {}
        ops = []
        for w0, w1, _, _ in code[d[0]:d[0] + d[1]].tolist():
            op = w0 & 0xFF
            if op == ir.ASSERT:
                ops.append(last.get((w1 >> 8) & 31, ir.ASSERT))
            elif ir.B_CONST <= op <= ir.B_FILL:
                last[w1 & 31] = op
                if w0 & I_ASSERT:
                    ops.append(op)
        out.append(ops)
    return out


def run_config(c, cfg, eng, repeat):
    from mythril_amd import _lib, ir
    from mythril_amd.smt import gpu_check

    gpu_check.reset_cache()
    _, failed, progs, _, keys = gpu_check.distinct_buckets([q.constraints for q in c.queries], c.kfm.registry, cfg)
    db = eng.upload(progs)
    try:
        res = eng.check(db, budget=cfg.budget, seed=cfg.seed, flags=cfg.flags)
    finally:
        db.free()
    missed = [i for i in range(len(progs)) if res.found[i] == 0xFFFFFFFF]
    out = {"hints": cfg.hints, "buckets": len(progs), "not_lowered": len(failed), "left": len(missed),
           "budget": cfg.budget, "rows": []}
    if not missed:
        return out
    mprogs = [progs[i] for i in missed]
    db = eng.upload(mprogs)
    try:
        ids = list(range(len(mprogs)))
        cens, t_cen, t_full, t_sc = None, [], [], []
        for _ in range(repeat):
            cens = eng.census(db, ids, budget=cfg.budget, seed=cfg.seed)
            t_cen.append(cens.kernel_ms)
            t_full.append(eng.check(db, budget=cfg.budget, seed=cfg.seed, flags=0).kernel_ms)
            t_sc.append(eng.check(db, budget=cfg.budget, seed=cfg.seed, flags=ir.FLAG_SHORTCIRCUIT).kernel_ms)
        batch = db.batch
        dcode, ddescs, _ = _lib.device_batch(batch.code, batch.consts, batch.descs)
        writers = site_writers(dcode, ddescs)
    finally:
        db.free()
    for j, i in enumerate(missed):
        holds = cens.holds[j].tolist()
        k = min(range(len(holds)), key=lambda s: (holds[s], s)) if holds else None
        out["rows"].append({
            "bucket": i, "conjuncts": len(keys[i]), "ins": int(ddescs[j][1]), "sites": len(holds),
            "op": ir.OPNAMES.get(writers[j][k], str(writers[j][k])) if k is not None else "-",
            "site": k, "holds": holds[k] if k is not None else 0,
            "alive_last": int(cens.alive[j][-1]) if holds else cfg.budget,
            "best_fails": int(cens.best_fails[j])})
    med = statistics.median
    out.update(census_ms=med(t_cen), full_ms=med(t_full), full_shortcircuit_ms=med(t_sc))
    return out


def _ratio(a, b) -> str:
    return f"{a / b:.2f}" if b > 0 else "n/a"


def note(results, args) -> str:
    lines = ["# Census of the buckets the search leaves on the bench corpus", "",
             f"`python tools/miss_census.py` — corpus.build({args.scenarios}, 2, seed=2024), budget "
             f"{results[0]['budget']:,} candidates per bucket, median of {args.repeat} runs per timing.", ""]
    for r in results:
        h = "on" if r["hints"] else "off"
        lines += [f"## Hints {h}", "",
                  f"{r['buckets']} distinct buckets searched ({r['not_lowered']} not lowered), "
                  f"{r['left']} left without a witness.", ""]
        if not r["rows"]:
            continue
        n = r["left"]
        lines += [f"Kernel time over the {n} left-over buckets as one batch (HIP events): census "
                  f"{r['census_ms']:.3f} ms = {r['census_ms'] / n:.4f} ms per bucket; plain full sweep without "
                  f"short-circuit {r['full_ms']:.3f} ms = {r['full_ms'] / n:.4f} ms per bucket (census / sweep = "
                  f"{_ratio(r['census_ms'], r['full_ms'])}); full sweep with short-circuit "
                  f"{r['full_shortcircuit_ms']:.3f} ms = {r['full_shortcircuit_ms'] / n:.4f} ms per bucket "
                  f"(census / sweep = {_ratio(r['census_ms'], r['full_shortcircuit_ms'])}).", ""]
        ops = Counter(row["op"] for row in r["rows"])
        lines += ["Most-blocking site by the opcode that writes it: " +
                  ", ".join(f"{op} {k}" for op, k in ops.most_common()) + ".",
                  "Fewest failing sites of any candidate: " +
                  ", ".join(f"{f} in {k} buckets" for f, k in sorted(Counter(row["best_fails"]
                                                                             for row in r["rows"]).items())) + ".", ""]
        lines += ["| bucket | conjuncts | device instructions | sites | most-blocking site | written by | "
                  "holds / budget | best_fails |", "|---|---|---|---|---|---|---|---|"]
        for row in r["rows"]:
            lines.append(f"| {row['bucket']} | {row['conjuncts']} | {row['ins']} | {row['sites']} | {row['site']} | "
                         f"{row['op']} | {row['holds']} / {r['budget']} | {row['best_fails']} |")
        lines.append("")
    return "\n".join(lines)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scenarios", type=int, default=48, help="corpus.build's scenario count (bench.py: 48)")
    ap.add_argument("--budget", type=int, default=None, help="candidates per bucket")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", metavar="FILE", help="write the note here instead of standard output")
    ap.add_argument("--oracle", action="store_true", help="the tests' oracle-backed engine instead of the GPU")
    args = ap.parse_args(argv)

    import mythril_amd.engine as E
    from mythril_amd import corpus
    from mythril_amd.smt import gpu_check

    if args.oracle:
        import pyoracle as O
        from census_model import CensusOracleEngine
        from mythril_amd import keccak_manager as KM
        from mythril_amd.smt import symbol_factory

        KM.KeccakFunctionManager.find_concrete_keccak = staticmethod(
            lambda data: symbol_factory.BitVecVal(
                int.from_bytes(O.keccak256(data.value.to_bytes(data.size() // 8, "big")), "big"), 256))
        eng = CensusOracleEngine()
        E.get_engine = lambda device=None: eng
        gpu_check.CONFIG.workers = 1
    else:
        eng = E.get_engine()
    base = replace(gpu_check.CONFIG, climb_rounds=0, parents=False)
    if args.budget:
        base = replace(base, budget=args.budget)
    c = corpus.build(args.scenarios, 2, seed=2024)
    results = [run_config(c, replace(base, hints=h), eng, args.repeat) for h in (True, False)]
    text = note(results, args)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
