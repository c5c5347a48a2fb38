"""Census of the assert sites of device programs, by the opcode that writes them (CPU only).

    python tools/assert_site_census.py                       # the bench corpus: corpus.build(48, 2, seed=2024)
    python tools/assert_site_census.py --scenarios 6 --out profiles/census_small.md

The climb scores a candidate at its assert sites — every PF_ASSERT and every B op carrying
PF_I_ASSERT of the *device program* (what pf_batch_create uploads).  Under the sites score only a
failing fused compare adds a distance; every other failing site adds 0.  This tool counts, over
the buckets check_sets lowers with hints off,

* all sites, by writer opcode (for a plain PF_ASSERT: the last writer of its B register), and
* the sites that fail under the generator's candidates 0..63, by the same opcode,

and writes the table to ``--out`` (default profiles/assert_site_census.md).  Nothing is searched:
check_sets runs on a collecting engine that finds no witness, so every bucket is lowered once."""

from __future__ import annotations

import argparse
import os
import sys
from collections import Counter
from dataclasses import replace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FUSED_DISTANCE = ("B_EQ", "B_ULT", "B_ULE", "B_SLT", "B_SLE")      # the sites score's gradient


def site_writers(dev):
    """[(pc of the site, opcode that wrote the asserted B value)] of one device program."""
    from mythril_amd import ir

    last = {}
    out = []
    for pc, (w0, w1, _, _) in enumerate(dev.code):
        op = w0 & 0xFF
        if op == ir.END:
            break
        if ir.B_CONST <= op <= ir.B_FILL:
            last[w1 & 31] = op
            if w0 & (1 << 24):
                out.append((pc, op))
        elif op == ir.ASSERT:
            out.append((pc, last.get((w1 >> 8) & 31, ir.ASSERT)))
    return out


def census(batches, n_cand=64, seed=0, progress=None):
    """(all sites by opcode, failing site evaluations by opcode, buckets, buckets with a failing
    site the sites score is flat at, site evaluations)."""
    import numpy as np

    import climb_model as CM
    import climb_tree_model as TM
    import pyoracle as O
    from mythril_amd import ir

    all_sites, failing = Counter(), Counter()
    buckets = flat_buckets = evals = 0
    cands = np.arange(n_cand, dtype=np.uint64)
    for batch in batches:
        devs = CM.device_sets(batch)
        for s, dev in enumerate(devs):
            writers = dict(site_writers(dev))
            for op in writers.values():
                all_sites[ir.OPNAMES[op]] += 1
            sv = O.SetView.from_batch(batch, s)
            flat = False
            for values in sv.gen_assignments(cands, seed):
                held = []
                TM.tree_run(dev, values, sites=held)
                assert [pc for pc, _ in held] == list(writers)
                for pc, ok in held:
                    evals += 1
                    if not ok:
                        name = ir.OPNAMES[writers[pc]]
                        failing[name] += 1
                        fused = dev.code[pc][0] & (1 << 24) and name in FUSED_DISTANCE
                        flat = flat or not fused
            buckets += 1
            flat_buckets += flat
            if progress and buckets % 100 == 0:
                progress(buckets)
    return all_sites, failing, buckets, flat_buckets, evals


class Collector:
    """An engine that keeps what check_sets uploads and finds nothing."""

    def __init__(self):
        self.batches = []

    def upload(self, programs):
        from mythril_amd import ir

        batch = programs if isinstance(programs, ir.Batch) else ir.Batch(programs)
        self.batches.append(batch)
        return _Held(batch)

    def check(self, db, budget=65536, seed=0, flags=0, timeout_ms=0):
        import numpy as np

        from mythril_amd.engine import NOT_FOUND, CheckResult

        return CheckResult(np.full(len(db), NOT_FOUND, dtype=np.uint32), 0, 0, 0, 0.0)


class _Held:
    def __init__(self, batch):
        self.batch = batch

    def __len__(self):
        return len(self.batch)

    def free(self):
        pass


def table(all_sites, failing, buckets, flat_buckets, evals, n_cand, title):
    n_all, n_fail = sum(all_sites.values()), sum(failing.values())
    lines = [f"# Assert-site census: {title}", "",
             f"{buckets} buckets (device programs, hints off), {n_all} assert sites; candidates 0..{n_cand - 1} of the "
             f"generator: {evals} site evaluations, {n_fail} of them failing.", "",
             "| writer of the site | sites | % | failing evaluations | % | distance under `sites` |", "|---|---|---|---|---|---|"]
    for name in sorted(set(all_sites) | set(failing), key=lambda n: -all_sites[n]):
        lines.append(f"| `{name}` | {all_sites[name]} | {100.0 * all_sites[name] / max(n_all, 1):.1f} | {failing[name]} | "
                     f"{100.0 * failing[name] / max(n_fail, 1):.1f} | {'when fused' if name in FUSED_DISTANCE else 'none'} |")
    lines += ["", f"Buckets with at least one failing site that adds 0 under the sites score: {flat_buckets} of {buckets}."]
    return "\n".join(lines) + "\n"


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scenarios", type=int, default=48, help="corpus.build's scenario count (bench.py: 48)")
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assert_site_census.md"))
    args = ap.parse_args(argv)

    import mythril_amd.engine as E
    import pyoracle as O
    from mythril_amd import corpus
    from mythril_amd import keccak_manager as KM
    from mythril_amd.smt import gpu_check, symbol_factory

    KM.KeccakFunctionManager.find_concrete_keccak = staticmethod(
        lambda data: symbol_factory.BitVecVal(
            int.from_bytes(O.keccak256(data.value.to_bytes(data.size() // 8, "big")), "big"), 256))
    eng = Collector()
    E.get_engine = lambda device=None: eng
    gpu_check.CONFIG.workers = 1
    cfg = replace(gpu_check.CONFIG, hints=False, climb_rounds=0)
    c = corpus.build(args.scenarios, 2, seed=2024)
    gpu_check.reset_cache()
    gpu_check.check_sets([q.constraints for q in c.queries], registry=c.kfm.registry, config=cfg)
    gpu_check.reset_cache()
    res = census(eng.batches, args.candidates, cfg.seed,
                 progress=lambda n: print(f"{n} buckets", file=sys.stderr, flush=True))
    text = table(*res, args.candidates, f"corpus.build({args.scenarios}, 2, seed=2024)")
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
