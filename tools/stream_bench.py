#!/usr/bin/env python3
"""The SoA candidate-streaming mode, measured ("HBM GB/s for the SoA
candidate-streaming mode"): pf_eval_batch_dev over device-generated candidates, against the same
job done one set at a time with pf_eval_assignments_dev on one stream.

Workloads (``--workloads``):
  config3   ``--sets`` config-3 sets (mythril_amd.synth) x ``--cands`` candidates
  light     ``--sets`` sets of one ULT over two 256-bit variables: almost no arithmetic per byte,
            the case where HBM is the bound
The candidates are torch.randint words made on the device; nothing is copied from the host.

Per workload the three jobs run in alternation, ``--reps`` times, each timed with device events
on one stream around everything it enqueues:
  stream      Engine.eval_stream, PF_FLAG_SHORTCIRCUIT on (the call's default)
  stream_full the same with the flag off
  loop        pf_eval_assignments_dev, set after set (one byte per verdict)
Reported: each repetition's times, the medians, the spread ((max - min) / median), evals/s, the
algorithmic HBM bytes — per set n_cand x 32 x n_vars read + n_cand / 8 written — as GB/s and as a
share of ``--peak-tbs`` TB/s, the ratio loop / stream, and whether stream was the faster in every
alternation.  The kernels' own time (pf_stats.kernel_ms) is reported beside the event time.  The
verdicts of the two paths are compared before anything is timed.  One JSON line at the end.

``--lib PATH`` loads another build of libpathfeas.so (an A/B of two builds alternates processes).
"""

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def programs(kind, n):
    from mythril_amd import ir, synth
    from mythril_amd.lower import Dag, lower

    if kind == "config3":
        return synth.random_dag_programs(50_000, n, plant=False)[0]
    out = []
    for i in range(n):
        dag = Dag()
        a, b = dag.var("a", 256), dag.var("b", 256)
        dag.assert_(dag.op(ir.B_ULT, 256, a, b))
        out.append(lower(dag, seed=i, name=f"ult{i}"))
    return out


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def run(engine, kind, args, torch):
    from mythril_amd import _lib, ir

    progs = programs(kind, args.sets)
    batch = ir.Batch(progs)
    db = engine.upload(batch)
    n, n_cand = len(progs), args.cands
    nv = [int(x) for x in batch.descs[:, 5]]
    off = [int(x) for x in batch.descs[:, 4]]
    V = int(batch.schema.shape[0])
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    # random bytes viewed as words: every bit of every limb is random
    soa = torch.randint(0, 256, (V * 8 * n_cand * 4,), dtype=torch.uint8, device=dev, generator=gen)
    soa = soa.view(torch.int32).view(V, 8, n_cand)
    words = (n_cand + 63) // 64
    out = (torch.empty((n, words), dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
           torch.empty(n, dtype=torch.int32, device=dev))
    loop_out = torch.empty((n, n_cand), dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    L = _lib.lib()
    row = 8 * n_cand * 4       # bytes per variable row

    def stream_job(sc):
        engine.eval_stream(db, soa, out=out, stream=st, shortcircuit=sc)

    def loop_job():
        for s in range(n):
            _lib.check(L.pf_eval_assignments_dev(db.handle, s, soa.data_ptr() + off[s] * row, n_cand,
                                                 loop_out.data_ptr() + s * n_cand, st.cuda_stream),
                       "pf_eval_assignments_dev")

    def timed(job):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        job()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    jobs = {"stream": lambda: stream_job(True), "stream_full": lambda: stream_job(False), "loop": loop_job}
    # warm-up, and the two paths' verdicts against each other
    for _ in range(args.warmup):
        for j in jobs.values():
            timed(j)
    timed(jobs["stream"])
    shifts = torch.arange(64, dtype=torch.int64, device=dev)
    same = True
    for s in range(n):           # set by set: the unpacked words are 8 bytes per verdict
        v = ((out[0][s].unsqueeze(-1) >> shifts) & 1).reshape(-1)[:n_cand].to(torch.uint8)
        same = same and bool(torch.equal(v, loop_out[s]))
        same = same and int(out[2][s].item()) == int(loop_out[s].sum().item())
    if not same:
        raise SystemExit(f"{kind}: the stream call and the per-set loop disagree")
    n_true = int(out[2].sum().item())

    times = {k: [] for k in jobs}
    for _ in range(args.reps):
        for k, j in jobs.items():
            times[k].append(timed(j))
    # the kernels' own time, by the library's events
    stats = _lib.pf_stats()
    ids = (ctypes.c_uint32 * n)(*range(n))
    kms = []
    for _ in range(3):
        _lib.check(L.pf_eval_batch_dev(db.handle, ids, n, soa.data_ptr(), n_cand, ir.FLAG_SHORTCIRCUIT, out[0].data_ptr(),
                                       out[1].data_ptr(), out[2].data_ptr(), ctypes.byref(stats), st.cuda_stream),
                   "pf_eval_batch_dev")
        kms.append(float(stats.kernel_ms))
    evals = n * n_cand
    hbm = sum(n_cand * 32 * v + n_cand // 8 for v in nv)
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {
        "workload": kind, "sets": n, "n_cand": n_cand, "variables": V,
        "hbm_bytes": hbm, "true_verdicts": n_true, "evals_full": int(stats.evals_full),
        "cands_decided": int(stats.cands_decided),
        "ms": {k: [round(x, 4) for x in v] for k, v in times.items()},
        "median_ms": {k: round(v, 4) for k, v in med.items()},
        "spread": {k: round(spread(v), 4) for k, v in times.items()},
        "kernel_ms": [round(x, 4) for x in kms],
        "evals_per_s": {k: evals / (v * 1e-3) for k, v in med.items()},
        "hbm_gbs": {k: hbm / (v * 1e-3) / 1e9 for k, v in med.items()},
        "hbm_gbs_kernel": hbm / (statistics.median(kms) * 1e-3) / 1e9,
        "share_of_peak": {k: hbm / (v * 1e-3) / (args.peak_tbs * 1e12) for k, v in med.items()},
        "ratio_loop_over_stream": med["loop"] / med["stream"],
        "ratio_loop_over_stream_full": med["loop"] / med["stream_full"],
        "stream_faster_every_time": all(a < b for a, b in zip(times["stream"], times["loop"])),
        "stream_full_faster_every_time": all(a < b for a, b in zip(times["stream_full"], times["loop"])),
        # faster by five spreads: the medians' gap against five times the larger spread, in ms
        "gap_over_5_spreads": (med["loop"] - med["stream"]) /
                              max(5 * max(spread(times["stream"]) * med["stream"], spread(times["loop"]) * med["loop"]),
                                  1e-9),
    }
    print(f"[{kind}] {n} sets x {n_cand} candidates, {V} variables, {hbm / 1e9:.3f} GB algorithmic, "
          f"{n_true} true verdicts", file=sys.stderr)
    for k in jobs:
        print(f"[{kind}] {k:11s} median {med[k]:9.3f} ms  spread {res['spread'][k]:.3f}  "
              f"{res['evals_per_s'][k] / 1e9:8.3f} G evals/s  {res['hbm_gbs'][k]:8.1f} GB/s "
              f"({100 * res['share_of_peak'][k]:.1f} % of {args.peak_tbs} TB/s)  {times[k]}", file=sys.stderr)
    print(f"[{kind}] kernel_ms {kms}; loop / stream = {res['ratio_loop_over_stream']:.2f}, "
          f"faster every time: {res['stream_faster_every_time']}", file=sys.stderr)
    del soa, out, loop_out
    db.free()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="light,config3")
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--cands", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--peak-tbs", type=float, default=8.0)
    ap.add_argument("--lib", default=None, help="another build of libpathfeas.so to load")
    args = ap.parse_args()
    import torch

    from mythril_amd import _lib

    if not torch.cuda.is_available():
        raise SystemExit("stream_bench: no GPU (there is no CPU fallback)")
    if args.lib:
        _lib.load_library(os.path.abspath(args.lib))
    from mythril_amd.engine import get_engine

    engine = get_engine(0)
    results = [run(engine, k, args, torch) for k in args.workloads.split(",") if k]
    print(json.dumps({"tool": "stream_bench", "lib": args.lib or "default", "results": results}))


if __name__ == "__main__":
    main()
