"""Replay a directory of ``--solver-log`` dumps on the GPU (BASELINE config 2 from files).

``replay_dir(DIR)`` / ``python -m mythril_amd.replay DIR``: every ``*.smt2`` file is read
(:mod:`mythril_amd.smtlib`, in worker processes), its keccak registry is recovered from its
own assertions (``smtlib.recover_registry`` — a dump carries no ``KeccakFunctionManager``),
the files are grouped by identical recovered registry, and each group is ONE
``gpu_check.check_sets`` call.  Every witness is then re-checked on the host against the
assertions read from its file; ``--models DIR`` writes it out as a certificate
(``<name>.model.smt2``) that any z3 answers ``sat`` to.

A file is ``objective`` (it has ``minimize`` / ``maximize``: minimising queries stay on z3 and
are never searched), ``error: <text>`` (it cannot be read or lowered, or a width with
symbolic keccak inputs has no single recovered interval), ``sat`` or ``unknown``.  One bad
file never stops the directory.  The witness caches of ``gpu_check`` are cleared before each
group: a cached witness is keyed by a registry summary, not by its concrete pairs, and a
file's answer must not depend on what else is in the directory.
"""

from __future__ import annotations

import json
import os
import sys
import time
from dataclasses import dataclass, field, replace
from typing import Dict, List, Optional, Tuple

from . import smtlib
from .lower import LoweringError
from .smt import terms as T

PHASES = ("read", "recover", "lower", "search", "recheck")
# check_sets' own phases (gpu_check.STATS.phase_s) under the report's names
_CHECK_PHASE = {"bucket": "lower", "lower": "lower", "probe": "search", "upload": "search",
                "search": "search", "climb": "search", "materialize": "search", "recheck": "recheck",
                "models": "recheck"}


@dataclass
class FileResult:
    name: str
    cls: str = "unknown"                 # "sat" | "unknown" | "objective" | "error: <text>"
    origin: Optional[str] = None         # witness provenance (gpu_check._origin) of a sat file:
                                         # "climb" / "search" / "hint" / "parent" / "first" / "cache"
    ms: float = 0.0                      # read + recover + re-check, plus the file's share of its group's check_sets
    model: Optional[object] = None       # the WitnessModel of a sat file
    query: Optional[smtlib.Query] = None
    registry: Optional[object] = None
    certificate: Optional[str] = None    # path of the written .model.smt2

    def values(self) -> Dict[str, str]:
        """The witness's free-symbol values, by name, as hex."""
        if self.model is None:
            return {}
        w = self.model.w
        out = {k: hex(v) for k, v in w.vars.items()}
        out.update({k: str(bool(v)).lower() for k, v in w.bools.items()})
        return dict(sorted(out.items()))

    def to_json(self) -> dict:
        return {"file": self.name, "class": self.cls, "origin": self.origin, "ms": round(self.ms, 3),
                "values": self.values()}


@dataclass
class ReplayReport:
    files: List[FileResult] = field(default_factory=list)
    phase_s: Dict[str, float] = field(default_factory=lambda: {p: 0.0 for p in PHASES})
    wall_s: float = 0.0
    groups: int = 0
    recheck_failures: int = 0            # witnesses the file-level re-check rejected (must stay 0)

    def count(self, cls: str) -> int:
        return sum(1 for f in self.files if f.cls == cls or (cls == "error" and f.cls.startswith("error:")))

    @property
    def files_per_s(self) -> float:
        return len(self.files) / self.wall_s if self.wall_s > 0 else 0.0

    @property
    def discharged_share(self) -> float:
        """Share of ``sat`` among the objective-free files."""
        free = len(self.files) - self.count("objective")
        return self.count("sat") / free if free else 0.0

    def totals(self) -> dict:
        return {"files": len(self.files), "sat": self.count("sat"), "unknown": self.count("unknown"),
                "objective": self.count("objective"), "error": self.count("error"),
                "groups": self.groups, "files_per_s": round(self.files_per_s, 3),
                "discharged_share": round(self.discharged_share, 4),
                "recheck_failures": self.recheck_failures, "wall_s": round(self.wall_s, 4),
                "phase_s": {k: round(v, 4) for k, v in self.phase_s.items()}}

    def json_lines(self) -> List[str]:
        """One line per file, in name order, then one ``{"totals": …}`` line."""
        return [json.dumps(f.to_json(), sort_keys=True) for f in self.files] + \
            [json.dumps({"totals": self.totals()}, sort_keys=True)]


def max_workers() -> int:
    """Reader processes: the CPUs this process may run on, 16 at the most."""
    return min(16, len(os.sched_getaffinity(0)))


def _read_job(path: str) -> Tuple[Optional[smtlib.Query], Optional[str], float]:
    """Worker: one file -> (query, error text, milliseconds).  The query's terms re-intern in
    the parent on unpickling."""
    t0 = time.perf_counter()
    try:
        with open(path) as f:
            q = smtlib.read_query(f.read())
        err = None
    except (ValueError, LoweringError, OSError, IndexError, KeyError, TypeError, RecursionError) as e:
        # tokenizer / reader errors; a truncated command shows as a short list
        q, err = None, f"{type(e).__name__}: {e}"
    return q, err, (time.perf_counter() - t0) * 1e3


def _read_all(paths: List[str], workers: int):
    n = max(1, min(workers, max_workers(), len(paths)))
    if n <= 1:
        return [_read_job(p) for p in paths]
    import multiprocessing as mp

    # spawn, never fork: this process may hold an initialised HIP runtime
    with mp.get_context("spawn").Pool(n) as pool:
        pending = [pool.apply_async(_read_job, (p,)) for p in paths]
        out = []
        for p, job in zip(paths, pending):
            try:
                out.append(job.get())
            except Exception:  # noqa: BLE001 - a result that does not pickle (nesting): read it here
                out.append(_read_job(p))
    return out


def _lowering_error(assertions: List[T.Term], reg, cfg) -> Optional[str]:
    """The text of the first bucket of the set that the lowering refuses, or None."""
    from .smt import gpu_check
    from .smt.independence import buckets

    cs = [c for c in assertions if c is not T.TRUE]
    try:
        bks = buckets(cs) if cfg.split else [cs]
    except (LoweringError, ValueError, RecursionError) as e:
        return str(e)
    for b in bks:
        try:
            gpu_check._lower_bucket(b, reg, None, cfg.hints)
        except (LoweringError, ValueError, OverflowError, RecursionError) as e:
            return str(e) if isinstance(e, LoweringError) else f"{type(e).__name__}: {e}"
    return None


# ---- witness certificates ----------------------------------------------------------------
_TAIL_COMMAND = ("check-sat", "get-model", "exit", "get-objectives")


def _strip_tail(text: str) -> str:
    """The dump without its ``(check-sat)`` / ``(get-model)`` / ``(exit)`` commands: the
    declarations and assertions verbatim."""
    import re

    return re.sub(r"\(\s*(?:%s)\s*\)[ \t]*\n?" % "|".join(_TAIL_COMMAND), "", text).rstrip() + "\n"


def certificate_pins(query: smtlib.Query, model) -> List[str]:
    """The ``assert`` lines that pin the witness: every declared free symbol, every base-array
    read the witness fixed, and every UF application of the file (the witness's tables and
    any application the lowering interpreted away), each at its value under the witness.
    Raises ``ValueError`` if the interpretation is not a function (two values for one
    application): such a witness has no certificate."""
    w = model.w
    lines = []
    for name, (doms, rng) in query.decls.items():
        if doms:
            continue
        if rng == T.BOOL:
            lines.append(f"(assert (= {smtlib.quote_symbol(name)} {str(bool(w.bools.get(name, False))).lower()}))")
        elif rng[0] == "bv":
            lines.append(f"(assert (= {smtlib.quote_symbol(name)} {smtlib.literal(w.vars.get(name, 0), rng[1])}))")
    for name, tab in sorted(w.tables().items()):
        srt = query.decls.get(name, ((), None))[1]
        if srt is None or srt[0] != "array":
            continue
        for iv, v in sorted(tab.items()):
            lines.append(f"(assert (= (select {smtlib.quote_symbol(name)} {smtlib.literal(iv, srt[1])}) "
                         f"{smtlib.literal(int(v), srt[2])}))")
    apps, seen, stack = [], set(), list(query.assertions)
    while stack:
        t = stack.pop()
        if t in seen:
            continue
        seen.add(t)
        if t.op == "apply":
            apps.append(t)
        stack.extend(t.args)
    apps += [app for (_, _, app) in w.uf_apps if app not in seen]
    table: Dict[tuple, int] = {}
    for app in apps:
        key = (app.val[0], tuple(int(w.ev(a)) for a in app.args))
        val = int(w.ev(app))
        if table.setdefault(key, val) != val:
            raise ValueError(f"{key[0]} takes two values at one argument under the witness")
    for (fname, argv), val in sorted(table.items()):
        doms, rng = query.decls[fname]
        args = " ".join(smtlib.literal(a, d[1]) for a, d in zip(argv, doms))
        lines.append(f"(assert (= ({smtlib.quote_symbol(fname)} {args}) {smtlib.literal(val, rng[1])}))")
    return lines


def write_certificate(path: str, text: str, query: smtlib.Query, model) -> None:
    """``<name>.model.smt2``: the dump's declarations and assertions verbatim, one assertion
    per pinned value, ``(check-sat)`` — ``z3 file`` prints ``sat``."""
    pins = certificate_pins(query, model)
    with open(path, "w") as f:
        f.write(_strip_tail(text))
        f.write("; witness\n")
        f.write("\n".join(pins))
        f.write("\n(check-sat)\n")


# ---- the replay ---------------------------------------------------------------------------
EXPLAIN_TERM_CHARS = 160    # a conjunct's s-expression in an --explain report is cut here


def explanation_lines(name: str, ex) -> List[str]:
    """The ``--explain`` report of one undischarged dump (``ex``: its
    ``gpu_check.SetExplanation``): per bucket its outcome and, for a miss, the blocking conjuncts
    — those that fail for some candidate — most blocking first (by ``alive``, then ``sole``),
    each s-expression cut at EXPLAIN_TERM_CHARS, then the nearest miss."""
    lines = [f"{name}: {ex.outcome}"]
    for k, b in enumerate(ex.buckets):
        lines.append(f"bucket {k}: {b.outcome} ({len(b.constraints)} conjuncts)")
        if b.outcome != "miss":
            continue
        folded = sum(1 for r in b.rows if r.folded)
        lines.append(f"  candidates {b.budget}, roots {len(b.rows)} ({folded} folded), "
                     f"nearest miss fails {b.best_fails} at candidate {b.best_cand}")
        for r in b.blocking():
            text = r.label
            if len(text) > EXPLAIN_TERM_CHARS:
                text = text[:EXPLAIN_TERM_CHARS] + "..."
            lines.append(f"  alive {r.alive:>8} sole {r.sole:>8} holds {r.holds:>8}  {text}")
        for sym, val in sorted(b.nearest.items()):
            if len(sym) > EXPLAIN_TERM_CHARS:
                sym = sym[:EXPLAIN_TERM_CHARS] + "..."
            lines.append(f"  nearest {sym} = {hex(val)}")
    return lines


def replay_dir(path: str, config=None, models_dir: Optional[str] = None,
               workers: Optional[int] = None, explain_dir: Optional[str] = None) -> ReplayReport:
    """Answer every ``*.smt2`` dump of directory ``path`` (see the module docstring).
    ``config``: a ``gpu_check.GpuConfig`` (budget, timeout, hints …), default
    ``gpu_check.CONFIG``; ``models_dir``: where to write the witness certificates;
    ``workers``: reader processes, never more than :func:`max_workers`; ``explain_dir``: where
    to write ``<name>.explain.txt`` for every dump left ``unknown`` (gpu_check.explain_sets: the
    conjuncts that block it) — the answers are what they are without it."""
    from . import engine as E
    from .smt import gpu_check

    cfg = config or replace(gpu_check.CONFIG)
    rep = ReplayReport()
    t_start = time.perf_counter()
    names = sorted(n for n in os.listdir(path) if n.endswith(".smt2"))
    paths = [os.path.join(path, n) for n in names]

    t0 = time.perf_counter()
    read = _read_all(paths, max_workers() if workers is None else workers)
    rep.phase_s["read"] = time.perf_counter() - t0

    t0 = time.perf_counter()
    live: List[FileResult] = []
    for name, (q, err, ms) in zip(names, read):
        fr = FileResult(name, ms=ms)
        rep.files.append(fr)
        if err is not None:
            fr.cls = f"error: {err}"
        elif not q.objective_free:
            fr.cls = "objective"
        else:
            t1 = time.perf_counter()
            fr.query = q
            fr.registry = smtlib.recover_registry(q.assertions, verify=False)
            fr.ms += (time.perf_counter() - t1) * 1e3
            live.append(fr)
    # every recovered pair of the directory against the real Keccak-256, in one batched call
    triples = sorted({(n, k, h) for fr in live for n, s in fr.registry.keccak.items()
                      for k, h in s.concrete.items()})
    if triples:
        good = dict(zip(triples, smtlib.verify_pairs(triples, E.get_engine())))
        for fr in live:
            smtlib.drop_unverified(fr.registry, lambda n, k, h: good[(n, k, h)])
    groups: Dict[tuple, List[FileResult]] = {}
    for fr in live:
        problems = fr.registry.recovery.problems(fr.registry)
        if problems:
            fr.cls = "error: " + "; ".join(problems)
        else:
            groups.setdefault(smtlib.registry_signature(fr.registry), []).append(fr)
    rep.phase_s["recover"] = time.perf_counter() - t0
    rep.groups = len(groups)

    for members in groups.values():
        reg = members[0].registry
        gpu_check.reset_cache()
        before = dict(gpu_check.STATS.phase_s)
        fails = sum(gpu_check.STATS.lowering_failures.values())
        t0 = time.perf_counter()
        models = gpu_check.check_sets([fr.query.assertions for fr in members], registry=reg, config=cfg)
        share = (time.perf_counter() - t0) * 1e3 / len(members)
        for k, v in gpu_check.STATS.phase_s.items():
            rep.phase_s[_CHECK_PHASE.get(k, "search")] += v - before.get(k, 0.0)
        refused = sum(gpu_check.STATS.lowering_failures.values()) > fails
        t0 = time.perf_counter()
        for fr, m in zip(members, models):
            t1 = time.perf_counter()
            if m is not None:
                # the file-level re-check: the witness under the assertions read from the file
                if all(m.w.ev(c) for c in fr.query.assertions):
                    fr.cls, fr.origin, fr.model = "sat", m.origin, m
                else:
                    rep.recheck_failures += 1
            elif refused:
                err = _lowering_error(fr.query.assertions, reg, cfg)
                if err is not None:
                    fr.cls = f"error: {err}"
            fr.ms += share + (time.perf_counter() - t1) * 1e3
        rep.phase_s["recheck"] += time.perf_counter() - t0
        left = [fr for fr in members if fr.cls == "unknown"]
        if explain_dir is not None and left:
            # after the group's answers are in: explain_sets records nothing, and the caches are
            # cleared before the next group anyway
            os.makedirs(explain_dir, exist_ok=True)
            exs = gpu_check.explain_sets([fr.query.assertions for fr in left], registry=reg, cfg=cfg)
            for fr, ex in zip(left, exs):
                with open(os.path.join(explain_dir, fr.name[:-len(".smt2")] + ".explain.txt"), "w") as f:
                    f.write("\n".join(explanation_lines(fr.name, ex)) + "\n")
    gpu_check.reset_cache()

    if models_dir is not None:
        os.makedirs(models_dir, exist_ok=True)
        for fr, p in zip(rep.files, paths):
            if fr.cls != "sat":
                continue
            out = os.path.join(models_dir, fr.name[:-len(".smt2")] + ".model.smt2")
            with open(p) as f:
                text = f.read()
            try:
                write_certificate(out, text, fr.query, fr.model)
                fr.certificate = out
            except ValueError as e:
                print(f"replay: no certificate for {fr.name}: {e}", file=sys.stderr)
    rep.wall_s = time.perf_counter() - t_start
    return rep


def _climb_arg(text: str) -> Tuple[int, Optional[int]]:
    """``ROUNDS`` or ``ROUNDS:CANDIDATES`` of ``--climb``."""
    import argparse

    head, _, tail = text.partition(":")
    try:
        rounds, cands = int(head), (int(tail) if tail else None)
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected ROUNDS[:CANDIDATES], got {text!r}")
    if rounds < 0 or (cands is not None and cands < 1):
        raise argparse.ArgumentTypeError(f"expected ROUNDS >= 0 and CANDIDATES >= 1, got {text!r}")
    return rounds, cands


def main(argv: Optional[List[str]] = None) -> int:
    import argparse

    from .smt import gpu_check

    ap = argparse.ArgumentParser(prog="python -m mythril_amd.replay",
                                 description="Answer a directory of --solver-log .smt2 dumps on the GPU.")
    ap.add_argument("dir")
    ap.add_argument("--out", metavar="FILE", help="write the JSON lines here instead of standard output")
    ap.add_argument("--budget", type=int, default=gpu_check.CONFIG.budget, help="candidates per bucket")
    ap.add_argument("--timeout-ms", type=int, default=gpu_check.CONFIG.timeout_ms)
    ap.add_argument("--models", metavar="DIR", help="write <name>.model.smt2 witness certificates here")
    ap.add_argument("--explain", metavar="DIR",
                    help="write <name>.explain.txt here for every dump that was not discharged: the conjuncts "
                         "that block it, by a census of the search's own candidates")
    ap.add_argument("--workers", type=int, default=None, help="reader processes (at most min(16, CPUs allowed))")
    ap.add_argument("--climb", metavar="ROUNDS[:CANDIDATES]", type=_climb_arg, default=None,
                    help="climb the buckets the search finds nothing for: ROUNDS scored rounds of CANDIDATES "
                         f"candidates (default {gpu_check.CONFIG.climb_candidates}); files answered that way "
                         "report the origin \"climb\"")
    ap.add_argument("--climb-score", choices=("sites", "tree"), default=None,
                    help=f"how the climb scores a candidate (default {gpu_check.CONFIG.climb_score}): distances "
                         "at fused compares only, or carried through the Boolean structure above them")
    args = ap.parse_args(argv)
    cfg = replace(gpu_check.CONFIG, budget=args.budget, timeout_ms=args.timeout_ms)
    if args.climb_score is not None:
        cfg = replace(cfg, climb_score=args.climb_score)
    if args.climb is not None:
        cfg = replace(cfg, climb_rounds=args.climb[0],
                      climb_candidates=args.climb[1] if args.climb[1] is not None else cfg.climb_candidates)
    # without the flag the call is what it was
    more = {"explain_dir": args.explain} if args.explain is not None else {}
    rep = replay_dir(args.dir, config=cfg, models_dir=args.models, workers=args.workers, **more)
    lines = rep.json_lines()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(lines[-1])
    else:
        print("\n".join(lines))
    return 0


if __name__ == "__main__":
    # run under the module's own name, so the reader processes import the same functions
    from mythril_amd.replay import main as _main

    sys.exit(_main())
