"""Host-side driver of the batched path-feasibility engine (one process per GPU).

This is the layer the SMT facade (mythril_amd.smt.solver) and the LASER plugin call.  It
replaces the two CPU paths of the reference's query funnel with one GPU batch:

* ``ModelCache.check_quick_sat`` — evaluate the conjunction under candidate models
  (mythril/support/support_utils.py:57-71), here 65,536 generated candidates per set
  instead of <= 100 cached z3 models;
* the objective-free ``Optimize.check`` (mythril/support/model.py:37-59, :99-125) whenever a
  witness is found; sets without a witness are left to z3 unchanged (soundness).
"""

from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from .ir import CLIMB_SCORE_SITES, CLIMB_WITNESS, FLAG_SHORTCIRCUIT, LIMBS, Batch, Program, climb_score_id, from_limbs

NOT_FOUND = 0xFFFFFFFF


@dataclass
class CheckResult:
    found: np.ndarray        # [n_sets] uint32 smallest witness index or NOT_FOUND
    evals_full: int
    cands_decided: int
    ops: int
    kernel_ms: float
    timed_out: bool = False   # the device deadline cut the search: NOT_FOUND is incomplete

    @property
    def sat(self) -> np.ndarray:
        return self.found != NOT_FOUND


@dataclass
class ClimbResult:
    """Engine.climb: one entry per requested set, in request order."""
    status: np.ndarray       # uint32 ir.CLIMB_NONE / CLIMB_WITNESS / CLIMB_CUT
    score: np.ndarray        # uint32 score of the final assignment
    round: np.ndarray        # uint32 the round that generated it
    values: list             # per set: its final assignment as limb rows [n_vars, 8] uint32
    evals: int = 0           # candidate evaluations over all rounds
    kernel_ms: float = 0.0
    timed_out: bool = False

    @property
    def sat(self) -> np.ndarray:
        return self.status == CLIMB_WITNESS


@dataclass
class CensusResult:
    """Engine.census: one entry per requested set, in request order (include/pf_bytecode.h,
    census contract)."""
    holds: list              # per set: uint32 [n_sites] candidates at which the site holds
    alive: list              # per set: uint32 [n_sites] candidates at which sites 0..j all hold
    sole: list               # per set: uint32 [n_sites] candidates whose only failing site is j
    best_fails: np.ndarray   # uint32 the fewest failing sites of any candidate
    best_cand: np.ndarray    # uint32 the smallest candidate index with so few
    status: np.ndarray       # uint32 ir.CENSUS_DONE / CENSUS_CUT
    evals: int = 0
    kernel_ms: float = 0.0
    timed_out: bool = False

    @property
    def sat(self) -> np.ndarray:
        return self.best_fails == 0


@dataclass
class StreamResult:
    """Engine.eval_batch / eval_stream: one row per requested set, in request order
    (include/pf_bytecode.h, stream contract).  eval_batch fills numpy arrays; eval_stream leaves
    device tensors (bits as int64 words, first and count as int32 — reinterpret the bit patterns)
    and no timing."""
    bits: object             # [n, ceil(n_cand / 64)] uint64: bit c & 63 of word c >> 6 = candidate c
    first: object            # [n] uint32 smallest satisfying candidate, or NOT_FOUND
    count: object            # [n] uint32 satisfying candidates
    n_cand: int
    kernel_ms: float = 0.0
    evals_full: int = 0
    cands_decided: int = 0
    n_sat: int = 0

    def verdicts(self) -> np.ndarray:
        """bits unpacked: bool [n, n_cand]."""
        bits = self.bits
        if not isinstance(bits, np.ndarray):     # a device tensor
            bits = bits.cpu().numpy()
        return unpack_bits(bits, self.n_cand)


def unpack_bits(bits: np.ndarray, n_cand: int) -> np.ndarray:
    """Verdict words [n, ceil(n_cand / 64)] (uint64, or the same bit patterns as int64) ->
    bool [n, n_cand]."""
    words = np.ascontiguousarray(bits).view(np.uint64).reshape(len(bits), -1)
    if words.shape[1] != (n_cand + 63) // 64:
        raise ValueError(f"{words.shape[1]} words per set for {n_cand} candidates")
    by = words.astype("<u8", copy=False).view(np.uint8).reshape(len(words), -1)
    return np.unpackbits(by, axis=1, bitorder="little")[:, :n_cand].astype(bool)


class DeviceBatch:
    """A :class:`~mythril_amd.ir.Batch` resident in one device's HBM (pf_batch_create_on)."""

    def __init__(self, batch: Batch, device: int = -1):
        L = _lib.lib()
        self.batch = batch
        self.device = device
        h = ctypes.c_uint64(0)
        descs = np.ascontiguousarray(batch.descs, dtype=np.uint32)
        code = np.ascontiguousarray(batch.code, dtype=np.uint32)
        consts = np.ascontiguousarray(batch.consts, dtype=np.uint32)
        schema = np.ascontiguousarray(batch.schema, dtype=np.uint32)
        parents = np.ascontiguousarray(batch.parents, dtype=np.uint32)
        _lib.check(L.pf_batch_create_on(
            device,
            _lib.ptr_u32(code.reshape(-1)) if code.size else None, code.shape[0],
            _lib.ptr_u32(consts.reshape(-1)) if consts.size else None, consts.shape[0],
            _lib.ptr_u32(schema.reshape(-1)) if schema.size else None, schema.shape[0],
            _lib.ptr_u32(parents.reshape(-1)) if parents.size else None, parents.shape[0],
            _lib.ptr_u32(descs.reshape(-1)) if descs.size else None, descs.shape[0],
            ctypes.byref(h)), "pf_batch_create_on")
        self.handle = h.value

    def __len__(self):
        return len(self.batch)

    def free(self):
        if self.handle:
            _lib.lib().pf_batch_free(self.handle)
            self.handle = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Engine:
    """The per-process engine: one GPU (one process per GPU) or several GPUs driven by one
    process (``devices``), one library stream per device."""

    def __init__(self, device: int = 0, devices: Optional[Sequence[int]] = None):
        self.devices = list(devices) if devices is not None else [device]
        if len(set(self.devices)) < len(self.devices):
            # a device named twice: one execution context (own stream) per entry, so the
            # node split (upload_sharded + check_many) runs its multi-device path on one GPU
            self.devices = _lib.init_contexts(self.devices)
        else:
            _lib.init(self.devices)
        self.device = self.devices[0]

    # ---- search -------------------------------------------------------------------
    def upload(self, programs: Sequence[Program] | Batch, device: Optional[int] = None) -> DeviceBatch:
        batch = programs if isinstance(programs, Batch) else Batch(programs)
        return DeviceBatch(batch, self.device if device is None else device)

    def check(self, db: DeviceBatch, budget: int = 65536, seed: int = 0, flags: int = 2,
              timeout_ms: int = 0) -> CheckResult:
        n = len(db)
        found = np.full(max(n, 1), NOT_FOUND, dtype=np.uint32)
        st = _lib.pf_stats()
        _lib.check(_lib.lib().pf_check_batch(db.handle, seed, budget, flags, timeout_ms,
                                            _lib.ptr_u32(found), None, ctypes.byref(st)),
                   "pf_check_batch")
        return CheckResult(found[:n], st.evals_full, st.cands_decided, st.ops, st.kernel_ms,
                           bool(st.timed_out))

    def check_linked(self, db: DeviceBatch, group_of: Sequence[int], budget: int = 65536, seed: int = 0,
                     flags: int = 2, timeout_ms: int = 0) -> CheckResult:
        """Linked search (pf_check_linked; include/pf_bytecode.h, link contract): ``group_of[s]``
        is set s's link group, ``found[g]`` of the result the smallest candidate at which every
        member of group g holds.  The members of a group share schema, constants, parents and
        seed (lower_parts makes them so), hence ``materialize`` of any member at the verdict is
        the group's assignment."""
        ids = np.ascontiguousarray([int(g) & 0xFFFFFFFF for g in group_of], dtype=np.uint32)
        if len(ids) != len(db):
            raise _lib.PathFeasError(f"check_linked: {len(ids)} group ids for {len(db)} sets")
        n_groups = int(ids.max()) + 1 if len(ids) else 0
        found = np.full(max(n_groups, 1), NOT_FOUND, dtype=np.uint32)
        st = _lib.pf_stats()
        _lib.check(_lib.lib().pf_check_linked(db.handle, seed, budget, flags, timeout_ms,
                                             _lib.ptr_u32(ids) if len(ids) else None, n_groups,
                                             _lib.ptr_u32(found), ctypes.byref(st)), "pf_check_linked")
        return CheckResult(found[:n_groups], st.evals_full, st.cands_decided, st.ops, st.kernel_ms,
                           bool(st.timed_out))

    def upload_sharded(self, programs: Sequence[Program], group_of: Optional[Sequence[int]] = None):
        """Size-balanced contiguous shards, one per device (mythril_amd.dist.shard_bounds
        over the bytecode cost model), each uploaded to its device.  With ``group_of`` — the
        programs' link groups, each group's members adjacent — the cuts fall between groups, so a
        group's members stay on one device, and the result is (batches, per batch its members'
        groups renumbered from 0) for check_linked."""
        from .dist import shard_bounds

        progs = list(programs)
        nd = len(self.devices)
        if group_of is None:
            if nd == 1 or len(progs) < 2:
                return [self.upload(progs)]
            out = []
            for (lo, hi), d in zip(shard_bounds([p.sched_cost() for p in progs], nd), self.devices):
                if hi > lo:
                    out.append(self.upload(progs[lo:hi], device=d))
            return out
        gids = [int(g) for g in group_of]
        if len(gids) != len(progs):
            raise _lib.PathFeasError(f"upload_sharded: {len(gids)} group ids for {len(progs)} programs")
        runs = []      # [first program, end) of every group, in order
        for i, g in enumerate(gids):
            if runs and gids[runs[-1][0]] == g:
                runs[-1][1] = i + 1
            else:
                runs.append([i, i + 1])
        if len({gids[lo] for lo, _ in runs}) != len(runs):
            raise _lib.PathFeasError("upload_sharded: a link group's members must be adjacent")
        costs = [sum(p.sched_cost() for p in progs[lo:hi]) for lo, hi in runs]
        bounds = [(0, len(runs))] if nd == 1 or len(runs) < 2 else shard_bounds(costs, nd)
        dbs, local = [], []
        for (lo, hi), d in zip(bounds, self.devices):
            if hi <= lo:
                continue
            p0, p1 = runs[lo][0], runs[hi - 1][1]
            dbs.append(self.upload(progs[p0:p1], device=d))
            renum = {gids[runs[r][0]]: r - lo for r in range(lo, hi)}
            local.append([renum[g] for g in gids[p0:p1]])
        return dbs, local

    def check_many(self, dbs: Sequence[DeviceBatch], budget: int = 65536, seed: int = 0,
                   flags: int = 2, timeout_ms: int = 0) -> CheckResult:
        """One search over several device batches at once (pf_check_batches: every device
        launches before any result is read); verdicts concatenated in batch order, the
        kernel time is the slowest device's."""
        if len(dbs) == 1:
            return self.check(dbs[0], budget, seed, flags, timeout_ms)
        n = sum(len(db) for db in dbs)
        found = np.full(max(n, 1), NOT_FOUND, dtype=np.uint32)
        stats = (_lib.pf_stats * len(dbs))()
        handles = np.array([db.handle for db in dbs], dtype=np.uint64)
        _lib.check(_lib.lib().pf_check_batches(_lib.ptr_u64(handles), len(dbs), seed, budget, flags,
                                              timeout_ms, _lib.ptr_u32(found), stats),
                   "pf_check_batches")
        return CheckResult(found[:n], sum(s.evals_full for s in stats),
                           sum(s.cands_decided for s in stats), sum(s.ops for s in stats),
                           max(s.kernel_ms for s in stats), any(s.timed_out for s in stats))

    def check_each(self, dbs: Sequence[DeviceBatch], budget: int = 65536, seed: int = 0,
                   flags: int = 2, timeout_ms: int = 0) -> List[CheckResult]:
        """check() of every batch, all enqueued before any result is read (pf_check_batches):
        batches on one device run back to back on its stream, with no host round trip
        between them (a stream of independent batches, e.g. bench steps)."""
        if not dbs:
            return []
        n = sum(len(db) for db in dbs)
        found = np.full(max(n, 1), NOT_FOUND, dtype=np.uint32)
        stats = (_lib.pf_stats * len(dbs))()
        handles = np.array([db.handle for db in dbs], dtype=np.uint64)
        _lib.check(_lib.lib().pf_check_batches(_lib.ptr_u64(handles), len(dbs), seed, budget, flags,
                                              timeout_ms, _lib.ptr_u32(found), stats),
                   "pf_check_batches")
        out, off = [], 0
        for db, s in zip(dbs, stats):
            out.append(CheckResult(found[off:off + len(db)].copy(), s.evals_full, s.cands_decided,
                                   s.ops, s.kernel_ms, bool(s.timed_out)))
            off += len(db)
        return out

    def materialize(self, db: DeviceBatch, set_ids: Sequence[int], cand_ids: Sequence[int],
                    seed: int = 0) -> List[List[int]]:
        """Concrete variable values of the given (set, candidate) pairs."""
        set_ids = np.ascontiguousarray(set_ids, dtype=np.uint32)
        cand_ids = np.ascontiguousarray(cand_ids, dtype=np.uint32)
        nv = [int(db.batch.descs[s][5]) for s in set_ids]
        total = sum(nv)
        out = np.zeros(max(total, 1) * LIMBS, dtype=np.uint32)
        if len(set_ids):
            _lib.check(_lib.lib().pf_materialize(db.handle, seed, _lib.ptr_u32(set_ids),
                                                _lib.ptr_u32(cand_ids), len(set_ids),
                                                _lib.ptr_u32(out)), "pf_materialize")
        res, off = [], 0
        rows = out.reshape(-1, LIMBS)
        for k in nv:
            res.append([from_limbs(rows[off + i]) for i in range(k)])
            off += k
        return res

    def climb(self, db, set_ids: Sequence[int], rounds: int, per_round: int, seed: int = 0,
              timeout_ms: int = 0, score="sites") -> ClimbResult:
        """Climb the given sets (pf_climb_batch; include/pf_bytecode.h, climb contract):
        ``rounds`` scored searches of ``per_round`` candidates, each round's best near miss
        the parent model of the next.  ``db`` is one DeviceBatch, or the list upload_sharded
        returned — ``set_ids`` then index the concatenation of its batches, as check_many's
        verdicts do, and every set is climbed on the batch that holds it.  ``score``: "sites"
        (pf_climb_batch) or "tree" (pf_climb_batch_scored, the tree score)."""
        score_id = climb_score_id(score)
        dbs = list(db) if isinstance(db, (list, tuple)) else [db]
        ids = [int(s) for s in set_ids]
        n = len(ids)
        status = np.zeros(n, dtype=np.uint32)
        score = np.zeros(n, dtype=np.uint32)
        rnd = np.zeros(n, dtype=np.uint32)
        values: List[Optional[np.ndarray]] = [None] * n
        total = sum(len(d) for d in dbs)
        if len(dbs) > 1:   # one batch: pf_climb_batch checks its own ids; several: none may fall through
            for s in ids:
                if not 0 <= s < total:
                    raise _lib.PathFeasError(f"climb: set {s} out of range ({total} sets)")
        evals = 0
        ms = 0.0
        cut = False
        base = 0
        for d in dbs:
            mine = list(range(n)) if len(dbs) == 1 else [i for i, s in enumerate(ids) if base <= s < base + len(d)]
            if mine or len(dbs) == 1:
                local = np.array([(ids[i] - base) & 0xFFFFFFFF for i in mine], dtype=np.uint32)
                nv = [int(d.batch.descs[s][5]) if s < len(d) else 0 for s in local]
                st_, sc_, rd_ = (np.zeros(max(len(mine), 1), dtype=np.uint32) for _ in range(3))
                vals = np.zeros(max(sum(nv), 1) * LIMBS, dtype=np.uint32)
                st = _lib.pf_stats()
                tail = (_lib.ptr_u32(local) if len(mine) else None, len(mine), _lib.ptr_u32(st_),
                        _lib.ptr_u32(sc_), _lib.ptr_u32(rd_), _lib.ptr_u32(vals), ctypes.byref(st))
                if score_id == CLIMB_SCORE_SITES:
                    _lib.check(_lib.lib().pf_climb_batch(d.handle, seed, rounds, per_round, timeout_ms, *tail),
                               "pf_climb_batch")
                else:
                    _lib.check(_lib.lib().pf_climb_batch_scored(d.handle, seed, rounds, per_round, score_id,
                                                                timeout_ms, *tail), "pf_climb_batch_scored")
                rows, off = vals.reshape(-1, LIMBS), 0
                for j, i in enumerate(mine):
                    status[i], score[i], rnd[i] = st_[j], sc_[j], rd_[j]
                    values[i] = rows[off:off + nv[j]].copy()
                    off += nv[j]
                evals += st.cands_decided
                ms += st.kernel_ms
                cut = cut or bool(st.timed_out)
            base += len(d)
        return ClimbResult(status, score, rnd, values, evals, ms, cut)

    def site_counts(self, db: DeviceBatch, set_ids: Sequence[int]) -> np.ndarray:
        """The assert sites of the given sets' device programs (pf_batch_site_counts)."""
        ids = np.ascontiguousarray(set_ids, dtype=np.uint32)
        out = np.zeros(max(len(ids), 1), dtype=np.uint32)
        if len(ids):
            _lib.check(_lib.lib().pf_batch_site_counts(db.handle, _lib.ptr_u32(ids), len(ids), _lib.ptr_u32(out)),
                       "pf_batch_site_counts")
        return out[:len(ids)]

    def census(self, db: DeviceBatch, set_ids: Sequence[int], budget: int = 65536, seed: int = 0,
               timeout_ms: int = 0) -> CensusResult:
        """What blocks the given sets (pf_census_batch; include/pf_bytecode.h, census contract):
        per assert site of the device program, how many of the plain search's candidates
        [0, budget) under ``seed`` hold there, are still alive there, and fail there alone — and
        the nearest miss.  A diagnostic call: nothing the search or the climb reads changes."""
        ids = np.ascontiguousarray([int(s) & 0xFFFFFFFF for s in set_ids], dtype=np.uint32)
        n = len(ids)
        # an id out of range is pf_census_batch's error: count its row as empty here
        known = [int(s) for s in ids if s < len(db)]
        cnt = dict(zip(known, self.site_counts(db, known).tolist())) if known else {}
        ks = [cnt.get(int(s), 0) for s in ids]
        total = sum(ks)
        rows = [np.zeros(max(total, 1), dtype=np.uint32) for _ in range(3)]
        bf, bc, status = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3))
        st = _lib.pf_stats()
        _lib.check(_lib.lib().pf_census_batch(db.handle, seed, budget, timeout_ms,
                                             _lib.ptr_u32(ids) if n else None, n, *(_lib.ptr_u32(r) for r in rows),
                                             _lib.ptr_u32(bf), _lib.ptr_u32(bc), _lib.ptr_u32(status),
                                             ctypes.byref(st)), "pf_census_batch")
        cols = [[], [], []]
        off = 0
        for k in ks:
            for c, r in zip(cols, rows):
                c.append(r[off:off + k].copy())
            off += k
        return CensusResult(cols[0], cols[1], cols[2], bf[:n], bc[:n], status[:n], st.cands_decided,
                            st.kernel_ms, bool(st.timed_out))

    def materialize_limbs(self, db: DeviceBatch, set_ids: Sequence[int], cand_ids: Sequence[int],
                          seed: int = 0) -> np.ndarray:
        """materialize() as limbs: the variables of every (set, candidate) pair back to back,
        one row of 8 little-endian u32 each (rows = sum of the sets' variable counts)."""
        set_ids = np.ascontiguousarray(set_ids, dtype=np.uint32)
        cand_ids = np.ascontiguousarray(cand_ids, dtype=np.uint32)
        total = int(db.batch.descs[set_ids, 5].sum()) if len(set_ids) else 0
        out = np.zeros(max(total, 1) * LIMBS, dtype=np.uint32)
        if len(set_ids):
            _lib.check(_lib.lib().pf_materialize(db.handle, seed, _lib.ptr_u32(set_ids),
                                                _lib.ptr_u32(cand_ids), len(set_ids),
                                                _lib.ptr_u32(out)), "pf_materialize")
        return out[:total * LIMBS].reshape(total, LIMBS)

    def eval_assignments(self, db: DeviceBatch, set_id: int, soa: np.ndarray) -> np.ndarray:
        """SAT flag of each explicit candidate; soa is [var][limb][cand] uint32."""
        soa = np.ascontiguousarray(soa, dtype=np.uint32)
        n_cand = soa.shape[-1]
        out = np.zeros(max(n_cand, 1), dtype=np.uint8)
        _lib.check(_lib.lib().pf_eval_assignments(db.handle, set_id, _lib.ptr_u32(soa.reshape(-1)),
                                                 n_cand, _lib.ptr_u8(out)), "pf_eval_assignments")
        return out[:n_cand].astype(bool)

    def eval_program(self, program: Program, soa: np.ndarray) -> np.ndarray:
        """SAT flag of each explicit candidate of one program, in one call (pf_eval_program:
        no batch object; the GPU-resident ModelCache's launch).  The packed arrays are kept
        on the program, so a second launch over it packs nothing."""
        pk = getattr(program, "_eval_pack", None)
        if pk is None:
            b = Batch([program])
            pk = (np.ascontiguousarray(b.code, dtype=np.uint32).reshape(-1),
                  np.ascontiguousarray(b.consts, dtype=np.uint32).reshape(-1),
                  np.ascontiguousarray(b.schema, dtype=np.uint32).reshape(-1))
            program._eval_pack = pk
        code, consts, schema = pk
        soa = np.ascontiguousarray(soa, dtype=np.uint32)
        n_cand = soa.shape[-1]
        out = np.zeros(max(n_cand, 1), dtype=np.uint8)
        z = np.zeros(8, dtype=np.uint32)
        _lib.check(_lib.lib().pf_eval_program(
            self.device, _lib.ptr_u32(code), code.size // 4,
            _lib.ptr_u32(consts if consts.size else z), consts.size // 8,
            _lib.ptr_u32(schema if schema.size else z), schema.size // 4,
            _lib.ptr_u32(soa.reshape(-1)), n_cand, _lib.ptr_u8(out)), "pf_eval_program")
        return out[:n_cand].astype(bool)

    def eval_programs(self, pack, soa: np.ndarray) -> np.ndarray:
        """SAT flags [program][candidate] of several programs over one call's explicit
        candidates (pf_eval_programs: one launch, a wave per program and 64 candidates).
        ``pack`` = the flat (code, consts, schema, descs) u32 arrays of an ir.Batch over the
        programs; ``soa`` = [var][limb][cand] over all programs' variables, program after
        program (their descriptors' var_off)."""
        code, consts, schema, descs = pack
        n_sets = descs.size // 8
        soa = np.ascontiguousarray(soa, dtype=np.uint32)
        n_cand = soa.shape[-1]
        out = np.zeros(max(n_sets * n_cand, 1), dtype=np.uint8)
        z = np.zeros(8, dtype=np.uint32)
        _lib.check(_lib.lib().pf_eval_programs(
            self.device, _lib.ptr_u32(code), code.size // 4,
            _lib.ptr_u32(consts if consts.size else z), consts.size // 8,
            _lib.ptr_u32(schema if schema.size else z), schema.size // 4,
            _lib.ptr_u32(descs), n_sets,
            _lib.ptr_u32(soa.reshape(-1) if soa.size else z), n_cand, _lib.ptr_u8(out)), "pf_eval_programs")
        return out[:n_sets * n_cand].reshape(n_sets, n_cand).astype(bool)

    # ---- stream: explicit candidates through every set of a batch ---------------------------
    @staticmethod
    def _stream_request(db: DeviceBatch, shape, set_ids) -> np.ndarray:
        """The request's set ids, after the checks the kernels cannot make: the SoA is
        [V][8][n_cand] over the batch's V variables."""
        n_vars = int(db.batch.schema.shape[0])
        if len(shape) != 3 or shape[1] != LIMBS:
            raise _lib.PathFeasError(f"stream: assignments of shape {tuple(shape)}, expected [V][{LIMBS}][n_cand]")
        if shape[0] != n_vars:
            raise _lib.PathFeasError(f"stream: {shape[0]} variable rows, the batch has {n_vars} "
                                     "(ir.pack_soa lays them out)")
        if shape[2] >= 1 << 32:
            raise _lib.PathFeasError(f"stream: {shape[2]} candidates (at most 2^32 - 1)")
        ids = range(len(db)) if set_ids is None else [int(s) & 0xFFFFFFFF for s in set_ids]
        return np.ascontiguousarray(ids, dtype=np.uint32)

    def eval_batch(self, db: DeviceBatch, soa: np.ndarray, set_ids: Optional[Sequence[int]] = None,
                   shortcircuit: bool = True) -> StreamResult:
        """Every explicit candidate of ``soa`` ([V][8][n_cand] uint32 over the batch's variables,
        ir.pack_soa) against every requested set (default: all) in one call — pf_eval_batch;
        include/pf_bytecode.h, stream contract."""
        soa = np.asarray(soa)
        if soa.dtype != np.uint32:
            raise _lib.PathFeasError(f"stream: assignments of dtype {soa.dtype}, expected uint32")
        ids = self._stream_request(db, soa.shape, set_ids)
        soa = np.ascontiguousarray(soa)
        n, n_cand = len(ids), int(soa.shape[2])
        words = (n_cand + 63) // 64
        bits = np.zeros((n, words), dtype=np.uint64)
        first = np.full(n, NOT_FOUND, dtype=np.uint32)
        count = np.zeros(n, dtype=np.uint32)
        st = _lib.pf_stats()
        _lib.check(_lib.lib().pf_eval_batch(
            db.handle, _lib.ptr_u32(ids) if n else None, n, _lib.ptr_u32(soa.reshape(-1)) if soa.size else None,
            n_cand, FLAG_SHORTCIRCUIT if shortcircuit else 0, _lib.ptr_u64(bits.reshape(-1)) if bits.size else None,
            _lib.ptr_u32(first) if n else None, _lib.ptr_u32(count) if n else None, ctypes.byref(st)),
            "pf_eval_batch")
        return StreamResult(bits, first, count, n_cand, st.kernel_ms, st.evals_full, st.cands_decided, st.n_sat)

    def eval_stream(self, db: DeviceBatch, soa_tensor, set_ids: Optional[Sequence[int]] = None, out=None,
                    stream=None, shortcircuit: bool = True) -> StreamResult:
        """eval_batch on device-resident candidates — pf_eval_batch_dev: ``soa_tensor`` is a
        contiguous int32 / uint32 torch tensor [V][8][n_cand] on the batch's device, read through
        its data_ptr() with no copy.  ``out``: a (bits, first, count) triple of device tensors to
        write (int64 [n, words], int32 [n], int32 [n]; any of them None for "not wanted", not
        all), default: new ones.  ``stream``: a torch stream (default: the current one).  Nothing
        here waits for the device, except the first call with a given request: results are
        ordered on the stream, which the caller synchronises."""
        import torch

        if not isinstance(soa_tensor, torch.Tensor) or not soa_tensor.is_cuda:
            raise _lib.PathFeasError("stream: eval_stream takes a tensor on the GPU (eval_batch takes numpy)")
        if soa_tensor.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
            raise _lib.PathFeasError(f"stream: assignments of dtype {soa_tensor.dtype}, expected int32 / uint32")
        if not soa_tensor.is_contiguous():
            raise _lib.PathFeasError("stream: the assignments tensor is not contiguous")
        ids = self._stream_request(db, tuple(soa_tensor.shape), set_ids)
        n, n_cand = len(ids), int(soa_tensor.shape[2])
        words = (n_cand + 63) // 64
        dev = soa_tensor.device
        if out is None:
            out = (torch.empty((n, words), dtype=torch.int64, device=dev),
                   torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
        bits, first, count = out
        for t, shape, dt, what in ((bits, (n, words), torch.int64, "bits"), (first, (n,), torch.int32, "first"),
                                   (count, (n,), torch.int32, "count")):
            if t is None:
                continue
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != dev:
                raise _lib.PathFeasError(f"stream: out {what} must be a contiguous {dt} tensor of shape {shape} "
                                         f"on {dev}")
        s = torch.cuda.current_stream(dev) if stream is None else stream
        ptrs = [t.data_ptr() if t is not None else None for t in (bits, first, count)]
        _lib.check(_lib.lib().pf_eval_batch_dev(
            db.handle, _lib.ptr_u32(ids) if n else None, n, soa_tensor.data_ptr(), n_cand,
            FLAG_SHORTCIRCUIT if shortcircuit else 0, *ptrs, None, s.cuda_stream), "pf_eval_batch_dev")
        return StreamResult(bits, first, count, n_cand)

    # ---- keccak -------------------------------------------------------------------
    def keccak256(self, messages: Sequence[bytes]) -> List[bytes]:
        n = len(messages)
        if n == 0:
            return []
        offsets = np.zeros(n + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(m) for m in messages], dtype=np.uint64)
        data = np.frombuffer(b"".join(messages) or b"\0", dtype=np.uint8).copy()
        out = np.zeros(32 * n, dtype=np.uint8)
        _lib.check(_lib.lib().pf_keccak256_batch(_lib.ptr_u8(data), _lib.ptr_u64(offsets), n,
                                                _lib.ptr_u8(out)), "pf_keccak256_batch")
        return [out[32 * i:32 * i + 32].tobytes() for i in range(n)]


_engine: Optional[Engine] = None


def get_engine(device: Optional[int] = None) -> Engine:
    """The process's engine.  Device selection: an explicit ``device``; else ``PF_DEVICES``
    (comma-separated indices, or ``all``: one process driving every visible GPU — the live
    analysis, which Mythril runs as one process; an index named twice, e.g. ``0,0``, makes two
    execution contexts on that GPU); else ``LOCAL_RANK`` (one process per GPU)."""
    global _engine
    if _engine is None:
        import os
        if device is not None:
            _engine = Engine(device)
        else:
            spec = os.environ.get("PF_DEVICES", "").strip()
            if spec == "all":
                _engine = Engine(devices=list(range(_lib.lib().pf_device_count())))
            elif spec:
                _engine = Engine(devices=[int(x) for x in spec.split(",")])
            else:
                _engine = Engine(int(os.environ.get("LOCAL_RANK", "0")))
    return _engine
