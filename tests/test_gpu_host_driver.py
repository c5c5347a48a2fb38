"""GPU: one batch driven through every entry point of the host driver in turn answers what a
batch created fresh for each call answers.  The entry points share one scratch (queue heads,
counter lines, t0), one pair of events and the found[] array, and each keeps a side block of its
own on the batch (climb, census, stream, link) behind the same acquire-or-grow code, so a call
must find nothing of the calls before it.

The batch: the members of two hand-made link groups of tests/link_sets.py, each group one member
on the 8-register and one on the 16-register file, every member with two assert sites.  Budgets
of 200 are 4 groups of 64 candidates with a partial last one."""

import dataclasses

import numpy as np
import pytest

import link_sets as LS
import pyoracle as O
import stream_model as M
from mythril_amd import ir
from mythril_amd.engine import NOT_FOUND

pytestmark = pytest.mark.gpu

SEED = LS.GSEED
EARLY = ir.FLAG_EARLY_EXIT
GROUP_OF = [0, 0, 1, 1]

# The link block of this batch (pf_check_linked: [group_of: 4 sets | parts: 2 groups | found: 2
# groups | count: records x 4 B | mask: records x 8 B], every region rounded up to 256 bytes,
# records = 2 groups x ceil(budget / 64)) is 5 x 256 = 1,280 bytes while the masks fit one region:
# up to 32 records, budgets up to 1,024.  At 200 it is 8 records in 1,280 bytes; at 4,096 it is
# 128 records, 768 + 512 + 1,024 = 2,304 bytes, so the second linked call replaces the block the
# first one acquired (unless the device pool handed the first call a larger one) and the third
# finds the larger block.
LINK_BUDGETS = (200, 4096, 200)


def programs():
    a = LS.make_group("driver-a", [LS.s_below(200), LS.s_from(50), LS.s_bit(2, 1), LS.mul_low(240)],
                      [[0, 1], [2, 3]], 0x901, wide={1})
    b = LS.make_group("driver-b", [LS.s_bit(0, 1), LS.b_is(True), LS.s_below(240), LS.p_is_parent()],
                      [[0, 1], [2, 3]], 0x902, wide={0})
    progs = a.members + b.members
    assert [M.is_wide(p) for p in progs] == [False, True, True, False]
    for p in progs:
        assert len(p.vars) >= 1 and sum(1 for ins in p.code if ins.op == ir.ASSERT) >= 2, p.name
    return progs


def candidates(batch, n):
    """n explicit candidates per set: the generator's own under the oracle."""
    return ir.pack_soa(batch, [O.SetView.from_batch(batch, s).gen_assignments(np.arange(n, dtype=np.uint64), SEED)
                               for s in range(len(batch.descs))])


def calls(engine, soa, witness):
    """(name, the call on a resident batch, whether its counters are a full sweep's and so the
    same on every run), in the order they are made on the one handle."""
    linked = [(f"check_linked {b} #{i}", lambda db, b=b: engine.check_linked(db, GROUP_OF, budget=b, seed=SEED, flags=EARLY),
               False) for i, b in enumerate(LINK_BUDGETS)]
    return [
        ("check", lambda db: engine.check(db, budget=200, seed=SEED, flags=EARLY), False),
        ("census [3,0]", lambda db: engine.census(db, [3, 0], budget=200, seed=SEED), True),
        ("climb [2,1,0]", lambda db: engine.climb(db, [2, 1, 0], 2, 128, seed=SEED), True),
        ("eval_batch [3,1]", lambda db: engine.eval_batch(db, soa, set_ids=[3, 1]), True),
        ("eval_batch [3,1] again", lambda db: engine.eval_batch(db, soa, set_ids=[3, 1]), True),   # no upload
        ("eval_batch [0,2,3]", lambda db: engine.eval_batch(db, soa, set_ids=[0, 2, 3]), True),
        *linked,
        ("materialize", lambda db: engine.materialize(db, [witness[0]], [witness[1]], seed=SEED), False),
        ("check again", lambda db: engine.check(db, budget=200, seed=SEED, flags=EARLY), False),
    ]


COUNTERS = ("evals_full", "cands_decided", "evals", "ops")


def same(a, b, counters):
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y, counters) for x, y in zip(a, b))
    if dataclasses.is_dataclass(a):
        return type(a) is type(b) and all(
            same(getattr(a, f.name), getattr(b, f.name), counters) for f in dataclasses.fields(a)
            if f.name != "kernel_ms" and (counters or f.name not in COUNTERS))
    return a == b


def test_one_batch_through_every_entry_point_equals_fresh_batches(engine):
    progs = programs()
    batch = ir.Batch(progs)
    soa = candidates(batch, 200)
    db = engine.upload(progs)
    try:
        # what the materialize call asks for: the first witness of the search itself
        probe = engine.upload(progs)
        found = engine.check(probe, budget=200, seed=SEED, flags=EARLY).found
        probe.free()
        hit = np.flatnonzero(found != NOT_FOUND)
        assert len(hit), "no set of the batch has a witness among 200 candidates"
        todo = calls(engine, soa, (int(hit[0]), int(found[hit[0]])))
        assert (engine.site_counts(db, range(4)) >= 2).all()
        got = [call(db) for _, call, _ in todo]
    finally:
        db.free()
    assert (got[0].found == found).all()
    for (name, call, full_sweep), g in zip(todo, got):
        fresh = engine.upload(progs)
        try:
            want = call(fresh)
        finally:
            fresh.free()
        print(name, g if not dataclasses.is_dataclass(g) else
              {f.name: getattr(g, f.name) for f in dataclasses.fields(g) if f.name in COUNTERS + ("found", "first", "status")})
        assert same(g, want, full_sweep), (name, g, want)
    # the calls did something: sets were climbed and censused, candidates streamed, groups decided
    assert len(got[1].holds) == 2 and len(got[2].status) == 3 and got[3].bits.shape == (2, 4)
    assert got[5].cands_decided == 3 * 200 and len(got[6].found) == 2 and len(got[9][0]) == len(progs[0].vars)
