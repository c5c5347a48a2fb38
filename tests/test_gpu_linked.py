"""GPU: pf_check_linked (Engine.check_linked) returns what the link contract's CPU model
(tests/link_model.py, the committed C oracle) returns, exactly, and what Engine.check returns for
the unsplit program of every group in the same batch — on the hand-made groups of
tests/link_sets.py, whose premises (where each target group's witness lies, that members hold
where their group does not) tests/test_link_cases.py asserts on the CPU.  Programs have at most
36 instructions, batches at most 147 sets, budgets at most 4,096."""

import ctypes

import numpy as np
import pytest

import coracle_py
import link_model as LM
import link_sets as LS
from mythril_amd import _lib, ir
from mythril_amd.engine import NOT_FOUND

pytestmark = pytest.mark.gpu

FLAG_SETS = (0, ir.FLAG_SHORTCIRCUIT, ir.FLAG_EARLY_EXIT, ir.FLAG_EARLY_EXIT | ir.FLAG_SHORTCIRCUIT)


class Resident:
    def __init__(self, engine, layout):
        self.layout = layout
        self.db = engine.upload(layout.programs)
        self.packed = coracle_py.Packed(self.db.batch)
        self._want = {}

    def want(self, budget, seed=LS.GSEED):
        """The model's verdicts, computed once per (budget, seed) and never changed."""
        key = (budget, seed)
        if key not in self._want:
            w = LM.check_linked(self.db.batch, self.layout.group_of, budget, seed, self.packed)
            w.setflags(write=False)
            self._want[key] = w
        return self._want[key]


@pytest.fixture(scope="module")
def big(engine):
    r = Resident(engine, LS.big_layout())
    yield r
    r.db.free()


@pytest.fixture(scope="module")
def bands(engine):
    r = Resident(engine, LS.bands_layout())
    yield r
    r.db.free()


@pytest.fixture(scope="module")
def small(engine):
    r = Resident(engine, LS.small_layout())
    yield r
    r.db.free()


def assert_call(engine, r, budget, flags, seed=LS.GSEED):
    L = r.layout
    got = engine.check_linked(r.db, L.group_of, budget=budget, seed=seed, flags=flags)
    plain = engine.check(r.db, budget=budget, seed=seed, flags=flags)
    want = r.want(budget, seed)
    assert not got.timed_out and len(got.found) == L.n_groups
    for g, u, p, s in zip(L.groups, L.unsplit_gid, L.parts_gid, L.unsplit_set):
        assert int(got.found[p]) == int(want[p]), (g.name, "parts against the model")
        assert int(got.found[u]) == int(want[u]), (g.name, "group of one against the model")
        assert int(got.found[p]) == int(plain.found[s]), (g.name, "parts against check() of the unsplit program")
        assert int(got.found[u]) == int(plain.found[s]), (g.name, "group of one against check()")
    return got


@pytest.mark.parametrize("flags", FLAG_SETS)
@pytest.mark.parametrize("budget", LS.BUDGETS)
def test_targets_and_special_members(engine, big, budget, flags):
    """K = 1, 2, 3, 7 with the witness at candidate 0, 62, 63, 64, 196, 4095 — every budget's last
    candidate — or past the budget; a member that holds nowhere, a bare END as lowered and as
    folded, the 8- and the 16-register file in one group; 72 groups, their sets interleaved."""
    got = assert_call(engine, big, budget, flags)
    L = big.layout
    by_name = {g.name: int(got.found[p]) for g, p in zip(L.groups, L.parts_gid)}
    for k in LS.KS:
        for t in LS.TARGETS:
            assert by_name[f"target{t}/k{k}"] == (t if t < budget else NOT_FOUND)
    assert by_name["nowhere"] == NOT_FOUND and by_name["all-bare"] == 0 and by_name["folded"] == 0
    if not flags & ir.FLAG_EARLY_EXIT and not flags & ir.FLAG_SHORTCIRCUIT:
        # a full sweep without short-circuit runs every lane of every member, or skips a whole
        # group of 64 that an earlier member failed
        assert got.cands_decided <= budget * len(L.programs) and got.evals_full == got.cands_decided


@pytest.mark.parametrize("flags", FLAG_SETS)
@pytest.mark.parametrize("budget", (197, 4096))
def test_64_groups_of_mixed_k(engine, bands, budget, flags):
    """64 link groups of 1, 2, 3, 4 and 7 members that each hold at many candidates and together
    at few, members of both register files: the queue interleaves the groups."""
    assert bands.layout.n_groups == 64
    assert_call(engine, bands, budget, flags)


@pytest.mark.parametrize("flags", FLAG_SETS + (ir.FLAG_EARLY_EXIT | ir.FLAG_NO_PROBE, ir.FLAG_COUNT_OPS))
def test_small_unfolded_batch_with_and_without_the_probe(engine, small, flags):
    """7 sets: below the fold gate, and — every set parented — within the probe launch's bounds."""
    for budget in (64, 65, 4096):
        got = assert_call(engine, small, budget, flags)
        assert (got.ops > 0) == bool(flags & ir.FLAG_COUNT_OPS)


def test_second_call_with_a_smaller_budget_and_another_grouping(engine, big):
    """The link block is reset by every call and re-sized: a smaller budget after a larger one
    (fewer records per group), a larger one again, other seeds, and every set a group of its own
    (more groups than before)."""
    L = big.layout
    assert_call(engine, big, 4096, ir.FLAG_EARLY_EXIT)
    assert_call(engine, big, 65, ir.FLAG_EARLY_EXIT)
    assert_call(engine, big, 65, 0)
    assert_call(engine, big, 4096, 0, seed=LS.GSEED + 1)
    assert_call(engine, big, 197, ir.FLAG_EARLY_EXIT)
    alone = list(range(len(L.programs)))
    got = engine.check_linked(big.db, alone, budget=197, seed=LS.GSEED, flags=ir.FLAG_EARLY_EXIT)
    plain = engine.check(big.db, budget=197, seed=LS.GSEED, flags=ir.FLAG_EARLY_EXIT)
    assert (got.found == plain.found).all()
    assert_call(engine, big, 4096, ir.FLAG_EARLY_EXIT)


def test_plain_search_is_unchanged_around_a_linked_call(engine, big, small):
    for r in (big, small):
        L = r.layout
        before = engine.check(r.db, budget=4096, seed=LS.GSEED, flags=ir.FLAG_EARLY_EXIT)
        full0 = engine.check(r.db, budget=256, seed=LS.GSEED, flags=0)
        engine.check_linked(r.db, L.group_of, budget=197, seed=LS.GSEED + 5, flags=0)
        after = engine.check(r.db, budget=4096, seed=LS.GSEED, flags=ir.FLAG_EARLY_EXIT)
        full1 = engine.check(r.db, budget=256, seed=LS.GSEED, flags=0)
        assert (before.found == after.found).all()
        assert (full0.found == full1.found).all() and full0.evals_full == full1.evals_full
        # the plain verdicts are per set: the members' own, not their groups'
        assert len(after.found) == len(L.programs)


def test_materialize_of_two_members_gives_equal_rows(engine, bands):
    L = bands.layout
    got = engine.check_linked(bands.db, L.group_of, budget=4096, seed=LS.GSEED, flags=ir.FLAG_EARLY_EXIT)
    seen = 0
    for g, p in zip(L.groups, L.parts_gid):
        c = int(got.found[p])
        sets = L.sets_of(p)
        if c == NOT_FOUND or len(sets) < 2:
            continue
        rows = engine.materialize(bands.db, sets, [c] * len(sets), seed=LS.GSEED)
        assert all(r == rows[0] for r in rows[1:]), g.name
        assert rows[0] == engine.materialize(bands.db, [L.unsplit_set[L.groups.index(g)]], [c], seed=LS.GSEED)[0]
        seen += 1
    assert seen >= 16


def raw_call(db, group_of, n_groups, budget, n_out):
    ids = np.ascontiguousarray(group_of, dtype=np.uint32)
    out = np.full(n_out, 0xA5A5A5A5, dtype=np.uint32)
    st = _lib.pf_stats()
    rc = _lib.lib().pf_check_linked(db.handle, LS.GSEED, budget, ir.FLAG_EARLY_EXIT, 0, _lib.ptr_u32(ids), n_groups,
                                    _lib.ptr_u32(out), ctypes.byref(st))
    return rc, out


def test_errors_launch_nothing_and_write_nothing(engine, small):
    L = small.layout
    n = len(L.programs)
    ok = list(L.group_of)

    def refused(group_of, n_groups, budget=64):
        rc, out = raw_call(small.db, group_of, n_groups, budget, max(n_groups, n) + 2)
        assert rc != 0 and (out == 0xA5A5A5A5).all()
        assert _lib.lib().pf_last_error()

    refused([L.n_groups] + ok[1:], L.n_groups)                 # an id out of range
    refused(ok, L.n_groups + 1)                                # an empty group
    refused(ok, L.n_groups, budget=0)                          # no budget
    # members that differ: sets of the two hand-made groups (other seeds) in one group
    a, b = L.sets_of(L.parts_gid[0])[0], L.sets_of(L.parts_gid[1])[0]
    mixed = list(range(n))
    mixed[b] = mixed[a]
    refused([sorted(set(mixed)).index(g) for g in mixed], n - 1)
    with pytest.raises(_lib.PathFeasError):
        engine.check_linked(small.db, ok[:-1], budget=64)
    # and the batch still answers
    rc, out = raw_call(small.db, ok, L.n_groups, 64, L.n_groups)
    assert rc == 0 and (out == small.want(64)).all()


def differing(field):
    """Two bare-END programs over one variable that differ in one thing the contract names."""
    progs = []
    for k in range(2):
        p = ir.Program(name=f"differs-{field}-{k}")
        width = 16 if (field == "schema" and k) else 8
        parent = {"parent": (7, 9)[k], "parent-absent": (7, None)[k]}.get(field, 7)
        p.vars.append(ir.Var("v", width, ir.VK_GENERIC, 0, 0, parent))
        p.consts = [3, 5 if (field == "const" and k) else 4]
        if field == "n_const" and k:
            p.consts.append(6)
        if field == "n_vars" and k:
            p.vars.append(ir.Var("u", 8))
        p.seed = 2 if (field == "seed" and k) else 1
        progs.append(p.finish())
    return progs


@pytest.mark.parametrize("field", ("same", "schema", "parent", "parent-absent", "const", "n_const", "n_vars", "seed"))
def test_members_must_share_what_the_contract_names(engine, field):
    db = engine.upload(differing(field))
    try:
        rc, out = raw_call(db, [0, 0], 1, 64, 2)
        if field == "same":
            assert rc == 0 and int(out[0]) == 0 and int(out[1]) == 0xA5A5A5A5
        else:
            assert rc != 0 and (out == 0xA5A5A5A5).all()
        rc, out = raw_call(db, [0, 1], 2, 64, 2)     # groups of one share nothing
        assert rc == 0 and (out == 0).all()
    finally:
        db.free()


def test_group_size_limit(engine):
    progs = [ir.Program(name=f"end{k}", seed=1).finish() for k in range(ir.LINK_MAX_PARTS + 1)]
    db = engine.upload(progs)
    try:
        rc, out = raw_call(db, [0] * len(progs), 1, 64, 1)
        assert rc != 0 and int(out[0]) == 0xA5A5A5A5
        rc, out = raw_call(db, [0] * ir.LINK_MAX_PARTS + [1], 2, 64, 2)
        assert rc == 0 and (out == 0).all()
    finally:
        db.free()
