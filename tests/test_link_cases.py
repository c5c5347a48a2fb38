"""CPU: the link contract's model (tests/link_model.py), lower_parts in both lowerings, and
check_sets with the link knob on an oracle-backed engine (LinkOracleEngine).

The hand-made groups of tests/link_sets.py are checked here for what the GPU test relies on; the
corpus buckets show that the parts of a bucket partition its roots, carry the unsplit program's
schema, constants, parents and seed, hold together exactly where the unsplit program holds, and
are the same arrays whether the Python or the native term pipeline made the DAG."""


import numpy as np
import pytest

import coracle_py
import link_model as LM
import link_sets as LS
import oracle_engine
from mythril_amd import corpus, ir, seed
from mythril_amd.engine import NOT_FOUND
from mythril_amd.lower import Dag, LoweringError, lower, lower_parts, part_bounds
from mythril_amd.smt import gpu_check
from mythril_amd.smt import native_terms as NT
from mythril_amd.smt.independence import buckets
from mythril_amd.smt.to_dag import TermLowering


# ---- the hand-made groups ------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    L = LS.big_layout()
    return L, ir.Batch(L.programs)


def test_target_groups_have_their_witness_where_they_were_built_for(big):
    L, batch = big
    packed = coracle_py.Packed(batch)
    for budget in LS.BUDGETS:
        found = LM.check_linked(batch, L.group_of, budget, LS.GSEED, packed)
        by_name = {g.name: (int(found[u]), int(found[p])) for g, u, p in zip(L.groups, L.unsplit_gid, L.parts_gid)}
        for k in LS.KS:
            for t in LS.TARGETS:
                want = t if t < budget else NOT_FOUND
                assert by_name[f"target{t}/k{k}"] == (want, want), (budget, k, t)
        assert all(u == p for u, p in by_name.values())
        assert by_name["nowhere"][1] == NOT_FOUND and by_name["all-bare"][1] == 0


def test_members_hold_where_their_group_does_not(big):
    """The premise of the early-exit rule: below a group's verdict some member holds at a
    candidate, in many groups, so a member's own hit must not end its item."""
    L, batch = big
    packed = coracle_py.Packed(batch)
    found = LM.check_linked(batch, L.group_of, 4096, LS.GSEED, packed)
    early = 0
    for g, p in zip(L.groups, L.parts_gid):
        v = int(found[p])
        sets = L.sets_of(p)
        if len(sets) < 2 or v == 0:
            continue
        upto = 4096 if v == NOT_FOUND else v
        early += any(packed.eval_generated(s, LS.GSEED, 0, upto).any() for s in sets)
    assert early >= 8


def test_layouts_are_what_the_gpu_test_says(big):
    L, batch = big
    assert max(len(p.code) for p in L.programs) <= 100 and L.n_groups == 72
    wide = [max((i.dst for i in p.code if i.op in (ir.W_VAR, ir.W_CONST)), default=0) >= ir.NW_NARROW for p in L.programs]
    mixed = 0
    for p in L.parts_gid:
        files = {wide[s] for s in L.sets_of(p)}
        mixed += len(files) == 2
    assert mixed >= 3
    B = LS.bands_layout()
    assert B.n_groups == 64 and {len(B.sets_of(g)) for g in range(B.n_groups)} >= {1, 2, 3, 4, 7}
    # the members of a group are not adjacent sets
    assert any(np.diff(B.sets_of(g)).max() > 1 for g in B.parts_gid)
    S = LS.small_layout()
    assert 2 <= len(S.programs) < 16 and all(p.has_parent for p in S.programs)


def test_model_refuses_what_the_contract_refuses(big):
    L, batch = big
    with pytest.raises(ValueError):
        LM.check_linked(batch, L.group_of, 0)
    with pytest.raises(ValueError):
        LM.check_linked(batch, [g + 1 for g in L.group_of], 64)       # group 0 is empty
    a, b = L.sets_of(L.parts_gid[0])[0], L.sets_of(L.parts_gid[1])[0]
    mixed = list(range(len(L.programs)))
    mixed[b] = mixed[a]
    ids = sorted(set(mixed))
    with pytest.raises(ValueError):
        LM.check_linked(batch, [ids.index(g) for g in mixed], 64)     # other seed, other constants


# ---- lower_parts ---------------------------------------------------------------------------
def test_part_bounds():
    assert part_bounds([1] * 10, 3) == [(0, 4), (4, 7), (7, 10)]
    assert part_bounds([100, 1, 1, 1], 4) == [(0, 1), (1, 4)]
    assert part_bounds([1, 1, 1, 100], 4) == [(0, 4)]
    assert part_bounds([5], 3) == [(0, 1)]
    assert part_bounds([1, 1, 1, 1], 7) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    for costs in ([3, 9, 2, 2, 7, 1], [0, 0, 0], [4] * 33):
        for n in (1, 2, 5, 64):
            b = part_bounds(costs, n)
            assert 1 <= len(b) <= n and b[0][0] == 0 and b[-1][1] == len(costs)
            assert all(lo < hi for lo, hi in b) and all(x[1] == y[0] for x, y in zip(b, b[1:]))


@pytest.fixture(scope="module")
def corpus_buckets():
    import mythril_amd.engine as E

    eng = oracle_engine.OracleEngine()
    saved = E.get_engine
    E.get_engine = lambda device=None: eng   # the corpus hashes concrete keccaks (host oracle)
    try:
        c = corpus.build(6, 2, seed=11)
    finally:
        E.get_engine = saved
    out, seen = [], set()
    for q in c.queries:
        for b in buckets(q.constraints):
            if tuple(b) not in seen:
                seen.add(tuple(b))
                out.append(b)
    return c, out


def assert_parts(dag, whole, parts, n_parts, gseed=5):
    """What lower_parts promises, on one DAG."""
    assert 1 <= len(parts) <= n_parts
    if len(parts) == 1 and parts[0] is whole:
        return
    spans = [p.link_roots for p in parts]
    assert spans[0][0] == 0 and spans[-1][1] == len(dag.roots)
    assert all(lo < hi for lo, hi in spans) and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    for p, (lo, hi) in zip(parts, spans):
        n_assert = sum(1 for i in p.code if i.op == ir.ASSERT)
        assert n_assert == hi - lo
    b = ir.Batch([whole] + list(parts))
    d0 = b.descs[0]
    nc, nv = int(d0[3]), int(d0[5])
    for s in range(1, len(b)):
        d = b.descs[s]
        assert int(d[3]) == nc and int(d[5]) == nv and int(d[6]) == int(d0[6])
        assert np.array_equal(b.consts[int(d[2]):int(d[2]) + nc], b.consts[int(d0[2]):int(d0[2]) + nc])
    assert LM.shared_error(b, list(range(len(b)))) == ""
    packed = coracle_py.Packed(b)
    both = LM.group_masks(packed, range(1, len(b)), 256, gseed)
    assert np.array_equal(both, packed.eval_generated(0, gseed, 0, 256))
    return b


def test_corpus_parts_in_both_lowerings(corpus_buckets):
    c, bks = corpus_buckets
    reg = c.kfm.registry
    split = lowered = 0
    for n, b in enumerate(bks):
        try:
            lo = TermLowering(reg, None).lower(b)
        except LoweringError:
            continue
        seed.apply_hints(lo.dag)
        whole = lower(lo.dag, seed=7 + n)
        k = (2, 3, 8, 16)[n % 4]
        parts = lower_parts(lo.dag, k, 7 + n, "b", whole)
        lowered += 1
        split += len(parts) > 1
        b1 = assert_parts(lo.dag, whole, parts, k)
        if NT.store() is not None and b1 is not None:
            _, w2, p2 = NT.lower_parts(b, reg, None, True, 7 + n, k)
            b2 = ir.Batch([w2] + p2)
            for name in ("code", "consts", "schema", "parents", "descs"):
                assert np.array_equal(getattr(b1, name), getattr(b2, name)), name
    assert lowered > 0.9 * len(bks) and split > 0.5 * lowered


def test_hand_built_dags():
    d = Dag()
    x = d.var("x", 256, parent=12345)
    y = d.var("y", 8)
    flag = d.var("f", 1, kind=ir.VK_BOOL)
    shared = d.op(ir.W_ADD, 256, x, d.const(77, 256))
    for i in range(6):
        e = d.op(ir.W_EXTRACT, 8, shared, aux=8 * i)
        d.assert_(d.op(ir.B_ULT, 8, e, d.const(200 - i, 8)))
    d.assert_(d.op(ir.B_OR, 1, flag, d.op(ir.B_EQ, 8, y, d.const(3, 8))))
    d.assert_(d.op(ir.B_ULE, 256, d.op(ir.W_MUL, 256, shared, shared), d.const(1 << 255, 256)))
    whole = lower(d, seed=3, name="hand")
    for k in (1, 2, 3, 8, 64):
        parts = lower_parts(d, k, 3, "hand", whole)
        assert_parts(d, whole, parts, k)
        assert all(p.vars == whole.vars and p.seed == whole.seed for p in parts)
    # the shared subterm is emitted again in every part that needs it
    parts = lower_parts(d, 8, 3, "hand", whole)
    assert sum(1 for p in parts for i in p.code if i.op == ir.W_ADD) > sum(1 for i in whole.code if i.op == ir.W_ADD)
    # one root, no root
    one = Dag()
    one.assert_(one.op(ir.B_EQ, 8, one.var("z", 8), one.const(1, 8)))
    assert len(lower_parts(one, 4, 1)) == 1
    assert len(lower_parts(Dag(), 4, 1)) == 1
    with pytest.raises(ValueError):
        lower_parts(d, 0, 3)
    with pytest.raises(ValueError):
        lower_parts(d, ir.LINK_MAX_PARTS + 1, 3)


# ---- check_sets with the knob --------------------------------------------------------------
def _install(monkeypatch):
    import mythril_amd.engine as E

    eng = LM.LinkOracleEngine()
    monkeypatch.setattr(E, "get_engine", lambda device=None: eng)
    monkeypatch.setattr(gpu_check.CONFIG, "workers", 1)
    monkeypatch.setattr(gpu_check.CONFIG, "budget", 1024)
    gpu_check.reset_cache()
    return eng


def _run(corpus_, cfg_link, monkeypatch):
    eng = _install(monkeypatch)
    monkeypatch.setattr(gpu_check.CONFIG, "link_min_ins", cfg_link[0])
    monkeypatch.setattr(gpu_check.CONFIG, "link_parts", cfg_link[1])
    sets = [q.constraints for q in corpus_.queries]
    models = []
    for i in range(0, len(sets), 16):
        models += gpu_check.check_sets(sets[i:i + 16], corpus_.kfm.registry)
    cache = {k: (None if v is None else [int(x) for x in gpu_check._values(v[1])]) for k, v in gpu_check._CACHE.items()}
    neg = set(gpu_check._NEG)
    return eng, models, cache, neg


def test_check_sets_answers_the_same_with_the_knob(corpus_buckets, monkeypatch):
    c, bks = corpus_buckets
    min_ins, k = 60, 4
    # the condition: at least a quarter of the corpus's buckets split at this setting
    reg = c.kfm.registry
    n_split = n_all = 0
    for b in bks:
        try:
            _, prog = gpu_check._lower_bucket(b, reg, None, True, (min_ins, k))
        except (LoweringError, ValueError):
            continue
        n_all += 1
        n_split += len(getattr(prog, "link_parts", None) or ()) > 1
    assert 4 * n_split >= n_all, (n_split, n_all)

    eng0, models0, cache0, neg0 = _run(c, (0, k), monkeypatch)
    assert eng0.linked_calls == [] and eng0.launches > 0          # the knob at 0: no linked call
    eng1, models1, cache1, neg1 = _run(c, (min_ins, k), monkeypatch)
    assert eng1.linked_calls and any(len(set(g)) < len(g) for g, *_ in eng1.linked_calls)
    assert [m is None for m in models0] == [m is None for m in models1]
    assert sum(m is not None for m in models0) > 0
    assert cache0 == cache1 and neg0 == neg1
    for a, b in zip(models0, models1):
        if a is not None:
            assert _witness_of(a) == _witness_of(b)


def _witness_of(m):
    """The bucket witnesses behind a model: per bucket its variables' values, and the origin."""
    return [[int(x) for x in gpu_check._values(p[1])] for p in m.parts], m.origin
