"""CPU: the census contract's model (tests/census_model.py) against the C oracle, on the fixture
sets of tests/census_sets.py — and the fixtures themselves: that they are not degenerate is
asserted here, so that the device comparison (test_gpu_census.py) cannot pass on zeros."""

import pytest

import census_model as M
import census_sets as CS
import climb_model as CM
import coracle_py
from mythril_amd import _lib, ir

BUDGET = CS.BUDGETS[0]


@pytest.fixture(scope="module", params=["big", "small"])
def case(request):
    progs = CS.big_batch() if request.param == "big" else CS.small_batch()
    batch = ir.Batch(progs)
    devs = CM.device_sets(batch)
    got = M.census(batch, range(len(progs)), BUDGET, CS.SEED, devs)
    return request.param, progs, batch, devs, got


def test_model_agrees_with_the_oracle(case):
    _, progs, batch, devs, got = case
    packed = coracle_py.Packed(batch)
    for s, (p, r) in enumerate(zip(progs, got)):
        sat = packed.eval_generated(s, CS.SEED, 0, BUDGET)
        first = packed.first_sat(s, CS.SEED, BUDGET)
        n = devs[s].sites
        assert len(r.holds) == len(r.alive) == len(r.sole) == n, p.name
        if n:
            assert r.alive[-1] == int(sat.sum()), p.name
        else:   # no site: every candidate is a witness
            assert sat.all() and (r.best_fails, r.best_cand) == (0, 0), p.name
        assert (r.best_fails == 0) == (first is not None), p.name
        if first is not None:
            assert r.best_cand == first, p.name
        assert all(h >= a for h, a in zip(r.holds, r.alive)), p.name
        assert all(a >= b for a, b in zip(r.alive, r.alive[1:])), p.name
        assert all(h <= BUDGET for h in r.holds) and sum(r.sole) <= BUDGET, p.name
        assert 0 <= r.best_cand < BUDGET and r.best_fails <= n, p.name


def test_fixtures_are_not_degenerate(case):
    which, progs, _, devs, got = case
    if which != "big":
        assert [d.sites for d in devs] == [2, 1, 3]        # not folded: x ^ x == 0 keeps its site
        return
    assert len(progs) >= 16                                  # folded, constants of its own
    by = {}
    for p, d, r in zip(progs, devs, got):
        by.setdefault(p.name, (d, r))
    assert any(r.best_fails == 0 for _, r in by.values())
    assert any(r.best_fails >= 2 for _, r in by.values())
    assert sum(1 for _, r in by.values() for x in r.sole if x > 0) >= 2
    assert by["bare-end"][0].sites == 0 and by["folded-away"][0].sites == 0
    assert len(by["folded-away"][0].code) == 1 and by["ground-true"][0].sites == 1
    assert by["one-site"][0].sites == 1 and by["many-sites"][0].sites > 32
    assert by["contra"][1].best_fails == 2
    # sites of every kind: plain PF_ASSERTs next to fused ones, in one set
    code = by["plain-sites"][0].code
    assert any((w0 & 0xFF) == ir.ASSERT for (w0, _, _, _) in code)
    assert any(w0 & CM.I_ASSERT for (w0, _, _, _) in code)
    # the Bool spill survives on the device, in scratch and (without the EXP) maybe in LDS
    for name in ("spilled-bool", "spilled-bool-exp", "spilled-bool-exp-b8"):
        ops = [w0 & 0xFF for (w0, _, _, _) in by[name][0].code]
        assert ir.B_SPILL in ops and ir.B_FILL in ops, name
    # rows that differ from site to site, so an offset error shows
    r = by["many-sites"][1]
    assert len(set(r.holds)) > 8 and len(set(r.alive)) > 4 and r.alive[0] > r.alive[-1]
    # candidate 0 of the parented set is one site away
    assert by["parented"][1].best_fails <= 1


def test_a_second_seed_gives_other_counts():
    progs = CS.small_batch()
    batch = ir.Batch(progs)
    a = M.census(batch, [0], BUDGET, CS.SEED)[0]
    b = M.census(batch, [0], BUDGET, CS.SEED2)[0]
    assert (a.holds, a.alive, a.sole) != (b.holds, b.alive, b.sole)


def test_site_counts_are_the_device_programs():
    """DeviceSet.sites, the model's site list and pf_device_sites count the same sites."""
    batch = ir.Batch(CS.big_batch())
    devs = CM.device_sets(batch)
    sites = _lib.device_sites(batch.code, batch.consts, batch.descs)
    assert [len(M.site_indices(d)) for d in devs] == [d.sites for d in devs] == [len(s) for s in sites]
