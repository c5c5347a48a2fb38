"""CPU, host only: pf_device_sites — which PF_ASSERT of the lowered program every assert site of
the device program stands for — against ordinals recomputed here from pf_device_batch's output
and the lowered program: a site and its assert have the same value under every assignment, and an
assert without a site is one the fold pass proved (it holds under every assignment).  With the
fold on, off (PF_DEVICE_FOLD=0) and alone (2), over the census fixtures, one of which loses its
first assert to the fold."""

import random

import census_model as M
import census_sets as CS
import climb_model as CM
from mythril_amd import _lib, ir

N_ASSIGN = 48


def lowered_set(batch, s):
    """Set s as lowered, readable by the device-program interpreter: the write-back bit of every
    W result set (pf_batch_create stamps it; the lowering packs none)."""
    d = batch.descs[s].tolist()
    rows = []
    for r in batch.code[d[0]:d[0] + d[1]]:
        w0, w1, a0, a1 = (int(x) for x in r)
        op = w0 & 0xFF
        if ir.W_CONST <= op <= ir.W_FILL and op != ir.W_SPILL:
            w0 |= CM.TR_WW
        rows.append((w0, w1, a0, a1))
    consts = [ir.from_limbs(c) for c in batch.consts[d[2]:d[2] + d[3]]]
    return CM.DeviceSet(rows, consts)


def assignments(prog, rng):
    out = []
    for _ in range(N_ASSIGN):
        out.append([rng.choice((0, 1, rng.getrandbits(v.width), ir.mask(v.width), 0x5A, 0x11, 70, 150, 250))
                    & ir.mask(v.width) for v in prog.vars])
    return out


def recomputed(batch, progs):
    """Per set: for every device site the lowered asserts that agree with it on every sampled
    assignment, and the set of lowered asserts that hold on all of them."""
    devs = CM.device_sets(batch)
    rng = random.Random(7)
    out = []
    for s, p in enumerate(progs):
        low = lowered_set(batch, s)
        assert len(M.site_indices(low)) == sum(1 for i in p.code if i.op == ir.ASSERT)
        asg = assignments(p, rng)
        lv = list(zip(*[M.site_values(low, a) for a in asg])) if M.site_indices(low) else []
        dv = list(zip(*[M.site_values(devs[s], a) for a in asg])) if devs[s].sites else []
        match = [[k for k, col in enumerate(lv) if col == site] for site in dv]
        out.append((match, {k for k, col in enumerate(lv) if all(col)}, len(lv)))
    return out


def check(progs, expect_fold):
    batch = ir.Batch(progs)
    got = _lib.device_sites(batch.code, batch.consts, batch.descs)
    want = recomputed(batch, progs)
    assert len(got) == len(progs)
    for p, g, (match, always, n_low) in zip(progs, got, want):
        g = g.tolist()
        assert len(g) == len(match), p.name
        assert len(set(g)) == len(g) and all(k < n_low for k in g), p.name
        for j, k in enumerate(g):
            assert k in match[j], (p.name, j, k, match[j])
        # an assert without a site was proved by the fold pass
        assert set(range(n_low)) - set(g) <= always, p.name
        if not expect_fold:
            assert sorted(g) == list(range(n_low)), p.name
    return {p.name: g.tolist() for p, g in zip(progs, got)}


def test_fold_on(monkeypatch):
    monkeypatch.delenv("PF_DEVICE_FOLD", raising=False)
    by = check(CS.big_batch(), True)
    assert by["folded-first"] == [1, 3]          # its first assert folds away, and its third
    assert by["folded-away"] == [] and by["bare-end"] == []
    assert by["many-sites"] == list(range(33))   # (the second of that name)
    assert by["spilled-bool-exp"] == [0, 1, 3]
    assert sorted(by["plain-sites"]) == [0, 1, 2, 3, 4]
    # below the gate nothing is folded, whatever the switch says
    small = check(CS.small_batch(), False)
    assert small["folded-away"] == [0]


def test_fold_off(monkeypatch):
    monkeypatch.setenv("PF_DEVICE_FOLD", "0")
    by = check(CS.big_batch(), False)
    assert by["folded-first"] == [0, 1, 2, 3]


def test_fold_alone(monkeypatch):
    """PF_DEVICE_FOLD=2: no peephole runs, so every site is a plain PF_ASSERT."""
    monkeypatch.setenv("PF_DEVICE_FOLD", "2")
    progs = CS.big_batch()
    by = check(progs, True)
    assert by["folded-first"] == [1, 3]
    batch = ir.Batch(progs)
    for d in CM.device_sets(batch):
        assert not any(w0 & CM.I_ASSERT for (w0, _, _, _) in d.code)


def test_matches_the_batch_site_counts_contract():
    """The map's length per set is n_sites of the census contract (DeviceSet.sites)."""
    batch = ir.Batch(CS.big_batch())
    assert [len(g) for g in _lib.device_sites(batch.code, batch.consts, batch.descs)] == \
        [d.sites for d in CM.device_sets(batch)]
