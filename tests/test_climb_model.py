"""CPU: the climb contract's model (tests/climb_model.py) checks itself, and the inputs the
GPU test relies on (tests/climb_sets.py) are what it takes them for: the plain search of
65,536 candidates finds nothing, the model's climb ends on a witness."""

import numpy as np
import pytest

import climb_model as CM
import climb_sets as CS
import coracle_py
import pyoracle as O
from mythril_amd import ir


@pytest.fixture(scope="module")
def near():
    batch = ir.Batch(CS.near_sets())
    return batch, CM.device_sets(batch)


@pytest.fixture(scope="module")
def near_climb(near):
    batch, devs = near
    return CM.climb(batch, range(len(batch)), CS.ROUNDS, CS.PER_ROUND, CS.SEED, devs=devs)


def test_round_seeds_differ_and_are_the_documented_function():
    seeds = [ir.climb_round_seed(CS.SEED, r) for r in range(64)]
    assert len(set(seeds + [CS.SEED])) == 65
    assert seeds[0] == (CS.SEED + 0x9E3779B97F4A7C15) % 2 ** 64
    assert ir.climb_round_seed(2 ** 64 - 1, 0) == 0x9E3779B97F4A7C14


def test_device_programs_fuse_the_compares(near):
    """The near sets' sites are what their builders say: fused compares (distance terms), or
    bool ops for the unfused set (512 or nothing)."""
    batch, devs = near
    by_name = {p.name: d for p, d in zip(batch.programs, devs)}
    fused = lambda d: [w0 & 0xFF for (w0, _, _, _) in d.code if w0 & CM.I_ASSERT]
    assert fused(by_name["bytes3"]) == [ir.B_EQ] * 3 and by_name["bytes3"].sites == 3
    assert fused(by_name["orderings"]) == [ir.B_ULT, ir.B_SLE, ir.B_SLT]
    assert fused(by_name["bytes3-unfused"]) == [ir.B_NOT] * 3
    assert by_name["bytes3-spill"].sites == 4
    ops = [w0 & 0xFF for (w0, _, _, _) in by_name["bytes3-spill"].code]
    assert ir.W_SPILL in ops and ir.W_FILL in ops


def test_score_is_512_per_site_exactly_on_witnesses(near):
    batch, devs = near
    rng = np.random.default_rng(5)
    for s, (prog, dev) in enumerate(zip(batch.programs, devs)):
        sv = O.SetView.from_batch(batch, s)
        sol = CS.X if prog.name.startswith("bytes3") else (((CS.X >> 1) & ~0xFFFF) + 17) ^ CS.K
        assert sv.evaluate([sol])
        assert dev.run([sol]) == (True, dev.target) and dev.target == 512 * dev.sites
        # the parent, its one-bit neighbours and random values: never the witness score
        others = [sv.parents[0]] + [sv.parents[0] ^ (1 << int(b)) for b in rng.integers(0, 256, 40)]
        others += [int.from_bytes(rng.bytes(32), "little") for _ in range(40)]
        for v in others:
            root, score = dev.run([v])
            assert root == sv.evaluate([v])
            assert (score == dev.target) == root and score <= dev.target


def test_distance_terms_on_hand_made_operands():
    # EQ: 256 - popcount(a ^ b)
    assert CM.near_term(ir.B_EQ, 0b1011, 0b0001) == 256 - 2
    assert CM.near_term(ir.B_EQ, 0, 2 ** 256 - 1) == 0
    # orderings: 256 - bitlen(|a - b|) on the unsigned register values, the signed ones too
    for op in (ir.B_ULT, ir.B_ULE, ir.B_SLT, ir.B_SLE):
        assert CM.near_term(op, 7, 7) == 256                    # a failing ULT / SLT of equals
        assert CM.near_term(op, 8, 7) == 255
        assert CM.near_term(op, 7 + 2 ** 100, 7) == 256 - 101
        assert CM.near_term(op, 2 ** 256 - 1, 0) == 0
        assert CM.near_term(op, 0, 2 ** 255) == 0               # "negative" b: still unsigned
    # any other failing site adds nothing
    assert CM.near_term(ir.B_UADD_NOOVF, 2 ** 256 - 1, 1) == 0
    assert CM.near_term(ir.B_NOT, 1, 0) == 0


def test_distance_terms_through_a_device_program(near):
    batch, devs = near
    dev = devs[[p.name for p in batch.programs].index("bytes3")]
    wrong = CS.X ^ (0b101 << CS.BYTES[1]) ^ (1 << CS.BYTES[2])
    assert dev.run([wrong]) == (False, 512 + (256 - 2) + (256 - 1))
    dev = devs[[p.name for p in batch.programs].index("orderings")]
    low = (CS.X >> 1) & ~0xFFFF
    t = low + 64 + (1 << 90)                                    # above the window
    assert dev.run([t ^ CS.K]) == (False, 512 + (256 - 91) + 512)
    t = low - (1 << 40)                                         # below it: ULT and SLT fail
    assert dev.run([t ^ CS.K]) == (False, 2 * (256 - 41) + 512)
    dev = devs[[p.name for p in batch.programs].index("bytes3-unfused")]
    assert dev.run([wrong]) == (False, 512)                     # bool sites: 512 or nothing


def test_tie_goes_to_the_smallest_index_and_index_0_is_left_out():
    assert CM.pick_best([3, 9, 9, 2, 9], 0) == 1
    assert CM.pick_best([9, 9, 3], 0) == 0
    assert CM.pick_best([9, 3, 7, 7], 1) == 2
    assert CM.pick_best([9], 1) is None


def _one_var_set():
    p = ir.Program(name="one")
    p.vars.append(ir.Var("x", 256))
    p.emit(ir.W_VAR, 256, dst=0, aux0=0)
    p.finish()
    batch = ir.Batch([p])
    return O.SetView.from_batch(batch, 0), CM.device_sets(batch)[0]


def test_sideways_moves_are_taken_and_worse_ones_are_not():
    sv, dev = _one_var_set()
    # a flat score: round 0 takes index 0, every later round index 1, each adopted (>=)
    r = CM.climb_set(sv, dev, 5, 64, 9, score_fn=lambda vals: 7)
    assert (r.score, r.round, r.index) == (7, 4, 1)
    a4 = r.values
    sv.parents = [CM.climb_set(sv, dev, 4, 64, 9, score_fn=lambda vals: 7).values[0]]
    assert a4 == sv.gen_assignments(np.array([1], dtype=np.uint64), ir.climb_round_seed(9, 4))[0]
    sv.parents = [None]
    # a score that peaks at round 0's candidate 0: whatever is adopted later is a copy of it
    # (the odd candidates that keep their parent), never one of the lower-scoring others
    first = sv.gen_assignments(np.arange(64, dtype=np.uint64), ir.climb_round_seed(9, 0))
    peak = first[0][0]
    r = CM.climb_set(sv, dev, 5, 64, 9, score_fn=lambda vals: 256 - bin(vals[0] ^ peak).count("1"))
    assert r.score == 256 and r.values == [peak]
    # ... and with one candidate per round there is nothing to move to after round 0
    r = CM.climb_set(sv, dev, 5, 1, 9, score_fn=lambda vals: 7)
    assert (r.score, r.round, r.index, r.values) == (7, 0, 0, [peak])


def test_round_0_uses_the_sets_own_parents_and_later_rounds_the_current_assignment(near):
    batch, devs = near
    sv = O.SetView.from_batch(batch, 0)
    own = sv.parents[0]
    r = CM.climb_set(sv, devs[0], 1, 8, CS.SEED)
    # candidate 0 of round 0 is the set's parent; with 8 candidates nothing scores higher
    assert r.round == 0 and r.values == [own] and sv.parents == [own]


def test_the_plain_search_misses_the_near_sets(near):
    batch, _ = near
    packed = coracle_py.Packed(batch)
    for s in range(len(batch)):
        assert packed.first_sat(s, CS.SEED, 65536) is None, batch.programs[s].name


def test_the_models_climb_reaches_the_near_sets(near, near_climb):
    batch, devs = near
    for s, r in enumerate(near_climb):
        name = batch.programs[s].name
        assert r.status == ir.CLIMB_WITNESS and r.score == devs[s].target, name
        assert 1 <= r.round < CS.ROUNDS, name                    # not by round 0's plain candidates
        assert O.SetView.from_batch(batch, s).evaluate(r.values), name


def test_trivial_sets_are_witnesses_in_round_0():
    batch = ir.Batch([CS.bare_end(), CS.no_vars(), CS.no_vars(False), CS.flat()])
    got = CM.climb(batch, range(4), 3, 100, 1)
    assert [(r.status, r.score, r.round) for r in got[:2]] == [(ir.CLIMB_WITNESS, 0, 0), (ir.CLIMB_WITNESS, 512, 0)]
    assert (got[2].status, got[2].score, got[2].round, got[2].values) == (ir.CLIMB_NONE, 254, 2, [])
    assert (got[3].status, got[3].score, got[3].round, got[3].index) == (ir.CLIMB_NONE, 254, 2, 1)
