"""The scaled Horner chain of pf::exp256_split (csrc/u256.h: the factor shifted once, the values
kept scaled by 2^c, shifts only where the scale outgrows a level's limbs) on the host, against
Python's pow(b, e, 2**256).

tools/exp_series_host.cpp is built at the configured split 8 and at splits whose schedule
un-scales at other levels and in its other forms: 10 and 11 (three un-scaling levels each, at
other depths), 16 (a level that only shifts its factor) and 84 (two levels, un-scaled at once);
8 itself has levels that shift both the inner value and the factor.  Per split (cases in
exp_scale_cases.py): n = (e >> M) at and around every un-scaling level and n = 2^246 - 1, under
bases whose t is all ones, 1 and random, e0 in {0, 255}; then 2,000 seeded random pairs.  The
same program is also built once with the address and undefined-behaviour sanitizers linked in
and run on a few hundred pairs.  CPU only."""
import os
import random
import subprocess

import exp_scale_cases as S
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "exp_series_host.cpp")
CLANG = "/opt/rocm/llvm/bin/clang++"
MOD = S.MOD

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="no host clang++")

SPLITS = [8, 10, 11, 16, 84]


def _check(exe, pairs):
    inp = "".join(f"{b:064x} {e:064x}\n" for b, e in pairs)
    p = subprocess.run([exe], input=inp, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])
    out = p.stdout.split()
    assert len(out) == len(pairs)
    bad = [(hex(b), hex(e), got, f"{pow(b, e, MOD):064x}")
           for (b, e), got in zip(pairs, out) if int(got, 16) != pow(b, e, MOD)]
    assert not bad, (len(bad), bad[:4])


def test_schedule_shapes():
    """The mirror of the header's schedule: where split 8 un-scales, that the other splits do
    so elsewhere and in every form, and that every chain ends unscaled."""
    assert S.unscaling_levels(8) == [1, 8, 15, 22]
    forms = set()
    for m in SPLITS:
        sched = S.schedule(m)
        assert sched[1][0] == 0 and all(0 <= c < 32 for c, _, _ in sched.values())
        forms |= {(un, sh) for _, un, sh in sched.values()}
        if m != 8:
            assert S.unscaling_levels(m) != S.unscaling_levels(8)
    assert forms == {(False, False), (True, False), (False, True), (True, True)}


def test_bases_have_the_t_they_claim():
    for m in SPLITS:
        ones, tiny = S.bases(m, random.Random(0), 0)
        assert (pow(ones, 1 << m, MOD) - 1) >> (m + 2) == (1 << (254 - m)) - 1
        assert (pow(tiny, 1 << m, MOD) - 1) >> (m + 2) == 1


@pytest.mark.parametrize("split", SPLITS)
def test_unscaling_levels_and_random_pairs(split, tmp_path):
    exe = os.path.join(str(tmp_path), f"exp_scale_host_{split}")
    subprocess.check_call([CLANG, "-O2", "-std=c++17", f"-DPF_EXP_SPLIT={split}", "-o", exe, SRC])
    _check(exe, S.pairs(split, nrandom_bases=6))
    rng = random.Random(0xE5CA1E + split)
    _check(exe, [(rng.getrandbits(256) | 1, rng.getrandbits(256)) for _ in range(2000)])


def test_under_sanitizers(tmp_path):
    """The sanitizers' runtimes are linked into the program itself: it runs as it is."""
    exe = os.path.join(str(tmp_path), "exp_scale_host_san")
    subprocess.check_call([CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, SRC])
    rng = random.Random(0x5A17)
    pairs = S.pairs(8, nrandom_bases=2)
    pairs += [(rng.getrandbits(256) | rng.getrandbits(1), rng.getrandbits(256)) for _ in range(300)]
    _check(exe, pairs)
