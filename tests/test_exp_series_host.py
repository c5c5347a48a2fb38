"""The division-free Horner chain of pf::exp256_split (csrc/u256.h) on the host, against Python's
pow(b, e, 2**256).  A stand-alone program (tools/exp_series_host.cpp, PF_HOST_MAC) prints
exp256_split(b, e) for the pairs given; the pairs are the shapes at which the chain can go
wrong, not random bulk:

* e = e0 + 256 n for n = 0..30: the binomials C(n, j) vanish for j > n, so the sum stops at level
  n and every level's constant K_i (and the innermost operand c) is exercised as the last one
  that matters; e0 in {0, 1, 255} puts nothing, one digit and every digit in the windowed part;
* n = 2^k for every k, n = 2^246 - 1, and exponents with bits 254 / 255 set (which must not
  matter for odd bases: the unit group mod 2^256 has exponent 2^254);
* odd bases 1, 3, 5, 7, 2^k +- 1 (t = (b^2 - 1) / 8 tiny, zero, all ones), 2^256 - 1 and random;
* even bases with e < 256 and e >= 256 (the series does not run: 0 or the windowed part).

Each host case is a one-lane wave.  The constants are computed in the header at compile time
(no generated table), so the program is also built with another split, for which the header
must derive another set.  CPU only."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "exp_series_host.cpp")
CLANG = "/opt/rocm/llvm/bin/clang++"
MOD = 1 << 256
MASK = MOD - 1

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="no host clang++")


def _exe(tmp, split):
    exe = os.path.join(str(tmp), f"exp_series_host_{split}")
    subprocess.check_call([CLANG, "-O2", "-std=c++17", f"-DPF_EXP_SPLIT={split}", "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _exe(tmp_path_factory.mktemp("exp_series"), 8)


def _check(exe, pairs):
    inp = "".join(f"{b:064x} {e:064x}\n" for b, e in pairs)
    out = subprocess.run([exe], input=inp, capture_output=True, text=True, check=True, timeout=300).stdout.split()
    assert len(out) == len(pairs)
    bad = [(hex(b), hex(e), got, f"{pow(b, e, MOD):064x}")
           for (b, e), got in zip(pairs, out) if int(got, 16) != pow(b, e, MOD)]
    assert not bad, (len(bad), bad[:4])


def _odd_bases(rng, nrandom):
    bases = [1, 3, 5, 7, MASK]
    for k in range(3, 256):
        bases += [(1 << k) - 1, (1 << k) + 1]
    bases += [rng.getrandbits(256) | 1 for _ in range(nrandom)]
    return bases


def _n_values():
    return ([1 << k for k in range(246)] + [(1 << 246) - 1])


def test_every_level_alone(host):
    """n = 0..30 under every odd base: level n is the last whose term is non-zero."""
    rng = random.Random(0x5E71E5)
    bases = _odd_bases(rng, 300)
    pairs = [(b, e0 + 256 * n) for b in bases for n in range(31) for e0 in (0, 1, 255)]
    _check(host, pairs)


def test_high_parts(host):
    """n a single bit at every position, n all ones, and the exponent bits that do not matter."""
    rng = random.Random(0x41A)
    bases = [1, 3, 5, 7, 9, MASK, (1 << 255) + 1, (1 << 128) - 1, (1 << 33) + 1] + \
            [rng.getrandbits(256) | 1 for _ in range(24)]
    pairs = []
    for b in bases:
        for n in _n_values():
            for e0 in (0, 1, 255):
                pairs.append((b, e0 + 256 * n))
        for top in (1 << 254, 1 << 255, 3 << 254):
            for low in (0, 1, 255, 256, 257, (1 << 254) - 1, rng.getrandbits(254)):
                pairs.append((b, top | low))
                # the bits at and above 254 do not change an odd base's power
                assert pow(b, top | low, MOD) == pow(b, low, MOD)
    _check(host, pairs)


def test_every_odd_base_shape(host):
    """Every odd base shape against a few exponents that run the whole chain."""
    rng = random.Random(0xBA5E)
    exps = [256, 257, 511, 256 * 27, 256 * 28 + 255, 256 * 29, MASK, MASK - 1, (1 << 254) - 1,
            (1 << 254) - 256, 0xAAAA_AAAA << 100] + [rng.getrandbits(256) for _ in range(6)]
    _check(host, [(b, e) for b in _odd_bases(rng, 300) for e in exps])


def test_even_bases(host):
    rng = random.Random(0xE7E4)
    bases = [0, 2, 4, 6, 1 << 31, 1 << 32, 1 << 255, MASK - 1, 3 << 100] + \
            [rng.getrandbits(256) & ~1 for _ in range(40)] + [rng.getrandbits(16) << 1 for _ in range(10)]
    exps = [0, 1, 2, 3, 7, 8, 63, 64, 127, 128, 254, 255, 256, 257, 511, 512, 1 << 32, 1 << 84,
            (1 << 254) + 3, (1 << 255) + 255, MASK]
    _check(host, [(b, e) for b in bases for e in exps])


def test_generated_columns_are_current(tmp_path, monkeypatch):
    """csrc/u256_cols.h (the columns and the truncated multiply-adds of the chain) is what
    tools/gen_u256_cols.py writes."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("gen_u256_cols", os.path.join(ROOT, "tools", "gen_u256_cols.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    committed = gen.OUT
    monkeypatch.setattr(gen, "OUT", str(tmp_path / "u256_cols.h"))
    gen.main()
    with open(committed) as f, open(gen.OUT) as g:
        assert f.read() == g.read()


@pytest.mark.parametrize("split", [9, 12, 20, 33])
def test_constants_follow_the_split(split, tmp_path):
    """Another PF_EXP_SPLIT has other levels, shifts and constants, all derived in the header."""
    rng = random.Random(split)
    exe = _exe(tmp_path, split)
    step = 1 << split
    bases = [1, 3, 5, 7, 15, 17, MASK, (1 << 200) - 1] + [rng.getrandbits(256) | 1 for _ in range(40)]
    pairs = [(b, e0 + step * n) for b in bases for n in list(range(40)) + [(1 << (254 - split)) - 1]
             for e0 in (0, step - 1)]
    pairs += [(b, rng.getrandbits(256)) for b in bases for _ in range(8)]
    pairs += [(b & ~1, e) for b in bases[:12] for e in (0, 5, 255, 256, step, MASK)]
    _check(exe, pairs)
