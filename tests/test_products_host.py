"""The product routines of csrc/u256.h on the host, against Python's * and pow: mul256, sqr256,
every tmul_add level of the configured split's Horner chain and exp256_split, through
tests/products_host_check.cpp (PF_HOST_MAC: the C mirrors of the generated columns), built with
the address and undefined-behaviour sanitizers and run as a child process.  The rows are those
of tests/test_gpu_products.py (products_cases.py: all carries, one carrying column, one-limb
operands, powers of two at limb boundaries; the exponent classes that exp256_split separates)
plus a few thousand seeded random ones.  Also: tools/gen_u256_cols.py reproduces the committed
u256_cols.h.

The host build runs the mirrors, not the inline asm; the asm rests on the GPU rows.  CPU only."""
import os
import random
import subprocess
import sys

import products_cases as C
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "products_host_check.cpp")
CLANG = "/opt/rocm/llvm/bin/clang++"   # u256.h uses clang's __builtin_addc
MOD = 1 << 256


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    assert os.path.exists(CLANG), "the host clang++ is needed to build tests/products_host_check.cpp"
    exe = str(tmp_path_factory.mktemp("products") / "products_host_check")
    # the sanitizers' runtimes are linked into the program itself: it runs as it is
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, SRC], check=True)
    return exe


def _run(exe, lines):
    p = subprocess.run([exe], input="".join(f"{op} {a:064x} {b:064x}\n" for op, a, b in lines),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])
    out = p.stdout.split("\n")
    assert out[-1] == ""
    levels = [ln.split() for ln in out if ln.startswith("level ")]
    res = [int(ln, 16) for ln in out[len(levels):-1]]
    assert len(res) == len(lines), (len(res), len(lines))
    return [(int(i), int(l), int(ly), int(k, 16)) for _, i, l, ly, k in levels], res


def _odd(i):
    return i >> ((i & -i).bit_length() - 1)


def _addend(i, j, limbs):
    """K_i = odd(i) ... odd(j) / (odd(1) ... odd(j)) mod 2^(32 limbs) (csrc/u256.h, exp_addend)."""
    num = den = 1
    for k in range(1, j + 1):
        den *= _odd(k)
        if k >= i:
            num *= _odd(k)
    return num * pow(den, -1, MOD) % (1 << (32 * limbs))


def test_mul_and_sqr(host):
    rng = random.Random(0x9120D)
    rows = C.mul_rows() + [(rng.getrandbits(256), rng.getrandbits(rng.choice((32, 64, 200, 256)))) for _ in range(3000)]
    lines = [("mul", a, b) for a, b in rows] + [("sqr", v, 0) for a, b in rows for v in (a, b)]
    _, got = _run(host, lines)
    want = [a * b % MOD for a, b in rows] + [v * v % MOD for a, b in rows for v in (a, b)]
    bad = [(lines[i][0], hex(lines[i][1]), hex(lines[i][2]), hex(got[i]), hex(want[i]))
           for i in range(len(lines)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:4])


def test_every_tmul_add_level(host):
    """a * b + K_I mod 2^(32 L) at each level's shape, K_I recomputed here."""
    levels, _ = _run(host, [])
    j = len(levels)
    assert j >= 20 and [lv[0] for lv in levels] == list(range(1, j + 1))
    rng = random.Random(0x7A11)
    lines, want = [], []
    for i, nl, ly, k in levels:
        assert k == _addend(i, j, min(nl, 8)), (i, hex(k))
        assert ly in (nl, nl - 1) and 1 <= nl <= 8
        ma, mb = (1 << (32 * nl)) - 1, (1 << (32 * ly)) - 1
        ops = [(C.M256, C.M256), (0, 0), (1, C.M256), (C.M256, 1)]
        ops += [(a, b) for a, b in C.mul_rows()[:6]]
        ops += [(rng.getrandbits(256), rng.getrandbits(256)) for _ in range(150)]
        for a, b in ops:
            a, b = a & ma, b & mb
            lines.append((f"t{i}", a, b))
            want.append((a * b + k) & ma)
    _, got = _run(host, lines)
    bad = [(lines[i][0], hex(lines[i][1]), hex(lines[i][2]), hex(got[i]), hex(want[i]))
           for i in range(len(lines)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:4])


def test_exp_split(host):
    rng = random.Random(0xE4B)
    rows = C.exp_rows()
    for name in C.WAVES:                       # the mixed waves' lanes, each as a wave of its own
        rows += C.wave(name, 0)
    for _ in range(1500):
        b = rng.getrandbits(256) | rng.getrandbits(1)
        e = rng.choice((rng.getrandbits(256), rng.getrandbits(9), 256 * rng.getrandbits(12) + rng.getrandbits(2)))
        rows.append((b, e))
    _, got = _run(host, [("exp", b, e) for b, e in rows])
    bad = [(hex(b), hex(e), hex(g)) for (b, e), g in zip(rows, got) if g != pow(b, e, MOD)]
    assert not bad, (len(bad), bad[:4])


def test_generator_reproduces_the_committed_columns(tmp_path):
    committed = os.path.join(ROOT, "mythril_amd", "csrc", "u256_cols.h")
    code = ("import importlib.util, sys\n"
            "spec = importlib.util.spec_from_file_location('gen', sys.argv[1])\n"
            "gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)\n"
            "gen.OUT = sys.argv[2]; gen.main()\n")
    out = str(tmp_path / "u256_cols.h")
    subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "tools", "gen_u256_cols.py"), out], check=True)
    with open(committed) as f, open(out) as g:
        assert f.read() == g.read()
