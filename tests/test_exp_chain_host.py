"""The fused powering chain of pf::exp256_split (csrc/u256.h: where the series runs, b^e0 is
the product of the squarings that climb to the series' step, one factor per set bit of e0) on
the host, against Python's pow(b, e, 2**256).

tools/exp_series_host.cpp is built at the configured split 8, at 9, 10 and 20 (the chain is as
long as the split; 20 is the last split that takes it) and at 21 (a 3-bit window: the windowed
loop and the step's own squarings are kept there).  Per split (cases in exp_chain_cases.py):
every e0 in 0..255 with n != 0 under an odd random base, a base whose t is all ones and an even
base; the single-bit and alternating patterns of e0 with n in {0, 1, 2^246 - 1}; bases 0, 1, 2,
2^32 and 2^256 - 1; the even bases' edges (2^255, 2^256 = 0, exponent bits >= 254).  One lane
is one wave here: a lane with n = 0 or an even base takes the windowed path, which the series'
lanes no longer share (the mixed waves are tests/test_gpu_exp_chain.py's).  The same program is
also built once with the address and undefined-behaviour sanitizers linked in.  CPU only."""
import os
import subprocess

import exp_chain_cases as C
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "exp_series_host.cpp")
CLANG = "/opt/rocm/llvm/bin/clang++"
MOD = 1 << 256

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="no host clang++")

SPLITS = [8, 9, 10, 20, 21]


def _check(exe, pairs):
    inp = "".join(f"{b:064x} {e:064x}\n" for b, e in pairs)
    p = subprocess.run([exe], input=inp, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])
    out = p.stdout.split()
    assert len(out) == len(pairs)
    bad = [(hex(b), hex(e), got, f"{pow(b, e, MOD):064x}")
           for (b, e), got in zip(pairs, out) if int(got, 16) != pow(b, e, MOD)]
    assert not bad, (len(bad), bad[:4])


def test_cases_are_what_they_claim():
    for m in SPLITS:
        odd, ones, even = C.three_bases(m)
        assert odd & 1 and ones & 1 and not even & 1
        assert (pow(ones, 1 << m, MOD) - 1) >> (m + 2) == (1 << (254 - m)) - 1
        rows = C.every_e0(m)
        with_n = [(b, e) for b, e in rows if C.split_e(e, m)[1]]
        for base in (odd, ones, even):
            assert sorted(e & 255 for b, e in with_n if b == base) == list(range(256))
        assert {e for b, e in rows if b == even and e < 256} == set(range(256))
        assert {(C.split_e(e, m)[0], C.split_e(e, m)[1]) for b, e in C.pattern_pairs(m) if b == odd} >= \
               {(e0, n) for e0 in C.PATTERNS for n in (0, 1, C.N_BIG >> (m - 8))}
        assert {b for b, _ in C.special_bases(m)} == {0, 1, 2, 1 << 32, MOD - 1}
    edges = C.even_edges(8)
    assert (2, 255) in edges and (2, 256) in edges and any(not b & 1 and e >> 254 for b, e in edges)
    assert pow(2, 255, MOD) == 1 << 255 and pow(2, 256, MOD) == 0


@pytest.mark.parametrize("split", SPLITS)
def test_chain_cases(split, tmp_path):
    exe = os.path.join(str(tmp_path), f"exp_chain_host_{split}")
    subprocess.check_call([CLANG, "-O2", "-std=c++17", f"-DPF_EXP_SPLIT={split}", "-o", exe, SRC])
    _check(exe, C.host_pairs(split))


def test_under_sanitizers(tmp_path):
    """The sanitizers' runtimes are linked into the program itself: it runs as it is."""
    exe = os.path.join(str(tmp_path), "exp_chain_host_san")
    subprocess.check_call([CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, SRC])
    _check(exe, C.host_pairs(8))
