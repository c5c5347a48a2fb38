"""CPU: the site bookkeeping of mythril_amd/csrc/pf_devprog.h (pf_device_sites) as a host
program of its own, tests/devsites_host_check.cpp, built here with AddressSanitizer +
UndefinedBehaviorSanitizer and run on the census fixtures with the fold on, off and alone.  The
program checks its map against the device program it builds beside it; this test checks that the
sanitizers stay silent and that the library returns the same map."""

import os
import subprocess

import numpy as np
import pytest

import census_sets as CS
from mythril_amd import _lib, ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "devsites_host_check.cpp")
CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(CLANG), "the host clang++ is needed to build tests/devsites_host_check.cpp"
    out = str(tmp_path_factory.mktemp("devsites") / "devsites_host_check")
    # the sanitizers' runtimes are linked into the program itself: it runs as it is
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", out, SRC], check=True)
    return out


def run(exe, batch, tmp_path, fold):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    code = np.ascontiguousarray(batch.code, dtype=np.uint32)
    consts = np.ascontiguousarray(batch.consts, dtype=np.uint32)
    descs = np.ascontiguousarray(batch.descs, dtype=np.uint32)
    with open(src, "wb") as f:
        np.array([len(code), len(consts.reshape(-1, 8)), len(descs)], dtype=np.uint64).tofile(f)
        for a in (code, consts, descs):
            a.tofile(f)
    p = subprocess.run([exe, src, dst, str(fold)], capture_output=True, text=True, timeout=300)
    assert p.stderr == "" and p.returncode == 0, (p.returncode, p.stdout, p.stderr[-3000:])
    with open(dst, "rb") as f:
        n_sites, n_sets = (int(x) for x in np.fromfile(f, dtype=np.uint64, count=2))
        sites = np.fromfile(f, dtype=np.uint32, count=n_sites)
        cnt = np.fromfile(f, dtype=np.uint32, count=n_sets)
        assert f.read() == b""
    out, off = [], 0
    for k in cnt.tolist():
        out.append(sites[off:off + k].tolist())
        off += k
    return out


@pytest.mark.parametrize("fold", [1, 0, 2])
@pytest.mark.parametrize("which", ["big", "small"])
def test_host_program_equals_the_library(exe, tmp_path, monkeypatch, fold, which):
    progs = CS.big_batch() if which == "big" else CS.small_batch()
    batch = ir.Batch(progs)
    got = run(exe, batch, tmp_path, fold)
    monkeypatch.setenv("PF_DEVICE_FOLD", str(fold))
    lib = [g.tolist() for g in _lib.device_sites(batch.code, batch.consts, batch.descs)]
    assert got == lib
    by = {p.name: g for p, g in zip(progs, got)}
    if which == "big":
        assert by["folded-first"] == ([0, 1, 2, 3] if fold == 0 else [1, 3])
    else:
        assert by["folded-away"] == [0]       # below the gate: never folded
