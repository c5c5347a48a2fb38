"""The host's shared evaluator (mythril_amd/csrc/pf_hostint.h: the fold pass's, the hint solver's
and Power's arithmetic), op by op and exactly: tests/host_ops_check.cpp built with the address
and undefined-behaviour sanitizers and run as a child process on
  - every vector of tests/golden/ops.json (18 ops x widths 1, 8, 160, 255, 256),
  - NOT, NEG, EXTRACT, CONCAT, SEXT (and AND, OR, XOR, EQ, MOV, which the golden file lacks)
    against the oracle's functions at the same widths,
  - PF_W_HASH against the oracle's, CRC-32 against zlib's.
CPU only."""

import os
import random
import shutil
import subprocess
import zlib

import pyoracle as O
import pytest
from conftest import ROOT, load_golden
from test_gpu_parity import _CMPS, _OPS

from mythril_amd import ir

WIDTHS = (1, 8, 160, 255, 256)
SALTS = (0, 0xFFFFFFFF, zlib.crc32(b"keccak256_512"))
NAMES = ("keccak256_512", "keccak256_32", "Power", "f", "some_uninterpreted_function@3")


def _operands(w, rng):
    m = O.M(w)
    return [v & m for v in (0, 1, 2, m, 1 << (w - 1), (1 << (w - 1)) - 1)] + [rng.getrandbits(w) for _ in range(3)]


def _cases():
    """(request line, expected output line), in order."""
    out = []

    def case(op, w, aux, a, b, want):
        out.append((f"{op:x} {w:x} {aux:x} {a:x} {b:x}", f"{int(want):064x}"))

    for v in load_golden("ops.json"):
        op = _OPS[v["op"]] if v["op"] in _OPS else _CMPS[v["op"]]
        r = v["r"] if isinstance(v["r"], int) else int(v["r"], 16)
        case(op, v["w"], 0, int(v["a"], 16), int(v["b"], 16), r)
    n_golden = len(out)

    rng = random.Random(20260111)
    for w in WIDTHS:
        xs = _operands(w, rng)
        for a in xs:
            case(ir.W_NOT, w, 0, a, 0, O.bvnot(a, w))
            case(ir.W_NEG, w, 0, a, 0, O.bvneg(a, w))
            for salt in SALTS:
                case(ir.W_HASH, w, salt, a, 0, O.uf_hash(a, salt) & O.M(w))
            # a w-bit source: its low and high bits, both halves, all of it, and into a wider result
            for lo, wr in {(0, w), (0, 1), (w - 1, 1), (0, (w + 1) // 2), (w // 2, w - w // 2)}:
                case(ir.W_EXTRACT, wr, lo, a, 0, O.extract(a, lo, wr))
            for wr in {w, (w + 1) // 2}:
                case(ir.W_MOV, wr, 0, a, 0, a & O.M(wr))
            # sign extension to w bits from 1 bit, half, all but one, all of them
            for ws in {1, (w + 1) // 2, max(w - 1, 1), w}:
                case(ir.W_SEXT, w, ws, a & O.M(ws), 0, O.sign_extend(a & O.M(ws), ws, w))
            for b in xs:
                case(ir.W_AND, w, 0, a, b, a & b)
                case(ir.W_OR, w, 0, a, b, a | b)
                case(ir.W_XOR, w, 0, a, b, a ^ b)
                case(ir.B_EQ, w, 0, a, b, a == b)
                # a w-bit result from a low part of 1 bit, half, all but one (w = 1: two 1-bit parts)
                for wr, wb in {(w, 1), (w, w // 2), (w, w - 1)} if w > 1 else {(2, 1)}:
                    if 1 <= wb < wr:
                        hi, lo = a & O.M(wr - wb), b & O.M(wb)
                        case(ir.W_CONCAT, wr, wb, hi, lo, O.concat(hi, lo, wb))
    n_ops = len(out) - n_golden

    for name in NAMES:
        out.append((f"crc {name}", f"{zlib.crc32(name.encode()):x}"))
    # an opcode that is no function of two values is reported, not evaluated
    for op in (ir.W_ITE, ir.W_VAR, ir.B_AND, ir.END):
        out.append((f"{op:x} 100 0 1 1", "?"))
    return out, n_golden, n_ops


def test_shared_evaluator_against_golden_vectors_and_the_oracle(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host_ops_check.cpp"
    exe = str(tmp_path / "host_ops_check")
    # the sanitizers' runtimes linked into the program itself: it runs as it is, in any environment
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-o", exe, os.path.join(ROOT, "tests", "host_ops_check.cpp")], check=True)
    cases, n_golden, n_ops = _cases()
    assert n_golden == 10152 and n_ops > 5 * 9 * 10
    p = subprocess.run([exe], input="".join(q + "\n" for q, _ in cases), capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])
    got = p.stdout.split("\n")
    assert got[-1] == "" and len(got) - 1 == len(cases)
    bad = [(q, want, g) for (q, want), g in zip(cases, got) if g != want]
    assert not bad, (len(bad), bad[:4])
