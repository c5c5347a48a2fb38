"""The host's shared evaluator (mythril_amd/csrc/pf_hostint.h: the fold pass's, the hint solver's,
Power's and the config-3 generator's arithmetic), op by op and exactly: tests/host_ops_check.cpp
built with the address and undefined-behaviour sanitizers and run as a child process on
  - every vector of tests/golden/ops.json (18 ops x widths 1, 8, 160, 255, 256),
  - NOT, NEG, EXTRACT, CONCAT, SEXT (and AND, OR, XOR, EQ, MOV, which the golden file lacks)
    against the oracle's functions at the same widths,
  - the multi-digit division against the oracle's: twelve pairs that take algorithm D's add-back
    step (widths 256, 160, 255, all five division ops) and 2,000 pairs of extreme digits,
  - EXP at every width over the edges of powmod's shortcuts, MUL at 256 bits,
  - PF_W_HASH against the oracle's, CRC-32 against zlib's,
  - the op-by-op section again at each of the other 251 widths of 1..256, and every arithmetic op
    and compare on the 8-row lists of tests/width_cases.py at every width.
CPU only."""

import os
import random
import shutil
import subprocess
import zlib

import pyoracle as O
import pytest
import width_cases as WC
from conftest import ROOT, load_golden
from test_gpu_parity import _CMPS, _OPS

from mythril_amd import ir

WIDTHS = (1, 8, 160, 255, 256)
SALTS = (0, 0xFFFFFFFF, zlib.crc32(b"keccak256_512"))
NAMES = ("keccak256_512", "keccak256_32", "Power", "f", "some_uninterpreted_function@3")


# (a, b) whose long division takes algorithm D's add-back step (the estimated quotient digit
# still one too large after its corrections): the first six with 32-bit digits, the last six
# with 64-bit digits.  A random pair takes it about twice in 2^32.
ADD_BACK = (
    (0xfffffffe000000017fffffff80000001, 0x7fffffff800000007fffffff),
    (0x20000000280000000fffffffe0000000180000001, 0x20000000280000000fffffffe0000000200000001),
    (0x7fffffff7fffffff800000000000000080000000ffffffffffffffff00000000, 0x17ffffffffffffffeffffffff7fffffff),
    (0xffffffff7fffffff7fffffffffffffff0000000200000000ffffffff00000000,
     0x800000010000000280000001800000000000000280000000fffffffe),
    (0xfffffffe80000000000000000000000000000002, 0xffffffff7fffffffffffffff80000000),
    (0x80000000800000000000000100000001000000017fffffff8000000100000000, 0x8000000100000001000000028000000180000001),
    (0x80000000000000008000000000000000ffffffffffffffff8000000000000001,
     0x80000000000000010000000000000002fffffffffffffffe),
    (0x8000000000000001800000000000000080000000000000000000000000000000,
     0x180000000000000017fffffffffffffffffffffffffffffff),
    (0x8000000000000001800000000000000100000000000000000000000000000001,
     0x800000000000000180000000000000018000000000000001),
    (0x8000000000000000ffffffffffffffff0000000000000000, 0x8000000000000000ffffffffffffffff8000000000000001),
    (0x7fffffffffffffff80000000000000017fffffffffffffff8000000000000000, 0x100000000000000000000000000000001),
    (0xfffffffffffffffe800000000000000080000000000000010000000000000001,
     0xfffffffffffffffe8000000000000000ffffffffffffffff0000000000000001),
)


def _structured_pairs():
    """1,000 (a, b) per digit size 32 and 64, their digits from the values at which a quotient
    digit's estimate goes wrong: about one pair in 150 takes the add-back, many more a correction."""
    rng = random.Random(20260114)
    out = []
    for d in (32, 64):
        B = 1 << d
        digits = (0, 1, 2, B - 1, B - 2, B // 2, B // 2 - 1, B // 2 + 1)
        n = 0
        while n < 1000:
            na = rng.randint(3, 256 // d)
            nb = rng.randint(2, na)
            a = sum(rng.choice(digits) << (d * i) for i in range(na))
            b = sum(rng.choice(digits) << (d * i) for i in range(nb))
            if a and b:
                out.append((a, b))
                n += 1
    return out


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

    def ops_at(w, rng):
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

    rng = random.Random(20260111)
    for w in WIDTHS:
        ops_at(w, rng)
    n_ops = len(out) - n_golden

    # the multi-digit division (Knuth's algorithm D), which the vectors above barely reach
    divs = ((ir.W_UDIV, O.bvudiv), (ir.W_UREM, O.bvurem), (ir.W_SDIV, O.bvsdiv), (ir.W_SREM, O.bvsrem),
            (ir.W_SMOD, O.bvsmod))
    for w in (256, 160, 255):
        for a, b in ADD_BACK:
            a, b = a & O.M(w), b & O.M(w)
            for op, f in divs:
                case(op, w, 0, a, b, f(a, b, w))
    for a, b in _structured_pairs():
        case(ir.W_UDIV, 256, 0, a, b, O.bvudiv(a, b, 256))
        case(ir.W_UREM, 256, 0, a, b, O.bvurem(a, b, 256))
    # EXP: 0^0 = 1, the even base's shortcut either side of an exponent of 256, the last squaring
    rng = random.Random(20260115)
    for w in WIDTHS:
        m = O.M(w)
        bases = [v & m for v in (0, 1, 2, 3, rng.getrandbits(w) & ~1, rng.getrandbits(w) | 1, 1 << (w - 1), m)]
        for a in bases:
            for e in (0, 1, 2, 255, 256, 257, 1 << 32, m):
                case(ir.W_EXP, w, 0, a, e & m, O.bvexp(a, e & m, w))
    xs = _operands(256, rng)
    for a in xs:
        for b in xs:
            case(ir.W_MUL, 256, 0, a, b, O.bvmul(a, b, 256))

    for name in NAMES:
        out.append((f"crc {name}", f"{zlib.crc32(name.encode()):x}"))
    # an opcode that is no function of two values is reported, not evaluated
    for op in (ir.W_ITE, ir.W_VAR, ir.B_AND, ir.END):
        out.append((f"{op:x} 100 0 1 1", "?"))

    # every width 1..256: the op-by-op section at the widths it has not run at above, then every
    # arithmetic op and compare on the width catalogue's 8-row lists (tests/width_cases.py, whose
    # expectations are Python integers: test_width_cases.py holds them against the oracle's)
    n_before = len(out)
    rng = random.Random(20260116)
    for w in range(1, 257):
        if w not in WIDTHS:
            ops_at(w, rng)
    n_wide = len(out) - n_before
    for key in WC.GROUND_KEYS:
        op = WC.BIN[key] if key in WC.BIN else WC.CMP[key]
        for w in WC.WIDTHS:
            for r in WC.rows(key, w, WC.N_SEARCH):
                case(op, w, 0, r.args[0], r.args[1], r.expect)
    return out, n_golden, n_ops, (n_wide, len(out) - n_before - n_wide)


def test_shared_evaluator_against_golden_vectors_and_the_oracle(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/host_ops_check.cpp"
    exe = str(tmp_path / "host_ops_check")
    # the sanitizers' runtimes linked into the program itself: it runs as it is, in any environment
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-o", exe, os.path.join(ROOT, "tests", "host_ops_check.cpp")], check=True)
    cases, n_golden, n_ops, (n_wide, n_catalogue) = _cases()
    assert n_golden == 10152 and n_ops > 5 * 9 * 10
    # the division, EXP and MUL cases and the 5 + 4 requests after them
    assert len(cases) - n_golden - n_ops - n_wide - n_catalogue == 3 * 12 * 5 + 2 * 2000 + 5 * 8 * 8 + 9 * 9 + 9
    # 251 more widths of the op-by-op section (at least what its smallest width gives), and
    # 15 ops + 7 compares x 256 widths x 8 rows
    assert n_wide > 251 * 9 * 10 and n_wide * 5 > n_ops * 251 // 2
    assert n_catalogue == 22 * 256 * 8
    p = subprocess.run([exe], input="".join(q + "\n" for q, _ in cases), capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])
    got = p.stdout.split("\n")
    assert got[-1] == "" and len(got) - 1 == len(cases)
    bad = [(q, want, g) for (q, want), g in zip(cases, got) if g != want]
    assert not bad, (len(bad), bad[:4])
