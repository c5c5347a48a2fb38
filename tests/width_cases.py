"""The width catalogue (test tooling, no GPU needed to import): every op, compare and generator
arm at every width 1..256.

For a catalogue key (an op, or an op with one of its second widths: ``sext:half``,
``extract:31``, ``concat:w-1``, ``hash:1``) and a width w, ``rows(key, w, n)`` is a list of
``Row(key, w, args, expect, bit)``: operand values, the expectation and the bit of it that the
corrupted twin flips.  Expectations are computed here with Python's integers, by definitions
written for this module (signed values as Python ints, floor division, ``pow``), not with
oracle/pyoracle.py's functions: tests/test_width_cases.py checks the oracle against them.

Operands are drawn with one fixed seed from the width's edge set (``edge_set``); the first rows
of every list are the repair: the pairs a condition of the catalogue needs (sign combinations,
a zero divisor, (most negative, -1), the shift amounts around w, EXP's exponents, both verdicts
of a compare).  tests/test_width_cases.py asserts the conditions on the lists themselves.
``rows(key, w, 8)`` is a prefix of ``rows(key, w, 40)``: 8 rows go through the search, census and
climb kernels by the candidate-0 protocol (op_programs.py), 40 through the stream and SoA
kernels as explicit candidates of one program per (key, w, base) (``explicit_set``).

``generator_set`` / ``width_pin_set_at`` put a VK_GENERIC and a VK_VALUE variable of every width
in front of the materialise kernel and the inlined generator."""

import functools
import random
from collections import namedtuple

import op_programs as P

from mythril_amd import ir

SEED = 0x5EED_0F_1D75
WIDTHS = tuple(range(1, 257))
N_SEARCH, N_EXPLICIT = 8, 40
HASH_SALTS = (0, 0x5A17, 0xFFFFFFFF)

Row = namedtuple("Row", "key w args expect bit")

BIN = {"add": ir.W_ADD, "sub": ir.W_SUB, "mul": ir.W_MUL, "udiv": ir.W_UDIV, "urem": ir.W_UREM,
       "sdiv": ir.W_SDIV, "srem": ir.W_SREM, "smod": ir.W_SMOD, "and": ir.W_AND, "or": ir.W_OR,
       "xor": ir.W_XOR, "shl": ir.W_SHL, "lshr": ir.W_LSHR, "ashr": ir.W_ASHR, "exp": ir.W_EXP}
CMP = {"eq": ir.B_EQ, "ult": ir.B_ULT, "ule": ir.B_ULE, "slt": ir.B_SLT, "sle": ir.B_SLE,
       "uadd_noovf": ir.B_UADD_NOOVF, "umul_noovf": ir.B_UMUL_NOOVF}
UN = {"not": ir.W_NOT, "neg": ir.W_NEG, "mov": ir.W_MOV}
SIGNED = ("sdiv", "srem", "smod")
SHIFTS = ("shl", "lshr", "ashr")
SEXTS = ("sext:1", "sext:half", "sext:w-1", "sext:w")
EXTRACTS = ("extract:0", "extract:1", "extract:31", "extract:32", "extract:top")
CONCATS = ("concat:1", "concat:half", "concat:w-1")
HASHES = tuple(f"hash:{i}" for i in range(len(HASH_SALTS)))
KEYS = tuple(BIN) + tuple(UN) + ("mov_narrow", "ite") + HASHES + tuple(CMP) + SEXTS + EXTRACTS + CONCATS
GROUND_KEYS = tuple(BIN) + tuple(CMP)      # op_programs.ground_set: two constants
NEAR_KEYS = ("eq", "ult", "ule", "slt", "sle")


def M(w):
    return (1 << w) - 1


def signed(x, w):
    return x - (1 << w) if x >> (w - 1) else x


# ---- what a key is at a width -----------------------------------------------------------------

Spec = namedtuple("Spec", "shape op wa wb aux0")     # wa, wb: operand widths; aux0 as emitted


def spec(key, w):
    """The key's instruction at width w, or None where it does not exist there."""
    if key in BIN:
        return Spec("bin", BIN[key], w, w, 0)
    if key in CMP:
        return Spec("cmp", CMP[key], w, w, 0)
    if key in UN:
        return Spec("un", UN[key], w, w, 0)
    if key == "mov_narrow":
        return Spec("un", ir.W_MOV, 256, w, 0) if w < 256 else None
    if key == "ite":
        return Spec("ite", ir.W_ITE, w, w, 0)
    if key in HASHES:
        return Spec("un", ir.W_HASH, 256, w, HASH_SALTS[HASHES.index(key)])
    if key in SEXTS:
        ws = {"sext:1": 1, "sext:half": (w + 1) // 2, "sext:w-1": w - 1, "sext:w": w}[key]
        return Spec("un", ir.W_SEXT, ws, w, ws) if ws >= 1 else None
    if key in EXTRACTS:
        lo = {"extract:0": 0, "extract:1": 1, "extract:31": 31, "extract:32": 32, "extract:top": 256 - w}[key]
        return Spec("un", ir.W_EXTRACT, 256, w, lo) if lo + w <= 256 else None
    if key in CONCATS:
        wb = {"concat:1": 1, "concat:half": w // 2, "concat:w-1": w - 1}[key]
        return Spec("bin", ir.W_CONCAT, w - wb, wb, wb) if w >= 2 else None
    raise KeyError(key)


def widths_of(key):
    return tuple(w for w in WIDTHS if spec(key, w) is not None)


# ---- expectations, in Python's integers -------------------------------------------------------

def _philox(ctr, key):
    """Philox-4x32-10 on Python ints (Salmon et al., SC'11: the multipliers and Weyl keys)."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [c0, c1, c2, c3]


def _hash(x, salt):
    """PF_W_HASH by include/pf_bytecode.h: two Philox blocks over the limbs of x, the second
    keyed differently and fed the first's output."""
    xs = [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
    h = _philox(xs[:4], (salt, 0x5BD1E995))
    g = _philox([xs[4 + i] ^ h[i] for i in range(4)], (salt, 0x27D4EB2F))
    return sum(v << (32 * i) for i, v in enumerate(h + g))


def _sdiv(a, b, w):
    sa, sb = signed(a, w), signed(b, w)
    if sb == 0:
        return 1 if sa < 0 else M(w)
    q = abs(sa) // abs(sb)                       # truncates towards zero
    return (-q if (sa < 0) != (sb < 0) else q) & M(w)


def _srem(a, b, w):
    sa, sb = signed(a, w), signed(b, w)
    if sb == 0:
        return a
    r = abs(sa) % abs(sb)                        # the sign of the dividend
    return (-r if sa < 0 else r) & M(w)


def _smod(a, b, w):
    sa, sb = signed(a, w), signed(b, w)
    return a if sb == 0 else (sa % sb) & M(w)    # Python's %: the sign of the divisor


def expectation(key, w, args):
    m = M(w)
    s = spec(key, w)
    if key == "ite":
        sel, a, b = args
        return a if sel else b
    a = args[0]
    b = args[1] if len(args) > 1 else None
    if key == "add":
        return (a + b) & m
    if key == "sub":
        return (a - b) & m
    if key == "mul":
        return (a * b) & m
    if key == "udiv":
        return a // b if b else m
    if key == "urem":
        return a % b if b else a
    if key == "sdiv":
        return _sdiv(a, b, w)
    if key == "srem":
        return _srem(a, b, w)
    if key == "smod":
        return _smod(a, b, w)
    if key == "and":
        return a & b
    if key == "or":
        return a | b
    if key == "xor":
        return a ^ b
    if key == "shl":
        return (a << b) & m if b < w else 0
    if key == "lshr":
        return a >> b if b < w else 0
    if key == "ashr":
        return (signed(a, w) >> min(b, w)) & m
    if key == "exp":
        return pow(a, b, 1 << w)
    if key == "not":
        return a ^ m
    if key == "neg":
        return -a & m
    if key in ("mov", "mov_narrow"):
        return a & m
    if key in HASHES:
        return _hash(a, s.aux0) & m
    if key == "eq":
        return a == b
    if key == "ult":
        return a < b
    if key == "ule":
        return a <= b
    if key == "slt":
        return signed(a, w) < signed(b, w)
    if key == "sle":
        return signed(a, w) <= signed(b, w)
    if key == "uadd_noovf":
        return a + b < 1 << w
    if key == "umul_noovf":
        return a * b < 1 << w
    if key in SEXTS:
        return signed(a, s.wa) & m
    if key in EXTRACTS:
        return (a >> s.aux0) & m
    if key in CONCATS:
        return (a << s.wb | b) & m
    raise KeyError(key)


# ---- operands ---------------------------------------------------------------------------------

def edge_set(w, rng):
    m = M(w)
    top, half = 1 << (w - 1), 1 << (w // 2)
    vals = [0, 1, 2, 3, m, m - 1, top, top + 1, top - 1, half, half - 1, w - 1, w, w + 1,
            rng.getrandbits(w), rng.getrandbits(w), rng.getrandbits(w) >> rng.randrange(w)]
    return [v & m for v in vals]


def shift_amounts(w):
    """The amounts every shift runs at (as w-bit values), the last with a high limb set."""
    return [v & M(w) for v in (0, 1, w - 1, w, w + 1)] + ([(1 << 32 | 1) << (w - 33)] if w > 32 else [])


def _required(key, w, rng, draw):
    """The operand tuples the catalogue's conditions need, before the free draws."""
    m, top = M(w), 1 << (w - 1)
    pos = lambda: draw(w) & (top - 1) | (1 if w > 1 else 0)      # non-negative, not 0 (w >= 2)
    neg = lambda: draw(w) & (top - 1) | top
    if key in SIGNED:
        return [(pos(), pos()), (pos(), neg()), (neg(), pos()), (neg(), neg()), (neg(), 0), (top, m)]
    if key in SHIFTS:
        return [(draw(w) | (top if i % 2 == 0 else 0), amt) for i, amt in enumerate(shift_amounts(w))]
    if key == "exp":
        return [(draw(w) & ~1, 0), (draw(w) | 1, 1), (draw(w) & ~1, 2 & m), (draw(w) | 1, m)]
    if key in ("udiv", "urem"):
        return [(draw(w), 0), (m, m), (m, 1)]
    if key in ("slt", "sle"):
        x = draw(w)
        return [(0, m), (m, 0), (x, x), (pos(), pos()), (neg(), neg())]
    if key in CMP:
        x = draw(w)
        return [(0, m), (m, 0), (x, x), (m, m), (m, 2 & m)]
    if key in SEXTS:
        ws = spec(key, w).wa
        return [(draw(ws) | 1 << (ws - 1),), (draw(ws) & M(ws - 1),)]
    return []


def _free(key, w, rng, draw, i):
    s = spec(key, w)
    if key == "ite":
        return (i & 1, draw(w), draw(w))
    if key == "eq":
        a = draw(w)
        return (a, a if i & 1 else a ^ 1 << rng.randrange(w))
    if key in SHIFTS and rng.random() < 0.6:
        return (draw(w), rng.choice(shift_amounts(w) + [rng.randrange(w)]))
    if key == "mov_narrow":
        return (draw(w) | (rng.getrandbits(256 - w) | 1) << w,)
    if key in HASHES:
        return (rng.choice((draw(256), rng.getrandbits(256))),)
    if key in EXTRACTS:
        lo = s.aux0
        return (rng.getrandbits(256) & ~(M(w) << lo) | draw(w) << lo,)
    if s.shape == "un":
        return (draw(s.wa),)
    return (draw(s.wa), draw(s.wb))


@functools.lru_cache(maxsize=None)
def rows(key, w, n=N_EXPLICIT):
    """n rows of the key at width w ([] where it does not exist there); a smaller n is a prefix
    of a larger one."""
    if spec(key, w) is None:
        return []
    if n != N_EXPLICIT:
        assert n <= N_EXPLICIT
        return rows(key, w)[:n]
    rng = random.Random(f"{SEED}/{key}/{w}")
    edges = {}

    def draw(width):
        if width not in edges:
            edges[width] = edge_set(width, rng)
        return rng.choice(edges[width])

    out = []
    ops = _required(key, w, rng, draw)
    assert len(ops) <= N_SEARCH
    while len(ops) < N_EXPLICIT:
        ops.append(_free(key, w, rng, draw, len(ops)))
    ew = 1 if key in CMP else w
    for i, args in enumerate(ops):
        bit = ew - 1 if i % 4 == 0 else rng.randrange(ew)       # the top bit in a quarter
        out.append(Row(key, w, tuple(args), expectation(key, w, tuple(args)), bit))
    return out


def corrupted(row):
    """The row's expectation with its bit flipped (a compare's: the other verdict)."""
    if isinstance(row.expect, bool):
        return not row.expect
    return row.expect ^ 1 << row.bit


def near_rows(key, w):
    """Pairs at which the compare ``key`` is false, for a directly asserted (fused) compare:
    the unsigned distance |a - b| of bit length 0 (strict compares), 1, ceil(w / 2) and w, and
    for the signed compares pairs whose signs differ.  (a, b, bit length of the distance)."""
    m, top = M(w), 1 << (w - 1)
    out, seen = [], set()
    rng = random.Random(f"{SEED}/near/{key}/{w}")
    for length in (0, 1, (w + 1) // 2, w):
        d = 0 if length == 0 else 1 << (length - 1)
        bases = [top - d, 0, top - 1 - d, top, m - d, rng.getrandbits(w) % (m - d + 1)]    # top - d: the signs differ
        found = 0
        for x in bases:
            if not 0 <= x <= m - d:
                continue
            for a, b in ((x + d, x), (x, x + d)):
                if found < 2 and not expectation(key, w, (a, b)) and (a, b) not in seen \
                        and abs(a - b).bit_length() == length:
                    seen.add((a, b))
                    out.append((a, b, length))
                    found += 1
    return out


# ---- programs: the candidate-0 protocol ---------------------------------------------------------

def search_set(row, base=0, twin=False, parents=True):
    """The row through op_programs' builders: ``twin`` asserts the corrupted expectation."""
    s = spec(row.key, row.w)
    e = corrupted(row) if twin else row.expect
    kw = dict(base=base, verdict=not twin, parents=parents)
    if s.shape == "bin":
        p = P.binop_set(s.op, row.w, *row.args, e, wa=s.wa, wb=s.wb, aux0=s.aux0, **kw)
    elif s.shape == "cmp":
        p = P.cmp_set(s.op, row.w, *row.args, e, **kw)
    elif s.shape == "ite":
        p = P.ite_set(row.w, *row.args, e, **kw)
    else:
        p = P.unop_set(s.op, row.w, row.args[0], e, wa=s.wa, aux0=s.aux0, **kw)
    p.row, p.twin = row, twin
    return p


def ground_set(row, base=0, twin=False):
    """The row with both operands constants (GROUND_KEYS)."""
    s = spec(row.key, row.w)
    p = P.ground_set(s.op, row.w, *row.args, corrupted(row) if twin else row.expect, base=base, verdict=not twin)
    p.row, p.twin = row, twin
    return p


def near_set(key, w, a, b, base=0):
    """ASSERT cmp(a, b) directly, where it is false: the compare and its assert fuse into one
    site of the device program, which the climb scores by the operands' distance."""
    p = P.cmp_set(CMP[key], w, a, b, True, base=base, verdict=False)
    p.row, p.twin = Row(key, w, (a, b), False, 0), False
    return p


def describe(p):
    """What a failure names: op, width, operands, which twin."""
    r = p.row
    return (r.key, f"w{r.w}", [hex(int(x)) for x in r.args],
            "corrupted twin (bit %d)" % r.bit if p.twin else "row", p.name)


# ---- programs: explicit candidates -----------------------------------------------------------

def explicit_set(key, w, base=0):
    """The key's instruction with every operand and the expectation a variable, so one program
    serves all rows of (key, w) as explicit candidates.  Variables in order: the operands (ITE:
    the Bool selector first), then the expectation (a compare's: a Bool).  Registers by the
    width's parity: the result in register 5 with the expectation in 6, or the operands in 5
    and 6 — the LDS registers of the 8-register kernels at base 0."""
    s = spec(key, w)
    ra, rb, rd, re = (0, 1, 5, 6) if w % 2 == 0 and s.shape != "cmp" else (5, 6, 2, 0)
    a = P.Asm(f"explicit:{key}/w{w}/base{base}", base, parents=False)
    if s.shape == "ite":
        a.bvar(3, None)
    a.wvar(ra, s.wa, None)
    if s.shape in ("bin", "cmp", "ite"):
        a.wvar(rb, s.wb, None)
    if s.shape == "cmp":
        a.cmp(s.op, w, 2, ra, rb)
        a.bvar(3, None)
        a.b(ir.B_XOR, 4, a=2, b=3)
        a.b(ir.B_NOT, 5, a=4)
        a.p.emit(ir.ASSERT, 1, a=5)
    else:
        if s.shape == "ite":
            a.w(ir.W_ITE, w, rd, ra, rb, c=3)
        elif s.shape == "bin":
            a.w(s.op, w, rd, ra, rb, aux0=s.aux0)
        else:
            a.w(s.op, w, rd, ra, aux0=s.aux0)
        a.wvar(re, w, None)
        a.cmp(ir.B_EQ, w, 0, rd, re)
        a.p.emit(ir.ASSERT, 1, a=0)
    return a.done(verdict=None)


def explicit_candidates(key, w, n=N_EXPLICIT):
    """(candidates, verdicts): every row held and corrupted, interleaved — 2n candidates."""
    cands, want = [], []
    for r in rows(key, w, n):
        cands += [[int(x) for x in r.args] + [int(r.expect)], [int(x) for x in r.args] + [int(corrupted(r))]]
        want += [True, False]
    return cands, want


# ---- the generator ---------------------------------------------------------------------------

GEN_LAYOUTS = ("bare", "consts", "bare-alternate", "consts-alternate")


def generator_set(layout, base=0, seed=0):
    """A VK_GENERIC and a VK_VALUE variable of every width 1..256 (512 variables: variable
    2 (w - 1) + j), without constants or with op_programs.GEN_POOL, without parents or with one
    on every other variable of each kind.  The code reads variable 0 only."""
    assert layout in GEN_LAYOUTS
    alternate = layout.endswith("alternate")
    s = P.Asm(f"widthgen:{layout}/base{base}", base, parents=alternate)
    s.p.seed = seed
    if layout.startswith("consts"):
        s.p.consts.extend(P.GEN_POOL)
    for w in WIDTHS:
        for j, kind in enumerate((ir.VK_GENERIC, ir.VK_VALUE)):
            k = 2 * (w - 1) + j
            parent = (P.GUARDS[k % 7] ^ (k * 0x0101_0101 << 96)) & ir.mask(w)
            s.var(w, parent, kind, parent=(w + j) % 2 == 0)
    s.p.emit(ir.W_VAR, 1, dst=base, aux0=0)
    s.cmp(ir.B_ULE, 1, 0, 0, 0)
    s.assert_(0)
    return s.done(verdict=None)


GEN_CANDS = tuple(range(256)) + (4095, 65535, 65536, (1 << 32) - 1)
GEN_SEEDS = (7, 0xDEADBEEF_00C0FFEE)
PIN_CANDS = (1, 63, 64, 65, 127)
PIN_BUDGET = 128
PIN_SEED = 0xDEADBEEF_00C0FFEE


def pin_cand(w):
    return PIN_CANDS[w % len(PIN_CANDS)]


def width_pin_set(w, target, base=0, seed=0):
    """One VK_GENERIC variable of width w, GEN_POOL plus the target as constant 8; ASSERT the
    variable equals the target."""
    s = P.Asm(f"widthpin:w{w}/base{base}", base, parents=False)
    s.p.seed = seed
    s.p.consts.extend(P.GEN_POOL + [target & ir.mask(256)])
    s.var(w, None, ir.VK_GENERIC)
    s.p.emit(ir.W_VAR, w, dst=base, aux0=0)
    s.p.emit(ir.W_CONST, 256, dst=1 + base, aux0=8)
    s.cmp(ir.B_EQ, w, 0, 0, 1)
    s.assert_(0)
    return s.done(verdict=None)


def width_pin_set_at(w, base=0, gseed=PIN_SEED):
    """width_pin_set whose target is the oracle's value of the variable at candidate
    pin_cand(w), by op_programs.pin_set_at's method: the target sits in the pool the generator's
    constant arm reads, so it is placed and the value recomputed until both agree."""
    import numpy as np
    import pyoracle as O

    start = PIN_CANDS.index(pin_cand(w))
    for k in PIN_CANDS[start:] + PIN_CANDS[:start]:    # a candidate that draws constant 8 +- 1
        target = 0                                      # never agrees: the next one then
        for _ in range(4):
            p = width_pin_set(w, target, base, seed=0x9E37 + w)
            sv = O.SetView.from_batch(ir.Batch([p]), 0)
            got = sv.gen_assignments(np.array([k], dtype=np.uint64), gseed)[0][0]
            if got == target:
                p.target, p.cand = target, k
                return p
            target = got
    raise AssertionError(f"width_pin_set_at({w}): no stable target")


# ---- samples ----------------------------------------------------------------------------------

def gate_sample_widths():
    """The widths w = 0, 1, 31 (mod 32) and one more per top limb: 24 + 8 widths."""
    out = {w for w in WIDTHS if w % 32 in (0, 1, 31)}
    out |= {32 * limb + 13 for limb in range(8)}
    return tuple(sorted(out))
