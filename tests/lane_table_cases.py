"""A chosen 64-lane wave in front of the kernels that generate their own candidates: the
lane-table protocol (no GPU needed to import).

The search, census and climb kernels draw every candidate from the generator, so a test cannot
hand them 64 operand pairs.  The wave is built inside the program instead, from a selector the
oracle can predict.  A lane-table set has two variables:

* ``k``: VK_SMALL, width 8, hint0 = K - 1 — an index into a table of K operand pairs;
* ``t``: a VK_KECCAK tag below 2^124 (117 random bits over a small base), different in every
  candidate with overwhelming probability (asserted for every seed used here).

The program selects ``a = T_a[k]`` and ``b = T_b[k]`` by a chain of B_EQ(k, i) / W_ITE over
constants, computes ``r = op(a, b)`` and asserts ``(r XOR t) == E`` (UMUL_NOOVF: ``(bit ? t :
NOT t) == E``).  Under a set seed S and the global seed G, lane j of the first wave holds the
known pair (k_j, t_j); set j of an entry carries E_j = op(T[k_j]) XOR t_j.  All 64 sets of an
entry share S, so they see the same 64 candidates, and the tags differ, so lane j is the only
witness of set j: ``found[j] == j`` says lane j computed its own value while the other 63 lanes
computed theirs.  Every set also exists with one bit of E_j flipped: no witness.

T[0] is a wave's special lane; the committed seeds are those under which k == 0 in exactly one
lane, at position 0, 31, 32 or 63 (hint0 = 63 sends about half the lanes to 4 or 36 by the
generator's ABI-aligned arm, the rest are uniform).  For the statistical EXP waves the seeds are
those under which the case module's predicate holds for the 64 realised lanes.
tests/test_lane_table_cases.py checks all of that, and the expectations, on the CPU;
``find_seed`` is how the constants were found (never called by a test).

Every W register is in 0..6, so ``base=0`` runs the 8-register kernels and ``base=8`` the
16-register ones.  Batches are assembled as arrays (64 sets and their twins share one code
template and differ in one constant), not through ir.Program."""

import functools
import random
from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple

import div_trim_cases as D
import exp_chain_cases as XC
import exp_scale_cases as XS
import exp_series_cases as XR
import numpy as np
import products_cases as PC
import pyoracle as O

from mythril_amd import ir

G = 0x7AB1E_0F_1A4E5                 # the global seed of every lane-table run
TAG_BASE = 0x5EED_0000_0000          # constant 0: the tag's base; tags stay below 2^124
NOT_FOUND = 0xFFFFFFFF
LANES = 64
M256 = ir.mask(256)

# (k, t, a, b, scratch, result): "low" stays in the VGPR registers of the 8-register file;
# "lds" has an operand and the result in registers 5 and 6 (LDS in the narrow kernels, next to
# EXP's window table and the entry UMUL_NOOVF parks an operand in); "lds_b" the other operand
# and the tag
PLACEMENTS = {"low": (0, 1, 2, 3, 4, 2), "lds": (0, 1, 5, 2, 3, 6), "lds_b": (4, 6, 0, 5, 1, 5)}


# ---- references in Python's own integers (z3's conventions for a zero divisor) ---------------

def _signed(x, w):
    return x - (1 << w) if x >> (w - 1) else x


def py_udiv(a, b, w):
    return a // b if b else ir.mask(w)


def py_urem(a, b, w):
    return a % b if b else a


def py_sdiv(a, b, w):
    x, y = _signed(a, w), _signed(b, w)
    if y == 0:
        return (1 if x < 0 else -1) & ir.mask(w)
    q = abs(x) // abs(y)
    return (-q if (x < 0) != (y < 0) else q) & ir.mask(w)


def py_srem(a, b, w):
    x, y = _signed(a, w), _signed(b, w)
    if y == 0:
        return a
    r = abs(x) % abs(y)
    return (-r if x < 0 else r) & ir.mask(w)


def py_smod(a, b, w):
    x, y = _signed(a, w), _signed(b, w)
    return (x % y) & ir.mask(w) if y else a     # Python's % takes the divisor's sign, as bvsmod


def py_exp(b, e, w):
    return pow(b, e, 1 << w)


def py_mul(a, b, w):
    return (a * b) & ir.mask(w)


def py_umul_noovf(a, b, w):
    return a * b < 1 << w


OPS = {   # name: (opcode, the oracle's function, Python's)
    "udiv": (ir.W_UDIV, O.bvudiv, py_udiv), "urem": (ir.W_UREM, O.bvurem, py_urem),
    "sdiv": (ir.W_SDIV, O.bvsdiv, py_sdiv), "srem": (ir.W_SREM, O.bvsrem, py_srem),
    "smod": (ir.W_SMOD, O.bvsmod, py_smod), "exp": (ir.W_EXP, O.bvexp, py_exp),
    "mul": (ir.W_MUL, O.bvmul, py_mul), "umul_noovf": (ir.B_UMUL_NOOVF, O.umul_noovf, py_umul_noovf),
}


# ---- the generator's first wave under a set seed -----------------------------------------------

@functools.lru_cache(maxsize=None)
def lanes_of(seed, K, gseed=G):
    """(k_j, t_j) of candidates 0..63 of a lane-table set with set seed ``seed``."""
    cands = np.arange(LANES, dtype=np.uint64)
    ks = O.gen_values(cands, 0, (ir.VK_SMALL | 8 << 8, K - 1, 0, ir.NO_PARENT), [TAG_BASE], None, seed, gseed)
    ts = O.gen_values(cands, 1, (ir.VK_KECCAK | 256 << 8, 0, 0, ir.NO_PARENT), [TAG_BASE], None, seed, gseed)
    return tuple(ks), tuple(ts)


@dataclass
class Entry:
    """One catalogue entry: a wave (and the position of its special lane) under one op."""
    family: str
    wave: str
    pos: Optional[int]
    opname: str
    w: int
    table: List[Tuple[int, int]]                 # T: the operand pairs the program selects from
    check: Callable                              # check(model lanes, pos): asserts the wave's property
    model: Optional[List[Tuple[int, int]]] = None  # per table row, what check() is to see (signed ops:
    #                                                the magnitudes the divider gets); default: the row

    @property
    def id(self):
        return f"{self.family}-{self.wave}" + (f"-p{self.pos}" if self.pos is not None else f"-w{self.w}")

    @property
    def K(self):
        return len(self.table)

    @property
    def seed(self):
        return SEEDS[self.id]

    @property
    def op(self):
        return OPS[self.opname][0]

    def ks(self, seed=None):
        return lanes_of(self.seed if seed is None else seed, self.K)[0]

    def tags(self, seed=None):
        return lanes_of(self.seed if seed is None else seed, self.K)[1]

    def realised(self, seed=None):
        """The 64 operand pairs T[k_j] of the wave as the kernel meets it."""
        return [self.table[k] for k in self.ks(seed)]

    def seen(self, seed=None):
        rows = self.model or self.table
        return [rows[k] for k in self.ks(seed)]

    def results(self, which=1):
        """op(T[k_j]) per lane, by the oracle (which=1) or by Python's integers (which=2)."""
        fn = OPS[self.opname][which]
        return [fn(a, b, self.w) for a, b in self.realised()]

    def expectations(self):
        """E_j per lane."""
        out = []
        for r, t in zip(self.results(), self.tags()):
            if self.op == ir.B_UMUL_NOOVF:
                out.append(t if r else t ^ M256)
            else:
                out.append((int(r) ^ t) & M256)
        return out

    def twin_bit(self, j):
        return (5 * j + 1) % (256 if self.op == ir.B_UMUL_NOOVF else self.w)

    def holds_property(self, seed=None):
        """Does the wave realised under ``seed`` have what it is named for?  The special lane in
        exactly one lane and at its position, distinct tags, the case module's own assertion."""
        ks, ts = lanes_of(self.seed if seed is None else seed, self.K)
        if len(set(ts)) != LANES or max(ts) >> 124:
            return False
        if self.pos is not None and [j for j, k in enumerate(ks) if k == 0] != [self.pos]:
            return False
        try:
            ok = self.check(self.seen(seed), self.pos)
        except AssertionError:
            return False
        return ok is None or bool(ok)

    def describe(self, j):
        a, b = self.realised()[j]
        return f"{self.id} lane {j} k={self.ks()[j]} a={a:#x} b={b:#x} t={self.tags()[j]:#x}"


def find_seed(entry, start=0, limit=200000):
    """The first set seed >= start under which the entry's wave has its property."""
    for s in range(start, start + limit):
        if entry.holds_property(s):
            return s
    raise AssertionError(f"{entry.id}: no seed below {start + limit}; change K or the table")


# ---- the catalogue ----------------------------------------------------------------------------

def _aligned_apart(lanes):
    """A 64-row table from a 64-lane wave whose property is a balance between even and odd
    lanes: rows 36 and 37 change places, so the generator's two aligned indices, 4 and 36, fall
    on lanes of either kind."""
    t = list(lanes)
    t[36], t[37] = t[37], t[36]
    return t


def _div_entries():
    out = []
    for name in D.WAVES:
        others, special = D.wave_parts(name, 8)
        for pos in D.POSITIONS:
            for op in ("udiv", "urem"):
                out.append(Entry(op, name, pos, op, 256, [special] + others,
                                 functools.partial(_check_div, name, 8)))
        others, special = D.wave_parts(name, 6)
        rows = [special] + others
        for n, op in enumerate(("sdiv", "srem", "smod")):
            # signs of (a, b) rotate over the rows, as test_gpu_div_trim._rows applies them; the
            # operands are below 2^192, so the divider gets the magnitudes as built
            signed = [((-a if (i + n) & 1 else a) & M256, (-b if (i + n) & 2 else b) & M256)
                      for i, (a, b) in enumerate(rows)]
            for pos in D.POSITIONS:
                out.append(Entry(op, name, pos, op, 256, signed, functools.partial(_check_div, name, 6),
                                 model=rows))
    return out


def _check_div(name, nl, lanes, pos):
    D.check_wave(name, lanes, pos, nl)


def _check_products(name, lanes, pos):
    odd = PC.exp_class(*lanes[pos])
    assert lanes[pos] == PC.WAVES[name][1]
    assert odd not in {PC.exp_class(*p) for i, p in enumerate(lanes) if i != pos}, name


def _exp_entries():
    out = []
    for name in sorted(PC.WAVES):
        rest, odd = PC.WAVES[name]
        for pos in PC.POSITIONS:
            out.append(Entry("exp_products", name, pos, "exp", 256, [odd] + [rest(i) for i in range(1, 64)],
                             functools.partial(_check_products, name)))
    for w in (256, 200):
        for name in sorted(XC.WAVES):
            make, has = XC.WAVES[name]
            out.append(Entry("exp_chain", name, None, "exp", w, _aligned_apart(make(w)),
                             lambda lanes, pos, has=has: has(lanes)))
        out.append(Entry("exp_scale", "mixed", None, "exp", w, _aligned_apart(XS.mixed_wave(w)),
                         lambda lanes, pos: XS.is_mixed_wave(lanes) and XC.runs_series(lanes)))
        out.append(Entry("exp_series", "mixed", None, "exp", w, _aligned_apart(XR.mixed_wave(w)),
                         lambda lanes, pos: XS.is_mixed_wave(lanes) and XC.runs_series(lanes)))
    return out


def _carries(a, b):
    return bool(PC.carrying_columns(a, b) & {1, 2, 3, 4, 5})


def _check_mul(lanes, pos):
    kinds = [_carries(a, b) for a, b in lanes]
    # both kinds in numbers, side by side, and every carrying column in some lane
    assert min(sum(kinds), LANES - sum(kinds)) >= 16
    assert sum(x != y for x, y in zip(kinds, kinds[1:])) >= 16
    cols = set()
    for a, b in lanes:
        cols |= PC.carrying_columns(a, b)
    assert cols >= {1, 2, 3, 4, 5}


def _mul_entry():
    rows = PC.mul_rows()
    carry = [r for r in rows if _carries(*r)]
    plain = [r for r in rows if not PC.carrying_columns(*r) and r[0] and r[1]]
    assert len(carry) >= 6 and len(plain) >= 32
    step = len(plain) // 32
    # carrying rows at even indices below 32 and at odd ones from 32 on: the aligned indices 4
    # and 36 are one of each
    table = [(carry[(i // 2) % len(carry)] if (i % 2 == 0) != (i >= 32) else plain[(i // 2) * step])
             for i in range(64)]
    return [Entry("mul", "carry_alternating", None, "mul", 256, table, _check_mul)]


def _check_umul(lanes, pos):
    assert [j for j, (a, b) in enumerate(lanes) if a == 0 or b == 0] == [pos]
    over = [a * b >= 1 << 256 for j, (a, b) in enumerate(lanes) if j != pos]
    assert min(sum(over), len(over) - sum(over)) >= 16


def _umul_entries():
    rng = random.Random(0x0F10)
    table = [(0, rng.getrandbits(256))]
    for i in range(1, 64):
        if (i % 2 == 0) != (i >= 32):            # overflow
            table.append((rng.getrandbits(256) | 1 << 255, rng.getrandbits(200) | 2))
        elif i % 4 == 1:                         # the product just fits / just does not
            a = rng.getrandbits(128) | 1 << 127
            table.append((a, M256 // a))
        else:
            table.append((rng.getrandbits(140) | 1, rng.getrandbits(100) | 1))
    out = []
    for pos in D.POSITIONS:
        t = list(table)
        if pos in (31, 63):                      # the zero on the other side
            t[0] = (t[0][1], 0)
        out.append(Entry("umul_noovf", "lone_zero_operand", pos, "umul_noovf", 256, t, _check_umul))
    return out


@functools.lru_cache(maxsize=None)
def catalogue():
    return tuple(_div_entries() + _exp_entries() + _mul_entry() + _umul_entries())


FAMILIES = ("udiv", "urem", "sdiv", "srem", "smod", "exp_products", "exp_chain", "exp_scale", "exp_series",
            "mul", "umul_noovf")


def family(name):
    return [e for e in catalogue() if e.family == name]


def sample():
    """What the census and climb kernels get: positions 0 and 63 of every div and products
    wave, and the exp_chain waves."""
    return [e for e in catalogue()
            if e.family == "exp_chain" or (e.pos in (0, 63) and e.family in
                                           ("udiv", "urem", "sdiv", "srem", "smod", "exp_products"))]


# ---- programs ---------------------------------------------------------------------------------

def _words(op, w, dst=0, a=0, b=0, c=0, aux0=0):
    return ((op & 0xFF) | (w & 0x3FF) << 8, (dst & 0xFF) | (a & 0xFF) << 8 | (b & 0xFF) << 16 | (c & 0xFF) << 24,
            aux0 & 0xFFFFFFFF, 0)


def template(entry, placement, base):
    """(code words [n, 4], constants) of the entry's lane-table set; constant 1 is E (0 here).
    Constants: 0 the tag's base, 1 E, 2 + i the index i (i < K), then T_a, then T_b."""
    rk, rt, ra, rb, rs, rr = (r + base for r in PLACEMENTS[placement])
    K, w, op = entry.K, entry.w, entry.op
    c_idx, c_a, c_b = 2, 2 + K, 2 + 2 * K
    consts = [TAG_BASE, 0] + list(range(K)) + [a for a, _ in entry.table] + [b for _, b in entry.table]
    assert len(consts) <= 256                    # a folded constant's index sits in a register field
    code = [_words(ir.W_VAR, 8, dst=rk, aux0=0), _words(ir.W_VAR, 256, dst=rt, aux0=1),
            _words(ir.W_CONST, w, dst=ra, aux0=c_a), _words(ir.W_CONST, w, dst=rb, aux0=c_b)]
    for i in range(1, K):
        code += [_words(ir.W_CONST, 8, dst=rs, aux0=c_idx + i),
                 _words(ir.B_EQ, 8, dst=0, a=rk, b=rs),
                 _words(ir.W_CONST, w, dst=rs, aux0=c_a + i),
                 _words(ir.W_ITE, w, dst=ra, a=rs, b=ra, c=0),
                 _words(ir.W_CONST, w, dst=rs, aux0=c_b + i),
                 _words(ir.W_ITE, w, dst=rb, a=rs, b=rb, c=0)]
    if op == ir.B_UMUL_NOOVF:
        code += [_words(op, w, dst=1, a=ra, b=rb),
                 _words(ir.W_NOT, 256, dst=rs, a=rt),
                 _words(ir.W_ITE, 256, dst=rr, a=rt, b=rs, c=1)]
    else:
        code += [_words(op, w, dst=rr, a=ra, b=rb),
                 _words(ir.W_XOR, 256, dst=rr, a=rr, b=rt)]
    code += [_words(ir.W_CONST, 256, dst=rs, aux0=1),
             _words(ir.B_EQ, 256, dst=2, a=rr, b=rs),
             _words(ir.ASSERT, 1, a=2),
             _words(ir.END, 1)]
    words = np.asarray(code, dtype=np.uint32)
    words[:, 3] = ir._reach_cost_words(words)
    words[-1, 3] = 0
    return words, consts


def program(entry, placement, base, E=0):
    """One lane-table set as an ir.Program (validated): what ``batch`` packs 128 times."""
    words, consts = template(entry, placement, base)
    consts[1] = E
    p = ir.PackedProgram(words, consts, [ir.Var("k", 8, ir.VK_SMALL, entry.K - 1, 0),
                                         ir.Var("t", 256, ir.VK_KECCAK, 0, 0)], seed=entry.seed,
                         name=f"{entry.id}/{placement}/base{base}")
    p.validate()
    return p


class LaneBatch(ir.Batch):
    """An ir.Batch assembled from arrays: ``index[s]`` is (entry, lane, is the twin) of set s and
    ``want[s]`` the candidate the search must return for it."""

    def __init__(self, entries, placement, base, only=None):
        """``only``: the (lane, twin) pairs to keep of every entry — a failing set on its own."""
        self.programs = []
        code, consts, descs, self.index = [], [], [], []
        n_code = n_const = 0
        for e in entries:
            words, cs = template(e, placement, base)
            block = ir.limbs_array(cs)
            Es = e.expectations()
            for j in range(LANES):
                for twin in (False, True):
                    if only is not None and (j, twin) not in only:
                        continue
                    E = Es[j] ^ (1 << e.twin_bit(j)) if twin else Es[j]
                    mine = block.copy()
                    mine[1] = ir.to_limbs(E)
                    code.append(words)
                    consts.append(mine)
                    s = len(descs)
                    descs.append((n_code, len(words), n_const, len(cs), 2 * s, 2, e.seed & 0xFFFFFFFF, ir.NO_PARENT))
                    n_code += len(words)
                    n_const += len(cs)
                    self.index.append((e, j, twin))
        self.programs = [None] * len(descs)
        self.code = np.concatenate(code) if code else np.zeros((0, 4), dtype=np.uint32)
        self.consts = np.concatenate(consts) if consts else np.zeros((0, 8), dtype=np.uint32)
        ksch = {K: (ir.VK_SMALL | 8 << 8, K - 1, 0, ir.NO_PARENT) for K in {e.K for e in entries}}
        tsch = (ir.VK_KECCAK | 256 << 8, 0, 0, ir.NO_PARENT)
        self.schema = np.asarray([row for e, _, _ in self.index for row in (ksch[e.K], tsch)],
                                 dtype=np.uint32).reshape(-1, 4)
        self.parents = np.zeros((0, 8), dtype=np.uint32)
        self.descs = np.asarray(descs, dtype=np.uint32).reshape(-1, 8)
        self.want = np.array([NOT_FOUND if twin else j for _, j, twin in self.index], dtype=np.uint32)

    def describe(self, s):
        e, j, twin = self.index[s]
        return ("corrupted " if twin else "") + e.describe(j)


def surviving_compares(batch, s):
    """B_EQ at width 8 in the device program of set s: the table's compares the fold pass left."""
    from mythril_amd import _lib

    code, descs, _ = _lib.device_batch(batch.code, batch.consts, batch.descs)
    d = descs[s]
    rows = code[int(d[0]):int(d[0]) + int(d[1])]
    return int(np.sum(((rows[:, 0] & 0xFF) == ir.B_EQ) & (((rows[:, 0] >> 8) & 0x3FF) == 8)))


# ---- the committed seeds: find_seed(entry) for every entry of the catalogue ---------------------

SEEDS = {
    "udiv-bz_in_general-p0": 9, "urem-bz_in_general-p0": 9, "udiv-bz_in_general-p31": 129,
    "urem-bz_in_general-p31": 129, "udiv-bz_in_general-p32": 63, "urem-bz_in_general-p32": 63,
    "udiv-bz_in_general-p63": 487, "urem-bz_in_general-p63": 487, "sdiv-bz_in_general-p0": 9,
    "sdiv-bz_in_general-p31": 129, "sdiv-bz_in_general-p32": 63, "sdiv-bz_in_general-p63": 487,
    "srem-bz_in_general-p0": 9, "srem-bz_in_general-p31": 129, "srem-bz_in_general-p32": 63,
    "srem-bz_in_general-p63": 487, "smod-bz_in_general-p0": 9, "smod-bz_in_general-p31": 129,
    "smod-bz_in_general-p32": 63, "smod-bz_in_general-p63": 487, "udiv-lone_high_digit-p0": 9,
    "urem-lone_high_digit-p0": 9, "udiv-lone_high_digit-p31": 129, "urem-lone_high_digit-p31": 129,
    "udiv-lone_high_digit-p32": 63, "urem-lone_high_digit-p32": 63, "udiv-lone_high_digit-p63": 487,
    "urem-lone_high_digit-p63": 487, "sdiv-lone_high_digit-p0": 9, "sdiv-lone_high_digit-p31": 129,
    "sdiv-lone_high_digit-p32": 63, "sdiv-lone_high_digit-p63": 487, "srem-lone_high_digit-p0": 9,
    "srem-lone_high_digit-p31": 129, "srem-lone_high_digit-p32": 63, "srem-lone_high_digit-p63": 487,
    "smod-lone_high_digit-p0": 9, "smod-lone_high_digit-p31": 129, "smod-lone_high_digit-p32": 63,
    "smod-lone_high_digit-p63": 487, "udiv-lone_low_digit-p0": 9, "urem-lone_low_digit-p0": 9,
    "udiv-lone_low_digit-p31": 129, "urem-lone_low_digit-p31": 129, "udiv-lone_low_digit-p32": 63,
    "urem-lone_low_digit-p32": 63, "udiv-lone_low_digit-p63": 487, "urem-lone_low_digit-p63": 487,
    "sdiv-lone_low_digit-p0": 9, "sdiv-lone_low_digit-p31": 129, "sdiv-lone_low_digit-p32": 63,
    "sdiv-lone_low_digit-p63": 487, "srem-lone_low_digit-p0": 9, "srem-lone_low_digit-p31": 129,
    "srem-lone_low_digit-p32": 63, "srem-lone_low_digit-p63": 487, "smod-lone_low_digit-p0": 9,
    "smod-lone_low_digit-p31": 129, "smod-lone_low_digit-p32": 63, "smod-lone_low_digit-p63": 487,
    "udiv-lone_addback_onedigit-p0": 9, "urem-lone_addback_onedigit-p0": 9, "udiv-lone_addback_onedigit-p31": 129,
    "urem-lone_addback_onedigit-p31": 129, "udiv-lone_addback_onedigit-p32": 63, "urem-lone_addback_onedigit-p32": 63,
    "udiv-lone_addback_onedigit-p63": 487, "urem-lone_addback_onedigit-p63": 487, "sdiv-lone_addback_onedigit-p0": 9,
    "sdiv-lone_addback_onedigit-p31": 129, "sdiv-lone_addback_onedigit-p32": 63,
    "sdiv-lone_addback_onedigit-p63": 487, "srem-lone_addback_onedigit-p0": 9, "srem-lone_addback_onedigit-p31": 129,
    "srem-lone_addback_onedigit-p32": 63, "srem-lone_addback_onedigit-p63": 487, "smod-lone_addback_onedigit-p0": 9,
    "smod-lone_addback_onedigit-p31": 129, "smod-lone_addback_onedigit-p32": 63,
    "smod-lone_addback_onedigit-p63": 487, "udiv-lone_addback_general-p0": 9, "urem-lone_addback_general-p0": 9,
    "udiv-lone_addback_general-p31": 129, "urem-lone_addback_general-p31": 129, "udiv-lone_addback_general-p32": 63,
    "urem-lone_addback_general-p32": 63, "udiv-lone_addback_general-p63": 487, "urem-lone_addback_general-p63": 487,
    "sdiv-lone_addback_general-p0": 9, "sdiv-lone_addback_general-p31": 129, "sdiv-lone_addback_general-p32": 63,
    "sdiv-lone_addback_general-p63": 487, "srem-lone_addback_general-p0": 9, "srem-lone_addback_general-p31": 129,
    "srem-lone_addback_general-p32": 63, "srem-lone_addback_general-p63": 487, "smod-lone_addback_general-p0": 9,
    "smod-lone_addback_general-p31": 129, "smod-lone_addback_general-p32": 63, "smod-lone_addback_general-p63": 487,
    "udiv-bhigh_next_to_one_limb-p0": 9, "urem-bhigh_next_to_one_limb-p0": 9, "udiv-bhigh_next_to_one_limb-p31": 129,
    "urem-bhigh_next_to_one_limb-p31": 129, "udiv-bhigh_next_to_one_limb-p32": 63,
    "urem-bhigh_next_to_one_limb-p32": 63, "udiv-bhigh_next_to_one_limb-p63": 487,
    "urem-bhigh_next_to_one_limb-p63": 487, "sdiv-bhigh_next_to_one_limb-p0": 9,
    "sdiv-bhigh_next_to_one_limb-p31": 129, "sdiv-bhigh_next_to_one_limb-p32": 63,
    "sdiv-bhigh_next_to_one_limb-p63": 487, "srem-bhigh_next_to_one_limb-p0": 9,
    "srem-bhigh_next_to_one_limb-p31": 129, "srem-bhigh_next_to_one_limb-p32": 63,
    "srem-bhigh_next_to_one_limb-p63": 487, "smod-bhigh_next_to_one_limb-p0": 9,
    "smod-bhigh_next_to_one_limb-p31": 129, "smod-bhigh_next_to_one_limb-p32": 63,
    "smod-bhigh_next_to_one_limb-p63": 487, "udiv-zeros_and_one_general-p0": 9, "urem-zeros_and_one_general-p0": 9,
    "udiv-zeros_and_one_general-p31": 129, "urem-zeros_and_one_general-p31": 129,
    "udiv-zeros_and_one_general-p32": 63, "urem-zeros_and_one_general-p32": 63, "udiv-zeros_and_one_general-p63": 487,
    "urem-zeros_and_one_general-p63": 487, "sdiv-zeros_and_one_general-p0": 9, "sdiv-zeros_and_one_general-p31": 129,
    "sdiv-zeros_and_one_general-p32": 63, "sdiv-zeros_and_one_general-p63": 487, "srem-zeros_and_one_general-p0": 9,
    "srem-zeros_and_one_general-p31": 129, "srem-zeros_and_one_general-p32": 63,
    "srem-zeros_and_one_general-p63": 487, "smod-zeros_and_one_general-p0": 9, "smod-zeros_and_one_general-p31": 129,
    "smod-zeros_and_one_general-p32": 63, "smod-zeros_and_one_general-p63": 487, "udiv-q0_in_onedigit-p0": 9,
    "urem-q0_in_onedigit-p0": 9, "udiv-q0_in_onedigit-p31": 129, "urem-q0_in_onedigit-p31": 129,
    "udiv-q0_in_onedigit-p32": 63, "urem-q0_in_onedigit-p32": 63, "udiv-q0_in_onedigit-p63": 487,
    "urem-q0_in_onedigit-p63": 487, "sdiv-q0_in_onedigit-p0": 9, "sdiv-q0_in_onedigit-p31": 129,
    "sdiv-q0_in_onedigit-p32": 63, "sdiv-q0_in_onedigit-p63": 487, "srem-q0_in_onedigit-p0": 9,
    "srem-q0_in_onedigit-p31": 129, "srem-q0_in_onedigit-p32": 63, "srem-q0_in_onedigit-p63": 487,
    "smod-q0_in_onedigit-p0": 9, "smod-q0_in_onedigit-p31": 129, "smod-q0_in_onedigit-p32": 63,
    "smod-q0_in_onedigit-p63": 487, "exp_products-nb0_0_one_lane_1-p0": 9, "exp_products-nb0_0_one_lane_1-p31": 129,
    "exp_products-nb0_0_one_lane_1-p32": 63, "exp_products-nb0_0_one_lane_1-p63": 487,
    "exp_products-nb0_0_one_lane_8-p0": 9, "exp_products-nb0_0_one_lane_8-p31": 129,
    "exp_products-nb0_0_one_lane_8-p32": 63, "exp_products-nb0_0_one_lane_8-p63": 487,
    "exp_products-nb0_0_one_lane_series-p0": 9, "exp_products-nb0_0_one_lane_series-p31": 129,
    "exp_products-nb0_0_one_lane_series-p32": 63, "exp_products-nb0_0_one_lane_series-p63": 487,
    "exp_products-nb0_1_one_lane_0-p0": 9, "exp_products-nb0_1_one_lane_0-p31": 129,
    "exp_products-nb0_1_one_lane_0-p32": 63, "exp_products-nb0_1_one_lane_0-p63": 487,
    "exp_products-nb0_1_one_lane_2-p0": 9, "exp_products-nb0_1_one_lane_2-p31": 129,
    "exp_products-nb0_1_one_lane_2-p32": 63, "exp_products-nb0_1_one_lane_2-p63": 487,
    "exp_products-nb0_1_one_lane_series-p0": 9, "exp_products-nb0_1_one_lane_series-p31": 129,
    "exp_products-nb0_1_one_lane_series-p32": 63, "exp_products-nb0_1_one_lane_series-p63": 487,
    "exp_products-nb0_2_one_lane_series-p0": 9, "exp_products-nb0_2_one_lane_series-p31": 129,
    "exp_products-nb0_2_one_lane_series-p32": 63, "exp_products-nb0_2_one_lane_series-p63": 487,
    "exp_products-series_nb0_0_one_lane_1-p0": 9, "exp_products-series_nb0_0_one_lane_1-p31": 129,
    "exp_products-series_nb0_0_one_lane_1-p32": 63, "exp_products-series_nb0_0_one_lane_1-p63": 487,
    "exp_products-series_nb0_0_one_lane_even-p0": 9, "exp_products-series_nb0_0_one_lane_even-p31": 129,
    "exp_products-series_nb0_0_one_lane_even-p32": 63, "exp_products-series_nb0_0_one_lane_even-p63": 487,
    "exp_products-series_nb0_0_one_lane_n0-p0": 9, "exp_products-series_nb0_0_one_lane_n0-p31": 129,
    "exp_products-series_nb0_0_one_lane_n0-p32": 63, "exp_products-series_nb0_0_one_lane_n0-p63": 487,
    "exp_products-series_nb0_1_one_lane_2-p0": 9, "exp_products-series_nb0_1_one_lane_2-p31": 129,
    "exp_products-series_nb0_1_one_lane_2-p32": 63, "exp_products-series_nb0_1_one_lane_2-p63": 487,
    "exp_products-series_nb0_8_one_lane_0-p0": 9, "exp_products-series_nb0_8_one_lane_0-p31": 129,
    "exp_products-series_nb0_8_one_lane_0-p32": 63, "exp_products-series_nb0_8_one_lane_0-p63": 487,
    "exp_chain-bits_3_6_clear-w256": 0, "exp_chain-mixed-w256": 450, "exp_chain-no_series_even-w256": 0,
    "exp_chain-no_series_n0-w256": 0, "exp_chain-short_e0-w256": 0, "exp_scale-mixed-w256": 0,
    "exp_series-mixed-w256": 0, "exp_chain-bits_3_6_clear-w200": 0, "exp_chain-mixed-w200": 450,
    "exp_chain-no_series_even-w200": 0, "exp_chain-no_series_n0-w200": 0, "exp_chain-short_e0-w200": 0,
    "exp_scale-mixed-w200": 0, "exp_series-mixed-w200": 0, "mul-carry_alternating-w256": 0,
    "umul_noovf-lone_zero_operand-p0": 9, "umul_noovf-lone_zero_operand-p31": 129,
    "umul_noovf-lone_zero_operand-p32": 63, "umul_noovf-lone_zero_operand-p63": 487,
}
