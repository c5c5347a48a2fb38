"""Test tooling (not a test; no GPU needed to import): programs for the Bool register file.

The 32 B registers are the bits of one VGPR in ``run_program`` (mythril_amd/csrc/pf_eval.hip),
and a spilled Bool is word 0 of a private-scratch slot or of LDS window-table entry 1..3
(``lds_spill_slots``, pf_devprog.h).  Two families:

* ``bool_pressure_dag`` — a DAG with more than 32 live Bool values, none of them cheap to
  recompute, so ``lower()`` itself emits B_SPILL / B_FILL;
* hand-emitted programs over ``op_programs.Asm`` where the test chooses the B registers and the
  spill slots: ``bfile_set`` (one B op between full B files), ``bspill_set`` (spills to chosen
  slots next to live W guards) and ``fused_set`` (ASSERTs that ``fuse_asserts`` moves, or does
  not move, to the last writer of their register).

The hand-emitted programs read the whole B file out into one 32-bit word — 32 W_ITE, one per
register, each selecting 2^r or 0, summed — and assert that it equals the W variable
``expect``: every candidate carries its own expected word, so 64 lanes with 64 different files
are checked by one program.  A builder called again with another ``word`` gives that
candidate's assignment (``.assignment``) and verdict (``.verdict``); the variable order does
not depend on the values.  tests/test_bool_file_cases.py checks the builders' bookkeeping
against the oracles on the CPU."""

import random

import op_programs as P
import pyoracle as O

from mythril_amd import ir
from mythril_amd.lower import Dag

M32 = ir.mask(32)


# ---- a. more than 32 live Bool values through lower() -------------------------------------

PRESSURE_VARS = 6
_C0 = 0x9E3779B97F4A7C15F39CC0605CEDC8341082276BF3A27251F86C6A11D0C18E95


def bool_pressure_dag(n, clobber=False, root="free", rare=0):
    """b_i = ULT(y_a * y_b + c_i, y_c) over six 256-bit variables, i < n: a compare behind a
    product is not rematerialised, so past 32 live values the lowering spills.  The b_i are
    consumed by two XOR chains, f in forward and r in reverse order (every b_i stays live
    until r reaches it).  ``clobber`` XORs a compare behind a W_EXP and a B_UMUL_NOOVF into
    r near its end — the spill segments still open there cross them — and equal-valued
    compares built without those ops (y^3 by two products, the overflow test with its
    operands swapped) into f.

    ``root="free"``: ASSERT ((sel ? f : r) ^ t) & q_1 .. q_rare with free VK_BOOL variables
    sel, t, q_j — f and r do not cancel, every b_i decides the verdict on either side of
    sel, and about 2^-(1 + rare) of all candidates hold.  ``root="identity"``: ASSERT f ^ r,
    which is false for every assignment — a single wrong bit in either chain is a witness."""
    assert root in ("free", "identity")
    dag = Dag()
    y = [dag.var(f"y{k}", 256) for k in range(PRESSURE_VARS)]

    def bit(i):
        a, b, c = i % 6, (i // 6 + i + 1) % 6, (i + 3) % 6
        prod = dag.op(ir.W_MUL, 256, y[a], y[b])
        return dag.op(ir.B_ULT, 256, dag.op(ir.W_ADD, 256, prod, dag.const(_C0 * (2 * i + 1), 256)), y[c])

    b = [bit(i) for i in range(n)]
    f = b[0]
    for i in range(1, n):
        f = dag.op(ir.B_XOR, 1, f, b[i])
    lo = [dag.op(ir.W_LSHR, 256, y[2], dag.const(127, 256)), dag.op(ir.W_LSHR, 256, y[3], dag.const(128, 256))]
    if clobber:
        cube = dag.op(ir.W_MUL, 256, dag.op(ir.W_MUL, 256, y[0], y[0]), y[0])
        f = dag.op(ir.B_XOR, 1, f, dag.op(ir.B_ULT, 256, cube, y[1]))
        f = dag.op(ir.B_XOR, 1, f, dag.op(ir.B_UMUL_NOOVF, 256, lo[1], lo[0]))
    r = b[n - 1]
    for i in range(n - 2, -1, -1):
        if clobber and i == n // 4:
            r = dag.op(ir.B_XOR, 1, r, dag.op(ir.B_ULT, 256, dag.op(ir.W_EXP, 256, y[0], dag.const(3, 256)), y[1]))
        if clobber and i == n // 8:
            r = dag.op(ir.B_XOR, 1, r, dag.op(ir.B_UMUL_NOOVF, 256, lo[0], lo[1]))
        r = dag.op(ir.B_XOR, 1, r, b[i])
    if root == "identity":
        dag.assert_(dag.op(ir.B_XOR, 1, f, r))
        return dag
    sel, t = dag.var("sel", 1, ir.VK_BOOL), dag.var("t", 1, ir.VK_BOOL)
    out = dag.op(ir.B_XOR, 1, dag.op(ir.B_ITE, 1, sel, f, r), t)
    for j in range(rare):
        out = dag.op(ir.B_AND, 1, out, dag.var(f"q{j}", 1, ir.VK_BOOL))
    dag.assert_(out)
    return dag


def pressure_values(dag, rng):
    """One random assignment of a pressure DAG's variables."""
    return [rng.getrandbits(v.width) for v in dag.vars]


# ---- b. hand-emitted programs ----------------------------------------------------------------

class BAsm(P.Asm):
    """Asm that keeps the B file's contents (``bits``) and the spill slots' as it emits."""

    def __init__(self, name, base=0, parents=True):
        super().__init__(name, base, parents)
        self.bits = [None] * ir.NB
        self.slots = {}

    def load_file(self, word):
        """All 32 B registers from 32 VK_BOOL variables: register r = bit r of ``word``."""
        for r in range(ir.NB):
            self.bload(r, (word >> r) & 1)

    def bload(self, r, v):
        self.bvar(r, v)
        self.bits[r] = int(bool(v))

    def bop(self, op, rd, ra=0, rb=0, rc=0, aux0=0):
        g = self.bits
        v = {ir.B_AND: lambda: g[ra] & g[rb], ir.B_OR: lambda: g[ra] | g[rb], ir.B_XOR: lambda: g[ra] ^ g[rb],
             ir.B_NOT: lambda: g[ra] ^ 1, ir.B_ITE: lambda: g[ra] if g[rc] else g[rb],
             ir.B_CONST: lambda: aux0 & 1}[op]()
        self.b(op, rd, a=ra, b=rb, c=rc, aux0=aux0)
        g[rd] = v

    def bcmp(self, op, w, rd, ra, rb, a, b):
        """B[rd] <- cmp(W[ra], W[rb]); a, b are the registers' values."""
        self.cmp(op, w, rd, ra, rb)
        self.bits[rd] = int(bool(O._BCMP[op](a, b, w)))

    def bspill(self, r, slot):
        self.b(ir.B_SPILL, 0, a=r, aux0=slot)
        self.slots[slot] = self.bits[r]

    def bfill(self, r, slot):
        self.b(ir.B_FILL, r, aux0=slot)
        self.bits[r] = self.slots[slot]

    def word(self):
        return sum(v << r for r, v in enumerate(self.bits))

    def readout(self, wrong=None, acc0=None, checks=()):
        """W0 <- acc0 (a value already in W0, or 0) + the B file as a word, through 32 W_ITE
        in registers 1..3; then ``checks`` ((register, value) pairs, compared with constants)
        and ASSERT W0 == the W variable ``expect``: the right word, or with bit ``wrong``
        flipped.  The B file is free once it is read, so the compares write B 0..."""
        if acc0 is None:
            self.wconst(0, 32, 0)
        self.wconst(2, 32, 0)
        for r in range(ir.NB):
            self.wconst(1, 32, 1 << r)
            self.w(ir.W_ITE, 32, 3, 1, 2, c=r)
            self.w(ir.W_ADD, 32, 0, 0, 3)
        expect = ((acc0 or 0) + self.word()) & M32
        if wrong is not None:
            expect ^= 1 << wrong
        for k, (reg, value) in enumerate(checks):
            self.assert_eq(256, reg, value, 1, bd=1 + k)
        self.wvar(1, 32, expect)
        self.cmp(ir.B_EQ, 32, 0, 0, 1)
        self.p.emit(ir.ASSERT, 1, a=0)
        return self.done(wrong is None)


BFILE_OPS = (ir.B_AND, ir.B_OR, ir.B_XOR, ir.B_NOT, ir.B_ITE, ir.B_CONST, ir.B_ULT, ir.B_EQ)


def bfile_set(op, ra, rb, rc, rd, word, base=0, parents=True, wrong=None):
    """The B-file analogue of op_programs.slot_set: all 32 B registers loaded, one B op with
    the chosen registers (B_CONST: the constant is ra & 1; a compare: 64-bit W variables
    derived from ``word`` in W0, W1, result in B[rd]), the whole file read out."""
    s = BAsm(f"bfile:{ir.OPNAMES[op]}/a{ra}/b{rb}/c{rc}/d{rd}/base{base}", base, parents)
    s.load_file(word)
    if op in ir.B_CMP:
        a = (word * 0x9E3779B97F4A7C15) & ir.mask(64)
        b = a if (op == ir.B_EQ and (word >> ((rd + 1) % 32)) & 1) else ((word ^ 0x5DEECE66D) * 0xD1B54A32D192ED03) & ir.mask(64)
        s.wvar(0, 64, a)
        s.wvar(1, 64, b)
        s.bcmp(op, 64, rd, 0, 1, a, b)
    elif op == ir.B_CONST:
        s.bop(op, rd, aux0=ra & 1)
    else:
        s.bop(op, rd, ra, rb, rc)
    return s.readout(wrong)


def bfile_result_differs(op, ra, rb, rc, rd, word):
    """Does the op change B[rd] under ``word``?  (A lost write shows only then.)"""
    p = bfile_set(op, ra, rb, rc, rd, word)
    return p.assignment[-1] != word


def bfile_tuples(op, base=0):
    """(ra, rb, rc, rd): every rd of 0..31 with sources elsewhere, rd equal to each source,
    and for B_ITE the condition register ranging over the file; a sample at base 8."""
    out = [((rd + 5) % 32, (rd + 11) % 32, (rd + 17) % 32, rd) for rd in range(32)]
    for r in (0, 1, 15, 30, 31):
        out.append((r, (r + 3) % 32, (r + 9) % 32, r))          # rd == ra
        if op in ir.B_LOGIC or op == ir.B_ITE:
            out.append(((r + 3) % 32, r, (r + 9) % 32, r))      # rd == rb
            out.append((r, r, (r + 9) % 32, (r + 1) % 32))      # ra == rb
        if op == ir.B_ITE:
            out.append(((r + 3) % 32, (r + 9) % 32, r, r))      # rd == rc
    if op == ir.B_ITE:
        out += [((rc + 1) % 32, (rc + 2) % 32, rc, (rc + 3) % 32) for rc in range(32)]
    if base:
        out = out[::7] + out[-3:] + (out[-32::5] if op == ir.B_ITE else [])
    return out


def bfile_word(op, ra, rb, rc, rd, seed):
    """A file under which the op changes B[rd] and, for B_ITE, the two arms differ (the
    condition then decides the result)."""
    rng = random.Random(seed)
    for _ in range(256):
        word = rng.getrandbits(32)
        arms = op != ir.B_ITE or ra == rb or (word >> ra) & 1 != (word >> rb) & 1
        if arms and bfile_result_differs(op, ra, rb, rc, rd, word):
            return word
    raise AssertionError(f"no file for {ir.OPNAMES[op]} {(ra, rb, rc, rd)}")


SPILL_REGS = (0, 31, 7, 16, 13)
SPILL_SLOTS = (0, 63, 7, 21, 40)          # 7: written by a W_SPILL before
SPILL_VARIANTS = ("plain", "exp", "umul")
_EXP_A, _EXP_B = P.GUARDS[1] | 1, P.GUARDS[2]
_UMUL_A, _UMUL_B = P.GUARDS[3] >> 129, P.GUARDS[4] >> 128


def bspill_set(variant, word, base=0, parents=True, wrong=None, rot=0):
    """Guards in W5, W6 (the narrow kernels' LDS registers, next to the LDS spill entries) and
    a W value through spill slot 7; the B file loaded; five B registers spilled to slots 0,
    63, 7, 21 and 40 (``rot`` rotates which register goes where, and with it which of them
    the device program moves to LDS: the first three in program order), complemented in
    place, then — ``variant`` — nothing, a W_EXP or a B_UMUL_NOOVF (result in B20), and
    filled back in reverse order, each slot into the next register of the list.  The
    readout also carries EXP's low word, and the guards and the W value are compared."""
    assert variant in SPILL_VARIANTS
    k = len(SPILL_REGS)
    regs = [SPILL_REGS[(i + rot) % k] for i in range(k)]
    slots = [SPILL_SLOTS[(i + 2 * rot) % k] for i in range(k)]
    s = BAsm(f"bspill:{variant}/rot{rot}/base{base}", base, parents)
    s.wvar(5, 256, P.GUARDS[5])
    s.wvar(6, 256, P.GUARDS[6])
    s.wvar(0, 256, P.GUARDS[0])
    s.w(ir.W_SPILL, 256, 0, 0, aux0=7)
    s.load_file(word)
    s.w(ir.W_FILL, 256, 4, aux0=7)
    for r, slot in zip(regs, slots):
        s.bspill(r, slot)
    for r in regs:
        s.bop(ir.B_NOT, r, r)
    acc0 = None
    if variant == "exp":
        s.wvar(1, 256, _EXP_A)
        s.wvar(2, 256, _EXP_B)
        s.w(ir.W_EXP, 256, 3, 1, 2)
        s.w(ir.W_EXTRACT, 32, 0, 3, aux0=0)
        acc0 = O.bvexp(_EXP_A, _EXP_B, 256) & M32
    elif variant == "umul":
        s.wvar(1, 256, _UMUL_A)
        s.wvar(2, 256, _UMUL_B)
        s.bcmp(ir.B_UMUL_NOOVF, 256, 20, 1, 2, _UMUL_A, _UMUL_B)
    for i in reversed(range(k)):
        s.bfill(regs[(i + 1) % k], slots[i])
    return s.readout(wrong, acc0, checks=((4, P.GUARDS[0]), (5, P.GUARDS[5]), (6, P.GUARDS[6])))


FUSED_KINDS = ("far", "fill", "var", "umul")
FUSED_BOOLS = 4


def fused_values(rng):
    """Four Bool values and two 64-bit operands whose product overflows about half the time."""
    return [rng.getrandbits(1) for _ in range(FUSED_BOOLS)] + [rng.getrandbits(33), rng.getrandbits(32)]


def fused_set(kind, values, base=0, parents=True):
    """Two ASSERTs each, the first several instructions after the last writer of its register:
    ``far`` a B_XOR (fuse_asserts moves the ASSERT onto it), ``fill`` a B_FILL (likewise),
    ``var`` a B_VAR and ``umul`` a B_UMUL_NOOVF (neither is fused: the plain ASSERT stays).
    The second ASSERT, of B2 | B3 through two B_NOTs, keeps the instructions in between
    alive.  ``verdict`` follows from ``values`` (fused_values)."""
    assert kind in FUSED_KINDS
    v, (x, y) = values[:FUSED_BOOLS], values[FUSED_BOOLS:]
    s = BAsm(f"fused:{kind}/base{base}", base, parents)
    for r in range(FUSED_BOOLS):
        s.bload(r, v[r])
    s.wvar(0, 64, x)
    s.wvar(1, 64, y)
    if kind == "far":
        s.bop(ir.B_XOR, 4, 0, 1)
    elif kind == "fill":
        s.bop(ir.B_XOR, 4, 0, 1)
        s.bspill(4, 5)
        s.bop(ir.B_NOT, 4, 4)
        s.bfill(4, 5)
    elif kind == "var":
        s.bload(4, v[0] ^ v[1])                      # a fifth variable
    else:
        s.bcmp(ir.B_UMUL_NOOVF, 64, 4, 0, 1, x, y)
    s.bop(ir.B_OR, 5, 2, 3)
    s.w(ir.W_ADD, 64, 2, 0, 1)
    s.bop(ir.B_NOT, 6, 5)
    s.bop(ir.B_NOT, 6, 6)
    s.p.emit(ir.ASSERT, 1, a=4)
    s.p.emit(ir.ASSERT, 1, a=6)
    return s.done(bool(s.bits[4] and s.bits[6]))


def fused_all(base=0):
    """The four kinds' first ASSERTs in one program without parents (the climb's scores then
    move in steps of PF_CLIMB_HOLDS over four sites)."""
    s = BAsm(f"fused:all/base{base}", base, parents=False)
    for r in range(6):
        s.bload(r, None)
    s.wvar(0, 64, None)
    s.wvar(1, 64, None)
    s.b(ir.B_XOR, 8, a=0, b=1)                       # far
    s.b(ir.B_OR, 9, a=2, b=3)
    s.b(ir.B_SPILL, 0, a=9, aux0=5)
    s.b(ir.B_NOT, 9, a=9)
    s.b(ir.B_FILL, 9, aux0=5)                        # fill
    s.cmp(ir.B_UMUL_NOOVF, 64, 10, 0, 1)             # umul: not fused
    s.b(ir.B_ITE, 11, a=4, b=5, c=8)
    for r in (8, 9, 10, 4, 11):                      # 4: a B_VAR, not fused
        s.p.emit(ir.ASSERT, 1, a=r)
    return s.done(verdict=None)


# ---- c. what the CPU checks and the GPU runs: the same programs, the same candidates ----------

def explicit(make, n, seed):
    """n candidates of one program: ``make(rng)`` builds it under values of rng's choosing.
    -> (the program, the assignments, the builder's verdicts)."""
    rng = random.Random(seed)
    progs = [make(rng) for _ in range(n)]
    return progs[0], [p.assignment for p in progs], [bool(p.verdict) for p in progs]


def _wrong(rng):
    """No corruption, or a bit of the expected word to flip: half of the candidates hold."""
    return rng.randrange(32) if rng.getrandbits(1) else None


def soa_cases():
    """(name, make) of every hand-emitted set that takes explicit candidates, without
    parents: per B op the tuples with rd = 31, rd = 0, rd a source and (B_ITE) the condition
    in B31 and B0; every spill variant at both bases and two rotations; every fused kind."""
    out = []
    for op in BFILE_OPS:
        tuples = bfile_tuples(op)
        picks = [tuples[31], tuples[0], tuples[32], tuples[-1]] + ([tuples[-32]] if op == ir.B_ITE else [])
        for base, (ra, rb, rc, rd) in zip((0, 8, 0, 8, 0), picks):
            out.append((f"bfile:{ir.OPNAMES[op]}/{ra}.{rb}.{rc}.{rd}/base{base}",
                        lambda rng, a=(op, ra, rb, rc, rd), base=base:
                        bfile_set(*a, rng.getrandbits(32), base=base, parents=False, wrong=_wrong(rng))))
    for variant in SPILL_VARIANTS:
        for base in (0, 8):
            for rot in (0, 1):
                out.append((f"bspill:{variant}/rot{rot}/base{base}",
                            lambda rng, a=(variant, base, rot):
                            bspill_set(a[0], rng.getrandbits(32), base=a[1], parents=False, wrong=_wrong(rng),
                                       rot=a[2])))
    for kind in FUSED_KINDS:
        for base in (0, 8):
            out.append((f"fused:{kind}/base{base}",
                        lambda rng, a=(kind, base): fused_set(a[0], fused_values(rng), base=a[1], parents=False)))
    return out


# name -> (n, clobber, root, rare, nw): nw = 7 runs the narrow kernels, W registers 5 and 6
# live next to the LDS entries; 15 the r16 kernels
PRESSURE = {
    "p40/free/r16": (40, False, "free", 5, 15),
    "p40/identity/r16": (40, False, "identity", 0, 15),
    "p64x/free/r16": (64, True, "free", 5, 15),
    "p64x/identity/r16": (64, True, "identity", 0, 15),
    "p40/free/narrow": (40, False, "free", 5, 7),
    "p40/identity/narrow": (40, False, "identity", 0, 7),
    "p90x/free/narrow": (90, True, "free", 5, 7),
    "p90x/identity/narrow": (90, True, "identity", 0, 7),
}


def pressure_program(name, rare=None):
    """The named pressure DAG (``rare`` overrides its count of extra free Bools) and its
    program as lower() emits it."""
    from mythril_amd.lower import lower

    n, clobber, root, r, nw = PRESSURE[name]
    dag = bool_pressure_dag(n, clobber, root, r if rare is None else rare)
    return dag, lower(dag, seed=len(name), name=name, nw=nw)


_SOA = None


def explicit_case(name, n):
    """explicit() of the named soa case under the seed every test uses for it."""
    global _SOA
    if _SOA is None:
        _SOA = dict(soa_cases())
    return explicit(_SOA[name], n, seed=len(name) * 7919 + n)


def pressure_explicit(name, n):
    """(dag, program, n random assignments) of the rare = 0 form of a named pressure program
    (the same code but for the q_j)."""
    dag, prog = pressure_program(name, rare=0)
    rng = random.Random(len(name) + n)
    return dag, prog, [pressure_values(dag, rng) for _ in range(n)]


def fused_rows(kind, base=0):
    """Candidate-0 forms of a fused set: one that holds, one whose first ASSERT fails and one
    whose second fails."""
    rng = random.Random(FUSED_KINDS.index(kind))
    while True:
        values = fused_values(rng)
        if fused_set(kind, values).verdict:
            break
    first = list(values)
    if kind == "umul":
        first[FUSED_BOOLS:] = [ir.mask(64), 3]                 # the product overflows
    else:
        first[0] ^= 1
    second = list(values)
    second[2] = second[3] = 0
    out = [fused_set(kind, v, base=base) for v in (values, first, second)]
    assert [p.verdict for p in out] == [True, False, False]
    return out


# ---- d. what the search tests upload -------------------------------------------------------------

FOLD_MIN_SETS = 16        # PF_FOLD_MIN_SETS (pf_devprog.h): pf_batch_create folds larger batches only
CHUNK = 12                # sets per upload that the fold pass must leave alone
BUDGET, GSEED = 1024, 0xB001_F11E     # the pressure programs' search


def bfile_rows(op, base):
    """Candidate-0 groups of the slot sets of one op: per tuple (and, for B_ITE, per two files:
    both values of the condition, mostly) the program that holds and two corrupted copies —
    one expects the old bit in rd, one a flipped bit elsewhere."""
    out = []
    for k, (ra, rb, rc, rd) in enumerate(bfile_tuples(op, base)):
        for seed in (k, 1000 + k) if op == ir.B_ITE else (k,):
            word = bfile_word(op, ra, rb, rc, rd, seed)
            out.append([bfile_set(op, ra, rb, rc, rd, word, base=base, wrong=w) for w in (None, rd, (rd + 13) % 32)])
    return out


def bspill_rows(base):
    """Candidate-0 groups of the spill sets: every variant, every rotation of registers over
    slots, each next to two corrupted copies."""
    out = []
    for variant in SPILL_VARIANTS:
        for rot in range(len(SPILL_REGS)):
            word = 0x5A5A_C33C ^ (0x0101_0101 * rot) ^ (0xFFFF_0000 if variant == "exp" else 0)
            out.append([bspill_set(variant, word, base=base, rot=rot, wrong=w) for w in (None, SPILL_REGS[rot], 31 - rot)])
    return out


def chunks(items, n=CHUNK):
    return [items[i:i + n] for i in range(0, len(items), n)]
