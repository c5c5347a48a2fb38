"""Hand-emitted single-operation programs for the search kernels (no GPU needed to import).

The per-operation parity tests of test_gpu_parity.py go through ``engine.eval_assignments``:
the SoA kernel, ``run_program<MODE_SOA, 16>``.  A search runs ``run_program<MODE_GEN, 8>``
(pf_check_kernel / pf_check_early_kernel) or ``<MODE_GEN, 16>`` (the r16 pair).  The builders
here put one explicit assignment in front of those kernels by the candidate-0 protocol:

* every variable carries ``parent=<value>`` and candidate 0 is the exact parent value
  (include/pf_bytecode.h), so a search with ``budget=1`` evaluates the program under exactly
  that assignment in lane 0 (a one-candidate search takes no probe launch);
* ``found[s] == 0`` iff the program holds under it, ``0xFFFFFFFF`` otherwise.

Programs are built with ``ir.Program.emit`` so the test, not ``lower()``, chooses register
numbers and instruction order.  ``base=8`` adds 8 to every W register: the set then writes a
register >= PF_NW_NARROW and runs the 16-register search kernels.

Every builder returns a Program with two extra attributes: ``verdict`` (what the caller said
the program evaluates to under its assignment) and ``assignment`` (the variable values, for
``parents=False`` sets that are evaluated with explicit candidates instead).

bool_file_cases.py builds on ``Asm`` for the Bool side: the B register file, B spills and
asserts fused into B-unit ops (test_bool_file_cases.py, test_gpu_bool_file.py)."""

from mythril_amd import ir

B_SCRATCH = 31     # B register of the negation of a compare expected to be false
GUARDS = tuple((0x9E3779B97F4A7C15F39CC0605CEDC834 * (2 * k + 3) ** 5 + (k << 250)) & ir.mask(256) | 1 << 255
               for k in range(7))


class Asm:
    """A Program under construction; W register numbers are offset by ``base``."""

    def __init__(self, name, base=0, parents=True):
        self.p = ir.Program(name=name)
        self.base = base
        self.parents = parents
        self.values = []

    def var(self, width, value, kind=ir.VK_GENERIC, hint0=0, hint1=0, parent=True):
        """A schema entry; its index.  ``value`` is the parent (candidate-0) value."""
        keep = self.parents and parent and value is not None
        self.p.vars.append(ir.Var(f"v{len(self.p.vars)}", width, kind, hint0, hint1,
                                  value if keep else None))
        self.values.append(0 if value is None else value & ir.mask(width))
        return len(self.p.vars) - 1

    def wvar(self, reg, width, value, **kw):
        self.p.emit(ir.W_VAR, width, dst=reg + self.base, aux0=self.var(width, value, **kw))

    def wconst(self, reg, width, value):
        self.p.emit(ir.W_CONST, width, dst=reg + self.base, aux0=self.p.const_index(value))

    def w(self, op, width, d, a=0, b=0, c=0, aux0=0):
        """A W-result op: d, a, b are W registers (b only where the op reads one), c a B one."""
        two = op in ir.W_BINARY or op in (ir.W_CONCAT, ir.W_ITE)
        self.p.emit(op, width, dst=d + self.base, a=a + self.base, b=b + self.base if two else 0,
                    c=c, aux0=aux0)

    def cmp(self, op, width, bd, a, b):
        self.p.emit(op, width, dst=bd, a=a + self.base, b=b + self.base)

    def bvar(self, bd, value):
        self.p.emit(ir.B_VAR, 1, dst=bd, aux0=self.var(1, int(bool(value)), ir.VK_BOOL))

    def b(self, op, bd, a=0, b=0, c=0, aux0=0):
        self.p.emit(op, 1, dst=bd, a=a, b=b, c=c, aux0=aux0)

    def assert_(self, breg, expect=True):
        if not expect:
            self.p.emit(ir.B_NOT, 1, dst=B_SCRATCH, a=breg)
            breg = B_SCRATCH
        self.p.emit(ir.ASSERT, 1, a=breg)

    def assert_eq(self, width, reg, value, scratch, bd=0):
        """ASSERT reg == value, the constant loaded into W register ``scratch`` (the device
        program folds it into the compare: PF_I_KB)."""
        self.wconst(scratch, width, value)
        self.cmp(ir.B_EQ, width, bd, reg, scratch)
        self.p.emit(ir.ASSERT, 1, a=bd)

    def done(self, verdict=True):
        self.p.finish().validate()
        self.p.verdict = verdict
        self.p.assignment = list(self.values)
        return self.p


def _name(tag, op, w, base):
    return f"{tag}:{ir.OPNAMES.get(op, op)}/w{w}/base{base}"


def _scratch(regs, n=7):
    """A register of 0..n-1 that is none of ``regs``."""
    return next(r for r in range(n) if r not in regs)


# ---- one operation, variable operands ------------------------------------------------

def binop_set(op, w, a, b, expect, regs=(0, 1, 2), base=0, wa=None, wb=None, aux0=0, verdict=True,
              parents=True):
    """vars a (width wa), b (width wb) in registers ra, rb; rd <- op(ra, rb) at width w;
    ASSERT rd == expect.  W_BINARY ops and W_CONCAT (aux0 = wb)."""
    ra, rb, rd = regs
    s = Asm(_name("bin", op, w, base), base, parents)
    s.wvar(ra, wa or w, a)
    s.wvar(rb, wb or w, b)
    s.w(op, w, rd, ra, rb, aux0=aux0)
    s.assert_eq(w, rd, expect, _scratch((rd,)))
    return s.done(verdict)


def unop_set(op, w, a, expect, regs=(0, 1), base=0, wa=None, aux0=0, verdict=True, parents=True):
    """var a (width wa) in ra; rd <- op(ra) at width w (aux0: EXTRACT's lo, SEXT's source
    width, HASH's salt); ASSERT rd == expect."""
    ra, rd = regs
    s = Asm(_name("un", op, w, base), base, parents)
    s.wvar(ra, wa or w, a)
    s.w(op, w, rd, ra, aux0=aux0)
    s.assert_eq(w, rd, expect, _scratch((rd,)))
    return s.done(verdict)


def ite_set(w, sel, a, b, expect, regs=(0, 1, 2), base=0, verdict=True, parents=True):
    """Bool var sel in B3, vars a, b; rd <- sel ? ra : rb; ASSERT rd == expect."""
    ra, rb, rd = regs
    s = Asm(_name("ite", ir.W_ITE, w, base), base, parents)
    s.bvar(3, sel)
    s.wvar(ra, w, a)
    s.wvar(rb, w, b)
    s.w(ir.W_ITE, w, rd, ra, rb, c=3)
    s.assert_eq(w, rd, expect, _scratch((rd,)))
    return s.done(verdict)


def cmp_set(op, w, a, b, expect, regs=(0, 1), base=0, verdict=True, parents=True, bd=2):
    """vars a, b; B[bd] <- cmp(ra, rb) at width w; ASSERT B[bd] == expect (a bool)."""
    ra, rb = regs
    s = Asm(_name("cmp", op, w, base), base, parents)
    s.wvar(ra, w, a)
    s.wvar(rb, w, b)
    s.cmp(op, w, bd, ra, rb)
    s.assert_(bd, bool(expect))
    return s.done(verdict)


def bool_set(op, ins, expect, base=0, verdict=True, parents=True):
    """Bool vars (B_CONST: the constant itself) in B registers 1, 2, 3; B5 <- op; ASSERT
    B5 == expect.  B_ITE reads (then, else, cond) = ins.  A W register is written too, so
    ``base`` still chooses the kernel."""
    s = Asm(_name("bool", op, 1, base), base, parents)
    s.wconst(0, 8, 0)
    if op == ir.B_CONST:
        s.b(ir.B_CONST, 5, aux0=int(ins[0]))
    else:
        for k, v in enumerate(ins):
            s.bvar(1 + k, v)
        if op == ir.B_NOT:
            s.b(op, 5, a=1)
        elif op == ir.B_ITE:
            s.b(op, 5, a=1, b=2, c=3)
        else:
            s.b(op, 5, a=1, b=2)
    s.assert_(5, bool(expect))
    return s.done(verdict)


# ---- one operation, constant operands --------------------------------------------------

def ground_set(op, w, a, b, expect, regs=(0, 1, 2), base=0, verdict=True):
    """binop_set / cmp_set with both operands W_CONST: the device program reads them as
    PF_I_KA / PF_I_KB scalar loads, uniform over the wave, which is what reaches the
    wave-uniform shortcuts of pf::udivrem256 and exp256_split from a search kernel."""
    ra, rb, rd = regs
    s = Asm(_name("ground", op, w, base), base)
    s.wconst(ra, w, a & ir.mask(w))
    s.wconst(rb, w, b & ir.mask(w))
    if op in ir.B_CMP:
        s.cmp(op, w, 2, ra, rb)
        s.assert_(2, bool(expect))
    else:
        s.w(op, w, rd, ra, rb)
        s.assert_eq(w, rd, expect, _scratch((rd,)))
    return s.done(verdict)


# ---- the register file ------------------------------------------------------------------

def slot_checks(op, ra, rb, rd):
    """Names of the compares a slot set makes after its op, in guards-first order: every
    register of 0..6 that still holds a loaded value, then the result."""
    scratch = slot_scratch(op, ra, rb, rd)
    w_result = op not in ir.B_CMP
    regs = [r for r in range(7) if r != scratch and not (w_result and r == rd)]
    return [f"W{r}" for r in regs] + ["result"]


def slot_scratch(op, ra, rb, rd):
    """The operand register that is dead after the op and does not hold its result: the
    expected constants of the compares are loaded there (deleted on the device)."""
    return rb if (op not in ir.B_CMP and rd == ra) else ra


def slot_set(op, ra, rb, rd, order, a, b, expect, base=0, w=256, verdict=True, only=None):
    """The op between full register files: operands in ra, rb, a distinct guard value in every
    other register of 0..6 (loaded between the operand loads and the op, so the op's operands
    are register reads, not forwarded), the result in rd (for a compare: B register rd).
    Afterwards every register that still holds a loaded value — the guards and the operand
    that is not the compare scratch — and the result are compared with their constants.
    ``order="guards_first"`` compares the result last (read back from its register: the
    write-back is tested), ``"result_first"`` right after the op (forwarded).  ``only`` keeps a
    single compare, by its name in slot_checks()."""
    assert ra != rb and order in ("guards_first", "result_first")
    s = Asm(f"slot:{ir.OPNAMES[op]}/a{ra}/b{rb}/d{rd}/{order}/base{base}", base)
    held = {ra: a & ir.mask(w), rb: b & ir.mask(w)}
    s.wvar(ra, w, a)
    s.wvar(rb, w, b)
    for r in range(7):
        if r not in (ra, rb):
            held[r] = GUARDS[r] & ir.mask(w)
            s.wvar(r, w, held[r])
    scratch = slot_scratch(op, ra, rb, rd)
    is_cmp = op in ir.B_CMP
    if is_cmp:
        s.cmp(op, w, rd, ra, rb)
    else:
        s.w(op, w, rd, ra, rb)
        held.pop(rd, None)
    held.pop(scratch, None)

    def result():
        if only not in (None, "result"):
            return
        if is_cmp:
            s.assert_(rd, bool(expect))
        else:
            s.assert_eq(w, rd, expect, scratch, bd=8)

    def guards():
        for r in sorted(held):
            if only in (None, f"W{r}"):
                s.assert_eq(w, r, held[r], scratch, bd=9 + r)

    if order == "result_first":
        result()
        guards()
    else:
        guards()
        result()
    return s.done(verdict)


# ---- identities over generated candidates ---------------------------------------------

def edge_pool(w):
    return [0, 1, (1 << 32) - 1, 1 << 32, ir.mask(w), 1 << (w - 1)]


IDENTITIES = ("udivrem", "sdivrem", "smod", "shl_exp", "lshr_udiv", "neg", "uadd_noovf")


def identity_set(name, w, base=0, false_variant=False, seed=0):
    """A set whose asserted formula is the *violation* of an identity between ops, over
    VK_GENERIC variables a, b (no parents) and a VK_SMALL shift amount k <= w + 1: any lane of
    any group that computes a wrong value is a witness, so the search must find none.  The
    constant pool holds the edge values, so the generator's boundary and constant +-1 arms land
    on them.  ``false_variant`` adds 1 to one side: the identity is then false and the search
    must return the oracle's witness."""
    s = Asm(f"ident:{name}/w{w}/base{base}/{'false' if false_variant else 'true'}", base, parents=False)
    s.p.seed = seed
    for c in edge_pool(w):
        s.p.const_index(c)
    M = ir.mask(w)
    bump = 1 if false_variant else 0

    def bumped(reg, scratch):
        if bump:
            s.wconst(scratch, w, 1)
            s.w(ir.W_ADD, w, reg, reg, scratch)

    s.wvar(0, w, None)                                         # a
    if name in ("shl_exp", "lshr_udiv"):
        s.wvar(1, w, None, kind=ir.VK_SMALL, hint0=w + 1)      # k
    elif name != "neg":
        s.wvar(1, w, None)                                     # b
    if name == "udivrem":
        s.w(ir.W_UDIV, w, 2, 0, 1)
        s.w(ir.W_UREM, w, 3, 0, 1)
        s.w(ir.W_MUL, w, 4, 2, 1)
        s.w(ir.W_ADD, w, 4, 4, 3)
        bumped(4, 5)
        s.cmp(ir.B_EQ, w, 0, 4, 0)
        s.cmp(ir.B_ULT, w, 1, 3, 1)
        s.b(ir.B_AND, 0, a=0, b=1)                             # B0: the b != 0 arm
        s.wconst(5, w, 0)
        s.cmp(ir.B_EQ, w, 2, 1, 5)                             # B2: b == 0
        s.wconst(5, w, M)
        s.cmp(ir.B_EQ, w, 3, 2, 5)
        s.cmp(ir.B_EQ, w, 4, 3, 0)
        s.b(ir.B_AND, 3, a=3, b=4)                             # B3: the b == 0 arm
        s.b(ir.B_ITE, 5, a=3, b=0, c=2)
        s.assert_(5, False)
    elif name == "sdivrem":
        s.w(ir.W_SDIV, w, 2, 0, 1)
        s.w(ir.W_SREM, w, 3, 0, 1)
        s.w(ir.W_MUL, w, 4, 2, 1)
        s.w(ir.W_ADD, w, 4, 4, 3)
        bumped(4, 5)
        s.cmp(ir.B_EQ, w, 0, 4, 0)
        s.wconst(5, w, 0)
        s.cmp(ir.B_EQ, w, 1, 1, 5)                             # B1: b == 0
        s.b(ir.B_OR, 2, a=0, b=1)
        s.assert_(2, False)
    elif name == "smod":
        s.w(ir.W_SMOD, w, 2, 0, 1)
        s.w(ir.W_SREM, w, 3, 0, 1)
        bumped(2, 5)
        s.cmp(ir.B_EQ, w, 0, 2, 3)
        s.w(ir.W_ADD, w, 4, 3, 1)
        s.cmp(ir.B_EQ, w, 1, 2, 4)
        s.b(ir.B_OR, 2, a=0, b=1)
        s.assert_(2, False)
    elif name == "shl_exp":
        s.w(ir.W_SHL, w, 2, 0, 1)
        s.wconst(3, w, 2)
        s.w(ir.W_EXP, w, 4, 3, 1)
        s.w(ir.W_MUL, w, 5, 0, 4)
        bumped(5, 6)
        s.cmp(ir.B_EQ, w, 0, 2, 5)
        s.assert_(0, False)
    elif name == "lshr_udiv":
        s.w(ir.W_LSHR, w, 2, 0, 1)
        s.wconst(3, w, 2)
        s.w(ir.W_EXP, w, 4, 3, 1)
        s.w(ir.W_UDIV, w, 5, 0, 4)
        bumped(5, 6)
        s.cmp(ir.B_EQ, w, 0, 2, 5)                             # B0: lshr == a / 2^k
        s.wconst(6, w, w)
        s.cmp(ir.B_ULT, w, 1, 1, 6)                            # B1: k <u w
        s.wconst(6, w, 0)
        s.cmp(ir.B_EQ, w, 2, 2, 6)                             # B2: lshr == 0
        s.b(ir.B_ITE, 3, a=0, b=2, c=1)
        s.assert_(3, False)
    elif name == "neg":
        s.w(ir.W_NEG, w, 1, 0)
        s.wconst(2, w, 0)
        s.w(ir.W_SUB, w, 3, 2, 0)
        bumped(3, 6)
        s.w(ir.W_NOT, w, 4, 0)
        s.wconst(5, w, 1)
        s.w(ir.W_ADD, w, 4, 4, 5)
        s.cmp(ir.B_EQ, w, 0, 1, 3)
        s.cmp(ir.B_EQ, w, 1, 1, 4)
        s.b(ir.B_AND, 2, a=0, b=1)
        s.assert_(2, False)
    elif name == "uadd_noovf":
        s.cmp(ir.B_UADD_NOOVF, w, 0, 0, 1)
        s.w(ir.W_ADD, w, 2, 0, 1)
        bumped(2, 3)
        s.cmp(ir.B_ULE, w, 1, 0, 2)
        s.b(ir.B_XOR, 2, a=0, b=1)
        s.assert_(2, True)
    else:
        raise ValueError(name)
    return s.done(verdict=None)


# ---- the generator, every kind ----------------------------------------------------------

GEN_WIDTHS = (1, 7, 8, 31, 32, 33, 64, 127, 128, 129, 160, 173, 255, 256)
GEN_POOL = [0xa9059cbb, (1 << 160) - 1, 1 << 255, 0xDEADBEEF << 128, ir.mask(256), 0x100,
            ir.mask(256) - 63, 0x1234_5678_9ABC_DEF0_0FED_CBA9_8765_4321 << 64]
GEN_LAYOUTS = ("bare", "consts", "parented", "alternate")


def generator_set(layout, base=0, seed=0):
    """One variable of every kind and case of the candidate generator, under one of four pool
    / parent layouts: no constants and no parents, 8 constants, 8 constants with every (or
    every other) variable parented.  Within what pf_batch_create accepts: without constants
    ACTOR has hint1 = 0, KECCAK is absent and CDBYTE spells from the whole (empty) pool.  The
    code reads only variable 0."""
    pool = layout != "bare"
    s = Asm(f"gen:{layout}/base{base}", base, parents=layout in ("parented", "alternate"))
    s.p.seed = seed
    if pool:
        s.p.consts.extend(GEN_POOL)
    specs = []
    for w in GEN_WIDTHS:
        specs.append((w, ir.VK_GENERIC, 0, 0))
        specs.append((w, ir.VK_VALUE, 0, 0))
    specs.append((1, ir.VK_BOOL, 0, 0))
    for w in (8, 256):
        for h in (0, 3, 4, 35, 36, 260, (1 << 32) - 2, (1 << 32) - 1):
            specs.append((w, ir.VK_SMALL, h, 0))
    for n in ((0, 1, 3, 4) if pool else (0,)):
        specs.append((160, ir.VK_ACTOR, 2 if pool else 0, n))
    if pool:
        specs.append((256, ir.VK_KECCAK, 6, 0))      # 2^256 - 64: the add wraps
        specs.append((256, ir.VK_KECCAK, 5, 0))      # a small base
    for pos in (0, 8, 120, 248):
        specs.append((8, ir.VK_CDBYTE, pos, 7 + pos))
        if pool:
            specs.append((8, ir.VK_CDBYTE, pos | 3 << 8 | 2 << 20, 0xFFFFFFFF))
    specs.append((8, ir.VK_CDBYTE, 16, 7))           # two bytes of one word: shared word id
    specs.append((8, ir.VK_CDBYTE, 24, 7))
    for k, (w, kind, h0, h1) in enumerate(specs):
        parent = (GUARDS[k % 7] ^ (k * 0x0101_0101 << 96)) & ir.mask(w)
        s.var(w, parent, kind, h0, h1, parent=(layout == "parented" or k % 2 == 0))
    s.p.emit(ir.W_VAR, s.p.vars[0].width, dst=base, aux0=0)
    s.cmp(ir.B_ULE, s.p.vars[0].width, 0, 0, 0)       # holds for every candidate; no constant
    s.assert_(0)
    return s.done(verdict=None)


PIN_VARS = ((256, ir.VK_GENERIC), (173, ir.VK_GENERIC), (129, ir.VK_GENERIC), (256, ir.VK_VALUE),
            (256, ir.VK_KECCAK))
PIN_CANDS = (1, 63, 64, 65, 127, 4095)


def pin_set(v, target, base=0, seed=0):
    """Five high-entropy variables (PIN_VARS, no parents, the 8-constant pool plus the target
    as constant 8, so the pool's size does not depend on the target); the code reads variable
    ``v`` and asserts it equals ``target`` — the oracle's value of it at a chosen candidate k
    — so the search's first witness is the first candidate whose generated value is that one,
    k or an earlier one."""
    s = Asm(f"pin:v{v}/base{base}", base, parents=False)
    s.p.seed = seed
    s.p.consts.extend(GEN_POOL + [target & ir.mask(256)])
    for w, kind in PIN_VARS:
        s.var(w, None, kind, 6 if kind == ir.VK_KECCAK else 0, 0)
    w = PIN_VARS[v][0]
    s.p.emit(ir.W_VAR, w, dst=base, aux0=v)
    s.p.emit(ir.W_CONST, 256, dst=1 + base, aux0=8)
    s.cmp(ir.B_EQ, w, 0, 0, 1)
    s.assert_(0)
    return s.done(verdict=None)


def pin_set_at(v, k, gseed, base=0, seed=0):
    """pin_set whose target is the oracle's value of variable v at candidate k under global
    seed ``gseed``.  The target sits in the constant pool, which the generator's constant arm
    reads, so it is placed and the value recomputed until both agree (at once, unless
    candidate k itself draws constant 8)."""
    import numpy as np
    import pyoracle as O

    target = 0
    for _ in range(4):
        p = pin_set(v, target, base, seed)
        sv = O.SetView.from_batch(ir.Batch([p]), 0)
        got = sv.gen_assignments(np.array([k], dtype=np.uint64), gseed)[0][v]
        if got == target:
            p.target = target
            return p
        target = got
    raise AssertionError(f"pin_set_at({v}, {k}): no stable target")


def corrupt(value, w, bit=0):
    """The expectation with one bit flipped."""
    return (value ^ (1 << (bit % w))) & ir.mask(w)
