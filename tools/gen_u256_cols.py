#!/usr/bin/env python3
"""Generate mythril_amd/csrc/u256_cols.h: one inline-asm block per product-scanning column, and
the truncated multiply-adds x * y + k mod 2^(32 L), L = 1..7, that EXP's series builds from them
(tmulk below).

A column accumulates n partial products x_t * y_t into a 64-bit accumulator with
v_mad_u64_u32; in the carrying form each mad's carry out of bit 63 goes to one of three
rotating SGPR pairs and is added into the 32-bit `hi` word by a v_addc issued two
instructions later.  `hi` is born inside the column: it is a write-only output and the first
carry add is 0 + 0 + carry, so no caller zeroes a register for it.  gfx950 needs 2 wait states
between a VALU writing an SGPR and a VALU reading it (hipcc pads its own add_co -> addc chains
with `s_nop 1`); the rotation provides them with useful work, and the generator inserts `s_nop`
only where a column is too short.
"""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "mythril_amd", "csrc", "u256_cols.h")
NEED = 2  # wait states between the SGPR write (mad carry) and its read (addc)


def col_args(n):
    return ", ".join([f"uint32_t x{t}" for t in range(n)] + [f"uint32_t y{t}" for t in range(n)])


def carry_col(n):
    seq = []  # (kind, t)
    for t in range(n):
        seq.append(("M", t))
        if t >= 2:
            seq.append(("A", t - 2))
    for t in range(max(0, n - 2), n):
        seq.append(("A", t))
    lines, pos_m, pos, born = [], {}, 0, False
    for kind, t in seq:
        p = f"%[p{t % 3}]"
        if kind == "M":
            lines.append(f"v_mad_u64_u32 %[acc], {p}, %[x{t}], %[y{t}], %[acc]")
            pos_m[t] = pos
            pos += 1
        else:
            gap = pos - pos_m[t] - 1
            if gap < NEED:
                lines.append(f"s_nop {NEED - gap - 1}")
                pos += NEED - gap
            lines.append(f"v_addc_co_u32_e64 %[hi], {p}, {'%[hi]' if born else '0'}, 0, {p}")
            born = True
            pos += 1
    ins = ", ".join([f'[x{t}] "v"(x{t})' for t in range(n)] + [f'[y{t}] "v"(y{t})' for t in range(n)])
    npairs = min(n, 3)
    decl = " ".join(f"uint64_t p{i};" for i in range(npairs))
    outs = ", ".join(['[acc] "+v"(acc)', '[hi] "=&v"(hi)'] + [f'[p{i}] "=&s"(p{i})' for i in range(npairs)])
    body = "\\n\\t".join(lines)
    return (f"PF_INL void col96_{n}(uint64_t& acc, uint32_t& hi, {col_args(n)}) {{\n"
            f"    {decl}\n"
            f"    asm(\"{body}\"\n        : {outs}\n        : {ins});\n}}\n")


def plain_col(n):
    lines = [f"v_mad_u64_u32 %[acc], %[p], %[x{t}], %[y{t}], %[acc]" for t in range(n)]
    ins = ", ".join([f'[x{t}] "v"(x{t})' for t in range(n)] + [f'[y{t}] "v"(y{t})' for t in range(n)])
    body = "\\n\\t".join(lines)
    return (f"PF_INL void col64_{n}(uint64_t& acc, {col_args(n)}) {{\n"
            f"    uint64_t p;\n"
            f"    asm(\"{body}\"\n        : [acc] \"+v\"(acc), [p] \"=&s\"(p)\n        : {ins});\n}}\n")


def host_col(n, carry):
    if carry:
        body = "    hi = 0u;\n" + "".join(f"    {{ unsigned __int128 t = (unsigned __int128)x{t} * y{t} + acc; acc = (uint64_t)t; hi += (uint32_t)(t >> 64); }}\n" for t in range(n))
        return f"PF_INL void col96_{n}(uint64_t& acc, uint32_t& hi, {col_args(n)}) {{\n{body}}}\n"
    body = "".join(f"    acc += (uint64_t)x{t} * y{t};\n" for t in range(n))
    return f"PF_INL void col64_{n}(uint64_t& acc, {col_args(n)}) {{\n{body}}}\n"


def tmulk(L, LY, addend):
    """x * y + k mod 2^(32 L) from the columns above: x and k have L limbs, y has LY <= L (its
    limbs >= LY are zero and their products are left out); k's limbs are template arguments.
    The addend rides in the column accumulator: k[0], k[1] are its starting value, and
    k[c + 2] is added to column c's `hi`, the word that becomes the accumulator's upper half when
    the column is shifted out: one 32-bit add with a literal.  `hi` counts the column's carries,
    at most one per mad, so the sum cannot leave 32 bits unless the limb is within n of 2^32,
    and that no limb is there is asserted where the constants are known; there is then no
    carry to hand to the next column.  A column carries into `hi` while that carry can still
    reach limb L - 1 (c <= L - 3).  Without an addend (tmul_L_LY) the columns are mul256's."""
    ks = ", ".join(f"uint32_t K{i}" for i in range(L))
    name = f"tmulk_{L}_{LY}" if addend else f"tmul_{L}_{LY}"
    out = ([f"template <{ks}>"] if addend else [])
    out.append(f"PF_INL void {name}(const uint32_t* x, const uint32_t* y, uint32_t* r) {{")
    out.append(f"    uint64_t acc = acc_const<K0, {'K1' if L >= 2 else '0u'}>();" if addend
               else "    uint64_t acc = 0;")
    if L >= 3:
        out.append("    uint32_t hi;")
    for c in range(L):
        ts = [t for t in range(c + 1) if c - t < LY]
        xs = ", ".join(f"x[{t}]" for t in ts)
        ys = ", ".join(f"y[{c - t}]" for t in ts)
        carrying = c <= L - 3
        out.append(f"    col96_{len(ts)}(acc, hi, {xs}, {ys});" if carrying
                   else f"    col64_{len(ts)}(acc, {xs}, {ys});")
        out.append(f"    r[{c}] = (uint32_t)acc;")
        if c == L - 1:
            break
        if carrying:
            if addend:
                out.append(f"    static_assert(K{c + 2} <= 0xFFFFFFFFu - {len(ts)}u, \"addend limb + {len(ts)} carries must fit 32 bits\");")
                out.append(f"    hi += K{c + 2};")
            out.append("    acc = (acc >> 32) | ((uint64_t)hi << 32);")
        else:
            out.append("    acc >>= 32;")
    out.append("}\n")
    return "\n".join(out)


# The accumulator's constant starting value.  Written as plain C it is a pair of v_mov that the
# compiler hoists out of every loop of the kernel, one live pair per product, and then spills;
# the volatile block keeps the two moves where the product is.
ACC_CONST = """template <uint32_t K0, uint32_t K1>
PF_INL uint64_t acc_const() {
#ifndef PF_HOST_MAC
    if constexpr (K0 != 0u || K1 != 0u) {
        uint32_t lo, up;
        asm volatile("v_mov_b32 %0, %2\\n\\tv_mov_b32 %1, %3" : "=v"(lo), "=v"(up) : "i"(K0), "i"(K1));
        return (uint64_t)lo | ((uint64_t)up << 32);
    }
#endif
    return (uint64_t)K0 | ((uint64_t)K1 << 32);
}
"""


def main():
    parts = ["// GENERATED by tools/gen_u256_cols.py — do not edit.\n"
             "// Product-scanning columns for mul256/sqr256 and the truncated multiply-adds built from\n"
             "// them (see the generator's docstrings).\n"
             "#pragma once\nnamespace pf {\n#ifndef PF_HOST_MAC\n"]
    for n in range(1, 7):
        parts.append(carry_col(n))
    for n in range(1, 9):
        parts.append(plain_col(n))
    parts.append("#else  // host build for tools/u256_host_check.cpp\n")
    for n in range(1, 7):
        parts.append(host_col(n, True))
    for n in range(1, 9):
        parts.append(host_col(n, False))
    parts.append("#endif\n")
    parts.append(ACC_CONST)
    shapes = [(L, LY) for L in range(1, 8) for LY in (L - 1, L) if LY >= 1]
    for L, LY in shapes:
        parts.append(tmulk(L, LY, True))
        parts.append(tmulk(L, LY, False))
    disp = ["// x * y + k mod 2^(32 L), k's limbs K0 .. K6 (those from L on are zero)\n"
            "template <int L, int LY, uint32_t K0, uint32_t K1, uint32_t K2, uint32_t K3, uint32_t K4, uint32_t K5, uint32_t K6>\n"
            "PF_INL void tmulk(const uint32_t* x, const uint32_t* y, uint32_t* r) {\n"
            "    static_assert(L >= 1 && L <= 7 && (LY == L || LY == L - 1) && LY >= 1, \"shape\");\n"
            "    constexpr bool ZERO = (K0 | K1 | K2 | K3 | K4 | K5 | K6) == 0u;"]
    for L, LY in shapes:
        ks = ", ".join(f"K{i}" for i in range(L))
        disp.append(f"    if constexpr (L == {L} && LY == {LY} && ZERO) tmul_{L}_{LY}(x, y, r);")
        disp.append(f"    if constexpr (L == {L} && LY == {LY} && !ZERO) tmulk_{L}_{LY}<{ks}>(x, y, r);")
    disp.append("}\n")
    parts.append("\n".join(disp))
    parts.append("}  // namespace pf\n")
    open(OUT, "w").write("\n".join(parts))
    print(OUT)


if __name__ == "__main__":
    main()
