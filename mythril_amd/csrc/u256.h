// u256.h — 256-bit two's-complement arithmetic on 8 x 32-bit limbs held in VGPRs.
//
// One lane holds one candidate's value; limbs are little-endian (x[0] = bits 0..31).
// Everything is fully unrolled so the limbs stay in registers; carry chains map onto
// v_add_co_u32 / v_addc_co_u32 (__builtin_addc) and products onto v_mad_u64_u32.
// Widths w < 256 are handled by the callers (mask / sign-extend at the op boundary).
// Semantics follow SMT-LIB2 (z3) — see oracle/pyoracle.py for the CPU restatement.
#pragma once
#include <math.h>
#include <stdint.h>

#define PF_INL __device__ __forceinline__

#include "u256_cols.h"

namespace pf {

struct u256 {
    uint32_t l[8];
};

PF_INL u256 zero256() {
    u256 r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = 0;
    return r;
}

PF_INL u256 ones256() {
    u256 r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = 0xffffffffu;
    return r;
}

PF_INL u256 add256(const u256& a, const u256& b) {
    u256 r;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint32_t co;
        r.l[i] = __builtin_addc(a.l[i], b.l[i], c, &co);
        c = co;
    }
    return r;
}

// a + b, returns carry-out in *cout
PF_INL u256 add256c(const u256& a, const u256& b, uint32_t* cout) {
    u256 r;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint32_t co;
        r.l[i] = __builtin_addc(a.l[i], b.l[i], c, &co);
        c = co;
    }
    *cout = c;
    return r;
}

PF_INL u256 sub256(const u256& a, const u256& b) {
    u256 r;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint32_t co;
        r.l[i] = __builtin_subc(a.l[i], b.l[i], c, &co);
        c = co;
    }
    return r;
}

// a - b, returns borrow-out (1 iff a < b unsigned)
PF_INL u256 sub256b(const u256& a, const u256& b, uint32_t* bout) {
    u256 r;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint32_t co;
        r.l[i] = __builtin_subc(a.l[i], b.l[i], c, &co);
        c = co;
    }
    *bout = c;
    return r;
}

PF_INL uint32_t ult256(const u256& a, const u256& b) {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint32_t co;
        (void)__builtin_subc(a.l[i], b.l[i], c, &co);
        c = co;
    }
    return c;
}

PF_INL uint32_t eq256(const u256& a, const u256& b) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d |= a.l[i] ^ b.l[i];
    return d == 0;
}

PF_INL uint32_t iszero256(const u256& a) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d |= a.l[i];
    return d == 0;
}

PF_INL u256 neg256(const u256& a) { return sub256(zero256(), a); }

PF_INL u256 not256(const u256& a) {
    u256 r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = ~a.l[i];
    return r;
}

// Per-lane all-ones / all-zero mask of a condition, opaque to the optimiser.  A select of
// whole 256-bit values written as `c ? a : b` (or `x & mask`) is turned by LLVM into an
// exec-masked branch when c is per-lane, and one divergent branch anywhere in the
// interpreter loop makes the AMDGPU structurizer rewrite the whole loop body's uniform
// dispatch into flag-driven flow blocks.  The empty asm hides the mask's
// origin, so the select below stays one v_bfi_b32 per limb.
PF_INL uint32_t lane_mask(uint32_t c) {
    uint32_t m = 0u - (uint32_t)(c != 0u);
#ifndef PF_HOST_MAC
    asm volatile("" : "+v"(m));
#endif
    return m;
}

// A zero the optimiser cannot see through: the 9th limb of the divider's remainder, which a
// borrow chain runs into.  As a literal 0 the chain's last step is folded into a negation
// and a separate subtraction of the borrow, made a 0/1 lane value first.
PF_INL uint32_t zero_limb() {
    uint32_t z = 0u;
#ifndef PF_HOST_MAC
    asm("" : "+v"(z));
#endif
    return z;
}

PF_INL u256 sel256(uint32_t c, const u256& a, const u256& b) {
    const uint32_t m = lane_mask(c);
    u256 r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = (a.l[i] & m) | (b.l[i] & ~m);
    return r;
}

// ---- wave-uniform helpers (identity on the host build) ------------------------------
#ifndef PF_HOST_MAC
PF_INL uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return __builtin_amdgcn_readfirstlane(v);
}
// The wave's lane mask of one direct compare (`x != 0u`, `d >= 1.0`, a carry-out `!= 0u`):
// the compare writes the mask into an SGPR pair and that pair is the result.  Conditions are
// combined as masks, with & | ~ in scalar code, never as 0/1 lane values ahead of the ballot:
// a ballot of `(uint32_t)(x >= y) & (skip ^ 1u)` makes the backend turn each mask into a 0/1
// VGPR (v_cndmask_b32), and them, and compare the result with zero again — two to four VALU
// instructions per test that the scalar form does not have.
PF_INL uint64_t wave_mask(bool p) { return __builtin_amdgcn_ballot_w64(p); }
#else
PF_INL uint32_t wave_max_u32(uint32_t v) { return v; }
PF_INL uint64_t wave_mask(bool p) { return p ? 1ull : 0ull; }  // a wave is one lane: bit 0
#endif
// wave-uniform tests of (scalar combinations of) lane masks; `m & ~n` is the only use of ~, so
// the host's one-bit masks need no trimming
PF_INL bool wave_any(uint64_t m) { return m != 0ull; }
PF_INL bool wave_none(uint64_t m) { return m == 0ull; }

// The wave's mask of a < b: the borrow chain with its last step's carry-out written to an SGPR
// pair, which the chain's carry flag as a C value never is — ballot(ult256(a, b) != 0u) has no
// compare to take the mask from, and hipcc then replaces the eight-step chain by sixteen limb
// compares and as many scalar and/ors.  gfx950 wants two wait states between a VALU writing
// vcc and a VALU reading it as carry-in; inside an asm block they are ours to place.
PF_INL uint64_t wave_mask_ult256(const u256& a, const u256& b) {
#ifndef PF_HOST_MAC
    uint64_t m;
    uint32_t t;
    asm("v_sub_co_u32 %1, vcc, %2, %10\n\ts_nop 1\n\t"
        "v_subb_co_u32 %1, vcc, %3, %11, vcc\n\ts_nop 1\n\t"
        "v_subb_co_u32 %1, vcc, %4, %12, vcc\n\ts_nop 1\n\t"
        "v_subb_co_u32 %1, vcc, %5, %13, vcc\n\ts_nop 1\n\t"
        "v_subb_co_u32 %1, vcc, %6, %14, vcc\n\ts_nop 1\n\t"
        "v_subb_co_u32 %1, vcc, %7, %15, vcc\n\ts_nop 1\n\t"
        "v_subb_co_u32 %1, vcc, %8, %16, vcc\n\ts_nop 1\n\t"
        "v_subb_co_u32 %1, %0, %9, %17, vcc"
        : "=s"(m), "=&v"(t)
        : "v"(a.l[0]), "v"(a.l[1]), "v"(a.l[2]), "v"(a.l[3]), "v"(a.l[4]), "v"(a.l[5]), "v"(a.l[6]),
          "v"(a.l[7]), "v"(b.l[0]), "v"(b.l[1]), "v"(b.l[2]), "v"(b.l[3]), "v"(b.l[4]), "v"(b.l[5]),
          "v"(b.l[6]), "v"(b.l[7])
        : "vcc");
    return m;
#else
    return wave_mask(ult256(a, b) != 0u);
#endif
}

// (uint32_t)min(x, 2^32 - 1) for a FINITE, NON-NEGATIVE x, truncated: one v_cvt_u32_f64, which
// saturates by itself (x >= 2^32 and +inf give 0xFFFFFFFF), where the C conversion is undefined
// out of range and so needed an fmin in front — and fmin brought a canonicalising v_max_f64 with
// its v_min_f64, two f64-rate instructions per digit.  The precondition is the host form's: for
// a negative x both give 0, but the hardware converts NaN to 0 and fmin(NaN, c) is c.  It holds
// at all three sites in udivrem256: every argument is fma(n, r, bias) with bias = 2^-12 > 0,
// n a Horner sum of uint32 limbs (finite, >= 0, < 2^289) and r the Newton reciprocal of a
// double in [1, 2^256) (finite, > 0), so the fma is finite and positive.
PF_INL uint32_t sat_u32(double x) {
#ifndef PF_HOST_MAC
    uint32_t r;
    asm("v_cvt_u32_f64 %0, %1" : "=v"(r) : "v"(x));
    return r;
#else
    return (uint32_t)fmin(x, 4294967295.0);
#endif
}

// ---- products ---------------------------------------------------------------------
// Product scanning (column by column) with a 96-bit column accumulator (acc, hi): every
// partial product is one v_mad_u64_u32 into acc, and while a column's carry can still
// reach limb 7 its carry out of bit 63 is added into hi, which each carrying column creates
// (its first carry add is 0 + 0 + carry: nothing zeroes hi between columns; the one zero is
// the first column's, which cannot carry).  The columns are inline-asm
// blocks generated by tools/gen_u256_cols.py (u256_cols.h), which also places the gfx950
// SGPR write->read wait states and, from the same columns, the truncated multiply-adds of
// EXP's series (tmulk, below at tmul_add); under PF_HOST_MAC the columns are portable C, so
// tools/u256_host_check.cpp and tools/exp_series_host.cpp run this header on the CPU.
#define PF_COL_NEXT(k)                                   \
    r.l[k] = (uint32_t)acc;                              \
    acc = (acc >> 32) | ((uint64_t)hi << 32);

// truncated 256 x 256 -> 256 product: 36 partial products
PF_INL u256 mul256(const u256& a, const u256& b) {
    const uint32_t *x = a.l, *y = b.l;
    u256 r;
    uint64_t acc = 0;
    uint32_t hi = 0;
    col64_1(acc, x[0], y[0]);  // a single product cannot carry out of 64 bits
    PF_COL_NEXT(0)
    col96_2(acc, hi, x[0], x[1], y[1], y[0]);
    PF_COL_NEXT(1)
    col96_3(acc, hi, x[0], x[1], x[2], y[2], y[1], y[0]);
    PF_COL_NEXT(2)
    col96_4(acc, hi, x[0], x[1], x[2], x[3], y[3], y[2], y[1], y[0]);
    PF_COL_NEXT(3)
    col96_5(acc, hi, x[0], x[1], x[2], x[3], x[4], y[4], y[3], y[2], y[1], y[0]);
    PF_COL_NEXT(4)
    col96_6(acc, hi, x[0], x[1], x[2], x[3], x[4], x[5], y[5], y[4], y[3], y[2], y[1], y[0]);
    PF_COL_NEXT(5)
    // column 6: a carry out of bit 63 would only reach limb 8
    col64_7(acc, x[0], x[1], x[2], x[3], x[4], x[5], x[6], y[6], y[5], y[4], y[3], y[2], y[1], y[0]);
    r.l[6] = (uint32_t)acc;
    acc >>= 32;
    col64_8(acc, x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], y[7], y[6], y[5], y[4], y[3], y[2], y[1], y[0]);
    r.l[7] = (uint32_t)acc;
    return r;
}

// truncated square: the 16 cross products a_i a_j (i < j, i + j <= 7) by column, doubled,
// plus the 4 diagonal squares a_i^2 (2i <= 7) — 20 partial products instead of 36.
PF_INL u256 sqr256(const u256& a) {
    const uint32_t* x = a.l;
    u256 r;
    r.l[0] = 0u;
    uint64_t acc = 0;
    uint32_t hi = 0;
    col64_1(acc, x[0], x[1]);
    PF_COL_NEXT(1)
    col96_1(acc, hi, x[0], x[2]);
    PF_COL_NEXT(2)
    col96_2(acc, hi, x[0], x[1], x[3], x[2]);
    PF_COL_NEXT(3)
    col96_2(acc, hi, x[0], x[1], x[4], x[3]);
    PF_COL_NEXT(4)
    col96_3(acc, hi, x[0], x[1], x[2], x[5], x[4], x[3]);
    PF_COL_NEXT(5)
    col64_3(acc, x[0], x[1], x[2], x[6], x[5], x[4]);
    r.l[6] = (uint32_t)acc;
    acc >>= 32;
    col64_4(acc, x[0], x[1], x[2], x[3], x[7], x[6], x[5], x[4]);
    r.l[7] = (uint32_t)acc;
    u256 c;
#pragma unroll
    for (int i = 7; i >= 1; i--) c.l[i] = (r.l[i] << 1) | (r.l[i - 1] >> 31);
    c.l[0] = 0u;
    u256 d;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uint64_t q = 0;
        col64_1(q, x[i], x[i]);
        d.l[2 * i] = (uint32_t)q;
        d.l[2 * i + 1] = (uint32_t)(q >> 32);
    }
    return add256(c, d);
}
#undef PF_COL_NEXT

// full product high half is non-zero? (a * b >= 2^256).  Used for bvumul_noovfl.
PF_INL uint32_t mul256_overflows(const u256& a, const u256& b) {
    // any a[i]*b[j] with i+j >= 8 non-zero, or carry out of the truncated product.
    uint32_t hi = 0;
    u256 r = zero256();
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (i + j < 8) {
                uint64_t t = (uint64_t)a.l[i] * b.l[j] + r.l[i + j] + carry;
                r.l[i + j] = (uint32_t)t;
                carry = t >> 32;
            } else {
                hi |= (a.l[i] != 0u && b.l[j] != 0u) ? 1u : 0u;
            }
        }
        hi |= (carry != 0) ? 1u : 0u;
    }
    return hi;
}

// logical shift left by s (per lane, any value); s >= 256 -> 0
PF_INL u256 shl256(const u256& a, uint32_t s, uint32_t big) {
    u256 x = a;
    // limb moves by 4, 2, 1 limbs
    if (__builtin_expect(1, 1)) {
        uint32_t m = (s >> 7) & 1;
#pragma unroll
        for (int i = 7; i >= 0; i--) x.l[i] = m ? (i >= 4 ? x.l[i - 4] : 0u) : x.l[i];
        m = (s >> 6) & 1;
#pragma unroll
        for (int i = 7; i >= 0; i--) x.l[i] = m ? (i >= 2 ? x.l[i - 2] : 0u) : x.l[i];
        m = (s >> 5) & 1;
#pragma unroll
        for (int i = 7; i >= 0; i--) x.l[i] = m ? (i >= 1 ? x.l[i - 1] : 0u) : x.l[i];
    }
    uint32_t bs = s & 31;
    u256 r;
#pragma unroll
    for (int i = 7; i >= 1; i--) r.l[i] = bs ? ((x.l[i] << bs) | (x.l[i - 1] >> (32 - bs))) : x.l[i];
    r.l[0] = x.l[0] << bs;
    return sel256(big, zero256(), r);
}

// shift right by s with fill word f (0 = logical, 0xffffffff = arithmetic fill); s < 256
PF_INL u256 shr256(const u256& a, uint32_t s, uint32_t f) {
    u256 x = a;
    uint32_t m = (s >> 7) & 1;
#pragma unroll
    for (int i = 0; i < 8; i++) x.l[i] = m ? (i + 4 < 8 ? x.l[i + 4] : f) : x.l[i];
    m = (s >> 6) & 1;
#pragma unroll
    for (int i = 0; i < 8; i++) x.l[i] = m ? (i + 2 < 8 ? x.l[i + 2] : f) : x.l[i];
    m = (s >> 5) & 1;
#pragma unroll
    for (int i = 0; i < 8; i++) x.l[i] = m ? (i + 1 < 8 ? x.l[i + 1] : f) : x.l[i];
    uint32_t bs = s & 31;
    u256 r;
#pragma unroll
    for (int i = 0; i < 7; i++) r.l[i] = bs ? ((x.l[i] >> bs) | (x.l[i + 1] << (32 - bs))) : x.l[i];
    r.l[7] = bs ? ((x.l[7] >> bs) | (f << (32 - bs))) : x.l[7];
    return r;
}

PF_INL uint32_t clz256(const u256& a) {
    uint32_t n = 0, done = 0;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        uint32_t z = a.l[i] ? (uint32_t)__builtin_clz(a.l[i]) : 32u;
        n += done ? 0u : z;
        done |= (a.l[i] != 0u);
    }
    return n;  // 256 for zero
}

// 1 / x in f64 to ~2^-52 relative: v_rcp_f64 and two Newton steps (x normal and positive
// here: 1 <= x < 2^256).  The IEEE-exact `1.0 / x` adds div_scale / div_fmas / div_fixup.
PF_INL double rcp_f64(double x) {
#ifndef PF_HOST_MAC
    double r = __builtin_amdgcn_rcp(x);
    double e = fma(-x, r, 1.0);
    r = fma(r, e, r);
    e = fma(-x, r, 1.0);
    return fma(r, e, r);
#else
    return 1.0 / x;
#endif
}

// value of a 256-bit number as a double (Horner over the limbs, relative error < 8 * 2^-53)
PF_INL double to_f64(const u256& a) {
    double d = 0.0;
#pragma unroll
    for (int i = 7; i >= 0; i--) d = fma(d, 4294967296.0, (double)a.l[i]);
    return d;
}

// unsigned divide: q = a / b, r = a % b, with z3 conventions for b == 0 (q = ~0, r = a).
// Wave-uniform fast paths first (all quotients 0, all divisors one limb, all quotients one
// digit), then the general path: long division with f64 digit estimates.  All limb indices
// are compile-time (fully unrolled): no scratch.
// The bias added to every f64 digit estimate, so that it is never below the true digit:
#define PF_DIV_BIAS 0x1p-12
PF_INL void udivrem256(const u256& a, const u256& b, u256* q, u256* r) {
    const uint32_t bz = iszero256(b);
    // the lanes that divide by zero, as a mask: every wave-uniform test below leaves them out
    // with one scalar and-not (bz itself stays a lane value for the final selects)
    const uint64_t m_bz = wave_mask(bz != 0u);
    // quotient 0 (a < b) or division by zero in every lane of the wave: no digit to
    // produce (a quarter of the divisions of the config-3 DAGs)
#ifndef PF_DIV_FORCE_GENERAL  // host fuzzing of the general path only (tools/u256_fuzz.py)
    if (wave_none(wave_mask(true) & ~(wave_mask_ult256(a, b) | m_bz))) {
        *q = sel256(bz, ones256(), zero256());
        *r = a;
        return;
    }
    // every lane's divisor fits one limb: short division, one 64/32 step per quotient digit
    // (an f64 estimate off by at most one, fixed exactly) instead of Knuth D's 8-limb
    // multiply-subtract per digit — these waves are the ones with 8-digit quotients
    if (wave_none(wave_mask((b.l[1] | b.l[2] | b.l[3] | b.l[4] | b.l[5] | b.l[6] | b.l[7]) != 0u))) {
        const uint32_t d = bz ? 1u : b.l[0];
        const double rd = rcp_f64((double)d);
        uint32_t rem = 0;
        u256 Q;
#pragma unroll
        for (int j = 7; j >= 0; j--) {
            const uint64_t num = ((uint64_t)rem << 32) | a.l[j];
            const double dn = (double)rem * 4294967296.0 + (double)a.l[j];
            // estimate biased up by 2^-12 (relative error < 2^-50, the digit < 2^32): never
            // below the true digit, at most one above it, so one downward correction (a mask,
            // no per-lane branch)
            uint32_t qj = sat_u32(fma(dn, rd, 0x1p-12));
            int64_t rr = (int64_t)(num - (uint64_t)qj * d);
            const uint32_t lo = (uint32_t)(rr < 0);
            qj -= lo;
            rr += (int64_t)(d & lane_mask(lo));
            Q.l[j] = qj;
            rem = (uint32_t)rr;
        }
        u256 R = zero256();
        R.l[0] = rem;
        *q = sel256(bz, ones256(), Q);
        *r = sel256(bz, a, R);
        return;
    }
#endif
    // the divisor as a double and its reciprocal: shared by the one-digit test and path and
    // by the general path's digit estimates
    const double rcp = rcp_f64(fmax(to_f64(b), 1.0));  // b = 0 -> 1 (z3 conventions below)
#ifndef PF_DIV_FORCE_GENERAL
    // every lane's quotient fits one digit: the quotient estimated from the operands as
    // doubles (relative error < 2^-49, so within 2^-17 of the true quotient when that is
    // below 2^32) decides it — estimate < 2^32 - 2 in every lane — and, biased up by
    // PF_DIV_BIAS = 2^-12 as in the general path below, is the digit: never below the true
    // quotient, at most one above it (only when the quotient's fraction exceeds 1 - 2^-12).
    // Then one 1 x 8-limb product and a 9-limb subtraction; the over-estimate shows as a
    // negative remainder and is fixed by one add-back under a wave-uniform branch that
    // almost never runs — no normalisation shifts, no digit loop, no upward correction
    const double qest = fma(to_f64(a), rcp, PF_DIV_BIAS);
    if (wave_none(wave_mask(qest >= 4294967294.0) & ~m_bz)) {
        uint32_t qh = sat_u32(qest);
        // p = qh * b over 9 limbs, rem = a - p (borrow = rem negative)
        u256 R, Q = zero256();
        uint32_t carry = 0, bw = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint64_t p = (uint64_t)qh * b.l[i] + carry;
            carry = (uint32_t)(p >> 32);
            uint32_t bo;
            R.l[i] = __builtin_subc(a.l[i], (uint32_t)p, bw, &bo);
            bw = bo;
        }
        // a < qh * b: the 9th limb of a - qh * b, 0 - carry - borrow, is non-zero — all ones,
        // as qh is at most one too large and so a - qh * b >= -b > -2^256 — and 0 otherwise
        // (a - qh * b <= a < 2^256; b = 0 lanes have p = 0).  One direct compare for the
        // wave's test, where the chain's carry-out itself has no compare to ballot
        uint32_t bo8;
        const uint32_t r8 = __builtin_subc(zero_limb(), carry, bw, &bo8);
        if (wave_any(wave_mask(r8 != 0u))) {  // over-estimate: add b back once, qh - 1
            const uint32_t neg = (uint32_t)(r8 != 0u);
            const uint32_t m = lane_mask(neg);
            uint32_t c = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                uint32_t co;
                R.l[i] = __builtin_addc(R.l[i], b.l[i] & m, c, &co);
                c = co;
            }
            qh -= neg;
        }
        Q.l[0] = qh;
        *q = sel256(bz, ones256(), Q);
        *r = R;  // b = 0 lanes: p = 0 and no add-back, so R = a already
        return;
    }
#endif
    // Long division with f64 digit estimates, no normalisation (the general path: waves
    // whose lanes mix divisor lengths and quotient lengths).  Digit j (from the top) is
    //   q_j = floor(rem / (b * 2^(32 j)))  estimated as  double(rem) * (1 / double(b)) * 2^-32j
    // — both conversions are Horner sums of at most 9 terms, so with the reciprocal and the
    // product the relative error is below 20 * 2^-53 < 2^-48.6, and as the true digit is
    // < 2^32 (invariant rem < b * 2^(32 (j + 1))) the estimate is within 2^-16.6 of it.
    // Biased up by PF_DIV_BIAS = 2^-12 and truncated, the digit is therefore never below
    // the true one and at most one above it (only when the true quotient's fraction
    // exceeds 1 - 2^-12): the multiply-subtract detects that over-estimate (negative
    // remainder) and b is added back once, under a wave-uniform branch that is almost never
    // taken — no under-estimate check.  A digit that rounds to 0 in every lane of the wave
    // is skipped.  Compared with Knuth D this drops the three variable 256-bit shifts of
    // (un)normalisation and the D3 refinement per digit.
    uint32_t u[9];
#pragma unroll
    for (int i = 0; i < 8; i++) u[i] = a.l[i];
    u256 Q = zero256();
    u[8] = zero_limb();  // the 9th limb: 0 between digits (below), its register kept through them
    uint32_t sfx[9];  // sfx[k] = b.l[k] | .. | b.l[7]: b * 2^32j exceeds 9 limbs iff sfx[9-j] != 0
    sfx[8] = 0u;
#pragma unroll
    for (int k = 7; k >= 0; k--) sfx[k] = sfx[k + 1] | b.l[k];
#pragma unroll
    for (int j = 7; j >= 0; j--) {
        const uint32_t bhigh = j >= 2 ? sfx[9 - j] : 0u;  // then q_j = 0
        // 0 <= rem <= a < 2^256 between digits (a digit's subtraction leaves it non-negative,
        // after the add-back if need be), so the 9th limb is a known zero here and the Horner
        // sum starts at limb 7
        double dr = (double)u[7];
#pragma unroll
        for (int i = 6; i >= j; i--) dr = fma(dr, 4294967296.0, (double)u[i]);
        // dr holds rem / 2^32j (its limbs below j only add a fraction < 1 ulp of a digit)
        const double qe = fma(dr, rcp, PF_DIV_BIAS);
        // m_bz and the bhigh masks do not change across the digits: formed once
        if (wave_none(wave_mask(qe >= 1.0) & ~(m_bz | wave_mask(bhigh != 0u)))) continue;  // digit 0 in every lane
        const uint32_t skip = bz | (uint32_t)(bhigh != 0u);
        uint32_t q = sat_u32(qe) & ~lane_mask(skip);
        // u[j .. 8] -= q * b
        uint64_t carry = 0;
        uint32_t borrow = 0;
#pragma unroll
        for (int i = 0; i + j <= 8; i++) {
            const uint64_t p = (uint64_t)q * (i < 8 ? b.l[i] : 0u) + carry;
            carry = p >> 32;
            uint32_t bo;
            u[j + i] = __builtin_subc(u[j + i], (uint32_t)p, borrow, &bo);
            borrow = bo;
        }
        // the borrow out of the chain is a carry flag, with no compare to ballot; the 9th limb
        // is one: rem - q * b * 2^32j is below 2^256 when non-negative (limb 8 = 0) and, q
        // being at most one too large, above -b * 2^32j > -2^257 when negative (limb 8 all
        // ones) — q >= 1 needs b * 2^32j <= rem / (1 - 2^-12) < 2^257
        if (wave_any(wave_mask(u[8] != 0u))) {  // over-estimate: add b * 2^32j back once
            // = borrow, as a lane value only here; the add-back runs through limb 8 too, which
            // puts its zero back (resetting it from a register per digit costs 2 VGPRs at
            // the search kernels' peak)
            const uint32_t neg = (uint32_t)(u[8] != 0u);
            const uint32_t m = 0u - neg;
            q -= neg;
            uint32_t c = 0;
#pragma unroll
            for (int i = 0; i + j <= 8; i++) {
                uint32_t co;
                u[j + i] = __builtin_addc(u[j + i], (i < 8 ? b.l[i] : 0u) & m, c, &co);
                c = co;
            }
        }
        Q.l[j] = q;
    }
    u256 R;
#pragma unroll
    for (int i = 0; i < 8; i++) R.l[i] = u[i];
    *q = sel256(bz, ones256(), Q);
    // b = 0 lanes: every digit was masked to 0, so u is still a — no select, and a's
    // registers are u's (no copy kept for one)
    *r = R;
}

// base^e mod 2^256, left-to-right over 3-bit exponent digits (fixed window): one square per
// bit and one multiply per digit by a table entry base^d, d = 0..7 (base^0 = 1, so the
// multiply is unconditional) — 255 squares + ~85 multiplies for a 256-bit exponent,
// against 2 products per bit for square-and-always-multiply.  The table lives in LDS:
// entry j, limb pair p of this lane at tbl[(j * 4 + p) * stride] (stride = lanes per wave:
// consecutive lanes hit consecutive 8-byte words, so the per-lane gathers are conflict
// free).  `nbits` (wave-uniform) must be >= every lane's bitlen(e): the digit loop is
// uniform, lanes differ only in the table entry they read.
PF_INL void tbl_put(uint2* tbl, uint32_t stride, uint32_t j, const u256& v) {
#pragma unroll
    for (int p = 0; p < 4; p++) tbl[(j * 4u + p) * stride] = make_uint2(v.l[2 * p], v.l[2 * p + 1]);
}
PF_INL u256 tbl_get(const uint2* tbl, uint32_t stride, uint32_t j) {
    u256 v;
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const uint2 q = tbl[(j * 4u + p) * stride];
        v.l[2 * p] = q.x;
        v.l[2 * p + 1] = q.y;
    }
    return v;
}

template <int WB = 3>
PF_INL u256 exp256(const u256& base, const u256& e, uint32_t nbits, uint2* tbl, uint32_t stride) {
    static_assert(WB >= 1 && WB <= 3, "window");
    constexpr uint32_t NT = 1u << WB;
    u256 r = zero256();
    r.l[0] = 1u;
    if (nbits == 0u) return r;
    tbl_put(tbl, stride, 0u, r);
    tbl_put(tbl, stride, 1u, base);
    if constexpr (WB == 2) {
        // base^2 by the dedicated squaring (20 partial products, not 36) and base^3 from it,
        // both kept in registers instead of re-read from the table
        const u256 b2 = sqr256(base);
        tbl_put(tbl, stride, 2u, b2);
        tbl_put(tbl, stride, 3u, mul256(b2, base));
    } else {
        // base^j = base^(j/2)^2 (j even) or base^(j-1) * base (j odd), one shared multiplier
#pragma unroll 1
        for (uint32_t j = 2; j < NT; j++) {
            const u256 f = tbl_get(tbl, stride, (j & 1u) ? j - 1u : j >> 1);
            const u256 g = (j & 1u) ? base : f;
            tbl_put(tbl, stride, j, mul256(f, g));
        }
    }
    const uint32_t nd = (nbits + WB - 1u) / WB;  // digits
    const uint32_t rest = WB * (nd - 1u);        // bits below the top digit
    // top digit (1..WB bits) starts the accumulator; the remaining digits are aligned at
    // the top of ex
    r = tbl_get(tbl, stride, shr256(e, rest, 0u).l[0] & (NT - 1u));
    u256 ex = shl256(e, (256u - rest) & 255u, 0u);
#pragma unroll 1
    for (uint32_t i = 1; i < nd; i++) {
#pragma unroll 1
        for (int k = 0; k < WB; k++) r = sqr256(r);
        const uint32_t d = ex.l[7] >> (32 - WB);
#pragma unroll
        for (int k = 7; k >= 1; k--) ex.l[k] = (ex.l[k] << WB) | (ex.l[k - 1] >> (32 - WB));
        ex.l[0] <<= WB;
        r = mul256(r, tbl_get(tbl, stride, d));
    }
    return r;
}

// base^e for an exponent that fits one 32-bit word (the low part e0 of the 2-adic split, in
// waves that do not run the series): the same windowed loop with the digits taken from that
// word — no 256-bit shifted exponent live across the squarings (8 VGPRs fewer at the
// kernel's peak)
template <int WB = 2>
PF_INL u256 exp256_w32(const u256& base, uint32_t e, uint32_t nbits, uint2* tbl, uint32_t stride) {
    static_assert(WB == 2, "window");
    // The table holds base^1..base^3 in entries 1..3 (entry 0 is not the table's: the
    // narrow kernels keep a W register there, pf_eval.hip); digit 0 selects 1.  Only what is
    // read is built: with nbits <= 1 every lane's e is 0 or 1 and the result comes straight
    // from registers.
    u256 one = zero256();
    one.l[0] = 1u;
    if (nbits <= 1u) return sel256((uint32_t)(e == 0u), one, base);
    const u256 b2 = sqr256(base);
    tbl_put(tbl, stride, 1u, base);
    tbl_put(tbl, stride, 2u, b2);
    tbl_put(tbl, stride, 3u, mul256(b2, base));
    const uint32_t nd = (nbits + WB - 1u) / WB;  // digits
    uint32_t d = (e >> (WB * (nd - 1u))) & 3u;
    u256 r = sel256((uint32_t)(d == 0u), one, tbl_get(tbl, stride, d));
#pragma unroll 1
    for (uint32_t i = nd - 1u; i-- > 0u;) {
#pragma unroll 1
        for (int k = 0; k < WB; k++) r = sqr256(r);
        d = (e >> (WB * i)) & 3u;
        r = mul256(r, sel256((uint32_t)(d == 0u), one, tbl_get(tbl, stride, d)));
    }
    return r;
}

// ---- EXP with a 2-adic split of the exponent ----------------------------------------
// For odd b the powers b^(2^k) (k >= 1) have the form 1 + 2^(k+2) t_k, and squaring gives
// the recurrence t_{k+1} = t_k + 2^(k+1) t_k^2.  Split e = e0 + 2^M n (e0 < 2^M; n = bits
// M..253 — bits >= 254 do not matter: the unit group mod 2^256 has exponent 2^254) and with
// x = 2^(M+2) t_M:
//   b^e = b^e0 * (1 + x)^n = b^e0 * sum_{j <= J} C(n, j) x^j  mod 2^256,
// where J is the last j with j (M+2) - v2(j!) < 256 (later terms vanish mod 2^256).  The sum
// is the Horner form h_1 of h_i = 1 + f_i h_{i+1}, h_{J+1} = 1, with the exact factors
//   f_i = (n - i + 1) t / odd(i) * 2^S_i,  S_i = M + 2 - v2(i),  odd(i) = i / 2^v2(i)
// (the power of two folded into x's shift), so f_1 ... f_j = C(n, j) x^j.  The divisions by
// odd(i) do not depend on the candidate and are folded into constants: with
//   E_i = odd(i) odd(i+1) ... odd(J)  (E_{J+1} = 1),  c = 1 / E_1 mod 2^256,
// the scaled values v_i = E_i c h_i obey, E_i = odd(i) E_{i+1} cancelling f_i's divisor,
//   v_i = K_i + (((n - i + 1) t) << S_i) v_{i+1},  K_i = E_i c,  v_{J+1} = c,
// and v_1 = E_1 c h_1 = h_1 exactly: J truncated products and J constant addends, no division
// (the K_i and c are computed at compile time, k256 below, for whatever M is configured).
// Level i lives mod 2^P_i, P_i = 256 - (valuation of d_1 ... d_{i-1}), on ceil(P_i / 32) limbs;
// below 8 limbs its product is scanned by column with K_i as the accumulator's starting value
// (tmul_add), at 8 limbs it is mul256 and one add256.
// Neither t nor the per-level shift S_i is ever formed.  x = b^(2^M) - 1 mod 2^256 is b
// squared M times (sqr256) less one, which is t_M mod 2^(254-M) — all of t_M that can
// matter — already shifted by M + 2; the chain carries the factor as ((n - i + 1) t) << (M + 2),
// a multiple of x that steps by x, and the levels' values scaled by the powers of two that
// the factors are too large by (the scale schedule, below at exp_sched).
// b^e0 comes from the same squarings: they pass through b^2, b^4, ... b^(2^(M-1)), and
//   b^e0 = prod_k (b^(2^k))^bit_k(e0),
// taken right to left on that one chain, needs no squaring of its own — M squarings and at
// most M - 1 products for the whole powering (8 + 7 at M = 8; a left-to-right 2-bit window
// for b^e0 and a second climb for x were 14 + 4), and no table.  The product of step k is
// skipped where no lane of the wave has bit k of e0.  Waves in which no lane runs the series
// (every base even or every n = 0) keep the windowed left-to-right loop over e0's bits
// (exp256_w32), as do splits whose e0 is wider than a word or whose window is 3 bits (exp256).
// Even b: b^e = 0 for e >= 256 (2-adic valuation >= e), else e = e0 + 2^M n with n the
// high part of a value < 256 — M >= 8 makes n = 0 and b^e = b^e0.
// (tools/u256_fuzz.py checks this against Python's pow on the host build.)
#ifndef PF_EXP_SPLIT
#define PF_EXP_SPLIT 8
#endif
// window of the left-to-right part and its LDS table size (entries per lane)
#define PF_EXP_WINDOW (PF_EXP_SPLIT <= 20 ? 2 : 3)
#define PF_EXP_TBL_ENTRIES (1 << PF_EXP_WINDOW)

// (hi:lo) >> s, s in [0, 31] -> low word (v_alignbit_b32)
PF_INL uint32_t funnel(uint32_t hi, uint32_t lo, uint32_t s) {
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> s);
}

constexpr int v2c(int i) { return (i & 1) ? 0 : 1 + v2c(i >> 1); }
constexpr int v2fact(int j) { return j <= 1 ? 0 : v2c(j) + v2fact(j - 1); }
constexpr int exp_terms(int m) {  // J: last j whose term can be nonzero mod 2^256
    int j = 1;
    while ((j + 1) * (m + 2) - v2fact(j + 1) < 256) j++;
    return j;
}
// lower bound of the 2-adic valuation of f_1 ... f_{i-1} (the factor in front of h_i)
constexpr int prefix_val(int m, int i) { return (i - 1) * (m + 2) - v2fact(i - 1); }

// ---- compile-time 256-bit constants of the series (no code: every use is a constexpr) ----
struct k256 {
    uint32_t l[8];
};
constexpr k256 k_small(uint32_t v) {
    k256 r{};
    r.l[0] = v;
    return r;
}
constexpr k256 k_mul(const k256& a, const k256& b) {  // a * b mod 2^256
    k256 r{};
    for (int i = 0; i < 8; i++) {
        uint64_t c = 0;
        for (int j = 0; i + j < 8; j++) {
            c = (uint64_t)a.l[i] * b.l[j] + r.l[i + j] + (c >> 32);
            r.l[i + j] = (uint32_t)c;
        }
    }
    return r;
}
constexpr k256 k_inv(const k256& o) {  // o^-1 mod 2^256, o odd (Newton: 7 doublings from 3 bits)
    k256 x = o;
    for (int it = 0; it < 7; it++) {
        const k256 ox = k_mul(o, x);
        k256 two_minus{};  // 2 - o x
        uint64_t bw = 0;
        for (int i = 0; i < 8; i++) {
            const uint64_t d = (uint64_t)(i == 0 ? 2u : 0u) - ox.l[i] - bw;
            two_minus.l[i] = (uint32_t)d;
            bw = (d >> 32) & 1u;
        }
        x = k_mul(x, two_minus);
    }
    return x;
}
// E_i = odd(i) odd(i + 1) ... odd(j) (1 for i > j), odd(i) = i / 2^v2(i)
constexpr k256 exp_oddprod(int i, int j) {
    k256 r = k_small(1u);
    for (int k = i; k <= j; k++) r = k_mul(r, k_small((uint32_t)(k >> v2c(k))));
    return r;
}
// K_i = E_i / E_1 mod 2^(32 limbs): the addend of Horner level i (K_{J+1} = 1 / E_1 is the
// innermost operand)
constexpr k256 exp_addend(int i, int j, int limbs) {
    k256 r = k_mul(exp_oddprod(i, j), k_inv(exp_oddprod(1, j)));
    for (int k = limbs; k < 8; k++) r.l[k] = 0u;
    return r;
}

// a * b + k mod 2^(32 L) (limbs >= L of the result zero; limbs >= L of a and k ignored), b of
// LY = L or L - 1 limbs (its limbs >= LY ignored: zero): product scanning with k as the column
// accumulator's starting value and its further limbs literals of the columns' adds
// (u256_cols.h, tmulk; K0 .. K6 repeat k's limbs as constants).  The
// full-width levels keep mul256 and one add256: the same products with the addend inside cost
// 8 VALU less per EXP and a spilled register in the interpreter loop.
template <int L, int LY, uint32_t K0, uint32_t K1, uint32_t K2, uint32_t K3, uint32_t K4, uint32_t K5, uint32_t K6>
PF_INL u256 tmul_add(const u256& a, const u256& b, const k256& k) {
    if constexpr (L >= 8) {
        u256 kk;
#pragma unroll
        for (int i = 0; i < 8; i++) kk.l[i] = k.l[i];
        return add256(mul256(a, b), kk);
    } else {
        u256 r = zero256();
        tmulk<L, LY, K0, K1, K2, K3, K4, K5, K6>(a.l, b.l, r.l);
        return r;
    }
}

// a - c mod 2^256, c a small constant
PF_INL u256 sub_small256(const u256& a, uint32_t c) {
    u256 r;
    uint32_t bw = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint32_t bo;
        r.l[i] = __builtin_subc(a.l[i], i == 0 ? c : 0u, bw, &bo);
        bw = bo;
    }
    return r;
}

// limbs 0 .. L-1 of a >> S, S in [0, 31] a compile-time constant (limbs >= L of the result zero)
template <int S, int L>
PF_INL u256 shr_const(const u256& a) {
    static_assert(S >= 0 && S < 32 && L >= 1 && L <= 8, "shape");
    u256 r = zero256();
#pragma unroll
    for (int i = 0; i < L; i++) r.l[i] = S ? funnel(i + 1 < 8 ? a.l[i + 1 < 8 ? i + 1 : 0] : 0u, a.l[i], S) : a.l[i];
    return r;
}

// k << s mod 2^(32 limbs), s in [0, 31]
constexpr k256 k_shl(const k256& k, int s, int limbs) {
    k256 r{};
    for (int i = 0; i < limbs; i++) {
        const uint64_t w = ((uint64_t)k.l[i] << 32) | (i ? k.l[i - 1] : 0u);
        r.l[i] = (uint32_t)(w >> (32 - s));
    }
    return r;
}
// the condition under which tmul_add's columns take k's limbs as literals (u256_cols.h, tmulk:
// limb c >= 2 plus the column's c - 1 carries must fit 32 bits); the 8-limb levels add k whole
constexpr bool exp_literal_ok(const k256& k, int limbs) {
    if (limbs >= 8) return true;
    for (int c = 2; c < limbs; c++)
        if (k.l[c] > 0xFFFFFFFFu - (uint32_t)(c - 1)) return false;
    return true;
}

// ---- the chain's scale schedule --------------------------------------------------------
// The factor of level I is d_I = ((n - I + 1) t) << (M + 2 - v2(I)): shifted per level, that is
// one funnel shift per limb per level.  Instead the chain carries G_I = ((n - I + 1) t) << (M + 2)
// (d_I = G_I >> v2(I); stepping a level adds t << (M + 2) = b^(2^M) - 1) and the scaled values
// w_I = 2^(c_I) v_I, which obey
//   w_I = (K_I << c_I) + G_I w_{I+1},  c_I = c_{I+1} + v2(I),  c_{J+1} = 0
// with no shift at all, as long as the P_I + c_I bits of w_I that matter fit the level's
// 32 L_I (G_I's M + 2 trailing zeros make the product read P_{I+1} + c_{I+1} bits of w_{I+1}).
// Where they do not, w_{I+1} is un-scaled first (>> c_{I+1}: exact, its low bits are zero) and
// c_I = v2(I); where that does not fit either, G_I is shifted down by v2(I) as well and
// c_I = 0, which is the unscaled level.  A level whose shifted addend fails the literal
// condition of tmul_add's columns falls through the same choices.  Level 1 has 256 bits on 8
// limbs, so the chain always ends with c_1 = 0 and w_1 = v_1.
constexpr int EXP_MAX_TERMS = 32;  // J = 28 at the smallest split (8)
struct exp_sched_t {
    int c[EXP_MAX_TERMS + 2];       // c_I, the scale of level I's value
    bool unscale[EXP_MAX_TERMS + 2];  // level I reads w_{I+1} >> c_{I+1}
    bool shift_g[EXP_MAX_TERMS + 2];  // level I multiplies by G_I >> v2(I)
};
constexpr exp_sched_t exp_sched(int m) {
    exp_sched_t s{};
    const int j = exp_terms(m);
    const k256 inv = k_inv(exp_oddprod(1, j));
    k256 e = k_small(1u);  // E_{i}, from E_{J+1} = 1 down
    for (int i = j; i >= 1; i--) {
        e = k_mul(e, k_small((uint32_t)(i >> v2c(i))));
        const int p = 256 - prefix_val(m, i), l = (p + 31) / 32, v = v2c(i), cin = s.c[i + 1];
        k256 k = k_mul(e, inv);
        for (int q = l; q < 8; q++) k.l[q] = 0u;
        if (p + cin + v <= 32 * l && exp_literal_ok(k_shl(k, cin + v, l), l)) {
            s.c[i] = cin + v;
        } else if (p + v <= 32 * l && exp_literal_ok(k_shl(k, v, l), l)) {
            s.c[i] = v;
            s.unscale[i] = cin != 0;
        } else {
            s.c[i] = 0;
            s.unscale[i] = cin != 0;
            s.shift_g[i] = v != 0;
        }
    }
    return s;
}
template <int M>
inline constexpr exp_sched_t EXP_SCHED = exp_sched(M);

// Horner level I of sum_j C(n, j) x^j in its division-free, scaled form (above):
// w_I = (K_I << c_I) + G_I w_{I+1} with w_{J+1} = K_{J+1}, computed mod 2^(P_I + c_I)
// (P_I = 256 - prefix_val(I): bits above are multiplied out of range by d_1..d_{I-1}) on
// L = ceil(P_I / 32) limbs.  P_{I+1} = P_I - S_I (S_I = M + 2 - v2(I)), so the inner value's
// limbs are all that the factor's trailing zeros leave in range.  G carries
// ((n - I + 1) t) << (M + 2) from level to level: it enters the innermost level for I = J and
// every level on the way out adds T = t << (M + 2) = b^(2^M) - 1 (on all 8 limbs: the outer
// levels read more of them than the inner ones), so no level multiplies t by its index or
// shifts it.
template <int M, int I, int J>
PF_INL u256 horner(u256& G, const u256& T) {
    static_assert(J <= EXP_MAX_TERMS, "schedule size");
    constexpr int V = v2c(I);
    constexpr int P = 256 - prefix_val(M, I);
    constexpr int L = (P + 31) / 32;
    constexpr int C = EXP_SCHED<M>.c[I];
    constexpr bool UNSCALE = EXP_SCHED<M>.unscale[I], SHIFT_G = EXP_SCHED<M>.shift_g[I];
    constexpr int CIN = EXP_SCHED<M>.c[I + 1];            // scale of w_{I+1} as the chain hands it up
    constexpr int CY = UNSCALE ? 0 : CIN;                 // ... and as the product reads it
    static_assert(C == CY + (SHIFT_G ? 0 : V) && C >= 0 && C < 32 && CIN < 32, "scale schedule");
    static_assert(P + C <= 32 * L, "the scaled level fits its limbs");
    static_assert(I > 1 || C == 0, "the chain ends unscaled");
    constexpr k256 K = k_shl(exp_addend(I, J, L), C, L);
    static_assert(exp_literal_ok(K, L), "shifted addend as column literals");
    // limbs of w_{I+1} (P_{I+1} + its scale bits) that the product reads: L, or L - 1 where
    // they are fewer (any further ones are zero)
    constexpr int PY = P - (M + 2 - V);
    constexpr int LY = (I == J || (PY + CY + 31) / 32 >= L || L == 1) ? L : L - 1;
    // the inner chain first: only its result (not this level's factor) stays live across it
    u256 inner = zero256();
    if constexpr (I < J) {
        inner = horner<M, I + 1, J>(G, T);
        G = add256(G, T);  // ((n - I + 1) t) << (M + 2) from level I + 1's
        if constexpr (UNSCALE) inner = shr_const<CIN, (PY + 31) / 32>(inner);
    } else {
        constexpr k256 C0 = exp_addend(J + 1, J, L);
#pragma unroll
        for (int i = 0; i < L; i++) inner.l[i] = C0.l[i];
    }
    if constexpr (SHIFT_G)
        return tmul_add<L, LY, K.l[0], K.l[1], K.l[2], K.l[3], K.l[4], K.l[5], K.l[6]>(shr_const<V, L>(G), inner, K);
    else
        return tmul_add<L, LY, K.l[0], K.l[1], K.l[2], K.l[3], K.l[4], K.l[5], K.l[6]>(G, inner, K);
}

// pt (profiling builds, tools/unitprof.py): s_memtime cycles of the three parts — the
// windowed b^e0 of waves that run no series, the powering chain (the squarings up to b^(2^M)
// with b^e0's products), the Horner chain and final product
PF_INL u256 exp256_split(const u256& base, const u256& e, uint2* tbl, uint32_t stride,
                         uint64_t* pt = nullptr) {
#if defined(PF_PROFILE_UNITS) && !defined(PF_HOST_MAC)
#define PF_EXP_STAMP(k)                                        \
    if (pt) {                                                  \
        const uint64_t t_ = __builtin_amdgcn_s_memtime();      \
        pt[k] += t_ - t_last;                                  \
        t_last = t_;                                           \
    }
    uint64_t t_last = __builtin_amdgcn_s_memtime();
#else
#define PF_EXP_STAMP(k)
    (void)pt;
#endif
    constexpr int M = PF_EXP_SPLIT;
    static_assert(M >= 8 && M <= 84, "split");
    constexpr int T = 254 - M;              // bits of n
    constexpr int TL = (T + 31) / 32;       // limbs of n
    constexpr uint32_t TM = (T % 32) ? ((1u << (T % 32)) - 1u) : 0xffffffffu;
    constexpr int J = exp_terms(M);
    constexpr int WB = PF_EXP_WINDOW;       // window of the left-to-right part
    const uint32_t odd = base.l[0] & 1u;
    const uint32_t e_big =
        (e.l[0] >= 256u) | ((e.l[1] | e.l[2] | e.l[3] | e.l[4] | e.l[5] | e.l[6] | e.l[7]) != 0u);
    u256 e0;
#pragma unroll
    for (int i = 0; i < 8; i++)
        e0.l[i] = 32 * i + 32 <= M ? e.l[i] : (32 * i < M ? e.l[i] & ((1u << (M % 32)) - 1u) : 0u);
    const uint32_t nb0 = wave_max_u32(256u - clz256(e0));
    u256 n = shr256(e, (uint32_t)M, 0u);
#pragma unroll
    for (int i = 0; i < 8; i++) n.l[i] = i < TL - 1 ? n.l[i] : (i == TL - 1 ? n.l[i] & TM : 0u);
    // the series runs if some lane has an odd base and n != 0 (wave-uniform)
    const bool series = wave_any(wave_mask(odd != 0u) & ~wave_mask(iszero256(n) != 0u));
    constexpr bool FUSED = M <= 32 && WB == 2;  // e0 is one word: its bits index at run time
    u256 one = zero256();
    one.l[0] = 1u;
    u256 r, X;
    if (FUSED && series) {
        // One chain of squarings X = b^(2^k), k = 1 .. M, serves both parts: its last value
        // less one is the series' step, and the values on the way are the factors of
        // b^e0 = prod_k (b^(2^k))^bit_k(e0), taken right to left — b^e0 costs M - 1 products
        // and no squaring or table of its own.  The lanes' bits are selects (lane_mask).
        const uint32_t e0w = e0.l[0];
        X = base;
        r = sel256(e0w & 1u, base, one);
#pragma unroll 1
        for (uint32_t k = 1; k < (uint32_t)M; k++) {
            X = sqr256(X);
            // no lane has bit k (all of them from the wave's longest e0 on): nothing to
            // multiply.  The test is wave-uniform, a scalar branch.
            if (k >= nb0 || wave_none(wave_mask(((e0w >> k) & 1u) != 0u))) continue;
            r = mul256(r, sel256((e0w >> k) & 1u, X, one));
        }
        X = sqr256(X);
    } else {
        if constexpr (FUSED)
            r = exp256_w32<WB>(base, e0.l[0], nb0 < (uint32_t)M ? nb0 : (uint32_t)M, tbl, stride);
        else
            r = exp256<WB>(base, e0, nb0 < (uint32_t)M ? nb0 : (uint32_t)M, tbl, stride);
        PF_EXP_STAMP(0)
        if (series) {  // a multi-limb e0 or a 3-bit window: the step by its own squarings
            X = sqr256(base);
#pragma unroll 1
            for (int k = 1; k < M; k++) X = sqr256(X);
        }
    }
    if (series) {
        // X = b^(2^M) - 1 = t_M << (M + 2) mod 2^256, the chain's step; b odd: no borrow
        X.l[0] -= 1u;
        // b^e0 waits in the LDS table's entry 1 while the Horner chain runs: 8 VGPRs fewer
        // at its peak
        tbl_put(tbl, stride, 1u, r);
        PF_EXP_STAMP(1)
        // the chain's innermost factor G_J = (n - J + 1) X: one borrow chain (mod 2^256: the
        // product is the same) and one product
        u256 G = mul256(sub_small256(n, (uint32_t)(J - 1)), X);
        u256 h = horner<M, 1, J>(G, X);
        h = sel256(odd, h, one);  // even base: n != 0 means e >= 256 -> result 0 below
        r = mul256(tbl_get(tbl, stride, 1u), h);
        PF_EXP_STAMP(2)
    }
    return sel256((odd ^ 1u) & e_big, zero256(), r);
#undef PF_EXP_STAMP
}

}  // namespace pf
