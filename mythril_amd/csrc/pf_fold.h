/*
 * pf_fold.h — constant folding, x-op-x identities and dead-code removal over one set's lowered
 * program, the first of pf_batch_create's device-program rewrites (pathfeas.hip
 * device_program_range; DESIGN.md §3 "device program rewrites").  Host C++ only.
 *
 * A forward walk keeps, per W register, B register and spill slot, what is known of the value
 * it holds: a constant (masked to its width), or a value number — two places with the same
 * number hold the same value for every candidate.  An instruction whose result the walk
 * knows is rewritten within what the device program can already say (no new opcode, flag or
 * immediate, no constant outside the set's pool, no growth):
 *   result == an operand      -> W_MOV from that register at the instruction's width
 *   constant B result         -> B_CONST
 *   constant W result         -> W_CONST idx when the pool holds the value,
 *                                W_XOR d, r, r when it is 0 (r: a register a kept instruction
 *                                wrote), else W_CONST of a constant of the device program's own
 *                                when the caller collects them (`extra`: pf_batch_create's
 *                                device pool, the set's constants followed by these), else the
 *                                instruction stays and its operands stay live
 *   ASSERT of constant true   -> dropped (a constant false stays)
 * A backward walk from the ASSERTs then drops every instruction whose W, B or spill result no
 * kept instruction reads before its next write.  Values the rewrite cannot express still
 * feed the folds downstream.
 *
 * Ranges.  Every value carries a bound: it is below 2^bound.  A constant's is its bit length;
 * an unknown result's follows from its operands' (result_bound) and is the instruction's
 * width where nothing better is known.  A result with bound 0 is the constant 0, and the
 * bound decides (x: bound p, c: a constant, all unsigned):
 *   0 <= x, x <= c for c >= 2^p - 1                      -> true
 *   x < 0, M(w) < x                                      -> false
 *   c >= 2^p:  x < c, x <= c -> true;  x == c, c == x, c < x, c <= x -> false
 *   signed < and <=: as the unsigned ones when both sides are below 2^(w-1)
 *   UADD_NOOVF of two values below 2^(w-1)               -> true
 *   x / c -> 0 and x % c -> x for c >= 2^p;  x & c -> x when c has bits 0..p-1 set;
 *   x >> c -> 0 for c >= p
 *
 * Every rule holds at every width 1..256 and under the total-division conventions of
 * include/pf_bytecode.h.  A rule is applied only where the operands fit the instruction's
 * width (values are kept zero-extended): M(w) below is the all-ones value of that width.
 * The 256-bit arithmetic is the fixed-width form of pf_recheck.cpp's evaluator (same
 * algorithms: schoolbook product, restoring division, square-and-multiply).
 */
#ifndef PF_FOLD_H
#define PF_FOLD_H

#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/pf_bytecode.h"

namespace pf_fold {

// ---- 256-bit host arithmetic (little-endian limbs) -------------------------------------
struct U {
    uint32_t l[8];
};

inline U uzero() {
    U r;
    memset(r.l, 0, sizeof r.l);
    return r;
}
inline U usmall(uint32_t v) {
    U r = uzero();
    r.l[0] = v;
    return r;
}
inline U umask(U a, uint32_t w) {
    for (uint32_t j = 0; j < 8; j++) {
        const uint32_t lo = 32u * j;
        a.l[j] &= w >= lo + 32u ? 0xffffffffu : (w > lo ? (1u << (w - lo)) - 1u : 0u);
    }
    return a;
}
inline U uones(uint32_t w) {
    U r;
    memset(r.l, 0xff, sizeof r.l);
    return umask(r, w);
}
inline bool uis0(const U& a) {
    uint32_t x = 0;
    for (int j = 0; j < 8; j++) x |= a.l[j];
    return x == 0;
}
inline bool ueq(const U& a, const U& b) { return memcmp(a.l, b.l, sizeof a.l) == 0; }
inline bool uis1(const U& a) { return ueq(a, usmall(1)); }
inline int ucmp(const U& a, const U& b) {
    for (int j = 7; j >= 0; j--)
        if (a.l[j] != b.l[j]) return a.l[j] < b.l[j] ? -1 : 1;
    return 0;
}
inline bool ubit(const U& a, uint32_t i) { return i < 256u && ((a.l[i / 32] >> (i % 32)) & 1u); }
inline uint32_t ubitlen(const U& a) {
    for (int j = 7; j >= 0; j--)
        if (a.l[j]) return 32u * (uint32_t)j + 32u - (uint32_t)__builtin_clz(a.l[j]);
    return 0;
}
inline U uadd(const U& a, const U& b, uint32_t* carry = nullptr) {
    U r;
    uint64_t c = 0;
    for (int j = 0; j < 8; j++) {
        c += (uint64_t)a.l[j] + b.l[j];
        r.l[j] = (uint32_t)c;
        c >>= 32;
    }
    if (carry) *carry = (uint32_t)c;
    return r;
}
inline U unot(U a) {
    for (int j = 0; j < 8; j++) a.l[j] = ~a.l[j];
    return a;
}
inline U uneg(const U& a) { return uadd(unot(a), usmall(1)); }
inline U usub(const U& a, const U& b) { return uadd(a, uneg(b)); }
inline U umul(const U& a, const U& b) {
    U r = uzero();
    for (int i = 0; i < 8; i++) {
        uint64_t c = 0;
        for (int j = 0; i + j < 8; j++) {
            c += (uint64_t)a.l[i] * b.l[j] + r.l[i + j];
            r.l[i + j] = (uint32_t)c;
            c >>= 32;
        }
    }
    return r;
}
inline U ushl(const U& a, uint32_t s) {  // s < 256
    U r = uzero();
    const uint32_t q = s / 32, b = s % 32;
    for (uint32_t i = q; i < 8; i++) {
        uint32_t x = a.l[i - q] << b;
        if (b && i > q) x |= a.l[i - q - 1] >> (32 - b);
        r.l[i] = x;
    }
    return r;
}
inline U ulshr(const U& a, uint32_t s) {  // s < 256
    U r = uzero();
    const uint32_t q = s / 32, b = s % 32;
    for (uint32_t i = 0; i + q < 8; i++) {
        uint32_t x = a.l[i + q] >> b;
        if (b && i + q + 1 < 8) x |= a.l[i + q + 1] << (32 - b);
        r.l[i] = x;
    }
    return r;
}
inline void udivmod(const U& a, const U& b, U* q, U* r) {  // restoring division, b != 0
    *q = uzero();
    U R = uzero();
    for (uint32_t i = ubitlen(a); i-- > 0;) {
        const uint32_t top = R.l[7] >> 31;
        R = ushl(R, 1);
        R.l[0] |= (uint32_t)ubit(a, i);
        if (top || ucmp(R, b) >= 0) {
            R = usub(R, b);
            q->l[i / 32] |= 1u << (i % 32);
        }
    }
    *r = R;
}
// the value of a register shift amount when it is below w, else w
inline uint32_t ushamt(const U& b, uint32_t w) {
    for (int j = 1; j < 8; j++)
        if (b.l[j]) return w;
    return b.l[0] < w ? b.l[0] : w;
}

// A binary W opcode on operands below 2^w (SMT-LIB2 total functions, pf_bytecode.h)
inline U eval_wbin(uint32_t op, const U& a, const U& b, uint32_t w) {
    const bool sa = ubit(a, w - 1), sb = ubit(b, w - 1);
    const U abs_a = sa ? umask(uneg(a), w) : a, abs_b = sb ? umask(uneg(b), w) : b;
    U q, r;
    switch (op) {
        case PF_W_ADD: return umask(uadd(a, b), w);
        case PF_W_SUB: return umask(usub(a, b), w);
        case PF_W_MUL: return umask(umul(a, b), w);
        case PF_W_UDIV:
            if (uis0(b)) return uones(w);
            udivmod(a, b, &q, &r);
            return q;
        case PF_W_UREM:
            if (uis0(b)) return a;
            udivmod(a, b, &q, &r);
            return r;
        case PF_W_SDIV:  // bvudiv on the magnitudes, negated when the signs differ (also b == 0)
            if (uis0(abs_b)) q = uones(w);
            else udivmod(abs_a, abs_b, &q, &r);
            return sa != sb ? umask(uneg(q), w) : q;
        case PF_W_SREM:  // sign of the dividend
            if (uis0(abs_b)) r = abs_a;
            else udivmod(abs_a, abs_b, &q, &r);
            return sa ? umask(uneg(r), w) : r;
        case PF_W_SMOD: {  // sign of the divisor
            if (uis0(abs_b)) r = abs_a;
            else udivmod(abs_a, abs_b, &q, &r);
            if (uis0(r)) return r;
            if (!sa && !sb) return r;
            if (sa && !sb) return umask(uadd(uneg(r), b), w);
            if (!sa && sb) return umask(uadd(r, b), w);
            return umask(uneg(r), w);
        }
        case PF_W_AND:
        case PF_W_OR:
        case PF_W_XOR: {
            U z;
            for (int j = 0; j < 8; j++)
                z.l[j] = op == PF_W_AND ? (a.l[j] & b.l[j]) : op == PF_W_OR ? (a.l[j] | b.l[j]) : (a.l[j] ^ b.l[j]);
            return z;
        }
        case PF_W_SHL: {
            const uint32_t s = ushamt(b, w);
            return s >= w ? uzero() : umask(ushl(a, s), w);
        }
        case PF_W_LSHR: {
            const uint32_t s = ushamt(b, w);
            return s >= w ? uzero() : ulshr(a, s);
        }
        case PF_W_ASHR: {
            const uint32_t s = ushamt(b, w);
            if (s >= w) return sa ? uones(w) : uzero();
            U z = ulshr(a, s);
            if (sa)
                for (uint32_t i = w - s; i < w; i++) z.l[i / 32] |= 1u << (i % 32);
            return z;
        }
        default: {  // PF_W_EXP
            U z = usmall(1), x = a;
            const uint32_t nb = ubitlen(b);
            for (uint32_t i = 0; i < nb; i++) {
                if (ubit(b, i)) z = umul(z, x);
                x = umul(x, x);
            }
            return umask(z, w);
        }
    }
}

// B_EQ .. B_SLE and B_UADD_NOOVF on operands below 2^w
inline bool eval_cmp(uint32_t op, const U& a, const U& b, uint32_t w) {
    const int c = ucmp(a, b);
    switch (op) {
        case PF_B_EQ: return c == 0;
        case PF_B_ULT: return c < 0;
        case PF_B_ULE: return c <= 0;
        case PF_B_SLT:
        case PF_B_SLE: {
            const bool sa = ubit(a, w - 1), sb = ubit(b, w - 1);
            if (sa != sb) return sa;
            return op == PF_B_SLT ? c < 0 : c <= 0;
        }
        default: {  // PF_B_UADD_NOOVF
            uint32_t carry;
            const U s = uadd(a, b, &carry);
            return !carry && ueq(s, umask(s, w));
        }
    }
}

// ---- abstract values -------------------------------------------------------------------
struct WV {          // a W register's (or spill slot's) value
    uint8_t konst;   // v is its value for every candidate
    uint16_t bound;  // the value is below 2^bound
    uint32_t vn;     // value number
    U v;
};
struct BV {
    uint8_t konst, v;
    uint32_t vn;
};
struct SV {  // a spill slot holds a W or a B value
    uint8_t is_b;
    WV w;
    BV b;
};

// per-thread scratch of the pass, reused from program to program
struct Scratch {
    WV W[16];
    BV B[PF_NB];
    SV S[PF_MAX_SPILL];
    std::vector<uint8_t> zero;      // instruction i: 1 = a constant-0 W result waiting for its register
    std::vector<uint8_t> zreg;      //   an operand register of i to fall back on (0xff: none)
    std::vector<uint16_t> written;  // W registers written before instruction i
    std::vector<U> own;             // constant results outside the pool, in program order
    struct Key {
        uint32_t opw, a, b, c, aux, vn;
    };
    std::vector<Key> keys;          // value numbering: (opcode, width, operand numbers, aux0) -> number
    std::vector<int32_t> heads, next;
    uint32_t n_vn;

    uint32_t fresh() { return ++n_vn; }
    uint32_t number(uint32_t opw, uint32_t a, uint32_t b, uint32_t c, uint32_t aux) {
        uint32_t h = opw * 0x9E3779B9u;
        h = (h ^ a) * 0x85EBCA6Bu;
        h = (h ^ b) * 0xC2B2AE35u;
        h = (h ^ c) * 0x27D4EB2Fu;
        h = (h ^ aux) * 0x165667B1u;
        h = (h ^ (h >> 15)) & (uint32_t)(heads.size() - 1);
        for (int32_t k = heads[h]; k >= 0; k = next[(size_t)k]) {
            const Key& e = keys[(size_t)k];
            if (e.opw == opw && e.a == a && e.b == b && e.c == c && e.aux == aux) return e.vn;
        }
        const uint32_t vn = fresh();
        keys.push_back(Key{opw, a, b, c, aux, vn});
        next.push_back(heads[h]);
        heads[h] = (int32_t)keys.size() - 1;
        return vn;
    }
};

inline uint32_t mk_w0(uint32_t op, uint32_t w) {
    return op | (w << 8) | (pf_op_traffic(op) << 18) | (pf_op_unit(op) << 21);
}

inline bool is_wbin(uint32_t op) {
    return (op >= PF_W_ADD && op <= PF_W_XOR) || (op >= PF_W_SHL && op <= PF_W_EXP);
}
inline bool is_cmp(uint32_t op) { return (op >= PF_B_EQ && op <= PF_B_SLE) || op == PF_B_UADD_NOOVF; }

// The bound of an unknown binary W result from its operands' (both at most w): the value is
// below 2^bound.  cb: operand b is the constant bv.  Sound under the total-division
// conventions: x % 0 = x keeps the dividend's bound, x / 0 = M(w) is why a division by an
// unknown divisor says nothing.
inline uint32_t result_bound(uint32_t op, uint32_t pa, uint32_t pb, bool cb, const U& bv, uint32_t w) {
    const uint32_t lo = pa < pb ? pa : pb, hi = pa < pb ? pb : pa;
    uint32_t bd = w;
    switch (op) {
        case PF_W_AND: bd = lo; break;
        case PF_W_OR:
        case PF_W_XOR: bd = hi; break;
        case PF_W_ADD: bd = hi + 1u; break;
        case PF_W_MUL: bd = pa + pb; break;
        case PF_W_UREM:
            bd = pa;
            if (cb && !uis0(bv) && ubitlen(bv) < bd) bd = ubitlen(bv);
            break;
        case PF_W_UDIV:
            if (cb && !uis0(bv)) bd = pa >= ubitlen(bv) ? pa - ubitlen(bv) + 1u : 0u;
            break;
        case PF_W_LSHR:
            if (cb) bd = pa > ushamt(bv, w) ? pa - ushamt(bv, w) : 0u;
            break;
        case PF_W_SHL:
            if (cb) bd = pa + ushamt(bv, w);
            break;
        default: break;
    }
    return bd < w ? bd : w;
}

// B_EQ / B_ULT / B_ULE of an unknown value below 2^p against the constant c, the unknown on
// the left (x op c) or on the right (c op x): 1 / 0 when the range decides it, else -1
inline int range_cmp(uint32_t op, bool x_left, uint32_t p, const U& c, uint32_t w) {
    const bool above = ubitlen(c) > p;  // c >= 2^p
    if (op == PF_B_EQ) return above ? 0 : -1;
    if (x_left) {
        if (op == PF_B_ULT) return uis0(c) ? 0 : above ? 1 : -1;
        return above || ueq(c, uones(p)) ? 1 : -1;  // x <= c for c >= 2^p - 1
    }
    if (op == PF_B_ULE) return uis0(c) ? 1 : above ? 0 : -1;
    return above || ueq(c, uones(w)) ? 0 : -1;  // c < x
}

// The pass can reason about the program: it ends with its only END, every opcode is known,
// every register, slot and width is in range, and no device flag is set yet.
inline bool well_formed(const uint32_t* P, uint32_t n) {
    if (n == 0 || (P[4 * (size_t)(n - 1)] & 0xffu) != PF_END) return false;
    for (uint32_t i = 0; i + 1 < n; i++) {
        const uint32_t w0 = P[4 * (size_t)i], w1 = P[4 * (size_t)i + 1], aux0 = P[4 * (size_t)i + 2];
        const uint32_t op = w0 & 0xffu, w = (w0 >> 8) & 0x3ffu, tr = pf_op_traffic(op);
        const uint32_t d = w1 & 0xffu, a = (w1 >> 8) & 0xffu, b = (w1 >> 16) & 0xffu, c = w1 >> 24;
        if (w0 >> 24) return false;
        if (op == PF_END || w < 1 || w > PF_MAX_WIDTH) return false;
        const bool known = (op >= PF_W_CONST && op <= PF_W_FILL) || (op >= PF_B_CONST && op <= PF_B_SPILL) ||
                           op == PF_ASSERT;
        if (!known) return false;
        if (((tr & PF_TR_RA) && a >= PF_NW) || ((tr & PF_TR_RB) && b >= PF_NW) || ((tr & PF_TR_WW) && d >= PF_NW))
            return false;
        if (PF_OP_WRITES_B(op) && d >= PF_NB) return false;
        if (((op >= PF_B_AND && op <= PF_B_ITE) || op == PF_B_SPILL || op == PF_ASSERT) && a >= PF_NB) return false;
        if (((op >= PF_B_AND && op <= PF_B_XOR) || op == PF_B_ITE) && b >= PF_NB) return false;
        if ((op == PF_W_ITE || op == PF_B_ITE) && c >= PF_NB) return false;
        if ((op == PF_W_SPILL || op == PF_W_FILL || op == PF_B_SPILL || op == PF_B_FILL) && aux0 >= PF_MAX_SPILL)
            return false;
        if ((op == PF_W_EXTRACT || op == PF_W_CONCAT) && aux0 >= 256u) return false;
    }
    return true;
}

// One set's program P (n instructions, traffic / unit bits set) folded in place; drop[i] = 1
// for every instruction the device program leaves out.  pool: the set's constants (n_pool x 8
// u32), or null when the caller passed none (then no constant is known).  extra (may be null):
// receives the constants of the device program's own, 8 u32 each; the k-th has index
// n_pool + k, one entry per value.
inline void fold_program(uint32_t* P, uint32_t n, uint8_t* drop, const uint32_t* pool, uint32_t n_pool,
                         Scratch& T, std::vector<uint32_t>* extra = nullptr) {
    if (!well_formed(P, n)) return;
    // A program that reads no variable stays as lowered.  Its verdict is one constant, which no
    // query sends (z3's simplify and the lowering have folded it away); the per-operation
    // kernel tests send them on purpose: constant operands are wave-uniform, the way into the
    // uniform shortcuts of the divider and of EXP, and folding would test the host instead.
    bool ground = true;
    for (uint32_t i = 0; i + 1 < n && ground; i++) {
        const uint32_t op = P[4 * (size_t)i] & 0xffu;
        ground = op != PF_W_VAR && op != PF_B_VAR;
    }
    if (ground) return;
    T.zero.assign(n, 0);
    T.zreg.assign(n, 0xff);
    T.written.assign(n, 0);
    T.keys.clear();
    T.next.clear();
    size_t hs = 16;
    while (hs < 2 * (size_t)n) hs <<= 1;
    T.heads.assign(hs, -1);
    T.n_vn = 0;
    for (WV& x : T.W) x = WV{0, 256, T.fresh(), uzero()};
    for (BV& x : T.B) x = BV{0, 0, T.fresh()};
    for (SV& x : T.S) x = SV{0, WV{0, 256, T.fresh(), uzero()}, BV{0, 0, T.fresh()}};

    auto pool_index = [&](const U& v) -> int64_t {
        for (uint32_t k = 0; pool && k < n_pool; k++)
            if (memcmp(pool + 8 * (size_t)k, v.l, 32) == 0) return k;
        return -1;
    };
    const size_t extra0 = extra ? extra->size() : 0;  // this set's own constants start here
    auto own_index = [&](const U& v) -> uint32_t {
        for (size_t k = extra0; k < extra->size(); k += 8)
            if (memcmp(extra->data() + k, v.l, 32) == 0) return n_pool + (uint32_t)((k - extra0) / 8);
        extra->insert(extra->end(), v.l, v.l + 8);
        return n_pool + (uint32_t)((extra->size() - extra0) / 8) - 1u;
    };
    constexpr uint8_t OWN_PENDING = 2;  // T.zero[i]: a W_CONST whose aux0 is an entry of T.own, no index yet
    T.own.clear();
    uint16_t written = 0;

    // ---- forward: what every result is, and the rewrites that need no liveness
    for (uint32_t i = 0; i + 1 < n; i++) {
        uint32_t* I = P + 4 * (size_t)i;
        const uint32_t op = I[0] & 0xffu, w = (I[0] >> 8) & 0x3ffu, aux0 = I[2];
        const uint32_t d = I[1] & 0xffu, a = (I[1] >> 8) & 0xffu, b = (I[1] >> 16) & 0xffu, c = I[1] >> 24;
        const uint32_t opw = I[0] & 0x3ffffu;
        T.written[i] = written;

        // a W result: constant val / the value of operand register src / a numbered unknown
        auto w_const = [&](const U& val, uint32_t operand) {
            T.W[d] = WV{1, (uint16_t)ubitlen(val), T.fresh(), val};
            written |= (uint16_t)(1u << d);
            if (op == PF_W_CONST) return;
            const int64_t k = pool_index(val);
            if (k >= 0) {
                I[0] = mk_w0(PF_W_CONST, w);
                I[1] = d;
                I[2] = (uint32_t)k;
            } else if (uis0(val)) {
                T.zero[i] = 1;
                T.zreg[i] = (uint8_t)operand;
            } else if (extra) {  // its index once the backward walk has kept it
                I[0] = mk_w0(PF_W_CONST, w);
                I[1] = d;
                I[2] = (uint32_t)T.own.size();
                T.own.push_back(val);
                T.zero[i] = OWN_PENDING;
            }
        };
        auto w_copy = [&](uint32_t src) {
            const WV v = T.W[src];
            if (op != PF_W_MOV) {
                if (src == d) {
                    drop[i] = 1;  // the register keeps the value it has
                    return;
                }
                I[0] = mk_w0(PF_W_MOV, w);
                I[1] = d | (src << 8);
                I[2] = 0;
            }
            T.W[d] = v;
            written |= (uint16_t)(1u << d);
        };
        auto w_unknown = [&](uint32_t vn, uint32_t bound) {
            T.W[d] = WV{0, (uint16_t)bound, vn, uzero()};
            written |= (uint16_t)(1u << d);
        };
        auto b_const = [&](bool v) {
            T.B[d] = BV{1, (uint8_t)v, T.fresh()};
            if (op == PF_B_CONST) return;
            I[0] = mk_w0(PF_B_CONST, w);
            I[1] = d;
            I[2] = v ? 1u : 0u;
        };
        auto b_unknown = [&](uint32_t vn) { T.B[d] = BV{0, 0, vn}; };

        if (is_wbin(op)) {
            const WV A = T.W[a], B = T.W[b];
            if (A.bound > w || B.bound > w) {  // not the typed program the rules speak of
                w_unknown(T.fresh(), 256);
                continue;
            }
            const bool ca = A.konst, cb = B.konst, same = A.vn == B.vn;
            const bool za = ca && uis0(A.v), zb = cb && uis0(B.v);
            const bool oa = ca && uis1(A.v), ob = cb && uis1(B.v);
            const bool ma = ca && ueq(A.v, uones(w)), mb = cb && ueq(B.v, uones(w));
            // the register of a constant operand: the cheaper writer to keep for a zero
            const uint32_t zr = cb ? b : a;
            enum { NONE, ZERO, ONE, ONES, CA, CB } r = NONE;
            if (ca && cb) {
                w_const(eval_wbin(op, A.v, B.v, w), zr);
                continue;
            }
            switch (op) {
                case PF_W_ADD: r = za ? CB : zb ? CA : NONE; break;
                case PF_W_SUB: r = same ? ZERO : zb ? CA : NONE; break;
                case PF_W_MUL: r = (za || zb) ? ZERO : oa ? CB : ob ? CA : NONE; break;
                case PF_W_UDIV: r = zb ? ONES : ob ? CA : NONE; break;
                case PF_W_SDIV: r = ob ? CA : NONE; break;
                case PF_W_UREM:
                case PF_W_SREM:
                case PF_W_SMOD: r = (same || za || ob) ? ZERO : zb ? CA : NONE; break;
                case PF_W_AND: r = (za || zb) ? ZERO : same ? CA : ma ? CB : mb ? CA : NONE; break;
                case PF_W_OR: r = (ma || mb) ? ONES : same ? CA : za ? CB : zb ? CA : NONE; break;
                case PF_W_XOR: r = same ? ZERO : za ? CB : zb ? CA : NONE; break;
                case PF_W_SHL:
                case PF_W_LSHR: r = (za || (cb && ushamt(B.v, w) >= w)) ? ZERO : zb ? CA : NONE; break;
                case PF_W_ASHR: r = za ? ZERO : zb ? CA : NONE; break;
                default: r = (zb || oa) ? ONE : ob ? CA : NONE; break;  // PF_W_EXP
            }
            if (r == NONE) {  // the range of the unknown operand against the constant one
                const bool a_low = ca && ueq(umask(A.v, B.bound), uones(B.bound));
                const bool b_low = cb && ueq(umask(B.v, A.bound), uones(A.bound));
                switch (op) {
                    case PF_W_UDIV: r = cb && ubitlen(B.v) > A.bound ? ZERO : NONE; break;
                    case PF_W_UREM: r = cb && ubitlen(B.v) > A.bound ? CA : NONE; break;
                    case PF_W_AND: r = b_low ? CA : a_low ? CB : NONE; break;
                    case PF_W_LSHR: r = cb && ushamt(B.v, w) >= A.bound ? ZERO : NONE; break;
                    default: break;
                }
            }
            const uint32_t bd = r == NONE ? result_bound(op, A.bound, B.bound, cb, B.v, w) : w;
            if (r == NONE && bd == 0) r = ZERO;
            switch (r) {
                case ZERO: w_const(uzero(), zr); break;
                case ONE: w_const(usmall(1), zr); break;
                case ONES: w_const(uones(w), zr); break;
                case CA: w_copy(a); break;
                case CB: w_copy(b); break;
                default: w_unknown(T.number(opw, A.vn, B.vn, 0, 0), bd); break;
            }
            continue;
        }
        if (is_cmp(op) || op == PF_B_UMUL_NOOVF) {
            const WV A = T.W[a], B = T.W[b];
            if (A.bound > w || B.bound > w) {
                b_unknown(T.fresh());
                continue;
            }
            const bool same = A.vn == B.vn;
            if (op == PF_B_UMUL_NOOVF) {  // a factor of 0 or 1 cannot overflow
                if ((A.konst && A.bound <= 1) || (B.konst && B.bound <= 1)) b_const(true);
                else b_unknown(T.number(opw, A.vn, B.vn, 0, 0));
            } else if (A.konst && B.konst) {
                b_const(eval_cmp(op, A.v, B.v, w));
            } else if (same && op != PF_B_UADD_NOOVF) {
                b_const(op == PF_B_EQ || op == PF_B_ULE || op == PF_B_SLE);
            } else {
                // below 2^(w-1) on both sides: no carry out of w bits, and signed order is unsigned order
                const bool small = A.bound < w && B.bound < w;
                const uint32_t uop = op == PF_B_SLT ? PF_B_ULT : op == PF_B_SLE ? PF_B_ULE : op;
                int verdict = -1;
                if (op == PF_B_UADD_NOOVF) verdict = small ? 1 : -1;
                else if (A.konst != B.konst && (uop == op || small))
                    verdict = B.konst ? range_cmp(uop, true, A.bound, B.v, w) : range_cmp(uop, false, B.bound, A.v, w);
                if (verdict >= 0) b_const(verdict != 0);
                else b_unknown(T.number(opw, A.vn, B.vn, 0, 0));
            }
            continue;
        }
        switch (op) {
            case PF_W_CONST:
                if (pool && aux0 < n_pool) {
                    U v;
                    memcpy(v.l, pool + 8 * (size_t)aux0, 32);
                    w_const(umask(v, w), 0xff);
                } else {
                    w_unknown(T.number(opw, 0, 0, 0, aux0), w);
                }
                break;
            case PF_W_VAR: w_unknown(T.number(opw, 0, 0, 0, aux0), w); break;
            case PF_W_MOV: {
                const WV A = T.W[a];
                if (A.bound <= w) w_copy(a);
                else if (A.konst) w_const(umask(A.v, w), a);
                else w_unknown(T.number(opw, A.vn, 0, 0, 0), w);
                break;
            }
            case PF_W_NOT:
            case PF_W_NEG: {
                const WV A = T.W[a];
                if (A.bound > w) w_unknown(T.fresh(), 256);
                else if (A.konst) w_const(umask(op == PF_W_NOT ? unot(A.v) : uneg(A.v), w), a);
                else w_unknown(T.number(opw, A.vn, 0, 0, 0), w);
                break;
            }
            case PF_W_EXTRACT: {
                const WV A = T.W[a];
                const uint32_t bd = A.bound > aux0 ? A.bound - aux0 : 0u;
                if (A.konst) w_const(umask(ulshr(A.v, aux0), w), a);
                else if (bd == 0) w_const(uzero(), a);
                else w_unknown(T.number(opw, A.vn, 0, 0, aux0), bd < w ? bd : w);
                break;
            }
            case PF_W_CONCAT: {
                const WV A = T.W[a], B = T.W[b];
                if (A.konst && B.konst && B.bound <= aux0) {
                    U v = ushl(A.v, aux0);
                    for (int j = 0; j < 8; j++) v.l[j] |= B.v.l[j];
                    w_const(umask(v, w), b);
                } else {
                    w_unknown(T.number(opw, A.vn, B.vn, 0, aux0), w);
                }
                break;
            }
            case PF_W_SEXT: {
                const WV A = T.W[a];
                if (A.konst && aux0 >= 1 && aux0 <= w && A.bound <= aux0) {
                    U v = A.v;
                    if (ubit(v, aux0 - 1))
                        for (uint32_t k = aux0; k < w; k++) v.l[k / 32] |= 1u << (k % 32);
                    w_const(v, a);
                } else {
                    w_unknown(T.number(opw, A.vn, 0, 0, aux0), w);
                }
                break;
            }
            case PF_W_ITE: {
                const WV A = T.W[a], B = T.W[b];
                const BV C = T.B[c];
                if (A.bound > w || B.bound > w) w_unknown(T.fresh(), 256);
                else if (C.konst) w_copy(C.v ? a : b);
                else if (A.vn == B.vn) w_copy(a);
                else if (A.konst && B.konst && ueq(A.v, B.v)) w_const(A.v, a);
                else w_unknown(T.number(opw, A.vn, B.vn, C.vn, 0), A.bound > B.bound ? A.bound : B.bound);
                break;
            }
            case PF_W_HASH: w_unknown(T.number(opw, T.W[a].vn, 0, 0, aux0), w); break;
            case PF_W_SPILL: T.S[aux0] = SV{0, T.W[a], BV{0, 0, 0}}; break;
            case PF_W_FILL: {
                const SV s = T.S[aux0];
                if (!s.is_b && s.w.bound <= w) {  // the value the slot holds, unchanged
                    if (s.w.konst) w_const(s.w.v, 0xff);
                    else w_unknown(s.w.vn, s.w.bound);
                } else if (!s.is_b && s.w.konst) {
                    w_const(umask(s.w.v, w), 0xff);
                } else {
                    w_unknown(T.fresh(), w);
                }
                break;
            }
            case PF_B_CONST: b_const(aux0 & 1u); break;
            case PF_B_VAR: b_unknown(T.number(opw, 0, 0, 0, aux0)); break;
            case PF_B_AND:
            case PF_B_OR: {
                const BV A = T.B[a], B = T.B[b];
                const uint8_t absorb = op == PF_B_AND ? 0 : 1;  // the value that decides the result
                if ((A.konst && A.v == absorb) || (B.konst && B.v == absorb)) b_const(absorb);
                else if (A.konst && B.konst) b_const(!absorb);
                else if (A.konst) T.B[d] = B;  // the neutral value: the other operand
                else if (B.konst || A.vn == B.vn) T.B[d] = A;
                else b_unknown(T.number(opw, A.vn, B.vn, 0, 0));
                break;
            }
            case PF_B_XOR: {
                const BV A = T.B[a], B = T.B[b];
                if (A.konst && B.konst) b_const(A.v != B.v);
                else if (A.vn == B.vn) b_const(false);
                else if (A.konst && !A.v) T.B[d] = B;
                else if (B.konst && !B.v) T.B[d] = A;
                else b_unknown(T.number(opw, A.vn, B.vn, 0, 0));
                break;
            }
            case PF_B_NOT: {
                const BV A = T.B[a];
                if (A.konst) b_const(!A.v);
                else b_unknown(T.number(opw, A.vn, 0, 0, 0));
                break;
            }
            case PF_B_ITE: {
                const BV A = T.B[a], B = T.B[b], C = T.B[c];
                const BV* arm = C.konst ? (C.v ? &A : &B) : (A.vn == B.vn ? &A : nullptr);
                if (!arm && A.konst && B.konst && A.v == B.v) arm = &A;
                if (arm && arm->konst) b_const(arm->v);
                else if (arm) T.B[d] = *arm;
                else b_unknown(T.number(opw, A.vn, B.vn, C.vn, 0));
                break;
            }
            case PF_B_SPILL: T.S[aux0] = SV{1, WV{0, 256, 0, uzero()}, T.B[a]}; break;
            case PF_B_FILL: {
                const SV s = T.S[aux0];
                if (s.is_b && s.b.konst) b_const(s.b.v);
                else if (s.is_b) T.B[d] = s.b;
                else if (s.w.konst) b_const(s.w.v.l[0] & 1u);
                else b_unknown(T.fresh());
                break;
            }
            default:  // PF_ASSERT
                if (T.B[a].konst && T.B[a].v) drop[i] = 1;
                break;
        }
    }

    // ---- backward: keep what the ASSERTs need, and give each kept zero its register
    uint32_t live_w = 0, live_b = 0;
    uint64_t live_s = 0;
    for (uint32_t i = n - 1; i-- > 0;) {
        if (drop[i]) continue;
        uint32_t* I = P + 4 * (size_t)i;
        uint32_t op = I[0] & 0xffu;
        const uint32_t w = (I[0] >> 8) & 0x3ffu, d = I[1] & 0xffu;
        bool keep = true;
        if (op == PF_W_SPILL || op == PF_B_SPILL) {
            keep = (live_s >> I[2]) & 1u;
            live_s &= ~(1ull << I[2]);
        } else if (pf_op_traffic(op) & PF_TR_WW) {
            keep = (live_w >> d) & 1u;
            live_w &= ~(1u << d);
        } else if (PF_OP_WRITES_B(op)) {
            keep = (live_b >> d) & 1u;
            live_b &= ~(1u << d);
        }
        if (!keep) {
            drop[i] = 1;
            continue;
        }
        if (T.zero[i] == 1) {
            // a register that is live here anyway costs nothing; else an operand of the
            // instruction (one writer stays instead of the datapath op and both)
            const uint32_t free_r = live_w & T.written[i] & ~(1u << d);
            const uint32_t r = free_r ? (uint32_t)__builtin_ctz(free_r) : T.zreg[i];
            if (r < PF_NW) {
                I[0] = mk_w0(PF_W_XOR, w);
                I[1] = d | (r << 8) | (r << 16);
                I[2] = 0;
                op = PF_W_XOR;
            }
        }
        const uint32_t tr = pf_op_traffic(op);
        const uint32_t a = (I[1] >> 8) & 0xffu, b = (I[1] >> 16) & 0xffu, c = I[1] >> 24;
        if (tr & PF_TR_RA) live_w |= 1u << a;
        if (tr & PF_TR_RB) live_w |= 1u << b;
        if ((op >= PF_B_AND && op <= PF_B_ITE) || op == PF_B_SPILL || op == PF_ASSERT) live_b |= 1u << a;
        if ((op >= PF_B_AND && op <= PF_B_XOR) || op == PF_B_ITE) live_b |= 1u << b;
        if (op == PF_W_ITE || op == PF_B_ITE) live_b |= 1u << c;
        if (op == PF_W_FILL || op == PF_B_FILL) live_s |= 1ull << I[2];
    }

    // ---- the kept constants of the program's own get their indices, in program order
    for (uint32_t i = 0; i + 1 < n && !T.own.empty(); i++) {
        uint32_t* I = P + 4 * (size_t)i;
        if (!drop[i] && T.zero[i] == OWN_PENDING) I[2] = own_index(T.own[I[2]]);
    }
}

}  // namespace pf_fold

#endif /* PF_FOLD_H */
