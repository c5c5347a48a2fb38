/*
 * pf_fold.h — constant folding, x-op-x identities and dead-code removal over one set's lowered
 * program, the first of pf_batch_create's device-program rewrites (pf_devprog.h
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
 * What an instruction is on constants is pf_hostint.h's eval_op, the evaluator the hint solver
 * shares; constants are its 256-bit integers, converted where they meet a pool's 8 x u32.
 */
#ifndef PF_FOLD_H
#define PF_FOLD_H

#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/pf_bytecode.h"
#include "pf_hostint.h"

namespace pf_fold {

using pf_host::bitlen;
using pf_host::eval_op;
using pf_host::lt;
using pf_host::mask;
using pf_host::mw;
using pf_host::U;

// the value of a register shift amount when it is below w, else w
inline uint32_t ushamt(const U& b, uint32_t w) { return lt(b, U::of(w)) ? (uint32_t)b.w[0] : w; }
// op(a, b) of an opcode the evaluator knows, which every caller below has checked
inline U eval(uint32_t op, uint32_t w, uint32_t aux, const U& a, const U& b = U()) {
    U r;
    eval_op(op, w, aux, a, b, &r);
    return r;
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

inline uint32_t mk_w0(uint32_t op, uint32_t w) { return pf_ins_stamp(op | (w << 8)); }

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
            if (cb && !bv.zero() && bitlen(bv) < bd) bd = bitlen(bv);
            break;
        case PF_W_UDIV:
            if (cb && !bv.zero()) bd = pa >= bitlen(bv) ? pa - bitlen(bv) + 1u : 0u;
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
    const bool above = bitlen(c) > p;  // c >= 2^p
    if (op == PF_B_EQ) return above ? 0 : -1;
    if (x_left) {
        if (op == PF_B_ULT) return c.zero() ? 0 : above ? 1 : -1;
        return above || c == mask(p) ? 1 : -1;  // x <= c for c >= 2^p - 1
    }
    if (op == PF_B_ULE) return c.zero() ? 1 : above ? 0 : -1;
    return above || c == mask(w) ? 0 : -1;  // c < x
}

// The pass can reason about the program: it ends with its only END, every opcode is known,
// every register, slot and width is in range, and no device flag is set yet.
inline bool well_formed(const uint32_t* P, uint32_t n) {
    if (n == 0 || pf_ins_op(P[4 * (size_t)(n - 1)]) != PF_END) return false;
    for (uint32_t i = 0; i + 1 < n; i++) {
        const uint32_t w0 = P[4 * (size_t)i], w1 = P[4 * (size_t)i + 1], aux0 = P[4 * (size_t)i + 2];
        const uint32_t op = pf_ins_op(w0), w = pf_ins_width(w0), tr = pf_op_traffic(op);
        const uint32_t d = pf_ins_dst(w1), a = pf_ins_a(w1), b = pf_ins_b(w1), c = pf_ins_c(w1);
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
        const uint32_t op = pf_ins_op(P[4 * (size_t)i]);
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
    for (WV& x : T.W) x = WV{0, 256, T.fresh(), U()};
    for (BV& x : T.B) x = BV{0, 0, T.fresh()};
    for (SV& x : T.S) x = SV{0, WV{0, 256, T.fresh(), U()}, BV{0, 0, T.fresh()}};

    auto pool_index = [&](const U& v) -> int64_t {
        uint32_t l[8];
        v.to32(l);
        for (uint32_t k = 0; pool && k < n_pool; k++)
            if (memcmp(pool + 8 * (size_t)k, l, 32) == 0) return k;
        return -1;
    };
    const size_t extra0 = extra ? extra->size() : 0;  // this set's own constants start here
    auto own_index = [&](const U& v) -> uint32_t {
        uint32_t l[8];
        v.to32(l);
        for (size_t k = extra0; k < extra->size(); k += 8)
            if (memcmp(extra->data() + k, l, 32) == 0) return n_pool + (uint32_t)((k - extra0) / 8);
        extra->insert(extra->end(), l, l + 8);
        return n_pool + (uint32_t)((extra->size() - extra0) / 8) - 1u;
    };
    constexpr uint8_t OWN_PENDING = 2;  // T.zero[i]: a W_CONST whose aux0 is an entry of T.own, no index yet
    T.own.clear();
    uint16_t written = 0;

    // ---- forward: what every result is, and the rewrites that need no liveness
    for (uint32_t i = 0; i + 1 < n; i++) {
        uint32_t* I = P + 4 * (size_t)i;
        const uint32_t op = pf_ins_op(I[0]), w = pf_ins_width(I[0]), aux0 = I[2];
        const uint32_t d = pf_ins_dst(I[1]), a = pf_ins_a(I[1]), b = pf_ins_b(I[1]), c = pf_ins_c(I[1]);
        const uint32_t opw = I[0] & 0x3ffffu;
        T.written[i] = written;

        // a W result: constant val / the value of operand register src / a numbered unknown
        auto w_const = [&](const U& val, uint32_t operand) {
            T.W[d] = WV{1, (uint16_t)bitlen(val), T.fresh(), val};
            written |= (uint16_t)(1u << d);
            if (op == PF_W_CONST) return;
            const int64_t k = pool_index(val);
            if (k >= 0) {
                I[0] = mk_w0(PF_W_CONST, w);
                I[1] = d;
                I[2] = (uint32_t)k;
            } else if (val.zero()) {
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
            T.W[d] = WV{0, (uint16_t)bound, vn, U()};
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
            const bool za = ca && A.v.zero(), zb = cb && B.v.zero();
            const bool oa = ca && A.v == U::of(1), ob = cb && B.v == U::of(1);
            const bool ma = ca && A.v == mask(w), mb = cb && B.v == mask(w);
            // the register of a constant operand: the cheaper writer to keep for a zero
            const uint32_t zr = cb ? b : a;
            enum { NONE, ZERO, ONE, ONES, CA, CB } r = NONE;
            if (ca && cb) {
                w_const(eval(op, w, 0, A.v, B.v), zr);
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
                const bool a_low = ca && mw(A.v, B.bound) == mask(B.bound);
                const bool b_low = cb && mw(B.v, A.bound) == mask(A.bound);
                switch (op) {
                    case PF_W_UDIV: r = cb && bitlen(B.v) > A.bound ? ZERO : NONE; break;
                    case PF_W_UREM: r = cb && bitlen(B.v) > A.bound ? CA : NONE; break;
                    case PF_W_AND: r = b_low ? CA : a_low ? CB : NONE; break;
                    case PF_W_LSHR: r = cb && ushamt(B.v, w) >= A.bound ? ZERO : NONE; break;
                    default: break;
                }
            }
            const uint32_t bd = r == NONE ? result_bound(op, A.bound, B.bound, cb, B.v, w) : w;
            if (r == NONE && bd == 0) r = ZERO;
            switch (r) {
                case ZERO: w_const(U(), zr); break;
                case ONE: w_const(U::of(1), zr); break;
                case ONES: w_const(mask(w), zr); break;
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
                b_const(!eval(op, w, 0, A.v, B.v).zero());
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
                    w_const(mw(U::from32(pool + 8 * (size_t)aux0), w), 0xff);
                } else {
                    w_unknown(T.number(opw, 0, 0, 0, aux0), w);
                }
                break;
            case PF_W_VAR: w_unknown(T.number(opw, 0, 0, 0, aux0), w); break;
            case PF_W_MOV: {
                const WV A = T.W[a];
                if (A.bound <= w) w_copy(a);
                else if (A.konst) w_const(mw(A.v, w), a);
                else w_unknown(T.number(opw, A.vn, 0, 0, 0), w);
                break;
            }
            case PF_W_NOT:
            case PF_W_NEG: {
                const WV A = T.W[a];
                if (A.bound > w) w_unknown(T.fresh(), 256);
                else if (A.konst) w_const(eval(op, w, 0, A.v), a);
                else w_unknown(T.number(opw, A.vn, 0, 0, 0), w);
                break;
            }
            case PF_W_EXTRACT: {
                const WV A = T.W[a];
                const uint32_t bd = A.bound > aux0 ? A.bound - aux0 : 0u;
                if (A.konst) w_const(eval(op, w, aux0, A.v), a);
                else if (bd == 0) w_const(U(), a);
                else w_unknown(T.number(opw, A.vn, 0, 0, aux0), bd < w ? bd : w);
                break;
            }
            case PF_W_CONCAT: {
                const WV A = T.W[a], B = T.W[b];
                if (A.konst && B.konst && B.bound <= aux0) {
                    w_const(eval(op, w, aux0, A.v, B.v), b);
                } else {
                    w_unknown(T.number(opw, A.vn, B.vn, 0, aux0), w);
                }
                break;
            }
            case PF_W_SEXT: {
                const WV A = T.W[a];
                if (A.konst && aux0 >= 1 && aux0 <= w && A.bound <= aux0) {
                    w_const(eval(op, w, aux0, A.v), a);
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
                else if (A.konst && B.konst && A.v == B.v) w_const(A.v, a);
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
                    w_const(mw(s.w.v, w), 0xff);
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
            case PF_B_SPILL: T.S[aux0] = SV{1, WV{0, 256, 0, U()}, T.B[a]}; break;
            case PF_B_FILL: {
                const SV s = T.S[aux0];
                if (s.is_b && s.b.konst) b_const(s.b.v);
                else if (s.is_b) T.B[d] = s.b;
                else if (s.w.konst) b_const(s.w.v.w[0] & 1u);
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
        uint32_t op = pf_ins_op(I[0]);
        const uint32_t w = pf_ins_width(I[0]), d = pf_ins_dst(I[1]);
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
        const uint32_t a = pf_ins_a(I[1]), b = pf_ins_b(I[1]), c = pf_ins_c(I[1]);
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
