/*
 * pf_hostint.h — the host's 256-bit integers and its one evaluator of bytecode opcodes on
 * them: what op(a, b) is at width w under the total-division conventions of
 * include/pf_bytecode.h.  The fold pass of device programs (pf_fold.h), the hint solver
 * (pf_seed.cpp), Power's concrete facts (pf_terms.cpp) and the planted values of the config-3
 * generator (pf_synth.cpp) all ask it; so a new opcode or convention is written here once,
 * and so are the algorithms that make it fast: Knuth's algorithm D on 64-bit digits, the low
 * half of a product alone, powers that stop at the exponent's top bit.  Also the keyed hash
 * behind PF_W_HASH (two Philox4x32-10 blocks) and zlib's CRC-32, which salts it with a
 * function's name.  tests/test_host_ops.py pins every opcode against the golden vectors and
 * the Python oracle.
 * Host C++ only, header-only, no HIP.  Values are 4 x u64 limbs, little-endian; constant
 * pools keep 8 x u32 (from32 / to32).
 */
#ifndef PF_HOSTINT_H
#define PF_HOSTINT_H

#include <stdint.h>

#include <string>

#include "../../include/pf_bytecode.h"

namespace pf_host {

// ---- 256-bit unsigned --------------------------------------------------------------------
struct U {
    uint64_t w[4] = {0, 0, 0, 0};
    static U from32(const uint32_t* p) {
        U r;
        for (int i = 0; i < 4; i++) r.w[i] = (uint64_t)p[2 * i] | ((uint64_t)p[2 * i + 1] << 32);
        return r;
    }
    static U of(uint64_t v) {
        U r;
        r.w[0] = v;
        return r;
    }
    void to32(uint32_t* p) const {
        for (int i = 0; i < 4; i++) {
            p[2 * i] = (uint32_t)w[i];
            p[2 * i + 1] = (uint32_t)(w[i] >> 32);
        }
    }
    bool zero() const { return !(w[0] | w[1] | w[2] | w[3]); }
    bool operator==(const U& o) const { return w[0] == o.w[0] && w[1] == o.w[1] && w[2] == o.w[2] && w[3] == o.w[3]; }
    bool operator!=(const U& o) const { return !(*this == o); }
};

inline int cmp(const U& a, const U& b) {
    for (int i = 3; i >= 0; i--)
        if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
    return 0;
}
inline bool lt(const U& a, const U& b) { return cmp(a, b) < 0; }
inline bool le(const U& a, const U& b) { return cmp(a, b) <= 0; }
inline U uand(const U& a, const U& b) { U r; for (int i = 0; i < 4; i++) r.w[i] = a.w[i] & b.w[i]; return r; }
inline U uor(const U& a, const U& b) { U r; for (int i = 0; i < 4; i++) r.w[i] = a.w[i] | b.w[i]; return r; }
inline U uxor(const U& a, const U& b) { U r; for (int i = 0; i < 4; i++) r.w[i] = a.w[i] ^ b.w[i]; return r; }
inline U unot(const U& a) { U r; for (int i = 0; i < 4; i++) r.w[i] = ~a.w[i]; return r; }
inline U add(const U& a, const U& b, uint64_t* carry = nullptr) {
    U r;
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; i++) {
        c += (unsigned __int128)a.w[i] + b.w[i];
        r.w[i] = (uint64_t)c;
        c >>= 64;
    }
    if (carry) *carry = (uint64_t)c;
    return r;
}
inline U sub(const U& a, const U& b) {
    U r;
    uint64_t br = 0;
    for (int i = 0; i < 4; i++) {
        const uint64_t x = a.w[i], y = b.w[i];
        const uint64_t d = x - y - br;
        br = (x < y) || (x - y < br);
        r.w[i] = d;
    }
    return r;
}
inline U neg(const U& a) { return sub(U(), a); }
inline U shl(const U& a, unsigned k) {
    U r;
    if (k >= 256) return r;
    const unsigned q = k / 64, s = k % 64;
    for (int i = 3; i >= 0; i--) {
        const int j = i - (int)q;
        uint64_t v = 0;
        if (j >= 0) {
            v = a.w[j] << s;
            if (s && j >= 1) v |= a.w[j - 1] >> (64 - s);
        }
        r.w[i] = v;
    }
    return r;
}
inline U shr(const U& a, unsigned k) {
    U r;
    if (k >= 256) return r;
    const unsigned q = k / 64, s = k % 64;
    for (int i = 0; i < 4; i++) {
        const unsigned j = i + q;
        uint64_t v = 0;
        if (j < 4) {
            v = a.w[j] >> s;
            if (s && j + 1 < 4) v |= a.w[j + 1] << (64 - s);
        }
        r.w[i] = v;
    }
    return r;
}
inline U mask_slow(unsigned w) {
    if (w >= 256) return unot(U());
    return sub(shl(U::of(1), w), U::of(1));
}
struct MaskTable {
    U m[257];
    MaskTable() {
        for (unsigned w = 0; w <= 256; w++) m[w] = mask_slow(w);
    }
};
inline const U& mask(unsigned w) {  // 2^w - 1
    static const MaskTable t;
    return t.m[w >= 256 ? 256 : w];
}
inline U mw(const U& a, unsigned w) { return uand(a, mask(w)); }
inline unsigned bitlen(const U& a) {
    for (int i = 3; i >= 0; i--)
        if (a.w[i]) return 64 * i + 64 - __builtin_clzll(a.w[i]);
    return 0;
}
inline bool bit(const U& a, unsigned k) { return k < 256 && ((a.w[k / 64] >> (k % 64)) & 1u); }
// full 512-bit product (lo, hi)
inline void mul_full(const U& a, const U& b, U* lo, U* hi) {
    uint64_t r[8] = {0};
    for (int i = 0; i < 4; i++) {
        unsigned __int128 c = 0;
        for (int j = 0; j < 4; j++) {
            c += (unsigned __int128)a.w[i] * b.w[j] + r[i + j];
            r[i + j] = (uint64_t)c;
            c >>= 64;
        }
        r[i + 4] = (uint64_t)c;
    }
    for (int i = 0; i < 4; i++) {
        lo->w[i] = r[i];
        hi->w[i] = r[i + 4];
    }
}
inline U mul(const U& a, const U& b) {  // the low 256 bits alone: 10 limb products
    U r;
    for (int i = 0; i < 4; i++) {
        unsigned __int128 c = 0;
        for (int j = 0; i + j < 4; j++) {
            c += (unsigned __int128)a.w[i] * b.w[j] + r.w[i + j];
            r.w[i + j] = (uint64_t)c;
            c >>= 64;
        }
    }
    return r;
}
inline void divmod(const U& a, const U& b, U* q, U* r) {  // b != 0
    if (lt(a, b)) {
        *q = U();
        *r = a;
        return;
    }
    if (!(b.w[1] | b.w[2] | b.w[3])) {  // one-limb divisor: 128/64 steps
        const uint64_t d = b.w[0];
        U Q;
        unsigned __int128 rem = 0;
        for (int i = 3; i >= 0; i--) {
            const unsigned __int128 cur = (rem << 64) | a.w[i];
            Q.w[i] = (uint64_t)(cur / d);
            rem = cur % d;
        }
        *q = Q;
        *r = U::of((uint64_t)rem);
        return;
    }
    // Knuth's algorithm D on 64-bit digits (Hacker's Delight divmnu): n >= 2 digits of b
    // under m >= n of a, both shifted so that b's top digit has its top bit set
    typedef unsigned __int128 u128;
    int n = 4, m = 4;
    while (!b.w[n - 1]) n--;
    while (!a.w[m - 1]) m--;
    const int s = __builtin_clzll(b.w[n - 1]);
    uint64_t vn[4], un[5];
    for (int i = n - 1; i > 0; i--) vn[i] = (b.w[i] << s) | (s ? b.w[i - 1] >> (64 - s) : 0);
    vn[0] = b.w[0] << s;
    un[m] = s ? a.w[m - 1] >> (64 - s) : 0;
    for (int i = m - 1; i > 0; i--) un[i] = (a.w[i] << s) | (s ? a.w[i - 1] >> (64 - s) : 0);
    un[0] = a.w[0] << s;
    U Q, R;
    for (int j = m - n; j >= 0; j--) {
        // the digit's estimate from the top two digits over b's top one, at most 2 too large
        // once the third digit is looked at; a top digit equal to b's makes it 2^64 - 1
        uint64_t qhat = ~0ull;
        u128 rhat = (u128)un[j + n - 1] + vn[n - 1];
        if (un[j + n] < vn[n - 1]) {
            const u128 num = ((u128)un[j + n] << 64) | un[j + n - 1];
            qhat = (uint64_t)(num / vn[n - 1]);
            rhat = num - (u128)qhat * vn[n - 1];
        }
        while (!(rhat >> 64) && (u128)qhat * vn[n - 2] > ((rhat << 64) | un[j + n - 2])) {
            qhat--;
            rhat += vn[n - 1];
        }
        uint64_t k = 0;  // un[j .. j + n] -= qhat * vn
        for (int i = 0; i < n; i++) {
            const u128 p = (u128)qhat * vn[i] + k;
            const uint64_t x = un[i + j], lo = (uint64_t)p;
            un[i + j] = x - lo;
            k = (uint64_t)(p >> 64) + (x < lo);
        }
        const bool over = un[j + n] < k;
        un[j + n] -= k;
        if (over) {  // one too large still: add b back
            qhat--;
            u128 c = 0;
            for (int i = 0; i < n; i++) {
                c += (u128)un[i + j] + vn[i];
                un[i + j] = (uint64_t)c;
                c >>= 64;
            }
            un[j + n] += (uint64_t)c;
        }
        Q.w[j] = qhat;
    }
    for (int i = 0; i < n - 1; i++) R.w[i] = (un[i] >> s) | (s ? un[i + 1] << (64 - s) : 0);
    R.w[n - 1] = un[n - 1] >> s;
    *q = Q;
    *r = R;
}
inline U powmod(U a, const U& e, unsigned w) {  // a^e mod 2^w
    const unsigned n = bitlen(e);
    if (!(a.w[0] & 1u) && n > 8) return U();  // even base, e >= 256: 2^256 divides the power
    U r = U::of(1);
    for (unsigned k = 0; k < n; k++) {
        if (bit(e, k)) r = mul(r, a);
        if (k + 1 < n) a = mul(a, a);
    }
    return mw(r, w);
}
inline bool negw(const U& a, unsigned w) { return w >= 1 && bit(a, w - 1); }
inline U absw(const U& a, unsigned w) { return negw(a, w) ? mw(neg(a), w) : a; }

// ---- PF_W_HASH and the CRC-32 of a function's name that salts it ---------------------------
inline void philox(uint32_t c[4], uint32_t k0, uint32_t k1) {  // Philox4x32-10
    for (int i = 0; i < 10; i++) {
        const uint64_t p0 = (uint64_t)PF_PHILOX_M0 * c[0], p1 = (uint64_t)PF_PHILOX_M1 * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1,
                       n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += PF_PHILOX_W0;
        k1 += PF_PHILOX_W1;
    }
}
inline void uf_hash32(const uint32_t x[8], uint32_t salt, uint32_t out[8]) {  // out may be x
    uint32_t h[4] = {x[0], x[1], x[2], x[3]};
    philox(h, salt, PF_HASH_K1A);
    uint32_t g[4] = {x[4] ^ h[0], x[5] ^ h[1], x[6] ^ h[2], x[7] ^ h[3]};
    philox(g, salt, PF_HASH_K1B);
    for (int i = 0; i < 4; i++) {
        out[i] = h[i];
        out[4 + i] = g[i];
    }
}
inline U uf_hash(const U& x, uint32_t salt) {
    uint32_t xs[8];
    x.to32(xs);
    uf_hash32(xs, salt, xs);
    return U::from32(xs);
}
inline uint32_t crc32(const std::string& s) {  // zlib.crc32
    uint32_t c = 0xffffffffu;
    for (unsigned char ch : s) {
        c ^= ch;
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return c ^ 0xffffffffu;
}

// ---- the evaluator -------------------------------------------------------------------------
// *out = op(a, b) at width w (1..256), below 2^w; a compare's is 0 or 1.  a and b are below
// 2^w for the binary W ops, NOT, NEG and the compares (whose w is the operands' width); the
// structural ops take operands of their own widths: MOV and EXTRACT any a, CONCAT a of
// w - aux bits over b of aux bits, SEXT a from aux bits.  aux: EXTRACT's low bit, CONCAT's
// and SEXT's low width, HASH's salt.  b is ignored by the unary ops.  False, *out untouched,
// for an opcode that is not a function of two values (leaves, ITE, the bool connectives,
// spills).
inline bool eval_op(uint32_t op, unsigned w, uint32_t aux, const U& a, const U& b, U* out) {
    auto B = [](bool v) { return U::of(v ? 1 : 0); };
    switch (op) {
        case PF_W_ADD: *out = mw(add(a, b), w); return true;
        case PF_W_SUB: *out = mw(sub(a, b), w); return true;
        case PF_W_MUL: *out = mw(mul(a, b), w); return true;
        case PF_W_UDIV:
        case PF_W_UREM: {
            U q = mask(w), r = a;
            if (!b.zero()) divmod(a, b, &q, &r);
            *out = mw(op == PF_W_UDIV ? q : r, w);
            return true;
        }
        case PF_W_SDIV: {
            const bool na = negw(a, w), nb = negw(b, w);
            U q = na ? U::of(1) : mask(w), r;
            if (!b.zero()) {
                divmod(absw(a, w), absw(b, w), &q, &r);
                if (na != nb) q = neg(q);
            }
            *out = mw(q, w);
            return true;
        }
        case PF_W_SREM: {  // sign of the dividend
            U q, r = a;
            if (!b.zero()) {
                divmod(absw(a, w), absw(b, w), &q, &r);
                if (negw(a, w)) r = neg(r);
            }
            *out = mw(r, w);
            return true;
        }
        case PF_W_SMOD: {  // floor mod of the signed values: sign of the divisor
            U q, r = a;
            if (!b.zero()) {
                const bool na = negw(a, w), nb = negw(b, w);
                const U mb = absw(b, w);
                divmod(absw(a, w), mb, &q, &r);
                if (!r.zero() && na != nb) r = sub(mb, r);
                if (nb) r = neg(r);
            }
            *out = mw(r, w);
            return true;
        }
        case PF_W_AND: *out = mw(uand(a, b), w); return true;
        case PF_W_OR: *out = mw(uor(a, b), w); return true;
        case PF_W_XOR: *out = mw(uxor(a, b), w); return true;
        case PF_W_SHL: *out = lt(b, U::of(w)) ? mw(shl(a, (unsigned)b.w[0]), w) : U(); return true;
        case PF_W_LSHR: *out = lt(b, U::of(w)) ? mw(shr(a, (unsigned)b.w[0]), w) : U(); return true;
        case PF_W_ASHR: {
            const bool na = negw(a, w);
            if (!lt(b, U::of(w))) {
                *out = na ? mask(w) : U();
                return true;
            }
            const unsigned s = (unsigned)b.w[0];
            U r = shr(a, s);
            if (na) r = uor(r, uand(mask(w), unot(mask(w - s))));
            *out = mw(r, w);
            return true;
        }
        case PF_W_EXP: *out = powmod(a, b, w); return true;
        case PF_W_NOT: *out = mw(unot(a), w); return true;
        case PF_W_NEG: *out = mw(neg(a), w); return true;
        case PF_W_MOV: *out = mw(a, w); return true;
        case PF_W_EXTRACT: *out = mw(shr(a, aux), w); return true;
        case PF_W_CONCAT: *out = mw(uor(shl(a, aux), b), w); return true;
        case PF_W_SEXT: {
            const U x = mw(a, aux);
            *out = mw(negw(x, aux) ? sub(x, shl(U::of(1), aux)) : x, w);
            return true;
        }
        case PF_W_HASH: *out = mw(uf_hash(a, aux), w); return true;
        case PF_B_EQ: *out = B(a == b); return true;
        case PF_B_ULT: *out = B(lt(a, b)); return true;
        case PF_B_ULE: *out = B(le(a, b)); return true;
        case PF_B_SLT:
        case PF_B_SLE: {  // across the signs the negative one is below; within them, unsigned order
            const bool na = negw(a, w), nb = negw(b, w);
            *out = B(na != nb ? na : op == PF_B_SLT ? lt(a, b) : le(a, b));
            return true;
        }
        case PF_B_UADD_NOOVF: {
            uint64_t c;
            const U s = add(a, b, &c);
            *out = B(!c && le(s, mask(w)));
            return true;
        }
        case PF_B_UMUL_NOOVF: {
            U lo, hi;
            mul_full(a, b, &lo, &hi);
            *out = B(hi.zero() && le(lo, mask(w)));
            return true;
        }
        default: return false;
    }
}

}  // namespace pf_host

#endif /* PF_HOSTINT_H */
