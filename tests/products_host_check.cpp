// Host build of the product routines of mythril_amd/csrc/u256.h (portable columns under
// PF_HOST_MAC, the mirrors that tools/gen_u256_cols.py writes beside the inline-asm ones).
// Reads lines "<op> <a: 64 hex> <b: 64 hex>" and prints one 64-hex result per line:
//   mul   mul256(a, b)
//   sqr   sqr256(a)
//   exp   exp256_split(a, b), one lane per "wave"
//   t<I>  level I of the series' Horner chain as horner<> instantiates it:
//         tmul_add<L, LY, K...>(a, b, K), a on L limbs and b on LY
// and first, one line "level I L LY K" per level of the configured split.
// tests/test_products_host.py builds it with the address and undefined-behaviour sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#define __device__
#define __forceinline__ inline
static inline unsigned long long __ballot(int p) { return p ? 1ull : 0ull; }
struct uint2 { uint32_t x, y; };
static inline uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{x, y}; }
#define PF_HOST_MAC
#include "../mythril_amd/csrc/u256.h"
using pf::u256;

constexpr int M = PF_EXP_SPLIT;
constexpr int J = pf::exp_terms(M);

// the shape and constant of level I, as in pf::horner
template <int I>
struct Level {
    static constexpr int S = M + 2 - pf::v2c(I);
    static constexpr int P = 256 - pf::prefix_val(M, I);
    static constexpr int L = (P + 31) / 32;
    static constexpr pf::k256 K = pf::exp_addend(I, J, L);
    static constexpr int LY = (I == J || (P - S + 31) / 32 >= L || L == 1) ? L : L - 1;
};

static void print(const u256& r) {
    for (int i = 7; i >= 0; i--) printf("%08x", r.l[i]);
    printf("\n");
}

template <int I>
static void list_levels() {
    using V = Level<I>;
    printf("level %d %d %d ", I, V::L, V::LY);
    u256 k;
    for (int i = 0; i < 8; i++) k.l[i] = V::K.l[i];
    print(k);
    if constexpr (I < J) list_levels<I + 1>();
}

template <int I>
static bool level(int want, const u256& a, const u256& b, u256* r) {
    using V = Level<I>;
    if (want == I) {
        *r = pf::tmul_add<V::L, V::LY, V::K.l[0], V::K.l[1], V::K.l[2], V::K.l[3], V::K.l[4], V::K.l[5],
                          V::K.l[6]>(a, b, V::K);
        return true;
    }
    if constexpr (I < J) return level<I + 1>(want, a, b, r);
    return false;
}

static bool parse(const char* s, u256* v) {
    if (strlen(s) != 64) return false;
    for (int i = 0; i < 8; i++) {
        char t[9];
        memcpy(t, s + 56 - 8 * i, 8);
        t[8] = 0;
        v->l[i] = (uint32_t)strtoul(t, 0, 16);
    }
    return true;
}

int main() {
    list_levels<1>();
    char op[16], as[80], bs[80];
    while (scanf("%15s %79s %79s", op, as, bs) == 3) {
        u256 a, b, r;
        if (!parse(as, &a) || !parse(bs, &b)) {
            fprintf(stderr, "bad line: %s %s %s\n", op, as, bs);
            return 2;
        }
        if (!strcmp(op, "mul")) {
            r = pf::mul256(a, b);
        } else if (!strcmp(op, "sqr")) {
            r = pf::sqr256(a);
        } else if (!strcmp(op, "exp")) {
            uint2 tbl[4 * PF_EXP_TBL_ENTRIES];
            r = pf::exp256_split(a, b, tbl, 1u);
        } else if (op[0] != 't' || !level<1>(atoi(op + 1), a, b, &r)) {
            fprintf(stderr, "bad op: %s\n", op);
            return 2;
        }
        print(r);
    }
    return 0;
}
