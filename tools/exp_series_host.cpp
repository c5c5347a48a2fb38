// Host build of pf::exp256_split alone (mythril_amd/csrc/u256.h, portable columns under
// PF_HOST_MAC): reads lines "base(64 hex) exponent(64 hex)" and prints base^exponent mod 2^256,
// one lane per "wave" as in tools/u256_host_check.cpp.  tests/test_exp_series_host.py feeds it
// the shapes at which the series' levels and constants can go wrong.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#define __device__
#define __forceinline__ inline
static inline unsigned long long __ballot(int p) { return p ? 1ull : 0ull; }
struct uint2 { uint32_t x, y; };
static inline uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{x, y}; }
#define PF_HOST_MAC
#include "../mythril_amd/csrc/u256.h"
using pf::u256;

static bool parse(const char* s, u256* v) {
    for (int k = 0; k < 64; k++)
        if (!s[k]) return false;
    if (s[64]) return false;
    for (int i = 0; i < 8; i++) {
        char t[9];
        for (int k = 0; k < 8; k++) t[k] = s[56 - 8 * i + k];
        t[8] = 0;
        v->l[i] = (uint32_t)strtoul(t, 0, 16);
    }
    return true;
}

int main() {
    char bs[80], es[80];
    while (scanf("%79s %79s", bs, es) == 2) {
        u256 b, e;
        if (!parse(bs, &b) || !parse(es, &e)) {
            fprintf(stderr, "bad line: %s %s\n", bs, es);
            return 2;
        }
        uint2 tbl[4 * PF_EXP_TBL_ENTRIES];
        const u256 r = pf::exp256_split(b, e, tbl, 1u);
        for (int i = 7; i >= 0; i--) printf("%08x", r.l[i]);
        printf("\n");
    }
    return 0;
}
