// Stand-alone host build of mythril_amd/csrc/pf_hostint.h: the shared evaluator, op by op
// (tests/test_host_ops.py compiles it with the address and undefined-behaviour sanitizers).
// stdin, one request per line, every number in hex:
//   <op> <w> <aux> <a> <b>   -> eval_op's result, or "?" for an opcode it does not know
//   crc <name>               -> the CRC-32 of the name
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../mythril_amd/csrc/pf_hostint.h"

using pf_host::U;

static U parse(const char* s) {  // hex, at most 64 digits
    uint32_t l[8] = {0};
    const size_t n = strlen(s);
    for (size_t i = 0; i < n && i < 64; i++) {
        const char c = s[n - 1 - i];
        const uint32_t d = c >= 'a' ? (uint32_t)(c - 'a' + 10) : c >= 'A' ? (uint32_t)(c - 'A' + 10) : (uint32_t)(c - '0');
        l[i / 8] |= d << (4 * (i % 8));
    }
    return U::from32(l);
}

int main() {
    char op[16], ws[16], aux[16], as[80], bs[80];
    while (scanf("%15s", op) == 1) {
        if (strcmp(op, "crc") == 0) {
            if (scanf("%79s", as) != 1) return 2;
            printf("%" PRIx32 "\n", pf_host::crc32(as));
            continue;
        }
        if (scanf("%15s %15s %79s %79s", ws, aux, as, bs) != 4) return 2;
        U r;
        if (!pf_host::eval_op((uint32_t)strtoul(op, nullptr, 16), (unsigned)strtoul(ws, nullptr, 16),
                              (uint32_t)strtoul(aux, nullptr, 16), parse(as), parse(bs), &r)) {
            printf("?\n");
            continue;
        }
        uint32_t l[8];
        r.to32(l);
        for (int i = 7; i >= 0; i--) printf("%08" PRIx32, l[i]);
        printf("\n");
    }
    return 0;
}
