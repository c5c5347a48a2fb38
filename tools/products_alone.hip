// The product routines alone, for static instruction counts (compile with the flags of
// mythril_amd/build.py plus `--cuda-device-only -S -I mythril_amd/csrc`): each kernel loads its
// operands, runs one routine and stores the result.  tmulk_alone is the 5-limb multiply-add of
// the series' level 13 at PF_EXP_SPLIT = 8 (three columns with a literal addend limb).
#include <hip/hip_runtime.h>
#include "u256.h"
#define PF_LOAD2                                     \
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; \
    pf::u256 ua, ub, ur;                             \
    _Pragma("unroll") for (int i = 0; i < 8; i++) {  \
        ua.l[i] = a[t * 8u + i];                     \
        ub.l[i] = b[t * 8u + i];                     \
    }
#define PF_STORE \
    _Pragma("unroll") for (int i = 0; i < 8; i++) r[t * 8u + i] = ur.l[i];

extern "C" __global__ void mul_alone(const uint32_t* a, const uint32_t* b, uint32_t* r) {
    PF_LOAD2
    ur = pf::mul256(ua, ub);
    PF_STORE
}
extern "C" __global__ void sqr_alone(const uint32_t* a, const uint32_t* b, uint32_t* r) {
    PF_LOAD2
    ur = pf::sqr256(ua);
    PF_STORE
}
extern "C" __global__ void tmulk_alone(const uint32_t* a, const uint32_t* b, uint32_t* r) {
    PF_LOAD2
    constexpr pf::k256 K = pf::exp_addend(13, 28, 5);
    ur = pf::tmul_add<5, 5, K.l[0], K.l[1], K.l[2], K.l[3], K.l[4], K.l[5], K.l[6]>(ua, ub, K);
    PF_STORE
}
