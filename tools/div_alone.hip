#include <hip/hip_runtime.h>
#include "u256.h"
extern "C" __global__ void div_alone(const uint32_t* a, const uint32_t* b, uint32_t* q, uint32_t* r) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    pf::u256 ua, ub, uq, ur;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        ua.l[i] = a[t * 8u + i];
        ub.l[i] = b[t * 8u + i];
    }
    pf::udivrem256(ua, ub, &uq, &ur);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        q[t * 8u + i] = uq.l[i];
        r[t * 8u + i] = ur.l[i];
    }
}
