// The activation and the window scan shared by the kernels of tpspp_bn_pool_train.hip: the forward and both backward
// passes recompute them from z, so they stand here once and every kernel forms the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace tpspp_bn_pool {

// per-channel constants of a(v) = relu((v - mean) * (gamma * rstd) + beta): bn_apply_kernel's expression, a subtraction, a
// product and a sum, each rounded on its own (the library is built with -ffp-contract=off, so nothing is fused here)
struct Act {
    float mean, scale, beta;
};

__device__ __forceinline__ Act load_act(const float* __restrict__ mean, const float* __restrict__ rstd,
                                        const float* __restrict__ gamma, const float* __restrict__ beta, unsigned c)
{
    return Act{mean[c], gamma[c] * rstd[c], beta[c]};
}

__device__ __forceinline__ float bn_relu(float v, const Act& k)
{
    const float t = (v - k.mean) * k.scale + k.beta;
    return t > 0.0f ? t : 0.0f;
}

// ATen's scan of a 2x2 window, row by row from its first element: v replaces m if v > m or v is a NaN, and the selected
// element is the last one that did (the first of equal maxima wins, a NaN wins).  Returns the selected index 0..3.
__device__ __forceinline__ int scan2x2(float a00, float a01, float a10, float a11, float& m)
{
    int k = 0;
    m = a00;
    if (a01 > m || a01 != a01) { m = a01; k = 1; }
    if (a10 > m || a10 != a10) { m = a10; k = 2; }
    if (a11 > m || a11 != a11) { m = a11; k = 3; }
    return k;
}

}  // namespace tpspp_bn_pool
