// The point-pair distance of gecco-jax/src/gecco_jax/geometry.py:8-24, shared by every metric kernel that forms it
// (metrics.hip: the distance matrix; emd.hip: the auction's costs), so that all of them compute the same bits.
//
// The roundings are spelled out (contraction off, explicit FMAs): left to the compiler, the fusion of these sums into FMAs
// depends on how each kernel's loop is vectorised, and two kernels would then disagree in the last bits of a cost.  The
// form is the one the distance-matrix kernel has always been compiled to.
#pragma once
#include <hip/hip_runtime.h>

// |p|^2 = fma(z, z, x x + y y)
static __device__ __forceinline__ float sq_norm(float x, float y, float z) {
#pragma clang fp contract(off)
    return __builtin_fmaf(z, z, x * x + y * y);
}

// d(a, b) exactly as the reference forms it: aa + bb - 2 ab, clamped at 0 (the clamp hides the cancellation noise of
// that form for near-identical points), sqrt unless `squared`; aa, bb from sq_norm
static __device__ __forceinline__ float pair_dist(float ax, float ay, float az, float aa, float bx, float by, float bz, float bb,
                                                  bool squared) {
#pragma clang fp contract(off)
    const float ab = __builtin_fmaf(az, bz, __builtin_fmaf(ax, bx, ay * by));
    const float d2 = fmaxf(__builtin_fmaf(-2.f, ab, aa + bb), 0.f);
    return squared ? d2 : sqrtf(d2);
}
