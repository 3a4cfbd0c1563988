// Optimizer step of the training path (gfx950): Adam + the EMA shadow weights in ONE pass over flat fp32 buffers.
//
// Reference: `Diffusion.configure_optimizers` = torch.optim.Adam(lr=1e-4) (diffusion.py:210-211) wrapped by
// `EMAOptimizer` (ema.py:200-325), whose `update()` runs `ema_update` (ema.py:187-194: ema = ema * decay +
// (1 - decay) * param) after every optimizer step — three full passes over the parameters and their three state
// tensors per step there (Adam's foreach kernels, the parameter copy, mul_ + add_).  Here every element is read and
// written once: p, g, m, v, ema in; p, m, v, ema out = 36 B per parameter, HBM-bound (13.5 M parameters = 485 MB:
// ~80 us at 6 TB/s against ~0.5 ms for the unfused sequence).
//
// Arithmetic follows torch.optim.Adam's single-tensor path op for op, in fp32:
//   g' = g * grad_scale (+ weight_decay * p)          (grad_scale: 1 / world size when the all-reduce summed)
//   m  = m + (1 - beta1) * (g' - m)                   (exp_avg.lerp_)
//   v  = beta2 * v + (1 - beta2) * g' * g'            (mul_ + addcmul_)
//   p  = p - (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
//   ema = ema * decay + (1 - decay) * p               (when do_ema)
// The flat buffers are 16-byte aligned and the element count is padded to a multiple of 4 by the host side.
//
// Gradient clipping (both shipped trainer settings clip: example_configs/shapenet_airplane_unconditional.py:74-76
// gradient_clip_algorithm="value", taskonomy_conditional.py:102-104 "norm", gradient_clip_val=1.0) is part of the same read of g:
//   norm  (torch.nn.utils.clip_grad_norm_):   g' = (g * grad_scale) * coef, coef = min(1, max_norm / (total_norm + 1e-6))
//   value (torch.nn.utils.clip_grad_value_):  g' = clamp(g * grad_scale, -clip, +clip)       (a NaN stays a NaN, like torch.clamp)
// both BEFORE weight_decay * p is added (torch clips p.grad; Adam adds the decay afterwards).  total_norm comes from
// `grad_sumsq_kernel` + `grad_norm_finish_kernel`: one extra 4-byte-per-parameter read of g, squares accumulated in DOUBLE (the
// square of an fp32 value cannot overflow a double, so the sum is non-finite if and only if a gradient is, and its rounding is far
// below one fp32 ulp of the norm), one double partial per block, the partials added in a fixed order by one block: no
// floating-point atomics, the same bits on every run.  The alignment pads between the parameters in the flat buffer are zero and
// stay zero (zero_grad, gather_grads), and a frozen parameter's gradient is zero: neither changes the norm.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)   // keep torch's op order: no fma contraction across its separate kernels

namespace {

// CLIP: 0 none (today's step: `stats` / `clip_val` are not read), 1 norm (stats[1] = the coefficient), 2 value (clip_val)
template <int CLIP>
__global__ __launch_bounds__(256) void adam_ema_kernel(AdamEmaArgs a, const float* __restrict__ stats, float clip_val) {
    const size_t n4 = a.n / 4;
    f32x4* __restrict__ p4 = reinterpret_cast<f32x4*>(a.p);
    const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(a.g);
    f32x4* __restrict__ m4 = reinterpret_cast<f32x4*>(a.m);
    f32x4* __restrict__ v4 = reinterpret_cast<f32x4*>(a.v);
    f32x4* __restrict__ e4 = reinterpret_cast<f32x4*>(a.ema);
    const float w1 = a.w1, w2 = a.w2, we = a.ema_w;
    float gscale = a.grad_scale, step_size = a.step_size, bc2_sqrt = a.bc2_sqrt;
    if (a.found_inf) {   // (launch-uniform) GradScaler protocol: decided on the device, the host never waits for the gradients
        if (*a.found_inf != 0.f) {   // inf / nan in the gradients: torch skips optimizer.step() (and with it the EMA update)
            if (a.skipped && blockIdx.x == 0 && threadIdx.x == 0) *a.skipped += 1;
            return;
        }
        if (a.amp_scale) gscale = gscale / *a.amp_scale;   // scales are powers of two: exact
        const int sk = a.skipped ? *a.skipped : 0;
        if (sk > 0) {   // Adam's step count did not advance on the skipped steps: bias corrections of the steps actually taken
            const double st = (double)(a.step - sk);
            step_size = (float)(a.lr / (1.0 - pow(a.beta1, st)));
            bc2_sqrt = (float)sqrt(1.0 - pow(a.beta2d, st));
        }
    }
    float coef = 1.f;
    if constexpr (CLIP == GECCO_CLIP_NORM) coef = stats[1];   // (launch-uniform) written by grad_norm_finish_kernel ahead of this launch
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        f32x4 p = p4[i], g = GECCO_NT_LOAD(g4 + i), m = m4[i], v = v4[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float ge = g[e] * gscale;
            if constexpr (CLIP == GECCO_CLIP_NORM) ge = ge * coef;   // a rounding of its own, like g.mul_(coef) after unscale_ / the mean
            if constexpr (CLIP == GECCO_CLIP_VALUE) ge = ge < -clip_val ? -clip_val : (ge > clip_val ? clip_val : ge);   // NaN passes
            if (a.weight_decay != 0.f) ge = ge + a.weight_decay * p[e];
            m[e] = __builtin_fmaf(w1, ge - m[e], m[e]);   // lerp_ (ATen: fma(weight, end - start, start))
            v[e] = v[e] * a.beta2 + w2 * (ge * ge);
            const float denom = sqrtf(v[e]) / bc2_sqrt + a.eps;
            p[e] = p[e] - step_size * (m[e] / denom);
        }
        p4[i] = p;
        m4[i] = m;
        v4[i] = v;
        if (a.do_ema) {
            f32x4 s = e4[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] = s[e] * a.ema_decay + we * p[e];
            e4[i] = s;
        }
    }
}

__global__ __launch_bounds__(256) void ema_only_kernel(const float* __restrict__ p, float* __restrict__ ema, size_t n,
                                                       float decay, float we) {
    const size_t n4 = n / 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const f32x4 x = reinterpret_cast<const f32x4*>(p)[i];
        f32x4 s = reinterpret_cast<f32x4*>(ema)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = s[e] * decay + we * x[e];
        reinterpret_cast<f32x4*>(ema)[i] = s;
    }
}

unsigned grid_for4(size_t n) {
    const size_t blocks = (n / 4 + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : (blocks > 256 * 16 ? 256 * 16 : blocks));
}

// sum over the block of one double per thread, in a fixed order: xor butterfly inside each wave64, then the 4 waves through LDS
// (waves 0, 1, 2, 3 added in that order by thread 0).  Returns the sum in thread 0 only.
__device__ __forceinline__ double block_sum_f64(double x, double* lds4) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds4[wave] = x;
    __syncthreads();
    return threadIdx.x == 0 ? ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3] : 0.0;
}

// partial[blockIdx.x] = sum of (double)g * (double)g over the block's grid-stride share of g.  Plain loads (not GECCO_NT_LOAD): the step
// reads the same buffer right afterwards.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, size_t n, double* __restrict__ partial) {
    __shared__ double lds4[4];
    const size_t n4 = n / 4, stride = (size_t)gridDim.x * blockDim.x;
    const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g);
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // independent chains: two vectors in flight, one per component
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + stride < n4; i += 2 * stride) {
        const f32x4 x = g4[i], y = g4[i + stride];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[e] += (double)x[e] * (double)x[e];
            acc[4 + e] += (double)y[e] * (double)y[e];
        }
    }
    if (i < n4) {
        const f32x4 x = g4[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += (double)x[e] * (double)x[e];
    }
    const double t = ((acc[0] + acc[4]) + (acc[1] + acc[5])) + ((acc[2] + acc[6]) + (acc[3] + acc[7]));
    const double s = block_sum_f64(t, lds4);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// ONE block: the partials in a fixed order (thread t takes t, t + 256, ...), then
//   stats[0] = total_norm = (float)(sqrt(sum) * |grad_scale| / *amp_scale)   the 2-norm of the TRUE gradients, rounded to fp32 once
//   stats[1] = clip_coef  = min(1, (1 / (total_norm + 1e-6f)) * max_norm)     fp32, op for op torch's `max_norm / (total_norm + 1e-6)`
//                                                                            (Tensor.__rtruediv__ = reciprocal() * scalar), clamp(max=1)
// max_norm <= 0: no clipping asked for, coef = 1.  A non-finite gradient gives inf / nan in both (torch.clamp keeps a NaN too).
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ partial, unsigned nparts, float grad_scale,
                                                               const float* __restrict__ amp_scale, float max_norm,
                                                               float* __restrict__ stats) {
    __shared__ double lds4[4];
    double x = 0.0;
    for (unsigned i = threadIdx.x; i < nparts; i += 256) x += partial[i];
    const double s = block_sum_f64(x, lds4);
    if (threadIdx.x == 0) {
        double norm = sqrt(s) * fabs((double)grad_scale);
        if (amp_scale) norm = norm / (double)*amp_scale;
        const float total = (float)norm;
        float coef = 1.f;
        if (max_norm > 0.f) {
            coef = (1.f / (total + 1e-6f)) * max_norm;
            coef = coef > 1.f ? 1.f : coef;   // NaN stays NaN
        }
        stats[0] = total;
        stats[1] = coef;
    }
}

}  // namespace

int adam_ema_launch(const AdamEmaArgs& a, hipStream_t st) {
    if (a.n % 4) return -2;
    if (a.n == 0) return 0;
    hipLaunchKernelGGL(adam_ema_kernel<GECCO_CLIP_NONE>, dim3(grid_for4(a.n)), dim3(256), 0, st, a, nullptr, 0.f);
    return (int)hipGetLastError();
}

int adam_ema_clip_launch(const AdamEmaArgs& a, int algorithm, const float* stats, float clip_val, hipStream_t st) {
    if (a.n % 4) return -2;
    if (algorithm == GECCO_CLIP_NORM ? !stats : algorithm != GECCO_CLIP_VALUE) return -2;
    if (a.n == 0) return 0;
    if (algorithm == GECCO_CLIP_NORM)
        hipLaunchKernelGGL(adam_ema_kernel<GECCO_CLIP_NORM>, dim3(grid_for4(a.n)), dim3(256), 0, st, a, stats, 0.f);
    else
        hipLaunchKernelGGL(adam_ema_kernel<GECCO_CLIP_VALUE>, dim3(grid_for4(a.n)), dim3(256), 0, st, a, nullptr, clip_val);
    return (int)hipGetLastError();
}

unsigned grad_norm_blocks(size_t n) { return grid_for4(n); }

int grad_norm_launch(const float* g, size_t n, float grad_scale, const float* amp_scale, float max_norm, double* partial, float* stats,
                     hipStream_t st) {
    if (n % 4) return -2;
    const unsigned blocks = n ? grid_for4(n) : 0;   // n == 0: the norm of nothing is 0
    if (blocks) {
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(256), 0, st, g, n, partial);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, st, partial, blocks, grad_scale, amp_scale, max_norm, stats);
    return (int)hipGetLastError();
}

int ema_update_launch(const float* p, float* ema, size_t n, double decay, hipStream_t st) {
    if (n % 4) return -2;
    if (n == 0) return 0;
    hipLaunchKernelGGL(ema_only_kernel, dim3(grid_for4(n)), dim3(256), 0, st, p, ema, n, (float)decay, (float)(1.0 - decay));
    return (int)hipGetLastError();
}
