// Matrix-free entropic optimal transport between two clouds, on the device (gfx950): log-domain Sinkhorn sweeps whose costs are
// recomputed from the coordinates, never stored, and the gradient of the resulting cost along the fixed plan.
//
// Reference: gecco-jax/src/gecco_jax/metrics.py:144-156 (`sinkhorn_emd`: ott's Sinkhorn on a PointCloud geometry, squared-Euclidean
// cost, uniform weights) and benchmark.py:21-39 / :73-77 (every pair of two sets, epsilon = 0.1).
//
// Definition (the iteration of gecco_sinkhorn_f32 and oracle/cpu_ref.py::sinkhorn_cost).  Clouds x (N, 3), y (M, 3), marginals 1/N, 1/M,
//     C_ij = pair_dist(x_i, y_j, squared)                  (pair_dist.h: max(|x|^2 + |y|^2 - 2 x.y, 0), the distance-matrix bits)
//     g = 0;  `iterations` times:  f_i = -eps LSE_j((g_j - C_ij) / eps - log M),   g_j = -eps LSE_i((f_i - C_ij) / eps - log N)
//     P_ij = exp((f_i + g_j - C_ij) / eps) / (N M),        value = sum_ij P_ij C_ij
// The sweep count is fixed: nothing is read back, every loop is bounded by `iterations`, no workgroup waits on another.
//
// Arithmetic (both kernel forms).  With k = log2(e) / eps the potentials are carried as k f, k g, so an entry is
//     v_ij = fma(-C_ij, k, k g_j),   one v_exp_f32 (exp2) per entry,
// and the log-sum-exp is online over chunks of SK_CHUNK columns: the running maximum moves once per chunk (one more exp2 to rescale
// the sum), not per entry.  A thread owns rows and reads a column (x, y, z, |p|^2 as one 16-byte LDS word, and its potential) at an
// address that is the same in every lane: a broadcast read, no bank conflicts.  The g half-sweep is the f half-sweep with the clouds
// and the potentials swapped: one body (`sk_walk`) serves both, the cost pass and the gradient pass.
//
// Resident form.  One workgroup of 1024 threads per pair and ONE launch per solve: both clouds and both potentials stay in LDS (20
// bytes per point), only the clouds are read from HBM and only the value (and f, g when asked for) is written.  Rows are taken 1024
// at a time; when fewer than 1024 rows are left the idle waves split the columns instead (CS column slices per row, merged in slice
// order through 8 KiB of LDS), so small clouds still use the whole workgroup.
//
// Streaming form.  Any N, M.  One row-pass kernel (`sk_stream_kernel<MODE>`): a block of 4 waves owns 128 rows in registers (2 per
// lane) and walks the other cloud and its potential through LDS in tiles of 1024 columns, each wave a quarter of every tile; the four
// partial results per row are merged in wave order.  MODE 0 writes the row potential, MODE 1 the row cost sum_j P_ij C_ij, MODE 2 the
// gradient row sum_j P_ij 2 (x_i - y_j).  A solve is 2 * iterations launches, the cost pass and a fixed-order fp64 sum.
//
// Gradient.  The plan is a constant of the gradient: d value / d x_i = sum_j P_ij 2 (x_i - y_j) on the saved f, g (also the envelope
// gradient of the entropic cost once the sweeps have converged).  MODE 2 over the rows of x gives dx, over the rows of the swapped
// problem dy.  No float atomics: every sum has a fixed order, so values and gradients are the same bits run to run and in any batch
// position.
//
// Non-finite coordinates.  A point whose coordinates (or |p|^2) are not finite gets a NaN potential; it reaches every potential of the
// pair within a sweep and the value is NaN.  Pairs share nothing, so no other pair is touched.
#include "../../include/gecco_hip.h"
#include "common.h"
#include "kernels.h"
#include "launch_state.h"
#include "pair_dist.h"

namespace {

constexpr int SK_CHUNK = 8;                          // columns per move of the running maximum
constexpr int SK_LDS_BYTES = 160 * 1024;             // per CU, all of it available to one workgroup
constexpr int SK_RES_THREADS = 1024;
constexpr int SK_RES_WAVES = SK_RES_THREADS / 64;
constexpr int SK_RES_SCRATCH = SK_RES_THREADS * 2 * 4;   // (max, sum) of every (row, column slice): rows * CS <= 1024
constexpr int SK_RES_STATIC = 256;                   // the fp64 wave sums of the value, and slack for alignment
constexpr int SK_PER_POINT = 16 + 4;                 // (x, y, z, |p|^2) and the potential
static_assert(GECCO_SINKHORN_RESIDENT_MAX_POINTS == (SK_LDS_BYTES - SK_RES_SCRATCH - SK_RES_STATIC) / SK_PER_POINT / 8 * 8,
              "the resident limit is what one CU's LDS holds, rounded down to a multiple of 8");
constexpr int SK_ROWS = 2;                           // streaming: rows per lane
constexpr int SK_BLOCK_ROWS = 64 * SK_ROWS;
constexpr int SK_TILE = 1024;                        // streaming: columns per LDS tile
constexpr int SK_WAVE_COLS = SK_TILE / 4;
constexpr float SK_NEG = -3.0e38f;

static __device__ __forceinline__ float ex2(float v) { return __builtin_amdgcn_exp2f(v); }
static __device__ __forceinline__ bool sk_finite(const f32x4 p) { return __builtin_isfinite(p[3]) && __builtin_isfinite(p[0] + p[1] + p[2]); }
static __device__ __forceinline__ f32x4 sk_point(const float* __restrict__ p, int i) {
    const float x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
    return f32x4{x, y, z, sq_norm(x, y, z)};
}

// One entry of a row: MODE 1 adds P C, MODE 2 adds P (x - y); t = k f_i - log2(N M), so P = exp2(v + t).
template <int MODE>
static __device__ __forceinline__ void sk_entry(const f32x4 x, float t, const f32x4 y, float gy, float k, float (&acc)[3]) {
    const float c = pair_dist(x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3], true);
    const float p = ex2(__builtin_fmaf(-c, k, gy) + t);
    if (MODE == 1) {
        acc[0] = __builtin_fmaf(p, c, acc[0]);
    } else {
        acc[0] = __builtin_fmaf(p, x[0] - y[0], acc[0]);
        acc[1] = __builtin_fmaf(p, x[1] - y[1], acc[1]);
        acc[2] = __builtin_fmaf(p, x[2] - y[2], acc[2]);
    }
}

// R rows against the columns [c0, c1) of a cloud in LDS (Y: points, gk: k * potential).  MODE 0: acc = (running max, sum of
// exp2(v - max)) of v_j = k (g_j - C_ij); MODE 1 / 2: see sk_entry.  The order over j is fixed.
template <int MODE, int R>
static __device__ __forceinline__ void sk_walk(const f32x4 (&x)[R], const float (&t)[R], const f32x4* __restrict__ Y,
                                               const float* __restrict__ gk, int c0, int c1, float k, float (&acc)[R][3]) {
    int j = c0;
    for (; j + SK_CHUNK <= c1; j += SK_CHUNK) {
        if (MODE == 0) {
            float v[R][SK_CHUNK];
#pragma unroll
            for (int u = 0; u < SK_CHUNK; ++u) {
                const f32x4 y = Y[j + u];
                const float gy = gk[j + u];
#pragma unroll
                for (int r = 0; r < R; ++r)
                    v[r][u] = __builtin_fmaf(-pair_dist(x[r][0], x[r][1], x[r][2], x[r][3], y[0], y[1], y[2], y[3], true), k, gy);
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float mn = acc[r][0];
#pragma unroll
                for (int u = 0; u < SK_CHUNK; ++u) mn = fmaxf(mn, v[r][u]);      // (a NaN entry is skipped here and lands in the sum)
                float s = acc[r][1] * ex2(acc[r][0] - mn);
#pragma unroll
                for (int u = 0; u < SK_CHUNK; ++u) s += ex2(v[r][u] - mn);
                acc[r][0] = mn;
                acc[r][1] = s;
            }
        } else {
#pragma unroll
            for (int u = 0; u < SK_CHUNK; ++u) {
                const f32x4 y = Y[j + u];
                const float gy = gk[j + u];
#pragma unroll
                for (int r = 0; r < R; ++r) sk_entry<MODE>(x[r], t[r], y, gy, k, acc[r]);
            }
        }
    }
    for (; j < c1; ++j) {
        const f32x4 y = Y[j];
        const float gy = gk[j];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (MODE == 0) {
                const float v = __builtin_fmaf(-pair_dist(x[r][0], x[r][1], x[r][2], x[r][3], y[0], y[1], y[2], y[3], true), k, gy);
                const float mn = fmaxf(acc[r][0], v);
                acc[r][1] = acc[r][1] * ex2(acc[r][0] - mn) + ex2(v - mn);
                acc[r][0] = mn;
            } else {
                sk_entry<MODE>(x[r], t[r], y, gy, k, acc[r]);
            }
        }
    }
}

template <int MODE>
static __device__ __forceinline__ void sk_init(float (&a)[3]) {
    a[0] = MODE == 0 ? SK_NEG : 0.f;
    a[1] = 0.f;
    a[2] = 0.f;
}
// merge the partial result b of a later column slice into a
template <int MODE>
static __device__ __forceinline__ void sk_merge(float (&a)[3], const float (&b)[3]) {
    if (MODE == 0) {
        const float mn = fmaxf(a[0], b[0]);
        a[1] = a[1] * ex2(a[0] - mn) + b[1] * ex2(b[0] - mn);
        a[0] = mn;
    } else {
        a[0] += b[0];
        a[1] += b[1];
        a[2] += b[2];
    }
}
// k * potential of a row from its (max, sum): -(log2 sum_j 2^(v_j) - log2 W), W the number of columns
static __device__ __forceinline__ float sk_potential(const float (&a)[3], float log2w) { return log2w - (a[0] + __log2f(a[1])); }

// ------------------------------------------------------------------------------------------------------------- resident form
// One half-sweep (MODE 0: pr[i] = k * potential of row i) or the cost pass (MODE 1: returns this thread's share of sum_i rowcost_i) of
// the rows R (n points, potentials pr) against the columns Cc (m points, potentials pc), all in LDS.
template <int MODE>
static __device__ __forceinline__ double sk_res_pass(const f32x4* __restrict__ R, float* __restrict__ pr, int n, const f32x4* __restrict__ Cc,
                                                     const float* __restrict__ pc, int m, float* __restrict__ scratch, float k, float logw) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double share = 0.0;
    for (int p0 = 0; p0 < n; p0 += SK_RES_THREADS) {
        const int rows = min(SK_RES_THREADS, n - p0), nw = (rows + 63) >> 6, CS = SK_RES_WAVES / nw;   // CS >= 1 column slices
        const int rw = wave / CS, cs = wave - rw * CS, li = rw * 64 + lane;
        const bool valid = rw < nw && li < rows;
        const int i = p0 + (valid ? li : 0);
        f32x4 x[1] = {R[i]};
        float t[1] = {MODE == 0 ? 0.f : pr[i] - logw};
        float acc[1][3];
        sk_init<MODE>(acc[0]);
        if (rw < nw) sk_walk<MODE, 1>(x, t, Cc, pc, (int)((long long)cs * m / CS), (int)((long long)(cs + 1) * m / CS), k, acc);
        if (CS > 1) {                                    // (uniform in the workgroup)
            if (valid) {
                scratch[2 * (cs * nw * 64 + li)] = acc[0][0];
                scratch[2 * (cs * nw * 64 + li) + 1] = acc[0][1];
            }
            __syncthreads();
            if (valid && cs == 0)
                for (int c = 1; c < CS; ++c) {
                    const float o[3] = {scratch[2 * (c * nw * 64 + li)], scratch[2 * (c * nw * 64 + li) + 1], 0.f};
                    sk_merge<MODE>(acc[0], o);
                }
        }
        if (valid && cs == 0) {
            if (MODE == 0) pr[i] = sk_finite(x[0]) ? sk_potential(acc[0], logw) : __builtin_nanf("");
            else share += (double)acc[0][0];
        }
    }
    __syncthreads();
    return share;
}

__global__ __launch_bounds__(SK_RES_THREADS) void sk_resident_kernel(const float* __restrict__ A, const float* __restrict__ Bc, float* __restrict__ f,
                                                                     float* __restrict__ g, float* __restrict__ out, int N, int M, int T,
                                                                     int set_mode, float k, float inv_k, int iterations) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sk_lds[];
    f32x4* lx = reinterpret_cast<f32x4*>(sk_lds);
    f32x4* ly = lx + N;
    float* px = reinterpret_cast<float*>(ly + M);
    float* py = px + N;
    float* scratch = py + M;
    __shared__ double s_red[SK_RES_WAVES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pair = blockIdx.x;                       // = s * T + t in set mode
    const int sa = set_mode ? pair / T : pair, sb = set_mode ? pair % T : pair;
    const float* a = A + (size_t)sa * N * 3;
    const float* b = Bc + (size_t)sb * M * 3;
    for (int i = tid; i < N; i += SK_RES_THREADS) { lx[i] = sk_point(a, i); px[i] = 0.f; }
    for (int j = tid; j < M; j += SK_RES_THREADS) { ly[j] = sk_point(b, j); py[j] = 0.f; }
    __syncthreads();
    const float l2n = __log2f((float)N), l2m = __log2f((float)M);
    for (int it = 0; it < iterations; ++it) {
        sk_res_pass<0>(lx, px, N, ly, py, M, scratch, k, l2m);
        sk_res_pass<0>(ly, py, M, lx, px, N, scratch, k, l2n);
    }
    double acc = sk_res_pass<1>(lx, px, N, ly, py, M, scratch, k, l2n + l2m);
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) s_red[wave] = acc;
    if (f)
        for (int i = tid; i < N; i += SK_RES_THREADS) f[(size_t)pair * N + i] = px[i] * inv_k;
    if (g)
        for (int j = tid; j < M; j += SK_RES_THREADS) g[(size_t)pair * M + j] = py[j] * inv_k;
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int w = 0; w < SK_RES_WAVES; ++w) total += s_red[w];
        out[pair] = (float)total;
    }
}

// ------------------------------------------------------------------------------------------------------------ streaming form
// Rows: cloud X (B, n, 3); columns: cloud Y (B, m, 3) with potential potY (B, m).  MODE 0: outp (B, n) = the potential of X's rows;
// MODE 1: outp (B, n) = sum_j P_ij C_ij; MODE 2: outp (B, n, 3) = gout[b] * sum_j P_ij 2 (x_i - y_j); potX (B, n) is read in MODE 1 / 2.
template <int MODE>
__global__ __launch_bounds__(256) void sk_stream_kernel(const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ potX,
                                                        const float* __restrict__ potY, float* __restrict__ outp, const float* __restrict__ gout,
                                                        int n, int m, float k, float inv_k, float logw) {
    __shared__ f32x4 sy[SK_TILE];
    __shared__ float sg[SK_TILE];
    constexpr int NP = MODE == 0 ? 2 : (MODE == 1 ? 1 : 3);   // floats of a partial result
    __shared__ float part[4][SK_BLOCK_ROWS][NP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, r0 = blockIdx.x * SK_BLOCK_ROWS;
    const float* xb = X + (size_t)b * n * 3;
    const float* yb = Y + (size_t)b * m * 3;
    const float* gb = potY + (size_t)b * m;

    f32x4 x[SK_ROWS];
    float t[SK_ROWS], acc[SK_ROWS][3];
#pragma unroll
    for (int r = 0; r < SK_ROWS; ++r) {
        const int i = min(r0 + lane + 64 * r, n - 1);
        x[r] = sk_point(xb, i);
        t[r] = MODE == 0 ? 0.f : __builtin_fmaf(potX[(size_t)b * n + i], k, -logw);
        sk_init<MODE>(acc[r]);
    }
    for (int t0 = 0; t0 < m; t0 += SK_TILE) {
        const int cnt = min(SK_TILE, m - t0);
        __syncthreads();                               // the previous tile has been read
        for (int j = tid; j < cnt; j += 256) {
            sy[j] = sk_point(yb, t0 + j);
            sg[j] = gb[t0 + j] * k;
        }
        __syncthreads();
        const int c0 = wave * SK_WAVE_COLS, c1 = min(c0 + SK_WAVE_COLS, cnt);
        if (c0 < c1) sk_walk<MODE, SK_ROWS>(x, t, sy, sg, c0, c1, k, acc);
    }
#pragma unroll
    for (int r = 0; r < SK_ROWS; ++r)
#pragma unroll
        for (int q = 0; q < NP; ++q) part[wave][lane + 64 * r][q] = acc[r][q];
    __syncthreads();
    const int i = r0 + tid;
    if (tid < SK_BLOCK_ROWS && i < n) {
        float a[3], o[3] = {0.f, 0.f, 0.f};
        sk_init<MODE>(a);
        for (int q = 0; q < NP; ++q) a[q] = part[0][tid][q];
        for (int w = 1; w < 4; ++w) {
            for (int q = 0; q < NP; ++q) o[q] = part[w][tid][q];
            sk_merge<MODE>(a, o);
        }
        if (MODE == 0) {
            outp[(size_t)b * n + i] = sk_finite(sk_point(xb, i)) ? sk_potential(a, logw) * inv_k : __builtin_nanf("");
        } else if (MODE == 1) {
            outp[(size_t)b * n + i] = a[0];
        } else {
            const float s = 2.f * gout[b];
            float* d = outp + ((size_t)b * n + i) * 3;
            d[0] = s * a[0];
            d[1] = s * a[1];
            d[2] = s * a[2];
        }
    }
}

// out[b] = sum_i v[b, i] in fp64, a fixed order
__global__ __launch_bounds__(256) void sk_sum_kernel(const float* __restrict__ v, float* __restrict__ out, int n) {
    __shared__ double red[256];
    const int b = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)v[(size_t)b * n + i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[b] = (float)red[0];
}

struct SkScale {
    float k, inv_k;
    explicit SkScale(float eps) : k((float)(1.4426950408889634 / (double)eps)), inv_k((float)((double)eps * 0.6931471805599453)) {}
};
inline dim3 sk_grid(int n, int B) { return dim3((n + SK_BLOCK_ROWS - 1) / SK_BLOCK_ROWS, B); }

}  // namespace

// pairs workgroups; set_mode == 0: pair p is (A[p], B[p]); set_mode != 0: pair p = s * T + t is (A[s], B[t]).  f (pairs, N), g (pairs, M): null or
// the potentials.
int sinkhorn_resident_launch(const float* A, const float* Bc, float* f, float* g, float* out, int pairs, int T, int set_mode, int N, int M,
                             float eps, int iterations, hipStream_t st) {
    if (pairs <= 0 || N < 1 || M < 1 || (long long)N + M > GECCO_SINKHORN_RESIDENT_MAX_POINTS || (set_mode && T <= 0) || iterations < 1 ||
        !(eps > 0.f))
        return -2;
    if (const hipError_t e = lds_opt_in<sk_resident_kernel>(SK_LDS_BYTES - SK_RES_STATIC)) return (int)e;
    const SkScale sc(eps);
    hipLaunchKernelGGL(sk_resident_kernel, dim3(pairs), dim3(SK_RES_THREADS), (size_t)SK_PER_POINT * (N + M) + SK_RES_SCRATCH, st, A, Bc, f, g, out,
                       N, M, T, set_mode, sc.k, sc.inv_k, iterations);
    return (int)hipGetLastError();
}

// f (B, N), g (B, M): the potentials (outputs); ws (B, N): the row costs
int sinkhorn_stream_launch(const float* A, const float* Bc, float* f, float* g, float* ws, float* out, int B, int N, int M, float eps,
                           int iterations, hipStream_t st) {
    if (B <= 0 || B > 65535 || N < 1 || M < 1 || iterations < 1 || !(eps > 0.f)) return -2;
    const SkScale sc(eps);
    const float l2n = log2f((float)N), l2m = log2f((float)M);
    hipError_t e = hipMemsetAsync(g, 0, (size_t)B * M * sizeof(float), st);
    if (e != hipSuccess) return (int)e;
    for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(sk_stream_kernel<0>, sk_grid(N, B), dim3(256), 0, st, A, Bc, (const float*)nullptr, (const float*)g, f,
                           (const float*)nullptr, N, M, sc.k, sc.inv_k, l2m);
        hipLaunchKernelGGL(sk_stream_kernel<0>, sk_grid(M, B), dim3(256), 0, st, Bc, A, (const float*)nullptr, (const float*)f, g,
                           (const float*)nullptr, M, N, sc.k, sc.inv_k, l2n);
    }
    hipLaunchKernelGGL(sk_stream_kernel<1>, sk_grid(N, B), dim3(256), 0, st, A, Bc, (const float*)f, (const float*)g, ws, (const float*)nullptr, N,
                       M, sc.k, sc.inv_k, l2n + l2m);
    hipLaunchKernelGGL(sk_sum_kernel, dim3(B), dim3(256), 0, st, (const float*)ws, out, N);
    return (int)hipGetLastError();
}

// dA (B, N, 3) and / or dB (B, M, 3) (either may be null) on the saved potentials
int sinkhorn_bwd_launch(const float* A, const float* Bc, const float* f, const float* g, const float* gout, float* dA, float* dB, int B, int N,
                        int M, float eps, hipStream_t st) {
    if (B <= 0 || B > 65535 || N < 1 || M < 1 || !(eps > 0.f)) return -2;
    const SkScale sc(eps);
    const float lnm = log2f((float)N) + log2f((float)M);
    if (dA) hipLaunchKernelGGL(sk_stream_kernel<2>, sk_grid(N, B), dim3(256), 0, st, A, Bc, f, g, dA, gout, N, M, sc.k, sc.inv_k, lnm);
    if (dB) hipLaunchKernelGGL(sk_stream_kernel<2>, sk_grid(M, B), dim3(256), 0, st, Bc, A, g, f, dB, gout, M, N, sc.k, sc.inv_k, lnm);
    return (int)hipGetLastError();
}
