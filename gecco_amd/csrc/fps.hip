// Farthest-point sampling of 3-D clouds on the device (gfx950): k points of a cloud of N, each the point farthest from those chosen
// before it.  The reference cuts clouds by random permutation only (gecco-jax data/torch_shapenet.py:20-21, data/taskonomy.py:84,
// data/shapenet_vol.py:148-150); this is the well-spread cut every point-cloud library ships beside it.
//
// Definition (gecco_fps_f32, include/gecco_hip.h; tests/_fps_ref.py restates it in numpy float32).  d_i = +inf; for t = 0 .. k-1:
//     idx[t] = s_t;  sel2[t] = d_{s_t};  d_i = min(d_i, dist2(p_i, p_{s_t}));  s_{t+1} = argmax_i d_i, the LOWEST index of equal maxima
// dist2(a, b) = (dx dx + dy dy) + dz dz on the coordinate differences, every operation rounded to fp32 and none contracted into an
// FMA (cloud_dist2 of cloud_nn.h spells the roundings out, as pair_dist.h does for its form and for the same reason): near-ties
// between candidates are closer than an FMA's rounding, so the roundings are part of the definition.
//
// The argmax is the maximum of ONE 64-bit key per candidate: d's bits in the high word (d >= 0, so they order as unsigned integers)
// and ~index in the low word, so the largest key is the largest d and, among equals, the lowest index.  A maximum of integers has
// no order of evaluation to fix: both forms give the same bits, run to run and in any batch position.  No float atomics, no atomics.
// A candidate enters with `d > best`, so a NaN distance never wins; min() keeps a NaN once it is there (as np.minimum does).  A
// thread (or a whole cloud) without a winning candidate contributes key 0, which decodes to an index >= N and is replaced by 0:
// every index written is in [0, N) whatever the coordinates are.
//
// Resident form.  One workgroup per cloud and ONE launch for all B clouds and all k steps.  A thread keeps P = 1, 2, 4 or 8 points
// (coordinates and running d) in registers, point tid + j * blockDim; a copy of the coordinates (16 B per point) sits in LDS so that
// every thread reads the winner's coordinates at one address (a broadcast read).  A step: update the P points, keep the local best,
// reduce the key over the wave (__shfl_xor), lane 0 writes the wave's key into one of 16 LDS slots, ONE __syncthreads, every thread
// takes the maximum of the 16 slots.  Two slot sets alternate: a wave that runs ahead writes the other set, and cannot come back to
// this one before every wave has passed the next barrier, i.e. has read it.
// The limit GECCO_FPS_RESIDENT_MAX_POINTS = 1024 threads * 8 points in registers = 8192; their LDS copy is 128 KiB of the CU's 160.
//
// Streaming form.  Any N.  A workgroup of 256 threads owns a slice of FPS_SLICE = 1024 points of one cloud; the running d lives in
// the workspace.  ONE LAUNCH PER SELECTED POINT: launch t reduces the per-workgroup keys launch t - 1 wrote (every workgroup does
// so, redundantly: N / 1024 entries), which is s_t; workgroup 0 of the cloud writes idx[t], sel2[t]; every workgroup updates its
// slice against p_{s_t} and writes its key into the other of two key buffers.  Launch 0 takes s_0 from `start` and d = +inf from
// nowhere, so the workspace is never read before it is written.  No workgroup waits on another inside a kernel: the order between
// steps is the stream's order between launches, so the chain cannot hang however few workgroups are co-resident.
#include "cloud_nn.h"
#include "kernels.h"
#include "launch_state.h"

namespace {

typedef unsigned long long fps_key;

constexpr int FPS_RES_THREADS = 1024;
constexpr int FPS_RES_WAVES = FPS_RES_THREADS / 64;
constexpr int FPS_RES_MAX_P = 8;                      // points per thread, in registers
constexpr int FPS_LDS_BYTES = 160 * 1024;             // per CU
static_assert(GECCO_FPS_RESIDENT_MAX_POINTS == FPS_RES_THREADS * FPS_RES_MAX_P, "the resident limit is 1024 threads * 8 points in registers");
static_assert(16 * GECCO_FPS_RESIDENT_MAX_POINTS + 2 * FPS_RES_WAVES * (int)sizeof(fps_key) <= FPS_LDS_BYTES, "the LDS copy of the cloud fits one CU");
constexpr int FPS_STR_THREADS = 256;
constexpr int FPS_STR_WAVES = FPS_STR_THREADS / 64;
constexpr int FPS_STR_P = GECCO_FPS_STREAM_SLICE / FPS_STR_THREADS;
static_assert(FPS_STR_P * FPS_STR_THREADS == GECCO_FPS_STREAM_SLICE, "a slice is a whole number of points per thread");

// min that keeps a NaN (np.minimum): a point with a NaN distance stays out of every later comparison
static __device__ __forceinline__ float fps_min(float d, float v) { return (v < d || v != v) ? v : d; }
static __device__ __forceinline__ fps_key fps_make_key(float d, int i) {
    return ((fps_key)__float_as_uint(d) << 32) | (fps_key)(~(unsigned)i);
}
static __device__ __forceinline__ fps_key fps_max(fps_key a, fps_key b) { return a > b ? a : b; }
static __device__ __forceinline__ fps_key fps_wave_max(fps_key v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fps_max(v, (fps_key)__shfl_xor((unsigned long long)v, off, 64));
    return v;
}
// key -> (index in [0, N), d of the winner)
static __device__ __forceinline__ int fps_decode(fps_key key, int N, float* d) {
    const unsigned i = ~(unsigned)(key & 0xffffffffu);
    *d = __uint_as_float((unsigned)(key >> 32));
    return i < (unsigned)N ? (int)i : 0;
}
static __device__ __forceinline__ int fps_start(const int* __restrict__ start, int b, int N) {
    const int s = start ? start[b] : 0;
    return min(max(s, 0), N - 1);
}

// ------------------------------------------------------------------------------------------------------------- resident form
template <int P>
__global__ __launch_bounds__(FPS_RES_THREADS) void fps_resident_kernel(const float* __restrict__ points, const int* __restrict__ start,
                                                                       int* __restrict__ idx, float* __restrict__ sel2, int N, int k) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fps_lds[];
    f32x4* lp = reinterpret_cast<f32x4*>(fps_lds);      // N points
    __shared__ __attribute__((aligned(16))) fps_key slots[2][FPS_RES_WAVES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = blockDim.x, b = blockIdx.x;
    const float* pb = points + (size_t)b * N * 3;
    float x[P], y[P], z[P], d[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int i = tid + j * T;
        const bool valid = i < N;
        x[j] = valid ? pb[3 * (size_t)i] : 0.f;
        y[j] = valid ? pb[3 * (size_t)i + 1] : 0.f;
        z[j] = valid ? pb[3 * (size_t)i + 2] : 0.f;
        d[j] = valid ? __builtin_inff() : -1.f;         // -1: below every distance, never a candidate
        if (valid) lp[i] = f32x4{x[j], y[j], z[j], 0.f};
    }
    if (tid < 2 * FPS_RES_WAVES) (&slots[0][0])[tid] = 0;   // the slots of waves that do not exist stay 0
    __syncthreads();

    int s = fps_start(start, b, N), par = 0;
    float ds = __builtin_inff();
    for (int t = 0;; ++t) {
        if (tid == 0) {
            idx[(size_t)b * k + t] = s;
            if (sel2) sel2[(size_t)b * k + t] = ds;
        }
        if (t == k - 1) break;
        const f32x4 c = lp[s];
        float bd = -1.f;
        int bj = 0;
#pragma unroll
        for (int j = 0; j < P; ++j) {                   // ascending j is ascending index: `>` keeps the lowest of equals
            d[j] = fps_min(d[j], cloud_dist2(x[j], y[j], z[j], c[0], c[1], c[2]));
            if (d[j] > bd) {
                bd = d[j];
                bj = j;
            }
        }
        const fps_key mine = fps_wave_max(bd >= 0.f ? fps_make_key(bd, tid + bj * T) : (fps_key)0);
        if (lane == 0) slots[par][wave] = mine;
        __syncthreads();
        fps_key best = 0;
#pragma unroll
        for (int w = 0; w < FPS_RES_WAVES; ++w) best = fps_max(best, slots[par][w]);
        s = fps_decode(best, N, &ds);
        par ^= 1;
    }
}

// ------------------------------------------------------------------------------------------------------------ streaming form
// Launch t of k.  d (B, N): the running distances; keys (2, B, G): the per-workgroup winners, set t & 1 written, set (t - 1) & 1 read.
__global__ __launch_bounds__(FPS_STR_THREADS) void fps_stream_kernel(const float* __restrict__ points, const int* __restrict__ start,
                                                                     int* __restrict__ idx, float* __restrict__ sel2, float* __restrict__ dws,
                                                                     fps_key* __restrict__ keys, int B, int N, int k, int G, int t) {
    __shared__ fps_key red[2][FPS_STR_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / G, g = blockIdx.x - b * G;
    const float* pb = points + (size_t)b * N * 3;

    int s;
    float ds = __builtin_inff();
    if (t == 0) {
        s = fps_start(start, b, N);
    } else {
        const fps_key* prev = keys + ((size_t)((t - 1) & 1) * B + b) * G;
        fps_key v = 0;
        for (int i = tid; i < G; i += FPS_STR_THREADS) v = fps_max(v, prev[i]);
        v = fps_wave_max(v);
        if (lane == 0) red[0][wave] = v;
        __syncthreads();
        v = red[0][0];
#pragma unroll
        for (int w = 1; w < FPS_STR_WAVES; ++w) v = fps_max(v, red[0][w]);
        s = fps_decode(v, N, &ds);
    }
    if (g == 0 && tid == 0) {
        idx[(size_t)b * k + t] = s;
        if (sel2) sel2[(size_t)b * k + t] = ds;
    }
    if (t == k - 1) return;                              // (uniform in the grid: nothing follows the last selection)

    const float cx = pb[3 * (size_t)s], cy = pb[3 * (size_t)s + 1], cz = pb[3 * (size_t)s + 2];
    float* db = dws + (size_t)b * N;
    float bd = -1.f;
    int bi = 0;
#pragma unroll
    for (int j = 0; j < FPS_STR_P; ++j) {
        const int i = g * GECCO_FPS_STREAM_SLICE + j * FPS_STR_THREADS + tid;
        if (i < N) {
            const float old = t == 0 ? __builtin_inff() : db[i];
            const float dn = fps_min(old, cloud_dist2(pb[3 * (size_t)i], pb[3 * (size_t)i + 1], pb[3 * (size_t)i + 2], cx, cy, cz));
            db[i] = dn;
            if (dn > bd) {
                bd = dn;
                bi = i;
            }
        }
    }
    const fps_key mine = fps_wave_max(bd >= 0.f ? fps_make_key(bd, bi) : (fps_key)0);
    if (lane == 0) red[1][wave] = mine;
    __syncthreads();
    if (tid == 0) {
        fps_key v = red[1][0];
#pragma unroll
        for (int w = 1; w < FPS_STR_WAVES; ++w) v = fps_max(v, red[1][w]);
        keys[((size_t)(t & 1) * B + b) * G + g] = v;
    }
}

template <int P>
void fps_resident_go(const float* points, const int* start, int* idx, float* sel2, int B, int N, int k, hipStream_t st) {
    const int per = (N + P - 1) / P, threads = min(FPS_RES_THREADS, (per + 63) / 64 * 64);
    hipLaunchKernelGGL(fps_resident_kernel<P>, dim3(B), dim3(threads), (size_t)16 * N, st, points, start, idx, sel2, N, k);
}

}  // namespace

int fps_resident_launch(const float* points, const int* start, int* idx, float* sel2, int B, int N, int k, hipStream_t st) {
    if (B < 1 || N < 1 || N > GECCO_FPS_RESIDENT_MAX_POINTS || k < 1 || k > N) return -2;
    if (const hipError_t e = lds_opt_in<fps_resident_kernel<1>, fps_resident_kernel<2>, fps_resident_kernel<4>, fps_resident_kernel<8>>(
            (size_t)16 * GECCO_FPS_RESIDENT_MAX_POINTS))
        return (int)e;
    const int per = (N + FPS_RES_THREADS - 1) / FPS_RES_THREADS;   // the fewest points per thread that cover the cloud
    if (per <= 1) fps_resident_go<1>(points, start, idx, sel2, B, N, k, st);
    else if (per <= 2) fps_resident_go<2>(points, start, idx, sel2, B, N, k, st);
    else if (per <= 4) fps_resident_go<4>(points, start, idx, sel2, B, N, k, st);
    else fps_resident_go<8>(points, start, idx, sel2, B, N, k, st);
    return (int)hipGetLastError();
}

// ws: gecco_fps_workspace_bytes(B, N) bytes — d (B, N) fp32, then (8-byte aligned) the two key buffers (2, B, G) of 8 bytes each
int fps_stream_launch(const float* points, const int* start, int* idx, float* sel2, void* ws, int B, int N, int k, hipStream_t st) {
    if (B < 1 || N < 1 || k < 1 || k > N || !ws) return -2;
    const int G = (N + GECCO_FPS_STREAM_SLICE - 1) / GECCO_FPS_STREAM_SLICE;
    if ((long long)B * G > 0x7fffffffLL) return -2;
    float* dws = static_cast<float*>(ws);
    fps_key* keys = reinterpret_cast<fps_key*>(static_cast<unsigned char*>(ws) + (((size_t)B * N * sizeof(float) + 7) & ~(size_t)7));
    for (int t = 0; t < k; ++t)
        hipLaunchKernelGGL(fps_stream_kernel, dim3(B * G), dim3(FPS_STR_THREADS), 0, st, points, start, idx, sel2, dws, keys, B, N, k, G, t);
    return (int)hipGetLastError();
}
