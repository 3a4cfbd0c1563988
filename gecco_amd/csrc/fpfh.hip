// Fast Point Feature Histograms and nearest-neighbour matching in feature space on the device (gfx950): what Open3D's
// compute_fpfh_feature / PCL's FPFHEstimation compute from the neighbour lists and the normals the library already produces, and the
// correspondences a global registration starts from (icp converges only from a good init, and nothing else in the library makes one).
// The reference has nothing of the kind; the route without this file is knn_gather -> the pair formulas in torch -> scatter_add
// histograms (float atomics) -> a gather and a weighted mean, and torch.cdist (an M x N matrix) -> argmin for the matching.
//
// Definition (gecco_fpfh_f32 and gecco_feature_nn_f32, include/gecco_hip.h; tests/_fpfh_ref.py restates both in numpy).
//   pair feature   fp64 on the fp32 inputs, every operation rounded, none contracted (fpfh_pair_bins, fpfh_pair.h): three bin coordinates u in
//                  [0, 11], bins clamp(floor(u), 0, 10) in three groups of 11
//   neighbourhood  entry t of idx[i, 0 .. k) counts when 0 <= j < N, j != i (by index), dist2(p_i, p_j) <= radius2 when there is a
//                  radius, and the twelve numbers of p_i, n_i, p_j, n_j are finite; m_i of them
//   SPFH           spfh[i, b] = fp32(100 count_b / m_i) in double, a zero row when m_i = 0: integer counts, one rounding
//   FPFH           over the counted entries with dist2 != 0 and m_j > 0, in list order: w = 1 / double(dist2), W = sum w, acc[b] =
//                  sum w double(spfh[j, b]); fpfh[i, b] = fp32(double(spfh[i, b]) + (W > 0 ? acc[b] / W : 0))
//   match          d2(i, j) = sum_c (a_ic - b_jc)^2 from 0 in channel order, fp32, none contracted, NaN -> +inf; the j of the smallest
//                  (d2, j): one monotone 64-bit key per pair (d2's bits above j), the spelling of the searches
//
// fpfh_spfh_kernel<T>: one thread per point, cloud_plan's grid over (cloud, tile of T points).  The tile's rows of idx are staged in
// LDS the way normals_kernel stages them (coalesced reads, row pitch k | 1).  A thread walks its k entries, computes the pair feature
// in fp64 and counts into 33 BYTE counters of its own in LDS, hist[bin][thread] (k <= 64 fits a byte): the bin index is dynamic, so
// counters in registers would go to scratch.  The tile's T x 33 outputs are then written by consecutive threads to consecutive words.
//
// fpfh_sum_kernel: FPFH_POINTS points per workgroup, 33 consecutive threads per point, thread = bin: the k rows of 33 floats a point
// gathers are 132 contiguous bytes each, read by consecutive lanes.  Every lane of a point evaluates the same predicate and the same
// w and W (the same loads: one request), and sums its own bin over t in list order in fp64.
//
// feature_nn_kernel<T, CP>: grid (cloud, tile of T queries, slice of b), one thread per query, the query's CP channels in registers
// (CP = the smallest of 4, 16, 36, 64 that holds C; channels C .. CP - 1 are zero on both sides, which adds exact zeros), b streamed
// through LDS in tiles of feature_tile_rows(CP) rows of CP floats (at most 32 KiB, pads zeroed once), read with broadcast b128 reads,
// four rows per step, ONE 64-bit key per thread.  Direct form: the thread writes idx and d2.  Split form: keys[(b * S + s) * M + i],
// and feature_nn_merge_kernel takes the minimum of a query's S keys, which is exact: both forms give the same bits.
//
// No atomics, no thread waits on another, every loop's trip count depends on the sizes alone; a row's bits depend on that row's inputs
// and nothing else, so they are the same run to run, in any batch position, for any launch geometry and in both forms.
#include "cloud_nn.h"
#include "fpfh_pair.h"
#include "kernels.h"
#include "launch_state.h"

namespace {

static_assert(GECCO_KNN_MAX_K <= 255, "a count fits a byte");   // (FPFH_BINS, fpfh_bin and fpfh_pair_bins: fpfh_pair.h)
constexpr int FPFH_SUM_THREADS = 256;
constexpr int FPFH_POINTS = FPFH_SUM_THREADS / FPFH_BINS;   // 7 points, 231 of 256 threads at work

// grid: B * tiles blocks, block (b, tile) owns points tile * T .. + T - 1 of cloud b.  LDS: T * (k | 1) words of idx, T words of m,
// 33 * T bytes of counters.
template <int T>
__global__ __launch_bounds__(T) void fpfh_spfh_kernel(const float* __restrict__ points, const float* __restrict__ normals,
                                                      const int* __restrict__ idx, float radius2, int use_radius, float* __restrict__ spfh,
                                                      int* __restrict__ count, int N, int k, int tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fpfh_lds[];
    const int pitch = k | 1;
    int* const ids = reinterpret_cast<int*>(fpfh_lds);
    int* const ms = ids + T * pitch;
    unsigned char* const hist = reinterpret_cast<unsigned char*>(ms + T);

    const int tid = threadIdx.x;
    const int qt = (int)(blockIdx.x % (unsigned)tiles), b = (int)(blockIdx.x / (unsigned)tiles);
    const int rows = min(T, N - qt * T);
    const size_t first = (size_t)b * N + (size_t)qt * T;   // the tile's first row
    {   // the tile's rows * k consecutive words of idx, word e to (row e / k, slot e % k); e advances by T per step
        const int words = rows * k, dr = T / k, dt = T % k;
        int r = tid / k, t = tid % k;
        for (int e = tid; e < words; e += T) {
            ids[r * pitch + t] = idx[first * k + e];
            r += dr;
            t += dt;
            if (t >= k) {
                t -= k;
                ++r;
            }
        }
    }
#pragma unroll
    for (int g = 0; g < FPFH_BINS; ++g) hist[g * T + tid] = 0;   // a thread's own bytes
    __syncthreads();

    int m = 0;
    if (tid < rows) {
        const int i = qt * T + tid;
        const float* pb = points + (size_t)b * N * 3;
        const float* nb = normals + (size_t)b * N * 3;
        const float pix = pb[3 * (size_t)i], piy = pb[3 * (size_t)i + 1], piz = pb[3 * (size_t)i + 2];
        const float nix = nb[3 * (size_t)i], niy = nb[3 * (size_t)i + 1], niz = nb[3 * (size_t)i + 2];
        const int* mine = ids + tid * pitch;
        if (cloud_finite3(pix, piy, piz) && cloud_finite3(nix, niy, niz)) {
            for (int t = 0; t < k; ++t) {
                const unsigned j = (unsigned)mine[t];
                if (j >= (unsigned)N || j == (unsigned)i) continue;   // an index outside [0, N) is never dereferenced
                const float pjx = pb[3 * (size_t)j], pjy = pb[3 * (size_t)j + 1], pjz = pb[3 * (size_t)j + 2];
                const float njx = nb[3 * (size_t)j], njy = nb[3 * (size_t)j + 1], njz = nb[3 * (size_t)j + 2];
                if (!cloud_finite3(pjx, pjy, pjz) || !cloud_finite3(njx, njy, njz)) continue;
                if (use_radius && !(cloud_dist2_inf(pix, piy, piz, pjx, pjy, pjz) <= radius2)) continue;
                int b0, b1, b2;
                fpfh_pair_bins(pix, piy, piz, nix, niy, niz, pjx, pjy, pjz, njx, njy, njz, b0, b1, b2);
                ++hist[b0 * T + tid];
                ++hist[(11 + b1) * T + tid];
                ++hist[(22 + b2) * T + tid];
                ++m;
            }
        }
        count[first + tid] = m;
    }
    ms[tid] = m;
    __syncthreads();
    // the tile's rows * 33 consecutive words of spfh: word e is (row e / 33, bin e % 33)
    const int words = rows * FPFH_BINS;
    for (int e = tid; e < words; e += T) {
        const int r = e / FPFH_BINS, g = e - r * FPFH_BINS;
        const int mr = ms[r];
        spfh[first * FPFH_BINS + e] = mr > 0 ? (float)((100.0 * (double)hist[g * T + r]) / (double)mr) : 0.f;
    }
}

// grid: B * tiles blocks, block (b, tile) owns points tile * FPFH_POINTS .. + FPFH_POINTS - 1, thread (point, bin)
__global__ __launch_bounds__(FPFH_SUM_THREADS) void fpfh_sum_kernel(const float* __restrict__ points, const float* __restrict__ normals,
                                                                    const int* __restrict__ idx, float radius2, int use_radius,
                                                                    const float* __restrict__ spfh, const int* __restrict__ count,
                                                                    float* __restrict__ fpfh, int N, int k, int tiles) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const int pl = tid / FPFH_BINS, g = tid - pl * FPFH_BINS;
    const int qt = (int)(blockIdx.x % (unsigned)tiles), b = (int)(blockIdx.x / (unsigned)tiles);
    const int i = qt * FPFH_POINTS + pl;
    if (pl >= FPFH_POINTS || i >= N) return;   // (no barrier in this kernel)
    const float* pb = points + (size_t)b * N * 3;
    const float* nb = normals + (size_t)b * N * 3;
    const float* sb = spfh + (size_t)b * N * FPFH_BINS;
    const int* cb = count + (size_t)b * N;
    const int* mine = idx + ((size_t)b * N + i) * k;
    const float pix = pb[3 * (size_t)i], piy = pb[3 * (size_t)i + 1], piz = pb[3 * (size_t)i + 2];
    const float nix = nb[3 * (size_t)i], niy = nb[3 * (size_t)i + 1], niz = nb[3 * (size_t)i + 2];
    double W = 0.0, acc = 0.0;
    if (cloud_finite3(pix, piy, piz) && cloud_finite3(nix, niy, niz)) {
        for (int t = 0; t < k; ++t) {
            const unsigned j = (unsigned)mine[t];
            if (j >= (unsigned)N || j == (unsigned)i) continue;
            const float pjx = pb[3 * (size_t)j], pjy = pb[3 * (size_t)j + 1], pjz = pb[3 * (size_t)j + 2];
            const float njx = nb[3 * (size_t)j], njy = nb[3 * (size_t)j + 1], njz = nb[3 * (size_t)j + 2];
            if (!cloud_finite3(pjx, pjy, pjz) || !cloud_finite3(njx, njy, njz)) continue;
            const float d2 = cloud_dist2_inf(pix, piy, piz, pjx, pjy, pjz);
            if (use_radius && !(d2 <= radius2)) continue;
            if (d2 == 0.f || cb[j] <= 0) continue;
            const double w = 1.0 / (double)d2;
            W = W + w;
            acc = acc + w * (double)sb[(size_t)j * FPFH_BINS + g];
        }
    }
    const size_t o = ((size_t)b * N + i) * FPFH_BINS + g;
    fpfh[o] = (float)((double)spfh[o] + (W > 0.0 ? acc / W : 0.0));
}

typedef unsigned long long feature_key;

// rows of b per LDS tile: CLOUD_TILE while they fit 32 KiB (two or more workgroups per CU whatever T), fewer for the wide rows
constexpr int feature_tile_rows(int CP) { return CP <= 16 ? CLOUD_TILE : CP <= 36 ? 224 : 128; }
static_assert(4 * 36 * feature_tile_rows(36) <= 32 * 1024 && 4 * 64 * feature_tile_rows(64) <= 32 * 1024 &&
              4 * 16 * feature_tile_rows(16) <= 32 * 1024 && GECCO_FEATURE_MAX_DIM == 64, "a tile of b stays within 32 KiB of LDS");

// d2 of the query in registers and one row of the tile, as the bits that order it (NaN -> +inf)
template <int CP>
static __device__ __forceinline__ unsigned feature_dist2_bits(const float (&q)[CP], const float* row) {
#pragma clang fp contract(off)
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < CP; c += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + c);   // every lane the same address: a broadcast read
        const float e0 = q[c] - v[0], e1 = q[c + 1] - v[1], e2 = q[c + 2] - v[2], e3 = q[c + 3] - v[3];
        acc = acc + e0 * e0;
        acc = acc + e1 * e1;
        acc = acc + e2 * e2;
        acc = acc + e3 * e3;
    }
    return __float_as_uint(__builtin_fminf(acc, __builtin_inff()));
}

// grid: B * tiles * S blocks, block (b, tile, s) scans rows [s * slice, min(N, (s + 1) * slice)) of b for queries tile * T ..
// keys null: the direct form (S = 1), idx and d2 are written; otherwise keys[(b * S + s) * M + i]
template <int T, int CP>
__global__ __launch_bounds__(T) void feature_nn_kernel(const float* __restrict__ a, const float* __restrict__ bf, int* __restrict__ idx,
                                                       float* __restrict__ d2, feature_key* __restrict__ keys, int M, int N, int C, int tiles,
                                                       int S, unsigned slice) {
    constexpr int TR = feature_tile_rows(CP);
    __shared__ __attribute__((aligned(16))) float tile[TR * CP];

    const int tid = threadIdx.x;
    const unsigned bid = blockIdx.x;
    const int s = (int)(bid % (unsigned)S), qt = (int)((bid / (unsigned)S) % (unsigned)tiles), b = (int)(bid / (unsigned)S / (unsigned)tiles);
    const unsigned lo = (unsigned)s * slice, hi = min((unsigned)N, lo + slice);
    const int i = qt * T + tid;
    const bool valid = i < M;

    float q[CP];
    {
        const float* ap = a + ((size_t)b * M + (valid ? i : 0)) * C;
#pragma unroll
        for (int c = 0; c < CP; ++c) q[c] = c < C ? ap[c] : 0.f;
    }
    for (int e = tid; e < TR * CP; e += T) tile[e] = 0.f;   // channels C .. CP - 1 stay zero: the loads below never touch them

    unsigned best_bits = 0xffffffffu, best_j = 0xffffffffu;   // above every key: dist2's bits are at most +inf's
    // j ascends in a scan, so an equal dist2 has the higher index and loses: the compare is on dist2's bits alone
    auto single = [&](unsigned u, unsigned j) {
        if (u < best_bits) {
            best_bits = u;
            best_j = j;
        }
    };
    const int dr = T / C, dt = T % C;
    for (unsigned base = lo; base < hi; base += TR) {
        __syncthreads();   // the scan of the previous tile (the zero fill) is over
        const int cnt = (int)min((unsigned)TR, hi - base);   // rows past cnt are never candidates
        {   // cnt * C consecutive words of b, word e to (row e / C, channel e % C); e advances by T per step
            const float* src = bf + ((size_t)b * N + base) * C;
            const int words = cnt * C;
            int r = tid / C, c = tid % C;
            for (int e = tid; e < words; e += T) {
                tile[r * CP + c] = src[e];
                r += dr;
                c += dt;
                if (c >= C) {
                    c -= C;
                    ++r;
                }
            }
        }
        __syncthreads();
        if (!valid) continue;
        int g = 0;
        for (; g + 4 <= cnt; g += 4) {
            const unsigned u0 = feature_dist2_bits<CP>(q, tile + g * CP), u1 = feature_dist2_bits<CP>(q, tile + (g + 1) * CP);
            const unsigned u2 = feature_dist2_bits<CP>(q, tile + (g + 2) * CP), u3 = feature_dist2_bits<CP>(q, tile + (g + 3) * CP);
            if (min(min(u0, u1), min(u2, u3)) < best_bits) {   // ascending j inside the step
                single(u0, base + g);
                single(u1, base + g + 1);
                single(u2, base + g + 2);
                single(u3, base + g + 3);
            }
        }
        for (; g < cnt; ++g) single(feature_dist2_bits<CP>(q, tile + g * CP), base + g);
    }
    if (!valid) return;
    if (keys) {
        keys[((size_t)b * S + s) * (size_t)M + i] = ((feature_key)best_bits << 32) | (feature_key)best_j;   // a slice holds a row: best_j < N
    } else {
        idx[(size_t)b * M + i] = (int)best_j;
        if (d2) d2[(size_t)b * M + i] = __uint_as_float(best_bits);
    }
}

// one thread per query: the minimum of its S slice keys.  total = B * M
__global__ __launch_bounds__(256) void feature_nn_merge_kernel(const feature_key* __restrict__ keys, int* __restrict__ idx,
                                                               float* __restrict__ d2, long long total, int M, int S) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long b = e / M, i = e - b * M;
    const feature_key* kb = keys + (size_t)b * S * (size_t)M + i;
    feature_key key = kb[0];
    for (int s = 1; s < S; ++s) {
        const feature_key other = kb[(size_t)s * M];
        key = other < key ? other : key;
    }
    idx[e] = (int)(unsigned)(key & 0xffffffffu);
    if (d2) d2[e] = __uint_as_float((unsigned)(key >> 32));
}

// f(std::integral_constant<int, CP>) for the smallest padded width CP of 4, 16, 36, 64 that holds C (33 lands on 36)
template <class F>
inline auto dispatch_width(int C, F f) {
    if (C <= 4) return f(std::integral_constant<int, 4>{});
    if (C <= 16) return f(std::integral_constant<int, 16>{});
    if (C <= 36) return f(std::integral_constant<int, 36>{});
    return f(std::integral_constant<int, 64>{});
}

}  // namespace

// Two launches.  radius2 <= 0, +inf or NaN: no radius.  -2: sizes out of range, -3: a grid would pass 2^31 - 1 workgroups
int fpfh_launch(const float* points, const float* normals, const int* idx, float radius2, float* fpfh, float* spfh, int* count, int B, int N,
                int k, hipStream_t st) {
    if (B < 1 || N < 1 || k < 1 || k > GECCO_KNN_MAX_K) return -2;
    const int use_radius = radius2 > 0.f && radius2 <= 3.402823466e38f ? 1 : 0;
    const CloudPlan p = cloud_plan(B, N, N, 1, false, cloud_max_threads(k), device_cus());
    const long long sum_tiles = ((long long)N + FPFH_POINTS - 1) / FPFH_POINTS;
    if (!p.fits() || (long long)B * sum_tiles > 0x7fffffffLL) return -3;
    const size_t lds = (size_t)4 * p.T * (k | 1) + (size_t)4 * p.T + (size_t)FPFH_BINS * p.T;
    dispatch_T(p.T, [&](auto t) {
        hipLaunchKernelGGL(fpfh_spfh_kernel<decltype(t)::value>, dim3((unsigned)p.blocks), dim3(p.T), lds, st, points, normals, idx, radius2,
                           use_radius, spfh, count, N, k, p.tiles);
    });
    hipLaunchKernelGGL(fpfh_sum_kernel, dim3((unsigned)(B * sum_tiles)), dim3(FPFH_SUM_THREADS), 0, st, points, normals, idx, radius2,
                       use_radius, spfh, count, fpfh, N, k, (int)sum_tiles);
    return (int)hipGetLastError();
}

// form 0 / 1 / 2: cloud_plan's forms (auto without ws runs the direct form); ws of GECCO_FEATURE_NN_WORKSPACE_BYTES(B, M, N) for the
// split form; d2 nullable.  -2: arguments out of range, -3: a grid would pass 2^31 - 1 workgroups
int feature_nn_launch(const float* a, const float* b, int* idx, float* d2, void* ws, int B, int M, int N, int C, int form, hipStream_t st) {
    if (B < 1 || M < 1 || N < 1 || C < 1 || C > GECCO_FEATURE_MAX_DIM || form < 0 || form > 2 || (form == 2 && !ws)) return -2;
    const CloudPlan p = cloud_plan(B, M, N, form, ws != nullptr, 256, device_cus());
    const long long total = (long long)B * M;
    if (!p.fits() || (total + 255) / 256 > 0x7fffffffLL) return -3;
    feature_key* keys = p.split ? static_cast<feature_key*>(ws) : nullptr;
    const unsigned slice = p.S == 1 ? (unsigned)N : (unsigned)GECCO_KNN_SPLIT_SLICE;
    dispatch_T(p.T, [&](auto t) {
        dispatch_width(C, [&](auto w) {
            hipLaunchKernelGGL((feature_nn_kernel<decltype(t)::value, decltype(w)::value>), dim3((unsigned)p.blocks), dim3(p.T), 0, st, a, b,
                               idx, d2, keys, M, N, C, p.tiles, p.S, slice);
        });
    });
    if (p.split)
        hipLaunchKernelGGL(feature_nn_merge_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, keys, idx, d2, total, M, p.S);
    return (int)hipGetLastError();
}
