// Fast Point Feature Histograms from radius neighbourhoods on the grid index of grid.hip (gfx950): Open3D's compute_fpfh_feature(
// KDTreeSearchParamRadius(r)), PCL's FPFHEstimation::setRadiusSearch.  The neighbourhood is every point within r, unbounded, the ball
// normals_grid.hip fits its normals to; fpfh.hip's lists come from the brute-force knn, stop at GECCO_KNN_MAX_K and count into bytes.
// Nothing here writes a neighbour list: a thread walks the cells its ball can reach, twice.
//
// Definition (gecco_fpfh_grid_f32, include/gecco_hip.h; tests/_fpfh_grid_ref.py restates it in numpy).  Per cloud, with r2 =
// fp32(radius^2) from the caller:
//   ball          of point i: the j with cloud_dist2_bits(p_i, p_j) <= r2 bits (radius.hip's predicate), visited in ascending sorted
//                 position of the index, the off-grid tail last (grid_walk's order, part of the definition as it is for ISS and
//                 normals_grid.hip).  A non-finite p_i has an empty ball, a non-finite p_j is in nobody's ball
//   counted       a member of the ball with j != i BY INDEX (an exact duplicate of the point stays a neighbour and contributes the zero
//   neighbour     triple, bins 5, 16, 27, as in fpfh.hip) and all six numbers of n_i and n_j finite.  m_i = their number, never clamped:
//                 it may exceed 64 and 255
//   pair feature  steps 1 - 9 of gecco_fpfh_f32's definition, by the same code (fpfh_pair.h)
//   SPFH          spfh[i, b] = fp32((100.0 count_b) / m_i) in double, 32-bit integer counts, a zero row when m_i = 0
//   FPFH          over the counted neighbours in ball order that have dist2 != 0 and m_j > 0: w = 1 / double(dist2), dist2 the value the
//                 walk tested; W = sum w, acc[b] = sum w double(spfh[j, b]), each sum one rounded fp64 operation per term, nothing
//                 contracted; fpfh[i, b] = fp32(double(spfh[i, b]) + (W > 0 ? acc[b] / W : 0))
// count and spfh are integer counts with one rounding, so they do not depend on the index's cell_size or origin; fpfh sums in ball
// order, which those fix: the same bits run to run, in any batch position and at any workgroup size, and with another cell or origin
// a difference in the last fp32 place at most.
//
// Two launches, one thread per SORTED POSITION in both (iss.hip's convention): thread t of a cloud owns the point at sorted[t], whose
// 16-byte load gives the coordinates and, in .w, the row i its outputs go to; a neighbour's coordinates come with the walk and its
// normal is gathered by j from the caller's array (in the first launch), so neither kernel reads a points array.  The lanes of a wave are neighbours in the
// sorted order: they probe the same cells and read the same runs.
//   fpfh_grid_spfh_kernel<T>  the visitor computes the pair bins and counts into the thread's own 33 32-BIT counters in LDS,
//                 hist[bin][thread] (the bin is dynamic: counters in registers would go to scratch).  33 T words, 33 KiB at T = 256,
//                 static.  Word bin * T + thread lies in bank thread % 64 whatever the bin (T is a multiple of the 64 banks), so the
//                 lanes of a wave never meet in a bank.  A thread reads and writes its own words only: no barrier.  It then writes its
//                 row of spfh and its count
//   fpfh_grid_sum_kernel<T>   the same walk and the same predicate, read off the counts (m_i > 0 says that p_i and n_i are finite, m_j >
//                 0 that n_j is: no normal is gathered again); the 33 fp64 accumulators in registers, the bin loop fully unrolled so
//                 that every index is static (no scratch).  fpfh_sum_kernel's layout, 33 lanes per point, repeats the walk (probes,
//                 dist2, the normal's finiteness) on 33 lanes for the sake of coalesced reads of the 132-byte rows: the same bits,
//                 and on an MI355X about twice the time of this kernel
// No atomics, no workspace, no thread waits on another, every loop is bounded by a constant, by cap or by N (grid_walk.h).
#include "cloud_nn.h"
#include "fpfh_pair.h"
#include "grid_walk.h"
#include "kernels.h"
#include "launch_state.h"

namespace {

// grid: B * tiles blocks of T sorted positions.  LDS: 33 * T words of counters
template <int T>
__global__ __launch_bounds__(T) void fpfh_grid_spfh_kernel(const GridView index, const float* __restrict__ normals, float R, unsigned r2_bits,
                                                           float* __restrict__ spfh, int* __restrict__ count, int tiles) {
    static_assert(T % 64 == 0, "a thread's counters share one LDS bank");
    __shared__ unsigned hist[FPFH_BINS * T];
    const int N = index.N, tid = (int)threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)tiles);
    const int t = (int)(blockIdx.x % (unsigned)tiles) * T + tid;
    if (t >= N) return;   // (no barrier below)
    const f32x4 own = index.cloud(b)[t];
    const unsigned i = __float_as_uint(own[3]);
    if (i >= (unsigned)N) return;   // a sorted array no build wrote: nothing outside the outputs is written
#pragma unroll
    for (int g = 0; g < FPFH_BINS; ++g) hist[g * T + tid] = 0u;   // the thread's own words
    const float pix = own[0], piy = own[1], piz = own[2];
    const float* nb = normals + (size_t)b * N * 3;
    const float nix = nb[3 * (size_t)i], niy = nb[3 * (size_t)i + 1], niz = nb[3 * (size_t)i + 2];
    int m = 0;
    if (cloud_finite3(pix, piy, piz) && cloud_finite3(nix, niy, niz))   // (a non-finite point has dist2 = +inf to everything)
        grid_walk(index, b, pix, piy, piz, R, r2_bits, [&](const f32x4 p, unsigned) {
            const unsigned j = __float_as_uint(p[3]);
            if (j >= (unsigned)N || j == i) return;   // an index outside [0, N) is never dereferenced
            const float njx = nb[3 * (size_t)j], njy = nb[3 * (size_t)j + 1], njz = nb[3 * (size_t)j + 2];
            if (!cloud_finite3(njx, njy, njz)) return;   // (p is finite: its dist2 is)
            int b0, b1, b2;
            fpfh_pair_bins(pix, piy, piz, nix, niy, niz, p[0], p[1], p[2], njx, njy, njz, b0, b1, b2);
            ++hist[b0 * T + tid];
            ++hist[(11 + b1) * T + tid];
            ++hist[(22 + b2) * T + tid];
            ++m;
        });
    const size_t row = (size_t)b * N + i;
    count[row] = m;
    float* out = spfh + row * FPFH_BINS;
#pragma unroll
    for (int g = 0; g < FPFH_BINS; ++g) out[g] = m > 0 ? (float)((100.0 * (double)hist[g * T + tid]) / (double)m) : 0.f;
}

// grid: B * tiles blocks of T sorted positions
template <int T>
__global__ __launch_bounds__(T) void fpfh_grid_sum_kernel(const GridView index, float R, unsigned r2_bits, const float* __restrict__ spfh,
                                                          const int* __restrict__ count, float* __restrict__ fpfh, int tiles) {
#pragma clang fp contract(off)
    const int N = index.N;
    const int b = (int)(blockIdx.x / (unsigned)tiles);
    const int t = (int)(blockIdx.x % (unsigned)tiles) * T + (int)threadIdx.x;
    if (t >= N) return;   // (no barrier below)
    const f32x4 own = index.cloud(b)[t];
    const unsigned i = __float_as_uint(own[3]);
    if (i >= (unsigned)N) return;
    const float* sb = spfh + (size_t)b * N * FPFH_BINS;
    const int* cb = count + (size_t)b * N;
    double W = 0.0, acc[FPFH_BINS];   // every index below is static: registers
#pragma unroll
    for (int g = 0; g < FPFH_BINS; ++g) acc[g] = 0.0;
    // The counts stand for the normals here.  m_i > 0: p_i and n_i are finite; m_i = 0: the sum is empty (no counted neighbour, or a
    // non-finite p_i or n_i, which counts nobody).  m_j > 0: n_j is finite, so j, in the ball and not i, is a counted neighbour
    if (cb[i] > 0)
        grid_walk(index, b, own[0], own[1], own[2], R, r2_bits, [&](const f32x4 p, unsigned u) {
#pragma clang fp contract(off)
            const unsigned j = __float_as_uint(p[3]);
            if (j >= (unsigned)N || j == i) return;
            if (u == 0u || cb[j] <= 0) return;   // u: the bits of dist2 >= 0, the value the walk tested
            const double w = 1.0 / (double)__uint_as_float(u);
            const float* sj = sb + (size_t)j * FPFH_BINS;
            W = W + w;
#pragma unroll
            for (int g = 0; g < FPFH_BINS; ++g) acc[g] = acc[g] + w * (double)sj[g];
        });
    const size_t o = ((size_t)b * N + i) * FPFH_BINS;
#pragma unroll
    for (int g = 0; g < FPFH_BINS; ++g) fpfh[o + g] = (float)((double)spfh[o + g] + (W > 0.0 ? acc[g] / W : 0.0));
}

}  // namespace

// Two launches.  -2: arguments out of range (a radius2 above fp32(cell_size^2) among them), -3: the grid would pass 2^31 - 1 workgroups
int fpfh_grid_launch(const float* normals, const GridIndexArgs& index, float r2, float* fpfh, float* spfh, int* count, int B, int N,
                     hipStream_t st) {
    const GridView g = grid_view(index, B, N);
    if (!g.sorted || !normals || !fpfh || !spfh || !count) return -2;
    if (!grid_radius2_ok(r2, index.cell_size)) return -2;
    const CloudPlan p = cloud_plan(B, N, N, 1, false, 256, device_cus());
    if (!p.fits()) return -3;
    return dispatch_T(p.T, [&](auto t) -> int {
        constexpr int T = decltype(t)::value;
        const dim3 grid((unsigned)p.blocks), block(T);
        const float R = grid_reach(r2);
        const unsigned r2_bits = __builtin_bit_cast(unsigned, r2);
        hipLaunchKernelGGL((fpfh_grid_spfh_kernel<T>), grid, block, 0, st, g, normals, R, r2_bits, spfh, count, p.tiles);
        hipLaunchKernelGGL((fpfh_grid_sum_kernel<T>), grid, block, 0, st, g, R, r2_bits, spfh, count, fpfh, p.tiles);
        return (int)hipGetLastError();
    });
}
