// What the neighbour family of the point-cloud kernels shares (fps.hip, knn.hip, normals.hip, icp.hip): the squared distance whose
// roundings define four public operators, the tile size of the brute-force scans, the launch plan of the direct and split forms, and
// the finite-triple predicate.  Device code is static __device__ __forceinline__, host helpers are inline.
#pragma once
#include <type_traits>

#include "../../include/gecco_hip.h"
#include "common.h"

// dist2(a, b) = (dx dx + dy dy) + dz dz on the coordinate differences, every operation rounded to fp32 and none contracted into an FMA:
// near-ties between candidates are closer than an FMA's rounding, so the roundings are part of the operators' definitions (pair_dist.h
// spells out the reference's aa + bb - 2ab form for the same reason).  A NaN stays a NaN here; fps_min relies on it.
static __device__ __forceinline__ float cloud_dist2(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}
// the searches' form: a NaN dist2 becomes +inf (minNum), so dist2 >= 0 or +inf and its bits order as unsigned integers
static __device__ __forceinline__ float cloud_dist2_inf(float qx, float qy, float qz, float px, float py, float pz) {
    return __builtin_fminf(cloud_dist2(qx, qy, qz, px, py, pz), __builtin_inff());
}
static __device__ __forceinline__ unsigned cloud_dist2_bits(float qx, float qy, float qz, const f32x4 p) {
    return __float_as_uint(cloud_dist2_inf(qx, qy, qz, p[0], p[1], p[2]));
}

static __device__ __forceinline__ bool cloud_finite3(float x, float y, float z) {
    return fabsf(x) <= 3.402823466e38f && fabsf(y) <= 3.402823466e38f && fabsf(z) <= 3.402823466e38f;   // false for NaN and inf
}

constexpr int CLOUD_TILE = 512;   // points of the reference cloud per LDS tile of a scan
static_assert(GECCO_KNN_SPLIT_SLICE % CLOUD_TILE == 0, "a slice is a whole number of tiles");

// The scan loop itself is written out in knn_scan_kernel and again in icp_match_kernel, on purpose.  As one template over the workgroup
// size with bound() / take(u, j) lambdas it compiled to the same registers, LDS and scratch and to 0 / +1 instructions, but with
// compares and one branch ordered differently, and three alternating runs of tools/bench_knn.py and tools/bench_icp.py on one MI355X
// put it outside the spread of the written-out loops' own runs at 100 000 points against themselves: kNN direct 8.260 -> 8.339 ms
// (spread 0.022), split 15.596 -> 15.639 (0.040); ICP, eleven passes, direct 40.90 -> 41.52 (0.09), one pass 3.723 -> 3.766 (0.013);
// at 2048 points against 100 000 the ICP match was 4.6 % faster (3.613 -> 3.450).  The two loops differ only in what a winning
// candidate does: change them together.

// The launch geometry of a kernel with one thread per query: the form, S slices of the reference cloud (1 in the direct form, and in
// the split form of a cloud of one slice), T threads per workgroup, tiles = ceil(M / T) workgroups per cloud and slice, blocks = the grid.
struct CloudPlan {
    bool split;
    int S, T, tiles;
    long long blocks;
    bool fits() const { return blocks <= 0x7fffffffLL; }   // a grid holds at most 2^31 - 1 workgroups
};

// the most threads whose per-query LDS of k entries stays within a workgroup's share
inline int cloud_max_threads(int k) { return k <= 16 ? 256 : k <= 32 ? 128 : 64; }

// form 0: split when the caller can take it (`can_split`: a workspace is there), N spans more than one slice and the direct grid at its
// smallest workgroup (64 queries) leaves CUs idle; 1: direct; 2: split.  T starts at max_T and is halved while the grid would leave the
// device short of two workgroups per CU.
inline CloudPlan cloud_plan(int B, int M, int N, int form, bool can_split, int max_T, int cus) {
    const int slices = (int)(((long long)N + GECCO_KNN_SPLIT_SLICE - 1) / GECCO_KNN_SPLIT_SLICE);
    CloudPlan p;
    p.split = form == 2 || (form == 0 && can_split && slices > 1 && (long long)B * ((M + 63) / 64) < cus);
    p.S = p.split ? slices : 1;
    p.T = max_T;
    while (p.T > 64 && (long long)B * p.S * ((M + p.T - 1) / p.T) < 2LL * cus) p.T >>= 1;
    p.tiles = (M + p.T - 1) / p.T;
    p.blocks = (long long)B * p.tiles * p.S;
    return p;
}

// f(std::integral_constant<int, T>) for T = 256, 128 or 64 (anything else: 64): a launcher names its instantiations once
template <class F>
inline auto dispatch_T(int T, F f) {
    if (T == 256) return f(std::integral_constant<int, 256>{});
    if (T == 128) return f(std::integral_constant<int, 128>{});
    return f(std::integral_constant<int, 64>{});
}
