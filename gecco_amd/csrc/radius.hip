// Fixed-radius neighbour search between 3-D clouds on the device (gfx950): for every query q_i of (B, M, 3) EVERY point of the reference
// cloud (B, N, 3) of the same batch element within r of it.  The second neighbourhood query of Open3D and PCL beside knn.hip's
// (search_radius_vector_3d, search_hybrid_vector_3d, remove_radius_outlier / RadiusOutlierRemoval, PointNet++'s ball_query).  The
// reference has no neighbourhood query at all; the route without this file is a materialised M x N distance matrix (cdist <= r: 40 GB
// at 100 000 points against themselves), nonzero over it, and aa + bb - 2ab roundings that put pairs at the bound on the wrong side.
//
// Definition (gecco_radius_count_f32 / gecco_radius_search_f32, include/gecco_hip.h; tests/_radius_ref.py restates it in numpy float32).
// With r2 = fp32(r * r) from the host (cluster_dbscan's eps2): dist2(q, p) is cloud_dist2_inf of cloud_nn.h ((dx dx + dy dy) + dz dz,
// every operation rounded to fp32, none contracted, NaN -> +inf); j is a neighbour of i when dist2(q_i, p_j) <= r2, inclusive, compared
// on the bits as unsigned integers (dist2 >= 0 or +inf).  A non-finite query has dist2 = +inf to everything and no neighbours, a
// non-finite reference point is nobody's neighbour.  Self mode skips the pair j == i by index, not by distance.  count_i = the number
// of neighbours, never clamped; a row lists its neighbours in ascending j.
//
// One scan kernel, three modes.
//   COUNT       count[b, i]
//   FILL_CSR    given row_start[b * M + i], the exclusive prefix sum of the counts over every row of the batch (int64: the total can
//               pass 2^31), neighbour t of row r goes to idx[row_start[r] + t] (and its dist2 to d2[...]).  The row is recounted by the
//               same predicate on the same bits, so exactly count[r] entries are written and no row reaches into the next
//   FILL_FIXED  the first K neighbours of row r go to idx[r, 0 .. K), the rest of the K slots are padded with -1 (d2: +inf), and the
//               unclamped count comes out of the same pass: one launch, no host synchronisation
// A thread owns one query and writes its own words only: no atomics, no workspace, no thread reads what another thread of the launch
// writes, so the outputs are the same bits run to run and in any batch position.  The row stores of the two fill modes are scattered by
// construction (each thread walks its own segment); they are direct stores, DESIGN.md says what that costs.
//
// The scan is the loop of knn_scan_kernel / dbscan_scan_kernel (cloud_nn.h says why it is written out per kernel rather than shared):
// the cloud streamed through LDS in tiles of CLOUD_TILE as (x, y, z, 0), the next tile prefetched into registers, four candidates per
// step behind one branch, and inside the branch the four singly in order, which is what makes a row ascend in j.  Only the direct form
// exists: few queries against many points leave compute units idle (2048 queries are 32 workgroups), a split form is the follow-up.
#include "cloud_nn.h"
#include "kernels.h"
#include "launch_state.h"

namespace {

enum { RADIUS_COUNT = 0, RADIUS_FILL_CSR = 1, RADIUS_FILL_FIXED = 2 };

// grid: B * tiles blocks of T queries.  COUNT: count.  FILL_CSR: row_start, idx, d2 (nullable).  FILL_FIXED: idx, d2 (nullable), count
// (nullable), K slots per row
template <int T, int MODE>
__global__ __launch_bounds__(T) void radius_scan_kernel(const float* __restrict__ query, const float* __restrict__ ref,
                                                        const long long* __restrict__ row_start, int* __restrict__ idx, float* __restrict__ d2,
                                                        int* __restrict__ count, unsigned r2_bits, int M, int N, int exclude_self, int tiles,
                                                        int K) {
    __shared__ __attribute__((aligned(16))) f32x4 tile[CLOUD_TILE];

    const int tid = threadIdx.x;
    const int qt = (int)(blockIdx.x % (unsigned)tiles), b = (int)(blockIdx.x / (unsigned)tiles);
    const float* rb = ref + (size_t)b * N * 3;
    const unsigned hi = (unsigned)N;
    const int i = qt * T + tid;
    const bool valid = i < M;
    const size_t row = (size_t)b * M + (valid ? i : 0);
    const float* qp = query + row * 3;
    const float qx = qp[0], qy = qp[1], qz = qp[2];
    const unsigned self = exclude_self ? (unsigned)i : 0xffffffffu;   // no j reaches 2^32 - 1
    // where this row's entries go: its segment of the CSR arrays, or its K slots
    const size_t o = MODE == RADIUS_FILL_CSR ? (size_t)row_start[row] : MODE == RADIUS_FILL_FIXED ? row * (size_t)K : 0;
    int n = 0;   // neighbours so far (n <= N)

    constexpr int PPT = CLOUD_TILE / T;
    float rx[PPT], ry[PPT], rz[PPT];
    auto fetch = [&](unsigned base) {
#pragma unroll
        for (int p = 0; p < PPT; ++p) {
            const unsigned j = base + (unsigned)(tid + p * T);
            const bool in = j < hi;
            rx[p] = in ? rb[3 * (size_t)j] : 0.f;
            ry[p] = in ? rb[3 * (size_t)j + 1] : 0.f;
            rz[p] = in ? rb[3 * (size_t)j + 2] : 0.f;
        }
    };
    auto single = [&](unsigned u, unsigned j) {
        if (u <= r2_bits && j != self) {
            if (MODE == RADIUS_FILL_CSR || (MODE == RADIUS_FILL_FIXED && n < K)) {
                idx[o + (size_t)n] = (int)j;
                if (d2) d2[o + (size_t)n] = __uint_as_float(u);
            }
            ++n;
        }
    };

    fetch(0);
    for (unsigned base = 0; base < hi; base += CLOUD_TILE) {
        __syncthreads();   // the scan of the previous tile is over
#pragma unroll
        for (int p = 0; p < PPT; ++p) tile[tid + p * T] = f32x4{rx[p], ry[p], rz[p], 0.f};
        __syncthreads();
        if (base + CLOUD_TILE < hi) fetch(base + CLOUD_TILE);
        if (!valid) continue;
        const int cnt = (int)min((unsigned)CLOUD_TILE, hi - base);   // entries past cnt are never candidates
        int g = 0;
        for (; g + 4 <= cnt; g += 4) {
            const unsigned u0 = cloud_dist2_bits(qx, qy, qz, tile[g]), u1 = cloud_dist2_bits(qx, qy, qz, tile[g + 1]);
            const unsigned u2 = cloud_dist2_bits(qx, qy, qz, tile[g + 2]), u3 = cloud_dist2_bits(qx, qy, qz, tile[g + 3]);
            if (min(min(u0, u1), min(u2, u3)) <= r2_bits) {   // dist2 >= 0 or +inf: its bits order as unsigned integers
                single(u0, base + g);                          // ascending j inside the step
                single(u1, base + g + 1);
                single(u2, base + g + 2);
                single(u3, base + g + 3);
            }
        }
        for (; g < cnt; ++g) single(cloud_dist2_bits(qx, qy, qz, tile[g]), base + g);
    }
    if (!valid) return;
    if (MODE == RADIUS_FILL_FIXED)
        for (int t = min(n, K); t < K; ++t) {
            idx[o + (size_t)t] = -1;
            if (d2) d2[o + (size_t)t] = __builtin_inff();
        }
    if (MODE != RADIUS_FILL_CSR && count) count[row] = n;
}

}  // namespace

// One launch.  idx null: COUNT (count required).  row_start given: FILL_CSR (K == 0; count is not written).  Otherwise FILL_FIXED with K >= 1
// slots per row (count nullable).  d2 nullable in both fill modes.  Returns -2 for arguments out of range, -3 when the grid would pass
// 2^31 - 1 workgroups.
int radius_launch(const float* query, const float* ref, const long long* row_start, int* idx, float* d2, int* count, int B, int M, int N,
                  float r2, int exclude_self, int K, hipStream_t st) {
    if (!query || !ref || B < 1 || M < 1 || N < 1 || !(r2 > 0.f) || !(r2 <= 3.402823466e38f) || (exclude_self && M != N)) return -2;
    if (idx ? (row_start != nullptr) == (K != 0) || K < 0 : !count || row_start || d2 || K != 0) return -2;
    const CloudPlan p = cloud_plan(B, M, N, 1, false, 256, device_cus());
    if (!p.fits()) return -3;
    const unsigned r2_bits = __builtin_bit_cast(unsigned, r2);
    const int self = exclude_self ? 1 : 0;
    return dispatch_T(p.T, [&](auto t) -> int {
        constexpr int T = decltype(t)::value;
        const dim3 grid((unsigned)p.blocks), block(T);
        if (!idx)
            hipLaunchKernelGGL((radius_scan_kernel<T, RADIUS_COUNT>), grid, block, 0, st, query, ref, row_start, idx, d2, count, r2_bits, M, N, self,
                               p.tiles, 0);
        else if (row_start)
            hipLaunchKernelGGL((radius_scan_kernel<T, RADIUS_FILL_CSR>), grid, block, 0, st, query, ref, row_start, idx, d2, count, r2_bits, M, N,
                               self, p.tiles, 0);
        else
            hipLaunchKernelGGL((radius_scan_kernel<T, RADIUS_FILL_FIXED>), grid, block, 0, st, query, ref, row_start, idx, d2, count, r2_bits, M,
                               N, self, p.tiles, K);
        return (int)hipGetLastError();
    });
}
