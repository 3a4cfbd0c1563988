// ISS keypoints (Intrinsic Shape Signatures, Zhong 2009; Open3D's compute_iss_keypoints, PCL's ISSKeypoint3D) on the grid index of
// grid.hip (gfx950): the points whose neighbourhood is not flat, not a line and not isotropic, thinned by non-maximum suppression.  Both
// steps pool over "every point within a radius", the unbounded neighbourhood the grid index serves; nothing here writes a neighbour
// list: a thread walks the cells its ball can reach and accumulates in registers.
//
// Definition (gecco_iss_keypoints_f32, include/gecco_hip.h; tests/_iss_ref.py restates it in numpy).  Per cloud, with r2s =
// fp32(salient_radius^2) and r2n = fp32(non_max_radius^2) from the caller:
//   ball       B_r(i) = the j with cloud_dist2_bits(p_i, p_j) <= r2 bits: radius.hip's predicate, the point itself INCLUDED by index
//              (Open3D's radius search returns the query).  A non-finite point is in nobody's ball, not even its own.  The ball is
//              visited in ascending sorted position of the index (by (cell key, j), the off-grid tail last): grid.hip's scan order,
//              and part of the definition as it is of the grid-ordered rows there
//   count      m_i = |B_r2s(i)|
//   moments    in fp64 on the fp32 coordinates, about the point itself, every operation rounded and none contracted:
//              d = double(p_j) - double(p_i) per axis;  S1 = sum d (3 sums), S2 = sum d d^T (xx, xy, xz, yy, yz, zz), each from 0 in
//              ball order;  inv = 1 / m;  mu = S1 inv;  C_ab = S2_ab inv - mu_a mu_b.  |d| <= the radius, so the raw moments cancel
//              against the radius and not against the cloud's distance from the origin
//   eigen      big = max |C_ab|;  A = C sc with sc = 1 / big;  SYM3_JACOBI_SWEEPS = 8 cyclic Jacobi sweeps over (0,1), (0,2), (1,2) with
//              the guarded rotation of rigid_fit.h (icp_rotate: a non-finite theta gives t = 0, a theta whose square would overflow
//              t = 1 / (2 theta)), a fixed count;  lambda = diag big, negative roundings clamped to 0, sorted lambda0 <= lambda1 <= lambda2
//   candidate  m_i >= min_neighbors, big a positive finite number (all of the ball identical: not a candidate, Open3D's
//              cov.isZero()), lambda1 < gamma_21 lambda2, lambda0 < gamma_32 lambda1 (fp64 products, no division) and lambda0 > 0.
//              saliency_i = lambda0 for a candidate, 0 otherwise;  eigenvalues_i = 0 where m_i < min_neighbors or big is not a
//              positive finite number
//   keypoint   i is a candidate, |B_r2n(i)| >= min_neighbors, and no j in B_r2n(i) has saliency_j > saliency_i (fp64 compare).  Equal
//              saliencies keep each other, as Open3D's IsLocalMaxima does: two exact duplicates of a keypoint are both kept
// A point's result depends on the cloud and on the index's cell_size and origin, which fix the order of the sums, and on nothing else:
// the same bits run to run, in any batch position and at any workgroup size.  Two indices with different cells may differ in the last
// bits of the eigenvalues (another order of the same sums); counts do not.
//
// Two launches, one thread per SORTED POSITION in both: thread t of a cloud owns the point at sorted[t], whose 16-byte load gives the
// coordinates and, in .w, the original index i its outputs go to.  The lanes of a wave are neighbours in the sorted order, so they
// probe the same cells and read the same runs.  iss_saliency_kernel walks the box of r2s, adds the count and the nine fp64 sums in
// registers, solves the 3 x 3 problem in registers (sym3_jacobi.h's sym3_eigen, the eigenvalues-only form of the solve that
// normals_grid.hip shares: the matrix and the rotations are scalars, no indexed local array, no scratch) and writes saliency,
// eigenvalues and counts at i.  iss_select_kernel starts from saliency[i] > 0 (other threads write false and return), walks the box of
// r2n, counts the ball and compares saliency[j], a gather by the index carried in .w, and writes the mask byte.  A thread writes its own
// words only: no atomics, no LDS, no workspace, no thread waits on another, every loop is bounded by a constant, by cap or by N.
//
// The walk (the reach, the clamped cells, the table probe, the runs, the tail, the scan of all N positions for a wide box) is grid_walk of
// grid_walk.h, the one grid_query_kernel calls, where it is proved to miss no neighbour and every loop is bounded.  The index comes in as
// one GridIndexArgs (kernels.h); both kernels take the GridView that grid_walk.h's grid_view makes of it, by value.
#include <cmath>

#include "cloud_nn.h"
#include "grid_walk.h"
#include "kernels.h"
#include "launch_state.h"
#include "sym3_jacobi.h"
#include "voxel_cell.h"

namespace {

// grid: B * tiles blocks of T sorted positions.  eigenvalues, counts nullable
template <int T>
__global__ __launch_bounds__(T) void iss_saliency_kernel(const GridView index, float R, unsigned r2_bits, double gamma_21, double gamma_32,
                                                         int min_neighbors, double* __restrict__ saliency, double* __restrict__ eigenvalues,
                                                         int* __restrict__ counts, int tiles) {
#pragma clang fp contract(off)
    const int N = index.N;
    const int b = (int)(blockIdx.x / (unsigned)tiles);
    const int t = (int)(blockIdx.x % (unsigned)tiles) * T + (int)threadIdx.x;
    if (t >= N) return;   // (no barrier below)
    const f32x4 own = index.cloud(b)[t];
    const unsigned i = __float_as_uint(own[3]);
    if (i >= (unsigned)N) return;   // a sorted array no build wrote: nothing outside the outputs is written
    const float qx = own[0], qy = own[1], qz = own[2];
    const double cx = (double)qx, cy = (double)qy, cz = (double)qz;
    Sym3Moments sums;   // the count and the nine fp64 sums, in registers
    if (cloud_finite3(qx, qy, qz))   // (a non-finite point has dist2 = +inf to everything)
        grid_walk(index, b, qx, qy, qz, R, r2_bits, [&](const f32x4 p, unsigned) {
            sums.add((double)p[0] - cx, (double)p[1] - cy, (double)p[2] - cz);
        });
    const int m = sums.m;
    double l0 = 0.0, l1 = 0.0, l2 = 0.0, sal = 0.0;
    if (m >= min_neighbors) {
        const Sym3Eigen e = sym3_eigen<false>(sums);   // (0 where big is no positive finite number)
        l0 = e.l0, l1 = e.l1, l2 = e.l2;
        if (e.solved && l1 < gamma_21 * l2 && l0 < gamma_32 * l1 && l0 > 0.0) sal = l0;
    }
    const size_t row = (size_t)b * N + i;
    saliency[row] = sal;
    if (eigenvalues) eigenvalues[row * 3] = l0, eigenvalues[row * 3 + 1] = l1, eigenvalues[row * 3 + 2] = l2;
    if (counts) counts[row] = m;
}

// grid: B * tiles blocks of T sorted positions
template <int T>
__global__ __launch_bounds__(T) void iss_select_kernel(const GridView index, float R, unsigned r2_bits, int min_neighbors,
                                                       const double* __restrict__ saliency, unsigned char* __restrict__ mask, int tiles) {
    const int N = index.N;
    const int b = (int)(blockIdx.x / (unsigned)tiles);
    const int t = (int)(blockIdx.x % (unsigned)tiles) * T + (int)threadIdx.x;
    if (t >= N) return;   // (no barrier below)
    const f32x4 own = index.cloud(b)[t];
    const unsigned i = __float_as_uint(own[3]);
    if (i >= (unsigned)N) return;
    const double* sal = saliency + (size_t)b * N;
    const double mine = sal[i];
    bool keep = false;
    if (mine > 0.0) {   // a candidate: its point is finite
        int n = 0;
        bool beaten = false;
        grid_walk(index, b, own[0], own[1], own[2], R, r2_bits, [&](const f32x4 p, unsigned) {
            const unsigned j = __float_as_uint(p[3]);
            ++n;
            beaten = beaten || (j < (unsigned)N && sal[j] > mine);
        });
        keep = n >= min_neighbors && !beaten;
    }
    mask[(size_t)b * N + i] = keep ? 1 : 0;
}

}  // namespace

// Two launches: the saliency of every point, then the selection.  eigenvalues, counts nullable.  -2: arguments out of range (a radius2
// above fp32(cell_size^2) among them), -3: the grid would pass 2^31 - 1 workgroups
int iss_launch(const GridIndexArgs& index, double* saliency, double* eigenvalues, int* counts, unsigned char* mask, int B, int N, float r2s,
               float r2n, double gamma_21, double gamma_32, int min_neighbors, hipStream_t st) {
    const GridView g = grid_view(index, B, N);
    if (!g.sorted || !saliency || !mask) return -2;
    if (!grid_radius2_ok(r2s, index.cell_size) || !grid_radius2_ok(r2n, index.cell_size) || min_neighbors < 1) return -2;
    if (!(gamma_21 > 0.0) || !(gamma_21 <= 1.7976931348623157e308) || !(gamma_32 > 0.0) || !(gamma_32 <= 1.7976931348623157e308)) return -2;
    const CloudPlan p = cloud_plan(B, N, N, 1, false, 256, device_cus());
    if (!p.fits()) return -3;
    return dispatch_T(p.T, [&](auto t) -> int {
        constexpr int T = decltype(t)::value;
        const dim3 grid((unsigned)p.blocks), block(T);
        hipLaunchKernelGGL((iss_saliency_kernel<T>), grid, block, 0, st, g, grid_reach(r2s), __builtin_bit_cast(unsigned, r2s), gamma_21,
                           gamma_32, min_neighbors, saliency, eigenvalues, counts, p.tiles);
        hipLaunchKernelGGL((iss_select_kernel<T>), grid, block, 0, st, g, grid_reach(r2n), __builtin_bit_cast(unsigned, r2n), min_neighbors,
                           saliency, mask, p.tiles);
        return (int)hipGetLastError();
    });
}
