// Normals and curvature from radius neighbourhoods on the grid index of grid.hip (gfx950): Open3D's estimate_normals(
// KDTreeSearchParamRadius(r)), PCL's NormalEstimation::setRadiusSearch.  The neighbourhood is every point within r, unbounded, the ball
// the grid index serves; normals.hip's k-neighbourhoods come from the brute-force knn and stop at GECCO_KNN_MAX_K.  Nothing here writes a
// neighbour list: a thread walks the cells its ball can reach, pools the moments in registers and keeps the eigenvector iss.hip drops.
//
// Definition (gecco_normals_grid_f32, include/gecco_hip.h; tests/_normals_grid_ref.py restates it in numpy).  Per cloud, with r2 =
// fp32(radius^2) from the caller:
//   queries    q_i: the points of the cloud themselves or other positions.  A point of the cloud is in its own ball because its dist2
//              is 0: nothing is excluded by index
//   ball       the j with cloud_dist2_bits(q_i, p_j) <= r2 bits (radius.hip's predicate), visited in ascending sorted position of the
//              index, the off-grid tail last (grid_walk's order, part of the definition as it is for ISS).  A non-finite query has an
//              empty ball, a non-finite point is in nobody's ball
//   count      m_i = the size of the ball, never clamped
//   moments,   the `moments` and `eigen` steps of gecco_iss_keypoints_f32, by the code iss.hip runs (sym3_jacobi.h): fp64 sums of d =
//   eigen      double(p_j) - double(q_i) in ball order, C = S2 / m - mu mu^T, big = max |C_ab|, A = C / big, eight cyclic Jacobi sweeps with
//              the guarded rotation, nothing contracted, lambda = diag big clamped at 0; the rotations accumulated into V from the identity
//   order      the three (lambda, column) pairs ascending by ISS's three compare-exchanges; a pair moves only when strictly smaller
//   normal     the column of lambda0 divided by its fp64 norm sqrt((xx + yy) + zz), each component rounded once to fp32
//   sign       after the rounding.  With a viewpoint v: flip when (n_x d_x + n_y d_y) + n_z d_z < 0 in fp64, d = double(v) - double(q_i)
//              (a NaN does not flip).  Without: the fp32 component of largest magnitude is positive, the lowest axis among equal
//              magnitudes (normals.hip's rule)
//   curvature  lambda0 / ((lambda0 + lambda1) + lambda2) in fp64, 0 where that sum is not > 0
//   invalid    m_i < min_neighbors, a non-finite query, big not a positive finite number (all of the ball identical): normal (0, 0, 1)
//              as in Open3D, eigenvalues 0, curvature 0, count still m_i.  A collinear ball is valid: some unit vector of the numerical
//              null space
// A row depends on the cloud, the query and the index's cell_size and origin, which fix the order of the sums, and on nothing else: the
// same bits run to run, in any batch position and at any workgroup size.
//
// One launch, one thread per query: thread t of a cloud answers query qorder[t] (null: query t) and writes that query's row,
// grid_query_kernel's convention, so that the lanes of a wave probe the same cells.  The thread reads the query's 12 bytes, calls
// grid_walk (grid_walk.h: proved there to miss no neighbour, every loop bounded) with a visitor that adds the count and the nine fp64
// sums in registers, solves the eigenproblem with sym3_eigen<true> (A and V are named scalars: nothing in scratch) and writes its own
// words only.  No atomics, no LDS, no workspace, no thread waits on another.
#include <cmath>

#include "cloud_nn.h"
#include "grid_walk.h"
#include "kernels.h"
#include "launch_state.h"
#include "sym3_jacobi.h"
#include "voxel_cell.h"

namespace {

// grid: B * tiles blocks of T queries.  viewpoint (B, 3), eigenvalues, curvature, counts nullable
template <int T>
__global__ __launch_bounds__(T) void normals_grid_kernel(const float* __restrict__ query, const int* __restrict__ qorder, const GridView index,
                                                         const float* __restrict__ viewpoint, float R, unsigned r2_bits, int min_neighbors,
                                                         float* __restrict__ normals, double* __restrict__ eigenvalues,
                                                         double* __restrict__ curvature, int* __restrict__ counts, int M, int tiles) {
#pragma clang fp contract(off)
    const int b = (int)(blockIdx.x / (unsigned)tiles);
    const int t = (int)(blockIdx.x % (unsigned)tiles) * T + (int)threadIdx.x;
    if (t >= M) return;   // (no barrier below)
    const int i = qorder ? qorder[(size_t)b * M + t] : t;
    if ((unsigned)i >= (unsigned)M) return;   // a qorder that is no permutation writes nothing outside the outputs
    const size_t row = (size_t)b * M + i;
    const float qx = query[row * 3], qy = query[row * 3 + 1], qz = query[row * 3 + 2];
    const double cx = (double)qx, cy = (double)qy, cz = (double)qz;
    Sym3Moments sums;   // the count and the nine fp64 sums, in registers
    if (cloud_finite3(qx, qy, qz))   // (a non-finite query has dist2 = +inf to everything)
        grid_walk(index, b, qx, qy, qz, R, r2_bits, [&](const f32x4 p, unsigned) {
            sums.add((double)p[0] - cx, (double)p[1] - cy, (double)p[2] - cz);
        });
    const int m = sums.m;
    float nx = 0.f, ny = 0.f, nz = 1.f;
    double l0 = 0.0, l1 = 0.0, l2 = 0.0, curv = 0.0;
    if (m >= min_neighbors) {   // (m >= 1: the query is finite)
        const Sym3Eigen e = sym3_eigen<true>(sums);
        if (e.solved) {
            l0 = e.l0, l1 = e.l1, l2 = e.l2;
            const double norm = sqrt((e.x * e.x + e.y * e.y) + e.z * e.z);
            nx = (float)(e.x / norm), ny = (float)(e.y / norm), nz = (float)(e.z / norm);
            const double sum = (l0 + l1) + l2;
            if (sum > 0.0) curv = l0 / sum;
            bool flip;
            if (viewpoint) {
                const float* v = viewpoint + 3 * (size_t)b;
                const double dx = (double)v[0] - cx, dy = (double)v[1] - cy, dz = (double)v[2] - cz;
                flip = ((double)nx * dx + (double)ny * dy) + (double)nz * dz < 0.0;
            } else {
                const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
                const float lead = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);   // the lowest axis among equal magnitudes
                flip = lead < 0.f;
            }
            if (flip) nx = -nx, ny = -ny, nz = -nz;
        }
    }
    normals[row * 3] = nx, normals[row * 3 + 1] = ny, normals[row * 3 + 2] = nz;
    if (eigenvalues) eigenvalues[row * 3] = l0, eigenvalues[row * 3 + 1] = l1, eigenvalues[row * 3 + 2] = l2;
    if (curvature) curvature[row] = curv;
    if (counts) counts[row] = m;
}

}  // namespace

// One launch.  qorder, viewpoint, eigenvalues, curvature, counts nullable.  -2: arguments out of range (a radius2 above
// fp32(cell_size^2) among them), -3: the grid would pass 2^31 - 1 workgroups
int normals_grid_launch(const float* query, const int* qorder, const GridIndexArgs& index, const float* viewpoint, float r2, int min_neighbors,
                        float* normals, double* eigenvalues, double* curvature, int* counts, int B, int M, int N, hipStream_t st) {
    const GridView g = grid_view(index, B, N);
    if (!g.sorted || !query || !normals || M < 1) return -2;
    if (!grid_radius2_ok(r2, index.cell_size) || min_neighbors < 1) return -2;
    const CloudPlan p = cloud_plan(B, M, N, 1, false, 256, device_cus());
    if (!p.fits()) return -3;
    return dispatch_T(p.T, [&](auto t) -> int {
        constexpr int T = decltype(t)::value;
        hipLaunchKernelGGL((normals_grid_kernel<T>), dim3((unsigned)p.blocks), dim3(T), 0, st, query, qorder, g, viewpoint, grid_reach(r2),
                           __builtin_bit_cast(unsigned, r2), min_neighbors, normals, eigenvalues, curvature, counts, M, p.tiles);
        return (int)hipGetLastError();
    });
}
