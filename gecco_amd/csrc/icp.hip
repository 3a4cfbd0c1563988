// Rigid registration of 3-D clouds by ICP on the device (gfx950), point-to-point and point-to-plane: the consumer PCL and Open3D put
// behind the neighbour search and the normals.  The reference has nothing of the kind; the route without this file is knn(k = 1) ->
// knn_gather -> torch.linalg.svd in a host loop with one synchronisation per iteration, and no point-to-plane form at all.
//
// Definition (gecco_icp_f32, include/gecco_hip.h, follows Open3D's registration_icp; tests/_icp_ref.py restates it in numpy).  Per
// cloud the state T is a 4 x 4 fp64 matrix starting at init, r2 = fp32(r * r) and the anchor c = double(target[0]).  Pass i = 0, 1, ...:
//   1 transform  Tf = fp32(T); p' = ((Tf[a][0] x + Tf[a][1] y) + Tf[a][2] z) + Tf[a][3] per axis a, every operation rounded to fp32,
//                none contracted (icp_transform)
//   2 match      (d2, j) = the first pair of the k = 1 search of p' in the target: cloud_nn.h's dist2 spelling, NaN -> +inf, equal
//                distances to the lowest index.  Inlier: d2 <= r2 and d2 < +inf (plane method: the three components of n_j finite as well)
//   3 measure    n inliers; fitness = n / M; rmse = sqrt(sum d2 / n) with the sum in fp64, 0 when n = 0
//   4 stop       at the first that holds: status 3, init has a non-finite entry (pass 0 only); status 0, i >= 1 and |fitness_i -
//                fitness_{i-1}| < relative_fitness and |rmse_i - rmse_{i-1}| < relative_rmse; status 1, i == max_iterations; status 2,
//                n < 3 (point) / n < 6 (plane) or a singular system.  T stays; the outputs are this pass's, iterations = i
//   5 update     T <- dT * double(Tf).  Point: Horn's quaternion from the fp64 moments about c of the inlier pairs, the largest
//                eigenvector of his 4 x 4 matrix by ICP_JACOBI_SWEEPS cyclic Jacobi sweeps.  Plane: the 6 x 6 normal equations of the
//                linearised residuals about c by LDL^T without pivoting, singular when a pivot is non-finite or <= 2^-36 max diag(A)
//
// Two launches per pass and nothing else: 2 * (max_iterations + 1) launches whatever the data, no atomics, no workgroup waits on
// another, no host synchronisation, so the call can be captured in a graph.  A stopped cloud's workgroups return at once.
//
// icp_match_kernel<T>: grid (cloud, tile of T source points, slice of the target), one thread per source point.  It reads its cloud's T
// (pass 0: from init, later: from the state in the workspace), transforms its point on load, and walks the slice through LDS tiles the
// way knn_scan_kernel does (the same loop; cloud_nn.h says why it is written out in both): (x, y, z, 0) entries, broadcast reads, four
// candidates per step, the next tile fetched while this one is scanned.  ONE 64-bit key (dist2's bits above j) lives in a register;
// there is no LDS list.  keys[(b * S + s) * M + m] gets it.  The minimum over a point's S slice keys is exact, so the direct (S = 1)
// and split forms give the same bits.
//
// icp_update_kernel<PLANE>: one workgroup of ICP_UPDATE_THREADS per cloud.  Thread t takes points t, t + T, ...: the minimum of the S
// keys, the gather of q (and n), the correspondence, and its fp64 sums (17 numbers for the point method, 29 for the plane method).  The
// sums are reduced inside the wave by a fixed shuffle tree and across the waves through LDS by thread 0 in wave order; thread 0 then
// runs steps 3 - 5 and writes the state and, on a stop, the outputs.  The geometry of this kernel never depends on the batch or the
// form, so a cloud's bits are the same run to run, in any batch position and in both forms.
#include "cloud_nn.h"
#include "kernels.h"
#include "launch_state.h"
#include "rigid_fit.h"

namespace {

typedef unsigned long long icp_key;
constexpr int ICP_UPDATE_THREADS = 512;
constexpr int ICP_STATE_DOUBLES = GECCO_ICP_STATE_BYTES / 8;   // T (16), fitness and rmse of the previous pass, the stopped flag
static_assert(ICP_STATE_DOUBLES >= 19, "the state of a cloud");

__device__ const double icp_identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

// where pass `pass` finds the T of cloud b: init (or the identity) before the first update, the state after it
static __device__ __forceinline__ const double* icp_T(const double* init, const double* state, int b, int pass) {
    if (pass > 0) return state + (size_t)b * ICP_STATE_DOUBLES;
    return init ? init + (size_t)b * 16 : icp_identity;
}

// grid: B * tiles * S blocks, block (b, tile, s) scans target points [s * slice, min(N, (s + 1) * slice)) for source points tile * T ..
template <int T>
__global__ __launch_bounds__(T) void icp_match_kernel(const float* __restrict__ source, const float* __restrict__ target,
                                                      const double* __restrict__ init, const double* __restrict__ state,
                                                      icp_key* __restrict__ keys, int pass, int M, int N, int tiles, int S, unsigned slice) {
    __shared__ __attribute__((aligned(16))) f32x4 tile[CLOUD_TILE];

    const int tid = threadIdx.x;
    const unsigned bid = blockIdx.x;
    const int s = (int)(bid % (unsigned)S), qt = (int)((bid / (unsigned)S) % (unsigned)tiles), b = (int)(bid / (unsigned)S / (unsigned)tiles);
    if (pass > 0 && state[(size_t)b * ICP_STATE_DOUBLES + 18] != 0.0) return;   // the cloud has stopped (uniform: no barrier is left behind)
    const unsigned lo = (unsigned)s * slice, hi = min((unsigned)N, lo + slice);
    const float* rb = target + (size_t)b * N * 3;
    const int i = qt * T + tid;
    const bool valid = i < M;

    float tf[12];
    {
        const double* Td = icp_T(init, state, b, pass);
#pragma unroll
        for (int e = 0; e < 12; ++e) tf[e] = (float)Td[e];
    }
    const float* sp = source + ((size_t)b * M + (valid ? i : 0)) * 3;
    float qx, qy, qz;
    icp_transform(tf, sp[0], sp[1], sp[2], qx, qy, qz);

    unsigned best_bits = 0xffffffffu, best_j = 0xffffffffu;   // above every key: dist2's bits are at most +inf's

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
    // j ascends in a scan, so an equal dist2 has the higher index and loses: the compare is on dist2's bits alone
    auto single = [&](unsigned u, unsigned j) {
        if (u < best_bits) {
            best_bits = u;
            best_j = j;
        }
    };

    fetch(lo);
    for (unsigned base = lo; base < hi; base += CLOUD_TILE) {
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
            if (min(min(u0, u1), min(u2, u3)) < best_bits) {   // ascending j inside the step
                single(u0, base + g);
                single(u1, base + g + 1);
                single(u2, base + g + 2);
                single(u3, base + g + 3);
            }
        }
        for (; g < cnt; ++g) single(cloud_dist2_bits(qx, qy, qz, tile[g]), base + g);
    }
    if (!valid) return;
    keys[((size_t)b * S + s) * (size_t)M + i] = ((icp_key)best_bits << 32) | (icp_key)best_j;   // a slice holds a point: best_j < N
}

// Point-to-plane step from the reduced sums: acc[2 + tri(r, e)] = A[r][e] for r <= e (21 numbers, rows first), acc[23 + r] = g[r].
// False when the system is singular.
static __device__ __noinline__ bool icp_solve_plane(const double* acc, const double* c, double* dT) {
    double L[6][6], d[6], x[6];
    double A[6][6];
    int o = 2;
    for (int r = 0; r < 6; ++r)
        for (int e = r; e < 6; ++e) A[r][e] = A[e][r] = acc[o++];
    double top = 0.0;
    for (int r = 0; r < 6; ++r) top = fmax(top, A[r][r]);
    const double floor_ = 0x1p-36 * top;
    for (int j = 0; j < 6; ++j) {   // A = L D L^T, no pivoting
        double dj = A[j][j];
        for (int k = 0; k < j; ++k) dj -= L[j][k] * L[j][k] * d[k];
        if (!icp_finite(dj) || !(dj > floor_)) return false;
        d[j] = dj;
        for (int r = j + 1; r < 6; ++r) {
            double v = A[r][j];
            for (int k = 0; k < j; ++k) v -= L[r][k] * L[j][k] * d[k];
            L[r][j] = v / dj;
        }
    }
    for (int r = 0; r < 6; ++r) {   // L y = -g
        double v = -acc[23 + r];
        for (int k = 0; k < r; ++k) v -= L[r][k] * x[k];
        x[r] = v;
    }
    for (int r = 0; r < 6; ++r) x[r] /= d[r];
    for (int r = 5; r >= 0; --r)    // L^T x = y
        for (int k = r + 1; k < 6; ++k) x[r] -= L[k][r] * x[k];
    for (int r = 0; r < 6; ++r)
        if (!icp_finite(x[r])) return false;
    const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
    double R[3][3];   // Rz(x2) Ry(x1) Rx(x0)
    R[0][0] = cg * cb;
    R[0][1] = cg * sb * sa - sg * ca;
    R[0][2] = cg * sb * ca + sg * sa;
    R[1][0] = sg * cb;
    R[1][1] = sg * sb * sa + cg * ca;
    R[1][2] = sg * sb * ca - cg * sa;
    R[2][0] = -sb;
    R[2][1] = cb * sa;
    R[2][2] = cb * ca;
    for (int r = 0; r < 3; ++r) {   // Trans(c) [R | x3..5] Trans(-c)
        for (int e = 0; e < 3; ++e) dT[4 * r + e] = R[r][e];
        dT[4 * r + 3] = (c[r] + x[3 + r]) - ((R[r][0] * c[0] + R[r][1] * c[1]) + R[r][2] * c[2]);
    }
    return true;
}

// grid: B blocks of ICP_UPDATE_THREADS.  method: PLANE ? point-to-plane : point-to-point
template <bool PLANE>
__global__ __launch_bounds__(ICP_UPDATE_THREADS) void icp_update_kernel(
    const float* __restrict__ source, const float* __restrict__ target, const float* __restrict__ normals, const double* __restrict__ init,
    double* __restrict__ state, const icp_key* __restrict__ keys, float r2, int pass, int max_iterations, double rel_fitness, double rel_rmse,
    double* __restrict__ transformation, float* __restrict__ fitness, float* __restrict__ inlier_rmse, int* __restrict__ iterations,
    int* __restrict__ status, int* __restrict__ correspondence, int M, int N, int S) {
    constexpr int NACC = PLANE ? 29 : 17;
    constexpr int WAVES = ICP_UPDATE_THREADS / 64;
    __shared__ double part[WAVES][NACC];

    const int tid = threadIdx.x, b = blockIdx.x;
    double* const st = state + (size_t)b * ICP_STATE_DOUBLES;
    if (pass > 0 && st[18] != 0.0) return;   // stopped (uniform)

    double Td[16];
    float tf[16];
    {
        const double* Tin = icp_T(init, state, b, pass);
#pragma unroll
        for (int e = 0; e < 16; ++e) Td[e] = Tin[e];
#pragma unroll
        for (int e = 0; e < 16; ++e) tf[e] = (float)Td[e];
    }
    const float* sb = source + (size_t)b * M * 3;
    const float* tb = target + (size_t)b * N * 3;
    const float* nb = PLANE ? normals + (size_t)b * N * 3 : nullptr;
    const icp_key* kb = keys + (size_t)b * S * (size_t)M;
    const double c[3] = {(double)tb[0], (double)tb[1], (double)tb[2]};

    double acc[NACC];
#pragma unroll
    for (int e = 0; e < NACC; ++e) acc[e] = 0.0;

    for (int m = tid; m < M; m += ICP_UPDATE_THREADS) {
        icp_key key = kb[m];
        for (int s = 1; s < S; ++s) {
            const icp_key other = kb[(size_t)s * M + m];
            key = other < key ? other : key;
        }
        const float d2 = __uint_as_float((unsigned)(key >> 32));
        const unsigned j = (unsigned)(key & 0xffffffffu);
        bool in = d2 <= r2 && d2 < __builtin_inff() && j < (unsigned)N;
        float nx = 0.f, ny = 0.f, nz = 0.f;
        if (PLANE && in) {
            nx = nb[3 * (size_t)j], ny = nb[3 * (size_t)j + 1], nz = nb[3 * (size_t)j + 2];
            in = cloud_finite3(nx, ny, nz);
        }
        if (correspondence) correspondence[(size_t)b * M + m] = in ? (int)j : -1;
        if (!in) continue;
        float pxf, pyf, pzf;
        icp_transform(tf, sb[3 * (size_t)m], sb[3 * (size_t)m + 1], sb[3 * (size_t)m + 2], pxf, pyf, pzf);
        const double p[3] = {(double)pxf - c[0], (double)pyf - c[1], (double)pzf - c[2]};
        const double q[3] = {(double)tb[3 * (size_t)j] - c[0], (double)tb[3 * (size_t)j + 1] - c[1], (double)tb[3 * (size_t)j + 2] - c[2]};
        acc[0] += 1.0;
        acc[1] += (double)d2;
        if (PLANE) {
            const double n[3] = {(double)nx, (double)ny, (double)nz};
            const double res = ((p[0] - q[0]) * n[0] + (p[1] - q[1]) * n[1]) + (p[2] - q[2]) * n[2];
            const double J[6] = {p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2]};
            int o = 2;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int e = r; e < 6; ++e) acc[o++] += J[r] * J[e];
#pragma unroll
            for (int r = 0; r < 6; ++r) acc[23 + r] += J[r] * res;
        } else {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                acc[2 + a] += p[a];
                acc[5 + a] += q[a];
#pragma unroll
                for (int e = 0; e < 3; ++e) acc[8 + 3 * a + e] += p[a] * q[e];
            }
        }
    }

    icp_wave_sums(acc, part);
    __syncthreads();
    if (tid != 0) return;   // (no barrier below)

    double sum[NACC];
    icp_block_sums(part, sum);
    const double n = sum[0];
    const double fit = n / (double)M;
    const double rmse = n > 0.0 ? sqrt(sum[1] / n) : 0.0;

    int stop = -1;
    double dT[12];
    if (pass == 0) {
        bool ok = true;
        for (int e = 0; e < 16; ++e) ok = ok && icp_finite(Td[e]);
        if (!ok) stop = 3;
    }
    if (stop < 0 && pass >= 1 && fabs(fit - st[16]) < rel_fitness && fabs(rmse - st[17]) < rel_rmse) stop = 0;
    if (stop < 0 && pass == max_iterations) stop = 1;
    if (stop < 0 && n < (PLANE ? 6.0 : 3.0)) stop = 2;
    if (stop < 0) {
        if (PLANE) {
            if (!icp_solve_plane(sum, c, dT)) stop = 2;
        } else {
            icp_solve_point(sum, n, c, dT);
            for (int e = 0; e < 12; ++e)
                if (!icp_finite(dT[e])) stop = 2;
        }
    }
    if (stop >= 0) {
        for (int e = 0; e < 16; ++e) transformation[(size_t)b * 16 + e] = Td[e];
        fitness[b] = (float)fit;
        inlier_rmse[b] = (float)rmse;
        iterations[b] = pass;
        status[b] = stop;
        for (int e = 0; e < 16; ++e) st[e] = Td[e];
        st[16] = fit;
        st[17] = rmse;
        st[18] = 1.0;
        return;
    }
    icp_compose(dT, tf, st);
    st[16] = fit;
    st[17] = rmse;
    st[18] = 0.0;
}

}  // namespace

// form 0 / 1 / 2: cloud_plan's forms; the workspace is mandatory, so the auto form can always split.  ws of
// GECCO_ICP_WORKSPACE_BYTES(B, M, N).  -2: arguments out of range, -3: a grid would pass 2^31 - 1
int icp_launch(const float* source, const float* target, const float* normals, const double* init, float r2, int method, int max_iterations,
               double rel_fitness, double rel_rmse, double* transformation, float* fitness, float* inlier_rmse, int* iterations, int* status,
               int* correspondence, void* ws, int B, int M, int N, int form, hipStream_t st) {
    if (B < 1 || M < 1 || N < 1 || form < 0 || form > 2 || method < 0 || method > 1 || max_iterations < 0 || !ws || (method == 1 && !normals))
        return -2;
    const CloudPlan p = cloud_plan(B, M, N, form, true, 256, device_cus());
    if (!p.fits()) return -3;
    double* state = static_cast<double*>(ws);
    icp_key* keys = reinterpret_cast<icp_key*>(state + (size_t)B * ICP_STATE_DOUBLES);
    const unsigned slice = p.S == 1 ? (unsigned)N : (unsigned)GECCO_KNN_SPLIT_SLICE;
    const auto update = method == 1 ? icp_update_kernel<true> : icp_update_kernel<false>;
    for (int pass = 0; pass <= max_iterations; ++pass) {
        dispatch_T(p.T, [&](auto t) {
            constexpr int T = decltype(t)::value;
            hipLaunchKernelGGL(icp_match_kernel<T>, dim3((unsigned)p.blocks), dim3(T), 0, st, source, target, init, state, keys, pass, M, N,
                               p.tiles, p.S, slice);
        });
        hipLaunchKernelGGL(update, dim3((unsigned)B), dim3(ICP_UPDATE_THREADS), 0, st, source, target, normals, init, state, keys, r2, pass,
                           max_iterations, rel_fitness, rel_rmse, transformation, fitness, inlier_rmse, iterations, status, correspondence, M,
                           N, p.S);
        const int rc = (int)hipGetLastError();
        if (rc) return rc;
    }
    return 0;
}
