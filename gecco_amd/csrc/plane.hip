// RANSAC plane segmentation on the device (gfx950): the dominant plane of a cloud (the floor, the table, a wall) and the points on it,
// Open3D's segment_plane and PCL's SACSegmentation with SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE at a fixed number of hypotheses;
// the step between "clean the cloud" (voxel.hip, knn.hip) and "cluster it" (dbscan.hip).  The reference has nothing of the kind; the
// route without this file is a host loop of randint triples, cross products, an (H, N) distance matrix in chunks, argmax and eigh.
//
// Definition: gecco_plane_ransac_f32 (include/gecco_hip.h; tests/_plane_ref.py restates it in numpy).  In short, per cloud: the usable
// points are the indices i in ascending order with three finite coordinates and a non-zero mask entry (K of them); hypothesis h draws
// three of them with the generator of gecco_ransac_f32 (ransac_draw.h), is checked for a degenerate triangle (code 1) and against the
// axis constraint (code 2) in fp64 without a division or a root; its plane is the fp32 pair (nf, cf) with cf the first drawn point; a
// point is an inlier when |((p - cf) . nf)| <= r in uncontracted fp32; the score is the count and the fp64 sum of t^2 accumulated
// sequentially in list order.  The winner is the best hypothesis with count >= max(3, min_inliers) under (count descending, sum
// ascending, h ascending), a total order; refine_passes least-squares refits on its inliers follow.
//
// Three launches whatever the data, no atomics, no workgroup waits on another, no host synchronisation.
//
// plane_points_kernel: one workgroup of PLANE_THREADS per cloud walks i in chunks of PLANE_THREADS; a ballot and the waves' totals in
// LDS give every kept i its rank, so the list is in ascending i: 16 bytes per point, (x, y, z, bits of i).  K goes to the cloud's
// header and to n_points.  Later kernels stream contiguous, aligned data and never touch points or mask again.
//
// plane_hyp_kernel: the hot path.  grid (cloud, block of PLANE_BLOCK_H = 1024 consecutive hypotheses), PLANE_THREADS = 256 threads.
//   phase 1   in four rounds thread t draws and checks hypothesis 256 round + t of the block.  Each round's survivors are appended to an
//             LDS list by ballot rank, so the list is in h order
//   phase 2   one thread per survivor, 256 survivors at a time, with (nf, cf, r) in registers.  The cloud's list passes through LDS
//             tiles of PLANE_TILE points that every thread of the block helps fetch (the next tile is in flight while this one is
//             scanned) and that are read as broadcasts: every lane reads the same 16 bytes, one LDS access per point and wave.  The
//             loop scores PLANE_UNROLL points per trip without a branch (a point outside adds +0.0).  Every thread reaches every
//             barrier: a thread without a survivor still stages tiles
//   phase 3   the block reduces its own results under the total order and writes ONE 16-byte record (count, h, sum) to the workspace:
//             O(B ceil(H / 1024) + B N) bytes instead of O(B H), and the select kernel reads H / 1024 records instead of H results.
//             The order is total, so the winner does not depend on how the hypotheses fall into blocks
//
// plane_select_kernel: one workgroup of PLANE_SELECT_THREADS per cloud reduces the records, rebuilds the winner's plane with the same
// routine (the same bits), then runs the refit passes: thread t takes points t, t + T, ..., the fp64 sums are reduced inside the wave
// by a fixed shuffle tree and across the waves in order, thread 0 solves the 3 x 3 eigenproblem (rigid_fit.h's guarded Jacobi rotation)
// and publishes the plane through LDS; the last evaluation writes the inlier mask, fitness and rmse.
#include "cloud_nn.h"
#include "kernels.h"
#include "ransac_draw.h"
#include "rigid_fit.h"

namespace {

constexpr int PLANE_THREADS = 256;
constexpr int PLANE_BLOCK_H = GECCO_PLANE_RANSAC_BLOCK_HYPOTHESES;
constexpr int PLANE_ROUNDS = PLANE_BLOCK_H / PLANE_THREADS;
constexpr int PLANE_TILE = 256;              // points per LDS tile: 16 bytes each, 4 KiB
constexpr int PLANE_SELECT_THREADS = 512;
constexpr int PLANE_WAVES = PLANE_THREADS / 64;
constexpr int PLANE_UNROLL = 8;             // points of a tile scored per trip of the scoring loop
static_assert(PLANE_TILE == PLANE_THREADS, "a thread fetches one point of a tile");
static_assert(PLANE_TILE % PLANE_UNROLL == 0 && (PLANE_UNROLL & (PLANE_UNROLL - 1)) == 0, "a tile is a whole number of groups");

static __device__ __forceinline__ void plane_load3(const f32x4* __restrict__ pl, int a0, int a1, int a2, double (&X)[3][3]) {
    const f32x4 p0 = pl[a0], p1 = pl[a1], p2 = pl[a2];
#pragma unroll
    for (int e = 0; e < 3; ++e) X[0][e] = (double)p0[e], X[1][e] = (double)p1[e], X[2][e] = (double)p2[e];
}

// n_raw = e1 x e2 of the triple, each component a difference of two rounded products (the spelling of ransac_degenerate)
static __device__ __forceinline__ void plane_cross(const double (&X)[3][3], double (&n)[3]) {
#pragma clang fp contract(off)
    const double e1[3] = {X[1][0] - X[0][0], X[1][1] - X[0][1], X[1][2] - X[0][2]};
    const double e2[3] = {X[2][0] - X[0][0], X[2][1] - X[0][1], X[2][2] - X[0][2]};
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
}

// code 2: the angle between n and the axis is above max_angle, (n . a)^2 < cos2 |n|^2 |a|^2
static __device__ __forceinline__ bool plane_off_axis(const double (&n)[3], const double* __restrict__ ax, double cos2) {
#pragma clang fp contract(off)
    const double a0 = ax[0], a1 = ax[1], a2 = ax[2];
    const double dot = (n[0] * a0 + n[1] * a1) + n[2] * a2;
    return dot * dot < (cos2 * ransac_len2(n[0], n[1], n[2])) * ransac_len2(a0, a1, a2);
}

// the fp64 plane (unit normal n, point c) of a drawn triple: n = n_raw / sqrt(|n_raw|^2), c = the first point
static __device__ __forceinline__ void plane_of_triple(const f32x4* __restrict__ pl, int a0, int a1, int a2, double (&n)[3], double (&c)[3]) {
#pragma clang fp contract(off)
    double X[3][3], nr[3];
    plane_load3(pl, a0, a1, a2, X);
    plane_cross(X, nr);
    const double len = sqrt(ransac_len2(nr[0], nr[1], nr[2]));
#pragma unroll
    for (int e = 0; e < 3; ++e) n[e] = nr[e] / len, c[e] = X[0][e];
}

// the fp64 plane of a candidate [a, b, c, d]: s = 1 / sqrt(|abc|^2), n = abc s, c = -(d s) n
static __device__ __forceinline__ void plane_of_candidate(const double* __restrict__ q, double (&n)[3], double (&c)[3]) {
#pragma clang fp contract(off)
    const double s = 1.0 / sqrt(ransac_len2(q[0], q[1], q[2]));
    const double ds = q[3] * s;
#pragma unroll
    for (int e = 0; e < 3; ++e) n[e] = q[e] * s, c[e] = -ds * n[e];
}

// code 4 of a candidate: a non-finite entry, or a normal whose squared length is zero or not finite
static __device__ __forceinline__ bool plane_bad_candidate(const double* __restrict__ q) {
    const double l2 = ransac_len2(q[0], q[1], q[2]);
    return !(icp_finite(q[0]) && icp_finite(q[1]) && icp_finite(q[2]) && icp_finite(q[3]) && l2 > 0.0 && icp_finite(l2));
}

// the signed distance of p from the plane (nf, cf): every operation rounded to fp32, none contracted
static __device__ __forceinline__ float plane_dist(float nx, float ny, float nz, float cx, float cy, float cz, float px, float py, float pz) {
#pragma clang fp contract(off)
    return ((px - cx) * nx + (py - cy) * ny) + (pz - cz) * nz;
}

// grid: B blocks of PLANE_THREADS
__global__ __launch_bounds__(PLANE_THREADS) void plane_points_kernel(const float* __restrict__ points, const unsigned char* __restrict__ mask,
                                                                     f32x4* __restrict__ list, int* __restrict__ header,
                                                                     int* __restrict__ n_points, int N) {
    __shared__ int wtot[PLANE_WAVES];
    const int tid = threadIdx.x, b = blockIdx.x;
    const float* pb = points + (size_t)b * N * 3;
    const unsigned char* mb = mask ? mask + (size_t)b * N : nullptr;
    f32x4* pl = list + (size_t)b * N;
    int base = 0;   // the usable points before this chunk (uniform)
    for (int i0 = 0; i0 < N; i0 += PLANE_THREADS) {
        const int i = i0 + tid;   // (N <= 2^31 - 1 and i0 < N: i0 + tid can pass 2^31 - 1 only when it is >= N, tested as unsigned)
        bool ok = false;
        float px = 0.f, py = 0.f, pz = 0.f;
        if ((unsigned)i < (unsigned)N && (!mb || mb[i] != 0)) {
            px = pb[3 * (size_t)i], py = pb[3 * (size_t)i + 1], pz = pb[3 * (size_t)i + 2];
            ok = cloud_finite3(px, py, pz);
        }
        const int slot = ransac_append<PLANE_WAVES>(ok, base, wtot);
        if (ok) pl[slot] = f32x4{px, py, pz, __int_as_float(i)};   // slot < K <= N
        __syncthreads();   // wtot is rewritten by the next chunk
    }
    if (tid == 0) {
        header[4 * b] = base;
        n_points[b] = base;
    }
}

// grid: B * bpc blocks of PLANE_THREADS, block (b, blk) owns hypotheses [blk * PLANE_BLOCK_H, min(H, (blk + 1) * PLANE_BLOCK_H))
__global__ __launch_bounds__(PLANE_THREADS) void plane_hyp_kernel(const f32x4* __restrict__ list, const int* __restrict__ header,
                                                                  const double* __restrict__ candidates, const double* __restrict__ axis,
                                                                  double cos2, float r, int min_count, unsigned long long seed,
                                                                  ConsensusRecord* __restrict__ records, int* __restrict__ hyp_triple,
                                                                  float* __restrict__ hyp_plane, int* __restrict__ hyp_count,
                                                                  double* __restrict__ hyp_sum, int H, int N, int bpc) {
    __shared__ __attribute__((aligned(16))) f32x4 tile[PLANE_TILE];
    __shared__ unsigned short surv[PLANE_BLOCK_H];   // the survivors of phase 1 as offsets into the block, in h order
    __shared__ int wtot[PLANE_WAVES];
    __shared__ ConsensusKeys<PLANE_THREADS> keys;

    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)bpc), blk = (int)(blockIdx.x % (unsigned)bpc);
    const int h0 = blk * PLANE_BLOCK_H;   // < H <= 2^24
    const int K = header[4 * b];
    const f32x4* pl = list + (size_t)b * N;
    const size_t hb = (size_t)b * H;
    const double* ax = axis ? axis + 3 * (size_t)b : nullptr;
    const double inf = (double)__builtin_inff();

    auto write = [&](int h, int count, double sum, float nx, float ny, float nz, float cx, float cy, float cz) {
        if (hyp_count) hyp_count[hb + h] = count;
        if (hyp_sum) hyp_sum[hb + h] = sum;
        if (hyp_plane) {
            float* q = hyp_plane + (hb + h) * 6;
            q[0] = nx, q[1] = ny, q[2] = nz, q[3] = cx, q[4] = cy, q[5] = cz;
        }
    };

    // phase 1
    int nsurv = 0;   // uniform
#pragma unroll 1
    for (int round = 0; round < PLANE_ROUNDS; ++round) {
        const int o = round * PLANE_THREADS + tid, h = h0 + o;
        bool live = false;
        if (h < H) {
            int code = 0, a0 = -1, a1 = -1, a2 = -1;
            if (K < 3) {
                code = 1;   // no triangle
            } else if (candidates) {
                const double* q = candidates + (hb + h) * 4;
                if (plane_bad_candidate(q)) {
                    code = 4;
                } else if (ax) {
                    const double nr[3] = {q[0], q[1], q[2]};
                    if (plane_off_axis(nr, ax, cos2)) code = 2;
                }
            } else {
                ransac_draw(seed, h, K, a0, a1, a2);
                double X[3][3];
                plane_load3(pl, a0, a1, a2, X);
                if (ransac_degenerate(X)) {
                    code = 1;
                } else if (ax) {
                    double nr[3];
                    plane_cross(X, nr);
                    if (plane_off_axis(nr, ax, cos2)) code = 2;
                }
            }
            if (hyp_triple) {
                int* t3 = hyp_triple + (hb + h) * 3;
                t3[0] = a0, t3[1] = a1, t3[2] = a2;
            }
            if (code)
                write(h, -code, inf, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f);
            else
                live = true;
        }
        const int slot = ransac_append<PLANE_WAVES>(live, nsurv, wtot);
        if (live) surv[slot] = (unsigned short)o;   // slot < PLANE_BLOCK_H
        __syncthreads();   // wtot is rewritten by the next round; after the last one, surv is complete
    }

    // phase 2
    int bc = 0, bh = -1;   // this thread's best among its survivors
    double bs = 0.0;
#pragma unroll 1
    for (int s0 = 0; s0 < nsurv; s0 += PLANE_THREADS) {
        const bool valid = s0 + tid < nsurv;
        int h = 0;
        float nx = 0.f, ny = 0.f, nz = 0.f, cx = 0.f, cy = 0.f, cz = 0.f;
        if (valid) {
            h = h0 + (int)surv[s0 + tid];
            double n[3], c[3];
            if (candidates) {
                plane_of_candidate(candidates + (hb + h) * 4, n, c);
            } else {
                int a0, a1, a2;
                ransac_draw(seed, h, K, a0, a1, a2);
                plane_of_triple(pl, a0, a1, a2, n, c);
            }
            nx = (float)n[0], ny = (float)n[1], nz = (float)n[2];
            cx = (float)c[0], cy = (float)c[1], cz = (float)c[2];
        }
        int count = 0;
        double sum = 0.0;

        f32x4 rp;
        const float nan = __builtin_nanf("");
        auto fetch = [&](int base) {
            const int a = base + tid;   // base < K <= N and K + 256 stays below 2^31 + 256: compared as unsigned
            rp = (unsigned)a < (unsigned)K ? pl[a] : f32x4{nan, nan, nan, 0.f};   // past the list: a point that is nobody's inlier
        };
        fetch(0);
        for (int base = 0; base < K; base += PLANE_TILE) {
            __syncthreads();   // the scan of the previous tile is over
            tile[tid] = rp;
            __syncthreads();
            if (K - base > PLANE_TILE) fetch(base + PLANE_TILE);
            if (!valid) continue;
            // list order: the sum is sequential.  No branch: a point outside adds +0.0, which changes no bit of a sum that starts at
            // +0.0 and only ever takes squares; PLANE_UNROLL reads are in flight at once, the NaN entries behind the list fill the last group
            const int cnt = (min(PLANE_TILE, K - base) + PLANE_UNROLL - 1) & ~(PLANE_UNROLL - 1);
            for (int g0 = 0; g0 < cnt; g0 += PLANE_UNROLL) {
                f32x4 p[PLANE_UNROLL];
#pragma unroll
                for (int u = 0; u < PLANE_UNROLL; ++u) p[u] = tile[g0 + u];
#pragma unroll
                for (int u = 0; u < PLANE_UNROLL; ++u) {
                    const float t = plane_dist(nx, ny, nz, cx, cy, cz, p[u][0], p[u][1], p[u][2]);
                    const bool in = fabsf(t) <= r;
                    count += in ? 1 : 0;
                    sum += in ? (double)t * (double)t : 0.0;   // exact in fp64
                }
            }
        }
        if (valid) {
            write(h, count, sum, nx, ny, nz, cx, cy, cz);
            if (count >= min_count && ransac_better(count, sum, h, bc, bs, bh)) bc = count, bs = sum, bh = h;
        }
    }

    // phase 3: the block's winner
    ransac_block_best(bc, bs, bh, keys);
    if (tid == 0) records[(size_t)b * bpc + blk] = ConsensusRecord{keys.c[0], keys.h[0], keys.s[0]};
}

constexpr int PLANE_NACC = 11;   // sum 1, sum t^2, sum d (3), sum d d^T (xx, xy, xz, yy, yz, zz) with d = p - c0

// The least-squares plane of the reduced sums about c0: C = S / n - m m^T scaled by its largest magnitude, 8 cyclic Jacobi sweeps over
// (0, 1), (0, 2), (1, 2) (icp_rotate on the 3 x 3 block of a 4 x 4 matrix whose last row and column are zero), the eigenvector of the
// smallest eigenvalue (the lowest index among equals), normalised.  n: the unit normal, c = c0 + m.  False when the result is not finite.
static __device__ __noinline__ bool plane_refit(const double* sum, const double* c0, double* n, double* c) {
    const double inv = 1.0 / sum[0];
    const double m[3] = {sum[2] * inv, sum[3] * inv, sum[4] * inv};
    double a[4][4], v[4][4];
    for (int r = 0; r < 4; ++r)
        for (int e = 0; e < 4; ++e) a[r][e] = 0.0, v[r][e] = r == e ? 1.0 : 0.0;
    a[0][0] = sum[5] * inv - m[0] * m[0];
    a[0][1] = a[1][0] = sum[6] * inv - m[0] * m[1];
    a[0][2] = a[2][0] = sum[7] * inv - m[0] * m[2];
    a[1][1] = sum[8] * inv - m[1] * m[1];
    a[1][2] = a[2][1] = sum[9] * inv - m[1] * m[2];
    a[2][2] = sum[10] * inv - m[2] * m[2];
    double big = 0.0;
    for (int r = 0; r < 3; ++r)
        for (int e = 0; e < 3; ++e) big = fmax(big, fabs(a[r][e]));
    if (big > 0.0 && icp_finite(big)) {
        const double sc = 1.0 / big;
        for (int r = 0; r < 3; ++r)
            for (int e = 0; e < 3; ++e) a[r][e] *= sc;
    }
    for (int sweep = 0; sweep < ICP_JACOBI_SWEEPS; ++sweep) {
        icp_rotate(a, v, 0, 1);
        icp_rotate(a, v, 0, 2);
        icp_rotate(a, v, 1, 2);
    }
    int low = 0;   // the smallest eigenvalue, the lowest index among equals
    for (int e = 1; e < 3; ++e)
        if (a[e][e] < a[low][low]) low = e;
    const double x = v[0][low], y = v[1][low], z = v[2][low];
    const double rn = 1.0 / sqrt(ransac_len2(x, y, z));
    n[0] = x * rn, n[1] = y * rn, n[2] = z * rn;
    bool ok = true;
    for (int e = 0; e < 3; ++e) {
        c[e] = c0[e] + m[e];
        ok = ok && icp_finite(n[e]) && icp_finite(c[e]);
    }
    return ok;
}

// [a, b, c, d] of the plane (n, c): the sign rule of normals.hip (towards the viewpoint, or the component of largest magnitude positive,
// the lowest axis among equals) in fp64, then d = -(n . c)
static __device__ void plane_publish(const double* n, const double* c, const float* __restrict__ vp, double* __restrict__ out) {
#pragma clang fp contract(off)
    bool flip;
    if (vp) {
        flip = (n[0] * ((double)vp[0] - c[0]) + n[1] * ((double)vp[1] - c[1])) + n[2] * ((double)vp[2] - c[2]) < 0.0;
    } else {
        const double ax = fabs(n[0]), ay = fabs(n[1]), az = fabs(n[2]);
        const double lead = (ax >= ay && ax >= az) ? n[0] : (ay >= az ? n[1] : n[2]);
        flip = lead < 0.0;
    }
    const double sg = flip ? -1.0 : 1.0;
    const double x = sg * n[0], y = sg * n[1], z = sg * n[2];
    out[0] = x, out[1] = y, out[2] = z;
    out[3] = -((x * c[0] + y * c[1]) + z * c[2]);
}

// grid: B blocks of PLANE_SELECT_THREADS
__global__ __launch_bounds__(PLANE_SELECT_THREADS) void plane_select_kernel(
    const f32x4* __restrict__ list, const int* __restrict__ header, const ConsensusRecord* __restrict__ records,
    const double* __restrict__ candidates, const float* __restrict__ viewpoint, float r, int refine_passes, unsigned long long seed,
    double* __restrict__ plane, float* __restrict__ fitness, float* __restrict__ inlier_rmse, int* __restrict__ n_inliers,
    int* __restrict__ best, int* __restrict__ status, unsigned char* __restrict__ inliers, int H, int N, int bpc) {
    constexpr int WAVES = PLANE_SELECT_THREADS / 64;
    __shared__ double part[WAVES][PLANE_NACC];
    __shared__ double Psh[6];   // the current plane in fp64: the unit normal, then the point it passes through
    __shared__ ConsensusKeys<PLANE_SELECT_THREADS> keys;
    __shared__ int done;

    const int tid = threadIdx.x, b = blockIdx.x;
    const int K = header[4 * b];
    const f32x4* pl = list + (size_t)b * N;
    unsigned char* const ib = inliers ? inliers + (size_t)b * N : nullptr;
    const float* vp = viewpoint ? viewpoint + 3 * (size_t)b : nullptr;
    double* const out = plane + 4 * (size_t)b;

    if (ib)
        for (int i = tid; i < N; i += PLANE_SELECT_THREADS) ib[i] = 0;

    ransac_best_record(records + (size_t)b * bpc, bpc, keys);
    if (tid == 0) {
        const int win = K >= 3 ? keys.h[0] : -1;
        if (win < 0) {
            out[0] = 0.0, out[1] = 0.0, out[2] = 1.0, out[3] = 0.0;
            fitness[b] = 0.f;
            inlier_rmse[b] = 0.f;
            n_inliers[b] = 0;
            best[b] = -1;
            status[b] = K < 3 ? 2 : 1;
            done = 1;
        } else {
            double n[3], c[3];
            if (candidates) {
                plane_of_candidate(candidates + ((size_t)b * H + win) * 4, n, c);
            } else {
                int a0, a1, a2;
                ransac_draw(seed, win, K, a0, a1, a2);
                plane_of_triple(pl, a0, a1, a2, n, c);   // the bits of the hypothesis kernel
            }
            for (int e = 0; e < 3; ++e) Psh[e] = n[e], Psh[3 + e] = c[e];
            best[b] = win;
            status[b] = 0;
            done = 0;
        }
    }
    __syncthreads();
    if (done) return;   // uniform; the inlier mask is all zero

    const f32x4 q0 = pl[0];   // K >= 3
    const double c0[3] = {(double)q0[0], (double)q0[1], (double)q0[2]};

    for (int pass = 0;; ++pass) {
        double Pd[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) Pd[e] = Psh[e];
        const float nx = (float)Pd[0], ny = (float)Pd[1], nz = (float)Pd[2], cx = (float)Pd[3], cy = (float)Pd[4], cz = (float)Pd[5];

        double acc[PLANE_NACC];
#pragma unroll
        for (int e = 0; e < PLANE_NACC; ++e) acc[e] = 0.0;
        for (int a = tid; a < K; a += PLANE_SELECT_THREADS) {
#pragma clang fp contract(off)
            const f32x4 p = pl[a];
            const float t = plane_dist(nx, ny, nz, cx, cy, cz, p[0], p[1], p[2]);
            const bool in = fabsf(t) <= r;
            if (ib) ib[__float_as_int(p[3])] = in ? 1 : 0;   // the last pass's stay; the index is the i the compaction stored, < N
            if (!in) continue;
            const double dx = (double)p[0] - c0[0], dy = (double)p[1] - c0[1], dz = (double)p[2] - c0[2];
            acc[0] += 1.0;
            acc[1] += (double)t * (double)t;
            acc[2] += dx, acc[3] += dy, acc[4] += dz;
            acc[5] += dx * dx, acc[6] += dx * dy, acc[7] += dx * dz;
            acc[8] += dy * dy, acc[9] += dy * dz, acc[10] += dz * dz;
        }
        icp_wave_sums(acc, part);
        __syncthreads();
        if (tid == 0) {
            double sum[PLANE_NACC];
            icp_block_sums(part, sum);
            const double n = sum[0];
            bool last = pass >= refine_passes || n < 3.0;
            double nn[3], cn[3];
            if (!last && !plane_refit(sum, c0, nn, cn)) last = true;
            if (last) {
                plane_publish(Pd, Pd + 3, vp, out);
                fitness[b] = (float)(n / (double)K);
                inlier_rmse[b] = n > 0.0 ? (float)sqrt(sum[1] / n) : 0.f;
                n_inliers[b] = (int)n;
                done = 1;
            } else {
                for (int e = 0; e < 3; ++e) Psh[e] = nn[e], Psh[3 + e] = cn[e];
            }
        }
        __syncthreads();
        if (done) return;   // uniform
    }
}

}  // namespace

// ws of GECCO_PLANE_RANSAC_WORKSPACE_BYTES(B, N, H), 16-byte aligned: the point lists (16 B N), the block records (16 B ceil(H / 1024)),
// the headers (16 B).  -2: arguments out of range, -3: a grid would pass 2^31 - 1
int plane_ransac_launch(const float* points, const unsigned char* mask, float r, int H, int refine_passes, unsigned long long seed,
                        const double* axis, double cos2, int min_inliers, const float* viewpoint, const double* candidates, double* plane,
                        float* fitness, float* inlier_rmse, int* n_points, int* n_inliers, int* best, int* status, unsigned char* inliers,
                        int* hyp_triple, float* hyp_plane, int* hyp_count, double* hyp_sum, void* ws, int B, int N, hipStream_t st) {
    if (B < 1 || N < 1 || H < 1 || H > GECCO_PLANE_RANSAC_MAX_HYPOTHESES || refine_passes < 0 ||
        refine_passes > GECCO_PLANE_RANSAC_MAX_REFINE || !ws)
        return -2;
    const int bpc = (H + PLANE_BLOCK_H - 1) / PLANE_BLOCK_H;
    if ((long long)B * bpc > 0x7fffffffLL) return -3;
    const int min_count = min_inliers > 3 ? min_inliers : 3;
    f32x4* list = static_cast<f32x4*>(ws);
    ConsensusRecord* records = reinterpret_cast<ConsensusRecord*>(list + (size_t)B * N);
    int* header = reinterpret_cast<int*>(records + (size_t)B * bpc);
    hipLaunchKernelGGL(plane_points_kernel, dim3((unsigned)B), dim3(PLANE_THREADS), 0, st, points, mask, list, header, n_points, N);
    hipLaunchKernelGGL(plane_hyp_kernel, dim3((unsigned)((long long)B * bpc)), dim3(PLANE_THREADS), 0, st, list, header, candidates, axis, cos2,
                       r, min_count, seed, records, hyp_triple, hyp_plane, hyp_count, hyp_sum, H, N, bpc);
    hipLaunchKernelGGL(plane_select_kernel, dim3((unsigned)B), dim3(PLANE_SELECT_THREADS), 0, st, list, header, records, candidates, viewpoint,
                       r, refine_passes, seed, plane, fitness, inlier_rmse, n_inliers, best, status, inliers, H, N, bpc);
    return (int)hipGetLastError();
}
