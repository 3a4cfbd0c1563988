// Global registration by RANSAC on correspondences on the device (gfx950): the pose estimator between match_features and icp, Open3D's
// registration_ransac_based_on_correspondence with a fixed number of hypotheses.  The reference has nothing of the kind; the route
// without this file is a host loop of randint triples, a batched SVD and an (H, K, 3) tensor per chunk.
//
// Definition: gecco_ransac_f32 (include/gecco_hip.h; tests/_ransac_ref.py restates it in numpy).  In short, per cloud: the pairs are
// the source indices i in ascending order whose corr[i] is in range and whose six coordinates are finite (K of them); hypothesis h draws
// three distinct pairs from a counter-based generator (pure integer work), is checked for a degenerate triangle (code 1) and for edge
// lengths (code 2) in fp64 without a division or a root, fitted by Horn's quaternion (rigid_fit.h: the routine of icp.hip; a non-finite
// T is code 4), checked for distance on its own three pairs under Tf = fp32(T) (code 3) and scored over all K pairs: count of d2 <= r2
// and the fp64 sum of those d2 accumulated sequentially in pair order.  The winner is the best survivor with count >= 3 under (count
// descending, sum ascending, h ascending), a total order; refine_passes least-squares refits on its inliers follow.
//
// Three launches whatever the data, no atomics, no workgroup waits on another, no host synchronisation.
//
// ransac_pairs_kernel: one workgroup of RANSAC_THREADS per cloud walks i in chunks of RANSAC_THREADS; a ballot and the waves' totals in
// LDS give every kept i its rank, so the list is in ascending i.  Pair a is written as two 16-byte entries, (P, bits of i) and
// (Q, bits of j), at pairs[2 a] and pairs[2 a + 1]; K goes to the cloud's header and to n_pairs.  Later kernels stream contiguous,
// aligned data and never touch corr again.
//
// ransac_hyp_kernel: the hot path.  grid (cloud, block of RANSAC_BLOCK_H = 1024 consecutive hypotheses), RANSAC_THREADS = 256 threads.
//   phase 1   in four rounds thread t draws and checks (codes 1, 2; with candidates: the finite test) hypothesis 256 round + t of the
//             block: cheap, no fit.  Each round's survivors are appended to an LDS list by ballot rank, so the list is in h order
//   phase 2   one thread per survivor, 256 survivors at a time: the fit (__noinline__, as in icp.hip), the distance check and the score.
//             The cloud's pairs pass through LDS tiles of RANSAC_TILE pairs that every thread of the block helps fetch (the next tile is
//             in flight while this one is scanned) and are read as broadcasts, the loop of knn_scan_kernel / icp_match_kernel.  Every
//             thread reaches every barrier: a thread without a survivor still stages tiles
//   phase 3   the block reduces its own survivors with count >= 3 under the total order and writes ONE 16-byte record (count, h, sum) to
//             the workspace (plane.hip's phase 3; ransac_draw.h holds what the two files share): the select kernel reads H / 1024
//             records.  A hypothesis's count and sum depend on h alone and the order is total, so the winner does not depend on how
//             the hypotheses fall into blocks.  Per-hypothesis stores remain only for hyp_triple, hyp_count and hyp_sum, when given
//
// ransac_select_kernel: one workgroup of RANSAC_SELECT_THREADS per cloud reduces the records (a total order: any tree gives the same
// winner), refits the winner's triple with the same routine (the same bits), then runs the refine passes: thread t takes pairs t, t + T,
// ..., the fp64 sums are reduced inside the wave by a fixed shuffle tree and across the waves in order, thread 0 solves and publishes T
// through LDS; the last evaluation writes fitness, rmse and the inlier list.
#include "cloud_nn.h"
#include "kernels.h"
#include "launch_state.h"
#include "ransac_draw.h"
#include "rigid_fit.h"

namespace {

constexpr int RANSAC_THREADS = 256;
constexpr int RANSAC_BLOCK_H = GECCO_RANSAC_BLOCK_HYPOTHESES;
constexpr int RANSAC_ROUNDS = RANSAC_BLOCK_H / RANSAC_THREADS;
constexpr int RANSAC_TILE = 256;             // pairs per LDS tile: two 16-byte entries each, 8 KiB
constexpr int RANSAC_SELECT_THREADS = 512;
constexpr int RANSAC_WAVES = RANSAC_THREADS / 64;
static_assert(RANSAC_TILE == RANSAC_THREADS, "a thread fetches one pair of a tile");

// checks 1 and 2 of the triple (a0, a1, a2): 0 when it passes, else the code
static __device__ __forceinline__ int ransac_precheck(const f32x4* __restrict__ pr, int a0, int a1, int a2, double s2) {
#pragma clang fp contract(off)
    const int a[3] = {a0, a1, a2};
    double P[3][3], Q[3][3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const f32x4 p = pr[2 * (size_t)a[t]], q = pr[2 * (size_t)a[t] + 1];
#pragma unroll
        for (int e = 0; e < 3; ++e) P[t][e] = (double)p[e], Q[t][e] = (double)q[e];
    }
    if (ransac_degenerate(P) || ransac_degenerate(Q)) return 1;
#pragma unroll
    for (int t = 0; t < 3; ++t) {   // the edges (a0, a1), (a1, a2), (a2, a0)
        const int u = (t + 1) % 3;
        const double dp = ransac_len2(P[t][0] - P[u][0], P[t][1] - P[u][1], P[t][2] - P[u][2]);
        const double dq = ransac_len2(Q[t][0] - Q[u][0], Q[t][1] - Q[u][1], Q[t][2] - Q[u][2]);
        if (!(dp >= s2 * dq) || !(dq >= s2 * dp)) return 2;
    }
    return 0;
}

// check 3: T (rows 0 .. 2, row-major 3 x 4) from the three pairs, moments about double(Q_a0) summed in the order a0, a1, a2 in the
// layout icp_solve_point reads.  False when T is not finite.  One routine for the hypothesis kernel and the winner's refit.
static __device__ __noinline__ bool ransac_fit_triple(const f32x4* __restrict__ pr, int a0, int a1, int a2, double* T) {
#pragma clang fp contract(off)
    const int a[3] = {a0, a1, a2};
    double acc[17];
    for (int e = 0; e < 17; ++e) acc[e] = 0.0;
    const f32x4 q0 = pr[2 * (size_t)a0 + 1];
    const double c[3] = {(double)q0[0], (double)q0[1], (double)q0[2]};
    for (int t = 0; t < 3; ++t) {
        const f32x4 pf = pr[2 * (size_t)a[t]], qf = pr[2 * (size_t)a[t] + 1];
        const double p[3] = {(double)pf[0] - c[0], (double)pf[1] - c[1], (double)pf[2] - c[2]};
        const double q[3] = {(double)qf[0] - c[0], (double)qf[1] - c[1], (double)qf[2] - c[2]};
        for (int r = 0; r < 3; ++r) {
            acc[2 + r] += p[r];
            acc[5 + r] += q[r];
            for (int e = 0; e < 3; ++e) acc[8 + 3 * r + e] += p[r] * q[e];
        }
    }
    icp_solve_point(acc, 3.0, c, T);
    bool ok = true;
    for (int e = 0; e < 12; ++e) ok = ok && icp_finite(T[e]);
    return ok;
}

// d2 of pair (p, q) under tf: icp's transform, then cloud_nn.h's dist2 of p' against q
static __device__ __forceinline__ float ransac_d2(const float* tf, const f32x4 p, const f32x4 q) {
    float x, y, z;
    icp_transform(tf, p[0], p[1], p[2], x, y, z);
    return cloud_dist2(x, y, z, q[0], q[1], q[2]);
}

// grid: B blocks of RANSAC_THREADS
__global__ __launch_bounds__(RANSAC_THREADS) void ransac_pairs_kernel(const float* __restrict__ source, const float* __restrict__ target,
                                                                      const int* __restrict__ corr, f32x4* __restrict__ pairs,
                                                                      int* __restrict__ header, int* __restrict__ n_pairs, int M, int N) {
    __shared__ int wtot[RANSAC_WAVES];
    const int tid = threadIdx.x, b = blockIdx.x;
    const float* sb = source + (size_t)b * M * 3;
    const float* tb = target + (size_t)b * N * 3;
    const int* cb = corr + (size_t)b * M;
    f32x4* pr = pairs + (size_t)b * M * 2;
    int base = 0;   // the pairs before this chunk (uniform)
    for (int i0 = 0; i0 < M; i0 += RANSAC_THREADS) {
        const int i = i0 + tid;   // (M <= 2^31 - 1 and i0 < M: i0 + tid can pass 2^31 - 1 only when it is >= M, tested as unsigned)
        bool ok = false;
        int j = -1;
        float px = 0.f, py = 0.f, pz = 0.f, qx = 0.f, qy = 0.f, qz = 0.f;
        if ((unsigned)i < (unsigned)M) {
            j = cb[i];
            if (j >= 0 && j < N) {
                px = sb[3 * (size_t)i], py = sb[3 * (size_t)i + 1], pz = sb[3 * (size_t)i + 2];
                qx = tb[3 * (size_t)j], qy = tb[3 * (size_t)j + 1], qz = tb[3 * (size_t)j + 2];
                ok = cloud_finite3(px, py, pz) && cloud_finite3(qx, qy, qz);
            }
        }
        const int slot = ransac_append<RANSAC_WAVES>(ok, base, wtot);
        if (ok) {   // slot < K <= M
            pr[2 * (size_t)slot] = f32x4{px, py, pz, __int_as_float(i)};
            pr[2 * (size_t)slot + 1] = f32x4{qx, qy, qz, __int_as_float(j)};
        }
        __syncthreads();   // wtot is rewritten by the next chunk
    }
    if (tid == 0) {
        header[4 * b] = base;
        n_pairs[b] = base;
    }
}

// grid: B * bpc blocks of RANSAC_THREADS, block (b, blk) owns hypotheses [blk * RANSAC_BLOCK_H, min(H, (blk + 1) * RANSAC_BLOCK_H))
__global__ __launch_bounds__(RANSAC_THREADS) void ransac_hyp_kernel(const f32x4* __restrict__ pairs, const int* __restrict__ header,
                                                                    const double* __restrict__ candidates, float r2, double s2,
                                                                    unsigned long long seed, ConsensusRecord* __restrict__ records,
                                                                    int* __restrict__ hyp_triple, int* __restrict__ hyp_count,
                                                                    double* __restrict__ hyp_sum, int H, int M, int bpc) {
    __shared__ __attribute__((aligned(16))) f32x4 tile[2 * RANSAC_TILE];
    __shared__ unsigned short surv[RANSAC_BLOCK_H];   // the survivors of phase 1 as offsets into the block, in h order
    __shared__ int wtot[RANSAC_WAVES];
    __shared__ ConsensusKeys<RANSAC_THREADS> keys;

    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)bpc), blk = (int)(blockIdx.x % (unsigned)bpc);
    const int h0 = blk * RANSAC_BLOCK_H;   // < H <= 2^24
    const int K = header[4 * b];
    const f32x4* pr = pairs + (size_t)b * M * 2;
    const size_t hb = (size_t)b * H;
    const double inf = (double)__builtin_inff();

    auto write = [&](int h, int count, double sum) {
        if (hyp_count) hyp_count[hb + h] = count;
        if (hyp_sum) hyp_sum[hb + h] = sum;
    };

    // phase 1
    int nsurv = 0;   // uniform
#pragma unroll 1
    for (int round = 0; round < RANSAC_ROUNDS; ++round) {
        const int o = round * RANSAC_THREADS + tid, h = h0 + o;
        bool live = false;
        if (h < H) {
            int code, a0 = -1, a1 = -1, a2 = -1;
            if (K < 3) {
                code = 1;   // no triangle
            } else if (candidates) {
                const double* Tc = candidates + (hb + h) * 16;
                bool ok = true;
#pragma unroll
                for (int e = 0; e < 16; ++e) ok = ok && icp_finite(Tc[e]);
                code = ok ? 0 : 4;
            } else {
                ransac_draw(seed, h, K, a0, a1, a2);
                code = ransac_precheck(pr, a0, a1, a2, s2);
            }
            if (hyp_triple) {
                int* t3 = hyp_triple + (hb + h) * 3;
                t3[0] = a0, t3[1] = a1, t3[2] = a2;
            }
            if (code)
                write(h, -code, inf);
            else
                live = true;
        }
        const int slot = ransac_append<RANSAC_WAVES>(live, nsurv, wtot);
        if (live) surv[slot] = (unsigned short)o;   // slot < RANSAC_BLOCK_H
        __syncthreads();   // wtot is rewritten by the next round; after the last one, surv is complete
    }

    // phase 2
    int bc = 0, bh = -1;   // this thread's best among its survivors
    double bs = 0.0;
#pragma unroll 1
    for (int s0 = 0; s0 < nsurv; s0 += RANSAC_THREADS) {
        const bool valid = s0 + tid < nsurv;
        int h = 0, code = 0;
        float tf[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) tf[e] = 0.f;
        if (valid) {
            h = h0 + (int)surv[s0 + tid];
            if (candidates) {
                const double* Tc = candidates + (hb + h) * 16;
#pragma unroll
                for (int e = 0; e < 12; ++e) tf[e] = (float)Tc[e];
            } else {
                double T[12];
                int a0, a1, a2;
                ransac_draw(seed, h, K, a0, a1, a2);
                if (!ransac_fit_triple(pr, a0, a1, a2, T)) code = 4;
#pragma unroll
                for (int e = 0; e < 12; ++e) tf[e] = (float)T[e];
                if (code == 0) {   // check 4
                    const int a[3] = {a0, a1, a2};
#pragma unroll
                    for (int t = 0; t < 3; ++t)
                        if (!(ransac_d2(tf, pr[2 * (size_t)a[t]], pr[2 * (size_t)a[t] + 1]) <= r2)) code = 3;
                }
            }
        }
        const bool scoring = valid && code == 0;
        int count = 0;
        double sum = 0.0;

        f32x4 rp, rq;
        auto fetch = [&](int base) {
            const int a = base + tid;   // base < K <= M and K + 256 stays below 2^31 + 256: compared as unsigned
            const bool in = (unsigned)a < (unsigned)K;
            rp = in ? pr[2 * (size_t)a] : f32x4{0.f, 0.f, 0.f, 0.f};
            rq = in ? pr[2 * (size_t)a + 1] : f32x4{0.f, 0.f, 0.f, 0.f};
        };
        fetch(0);
        for (int base = 0; base < K; base += RANSAC_TILE) {
            __syncthreads();   // the scan of the previous tile is over
            tile[2 * tid] = rp;
            tile[2 * tid + 1] = rq;
            __syncthreads();
            if (K - base > RANSAC_TILE) fetch(base + RANSAC_TILE);
            if (!scoring) continue;
            const int cnt = min(RANSAC_TILE, K - base);   // entries past cnt are never pairs
            for (int g = 0; g < cnt; ++g) {   // pair order: the sum is sequential
                const float d2 = ransac_d2(tf, tile[2 * g], tile[2 * g + 1]);
                if (d2 <= r2) {
                    count += 1;
                    sum += (double)d2;
                }
            }
        }
        if (valid) {
            if (code) {
                write(h, -code, inf);
            } else {
                write(h, count, sum);
                if (count >= 3 && ransac_better(count, sum, h, bc, bs, bh)) bc = count, bs = sum, bh = h;
            }
        }
    }

    // phase 3: the block's winner
    ransac_block_best(bc, bs, bh, keys);
    if (tid == 0) records[(size_t)b * bpc + blk] = ConsensusRecord{keys.c[0], keys.h[0], keys.s[0]};
}

// grid: B blocks of RANSAC_SELECT_THREADS
__global__ __launch_bounds__(RANSAC_SELECT_THREADS) void ransac_select_kernel(
    const f32x4* __restrict__ pairs, const int* __restrict__ header, const ConsensusRecord* __restrict__ records,
    const double* __restrict__ candidates, float r2, int refine_passes, unsigned long long seed, double* __restrict__ transformation,
    float* __restrict__ fitness, float* __restrict__ inlier_rmse, int* __restrict__ best, int* __restrict__ status, int* __restrict__ inliers,
    int H, int M, int bpc) {
    constexpr int NACC = 17;
    constexpr int WAVES = RANSAC_SELECT_THREADS / 64;
    __shared__ double part[WAVES][NACC];
    __shared__ double Tsh[16];
    __shared__ ConsensusKeys<RANSAC_SELECT_THREADS> keys;
    __shared__ int done;

    const int tid = threadIdx.x, b = blockIdx.x;
    const int K = header[4 * b];
    const f32x4* pr = pairs + (size_t)b * M * 2;
    int* const ib = inliers ? inliers + (size_t)b * M : nullptr;

    if (ib)
        for (int i = tid; i < M; i += RANSAC_SELECT_THREADS) ib[i] = -1;

    ransac_best_record(records + (size_t)b * bpc, bpc, keys);
    if (tid == 0) {
        const int win = K >= 3 ? keys.h[0] : -1;
        bool found = win >= 0;
        double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        if (found) {
            if (candidates) {
                for (int e = 0; e < 16; ++e) T[e] = candidates[((size_t)b * H + win) * 16 + e];
            } else {
                int a0, a1, a2;
                ransac_draw(seed, win, K, a0, a1, a2);
                found = ransac_fit_triple(pr, a0, a1, a2, T);   // the bits of the hypothesis kernel: it succeeds as it did there
                if (!found)
                    for (int e = 0; e < 12; ++e) T[e] = (e % 5 == 0) ? 1.0 : 0.0;
            }
        }
        for (int e = 0; e < 16; ++e) Tsh[e] = T[e];
        done = found ? 0 : 1;
        if (!found) {
            for (int e = 0; e < 16; ++e) transformation[(size_t)b * 16 + e] = T[e];
            fitness[b] = 0.f;
            inlier_rmse[b] = 0.f;
            best[b] = -1;
            status[b] = K < 3 ? 2 : 1;
        } else {
            best[b] = win;
            status[b] = 0;
        }
    }
    __syncthreads();
    if (done) return;   // uniform; the inlier list is all -1

    const f32x4 q0 = pr[1];   // K >= 3
    const double c[3] = {(double)q0[0], (double)q0[1], (double)q0[2]};

    for (int pass = 0;; ++pass) {
        double Td[16];
        float tf[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) Td[e] = Tsh[e];
#pragma unroll
        for (int e = 0; e < 16; ++e) tf[e] = (float)Td[e];

        double acc[NACC];
#pragma unroll
        for (int e = 0; e < NACC; ++e) acc[e] = 0.0;
        for (int a = tid; a < K; a += RANSAC_SELECT_THREADS) {
            const f32x4 pf = pr[2 * (size_t)a], qf = pr[2 * (size_t)a + 1];
            float pxf, pyf, pzf;
            icp_transform(tf, pf[0], pf[1], pf[2], pxf, pyf, pzf);
            const float d2 = cloud_dist2(pxf, pyf, pzf, qf[0], qf[1], qf[2]);
            const bool in = d2 <= r2;
            if (ib) ib[__float_as_int(pf[3])] = in ? __float_as_int(qf[3]) : -1;   // the last pass's stay; the index is the i the compaction stored, < M
            if (!in) continue;
            const double p[3] = {(double)pxf - c[0], (double)pyf - c[1], (double)pzf - c[2]};
            const double q[3] = {(double)qf[0] - c[0], (double)qf[1] - c[1], (double)qf[2] - c[2]};
            acc[0] += 1.0;
            acc[1] += (double)d2;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                acc[2 + r] += p[r];
                acc[5 + r] += q[r];
#pragma unroll
                for (int e = 0; e < 3; ++e) acc[8 + 3 * r + e] += p[r] * q[e];
            }
        }
        icp_wave_sums(acc, part);
        __syncthreads();
        if (tid == 0) {
            double sum[NACC];
            icp_block_sums(part, sum);
            const double n = sum[0];
            bool last = pass >= refine_passes || n < 3.0;
            double dT[12];
            if (!last) {
                icp_solve_point(sum, n, c, dT);
                for (int e = 0; e < 12; ++e)
                    if (!icp_finite(dT[e])) last = true;
            }
            if (last) {
                for (int e = 0; e < 16; ++e) transformation[(size_t)b * 16 + e] = Td[e];
                fitness[b] = (float)(n / (double)K);
                inlier_rmse[b] = n > 0.0 ? (float)sqrt(sum[1] / n) : 0.f;
                done = 1;
            } else {
                icp_compose(dT, tf, Tsh);
            }
        }
        __syncthreads();
        if (done) return;   // uniform
    }
}

}  // namespace

// ws of GECCO_RANSAC_WORKSPACE_BYTES(B, M, H), 16-byte aligned: the pairs (32 B M), the block records (16 B ceil(H / 1024)), the headers
// (16 B).  -2: arguments out of range, -3: a grid would pass 2^31 - 1
int ransac_launch(const float* source, const float* target, const int* corr, float r2, double s2, int H, int refine_passes,
                  unsigned long long seed, double* transformation, float* fitness, float* inlier_rmse, int* n_pairs, int* best, int* status,
                  int* inliers, int* hyp_triple, int* hyp_count, double* hyp_sum, const double* candidates, void* ws, int B, int M, int N,
                  hipStream_t st) {
    if (B < 1 || M < 1 || N < 1 || H < 1 || H > GECCO_RANSAC_MAX_HYPOTHESES || refine_passes < 0 || refine_passes > GECCO_RANSAC_MAX_REFINE ||
        !ws)
        return -2;
    const int bpc = (H + RANSAC_BLOCK_H - 1) / RANSAC_BLOCK_H;
    if ((long long)B * bpc > 0x7fffffffLL) return -3;
    f32x4* pairs = static_cast<f32x4*>(ws);
    ConsensusRecord* records = reinterpret_cast<ConsensusRecord*>(pairs + (size_t)B * M * 2);
    int* header = reinterpret_cast<int*>(records + (size_t)B * bpc);
    hipLaunchKernelGGL(ransac_pairs_kernel, dim3((unsigned)B), dim3(RANSAC_THREADS), 0, st, source, target, corr, pairs, header, n_pairs, M, N);
    hipLaunchKernelGGL(ransac_hyp_kernel, dim3((unsigned)((long long)B * bpc)), dim3(RANSAC_THREADS), 0, st, pairs, header, candidates, r2, s2,
                       seed, records, hyp_triple, hyp_count, hyp_sum, H, M, bpc);
    hipLaunchKernelGGL(ransac_select_kernel, dim3((unsigned)B), dim3(RANSAC_SELECT_THREADS), 0, st, pairs, header, records, candidates, r2,
                       refine_passes, seed, transformation, fitness, inlier_rmse, best, status, inliers, H, M, bpc);
    return (int)hipGetLastError();
}
