// DBSCAN clustering of 3-D clouds on the device (gfx950): "which points belong together", the step PCL and Open3D put behind the voxel
// filter and the outlier filter (Open3D cluster_dbscan, scikit-learn DBSCAN; with min_points = 1 PCL's EuclideanClusterExtraction).  The
// reference has nothing of the kind; the route without this file is an N x N adjacency matrix in torch (10 GB of booleans at 100 000
// points) and a host loop over it.
//
// Definition (gecco_dbscan_f32, include/gecco_hip.h; tests/_dbscan_ref.py restates it in numpy float32).  Per cloud, with eps2 =
// fp32(eps * eps) from the host: dist2(i, j) is cloud_dist2_inf of cloud_nn.h ((dx dx + dy dy) + dz dz, every operation rounded to fp32,
// none contracted, NaN -> +inf; bitwise symmetric; a point with a non-finite coordinate is nobody's neighbour, not even its own).
// j is a neighbour of i when dist2(i, j) <= eps2 (inclusive; a finite point is its own neighbour); count_i = the number of neighbours;
// core: count_i >= min_points.  The core points form a graph with an edge between neighbours; root_i = the lowest index of i's
// connected component; the cluster id of a component is the rank of its root among all roots, ascending.  A non-core point with a core
// neighbour (border) takes the lowest cluster id among its core neighbours, which is that of the lowest root; everything else is noise, -1.
// The result is unique, and it is the labelling Open3D and scikit-learn produce (both visit points in index order and finish a cluster
// before they open the next).
//
// Two forms, one definition and one forest.  They differ only in how the three passes that ask "who is within eps of i" (count, hook,
// border) find their candidates: the direct form (gecco_dbscan_f32) scans the whole cloud, the grid form (gecco_dbscan_grid_f32) walks
// the cells of a grid index (grid.hip) that the ball can reach.  The cells only filter: membership is cloud_dist2_bits(q, p) <=
// eps2_bits in both, so all six outputs are the same bits, rounds and the labels of a run stopped by the round limit included.
//
// Launches: 1 + 2 R + 2 (direct) or 2 + 2 R + 2 (grid) for R = max_rounds, whatever the data; no host synchronisation, no allocation, so
// a call can be captured in a graph.  Both forms run them through one driver (dbscan_drive); a form supplies how a pass is launched.
//   init           grid form only, in index order: parent_i = DBSCAN_NONE, hook_i = i, root_i = -1, count_i = 0, the round flags cleared
//   count          scan / walk: count_i; parent_i = i for a core point, DBSCAN_NONE (above every index) for a non-core one; in the
//                  direct form also hook_i = i and the cloud's round flags cleared
//   R x hook       scan / walk: Shiloach-Vishkin with minimum hooking.  Before a round the forest is a set of stars (parent[parent[i]]
//                  == parent[i]).  A core i takes m_i = the minimum of parent[j] over its core neighbours j; when m_i < parent[i] it does
//                  an integer atomicMin of m_i into hook[parent[i]] and sets the cloud's flag of this round
//       compress   every core point chases hook from its parent to a fixed point (hook[r] <= r, so the walk descends and ends) and
//                  writes the new parent: stars again.  It also resets the other hook buffer to hook_i = i for the next round
//   border         scan / walk: a core point writes its root (= its parent); a non-core point the minimum root over its core neighbours
//                  or -1
//   label          one workgroup per cloud: the exclusive prefix count of "root_i == i" over the point index numbers the clusters;
//                  labels, n_clusters, rounds and status
// A round whose hook pass set no flag has found the fixed point: its compress and every later workgroup of that cloud return at once,
// uniformly per workgroup (the stopped cloud of icp.hip).  rounds = the number of rounds run, that one included, status 0; a cloud whose
// every one of the R rounds hooked has rounds = R and status 1, and its labels describe the forest as it stood: a refinement of the
// true clusters.
//
// Determinism.  In every launch each buffer that a thread reads is written by no thread of that launch; the exceptions are the
// atomicMin target and the round's flag, which no thread of that launch reads.  So the parents ping-pong between two buffers (round r
// reads buffer r & 1 and writes the other one; a cloud that stopped in round k, or ran out of rounds with k = R, has its forest in
// buffer k & 1, which every workgroup of the border launch works out from the flags), and so do the hook words (compress of round r
// prepares buffer (r + 1) & 1).  A minimum of integers does not depend on arrival order, nor on the order in which a thread meets its
// neighbours, so the state after a round is a pure function of the state before it, the same function in both forms: rounds, and the
// labels of a run that hit the limit, are the same bits run to run, in any batch position, at any workgroup size and through any index.
// The label launch is the one place where a workgroup reads what it wrote itself, the ranks of the roots, on the two sides of a
// barrier; no other workgroup touches that cloud's words.  No float atomics, integer atomicMin in global memory only.
//
// The direct scan is the loop of knn_scan_kernel (cloud_nn.h says why it is written out per kernel rather than shared): one thread per
// point, the cloud streamed through LDS in tiles of CLOUD_TILE as (x, y, z, w), the next tile prefetched into registers, four candidates
// per step and one branch.  Here w, which knn leaves 0, carries the integer the pass needs (parent[j]), and the three scans are one loop
// with the pass as a template argument.  The queries are the cloud itself (M = N), so the grid B * ceil(N / T) fills the device wherever
// the N * N work is worth filling it for.
//
// The grid walk is grid_walk of grid_walk.h, the one grid.hip and iss.hip call, where it is proved to miss no neighbour and every loop
// is bounded; the three walks are one kernel with the pass as a template argument, which takes the index as one GridView by value (made
// by grid_walk.h's grid_view of the launcher's GridIndexArgs, kernels.h) and runs, as iss.hip's kernels do, one thread per SORTED
// POSITION, whose 16-byte load gives the coordinates and, in .w, the original index i.  Every workspace array stays indexed
// by the original index, so compress and label are the direct form's kernels: a neighbour's parent is a 4-byte gather by the index in
// the visited entry's .w, made only for entries inside the ball.  The index is the caller's memory: i and every gathered j are checked
// against N before they address anything, and the init launch writes every word a later kernel reads, so whatever `sorted` holds (not a
// permutation, say) compress and label chase in-range values only.  With a real index each point is owned by exactly one thread and the
// init values of count, parent and root are all overwritten.  The walks take 32 (count), 36 (hook) and 38 (border) VGPRs at every
// workgroup size, no LDS and no scratch.
#include "cloud_nn.h"
#include "grid_walk.h"
#include "kernels.h"
#include "launch_state.h"

namespace {

constexpr int DBSCAN_NONE = 0x7fffffff;      // "no parent": above every index
constexpr int DBSCAN_THREADS = 256;          // compress
constexpr int DBSCAN_LABEL_THREADS = 1024;   // label: one workgroup per cloud
constexpr int DBSCAN_LABEL_ITEMS = 4;        // consecutive points per thread and scan step: chunks of 4096 points
enum { DBSCAN_COUNT = 0, DBSCAN_HOOK = 1, DBSCAN_BORDER = 2 };

// the number of rounds of cloud b that hooked something, k: its forest is in parent buffer k & 1.  k < R: round k found the fixed point
static __device__ __forceinline__ int dbscan_hooked_rounds(const int* __restrict__ flags, int b, int R) {
    const int* f = flags + (size_t)b * R;
    int k = 0;
    while (k < R && f[k] != 0) ++k;
    return k;
}

// grid: B * tiles blocks of T points.  COUNT: out = parent buffer 0.  HOOK (round `round`): out = hook buffer round & 1.  BORDER: out = root
template <int T, int PASS>
__global__ __launch_bounds__(T) void dbscan_scan_kernel(const float* __restrict__ points, const int* __restrict__ par0, const int* __restrict__ par1,
                                                        int* __restrict__ out, int* __restrict__ hook0, int* __restrict__ count,
                                                        int* __restrict__ flags, unsigned eps2_bits, int min_points, int N, int tiles, int R,
                                                        int round) {
    __shared__ __attribute__((aligned(16))) f32x4 tile[CLOUD_TILE];

    const int tid = threadIdx.x;
    const int qt = (int)(blockIdx.x % (unsigned)tiles), b = (int)(blockIdx.x / (unsigned)tiles);
    int sel = 0;
    if (PASS == DBSCAN_HOOK) {
        if (round > 0 && flags[(size_t)b * R + round - 1] == 0) return;   // the cloud has stopped (uniform: no barrier is left behind)
        sel = round & 1;
    }
    if (PASS == DBSCAN_BORDER) sel = dbscan_hooked_rounds(flags, b, R) & 1;
    const int* par = PASS == DBSCAN_COUNT ? nullptr : (sel ? par1 : par0) + (size_t)b * N;
    const float* rb = points + (size_t)b * N * 3;
    const unsigned hi = (unsigned)N;
    const int i = qt * T + tid;
    const bool valid = i < N;
    const float* qp = rb + 3 * (size_t)(valid ? i : 0);
    const float qx = qp[0], qy = qp[1], qz = qp[2];
    const int own = PASS == DBSCAN_COUNT ? 0 : par[valid ? i : 0];
    // who walks the cloud: every point counts; a core point hooks; a non-core point looks for its border root
    const bool scans = valid && (PASS == DBSCAN_COUNT || (PASS == DBSCAN_HOOK ? own != DBSCAN_NONE : own == DBSCAN_NONE));
    int acc = PASS == DBSCAN_COUNT ? 0 : DBSCAN_NONE;   // the neighbour count, or the minimum parent over the core neighbours

    if (PASS == DBSCAN_COUNT && qt == 0)
        for (int r = tid; r < R; r += T) flags[(size_t)b * R + r] = 0;

    constexpr int PPT = CLOUD_TILE / T;
    float rx[PPT], ry[PPT], rz[PPT];
    int rw[PPT];
    auto fetch = [&](unsigned base) {
#pragma unroll
        for (int p = 0; p < PPT; ++p) {
            const unsigned j = base + (unsigned)(tid + p * T);
            const bool in = j < hi;
            rx[p] = in ? rb[3 * (size_t)j] : 0.f;
            ry[p] = in ? rb[3 * (size_t)j + 1] : 0.f;
            rz[p] = in ? rb[3 * (size_t)j + 2] : 0.f;
            rw[p] = PASS == DBSCAN_COUNT ? 0 : in ? par[j] : DBSCAN_NONE;
        }
    };
    auto single = [&](unsigned u, const f32x4 e) {
        if (u <= eps2_bits) acc = PASS == DBSCAN_COUNT ? acc + 1 : min(acc, __float_as_int(e[3]));   // (a move of bits, no arithmetic)
    };

    fetch(0);
    for (unsigned base = 0; base < hi; base += CLOUD_TILE) {
        __syncthreads();   // the scan of the previous tile is over
#pragma unroll
        for (int p = 0; p < PPT; ++p) tile[tid + p * T] = f32x4{rx[p], ry[p], rz[p], __int_as_float(rw[p])};
        __syncthreads();
        if (base + CLOUD_TILE < hi) fetch(base + CLOUD_TILE);
        if (!scans) continue;
        const int cnt = (int)min((unsigned)CLOUD_TILE, hi - base);   // entries past cnt are never candidates
        int g = 0;
        for (; g + 4 <= cnt; g += 4) {
            const f32x4 e0 = tile[g], e1 = tile[g + 1], e2 = tile[g + 2], e3 = tile[g + 3];
            const unsigned u0 = cloud_dist2_bits(qx, qy, qz, e0), u1 = cloud_dist2_bits(qx, qy, qz, e1);
            const unsigned u2 = cloud_dist2_bits(qx, qy, qz, e2), u3 = cloud_dist2_bits(qx, qy, qz, e3);
            if (min(min(u0, u1), min(u2, u3)) <= eps2_bits) {   // dist2 >= 0 or +inf: its bits order as unsigned integers
                single(u0, e0);
                single(u1, e1);
                single(u2, e2);
                single(u3, e3);
            }
        }
        for (; g < cnt; ++g) {
            const f32x4 e = tile[g];
            single(cloud_dist2_bits(qx, qy, qz, e), e);
        }
    }
    if (!valid) return;
    const size_t o = (size_t)b * N + i;
    if (PASS == DBSCAN_COUNT) {
        if (count) count[o] = acc;
        out[o] = acc >= min_points ? i : DBSCAN_NONE;
        hook0[o] = i;
    } else if (PASS == DBSCAN_HOOK) {
        if (scans && acc < own) {   // own is a root of the star forest and a core point: an index of this cloud
            atomicMin(out + (size_t)b * N + own, acc);
            flags[(size_t)b * R + round] = 1;
        }
    } else {
        out[o] = own != DBSCAN_NONE ? own : acc == DBSCAN_NONE ? -1 : acc;
    }
}

// grid: B * chunks blocks of DBSCAN_THREADS points.  The grid form's first launch: every word compress, the walks and label read
__global__ __launch_bounds__(DBSCAN_THREADS) void dbscan_grid_init_kernel(int* __restrict__ par0, int* __restrict__ hook0, int* __restrict__ root,
                                                                          int* __restrict__ count, int* __restrict__ flags, int N, int chunks,
                                                                          int R) {
    const int b = (int)(blockIdx.x / (unsigned)chunks), chunk = (int)(blockIdx.x % (unsigned)chunks);
    if (chunk == 0)
        for (int r = threadIdx.x; r < R; r += DBSCAN_THREADS) flags[(size_t)b * R + r] = 0;
    const int i = chunk * DBSCAN_THREADS + (int)threadIdx.x;
    if (i >= N) return;   // (no barrier below)
    const size_t o = (size_t)b * N + i;
    par0[o] = DBSCAN_NONE;
    hook0[o] = i;
    root[o] = -1;
    if (count) count[o] = 0;
}

// grid: B * tiles blocks of T sorted positions.  COUNT: out = parent buffer 0.  HOOK (round `round`): out = hook buffer round & 1.
// BORDER: out = root.  The passes of dbscan_scan_kernel, the neighbours found by grid_walk; acc, own and who walks are the same
template <int T, int PASS>
__global__ __launch_bounds__(T) void dbscan_grid_kernel(const GridView index, float reach, unsigned eps2_bits, const int* __restrict__ par0,
                                                        const int* __restrict__ par1, int* __restrict__ out, int* __restrict__ count,
                                                        int* __restrict__ flags, int min_points, int tiles, int R, int round) {
    const int N = index.N;
    const int b = (int)(blockIdx.x / (unsigned)tiles);
    int sel = 0;
    if (PASS == DBSCAN_HOOK) {
        if (round > 0 && flags[(size_t)b * R + round - 1] == 0) return;   // the cloud has stopped (uniform)
        sel = round & 1;
    }
    if (PASS == DBSCAN_BORDER) sel = dbscan_hooked_rounds(flags, b, R) & 1;
    const int t = (int)(blockIdx.x % (unsigned)tiles) * T + (int)threadIdx.x;
    if (t >= N) return;   // (no barrier below)
    const f32x4 q = index.cloud(b)[t];
    const unsigned i = __float_as_uint(q[3]);
    if (i >= (unsigned)N) return;   // a sorted array no build wrote: the init launch's words stand
    const size_t o = (size_t)b * N;
    const int* par = PASS == DBSCAN_COUNT ? nullptr : (sel ? par1 : par0) + o;
    const int own = PASS == DBSCAN_COUNT ? 0 : par[i];
    // who walks: every finite point counts; a core point hooks; a non-core point looks for its border root
    const bool walks = cloud_finite3(q[0], q[1], q[2]) && (PASS == DBSCAN_COUNT || (PASS == DBSCAN_HOOK ? own != DBSCAN_NONE : own == DBSCAN_NONE));
    int acc = PASS == DBSCAN_COUNT ? 0 : DBSCAN_NONE;   // the neighbour count, or the minimum parent over the core neighbours
    if (walks)
        grid_walk(index, b, q[0], q[1], q[2], reach, eps2_bits, [&](const f32x4 p, unsigned) {
            if (PASS == DBSCAN_COUNT) {
                ++acc;
            } else {
                const unsigned j = __float_as_uint(p[3]);
                if (j < (unsigned)N) acc = min(acc, par[j]);   // a 4-byte gather, for entries inside the ball only
            }
        });
    if (PASS == DBSCAN_COUNT) {
        if (count) count[o + i] = acc;
        out[o + i] = acc >= min_points ? (int)i : DBSCAN_NONE;
    } else if (PASS == DBSCAN_HOOK) {
        if (walks && acc < own) {   // own is a parent the init, count or compress launch wrote and not NONE: an index of this cloud
            atomicMin(out + o + own, acc);
            flags[(size_t)b * R + round] = 1;
        }
    } else {
        out[o + i] = own != DBSCAN_NONE ? own : acc == DBSCAN_NONE ? -1 : acc;
    }
}

// grid: B * chunks blocks of DBSCAN_THREADS points.  Round `round`: reads parent and hook buffer round & 1, writes the other two
__global__ __launch_bounds__(DBSCAN_THREADS) void dbscan_compress_kernel(const int* __restrict__ par_in, const int* __restrict__ hook_in,
                                                                         int* __restrict__ par_out, int* __restrict__ hook_out,
                                                                         const int* __restrict__ flags, int N, int chunks, int R, int round) {
    const int b = (int)(blockIdx.x / (unsigned)chunks);
    if (flags[(size_t)b * R + round] == 0) return;   // nothing hooked in this round, or the cloud stopped before it (uniform)
    const int i = (int)(blockIdx.x % (unsigned)chunks) * DBSCAN_THREADS + (int)threadIdx.x;
    if (i >= N) return;   // (no barrier below)
    const size_t o = (size_t)b * N;
    int p = par_in[o + i];
    if (p != DBSCAN_NONE) {
        for (;;) {   // hook[r] <= r with equality at a fixed point: a descending walk over indices of this cloud
            const int h = hook_in[o + p];
            if (h >= p) break;
            p = h;
        }
    }
    par_out[o + i] = p;
    hook_out[o + i] = i;
}

// grid: B blocks.  Point i is a root when root[i] == i; the exclusive scan of that flag over i is the cluster id.  `rank` (the words of hook
// buffer 0, dead by now) takes the ids of the roots; the same workgroup reads them back behind a barrier.
__global__ __launch_bounds__(DBSCAN_LABEL_THREADS) void dbscan_label_kernel(const int* __restrict__ root, int* rank, const int* __restrict__ flags,
                                                                            int* __restrict__ labels, int* __restrict__ n_clusters,
                                                                            int* __restrict__ rounds, int* __restrict__ status, int N, int R) {
    constexpr int WAVES = DBSCAN_LABEL_THREADS / GECCO_WAVE;
    __shared__ int wave_sum[WAVES];
    __shared__ int chunk_sum;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (GECCO_WAVE - 1), wave = tid / GECCO_WAVE;
    const int* rt = root + (size_t)b * N;
    int* rk = rank + (size_t)b * N;
    int base = 0;   // clusters before this chunk (the same in every thread)
    for (long long lo = 0; lo < N; lo += DBSCAN_LABEL_THREADS * DBSCAN_LABEL_ITEMS) {
        bool is_root[DBSCAN_LABEL_ITEMS];
        int mine = 0;
#pragma unroll
        for (int j = 0; j < DBSCAN_LABEL_ITEMS; ++j) {
            const long long i = lo + tid * DBSCAN_LABEL_ITEMS + j;
            is_root[j] = i < N && rt[i] == (int)i;
            mine += is_root[j] ? 1 : 0;
        }
        int incl = mine;   // inclusive scan over the wave, then over the waves
#pragma unroll
        for (int d = 1; d < GECCO_WAVE; d <<= 1) {
            const int up = __shfl_up(incl, d, GECCO_WAVE);
            if (lane >= d) incl += up;
        }
        if (lane == GECCO_WAVE - 1) wave_sum[wave] = incl;
        __syncthreads();
        if (wave == 0) {
            const int own = lane < WAVES ? wave_sum[lane] : 0;
            int s = own;
#pragma unroll
            for (int d = 1; d < WAVES; d <<= 1) {
                const int up = __shfl_up(s, d, GECCO_WAVE);
                if (lane >= d) s += up;
            }
            if (lane < WAVES) wave_sum[lane] = s - own;   // exclusive
            if (lane == WAVES - 1) chunk_sum = s;
        }
        __syncthreads();
        int id = base + wave_sum[wave] + incl - mine;
        base += chunk_sum;
#pragma unroll
        for (int j = 0; j < DBSCAN_LABEL_ITEMS; ++j)
            if (is_root[j]) rk[lo + tid * DBSCAN_LABEL_ITEMS + j] = id++;
        __syncthreads();   // wave_sum and chunk_sum are rewritten by the next chunk
    }
    if (tid == 0) {
        const int k = dbscan_hooked_rounds(flags, b, R);
        n_clusters[b] = base;
        if (rounds) rounds[b] = k < R ? k + 1 : R;
        status[b] = k < R ? 0 : 1;
    }
    __threadfence_block();
    __syncthreads();   // every root's rank is written and visible to this workgroup
    for (int i = tid; i < N; i += DBSCAN_LABEL_THREADS) {
        const int r = rt[i];   // -1, or a root of this cloud: rank[r] was written above
        labels[(size_t)b * N + i] = r < 0 ? -1 : rk[r];
    }
}

// ws of GECCO_DBSCAN_WORKSPACE_BYTES(B, N, R), as both forms carve it: two parent buffers, two hook buffers and the roots, (B, N) int32
// each, then the round flags (B, R)
struct DbscanCarve {
    int *par[2], *hook[2], *root, *flags;
    DbscanCarve(void* ws, int B, int N) {
        const size_t pts = (size_t)B * N;
        int* w = static_cast<int*>(ws);
        par[0] = w, par[1] = w + pts;
        hook[0] = w + 2 * pts, hook[1] = w + 3 * pts;
        root = w + 4 * pts;
        flags = w + 5 * pts;
        static_assert(GECCO_DBSCAN_WORKSPACE_BYTES(1, 1, 1) == 24, "the carve above is the header's formula");
    }
};

// What both forms test and plan before their first launch: -2 for arguments out of range, -3 when the grid of a neighbourhood pass would
// pass 2^31 - 1 workgroups (T <= DBSCAN_THREADS: the init and compress grids are no larger), 0 with the plan of the passes in p
int dbscan_plan(int B, int N, float eps2, int min_points, int R, const void* ws, CloudPlan& p) {
    if (B < 1 || N < 1 || !(eps2 > 0.f) || !(eps2 <= 3.402823466e38f) || min_points < 1 || R < 0 || R > GECCO_DBSCAN_MAX_ROUNDS || !ws) return -2;
    p = cloud_plan(B, N, N, 1, false, 256, device_cus());
    return p.fits() ? 0 : -3;
}

// The launches of both forms, in the order of the header's table: the count pass, R x (hook pass, compress), the border pass, label.
// pass(kind, out, count, round) launches one neighbourhood pass of the form, kind an integral_constant of DBSCAN_COUNT / HOOK / BORDER
// (the grid form's launches its init kernel ahead of the count pass); the buffers a pass and a compress read and write are chosen here
template <class Pass>
int dbscan_drive(const DbscanCarve& c, int* labels, int* n_clusters, int* count, int* rounds, int* status, int B, int N, int R, int chunks,
                 hipStream_t st, Pass pass) {
    pass(std::integral_constant<int, DBSCAN_COUNT>{}, c.par[0], count, 0);
    for (int r = 0; r < R; ++r) {
        pass(std::integral_constant<int, DBSCAN_HOOK>{}, c.hook[r & 1], nullptr, r);
        hipLaunchKernelGGL(dbscan_compress_kernel, dim3((unsigned)(B * chunks)), dim3(DBSCAN_THREADS), 0, st, (const int*)c.par[r & 1],
                           (const int*)c.hook[r & 1], c.par[(r + 1) & 1], c.hook[(r + 1) & 1], (const int*)c.flags, N, chunks, R, r);
        const int rc = (int)hipGetLastError();
        if (rc) return rc;
    }
    pass(std::integral_constant<int, DBSCAN_BORDER>{}, c.root, nullptr, 0);
    hipLaunchKernelGGL(dbscan_label_kernel, dim3((unsigned)B), dim3(DBSCAN_LABEL_THREADS), 0, st, (const int*)c.root, c.hook[0],
                       (const int*)c.flags, labels, n_clusters, rounds, status, N, R);
    return (int)hipGetLastError();
}

}  // namespace

// The direct form: 1 + 2 R + 2 launches.  Returns -2 for arguments out of range, -3 when the grid would pass 2^31 - 1 workgroups.
int dbscan_launch(const float* points, int* labels, int* n_clusters, int* count, int* rounds, int* status, void* ws, int B, int N, float eps2,
                  int min_points, int R, hipStream_t st) {
    CloudPlan p;
    if (const int rc = dbscan_plan(B, N, eps2, min_points, R, ws, p)) return rc;
    const int chunks = (N + DBSCAN_THREADS - 1) / DBSCAN_THREADS;
    const DbscanCarve c(ws, B, N);
    const unsigned eps2_bits = __builtin_bit_cast(unsigned, eps2);
    return dispatch_T(p.T, [&](auto t) -> int {
        constexpr int T = decltype(t)::value;
        return dbscan_drive(c, labels, n_clusters, count, rounds, status, B, N, R, chunks, st, [&](auto pass, int* out, int* cnt, int round) {
            constexpr bool first = decltype(pass)::value == DBSCAN_COUNT;   // reads no parents, prepares hook buffer 0
            hipLaunchKernelGGL((dbscan_scan_kernel<T, decltype(pass)::value>), dim3((unsigned)p.blocks), dim3(T), 0, st, points,
                               first ? nullptr : (const int*)c.par[0], first ? nullptr : (const int*)c.par[1], out,
                               first ? c.hook[0] : nullptr, cnt, c.flags, eps2_bits, min_points, N, p.tiles, R, round);
        });
    });
}

// The grid form: 2 + 2 R + 2 launches, compress and label the direct form's own.  Returns -2 for arguments out of range (an eps2 above
// fp32(cell_size^2) among them), -3 when the grid would pass 2^31 - 1 workgroups.
int dbscan_grid_launch(const GridIndexArgs& index, int* labels, int* n_clusters, int* count, int* rounds, int* status, void* ws, int B, int N,
                       float eps2, int min_points, int R, hipStream_t st) {
    const GridView g = grid_view(index, B, N);
    if (!g.sorted || !labels || !n_clusters || !status || !grid_radius2_ok(eps2, index.cell_size)) return -2;
    CloudPlan p;
    if (const int rc = dbscan_plan(B, N, eps2, min_points, R, ws, p)) return rc;
    const int chunks = (N + DBSCAN_THREADS - 1) / DBSCAN_THREADS;
    const DbscanCarve c(ws, B, N);
    const unsigned eps2_bits = __builtin_bit_cast(unsigned, eps2);
    const float reach = grid_reach(eps2);
    return dispatch_T(p.T, [&](auto t) -> int {
        constexpr int T = decltype(t)::value;
        return dbscan_drive(c, labels, n_clusters, count, rounds, status, B, N, R, chunks, st, [&](auto pass, int* out, int* cnt, int round) {
            constexpr bool first = decltype(pass)::value == DBSCAN_COUNT;   // reads no parents, follows the init launch
            if (first)
                hipLaunchKernelGGL(dbscan_grid_init_kernel, dim3((unsigned)(B * chunks)), dim3(DBSCAN_THREADS), 0, st, c.par[0], c.hook[0],
                                   c.root, count, c.flags, N, chunks, R);
            hipLaunchKernelGGL((dbscan_grid_kernel<T, decltype(pass)::value>), dim3((unsigned)p.blocks), dim3(T), 0, st, g, reach, eps2_bits,
                               first ? nullptr : (const int*)c.par[0], first ? nullptr : (const int*)c.par[1], out, cnt, c.flags, min_points,
                               p.tiles, R, round);
        });
    });
}
