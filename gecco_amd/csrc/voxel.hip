// Voxel-grid downsampling of 3-D clouds on the device (gfx950): one output point per occupied cell of a regular grid, at the centroid of
// the cell's points, with the point-to-voxel map (first / count / inverse).  The reference has nothing of the kind; the route without
// this file is floor -> unique(dim=0) (a sort over N rows and a synchronisation) -> index_add (float atomics).
//
// Definition (gecco_voxel_downsample_f32, include/gecco_hip.h; tests/_voxel_ref.py restates it in numpy).  Per axis t = fp32(p - o),
// u = fp32(t * inv) with inv = fp32(1 / s) from the host, c = floor(u); a point with a non-finite u or a c outside [-2^20, 2^20) is
// dropped.  key = (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20).  Voxels are the distinct keys, numbered by first occurrence.
// frac = fp32(u - c), q = (uint64) trunc(frac * 2^32), S = the integer sum of q over the voxel, centroid = fp32(double(o) + (double(c) +
// double(S) / (double(count) * 2^32)) * double(s)).  voxel_cell (voxel_cell.h, shared with grid.hip) spells the fp32 roundings out,
// voxel_finalise_kernel the fp64 ones; both with contraction off (u - c would otherwise fuse with the product that made u).
//
// Why a table and integer sums, not a sort.  A sort of N 64-bit keys costs several passes over the cloud and gives an order (by key)
// that nobody asked for; the first-occurrence order wanted here is a scan over the POINT index, which needs no sort at all once every
// point knows whether it is the lowest index of its cell.  That is one atomic minimum per point on the cell's table slot.  Sums of
// 32.32 fixed-point fractions are exact integers, so they do not depend on the order the adds arrive in: the outputs are the same bits
// run to run, in any batch position and for any launch geometry, with no float atomics anywhere.
//
// Workspace (voxel_launch carves it; cap = GECCO_VOXEL_CAPACITY(N) slots per cloud, V = max_voxels):
//     keys   (B, cap) u64   the slot's key, VOXEL_EMPTY = ~0 (no key has bit 63)          filled with ones
//     sfirst (B, cap) u32   the lowest point index that landed in the slot                 filled with ones
//     S      (B, V, 3) u64  the sums of q; vcount (B, V) i32                               filled with zeros
//     svid   (B, cap) i32   the slot's voxel number: written by rank for every occupied slot (each has exactly one first point),
//                           read by accumulate only through the slot of a kept point
//     pslot  (B, N) i32     the slot of each point, -1 for a dropped one: written by insert for every point
//     vfirst (B, V) i32     first[] (the caller's may be null): written by rank for v < min(n_voxels, V), read by finalise there
//     nvox   (B) i32        n_voxels: written by rank
// Five ordinary launches on one stream; no thread waits on another: the probe loop of insert ends at an empty slot or at its own key, and
// a table at load <= 0.5 always holds an empty slot (the loop is bounded by cap all the same).
#include "../../include/gecco_hip.h"
#include "common.h"
#include "kernels.h"
#include "launch_state.h"
#include "voxel_cell.h"

namespace {

constexpr int VOXEL_THREADS = 256;        // insert, accumulate, finalise, fill
constexpr int VOXEL_RANK_THREADS = 1024;  // rank: one workgroup per cloud
constexpr int VOXEL_RANK_ITEMS = 4;       // consecutive points per thread and scan step: chunks of 4096 points

// words [0, ones) = ~0, words [ones, ones + zeros) = 0
__global__ __launch_bounds__(VOXEL_THREADS) void voxel_fill_kernel(unsigned* __restrict__ ws, size_t ones, size_t zeros) {
    const size_t n = ones + zeros, step = (size_t)gridDim.x * VOXEL_THREADS;
    for (size_t w = (size_t)blockIdx.x * VOXEL_THREADS + threadIdx.x; w < n; w += step) ws[w] = w < ones ? 0xffffffffu : 0u;
}

// grid: B * chunks blocks of VOXEL_THREADS points
__global__ __launch_bounds__(VOXEL_THREADS) void voxel_insert_kernel(const float* __restrict__ points, const float* __restrict__ origin, float inv,
                                                                     u64* __restrict__ keys, unsigned* __restrict__ sfirst,
                                                                     int* __restrict__ pslot, int N, unsigned cap, int chunks) {
    const int b = (int)(blockIdx.x / (unsigned)chunks);
    const int i = (int)(blockIdx.x % (unsigned)chunks) * VOXEL_THREADS + (int)threadIdx.x;
    if (i >= N) return;   // (no barrier below)
    const float ox = origin ? origin[3 * b] : 0.f, oy = origin ? origin[3 * b + 1] : 0.f, oz = origin ? origin[3 * b + 2] : 0.f;
    const VoxelCell v = voxel_cell(points + ((size_t)b * N + i) * 3, ox, oy, oz, inv);
    int slot = -1;
    if (v.kept) {
        const u64 key = voxel_key(v);
        u64* kb = keys + (size_t)b * cap;
        const unsigned mask = cap - 1;
        unsigned h = voxel_hash(key, mask);
        for (unsigned probe = 0; probe < cap; ++probe) {   // ends at an empty slot or at this key: at most N of the >= 2 N slots are taken
            const u64 seen = atomicCAS(kb + h, VOXEL_EMPTY, key);
            if (seen == VOXEL_EMPTY || seen == key) {
                slot = (int)h;
                break;
            }
            h = (h + 1) & mask;
        }
        if (slot >= 0) atomicMin(sfirst + (size_t)b * cap + slot, (unsigned)i);
    }
    pslot[(size_t)b * N + i] = slot;
}

// grid: B blocks.  Point i is its voxel's representative when sfirst[slot_i] == i; the exclusive scan of that flag over i is the voxel's
// number in first-occurrence order.
__global__ __launch_bounds__(VOXEL_RANK_THREADS) void voxel_rank_kernel(const int* __restrict__ pslot, const unsigned* __restrict__ sfirst,
                                                                        int* __restrict__ svid, int* __restrict__ vfirst,
                                                                        int* __restrict__ nvox, int* __restrict__ n_voxels, int N,
                                                                        unsigned cap, int V) {
    constexpr int WAVES = VOXEL_RANK_THREADS / GECCO_WAVE;
    __shared__ int wave_sum[WAVES];
    __shared__ int chunk_sum;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (GECCO_WAVE - 1), wave = tid / GECCO_WAVE;
    const int* ps = pslot + (size_t)b * N;
    const unsigned* sf = sfirst + (size_t)b * cap;
    int* sv = svid + (size_t)b * cap;
    int base = 0;   // voxels before this chunk (the same in every thread)
    for (long long lo = 0; lo < N; lo += VOXEL_RANK_THREADS * VOXEL_RANK_ITEMS) {
        int slot[VOXEL_RANK_ITEMS], mine = 0;
        bool rep[VOXEL_RANK_ITEMS];
#pragma unroll
        for (int j = 0; j < VOXEL_RANK_ITEMS; ++j) {
            const long long i = lo + tid * VOXEL_RANK_ITEMS + j;
            slot[j] = i < N ? ps[i] : -1;
        }
#pragma unroll
        for (int j = 0; j < VOXEL_RANK_ITEMS; ++j) {
            const long long i = lo + tid * VOXEL_RANK_ITEMS + j;
            rep[j] = slot[j] >= 0 && sf[slot[j]] == (unsigned)i;
            mine += rep[j] ? 1 : 0;
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
        int vid = base + wave_sum[wave] + incl - mine;
        base += chunk_sum;
#pragma unroll
        for (int j = 0; j < VOXEL_RANK_ITEMS; ++j) {
            if (rep[j]) {
                const int i = (int)(lo + tid * VOXEL_RANK_ITEMS + j);
                sv[slot[j]] = vid;
                if (vid < V) vfirst[(size_t)b * V + vid] = i;
                ++vid;
            }
        }
        __syncthreads();   // wave_sum and chunk_sum are rewritten by the next chunk
    }
    if (tid == 0) {
        nvox[b] = base;
        n_voxels[b] = base;
    }
}

// grid: B * chunks blocks of VOXEL_THREADS points.  Lanes of a wave that follow each other into the same voxel (a run) are summed by a
// segmented scan first and the run's last lane issues the four integer adds: a cloud that lies in one voxel costs four atomics per
// wave, not four per point, and a spatially ordered cloud a few per wave.
__global__ __launch_bounds__(VOXEL_THREADS) void voxel_accumulate_kernel(const float* __restrict__ points, const float* __restrict__ origin,
                                                                         float inv, const int* __restrict__ pslot, const int* __restrict__ svid,
                                                                         u64* __restrict__ S, int* __restrict__ vcount, int* __restrict__ inverse,
                                                                         int N, unsigned cap, int V, int chunks) {
    const int b = (int)(blockIdx.x / (unsigned)chunks);
    const int i = (int)(blockIdx.x % (unsigned)chunks) * VOXEL_THREADS + (int)threadIdx.x;
    const int lane = (int)threadIdx.x & (GECCO_WAVE - 1);
    int vid = -1;   // no voxel: past the cloud, dropped, or a voxel numbered V or higher
    u64 q0 = 0, q1 = 0, q2 = 0;
    if (i < N) {
        const int slot = pslot[(size_t)b * N + i];
        if (slot >= 0) {
            const int v = svid[(size_t)b * cap + slot];
            if (v < V) {
                vid = v;
                const float ox = origin ? origin[3 * b] : 0.f, oy = origin ? origin[3 * b + 1] : 0.f, oz = origin ? origin[3 * b + 2] : 0.f;
                const VoxelCell c = voxel_cell(points + ((size_t)b * N + i) * 3, ox, oy, oz, inv);
                q0 = c.q[0], q1 = c.q[1], q2 = c.q[2];
            }
        }
        if (inverse) inverse[(size_t)b * N + i] = vid;
    }
    // runs of equal vid among neighbouring lanes (every lane of the wave takes part in the shuffles)
    const int before = __shfl_up(vid, 1, GECCO_WAVE), after = __shfl_down(vid, 1, GECCO_WAVE);
    const bool head = lane == 0 || before != vid;
    const bool tail = lane == GECCO_WAVE - 1 || after != vid;
    const u64 heads = __ballot(head);
    const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));   // the run's first lane (lane 0 is always a head)
#pragma unroll
    for (int d = 1; d < GECCO_WAVE; d <<= 1) {
        const u64 u0 = __shfl_up(q0, d, GECCO_WAVE), u1 = __shfl_up(q1, d, GECCO_WAVE), u2 = __shfl_up(q2, d, GECCO_WAVE);
        if (lane - d >= start) q0 += u0, q1 += u1, q2 += u2;
    }
    if (tail && vid >= 0) {
        const size_t row = (size_t)b * V + vid;
        atomicAdd(vcount + row, lane - start + 1);
        atomicAdd(S + row * 3, q0);
        atomicAdd(S + row * 3 + 1, q1);
        atomicAdd(S + row * 3 + 2, q2);
    }
}

// grid: ceil(B * V / VOXEL_THREADS) blocks, one thread per output row; the fp64 roundings of the definition
__global__ __launch_bounds__(VOXEL_THREADS) void voxel_finalise_kernel(const float* __restrict__ points, const float* __restrict__ origin, float s,
                                                                       float inv, const u64* __restrict__ S, const int* __restrict__ vcount,
                                                                       const int* __restrict__ vfirst, const int* __restrict__ nvox,
                                                                       float* __restrict__ centroids, int* __restrict__ first,
                                                                       int* __restrict__ count, int N, int V, size_t rows) {
#pragma clang fp contract(off)
    const size_t row = (size_t)blockIdx.x * VOXEL_THREADS + threadIdx.x;
    if (row >= rows) return;
    const int b = (int)(row / (size_t)V), v = (int)(row % (size_t)V);
    float cx = 0.f, cy = 0.f, cz = 0.f;
    int f = -1, n = 0;
    if (v < nvox[b]) {
        f = vfirst[row];
        n = vcount[row];
        const float o[3] = {origin ? origin[3 * b] : 0.f, origin ? origin[3 * b + 1] : 0.f, origin ? origin[3 * b + 2] : 0.f};
        const VoxelCell c = voxel_cell(points + ((size_t)b * N + f) * 3, o[0], o[1], o[2], inv);
        const double den = (double)n * 4294967296.0;
        float out[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double mean = (double)S[row * 3 + a] / den;
            const double inside = (double)c.c[a] + mean;
            const double scaled = inside * (double)s;
            out[a] = (float)((double)o[a] + scaled);
        }
        cx = out[0], cy = out[1], cz = out[2];
    }
    centroids[row * 3] = cx;
    centroids[row * 3 + 1] = cy;
    centroids[row * 3 + 2] = cz;
    if (first) first[row] = f;
    if (count) count[row] = n;
}

}  // namespace

// Five launches.  Returns -2 for sizes out of range, -3 when a grid would pass 2^31 - 1 workgroups.
int voxel_launch(const float* points, const float* origin, float voxel_size, float* centroids, int* first, int* count, int* inverse,
                 int* n_voxels, void* ws, int B, int N, int V, hipStream_t st) {
    if (B < 1 || N < 1 || N > GECCO_VOXEL_MAX_POINTS || V < 1 || V > N) return -2;
    const int chunks = (N + VOXEL_THREADS - 1) / VOXEL_THREADS;
    const size_t rows = (size_t)B * V;
    if ((long long)B * chunks > 0x7fffffffLL || (rows + VOXEL_THREADS - 1) / VOXEL_THREADS > 0x7fffffffull) return -3;
    const size_t cap = GECCO_VOXEL_CAPACITY(N), slots = (size_t)B * cap, pts = (size_t)B * N;
    const float inv = 1.0f / voxel_size;   // fp32, once, on the host

    char* w = static_cast<char*>(ws);
    u64* keys = reinterpret_cast<u64*>(w);
    unsigned* sfirst = reinterpret_cast<unsigned*>(w + 8 * slots);
    u64* S = reinterpret_cast<u64*>(w + 12 * slots);   // cap is even: 8-byte aligned
    int* vcount = reinterpret_cast<int*>(w + 12 * slots + 24 * rows);
    int* svid = reinterpret_cast<int*>(w + 12 * slots + 28 * pts);   // (S and vcount are carved for V = N)
    int* pslot = svid + slots;
    int* vfirst = pslot + pts;
    int* nvox = vfirst + pts;
    static_assert(GECCO_VOXEL_WORKSPACE_BYTES(1, 1) == ((16 * 2 + 36 + 4 + 7) & ~7), "the carve above is the header's formula");

    const size_t ones = 3 * slots, zeros = 7 * rows;   // 4-byte words: keys | sfirst, then S | vcount
    const size_t fill_blocks = (ones + zeros + VOXEL_THREADS - 1) / VOXEL_THREADS;
    const size_t fill_cap = (size_t)device_cus() * 8;
    hipLaunchKernelGGL(voxel_fill_kernel, dim3((unsigned)(fill_blocks < fill_cap ? fill_blocks : fill_cap)), dim3(VOXEL_THREADS), 0, st,
                       reinterpret_cast<unsigned*>(w), ones, zeros);
    hipLaunchKernelGGL(voxel_insert_kernel, dim3((unsigned)(B * chunks)), dim3(VOXEL_THREADS), 0, st, points, origin, inv, keys, sfirst, pslot,
                       N, (unsigned)cap, chunks);
    hipLaunchKernelGGL(voxel_rank_kernel, dim3((unsigned)B), dim3(VOXEL_RANK_THREADS), 0, st, pslot, sfirst, svid, vfirst, nvox, n_voxels, N,
                       (unsigned)cap, V);
    hipLaunchKernelGGL(voxel_accumulate_kernel, dim3((unsigned)(B * chunks)), dim3(VOXEL_THREADS), 0, st, points, origin, inv, pslot, svid, S,
                       vcount, inverse, N, (unsigned)cap, V, chunks);
    hipLaunchKernelGGL(voxel_finalise_kernel, dim3((unsigned)((rows + VOXEL_THREADS - 1) / VOXEL_THREADS)), dim3(VOXEL_THREADS), 0, st, points,
                       origin, voxel_size, inv, S, vcount, vfirst, nvox, centroids, first, count, N, V, rows);
    return (int)hipGetLastError();
}
