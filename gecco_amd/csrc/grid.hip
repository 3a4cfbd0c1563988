// A uniform-grid index for the fixed-radius neighbour search (gfx950): radius.hip answers "every point within r" by walking the whole
// reference cloud for every query (100 000 candidates per query at 100 000 points); with the cloud sorted into cells of edge >= r a
// query looks at the few cells its ball can reach (about 250 candidates at DESIGN.md's shape) and at nothing else.  The results are
// radius.hip's, element for element and bit for bit: the cells only choose which candidates are tested, the test itself is unchanged.
//
// Definition (gecco_grid_keys_f32 / gecco_grid_build_f32 / gecco_grid_radius_count_f32 / gecco_grid_radius_search_f32,
// include/gecco_hip.h; tests/_grid_ref.py restates it in numpy float32).
//   cell     voxel.hip's, for voxel_size = cell_size (voxel_cell.h): per axis t = fp32(p - o), u = fp32(t * inv), c = floor(u), with
//            inv = fp32(1 / cell_size) from the host; key = (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20).  A point with a
//            non-finite u or a c outside [-2^20, 2^20) is OFF-GRID: its key is GRID_OFF = 2^63 (no real key has bit 63)
//   order    the caller sorts the keys of a cloud as UNSIGNED integers, stably: cells ascend in key, a cell's points in original index,
//            the off-grid points come last (the tail), also in original index.  perm[s] = the original index at sorted position s
//   build    from position s: sorted[s] = (x, y, z, bits of perm[s]) as one 16-byte store; at a run's first position (key[s] != key[s-1])
//            and at its last (key[s] != key[s+1]) the key is found or inserted in the cloud's open-addressing table of cap =
//            GECCO_GRID_CAPACITY(N) slots (the power of two >= 2 N: load <= 0.5) by atomicCAS on the key word, voxel_insert_kernel's
//            loop, idempotent for a key that is there, and range[slot] takes the run's start or end; n_in_grid = where the tail starts.
//            No thread waits on another; the probe loop ends at an empty slot or at its own key and is bounded by cap all the same
//   query    one thread per query q.  With R the host's fp32 reach (below), per axis the cells lo = cell(fp32(q - R)) .. hi =
//            cell(fp32(q + R)), same u and floor, clamped to the grid; the box is walked with x outermost and z innermost, which is
//            ascending key order; every occupied cell's run sorted[start .. end) is scanned, then the tail sorted[n_in_grid .. N).
//            j is a neighbour when cloud_dist2_bits(q, p_j) <= r2_bits (radius.hip's predicate on radius.hip's bits); self mode skips
//            j == i by the original index carried in .w.  COUNT writes count[b, i]; FILL_CSR writes neighbour t of row r to
//            idx[row_start[r] + t] (d2 likewise) in scan order: ascending position in the sorted order
// A thread writes its own words only: no atomics in the query, no workspace, no thread reads what another writes; the outputs are the
// same bits run to run and in any batch position (which slot a key takes in the table may differ from run to run; what a query finds
// there does not).  With qorder (a permutation of the queries, by cell) thread t answers query qorder[t] and writes THAT query's row:
// the lanes of a wave probe the same cells and read the same runs, which the L2 then serves once.
//
// The walk itself (the reach, the box, the probe, the runs, the tail, the scan of the whole cloud for a box wider than GRID_BOX cells) is
// grid_walk of grid_walk.h, which iss.hip's and dbscan.hip's kernels call as well; that header proves that the walk misses no neighbour
// and bounds every loop.  The built index reaches a launcher as one GridIndexArgs (kernels.h), of which grid_walk.h's grid_view makes
// the GridView the walk reads (the tests, the casts, inv and cap); grid_query_kernel is handed that view's members (its own comment).
//
// The radius may not exceed the cell edge; an index serves every smaller radius (at r = cell_size / 2 the 27 to 64 cells hold 8 times
// the candidates that cells of edge r would: build another index when that matters).  The fixed-width forms stay on radius.hip.
#include <cmath>

#include "cloud_nn.h"
#include "grid_walk.h"
#include "kernels.h"
#include "launch_state.h"
#include "voxel_cell.h"

namespace {

constexpr u64 GRID_OFF = 1ull << 63;   // the key of an off-grid point: above every real key as an unsigned integer
constexpr int GRID_THREADS = 256;      // keys, build, fill

enum { GRID_COUNT = 0, GRID_FILL_CSR = 1 };

// grid: B * chunks blocks of GRID_THREADS points
__global__ __launch_bounds__(GRID_THREADS) void grid_keys_kernel(const float* __restrict__ points, const float* __restrict__ origin, float inv,
                                                                 u64* __restrict__ keys, int N, int chunks) {
    const int b = (int)(blockIdx.x / (unsigned)chunks);
    const int i = (int)(blockIdx.x % (unsigned)chunks) * GRID_THREADS + (int)threadIdx.x;
    if (i >= N) return;
    const float ox = origin ? origin[3 * b] : 0.f, oy = origin ? origin[3 * b + 1] : 0.f, oz = origin ? origin[3 * b + 2] : 0.f;
    const VoxelCell v = voxel_cell(points + ((size_t)b * N + i) * 3, ox, oy, oz, inv);
    keys[(size_t)b * N + i] = v.kept ? voxel_key(v) : GRID_OFF;
}

__global__ __launch_bounds__(GRID_THREADS) void grid_fill_kernel(u64* __restrict__ table_keys, size_t slots) {
    const size_t step = (size_t)gridDim.x * GRID_THREADS;
    for (size_t w = (size_t)blockIdx.x * GRID_THREADS + threadIdx.x; w < slots; w += step) table_keys[w] = VOXEL_EMPTY;
}

// grid: B * chunks blocks of GRID_THREADS sorted positions
__global__ __launch_bounds__(GRID_THREADS) void grid_build_kernel(const float* __restrict__ points, const u64* __restrict__ keys,
                                                                  const int* __restrict__ perm, f32x4* __restrict__ sorted,
                                                                  u64* __restrict__ table_keys, int* __restrict__ table_range,
                                                                  int* __restrict__ n_in_grid, int N, unsigned cap, int chunks) {
    const int b = (int)(blockIdx.x / (unsigned)chunks);
    const int s = (int)(blockIdx.x % (unsigned)chunks) * GRID_THREADS + (int)threadIdx.x;
    if (s >= N) return;   // (no barrier below)
    const u64* kb = keys + (size_t)b * N;
    const u64 key = kb[s];
    const int given = perm[(size_t)b * N + s];
    const int j = (unsigned)given < (unsigned)N ? given : 0;   // a perm that is none reads inside the cloud all the same
    const float* p = points + ((size_t)b * N + j) * 3;
    sorted[(size_t)b * N + s] = f32x4{p[0], p[1], p[2], __int_as_float(j)};
    if (key >> 63) {   // the tail
        if (s == 0) n_in_grid[b] = 0;
        return;
    }
    const u64 next = s + 1 < N ? kb[s + 1] : GRID_OFF;
    if (next >> 63) n_in_grid[b] = s + 1;   // exactly one position of a sorted cloud is the last before the tail (or s = 0 above)
    const bool head = s == 0 || kb[s - 1] != key, last = next != key;
    if (!head && !last) return;
    u64* tk = table_keys + (size_t)b * cap;
    const unsigned mask = cap - 1;
    unsigned h = voxel_hash(key, mask);
    for (unsigned probe = 0; probe < cap; ++probe) {   // ends at an empty slot or at this key: at most N of the >= 2 N slots are taken
        const u64 seen = atomicCAS(tk + h, VOXEL_EMPTY, key);
        if (seen == VOXEL_EMPTY || seen == key) {
            int* range = table_range + ((size_t)b * cap + h) * 2;
            if (head) range[0] = s;
            if (last) range[1] = s + 1;
            break;
        }
        h = (h + 1) & mask;
    }
}

// grid: B * tiles blocks of T queries.  COUNT: count.  FILL_CSR: row_start, idx, d2 (nullable).  The walk is grid_walk (grid_walk.h); what
// is this kernel's own is the visitor: self exclusion by the index in .w, the stores, the counter.  The index comes in as the view's
// members, each pointer __restrict__, and the view is put together here: with the view as one parameter the CSR fill at 16 x 2048 measured
// 2.5 % slower than the parent, and a struct member cannot carry the noalias a parameter does
template <int T, int MODE>
__global__ __launch_bounds__(T) void grid_query_kernel(const float* __restrict__ query, const int* __restrict__ qorder,
                                                       const f32x4* __restrict__ sorted, const u64* __restrict__ table_keys,
                                                       const int2* __restrict__ table_range, const int* __restrict__ n_in_grid,
                                                       const float* __restrict__ origin, float inv, float R,
                                                       const long long* __restrict__ row_start, int* __restrict__ idx, float* __restrict__ d2,
                                                       int* __restrict__ count, unsigned r2_bits, int M, int N, unsigned cap, int exclude_self,
                                                       int tiles) {
    const GridView index{sorted, table_keys, table_range, n_in_grid, origin, inv, N, cap};
    const int b = (int)(blockIdx.x / (unsigned)tiles);
    const int t = (int)(blockIdx.x % (unsigned)tiles) * T + (int)threadIdx.x;
    if (t >= M) return;   // (no barrier below)
    const int i = qorder ? qorder[(size_t)b * M + t] : t;
    if ((unsigned)i >= (unsigned)M) return;   // a qorder that is no permutation writes nothing outside the outputs
    const size_t row = (size_t)b * M + i;
    const float qx = query[row * 3], qy = query[row * 3 + 1], qz = query[row * 3 + 2];
    const unsigned self = exclude_self ? (unsigned)i : 0xffffffffu;   // no j reaches 2^32 - 1
    const size_t o = MODE == GRID_FILL_CSR ? (size_t)row_start[row] : 0;
    int n = 0;   // neighbours so far (n <= N)
    if (cloud_finite3(qx, qy, qz))   // (a non-finite query has dist2 = +inf to everything)
        grid_walk(index, b, qx, qy, qz, R, r2_bits, [&](const f32x4 p, unsigned u) {
            const unsigned j = __float_as_uint(p[3]);
            if (j != self) {
                if (MODE == GRID_FILL_CSR) {
                    idx[o + (size_t)n] = (int)j;
                    if (d2) d2[o + (size_t)n] = __uint_as_float(u);
                }
                ++n;
            }
        });
    if (MODE == GRID_COUNT) count[row] = n;
}

}  // namespace

// key[b, i] of every point.  -2: arguments out of range, -3: the grid would pass 2^31 - 1 workgroups
int grid_keys_launch(const float* points, const float* origin, float cell_size, long long* keys, int B, int N, hipStream_t st) {
    if (!points || !keys || B < 1 || N < 1 || N > GECCO_VOXEL_MAX_POINTS) return -2;
    const int chunks = (N + GRID_THREADS - 1) / GRID_THREADS;
    if ((long long)B * chunks > 0x7fffffffLL) return -3;
    const float inv = 1.0f / cell_size;   // fp32, once, on the host
    hipLaunchKernelGGL(grid_keys_kernel, dim3((unsigned)(B * chunks)), dim3(GRID_THREADS), 0, st, points, origin, inv,
                       reinterpret_cast<u64*>(keys), N, chunks);
    return (int)hipGetLastError();
}

// Two launches: the table filled with the empty key, then the build.  -2: arguments out of range, -3: a grid would pass 2^31 - 1 workgroups
int grid_build_launch(const float* points, const long long* keys, const int* perm, float* sorted, long long* table_keys, int* table_range,
                      int* n_in_grid, int B, int N, hipStream_t st) {
    if (!points || !keys || !perm || !sorted || !table_keys || !table_range || !n_in_grid || B < 1 || N < 1 || N > GECCO_VOXEL_MAX_POINTS)
        return -2;
    const int chunks = (N + GRID_THREADS - 1) / GRID_THREADS;
    if ((long long)B * chunks > 0x7fffffffLL) return -3;
    const size_t cap = GECCO_GRID_CAPACITY(N), slots = (size_t)B * cap;
    const size_t fill_blocks = (slots + GRID_THREADS - 1) / GRID_THREADS, fill_cap = (size_t)device_cus() * 8;
    hipLaunchKernelGGL(grid_fill_kernel, dim3((unsigned)(fill_blocks < fill_cap ? fill_blocks : fill_cap)), dim3(GRID_THREADS), 0, st,
                       reinterpret_cast<u64*>(table_keys), slots);
    hipLaunchKernelGGL(grid_build_kernel, dim3((unsigned)(B * chunks)), dim3(GRID_THREADS), 0, st, points, reinterpret_cast<const u64*>(keys),
                       perm, reinterpret_cast<f32x4*>(sorted), reinterpret_cast<u64*>(table_keys), table_range, n_in_grid, N, (unsigned)cap,
                       chunks);
    return (int)hipGetLastError();
}

// One launch.  idx null: COUNT (count required, row_start and d2 null).  Otherwise FILL_CSR (row_start required, d2 nullable, count not
// written).  -2: arguments out of range (radius2 above fp32(cell_size^2) among them), -3: the grid would pass 2^31 - 1 workgroups
int grid_radius_launch(const float* query, const int* qorder, const GridIndexArgs& index, const long long* row_start, int* idx, float* d2,
                       int* count, int B, int M, int N, float r2, int exclude_self, hipStream_t st) {
    const GridView g = grid_view(index, B, N);
    if (!g.sorted || !query || M < 1 || !grid_radius2_ok(r2, index.cell_size) || (exclude_self && M != N)) return -2;
    if (idx ? !row_start : !count || row_start || d2) return -2;
    const CloudPlan p = cloud_plan(B, M, N, 1, false, 256, device_cus());
    if (!p.fits()) return -3;
    const unsigned r2_bits = __builtin_bit_cast(unsigned, r2);
    const float R = grid_reach(r2);
    const int self = exclude_self ? 1 : 0;
    return dispatch_T(p.T, [&](auto t) -> int {
        constexpr int T = decltype(t)::value;
        const dim3 grid((unsigned)p.blocks), block(T);
        if (!idx)
            hipLaunchKernelGGL((grid_query_kernel<T, GRID_COUNT>), grid, block, 0, st, query, qorder, g.sorted, g.table_keys, g.table_range,
                               g.n_in_grid, g.origin, g.inv, R, row_start, idx, d2, count, r2_bits, M, N, g.cap, self, p.tiles);
        else
            hipLaunchKernelGGL((grid_query_kernel<T, GRID_FILL_CSR>), grid, block, 0, st, query, qorder, g.sorted, g.table_keys, g.table_range,
                               g.n_in_grid, g.origin, g.inv, R, row_start, idx, d2, count, r2_bits, M, N, g.cap, self, p.tiles);
        return (int)hipGetLastError();
    });
}
