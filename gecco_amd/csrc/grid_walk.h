// The cell walk of the grid index, as every kernel that reads the index shares it (grid.hip's grid_query_kernel, iss.hip's two kernels,
// dbscan.hip's dbscan_grid_kernel): the reach of a ball, the clamped box of cells it can touch, the table probe, the runs, the off-grid
// tail and the scan of the whole cloud for a box too wide to walk.  The proofs that the walk misses no neighbour and that every loop is
// bounded stand here, once, beside the one spelling of the code they are about.  Device code is static __device__ __forceinline__, host
// helpers are inline.
//
// How the index travels.  A launcher is handed the six values of the C ABI as one GridIndexArgs (kernels.h) and makes one GridView of
// them (grid_view, below: the null and range tests, the casts, inv and cap, written once); a kernel takes the view by value
// (grid_query_kernel its members, for the reason given there), reads its own cloud's sorted points through view.cloud(b) and hands the
// view and b to grid_walk, which forms the cloud's tables itself.
//
// The walk (grid.hip's header defines the index: cells, keys, the sorted order, the table, n_in_grid).  For a finite point q, with R the
// host's fp32 reach (grid_reach), per axis the cells lo = cell(fp32(q - R)) .. hi = cell(fp32(q + R)), voxel_cell's u and floor, clamped
// to the grid; the box is walked with x outermost and z innermost, which is ascending key order; every occupied cell's run
// sorted[start .. end) is scanned, then the tail sorted[n_in_grid .. N).  An entry p is in the ball when cloud_dist2_bits(q, p) <=
// r2_bits (radius.hip's predicate on radius.hip's bits), and the ball is visited in ascending sorted position.
//
// Why no neighbour is missed.  Let dist2(q, p) <= r2 and take one axis, d = fp32(q - p).  Rounding and adding non-negative numbers are
// monotone, so fp32(d d) <= dist2 <= r2, hence the real d d <= r2 (1 + 2^-24) + 2^-150 (half a unit above r2, the second term when r2
// is subnormal), and the real |q - p| <= |d| (1 + 2^-24).  grid_reach forms, in double and rounded UP to fp32,
//     R >= sqrt(r2 (1 + 2^-23) + 2^-149) (1 + 2^-16),
// which is above that bound (and above r (1 + 2^-16), since r2 >= r r (1 - 2^-24)).  So p >= q - R in the reals, and p being an fp32
// number, p >= fp32(q - R): rounding to nearest never crosses a representable number.  Subtracting o, multiplying by inv > 0 and
// floor are each monotone in fp32 as well, so cell(p) >= cell(fp32(q - R)) = lo, and symmetrically cell(p) <= hi.  An on-grid p has its
// cell inside the grid, so clamping lo and hi to the grid loses nothing; an off-grid p is in the tail, which every query scans.  Extra
// cells cost time, never correctness: the cells are a filter, membership is dist2 <= r2 alone.
//
// How wide the box can be.  The entry points refuse radius2 > fp32(cell_size^2) (grid_radius2_ok), so for a normal r2 R <= cell_size
// (1 + 2^-15) and 2 R inv <= 2.0001.  fp32(q + R) - fp32(q - R) <= 2 R + (the spacing of fp32 numbers at |q| + R), and inside the grid
// (|u| < 2^20) the two roundings of t add at most 1/8 cell and the two of u at most 1/8.  So where fp32 resolves the coordinates to
// better than 0.7 of a cell, every cloud a grid makes sense for, u(q + R) - u(q - R) < 3 and the box touches AT MOST GRID_BOX = 4 CELLS
// PER AXIS, 64 in all (tests/test_grid_cpu.py asserts it on its inputs, coordinates near 1000 at r = 0.01 and cells at +-2^20 among
// them).  The three loops are bounded by that constant.  Where the arithmetic gives a wider box all the same (coordinates fp32
// resolves more coarsely than a cell, a subnormal r2, a non-finite origin) the thread scans the whole sorted cloud instead,
// sorted[0 .. N), and then neither the cells nor the tail: the scan of radius.hip in another order, the same neighbours, each once,
// still ascending in sorted position.  No input makes a thread walk an unbounded box and none loses a neighbour to the bound.
#pragma once
#include <cmath>

#include "cloud_nn.h"
#include "kernels.h"
#include "voxel_cell.h"

constexpr int GRID_BOX = 4;   // cells per axis a walk visits; a wider box is answered by a scan of the whole cloud
constexpr int GRID_HALF = 1 << 20;

// floor(u) of the fp32 coordinate x on one axis: voxel_cell's roundings
static __device__ __forceinline__ float grid_u(float x, float o, float inv) {
#pragma clang fp contract(off)
    const float t = x - o;
    return floorf(t * inv);
}

// The reach R of a ball's box (above): the least fp32 number >= sqrt(r2 (1 + 2^-23) + 2^-149) (1 + 2^-16), formed in double
inline float grid_reach(float r2) {
    const double bound = std::sqrt((double)r2 * (1.0 + 0x1p-23) + 0x1p-149) * (1.0 + 0x1p-16);
    float R = (float)bound;
    if ((double)R < bound) R = std::nextafterf(R, INFINITY);
    return R;
}

// a radius2 an index of this cell_size serves: a finite number > 0 (false for NaN) and not above fp32(cell_size^2)
inline bool grid_radius2_ok(float r2, float cell_size) { return r2 > 0.f && r2 <= 3.402823466e38f && r2 <= cell_size * cell_size; }

// The index of B clouds of N points as a kernel reads it, passed by value
struct GridView {
    const f32x4* sorted;       // (B, N): (x, y, z, the bits of perm) per sorted position
    const u64* table_keys;     // (B, cap)
    const int2* table_range;   // (B, cap): the run [start, end) of the slot's key
    const int* n_in_grid;      // (B,): where the tail starts
    const float* origin;       // (B, 3), or null: 0
    float inv;                 // fp32(1 / cell_size), once, on the host
    int N;
    unsigned cap;              // GECCO_GRID_CAPACITY(N)
    __device__ __forceinline__ const f32x4* cloud(int b) const { return sorted + (size_t)b * N; }
};

// The view of the index `g` over B clouds of N points; sorted == nullptr (a launcher's -2) when a required pointer is null or B, N are
// out of range
inline GridView grid_view(const GridIndexArgs& g, int B, int N) {
    if (!g.sorted || !g.table_keys || !g.table_range || !g.n_in_grid || B < 1 || N < 1 || N > GECCO_VOXEL_MAX_POINTS) return GridView{};
    return GridView{reinterpret_cast<const f32x4*>(g.sorted), reinterpret_cast<const u64*>(g.table_keys),
                    reinterpret_cast<const int2*>(g.table_range), g.n_in_grid, g.origin, 1.0f / g.cell_size, N,
                    (unsigned)GECCO_GRID_CAPACITY(N)};
}

// The walk for the finite point (qx, qy, qz) of cloud b: visit(p, u) for every sorted entry p with u = cloud_dist2_bits(q, p) <=
// r2_bits, in ascending sorted position, each entry once
template <class Visit>
static __device__ __forceinline__ void grid_walk(const GridView& g, int b, float qx, float qy, float qz, float R, unsigned r2_bits,
                                                 Visit visit) {
#pragma clang fp contract(off)
    const f32x4* sb = g.cloud(b);   // the cloud's own sorted points, table and tail
    const u64* tk = g.table_keys + (size_t)b * g.cap;
    const int2* tr = g.table_range + (size_t)b * g.cap;
    const int N = g.N, tail = g.n_in_grid[b];
    const unsigned cap = g.cap;
    auto scan = [&](int from, int to) {
        for (int s = from; s < to; ++s) {
            const f32x4 p = sb[s];   // one 16-byte load
            const unsigned u = cloud_dist2_bits(qx, qy, qz, p);
            if (u <= r2_bits) visit(p, u);
        }
    };
    const float q[3] = {qx, qy, qz};
    int lo[3], hi[3];
    bool wide = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float org = g.origin ? g.origin[3 * b + a] : 0.f;
        const float below = q[a] - R, above = q[a] + R;   // rounded to fp32 before the cell arithmetic
        const float fl = grid_u(below, org, g.inv), fh = grid_u(above, org, g.inv);
        // clamped to the grid: a bound beyond it on the far side leaves an empty box, a NaN (a non-finite origin) the widest one
        lo[a] = fl >= -VOXEL_HALF ? (fl < VOXEL_HALF ? (int)fl : GRID_HALF) : -GRID_HALF;
        hi[a] = fh < VOXEL_HALF ? (fh >= -VOXEL_HALF ? (int)fh : -GRID_HALF - 1) : GRID_HALF - 1;
        wide = wide || hi[a] - lo[a] >= GRID_BOX;
    }
    if (wide) {   // above: never for coordinates that fp32 resolves inside a cell
        scan(0, N);
        return;
    }
    const unsigned mask = cap - 1;
    for (int cx = lo[0]; cx < lo[0] + GRID_BOX && cx <= hi[0]; ++cx)
        for (int cy = lo[1]; cy < lo[1] + GRID_BOX && cy <= hi[1]; ++cy)
            for (int cz = lo[2]; cz < lo[2] + GRID_BOX && cz <= hi[2]; ++cz) {   // ascending key
                const u64 key = voxel_key(cx, cy, cz);
                unsigned h = voxel_hash(key, mask);
                for (unsigned probe = 0; probe < cap; ++probe) {   // ends at the key or at an empty slot (load <= 0.5)
                    const u64 seen = tk[h];
                    if (seen == key) {
                        const int2 r = tr[h];
                        scan(max(r.x, 0), min(r.y, N));
                        break;
                    }
                    if (seen == VOXEL_EMPTY) break;
                    h = (h + 1) & mask;
                }
            }
    scan(min(max(tail, 0), N), N);   // the off-grid tail
}
