// The cell of a point in a regular grid, as voxel.hip (gecco_voxel_downsample_f32) and grid.hip (gecco_grid_keys_f32) share it: the fp32
// roundings that put a point into a cell, the 63-bit key of a cell and the hash of a key into an open-addressing table.  Two operators
// that must agree on which points share a cell read one spelling.  Device code is static __device__ __forceinline__.
#pragma once
#include "common.h"

typedef unsigned long long u64;
constexpr u64 VOXEL_EMPTY = ~0ull;        // an empty table slot (no key has bit 63)
constexpr float VOXEL_HALF = 1048576.f;   // 2^20: cells lie in [-2^20, 2^20) per axis

struct VoxelCell {
    int c[3];
    u64 q[3];
    bool kept;
};

// the fp32 roundings of the definition: t = p - o, u = t * inv, c = floor(u), frac = u - c, q = trunc(frac * 2^32)
static __device__ __forceinline__ VoxelCell voxel_cell(const float* __restrict__ p, float ox, float oy, float oz, float inv) {
#pragma clang fp contract(off)
    VoxelCell r;
    const float o[3] = {ox, oy, oz};
    r.kept = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float t = p[a] - o[a];
        const float u = t * inv;
        const float c = floorf(u);
        const bool ok = __builtin_isfinite(u) && c >= -VOXEL_HALF && c < VOXEL_HALF;
        r.kept = r.kept && ok;
        const float frac = u - c;                                   // in [0, 1]; 1.0 for a tiny negative u
        r.c[a] = ok ? (int)c : 0;
        r.q[a] = ok ? (u64)(frac * 4294967296.0f) : 0ull;           // exact scaling, truncation
    }
    return r;
}

static __device__ __forceinline__ u64 voxel_key(int cx, int cy, int cz) {
    return ((u64)(unsigned)(cx + (1 << 20)) << 42) | ((u64)(unsigned)(cy + (1 << 20)) << 21) | (u64)(unsigned)(cz + (1 << 20));
}
static __device__ __forceinline__ u64 voxel_key(const VoxelCell& v) { return voxel_key(v.c[0], v.c[1], v.c[2]); }

// murmur3's 64-bit finaliser: every bit of the key reaches every bit of the slot index, so cells along one axis, or a power-of-two
// stride apart, spread over the table instead of piling into one probe run
static __device__ __forceinline__ unsigned voxel_hash(u64 k, unsigned mask) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (unsigned)k & mask;
}
