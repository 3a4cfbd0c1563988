// What the consensus kernels share (ransac.hip, plane.hip): the counter-based draw of three distinct indices, the squared length and the
// degenerate-triangle test in fp64 without a division or a root, the ordered append of the compactions and of phase 1, the total order
// of the scores, the 16-byte record a workgroup leaves and the reductions under that order.  One implementation, so that a hypothesis h
// of seed s names the same triple and the same winner in gecco_ransac_f32 and gecco_plane_ransac_f32 (include/gecco_hip.h: the
// definitions; tests/_ransac_ref.py restates the draw).  Device code is static __device__ __forceinline__.
#pragma once
#include "common.h"

static __device__ __forceinline__ unsigned long long ransac_mix(unsigned long long z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// three distinct indices in [0, K), K >= 3, without a rejection loop
static __device__ __forceinline__ void ransac_draw(unsigned long long seed, int h, int K, int& a0, int& a1, int& a2) {
    unsigned d[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const unsigned long long u = ransac_mix(seed + (3ull * (unsigned long long)h + (unsigned long long)(t + 1)) * 0x9E3779B97F4A7C15ull);
        d[t] = (unsigned)(((u >> 32) * (unsigned long long)(K - t)) >> 32);
    }
    const unsigned b0 = d[0];
    const unsigned b1 = d[1] + (d[1] >= b0 ? 1u : 0u);
    const unsigned lo = min(b0, b1), hi = max(b0, b1);
    unsigned b2 = d[2];
    b2 += b2 >= lo ? 1u : 0u;
    b2 += b2 >= hi ? 1u : 0u;
    a0 = (int)b0, a1 = (int)b1, a2 = (int)b2;
}

static __device__ __forceinline__ double ransac_len2(double x, double y, double z) {
#pragma clang fp contract(off)
    return (x * x + y * y) + z * z;
}

// check 1 on one side of the triple: |e1 x e2|^2 <= 2^-20 |e1|^2 |e2|^2
static __device__ __forceinline__ bool ransac_degenerate(const double (&X)[3][3]) {
#pragma clang fp contract(off)
    const double e1[3] = {X[1][0] - X[0][0], X[1][1] - X[0][1], X[1][2] - X[0][2]};
    const double e2[3] = {X[2][0] - X[0][0], X[2][1] - X[0][1], X[2][2] - X[0][2]};
    const double nx = e1[1] * e2[2] - e1[2] * e2[1];
    const double ny = e1[2] * e2[0] - e1[0] * e2[2];
    const double nz = e1[0] * e2[1] - e1[1] * e2[0];
    return ransac_len2(nx, ny, nz) <= 0x1p-20 * (ransac_len2(e1[0], e1[1], e1[2]) * ransac_len2(e2[0], e2[1], e2[2]));
}

// (count, sum, h) beats (bc, bs, bh): count descending, sum ascending, h ascending; bh < 0: nothing yet
static __device__ __forceinline__ bool ransac_better(int c, double s, int h, int bc, double bs, int bh) {
    if (h < 0) return false;
    if (bh < 0) return true;
    if (c != bc) return c > bc;
    if (s != bs) return s < bs;
    return h < bh;
}

// Ordered append: the slot of a kept item in a list that holds the kept items of all earlier calls and of the lower threads of this
// one (a ballot, the rank inside the wave, the waves' totals in wtot[WAVES] of LDS), and base advanced by this call's total (uniform).
// Every thread of the block calls it.  wtot is read after the barrier inside: the caller stores its item and then places the second
// barrier itself (__syncthreads()) before the next call rewrites wtot, which is also where an LDS list becomes readable.
template <int WAVES>
static __device__ __forceinline__ int ransac_append(bool keep, int& base, int* wtot) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(keep);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[w] = __popcll(m);
    __syncthreads();
    int off = base, total = 0;
#pragma unroll
    for (int ww = 0; ww < WAVES; ++ww) {
        if (ww < w) off += wtot[ww];
        total += wtot[ww];
    }
    base += total;
    return off + before;
}

// What a workgroup of a hypothesis kernel leaves in the workspace: the best of its hypotheses that reached the bar, under ransac_better
struct __attribute__((aligned(16))) ConsensusRecord {
    int count;    // 0 when no hypothesis of the block reached the bar
    int h;        // its hypothesis, -1 when there is none
    double sum;
};
static_assert(sizeof(ConsensusRecord) == 16, "16 bytes per block");

// The LDS of a reduction under ransac_better by THREADS threads
template <int THREADS>
struct ConsensusKeys {
    int c[THREADS], h[THREADS];
    double s[THREADS];
};

// Block best: every thread brings its own best (bc, bs, bh); afterwards the workgroup's best is in slot 0 of k, readable by every thread.
// The order is total, so the shape of the tree cannot change the winner.
template <int THREADS>
static __device__ __forceinline__ void ransac_block_best(int bc, double bs, int bh, ConsensusKeys<THREADS>& k) {
    const int tid = threadIdx.x;
    k.c[tid] = bc, k.s[tid] = bs, k.h[tid] = bh;
    __syncthreads();
    for (int off = THREADS / 2; off > 0; off >>= 1) {
        if (tid < off && ransac_better(k.c[tid + off], k.s[tid + off], k.h[tid + off], k.c[tid], k.s[tid], k.h[tid]))
            k.c[tid] = k.c[tid + off], k.s[tid] = k.s[tid + off], k.h[tid] = k.h[tid + off];
        __syncthreads();
    }
}

// The first step of a select kernel: the best of a cloud's n records, strided over the threads, then the tree
template <int THREADS>
static __device__ __forceinline__ void ransac_best_record(const ConsensusRecord* __restrict__ records, int n, ConsensusKeys<THREADS>& k) {
    int bc = 0, bh = -1;
    double bs = 0.0;
    for (int i = threadIdx.x; i < n; i += THREADS) {
        const ConsensusRecord q = records[i];
        if (ransac_better(q.count, q.sum, q.h, bc, bs, bh)) bc = q.count, bs = q.sum, bh = q.h;
    }
    ransac_block_best(bc, bs, bh, k);
}
