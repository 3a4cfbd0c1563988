// The rigid fit icp.hip and ransac.hip share: the fp32 transform of a point, Horn's quaternion from fp64 moments of point pairs about an
// anchor, its 4 x 4 symmetric eigenproblem by a fixed number of cyclic Jacobi sweeps, the finite test, the fixed-order reduction of the
// fp64 sums that feed it (plane.hip's refit reduces the same way) and the compose step.  One implementation, so that a fit of the same
// sums is the same bits wherever it runs; the steps are part of the definitions of gecco_icp_f32 and gecco_ransac_f32 (include/gecco_hip.h).
// Device code is static __device__; icp_solve_point stays __noinline__ (one copy per kernel, its arrays in scratch once).
#pragma once
#include "common.h"

constexpr int ICP_JACOBI_SWEEPS = 8;   // cyclic sweeps over the six pairs of Horn's 4 x 4 matrix: quadratic convergence, fp64 by the fifth

// step 1: rows 0 .. 2 of Tf = fp32(T) applied to (x, y, z)
static __device__ __forceinline__ void icp_transform(const float* tf, float x, float y, float z, float& px, float& py, float& pz) {
#pragma clang fp contract(off)
    px = ((tf[0] * x + tf[1] * y) + tf[2] * z) + tf[3];
    py = ((tf[4] * x + tf[5] * y) + tf[6] * z) + tf[7];
    pz = ((tf[8] * x + tf[9] * y) + tf[10] * z) + tf[11];
}

static __device__ __forceinline__ bool icp_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN and inf

// One Jacobi rotation of the symmetric 4 x 4 matrix a that annihilates a[p][q], accumulated into the eigenvector columns v.  The
// guard of normals_rotate: a non-finite theta gives t = 0 (the entry is already nothing beside the diagonal and is dropped), a theta
// whose square would overflow gives t = 1 / (2 theta).
static __device__ __forceinline__ void icp_rotate(double (&a)[4][4], double (&v)[4][4], int p, int q) {
    const double apq = a[p][q];
    double t = 0.0;
    if (apq != 0.0) {
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double at = fabs(theta);
        if (at <= 1e150)
            t = copysign(1.0, theta) / (at + sqrt(theta * theta + 1.0));
        else if (icp_finite(at))
            t = 0.5 / theta;
    }
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    a[p][p] -= t * apq;
    a[q][q] += t * apq;
    a[p][q] = a[q][p] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r != p && r != q) {
            const double rp = a[r][p], rq = a[r][q];
            a[r][p] = a[p][r] = c * rp - s * rq;
            a[r][q] = a[q][r] = s * rp + c * rq;
        }
        const double vp = v[r][p], vq = v[r][q];
        v[r][p] = c * vp - s * vq;
        v[r][q] = s * vp + c * vq;
    }
}

// Fixed-order sums of a workgroup's fp64 accumulators, the order the definitions name: a fixed tree inside the wave, then the waves in
// order.  icp_wave_sums: every thread brings acc[NACC]; the shuffle tree 32, 16, .., 1 leaves each wave's sums in part[wave].  After
// the caller's barrier, icp_block_sums (one thread) adds wave 0 + wave 1 + .. into sum[NACC].
template <int NACC, int WAVES>
static __device__ __forceinline__ void icp_wave_sums(const double (&acc)[NACC], double (&part)[WAVES][NACC]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int e = 0; e < NACC; ++e) {
        double v = acc[e];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((tid & 63) == 0) part[tid >> 6][e] = v;
    }
}

template <int NACC, int WAVES>
static __device__ __forceinline__ void icp_block_sums(const double (&part)[WAVES][NACC], double (&sum)[NACC]) {
    for (int e = 0; e < NACC; ++e) {
        double v = part[0][e];
        for (int w = 1; w < WAVES; ++w) v += part[w][e];
        sum[e] = v;
    }
}

// step 5's compose: T <- dT * double(Tf), dT (3 x 4) having the bottom row (0, 0, 0, 1); tf holds all 16 entries of Tf.  It stands
// outside any fp contract(off) region, so this is the one place where the compiler decides how its products and sums fuse.
static __device__ __forceinline__ void icp_compose(const double* dT, const float* tf, double* T) {
    for (int r = 0; r < 3; ++r)
        for (int e = 0; e < 4; ++e)
            T[4 * r + e] = ((dT[4 * r] * (double)tf[e] + dT[4 * r + 1] * (double)tf[4 + e]) + dT[4 * r + 2] * (double)tf[8 + e]) +
                           dT[4 * r + 3] * (double)tf[12 + e];
    for (int e = 0; e < 4; ++e) T[12 + e] = (double)tf[12 + e];
}

// Point-to-point step from the reduced sums: acc[2..4] = sum (P - c), acc[5..7] = sum (Q - c), acc[8 + 3 a + e] = sum (P - c)_a (Q - c)_e.
// dT (3 x 4, row-major) maps p' onto q.
static __device__ __noinline__ void icp_solve_point(const double* acc, double n, const double* c, double* dT) {
    const double inv = 1.0 / n;
    double mp[3], mq[3], Sm[3][3];
    for (int a = 0; a < 3; ++a) mp[a] = acc[2 + a] * inv, mq[a] = acc[5 + a] * inv;
    for (int a = 0; a < 3; ++a)
        for (int e = 0; e < 3; ++e) Sm[a][e] = acc[8 + 3 * a + e] * inv - mp[a] * mq[e];
    double a[4][4], v[4][4];
    a[0][0] = (Sm[0][0] + Sm[1][1]) + Sm[2][2];
    a[1][1] = (Sm[0][0] - Sm[1][1]) - Sm[2][2];
    a[2][2] = (Sm[1][1] - Sm[0][0]) - Sm[2][2];
    a[3][3] = (Sm[2][2] - Sm[0][0]) - Sm[1][1];
    a[0][1] = a[1][0] = Sm[1][2] - Sm[2][1];
    a[0][2] = a[2][0] = Sm[2][0] - Sm[0][2];
    a[0][3] = a[3][0] = Sm[0][1] - Sm[1][0];
    a[1][2] = a[2][1] = Sm[0][1] + Sm[1][0];
    a[1][3] = a[3][1] = Sm[2][0] + Sm[0][2];
    a[2][3] = a[3][2] = Sm[1][2] + Sm[2][1];
    double big = 0.0;
    for (int r = 0; r < 4; ++r)
        for (int e = 0; e < 4; ++e) big = fmax(big, fabs(a[r][e]));
    if (big > 0.0 && icp_finite(big)) {
        const double sc = 1.0 / big;
        for (int r = 0; r < 4; ++r)
            for (int e = 0; e < 4; ++e) a[r][e] *= sc;
    }
    for (int r = 0; r < 4; ++r)
        for (int e = 0; e < 4; ++e) v[r][e] = r == e ? 1.0 : 0.0;
    for (int sweep = 0; sweep < ICP_JACOBI_SWEEPS; ++sweep) {
        icp_rotate(a, v, 0, 1);
        icp_rotate(a, v, 0, 2);
        icp_rotate(a, v, 0, 3);
        icp_rotate(a, v, 1, 2);
        icp_rotate(a, v, 1, 3);
        icp_rotate(a, v, 2, 3);
    }
    int top = 0;   // the largest eigenvalue, the lowest index among equals (all zero: the identity)
    for (int e = 1; e < 4; ++e)
        if (a[e][e] > a[top][top]) top = e;
    double qw = v[0][top], qx = v[1][top], qy = v[2][top], qz = v[3][top];
    const double rn = 1.0 / sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    const double sg = qw < 0.0 ? -rn : rn;
    qw *= sg, qx *= sg, qy *= sg, qz *= sg;
    double R[3][3];
    R[0][0] = 1.0 - 2.0 * (qy * qy + qz * qz);
    R[0][1] = 2.0 * (qx * qy - qw * qz);
    R[0][2] = 2.0 * (qx * qz + qw * qy);
    R[1][0] = 2.0 * (qx * qy + qw * qz);
    R[1][1] = 1.0 - 2.0 * (qx * qx + qz * qz);
    R[1][2] = 2.0 * (qy * qz - qw * qx);
    R[2][0] = 2.0 * (qx * qz - qw * qy);
    R[2][1] = 2.0 * (qy * qz + qw * qx);
    R[2][2] = 1.0 - 2.0 * (qx * qx + qy * qy);
    // t = mu_q - R mu_p with mu = c + m:  c + mq - R (c + mp)
    for (int r = 0; r < 3; ++r) {
        for (int e = 0; e < 3; ++e) dT[4 * r + e] = R[r][e];
        dT[4 * r + 3] = (c[r] + mq[r]) - ((R[r][0] * (c[0] + mp[0]) + R[r][1] * (c[1] + mp[1])) + R[r][2] * (c[2] + mp[2]));
    }
}
