// The eigenproblem of a ball's 3 x 3 covariance, solved in registers, as the kernels that pool the fp64 moments of a radius ball share
// it (iss.hip's iss_saliency_kernel: the eigenvalues; normals_grid.hip's normals_grid_kernel: the eigenvalues and the eigenvectors).
// One spelling of the `moments` and `eigen` steps of gecco_iss_keypoints_f32 (include/gecco_hip.h), from the count and the nine sums a
// walk's visitor adds in registers (Sym3Moments) to the sorted eigenvalues:
//   moments     d = double(p_j) - double(q) per axis from the caller;  m counts, S1 = sum d (3 sums), S2 = sum d d^T (xx, xy, xz, yy,
//               yz, zz), each from 0 in the order of the calls
//   covariance  inv = 1 / m;  mu = S1 inv;  C_ab = S2_ab inv - mu_a mu_b
//   eigen       big = max |C_ab|;  A = C sc with sc = 1 / big;  SYM3_JACOBI_SWEEPS = 8 cyclic Jacobi sweeps over (0,1), (0,2), (1,2) with
//               the guarded rotation of rigid_fit.h (icp_rotate: a non-finite theta gives t = 0, a theta whose square would overflow
//               t = 1 / (2 theta)), a fixed count;  lambda = diag big, negative roundings clamped to 0
//   vectors     (VECTORS only) V starts as the identity and takes every rotation: its columns p and q rotate as the rows and columns
//               p and q of A do, icp_rotate's v[r][p] = c v_rp - s v_rq, v[r][q] = s v_rp + c v_rq
//   order       three compare-exchanges, (0,1), (1,2), (0,1): lambda0 <= lambda1 <= lambda2; a column follows its eigenvalue, and
//               moves only when that is STRICTLY smaller, so equal eigenvalues keep their column order
// Every operation is rounded to fp64 and none is contracted.  The matrix, the rotations and V are named scalars: no indexed local
// array, nothing in scratch (plane.hip's refit keeps arrays in scratch because one thread per cloud runs it; here every thread does).
// VECTORS is a compile-time option: the eigenvalues are the same operations in the same order with it and without, so the two forms
// agree bit for bit, and the form without carries no instruction of the other.
#pragma once
#include <cmath>

constexpr int SYM3_JACOBI_SWEEPS = 8;   // rigid_fit.h's count: quadratic convergence, fp64 by the fifth

static __device__ __forceinline__ bool sym3_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN and inf

// icp_rotate (rigid_fit.h) for a symmetric 3 x 3 matrix held in scalars: the rotation that annihilates a_pq; arp, arq are the entries
// of the third row r against p and q; v0p .. v2q the columns p and q of V (VECTORS only).  Same guard, same order of operations
template <bool VECTORS>
static __device__ __forceinline__ void sym3_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                                   double& v1p, double& v1q, double& v2p, double& v2q) {
#pragma clang fp contract(off)
    double t = 0.0;
    if (apq != 0.0) {
        const double theta = (aqq - app) / (2.0 * apq);
        const double at = fabs(theta);
        if (at <= 1e150)
            t = copysign(1.0, theta) / (at + sqrt(theta * theta + 1.0));
        else if (sym3_finite(at))
            t = 0.5 / theta;
    }
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const double shift = t * apq;
    app -= shift;
    aqq += shift;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
    if (VECTORS) {
        const double p0 = v0p, q0 = v0q, p1 = v1p, q1 = v1q, p2 = v2p, q2 = v2q;
        v0p = c * p0 - s * q0, v0q = s * p0 + c * q0;
        v1p = c * p1 - s * q1, v1q = s * p1 + c * q1;
        v2p = c * p2 - s * q2, v2q = s * p2 + c * q2;
    }
}

// The count and the nine fp64 sums of a ball, in registers: add(d) per visited point, in ball order
struct Sym3Moments {
    int m = 0;
    double sx = 0.0, sy = 0.0, sz = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
    __device__ __forceinline__ void add(double dx, double dy, double dz) {
#pragma clang fp contract(off)
        ++m;
        sx += dx, sy += dy, sz += dz;
        sxx += dx * dx, sxy += dx * dy, sxz += dx * dz;
        syy += dy * dy, syz += dy * dz, szz += dz * dz;
    }
};

// What sym3_eigen leaves: l0 <= l1 <= l2 and, with VECTORS, (x, y, z) = the column of V that belongs to l0, not normalised.  All 0
// where the problem was not solved
struct Sym3Eigen {
    double l0, l1, l2;
    double x, y, z;
    bool solved;   // big a positive finite number
};

// The steps above from the moments of a ball of s.m >= 1 points
template <bool VECTORS>
static __device__ __forceinline__ Sym3Eigen sym3_eigen(const Sym3Moments& s) {
#pragma clang fp contract(off)
    Sym3Eigen e{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, false};
    const double im = 1.0 / (double)s.m;
    const double mx = s.sx * im, my = s.sy * im, mz = s.sz * im;
    double a00 = s.sxx * im - mx * mx, a01 = s.sxy * im - mx * my, a02 = s.sxz * im - mx * mz;
    double a11 = s.syy * im - my * my, a12 = s.syz * im - my * mz, a22 = s.szz * im - mz * mz;
    const double big = fmax(fmax(fmax(fabs(a00), fabs(a01)), fmax(fabs(a02), fabs(a11))), fmax(fabs(a12), fabs(a22)));
    if (!(big > 0.0 && sym3_finite(big))) return e;
    const double sc = 1.0 / big;
    a00 *= sc, a01 *= sc, a02 *= sc, a11 *= sc, a12 *= sc, a22 *= sc;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;   // V[row][column]
    auto sweep = [&] {
        sym3_rotate<VECTORS>(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0, 1): the third row is 2
        sym3_rotate<VECTORS>(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0, 2): the third row is 1
        sym3_rotate<VECTORS>(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1, 2): the third row is 0
    };
    if (VECTORS) {   // kept as a loop: unrolled, the 24 rotations with V are scheduled into 144 VGPRs (3 waves a SIMD)
#pragma unroll 1
        for (int n = 0; n < SYM3_JACOBI_SWEEPS; ++n) sweep();
    } else {
        for (int n = 0; n < SYM3_JACOBI_SWEEPS; ++n) sweep();
    }
    double l0 = fmax(a00 * big, 0.0), l1 = fmax(a11 * big, 0.0), l2 = fmax(a22 * big, 0.0);
    // three compare-exchanges; the column of the smallest follows through the two it takes part in with a strict compare
    const bool first = l1 < l0;   // (0, 1): column 1 comes to the front
    double lo = fmin(l0, l1), hi = fmax(l0, l1);
    l0 = lo, l1 = hi;
    double x0 = first ? v01 : v00, y0 = first ? v11 : v10, z0 = first ? v21 : v20;   // the column at place 0
    double x1 = first ? v00 : v01, y1 = first ? v10 : v11, z1 = first ? v20 : v21;   // the column at place 1
    const bool second = l2 < l1;   // (1, 2)
    lo = fmin(l1, l2), hi = fmax(l1, l2);
    l1 = lo, l2 = hi;
    if (VECTORS && second) x1 = v02, y1 = v12, z1 = v22;
    const bool third = l1 < l0;   // (0, 1)
    lo = fmin(l0, l1), hi = fmax(l0, l1);
    l0 = lo, l1 = hi;
    if (VECTORS && third) x0 = x1, y0 = y1, z0 = z1;
    e.l0 = l0, e.l1 = l1, e.l2 = l2, e.solved = true;
    if (VECTORS) e.x = x0, e.y = y0, e.z = z0;
    return e;
}
