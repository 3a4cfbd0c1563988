// The pair feature of FPFH, as both descriptor families compute it (fpfh.hip on kNN lists, fpfh_grid.hip on the radius balls of the grid
// index): steps 1 - 8 of gecco_fpfh_f32's definition (include/gecco_hip.h; tests/_fpfh_ref.py restates them in numpy) and the bin of a
// coordinate.  fp64 on the fp32 inputs, every operation rounded, none contracted: bin edges make the histogram discontinuous, so the
// roundings are part of the definition and there is one spelling of them.  Device code is static __device__ __forceinline__.
#pragma once
#include "cloud_nn.h"

constexpr int FPFH_BINS = GECCO_FPFH_BINS;   // 3 groups of 11
static_assert(FPFH_BINS == 33, "three groups of 11 bins");

static __device__ __forceinline__ int fpfh_bin(double u) { return u >= 10.0 ? 10 : (u >= 1.0 ? (int)u : 0); }   // a NaN: bin 0

// steps 1 - 8 of the definition for the pair (point i, neighbour j)
static __device__ __forceinline__ void fpfh_pair_bins(float pix, float piy, float piz, float nix, float niy, float niz, float pjx, float pjy,
                                                      float pjz, float njx, float njy, float njz, int& b0, int& b1, int& b2) {
#pragma clang fp contract(off)
    constexpr double PI = 3.14159265358979323846;
    double n1x = nix, n1y = niy, n1z = niz, n2x = njx, n2y = njy, n2z = njz;
    double dx = (double)pjx - (double)pix, dy = (double)pjy - (double)piy, dz = (double)pjz - (double)piz;
    const double d = sqrt((dx * dx + dy * dy) + dz * dz);
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;
    if (d != 0.0) {
        const double a1 = ((n1x * dx + n1y * dy) + n1z * dz) / d;
        const double a2 = ((n2x * dx + n2y * dy) + n2z * dz) / d;
        double g2 = a1;
        if (fabs(a1) < fabs(a2)) {   // the frame sits at the point whose normal is nearer the line: acos(|a1|) > acos(|a2|)
            double s;
            s = n1x, n1x = n2x, n2x = s;
            s = n1y, n1y = n2y, n2y = s;
            s = n1z, n1z = n2z, n2z = s;
            dx = -dx, dy = -dy, dz = -dz;
            g2 = -a2;
        }
        double vx = dy * n1z - dz * n1y, vy = dz * n1x - dx * n1z, vz = dx * n1y - dy * n1x;   // dp x N1
        const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
        if (vn != 0.0) {
            vx = vx / vn, vy = vy / vn, vz = vz / vn;
            const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;   // N1 x v
            f1 = (vx * n2x + vy * n2y) + vz * n2z;
            f0 = atan2((wx * n2x + wy * n2y) + wz * n2z, (n1x * n2x + n1y * n2y) + n1z * n2z);
            f2 = g2;
        }
    }
    b0 = fpfh_bin((11.0 * (f0 + PI)) / (2.0 * PI));
    b1 = fpfh_bin((11.0 * (f1 + 1.0)) * 0.5);
    b2 = fpfh_bin((11.0 * (f2 + 1.0)) * 0.5);
}
