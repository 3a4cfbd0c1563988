// Surface normals and curvature of 3-D clouds from their k-nearest-neighbour lists on the device (gfx950): the PCA normal of each
// query's neighbourhood and its "surface variation", what PCL and Open3D compute directly after the neighbour search.  The reference
// has nothing of the kind; the route without this file is knn_gather (a (B, M, k, 3) tensor), a mean, an einsum and torch.linalg.eigh
// on B * M little 3 x 3 matrices.
//
// Definition (gecco_normals_f32, include/gecco_hip.h; tests/_normals_ref.py restates it in numpy float32).  For query i the
// neighbourhood is the points idx[i, t] with d2[i, t] <= radius2 (all k without a radius), m of them; mu = sum p / m and
// C = sum (p - mu)(p - mu)^T / m in TWO passes, centred, in fp32; the eigenpairs of C by NORMALS_SWEEPS cyclic Jacobi sweeps over
// (0,1), (0,2), (1,2) on C / trace(C); normal = the unit eigenvector of the smallest eigenvalue, curvature = lambda0 / (lambda0 +
// lambda1 + lambda2).  Rows with m < 3, a non-finite coordinate or a trace that is not a positive finite number are invalid: (0, 0, 1),
// zeros.  Sign: towards the viewpoint, or the component of largest magnitude positive (the lowest axis among equals).
//
// Kernel.  One thread owns one query; a workgroup of T = 64, 128 or 256 threads owns T consecutive rows of idx (and of d2 when a radius
// uses it), which are T * k consecutive words of memory: they are read coalesced and staged in LDS with the row pitch k | 1 (odd, so
// the lanes of a wave, each walking its own row, fall on different banks).  A row read straight from memory by its lane would be a
// stride-k access.  The two passes gather the neighbours' coordinates from the reference cloud (12-byte reads at random places of a
// cloud that sits in L2: 100 000 points are 1.2 MB); the second pass finds them in cache.  Which of the k entries count is a 64-bit
// mask in registers (k <= 64).  Every loop has a trip count that depends on k alone; nothing is shared between queries after the
// staging, there are no atomics and no workgroup waits on another, so a row's bits depend on that row's inputs and nothing else.
#include "cloud_nn.h"
#include "kernels.h"
#include "launch_state.h"

namespace {

constexpr int NORMALS_SWEEPS = 4;
static_assert(GECCO_KNN_MAX_K <= 64, "the neighbourhood mask of a query is one 64-bit word");
static_assert(2 * 4 * 256 * 17 <= 64 * 1024 && 2 * 4 * 128 * 33 <= 64 * 1024 && 2 * 4 * 64 * (GECCO_KNN_MAX_K | 1) <= 64 * 1024,
              "the idx and d2 tiles of a workgroup fit the LDS a kernel has without an opt-in (cloud_max_threads)");

// One Jacobi rotation that annihilates a_pq: app, aqq, apq the 2 x 2 block, (arp, arq) the third row's two entries, (v?p, v?q) the two
// eigenvector columns.  theta = (aqq - app) / (2 apq) overflows when apq is tiny: a non-finite theta gives t = 0 (the entry is already
// nothing beside the diagonal and is dropped), a theta whose square would overflow gives t = 1 / (2 theta).
static __device__ __forceinline__ void normals_rotate(float& app, float& aqq, float& apq, float& arp, float& arq, float& v0p, float& v0q,
                                                      float& v1p, float& v1q, float& v2p, float& v2q) {
    float t = 0.f;
    if (apq != 0.f) {
        const float theta = (aqq - app) / (2.f * apq);
        const float at = fabsf(theta);
        if (at <= 1e18f)
            t = copysignf(1.f, theta) / (at + sqrtf(theta * theta + 1.f));
        else if (at <= 3.402823466e38f)
            t = 0.5f / theta;
    }
    const float c = 1.f / sqrtf(t * t + 1.f), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.f;
    const float rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
    const float a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
    v0p = c * a0 - s * b0;
    v0q = s * a0 + c * b0;
    v1p = c * a1 - s * b1;
    v1q = s * a1 + c * b1;
    v2p = c * a2 - s * b2;
    v2q = s * a2 + c * b2;
}

// (lambda_a, column a) <-> (lambda_b, column b) when lambda_b < lambda_a
static __device__ __forceinline__ void normals_order(float& la, float& lb, float& xa, float& ya, float& za, float& xb, float& yb, float& zb) {
    if (lb < la) {
        float s;
        s = la, la = lb, lb = s;
        s = xa, xa = xb, xb = s;
        s = ya, ya = yb, yb = s;
        s = za, za = zb, zb = s;
    }
}

// grid: B * tiles blocks, block (b, tile) owns queries tile * T .. + T - 1 of cloud b.  d2 == null with a radius: the distances are
// recomputed from the coordinates (cloud_dist2_inf: the search's own roundings).  LDS: T * (k | 1) words of idx, then as many of d2
// when use_d2.
template <int T>
__global__ __launch_bounds__(T) void normals_kernel(const float* __restrict__ ref, const float* __restrict__ query, const int* __restrict__ idx,
                                                    const float* __restrict__ d2, const float* __restrict__ viewpoint, float radius2,
                                                    int use_radius, float* __restrict__ normal, float* __restrict__ eigenvalues,
                                                    float* __restrict__ curvature, int* __restrict__ count, int M, int N, int k, int tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char normals_lds[];
    const int pitch = k | 1;
    int* const ids = reinterpret_cast<int*>(normals_lds);
    float* const dds = reinterpret_cast<float*>(normals_lds) + T * pitch;
    const bool use_d2 = use_radius && d2;

    const int tid = threadIdx.x;
    const int qt = (int)(blockIdx.x % (unsigned)tiles), b = (int)(blockIdx.x / (unsigned)tiles);
    const int rows = min(T, M - qt * T);
    const size_t base = ((size_t)b * M + (size_t)qt * T) * k;
    {   // the tile's rows * k consecutive words, word e of the tile to (row e / k, slot e % k); e advances by T per step
        const int words = rows * k, dr = T / k, dt = T % k;
        int r = tid / k, t = tid % k;
        for (int e = tid; e < words; e += T) {
            ids[r * pitch + t] = idx[base + e];
            if (use_d2) dds[r * pitch + t] = d2[base + e];
            r += dr;
            t += dt;
            if (t >= k) {
                t -= k;
                ++r;
            }
        }
    }
    __syncthreads();
    if (tid >= rows) return;   // (no barrier below)

    const int i = qt * T + tid;
    const size_t row = (size_t)b * M + i;
    const float* rb = ref + (size_t)b * N * 3;
    const float qx = query[row * 3], qy = query[row * 3 + 1], qz = query[row * 3 + 2];
    const int* mine = ids + tid * pitch;
    const float* myd = dds + tid * pitch;

    // pass 1: which entries count, their number and their sum.  An index outside [0, N) is never dereferenced: the row is invalid
    unsigned long long mask = 0;
    bool ok = cloud_finite3(qx, qy, qz);
    int m = 0;
    float sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll 4
    for (int t = 0; t < k; ++t) {
        const unsigned j = (unsigned)mine[t];
        if (j >= (unsigned)N) {
            ok = false;
            continue;
        }
        const float px = rb[3 * (size_t)j], py = rb[3 * (size_t)j + 1], pz = rb[3 * (size_t)j + 2];
        if (use_radius) {
            const float d = use_d2 ? myd[t] : cloud_dist2_inf(qx, qy, qz, px, py, pz);
            if (!(d <= radius2)) continue;
        }
        mask |= 1ull << t;
        ++m;
        ok = ok && cloud_finite3(px, py, pz);
        sx += px;
        sy += py;
        sz += pz;
    }
    const float inv_m = 1.f / (float)max(m, 1);
    const float ux = sx * inv_m, uy = sy * inv_m, uz = sz * inv_m;

    // pass 2: the centred second moments
    float cxx = 0.f, cxy = 0.f, cxz = 0.f, cyy = 0.f, cyz = 0.f, czz = 0.f;
#pragma unroll 4
    for (int t = 0; t < k; ++t) {
        if (!((mask >> t) & 1ull)) continue;
        const size_t j = (size_t)(unsigned)mine[t];
        const float dx = rb[3 * j] - ux, dy = rb[3 * j + 1] - uy, dz = rb[3 * j + 2] - uz;
        cxx += dx * dx;
        cxy += dx * dy;
        cxz += dx * dz;
        cyy += dy * dy;
        cyz += dy * dz;
        czz += dz * dz;
    }
    cxx *= inv_m, cxy *= inv_m, cxz *= inv_m, cyy *= inv_m, cyz *= inv_m, czz *= inv_m;
    const float trace = (cxx + cyy) + czz;
    ok = ok && m >= 3 && trace > 0.f && trace <= 3.402823466e38f;

    float nx = 0.f, ny = 0.f, nz = 1.f, l0 = 0.f, l1 = 0.f, l2 = 0.f, curv = 0.f;
    if (ok) {
        const float s = 1.f / trace;
        float a00 = cxx * s, a01 = cxy * s, a02 = cxz * s, a11 = cyy * s, a12 = cyz * s, a22 = czz * s;
        float v00 = 1.f, v01 = 0.f, v02 = 0.f, v10 = 0.f, v11 = 1.f, v12 = 0.f, v20 = 0.f, v21 = 0.f, v22 = 1.f;   // v[row][column]
#pragma unroll
        for (int sweep = 0; sweep < NORMALS_SWEEPS; ++sweep) {
            normals_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
            normals_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
            normals_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
        }
        l0 = fmaxf(a00, 0.f) * trace, l1 = fmaxf(a11, 0.f) * trace, l2 = fmaxf(a22, 0.f) * trace;   // C is positive semi-definite
        normals_order(l0, l1, v00, v10, v20, v01, v11, v21);
        normals_order(l1, l2, v01, v11, v21, v02, v12, v22);
        normals_order(l0, l1, v00, v10, v20, v01, v11, v21);
        const float rn = 1.f / sqrtf((v00 * v00 + v10 * v10) + v20 * v20);
        nx = v00 * rn, ny = v10 * rn, nz = v20 * rn;
        curv = l0 / ((l0 + l1) + l2);
        bool flip;
        if (viewpoint) {
            const float* v = viewpoint + 3 * (size_t)b;
            flip = (nx * (v[0] - qx) + ny * (v[1] - qy)) + nz * (v[2] - qz) < 0.f;
        } else {
            const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
            const float lead = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);   // the lowest axis among equal magnitudes
            flip = lead < 0.f;
        }
        if (flip) nx = -nx, ny = -ny, nz = -nz;
    }
    normal[row * 3] = nx;
    normal[row * 3 + 1] = ny;
    normal[row * 3 + 2] = nz;
    if (eigenvalues) {
        eigenvalues[row * 3] = l0;
        eigenvalues[row * 3 + 1] = l1;
        eigenvalues[row * 3 + 2] = l2;
    }
    if (curvature) curvature[row] = curv;
    if (count) count[row] = m;
}

}  // namespace

// One launch.  radius2 <= 0, +inf or NaN: no radius.  Returns -2 for sizes out of range, -3 when the grid would pass 2^31 - 1 workgroups.
int normals_launch(const float* ref, const float* query, const int* idx, const float* d2, const float* viewpoint, float radius2, float* normal,
                   float* eigenvalues, float* curvature, int* count, int B, int M, int N, int k, hipStream_t st) {
    if (B < 1 || M < 1 || N < 1 || k < 1 || k > GECCO_KNN_MAX_K) return -2;
    const int use_radius = radius2 > 0.f && radius2 <= 3.402823466e38f ? 1 : 0;
    // T: the most threads whose tiles stay near 32 KiB, halved by the plan (the direct form: one slice)
    const CloudPlan p = cloud_plan(B, M, N, 1, false, cloud_max_threads(k), device_cus());
    if (!p.fits()) return -3;
    const size_t lds = (size_t)4 * p.T * (k | 1) * ((use_radius && d2) ? 2 : 1);
    dispatch_T(p.T, [&](auto t) {
        hipLaunchKernelGGL(normals_kernel<decltype(t)::value>, dim3((unsigned)p.blocks), dim3(p.T), lds, st, ref, query, idx, d2, viewpoint,
                           radius2, use_radius, normal, eigenvalues, curvature, count, M, N, k, p.tiles);
    });
    return (int)hipGetLastError();
}
