// Layer 0 of a LinearLift evaluation from the 3-D points (option "lift0"), gfx950.
//
// The layer's input is x0 = lift(c_in p), an affine map of the points, and broadcast_norm is a per-sample, per-channel affine map
// (a1 * x0 + o1).  So for sample b every row of the layer's K | V | q is an affine function of three numbers:
//     [K | V | q](n) = M_b pt_n + c_b,   pt_n = c_in(sigma_b) p_n,
//     M_b = W diag(a1_b) W_lift  (3C x 3),   c_b = W (a1_b * b_lift + o1_b) + bias  (in_proj_b on the q rows, none on K | V).
// Three kernels, all fp32 with a fixed summation order:
//   lift0_fold_kernel   (M_b | c_b) as one float4 per output row: B x 3C x C x 4 multiply-adds;
//   lift0_rows_kernel   column ranges of M_b pt_n + c_b as fp16 / fp32 rows, head-major or row-major, in 16-byte pieces: replaces the
//                       (B N) x C -> 3C matrix product by a store stream;
//   lift0_pool_kernel   the pool attention of the 64 inducers over the N points without K | V: the scores are u_i . pt_n + w_i
//                       (u_i = scale A_k^T q_i, w_i = scale c_k . q_i) and the pooled values A_v (sum_n P_n pt_n) + c_v sum_n P_n, so a
//                       block keeps (max, sum P, sum P pt) per inducer and writes pool_attn_x3_kernel's partials.
#include "common.h"
#include "kernels.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int FOLD_MAX_C = 1024;    // channels of the fold's LDS table
constexpr int ROWS_THREADS = 192;   // a multiple of every piece count per row group the rows kernel takes (1, 2, 3, 4, 6, 8)
constexpr int ROWS_TILE = 256;      // rows per block
constexpr int POOL_WAVES = 16;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// mc[b, j] = {M_b[j, 0..2], c_b[j]} for rows j = row0 .. row1 - 1 of [kv_proj (2C) | q rows of in_proj (C)].
// One block = (256 rows, sample), one thread = one row: it walks its row of W four channels at a time against the sample's table in LDS
// (every lane reads the same entry: a broadcast) with one accumulator set per channel residue — four independent chains of C / 4 fused
// multiply-adds, summed 0 + 1 + 2 + 3 at the end: the same order on every run.  W (a few MB) stays in L2 across the samples.
__global__ __launch_bounds__(256) void lift0_fold_kernel(const float* __restrict__ kv_w, const float* __restrict__ q_w,
                                                         const float* __restrict__ q_b, const float* __restrict__ lift_w,
                                                         const float* __restrict__ lift_b, const float* __restrict__ a1,
                                                         const float* __restrict__ o1, float4* __restrict__ mc, int row0,
                                                         int row1, int C) {
    __shared__ float4 g[FOLD_MAX_C];   // per channel k: a1 * W_lift[k, 0..2], a1 * b_lift[k] + o1
    const int b = blockIdx.y;
    for (int k = threadIdx.x; k < C; k += 256) {
        const float a = a1[(size_t)b * C + k], o = o1[(size_t)b * C + k];
        g[k] = make_float4(a * lift_w[k * 3 + 0], a * lift_w[k * 3 + 1], a * lift_w[k * 3 + 2], fmaf(a, lift_b ? lift_b[k] : 0.f, o));
    }
    __syncthreads();
    const int j = row0 + blockIdx.x * 256 + threadIdx.x;
    if (j >= row1) return;
    const f32x4* wr = reinterpret_cast<const f32x4*>(j < 2 * C ? kv_w + (size_t)j * C : q_w + (size_t)(j - 2 * C) * C);   // C % 8 == 0
    float4 acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int k4 = 0; k4 < C / 4; ++k4) {
        const f32x4 wv = wr[k4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float4 gk = g[k4 * 4 + e];
            acc[e].x = fmaf(wv[e], gk.x, acc[e].x); acc[e].y = fmaf(wv[e], gk.y, acc[e].y);
            acc[e].z = fmaf(wv[e], gk.z, acc[e].z); acc[e].w = fmaf(wv[e], gk.w, acc[e].w);
        }
    }
    const float bias = (j >= 2 * C && q_b) ? q_b[j - 2 * C] : 0.f;
    mc[(size_t)b * 3 * C + j] = make_float4(((acc[0].x + acc[1].x) + acc[2].x) + acc[3].x, ((acc[0].y + acc[1].y) + acc[2].y) + acc[3].y,
                                            ((acc[0].z + acc[1].z) + acc[2].z) + acc[3].z, (((acc[0].w + acc[1].w) + acc[2].w) + acc[3].w) + bias);
}

struct RowsSeg {
    void* out;
    int col0, gw, ngroups, hm;   // first row of mc; columns per group (a head, or a slice of a row); groups; head-major
    int ld;                      // row-major: elements per row
};

// out[b, n, col0 + g * gw + 8 * piece ..] = M_b pt_n + c_b.  One block = (256-row tile, column group, sample); a thread keeps the
// (M | c) of its eight columns in registers and walks the tile's rows: every store is a whole 16-byte (fp16) / 32-byte (fp32) piece.
template <bool F16>
__global__ __launch_bounds__(ROWS_THREADS) void lift0_rows_kernel(const float* __restrict__ x, const float* __restrict__ coef,
                                                                  const float4* __restrict__ mc, RowsSeg s0, RowsSeg s1, int N,
                                                                  int C) {
    __shared__ float xs[ROWS_TILE * 3];
    const int b = blockIdx.z, n0 = blockIdx.x * ROWS_TILE, rows = min(ROWS_TILE, N - n0);
    const bool first = (int)blockIdx.y < s0.ngroups;
    const RowsSeg& s = first ? s0 : s1;
    const int grp = first ? blockIdx.y : blockIdx.y - s0.ngroups;
    const float cin = coef[4 * b + 2];
    for (int i = threadIdx.x; i < rows * 3; i += ROWS_THREADS) xs[i] = cin * x[((size_t)b * N + n0) * 3 + i];   // lift_kernel's c_in p
    const int P = s.gw >> 3, piece = threadIdx.x % P, rstep = ROWS_THREADS / P;
    float4 m[8];
    const float4* mp = mc + (size_t)b * 3 * C + s.col0 + grp * s.gw + piece * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = mp[e];
    __syncthreads();
    const size_t base = s.hm ? ((size_t)(b * s.ngroups + grp) * N + n0) * s.gw + piece * 8
                             : ((size_t)b * N + n0) * s.ld + grp * s.gw + piece * 8;
    const size_t rstride = s.hm ? s.gw : s.ld;
    for (int r = threadIdx.x / P; r < rows; r += rstep) {
        const float p0 = xs[r * 3 + 0], p1 = xs[r * 3 + 1], p2 = xs[r * 3 + 2];
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaf(p2, m[e].z, fmaf(p1, m[e].y, fmaf(p0, m[e].x, m[e].w)));
        if (F16) {
            u32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                typedef _Float16 h2 __attribute__((ext_vector_type(2)));
                const h2 pk = {(_Float16)v[2 * e], (_Float16)v[2 * e + 1]};
                o[e] = __builtin_bit_cast(unsigned, pk);
            }
            *reinterpret_cast<u32x4*>(static_cast<_Float16*>(s.out) + base + r * rstride) = o;
        } else {
            float* dst = static_cast<float*>(s.out) + base + r * rstride;
            *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
            *reinterpret_cast<f32x4*>(dst + 4) = f32x4{v[4], v[5], v[6], v[7]};
        }
    }
}

// One block = (sample, head, key split), the splits as pool_attn_x3_kernel cuts them.  Thread (wave, lane) = inducer `lane` over the
// keys wave, wave + 16, .. of the split.  A key is the same three numbers for every lane of a wave: its address is wave-uniform, so the
// points come through the scalar data cache into scalar registers (the constant address space and a wave index pinned in a scalar
// register keep the loop scalar code after the barriers too) and the key loop is vector arithmetic only: no LDS staging.  c_in is
// folded into u going in and into sum P pt coming out.  One pass with a running maximum per (wave, inducer) that shifts the sums kept so
// far (once per four keys) and the new terms alike, so every exponent is <= 0; the waves' (m, sums) are merged the way the splits' are.  part_o = sum_n P_n V_n (unnormalised), part_ml = (max, sum_n P_n)
// in the log2 domain: what inducer_chain_f16_kernel / pool_merge_kernel merge.  Every cross-wave sum runs in wave order.
__global__ __launch_bounds__(POOL_WAVES * 64) void lift0_pool_kernel(const float* __restrict__ x, const float* __restrict__ coef,
                                                                     const float4* __restrict__ mc, const float* __restrict__ ind,
                                                                     float* __restrict__ part_o, float* __restrict__ part_ml, int N,
                                                                     int C, int H, int HD, int nsplit) {
    constexpr int NW = POOL_WAVES;
    __shared__ float4 red[NW][64];
    __shared__ float redl[NW][64];
    const int lane = threadIdx.x & 63;
    int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    asm volatile("" : "+s"(wave));   // held in a scalar register: the key loops and their loads below are then scalar code
    const int bh = blockIdx.x / nsplit, split = blockIdx.x % nsplit;
    const int b = bh / H, hh = bh % H;
    const int ks = (((N + nsplit - 1) / nsplit) + 31) / 32 * 32;
    const int k_begin = split * ks, k_end = min(N, k_begin + ks);
    const int cnt = max(k_end - k_begin, 0);
    const float cin = coef[4 * b + 2];
    const float4* mk = mc + (size_t)b * 3 * C + hh * HD;   // this head's K rows; its V rows are C further
    const float4* mv = mk + C;
    // the split's points, read-only for the whole launch: through the constant address space, so that a wave-uniform address is a scalar load
    // after the barriers too
    typedef const __attribute__((address_space(4))) float* cfloat_p;
    const cfloat_p xp = (cfloat_p)(x + ((size_t)b * N + k_begin) * 3);

    // u (x, y, z) and w of inducer `lane`: the head dim in 4-wide pieces dealt to the waves
    {
        const float scale = LOG2E * rsqrtf((float)HD);
        const float* qi = ind + ((size_t)hh * 64 + lane) * HD;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int d0 = wave * 4; d0 < HD; d0 += NW * 4) {
            const f32x4 q4 = *reinterpret_cast<const f32x4*>(qi + d0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float4 k4 = mk[d0 + e];
                const float qs = q4[e] * scale;   // the scaled query, as pool_attn_x3_kernel forms it
                acc.x = fmaf(qs, k4.x, acc.x); acc.y = fmaf(qs, k4.y, acc.y); acc.z = fmaf(qs, k4.z, acc.z); acc.w = fmaf(qs, k4.w, acc.w);
            }
        }
        red[wave][lane] = acc;
    }
    __syncthreads();
    float4 u = red[0][lane];
#pragma unroll
    for (int w = 1; w < NW; ++w) { const float4 t = red[w][lane]; u.x += t.x; u.y += t.y; u.z += t.z; u.w += t.w; }
    __syncthreads();   // red is written again below
    u.x *= cin; u.y *= cin; u.z *= cin;   // scores on the raw points
    auto score = [&](float p0, float p1, float p2) { return fmaf(u.z, p2, fmaf(u.y, p1, fmaf(u.x, p0, u.w))); };

    // one pass, four keys at a time: the running maximum m shifts the sums kept so far (once per four keys) and the new terms alike, so
    // every exponent is <= 0.  A key past the split's end scores -inf (its term is 0); its address is clamped to the last key
    float m = -INFINITY, l = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
    for (int k = wave; k < cnt; k += 4 * NW) {
        float p[4][3], sc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int kk = k + j * NW, kc = min(kk, cnt - 1);
#pragma unroll
            for (int e = 0; e < 3; ++e) p[j][e] = xp[kc * 3 + e];
            sc[j] = kk < cnt ? score(p[j][0], p[j][1], p[j][2]) : -INFINITY;
        }
        const float mn = fmaxf(fmaxf(m, fmaxf(sc[0], sc[1])), fmaxf(sc[2], sc[3]));
        const float a = __builtin_amdgcn_exp2f(m - mn);   // v_exp_f32; m = -inf: 0
        l *= a; sx *= a; sy *= a; sz *= a;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float e = __builtin_amdgcn_exp2f(sc[j] - mn);
            l += e;
            sx = fmaf(e, p[j][0], sx); sy = fmaf(e, p[j][1], sy); sz = fmaf(e, p[j][2], sz);
        }
        m = mn;
    }
    redl[wave][lane] = m;
    red[wave][lane] = make_float4(sx, sy, sz, l);   // (the barrier above: every wave has read red's partial u)
    __syncthreads();
    float M = redl[0][lane];
#pragma unroll
    for (int w = 1; w < NW; ++w) M = fmaxf(M, redl[w][lane]);
    float4 S = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const float mw = redl[w][lane];
        const float f = mw == -INFINITY ? 0.f : exp2f(mw - M);   // a wave without keys (or a split without): nothing
        const float4 t = red[w][lane];
        S.x = fmaf(f, t.x, S.x); S.y = fmaf(f, t.y, S.y); S.z = fmaf(f, t.z, S.z); S.w = fmaf(f, t.w, S.w);
    }
    S.x *= cin; S.y *= cin; S.z *= cin;   // sum_n P_n (c_in p_n)
    const size_t pbase = ((size_t)bh * nsplit + split) * 64 + lane;
    for (int d = wave; d < HD; d += NW) {
        const float4 v4 = mv[d];
        part_o[pbase * HD + d] = fmaf(v4.z, S.z, fmaf(v4.y, S.y, fmaf(v4.x, S.x, v4.w * S.w)));
    }
    if (wave == 0) {
        part_ml[pbase * 2 + 0] = M;
        part_ml[pbase * 2 + 1] = S.w;
    }
}

int group_width(int ncols) {   // row-major: the widest column slice whose 16-byte pieces divide the block
    for (int gw : {64, 48, 32, 16, 8})
        if (ncols % gw == 0) return gw;
    return 0;
}

}  // namespace

bool lift0_supported(int C, int H) { return C >= 8 && C % 8 == 0 && C <= FOLD_MAX_C && H > 0 && C % H == 0; }
bool lift0_head_major_ok(int hd) { return hd >= 8 && hd % 8 == 0 && ROWS_THREADS % (hd / 8) == 0; }
bool lift0_pool_supported(int C, int H) { return lift0_supported(C, H) && (C / H) % 4 == 0; }

int lift0_fold_launch(const float* kv_w, const float* q_w, const float* q_b, const float* lift_w, const float* lift_b, const float* a1,
                      const float* o1, float* mc, int row0, int row1, int B, int C, hipStream_t st) {
    if (C > FOLD_MAX_C || row0 < 0 || row1 > 3 * C || row0 >= row1 || (row0 < 2 * C && !kv_w) || (row1 > 2 * C && !q_w)) return -3;
    if (B <= 0) return 0;
    hipLaunchKernelGGL(lift0_fold_kernel, dim3((row1 - row0 + 255) / 256, B), dim3(256), 0, st, kv_w, q_w, q_b, lift_w, lift_b, a1, o1,
                       reinterpret_cast<float4*>(mc), row0, row1, C);
    return (int)hipGetLastError();
}

int lift0_rows_launch(const float* x, const float* coef, const float* mc, const Lift0Seg* segs, int nseg, int f16, int B, int N, int C,
                      hipStream_t st) {
    if (nseg < 1 || nseg > 2 || B > 65535) return -3;
    if (B <= 0 || N <= 0) return 0;
    RowsSeg rs[2] = {};
    for (int i = 0; i < nseg; ++i) {
        const Lift0Seg& s = segs[i];
        if (s.ncols <= 0 || s.ncols % 8 || s.col0 < 0 || s.col0 + s.ncols > 3 * C) return -3;
        if (s.hd && (!lift0_head_major_ok(s.hd) || s.ncols % s.hd)) return -3;
        const int gw = s.hd ? s.hd : group_width(s.ncols);
        rs[i] = RowsSeg{s.out, s.col0, gw, s.ncols / gw, s.hd != 0, s.ncols};
    }
    const dim3 grid((N + ROWS_TILE - 1) / ROWS_TILE, rs[0].ngroups + rs[1].ngroups, B);
    if (f16) hipLaunchKernelGGL(lift0_rows_kernel<true>, grid, dim3(ROWS_THREADS), 0, st, x, coef, reinterpret_cast<const float4*>(mc), rs[0], rs[1], N, C);
    else hipLaunchKernelGGL(lift0_rows_kernel<false>, grid, dim3(ROWS_THREADS), 0, st, x, coef, reinterpret_cast<const float4*>(mc), rs[0], rs[1], N, C);
    return (int)hipGetLastError();
}

int lift0_pool_launch(const float* x, const float* coef, const float* mc, const float* inducers, float* part_o, float* part_ml, int B,
                      int N, int C, int H, int nsplit, hipStream_t st) {
    if (!lift0_pool_supported(C, H) || nsplit < 1) return -3;
    if (B <= 0) return 0;
    hipLaunchKernelGGL(lift0_pool_kernel, dim3(B * H * nsplit), dim3(POOL_WAVES * 64), 0, st, x, coef, reinterpret_cast<const float4*>(mc), inducers,
                       part_o, part_ml, N, C, H, C / H, nsplit);
    return (int)hipGetLastError();
}
