// C ABI of libgecco_hip.so, part 3 of 4: AdaGN, attention forward and backward, lift / lower, the projective lookup,
// reparametrisation, the sampler, the pointwise backward kernels, the optimizer and the ConvNeXt conditioner.
#include "api_common.h"

#include <math.h>

using namespace gecco_api;

int gecco_api::make_lookup_args(const GeccoReparam* rp, const GeccoPyramid* pyr, LookupArgs* a) {
    if (!pyr || pyr->n_levels < 1 || pyr->n_levels > 4) return fail(-8, "lookup: 1..4 pyramid levels required");
    a->n_levels = pyr->n_levels;
    a->c_total = 0;
    for (int l = 0; l < 4; ++l) {
        const bool on = l < pyr->n_levels;
        a->C[l] = on ? pyr->C[l] : 0;
        a->H[l] = on ? pyr->H[l] : 1;
        a->W[l] = on ? pyr->W[l] : 1;
        a->feat[l] = on ? pyr->feat[l] : nullptr;
        if (on && !pyr->feat[l]) return fail(-1, "lookup: null pyramid level %d", l);
        a->c_total += a->C[l];
    }
    a->texel_f16 = pyr->texel_f16 ? 1 : 0;
    a->out_f16 = 0;
    a->reparam_kind = rp ? rp->kind : 0;
    a->rp_mean = rp ? rp->mean : nullptr;
    a->rp_std = rp ? rp->std : nullptr;
    a->logit_scale = rp ? rp->logit_scale : 1.1f;
    if (a->reparam_kind && (!a->rp_mean || !a->rp_std)) return fail(-1, "lookup: reparam buffers missing");
    return 0;
}

extern "C" {

int gecco_affine_cast_f16(const float* x, const float* a, const float* o, void* y16, int B, int rows, int C,
                          void* stream) {
    if (C % 8) return fail(-2, "affine_cast_f16: C must be a multiple of 8");
    TRY(affine_cast_f16_launch(x, a, o, y16, B, rows, C, (hipStream_t)stream), "affine_cast_f16");
    return 0;
}

int gecco_pool_attn_f16in(const void* KV16, const float* inducers, float* merged, int B, int N, int C, int H, int I,
                          int head_major, void* ws, size_t ws_bytes, void* stream) {
    if (ws_bytes < gecco_pool_attn_workspace_bytes(B, N, C, H, I)) return fail(-7, "pool_attn: workspace too small");
    Carver c(ws);
    const int ns = pool_attn_nsplit(B, N, H);
    float* po = c.f32((size_t)B * H * ns * 64 * (C / H));
    float* pml = c.f32((size_t)B * H * ns * 64 * 2);
    int rc = pool_attn_launch(static_cast<const float*>(KV16), inducers, po, pml, merged, B, N, C, H, I, ns,
                              (hipStream_t)stream, 2, 1, head_major != 0);
    if (rc == -9) return fail(-2, "pool_attn_f16in: head dim must be 16, 32, 48 or 64");
    TRY(rc, "pool_attn_f16in");
    return 0;
}

int gecco_lift0_fold_f32(const float* kv_w, const float* q_w, const float* q_b, const float* lift_w, const float* lift_b, const float* a1,
                         const float* o1, float* mc, int B, int C, int H, void* stream) {
    if (!kv_w || !q_w || !lift_w || !a1 || !o1 || !mc) return fail(-1, "lift0_fold: null argument");
    if (!lift0_supported(C, H)) return fail(-2, "lift0_fold: feature_dim must be a multiple of 8 and of the head count, at most 1024");
    TRY(lift0_fold_launch(kv_w, q_w, q_b, lift_w, lift_b, a1, o1, mc, 0, 3 * C, B, C, (hipStream_t)stream), "lift0_fold");
    return 0;
}

int gecco_lift0_rows(const float* x, const float* coef, const float* mc, void* out, int col0, int ncols, int head_dim, int out_f16,
                     int B, int N, int C, void* stream) {
    if (!x || !coef || !mc || !out) return fail(-1, "lift0_rows: null argument");
    if (ncols <= 0 || ncols % 8 || col0 < 0 || col0 + ncols > 3 * C) return fail(-2, "lift0_rows: columns must be a multiple of 8 inside 0 .. 3 * feature_dim");
    if (head_dim && (!lift0_head_major_ok(head_dim) || ncols % head_dim)) return fail(-2, "lift0_rows: head dim %d has no head-major form", head_dim);
    const Lift0Seg seg{out, col0, ncols, head_dim};
    TRY(lift0_rows_launch(x, coef, mc, &seg, 1, out_f16 != 0, B, N, C, (hipStream_t)stream), "lift0_rows");
    return 0;
}

int gecco_lift0_pool_f32(const float* x, const float* coef, const float* mc, const float* inducers, float* merged, int B, int N, int C,
                         int H, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !coef || !mc || !inducers || !merged || !ws) return fail(-1, "lift0_pool: null argument");
    if (!lift0_pool_supported(C, H)) return fail(-2, "lift0_pool: feature_dim must be a multiple of 8, at most 1024, the head dim a multiple of 4");
    if (ws_bytes < gecco_pool_attn_workspace_bytes(B, N, C, H, 64)) return fail(-7, "lift0_pool: workspace too small");
    Carver c(ws);
    const int ns = pool_attn_nsplit(B, N, H);
    float* po = c.f32((size_t)B * H * ns * 64 * (C / H));
    float* pml = c.f32((size_t)B * H * ns * 64 * 2);
    TRY(lift0_pool_launch(x, coef, mc, inducers, po, pml, B, N, C, H, ns, (hipStream_t)stream), "lift0_pool");
    TRY(pool_merge_launch(po, pml, merged, B, C, H, ns, (hipStream_t)stream), "lift0_pool merge");
    return 0;
}

int gecco_unpool_attn_f16io(const void* q16, const float* kvh, void* out16, int B, int N, int C, int H, int I,
                            int head_major, void* stream) {
    int rc = unpool_attn_launch(static_cast<const float*>(q16), kvh, static_cast<float*>(out16), B, N, C, H, I,
                                (hipStream_t)stream, 2, 1, head_major != 0);
    if (rc == -9) return fail(-2, "unpool_attn_f16io: head dim must be 16, 32, 48 or 64");
    TRY(rc, "unpool_attn_f16io");
    return 0;
}

int gecco_col_stats_f32(const float* x, float* stats, int B, int rows, int C, void* stream) {
    TRY(col_stats_launch(x, stats, B, rows, C, (hipStream_t)stream), "col_stats");
    return 0;
}

int gecco_adagn_coeffs_f32(const float* stats, int T, int rows, const float* t, int ctx_dim, const GeccoAdaGN* p,
                           float* a, float* o, int B, int C, int G, float eps, void* stream) {
    TRY(adagn_coeffs_launch(stats, T, rows, t, ctx_dim, p ? p->scale_w : nullptr, p ? p->scale_b : nullptr,
                            p ? p->bias_w : nullptr, p ? p->bias_b : nullptr, a, o, B, C, G, eps,
                            (hipStream_t)stream), "adagn_coeffs");
    return 0;
}

int gecco_affine_apply_f32(const float* x, const float* a, const float* o, float* y, int B, int rows, int C,
                           void* stream) {
    TRY(affine_apply_launch(x, a, o, y, B, rows, C, (hipStream_t)stream), "affine_apply");
    return 0;
}

size_t gecco_adagn_workspace_bytes(int B, int rows, int C) {
    Carver c(nullptr);
    c.f32((size_t)B * row_tiles_stats(rows) * 2 * C);
    c.f32((size_t)B * C);
    c.f32((size_t)B * C);
    return (c.off + 255) & ~size_t(255);
}

int gecco_adagn_f32(const float* x, const float* t, int ctx_dim, const GeccoAdaGN* p, float* y, int B, int rows,
                    int C, int G, float eps, void* ws, size_t ws_bytes, void* stream) {
    if (ws_bytes < gecco_adagn_workspace_bytes(B, rows, C)) return fail(-7, "adagn: workspace too small");
    Carver c(ws);
    float* stats = c.f32((size_t)B * row_tiles_stats(rows) * 2 * C);
    float* a = c.f32((size_t)B * C);
    float* o = c.f32((size_t)B * C);
    hipStream_t s = (hipStream_t)stream;
    TRY(col_stats_launch(x, stats, B, rows, C, s), "col_stats");
    TRY(adagn_coeffs_launch(stats, row_tiles_stats(rows), rows, t, ctx_dim, p ? p->scale_w : nullptr,
                            p ? p->scale_b : nullptr, p ? p->bias_w : nullptr, p ? p->bias_b : nullptr, a, o, B, C, G,
                            eps, s), "adagn_coeffs");
    TRY(affine_apply_launch(x, a, o, y, B, rows, C, s), "affine_apply");
    return 0;
}

size_t gecco_pool_attn_workspace_bytes(int B, int N, int C, int H, int I) {
    (void)I;
    Carver c(nullptr);
    const int ns = pool_attn_nsplit(B, N, H);
    c.f32((size_t)B * H * ns * 64 * (C / H));
    c.f32((size_t)B * H * ns * 64 * 2);
    return (c.off + 255) & ~size_t(255);
}

int gecco_pool_attn_ex_f32(const float* KV, const float* inducers, float* merged, int B, int N, int C, int H, int I,
                           int precision, void* ws, size_t ws_bytes, void* stream) {
    if (precision < 0 || precision > 2) return fail(-2, "pool_attn: precision must be 0 (fp32), 1 (split-bf16) or 2 (fp16)");
    if (ws_bytes < gecco_pool_attn_workspace_bytes(B, N, C, H, I)) return fail(-7, "pool_attn: workspace too small");
    Carver c(ws);
    const int ns = pool_attn_nsplit(B, N, H);
    float* po = c.f32((size_t)B * H * ns * 64 * (C / H));
    float* pml = c.f32((size_t)B * H * ns * 64 * 2);
    TRY(pool_attn_launch(KV, inducers, po, pml, merged, B, N, C, H, I, ns, (hipStream_t)stream, precision), "pool_attn");
    return 0;
}

int gecco_pool_attn_lse_f32(const void* ws, size_t ws_bytes, float* lse, int B, int N, int C, int H, int I, void* stream) {
    if (ws_bytes < gecco_pool_attn_workspace_bytes(B, N, C, H, I)) return fail(-7, "pool_attn_lse: workspace too small");
    Carver c(const_cast<void*>(ws));
    const int ns = pool_attn_nsplit(B, N, H);
    c.f32((size_t)B * H * ns * 64 * (C / H));
    const float* pml = c.f32((size_t)B * H * ns * 64 * 2);
    TRY(pool_attn_lse_launch(pml, lse, B, H, ns, (hipStream_t)stream), "pool_attn_lse");
    return 0;
}

int gecco_pool_attn_bwd_partials(int B, int N, int H) { return pool_attn_bwd_nsplit(B, N, H); }
int gecco_unpool_attn_bwd_partials(int B, int N, int H) { return unpool_attn_bwd_chunks(B, N, H, nullptr); }

int gecco_pool_attn_bwd_f32(const float* KV, const float* inducers, const float* merged, const float* lse, const float* dO,
                            float* dKV, float* dQ_partials, int B, int N, int C, int H, int I, void* stream) {
    return gecco_pool_attn_bwd_ex_f32(KV, inducers, merged, lse, dO, dKV, dQ_partials, B, N, C, H, I, 0, stream);
}
int gecco_unpool_attn_bwd_f32(const float* q, const float* kvh, const float* dO, float* dq, float* dkv_partials, int B, int N,
                              int C, int H, int I, void* stream) {
    return gecco_unpool_attn_bwd_ex_f32(q, kvh, dO, dq, dkv_partials, B, N, C, H, I, 0, stream);
}

int gecco_pool_attn_bwd_ex_f32(const float* KV, const float* inducers, const float* merged, const float* lse, const float* dO,
                               float* dKV, float* dQ_partials, int B, int N, int C, int H, int I, int precision, void* stream) {
    if (B <= 0 || N <= 0) return fail(-2, "pool_attn_bwd: empty batch");
    if (precision < 0 || precision > 3) return fail(-2, "pool_attn_bwd: precision must be 0 (fp32), 1 (split-bf16), 2 (fp16 operands) or 3 (fp16 operands, fp16 KV / dKV tensors)");
    const int rc = pool_attn_bwd_launch(KV, inducers, merged, lse, dO, dKV, dQ_partials, B, N, C, H, I, pool_attn_bwd_nsplit(B, N, H),
                                        (hipStream_t)stream, precision);
    if (rc == -3 || rc == -4) return fail(-2, "pool_attn_bwd: needs I == 64 and a head dim that is a multiple of 8 up to 64");
    TRY(rc, "pool_attn_bwd");
    return 0;
}

int gecco_unpool_attn_bwd_ex_f32(const float* q, const float* kvh, const float* dO, float* dq, float* dkv_partials, int B, int N,
                                 int C, int H, int I, int precision, void* stream) {
    if (B <= 0 || N <= 0) return fail(-2, "unpool_attn_bwd: empty batch");
    if (precision < 0 || precision > 3) return fail(-2, "unpool_attn_bwd: precision must be 0 (fp32), 1 (split-bf16), 2 (fp16 operands) or 3 (fp16 operands, fp16 q / dO / dq tensors)");
    const int rc = unpool_attn_bwd_launch(q, kvh, dO, dq, dkv_partials, B, N, C, H, I, (hipStream_t)stream, precision);
    if (rc == -3 || rc == -4) return fail(-2, "unpool_attn_bwd: needs I == 64 and a head dim that is a multiple of 8 up to 64");
    TRY(rc, "unpool_attn_bwd");
    return 0;
}

int gecco_pool_attn_f32(const float* KV, const float* inducers, float* merged, int B, int N, int C, int H, int I,
                        void* ws, size_t ws_bytes, void* stream) {
    return gecco_pool_attn_ex_f32(KV, inducers, merged, B, N, C, H, I, 0, ws, ws_bytes, stream);
}

int gecco_unpool_attn_ex_f32(const float* q, const float* kvh, float* out, int B, int N, int C, int H, int I,
                             int precision, void* stream) {
    if (precision < 0 || precision > 2) return fail(-2, "unpool_attn: precision must be 0 (fp32), 1 (split-bf16) or 2 (fp16)");
    TRY(unpool_attn_launch(q, kvh, out, B, N, C, H, I, (hipStream_t)stream, precision), "unpool_attn");
    return 0;
}

int gecco_unpool_attn_f32(const float* q, const float* kvh, float* out, int B, int N, int C, int H, int I,
                          void* stream) {
    return gecco_unpool_attn_ex_f32(q, kvh, out, B, N, C, H, I, 0, stream);
}

int gecco_edm_coeffs_f32(const float* sigma, float sigma_data, float* coef, int B, void* stream) {
    TRY(edm_coeffs_launch(sigma, sigma_data, coef, B, (hipStream_t)stream), "edm_coeffs");
    return 0;
}

int gecco_lift_f32(const float* x, const float* coef, const float* W, const float* bias, float* out, float* stats,
                   int B, int N, int C, void* stream) {
    TRY(lift_launch(x, coef, W, bias, out, stats, B, N, C, (hipStream_t)stream), "lift");
    return 0;
}

int gecco_lower_edm_f32(const float* feat, const float* x, const float* coef, const float* W, const float* bias,
                        const float* gn_a, const float* gn_o, float* out, float* raw, int B, int N, int C, float eps,
                        void* stream) {
    if (coef && !x) return fail(-1, "lower_edm: x required with coef");
    TRY(lower_edm_launch(feat, x, coef, W, bias, gn_a, gn_o, out, raw, B, N, C, eps, (hipStream_t)stream), "lower_edm");
    return 0;
}

int gecco_lift_g_f32(const float* x, const float* coef, const float* W, const float* bias, float* out, float* stats,
                     int B, int N, int C, int G, void* stream) {
    if (G < 1 || G > GECCO_MAX_GEOMETRY_DIM) return fail(-2, "lift_g: geometry_dim %d outside 1 .. %d", G, GECCO_MAX_GEOMETRY_DIM);
    TRY(lift_g_launch(x, coef, W, bias, out, stats, B, N, C, G, (hipStream_t)stream), "lift_g");
    return 0;
}

int gecco_lower_edm_g_f32(const float* feat, const float* x, const float* coef, const float* W, const float* bias, float* out,
                          float* raw, int B, int N, int C, int G, int do_norm, float eps, void* stream) {
    if (coef && !x) return fail(-1, "lower_edm_g: x required with coef");
    if (G < 1 || G > GECCO_MAX_GEOMETRY_DIM) return fail(-2, "lower_edm_g: geometry_dim %d outside 1 .. %d", G, GECCO_MAX_GEOMETRY_DIM);
    if (C <= 0 || C % 4 || C > 512) return fail(-2, "lower_edm_g: feature_dim %d (needs C %% 4 == 0, C <= 512)", C);
    TRY(lower_g_launch(feat, x, coef, W, bias, out, raw, B, N, C, G, do_norm, eps, (hipStream_t)stream), "lower_edm_g");
    return 0;
}

// ---------------------------------------------------------------------------- conditional path
int gecco_nchw_to_nhwc_f32(const float* src, float* dst, int B, int C, int H, int W, void* stream) {
    TRY(nchw_to_nhwc_launch(src, dst, B, C, H, W, (hipStream_t)stream), "nchw_to_nhwc");
    return 0;
}

int gecco_bilinear_taps_f32(const float* uv, int H, int W, int* x0, int* y0, float* wx1, float* wy1, size_t n,
                            void* stream) {
    TRY(bilinear_taps_launch(uv, H, W, x0, y0, wx1, wy1, n, (hipStream_t)stream), "bilinear_taps");
    return 0;
}

int gecco_lookup_row_tiles(int N) { return (N + lookup_row_tile() - 1) / lookup_row_tile(); }

int gecco_cast_f16(const float* src, void* dst, size_t n, void* stream) {
    if (n && (!src || !dst)) return fail(-1, "cast_f16: null argument");
    TRY(cast_f16_launch(src, dst, n, (hipStream_t)stream), "cast_f16");
    return 0;
}

int gecco_ray_lookup_f32(const float* geom, const float* coef, const float* K, const GeccoReparam* rp,
                         const GeccoPyramid* pyr, float* out, float* stats, int B, int N, void* stream) {
    if (!geom || !K || !out) return fail(-1, "ray_lookup: null argument");
    LookupArgs a;
    int rc = make_lookup_args(rp, pyr, &a);
    if (rc) return rc;
    TRY(ray_lookup_launch(geom, coef, K, a, out, stats, B, N, (hipStream_t)stream), "ray_lookup");
    return 0;
}

int gecco_ray_lookup_taps_f32(const float* geom, const float* coef, const float* K, const GeccoReparam* rp, const GeccoPyramid* pyr, float* uv,
                              int* x0, int* y0, float* wx1, float* wy1, int B, int N, void* stream) {
    if (!geom || !K || !pyr || !uv || !x0 || !y0 || !wx1 || !wy1) return fail(-1, "ray_lookup_taps: null argument");
    LookupArgs a;
    int rc = make_lookup_args(rp, pyr, &a);
    if (rc) return rc;
    TRY(ray_lookup_taps_launch(geom, coef, K, a, uv, x0, y0, wx1, wy1, B, N, (hipStream_t)stream), "ray_lookup_taps");
    return 0;
}

int gecco_ray_lookup_bwd_f32(const float* geom, const float* coef, const float* K, const GeccoReparam* rp,
                             const GeccoPyramid* pyr, const float* dout, float* const* dfeat, int B, int N,
                             void* stream) {
    if (!geom || !K || !dout || !dfeat || !pyr) return fail(-1, "ray_lookup_bwd: null argument");
    LookupArgs a;
    int rc = make_lookup_args(rp, pyr, &a);
    if (rc) return rc;
    if (a.texel_f16) return fail(-2, "ray_lookup_bwd: fp16 texel pyramids serve the forward lookup only (pass the fp32 levels)");
    for (int l = 0; l < a.n_levels; ++l)
        if (!dfeat[l]) return fail(-1, "ray_lookup_bwd: null gradient level");
    TRY(ray_lookup_bwd_launch(geom, coef, K, a, dfeat, dout, B, N, (hipStream_t)stream), "ray_lookup_bwd");
    return 0;
}

int gecco_ray_lookup_dgeom_f32(const float* geom, const float* K, const GeccoReparam* rp, const GeccoPyramid* pyr, const float* dout,
                               float* dgeom, float* dK_partials, int B, int N, void* stream) {
    if (!geom || !K || !dout || !pyr || (!dgeom && !dK_partials)) return fail(-1, "ray_lookup_dgeom: null argument");
    LookupArgs a;
    int rc = make_lookup_args(rp, pyr, &a);
    if (rc) return rc;
    if (a.texel_f16) return fail(-2, "ray_lookup_dgeom: fp16 texel pyramids serve the forward lookup only (pass the fp32 levels)");
    TRY(ray_lookup_dgeom_launch(geom, K, a, dout, dgeom, dK_partials, B, N, (hipStream_t)stream), "ray_lookup_dgeom");
    return 0;
}

size_t gecco_ray_lookup_bwd_sorted_workspace_bytes(const GeccoPyramid* pyr, int B, int N) {
    LookupArgs a;
    if (!pyr || make_lookup_args(nullptr, pyr, &a) || !ray_lookup_bwd_sorted_supported(a, N)) return 0;
    return ray_lookup_bwd_sorted_ws_bytes(a, B, N);
}
int gecco_ray_lookup_bwd_sorted_f32(const float* geom, const float* coef, const float* K, const GeccoReparam* rp,
                                    const GeccoPyramid* pyr, const float* dout, float* const* dfeat, int B, int N, void* ws,
                                    size_t ws_bytes, void* stream) {
    if (!geom || !K || !dout || !dfeat || !pyr || !ws) return fail(-1, "ray_lookup_bwd_sorted: null argument");
    LookupArgs a;
    int rc = make_lookup_args(rp, pyr, &a);
    if (rc) return rc;
    if (a.texel_f16) return fail(-2, "ray_lookup_bwd_sorted: fp16 texel pyramids serve the forward lookup only (pass the fp32 levels)");
    for (int l = 0; l < a.n_levels; ++l)
        if (!dfeat[l]) return fail(-1, "ray_lookup_bwd_sorted: null gradient level");
    if (!ray_lookup_bwd_sorted_supported(a, N)) return fail(-2, "ray_lookup_bwd_sorted: needs N <= 4096 and H W <= 2^17 per level");
    if (ws_bytes < ray_lookup_bwd_sorted_ws_bytes(a, B, N)) return fail(-3, "ray_lookup_bwd_sorted: workspace too small");
    TRY(ray_lookup_bwd_sorted_launch(geom, coef, K, a, dfeat, dout, B, N, ws, (hipStream_t)stream), "ray_lookup_bwd_sorted");
    return 0;
}

// ---------------------------------------------------------------------------- reparam / activation / sampler
int gecco_gaussian_reparam(const void* x, const float* mean, const float* sigma, void* y, size_t n_elems, int dim,
                           int inverse, int is_f64, void* stream) {
    TRY(gaussian_reparam_launch(x, mean, sigma, y, n_elems, dim, inverse, is_f64, (hipStream_t)stream),
        "gaussian_reparam");
    return 0;
}
int gecco_uvl_reparam(const void* x, const float* K, const float* uvl_mean, const float* uvl_std, double logit_scale,
                      void* y, int B, int N, int inverse, int is_f64, void* stream) {
    TRY(uvl_reparam_launch(x, K, uvl_mean, uvl_std, logit_scale, y, B, N, inverse, is_f64, (hipStream_t)stream),
        "uvl_reparam");
    return 0;
}
int gecco_relu_f32(const float* x, float* y, size_t n, void* stream) {
    TRY(relu_launch(x, y, n, (hipStream_t)stream), "relu");
    return 0;
}
int gecco_relu_bwd_f32(const float* y, const float* dy, float* du, size_t n, void* stream) {
    TRY(relu_bwd_launch(y, dy, du, n, (hipStream_t)stream), "relu_bwd");
    return 0;
}
int gecco_gaussian_act_f32(const float* x, const float* alpha, float* y, size_t n, int normalized, void* stream) {
    TRY(gaussian_act_launch(x, alpha, y, n, normalized, (hipStream_t)stream), "gaussian_act");
    return 0;
}
int gecco_sampler_add_noise_f64(const double* x_cur, const float* noise, size_t noise_step_stride, const double* sched,
                                const int* step, int col, int sigma_col, double* x_out, float* x_in, float* sigma,
                                size_t n, int B, void* stream) {
    TRY(sampler_add_noise_f64_launch(x_cur, noise, noise_step_stride, sched, step, col, sigma_col, x_out, x_in, sigma,
                                     n, B, (hipStream_t)stream), "sampler_add_noise_f64");
    return 0;
}
int gecco_sampler_add_noise_f32(const float* x, const float* noise, size_t noise_step_stride, const double* sched,
                                const int* step, int col, float* out, float* sigma, size_t n, int B, void* stream) {
    TRY(sampler_add_noise_f32_launch(x, noise, noise_step_stride, sched, step, col, out, sigma, n, B,
                                     (hipStream_t)stream), "sampler_add_noise_f32");
    return 0;
}
int gecco_sampler_euler_f64(const double* x_hat, const float* den, const double* sched, const int* step, double* d_cur,
                            double* x_next, float* x_in, float* sigma, size_t n, int B, void* stream) {
    TRY(sampler_euler_launch(x_hat, den, sched, step, d_cur, x_next, x_in, sigma, n, B, (hipStream_t)stream),
        "sampler_euler");
    return 0;
}
int gecco_sampler_heun_f64(const double* x_hat, const double* x_next, const float* den, const double* d_cur,
                           const double* sched, const int* step, double* x_out, size_t n, void* stream) {
    TRY(sampler_heun_launch(x_hat, x_next, den, d_cur, sched, step, x_out, n, (hipStream_t)stream), "sampler_heun");
    return 0;
}
int gecco_sampler_advance(int* step, int delta, void* stream) {
    TRY(sampler_advance_launch(step, delta, (hipStream_t)stream), "sampler_advance");
    return 0;
}
int gecco_sampler_scale_f64(const float* latents, double t0, double* x, size_t n, void* stream) {
    TRY(sampler_scale_launch(latents, t0, x, n, (hipStream_t)stream), "sampler_scale");
    return 0;
}

// ---------------------------------------------------------------------------- training path
int gecco_reduce_batch_f32(const float* parts, float* out, size_t n, int Z, size_t stride, int accumulate, void* stream) {
    TRY(reduce_batch_launch(parts, out, n, Z, stride, accumulate, (hipStream_t)stream), "reduce_batch");
    return 0;
}
int gecco_softmax_fwd_f32(const float* S, float* P, size_t rows, int n, float scale, void* stream) {
    TRY(softmax_fwd_launch(S, P, rows, n, scale, (hipStream_t)stream), "softmax_fwd");
    return 0;
}
int gecco_softmax_bwd_f32(const float* P, const float* dP, float* dS, size_t rows, int n, float scale, void* stream) {
    TRY(softmax_bwd_launch(P, dP, dS, rows, n, scale, (hipStream_t)stream), "softmax_bwd");
    return 0;
}
int gecco_gauss_act_bwd_blocks(size_t n) { return gauss_act_bwd_blocks(n); }
int gecco_gauss_act_bwd_f32(const float* u, const float* dy, const float* alpha, float* du, float* partial, size_t n,
                            int normalized, void* stream) {
    TRY(gauss_act_bwd_launch(u, dy, alpha, du, partial, n, normalized, (hipStream_t)stream), "gauss_act_bwd");
    return 0;
}
int gecco_col_dot_stats_f32(const float* dy, const float* x, float* gstats, int B, int rows, int C, void* stream) {
    TRY(col_dot_stats_launch(dy, x, gstats, B, rows, C, (hipStream_t)stream), "col_dot_stats");
    return 0;
}
int gecco_adagn_bwd_coeffs_f32(const float* xstats, int Tx, const float* gstats, int Tg, int rows, const float* t,
                               int ctx_dim, const GeccoAdaGN* p, float* cA, float* cB, float* cC, float* ds, float* dz,
                               int B, int C, int G, float eps, void* stream) {
    TRY(adagn_bwd_coeffs_launch(xstats, Tx, gstats, Tg, rows, t, ctx_dim, p ? p->scale_w : nullptr,
                                p ? p->scale_b : nullptr, cA, cB, cC, ds, dz, B, C, G, eps, (hipStream_t)stream),
        "adagn_bwd_coeffs");
    return 0;
}
int gecco_affine2_apply_f32(const float* dy, const float* x, const float* cA, const float* cB, const float* cC,
                            float* dx, int B, int rows, int C, void* stream) {
    TRY(affine2_apply_launch(dy, x, cA, cB, cC, dx, B, rows, C, (hipStream_t)stream), "affine2_apply");
    return 0;
}
int gecco_affine2_apply_add_f32(const float* dy, const float* x, const float* cA, const float* cB, const float* cC,
                                const float* add, float* dx, int B, int rows, int C, void* stream) {
    TRY(affine2_apply_launch(dy, x, cA, cB, cC, dx, B, rows, C, (hipStream_t)stream, add), "affine2_apply_add");
    return 0;
}
int gecco_adagn_param_grads_f32(const float* ds, const float* dz, const float* t, int B, int C, int ctx_dim,
                                float* d_scale_w, float* d_scale_b, float* d_bias_w, float* d_bias_b, void* stream) {
    TRY(adagn_param_grads_launch(ds, dz, t, B, C, ctx_dim, d_scale_w, d_scale_b, d_bias_w, d_bias_b,
                                 (hipStream_t)stream), "adagn_param_grads");
    return 0;
}
int gecco_lift_bwd_f32(const float* dY, const float* xin, float* partial, int B, int N, int C, void* stream) {
    TRY(lift_bwd_launch(dY, xin, partial, B, N, C, (hipStream_t)stream), "lift_bwd");
    return 0;
}
int gecco_lower_bwd_blocks(size_t rows) { return lower_bwd_blocks(rows); }
int gecco_lower_bwd_f32(const float* feat, const float* dF, const float* W, float* dfeat, float* partial, size_t rows,
                        int C, float eps, void* stream) {
    TRY(lower_bwd_launch(feat, dF, W, dfeat, partial, rows, C, eps, (hipStream_t)stream), "lower_bwd");
    return 0;
}

int gecco_lift_g_bwd_f32(const float* dY, const float* xin, float* partial, int B, int N, int C, int G, void* stream) {
    if (G < 1 || G > GECCO_MAX_GEOMETRY_DIM) return fail(-2, "lift_g_bwd: geometry_dim %d outside 1 .. %d", G, GECCO_MAX_GEOMETRY_DIM);
    TRY(lift_g_bwd_launch(dY, xin, partial, B, N, C, G, (hipStream_t)stream), "lift_g_bwd");
    return 0;
}
int gecco_lower_g_bwd_blocks(size_t rows) { return lower_g_bwd_blocks(rows); }
int gecco_lower_g_bwd_f32(const float* feat, const float* dF, const float* W, float* dfeat, float* partial, size_t rows,
                          int C, int G, int do_norm, float eps, void* stream) {
    if (G < 1 || G > GECCO_MAX_GEOMETRY_DIM) return fail(-2, "lower_g_bwd: geometry_dim %d outside 1 .. %d", G, GECCO_MAX_GEOMETRY_DIM);
    if (C <= 0 || C % 4 || C > 512) return fail(-2, "lower_g_bwd: feature_dim %d (needs C %% 4 == 0, C <= 512)", C);
    TRY(lower_g_bwd_launch(feat, dF, W, dfeat, partial, rows, C, G, do_norm, eps, (hipStream_t)stream), "lower_g_bwd");
    return 0;
}

// ---------------------------------------------------------------------------- optimizer
int gecco_adam_ema_step_f32(const GeccoAdamEma* a, void* stream) {
    return gecco_adam_ema_step_amp_f32(a, nullptr, nullptr, nullptr, stream);
}

// the argument checks and the derived scalars of a step; algorithm GECCO_CLIP_NONE: the unclipped kernel
static int adam_ema_step(const GeccoAdamEma* a, int algorithm, float clip_val, const float* stats, const float* amp_scale,
                         const float* found_inf, int* skipped, void* stream);

int gecco_adam_ema_step_amp_f32(const GeccoAdamEma* a, const float* amp_scale, const float* found_inf, int* skipped, void* stream) {
    return adam_ema_step(a, GECCO_CLIP_NONE, 0.f, nullptr, amp_scale, found_inf, skipped, stream);
}

int gecco_adam_ema_step_clip_f32(const GeccoAdamEma* a, int algorithm, float clip_val, const float* stats, const float* amp_scale,
                                 const float* found_inf, int* skipped, void* stream) {
    if (algorithm != GECCO_CLIP_NORM && algorithm != GECCO_CLIP_VALUE)
        return fail(-2, "adam_ema_clip: algorithm %d (1: norm, 2: value)", algorithm);
    if (algorithm == GECCO_CLIP_NORM) {
        if (!stats) return fail(-1, "adam_ema_clip: norm clipping reads stats[1] (gecco_grad_norm_f32 writes it)");
        if ((uintptr_t)stats & 3) return fail(-2, "adam_ema_clip: stats must be 4-byte aligned");
    } else if (!(clip_val >= 0.f) || !std::isfinite(clip_val)) {
        return fail(-2, "adam_ema_clip: clip_val must be finite and >= 0");
    }
    return adam_ema_step(a, algorithm, clip_val, stats, amp_scale, found_inf, skipped, stream);
}

size_t gecco_grad_norm_workspace_bytes(size_t n) { return (size_t)grad_norm_blocks(n) * sizeof(double); }

int gecco_grad_norm_f32(const float* g, size_t n, float grad_scale, const float* amp_scale, float max_norm, void* workspace,
                        size_t workspace_bytes, float* stats, void* stream) {
    if (!stats || (n && (!g || !workspace))) return fail(-1, "grad_norm: null argument");
    if (n % 4) return fail(-2, "grad_norm: n must be a multiple of 4 (pad the flat buffer)");
    if (((uintptr_t)g & 15) || ((uintptr_t)workspace & 7) || ((uintptr_t)stats & 3) || ((uintptr_t)amp_scale & 3))
        return fail(-2, "grad_norm: g must be 16-byte, workspace 8-byte, stats / amp_scale 4-byte aligned");
    if (n && workspace_bytes < gecco_grad_norm_workspace_bytes(n))
        return fail(-2, "grad_norm: workspace of %zu bytes, %zu needed", workspace_bytes, gecco_grad_norm_workspace_bytes(n));
    if (!std::isfinite(max_norm)) return fail(-2, "grad_norm: max_norm must be finite (<= 0: no clipping, coef = 1)");
    if (!std::isfinite(grad_scale)) return fail(-2, "grad_norm: grad_scale must be finite");
    TRY(grad_norm_launch(g, n, grad_scale, amp_scale, max_norm, (double*)workspace, stats, (hipStream_t)stream), "grad_norm");
    return 0;
}

static int adam_ema_step(const GeccoAdamEma* a, int algorithm, float clip_val, const float* stats, const float* amp_scale,
                         const float* found_inf, int* skipped, void* stream) {
    if (!a || !a->p || !a->g || !a->m || !a->v) return fail(-1, "adam_ema: null argument");
    if ((amp_scale || skipped) && !found_inf) return fail(-1, "adam_ema: amp_scale / skipped come with found_inf (the GradScaler protocol)");
    if (a->do_ema && !a->ema) return fail(-1, "adam_ema: do_ema needs the ema buffer");
    if (a->n % 4) return fail(-2, "adam_ema: n must be a multiple of 4 (pad the flat buffers)");
    if (a->step < 1) return fail(-2, "adam_ema: step is 1-based");
    const uintptr_t al = (uintptr_t)a->p | (uintptr_t)a->g | (uintptr_t)a->m | (uintptr_t)a->v | (uintptr_t)a->ema;
    if (al & 15) return fail(-2, "adam_ema: buffers must be 16-byte aligned");
    AdamEmaArgs k{};
    k.p = a->p; k.g = a->g; k.m = a->m; k.v = a->v; k.ema = a->ema; k.n = a->n;
    // every derived scalar in double first, like torch's Python scalars (torch/optim/adam.py _single_tensor_adam:
    // 1 - beta1, 1 - beta2, bias corrections, lr / bc1; ema.py:187-194: 1 - decay), then one rounding to fp32
    k.beta2 = (float)a->beta2; k.eps = (float)a->eps; k.weight_decay = (float)a->weight_decay;
    k.w1 = (float)(1.0 - a->beta1); k.w2 = (float)(1.0 - a->beta2);
    const double bc1 = 1.0 - pow(a->beta1, (double)a->step), bc2 = 1.0 - pow(a->beta2, (double)a->step);
    k.step_size = (float)(a->lr / bc1);
    k.bc2_sqrt = (float)sqrt(bc2);
    k.grad_scale = a->grad_scale; k.ema_decay = (float)a->ema_decay; k.ema_w = (float)(1.0 - a->ema_decay); k.do_ema = a->do_ema;
    k.amp_scale = amp_scale; k.found_inf = found_inf; k.skipped = skipped;
    k.lr = a->lr; k.beta1 = a->beta1; k.beta2d = a->beta2; k.step = a->step;
    if (algorithm == GECCO_CLIP_NONE) {
        TRY(adam_ema_launch(k, (hipStream_t)stream), "adam_ema");
    } else {
        TRY(adam_ema_clip_launch(k, algorithm, stats, clip_val, (hipStream_t)stream), "adam_ema_clip");
    }
    return 0;
}
int gecco_ema_update_f32(const float* p, float* ema, size_t n, double decay, void* stream) {
    if (!p || !ema) return fail(-1, "ema_update: null argument");
    if ((n % 4) || (((uintptr_t)p | (uintptr_t)ema) & 15)) return fail(-2, "ema_update: n %% 4 == 0 and 16-byte aligned buffers");
    TRY(ema_update_launch(p, ema, n, decay, (hipStream_t)stream), "ema_update");
    return 0;
}

// ---------------------------------------------------------------------------- samplers / metrics of the "next" rows
int gecco_sampler_refresh_known_f64(double* x, const float* known, const float* noise, const double* sched, const int* step,
                                    int col, int m, int n_known, int B, void* stream) {
    if (!x || !known || !noise || !sched || !step) return fail(-1, "sampler_refresh_known: null argument");
    TRY(sampler_refresh_known_launch(x, known, noise, sched, step, col, m, n_known, B, (hipStream_t)stream), "sampler_refresh_known");
    return 0;
}
int gecco_sampler_refresh_known_g_f64(double* x, const float* known, const float* noise, const double* sched, const int* step,
                                      int col, int m, int n_known, int width, int B, void* stream) {
    if (!x || !known || !noise || !sched || !step) return fail(-1, "sampler_refresh_known_g: null argument");
    if (width < 1) return fail(-2, "sampler_refresh_known_g: width %d", width);
    TRY(sampler_refresh_known_w_launch(x, known, noise, sched, step, col, m, n_known, width, B, (hipStream_t)stream),
        "sampler_refresh_known_g");
    return 0;
}

// ---------------------------------------------------------------------------- ConvNeXt conditioner (channels-last)
int gecco_convnext_stem_f32(const float* x, const float* w, const float* bias, const float* ln_w, const float* ln_b, float* out,
                            int B, int H, int W, int C, float eps, void* stream) {
    if (!x || !w || !bias || !ln_w || !ln_b || !out) return fail(-1, "convnext_stem: null argument");
    int rc = cnx_stem_launch(x, w, bias, ln_w, ln_b, out, nullptr, B, H, W, C, eps, (hipStream_t)stream);
    if (rc == -9) return fail(-2, "convnext_stem: needs C == 96 and H, W >= 4");
    TRY(rc, "convnext_stem");
    return 0;
}
int gecco_convnext_dwconv_ln_f32(const float* x, const float* w, const float* bias, const float* ln_w, const float* ln_b, float* out,
                                 int B, int H, int W, int C, float eps, void* stream) {
    if (!x || !w || !bias || !ln_w || !ln_b || !out) return fail(-1, "convnext_dwconv_ln: null argument");
    int rc = cnx_dwconv_ln_launch(x, w, bias, ln_w, ln_b, out, nullptr, B, H, W, C, eps, (hipStream_t)stream);
    if (rc == -9) return fail(-2, "convnext_dwconv_ln: C must be 96, 192, 384 or 768");
    TRY(rc, "convnext_dwconv_ln");
    return 0;
}
int gecco_convnext_ln_patch2_f32(const float* x, const float* ln_w, const float* ln_b, float* out, int B, int H, int W, int C,
                                 float eps, void* stream) {
    if (!x || !ln_w || !ln_b || !out) return fail(-1, "convnext_ln_patch2: null argument");
    int rc = cnx_ln_patch2_launch(x, ln_w, ln_b, out, B, H, W, C, eps, (hipStream_t)stream);
    if (rc == -9) return fail(-2, "convnext_ln_patch2: C must be 96, 192 or 384 and H, W >= 2");
    TRY(rc, "convnext_ln_patch2");
    return 0;
}
int gecco_convnext_fold_scale_f32(const float* W, const float* b, const float* s, float* Wo, float* bo, int N, int K, void* stream) {
    if (!W || !b || !s || !Wo || !bo) return fail(-1, "convnext_fold_scale: null argument");
    TRY(cnx_fold_scale_launch(W, b, s, Wo, bo, N, K, (hipStream_t)stream), "convnext_fold_scale");
    return 0;
}

// ---- the conditioner's training path
int gecco_convnext_stem_train_f32(const float* x, const float* w, const float* bias, const float* ln_w, const float* ln_b, float* out,
                                  float* z, int B, int H, int W, int C, float eps, void* stream) {
    if (!x || !w || !bias || !ln_w || !ln_b || !out || !z) return fail(-1, "convnext_stem_train: null argument");
    int rc = cnx_stem_launch(x, w, bias, ln_w, ln_b, out, z, B, H, W, C, eps, (hipStream_t)stream);
    if (rc == -9) return fail(-2, "convnext_stem_train: needs C == 96 and H, W >= 4");
    TRY(rc, "convnext_stem_train");
    return 0;
}
int gecco_convnext_dwconv_ln_train_f32(const float* x, const float* w, const float* bias, const float* ln_w, const float* ln_b,
                                       float* out, float* z, int B, int H, int W, int C, float eps, void* stream) {
    if (!x || !w || !bias || !ln_w || !ln_b || !out || !z) return fail(-1, "convnext_dwconv_ln_train: null argument");
    int rc = cnx_dwconv_ln_launch(x, w, bias, ln_w, ln_b, out, z, B, H, W, C, eps, (hipStream_t)stream);
    if (rc == -9) return fail(-2, "convnext_dwconv_ln_train: C must be 96, 192, 384 or 768");
    TRY(rc, "convnext_dwconv_ln_train");
    return 0;
}
int gecco_convnext_dwconv_f32(const float* x, const float* w, const float* bias, float* out, int B, int H, int W, int C, void* stream) {
    if (!x || !w || !out) return fail(-1, "convnext_dwconv: null argument");
    int rc = cnx_dwconv_ln_launch(x, w, bias, nullptr, nullptr, out, nullptr, B, H, W, C, 0.f, (hipStream_t)stream);
    if (rc == -9) return fail(-2, "convnext_dwconv: C must be 96, 192, 384 or 768");
    TRY(rc, "convnext_dwconv");
    return 0;
}
int gecco_convnext_dwconv_bwd_f32(const float* dz, const float* w, const float* add, float* dx, int B, int H, int W, int C, void* stream) {
    if (!dz || !w || !dx) return fail(-1, "convnext_dwconv_bwd: null argument");
    int rc = cnx_dwconv_ln_launch(dz, w, nullptr, nullptr, nullptr, dx, nullptr, B, H, W, C, 0.f, (hipStream_t)stream, add, 1);
    if (rc == -9) return fail(-2, "convnext_dwconv_bwd: C must be 96, 192, 384 or 768");
    TRY(rc, "convnext_dwconv_bwd");
    return 0;
}
int gecco_convnext_fold_scale_bwd_f32(const float* dWp, const float* dbp, const float* W, const float* b, const float* s, float* dW,
                                      float* db, float* ds, int N, int K, void* stream) {
    if (!dWp || !dbp || !W || !b || !s || !dW || !db || !ds) return fail(-1, "convnext_fold_scale_bwd: null argument");
    TRY(cnx_fold_scale_bwd_launch(dWp, dbp, W, b, s, dW, db, ds, N, K, (hipStream_t)stream), "convnext_fold_scale_bwd");
    return 0;
}
int gecco_convnext_ln_bwd_blocks(int B, int H, int W, int C) { return cnx_ln_bwd_blocks(B, H, W, C); }
int gecco_convnext_ln_bwd_f32(const float* z, const float* dy, const float* ln_w, float* dz, float* parts, int B, int H, int W, int C,
                              float eps, int patch2, void* stream) {
    if (!z || !dy || !ln_w || !dz || !parts) return fail(-1, "convnext_ln_bwd: null argument");
    int rc = cnx_ln_bwd_launch(z, dy, ln_w, dz, parts, B, H, W, C, eps, patch2, (hipStream_t)stream);
    if (rc == -9) return fail(-2, "convnext_ln_bwd: C must be 96, 192, 384 or 768 (and H, W >= 2 for the patch layout)");
    TRY(rc, "convnext_ln_bwd");
    return 0;
}
int gecco_convnext_dwconv_dw_blocks(int B, int H, int W, int C) { return cnx_dwconv_dw_blocks(B, H, W, C); }
int gecco_convnext_dwconv_dw_f32(const float* x, const float* dz, float* parts, int B, int H, int W, int C, void* stream) {
    if (!x || !dz || !parts) return fail(-1, "convnext_dwconv_dw: null argument");
    int rc = cnx_dwconv_dw_launch(x, dz, parts, B, H, W, C, (hipStream_t)stream);
    if (rc == -9) return fail(-2, "convnext_dwconv_dw: C must be 96, 192, 384 or 768");
    TRY(rc, "convnext_dwconv_dw");
    return 0;
}
int gecco_gelu_f32(const float* u, float* y, size_t n, void* stream) {
    if (!u || !y) return fail(-1, "gelu: null argument");
    int rc = gelu_launch(u, y, n, (hipStream_t)stream);
    if (rc == -9) return fail(-2, "gelu: n must be a multiple of 4");
    TRY(rc, "gelu");
    return 0;
}
int gecco_gelu_bwd_f32(const float* u, const float* dy, float* du, size_t n, void* stream) {
    if (!u || !dy || !du) return fail(-1, "gelu_bwd: null argument");
    int rc = gelu_bwd_launch(u, dy, du, n, (hipStream_t)stream);
    if (rc == -9) return fail(-2, "gelu_bwd: n must be a multiple of 4");
    TRY(rc, "gelu_bwd");
    return 0;
}
int gecco_convnext_im2col4_f32(const float* x, float* out, int B, int H, int W, void* stream) {
    if (!x || !out) return fail(-1, "convnext_im2col4: null argument");
    int rc = cnx_im2col4_launch(x, out, B, H, W, (hipStream_t)stream);
    if (rc == -9) return fail(-2, "convnext_im2col4: H, W must be >= 4");
    TRY(rc, "convnext_im2col4");
    return 0;
}

}  // extern "C"
