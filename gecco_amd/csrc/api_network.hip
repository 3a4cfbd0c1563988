// C ABI of libgecco_hip.so (declared in include/gecco_hip.h), part 1 of 4: the host-side orchestration of a SetTransformer evaluation (which kernel
// runs when, which buffer feeds which), its entry points, and the error buffer, option table and linears the other units share (api_common.h, api_linear.h).
// Nothing here allocates, synchronises or reads device memory, so a caller may capture any entry point in a hipGraph.
#include "api_linear.h"

#include <atomic>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <stdio.h>

using namespace gecco_api;

namespace {

// The option table (the OPT_* indices: api_common.h)
std::atomic<int> g_options[OPT_COUNT] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
const char* const g_option_names[OPT_COUNT] = {"astat", "chain", "headmajor", "mlpfused", "unpoolfused", "lo8", "actimg", "h8", "kvq64", "h8areg", "chain2", "unpoolh8", "mlpw", "chaincl", "h6", "kvfold", "mlpwshare", "kvqperm", "imgproj16", "lift0"};
const char* const g_option_env[OPT_COUNT] = {"GECCO_ASTAT", "GECCO_CHAIN", "GECCO_HEADMAJOR", "GECCO_MLPFUSED", "GECCO_UNPOOLFUSED", "GECCO_LO8",
                                             "GECCO_ACTIMG", "GECCO_H8", "GECCO_KVQ64", "GECCO_H8AREG", "GECCO_CHAIN2", "GECCO_UNPOOLH8", "GECCO_MLPW", "GECCO_CHAINCL", "GECCO_H6", "GECCO_KVFOLD", "GECCO_MLPWSHARE",
                                             "GECCO_KVQPERM", "GECCO_IMGPROJ16", "GECCO_LIFT0"};
// A plan's own switches (GeccoSetTransformer.opt_mask / opt_vals: gecco_option_index(name) is the bit) win over the process-wide ones
// while that plan's forward runs on this thread: two plans, or two host threads, never see each other's settings.
thread_local const GeccoSetTransformer* t_plan = nullptr;
struct PlanScope {
    const GeccoSetTransformer* prev;
    explicit PlanScope(const GeccoSetTransformer* p) : prev(t_plan) { t_plan = p; }
    ~PlanScope() { t_plan = prev; }
};

}  // namespace

namespace gecco_api {

thread_local char g_err[512] = "";

int fail(int rc, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return rc;
}

int option(int which) {
    if (t_plan && ((t_plan->opt_mask >> which) & 1u)) {
        const int v = (int)((t_plan->opt_vals >> which) & 1u);
        return which == OPT_LIFT0 && v ? v + (int)((t_plan->opt_vals >> OPT_LIFT0_HI) & 1u) : v;
    }
    int v = g_options[which].load(std::memory_order_relaxed);
    if (v < 0) {
        const char* e = getenv(g_option_env[which]);
        // "mlpwshare" (the one-launch MLP leaves CUs to a second stream's kernels) is off unless the caller runs two streams: hip_ops.py
        // sets it around a two-stream evaluation
        // "imgproj16" (img_feature_proj on one-term fp16 operands) is opt-in: 2 % of a C3 evaluation for a fifth of the w2 mode's error budget
        // "lift0" (layer 0 of a LinearLift evaluation from the 3-D points) has levels: 1 the projection, 2 the pool attention too; unset, it is 3:
        // level 2 at the widths where st_route finds it faster, 0 below them
        const int fill = which == OPT_LIFT0 ? (e ? (atoi(e) < 0 ? 0 : atoi(e) > 2 ? 2 : atoi(e)) : 3)
                         : e ? (atoi(e) != 0) : (which != OPT_MLPWSHARE && which != OPT_IMGPROJ16);
        // concurrent first reads fill in the same value; a gecco_set_option that got in between wins (v then holds its value)
        if (g_options[which].compare_exchange_strong(v, fill, std::memory_order_relaxed)) v = fill;
    }
    return v;
}

int linear(Lin& a, hipStream_t s) {   // works on a.g in place: no copy of the operands on the eager path
    GemmArgs& g = a.g;   // (mul_u / mul_kind / agrad: activation backward as the epilogue, LDS-DMA kernels only)
    const int precision = a.prec;
    g.precision = 0; g.w_img = nullptr;
    if (g.act < 0 || g.act > 4) return -6;
    if ((g.act == 1 || g.act == 2) && !g.alpha) return -6;
    const bool fast = precision == 1 ? gemm_f32_dma_supported(g, 1) : precision == 2 ? gemm_f16_dma_supported(g) : false;
    const bool img = a.wsplit || a.img_ready;
    if ((g.a_f16 || g.c_f16) && !(fast && precision == 2 && img)) return -9;
    if ((g.a_img || g.c_img) && !(fast && precision == 1 && img)) return -9;
    if ((g.mul_u || g.pre_out || g.dot_x) && !(precision == 0 ? gemm_f32_dma_supported(g, 0) : (fast && img))) return -9;
    if (!g.W && !(fast && a.img_ready)) return -9;
    if (fast && img) {
        if (a.img_ready) {
            g.w_img = a.img_ready;   // already converted this forward
        } else {
            int rc = precision == 1 ? split_bf16_tiled_launch(g.W, a.wsplit, g.Nout, g.K, g.ldw, s) : split_f16_tiled_launch(g.W, a.wsplit, g.Nout, g.K, g.ldw, s);
            if (rc) return rc;
            g.w_img = a.wsplit;
        }
        g.precision = precision;
    }
    return gemm_f32_launch(g, s);
}

int linear_pair(const Lin& a, const float* W2, const float* b2, int Nout2, float* C2, hipStream_t s) {
    GemmArgs g = a.g;
    const int precision = a.prec, Nout1 = a.g.Nout, K = a.g.K;
    if ((g.c_f16 || g.a_f16) && precision != 2) return -9;
    g.Nout = Nout1 + Nout2;
    g.C2 = C2; g.W2 = W2; g.bias2 = b2; g.n_split = Nout1; g.ldc2 = Nout2;
    if (precision == 2 ? !gemm_f16_dma_supported(g) : !gemm_f32_dma_supported(g)) return 1;
    if (precision == 1 || precision == 2) {
        if (a.img_ready) {
            g.w_img = a.img_ready;
        } else {
            if (!a.wsplit) return 1;
            const bool x3 = precision == 1;
            const ImageFormat plain = x3 ? ImageFormat(BF16_PLAIN) : ImageFormat(F16_PLAIN);
            const int rc = build_images(x3 ? launch_each<split_bf16_tiled_launch> : launch_each<split_f16_tiled_launch>, a.wsplit, K, s, {g.W, Nout1, K, plain}, {W2, Nout2, K, plain},
                                        x3 ? split_bf16_image_bytes(Nout1, K) : split_f16_image_bytes(Nout1, K));
            if (rc) return rc;
            g.w_img = a.wsplit;
        }
        g.precision = precision;
    }
    if (precision == 2) return gemm_f16_dma_launch(g, s);
    return gemm_f32_dma_launch(g, s);
}

}  // namespace gecco_api

namespace {

struct STWorkspace {
    float *big, *q, *attn;             // (B,N,2C), (B,N,C), (B,N,C)
    float *stats_x, *stats_s;          // (B,T,2,C) stream partials; (B,1,2,2C) inducer partials
    float *a1, *o1, *a2, *o2, *as, *os;  // AdaGN coefficients (B,C)
    float *part_o, *part_ml;           // pool partials
    float *merged, *h0, *u, *h2, *h, *kvh;  // inducer chain (B,I,*)
    float* wsplit;                     // tiled bf16 hi | lo image of the weight in use (unit calls, split-bf16 mode)
    float* wimg;                       // images of every layer's N-token weights, built once per forward
    // One layer's slot of `wimg`: where the image of each weight starts, in floats from the slot's start (kv_proj at 0).  A place is as large as the
    // weight's tiled image in the mode's own arithmetic (carve_st).  The image builder and the launches both read these.
    size_t wimg_layer, o_q, o_out, o_w0, o_w2;   // floats per layer; q_proj, unpool.out_proj, mlp.0, mlp.2
    size_t o_pout, o_b0, o_b2, o_ukv, b2_half;   // the 64-inducer chain: pool.out_proj, broadcast mlp, unpool k|v; its one-launch forms walk mlp.2 K-half by K-half
    size_t o_mf;                                 // fused point MLP: fp16 mode, its one stream (mlp_fused_f16_stream_jobs); w2 mode, mlp_fused_w.hip's
    size_t o_q16, o_kv_lo, o_q64;                // mixed mode: fp16 hi images of kv_proj | q_proj back to back, then kv_proj's lo image; the kvq stream's q tiles
    float* mc;                         // option "lift0": layer 0's folded (M_b | c_b), (B, 3C, 4)
    size_t bytes;
};

// What layer 0 of a LinearLift evaluation is an affine function of (option "lift0"): the points, the EDM coefficients (c_in) and the lift
struct Lift0In { const float *x, *coef, *lift_w, *lift_b; };

int max_i(int a, int b) { return a > b ? a : b; }

STWorkspace carve_st(const GeccoSetTransformer* st, int B, int N, void* base) {
    Carver c(base);
    STWorkspace w;
    const size_t C = st->C, I = st->I, W = st->width;
    const size_t big = (size_t)B * N * (2 * C > W ? 2 * C : W);
    w.big = c.f32(big);
    w.q = c.f32((size_t)B * N * C);
    w.attn = c.f32((size_t)B * N * C);
    const int T = max_i(row_tiles_gemm(N), row_tiles_stats(N));
    w.stats_x = c.f32((size_t)B * T * 2 * C);
    w.stats_s = c.f32((size_t)B * 2 * 2 * (2 * C > W ? 2 * C : W));
    w.a1 = c.f32(B * C); w.o1 = c.f32(B * C);
    w.a2 = c.f32(B * C); w.o2 = c.f32(B * C);
    w.as = c.f32(B * C); w.os = c.f32(B * C);
    const int ns = pool_attn_nsplit(B, N, st->H);
    const size_t HD = C / st->H;
    w.part_o = c.f32((size_t)B * st->H * ns * 64 * HD);
    w.part_ml = c.f32((size_t)B * st->H * ns * 64 * 2);
    w.merged = c.f32(B * I * C);
    w.h0 = c.f32(B * I * C);
    w.u = c.f32(B * I * W);
    w.h2 = c.f32(B * I * C);
    w.h = c.f32(B * I * C);
    w.kvh = c.f32(B * I * 2 * C);
    {   // tiled bf16 hi | lo image of the weight in use: output rows padded to the 128-column GEMM tile
        const size_t wmax = 3 * C + 128 > W ? 3 * C + 128 : W;   // kv_proj | q_proj share one image
        w.wsplit = c.f32(((wmax + 127) / 128 * 128) * (size_t)(W > C ? W : C));
    }
    {   // per layer: kv_proj | q_proj (contiguous: the fused pair streams them as one image), out_proj, mlp.0, mlp.2
        const int prec = st->precision == 4 ? 3 : st->precision;   // 4 ("w2") = the mixed mode with the one-launch point MLP
        // The size of a place, in floats: the weight's F16_PLAIN image in fp16 mode, else its BF16_PLAIN image.  The mixed mode keeps the split-bf16
        // size and builds its own formats (H8_*, the kvq stream, F16_HI_LO, F16_PLAIN + a lo image) inside it: none of them is larger
        auto img = [prec](size_t n, size_t k) { return (prec == 2 ? split_f16_image_bytes((int)n, (int)k) : split_bf16_image_bytes((int)n, (int)k)) / sizeof(float); };
        w.o_q = img(2 * C, C);
        w.o_out = w.o_q + img(C, C);
        w.o_w0 = w.o_out + img(C, C);
        w.o_w2 = w.o_w0 + img(W, C);
        w.o_pout = w.o_w2 + img(C, W);
        w.o_b0 = w.o_pout + img(C, C);
        w.o_b2 = w.o_b0 + img(W, C);
        w.o_ukv = w.o_b2 + img(C, W);
        w.o_mf = w.o_ukv + img(2 * C, C);
        w.wimg_layer = w.o_mf + (prec == 2 ? img(W, C) + img(C, W) : 0);   // (the stream of mlp_fused_f16_stream_jobs: as large as mlp.0's and mlp.2's images)
        // "w2" mode: the weight stream of the one-launch point MLP (mlp_fused_w.hip) at o_mf
        if (st->precision == 4 && mlp_fused_w_supported((int)C, (int)W, 128)) w.wimg_layer += mlp_fused_w_image_bytes((int)C, (int)W) / sizeof(float);
        w.wimg = prec >= 1 ? c.f32(w.wimg_layer * st->n_layers) : nullptr;
        w.b2_half = img(C, C);   // the image of one (C, C) K-half of the broadcast mlp.2: read by the one-launch chains only (chain_stream_fits)
        const size_t f16_kv = split_f16_image_bytes(2 * (int)C, (int)C) / sizeof(float), f16_q = split_f16_image_bytes((int)C, (int)C) / sizeof(float);
        w.o_q16 = f16_kv; w.o_kv_lo = f16_kv + f16_q;
        w.o_q64 = kvq_image_bytes(2 * (int)C, (int)C, (int)C) / sizeof(float);
    }
    w.mc = c.f32((size_t)B * 3 * C * 4);   // (last: every other place is where it was)
    w.bytes = (c.off + 255) & ~size_t(255);
    return w;
}

// The one-launch inducer chain reads pool.out_proj | broadcast.mlp.0 | mlp.2 | unpool k|v as ONE stream from o_pout: the four places must be consecutive and
// exactly filled by their images (fp16; at 4 bytes per weight element the hi | lo blocks of a two-term one), mlp.2's by its width / C K-half images
bool chain_stream_fits(const GeccoSetTransformer* st, const STWorkspace& w) {
    const size_t C = st->C, W = st->width;   // (false only after an edit that breaks carve_st: no shape the chain takes gets here)
    const bool f16 = st->precision == 2;      // the chain's F16_PLAIN images; else its F16_HI_LO ones: twice those, a BF16_PLAIN image's size
    auto img = [f16](size_t n, size_t k) { return (f16 ? split_f16_image_bytes((int)n, (int)k) : 2 * split_f16_image_bytes((int)n, (int)k)) / sizeof(float); };
    if (C % 128) return false;   // (a K-half image pads its C rows up to the column tile: the halves fill mlp.2's place only without pad rows)
    return w.o_b0 - w.o_pout == img(C, C) && w.o_b2 - w.o_b0 == img(W, C) && w.o_ukv - w.o_b2 == W / C * w.b2_half && w.o_mf - w.o_ukv == img(2 * C, C);
}

// fp16 mode: C16 (| C2_16) = fp16(act(fp16(x * pa + po) W^T + bias)) in one pass over x (gemm_f16_astat.hip).
// Returns 1 when the shape is outside that kernel's reach (caller: cast pass + streaming GEMM), 0 on success.
// kvq_perm / lo_fp8 say how the caller's builder made `img` / `img_lo` (StRoute::kvq_p48, StRoute::lo8).
int astat_linear(const float* x, const float* pa, const float* po, const float* img, const float* bias1, int Nout1,
                 float* C1, const float* bias2, int Nout2, float* C2, const float* alpha, int act, int B, int rows,
                 int K, hipStream_t s, int hm_hd = 0, const float* img_lo = nullptr, int use64 = 0, int kvq_perm = 0, int lo_fp8 = 0) {
    GemmArgs g = gemm_args_pair(x, bias1, C1, Nout1, bias2, C2, Nout2, B, rows, K);
    g.pro_a = pa; g.pro_o = po; g.precision = 2; g.w_img = img; g.c_f16 = 1; g.hm_hd = hm_hd;
    if (use64) {
        // mixed mode on the 64-column-tile kernel (gemm_h8_astat.hip: gemm_kvq_astat_kernel): `img` is the kvq stream — Nout1's
        // tiles, the V half of a K | V pair with its fp8 second weight term (use64 == 2), then Nout2's
        g.kvq_perm = kvq_perm; if (use64 == 2) { g.lo_begin = Nout1 / 128; g.lo_tiles = Nout1 / 64; }
        if (!img || act || !gemm_kvq_astat_supported(g)) return 1;
        return gemm_kvq_astat_launch(g, s);
    }
    g.alpha = alpha; g.act = act; g.w_img2 = img_lo;   // img_lo: two-term weights (mixed mode)
    // kv_proj | q_proj: two-term weights for the V half only; the K half and the q segment stay one-term
    if (img_lo && C2) { g.lo_begin = Nout1 / 256; g.lo_tiles = Nout1 / 128; }
    g.lo_fp8 = img_lo && lo_fp8;
    if (!img || !gemm_f16_astat_supported(g)) return 1;
    return gemm_f16_astat_launch(g, s);
}

// mixed mode: C = residual + A W^T + bias (+ statistics) with A an h8 activation image and W the 128-column-tile h8 stream
// (gemm_h8_areg.hip): mlp.2 and out_proj
int h8_linear(const float* a_img, const float* w_img, const float* bias, const float* res, float* C, float* stats, int B, int rows,
              int K, int Nout, hipStream_t s) {
    GemmArgs g = gemm_args(a_img, nullptr, bias, C, B, rows, K, Nout);
    g.residual = res; g.stats = stats; g.a_img = 2; g.w_img = w_img; g.precision = 1;
    return gemm_h8_areg_launch(g, s);
}

int coeffs(const float* stats, int T, int rows, const float* t, int ctx, const GeccoAdaGN* p, float* a, float* o,
           int B, int C, int G, hipStream_t s) {
    return adagn_coeffs_launch(stats, T, rows, t, ctx, p ? p->scale_w : nullptr, p ? p->scale_b : nullptr,
                               p ? p->bias_w : nullptr, p ? p->bias_b : nullptr, a, o, B, C, G, 1e-5f, s);
}

// The route of one SetTransformer evaluation: every path decision, taken ONCE (st_route) from the plan, the shape and the option table.
// The image builder and the launches read the same flags, so an image is in the format its consumer assumes.  This is the table of paths:
// a new kernel of this family adds its flag here and its condition to st_route.
struct StRoute {
    int rc;       // != 0: the evaluation is refused (the text is in g_err)
    int pr, apr, kmod, Tn, Ti, ns;   // arithmetic of the generic linears / of the attention products; K granularity of the fast kernels; row tiles of N / I; pool splits
    // precision 3 ("mixed"): kv_proj | q_proj with fp16 activations and TWO-TERM fp16 weights (A-stationary kernel), fp16 K | V / q and fp16 attention products; everything
    // that feeds the residual stream or the shared inducer states (pool.out_proj .. unpool k|v on the 64 inducers, unpool.out_proj, the point MLP) in split-bf16 arithmetic.
    // tools/experiments/fp16_site_sensitivity.py: those are the products whose operand rounding reaches the output. Shapes the A-stationary kv_proj | q_proj kernel does not
    // take (rows not a multiple of 128, C outside 128 .. 512 in steps of 128, head dims the fp16 attention kernels do not have) run the whole evaluation in split-bf16 — at
    // least as accurate, slower — instead of failing: a drop-in caller's N need not be a multiple of 128.
    bool mixed;
    bool astat;   // option "astat" = 0 falls back to the cast pass + streaming GEMM (A/B runs; same bits)
    bool imgs, build;   // the workspace holds every layer's weight images; this forward builds them (build_weight_images)
    // fp16 mode: the point-stream intermediates every consumer rounds to fp16 anyway (K|V, q, the attention output, the MLP hidden layer) are STORED as fp16 — the same bits
    // reach the matrix pipe, a third of the layer's HBM bytes never move.  x (the residual stream) and everything on the 64 inducers stay fp32.
    bool io16;
    bool a16;     // fp16-stored operands of the generic linears (fp16 mode only)
    // K | V and q leave the A-stationary kernel head-major: one contiguous (N, hd) slab per (sample, head), which is what a pool / unpool block streams (row-major: hd-wide
    // pieces of rows shared by all heads)
    int hd_try;
    // fp16 mode: the point-stream MLP of a layer (AdaGN, mlp.0, activation, mlp.2, residual, statistics) is one launch
    bool mlpf_on;
    // mixed mode: mlp.0 as fp16 main product + two fp8 cross terms, A-stationary over 256-row blocks (gemm_h8_astat.hip); its output is the tiled split image mlp.2 loads into
    // registers (option "actimg")
    bool h8_on;
    // mixed mode: kv_proj | q_proj on the 64-column-tile A-stationary kernel (option "kvq64"; two 128-row blocks per CU, W bytes shared by 128 rows, 16-byte head-major
    // stores).  The weight images are then built in the kvq format: a shape the kernel rejects is an error (-3) of the mixed mode, not a fallback (option "kvq64" = 0 selects
    // the 128-column-tile kernel and its images)
    bool kvq_on;
    // fp16 mode at feature_dim 512: the 128-column-tile A-stationary kernel needs 128 fragment registers + 128 accumulator registers there and spills
    // (gemm_f16_astat_kernel<16, 4, *>: 24 - 54 VGPRs to scratch); the 64-column-tile kernel takes the same one-term product without scratch (gemm_kvq_astat_kernel<8, 6>, no
    // L stages)
    bool kvq16_on;
    int use64;    // astat_linear's kernel for kv_proj | q_proj: 2 the kvq stream with L stages, 1 the one-term kvq stream, 0 128-column tiles
    bool kvq_p48; // head dim 48 has the kvq stream in the head-aligned column order (KVQ_HEAD48; option "kvqperm")
    bool lo8;     // the lo image of kv_proj as fp8 x 2^19 in 64-k blocks, where the A-stationary kernel has that form (option "lo8")
    // ... and mlp.2 / out_proj as h8 products fed from h8 activation images (gemm_h8_areg.hip; option "h8areg")
    bool h8x, h8o;
    // mixed mode, option "h6": mlp.0's two cross terms as fp6 x fp6 with per-block scales (half the matrix cycles of the fp8 form; its weight stream is built in the h6 form)
    // — where mlp.0 writes the h8 activation image (the kernel's only F6 instantiations)
    bool h6_on;
    // mixed mode: unpool attention + out_proj (h8) + residual + statistics in ONE launch (unpool_outproj_h8.hip; option "unpoolh8"): the attention output of a row block is
    // the stationary operand of out_proj and never leaves the CU.  Needs the head-major fp16 q of the kvq kernel; the k | v image of the inducers lives in the (then idle)
    // attention-output buffer
    bool uo8_on;
    // fp16 mode, head-major q: attention, out_proj, residual and statistics in one launch (the attention output of a row block is the A operand of out_proj for the same rows
    // and never leaves the CU)
    bool uof_on;
    // mixed mode: fp16 q in, fp32 attention output (io16 = 2) = the operand of the split-bf16 out_proj — handed over as a tiled split image where out_proj can load it
    // straight into registers (gemm_x3_areg.hip); o8: as the h8 activation image
    int aimg;
    bool o8;
    // split-bf16 products: the hidden layer goes from mlp.0 to mlp.2 as a tiled split image (same bytes as the fp32 tensor it replaces, in the same buffer): contiguous DMA
    // pieces and no hi / lo split in mlp.2's K loop
    int himg;
    // "w2" mode (option "mlpw" = 0 runs it as the mixed mode): the point MLP as ONE launch, the hidden layer kept as register fragments, its second term dropped
    // (mlp_fused_w.hip); the weight stream (1.9 MB at d = 384) has its own workspace slot (o_mf).  Shapes the kernel does not take (feature_dim off 128 .. 512 in steps of
    // 128, point counts off 128) run the mixed mode's two launches — at least as accurate
    bool mfw_on;
    int mfw_share;   // option "mlpwshare": that launch leaves CUs to a second stream's kernels
    // fp16 mode: everything on the 64 inducers between the two attentions is one launch (inducer_chain_f16.hip)
    bool chain_on;
    // mixed mode: the same one-launch chain with TWO-TERM fp16 weights (option "chain2") instead of five 64-row split-bf16 GEMMs and their coefficient launches: the chain's
    // activation rounding does not reach the output, its weight rounding does (tools/experiments/precision_search.py: chain = x2a keeps F_x at 1.0e-4 .. 1.3e-4) feature_dim
    // <= 384: at 512 one block per sample streams 7 MB of weights through one CU and loses to the five launches (C4, B = 32: 10.25 vs 10.03 ms per evaluation); the cluster
    // form (option "chaincl": 4 blocks per sample) wins there too (9.94 vs 10.12)
    bool chain2_on;
    bool chain;      // either of them, with the images there
    // the cluster form of the one-launch chain (option "chaincl"): its per-(layer, sample) counters live in `merged` (unused by the chain, 64 * C floats per sample) and are
    // zeroed once per forward
    bool chain_cl;
    // option "kvfold": the chain's last epilogue writes the fused unpool kernel's k | v image itself.  Only when EVERY layer runs the chain (no cached inducer states: their
    // layers bring the fp16 cast of x into the same buffer) — the image's pad positions are zeroed once per forward, and nothing else touches the buffer in between
    bool kvfold;
    // option "lift0", a LinearLift evaluation (the caller hands the points over): layer 0's K | V | q are M_b (c_in p_n) + c_b (lift0.hip).  1: K | V and q are written
    // from the points instead of by the (B N) x C -> 3C product; 2: q only, and the pool attention runs on the points — K | V of layer 0 never exist.  Any arithmetic
    // mode, any N; the tensors keep the element type (io16) and layout (lift0_hm: head-major) their consumers read
    int lift0;
    bool lift0_hm;
};

StRoute st_route(const GeccoSetTransformer* st, int B, int N, const float* const* h_in, bool points) {
    StRoute r{};
    const int C = st->C, I = st->I, H = st->H, G = st->G, Wd = st->width, act = st->act;
    const int prec = st->precision == 4 ? 3 : st->precision;   // 4 ("w2"): the mixed mode with the point MLP as one launch
    const bool wimg = prec >= 1;                                // carve_st gives the images their place in every mode but fp32
    const void* const some_img = st;                            // the *_supported tests only ask whether an image is there
    r.mixed = prec == 3 && N >= 128 && N % 128 == 0 && C % 128 == 0 && C <= 512 && !(C % H) &&
              attn_x3_supported(C / H) && st->I == 64 && option(OPT_ASTAT);
    const bool mixed = r.mixed;
    const int pr = r.pr = mixed ? 1 : (prec == 3 ? 1 : prec);
    r.apr = mixed ? 2 : pr;
    r.Tn = row_tiles_gemm(N); r.Ti = row_tiles_gemm(I); r.kmod = (pr == 2 || mixed) ? 32 : 16;
    const int ns = r.ns = pool_attn_nsplit(B, N, H);
    r.mlpf_on = pr == 2 && wimg && option(OPT_MLPFUSED) && mlp_fused_f16_supported(C, Wd, N);
    if (mixed && wimg && option(OPT_H8) && option(OPT_ACTIMG) && (act == 0 || (act >= 1 && act <= 3))) {
        GemmArgs hg{};
        hg.c_img = 1; hg.w_img = some_img; hg.rows = N; hg.Nout = Wd; hg.K = C; hg.lda = C; hg.act = act;
        r.h8_on = gemm_h8_astat_supported(hg) && Wd % 16 == 0 && C % 16 == 0;
    }
    r.kvq_on = mixed && wimg && option(OPT_KVQ64) && option(OPT_HEADMAJOR) && (C == 128 || C == 256 || C == 384 || C == 512) && !((C / H) & 7);
    r.kvq16_on = !mixed && pr == 2 && wimg && option(OPT_KVQ64) && option(OPT_HEADMAJOR) && option(OPT_ASTAT) && C == 512 &&
                 !((C / H) & 7) && N >= 128 && N % 128 == 0;
    auto h8_areg_takes = [&](int K) {   // an (N, K) h8 activation image times a (C, K) h8 stream
        GemmArgs hg{};
        hg.a_img = 2; hg.w_img = some_img; hg.rows = N; hg.Nout = C; hg.K = K; hg.lda = K; hg.ldc = C; hg.ldr = C;
        return gemm_h8_areg_supported(hg);
    };
    r.h8x = mixed && wimg && option(OPT_H8AREG) && option(OPT_ACTIMG) && Wd % 64 == 0 && N % 128 == 0 && h8_areg_takes(Wd);
    r.h8o = mixed && wimg && option(OPT_H8AREG) && option(OPT_ACTIMG) && I == 64 && C % 64 == 0 && attn_x3_supported(C / H) && h8_areg_takes(C);
    r.h6_on = r.h8_on && r.h8x && option(OPT_H6);
    r.uo8_on = r.h8o && r.kvq_on && option(OPT_UNPOOLH8) && I == 64 && unpool_outproj_h8_supported(C, H, N) &&
               unpool_outproj_h8_kv_bytes(B, C, H) <= (size_t)B * N * C * sizeof(float);
    r.mfw_on = mixed && st->precision == 4 && option(OPT_MLPW) && wimg && mlp_fused_w_supported(C, Wd, N) &&
               (size_t)B * N * C * sizeof(float) < ((size_t)1 << 31);
    r.mfw_share = r.mfw_on ? option(OPT_MLPWSHARE) : 0;
    r.chain_on = pr == 2 && wimg && option(OPT_CHAIN) && inducer_chain_f16_supported(C, Wd, H, G, I) &&
                 (ns == 1 || ns == 2 || ns == 4 || ns == 8);
    const bool cl_ok = option(OPT_CHAINCL) && C >= 256 && (size_t)st->n_layers * 8 <= (size_t)I * C;
    r.chain2_on = mixed && wimg && option(OPT_CHAIN2) && (C <= 384 || cl_ok) && inducer_chain_f16_supported(C, Wd, H, G, I) &&
                  (ns == 1 || ns == 2 || ns == 4 || ns == 8) && (act >= 0 && act <= 3);
    r.imgs = pr >= 1 && wimg && !(C % r.kmod) && !(Wd % r.kmod);
    r.build = r.imgs && !st->images_ready;
    r.astat = option(OPT_ASTAT);
    r.hd_try = option(OPT_HEADMAJOR) ? C / H : 0;
    r.use64 = r.kvq_on ? 2 : r.kvq16_on ? 1 : 0;
    r.kvq_p48 = r.kvq_on && option(OPT_KVQPERM) && r.hd_try && kvq_perm48_ok(C / H, C, 2 * C, C);
    r.lo8 = mixed && !r.kvq_on && option(OPT_LO8) && gemm_f16_astat_lo8_supported(C);
    r.io16 = (pr == 2 || mixed) && r.imgs && N >= 128 && attn_x3_supported(C / H) && !(C % 8) && !(Wd % 8);
    if (mixed && !(r.io16 && !(N % 128) && !(C % 128))) {
        r.rc = fail(-3, "set_transformer: the mixed mode needs rows %% 128 == 0, feature_dim %% 128 == 0 and a head dim of 16 / 32 / 48 / 64");
        return r;
    }
    r.a16 = r.io16 && !mixed;
    r.uof_on = !mixed && r.imgs && I == 64 && option(OPT_UNPOOLFUSED) && unpool_outproj_f16_supported(C, H, N);
    r.aimg = pr == 1 && !r.a16 && r.imgs && option(OPT_ACTIMG) && I == 64 && attn_x3_supported(C / H) && N >= 128 && N % 128 == 0 && C % 64 == 0;
    r.o8 = r.h8o && r.aimg && N % 128 == 0;
    r.himg = pr == 1 && !r.a16 && r.imgs && option(OPT_ACTIMG) && N >= 128 && N % 128 == 0 && Wd % 16 == 0 && C % 16 == 0;
    r.chain = (r.chain_on || r.chain2_on) && r.imgs;
    r.chain_cl = r.chain && cl_ok;
    r.kvfold = r.uo8_on && r.chain && option(OPT_KVFOLD);
    for (int li = 0; r.kvfold && li < st->n_layers; ++li)
        if (h_in && h_in[li]) r.kvfold = false;
    r.lift0 = points && lift0_supported(C, H) ? option(OPT_LIFT0) : 0;
    // unset: where it pays.  The kernels that replace the product cost about the same at every width (the pool on the points does not depend on it), the product
    // itself goes with C^2: B = 64, N = 2048, w2: C = 384 4.43 -> 4.33 ms per evaluation, C = 128 0.77 -> 0.80 ms (profiles/lift0_ab.txt)
    if (r.lift0 == 3) r.lift0 = C >= 256 ? 2 : 0;
    if (r.lift0 == 2 && !lift0_pool_supported(C, H)) r.lift0 = 1;
    r.lift0_hm = r.lift0 && r.io16 && r.astat && r.hd_try && lift0_head_major_ok(C / H);
    if (r.lift0 && r.uo8_on && !r.lift0_hm) r.lift0 = 0;   // (the fused unpool reads head-major q: every shape it takes has it)
    return r;
}

// Append to the job table of an image kernel.  Every insertion goes through here: the table is flushed (`launch`) BEFORE a write that would not fit.
template <class Job, int Cap, class Launch>
int push_job(Job (&table)[Cap], int& n, const Job& job, Launch launch) {
    if (n >= Cap) { const int rc = launch(); n = 0; if (rc) return rc; }
    table[n++] = job;
    return 0;
}
struct JobQueue {   // a SplitJobs table and the kernel that takes it
    SplitJobs jobs;
    int (*launch)(const SplitJobs&, hipStream_t);
    hipStream_t s;
    JobQueue(int (*launch_)(const SplitJobs&, hipStream_t), hipStream_t s_) : launch(launch_), s(s_) { jobs.n = 0; }
    int flush() { const int rc = launch(jobs, s); jobs.n = 0; return rc; }
    int push(const float* Wp, float* img, int Nout, int K, int ldw, ImageFormat format) {   // (a format of the builder `launch` is)
        return push_job(jobs.job, jobs.n, SplitJob{Wp, img, Nout, K, ldw, format}, [this] { return launch(jobs, s); });
    }
};

// Every N-token weight of every layer becomes its image in the layer's slot of w.wimg, in the format the route's consumer reads (weight_images.h): ONE launch
// per image kernel and 6 layers (weights may change between calls: nothing is cached across forwards unless the caller vouches for the workspace's images —
// GeccoSetTransformer.images_ready)
int build_weight_images(const StRoute& r, const GeccoSetTransformer* st, const STWorkspace& w, const float* const* h_in, hipStream_t s) {
    const int C = st->C, Wd = st->width, act = st->act;
    JobQueue jobs(r.pr == 2 ? split_f16_tiled_multi_launch : split_bf16_tiled_multi_launch, s);   // the tiled images of the mode's own arithmetic ...
    const ImageFormat plain = r.pr == 2 ? ImageFormat(F16_PLAIN) : ImageFormat(BF16_PLAIN);          // ... all in its builder's plain format
    JobQueue jobs16(split_f16_tiled_multi_launch, s);   // the fp16 images of the mixed mode (kv_proj | q_proj, hi and lo; the two-term chain)
    JobQueue jobs8(h8_image_multi_launch, s);           // the h8 images and the kvq streams
    MlpWImageJob mjobs[16];   // the one-launch point MLP's streams (w2 mode)
    int nmj = 0;
    auto flush_mj = [&] { return mlp_fused_w_images_launch(mjobs, nmj, C, Wd, act, s); };
    for (int li = 0; li < st->n_layers; ++li) {
        const GeccoLayer& L = st->layers[li];
        float* base = w.wimg + (size_t)li * w.wimg_layer;
        const bool cached = h_in && h_in[li];   // the layer's inducer states come from the caller: only q, out_proj and the point MLP run
        const bool own_kvq = r.mixed || r.kvq16_on;   // kv_proj | q_proj in an A-stationary kernel's own format
        const bool pts = li == 0 && r.lift0;          // layer 0's K | V | q come from the points: no stream of kv_proj / q_proj
        const bool kv_img = !cached && !pts, q_img = !pts;
        if (r.kvq_on) {
            // the kvq stream: K | V tiles (the V half with L stages), then the q tiles
            const KvqOrder order = r.kvq_p48 ? KVQ_HEAD48 : KVQ_PLAIN;
            if (kv_img) TRY(jobs8.push(L.kv_proj_w, base, 2 * C, C, C, kvq_format(C / 64, 2 * C / 64, order)), "split(kv_proj, kvq)");
            if (q_img) TRY(jobs8.push(L.in_proj_w, base + w.o_q64, C, C, C, kvq_format(0, 0, order)), "split(q_proj, kvq)");
        } else if (r.mixed) {
            // fp16 hi images of kv_proj | q_proj back to back (one stream for the A-stationary kernel), then kv_proj's lo image
            if (kv_img) TRY(jobs16.push(L.kv_proj_w, base, 2 * C, C, C, F16_PLAIN), "split(weights)");
            if (q_img) TRY(jobs16.push(L.in_proj_w, base + w.o_q16, C, C, C, F16_PLAIN), "split(weights)");   // q_proj is one-term: no lo image
            if (kv_img) TRY(jobs16.push(L.kv_proj_w, base + w.o_kv_lo, 2 * C, C, C, r.lo8 ? F16_LO_FP8 : F16_LO), "split(weights)");
        }
        const bool chain2_here = r.chain2_on && !cached;
        if (chain2_here) {
            // one stream of fp16 blocks, hi | lo per column tile, in the order the chain consumes them: pool.out_proj, broadcast.mlp.0,
            // broadcast.mlp.2 K-half by K-half, unpool k|v (carve_st: the four places are consecutive and as large as these images)
            TRY(jobs16.push(L.pool_out_w, base + w.o_pout, C, C, C, F16_HI_LO), "split(pool.out_proj, two-term)");
            TRY(jobs16.push(L.bmlp.w0, base + w.o_b0, Wd, C, C, F16_HI_LO), "split(broadcast.mlp.0, two-term)");
            for (int hf = 0; hf < Wd / C; ++hf)
                TRY(jobs16.push(L.bmlp.w2 + (size_t)hf * C, base + w.o_b2 + hf * w.b2_half, C, C, Wd, F16_HI_LO), "split(broadcast.mlp.2 K-half, two-term)");
            TRY(jobs16.push(L.in_proj_w + (size_t)C * C, base + w.o_ukv, 2 * C, C, C, F16_HI_LO), "split(unpool.in_proj kv, two-term)");
        }
        if (r.kvq16_on) {   // one-term kvq stream: K | V tiles, then the q tiles (o_q = the end of the kv image: 2 bytes per weight)
            if (kv_img) TRY(jobs8.push(L.kv_proj_w, base, 2 * C, C, C, kvq_format(0, 0)), "split(kv_proj, kvq)");
            if (q_img) TRY(jobs8.push(L.in_proj_w, base + w.o_q, C, C, C, kvq_format(0, 0)), "split(q_proj, kvq)");
        }
        if (!cached && !chain2_here) {
            if (!own_kvq && kv_img) TRY(jobs.push(L.kv_proj_w, base, 2 * C, C, C, plain), "split(kv_proj)");
            TRY(jobs.push(L.pool_out_w, base + w.o_pout, C, C, C, plain), "split(pool.out_proj)");
            TRY(jobs.push(L.bmlp.w0, base + w.o_b0, Wd, C, C, plain), "split(broadcast.mlp.0)");
            if (r.chain_on) {   // the one-launch chain walks mlp.2 K-half by K-half: one (C x C) image per half
                for (int hf = 0; hf < Wd / C; ++hf)
                    TRY(jobs.push(L.bmlp.w2 + (size_t)hf * C, base + w.o_b2 + hf * w.b2_half, C, C, Wd, plain), "split(broadcast.mlp.2 K-half)");
            } else {
                TRY(jobs.push(L.bmlp.w2, base + w.o_b2, C, Wd, Wd, plain), "split(broadcast.mlp.2)");
            }
        }
        if (!chain2_here) TRY(jobs.push(L.in_proj_w + (size_t)C * C, base + w.o_ukv, 2 * C, C, C, plain), "split(unpool.in_proj kv)");
        if (!own_kvq && q_img) TRY(jobs.push(L.in_proj_w, base + w.o_q, C, C, C, plain), "split(q_proj)");
        if (r.h8o) TRY(jobs8.push(L.unpool_out_w, base + w.o_out, C, C, C, r.uo8_on ? H8_ATTN_ORDER : H8_W128), "split(out_proj, h8)");
        else TRY(jobs.push(L.unpool_out_w, base + w.o_out, C, C, C, plain), "split(out_proj)");
        if (r.mlpf_on) {   // one stream in the kernel's consumption order (fp16 mode: `jobs` is the fp16 builder's queue)
            const int rc = mlp_fused_f16_stream_jobs(L.mlp.w0, L.mlp.w2, C, Wd, base + w.o_mf, [&jobs](const float* W, float* at, int Nout, int K, int ldw, F16Image format, const char* what) {
                return check(jobs.push(W, at, Nout, K, ldw, format), what);   // "split(mlp.0 tile)" / "split(mlp.2 K-slice)"
            });
            if (rc) return rc;
        } else if (r.mfw_on) {   // the one-launch point MLP's streams: all layers in one launch, behind the loop
            TRY(push_job(mjobs, nmj, MlpWImageJob{L.mlp.w0, L.mlp.b0, L.mlp.w2, L.mlp.b2, base + w.o_mf, L.mlp.alpha}, flush_mj), "split(mlp, w2 streams)");
        } else {
            // h8: same bytes as the split-bf16 image it replaces: fp16 hi + fp8 lo + fp8 W per element
            if (r.h8_on) TRY(jobs8.push(L.mlp.w0, base + w.o_w0, Wd, C, C, r.h6_on ? H8_H6 : H8_MLP0), "split(mlp.0, h8)");
            else TRY(jobs.push(L.mlp.w0, base + w.o_w0, Wd, C, C, plain), "split(mlp.0)");
            if (r.h8x) TRY(jobs8.push(L.mlp.w2, base + w.o_w2, C, Wd, Wd, H8_W128), "split(mlp.2, h8)");
            else TRY(jobs.push(L.mlp.w2, base + w.o_w2, C, Wd, Wd, plain), "split(mlp.2)");
        }
    }
    TRY(jobs.flush(), "split(weights)");
    if (r.mixed) TRY(jobs16.flush(), "split(weights, fp16)");
    TRY(jobs8.flush(), "split(mlp.0, h8)");
    if (nmj) TRY(flush_mj(), "split(mlp, w2 streams)");
    return 0;
}

// One layer of one evaluation: what its stages read, and what they hand each other
struct StLayer {
    const GeccoSetTransformer* st; const StRoute& r; const STWorkspace& w; const GeccoLayer& L; int li;
    const float* im;   // the layer's slot of weight images (null: none)
    float* x; const float* t; int B, N; hipStream_t s;
    const float* h;    // the inducer states: the caller's (cached: upsampling), else this layer's own once the inducer stage has run
    float *hdst, *so;  // where this layer's own inducer states go; where the point MLP leaves the statistics of its output
    bool cached, q_done = false, kvh_done = false, kv_img_done = false;
    int hm = 0;        // K | V and q of this layer are head-major
    const Lift0In* pts = nullptr;   // layer 0 on the route's "lift0" path: its K | V | q come from these
    const float* img(size_t off) const { return im ? im + off : nullptr; }
};

// kv_proj and the unpool's q projection read the same AdaGN(x): one launch, x read once.  y = AdaGN(x) is never materialised: (a1, o1) ride
// in the prologue of the GEMMs that read x
int project_stage(StLayer& c, bool with_kv) {
    const StRoute& r = c.r; const STWorkspace& w = c.w; const GeccoLayer& L = c.L;
    const int C = c.st->C, B = c.B, N = c.N;
    const bool io16 = r.io16, go = io16 && r.astat;
    // K | V (two-term V in the mixed mode) and q as two segments of one stream — or, over cached inducer states, q alone (one-term: its rounding stays inside)
    struct Seg { const float *img, *img_lo, *b1; int n1; float* c1; const float* b2; int n2; float* c2; int use64; };
    const Seg a = with_kv ? Seg{(2 * C) % 128 == 0 ? c.im : nullptr, r.mixed ? c.img(w.o_kv_lo) : nullptr, nullptr, 2 * C, w.big, L.in_proj_b, C, w.q, r.use64}
                          : Seg{c.img(r.kvq_on ? w.o_q64 : r.mixed ? w.o_q16 : w.o_q), nullptr, L.in_proj_b, C, w.q, nullptr, 0, nullptr, r.use64 ? 1 : 0};
    auto astat = [&](int hd) {   // (the head-aligned column order of the kvq stream is a head-major form)
        return astat_linear(c.x, w.a1, w.o1, a.img, a.b1, a.n1, a.c1, a.b2, a.n2, a.c2, nullptr, 0, B, N, C, c.s, hd, a.img_lo, a.use64, hd && r.kvq_p48, r.lo8);
    };
    int rc = go ? astat(r.hd_try) : 1;
    if (go && rc == 1 && r.hd_try) rc = astat(0);   // shape outside the head-major form: row-major
    if ((r.mixed || r.kvq16_on) && rc != 0)
        return with_kv ? fail(rc < 0 ? rc : -3, "set_transformer: kv_proj | q_proj outside the A-stationary kernel's reach (its weight images are in that kernel's format)")
                       : fail(rc < 0 ? rc : -3, "set_transformer: q projection outside the A-stationary kernel's reach (its weight image is in that kernel's format)");
    if (rc == 0 && r.hd_try) c.hm = 1;
    if (rc < 0) return check(rc, with_kv ? "kv_proj|q_proj (A-stationary)" : "unpool.in_proj(q) (A-stationary)");
    c.q_done = rc == 0;
    if (c.q_done || !with_kv) return 0;
    // the streaming kernels.  fp16 mode: AdaGN(x) is formed once as the fp16 operand both projections read (in the attention-output
    // buffer, idle until the unpool) instead of on every column tile's fragments
    if (io16) TRY(affine_cast_f16_launch(c.x, w.a1, w.o1, w.attn, B, N, C, c.s), "broadcast_norm -> fp16");
    Lin kv = Lin(io16 ? w.attn : c.x, L.kv_proj_w, nullptr, w.big, B, N, C, 2 * C).pro(io16 ? nullptr : w.a1, io16 ? nullptr : w.o1).f16(io16, io16);
    rc = linear_pair(Lin(kv).weights(r.pr, w.wsplit, (2 * C) % 128 == 0 ? c.im : nullptr), L.in_proj_w, L.in_proj_b, C, w.q, c.s);
    if (rc < 0) return check(rc, "kv_proj|q_proj");
    c.q_done = rc == 0;
    if (!c.q_done) TRY(linear(kv.weights(r.pr, w.wsplit, c.im), c.s), "kv_proj");
    return 0;
}

// Layer 0 on the "lift0" path: the fold of (a1, o1) and the lift into kv_proj | q_proj, then K | V | q (level 1), or q alone (level 2, and over cached inducer
// states), written from the points in the element type and layout project_stage leaves them in
int project_from_points(StLayer& c, bool with_kv) {
    const StRoute& r = c.r; const STWorkspace& w = c.w; const GeccoLayer& L = c.L;
    const int C = c.st->C, H = c.st->H, B = c.B, N = c.N;
    TRY(lift0_fold_launch(L.kv_proj_w, L.in_proj_w, L.in_proj_b, c.pts->lift_w, c.pts->lift_b, w.a1, w.o1, w.mc, with_kv ? 0 : 2 * C, 3 * C, B, C, c.s), "lift0 fold");
    const int hd = r.lift0_hm ? C / H : 0;
    const Lift0Seg segs[2] = {{w.q, 2 * C, C, hd}, {w.big, 0, 2 * C, hd}};
    TRY(lift0_rows_launch(c.pts->x, c.pts->coef, w.mc, segs, with_kv && r.lift0 == 1 ? 2 : 1, r.io16, B, N, C, c.s), "lift0 rows");
    c.hm = hd != 0;
    c.q_done = true;
    return 0;
}

// pool: the 64 inducer queries over the N points, then everything on the inducers up to the unpool's k | v — the one-launch chain, or
// out_proj, h = norm_2(mlp(norm_1(h0))) as five launches (the unpool stage then projects k | v)
int inducer_stage(StLayer& c) {
    const StRoute& r = c.r; const STWorkspace& w = c.w; const GeccoLayer& L = c.L; const GeccoSetTransformer* st = c.st; hipStream_t s = c.s;
    const int C = st->C, I = st->I, H = st->H, G = st->G, Wd = st->width, ctx = st->ctx_dim, act = st->act, B = c.B, pr = r.pr;
    if (c.pts && r.lift0 == 2) {   // the pool on the points: the same partials, K | V (w.big) neither written nor read
        TRY(lift0_pool_launch(c.pts->x, c.pts->coef, w.mc, L.inducers, w.part_o, w.part_ml, B, c.N, C, H, r.ns, s), "pool_attn (points)");
        if (!r.chain) TRY(pool_merge_launch(w.part_o, w.part_ml, w.merged, B, C, H, r.ns, s), "pool_attn merge");
    } else {
        TRY(pool_attn_launch(w.big, L.inducers, w.part_o, w.part_ml, r.chain ? nullptr : w.merged, B, c.N, C, H, I, r.ns, s, r.apr, r.io16, c.hm), "pool_attn");
    }
    if (r.chain) {
        ChainArgs ca{};
        ca.part_o = w.part_o; ca.part_ml = w.part_ml; ca.nsplit = r.ns; ca.H = H;
        ca.w_stream = c.im + w.o_pout;   // o_pout, o_b0, o_b2, o_ukv are consecutive (carve_st)
        ca.b0 = L.bmlp.b0; ca.b2 = L.bmlp.b2; ca.bkv = L.in_proj_b + C; ca.alpha = L.bmlp.alpha; ca.act = act; ca.two_term = r.chain2_on ? 1 : 0;
        ca.n1_scale_w = L.norm_1.scale_w; ca.n1_scale_b = L.norm_1.scale_b; ca.n1_bias_w = L.norm_1.bias_w; ca.n1_bias_b = L.norm_1.bias_b;
        ca.n2_scale_w = L.norm_2.scale_w; ca.n2_scale_b = L.norm_2.scale_b; ca.n2_bias_w = L.norm_2.bias_w; ca.n2_bias_b = L.norm_2.bias_b;
        ca.t = c.t; ca.ctx_dim = ctx; ca.G = G; ca.eps = 1e-5f; ca.h_out = c.hdst; ca.kvh = w.kvh; ca.B = B;
        if (r.chain_cl) {   // C / 128 blocks per sample; the stand-alone chain's buffers carry what they hand each other
            ca.cluster = 1; ca.x1 = w.h0; ca.x3 = w.h2; ca.xu = reinterpret_cast<unsigned*>(w.u);
            ca.flags = reinterpret_cast<unsigned*>(w.merged) + (size_t)c.li * B * 8;
        }
        if (r.kvfold) {   // k | v leave the chain as the fused unpool kernel's fp16 image (pads zeroed by st_forward): no fp32 kvh, no reformat pass
            ca.kv_img = reinterpret_cast<unsigned short*>(w.attn);
            ca.kv_img_bytes = (int)(unpool_outproj_h8_kv_bytes(1, C, H) / H);
            c.kv_img_done = true;
        }
        if ((act == 1 || act == 2) && !L.bmlp.alpha) return fail(-6, "inducer chain: GaussianActivation needs alpha");
        TRY(inducer_chain_f16_launch(ca, C, Wd, s), "inducer chain");
        c.kvh_done = true;
    } else {
        TRY(linear(Lin(w.merged, L.pool_out_w, nullptr, w.h0, B, I, C, C).with_stats(w.stats_s).weights(pr, w.wsplit, c.img(w.o_pout)), s), "pool.out_proj");
        TRY(coeffs(w.stats_s, r.Ti, I, c.t, ctx, &L.norm_1, w.as, w.os, B, C, G, s), "adagn_coeffs(norm_1)");
        TRY(linear(Lin(w.h0, L.bmlp.w0, L.bmlp.b0, w.u, B, I, C, Wd).pro(w.as, w.os).activation(act, L.bmlp.alpha).weights(pr, w.wsplit, c.img(w.o_b0)), s), "broadcast.mlp.0");
        TRY(linear(Lin(w.u, L.bmlp.w2, L.bmlp.b2, w.h2, B, I, Wd, C).with_stats(w.stats_s).weights(pr, w.wsplit, c.img(w.o_b2)), s), "broadcast.mlp.2");
        TRY(coeffs(w.stats_s, r.Ti, I, c.t, ctx, &L.norm_2, w.as, w.os, B, C, G, s), "adagn_coeffs(norm_2)");
        TRY(affine_apply_launch(w.h2, w.as, w.os, c.hdst, B, I, C, s), "norm_2 apply");
    }
    c.h = c.hdst;
    return 0;
}

// unpool: k|v of the 64 inducer states, q of the N points (unless the projection stage made it), attention, out_proj + residual
int unpool_stage(StLayer& c) {
    const StRoute& r = c.r; const STWorkspace& w = c.w; const GeccoLayer& L = c.L; float* x = c.x; hipStream_t s = c.s;
    const int C = c.st->C, I = c.st->I, H = c.st->H, B = c.B, N = c.N, pr = r.pr;
    const bool io16 = r.io16;
    if (!c.kvh_done)
        TRY(linear(Lin(c.h, L.in_proj_w + (size_t)C * C, L.in_proj_b + C, w.kvh, B, I, C, 2 * C).weights(pr, w.wsplit, c.img(w.o_ukv)), s), "unpool.in_proj(kv)");
    if (!c.q_done && io16 && c.cached)
        if (const int rc = project_stage(c, false)) return rc;
    if (!c.q_done) {
        if (io16 && c.cached) TRY(affine_cast_f16_launch(x, w.a1, w.o1, w.attn, B, N, C, s), "broadcast_norm -> fp16");
        TRY(linear(Lin(io16 ? w.attn : x, L.in_proj_w, L.in_proj_b, w.q, B, N, C, C).pro(io16 ? nullptr : w.a1, io16 ? nullptr : w.o1)
                       .weights(pr, w.wsplit, c.img(w.o_q)).f16(io16, io16), s), "unpool.in_proj(q)");
    }
    if (r.uo8_on) {
        if (!c.hm || !c.im) return fail(-3, "set_transformer: unpool + out_proj (h8) needs the head-major fp16 q");
        if (!c.kv_img_done) TRY(kvh_image_launch(w.kvh, w.attn, B, C, H, s), "unpool k | v image");
        UnpoolH8Args ua{};
        ua.x = x; ua.q16 = w.q; ua.kv_img = w.attn; ua.w_img = c.im + w.o_out; ua.bias = L.unpool_out_b; ua.stats = w.stats_x; ua.B = B; ua.rows = N; ua.H = H;
        TRY(unpool_outproj_h8_launch(ua, C, s), "unpool attention + out_proj (h8)");
    } else if (r.uof_on && c.hm) {
        UnpoolProjArgs ua{};
        ua.x = x; ua.q16 = w.q; ua.kvh = w.kvh; ua.w_stream = c.im + w.o_out; ua.bias = L.unpool_out_b; ua.stats = w.stats_x; ua.B = B; ua.rows = N; ua.H = H;
        TRY(unpool_outproj_f16_launch(ua, C, s), "unpool attention + out_proj");
    } else {
        TRY(unpool_attn_launch(w.q, w.kvh, w.attn, B, N, C, H, I, s, r.apr, r.mixed ? 2 : (int)io16, c.hm, r.o8 ? 2 : r.aimg), "unpool_attn");
        if (r.o8)
            TRY(h8_linear(w.attn, c.im + w.o_out, L.unpool_out_b, x, x, w.stats_x, B, N, C, C, s), "unpool.out_proj+residual (h8)");
        else
            TRY(linear(Lin(w.attn, L.unpool_out_w, L.unpool_out_b, x, B, N, C, C).plus(x).with_stats(w.stats_x).weights(pr, w.wsplit, c.img(w.o_out))
                           .f16(r.a16, 0).image(r.aimg, 0), s), "unpool.out_proj+residual");
    }
    return 0;
}

// x += mlp(AdaGN(x)), the statistics of the result to c.so: fused fp16 / one launch (w2) / the h8 pair / the generic linears
int mlp_stage(StLayer& c) {
    const StRoute& r = c.r; const STWorkspace& w = c.w; const GeccoLayer& L = c.L; const GeccoSetTransformer* st = c.st; hipStream_t s = c.s;
    const int C = st->C, G = st->G, Wd = st->width, act = st->act, B = c.B, N = c.N, pr = r.pr, himg = r.himg;
    const bool a16 = r.a16; float *x = c.x, *so = c.so;
    TRY(coeffs(w.stats_x, r.Tn, N, c.t, st->ctx_dim, &L.mlp_norm, w.a2, w.o2, B, C, G, s), "adagn_coeffs(mlp_norm)");
    if (r.mlpf_on && c.im) {
        MlpArgs ma{};
        ma.x = x; ma.pro_a = w.a2; ma.pro_o = w.o2; ma.w_stream = c.im + w.o_mf;
        ma.b0 = L.mlp.b0; ma.b2 = L.mlp.b2; ma.alpha = L.mlp.alpha; ma.act = act; ma.stats = so; ma.B = B; ma.rows = N;
        if ((act == 1 || act == 2) && !L.mlp.alpha) return fail(-6, "mlp: GaussianActivation needs alpha");
        TRY(mlp_fused_f16_launch(ma, C, Wd, s), "mlp (fused)");
        return 0;
    }
    int m0_done = a16 && r.astat ? astat_linear(x, w.a2, w.o2, c.img(w.o_w0), L.mlp.b0, Wd, w.big, nullptr, 0, nullptr, L.mlp.alpha, act, B, N, C, s) : 1;
    if (m0_done < 0) TRY(m0_done, "mlp.0 (A-stationary)");
    if (m0_done == 1 && r.mfw_on && c.im) {
        MlpWArgs ma{};
        ma.x = x; ma.out = x; ma.pro_a = w.a2; ma.pro_o = w.o2; ma.w_img = c.im + w.o_mf; ma.alpha = L.mlp.alpha;
        ma.act = act; ma.stats = so; ma.B = B; ma.rows = N; ma.share = r.mfw_share;
        if ((act == 1 || act == 2) && !L.mlp.alpha) return fail(-6, "mlp: GaussianActivation needs alpha");
        TRY(mlp_fused_w_launch(ma, C, Wd, s), "mlp (one launch, w2)");
        return 0;
    }
    if (m0_done == 1 && r.h8_on && himg && c.im) {
        GemmArgs hg{};
        hg.A = x; hg.pro_a = w.a2; hg.pro_o = w.o2; hg.bias = L.mlp.b0; hg.alpha = L.mlp.alpha; hg.act = act; hg.C = w.big;
        hg.B = B; hg.rows = N; hg.K = C; hg.Nout = Wd; hg.lda = C; hg.ldw = C; hg.ldc = Wd; hg.c_img = r.h8x ? 2 : 1; hg.w_img = c.im + w.o_w0; hg.h6 = r.h6_on ? 1 : 0;
        if ((act == 1 || act == 2) && !L.mlp.alpha) return fail(-6, "mlp.0: GaussianActivation needs alpha");
        TRY(gemm_h8_astat_launch(hg, s), "mlp.0 (h8)");
        m0_done = 0;
    }
    if (m0_done == 1) {
        if (a16) TRY(affine_cast_f16_launch(x, w.a2, w.o2, w.attn, B, N, C, s), "mlp_norm -> fp16");
        TRY(linear(Lin(a16 ? w.attn : x, L.mlp.w0, L.mlp.b0, w.big, B, N, C, Wd).pro(a16 ? nullptr : w.a2, a16 ? nullptr : w.o2).activation(act, L.mlp.alpha)
                       .weights(pr, w.wsplit, c.img(w.o_w0)).f16(a16, a16).image(0, (himg && r.h8x) ? 2 : himg), s), "mlp.0");
    }
    // mlp.2 as the h8 product where mlp.0 wrote the h8 activation image: the h8 kernel, or (feature_dim 512) the split-bf16 kernel
    if (himg && r.h8x && c.im) {
        TRY(h8_linear(w.big, c.im + w.o_w2, L.mlp.b2, x, x, so, B, N, Wd, C, s), "mlp.2+residual (h8)");
        return 0;
    }
    TRY(linear(Lin(w.big, L.mlp.w2, L.mlp.b2, x, B, N, Wd, C).plus(x).with_stats(so).weights(pr, w.wsplit, c.img(w.o_w2)).f16(a16, 0).image(himg, 0), s), "mlp.2+residual");
    return 0;
}

int st_forward(const GeccoSetTransformer* st, float* x, const float* t, const float* stats_x, int stats_T,
               const float* const* h_in, float* const* h_out, float* stats_out, int B, int N, void* ws,
               size_t ws_bytes, hipStream_t s, const Lift0In* pts = nullptr) {   // pts: x is lift(c_in p) of these (LinearLift)
    if (!st || !x || !t || !ws) return fail(-1, "set_transformer: null argument");
    if (st->I != 64) return fail(-3, "set_transformer: num_inducers must be 64 (got %d)", st->I);
    if (st->C % st->H || st->C % st->G || st->C % 4) return fail(-3, "set_transformer: bad feature_dim %d", st->C);
    if (st->act < 0 || st->act > 3) return fail(-3, "set_transformer: act must be 0 (identity), 1 / 2 (GaussianActivation normalized / raw) or 3 (ReLU)");
    PlanScope plan_scope(st);
    const STWorkspace w = carve_st(st, B, N, ws);
    if (ws_bytes < w.bytes) return fail(-7, "set_transformer: workspace too small (%zu < %zu)", ws_bytes, w.bytes);
    const StRoute r = st_route(st, B, N, h_in, pts != nullptr);
    if (r.rc) return r.rc;
    if (r.chain && !chain_stream_fits(st, w)) return fail(-3, "set_transformer: the inducer chain's weight stream does not fill its places in the workspace");
    const int C = st->C, H = st->H, G = st->G;
    const float* sx = stats_x; int sT = stats_T;
    if (!sx) {
        TRY(col_stats_launch(x, w.stats_x, B, N, C, s), "col_stats");
        sx = w.stats_x;
        sT = row_tiles_stats(N);
    }
    int rc = r.build ? build_weight_images(r, st, w, h_in, s) : 0;
    if (rc) return rc;
    if (r.chain_cl) TRY((int)hipMemsetAsync(w.merged, 0, (size_t)st->n_layers * B * 8 * sizeof(unsigned), s), "inducer chain counters");
    if (r.kvfold) TRY((int)hipMemsetAsync(w.attn, 0, unpool_outproj_h8_kv_bytes(B, C, H), s), "k | v image pads");
    for (int li = 0; li < st->n_layers; ++li) {
        const GeccoLayer& L = st->layers[li];
        const bool cached = h_in && h_in[li];
        StLayer c{st, r, w, L, li, r.imgs ? w.wimg + (size_t)li * w.wimg_layer : nullptr, x, t, B, N, s, cached ? h_in[li] : nullptr,
                  (h_out && h_out[li]) ? h_out[li] : w.h, (li + 1 < st->n_layers) ? w.stats_x : stats_out, cached};
        TRY(coeffs(sx, sT, N, t, st->ctx_dim, &L.broadcast_norm, w.a1, w.o1, B, C, G, s), "adagn_coeffs(broadcast_norm)");
        if (li == 0 && r.lift0) c.pts = pts;
        rc = c.pts ? project_from_points(c, !cached) : cached ? 0 : project_stage(c, true);
        if (!rc && !cached) rc = inducer_stage(c);
        if (!rc) rc = unpool_stage(c);
        if (!rc) rc = mlp_stage(c);
        if (rc) return rc;
        sx = w.stats_x;   // every form of the point MLP leaves the next layer's statistics there
        sT = r.Tn;
    }
    return 0;
}

struct LLWorkspace {
    float *feat, *coef, *stats;
    void* st_ws;
    size_t st_bytes, bytes;
};

LLWorkspace carve_ll(const GeccoLinearLift* m, int B, int N, void* base) {
    Carver c(base);
    LLWorkspace w;
    w.feat = c.f32((size_t)B * N * m->inner.C);
    w.coef = c.f32((size_t)B * 5);
    w.stats = c.f32((size_t)B * row_tiles_stats(N) * 2 * m->inner.C);
    c.off = (c.off + 255) & ~size_t(255);
    w.st_bytes = carve_st(&m->inner, B, N, nullptr).bytes;
    w.st_ws = base ? static_cast<char*>(base) + c.off : nullptr;
    w.bytes = c.off + w.st_bytes;
    return w;
}

struct RNWorkspace {
    float *feat, *raw, *coef, *stats_raw, *stats_x, *stats_out, *a_raw, *o_raw, *a_out, *o_out, *wsplit, *wfold, *bfold;
    void* st_ws;
    size_t st_bytes, bytes;
};

RNWorkspace carve_rn(const GeccoRayNetwork* m, int c_total, int B, int N, void* base) {
    Carver c(base);
    RNWorkspace w;
    const size_t C = m->backbone.C;
    w.feat = c.f32((size_t)B * N * C);
    w.raw = c.f32((size_t)B * N * c_total);
    w.coef = c.f32((size_t)B * 5);
    w.stats_raw = c.f32((size_t)B * gecco_lookup_row_tiles(N) * 2 * c_total);
    w.stats_x = c.f32((size_t)B * row_tiles_gemm(N) * 2 * C);
    w.stats_out = c.f32((size_t)B * row_tiles_gemm(N) * 2 * C);
    w.a_raw = c.f32((size_t)B * c_total);
    w.o_raw = c.f32((size_t)B * c_total);
    w.a_out = c.f32((size_t)B * C);
    w.o_out = c.f32((size_t)B * C);
    w.wsplit = c.f32(((C + 127) / 128 * 128) * (size_t)c_total);   // tiled image of img_feature_proj (precision 1 / 2)
    // "w2" mode ("imgproj16"): per-sample fp16 images of img_feature_proj with GN16's scale folded in, and the biases with its offsets
    const bool fold = m->backbone.precision == 4;
    w.wfold = fold ? c.f32((size_t)B * ((C + 127) / 128 * 128) * c_total / 2) : nullptr;
    w.bfold = fold ? c.f32((size_t)B * C) : nullptr;
    c.off = (c.off + 255) & ~size_t(255);
    w.st_bytes = carve_st(&m->backbone, B, N, nullptr).bytes;
    w.st_ws = base ? static_cast<char*>(base) + c.off : nullptr;
    w.bytes = c.off + w.st_bytes;
    return w;
}

}  // namespace

extern "C" {

int gecco_abi_version(void) { return GECCO_ABI_VERSION; }
const char* gecco_build_arch(void) { return "gfx950"; }
const char* gecco_last_error(void) { return g_err; }

int gecco_option_index(const char* name) {
    if (name)
        for (int i = 0; i < OPT_COUNT; ++i)
            if (!strcmp(name, g_option_names[i])) return i;
    return -1;
}

int gecco_set_option(const char* name, int value) {
    if (!name) return fail(-1, "set_option: null name");
    for (int i = 0; i < OPT_COUNT; ++i)
        if (!strcmp(name, g_option_names[i])) {
            g_options[i].store(value < 0 ? -1 : i == OPT_LIFT0 ? (value > 2 ? 2 : value) : (value != 0), std::memory_order_relaxed);   // < 0: back to the environment / default
            return 0;
        }
    return fail(-2, "set_option: unknown option '%s' (astat, chain, headmajor, mlpfused, unpoolfused, lo8, actimg, h8, kvq64, h8areg, chain2, unpoolh8, mlpw, chaincl, h6, kvfold, mlpwshare, kvqperm, imgproj16, lift0)", name);
}

size_t gecco_set_transformer_workspace_bytes(const GeccoSetTransformer* st, int B, int N) {
    return carve_st(st, B, N, nullptr).bytes;
}

int gecco_set_transformer_fwd_f32(const GeccoSetTransformer* st, float* x, const float* t, const float* stats_x,
                                  int stats_T, const float* const* h_in, float* const* h_out, float* stats_out,
                                  int B, int N, void* ws, size_t ws_bytes, void* stream) {
    return st_forward(st, x, t, stats_x, stats_T, h_in, h_out, stats_out, B, N, ws, ws_bytes, (hipStream_t)stream);
}

size_t gecco_linear_lift_workspace_bytes(const GeccoLinearLift* m, int B, int N) {
    return carve_ll(m, B, N, nullptr).bytes;
}

int gecco_linear_lift_fwd_f32(const GeccoLinearLift* m, const float* x, const float* sigma, float* denoised,
                              float* raw, const float* const* h_in, float* const* h_out, int B, int N, void* ws,
                              size_t ws_bytes, void* stream) {
    if (!m || !x || !sigma || !(denoised || raw)) return fail(-1, "linear_lift: null argument");
    LLWorkspace w = carve_ll(m, B, N, ws);
    if (ws_bytes < w.bytes) return fail(-7, "linear_lift: workspace too small (%zu < %zu)", ws_bytes, w.bytes);
    hipStream_t s = (hipStream_t)stream;
    const int C = m->inner.C;
    TRY(edm_coeffs_launch(sigma, m->sigma_data, w.coef, B, s), "edm_coeffs");
    TRY(lift_launch(x, w.coef, m->lift_w, m->lift_b, w.feat, w.stats, B, N, C, s), "lift");
    // AdaGN reads t as a packed (B, ctx_dim) array; under EDMPrecond ctx_dim == 1 and t = c_noise,
    // which edm_coeffs also writes packed at coef[4B .. 5B).
    if (m->inner.ctx_dim != 1) return fail(-3, "linear_lift: t_embed_dim must be 1 under EDMPrecond");
    const Lift0In pts{x, w.coef, m->lift_w, m->lift_b};
    int rc = st_forward(&m->inner, w.feat, w.coef + 4 * (size_t)B, w.stats, row_tiles_stats(N), h_in, h_out, nullptr, B,
                        N, w.st_ws, w.st_bytes, s, &pts);
    if (rc) return rc;
    TRY(lower_edm_launch(w.feat, x, w.coef, m->lower_w, m->lower_b, nullptr, nullptr, denoised, raw, B, N, C, 1e-5f, s),
        "lower_edm");
    return 0;
}

size_t gecco_linear_lift_g_workspace_bytes(const GeccoLinearLiftG* m, int B, int N) {
    return carve_ll(&m->base, B, N, nullptr).bytes;
}

int gecco_linear_lift_g_fwd_f32(const GeccoLinearLiftG* m, const float* x, const float* sigma, float* denoised,
                                float* raw, const float* const* h_in, float* const* h_out, int B, int N, void* ws,
                                size_t ws_bytes, void* stream) {
    if (!m || !x || !sigma || !(denoised || raw)) return fail(-1, "linear_lift_g: null argument");
    const int G = m->geometry_dim, C = m->base.inner.C;
    if (G < 1 || G > GECCO_MAX_GEOMETRY_DIM)
        return fail(-2, "linear_lift_g: geometry_dim %d outside 1 .. %d", G, GECCO_MAX_GEOMETRY_DIM);
    if (C % 4 || C > 512) return fail(-2, "linear_lift_g: feature_dim %d (needs C %% 4 == 0, C <= 512)", C);
    LLWorkspace w = carve_ll(&m->base, B, N, ws);
    if (ws_bytes < w.bytes) return fail(-7, "linear_lift_g: workspace too small (%zu < %zu)", ws_bytes, w.bytes);
    hipStream_t s = (hipStream_t)stream;
    if (m->base.inner.ctx_dim != 1) return fail(-3, "linear_lift_g: t_embed_dim must be 1 under EDMPrecond");
    TRY(edm_coeffs_launch(sigma, m->base.sigma_data, w.coef, B, s), "edm_coeffs");
    TRY(lift_g_launch(x, w.coef, m->base.lift_w, m->base.lift_b, w.feat, w.stats, B, N, C, G, s), "lift_g");
    int rc = st_forward(&m->base.inner, w.feat, w.coef + 4 * (size_t)B, w.stats, row_tiles_stats(N), h_in, h_out, nullptr, B,
                        N, w.st_ws, w.st_bytes, s);
    if (rc) return rc;
    TRY(lower_g_launch(w.feat, x, w.coef, m->base.lower_w, m->base.lower_b, denoised, raw, B, N, C, G, m->do_norm, 1e-5f, s),
        "lower_edm_g");
    return 0;
}

size_t gecco_ray_network_workspace_bytes(const GeccoRayNetwork* m, const GeccoPyramid* pyr, int B, int N) {
    int ct = 0;
    for (int l = 0; l < pyr->n_levels && l < 4; ++l) ct += pyr->C[l];
    return carve_rn(m, ct, B, N, nullptr).bytes;
}

int gecco_ray_network_fwd_f32(const GeccoRayNetwork* m, const float* x, const float* sigma, const float* K,
                              const GeccoPyramid* pyr, float* denoised, float* raw, const float* const* h_in,
                              float* const* h_out, int B, int N, void* ws, size_t ws_bytes, void* stream) {
    if (!m || !x || !sigma || !K || !(denoised || raw)) return fail(-1, "ray_network: null argument");
    if (m->backbone.ctx_dim != 1) return fail(-3, "ray_network: t_embed_dim must be 1 under EDMPrecond");
    LookupArgs a;
    int rc = make_lookup_args(&m->reparam, pyr, &a);
    if (rc) return rc;
    RNWorkspace w = carve_rn(m, a.c_total, B, N, ws);
    if (ws_bytes < w.bytes) return fail(-7, "ray_network: workspace too small (%zu < %zu)", ws_bytes, w.bytes);
    hipStream_t s = (hipStream_t)stream;
    const int C = m->backbone.C;
    TRY(edm_coeffs_launch(sigma, m->sigma_data, w.coef, B, s), "edm_coeffs");
    // xyz_embed(c_in * x)  (models/ray.py:99)
    TRY(lift_launch(x, w.coef, m->xyz_w, m->xyz_b, w.feat, nullptr, B, N, C, s), "xyz_embed");
    // projective lookup on c_in * x, fp32 always (models/ray.py:103-109) + GN(16) partials
    // "w2" with option "imgproj16" (opt-in: it moves C3's F_x from 2.3e-4 to 2.7e-4 of the mode's 5e-4 for 2 % of the evaluation): the lookup leaves halves, GN16's apply goes INTO the weights (per-sample images of W * a, biases + W o) and
    // img_feature_proj multiplies fp16(lookup) by them, one term each, on the fp16-operand streaming kernel: a third of split-bf16's matrix
    // work on half its operand bytes (the mode's one-term operands are the hidden layer, K and q already)
    PlanScope plan_scope(&m->backbone);
    const bool img16 = m->backbone.precision == 4 && option(OPT_IMGPROJ16) && a.c_total % 32 == 0 && N >= 128 && C % 4 == 0;
    a.out_f16 = img16;
    TRY(ray_lookup_launch(x, w.coef, K, a, w.raw, w.stats_raw, B, N, s), "ray_lookup");
    TRY(adagn_coeffs_launch(w.stats_raw, gecco_lookup_row_tiles(N), N, nullptr, 0, nullptr, nullptr, nullptr, nullptr,
                            w.a_raw, w.o_raw, B, a.c_total, 16, 1e-5f, s), "gn16(img)");
    // point_features = xyz_features + Linear(GN16(lookup))  (models/ray.py:112-113): GN apply in the GEMM
    // prologue, the add as its residual, the first AdaGN's statistics in its epilogue
    if (img16) {
        TRY(fold_f16_image_launch(m->img_w, m->img_b, w.a_raw, w.o_raw, w.wfold, w.bfold, B, C, a.c_total, a.c_total, s), "img_feature_proj fold");
        GemmArgs g{};
        g.A = w.raw; g.a_f16 = 1; g.bias = w.bfold; g.bias_bstride = C; g.residual = w.feat; g.C = w.feat; g.stats = w.stats_x;
        g.B = B; g.rows = N; g.K = a.c_total; g.Nout = C; g.lda = a.c_total; g.ldw = a.c_total; g.ldc = C; g.ldr = C;
        g.precision = 2; g.w_img = w.wfold; g.w_img_bstride = (size_t)((C + 127) / 128 * 128) * a.c_total / 2;
        if (!gemm_f16_dma_supported(g)) return fail(-9, "img_feature_proj: shape outside the fp16 streaming kernel");
        TRY(gemm_f32_launch(g, s), "img_feature_proj");
    } else {
        TRY(linear(Lin(w.raw, m->img_w, m->img_b, w.feat, B, N, a.c_total, C).pro(w.a_raw, w.o_raw).plus(w.feat).with_stats(w.stats_x)
                       .weights(m->backbone.precision >= 3 ? 1 : m->backbone.precision, w.wsplit), s), "img_feature_proj");   // mixed mode: split-bf16
    }
    rc = st_forward(&m->backbone, w.feat, w.coef + 4 * (size_t)B, w.stats_x, row_tiles_gemm(N), h_in, h_out,
                    w.stats_out, B, N, w.st_ws, w.st_bytes, s);
    if (rc) return rc;
    // output_proj = Linear(GN16(.)) (models/ray.py:56-59,120) + EDM combine (diffusion.py:57)
    TRY(adagn_coeffs_launch(w.stats_out, row_tiles_gemm(N), N, nullptr, 0, nullptr, nullptr, nullptr, nullptr, w.a_out,
                            w.o_out, B, C, 16, 1e-5f, s), "gn16(out)");
    TRY(lower_edm_launch(w.feat, x, w.coef, m->out_w, m->out_b, w.a_out, w.o_out, denoised, raw, B, N, C, 1e-5f, s),
        "output_proj+edm");
    return 0;
}

}  // extern "C"
