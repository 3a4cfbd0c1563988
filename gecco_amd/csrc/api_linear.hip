// C ABI of libgecco_hip.so, part 2 of 4: the unit linears, the weight-image builders and their shape queries, the TN GEMMs
// and the fused-kernel unit calls.
#include "api_linear.h"

using namespace gecco_api;

extern "C" {

int gecco_linear_row_tiles(int rows) { return row_tiles_gemm(rows); }
int gecco_stats_row_tiles(int rows) { return row_tiles_stats(rows); }

int gecco_linear_f32(const float* A, const float* W, const float* bias, const float* pro_a, const float* pro_o,
                     const float* alpha, const float* residual, float* C, float* stats, int B, int rows, int K,
                     int Nout, int act, void* stream) {
    if (!A || !W || !C) return fail(-1, "linear: null argument");
    if (int rc = check_pro_pair("linear", pro_a, pro_o)) return rc;
    TRY(linear(Lin(A, W, bias, C, B, rows, K, Nout).pro(pro_a, pro_o).activation(act, alpha).plus(residual).with_stats(stats), (hipStream_t)stream), "linear");
    return 0;
}

int gecco_linear_ex_f32(const float* A, const float* W, const float* bias, const float* pro_a, const float* pro_o,
                        const float* alpha, const float* residual, float* C, float* stats, int B, int rows, int K,
                        int Nout, int act, int precision, void* wsplit, void* stream) {
    if (!A || !C) return fail(-1, "linear: null argument");
    if (int rc = check_pro_pair("linear", pro_a, pro_o)) return rc;
    if (int rc = check_precision("linear", precision, wsplit)) return rc;
    if (!W) {   // wsplit already holds the image of W (gecco_split_bf16_images_f32 / gecco_split_f16_images_f32): kernel launch only
        if (precision == 0 || !(precision == 1 ? gecco_linear_image_ok(rows, K, Nout, pro_a != nullptr)
                                               : gecco_linear_image_ok_f16(rows, K, Nout, pro_a != nullptr)))
            return fail(-2, "linear: W == NULL (image ready) needs precision 1 / 2 and a shape gecco_linear_image_ok[_f16] accepts");
    }
    TRY(linear(Lin(A, W, bias, C, B, rows, K, Nout).pro(pro_a, pro_o).activation(act, alpha).plus(residual).with_stats(stats).weights_or_image(precision, wsplit),
               (hipStream_t)stream), "linear");
    return 0;
}

int gecco_linear_pair_f32(const float* A, const float* W1, const float* bias1, int Nout1, float* C1, const float* W2,
                          const float* bias2, int Nout2, float* C2, const float* pro_a, const float* pro_o, int B,
                          int rows, int K, int precision, void* wsplit, void* stream) {
    if (!A || !C1 || !C2 || (!W1) != (!W2)) return fail(-1, "linear_pair: null argument");
    if (int rc = check_pro_pair("linear_pair", pro_a, pro_o)) return rc;
    if (int rc = check_precision("linear_pair", precision, wsplit)) return rc;
    hipStream_t s = (hipStream_t)stream;
    float* ws = static_cast<float*>(wsplit);
    if (!W1) {   // wsplit holds the images of W1 and, from the next 128-column tile boundary, W2
        if (precision == 0) return fail(-2, "linear_pair: W == NULL (images ready) needs precision 1 / 2");
        int rc = linear_pair(Lin(A, nullptr, bias1, C1, B, rows, K, Nout1).pro(pro_a, pro_o).weights(precision, nullptr, ws), nullptr, bias2, Nout2, C2, s);
        if (rc == 1) return fail(-2, "linear_pair: images ready, but the shape is outside the fused kernel's reach");
        TRY(rc, "linear_pair");
        return 0;
    }
    Lin first = Lin(A, W1, bias1, C1, B, rows, K, Nout1).pro(pro_a, pro_o).weights(precision, ws);
    int rc = linear_pair(first, W2, bias2, Nout2, C2, s);
    if (rc < 0) TRY(rc, "linear_pair");
    if (rc == 1) {   // shape outside the fused kernel's reach: the two linears, same results
        TRY(linear(first, s), "linear_pair[0]");
        TRY(linear(Lin(A, W2, bias2, C2, B, rows, K, Nout2).pro(pro_a, pro_o).weights(precision, ws), s), "linear_pair[1]");
    }
    return 0;
}

static int dma_ok(int rows, int K, int Nout, int with_prologue, int precision) {   // a plain linear of this shape is within the LDS-DMA kernels' reach
    float dummy = 0.f;
    GemmArgs g = gemm_args(&dummy, &dummy, nullptr, &dummy, 1, rows, K, Nout);
    g.pro_a = g.pro_o = with_prologue ? &dummy : nullptr;
    return (precision == 2 ? gemm_f16_dma_supported(g) : gemm_f32_dma_supported(g, precision)) ? 1 : 0;
}
int gecco_linear_image_ok(int rows, int K, int Nout, int with_prologue) { return dma_ok(rows, K, Nout, with_prologue, 1); }
int gecco_linear_image_ok_f16(int rows, int K, int Nout, int with_prologue) { return dma_ok(rows, K, Nout, with_prologue, 2); }
size_t gecco_split_f16_image_bytes(int Nout, int K) { return split_f16_image_bytes(Nout, K); }
int gecco_split_f16_images_f32(const GeccoSplitJob* jobs, int n, void* stream) {
    return image_batch("split_f16_images", "K % 32 == 0 (and ldw % 4 == 0 unless transposed)", jobs, n,
                       [](const GeccoSplitJob& j) -> std::optional<ImageFormat> {
                           if ((j.K % 32) || (!j.transposed && (j.ldw & 3))) return std::nullopt;
                           return j.transposed ? F16_TRANSPOSED : F16_PLAIN;
                       },
                       split_f16_tiled_multi_launch, (hipStream_t)stream);
}
size_t gecco_split_bf16_image_bytes(int Nout, int K) { return split_bf16_image_bytes(Nout, K); }
int gecco_split_bf16_images_f32(const GeccoSplitJob* jobs, int n, void* stream) {
    return image_batch("split_bf16_images", "K % 16 == 0 (and ldw % 4 == 0 unless transposed)", jobs, n,
                       [](const GeccoSplitJob& j) -> std::optional<ImageFormat> {
                           if ((j.K % 16) || (!j.transposed && (j.ldw & 3))) return std::nullopt;
                           return j.transposed ? BF16_TRANSPOSED : BF16_PLAIN;
                       },
                       split_bf16_tiled_multi_launch, (hipStream_t)stream);
}

int gecco_linear_actbwd_ok(int rows, int K, int Nout, int precision) { return precision >= 0 && precision <= 2 ? dma_ok(rows, K, Nout, 0, precision) : 0; }
size_t gecco_linear_actbwd_tiles(int B, int rows, int Nout) { return (size_t)B * ((rows + 63) / 64) * ((Nout + 127) / 128); }   // one slot per 64 rows
int gecco_linear_actbwd_f32(const float* A, const float* W, const float* u, const float* alpha, int kind, const float* residual,
                            float* C, float* agrad, int B, int rows, int K, int Nout, int precision, void* wsplit, void* stream) {
    if (!A || !u || !C) return fail(-1, "linear_actbwd: null argument");
    if (kind < 1 || kind > 4) return fail(-2, "linear_actbwd: kind must be 1 / 2 (GaussianActivation), 3 (ReLU) or 4 (GELU)");
    if ((kind == 1 || kind == 2) && (!alpha || !agrad)) return fail(-1, "linear_actbwd: GaussianActivation needs alpha and the agrad partials");
    if (int rc = check_dma_linear("linear_actbwd", gecco_linear_actbwd_ok(rows, K, Nout, precision), W, precision, wsplit)) return rc;
    Lin l = Lin(A, W, nullptr, C, B, rows, K, Nout).activation(0, alpha).plus(residual).weights_or_image(precision, wsplit);
    l.g.mul_u = u; l.g.mul_kind = kind; l.g.agrad = (kind == 1 || kind == 2) ? agrad : nullptr;
    TRY(linear(l, (hipStream_t)stream), "linear_actbwd");
    return 0;
}

int gecco_linear_dotstats_f32(const float* A, const float* W, const float* dot_x, float* C, float* stats, int B, int rows, int K, int Nout,
                              int precision, void* wsplit, void* stream) {
    if (!A || !dot_x || !C || !stats) return fail(-1, "linear_dotstats: null argument");
    if (int rc = check_dma_linear("linear_dotstats", gecco_linear_actbwd_ok(rows, K, Nout, precision), W, precision, wsplit)) return rc;
    Lin l = Lin(A, W, nullptr, C, B, rows, K, Nout).with_stats(stats).weights_or_image(precision, wsplit);
    l.g.dot_x = dot_x;
    TRY(linear(l, (hipStream_t)stream), "linear_dotstats");
    return 0;
}

int gecco_linear_dotstats_a16_f32(const void* A16, const float* W, const float* dot_x, const float* residual, float* C, float* stats, int B, int rows,
                                  int K, int Nout, void* wsplit, void* stream) {
    if (!A16 || !dot_x || !C || !stats || !wsplit) return fail(-1, "linear_dotstats_a16: null argument");
    if (!gecco_linear_actbwd_ok(rows, K, Nout, 2) || (K & 7) || rows < 128) return fail(-2, "linear_dotstats_a16: shape outside the fp16 LDS-DMA kernel's reach");
    Lin l = Lin(static_cast<const float*>(A16), W, nullptr, C, B, rows, K, Nout).plus(residual).with_stats(stats).weights_or_image(2, wsplit).f16(1, 0);
    l.g.dot_x = dot_x;
    int rc = linear(l, (hipStream_t)stream);
    if (rc == -9) return fail(-2, "linear_dotstats_a16: shape outside the fp16 LDS-DMA kernel's reach");
    TRY(rc, "linear_dotstats_a16");
    return 0;
}

int gecco_linear_act_keep_f32(const float* A, const float* W, const float* bias, const float* alpha, int act, float* pre_out,
                              float* C, int B, int rows, int K, int Nout, int precision, void* wsplit, void* stream) {
    return gecco_linear_act_keep_pro_f32(A, W, bias, nullptr, nullptr, alpha, act, pre_out, C, B, rows, K, Nout, precision, wsplit, stream);
}

int gecco_linear_act_keep_pro_f32(const float* A, const float* W, const float* bias, const float* pro_a, const float* pro_o,
                                  const float* alpha, int act, float* pre_out, float* C, int B, int rows, int K, int Nout,
                                  int precision, void* wsplit, void* stream) {
    if (!A || !pre_out || !C) return fail(-1, "linear_act_keep: null argument");
    if (int rc = check_pro_pair("linear_act_keep", pro_a, pro_o, true)) return rc;
    if (pro_a && K > 1024) return fail(-2, "linear_act_keep: the AdaGN prologue needs K <= 1024");
    if (act < 1 || act > 4) return fail(-2, "linear_act_keep: act must be 1 / 2 (GaussianActivation), 3 (ReLU) or 4 (GELU)");
    if (int rc = check_alpha("linear_act_keep", act, alpha, -1)) return rc;
    if (int rc = check_dma_linear("linear_act_keep", gecco_linear_actbwd_ok(rows, K, Nout, precision), W, precision, wsplit)) return rc;
    Lin l = Lin(A, W, bias, C, B, rows, K, Nout).pro(pro_a, pro_o).activation(act, alpha).weights_or_image(precision, wsplit);
    l.g.pre_out = pre_out;
    TRY(linear(l, (hipStream_t)stream), "linear_act_keep");
    return 0;
}

/* ---- the training forward in h8 arithmetic with fp32 tensors (gemm_h8_astat.hip, OUT forms of gemm_h8_astat_kernel) ---- */
size_t gecco_h8_image_bytes(int Nout, int K) { return (Nout % 64 || K % 64) ? 0 : h8_image_bytes(Nout, K); }
int gecco_linear_h8_train_ok(int rows, int K, int Nout) {
    return rows >= 128 && rows % 128 == 0 && (K == 128 || K == 256 || K == 384) && Nout % 64 == 0 && Nout >= 128 && Nout <= 4096;
}
int gecco_h8_images_f32(const GeccoSplitJob* jobs, int n, void* stream) {
    return image_batch("h8_images", "Nout % 64 == 0, K % 64 == 0, ldw % 4 == 0, not transposed", jobs, n,
                       [](const GeccoSplitJob& j) -> std::optional<ImageFormat> {
                           if ((j.Nout % 64) || (j.K % 64) || (j.ldw & 3) || j.transposed) return std::nullopt;
                           return H8_MLP0;
                       },
                       h8_image_multi_launch, (hipStream_t)stream);
}

int gecco_linear_h8_train_f32(const float* x, const float* pro_a, const float* pro_o, const float* W1, const float* bias1, int Nout1, float* C1,
                              const float* W2, const float* bias2, int Nout2, float* C2, const float* alpha, int act, float* pre_out, int B,
                              int rows, int K, void* wsplit, void* stream) {
    if (!x || !C1 || !wsplit || (Nout2 > 0 && !C2)) return fail(-1, "linear_h8_train: null argument");
    if (int rc = check_pro_pair("linear_h8_train", pro_a, pro_o, true)) return rc;
    if (Nout2 > 0 && ((W1 == nullptr) != (W2 == nullptr))) return fail(-1, "linear_h8_train: W1 / W2 both given or both ready");
    if ((act != 0) != (pre_out != nullptr)) return fail(-2, "linear_h8_train: an activation comes with pre_out (the keep form), and only with it");
    if (int rc = check_alpha("linear_h8_train", act, alpha, -1)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int n2 = Nout2 > 0 ? Nout2 : 0;   // (<= 0: no second segment)
    GemmArgs g = gemm_args_pair(x, bias1, C1, Nout1, bias2, n2 ? C2 : nullptr, n2, B, rows, K);
    g.pro_a = pro_a; g.pro_o = pro_o; g.alpha = alpha; g.act = act; g.pre_out = pre_out; g.precision = 1; g.w_img = wsplit;
    if (!gemm_h8_train_supported(g))
        return fail(-2, "linear_h8_train: needs rows %% 128 == 0, K in {128, 256, 384}, Nout (each segment) %% 64 == 0, Nout >= 128, act 0 .. 3");
    if (W1) TRY(build_images(h8_image_multi_launch, wsplit, K, s, {W1, Nout1, K, H8_MLP0}, {n2 ? W2 : nullptr, n2, K, H8_MLP0}, h8_image_bytes(Nout1, K)), "linear_h8_train(image)");
    TRY(gemm_h8_train_launch(g, s), "linear_h8_train");
    return 0;
}

/* ---- A-stationary fp16 linears with fp32 tensors: the training path's 384-wide products under autocast(float16) (gemm_h8_astat.hip,
 * OUT forms of gemm_kvq_astat_kernel) ---- */
size_t gecco_astat16_image_bytes(int Nout, int K) { return (Nout % 64 || K % 64) ? 0 : kvq_image_bytes(Nout, K, 0); }
int gecco_linear_astat16_ok(int rows, int K, int Nout) {
    return rows >= 128 && rows % 128 == 0 && (K == 128 || K == 256 || K == 384 || K == 512) && Nout % 64 == 0 && Nout >= 128 && Nout <= 4096;
}
int gecco_astat16_images_f32(const GeccoSplitJob* jobs, int n, void* stream) {
    return image_batch("astat16_images", "Nout % 64 == 0, K % 64 == 0 (and ldw % 4 == 0 unless transposed)", jobs, n,
                       [](const GeccoSplitJob& j) -> std::optional<ImageFormat> {   // the one-term kvq stream
                           if ((j.Nout % 64) || (j.K % 64) || (!j.transposed && (j.ldw & 3))) return std::nullopt;
                           return kvq_format(0, 0, j.transposed ? KVQ_TRANSPOSED : KVQ_PLAIN);
                       },
                       h8_image_multi_launch, (hipStream_t)stream);
}

int gecco_linear_astat16_f32(const float* x, const float* pro_a, const float* pro_o, const float* W1, const float* bias1, int Nout1, float* C1,
                             const float* W2, const float* bias2, int Nout2, float* C2, const float* residual, int transposed, int B, int rows,
                             int K, void* wsplit, void* stream) {
    if (!x || !C1 || !wsplit || (Nout2 > 0 && !C2)) return fail(-1, "linear_astat16: null argument");
#ifndef GECCO_EXPERIMENTAL
    // C1 = x W + another gradient: measured, no gain inside the step (19.31 vs 19.27 ms) — not part of the shipped surface
    if (residual) return fail(-2, "linear_astat16: the residual form is an experiment (build with -DGECCO_EXPERIMENTAL); pass NULL");
#endif
    if (residual && (Nout2 > 0 || pro_a || bias1)) return fail(-2, "linear_astat16: the residual form takes one weight, no prologue, no bias");
    if (int rc = check_pro_pair("linear_astat16", pro_a, pro_o, true)) return rc;
    if (Nout2 > 0 && ((W1 == nullptr) != (W2 == nullptr))) return fail(-1, "linear_astat16: W1 / W2 both given or both ready");
    hipStream_t s = (hipStream_t)stream;
    const int n2 = Nout2 > 0 ? Nout2 : 0;   // (<= 0: no second segment)
    GemmArgs g = gemm_args_pair(x, bias1, C1, Nout1, bias2, n2 ? C2 : nullptr, n2, B, rows, K);
    g.pro_a = pro_a; g.pro_o = pro_o; g.precision = 2; g.w_img = wsplit;
    if (residual) { g.mul_u = residual; g.mul_kind = 0; }   // C1 = x W^T + residual (the epilogue form that reads a second tensor)
    if (!gemm_astat_train_supported(g))
        return fail(-2, "linear_astat16: needs rows %% 128 == 0, K in {128, 256, 384, 512}, Nout (each segment) %% 64 == 0, Nout >= 128");
    if (W1) {
        if (transposed && Nout2 > 0) return fail(-2, "linear_astat16: the transposed form takes one weight");
        TRY(build_images(h8_image_multi_launch, wsplit, K, s, {W1, Nout1, transposed ? Nout1 : K, kvq_format(0, 0, transposed ? KVQ_TRANSPOSED : KVQ_PLAIN)}, {n2 ? W2 : nullptr, n2, K, kvq_format(0, 0)},
                         kvq_image_bytes(Nout1, K, 0)), "linear_astat16(image)");
    }
    TRY(gemm_astat_train_launch(g, s), "linear_astat16");
    return 0;
}

int gecco_linear_astat16_keep(const float* x, const float* pro_a, const float* pro_o, const float* W, const float* bias, const float* alpha,
                              int act, float* pre_out, void* C16out, int B, int rows, int K, int Nout, void* wsplit, void* stream) {
    return gecco_linear_astat16_keep_y16(x, pro_a, pro_o, W, bias, alpha, act, pre_out, C16out, nullptr, B, rows, K, Nout, wsplit, stream);
}

int gecco_linear_astat16_keep_y16(const float* x, const float* pro_a, const float* pro_o, const float* W, const float* bias, const float* alpha,
                                  int act, float* pre_out, void* C16out, void* y16, int B, int rows, int K, int Nout, void* wsplit,
                                  void* stream) {
    if (!x || !pre_out || !C16out || !wsplit) return fail(-1, "linear_astat16_keep: null argument");
    if (int rc = check_pro_pair("linear_astat16_keep", pro_a, pro_o, true)) return rc;
    if (int rc = check_alpha("linear_astat16_keep", act, alpha, -1)) return rc;
    hipStream_t s = (hipStream_t)stream;
    GemmArgs g = gemm_args(x, nullptr, bias, static_cast<float*>(C16out), B, rows, K, Nout);
    g.pro_a = pro_a; g.pro_o = pro_o; g.alpha = alpha; g.act = act; g.pre_out = pre_out; g.precision = 2; g.w_img = wsplit; g.y16_out = y16;
    if (!gemm_astat_train_supported(g))
        return fail(-2, "linear_astat16_keep: needs rows %% 128 == 0, K in {128, 256, 384, 512}, Nout %% 64 == 0, act 1 / 2 (GaussianActivation) or 3 (ReLU)");
    if (W) TRY(build_images(h8_image_multi_launch, wsplit, K, s, {W, Nout, K, kvq_format(0, 0)}), "linear_astat16_keep(image)");
    TRY(gemm_astat_train_launch(g, s), "linear_astat16_keep");
    return 0;
}

int gecco_linear_astat16_actbwd(const float* dy, const float* W, const float* u, const float* alpha, int kind, float* C, float* agrad, int B,
                                int rows, int K, int Nout, void* wsplit, void* stream) {
    if (!dy || !u || !C || !wsplit) return fail(-1, "linear_astat16_actbwd: null argument");
    if ((kind == 1 || kind == 2) && (!alpha || !agrad)) return fail(-1, "linear_astat16_actbwd: GaussianActivation needs alpha and the agrad partials");
    hipStream_t s = (hipStream_t)stream;
    GemmArgs g = gemm_args(dy, nullptr, nullptr, C, B, rows, K, Nout);
    g.alpha = alpha; g.mul_u = u; g.mul_kind = kind; g.agrad = (kind == 1 || kind == 2) ? agrad : nullptr; g.precision = 2; g.w_img = wsplit;
    if (!gemm_astat_train_supported(g))
        return fail(-2, "linear_astat16_actbwd: needs rows %% 128 == 0, K in {128, 256, 384, 512}, Nout %% 64 == 0, kind 1 / 2 (GaussianActivation) or 3 (ReLU)");
    // the linear's own weight (K, Nout): the stream of its transpose, straight from it
    if (W) TRY(build_images(h8_image_multi_launch, wsplit, K, s, {W, Nout, Nout, kvq_format(0, 0, KVQ_TRANSPOSED)}), "linear_astat16_actbwd(image)");
    TRY(gemm_astat_train_launch(g, s), "linear_astat16_actbwd");
    return 0;
}

int gecco_linear_astat16_actbwd_h16(const float* dy, const float* W, const float* u, const float* alpha, int kind, void* C16out, float* agrad, int B,
                                    int rows, int K, int Nout, void* wsplit, void* stream) {
    if (!dy || !u || !C16out || !wsplit) return fail(-1, "linear_astat16_actbwd_h16: null argument");
    if (kind < 1 || kind > 3) return fail(-2, "linear_astat16_actbwd_h16: kind 1 / 2 (GaussianActivation) or 3 (ReLU)");
    if ((kind == 1 || kind == 2) && (!alpha || !agrad)) return fail(-1, "linear_astat16_actbwd_h16: GaussianActivation needs alpha and the agrad partials");
    hipStream_t s = (hipStream_t)stream;
    GemmArgs g = gemm_args(dy, nullptr, nullptr, static_cast<float*>(C16out), B, rows, K, Nout);
    g.alpha = alpha; g.mul_u = u; g.mul_kind = kind; g.agrad = (kind == 1 || kind == 2) ? agrad : nullptr; g.precision = 2; g.w_img = wsplit; g.c_f16 = 1;
    if (!gemm_astat_train_supported(g))
        return fail(-2, "linear_astat16_actbwd_h16: needs rows %% 128 == 0, K in {128, 256, 384, 512}, Nout %% 64 == 0");
    if (W) TRY(build_images(h8_image_multi_launch, wsplit, K, s, {W, Nout, Nout, kvq_format(0, 0, KVQ_TRANSPOSED)}), "linear_astat16_actbwd_h16(image)");
    TRY(gemm_astat_train_launch(g, s), "linear_astat16_actbwd_h16");
    return 0;
}

int gecco_linear_act_keep_h16(const float* A, const float* W, const float* bias, const float* pro_a, const float* pro_o,
                              const float* alpha, int act, float* pre_out, void* C16out, int B, int rows, int K, int Nout, void* wsplit,
                              void* stream) {
    if (!A || !pre_out || !C16out || !wsplit) return fail(-1, "linear_act_keep_h16: null argument");
    if (int rc = check_pro_pair("linear_act_keep_h16", pro_a, pro_o, true)) return rc;
    if (act < 1 || act > 4) return fail(-2, "linear_act_keep_h16: act must be 1 / 2 (GaussianActivation), 3 (ReLU) or 4 (GELU)");
    if (int rc = check_alpha("linear_act_keep_h16", act, alpha, -1)) return rc;
    Lin l = Lin(A, W, bias, static_cast<float*>(C16out), B, rows, K, Nout).pro(pro_a, pro_o).activation(act, alpha).weights_or_image(2, wsplit).f16(0, 1);
    l.g.pre_out = pre_out;
    int rc = linear(l, (hipStream_t)stream);
    if (rc == -9) return fail(-2, "linear_act_keep_h16: needs rows >= 128, K %% 32 == 0, K <= 1024 with a prologue, Nout %% 4 == 0");
    TRY(rc, "linear_act_keep_h16");
    return 0;
}

int gecco_linear_f16io(const void* A, const float* W, const float* bias, const float* alpha, const float* residual,
                       void* C, float* stats, int B, int rows, int K, int Nout, int act, int a_f16, int c_f16,
                       void* wsplit, void* stream) {
    if (!A || !C || !wsplit) return fail(-1, "linear_f16io: null argument");
    if (!a_f16 && !c_f16) return fail(-2, "linear_f16io: at least one of A / C must be an fp16 tensor (else gecco_linear_ex_f32)");
    // W == NULL: wsplit already holds the fp16 image of W (gecco_split_f16_images_f32): kernel launch only
    int rc = linear(Lin(static_cast<const float*>(A), W, bias, static_cast<float*>(C), B, rows, K, Nout).activation(act, alpha).plus(residual).with_stats(stats)
                        .weights_or_image(2, wsplit).f16(a_f16, c_f16), (hipStream_t)stream);
    if (rc == -9) return fail(-2, "linear_f16io: needs rows >= 128, K %% 32 == 0, lda %% 8 == 0; fp16 C excludes residual / stats");
    TRY(rc, "linear_f16io");
    return 0;
}

int gecco_linear_pair_f16io(const void* A, const float* W1, const float* bias1, int Nout1, void* C1, const float* W2,
                            const float* bias2, int Nout2, void* C2, int B, int rows, int K, void* wsplit,
                            void* stream) {
    if (!A || !W1 || !W2 || !C1 || !C2 || !wsplit) return fail(-1, "linear_pair_f16io: null argument");
    int rc = linear_pair(Lin(static_cast<const float*>(A), W1, bias1, static_cast<float*>(C1), B, rows, K, Nout1).weights(2, static_cast<float*>(wsplit)).f16(1, 1),
                         W2, bias2, Nout2, static_cast<float*>(C2), (hipStream_t)stream);
    if (rc == 1 || rc == -9) return fail(-2, "linear_pair_f16io: needs rows >= 128, K %% 32 == 0, Nout1 %% 128 == 0");
    TRY(rc, "linear_pair_f16io");
    return 0;
}

int gecco_linear_astat_f16(const float* x, const float* pro_a, const float* pro_o, const float* W1, const float* bias1,
                           int Nout1, void* C1, const float* W2, const float* bias2, int Nout2, void* C2,
                           const float* alpha, int act, int B, int rows, int K, int head_dim, void* wsplit, void* stream) {
    if (!x || !C1 || !wsplit) return fail(-1, "linear_astat: null argument");
    const bool image_ready = W1 == nullptr;   // wsplit holds the images a previous call made from the same weights
    if (int rc = check_pro_pair("linear_astat", pro_a, pro_o)) return rc;
    if (!image_ready && (W2 == nullptr) != (C2 == nullptr)) return fail(-1, "linear_astat: W2 and C2 go together");
    hipStream_t s = (hipStream_t)stream;
    if (!image_ready)
        TRY(build_images(launch_each<split_f16_tiled_launch>, wsplit, K, s, {W1, Nout1, K, F16_PLAIN}, {W2, Nout2, K, F16_PLAIN}, split_f16_image_bytes(Nout1, K)), "linear_astat(split)");
    GemmArgs g = gemm_args_pair(x, bias1, static_cast<float*>(C1), Nout1, bias2, static_cast<float*>(C2), C2 ? Nout2 : 0, B, rows, K);
    g.pro_a = pro_a; g.pro_o = pro_o; g.alpha = alpha; g.act = act; g.precision = 2; g.w_img = wsplit; g.c_f16 = 1; g.hm_hd = head_dim;
    if (int rc = check_alpha("linear_astat", act, alpha, -6)) return rc;
    if (head_dim < 0) return fail(-2, "linear_astat: head_dim < 0");
    if (!gemm_f16_astat_supported(g))
        return fail(-2, "linear_astat: needs rows %% 128 == 0, Nout %% 128 == 0, K in {128, 256, 384, 512}; head-major: "
                        "even head_dim >= 8 dividing both segment widths");
    TRY(gemm_f16_astat_launch(g, s), "linear_astat");
    return 0;
}

int gecco_linear_kvq_f16(const float* x, const float* pro_a, const float* pro_o, const float* W1, const float* bias1, int Nout1,
                         void* C1, const float* W2, const float* bias2, int Nout2, void* C2, int B, int rows, int K, int head_dim,
                         int lo_begin, int lo_end, void* wsplit, void* stream) {
    return gecco_linear_kvq_y16_f16(x, pro_a, pro_o, W1, bias1, Nout1, C1, W2, bias2, Nout2, C2, nullptr, B, rows, K, head_dim, lo_begin, lo_end,
                                    wsplit, stream);
}

int gecco_linear_kvq_y16_f16(const float* x, const float* pro_a, const float* pro_o, const float* W1, const float* bias1, int Nout1,
                             void* C1, const float* W2, const float* bias2, int Nout2, void* C2, void* y16, int B, int rows, int K,
                             int head_dim, int lo_begin, int lo_end, void* wsplit, void* stream) {
    if (!x || !C1 || !wsplit) return fail(-1, "linear_kvq: null argument");
    if (int rc = check_pro_pair("linear_kvq", pro_a, pro_o)) return rc;
    if ((Nout2 > 0) != (C2 != nullptr)) return fail(-1, "linear_kvq: Nout2 and C2 go together");
    if (head_dim < 0 || lo_begin < 0 || lo_end < lo_begin || lo_end > Nout1 || (lo_begin & 63) || (lo_end & 63) || (Nout1 & 63) || (Nout2 & 63) ||
        K <= 0 || (K & 127))
        return fail(-2, "linear_kvq: head_dim >= 0; lo range inside the first segment, multiples of 64; Nout %% 64 == 0; K %% 128 == 0");
    hipStream_t s = (hipStream_t)stream;
    GemmArgs g = gemm_args_pair(x, bias1, static_cast<float*>(C1), Nout1, bias2, static_cast<float*>(C2), Nout2, B, rows, K);
    g.pro_a = pro_a; g.pro_o = pro_o; g.precision = 2; g.w_img = wsplit; g.c_f16 = 1; g.hm_hd = head_dim; g.lo_begin = lo_begin / 64; g.lo_tiles = lo_end / 64;
    g.y16_out = y16;
    // (the two-term range must be whole 384-column segments: it is a range of TILES in the stream)
    g.kvq_perm = option(OPT_KVQPERM) && kvq_perm48_ok(head_dim, K, Nout1, Nout2) && lo_begin % 384 == 0 && lo_end % 384 == 0;
    const KvqOrder order = g.kvq_perm ? KVQ_HEAD48 : KVQ_PLAIN;
    if (!gemm_kvq_astat_supported(g))
        return fail(-2, "linear_kvq: needs rows %% 128 == 0, Nout1 + Nout2 >= 128, K in {128, 256, 384, 512}; head-major: head_dim %% 8 == 0 "
                        "dividing both segment widths");
    if (W1) {   // NULL: wsplit still holds the stream a previous call made from the same weights
        if (Nout2 > 0 && !W2) return fail(-1, "linear_kvq: W2 missing");
        TRY(build_images(h8_image_multi_launch, wsplit, K, s, {W1, Nout1, K, kvq_format(lo_begin / 64, lo_end / 64, order)},
                         {Nout2 > 0 ? W2 : nullptr, Nout2, K, kvq_format(0, 0, order)}, kvq_image_bytes(Nout1, K, lo_end - lo_begin)), "linear_kvq(image)");
    }
    TRY(gemm_kvq_astat_launch(g, s), "linear_kvq");
    return 0;
}

int gecco_linear_h8_img_f32(const float* x, const float* pro_a, const float* pro_o, const float* W, const float* bias,
                            const float* alpha, int act, void* c_img, int image_kind, int B, int rows, int K, int Nout, void* wsplit,
                            void* stream) {
    if (!x || !c_img || !wsplit) return fail(-1, "linear_h8_img: null argument");
    if (image_kind != 1 && image_kind != 2) return fail(-2, "linear_h8_img: image_kind must be 1 (tiled split image) or 2 (h8 activation image)");
    if (int rc = check_pro_pair("linear_h8_img", pro_a, pro_o)) return rc;
    if (int rc = check_alpha("linear_h8_img", act, alpha, -6)) return rc;
    hipStream_t s = (hipStream_t)stream;
    GemmArgs g = gemm_args(x, nullptr, bias, static_cast<float*>(c_img), B, rows, K, Nout);
    g.ldr = 0;   // (no residual: this form has never named its stride)
    g.pro_a = pro_a; g.pro_o = pro_o; g.alpha = alpha; g.act = act; g.c_img = image_kind; g.w_img = wsplit;
    g.h6 = image_kind == 2 && option(OPT_H6) ? 1 : 0;   // option "h6": the cross terms in fp6 with block scales (the network's mlp.0)
    if (!gemm_h8_astat_supported(g))
        return fail(-2, "linear_h8_img: needs rows %% 128 == 0, Nout %% 64 == 0, Nout >= 128, K in {128, 256, 384}, act in 0 .. 3");
    // W == NULL: wsplit still holds the image a previous call made from the same weights
    if (W) TRY(build_images(h8_image_multi_launch, wsplit, K, s, {W, Nout, K, g.h6 ? H8_H6 : H8_MLP0}), "linear_h8_img(image)");
    TRY(gemm_h8_astat_launch(g, s), "linear_h8_img");
    return 0;
}

int gecco_linear_h8_areg_f32(const void* a_img, const float* W, const float* bias, const float* residual, float* C, float* stats,
                             int B, int rows, int K, int Nout, void* wsplit, void* stream) {
    if (!a_img || !C || !wsplit) return fail(-1, "linear_h8_areg: null argument");
    hipStream_t s = (hipStream_t)stream;
    GemmArgs g = gemm_args(static_cast<const float*>(a_img), nullptr, bias, C, B, rows, K, Nout);
    g.residual = residual; g.stats = stats; g.a_img = 2; g.w_img = wsplit; g.precision = 1;
    if (!gemm_h8_areg_supported(g))
        return fail(-2, "linear_h8_areg: needs rows %% 128 == 0, K in {128, 256, 384, 512, 768, 1024}, Nout %% 4 == 0");
    // W == NULL: wsplit still holds the image a previous call made from the same weights
    if (W) TRY(build_images(h8_image_multi_launch, wsplit, K, s, {W, Nout, K, H8_W128}), "linear_h8_areg(image)");
    TRY(gemm_h8_areg_launch(g, s), "linear_h8_areg");
    return 0;
}

int gecco_mlp_fused_f16(float* x, const float* pro_a, const float* pro_o, const float* W0, const float* b0, const float* W2,
                        const float* b2, const float* alpha, int act, float* stats, int B, int rows, int C, int width,
                        void* wsplit, void* stream) {
    if (!x || !pro_a || !pro_o || !wsplit || ((W0 == nullptr) != (W2 == nullptr))) return fail(-1, "mlp_fused: null argument");
    if (int rc = check_alpha("mlp_fused", act, alpha, -6)) return rc;
    if (!mlp_fused_f16_supported(C, width, rows))
        return fail(-2, "mlp_fused: needs C in {128, 256, 384}, width == 2 C, rows %% 128 == 0");
    hipStream_t s = (hipStream_t)stream;
    float* img = static_cast<float*>(wsplit);
    if (W0) {   // W0 == W2 == NULL: wsplit holds the image already
        SplitJobs jobs;   // (3 jobs per hidden chunk, width <= 768: 18 of the table's 96)
        jobs.n = 0;
        TRY(mlp_fused_f16_stream_jobs(W0, W2, C, width, img, [&jobs](const float* W, float* at, int Nout, int K, int ldw, F16Image format, const char*) {
                if (jobs.n >= (int)(sizeof jobs.job / sizeof jobs.job[0])) return -9;
                jobs.job[jobs.n++] = SplitJob{W, at, Nout, K, ldw, format};
                return 0;
            }), "mlp_fused(split)");
        TRY(split_f16_tiled_multi_launch(jobs, s), "mlp_fused(split)");
    }
    MlpArgs ma{};
    ma.x = x; ma.pro_a = pro_a; ma.pro_o = pro_o; ma.w_stream = img; ma.b0 = b0; ma.b2 = b2; ma.alpha = alpha; ma.act = act;
    ma.stats = stats; ma.B = B; ma.rows = rows;
    TRY(mlp_fused_f16_launch(ma, C, width, s), "mlp_fused");
    return 0;
}

int gecco_unpool_outproj_f16(float* x, const void* q16, const float* kvh, const float* W, const float* bias, float* stats,
                             int B, int rows, int C, int H, void* wsplit, void* stream) {
    if (!x || !q16 || !kvh || !wsplit) return fail(-1, "unpool_outproj: null argument");
    if (!unpool_outproj_f16_supported(C, H, rows))
        return fail(-2, "unpool_outproj: needs (C, head dim) in {(128, 16), (256, 32), (384, 48)}, rows %% 128 == 0");
    hipStream_t s = (hipStream_t)stream;
    if (W) TRY(split_f16_tiled_launch(W, wsplit, C, C, C, s), "unpool_outproj(split)");   // W == NULL: image ready
    UnpoolProjArgs ua{};
    ua.x = x; ua.q16 = q16; ua.kvh = kvh; ua.w_stream = static_cast<const float*>(wsplit); ua.bias = bias; ua.stats = stats;
    ua.B = B; ua.rows = rows; ua.H = H;
    TRY(unpool_outproj_f16_launch(ua, C, s), "unpool_outproj");
    return 0;
}

int gecco_unpool_outproj_h8(float* x, const void* q16, const float* kvh, const float* W, const float* bias, float* stats,
                            int B, int rows, int C, int H, void* wsplit, void* stream) {
    if (!x || !q16 || !kvh || !wsplit) return fail(-1, "unpool_outproj_h8: null argument");
    if (!unpool_outproj_h8_supported(C, H, rows))
        return fail(-2, "unpool_outproj_h8: needs (C, head dim) in {(128, 16), (256, 32), (384, 48)}, rows %% 128 == 0");
    hipStream_t s = (hipStream_t)stream;
    if (W) TRY(build_images(h8_image_multi_launch, wsplit, C, s, {W, C, C, H8_ATTN_ORDER}), "unpool_outproj_h8(split)");   // W == NULL: image ready
    void* kvimg = static_cast<char*>(wsplit) + h8_image_bytes(C, C);
    TRY(kvh_image_launch(kvh, kvimg, B, C, H, s), "unpool_outproj_h8(k | v image)");
    UnpoolH8Args ua{};
    ua.x = x; ua.q16 = q16; ua.kv_img = kvimg; ua.w_img = wsplit; ua.bias = bias; ua.stats = stats; ua.B = B; ua.rows = rows; ua.H = H;
    TRY(unpool_outproj_h8_launch(ua, C, s), "unpool_outproj_h8");
    return 0;
}

int gecco_mlp_fused_w(const float* x, float* out, const float* pro_a, const float* pro_o, const float* W0, const float* b0, const float* W2,
                      const float* b2, const float* alpha, int act, float* stats, int B, int rows, int C, int width, void* wsplit, float* dbg_u,
                      void* stream) {
    if (!x || !out || !pro_a || !pro_o || !wsplit) return fail(-1, "mlp_fused_w: null argument");
    if (!mlp_fused_w_supported(C, width, rows)) return fail(-2, "mlp_fused_w: needs C in {128, 256, 384, 512}, width == 2 C, rows %% 128 == 0");
    if (act < 0 || act > 3) return fail(-6, "mlp_fused_w: act must be 0 .. 3");
    if (int rc = check_alpha("mlp_fused_w", act, alpha, -6)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (W0 && W2) TRY(mlp_fused_w_image_launch(W0, b0, W2, b2, wsplit, C, width, alpha, act, s), "mlp_fused_w(image)");   // W0 == NULL: image ready (biases included)
    MlpWArgs ma{};
    ma.x = x; ma.out = out; ma.pro_a = pro_a; ma.pro_o = pro_o; ma.w_img = wsplit; ma.alpha = alpha; ma.act = act; ma.stats = stats;
    ma.B = B; ma.rows = rows; ma.dbg_u = dbg_u; ma.share = option(OPT_MLPWSHARE);
    TRY(mlp_fused_w_launch(ma, C, width, s), "mlp_fused_w");
    return 0;
}

size_t gecco_mlp_fused_w_wsplit_bytes(int C, int width) { return mlp_fused_w_image_bytes(C, width); }

size_t gecco_unpool_outproj_h8_wsplit_bytes(int B, int C, int H) {
    if (H <= 0 || C % H) return 0;
    return h8_image_bytes(C, C) + unpool_outproj_h8_kv_bytes(B, C, H);
}

int gecco_unpool_attn_h8img(const void* q16, const float* kvh, void* out_img, int B, int N, int C, int H, void* stream) {
    if (!q16 || !kvh || !out_img) return fail(-1, "unpool_attn_h8img: null argument");
    if (N % 128 || C % 64 || H <= 0 || C % H || !attn_x3_supported(C / H)) return fail(-2, "unpool_attn_h8img: needs N %% 128 == 0, C %% 64 == 0, head dim 16 / 32 / 48 / 64");
    TRY(unpool_attn_launch(static_cast<const float*>(q16), kvh, static_cast<float*>(out_img), B, N, C, H, 64, (hipStream_t)stream, 2, 2, 1, 2),
        "unpool_attn_h8img");
    return 0;
}

int gecco_gemm_tn_x3_f32(const float* A, const float* Bm, float* parts, int Z, int R, int N, int K, int group, void* stream) {
    return gecco_gemm_tn_x3_bias_f32(A, Bm, parts, nullptr, Z, R, N, K, group, stream);
}

int gecco_gemm_tn_x3_bias_f32(const float* A, const float* Bm, float* parts, float* colsum_parts, int Z, int R, int N, int K,
                              int group, void* stream) {
    return gecco_gemm_tn_x3_pro_f32(A, Bm, nullptr, nullptr, parts, colsum_parts, Z, R, N, K, group, stream);
}

// The operands every TN product (parts[z / group] += A_z^T Bm_z over contiguous (R, N) and (R, K) samples) has
static TnArgs tn_args(const void* A, const void* Bm, const float* pro_a, const float* pro_o, float* parts, float* colsum_parts, int Z, int R, int N, int K, int group) {
    TnArgs g{};
    g.pro_a = pro_a; g.pro_o = pro_o;
    g.A = static_cast<const float*>(A); g.Bm = static_cast<const float*>(Bm); g.C = parts; g.Z = Z; g.R = R; g.N = N; g.K = K; g.lda = N; g.ldb = K;
    g.sA = (size_t)R * N; g.sB = (size_t)R * K; g.group = group; g.colsum = colsum_parts;
    return g;
}

int gecco_gemm_tn_x3_pro_f32(const float* A, const float* Bm, const float* pro_a, const float* pro_o, float* parts,
                             float* colsum_parts, int Z, int R, int N, int K, int group, void* stream) {
    if (!A || !Bm || !parts) return fail(-1, "gemm_tn_x3: null argument");
    if (int rc = check_pro_pair("gemm_tn_x3", pro_a, pro_o, true)) return rc;
    const TnArgs g = tn_args(A, Bm, pro_a, pro_o, parts, colsum_parts, Z, R, N, K, group);
    if (!gemm_tn_x3_supported(g)) return fail(-2, "gemm_tn_x3: needs R %% 32 == 0, N %% 4 == 0, K %% 4 == 0, group > 0");
    TRY(gemm_tn_x3_launch(g, (hipStream_t)stream), "gemm_tn_x3");
    return 0;
}

// The fp16 TN product's entry points differ in which operand is an fp16 tensor, and in how they word (`needs`) what the kernel takes
static int gemm_tn_f16(const char* who, const char* needs, const void* A, int a_f16, const void* Bm, int b_f16, const float* pro_a, const float* pro_o, float* parts,
                       float* colsum_parts, float* out, float* colsum_out, unsigned* counters, int Z, int R, int N, int K, int group, void* stream) {
    if (!A || !Bm || !parts) return fail(-1, "%s: null argument", who);
    if (int rc = check_pro_pair(who, pro_a, pro_o, true)) return rc;
    TnArgs g = tn_args(A, Bm, pro_a, pro_o, parts, colsum_parts, Z, R, N, K, group);
    g.f16 = 1; g.a_f16 = a_f16; g.b_f16 = b_f16; g.counters = counters; g.out = out; g.colsum_out = colsum_out;
    if (!gemm_tn_f16_supported(g)) return fail(-2, "%s: needs %s", who, needs);
    TRY(gemm_tn_f16_launch(g, (hipStream_t)stream), who);
    return 0;
}

int gecco_gemm_tn_f16_b16_f32(const float* A, const void* B16, float* parts, float* colsum_parts, int Z, int R, int N, int K, int group,
                              void* stream) {
    return gemm_tn_f16("gemm_tn_f16_b16", "R % 32 == 0, N % 4 == 0, K % 8 == 0, group > 0", A, 0, B16, 1, nullptr, nullptr, parts, colsum_parts, nullptr, nullptr, nullptr,
                       Z, R, N, K, group, stream);
}

int gecco_gemm_tn_f16_ex_f32(const void* A, int a_f16, const void* Bm, int b_f16, const float* pro_a, const float* pro_o, float* parts,
                             float* colsum_parts, float* out, float* colsum_out, unsigned* counters, int Z, int R, int N, int K, int group,
                             void* stream) {
    if (!A || !Bm || !parts) return fail(-1, "gemm_tn_f16_ex: null argument");   // (its own checks sit between these two and the kernel's)
    if (int rc = check_pro_pair("gemm_tn_f16_ex", pro_a, pro_o, true)) return rc;
    if ((counters != nullptr) != (out != nullptr) || (colsum_out && !(colsum_parts && counters)))
        return fail(-1, "gemm_tn_f16_ex: counters and out go together; colsum_out needs colsum_parts and counters");
    if (a_f16 && b_f16 && (pro_a || counters || N % 128 || K % 128))
        return fail(-2, "gemm_tn_f16_ex: both operands fp16: whole 128 x 128 tiles, no AdaGN apply, the separate reduction");
    return gemm_tn_f16("gemm_tn_f16_ex", "R % 32 == 0, N % 4 == 0, K % 4 == 0 (8 for an fp16 operand's width), group > 0", A, a_f16 != 0, Bm, b_f16 != 0, pro_a, pro_o,
                       parts, colsum_parts, out, colsum_out, counters, Z, R, N, K, group, stream);
}

int gecco_gemm_tn_f16_a16_f32(const void* A16, const float* Bm, const float* pro_a, const float* pro_o, float* parts, float* colsum_parts,
                              int Z, int R, int N, int K, int group, void* stream) {
    return gemm_tn_f16("gemm_tn_f16_a16", "R % 32 == 0, N % 8 == 0, K % 4 == 0, group > 0", A16, 1, Bm, 0, pro_a, pro_o, parts, colsum_parts, nullptr, nullptr, nullptr,
                       Z, R, N, K, group, stream);
}

int gecco_gemm_tn_f16_f32(const float* A, const float* Bm, const float* pro_a, const float* pro_o, float* parts,
                          float* colsum_parts, int Z, int R, int N, int K, int group, void* stream) {
    return gemm_tn_f16("gemm_tn_f16", "R % 32 == 0, N % 4 == 0, K % 4 == 0, group > 0", A, 0, Bm, 0, pro_a, pro_o, parts, colsum_parts, nullptr, nullptr, nullptr,
                       Z, R, N, K, group, stream);
}
int gecco_gemm_tn_f16_tiles(int N, int K) { return gemm_tn_f16_tiles(N, K); }

int gecco_gemm_f32(const GeccoGemm* g, void* stream) {
    if (!g || !g->A || !g->B || !g->C) return fail(-1, "gemm: null argument");
    GemmGeneralArgs a;
    a.A = g->A; a.B = g->B; a.bias = g->bias; a.C = g->C; a.Z = g->Z; a.zdiv = g->zdiv > 0 ? g->zdiv : 1;
    a.M = g->M; a.N = g->N; a.K = g->K; a.lda = g->lda; a.ldb = g->ldb; a.ldc = g->ldc;
    a.sA1 = g->sA1; a.sA2 = g->sA2; a.sB1 = g->sB1; a.sB2 = g->sB2; a.sC1 = g->sC1; a.sC2 = g->sC2;
    a.a_kmajor = g->a_kmajor; a.b_kmajor = g->b_kmajor; a.scale = g->scale;
    TRY(gemm_general_launch(a, (hipStream_t)stream), "gemm");
    return 0;
}

}  // extern "C"
