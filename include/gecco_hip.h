/* gecco_hip.h — C ABI of libgecco_hip.so: the MI355X (gfx950) implementation of the GECCO
 * denoiser hot path.
 *
 * The reference (cvlab-epfl/gecco, gecco-torch) has no FFI/plugin layer: its extension surface
 * is "Python that constructs nn.Modules".  This header is therefore the boundary a maintainer
 * binds (ctypes stub in INTEGRATION.md) underneath the same-named Python modules; every entry
 * point cites the reference code it replaces (paths relative to
 * gecco-torch/src/gecco_torch/).
 *
 * Conventions
 *  - all pointers are raw DEVICE pointers to contiguous fp32 (fp64 where the name says so);
 *    activations are channels-last (B, n, C) row-major, weights are nn.Linear layout (out, in);
 *  - `stream` is a hipStream_t (0 = default stream); calls only enqueue work: no allocation, no
 *    synchronisation, no host reads — they are hipGraph-capture safe;
 *  - scratch memory is caller-provided (`ws`, size from the matching *_workspace_bytes());
 *  - return value 0 = success; negative = argument error (see gecco_last_error()); positive =
 *    hipError_t of the launch.
 */
#ifndef GECCO_HIP_H
#define GECCO_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GECCO_ABI_VERSION 15

int gecco_abi_version(void);
const char* gecco_build_arch(void);   /* "gfx950" */
const char* gecco_last_error(void);   /* thread-local description of the last non-zero return */

/* ---- parameter tables (device pointers into the module's own state-dict tensors) ------------ */
typedef struct GeccoAdaGN {   /* AdaGN, models/normalization.py:14-44 */
    const float* scale_w;     /* scale.weight (C, ctx_dim) */
    const float* scale_b;     /* scale.bias   (C)          */
    const float* bias_w;      /* bias.weight  (C, ctx_dim) */
    const float* bias_b;      /* bias.bias    (C)          */
} GeccoAdaGN;

typedef struct GeccoMLP {     /* MLP(depth=1) + GaussianActivation, models/mlp.py:5-39, activation.py */
    const float* w0;          /* 0.weight (width, C) */
    const float* b0;          /* 0.bias   (width)    */
    const float* alpha;       /* 1.alpha  ()         */
    const float* w2;          /* 2.weight (C, width) */
    const float* b2;          /* 2.bias   (C)        */
} GeccoMLP;

typedef struct GeccoLayer {   /* BroadcastingLayer, models/set_transformer.py:120-168 */
    GeccoAdaGN broadcast_norm;
    const float* inducers;    /* broadcast.pool.inducers (1, H, I, hd)   */
    const float* kv_proj_w;   /* broadcast.pool.kv_proj.weight (2C, C)   */
    const float* pool_out_w;  /* broadcast.pool.out_proj.weight (C, C)   */
    GeccoAdaGN norm_1;
    GeccoMLP bmlp;            /* broadcast.mlp */
    GeccoAdaGN norm_2;
    const float* in_proj_w;   /* broadcast.unpool.in_proj_weight (3C, C) */
    const float* in_proj_b;   /* broadcast.unpool.in_proj_bias (3C)      */
    const float* unpool_out_w;/* broadcast.unpool.out_proj.weight (C, C) */
    const float* unpool_out_b;/* broadcast.unpool.out_proj.bias (C)      */
    GeccoAdaGN mlp_norm;
    GeccoMLP mlp;
} GeccoLayer;

typedef struct GeccoSetTransformer {  /* SetTransformer, models/set_transformer.py:171-216 */
    int n_layers, C, H, I, ctx_dim, G, width, act;  /* act of the MLPs: 0 identity, 1 GaussianActivation(normalized), 2 raw, 3 nn.ReLU */
    int precision;  /* arithmetic of the linears and attention products: 0 exact fp32 MFMA (~1e-6 vs the fp32
                     * reference), 1 split-bf16 on bf16 MFMA, fp32 accumulate (a = hi + lo; 3 MFMAs; ~2e-5),
                     * 2 fp16 operands (round to nearest even), fp32 accumulate, fp16-stored intermediates (D ~4e-4, F_x ~1e-3),
                     * 3 "mixed": kv_proj | q_proj with fp16 activations and two-term fp16 weights, fp16 K | V / q and attention
                     *   products; every product that feeds the residual stream or the shared inducer states (the 64-inducer
                     *   chain, unpool.out_proj, the point MLP) in split-bf16 (~6e-5 on both outputs); point counts that are
                     *   not a multiple of 128 (and widths / head dims outside the fp16 kernels' set) run as mode 1,
                     * 4 "w2": mode 3 with the point MLP of every layer as ONE launch whose hidden layer stays in registers as fp16
                     *   (gecco_mlp_fused_w: two-term weights and AdaGN(x), one-term hidden layer): F_x ~3.5e-4, inside a 5e-4 bar;
                     *   feature_dim 128, 256, 384 or 512 with point counts in multiples of 128, anything else runs as mode 3 */
    int images_ready;  /* 0: every forward rebuilds the weight images it streams (weights may change between calls; the default).
                        * 1: the caller guarantees that the workspace of this call still holds the images the previous forward with this
                        *    table, the same (B, N), the same options and the same cached / uncached form built in it, and that no weight
                        *    changed since: the forward skips the image launches (a sampler's 2nd .. 255th evaluation) */
    unsigned opt_mask, opt_vals;  /* this plan's own path switches (ABI 14): bit gecco_option_index(name) of opt_mask set = the option is
                                   * pinned to the same bit of opt_vals for every forward with this table, whatever gecco_set_option /
                                   * the environment say; clear = follow the process-wide default.  The reference's modules are
                                   * self-contained (models/set_transformer.py:176-216): so are these tables. */
    const GeccoLayer* layers;                       /* HOST array of n_layers tables */
} GeccoSetTransformer;

/* ---- unit operators --------------------------------------------------------------------- */

/* C = residual + act((A*pro_a + pro_o) @ W^T + bias); optional GroupNorm partial statistics of C.
 * Replaces nn.Linear call sites of models/set_transformer.py:49,65,112,165-166 and models/mlp.py.
 * stats: (B, T, 2, Nout) with T = gecco_linear_row_tiles(rows).  Any of bias/pro/alpha/residual/stats
 * may be NULL.  act: 0 none, 1 / 2 GaussianActivation normalized / raw (alpha required), 3 ReLU (the reference's
 * default activation, models/mlp.py:12), 4 GELU in its exact erf form (the conditioner's CNBlocks). */
int gecco_linear_f32(const float* A, const float* W, const float* bias, const float* pro_a, const float* pro_o,
                     const float* alpha, const float* residual, float* C, float* stats, int B, int rows, int K,
                     int Nout, int act, void* stream);
/* Path switches for A/B measurements and tests (the results agree to rounding):
 *   "astat" (default 1): fp16 mode runs AdaGN + kv|q and AdaGN + mlp.0 as one A-stationary pass over x;
 *   "chain" (default 1): fp16 mode runs the 64-inducer chain of a layer (pool merge .. unpool k|v) as one launch;
 *   "headmajor" (default 1): fp16 mode stores K | V and q head-major (needs "astat");
 *   "mlpfused" (default 1): fp16 mode runs AdaGN + mlp.0 + activation + mlp.2 + residual + statistics as one launch;
 *   "unpoolfused" (default 1): fp16 mode runs unpool attention + out_proj + residual + statistics as one launch
 *   (needs "headmajor").
 *   "lo8" (default 1): mixed mode streams the second term of the V projection's two-term weights as fp8 (e4m3, x 2^19) on
 *   v_mfma_scale_f32_32x32x64_f8f6f4 (d = 256, 384) instead of as fp16: same result to ~1e-6 of the output.
 *   "actimg" (default 1): split-bf16 / mixed modes hand the MLP hidden layer and the unpool attention output to the next
 *   GEMM as tiled split images (bf16 hi | lo planes in 8 KiB blocks, same bytes as the fp32 tensor) which that GEMM loads
 *   global -> registers (gemm_x3_areg.hip): same bits as the fp32 hand-over.
 *   "h8" (default 1): mixed mode runs mlp.0 as an fp16 main product plus two fp8 cross terms (v_mfma_scale_f32_32x32x64_f8f6f4)
 *   on the A-stationary kernel (gemm_h8_astat.hip: 128-row blocks; needs "actimg", rows % 128 == 0, feature_dim 128 / 256 / 384, or 512 at one block per CU) instead of as a
 *   split-bf16 product: 2 instead of 3 matrix-pipe units per product, same accuracy (~6e-5 on F_x).
 *   "h8areg" (default 1): mixed mode hands the MLP hidden layer and the unpool attention output on as h8 activation images
 *   (fp16 hi + fp8 lo, 3 bytes per element) and runs mlp.2 / out_proj as h8 products (gecco_linear_h8_areg_f32) instead of
 *   split-bf16 products on tiled split images: 2 instead of 3 matrix-pipe units per product, same accuracy (needs "h8").
 *   "unpoolh8" (default 1): mixed mode runs unpool attention + out_proj (h8) + residual + statistics as one launch
 *   (gecco_unpool_outproj_h8) instead of the attention writing an h8 activation image for gecco_linear_h8_areg_f32; needs
 *   "kvq64" (head-major fp16 q), "h8areg", feature_dim in {128, 256, 384, 512} with 8 heads.
 *   "mlpw" (default 1): the "w2" mode (precision 4) runs the point MLP of a layer (AdaGN apply, mlp.0, activation, mlp.2, residual,
 *   statistics) as one launch (gecco_mlp_fused_w); 0: as the mixed mode does (gecco_linear_h8_img_f32 + gecco_linear_h8_areg_f32).
 *   "mlpwshare" (default 0): gecco_mlp_fused_w launches (a block fills its CU) take three quarters of the CUs instead of all of them, so
 *   that another stream's kernels run beside them: set around an evaluation issued as two half batches on two streams.
 *   "h6" (default 1): mixed mode computes mlp.0's two cross terms as fp6 (e2m3) x fp6 with one E8M0 scale per lane and 64-k group (the
 *   scale blocks of v_mfma_scale_f32_32x32x64_f8f6f4) instead of fp8 with fixed scales: half their matrix cycles, the same accuracy;
 *   gecco_linear_h8_img_f32 with image_kind 2 follows it too.
 *   "chaincl" (default 1): the one-launch inducer chain ("chain" / "chain2") runs as a cluster of feature_dim / 128 blocks per sample that
 *   hand each other their column tiles through L2 (bit-identical to one block per sample; feature_dim >= 256); with it the mixed mode
 *   runs the one-launch chain at feature_dim 512 too.
 *   "kvfold" (default 1): mixed mode with "unpoolh8": the chain's last epilogue writes the fp16 k | v image gecco_unpool_outproj_h8
 *   streams instead of fp32 k | v for a reformatting launch (same bits).
 *   "chain2" (default 1): mixed mode runs the 64-inducer chain of a layer (pool merge .. unpool k|v) as the ONE launch of the fp16
 *   mode with two-term fp16 weights (hi | lo blocks per column tile) instead of five 64-row split-bf16 GEMMs + their AdaGN
 *   coefficient launches: 16 -> 9 launches per layer; F_x 6e-5 -> ~1e-4 (its activations are rounded to fp16 once).
 *   "kvq64" (default 1): mixed mode runs kv_proj | q_proj on the 64-column-tile A-stationary kernel (gecco_linear_kvq_f16; needs
 *   "headmajor") instead of the 128-column-tile one (gecco_linear_astat_f16 + lo image): same arithmetic, also at feature_dim 512.
 *   "kvqperm" (default 1): mixed mode at head dim 48 (feature_dim 384): the kvq stream deals the columns of K, V and q to the 64-column tiles
 *   head-aligned (a tile = one head + a third of another) and gecco_linear_kvq_f16's epilogue writes a head's (32 rows, 48) slab as three
 *   contiguous 1 KiB stores through LDS instead of as 32-byte pieces: the same bits, fewer partial cache lines.
 *   "imgproj16" (default 0: opt-in): "w2" mode of gecco_ray_network_fwd_f32: the lookup leaves halves, GroupNorm(16)'s apply is folded into
 *   per-sample fp16 images of img_feature_proj's weight (and its offsets into the bias), and the product fp16(lookup) x fp16(W a) runs one
 *   term each on the fp16-operand streaming kernel instead of split-bf16: 280 -> 154 + 24 us at C3 (2 % of an evaluation) for F_x 2.3e-4 ->
 *   2.7e-4 at C3 and up to 3.2e-4 -> 4.7e-4 on small pyramids (the mode's bar is 5e-4) — off unless asked for.
 *   "lift0" (levels 0 / 1 / 2; default: 2 at feature_dim >= 256, where it is faster, 0 below): gecco_linear_lift_fwd_f32 computes layer 0's K | V | q from the 3-D points — they are an affine map
 *   of three numbers per point — instead of as a (B N) x C -> 3C matrix product: 1 writes K | V and q from the points (gecco_lift0_fold_f32 +
 *   gecco_lift0_rows), 2 writes q only and runs the layer's pool attention on the points (gecco_lift0_pool_f32), so its K | V never exist;
 *   0 the launches of every other layer.  Any arithmetic mode, any point count.  In a plan's table (opt_mask / opt_vals) the option takes its
 *   own bit for "level >= 1" and the bit above it for "level 2".
 * value < 0 returns the option to its default / environment (GECCO_ASTAT, GECCO_CHAIN, GECCO_HEADMAJOR, GECCO_MLPFUSED,
 * GECCO_UNPOOLFUSED, GECCO_LO8, GECCO_ACTIMG, GECCO_H8, GECCO_KVQ64, GECCO_H8AREG, GECCO_CHAIN2).
 * Process-wide DEFAULT: a network forward consults its own table first (GeccoSetTransformer.opt_mask / opt_vals, ABI 14), so two
 * plans — or two host threads — with different settings never alias; the unit operators below follow the process-wide value. */
int gecco_set_option(const char* name, int value);
/* Bit position of an option in GeccoSetTransformer.opt_mask / opt_vals (-1: unknown name). */
int gecco_option_index(const char* name);

int gecco_linear_row_tiles(int rows);
/* The same with the arithmetic selectable: precision 0 = exact fp32 MFMA, 1 = split-bf16, 2 = fp16 (see GeccoSetTransformer);
 * wsplit: scratch of >= ceil(Nout/128)*128*K*4 bytes for the tiled image of W (bf16 hi | lo, or fp16; precision 1 / 2). */
int gecco_linear_ex_f32(const float* A, const float* W, const float* bias, const float* pro_a, const float* pro_o,
                        const float* alpha, const float* residual, float* C, float* stats, int B, int rows, int K,
                        int Nout, int act, int precision, void* wsplit, void* stream);
/* Two linears over the same (optionally AdaGN-modulated) input in one launch, A read once:
 *   C1 (B, rows, Nout1) = A' W1^T + bias1,  C2 (B, rows, Nout2) = A' W2^T + bias2,  A' = A*pro_a + pro_o.
 * The layer uses it for AttentionPool.kv_proj and the q rows of nn.MultiheadAttention.in_proj, which both read
 * broadcast_norm(x) (models/set_transformer.py:49 and :112 under :150-155).  Falls back to two launches when
 * Nout1 % 128 != 0 or rows < 128.  wsplit: >= (ceil(Nout1/128) + ceil(Nout2/128))*128*K*4 bytes (precision 1). */
int gecco_linear_pair_f32(const float* A, const float* W1, const float* bias1, int Nout1, float* C1, const float* W2,
                          const float* bias2, int Nout2, float* C2, const float* pro_a, const float* pro_o, int B,
                          int rows, int K, int precision, void* wsplit, void* stream);
/* Weight images prepared AHEAD of the linears that use them (the training step: one launch per <= 96 weights at its start
 * instead of one per linear call, and the dX products' W^T images straight from W — no transposed copy).  A job writes the
 * tiled split-bf16 image (gecco_split_bf16_image_bytes(Nout, K) bytes) of the (Nout, K) matrix W (row stride ldw), or, with
 * transposed != 0, of W^T where W is (K, ldw >= Nout).  gecco_linear_ex_f32 / gecco_linear_pair_f32 with W == NULL (W1 ==
 * W2 == NULL) and precision 1 take `wsplit` as that READY image (pair: the image of W1, then from the next 128-row tile
 * boundary that of W2) and only launch the GEMM; the shape must satisfy gecco_linear_image_ok(rows, K, Nout, prologue?). */
typedef struct GeccoSplitJob { const float* W; void* img; int Nout, K, ldw, transposed; } GeccoSplitJob;
int gecco_split_bf16_images_f32(const GeccoSplitJob* jobs, int n, void* stream);
size_t gecco_split_bf16_image_bytes(int Nout, int K);
int gecco_linear_image_ok(int rows, int K, int Nout, int with_prologue);
/* The same for precision 2 — fp16 operands, fp32 accumulation: the arithmetic of the reference's own trainer setting
 * (example_configs: precision="16-mixed" = torch.autocast(float16) around training_step, diffusion.py:213-222), which the
 * training path selects when it runs under that autocast.  Images are 2 bytes per weight element; K % 32 == 0. */
int gecco_split_f16_images_f32(const GeccoSplitJob* jobs, int n, void* stream);
size_t gecco_split_f16_image_bytes(int Nout, int K);
int gecco_linear_image_ok_f16(int rows, int K, int Nout, int with_prologue);
/* The dX product of the linear that FOLLOWS an activation, with the activation's backward as its epilogue (training:
 * autograd of models/mlp.py's Linear -> act -> Linear, and of a CNBlock's Linear -> GELU -> Linear):
 *   C = residual + (A W^T) * act'(u),   A = dY (B, rows, K), W (Nout, K) = W2^T (or NULL: its ready image in wsplit),
 *   u (B, rows, Nout) the pre-activation the forward kept; dh = dY W2 is never written.
 * kind: 1 / 2 GaussianActivation normalized / raw, 3 ReLU, 4 GELU.  GaussianActivation: alpha (device scalar), and agrad —
 * gecco_linear_actbwd_tiles(B, rows, Nout) floats, ZEROED by the caller — receives per output tile
 * sum (A W^T) * d act / d alpha (u): d alpha = their sum (gecco_reduce_batch_f32).  Shapes: gecco_linear_actbwd_ok. */
int gecco_linear_actbwd_ok(int rows, int K, int Nout, int precision);
size_t gecco_linear_actbwd_tiles(int B, int rows, int Nout);
int gecco_linear_actbwd_f32(const float* A, const float* W, const float* u, const float* alpha, int kind, const float* residual,
                            float* C, float* agrad, int B, int rows, int K, int Nout, int precision, void* wsplit, void* stream);
/* A dX product that also leaves the column statistics the AdaGN backward of its consumer needs: C = A W^T and
 * stats (B, gecco_linear_row_tiles(rows), 2, Nout) = per row tile {sum_rows C, sum_rows C * dot_x}, dot_x (B, rows, Nout) the tensor
 * that AdaGN normalised — what gecco_col_dot_stats_f32 computes from C and dot_x in a pass of its own (autograd of
 * models/normalization.py:36-44 behind a linear: set_transformer.py:165-166).  Shapes: gecco_linear_actbwd_ok; W == NULL: image ready. */
int gecco_linear_dotstats_f32(const float* A, const float* W, const float* dot_x, float* C, float* stats, int B, int rows, int K, int Nout,
                              int precision, void* wsplit, void* stream);
/* The same from an fp16 A tensor (the du of gecco_linear_astat16_actbwd_h16; the dq of an fp16-tensor layer), fp16 arithmetic:
 * C = A16 W^T + residual (fp32; residual may be NULL: another gradient contribution to the same tensor) + the {sum C, sum C x} partials of
 * the SUM.  rows >= 128, K % 32 == 0.  W == NULL: wsplit holds the ready fp16 image. */
int gecco_linear_dotstats_a16_f32(const void* A16, const float* W, const float* dot_x, const float* residual, float* C, float* stats, int B,
                                  int rows, int K, int Nout, void* wsplit, void* stream);
/* Its forward companion: C = act(A W^T + bias) AND pre_out = A W^T + bias (the u the backward needs) from one epilogue — the
 * training forward of Linear -> act without a separate activation pass.  act 1 / 2 / 3 / 4 as above; W == NULL: image ready. */
int gecco_linear_act_keep_f32(const float* A, const float* W, const float* bias, const float* alpha, int act, float* pre_out,
                              float* C, int B, int rows, int K, int Nout, int precision, void* wsplit, void* stream);
/* the same with the AdaGN apply as the prologue of the product: A' = A * pro_a[b, k] + pro_o[b, k] (K <= 1024) */
int gecco_linear_act_keep_pro_f32(const float* A, const float* W, const float* bias, const float* pro_a, const float* pro_o,
                                  const float* alpha, int act, float* pre_out, float* C, int B, int rows, int K, int Nout,
                                  int precision, void* wsplit, void* stream);
/* the same in fp16 arithmetic (precision 2) with act(u) STORED as fp16 (C16out: (B, rows, Nout) halves) beside the fp32
 * pre-activation: under the reference's autocast(float16) trainer setting the hidden layer of an MLP is read again only by the
 * matrix pipe (mlp.2's forward through gecco_linear_f16io with an fp16 A, its weight gradient through
 * gecco_gemm_tn_f16_b16_f32) — as fp16 either way; storing it so halves its bytes.  pro_a / pro_o may be NULL; W == NULL: the fp16
 * image of W is ready in wsplit.  rows >= 128. */
int gecco_linear_act_keep_h16(const float* A, const float* W, const float* bias, const float* pro_a, const float* pro_o,
                              const float* alpha, int act, float* pre_out, void* C16out, int B, int rows, int K, int Nout, void* wsplit,
                              void* stream);

/* ---- The training FORWARD's AdaGN-prologue products in h8 arithmetic (fp16 main product + two fp8 cross terms: as accurate as split-bf16,
 * two matrix units instead of three) on the A-stationary kernel, fp32 tensors: C1 (| C2) = x' W1^T + bias1 (| x' W2^T + bias2),
 * x' = x * pro_a[b] + pro_o[b] or x — broadcast_norm -> kv_proj | q (models/set_transformer.py:161-162 -> :49, :112); with act != 0
 * (1 / 2 GaussianActivation normalized / raw, 3 ReLU; one weight) pre_out = the pre-activation and C1 = act(pre_out): the first linear of
 * an MLP (models/mlp.py:5-39) with what its backward needs.  rows % 128 == 0, K in {128, 256, 384}, Nout % 64 == 0, Nout >= 128
 * (gecco_linear_h8_train_ok).  wsplit: gecco_h8_image_bytes per weight (4 bytes per element); NULL weights: the streams are ready
 * (gecco_h8_images_f32).  The backward products keep split-bf16: unscaled gradients do not fit fp16 / fp8 operands. */
size_t gecco_h8_image_bytes(int Nout, int K);
int gecco_linear_h8_train_ok(int rows, int K, int Nout);
int gecco_h8_images_f32(const GeccoSplitJob* jobs, int n, void* stream);
int gecco_linear_h8_train_f32(const float* x, const float* pro_a, const float* pro_o, const float* W1, const float* bias1, int Nout1, float* C1,
                              const float* W2, const float* bias2, int Nout2, float* C2, const float* alpha, int act, float* pre_out, int B,
                              int rows, int K, void* wsplit, void* stream);

/* ---- A-stationary forms of the training path's products out of a <= 512-wide operand, in the autocast(float16) arithmetic (fp16
 * operands, fp32 accumulation, fp32 tensors): a 128-row block keeps its rows of x (after the optional AdaGN apply) in registers for the
 * whole launch and streams W once — the LDS-DMA GEMM re-fetches the rows for every 128-column tile and is bound by that fill, not by
 * the matrix pipe, once a product is one MFMA.  rows % 128 == 0, K in {128, 256, 384, 512}, Nout % 64 == 0,
 * Nout >= 128 (gecco_linear_astat16_ok).  wsplit: gecco_astat16_image_bytes(Nout, K) bytes per weight (2 per element); a NULL weight
 * means wsplit holds the stream already (gecco_astat16_images_f32: batched, transposed != 0 = the stream of W^T from W (K, ldw)).
 *   _f32:    C1 (| C2) = x' W1^T + bias1 (| x' W2^T + bias2), x' = x * pro_a[b] + pro_o[b] or x — broadcast_norm -> kv_proj | q
 *            (models/set_transformer.py:161-162 -> :49, :112); transposed != 0 (one weight): W1 is (K, Nout1) and C1 = x W1 — a dX product;
 *            residual: pass NULL (a form that adds another gradient contribution to C1 exists only in -DGECCO_EXPERIMENTAL builds: it
 *            bought nothing inside the training step and is not part of the shipped surface);
 *   _keep:   pre_out = u = x' W^T + bias (fp32) and C16out = fp16(act(u)) — the first linear of an MLP (models/mlp.py:5-39), act 1 / 2
 *            GaussianActivation (normalized / raw), 3 ReLU;
 *   _actbwd: C = (dy W) * act'(u), W the linear's own (K, Nout) weight, + for GaussianActivation agrad[B * rows / 128] = per-block
 *            partials of d alpha (their sum is the gradient) — the dX product through the activation. */
size_t gecco_astat16_image_bytes(int Nout, int K);
int gecco_linear_astat16_ok(int rows, int K, int Nout);
int gecco_astat16_images_f32(const GeccoSplitJob* jobs, int n, void* stream);
int gecco_linear_astat16_f32(const float* x, const float* pro_a, const float* pro_o, const float* W1, const float* bias1, int Nout1, float* C1,
                             const float* W2, const float* bias2, int Nout2, float* C2, const float* residual, int transposed, int B, int rows,
                             int K, void* wsplit, void* stream);
int gecco_linear_astat16_keep(const float* x, const float* pro_a, const float* pro_o, const float* W, const float* bias, const float* alpha,
                              int act, float* pre_out, void* C16out, int B, int rows, int K, int Nout, void* wsplit, void* stream);
/* ... and with y16 = fp16(x * pro_a + pro_o) stored as well (see gecco_linear_kvq_y16_f16). */
int gecco_linear_astat16_keep_y16(const float* x, const float* pro_a, const float* pro_o, const float* W, const float* bias, const float* alpha,
                                  int act, float* pre_out, void* C16out, void* y16, int B, int rows, int K, int Nout, void* wsplit,
                                  void* stream);
int gecco_linear_astat16_actbwd(const float* dy, const float* W, const float* u, const float* alpha, int kind, float* C, float* agrad, int B,
                                int rows, int K, int Nout, void* wsplit, void* stream);
/* The same with the result stored as HALVES (round 6): du = (dy W) act'(u) of an MLP's backward is read again only by the matrix pipe — the
 * first linear's weight gradient (gecco_gemm_tn_f16_a16_f32) and its dX product (gecco_linear_dotstats_a16_f32) — as an fp16 operand either
 * way; storing it so halves its three crossings of HBM.  The reference's autocast(float16) backward holds this gradient as an fp16
 * tensor too (autograd of models/mlp.py:5-39 under Lightning's precision="16-mixed", diffusion.py:213-222).  kind 1 / 2 / 3. */
int gecco_linear_astat16_actbwd_h16(const float* dy, const float* W, const float* u, const float* alpha, int kind, void* C16, float* agrad,
                                    int B, int rows, int K, int Nout, void* wsplit, void* stream);

/* GroupNorm partial statistics of x (B, rows, C): stats (B, T, 2, C), T = gecco_stats_row_tiles(rows). */
int gecco_col_stats_f32(const float* x, float* stats, int B, int rows, int C, void* stream);
int gecco_stats_row_tiles(int rows);

/* AdaGN folded to y = a*x + o (models/normalization.py:36-44); p == NULL -> plain GroupNorm (models/ray.py:20-30).
 * t: (B, ctx_dim).  a, o: (B, C). */
int gecco_adagn_coeffs_f32(const float* stats, int T, int rows, const float* t, int ctx_dim, const GeccoAdaGN* p,
                           float* a, float* o, int B, int C, int G, float eps, void* stream);
int gecco_affine_apply_f32(const float* x, const float* a, const float* o, float* y, int B, int rows, int C,
                           void* stream);
/* Full AdaGN.forward: y = AdaGN(x, t).  ws >= gecco_adagn_workspace_bytes(B, rows, C). */
int gecco_adagn_f32(const float* x, const float* t, int ctx_dim, const GeccoAdaGN* p, float* y, int B, int rows,
                    int C, int G, float eps, void* ws, size_t ws_bytes, void* stream);
size_t gecco_adagn_workspace_bytes(int B, int rows, int C);

/* ---- fp16-stored intermediates of the fp16 mode (precision 2) ------------------------------------------------
 * In that mode every point-stream tensor whose only consumer rounds it to fp16 anyway (AdaGN(x) as a GEMM operand,
 * K|V, q, the attention output, the MLP hidden layer) is STORED as fp16: the matrix pipe sees the same bits, a
 * third of the layer's HBM bytes never move.  The residual stream and all statistics stay fp32.  These are the unit
 * forms of the launches gecco_set_transformer_fwd_f32 makes; leading dimensions count elements of the tensor's type. */
/* C = residual + act(A @ W^T + bias) with A and / or C an fp16 tensor (a_f16 / c_f16).  fp16 A: no AdaGN prologue
 * (use gecco_affine_cast_f16 first); fp16 C: no residual, no stats.  rows >= 128, K % 32 == 0.  wsplit as above. */
int gecco_linear_f16io(const void* A, const float* W, const float* bias, const float* alpha, const float* residual,
                       void* C, float* stats, int B, int rows, int K, int Nout, int act, int a_f16, int c_f16,
                       void* wsplit, void* stream);
/* gecco_linear_pair_f32 with fp16 A and fp16 outputs (kv_proj | q_proj of the fp16 mode). */
int gecco_linear_pair_f16io(const void* A, const float* W1, const float* bias1, int Nout1, void* C1, const float* W2,
                            const float* bias2, int Nout2, void* C2, int B, int rows, int K, void* wsplit,
                            void* stream);
/* Image-ready calls (gecco_linear_astat_f16, gecco_mlp_fused_f16, gecco_unpool_outproj_f16): a NULL weight pointer
 * (W1 / W0 and W2 / W) means "wsplit still holds the fp16 weight image a previous call of the same function made from
 * the same weights" — the call then launches the kernel alone (what the network entry points do once per forward, and
 * what bench.py times).
 *
The one-pass form the network uses for kv_proj | q_proj and mlp.0 in the fp16 mode: AdaGN apply + fp16 rounding +
 * all output columns in one pass over x (the block keeps fp16(x*pro_a + pro_o) of its 128 rows in registers and walks
 * every 128-column tile of W1 | W2).  C1 (B, rows, Nout1) and C2 (B, rows, Nout2; W2/bias2/C2 may be NULL) are fp16;
 * act as in gecco_linear_f32.  Bit-identical to gecco_affine_cast_f16 + gecco_linear(_pair)_f16io.
 * rows % 128 == 0, Nout1 % 128 == 0, Nout2 % 128 == 0, K in {128, 256, 384, 512}; wsplit as for the pair.
 * head_dim > 0: head-major outputs — C1 is (B, Nout1 / head_dim, rows, head_dim) and C2 (B, Nout2 / head_dim, rows,
 * head_dim), i.e. "b n (g d) -> b g n d" applied to the row-major result: for kv_proj | q_proj that is one contiguous
 * (rows, head_dim) slab per (sample, K or V, head), the unit a pool / unpool attention block streams (the einops
 * rearranges of models/set_transformer.py:51-52,70 done by the store addressing).  head_dim even, >= 8, dividing
 * Nout1 and Nout2.  0: row-major. */
int gecco_linear_astat_f16(const float* x, const float* pro_a, const float* pro_o, const float* W1, const float* bias1,
                           int Nout1, void* C1, const float* W2, const float* bias2, int Nout2, void* C2,
                           const float* alpha, int act, int B, int rows, int K, int head_dim, void* wsplit,
                           void* stream);
/* kv_proj | q_proj of the mixed mode (models/set_transformer.py:49-52 `kv_proj`, :65-70 the q rows of nn.MultiheadAttention's
 * in_proj, both over AdaGN(x), models/normalization.py:36-44) on the 64-column-tile A-stationary kernel:
 *   C1 (B, rows, Nout1) | C2 (B, rows, Nout2) = fp16( fp16(x*pro_a + pro_o) @ fp16(W)^T + bias ),  fp32 accumulate,
 * where the columns [lo_begin, lo_end) of the first segment (the V projection) add the second weight term
 * fp8(y) @ fp8(2^19 (W - fp16(W)))^T on v_mfma_scale_f32_32x32x64_f8f6f4 (two-term weights: their rounding is the part of this
 * product's error that reaches the output).  head_dim > 0: head-major outputs as gecco_linear_astat_f16.
 * rows % 128 == 0, Nout1, Nout2, lo_begin, lo_end % 64 == 0, K in {128, 256, 384, 512}, head_dim % 8 == 0.
 * wsplit: (Nout1 + Nout2) * K * 2 + (lo_end - lo_begin) * K bytes; W1 == NULL: image-ready call.  Option "kvq64". */
int gecco_linear_kvq_f16(const float* x, const float* pro_a, const float* pro_o, const float* W1, const float* bias1, int Nout1,
                         void* C1, const float* W2, const float* bias2, int Nout2, void* C2, int B, int rows, int K, int head_dim,
                         int lo_begin, int lo_end, void* wsplit, void* stream);
/* The same with the operand the kernel forms, y16 = fp16(x * pro_a + pro_o) (B, rows, K), stored beside the products (round 6): the weight
 * gradients of these very linears read it back as their fp16 X operand (gecco_gemm_tn_f16_ex_f32 with both operands fp16).  y16 may be NULL. */
int gecco_linear_kvq_y16_f16(const float* x, const float* pro_a, const float* pro_o, const float* W1, const float* bias1, int Nout1,
                             void* C1, const float* W2, const float* bias2, int Nout2, void* C2, void* y16, int B, int rows, int K,
                             int head_dim, int lo_begin, int lo_end, void* wsplit, void* stream);
/* mlp.0 of a BroadcastingLayer's point MLP in the mixed mode (models/set_transformer.py:164-166: the first linear of
 * `x + mlp(mlp_norm(x))` with the AdaGN apply of models/normalization.py:44 folded in; models/mlp.py:5-39; activation.py:17-24):
 *   u = act((x*pro_a + pro_o) @ W^T + bias),   product = fp16(y) fp16(W) + fp8(y) fp8(W - fp16(W)) + fp8(y - fp16(y)) fp8(W)
 * (fp32 accumulate; the cross terms on v_mfma_scale_f32_32x32x64_f8f6f4), written as the TILED SPLIT IMAGE the next linear
 * loads into registers.  image_kind 1 — the tiled split image of the split-bf16 consumer: per (sample, 128-row tile, 16-column
 * step) one 8 KiB block, bf16 hi plane [128][16] (the 16-byte half of a row swapped when (row >> 3) & 1), then the lo plane;
 * B * rows * Nout * 4 bytes.  image_kind 2 — the h8 activation image of gecco_linear_h8_areg_f32: per (sample, 128-row tile,
 * 64-column group) one 24 KiB block: 16 KiB of fp16 MFMA fragments [32-row tile][sub][c][lane] (row 32 rt + (lane & 31), columns
 * 32 sub + 16 (lane >> 5) + 8 c + 0 .. 7), then 8 KiB of fp8(2^14 (u - fp16(u))) halves [32-row tile][t][lane] (columns 32 t +
 * 16 (lane >> 5) + 0 .. 15); B * rows * Nout * 3 bytes.
 * rows % 128 == 0, Nout % 64 == 0, K in {128, 256, 384}, act 0 .. 3.  wsplit: Nout * K * 4 bytes; W == NULL: image-ready call. */
int gecco_linear_h8_img_f32(const float* x, const float* pro_a, const float* pro_o, const float* W, const float* bias,
                            const float* alpha, int act, void* c_img, int image_kind, int B, int rows, int K, int Nout,
                            void* wsplit, void* stream);
/* The linear that consumes an h8 activation image (mixed mode: mlp.2 of the point MLP and the unpool attention's out_proj;
 * models/set_transformer.py:112,164-166, models/mlp.py:5-39):  C = residual + A @ W^T + bias  (+ GroupNorm partials `stats`
 * (B, rows / 128, 2, Nout) of C), A = hi + 2^-14 lo read from the image, product = fp16 main term + two fp8 cross terms as in
 * gecco_linear_h8_img_f32, fp32 accumulate.  C may alias residual.  rows % 128 == 0, K in {128, 256, 384, 512, 768, 1024},
 * Nout % 4 == 0.  wsplit: ceil(Nout / 128) * 128 * K * 4 bytes; W == NULL: image-ready call.  Option "h8areg". */
int gecco_linear_h8_areg_f32(const void* a_img, const float* W, const float* bias, const float* residual, float* C, float* stats,
                             int B, int rows, int K, int Nout, void* wsplit, void* stream);
/* The point-stream MLP of a BroadcastingLayer in one launch (fp16 mode; models/set_transformer.py:165-166 with the
 * AdaGN apply of :164 folded in): x += (GaussianActivation(fp16(x*pro_a + pro_o) @ W0^T + b0)) @ W2^T + b2, in place on
 * the fp32 x (B, rows, C); the 2C-wide hidden layer never leaves the CU.  stats (B, rows / 128, 2, C) or NULL: GroupNorm
 * partials of the updated x.  Bit-identical x and stats to gecco_linear_astat_f16 (act) followed by gecco_linear_f16io
 * (fp16 A, residual, stats).  C in {128, 256, 384}, width == 2 C, rows % 128 == 0; wsplit: 4 * C * width bytes. */
int gecco_mlp_fused_f16(float* x, const float* pro_a, const float* pro_o, const float* W0, const float* b0, const float* W2,
                        const float* b2, const float* alpha, int act, float* stats, int B, int rows, int C, int width,
                        void* wsplit, void* stream);
/* The unpool half of a BroadcastingLayer in one launch (fp16 mode; models/set_transformer.py:112 = nn.MultiheadAttention
 * with the 64 inducer states as keys / values, its out_proj, and the residual of :164): x += softmax(q k^T / sqrt(hd)) v @
 * W^T + bias, in place on the fp32 x (B, rows, C).  q16: head-major fp16 (B, H, rows, hd) as gecco_linear_astat_f16
 * (head_dim = hd) writes it; kvh (B, 64, 2C) fp32; stats (B, rows / 128, 2, C) or NULL.  Bit-identical x and stats to
 * gecco_unpool_attn_f16io (head_major) followed by gecco_linear_f16io (fp16 A, residual, stats).
 * (C, hd) in {(128, 16), (256, 32), (384, 48)}, rows % 128 == 0; wsplit: 2 * C * C bytes. */
int gecco_unpool_outproj_f16(float* x, const void* q16, const float* kvh, const float* W, const float* bias, float* stats,
                             int B, int rows, int C, int H, void* wsplit, void* stream);
/* The point MLP of a layer in the "w2" mode, one launch (mlp_fused_w.hip): out = x + mlp.2(act(mlp.0(x * pro_a + pro_o))) — out may be
 * x — with the 2 C wide hidden layer kept in registers.  Arithmetic: fp16 products with fp6 (e2m3, block-scaled) second terms; AdaGN(x)
 * and both weights carry two terms, the hidden layer one (fp16): ~2e-4 of the MLP's output scale against fp32, ~3.5e-4 on a network's
 * F_x (the mixed mode: 6e-5).  stats (B, rows / 128, 2, C) or NULL: GroupNorm partials of out.  Replaces
 * models/set_transformer.py:164-166, models/mlp.py:5-39, models/activation.py:17-24, models/normalization.py:36-44.
 * C in {128, 256, 384, 512} (512: two passes over the hidden width, mlp_fused_w.hip), width == 2 C, rows % 128 == 0; act 0 .. 3; wsplit: gecco_mlp_fused_w_wsplit_bytes(C, width) bytes; W0 == NULL: the weight
 * stream of an earlier call (same weights, biases, activation and alpha: the stream holds them all) is in wsplit.  dbg_u: NULL, or (B, rows, width) receiving mlp.0's
 * pre-activations times sqrt(log2(e) / 2) / |alpha| for the Gaussian activations (the form the kernel computes them in; diagnostics). */
int gecco_mlp_fused_w(const float* x, float* out, const float* pro_a, const float* pro_o, const float* W0, const float* b0, const float* W2,
                      const float* b2, const float* alpha, int act, float* stats, int B, int rows, int C, int width, void* wsplit, float* dbg_u,
                      void* stream);
size_t gecco_mlp_fused_w_wsplit_bytes(int C, int width);
/* The same half of the layer in the MIXED mode, one launch (unpool_outproj_h8.hip; option "unpoolh8", default 1): attention in
 * fp16 (the bits of gecco_unpool_attn_h8img), out_proj as the h8 product (fp16 main product + two fp8 cross terms, as
 * gecco_linear_h8_areg_f32), + bias + residual, in place on x, + GroupNorm partials; the attention output stays in registers as
 * the stationary operand.  Replaces models/set_transformer.py:70-75, 112 and the residual of :164.  Equal to
 * gecco_unpool_attn_h8img followed by gecco_linear_h8_areg_f32 up to fp32 summation order (~1e-6).  (C, hd) in {(128, 16),
 * (256, 32), (384, 48)}, rows % 128 == 0; wsplit: gecco_unpool_outproj_h8_wsplit_bytes(B, C, H) (weight image, then the fp16
 * k | v image of the inducers); W == NULL: the weight image is ready. */
int gecco_unpool_outproj_h8(float* x, const void* q16, const float* kvh, const float* W, const float* bias, float* stats,
                            int B, int rows, int C, int H, void* wsplit, void* stream);
size_t gecco_unpool_outproj_h8_wsplit_bytes(int B, int C, int H);
/* The mixed mode's unpool attention alone (nn.MultiheadAttention core, models/set_transformer.py:112): head-major fp16 q16
 * (B, H, N, hd), kvh (B, 64, 2C) fp32 -> the h8 activation image (image_kind 2 of gecco_linear_h8_img_f32: B * N * C * 3 bytes)
 * that gecco_linear_h8_areg_f32 consumes.  N % 128 == 0, C % 64 == 0, hd in {16, 32, 48, 64}. */
int gecco_unpool_attn_h8img(const void* q16, const float* kvh, void* out_img, int B, int N, int C, int H, void* stream);
/* y16[b, m, c] = fp16(a[b, c] * x[b, m, c] + o[b, c]) — the AdaGN apply (models/normalization.py:44) rounded once,
 * exactly the operand the fp16 GEMM's prologue would form.  C % 8 == 0. */
int gecco_affine_cast_f16(const float* x, const float* a, const float* o, void* y16, int B, int rows, int C,
                          void* stream);
/* gecco_pool_attn_ex_f32 (precision 2) reading an fp16 KV; gecco_unpool_attn_ex_f32 (precision 2) with fp16 q / out.
 * head_major != 0: KV16 is (B, 2H, N, hd) = K heads then V heads, q16 is (B, H, N, hd) (gecco_linear_astat_f16 with
 * head_dim = hd); out16 stays (B, N, C).  Same bits either way. */
int gecco_pool_attn_f16in(const void* KV16, const float* inducers, float* merged, int B, int N, int C, int H, int I,
                          int head_major, void* ws, size_t ws_bytes, void* stream);
int gecco_unpool_attn_f16io(const void* q16, const float* kvh, void* out16, int B, int N, int C, int H, int I,
                            int head_major, void* stream);

/* AttentionPool core (models/set_transformer.py:47-63, without out_proj): KV (B, N, 2C) -> merged (B, I, C). */
int gecco_pool_attn_f32(const float* KV, const float* inducers, float* merged, int B, int N, int C, int H, int I,
                        void* ws, size_t ws_bytes, void* stream);
/* Same with the arithmetic selected: precision 0 = exact fp32 MFMA, 1 = split-bf16 (head dims 16/32/48/64;
 * other head dims run the fp32 kernel).  Same workspace. */
int gecco_pool_attn_ex_f32(const float* KV, const float* inducers, float* merged, int B, int N, int C, int H, int I,
                           int precision, void* ws, size_t ws_bytes, void* stream);
size_t gecco_pool_attn_workspace_bytes(int B, int N, int C, int H, int I);
/* Layer 0 of gecco_linear_lift_fwd_f32 from the 3-D points (option "lift0"): its input is lift(c_in p), an affine map of the points, and
 * broadcast_norm is a per-sample affine map (a1, o1), so [K | V | q](n) = M_b (c_in p_n) + c_b with M_b = W diag(a1_b) W_lift and
 * c_b = W (a1_b * b_lift + o1_b) + bias, W = [kv_proj (2C) | q rows of in_proj (C)] (models/set_transformer.py:49,112,150-155).  The
 * three kernels of that path, for tests: the fold writes mc (B, 3C, 4) = {M_b rows, c_b}; `rows` writes columns col0 .. col0 + ncols of
 * M_b (c_in p_n) + c_b as fp16 (out_f16) or fp32, (B, N, ncols) or head-major (B, ncols / head_dim, N, head_dim); `pool` the merged pool
 * attention (B, 64, C) of `inducers` over the points, K | V never formed (ws: gecco_pool_attn_workspace_bytes(B, N, C, H, 64)).
 * coef: gecco_edm_coeffs_f32's output (c_in at coef[4b + 2]). */
int gecco_lift0_fold_f32(const float* kv_w, const float* q_w, const float* q_b, const float* lift_w, const float* lift_b, const float* a1,
                         const float* o1, float* mc, int B, int C, int H, void* stream);
int gecco_lift0_rows(const float* x, const float* coef, const float* mc, void* out, int col0, int ncols, int head_dim, int out_f16,
                     int B, int N, int C, void* stream);
int gecco_lift0_pool_f32(const float* x, const float* coef, const float* mc, const float* inducers, float* merged, int B, int N, int C,
                         int H, void* ws, size_t ws_bytes, void* stream);

/* Training path: backward of the two attention cores (autograd through F.scaled_dot_product_attention,
 * models/set_transformer.py:55-63, and through nn.MultiheadAttention, :112, under loss.backward(), diffusion.py:213-222),
 * fused: probabilities are recomputed per tile, nothing of shape (B, H, N, I) touches HBM.
 *   gecco_pool_attn_lse_f32: after gecco_pool_attn_ex_f32 on the same workspace, lse (B, H, I) = log2-domain
 *     log-sum-exp of the scaled scores (what the backward needs to recompute P).
 *   gecco_pool_attn_bwd_f32: dO (B, I, C) -> dKV (B, N, 2C) and dQ_partials (P, H, I, hd) with
 *     P = B * gecco_pool_attn_bwd_partials(B, N, H); the caller sums the P partials in order (gecco_reduce_batch_f32).
 *   gecco_unpool_attn_bwd_f32: dO (B, N, C) -> dq (B, N, C) and dkv_partials (P, B, I, 2C) with
 *     P = gecco_unpool_attn_bwd_partials(B, N, H); summed over P by the caller. */
int gecco_pool_attn_lse_f32(const void* ws, size_t ws_bytes, float* lse, int B, int N, int C, int H, int I, void* stream);
int gecco_pool_attn_bwd_partials(int B, int N, int H);
int gecco_pool_attn_bwd_f32(const float* KV, const float* inducers, const float* merged, const float* lse, const float* dO,
                            float* dKV, float* dQ_partials, int B, int N, int C, int H, int I, void* stream);
int gecco_unpool_attn_bwd_partials(int B, int N, int H);
int gecco_unpool_attn_bwd_f32(const float* q, const float* kvh, const float* dO, float* dq, float* dkv_partials, int B, int N,
                              int C, int H, int I, void* stream);
/* the same with the arithmetic selected: precision 0 = exact fp32 MFMA, 1 = split-bf16 (head dims 16 / 32 / 48 / 64; other head
 * dims run the fp32 kernels), 2 = fp16 operands (the reference's autocast(float16) backward: one MFMA per product),
 * 3 (round 6) = 2 with the point-stream tensors as fp16 TENSORS, row-major: pool — KV and dKV (B, N, 2C) halves; unpool — q, dO and dq
 * (B, N, C) halves (pass the pointers through the float* parameters); the inducer-side tensors (inducers, merged, lse, dO of the pool;
 * kvh, the dkv partials) stay fp32.  Head dims 16 / 32 / 48 / 64 only. */
int gecco_pool_attn_bwd_ex_f32(const float* KV, const float* inducers, const float* merged, const float* lse, const float* dO,
                               float* dKV, float* dQ_partials, int B, int N, int C, int H, int I, int precision, void* stream);
int gecco_unpool_attn_bwd_ex_f32(const float* q, const float* kvh, const float* dO, float* dq, float* dkv_partials, int B, int N,
                                 int C, int H, int I, int precision, void* stream);

/* nn.MultiheadAttention core (models/set_transformer.py:112, between in_proj and out_proj):
 * q (B, N, C) projected queries, kvh (B, I, 2C) projected inducer keys|values -> out (B, N, C). */
int gecco_unpool_attn_f32(const float* q, const float* kvh, float* out, int B, int N, int C, int H, int I,
                          void* stream);
int gecco_unpool_attn_ex_f32(const float* q, const float* kvh, float* out, int B, int N, int C, int H, int I,
                             int precision, void* stream);

/* coef: 5*B floats: coef[4b..4b+3] = {c_skip, c_out, c_in, c_noise} (diffusion.py:46-51) and
 * coef[4B + b] = c_noise packed (the AdaGN `t` input for t_embed_dim == 1). */
int gecco_edm_coeffs_f32(const float* sigma, float sigma_data, float* coef, int B, void* stream);
/* out = (c_in * x) @ W^T + b  (linear_lift.py:44 / ray.py:99); coef may be NULL (c_in = 1);
 * stats (B, gecco_stats_row_tiles(N), 2, C) may be NULL. */
int gecco_lift_f32(const float* x, const float* coef, const float* W, const float* bias, float* out, float* stats,
                   int B, int N, int C, void* stream);
/* F = Linear(C->3)(norm(feat)); D = c_skip*x + c_out*F (linear_lift.py:25-29,46; ray.py:56-59,120;
 * diffusion.py:57).  gn_a/gn_o NULL -> per-point LayerNorm; else y = gn_a*feat + gn_o.  out and/or raw. */
int gecco_lower_edm_f32(const float* feat, const float* x, const float* coef, const float* W, const float* bias,
                        const float* gn_a, const float* gn_o, float* out, float* raw, int B, int N, int C, float eps,
                        void* stream);

/* ---- network-level entry points ------------------------------------------------------------ */

/* SetTransformer.forward (models/set_transformer.py:198-216), in place on x (B, N, C).
 * t (B, ctx_dim).  stats_x/stats_T: GroupNorm partials of x from its producer (NULL -> computed here).
 * h_in: NULL or host array of n_layers device pointers (B, I, C) = cached inducer states (`hs`).
 * h_out: NULL or host array of n_layers device pointers to receive them (`return_h`).
 * stats_out: NULL or (B, gecco_linear_row_tiles(N), 2, C) partials of the output (for a GN head). */
int gecco_set_transformer_fwd_f32(const GeccoSetTransformer* st, float* x, const float* t, const float* stats_x,
                                  int stats_T, const float* const* h_in, float* const* h_out, float* stats_out,
                                  int B, int N, void* ws, size_t ws_bytes, void* stream);
size_t gecco_set_transformer_workspace_bytes(const GeccoSetTransformer* st, int B, int N);

typedef struct GeccoLinearLift {   /* EDMPrecond(LinearLift(SetTransformer)), diffusion.py:22-62, linear_lift.py */
    GeccoSetTransformer inner;
    const float* lift_w;    /* lift.weight (C, 3)    */
    const float* lift_b;    /* lift.bias (C)         */
    const float* lower_w;   /* lower.1.weight (3, C) */
    const float* lower_b;   /* lower.1.bias (3)      */
    float sigma_data;
} GeccoLinearLift;

/* Diffusion.forward for the unconditional model (diffusion.py:233-247): x (B, N, 3), sigma (B) ->
 * denoised (B, N, 3); raw (optional) receives F_x. */
int gecco_linear_lift_fwd_f32(const GeccoLinearLift* m, const float* x, const float* sigma, float* denoised,
                              float* raw, const float* const* h_in, float* const* h_out, int B, int N, void* ws,
                              size_t ws_bytes, void* stream);
size_t gecco_linear_lift_workspace_bytes(const GeccoLinearLift* m, int B, int N);

/* ---- geometry width G and LinearLift(do_norm=False) (linear_lift.py:14-31), 1 <= G <= GECCO_MAX_GEOMETRY_DIM ---------------
 * G = 3 with the LayerNorm stays on gecco_lift_f32 / gecco_lower_edm_f32 / GeccoLinearLift above. */
#define GECCO_MAX_GEOMETRY_DIM 16
/* out = (c_in * x) @ W^T + b: x (B, N, G), W (C, G); coef / bias / stats as gecco_lift_f32. */
int gecco_lift_g_f32(const float* x, const float* coef, const float* W, const float* bias, float* out, float* stats,
                     int B, int N, int C, int G, void* stream);
/* F = Linear(C->G)(LayerNorm(feat)) (do_norm != 0) or Linear(C->G)(feat); D = c_skip*x + c_out*F.  W (G, C), bias (G) or NULL;
 * x / out / raw (B, N, G).  C % 4 == 0, C <= 512. */
int gecco_lower_edm_g_f32(const float* feat, const float* x, const float* coef, const float* W, const float* bias, float* out,
                          float* raw, int B, int N, int C, int G, int do_norm, float eps, void* stream);

typedef struct GeccoLinearLiftG {   /* LinearLift(geometry_dim = G, do_norm) under EDMPrecond */
    GeccoLinearLift base;           /* lower_w (G, C): lower.1.weight (do_norm) or lower.weight; lift_w (C, G) */
    int geometry_dim;
    int do_norm;
} GeccoLinearLiftG;

/* gecco_linear_lift_fwd_f32 for a GeccoLinearLiftG: x / denoised / raw (B, N, G). */
int gecco_linear_lift_g_fwd_f32(const GeccoLinearLiftG* m, const float* x, const float* sigma, float* denoised,
                                float* raw, const float* const* h_in, float* const* h_out, int B, int N, void* ws,
                                size_t ws_bytes, void* stream);
size_t gecco_linear_lift_g_workspace_bytes(const GeccoLinearLiftG* m, int B, int N);

/* ---- image-conditional path ------------------------------------------------------------------- */

/* dst[i] = fp16(src[i]) (round to nearest even), n elements: the fp16 texel image of a channels-last pyramid level. */
int gecco_cast_f16(const float* src, void* dst, size_t n, void* stream);

typedef struct GeccoPyramid {     /* FeaturePyramidContext.features, models/feature_pyramid.py:17-20 */
    int n_levels;                 /* <= 4 */
    int C[4], H[4], W[4];
    const float* feat[4];         /* CHANNELS-LAST (B, H, W, C) per level (see gecco_nchw_to_nhwc_f32): fp32, or — texel_f16 — fp16 */
    int texel_f16;                /* 1: the levels hold fp16 texels (gecco_cast_f16 of the fp32 image, made once per conditioner call): the
                                   * forward lookups (gecco_ray_lookup_f32, gecco_ray_network_fwd_f32) gather half the bytes; coordinates, taps
                                   * and weights stay fp32 and bit-exact, the interpolation runs in fp32 on the converted texels.  The gradient
                                   * entry points take fp32 levels only.  The "w2" plans use it; fp32 / bf16x3 / mixed keep fp32 texels. */
} GeccoPyramid;

typedef struct GeccoReparam {     /* reparam.py: 0 NoReparam, 1 GaussianReparam(mean, sigma), 2 UVLReparam */
    int kind;
    const float* mean;            /* (3) mean | uvl_mean */
    const float* std;             /* (3) sigma | uvl_std */
    float logit_scale;            /* UVLReparam.logit_scale (1.1) */
} GeccoReparam;

/* (B, C, H, W) -> (B, H, W, C).  Once per conditioner call; the lookup then runs 2*steps-1 times. */
int gecco_nchw_to_nhwc_f32(const float* src, float* dst, int B, int C, int H, int W, void* stream);

/* F.grid_sample(bilinear, zeros, align_corners=False) tap indices for uv in [0,1]^2 (models/ray.py:79-82):
 * x0,y0 int32 (n), wx1 = ix - x0, wy1 = iy - y0.  Bit-exact against the oracle's op order. */
int gecco_bilinear_taps_f32(const float* uv, int H, int W, int* x0, int* y0, float* wx1, float* wy1, size_t n,
                            void* stream);
/* The fused lookup's whole coordinate chain for every point — geometry (x c_in[b] when coef is given) -> reparametrisation ->
 * project_points -> the bilinear taps of every pyramid level — computed by the SAME device functions gecco_ray_lookup_f32's kernel
 * calls (models/ray.py:64-87, reparam.py:102-110, 159-177, 131-137).  Diagnostics and the bit-exactness tests of the index math:
 * uv (B, N, 2); x0 / y0 int32 and wx1 = ix - x0 / wy1 = iy - y0, each (n_levels, B, N).  Pyramid pointers are not read. */
int gecco_ray_lookup_taps_f32(const float* geom, const float* coef, const float* K, const GeccoReparam* rp, const GeccoPyramid* pyr, float* uv,
                              int* x0, int* y0, float* wx1, float* wy1, int B, int N, void* stream);

/* RayNetwork.extract_image_features (models/ray.py:64-87): geom (B, N, 3) diffusion-space geometry
 * (multiplied by coef's c_in when coef != NULL), K (B, 3, 3) -> out (B, N, sum C).  stats: NULL or
 * (B, gecco_lookup_row_tiles(N), 2, sum C) GroupNorm partials of out. */
int gecco_ray_lookup_f32(const float* geom, const float* coef, const float* K, const GeccoReparam* rp,
                         const GeccoPyramid* pyr, float* out, float* stats, int B, int N, void* stream);
int gecco_lookup_row_tiles(int N);
/* Its backward w.r.t. the pyramids (autograd of F.grid_sample's input under loss.backward(), models/ray.py:82-85):
 * dfeat[l] (B, H_l, W_l, C_l) channels-last, ZEROED by the caller, += tap weight * dout (B, N, sum C).  pyr gives the
 * level shapes (its feat pointers are not read).  Float atomics, like torch's grid_sampler backward: any N; the sorted form
 * below is the one the training path uses for N <= 4096. */
int gecco_ray_lookup_bwd_f32(const float* geom, const float* coef, const float* K, const GeccoReparam* rp,
                             const GeccoPyramid* pyr, const float* dout, float* const* dfeat, int B, int N,
                             void* stream);
/* The lookup's gradient with respect to the GEOMETRY: dgeom (B, N, 3) = autograd of F.grid_sample w.r.t. its grid through the
 * projection and the reparametrisation (models/ray.py:64-87), for a caller that differentiates the conditional denoiser with respect
 * to its input cloud; geom is the diffusion-space geometry the forward saw (c_in already applied), pyr the pyramid it read.
 * dK_partials (optional; dgeom may then be NULL): (B, gecco_lookup_row_tiles(N), 4) partial sums of the gradient with respect to
 * (fx, cx, fy, cy) of each sample's camera matrix — the projection and, for the UVL reparametrisation, the unprojection in front. */
int gecco_ray_lookup_dgeom_f32(const float* geom, const float* K, const GeccoReparam* rp, const GeccoPyramid* pyr, const float* dout,
                               float* dgeom, float* dK_partials, int B, int N, void* stream);
/* The same gradient by SORT + GATHER: per (image, level) the 4 N (texel, point, tap) entries are sorted by texel in LDS, then
 * every texel's threads walk its list — no atomics, a fixed summation order (bit-reproducible), and every texel of dfeat is
 * WRITTEN (no zero fill).  Needs N <= 4096 and H_l W_l <= 2^17 (gecco_ray_lookup_bwd_sorted_workspace_bytes returns 0
 * otherwise: use the atomic form); ws: that many bytes of scratch. */
size_t gecco_ray_lookup_bwd_sorted_workspace_bytes(const GeccoPyramid* pyr, int B, int N);
int gecco_ray_lookup_bwd_sorted_f32(const float* geom, const float* coef, const float* K, const GeccoReparam* rp,
                                    const GeccoPyramid* pyr, const float* dout, float* const* dfeat, int B, int N, void* ws,
                                    size_t ws_bytes, void* stream);

typedef struct GeccoRayNetwork {  /* EDMPrecond(RayNetwork(SetTransformer, reparam)), models/ray.py:33-120 */
    GeccoSetTransformer backbone;
    const float* xyz_w;  const float* xyz_b;   /* xyz_embed (C, 3), (C)                  */
    const float* img_w;  const float* img_b;   /* img_feature_proj.1 (C, sum C_l), (C)   */
    const float* out_w;  const float* out_b;   /* output_proj.1 (3, C), (3)              */
    GeccoReparam reparam;
    float sigma_data;
} GeccoRayNetwork;

/* Diffusion.forward for the image-conditional model with a precomputed feature pyramid
 * (diffusion.py:233-247, post_context given). */
int gecco_ray_network_fwd_f32(const GeccoRayNetwork* m, const float* x, const float* sigma, const float* K,
                              const GeccoPyramid* pyr, float* denoised, float* raw, const float* const* h_in,
                              float* const* h_out, int B, int N, void* ws, size_t ws_bytes, void* stream);
size_t gecco_ray_network_workspace_bytes(const GeccoRayNetwork* m, const GeccoPyramid* pyr, int B, int N);

/* ---- reparameterisations and activation (reparam.py, models/activation.py) -------------------- */
/* inverse = 0: data_to_diffusion, 1: diffusion_to_data.  is_f64 selects float/double x, y (the sampler state is fp64). */
int gecco_gaussian_reparam(const void* x, const float* mean, const float* sigma, void* y, size_t n_elems, int dim,
                           int inverse, int is_f64, void* stream);
int gecco_uvl_reparam(const void* x, const float* K, const float* uvl_mean, const float* uvl_std, double logit_scale,
                      void* y, int B, int N, int inverse, int is_f64, void* stream);
/* nn.ReLU, the reference's default `activation` (models/mlp.py:12, set_transformer.py:81,133), stand-alone and its
 * backward du = dy * (y > 0) (training path).  In the fused kernels ReLU is epilogue code act = 3. */
int gecco_relu_f32(const float* x, float* y, size_t n, void* stream);
int gecco_relu_bwd_f32(const float* y, const float* dy, float* du, size_t n, void* stream);
int gecco_gaussian_act_f32(const float* x, const float* alpha, float* y, size_t n, int normalized, void* stream);

/* ---- sampler state kernels (diffusion.py:271-352, 354-470) ------------------------------------- */
/* sched: DEVICE table of doubles, GECCO_SCHED_COLS per step: {t_cur, t_hat, t_next, churn, redo, 0, 0, 0} with
 * churn = sqrt(t_hat^2 - t_cur^2) * S_noise, redo = sqrt(t_cur^2 - t_next^2); step: DEVICE int (current row).
 * noise pointers are advanced by step * noise_step_stride elements inside the kernel. */
#define GECCO_SCHED_COLS 8
/* x_out = x_cur + (double)((float)sched[step][col] * noise); x_in = (float)x_out; sigma[b] = (float)sched[step][sigma_col] */
int gecco_sampler_add_noise_f64(const double* x_cur, const float* noise, size_t noise_step_stride, const double* sched,
                                const int* step, int col, int sigma_col, double* x_out, float* x_in, float* sigma,
                                size_t n, int B, void* stream);
/* out = x + noise * (float)sched[step][col]; sigma[b] = that coefficient (upsampler's data_ctx, diffusion.py:430) */
int gecco_sampler_add_noise_f32(const float* x, const float* noise, size_t noise_step_stride, const double* sched,
                                const int* step, int col, float* out, float* sigma, size_t n, int B, void* stream);
/* d_cur = (x_hat - den)/t_hat; x_next = x_hat + (t_next - t_hat) d_cur; x_in = (float)x_next; sigma[b] = t_next */
int gecco_sampler_euler_f64(const double* x_hat, const float* den, const double* sched, const int* step, double* d_cur,
                            double* x_next, float* x_in, float* sigma, size_t n, int B, void* stream);
/* x_out = x_hat + (t_next - t_hat) (0.5 d_cur + 0.5 (x_next - den)/t_next) */
int gecco_sampler_heun_f64(const double* x_hat, const double* x_next, const float* den, const double* d_cur,
                           const double* sched, const int* step, double* x_out, size_t n, void* stream);
int gecco_sampler_advance(int* step, int delta, void* stream);
/* x = (double)latents * t0 */
int gecco_sampler_scale_f64(const float* latents, double t0, double* x, size_t n, void* stream);

/* ---- training path (EDMLoss.backward: diffusion.py:136-143 through autograd) ------------------------ */

/* C[z](M x N) = scale * op(A[z]) op(B[z]) (+ bias[n]);  X row-major in its own index (k contiguous) or "k-major"
 * (X[k][row]).  z = z1*zdiv + z2 with element strides (s?1, s?2) per operand.  Backward products use the SAME
 * tensors as the forward ones, only with other layout flags (dX = dY W: B k-major; dW = dY^T X: both k-major). */
typedef struct GeccoGemm {
    const float* A; const float* B; const float* bias; float* C;
    int Z, zdiv, M, N, K, lda, ldb, ldc;
    long long sA1, sA2, sB1, sB2, sC1, sC2;
    int a_kmajor, b_kmajor;
    float scale;
} GeccoGemm;
int gecco_gemm_f32(const GeccoGemm* g, void* stream);
/* out[i] (+)= sum_z parts[z*stride + i], fixed order (deterministic parameter gradients). */
/* Weight gradient of a linear in split-bf16 arithmetic (training path; autograd of every nn.Linear on the point stream):
 * parts[g] = sum over the samples z of group g of A[z]^T @ B[z], A (Z, R, N) = dY, B (Z, R, K) = X, parts
 * (ceil(Z / group), N, K); dW = gecco_reduce_batch_f32 over the groups (fixed order: bit-reproducible).
 * R % 32 == 0, N % 4 == 0, K % 4 == 0 (128 x 128 output tiles; the last tile of a dimension may be partial). */
int gecco_gemm_tn_x3_f32(const float* A, const float* Bm, float* parts, int Z, int R, int N, int K, int group, void* stream);
/* the same, also leaving colsum_parts[g] (ceil(Z / group), N) = column sums of A over the group's rows: the bias gradient
 * db = sum_rows dY comes out of the pass that reads dY for dW (colsum_parts may be NULL) */
int gecco_gemm_tn_x3_bias_f32(const float* A, const float* Bm, float* parts, float* colsum_parts, int Z, int R, int N, int K,
                              int group, void* stream);
/* the same with B read through an AdaGN apply, B'[z, m, k] = B[z, m, k] * pro_a[z, k] + pro_o[z, k] (pro_a / pro_o (Z, K) or
 * both NULL): the weight gradient of a linear whose input was AdaGN(x), formed from x — AdaGN(x) is never materialised */
int gecco_gemm_tn_x3_pro_f32(const float* A, const float* Bm, const float* pro_a, const float* pro_o, float* parts,
                             float* colsum_parts, int Z, int R, int N, int K, int group, void* stream);
/* the same product with both operands rounded to fp16 and ONE MFMA per product (fp32 accumulation, fp32 partials): the weight
 * gradient under the reference's autocast(float16) trainer setting (torch computes it as an fp16 matmul there); pro_a / pro_o
 * and colsum_parts may be NULL.  The caller's GradScaler keeps dY inside fp16's range, as it does for the reference. */
int gecco_gemm_tn_f16_f32(const float* A, const float* Bm, const float* pro_a, const float* pro_o, float* parts,
                          float* colsum_parts, int Z, int R, int N, int K, int group, void* stream);
/* output tiles per sample group of that kernel for an (N, K) gradient (its block tile is 128 x 128, 256 x 128 or 128 x 256 by shape):
 * the caller sizes `group` so that groups x tiles fill the chip */
int gecco_gemm_tn_f16_tiles(int N, int K);
/* the same with B already an fp16 tensor (Z, R, K) — the hidden layer of an MLP that gecco_linear_act_keep_h16 stored that way:
 * its tiles go to LDS as they are (no AdaGN apply) */
int gecco_gemm_tn_f16_b16_f32(const float* A, const void* B16, float* parts, float* colsum_parts, int Z, int R, int N, int K, int group,
                              void* stream);
/* ... and with A (dY) an fp16 tensor (N % 8 == 0), B fp32 with the optional AdaGN apply: the weight gradient of an MLP's first linear from du
 * stored as halves; the bias gradient's column sums are formed from those halves. */
int gecco_gemm_tn_f16_a16_f32(const void* A16, const float* Bm, const float* pro_a, const float* pro_o, float* parts, float* colsum_parts,
                              int Z, int R, int N, int K, int group, void* stream);
/* The general form (round 6): either operand may be the fp16 tensor (a_f16 / b_f16, not both), and — with `counters`, `out` — the
 * fixed-order sum of the group partials happens INSIDE the launch: counters = one zeroed unsigned per output tile
 * (gecco_gemm_tn_f16_tiles(N, K) of them; the kernel leaves them zero), out (N, K) = sum over groups of parts in group order,
 * colsum_out (N) likewise of colsum_parts — the bits gecco_reduce_batch_f32 gives, without its launches (autograd of every nn.Linear
 * under the reference's precision="16-mixed": diffusion.py:213-222). */
int gecco_gemm_tn_f16_ex_f32(const void* A, int a_f16, const void* Bm, int b_f16, const float* pro_a, const float* pro_o, float* parts,
                             float* colsum_parts, float* out, float* colsum_out, unsigned* counters, int Z, int R, int N, int K, int group,
                             void* stream);
int gecco_reduce_batch_f32(const float* parts, float* out, size_t n, int Z, size_t stride, int accumulate, void* stream);

/* Row softmax of the materialised attention scores: P = softmax(scale*S) over the last dim n; and its backward
 * dS = scale * P * (dP - sum(P*dP)). */
int gecco_softmax_fwd_f32(const float* S, float* P, size_t rows, int n, float scale, void* stream);
int gecco_softmax_bwd_f32(const float* P, const float* dP, float* dS, size_t rows, int n, float scale, void* stream);

/* GaussianActivation backward: du = dy*g'(u); partial (gecco_gauss_act_bwd_blocks(n)) per-block sums of dy*dg/dalpha. */
int gecco_gauss_act_bwd_f32(const float* u, const float* dy, const float* alpha, float* du, float* partial, size_t n,
                            int normalized, void* stream);
int gecco_gauss_act_bwd_blocks(size_t n);

/* AdaGN / GroupNorm backward.  gstats (B, gecco_stats_row_tiles(rows), 2, C) = {sum dy, sum dy*x};
 * coefficients give dx = dy*cA + x*cB + cC; ds, dz (B, C) are the grads of the per-(b,c) scale and shift. */
int gecco_col_dot_stats_f32(const float* dy, const float* x, float* gstats, int B, int rows, int C, void* stream);
int gecco_adagn_bwd_coeffs_f32(const float* xstats, int Tx, const float* gstats, int Tg, int rows, const float* t,
                               int ctx_dim, const GeccoAdaGN* p, float* cA, float* cB, float* cC, float* ds, float* dz,
                               int B, int C, int G, float eps, void* stream);
int gecco_affine2_apply_f32(const float* dy, const float* x, const float* cA, const float* cB, const float* cC,
                            float* dx, int B, int rows, int C, void* stream);
/* the same with the gradient that reaches x through the residual connection added in the same pass
 * (x = x + f(norm(x)), models/set_transformer.py:164-166): dx = dy*cA + x*cB + cC + add; add may be NULL */
int gecco_affine2_apply_add_f32(const float* dy, const float* x, const float* cA, const float* cB, const float* cC,
                                const float* add, float* dx, int B, int rows, int C, void* stream);
int gecco_adagn_param_grads_f32(const float* ds, const float* dz, const float* t, int B, int C, int ctx_dim,
                                float* d_scale_w, float* d_scale_b, float* d_bias_w, float* d_bias_b, void* stream);

/* lift backward: partial (B, gecco_stats_row_tiles(N), 4, C) = {dW[:,0], dW[:,1], dW[:,2], db} per row tile. */
int gecco_lift_bwd_f32(const float* dY, const float* xin, float* partial, int B, int N, int C, void* stream);
/* lower backward (LayerNorm + Linear(C->3)): dfeat (rows, C); partial (gecco_lower_bwd_blocks(rows), 3*C + 4). */
int gecco_lower_bwd_f32(const float* feat, const float* dF, const float* W, float* dfeat, float* partial, size_t rows,
                        int C, float eps, void* stream);
int gecco_lower_bwd_blocks(size_t rows);
/* the same for G components (1 .. 16) and either do_norm: lift partial (B, gecco_stats_row_tiles(N), G + 1, C) = {dW^T, db};
 * lower dfeat (rows, C), partial (gecco_lower_g_bwd_blocks(rows), G*C + 16) = {dW (G, C), db (G), 16 - G zeros}. */
int gecco_lift_g_bwd_f32(const float* dY, const float* xin, float* partial, int B, int N, int C, int G, void* stream);
int gecco_lower_g_bwd_f32(const float* feat, const float* dF, const float* W, float* dfeat, float* partial, size_t rows,
                          int C, int G, int do_norm, float eps, void* stream);
int gecco_lower_g_bwd_blocks(size_t rows);

/* ---- optimizer step -------------------------------------------------------------------
 * torch.optim.Adam(lr=1e-4) of Diffusion.configure_optimizers (diffusion.py:210-211) fused with the EMA shadow-weight
 * update the reference runs after every step (EMAOptimizer.step / update, ema.py:273-325; ema_update, ema.py:187-194:
 * ema = ema * decay + (1 - decay) * param): ONE pass over flat, 16-byte aligned fp32 buffers of n elements (n % 4 == 0),
 * 36 bytes per parameter.  Same operation order as torch's single-tensor Adam, in fp32:
 *   g' = g * grad_scale (+ weight_decay * p);  m += (1 - beta1) (g' - m);  v = beta2 v + (1 - beta2) g'^2;
 *   p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps);  ema = decay * ema + (1 - decay) * p.
 * `step` is the 1-based count of this update (Adam's state["step"] after it).  `grad_scale` folds the 1 / world_size of
 * a summing gradient all-reduce into the read of g.  ema may be NULL when do_ema == 0. */
typedef struct GeccoAdamEma {
    float* p; const float* g; float* m; float* v; float* ema;
    size_t n;
    double lr, beta1, beta2, eps, weight_decay;   /* doubles: torch derives 1 - beta, lr / bc1, 1 - decay in double, then rounds */
    double ema_decay;
    float grad_scale;
    int step;
    int do_ema;
} GeccoAdamEma;
int gecco_adam_ema_step_f32(const GeccoAdamEma* a, void* stream);
/* The same step inside torch.amp.GradScaler's protocol for optimizers that handle the scale themselves
 * (`_step_supports_amp_scaling`, torch/amp/grad_scaler.py: the scaler hands over its scale and found_inf tensors instead of
 * unscaling and reading found_inf back on the host — the reference's `precision="16-mixed"` trainer, example_configs): every
 * gradient is divided by *amp_scale while it is read (NULL: already unscaled), and when *found_inf != 0 NOTHING is written
 * (torch skips optimizer.step(), and the EMA update inside it, then) and *skipped is incremented; the bias corrections use
 * step - *skipped, Adam's own step count.  All three are device scalars; the host never waits for the gradients. */
int gecco_adam_ema_step_amp_f32(const GeccoAdamEma* a, const float* amp_scale, const float* found_inf, int* skipped, void* stream);
/* Gradient clipping of the reference's trainer settings inside that step (example_configs/shapenet_airplane_unconditional.py:74-76:
 * gradient_clip_val=1.0, gradient_clip_algorithm="value"; example_configs/taskonomy_conditional.py:102-104: the same with "norm";
 * Lightning runs torch.nn.utils.clip_grad_value_ / clip_grad_norm_ for them, which are the definitions followed here).
 *
 * gecco_grad_norm_f32: the 2-norm of the flat gradient buffer g (n floats, n % 4 == 0, 16-byte aligned) as the TRUE gradients have
 * it, stats[0] = total_norm = sqrt(sum g^2) * |grad_scale| / *amp_scale (amp_scale NULL: 1), and the coefficient
 * clip_grad_norm_ multiplies every gradient by, stats[1] = clip_coef = min(1, max_norm / (total_norm + 1e-6)) in fp32 with torch's
 * operations (reciprocal, times max_norm, clamp); max_norm <= 0: clip_coef = 1.  The squares are accumulated in double, one
 * partial per block in `workspace` (gecco_grad_norm_workspace_bytes(n) bytes, 8-byte aligned, no initialisation needed), added in
 * a fixed order: no floating-point atomics, the same bits on every run; the sum is non-finite exactly when a gradient is, and
 * stats then holds inf / nan (also on a step the GradScaler protocol skips).  Zero pads and the zero gradients of frozen
 * parameters do not change the norm.  Two launches on `stream`, no synchronisation. */
size_t gecco_grad_norm_workspace_bytes(size_t n);
int gecco_grad_norm_f32(const float* g, size_t n, float grad_scale, const float* amp_scale, float max_norm, void* workspace,
                        size_t workspace_bytes, float* stats, void* stream);
/* gecco_adam_ema_step_amp_f32 with the gradient clipped while it is read, BEFORE weight_decay * p is added (torch clips p.grad, Adam
 * adds the decay): algorithm GECCO_CLIP_NORM: g' = (g * grad_scale / *amp_scale) * stats[1], stats as gecco_grad_norm_f32 wrote it
 * earlier on the same stream (clip_val unused); GECCO_CLIP_VALUE: g' = clamp(g * grad_scale / *amp_scale, -clip_val, +clip_val)
 * with torch.clamp's NaN behaviour (a NaN stays a NaN; stats unused, may be NULL), clip_val finite and >= 0.  amp_scale,
 * found_inf and skipped as above, all may be NULL; a skipped step writes nothing. */
#define GECCO_CLIP_NORM 1
#define GECCO_CLIP_VALUE 2
int gecco_adam_ema_step_clip_f32(const GeccoAdamEma* a, int algorithm, float clip_val, const float* stats, const float* amp_scale,
                                 const float* found_inf, int* skipped, void* stream);
/* ema = ema * decay + (1 - decay) * p alone (ema_update, ema.py:187-194), for optimizers other than the fused Adam. */
int gecco_ema_update_f32(const float* p, float* ema, size_t n, double decay, void* stream);

/* ---- samplers and metrics behind the hot path (gecco-torch/README.md:49-52 lists them as absent
 * from the torch package, the JAX package has them) ------------------------------------------------------------------ */

/* Inpainting sampler (gecco-jax models/stochastic.py:101-187): every sub-step re-draws the KNOWN points of the state at
 * the current noise level: x[b, m + j, :] = known[b, j, :] + noise[b, j, :] * sched[step][col]; x (B, m + n_known, 3)
 * fp64, known / noise (B, n_known, 3) fp32 (diffusion space). */
int gecco_sampler_refresh_known_f64(double* x, const float* known, const float* noise, const double* sched, const int* step,
                                    int col, int m, int n_known, int B, void* stream);
/* the same for rows of `width` components: x (B, m + n_known, width), known / noise (B, n_known, width). */
int gecco_sampler_refresh_known_g_f64(double* x, const float* known, const float* noise, const double* sched, const int* step,
                                      int col, int m, int n_known, int width, int B, void* stream);
/* D[b, i, j] = |a[b, i] - b[b, j]| formed as sqrt(max(|a|^2 + |b|^2 - 2 a.b, 0)) (gecco-jax geometry.py:8-24); squared != 0:
 * no square root.  a (B, N, 3), b (B, M, 3), D (B, N, M). */
int gecco_distance_matrix_f32(const float* a, const float* b, float* D, int B, int N, int M, int squared, void* stream);
/* Chamfer distance per sample (gecco-jax metrics.py:92-103): out[b] = (mean_i min_j d(a_i, b_j) + mean_j min_i d) / 2.
 * ws: B * (N + M) floats. */
int gecco_chamfer_f32(const float* a, const float* b, float* out, float* ws, int B, int N, int M, int squared, void* stream);
/* The same forward, which also records the correspondences a gradient needs (gecco-jax metrics.py:92-103: the `jnp.min` over the
 * distance matrix that JAX differentiates through its argmin): ia (B, N) / ib (B, M) int32, for every point the index of its nearest
 * neighbour in the other cloud, the LOWEST index of equal minima (numpy / jnp / torch argmin).  `out` is bit-identical to
 * gecco_chamfer_f32's on the same inputs (same distance formula, tile order and reduction); matrix-free like it.  ws: B * (N + M)
 * floats.  B, N, M >= 1 (B <= 65535), squared 0 / 1. */
int gecco_chamfer_idx_f32(const float* a, const float* b, float* out, float* ws, int* ia, int* ib, int B, int N, int M, int squared,
                          void* stream);
/* Chamfer backward at recorded correspondences (the gradient of metrics.py:92-103 with the argmin held fixed, which is what JAX's
 * `min` rule computes).  With w = gout[b] / 2:
 *   da[b, i] = (w / N) g(a_i, b_{ia[i]}) + (w / M) sum_{j : ib[j] == i} g(a_i, b_j),     db symmetrically,
 * g(p, q) = d/dp d(p, q) taken on the coordinate difference e = p - q, not on the expanded |p|^2 + |q|^2 - 2 p.q: 2 e for
 * squared != 0, e / |e| otherwise, and 0 WHERE |e| == 0: the reference's formula differentiates to NaN there (sqrt'(0) * 0); this
 * library defines the subgradient 0.  Deterministic, no float atomics: the second sum is a gather — every point scans the other
 * cloud's indices (staged through LDS) and adds its matches in index order — so gradients are bit-reproducible run to run.
 * gout (B), da (B, N, 3), db (B, M, 3); da or db (not both) may be null: that gradient is not computed.  An index outside the
 * other cloud is not dereferenced.  B, N, M >= 1 (B <= 65535), squared 0 / 1. */
int gecco_chamfer_bwd_f32(const float* a, const float* b, const int* ia, const int* ib, const float* gout, float* da, float* db, int B,
                          int N, int M, int squared, void* stream);
/* Set-vs-set Chamfer distances (gecco-jax benchmark.py:21-39 `batched_pairwise_distance` with `chamfer_distance` / `_squared`):
 * out (S, T) row-major, out[s, t] = Chamfer(a[s], b[t]) for a (S, N, 3) and b (T, M, 3) — two launches (one per direction), no
 * N x M matrix anywhere.  The minimum is taken over |b|^2 - 2 a.b with |a|^2 added after it (the reference adds it before: equal up
 * to the rounding of that addition). */
int gecco_set_chamfer_f32(const float* a, const float* b, float* out, int S, int T, int N, int M, int squared, void* stream);
/* 1-NN accuracy, minimum matching distance, coverage of a generated set against a reference set of n clouds each (gecco-jax
 * benchmark.py:128-156: `_assemble_dist_m`, `_one_nn_acc`, `_mmd`, `_cov`, reference semantics to the letter incl. the `<= n` of
 * `_one_nn_acc` and numpy's first-of-equals argmin): ss (n, n) sample-sample, sd (n, n) sample-data, dd (n, n) data-data distances;
 * out3 = {1-NNA, MMD, COV}; flags: n ints of scratch. */
int gecco_set_metrics_f32(const float* ss, const float* sd, const float* dd, int n, float* out3, int* flags, void* stream);
/* Entropic optimal transport between uniform marginals on a cost matrix C (B, N, M) (gecco-jax metrics.py:141-156:
 * `sinkhorn_emd` through ott): `iterations` log-domain Sinkhorn sweeps, then out[b] = <P, C> with
 * P_ij = exp((f_i + g_j - C_ij) / epsilon) / (N M).  f (B, N), g (B, M), rowcost (B, N) are caller scratch / outputs. */
int gecco_sinkhorn_f32(const float* C, float* f, float* g, float* rowcost, float* out, int B, int N, int M, float epsilon,
                       int iterations, void* stream);
/* Exact earth mover's distance (gecco-jax metrics.py:114-142: `_scipy_lsa` = scipy's linear_sum_assignment on the distance
 * matrix, then `scipy_emd`'s mean of the `average` distance along the assignment), solved on the device by an epsilon-scaling
 * auction, one workgroup per pair, the whole state in LDS (csrc/emd.hip).  The match cost (squared != 0: l2) is quantised to
 * k = rint(c * 2^GECCO_EMD_Q / c_max), c_max = 2^e with e the frexp exponent of the pair's largest match cost (at least 2^-100),
 * and the integer problem is solved exactly: the assignment's match cost exceeds the optimum of the fp32 costs by at most
 * N * c_max * 2^-GECCO_EMD_Q.  Value and assignment are deterministic (the same bits in any batch position).  Clouds have
 * N == M points, 1 <= N <= GECCO_EMD_MAX_POINTS.  status[p]: 0 solved; 1 a non-finite coordinate (or costs that overflow
 * fp32); 2 more than max_rounds bidding rounds (0: GECCO_EMD_DEFAULT_ROUNDS).  A pair with status != 0 gets NaN and an
 * assignment of -1. */
#define GECCO_EMD_MAX_POINTS 2048
#define GECCO_EMD_Q 24
#define GECCO_EMD_DEFAULT_ROUNDS (1 << 20)
/* B pairs (a[p], b[p]), a and b (B, N, 3): out (B), assign (B, N) int32 (nullable: the column of each row), status (B) int32. */
int gecco_emd_f32(const float* a, const float* b, int B, int N, int match_squared, int average_squared, float* out, int* assign,
                  int* status, int max_rounds, void* stream);
/* EMD backward along an assignment (gecco-jax metrics.py:130-142: `scipy_emd` gathers distance_matrix(...)[rows, cols] along an
 * assignment that comes out of a callback, a constant of the gradient): da[b, i] = (gout[b] / N) g(a_i, b_{cols[i]}),
 * db[b, cols[i]] = -da[b, i], g as in gecco_chamfer_bwd_f32 for the `average` distance (the same rule at distance 0).  cols (B, N)
 * int32 is gecco_emd_f32's `assign`, a permutation: every db row has one writer, no atomics.  A column outside [0, N) is not
 * dereferenced (its da row is 0, no db row is written for it).  da or db (not both) may be null.  B, N >= 1 (B <= 65535). */
int gecco_emd_bwd_f32(const float* a, const float* b, const int* cols, const float* gout, float* da, float* db, int B, int N,
                      int average_squared, void* stream);
/* every pair of a (S, N, 3) set and a (T, N, 3) set in one launch (gecco-jax benchmark.py:21-39 `batched_pairwise_distance`
 * with an exact EMD): out (S, T) row-major, status (S, T) int32; no expanded copies of the clouds. */
int gecco_set_emd_f32(const float* a, const float* b, int S, int T, int N, int match_squared, int average_squared, float* out,
                      int* status, int max_rounds, void* stream);
/* Matrix-free entropic optimal transport between uniform clouds a (B, N, 3), b (B, M, 3) (gecco-jax metrics.py:144-156: `sinkhorn_emd`,
 * ott's Sinkhorn on the squared-Euclidean point-cloud cost), csrc/sinkhorn.hip.  The iteration is gecco_sinkhorn_f32's, with the costs
 * recomputed from the coordinates instead of read from a matrix: C_ij = max(|a_i|^2 + |b_j|^2 - 2 a_i.b_j, 0) (the bits
 * gecco_distance_matrix_f32(squared = 1) writes), g = 0, then `iterations` sweeps f_i = -eps LSE_j((g_j - C_ij) / eps - log M),
 * g_j = -eps LSE_i((f_i - C_ij) / eps - log N); P_ij = exp((f_i + g_j - C_ij) / eps) / (N M); out[b] = sum_ij P_ij C_ij.  The sweep count
 * is fixed and nothing is read back.  form 0: auto (resident when it fits), 1: resident (one workgroup per pair and one launch per solve,
 * clouds and potentials in LDS, N + M <= GECCO_SINKHORN_RESIDENT_MAX_POINTS), 2: streaming (any N, M; 2 * iterations + 2 launches).
 * f (B, N), g (B, M): the potentials on return; ws (B, N): scratch.  The resident form takes null f, g, ws (f and g are written when
 * given); the streaming form needs all three.  Gradient rule: the plan P is a constant of the gradient (gecco_sinkhorn_cloud_bwd_f32).
 * Every reduction has a fixed order, no float atomics: the same bits run to run and in any batch position.  A non-finite coordinate makes
 * its own pair NaN.  The limit: (160 KiB of LDS - 8 KiB of merge scratch - 256 B) / 20 B per point, rounded down to a multiple of 8. */
#define GECCO_SINKHORN_RESIDENT_MAX_POINTS 7768
int gecco_sinkhorn_cloud_f32(const float* a, const float* b, float* f, float* g, float* ws, float* out, int B, int N, int M, float epsilon,
                             int iterations, int form, void* stream);
/* every pair of a (S, N, 3) set and a (T, M, 3) set in one launch of the resident form (gecco-jax benchmark.py:21-39
 * `batched_pairwise_distance` over metrics.py:144-156 `sinkhorn_emd`; BenchmarkCallback uses epsilon = 0.1): out (S, T) row-major,
 * out[s, t] = the value of gecco_sinkhorn_cloud_f32 (same definition, same bits as its resident form) for (a[s], b[t]); no scratch, no
 * expanded copies of the clouds.  N + M <= GECCO_SINKHORN_RESIDENT_MAX_POINTS.  The plan is a constant of the gradient (fixed-plan rule
 * of gecco_sinkhorn_cloud_bwd_f32); fixed-order reductions, no float atomics. */
int gecco_set_sinkhorn_f32(const float* a, const float* b, float* out, int S, int T, int N, int M, float epsilon, int iterations,
                           void* stream);
/* Backward of gecco_sinkhorn_cloud_f32 (gecco-jax metrics.py:144-156) along the FIXED plan P_ij = exp((f_i + g_j - C_ij) / eps) / (N M) of
 * the saved potentials f (B, N), g (B, M) (same definition of C as above): da[b, i] = gout[b] sum_j P_ij 2 (a_i - b_j),
 * db[b, j] = gout[b] sum_i P_ij 2 (b_j - a_i).  The plan is a constant of the gradient, as the exact EMD's assignment is; this is also the
 * envelope gradient of the entropic cost, exact only once the sweeps have converged.  Any N, M (the streaming kernel in gradient mode,
 * one launch per gradient); every row has one writer and a fixed summation order, no float atomics: bit-reproducible.  da or db (not
 * both) may be null.  B, N, M >= 1 (B <= 65535). */
int gecco_sinkhorn_cloud_bwd_f32(const float* a, const float* b, const float* f, const float* g, const float* gout, float* da, float* db,
                                 int B, int N, int M, float epsilon, void* stream);
/* Farthest-point sampling of 3-D clouds (csrc/fps.hip): k of the N points of each cloud of points (B, N, 3), each the point farthest from
 * those chosen before it.  It replaces the random cut the reference's loaders make (gecco-jax data/torch_shapenet.py:20-21 and
 * data/taskonomy.py:84: `randperm[:n_points]`) where a well-spread subset is wanted.  Definition, per cloud, with s_0 = start[b]:
 *     d_i = +inf for all i;  for t = 0 .. k-1:
 *         idx[t] = s_t;  sel2[t] = d_{s_t}    (+inf at t = 0: the squared distance from s_t to the points chosen before it)
 *         d_i = min(d_i, dist2(p_i, p_{s_t})) for all i
 *         s_{t+1} = argmax_i d_i, the LOWEST index among equal maxima
 * dist2(a, b) = (dx*dx + dy*dy) + dz*dz on dx = a.x - b.x, ..., every operation rounded to fp32 and no FMA contraction: the roundings
 * are the definition (runners-up come within 5e-6 relative of a winner), and a numpy float32 restatement gives the same indices.
 * Duplicate points: a chosen point has d = 0; once every d is 0 the lowest index wins again and indices repeat (ten identical points,
 * start 3, k = 4: 3, 0, 0, 0) — documented behaviour, not an error.  NaN coordinates: the selection is unspecified; a candidate enters
 * with `>`, so a NaN never wins, every index stays in [0, N) and the kernels terminate; other clouds of the batch are untouched.
 * start (B) int32 or NULL (= 0 for every cloud); a start outside [0, N) cannot be checked on the host: the kernel clamps it into
 * [0, N).  idx (B, k) int32; sel2 (B, k) fp32 or NULL; every element of both is written.  1 <= k <= N.
 * form 0: auto (resident when it fits), 1: resident (N <= GECCO_FPS_RESIDENT_MAX_POINTS: one workgroup per cloud, one launch for all
 * clouds and steps, coordinates and d in registers, a copy of the coordinates in LDS), 2: streaming (any N: workgroups of
 * GECCO_FPS_STREAM_SLICE points share a cloud, ONE launch per selected point, no workgroup waits on another inside a kernel).
 * ws: GECCO_FPS_WORKSPACE_BYTES(B, N) bytes, 8-byte aligned, = 4 B N (the running d, rounded up to 8) + 16 B ceil(N /
 * GECCO_FPS_STREAM_SLICE) (two buffers of per-workgroup winners); NULL is allowed when the resident form runs.  The workspace is never
 * read before it is written.  The argmax is a maximum of integer keys (d's bits, then ~index): no float atomics, no order to fix, the
 * same bits run to run, in any batch position and in both forms.  Asynchronous on `stream`, no allocation, no synchronisation.
 * The limit: 1024 threads * 8 points in registers (their LDS copy, 16 B per point, is 128 KiB of a CU's 160). */
#define GECCO_FPS_RESIDENT_MAX_POINTS 8192
#define GECCO_FPS_STREAM_SLICE 1024
#define GECCO_FPS_WORKSPACE_BYTES(B, N) \
    ((((size_t)(B) * (size_t)(N) * 4 + 7) & ~(size_t)7) + (size_t)16 * (size_t)(B) * (((size_t)(N) + GECCO_FPS_STREAM_SLICE - 1) / GECCO_FPS_STREAM_SLICE))
int gecco_fps_f32(const float* points, const int* start, int* idx, float* sel2, void* ws, int B, int N, int k, int form, void* stream);
/* k-nearest-neighbour search between 3-D clouds (csrc/knn.hip): for every query q_i (i < M) of query (B, M, 3) the k points p_j (j < N)
 * of ref (B, N, 3), same batch element, that are nearest to it.  The reference has no neighbourhood query; without this entry the only
 * route is an M x N distance matrix and a top-k over it.  Definition:
 *     dist2(q, p) = (dx*dx + dy*dy) + dz*dz    on dx = q.x - p.x, ..., every operation rounded to fp32 and no FMA contraction (the
 *                                              spelling of gecco_fps_f32, NOT pair_dist.h's aa + bb - 2ab, whose cancellation noise
 *                                              reorders near neighbours); a NaN dist2 is replaced by +inf
 *     the pairs of query i are ordered by (dist2, j) ascending: equal distances go to the LOWEST index
 *     idx[i, t], d2[i, t] (t < k) = the first k pairs in that order; d2 is non-decreasing in t
 * exclude_self != 0 (self mode; the query cloud is the reference cloud, M == N required): the pair j == i is skipped by index, not by
 * distance, so exact duplicates of a point remain candidates at distance 0.  Worked examples (a numpy float32 restatement,
 * tests/_knn_ref.py, gives the same): on the 6 x 6 x 6 integer grid (meshgrid(indexing="ij").reshape(-1, 3)) in self mode with k = 7,
 * query 0 gets 1, 6, 36, 7, 37, 42, 43 with d2 = 1, 1, 1, 2, 2, 2, 3 and query 215 gets 179, 209, 214, 173, 178, 208, 172; without self
 * exclusion, k = 4, query 0 gets 0, 1, 6, 36.  Ten identical points, query 3, k = 4: self mode gives 0, 1, 2, 4, all at distance 0;
 * without exclusion 0, 1, 2, 3.  Indices are always in [0, N).  A NaN coordinate affects only the rows and candidates it touches: a NaN
 * reference point is chosen only after every finite one, a NaN query returns 0, 1, ..., k-1 (in self mode the first k indices other than
 * its own) with d2 = +inf, other batch elements are untouched.
 * The order is the order of ONE monotone integer key per pair (dist2's bits above j), so it is total and the split form's merge is
 * exact: the outputs are the same bits run to run, in any batch position and in both forms; no float atomics, and no workgroup ever
 * waits on another.
 * idx (B, M, k) int32 and d2 (B, M, k) fp32 or NULL: every element is written.  query == ref is allowed.
 * 1 <= k <= GECCO_KNN_MAX_K, k <= N (k <= N - 1 in self mode); any M, N >= 1; B clouds with the same M and N.
 * form 1: "direct", one launch, one thread per query, the reference cloud streamed through LDS tiles, the running k-best list of a
 * thread in LDS with its worst key in registers (a candidate no better than it costs one compare).  form 2: "split", for few queries
 * against many points: the reference cloud is cut into slices of GECCO_KNN_SPLIT_SLICE points, a first launch over (query tile x slice)
 * writes each slice's k best keys to ws, a second launch merges the slices of each query; both are ordinary grids.  form 0: auto =
 * split when ws is given, N spans more than one slice and the direct grid (64 queries per workgroup) would leave compute units idle;
 * direct otherwise (a rule fitted to M = 2048, N = 100 000: DESIGN.md).
 * ws: gecco_knn_workspace_bytes(B, M, N, k) = GECCO_KNN_WORKSPACE_BYTES(B, M, N, k) bytes, 8-byte aligned = 8 B M k ceil(N /
 * GECCO_KNN_SPLIT_SLICE); NULL is allowed when the direct form runs (form 0 with NULL runs the direct form).  The workspace is never read
 * before it is written.  Negative return (and gecco_last_error) before anything is enqueued for: null query / ref / idx, non-positive
 * sizes, k out of range, exclude_self with M != N, an unknown form, form 2 without ws.  Asynchronous on `stream`, no allocation, no
 * synchronisation.  gecco_knn_workspace_bytes needs no GPU and returns 0 for non-positive arguments. */
#define GECCO_KNN_MAX_K 64
#define GECCO_KNN_SPLIT_SLICE 4096
#define GECCO_KNN_WORKSPACE_BYTES(B, M, N, k) \
    ((size_t)8 * (size_t)(B) * (size_t)(M) * (size_t)(k) * (((size_t)(N) + GECCO_KNN_SPLIT_SLICE - 1) / GECCO_KNN_SPLIT_SLICE))
int gecco_knn_f32(const float* query, const float* ref, int32_t* idx, float* d2, void* ws, int B, int M, int N, int k, int exclude_self,
                  int form, void* stream);
size_t gecco_knn_workspace_bytes(int B, int M, int N, int k);
/* Surface normals and curvature of 3-D clouds from their k-nearest-neighbour lists (csrc/normals.hip): the PCA normal of every query's
 * neighbourhood and its "surface variation", what PCL and Open3D compute directly after the neighbour search.  The reference has nothing
 * of the kind; without this entry the route is a gathered (B, M, k, 3) tensor, a mean, an einsum and a batched 3 x 3 eigen-solver.
 * ref (B, N, 3) and query (B, M, 3) fp32 (query == ref is allowed); idx (B, M, k) int32 and d2 (B, M, k) fp32 exactly as gecco_knn_f32
 * writes them (searched WITHOUT exclude_self when the queries are the cloud's own points: a point belongs to its own neighbourhood, as
 * in PCL and Open3D).  Definition, for query i:
 *     neighbourhood  the reference points idx[i, t] with d2[i, t] <= radius2, or all k of them when there is no radius (radius2 <= 0,
 *                    +inf or NaN); their number is m, which is what count holds (the hybrid search of Open3D).  d2 == NULL: the
 *                    distances are recomputed from the coordinates with the spelling of gecco_knn_f32, dist2(q, p) = (dx*dx + dy*dy)
 *                    + dz*dz rounded to fp32 with no FMA contraction, NaN -> +inf, so they are the bits the search would have written;
 *                    d2 is not read at all when there is no radius
 *     covariance     mu = sum p / m;  C = sum (p - mu)(p - mu)^T / m: two passes, centred, in fp32 (NOT the raw moments
 *                    E[p p^T] - mu mu^T, which lose every digit on a cloud far from the origin)
 *     eigenpairs     of C, lambda0 <= lambda1 <= lambda2, by 4 cyclic Jacobi sweeps over the entries (0,1), (0,2), (1,2) of C / trace(C):
 *                    a fixed count, never a convergence test.  A rotation whose parameter theta = (a_qq - a_pp) / (2 a_pq) is not
 *                    finite is skipped (a_pq is dropped), one whose square would overflow takes t = 1 / (2 theta).  Negative
 *                    roundings of an eigenvalue are clamped to 0
 *     normal         the unit eigenvector of lambda0;  curvature = lambda0 / (lambda0 + lambda1 + lambda2)
 *     invalid rows   m < 3, or a non-finite coordinate in the query or in a counted neighbour, or trace(C) not a positive finite number
 *                    (0: all counted points are identical), or an index outside [0, N) (never dereferenced, not counted):
 *                    normal = (0, 0, 1) as in Open3D, eigenvalues = 0, curvature = 0; count still holds m.  A collinear neighbourhood
 *                    is valid: its normal is some unit vector of the null space
 *     sign           valid rows only.  viewpoint (B, 3) given: flipped so that n . (viewpoint_b - q_i) >= 0.  viewpoint == NULL: flipped
 *                    so that the component of largest magnitude is positive; among equal magnitudes the lowest axis decides
 * normal (B, M, 3) fp32; eigenvalues (B, M, 3) fp32 ascending, curvature (B, M) fp32 and count (B, M) int32 may each be NULL; every
 * element of a given output is written.  1 <= k <= GECCO_KNN_MAX_K; any B, M, N >= 1.
 * One query's result depends on nothing but its own row of idx and d2 and the points those name: one thread per query, no atomics, no
 * workgroup waits on another; the outputs are the same bits run to run and in any batch position.  Against float64 eigh of the float64
 * covariance of the same fp32 coordinates: |C n - lambda0 n| and every |lambda_t - lambda_t^64| stay within 32 * 2^-24 * trace(C)
 * (tests/test_hip_normals.py).  Negative return (and gecco_last_error) before anything is enqueued for: null ref / query / idx / normal,
 * non-positive sizes, k out of range.  Asynchronous on `stream`, no allocation, no synchronisation. */
int gecco_normals_f32(const float* ref, const float* query, const int32_t* idx, const float* d2, const float* viewpoint, float radius2,
                      float* normal, float* eigenvalues, float* curvature, int32_t* count, int B, int M, int N, int k, void* stream);
/* Rigid registration of 3-D clouds by ICP (csrc/icp.hip), point-to-point (method 0) and point-to-plane (method 1): the transformation
 * that maps source (B, M, 3) onto target (B, N, 3), the consumer PCL and Open3D put behind the neighbour search and the normals.  The
 * reference has nothing of the kind; without this entry the route is gecco_knn_f32 at k = 1, a gather and a batched SVD in a host loop
 * with one synchronisation per iteration.  The definition follows Open3D's registration_icp (tests/_icp_ref.py restates it in numpy).
 * Each cloud of the batch is independent.  Its state T is a 4 x 4 fp64 matrix (row-major), starting at init[b] (NULL: the identity);
 * r2 = fp32(r * r) with the product taken in double; the anchor is c = double(target[0]).  Pass i = 0, 1, ...:
 *     1 transform  Tf = fp32(T);  p'_m = ((Tf[a][0] x + Tf[a][1] y) + Tf[a][2] z) + Tf[a][3] per axis a, every operation rounded to fp32
 *                  and none contracted into an FMA
 *     2 match      (d2_m, j_m) = the first pair of gecco_knn_f32(p', target, k = 1): its dist2 spelling, NaN -> +inf, equal distances to
 *                  the LOWEST index.  Pair m is an inlier when d2_m <= r2 (and d2_m < +inf: a NaN source point is never an inlier); in
 *                  the plane method the three components of normals[j_m] must be finite as well
 *     3 measure    n = the number of inliers;  fitness_i = n / M;  rmse_i = sqrt(sum d2 / n), the sum in fp64, 0 when n = 0
 *     4 stop       at the first of these that holds, with status
 *                    3  init has a non-finite entry (tested at pass 0 only)
 *                    0  i >= 1 and |fitness_i - fitness_{i-1}| < relative_fitness and |rmse_i - rmse_{i-1}| < relative_rmse (absolute
 *                       differences, as in Open3D despite the names)
 *                    1  i == max_iterations
 *                    2  n < 3 (point) or n < 6 (plane), or a singular system (step 5)
 *                  T is left as it is; the outputs are this pass's fitness, rmse and correspondences (j_m for inliers, -1 otherwise)
 *                  and iterations = i
 *     5 update     T <- dT * double(Tf).
 *                  point-to-point: for the inlier pairs P = double(p'), Q = double(q) the centroids and the cross-covariance S from
 *                  moments about c in fp64; Horn's 4 x 4 symmetric matrix of S (scaled by its largest magnitude); its largest
 *                  eigenvector by 8 cyclic Jacobi sweeps over (0,1), (0,2), (0,3), (1,2), (1,3), (2,3) in fp64, a fixed count (a
 *                  rotation whose parameter theta is not finite is skipped, one whose square would overflow takes t = 1 / (2 theta),
 *                  as in gecco_normals_f32); the quaternion normalised with w >= 0; R from it, t = mu_q - R mu_p.  A collinear
 *                  inlier set is valid: it yields some rotation.  A non-finite dT counts as singular
 *                  point-to-plane: res_m = (p'_m - q_m) . n_m,  J_m = [ (p'_m - c) x n_m , n_m ],  A = sum J^T J,  g = sum J res in
 *                  fp64;  A x = -g by LDL^T without pivoting, singular when a pivot is non-finite or <= 2^-36 max diag(A);
 *                  dT = Trans(c) [ Rz(x2) Ry(x1) Rx(x0) | x3..5 ] Trans(-c).  Normals are used as given (not normalised)
 * max_iterations = 0 is Open3D's evaluate_registration: one matching pass under init, status 1, T = init.  A NaN target point is never
 * matched while a finite one exists.  Neither a NaN point nor a NaN init disturbs another cloud.
 * Outputs, every element written: transformation (B, 16) fp64; fitness (B) and inlier_rmse (B) fp32; iterations (B) and status (B)
 * int32; correspondence (B, M) int32 or NULL.  init (B, 16) fp64 or NULL; normals (B, N, 3) fp32, required for method 1 and not read
 * for method 0.  0 <= max_iterations <= GECCO_ICP_MAX_ITERATIONS; r a finite number > 0; the tolerances >= 0.
 * Launches: 2 * (max_iterations + 1), a number that depends on max_iterations alone: per pass a match launch over (cloud x tile of
 * source points x slice of the target) that keeps ONE 64-bit key (dist2's bits above j) per thread and applies Tf on load, and an
 * update launch of one workgroup per cloud that reduces the fp64 sums in a fixed order, solves, tests and writes the state.  A stopped
 * cloud's workgroups return at once.  No atomics, no workgroup waits on another, no synchronisation: the call can be captured in a
 * graph.  form 1: "direct", a thread scans the whole target; form 2: "split", slices of GECCO_KNN_SPLIT_SLICE points, the update takes
 * the minimum of a point's slice keys (exact); form 0: the auto rule of gecco_knn_f32.  The outputs are the same bits run to run, in any
 * batch position and in both forms.
 * ws: gecco_icp_workspace_bytes(B, M, N) = GECCO_ICP_WORKSPACE_BYTES(B, M, N) bytes, 8-byte aligned = GECCO_ICP_STATE_BYTES per cloud
 * (T, the previous pass's fitness and rmse, the stopped flag) + 8 B M ceil(N / GECCO_KNN_SPLIT_SLICE) of keys; required; never read
 * before it is written.  Negative return (and gecco_last_error) before anything is enqueued for: a null source / target / output / ws,
 * method 1 without normals, non-positive sizes, an unknown method or form, max_iterations out of range, r not a finite number > 0, a
 * negative or NaN tolerance.  gecco_icp_workspace_bytes needs no GPU and returns 0 for non-positive arguments. */
#define GECCO_ICP_MAX_ITERATIONS 1000
#define GECCO_ICP_STATE_BYTES 160
#define GECCO_ICP_WORKSPACE_BYTES(B, M, N)           \
    ((size_t)(B) * GECCO_ICP_STATE_BYTES +           \
     (size_t)8 * (size_t)(B) * (size_t)(M) * (((size_t)(N) + GECCO_KNN_SPLIT_SLICE - 1) / GECCO_KNN_SPLIT_SLICE))
int gecco_icp_f32(const float* source, const float* target, const float* normals, const double* init, float r, int method,
                  int max_iterations, double relative_fitness, double relative_rmse, double* transformation, float* fitness,
                  float* inlier_rmse, int32_t* iterations, int32_t* status, int32_t* correspondence, void* ws, int B, int M, int N, int form,
                  void* stream);
size_t gecco_icp_workspace_bytes(int B, int M, int N);
/* Fast Point Feature Histograms (csrc/fpfh.hip; Rusu et al. 2009) in the form Open3D's compute_fpfh_feature and PCL's FPFHEstimation
 * compute: GECCO_FPFH_BINS = 33 numbers per point of points (B, N, 3) from the point's k-neighbourhood and normals (B, N, 3), the
 * descriptor a global registration matches to find the init that gecco_icp_f32 needs.  The reference has nothing of the kind; without
 * this entry the route is a gathered (B, N, k, .) tensor, the pair formulas elementwise, scatter_add histograms (float atomics) and a
 * gather with a weighted mean.  tests/_fpfh_ref.py restates the definition in numpy.
 *     pair feature   for point i and neighbour j, in fp64 on the fp32 inputs, every operation rounded and none contracted into an FMA
 *                    (bin edges make the histogram discontinuous: in fp32 two evaluations disagree on a bin every few thousand pairs)
 *                      1  P1, N1, P2, N2 = double(p_i, n_i, p_j, n_j);  dp = P2 - P1;  d = sqrt((dx dx + dy dy) + dz dz)
 *                      2  d == 0: f = (0, 0, 0)
 *                      3  a1 = ((N1x dpx + N1y dpy) + N1z dpz) / d;  a2 the same with N2
 *                      4  |a1| < |a2|: swap N1 <-> N2, negate dp, f2 = -a2; otherwise f2 = a1 (Open3D's acos(|a1|) > acos(|a2|))
 *                      5  v = dp x N1, each component a difference of two rounded products;  vn = |v| in the spelling of d
 *                      6  vn == 0: f = (0, 0, 0), all three components, as in Open3D
 *                      7  v = v / vn per component;  w = N1 x v;  f1 = v . N2;  f0 = atan2(w . N2, N1 . N2), every dot product
 *                         (x + y) + z
 *                      8  u0 = (11 (f0 + pi)) / (2 pi);  u1 = (11 (f1 + 1)) 0.5;  u2 = (11 (f2 + 1)) 0.5;  b_g = clamp(floor(u_g), 0, 10)
 *                         (a NaN u: bin 0)
 *                      9  the pair adds one count to each of the bins b0, 11 + b1 and 22 + b2
 *                    Normals are used as given (not normalised)
 *     neighbourhood  idx (B, N, k) int32 is the list of gecco_knn_f32(points, points, k) WITHOUT exclude_self, the list
 *                    gecco_normals_f32 uses: one search serves both.  Entry t counts when 0 <= j < N (an index outside is never
 *                    dereferenced);  j != i, by index, so an exact duplicate of the point stays a neighbour and contributes the zero
 *                    triple (bins 5, 16, 27);  with a radius (radius2 > 0 and finite; 0 or +inf: none), dist2(p_i, p_j) <= radius2 in
 *                    the spelling of gecco_knn_f32, recomputed from the coordinates;  and all twelve numbers of p_i, n_i, p_j, n_j are
 *                    finite.  m_i is the number of counted entries: count (B, N)
 *     SPFH           spfh[i, b] = fp32((100.0 count_b) / m_i) in double, a zero row when m_i = 0.  Counts are integers, so this pass
 *                    is exact; each of the three groups of a non-empty row sums to 100
 *     FPFH           over the entries of i's list in list order that were counted above, have dist2 != 0 and m_j > 0:
 *                    w_t = 1 / double(dist2_t);  W = sum w_t;  acc[b] = sum w_t double(spfh[j_t, b]);
 *                    fpfh[i, b] = fp32(double(spfh[i, b]) + (W > 0 ? acc[b] / W : 0)).  Open3D normalises each group of 11 bins by
 *                    100 / sum_group; every non-empty SPFH group sums to 100, so that factor is 1 / W, written directly so that no
 *                    cross-bin reduction order enters the definition.  The point's own SPFH is added unweighted, as in PCL and Open3D
 * Worked examples.  (a) points (0,0,0), (1,0,0), (0,1,0), all normals (0,0,1), k = 3: every pair gives f = (0, 0, 0), u = 5.5, bin 5 of
 * every group; every SPFH row is 100 at bins 5, 16, 27 and every FPFH row 200 there, 0 elsewhere.  (b) points (0,0,0) with normal
 * (0,0,1) and (1,0,0) with normal (0.6, 0, 0.8), k = 2: from point 0, a1 = 0 and a2 = 0.6, so the swap happens, f2 = -0.6, u2 = 2.2,
 * v = (0,1,0), f1 = 0, u1 = 5.5, f0 = atan2(0.6, 0.8), u0 = 6.63; from point 1 no swap and the same triple; both SPFH rows are 100 at
 * bins 6, 16, 24 and both FPFH rows 200 there.
 * Outputs, every element written: fpfh (B, N, 33) fp32; spfh (B, N, 33) fp32 and count (B, N) int32, REQUIRED: they are the first
 * launch's outputs, which the second reads.  1 <= k <= GECCO_KNN_MAX_K, k <= N; any B, N >= 1.
 * Two launches: one thread per point counts into 33 byte counters of its own in LDS; then 33 consecutive threads per point, one per
 * bin, sum the neighbours' rows in list order.  No atomics and no thread waits on another; a row of spfh depends on that point's list
 * and the points and normals it names, a row of fpfh on those and on the spfh rows of the points its list names, nothing else: the
 * same bits run to run and in any batch position, and a non-finite point or normal changes only the rows that reach it this way.
 * Negative return (and gecco_last_error) before anything is enqueued for: a null argument, B or N < 1, k outside 1 ..
 * GECCO_KNN_MAX_K or above N, a negative or NaN radius2, a grid above 2^31 - 1 workgroups.  Asynchronous on `stream`, no allocation,
 * no synchronisation. */
#define GECCO_FPFH_BINS 33
int gecco_fpfh_f32(const float* points, const float* normals, const int32_t* idx, float radius2, float* fpfh, float* spfh, int32_t* count,
                   int B, int N, int k, void* stream);
/* Nearest neighbour in feature space (csrc/fpfh.hip): for every row of a (B, M, C) the nearest row of b (B, N, C), 1 <= C <=
 * GECCO_FEATURE_MAX_DIM, with no M x N matrix (the route without this entry is cdist -> argmin).
 *     d2(i, j) = sum_c (a_ic - b_jc)^2, accumulated from 0 in the order c = 0 .. C - 1, every operation rounded to fp32 and none
 *     contracted into an FMA; a NaN d2 becomes +inf.  The match of row i is the j of the smallest (d2, j): the LOWEST index among
 *     equal distances, one monotone 64-bit key per pair (d2's bits above j), the spelling of gecco_knn_f32.  A query whose every d2 is
 *     +inf (a NaN channel) gets j = 0 and d2 = +inf; a row of b with a NaN channel is never matched while a finite row exists.
 * Zero-filling channels up to a multiple of 4 adds exact zeros and changes no bit: the kernel pads on load to a compile-time width
 * (the smallest of 4, 16, 36, 64 that holds C) and makes no padded copy in memory.  idx (B, M) int32; d2 (B, M) fp32 or NULL.
 * form 1: "direct", one launch, one thread per query, b streamed through LDS; form 2: "split", slices of GECCO_KNN_SPLIT_SLICE rows of
 * b, one key per (query, slice), a second launch takes the minimum (exact); form 0: the auto rule of gecco_knn_f32 (without ws: direct).
 * The same bits run to run, in any batch position and in both forms; no atomics, no thread waits on another.
 * ws: gecco_feature_nn_workspace_bytes(B, M, N) = GECCO_FEATURE_NN_WORKSPACE_BYTES(B, M, N) = 8 B M ceil(N / GECCO_KNN_SPLIT_SLICE)
 * bytes, 8-byte aligned, for the split form; never read before it is written.  Negative return (and gecco_last_error) before anything
 * is enqueued for: a null a / b / idx, B, M or N < 1, C outside 1 .. GECCO_FEATURE_MAX_DIM, an unknown form, the split form without
 * ws, a grid above 2^31 - 1 workgroups.  gecco_feature_nn_workspace_bytes needs no GPU and returns 0 for non-positive arguments. */
#define GECCO_FEATURE_MAX_DIM 64
#define GECCO_FEATURE_NN_WORKSPACE_BYTES(B, M, N) \
    ((size_t)8 * (size_t)(B) * (size_t)(M) * (((size_t)(N) + GECCO_KNN_SPLIT_SLICE - 1) / GECCO_KNN_SPLIT_SLICE))
int gecco_feature_nn_f32(const float* a, const float* b, int32_t* idx, float* d2, void* ws, int B, int M, int N, int C, int form,
                         void* stream);
size_t gecco_feature_nn_workspace_bytes(int B, int M, int N);
/* Global registration by RANSAC on correspondences (csrc/ransac.hip): the pose that gecco_icp_f32 needs as `init`, from the pairs
 * gecco_feature_nn_f32 finds.  It is Open3D's registration_ransac_based_on_correspondence (the core of
 * registration_ransac_based_on_feature_matching) with a fixed number of hypotheses.  The reference has nothing of the kind; without this
 * entry the route is a host loop of randint triples, a batched SVD and an (H, K, 3) tensor per chunk.  tests/_ransac_ref.py restates the
 * definition in numpy.  source (B, M, 3), target (B, N, 3) fp32; corr (B, M) int32, corr[i] the target index matched to source point
 * i or -1 (what the matching returns, mutual or not).  Each cloud is independent and one seed serves every cloud, so a cloud's result
 * does not depend on its batch position.  r2 = fp32(r * r) with the product taken in double, as in gecco_icp_f32.
 *     pairs      the source indices i in ascending order with 0 <= corr[i] < N (an index outside is never dereferenced) and all six
 *                coordinates of p_i and q_corr[i] finite.  K = their number (n_pairs); P_a, Q_a the a-th pair; c = double(Q_0)
 *     draw       for h = 0 .. H - 1, all mod 2^64:
 *                  mix(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
 *                  u_t = mix(seed + (3 h + t + 1) * 0x9E3779B97F4A7C15), t = 0, 1, 2;   draw_t = ((u_t >> 32) * (K - t)) >> 32
 *                  a0 = draw_0;  a1 = draw_1 + (draw_1 >= a0);  lo = min(a0, a1), hi = max(a0, a1)
 *                  a2 = draw_2;  a2 += (a2 >= lo);  a2 += (a2 >= hi)
 *                three distinct indices in [0, K) without a rejection loop
 *     checks     in this order, in fp64 on the fp32 coordinates, every operation rounded and none contracted into an FMA;
 *                |d|^2 = (dx dx + dy dy) + dz dz; no division and no root
 *                  1  degenerate triangle, for X = P and then X = Q: e1 = X_a1 - X_a0, e2 = X_a2 - X_a0, n = e1 x e2 (each component
 *                     a difference of two rounded products); rejected when |n|^2 <= 2^-20 (|e1|^2 |e2|^2); this also catches
 *                     coincident points.  Code 1
 *                  2  edge length (Open3D's CorrespondenceCheckerBasedOnEdgeLength): s2 = edge_similarity^2 in double; every edge
 *                     (a0, a1), (a1, a2), (a2, a0) needs |P_a - P_b|^2 >= s2 |Q_a - Q_b|^2 and |Q_a - Q_b|^2 >= s2 |P_a - P_b|^2;
 *                     edge_similarity = 0 switches it off.  Code 2
 *                  3  fit: Horn's quaternion on the three pairs from the fp64 moments about double(Q_a0) summed in the order a0, a1,
 *                     a2, by the routine of gecco_icp_f32's step 5 (csrc/rigid_fit.h).  A non-finite T: code 4
 *                  4  distance (Open3D's CorrespondenceCheckerBasedOnDistance): under Tf = fp32(T), with gecco_icp_f32's transform
 *                     spelling and gecco_knn_f32's dist2 spelling (p' - q), each of the three pairs needs d2 <= r2.  Code 3
 *                  5  score over all K pairs in pair order: count = the number with d2 <= r2, sum = the fp64 sum of double(d2) over
 *                     those, accumulated SEQUENTIALLY in pair order (so that it can be restated bit for bit given T)
 *                hyp_triple (B, H, 3): the drawn triple;  hyp_count (B, H): count, or -code for a rejected hypothesis;  hyp_sum
 *                (B, H): sum, or +inf for a rejected hypothesis.  K < 3: every hypothesis has triple -1, count -1, sum +inf
 *     candidates (B, H, 16) fp64 or NULL.  Given, T = candidates[b, h] replaces the draw and checks 1 - 3 and check 4 is skipped; a
 *                non-finite entry gets code 4; hyp_triple is -1.  It scores poses of the caller's own (symmetric alternatives)
 *     select     the winner is the surviving hypothesis with count >= 3 that is best under (count descending, then sum ascending,
 *                then h ascending): a total order, so the shape of the reduction cannot change it.  best = its h, or -1
 *     refine     refine_passes times, 0 <= refine_passes <= GECCO_RANSAC_MAX_REFINE: the inliers (d2 <= r2) of the current T among the
 *                K pairs, their fp64 moments about c reduced in a fixed order as in gecco_icp_f32, Horn, T <- dT * double(Tf).  A
 *                pass with fewer than 3 inliers or a non-finite dT leaves T unchanged and ends the refinement.  The refit is ALWAYS
 *                accepted: it is a least-squares polish on the consensus set, not a second search (Open3D leaves refinement to ICP);
 *                a rule "keep only if the count does not fall" would discard the better pose when one borderline pair drops out
 * Outputs, every element written: transformation (B, 16) fp64, the identity when there is no winner; fitness (B) fp32 = n / K with n
 * the number of inliers under the final T (Open3D divides by the number of correspondences), 0 without a winner; inlier_rmse (B) fp32
 * = sqrt(sum / n), 0 when n = 0; n_pairs (B) = K; best (B); status (B): 0 found, 1 no surviving hypothesis with count >= 3, 2 K < 3;
 * inliers (B, M) int32 or NULL: corr[i] for the pairs that are inliers under the final T, -1 elsewhere.  hyp_triple, hyp_count,
 * hyp_sum: NULL or as above.
 * Three launches whatever the data: a compaction of the pairs (one workgroup per cloud, an ordered scan, each pair as two 16-byte
 * entries (P, i), (Q, j)); the hypothesis kernel (a workgroup of 256 threads per 1024 consecutive hypotheses of a cloud: draw and
 * checks 1 - 2 for four hypotheses per thread, the survivors compacted in h order in LDS, then one thread per survivor fits and
 * scores against the pairs streamed through LDS tiles; the workgroup leaves one 16-byte record, its best survivor with count >= 3
 * under the total order); select + refine (one workgroup per cloud, reading one record per GECCO_RANSAC_BLOCK_HYPOTHESES hypotheses).
 * No atomics, no workgroup waits on another, no allocation and no host synchronisation: the call can be captured in a graph.  The
 * outputs are the same bits run to run, in any batch position and however H is split across workgroups.
 * ws: gecco_ransac_workspace_bytes(B, M, hypotheses) = GECCO_RANSAC_WORKSPACE_BYTES(B, M, H) bytes, 16-byte aligned; required; never
 * read before it is written.  Negative return (and gecco_last_error) before anything is enqueued for: a null source / target / corr /
 * required output / ws, non-positive sizes, hypotheses outside 1 .. GECCO_RANSAC_MAX_HYPOTHESES, r not a finite number > 0,
 * edge_similarity outside [0, 1] or NaN, refine_passes out of range, a grid above 2^31 - 1 workgroups.  gecco_ransac_workspace_bytes
 * needs no GPU and returns 0 for arguments out of range. */
#define GECCO_RANSAC_MAX_HYPOTHESES (1 << 24)
#define GECCO_RANSAC_MAX_REFINE 8
#define GECCO_RANSAC_BLOCK_HYPOTHESES 1024
#define GECCO_RANSAC_WORKSPACE_BYTES(B, M, H)                                                                                 \
    ((size_t)32 * (size_t)(B) * (size_t)(M) +                                                                                 \
     (size_t)16 * (size_t)(B) * (((size_t)(H) + GECCO_RANSAC_BLOCK_HYPOTHESES - 1) / GECCO_RANSAC_BLOCK_HYPOTHESES) +     \
     (size_t)16 * (size_t)(B))
int gecco_ransac_f32(const float* source, const float* target, const int32_t* corr, float r, double edge_similarity, int hypotheses,
                     int refine_passes, uint64_t seed, double* transformation, float* fitness, float* inlier_rmse, int32_t* n_pairs,
                     int32_t* best, int32_t* status, int32_t* inliers, int32_t* hyp_triple, int32_t* hyp_count, double* hyp_sum,
                     const double* candidates, void* ws, int B, int M, int N, void* stream);
size_t gecco_ransac_workspace_bytes(int B, int M, int hypotheses);
/* RANSAC plane segmentation (csrc/plane.hip): the dominant plane of each cloud of points (B, N, 3) and the points on it, the step
 * between the filters and gecco_dbscan_f32 (a support plane joins every object standing on it into one cluster).  It is Open3D's
 * segment_plane and PCL's SACSegmentation with SACMODEL_PLANE (with `axis`: SACMODEL_PERPENDICULAR_PLANE) at a fixed number of
 * hypotheses.  The reference has nothing of the kind; without this entry the route is a host loop of randint triples, cross products,
 * an (H, N) distance matrix in chunks, argmax and eigh.  tests/_plane_ref.py restates the definition in numpy.  Each cloud is
 * independent and one seed serves every cloud, so a cloud's result does not depend on its batch position.  r is the distance
 * threshold, an fp32 value.
 *     usable     the indices i in ascending order whose three coordinates are finite and, with mask (B, N) uint8, whose mask[i] != 0.
 *                K = their number (n_points); c0 = double(the first usable point).  Every later step streams the packed list
 *                (x, y, z, bits of i), 16 bytes per point
 *     draw       hypothesis h = 0 .. H - 1 draws three distinct usable points a0, a1, a2 with the generator of gecco_ransac_f32 (its
 *                `draw` paragraph, with K the number of usable points): the same bits for the same seed, h and K
 *     checks     in fp64 on the fp32 coordinates, every operation rounded and none contracted; no division and no root
 *                  1  degenerate triangle: check 1 of gecco_ransac_f32 on the three points.  Code 1
 *                  2  only with axis (B, 3) fp64: n_raw = e1 x e2 (e1 = p_a1 - p_a0, e2 = p_a2 - p_a0, each component a difference
 *                     of two rounded products); rejected when (n_raw . a)^2 < (cos2 |n_raw|^2) |a|^2 with a = axis[b],
 *                     n_raw . a = (n0 a0 + n1 a1) + n2 a2 and cos2 = cos(max_angle)^2, formed in double by the caller: the angle
 *                     between the normal and the axis, either sense, is above max_angle.  Code 2
 *     plane      of a hypothesis: the fp32 pair (nf, cf).  n = n_raw / sqrt(|n_raw|^2) in fp64, nf = fp32(n); c = double(p_a0) and
 *                cf = p_a0 itself: exact, so no d = -n . p cancellation happens on a cloud far from the origin
 *     candidates (B, H, 4) fp64 or NULL.  Given, [a, b, c, d] = candidates[b, h] replaces the draw and check 1: a non-finite entry or
 *                an |abc|^2 that is zero or not finite gets code 4; check 2 applies to n_raw = abc; s = 1 / sqrt(|abc|^2),
 *                n = abc s, c = -(d s) n, nf = fp32(n), cf = fp32(c); hyp_triple is -1
 *     distance   t = ((px - cx) nx + (py - cy) ny) + (pz - cz) nz on (nf, cf), every operation rounded to fp32 and none contracted;
 *                p is an inlier iff |t| <= r, so a NaN is never an inlier
 *     score      count = the number of inliers among the K usable points, sum = the fp64 sum of double(t) double(t) (exact
 *                products) over them, accumulated SEQUENTIALLY in list order (so that it can be restated bit for bit given (nf, cf))
 *                hyp_triple (B, H, 3): the drawn triple;  hyp_plane (B, H, 6) fp32: the (nf, cf) scored, zeros for a rejected
 *                hypothesis;  hyp_count (B, H): count, or -code;  hyp_sum (B, H): sum, or +inf for a rejected hypothesis.  K < 3:
 *                every hypothesis has triple -1, count -1, sum +inf
 *     select     the winner is the hypothesis with code 0 and count >= max(3, min_inliers) that is best under (count descending,
 *                then sum ascending, then h ascending): the total order of gecco_ransac_f32, so neither the shape of the reduction
 *                nor the way the hypotheses fall into workgroups can change it.  best = its h, or -1
 *     refit      refine_passes times, 0 <= refine_passes <= GECCO_PLANE_RANSAC_MAX_REFINE, on the inliers of the current plane
 *                (fp32(n), fp32(c)): the fp64 sums about c0 of 1, t^2, d = double(p) - c0 and the six distinct entries of d d^T
 *                (products rounded, none contracted), each thread over its strided points, the wave by a fixed shuffle tree, the waves
 *                in order.  C = S / n - m m^T with m the mean of d, scaled by its largest magnitude; 8 cyclic Jacobi sweeps over
 *                (0, 1), (0, 2), (1, 2) with the guarded rotation of gecco_icp_f32's step 5; the eigenvector of the smallest
 *                eigenvalue (the lowest index among equals), normalised, is the new n and c0 + m the new c.  A pass with fewer than 3
 *                inliers or a result that is not finite leaves the plane unchanged and ends the refits.  The refit is ALWAYS
 *                accepted, as in gecco_ransac_f32
 *     final      the last evaluation under (fp32(n), fp32(c)) gives inliers (B, N) uint8 (1 for an inlier, 0 elsewhere, unusable
 *                points included), n_inliers, fitness = fp32(n_inliers / K) and inlier_rmse = fp32(sqrt(sum / n_inliers))
 *     plane      (B, 4) fp64 [a, b, c, d]: the unit normal n in fp64 and d = -((a cx + b cy) + c cz) with c the fp64 point above.
 *                Sign, the rule of gecco_normals_f32 in fp64: with viewpoint (B, 3) fp32, n . (v - c) >= 0; without, the component
 *                of largest magnitude is positive, the lowest axis among equal magnitudes
 *     status     0 found;  1 no hypothesis reached the inlier bar: plane = [0, 0, 1, 0], inliers all 0, n_inliers, fitness and rmse
 *                0, best -1;  2 K < 3: the same outputs
 * Every element of every given output is written.  mask, axis, viewpoint, candidates, inliers, hyp_triple, hyp_plane, hyp_count and
 * hyp_sum may each be NULL.  Three launches whatever the data: the compaction (one workgroup per cloud, an ordered scan); the
 * hypothesis kernel (a workgroup of 256 threads per GECCO_PLANE_RANSAC_BLOCK_HYPOTHESES consecutive hypotheses of a cloud: draw and
 * checks for four hypotheses per thread, the survivors compacted in h order in LDS, one thread per survivor scoring against the list
 * streamed through LDS tiles, then the workgroup's own winner under the total order: ONE 16-byte record per workgroup); select + refit
 * (one workgroup per cloud).  No atomics, no workgroup waits on another, no allocation and no host synchronisation: the call can be
 * captured in a graph.  The outputs are the same bits run to run, in any batch position and however H is split across workgroups.
 * ws: gecco_plane_ransac_workspace_bytes(B, N, hypotheses) = GECCO_PLANE_RANSAC_WORKSPACE_BYTES(B, N, H) bytes, 16-byte aligned;
 * required; never read before it is written.  Negative return (and gecco_last_error) before anything is enqueued for: a null points /
 * required output / ws, non-positive sizes, hypotheses outside 1 .. GECCO_PLANE_RANSAC_MAX_HYPOTHESES, r not a finite number > 0,
 * refine_passes out of range, min_inliers < 0, cos2 outside [0, 1] or NaN when axis is given, a grid above 2^31 - 1 workgroups.
 * gecco_plane_ransac_workspace_bytes needs no GPU and returns 0 for arguments out of range. */
#define GECCO_PLANE_RANSAC_MAX_HYPOTHESES (1 << 24)
#define GECCO_PLANE_RANSAC_MAX_REFINE 8
#define GECCO_PLANE_RANSAC_BLOCK_HYPOTHESES 1024
#define GECCO_PLANE_RANSAC_WORKSPACE_BYTES(B, N, H)                                                                           \
    ((size_t)16 * (size_t)(B) * (size_t)(N) +                                                                                 \
     (size_t)16 * (size_t)(B) * (((size_t)(H) + GECCO_PLANE_RANSAC_BLOCK_HYPOTHESES - 1) / GECCO_PLANE_RANSAC_BLOCK_HYPOTHESES) + \
     (size_t)16 * (size_t)(B))
int gecco_plane_ransac_f32(const float* points, const uint8_t* mask, float r, int hypotheses, int refine_passes, uint64_t seed,
                           const double* axis, double cos2, int min_inliers, const float* viewpoint, const double* candidates,
                           double* plane, float* fitness, float* inlier_rmse, int32_t* n_points, int32_t* n_inliers, int32_t* best,
                           int32_t* status, uint8_t* inliers, int32_t* hyp_triple, float* hyp_plane, int32_t* hyp_count, double* hyp_sum,
                           void* ws, int B, int N, void* stream);
size_t gecco_plane_ransac_workspace_bytes(int B, int N, int hypotheses);
/* Voxel-grid downsampling of 3-D clouds (csrc/voxel.hip): one output point per occupied cell of a regular grid of edge voxel_size, at
 * the centroid of the points of points (B, N, 3) that fall in the cell, with the point-to-voxel map.  What PCL and Open3D put before
 * the neighbour search; O(N) and a fixed number of launches whatever the output size.  The reference has nothing of the kind (its
 * loaders cut by `randperm[:n_points]`); without this entry the route is floor -> unique(dim=0) (a sort and a synchronisation) ->
 * index_add (float atomics, not reproducible).  Definition, per cloud, with s = voxel_size (an fp32 value > 0), o = origin[b] (three
 * fp32 values; NULL: 0, a grid anchored at the world origin) and inv = fp32(1 / s), computed once on the host in fp32:
 *     cell      per axis t = fp32(p - o), u = fp32(t * inv), c = floor(u): a subtraction, then a multiplication, nothing to contract.
 *               A point is DROPPED when any u is not finite or any c is outside [-2^20, 2^20): it belongs to no voxel, inverse = -1
 *     key       (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20): 63 bits, so all-ones means "empty"
 *     voxels    the distinct keys of the kept points, numbered in order of FIRST OCCURRENCE: voxel v comes before voxel w when the
 *               lowest point index in v is below the lowest in w.  first[v] = that lowest index, count[v] = the number of points in v,
 *               inverse[i] = the voxel of point i, n_voxels = the number of voxels
 *     centroid  no float sums.  Per axis frac = fp32(u - c) (it can round to 1.0 for a tiny negative u: part of the definition),
 *               q = (uint64) trunc(frac * 2^32), S[v] = the exact integer sum of q over the voxel (64 bits hold any N), and
 *               centroid = fp32( double(o) + (double(c) + double(S) / (double(count) * 2^32)) * double(s) ), every fp64 operation
 *               rounded and none contracted
 *     max_voxels  every output holds max_voxels rows per cloud; rows at or after n_voxels are zero with count = 0 and first = -1;
 *               points of voxels numbered max_voxels or higher get inverse = -1 (their voxels are not written); n_voxels is reported
 *               UNCLAMPED, so a caller sees the overflow.  max_voxels = N can never overflow
 * Worked example (a numpy restatement, tests/_voxel_ref.py, gives the same): s = 1, o = 0, points (.5,.5,.5), (.6,.5,.5), (1.5,.5,.5),
 * (.4,.4,.4), (-.25,.5,.5), (NaN,0,0): inverse = 0, 0, 1, 0, 2, -1; first = 0, 2, 4; count = 3, 1, 1; centroids (0.5, 0.46666667,
 * 0.46666667), (1.5, .5, .5), (-.25, .5, .5).
 * Integer sums do not depend on arrival order and the numbering is a scan over the point index, so the outputs are the same bits run to
 * run, in any batch position and for any launch geometry.  Five launches: fill (table slots and accumulators), insert (one thread per
 * point into the cloud's open-addressing table of the power of two >= 2 N slots of 64-bit keys: compare-and-swap with linear probing
 * from a hash that mixes all three cell fields, a minimum on the slot's first-index word), rank (one workgroup per cloud: an exclusive
 * scan of "this point is its slot's first" over the point index), accumulate (inverse; integer adds on count and S, lanes of a wave
 * that follow each other into the same voxel combined first) and finalise (one thread per output row).  A table at load <= 0.5 always
 * has an empty slot; no thread ever waits on another, no float atomics.
 * centroids (B, max_voxels, 3) fp32 and n_voxels (B) int32 are required; first (B, max_voxels) int32, count (B, max_voxels) int32 and
 * inverse (B, N) int32 may each be NULL; every element of a given output is written, padding included.  workspace:
 * gecco_voxel_workspace_bytes(B, N) = GECCO_VOXEL_WORKSPACE_BYTES(B, N) bytes, 8-byte aligned = 16 B capacity (keys, first-index and
 * voxel-number words of the slots) + 36 B N (S, count, first, the slot of each point) + 4 B, rounded up to 8; every word of it that
 * the call reads was written by the call.  Negative return (and gecco_last_error) before anything is enqueued for: null points /
 * centroids / n_voxels / workspace, B or N < 1, N above GECCO_VOXEL_MAX_POINTS, max_voxels outside 1 .. N, a voxel_size that is not a
 * finite number > 0.  Asynchronous on `stream`, no allocation, no synchronisation.  gecco_voxel_workspace_bytes needs no GPU and
 * returns 0 for arguments out of range. */
#define GECCO_VOXEL_MAX_POINTS (1 << 30)
#define GECCO_VOXEL_SMEAR_(x, k) ((x) | ((x) >> (k)))
#define GECCO_VOXEL_CAPACITY(N) /* the power of two >= 2 N, for 1 <= N <= GECCO_VOXEL_MAX_POINTS */ \
    (GECCO_VOXEL_SMEAR_(GECCO_VOXEL_SMEAR_(GECCO_VOXEL_SMEAR_(GECCO_VOXEL_SMEAR_(GECCO_VOXEL_SMEAR_(2 * (size_t)(N) - 1, 1), 2), 4), 8), 16) + 1)
#define GECCO_VOXEL_WORKSPACE_BYTES(B, N) \
    (((size_t)(B) * (16 * GECCO_VOXEL_CAPACITY(N) + 36 * (size_t)(N) + 4) + 7) & ~(size_t)7)
int gecco_voxel_downsample_f32(const float* points, const float* origin, float voxel_size, float* centroids, int32_t* first, int32_t* count,
                               int32_t* inverse, int32_t* n_voxels, void* workspace, int B, int N, int max_voxels, void* stream);
size_t gecco_voxel_workspace_bytes(int B, int N);
/* DBSCAN clustering of 3-D clouds (csrc/dbscan.hip): the cluster of every point of points (B, N, 3), "which points belong together",
 * the step Open3D (cluster_dbscan), PCL (EuclideanClusterExtraction: the same thing with min_points = 1, every point a core point) and
 * scikit-learn (DBSCAN) put behind the voxel filter and the outlier filter.  The reference has nothing of the kind and this entry
 * replaces nothing in it; without it the route is an N x N adjacency matrix (cdist <= eps: 10 GB of booleans at 100 000 points) and a
 * host loop of masked row minima.  tests/_dbscan_ref.py restates the definition in numpy float32.  Per cloud, with eps2 a finite fp32
 * number > 0 (the caller's fp32(eps * eps), formed once on the host as the radius2 of gecco_normals_f32 is) and min_points >= 1:
 *     dist2(i, j)  (dx dx + dy dy) + dz dz on the coordinate differences, every operation rounded to fp32 and none contracted into an
 *                  FMA, a NaN replaced by +inf: the spelling of gecco_knn_f32.  It is bitwise symmetric in i and j.  A point with a
 *                  non-finite coordinate is nobody's neighbour, not even its own
 *     neighbour    dist2(i, j) <= eps2, the bound INCLUSIVE; a finite point is its own neighbour
 *     core         count_i = the number of neighbours of i (count, (B, N));  i is a core point when count_i >= min_points
 *     clusters     the core points form a graph with an edge wherever two of them are neighbours;  root_i of a core point is the
 *                  lowest index of its connected component;  the cluster id of a component is the rank of its root among all roots,
 *                  ascending: 0 .. C - 1 (n_clusters = C)
 *     border       a non-core point with at least one core neighbour takes the LOWEST cluster id among its core neighbours, which is
 *                  the cluster of the lowest root among them
 *     noise        everything else: label -1
 * This is the labelling of Open3D's cluster_dbscan and scikit-learn's DBSCAN, index for index: both visit the points in index order
 * and finish cluster c before they open c + 1, so clusters are numbered by their lowest core index and a border point keeps the first
 * cluster that reached it.  The result is unique: no order of evaluation enters it.
 * Worked example: points x = 0, 1, 2, 10, 11, 5.5 on a line, eps2 = 1, min_points = 2: counts 2, 3, 2, 2, 2, 1; labels 0, 0, 0, 1,
 * 1, -1.  With min_points = 3 only point 1 is core: labels 0, 0, 0, -1, -1, -1 (points 0 and 2 are border points).
 * 1 + 2 max_rounds + 2 launches whatever the data: count (count_i, the core flag, parent_i = i); max_rounds rounds of hook + compress
 * (Shiloach-Vishkin with minimum hooking on a forest of stars: every core i takes m_i = the minimum parent over its core neighbours
 * and, when m_i < parent_i, does an integer atomicMin of m_i into hook[parent_i]; then every point chases hook from its parent to a
 * fixed point); border + roots; label (one workgroup per cloud, an exclusive prefix count of the roots over the point index).  A round
 * that hooked nothing has found the fixed point: rounds (B) = the number of rounds run, that one included, status (B) = 0, and the
 * cloud's later workgroups return at once.  A cloud whose every round hooked has rounds = max_rounds and status = 1: its labels
 * describe the forest as it stood, a refinement of the true clusters (max_rounds = 0: every core point its own cluster).  ceil(log2 N)
 * + 2 rounds cannot be exceeded: of two joined stars the one with the higher root hooks, so at most ceil(log2 N) rounds change the
 * forest, one more sees no change and one is slack.  In every launch a buffer that is read is written by no thread of that launch
 * (parents and hooks ping-pong; the atomicMin target and the round's flag are written only), so the state after a round is a pure
 * function of the state before it: labels, rounds and status are the same bits run to run and in any batch position, also for a run
 * that hit the limit.  No float atomics, no thread waits on another, no allocation, no host synchronisation: the call can be captured
 * in a graph.
 * labels (B, N), n_clusters (B) and status (B) int32 are required; count (B, N) and rounds (B) int32 may each be NULL; every element of
 * a given output is written.  ws: gecco_dbscan_workspace_bytes(B, N, max_rounds) = GECCO_DBSCAN_WORKSPACE_BYTES(B, N, max_rounds)
 * bytes, 4-byte aligned = 20 B N (two parent buffers, two hook buffers, the roots) + 4 B max_rounds (the round flags), rounded up to
 * 8; required; never read before the call has written it.  Negative return (and gecco_last_error) before anything is enqueued for:
 * null points / labels / n_clusters / status / ws, B or N < 1, an eps2 that is not a finite number > 0, min_points < 1, max_rounds
 * outside 0 .. GECCO_DBSCAN_MAX_ROUNDS, a grid above 2^31 - 1 workgroups.  Asynchronous on `stream`.  gecco_dbscan_workspace_bytes
 * needs no GPU and returns 0 for arguments out of range. */
#define GECCO_DBSCAN_MAX_ROUNDS 64
#define GECCO_DBSCAN_WORKSPACE_BYTES(B, N, R) \
    (((size_t)4 * (size_t)(B) * (5 * (size_t)(N) + (size_t)(R)) + 7) & ~(size_t)7)
int gecco_dbscan_f32(const float* points, int32_t* labels, int32_t* n_clusters, int32_t* count, int32_t* rounds, int32_t* status, void* ws,
                     int B, int N, float eps2, int min_points, int max_rounds, void* stream);
size_t gecco_dbscan_workspace_bytes(int B, int N, int max_rounds);
/* Fixed-radius neighbour search between 3-D clouds (csrc/radius.hip): for every query of query (B, M, 3) EVERY point of ref (B, N, 3)
 * of the same batch element within r of it; the second neighbourhood query of Open3D and PCL beside gecco_knn_f32
 * (search_radius_vector_3d, search_hybrid_vector_3d, remove_radius_outlier / RadiusOutlierRemoval, PointNet++'s ball_query).  The
 * reference has nothing of the kind and these entries replace nothing in it; without them the route is an M x N distance matrix
 * (cdist <= r: 40 GB at 100 000 points against themselves) and nonzero over it, with aa + bb - 2ab roundings that put pairs at the
 * bound on the wrong side.  tests/_radius_ref.py restates the definition in numpy float32.  Per batch element, for queries q_i
 * (i < M) and reference points p_j (j < N), with radius2 a finite fp32 number > 0 (the caller's fp32(r * r), the product taken in
 * double and rounded once: the eps2 of gecco_dbscan_f32):
 *     dist2(q, p)  (dx dx + dy dy) + dz dz on the coordinate differences, every operation rounded to fp32 and none contracted into an
 *                  FMA, a NaN replaced by +inf: the spelling of gecco_knn_f32
 *     neighbour    j is a neighbour of i when dist2(q_i, p_j) <= radius2, the bound INCLUSIVE, compared on the bits as unsigned
 *                  integers (dist2 >= 0 or +inf).  The bound is defined on radius2 and not on r because the two disagree:
 *                  fp32(fp32(sqrt 2)^2) = 1.99999988, so r = fp32(sqrt 2) excludes a pair at dist2 = 2 although sqrt(2) rounds to r
 *     non-finite   a query with a non-finite coordinate has no neighbours; a reference point with one is nobody's neighbour; neither
 *                  disturbs another row or cloud
 *     self mode    exclude_self (M == N, the query cloud is the reference cloud) skips the pair j == i by index, not by distance:
 *                  exact duplicates of a point remain its neighbours
 *     count        count[i] = the number of neighbours of i, never clamped
 *     order        a row lists its neighbours in ascending j
 * Worked example: the 6 x 6 x 6 integer grid (x slowest), self mode, radius2 = 2.25: query 0 gets 1, 6, 7, 36, 37, 42 with dist2 1, 1,
 * 2, 1, 2, 2 (43 lies at dist2 3), query 215 gets 173, 178, 179, 208, 209, 214, an interior point has 18 neighbours, and without
 * exclude_self every count is one higher; radius2 = 1: query 0 gets 1, 6, 36.  Ten identical points, query 3: self mode 0, 1, 2, 4,
 * .., 9 (count 9), without it all ten.
 * gecco_radius_count_f32: count (B, M) int32.  gecco_radius_search_f32 has two forms, one launch each:
 *     CSR          row_start given (int64, B M entries: the exclusive prefix sum of the counts over the rows r = b M + i of the whole
 *                  batch; the total may pass 2^31) and max_neighbors = 0: neighbour t of row r goes to idx[row_start[r] + t] (int32,
 *                  an index into the row's own cloud) and, when d2 is given, its dist2 to d2[row_start[r] + t].  The row is
 *                  recounted by the same predicate on the same bits: exactly count[r] entries are written, nothing else of idx and
 *                  d2 is touched, and count is neither read nor written
 *     fixed width  row_start NULL and max_neighbors = K >= 1: the first K neighbours of row r go to idx[r, 0 .. K) (d2 likewise), the
 *                  remaining slots are padded with -1 (d2: +inf), every element of idx (B, M, K) and d2 (B, M, K) is written, and
 *                  count (B, M), when given, takes the unclamped counts from the same pass.  K is not bounded by N
 * One thread per query, the reference cloud streamed through LDS (the scan of gecco_knn_f32's direct form; there is no split form, so
 * few queries against many points leave compute units idle).  A thread writes its own words only: no atomics, no workspace, no
 * allocation, no host synchronisation (a call can be captured in a graph), and the outputs are the same bits run to run and in any
 * batch position.  ref == query is allowed.  Returns before anything is enqueued (and sets gecco_last_error) with -2 for: null query /
 * ref / count (count form) or query / ref / idx (search form), B, M or N < 1, a radius2 that is not a finite number > 0,
 * exclude_self with M != N, row_start together with max_neighbors != 0 or neither of them (max_neighbors < 1 without row_start); with
 * -3 for a grid above 2^31 - 1 workgroups.  Asynchronous on `stream`. */
int gecco_radius_count_f32(const float* query, const float* ref, int32_t* count, int B, int M, int N, float radius2, int exclude_self,
                           void* stream);
int gecco_radius_search_f32(const float* query, const float* ref, const int64_t* row_start, int32_t* idx, float* d2, int32_t* count, int B,
                            int M, int N, float radius2, int exclude_self, int max_neighbors, void* stream);
/* A uniform-grid index for the fixed-radius search (csrc/grid.hip): the two entries above walk the whole reference cloud for every
 * query; with the cloud sorted into cells of edge cell_size >= r a query tests the points of the cells its ball can reach and no
 * others.  The neighbours, their counts and the bits of dist2 are those of gecco_radius_count_f32 / gecco_radius_search_f32; only the
 * order of a CSR row differs (below).  tests/_grid_ref.py restates the definition in numpy float32.  Per batch element:
 *     cell        that of gecco_voxel_downsample_f32 for voxel_size = cell_size (a finite fp32 number > 0 with a finite fp32(1 /
 *                 cell_size)): per axis t = fp32(p - o), u = fp32(t * inv), c = floor(u), key = (cx + 2^20) << 42 | (cy + 2^20) << 21 |
 *                 (cz + 2^20).  A point that the voxel filter would drop (a non-finite u, a c outside [-2^20, 2^20)) is OFF-GRID: its
 *                 key is 2^63, the sign bit alone (no real key has bit 63).  gecco_grid_keys_f32 writes key (B, N) int64
 *     order       the CALLER sorts every cloud's keys as UNSIGNED integers, stably (a signed sort of key ^ 2^63 is that order): cells
 *                 ascend in key, a cell's points in original index, the off-grid points come last (the tail) in original index.
 *                 perm (B, N) int32: the original index at each sorted position
 *     build       gecco_grid_build_f32, from the sorted keys and perm: sorted (B, N, 4) fp32 = (x, y, z, the bits of perm) per
 *                 position; table_keys (B, cap) int64 and table_range (B, cap, 2) int32 with cap = GECCO_GRID_CAPACITY(N), the power
 *                 of two >= 2 N: an open-addressing table (linear probing from the hash of gecco_voxel_downsample_f32; an empty slot
 *                 holds -1) that maps a key to its run [start, end) of sorted positions (range words of empty slots are not
 *                 written); n_in_grid (B) int32: where the tail starts.  Which slot a key takes may differ from run to run, what a
 *                 lookup finds does not.  Two launches (the table fill and the build); compare-and-swap on the key word, no thread
 *                 waits on another, every probe loop is bounded by cap
 *     query       with R the least fp32 number >= sqrt(radius2 (1 + 2^-23) + 2^-149) (1 + 2^-16), formed in double by the library, a
 *                 query q looks, per axis, at the cells cell(fp32(q - R)) .. cell(fp32(q + R)) (same u and floor, clamped to the
 *                 grid), x outermost and z innermost (ascending key), then at the tail.  A box wider than 4 cells on an axis (never
 *                 where fp32 resolves the coordinates inside a cell) is answered by a scan of all N sorted positions instead.  Among
 *                 those candidates j is a neighbour exactly when gecco_radius_search_f32 says so: dist2(q, p_j) <= radius2 on the
 *                 bits, exclude_self skipping j == i by index.  csrc/grid.hip proves that no neighbour lies outside the box
 *     rows        gecco_grid_radius_search_f32 is the CSR form of gecco_radius_search_f32 (row_start required, no max_neighbors):
 *                 a row lists its neighbours in ascending SORTED POSITION, that is by (key, j) with the tail last; sort a row by j
 *                 for the order of gecco_radius_search_f32
 *     qorder      (B, M) int32 or NULL: thread t answers query qorder[b, t] and writes that query's row, so that neighbouring threads
 *                 read the same cells.  A permutation of 0 .. M - 1 per cloud (perm itself in self mode); entries outside 0 .. M - 1
 *                 are skipped, their rows are not written
 * Worked example: the 6 x 6 x 6 integer grid (x slowest) of the radius block, cell_size 1.5, origin 0: coordinates {0, 1 | 2 | 3, 4 | 5}
 * share a cell per axis, 64 cells.  Self mode, radius2 = 2.25: query 0 gets 1, 6, 7, 36, 37, 42, all six in its own cell (0, 0, 0), so
 * the row is also ascending in j; query 43 = (1, 1, 1) has 18 neighbours in 7 cells and its row is 1, 6, 7, 36, 37, 42 (cell (0, 0,
 * 0)), 8, 38, 44 (cell (0, 0, 1)), 13, 48, 49 (cell (0, 1, 0)), 50, then 73, 78, 79, 80, 85 from the cells with cx = 1: by cell
 * first, by j inside a cell.
 * Every entry is asynchronous on `stream`, allocates nothing and does not synchronise; the query writes with no atomics and no
 * workspace, the same bits run to run and in any batch position.  origin (B, 3) may be NULL (zeros); d2 may be NULL.  Return -2 before
 * anything is enqueued (and gecco_last_error) for: a null required pointer, B, M or N < 1, N above GECCO_VOXEL_MAX_POINTS, a cell_size
 * that is not a finite number > 0 with a finite reciprocal, a radius2 that is not a finite number > 0 or is above fp32(cell_size *
 * cell_size) (build an index with a larger cell), exclude_self with M != N; -3 for a grid above 2^31 - 1 workgroups. */
#define GECCO_GRID_CAPACITY(N) GECCO_VOXEL_CAPACITY(N)
int gecco_grid_keys_f32(const float* points, const float* origin, float cell_size, int64_t* keys, int B, int N, void* stream);
int gecco_grid_build_f32(const float* points, const int64_t* sorted_keys, const int32_t* perm, float* sorted, int64_t* table_keys,
                         int32_t* table_range, int32_t* n_in_grid, int B, int N, void* stream);
int gecco_grid_radius_count_f32(const float* query, const int32_t* qorder, const float* sorted, const int64_t* table_keys,
                                const int32_t* table_range, const int32_t* n_in_grid, const float* origin, float cell_size, int32_t* count,
                                int B, int M, int N, float radius2, int exclude_self, void* stream);
int gecco_grid_radius_search_f32(const float* query, const int32_t* qorder, const float* sorted, const int64_t* table_keys,
                                 const int32_t* table_range, const int32_t* n_in_grid, const float* origin, float cell_size,
                                 const int64_t* row_start, int32_t* idx, float* d2, int B, int M, int N, float radius2, int exclude_self,
                                 void* stream);
/* ISS keypoints (Intrinsic Shape Signatures, Zhong 2009; Open3D's compute_iss_keypoints, PCL's ISSKeypoint3D) on the grid index above
 * (csrc/iss.hip): the points whose neighbourhood is not flat, not a line and not isotropic, thinned by non-maximum suppression.  The
 * cloud is the one the index was built over; sorted, table_keys, table_range, n_in_grid, origin and cell_size are that index.
 * tests/_iss_ref.py restates the definition in numpy.  Per batch element, with r2s = salient_radius2 = fp32(salient_radius^2) and
 * r2n = non_max_radius2 = fp32(non_max_radius^2) from the caller:
 *     ball        B_r(i) = the j with dist2(p_i, p_j) <= r2 on the bits, gecco_radius_count_f32's predicate, the point itself INCLUDED
 *                 by index (Open3D's radius search returns the query).  A non-finite point is in nobody's ball, not even its own.  The
 *                 ball is visited in ascending sorted position of the index (by (cell key, j), the off-grid tail last), the order of
 *                 a row of gecco_grid_radius_search_f32: that order is part of the definition
 *     count       m_i = |B_r2s(i)|
 *     moments     in fp64 on the fp32 coordinates, about the point itself, every operation rounded and none contracted:
 *                 d = double(p_j) - double(p_i) per axis;  S1 = sum d (3 sums), S2 = sum d d^T (xx, xy, xz, yy, yz, zz), each from 0
 *                 in ball order;  inv = 1 / m;  mu = S1 inv;  C_ab = S2_ab inv - mu_a mu_b.  |d| <= the radius, so the raw moments
 *                 cancel against the radius and not against the cloud's distance from the origin
 *     eigen       big = max |C_ab|;  A = C sc with sc = 1 / big;  8 cyclic Jacobi sweeps over (0,1), (0,2), (1,2) with the guarded
 *                 rotation of gecco_icp_f32 (a non-finite theta gives t = 0, a theta whose square would overflow t = 1 / (2 theta)),
 *                 a fixed count, none of its operations contracted;  lambda = diag big, negative roundings clamped to 0, sorted
 *                 lambda0 <= lambda1 <= lambda2
 *     candidate   m_i >= min_neighbors, big a positive finite number (all of the ball identical: not a candidate, Open3D's
 *                 cov.isZero()), lambda1 < gamma_21 lambda2, lambda0 < gamma_32 lambda1 (fp64 products, no division) and
 *                 lambda0 > 0.  saliency_i = lambda0 for a candidate, 0 otherwise;  eigenvalues_i = 0 where m_i < min_neighbors or
 *                 big is not a positive finite number
 *     keypoint    i is a candidate, |B_r2n(i)| >= min_neighbors, and no j in B_r2n(i) has saliency_j > saliency_i (fp64 compare).
 *                 Equal saliencies keep each other, as Open3D's IsLocalMaxima does: two exact duplicates of a keypoint are both kept
 * Outputs, at the ORIGINAL index of a point: saliency (B, N) fp64, eigenvalues (B, N, 3) fp64 ascending (may be NULL), counts (B, N)
 * int32 = m_i (may be NULL), mask (B, N) one byte per point, 1 for a keypoint and 0 otherwise.  A point's result depends on the cloud
 * and on the index's cell_size and origin, which fix the order of the sums, and on nothing else: the same bits run to run, in any
 * batch position and at any workgroup size.  Two indices with different cells may differ in the last bits of the eigenvalues.
 * Worked example: the 6 x 6 x 6 integer grid (x slowest) of the radius block, cell_size 1.5, origin 0, both radii 1.5 (radius2 2.25),
 * gammas 0.975, min_neighbors 5.  Point 0, a corner: m = 7, S1 = (3, 3, 3), S2 = 3 on the diagonal and 1 off it, C = 12/49 on the
 * diagonal and -2/49 off it, lambda = (8/49, 2/7, 2/7): lambda1 = lambda2, not a candidate.  Point 1 = (0, 0, 1), on an edge: m = 10,
 * lambda = (0.18, 0.3, 0.6), saliency 0.18.  Point 7 = (0, 1, 1), on a face: m = 14, lambda1 = lambda2 = 4/7; point 43 = (1, 1, 1): m =
 * 19, lambda = 10/19 three times.  The candidates are the 48 points inside the 12 edges, all with saliency 0.18 up to rounding in
 * the last place; every one is a keypoint (a non-maximum ball holds 10 points and no larger saliency), and nothing else is.
 * Two launches, one thread per sorted position in both: the saliency of every point (a walk over the cells its ball can reach, the one walk of
 * csrc/grid_walk.h that gecco_grid_radius_count_f32 / _search_f32 make as well, the count and the nine sums in registers, the 3 x 3 problem in registers), then the selection (the same walk at r2n, a gather of
 * saliency by index).  A thread writes its own words only: no atomics, no workspace, no allocation, no synchronisation, asynchronous
 * on `stream`.  Return -2 before anything is enqueued (and gecco_last_error) for: a null required pointer, B or N < 1, N above
 * GECCO_VOXEL_MAX_POINTS, a cell_size that is not a finite number > 0 with a finite reciprocal, a radius2 that is not a finite
 * number > 0 or is above fp32(cell_size * cell_size) (build an index with a larger cell), a gamma that is not a finite number > 0,
 * min_neighbors < 1; -3 for a grid above 2^31 - 1 workgroups. */
int gecco_iss_keypoints_f32(const float* sorted, const int64_t* table_keys, const int32_t* table_range, const int32_t* n_in_grid,
                            const float* origin, float cell_size, double* saliency, double* eigenvalues, int32_t* counts, uint8_t* mask, int B,
                            int N, float salient_radius2, float non_max_radius2, double gamma_21, double gamma_32, int min_neighbors,
                            void* stream);
/* Normals and curvature from RADIUS neighbourhoods on the grid index above (csrc/normals_grid.hip): Open3D's estimate_normals(
 * KDTreeSearchParamRadius(r)), PCL's NormalEstimation::setRadiusSearch, every point within r and no cap (gecco_normals_f32 reads the
 * k <= GECCO_KNN_MAX_K neighbours of the brute-force search).  sorted, table_keys, table_range, n_in_grid, origin and cell_size are the
 * index of the cloud; query (B, M, 3) and qorder are gecco_grid_radius_count_f32's.  tests/_normals_grid_ref.py restates the definition
 * in numpy.  Per batch element, with r2 = radius2 = fp32(radius^2) from the caller:
 *     queries     q_i: the points of the cloud themselves (query = the cloud, M = N) or other positions.  A point of the cloud is in its
 *                 own ball because its dist2 is 0: nothing is excluded by index
 *     ball        the j with dist2(q_i, p_j) <= r2 on the bits, gecco_radius_count_f32's predicate, visited in ascending sorted position
 *                 of the index (by (cell key, j), the off-grid tail last): that order is part of the definition, as it is for ISS.  A
 *                 non-finite query has an empty ball; a non-finite point is in nobody's ball
 *     count       m_i = the size of the ball, never clamped
 *     moments,    exactly the `moments` and `eigen` steps of gecco_iss_keypoints_f32 above, about the query: fp64 sums of d =
 *     eigen       double(p_j) - double(q_i) in ball order, C = S2 / m - mu mu^T, big = max |C_ab|, A = C / big, 8 cyclic Jacobi sweeps over
 *                 (0,1), (0,2), (1,2) with the guarded rotation, nothing contracted, lambda = diag big clamped at 0.  The same rotations
 *                 are accumulated into V, which starts as the identity: the columns p, q of V rotate as the rows and columns of A do
 *                 (v_rp' = c v_rp - s v_rq, v_rq' = s v_rp + c v_rq)
 *     order       the three (lambda, column) pairs sorted ascending by the three compare-exchanges (0,1), (1,2), (0,1) that ISS uses on
 *                 its eigenvalues; a pair moves only when strictly smaller, so equal eigenvalues keep their column order
 *     normal      the column of lambda0 divided by its fp64 norm sqrt((xx + yy) + zz), each component rounded once to fp32
 *     sign        applied after the rounding, so it can be checked exactly on the output.  With a viewpoint v (B, 3): flip when
 *                 (n_x d_x + n_y d_y) + n_z d_z < 0 in fp64, d = double(v) - double(q_i); a NaN does not flip.  Without (NULL): the fp32
 *                 component of largest magnitude is positive, the lowest axis among equal magnitudes (gecco_normals_f32's rule)
 *     curvature   lambda0 / ((lambda0 + lambda1) + lambda2) in fp64, 0 where that sum is not > 0
 *     invalid     m_i < min_neighbors, a non-finite query, big not a positive finite number (all of the ball identical): normal
 *                 (0, 0, 1) as in Open3D, eigenvalues 0, curvature 0, count still m_i.  A collinear ball is valid: its normal is some
 *                 unit vector of the numerical null space
 * Outputs, at the row of the query: normals (B, M, 3) fp32, eigenvalues (B, M, 3) fp64 ascending (may be NULL), curvature (B, M) fp64
 * (may be NULL), counts (B, M) int32 = m_i (may be NULL).  A row depends on the cloud, the query and the index's cell_size and origin,
 * which fix the order of the sums, and on nothing else: the same bits run to run, in any batch position and at any workgroup size.
 * Worked example: the 6 x 6 x 6 integer grid (x slowest) of the radius block, cell_size 1.5, origin 0, radius2 2.25, the cloud its own
 * queries.  Point 0, a corner: m = 7, lambda = (8/49, 2/7, 2/7), normal (1, 1, 1) / sqrt(3), curvature 2/9.  Point 7 = (0, 1, 1), on a
 * face: m = 14, lambda = (45/196, 4/7, 4/7), normal (1, 0, 0), curvature 45/269.
 * One launch, one thread per query (thread t answers query qorder[b, t]; NULL: query t): the walk of csrc/grid_walk.h, the count and
 * the nine sums in registers, the solve of csrc/sym3_jacobi.h that gecco_iss_keypoints_f32 runs without the vectors.  A thread writes
 * its own words only: no atomics, no workspace, no allocation, no synchronisation, asynchronous on `stream`.  Return -2 before anything
 * is enqueued (and gecco_last_error) for: a null required pointer, B, M or N < 1, N above GECCO_VOXEL_MAX_POINTS, a cell_size that is
 * not a finite number > 0 with a finite reciprocal, a radius2 that is not a finite number > 0 or is above fp32(cell_size * cell_size)
 * (build an index with a larger cell), min_neighbors < 1; -3 for a grid above 2^31 - 1 workgroups. */
int gecco_normals_grid_f32(const float* query, const int32_t* qorder, const float* sorted, const int64_t* table_keys,
                           const int32_t* table_range, const int32_t* n_in_grid, const float* origin, float cell_size, const float* viewpoint,
                           float radius2, int min_neighbors, float* normals, double* eigenvalues, double* curvature, int32_t* counts, int B,
                           int M, int N, void* stream);
/* Fast Point Feature Histograms from RADIUS neighbourhoods on the grid index above (csrc/fpfh_grid.hip): Open3D's compute_fpfh_feature(
 * KDTreeSearchParamRadius(r)), PCL's FPFHEstimation::setRadiusSearch, every point within r and no cap, the ball gecco_normals_grid_f32
 * fits its normals to (gecco_fpfh_f32 reads the k <= GECCO_KNN_MAX_K neighbours of the brute-force search and counts into bytes).  The
 * cloud is the one the index was built over; sorted, table_keys, table_range, n_in_grid, origin and cell_size are that index, as
 * gecco_iss_keypoints_f32 takes it; normals (B, N, 3) are indexed as the cloud was.  tests/_fpfh_grid_ref.py restates the definition in
 * numpy.  Per batch element, with r2 = radius2 = fp32(radius^2) from the caller:
 *     ball           of point i: the j with dist2(p_i, p_j) <= r2 on the bits, gecco_radius_count_f32's predicate, visited in ascending
 *                    sorted position of the index (by (cell key, j), the off-grid tail last): that order is part of the definition, as
 *                    it is for ISS and gecco_normals_grid_f32.  A non-finite p_i has an empty ball; a non-finite p_j is in nobody's ball
 *     counted        a member of the ball with j != i BY INDEX (an exact duplicate of the point stays a neighbour and contributes the
 *     neighbour      zero triple, bins 5, 16, 27, as in gecco_fpfh_f32) and all six numbers of n_i and n_j finite.  m_i = the number
 *                    of counted neighbours, never clamped: it may exceed 64 and 255
 *     pair feature   steps 1 - 9 of gecco_fpfh_f32's definition above, by the same code (csrc/fpfh_pair.h)
 *     SPFH           spfh[i, b] = fp32((100.0 * count_b) / m_i) in double, 32-bit integer counts; a zero row when m_i = 0
 *     FPFH           over the counted neighbours in ball order that have dist2 != 0 and m_j > 0: w = 1 / double(dist2), dist2 the
 *                    value the walk tested; W = sum w and acc[b] = sum w * double(spfh[j, b]), each sum one rounded fp64 operation
 *                    per term, nothing contracted; fpfh[i, b] = fp32(double(spfh[i, b]) + (W > 0 ? acc[b] / W : 0))
 * Outputs, every element written: fpfh (B, N, 33) fp32; spfh (B, N, 33) fp32 and count (B, N) int32 = m_i, REQUIRED: they are the first
 * launch's outputs and the second launch's inputs; there is no other workspace.  count and spfh do not depend on the index's cell_size
 * or origin (integer counts, one rounding).  fpfh has the same bits run to run, in any batch position and at any workgroup size; with
 * another cell_size or origin, which change the ball order, it may differ in the last fp32 place only.  The worked examples of
 * gecco_fpfh_f32 hold at any radius that contains them (radius2 = 4, cell_size 2).
 * Two launches, one thread per sorted position (thread t owns the point at sorted[b, t] and writes row perm = the bits of its .w; a
 * perm outside [0, N) writes nothing): the walk of csrc/grid_walk.h twice, first counting into 33 32-bit counters of the thread's own
 * in LDS, then summing into 33 fp64 accumulators in registers.  No atomics, no allocation, no synchronisation, asynchronous on
 * `stream`.  Return -2 before anything is enqueued (and gecco_last_error) for: a null pointer other than origin, B or N < 1, N above
 * GECCO_VOXEL_MAX_POINTS, a cell_size that is not a finite number > 0 with a finite reciprocal, a radius2 that is not a finite number
 * > 0 or is above fp32(cell_size * cell_size) (build an index with a larger cell); -3 for a grid above 2^31 - 1 workgroups. */
int gecco_fpfh_grid_f32(const float* normals, const float* sorted, const int64_t* table_keys, const int32_t* table_range,
                        const int32_t* n_in_grid, const float* origin, float cell_size, float radius2, float* fpfh, float* spfh, int32_t* count,
                        int B, int N, void* stream);
/* DBSCAN clustering on the grid index above (csrc/dbscan.hip, the grid form): gecco_dbscan_f32 with its three scans of the whole cloud
 * (count, hook, border) replaced by walks over the cells a ball of eps can reach.  The cloud is the one the index was built over;
 * sorted, table_keys, table_range, n_in_grid, origin and cell_size are that index, as gecco_iss_keypoints_f32 takes it.
 * The DEFINITION is gecco_dbscan_f32's, word for word: the cells only filter, j is a neighbour of i iff dist2(i, j) <= eps2 on the
 * bits, and nothing else.  labels, n_clusters, count, rounds and status are the direct form's bit for bit, through any index whose
 * cell_size serves eps2 (any origin, any cell), also rounds and the labels of a run stopped by max_rounds: a minimum of integers depends
 * neither on arrival order nor on the order in which a thread meets its neighbours, so the state after a round is the same function
 * of the state before it in both forms.  The same bits run to run, in any batch position and at any workgroup size.
 * 2 + 2 max_rounds + 2 launches whatever the data: init (in index order: no parent, hook_i = i, no root, count 0, the round flags
 * cleared), count, max_rounds rounds of hook + compress, border, label.  The walks are one thread per sorted position (the one walk of
 * csrc/grid_walk.h); every workspace array stays indexed by the original point index, compress and label are gecco_dbscan_f32's own
 * kernels, and a neighbour's parent is a 4-byte gather for the entries inside the ball.  Memory safety does not depend on the index's
 * contents: the original index in sorted[.].w is checked against N before it addresses anything and the init launch writes every word a
 * later kernel reads, so a `sorted` that is no permutation gives meaningless labels and no access outside the buffers.
 * Outputs and workspace are gecco_dbscan_f32's: labels (B, N), n_clusters (B), status (B) int32 required, count (B, N) and rounds (B)
 * may each be NULL, every element of a given output is written; ws of GECCO_DBSCAN_WORKSPACE_BYTES(B, N, max_rounds) bytes, carved the
 * same way, never read before the call has written it; origin may be NULL (zeros).  No float atomics (the integer atomicMin of the
 * hook pass only), no allocation, no host synchronisation, asynchronous on `stream`: the call can be captured in a graph.
 * Return -2 before anything is enqueued (and gecco_last_error) for: a null required pointer, B or N < 1, N above
 * GECCO_VOXEL_MAX_POINTS, an eps2 that is not a finite number > 0, a cell_size that is not a finite number > 0 with a finite
 * reciprocal, an eps2 above fp32(cell_size * cell_size) (build an index with a larger cell), min_points < 1, max_rounds outside 0 ..
 * GECCO_DBSCAN_MAX_ROUNDS; -3 for a grid above 2^31 - 1 workgroups. */
int gecco_dbscan_grid_f32(const float* sorted, const int64_t* table_keys, const int32_t* table_range, const int32_t* n_in_grid,
                          const float* origin, float cell_size, int32_t* labels, int32_t* n_clusters, int32_t* count, int32_t* rounds,
                          int32_t* status, void* ws, int B, int N, float eps2, int min_points, int max_rounds, void* stream);

/* ---- ConvNeXt conditioner, channels-last on the device (ConvNeXtExtractor, models/feature_pyramid.py:28-73,
 * = torchvision's ConvNeXt stages).  Activations are (B, H, W, C) fp32.  The pointwise linears of a CNBlock run through
 * gecco_linear_ex_f32 on rows = B H W (act = 4: exact-erf GELU; the second one with the block input as residual and
 * layer_scale folded into its weights by gecco_convnext_fold_scale_f32); these are the rest of a block. */
/* stem: out = LayerNorm_C(Conv2d(3 -> C, k4, s4)(x) + bias); x NCHW (B, 3, H, W), w (C, 3, 4, 4), out (B, H/4, W/4, C); C == 96.
 * H, W >= 4, any residue mod 4: H/4, W/4 floor like Conv2d (the last H % 4 rows and W % 4 columns are not read). */
int gecco_convnext_stem_f32(const float* x, const float* w, const float* bias, const float* ln_w, const float* ln_b, float* out,
                            int B, int H, int W, int C, float eps, void* stream);
/* CNBlock front half: out = LayerNorm_C(dwconv7x7(x, padding 3) + bias); w TAP-MAJOR (49, C) = the module's weight
 * (C, 1, 7, 7) reshaped to (C, 49) and transposed (a re-layout of 19 .. 75 KB of parameters, like the 2 x 2 downsample
 * weight's); C in {96, 192, 384, 768}; any H, W */
int gecco_convnext_dwconv_ln_f32(const float* x, const float* w, const float* bias, const float* ln_w, const float* ln_b, float* out,
                                 int B, int H, int W, int C, float eps, void* stream);
/* downsample front half: LayerNorm_C per texel, written as the 2 x 2 stride-2 conv's GEMM operand (B, H/2, W/2, (dy, dx, c)).
 * H, W >= 2; an odd H or W floors like the strided Conv2d: the last row / column of the map is neither read nor written. */
int gecco_convnext_ln_patch2_f32(const float* x, const float* ln_w, const float* ln_b, float* out, int B, int H, int W, int C,
                                 float eps, void* stream);
/* Wo[n, k] = s[n] W[n, k], bo[n] = s[n] b[n] (CNBlock.layer_scale folded into its second linear) */
int gecco_convnext_fold_scale_f32(const float* W, const float* b, const float* s, float* Wo, float* bo, int N, int K, void* stream);

/* ---- the conditioner's TRAINING path.  The reference trains ConvNeXtExtractor with the denoiser (it is a sub-module of
 * Diffusion: diffusion.py:203-222 optimises self.parameters(); feature_pyramid.py:55-59 only removes stochastic depth), so
 * the pyramid gradient of gecco_ray_lookup_bwd_f32 continues through these.  The pointwise linears' dX / dW / db are the
 * GEMM entries of the denoiser's training path (gecco_linear_ex_f32 on W^T, gecco_gemm_tn_x3_bias_f32, gecco_gemm_f32). */
/* the two forward entries above that also keep z, the LayerNorm's input (same shape as out) */
int gecco_convnext_stem_train_f32(const float* x, const float* w, const float* bias, const float* ln_w, const float* ln_b, float* out,
                                  float* z, int B, int H, int W, int C, float eps, void* stream);
int gecco_convnext_dwconv_ln_train_f32(const float* x, const float* w, const float* bias, const float* ln_w, const float* ln_b,
                                       float* out, float* z, int B, int H, int W, int C, float eps, void* stream);
/* out = dwconv7x7(x, padding 3) (+ bias when non-null), w tap-major (49, C).  With the taps reversed (w[48 - tap]) and dz as
 * x this is the depthwise convolution's input gradient. */
int gecco_convnext_dwconv_f32(const float* x, const float* w, const float* bias, float* out, int B, int H, int W, int C, void* stream);
/* the depthwise convolution's input gradient in one launch: dx = dwconv7x7(dz, taps reversed) (+ add: the gradient that reached
 * the block input through its skip connection); w is the FORWARD tap-major weight (the kernel stages it reversed) */
int gecco_convnext_dwconv_bwd_f32(const float* dz, const float* w, const float* add, float* dx, int B, int H, int W, int C, void* stream);
/* backward of gecco_convnext_fold_scale_f32: dW = s dW', db = s db', ds[n] = sum_k dW'[n, k] W[n, k] + db'[n] b[n] */
int gecco_convnext_fold_scale_bwd_f32(const float* dWp, const float* dbp, const float* W, const float* b, const float* s, float* dW,
                                      float* db, float* ds, int N, int K, void* stream);
/* LayerNorm_C backward per texel from its input z (B, H, W, C) (statistics recomputed): dz, and per-block column partials
 * parts (gecco_convnext_ln_bwd_blocks(B, H, W, C), 3, C) = [d ln_w | d ln_b | column sums of dz] (the last is the bias
 * gradient of the convolution that produced z); reduce with gecco_reduce_batch_f32.  patch2 != 0: dy is laid out as the
 * downsample GEMM's operand (B, H/2, W/2, (dy, dx, c)) — the backward of gecco_convnext_ln_patch2_f32; the last row / column
 * of an odd map is in no patch: its dz is 0 and dy is not read there.  C in {96, 192, 384, 768}. */
int gecco_convnext_ln_bwd_blocks(int B, int H, int W, int C);
int gecco_convnext_ln_bwd_f32(const float* z, const float* dy, const float* ln_w, float* dz, float* parts, int B, int H, int W, int C,
                              float eps, int patch2, void* stream);
/* depthwise 7 x 7 weight gradient, tap-major: parts (gecco_convnext_dwconv_dw_blocks(B, H, W, C), 49, C) per-block partials of
 * dW[tap][c] = sum_texels dz[b, y, x, c] x[b, y + dy - 3, x + dx - 3, c] */
int gecco_convnext_dwconv_dw_blocks(int B, int H, int W, int C);
int gecco_convnext_dwconv_dw_f32(const float* x, const float* dz, float* parts, int B, int H, int W, int C, void* stream);
/* y = GELU(u) (exact erf form, nn.GELU()) and du = dy GELU'(u) on n values (n % 4 == 0) */
int gecco_gelu_f32(const float* u, float* y, size_t n, void* stream);
int gecco_gelu_bwd_f32(const float* u, const float* dy, float* du, size_t n, void* stream);
/* the stem's patch matrix (B H/4 W/4, 48), k = (ci, dy, dx) as in conv.weight.reshape(C, 48): its weight gradient is dz^T @ patches.
 * H, W >= 4, floored like the stem */
int gecco_convnext_im2col4_f32(const float* x, float* out, int B, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif
