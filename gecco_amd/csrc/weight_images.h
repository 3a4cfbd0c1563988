// The weight-image formats.  A weight image ("stream") is a weight matrix W (Nout, ldw) fp32 re-laid-out as the LDS tiles of ONE consumer
// kernel; the consumer assumes the format, so the builder, the consumer, the job tables that name the format (api_linear.hip,
// api_network.hip) and the workspace carve (carve_st) must agree on it.  This header owns the names: one enum per image builder (a job
// table goes to exactly one of the three), the job record that carries a value of them, and the kvq stream's packed lo range.
// Host + device; included by kernels.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// split_bf16_tiled_multi_kernel (gemm_f32_dma.hip): bf16 hi | lo planes in 128-column x 16-k tiles, split_bf16_image_bytes(Nout, K)
enum Bf16Image : int {
    BF16_PLAIN = 0,        // the image of W: GemmArgs::w_img of the split-bf16 LDS-DMA GEMM (gemm_f32_dma.hip) and of gemm_x3_areg.hip
    BF16_TRANSPOSED = 4,   // W is (K, ldw) and the image is of W^T, read straight from W: the same consumers (the training path's dX products)
};

// split_f16_tiled_multi_kernel (gemm_f16_dma.hip): fp16 in 128-column x 32-k tiles, split_f16_image_bytes(Nout, K) unless noted
enum F16Image : int {
    F16_PLAIN = 0,         // fp16(W): w_img of gemm_f16_dma.hip / gemm_f16_astat.hip, the streams of mlp_fused_f16.hip, unpool_outproj_f16.hip and
                           // inducer_chain_f16.hip
    F16_LO = 1,            // the LOW part fp16(W - fp16(W)) in the same layout: GemmArgs::w_img2 of gemm_f16_astat.hip (two-term weights, mixed mode)
    F16_LO_FP8 = 2,        // the low part as fp8 (e4m3) x H8_WL_SCALE in 64-k blocks, half the bytes: w_img2 with GemmArgs::lo_fp8
    F16_TRANSPOSED = 4,    // W is (K, ldw) and the image is of W^T: F16_PLAIN's consumers (the training path's dX products)
    F16_HI_LO = 8,         // per column tile the blocks of fp16(W), then those of the low part, twice the bytes: inducer_chain_f16.hip with
                           // ChainArgs::two_term (one stream for both terms)
};

// h8_image_multi_kernel (gemm_h8_astat.hip).  H8_KVQ is a FLAG: a kvq format is kvq_format(...) below, never the bare enumerator
enum H8Image : int {
    H8_MLP0 = 0,           // the h8 stream (fp16 W + fp8 cross-term operands), 64-column tiles, h8_image_bytes: gemm_h8_astat_kernel (mlp.0 of the
                           // mixed mode, the h8 training forward)
    H8_KVQ = 1,            // the kv_proj | q_proj stream, 64-column tiles, fp16 with fp8 L stages behind the tiles of the lo range,
                           // kvq_image_bytes: gemm_kvq_astat_kernel and its fp32-output training forms
    H8_W128 = 2,           // H8_MLP0's content in 128-column tiles (Nout padded up to whole tiles), h8_w128_image_bytes: gemm_h8_areg.hip
    H8_ATTN_ORDER = 16,    // H8_MLP0's tiles with k in the attention accumulator's order, h8_image_bytes: unpool_outproj_h8.hip
    H8_H6 = 32,            // H8_MLP0 with the cross-term operands as fp6 with block scales, h8_image_bytes: gemm_h8_astat_kernel's F6 forms (GemmArgs::h6)
};
enum KvqOrder : int {      // what kvq_format adds to H8_KVQ
    KVQ_PLAIN = 0,
    KVQ_TRANSPOSED = 4,    // W is (K, ldw) and the stream is of W^T; one-term (the lo range is ignored): the training path's dX products
    KVQ_HEAD48 = 64,       // head dim 48: the columns of every 384-column segment dealt head-aligned to its six tiles (GemmArgs::kvq_perm, kvq_perm48_col)
};
constexpr int H8_INVALID = -1;   // kvq_format's answer to a range it cannot pack; h8_image_multi_launch refuses the job (-9)

// A value of one builder's enum as a job carries it.  No conversion from int: nobody writes the numbers.
class ImageFormat {
    int bits_;
    constexpr explicit __host__ __device__ ImageFormat(int bits) : bits_(bits) {}
    friend constexpr __host__ __device__ ImageFormat kvq_format(int, int, KvqOrder);

 public:
    ImageFormat() = default;
    constexpr __host__ __device__ ImageFormat(Bf16Image f) : bits_(f) {}
    constexpr __host__ __device__ ImageFormat(F16Image f) : bits_(f) {}
    constexpr __host__ __device__ ImageFormat(H8Image f) : bits_(f) {}
    constexpr __host__ __device__ int bits() const { return bits_; }
};

// The kvq stream whose 64-column tiles [lo_begin_tile, lo_end_tile) carry the second (fp8) weight term.  The two indices ride in the
// format word, 12 bits each: this function and the two accessors are the only place that knows where.
constexpr int KVQ_LO_BITS = 12, KVQ_LO_BEGIN_SHIFT = 8, KVQ_LO_END_SHIFT = 20, KVQ_LO_MASK = (1 << KVQ_LO_BITS) - 1;
constexpr __host__ __device__ ImageFormat kvq_format(int lo_begin_tile, int lo_end_tile, KvqOrder order = KVQ_PLAIN) {
    return ((lo_begin_tile | lo_end_tile) & ~KVQ_LO_MASK)
               ? ImageFormat(H8_INVALID)
               : ImageFormat((int)((unsigned)(H8_KVQ | order) | (unsigned)lo_begin_tile << KVQ_LO_BEGIN_SHIFT | (unsigned)lo_end_tile << KVQ_LO_END_SHIFT));
}
constexpr __host__ __device__ int kvq_lo_begin(ImageFormat f) { return (f.bits() >> KVQ_LO_BEGIN_SHIFT) & KVQ_LO_MASK; }
constexpr __host__ __device__ int kvq_lo_end(ImageFormat f) { return (f.bits() >> KVQ_LO_END_SHIFT) & KVQ_LO_MASK; }
static_assert(kvq_format(6, 12, KVQ_HEAD48).bits() == (1 | 64 | 6 << 8 | 12 << 20) && kvq_lo_begin(kvq_format(6, 12)) == 6 && kvq_lo_end(kvq_format(6, 4095)) == 4095 &&
                  kvq_format(0, 4096).bits() == H8_INVALID && kvq_format(-1, 0).bits() == H8_INVALID,
              "the format words are kernel arguments: their values do not change");

struct SplitJob { const float* W; float* img; int Nout, K, ldw; ImageFormat format; };   // one image: W (Nout, ldw) -> img, in `format` of the builder the table goes to
struct SplitJobs { SplitJob job[96]; int n; };   // 3 KiB of kernel arguments
static_assert(sizeof(SplitJob) == 32 && sizeof(SplitJobs) == 3 * 1024 + 8, "the job table is passed by value as kernel arguments");
