// What every translation unit of the C ABI (api_*.hip) needs: the error buffer, the workspace carver, the option table's reader, the GemmArgs
// fills and the argument checks the entry points share.  Internal (not installed); namespace gecco_api, so that nothing here looks like ABI.
#pragma once
#include "../../include/gecco_hip.h"
#include "kernels.h"

namespace gecco_api {

// One buffer per thread for the whole library (gecco_last_error reads it): defined, with fail(), in api_network.hip
extern thread_local char g_err[512];
int fail(int rc, const char* fmt, ...);

inline int check(int rc, const char* what) {
    if (rc == 0) return 0;
    if (rc > 0) return fail(rc, "%s: HIP error %d (%s)", what, rc, hipGetErrorString((hipError_t)rc));
    return fail(rc, "%s: unsupported arguments (code %d)", what, rc);
}
#define TRY(expr, what)                  \
    do {                                 \
        int rc_ = check((expr), (what)); \
        if (rc_) return rc_;             \
    } while (0)

// Bump allocator over the caller's workspace (256-byte aligned carves).  With base == nullptr it
// only measures, so *_workspace_bytes() and the forward use the same code path.
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(void* b) : base(static_cast<char*>(b)) {}
    float* f32(size_t n) {
        off = (off + 255) & ~size_t(255);
        float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
        off += n * sizeof(float);
        return p;
    }
};

inline int row_tiles_gemm(int rows) { const int bm = gemm_row_tile(rows); return (rows + bm - 1) / bm; }
inline int row_tiles_stats(int rows) { const int bm = stats_row_tile(rows); return (rows + bm - 1) / bm; }

// Path switches for A/B runs and tests: gecco_set_option, or the environment (GECCO_ASTAT, GECCO_CHAIN) on first use (api_network.hip)
enum { OPT_ASTAT = 0, OPT_CHAIN = 1, OPT_HEADMAJOR = 2, OPT_MLPFUSED = 3, OPT_UNPOOLFUSED = 4, OPT_LO8 = 5, OPT_ACTIMG = 6, OPT_H8 = 7, OPT_KVQ64 = 8, OPT_H8AREG = 9, OPT_CHAIN2 = 10, OPT_UNPOOLH8 = 11, OPT_MLPW = 12, OPT_CHAINCL = 13, OPT_H6 = 14, OPT_KVFOLD = 15, OPT_MLPWSHARE = 16, OPT_KVQPERM = 17, OPT_IMGPROJ16 = 18, OPT_LIFT0 = 19, OPT_COUNT = 20 };
// "lift0" is the one option with three levels (0, 1, 2): a plan's table holds "level >= 1" at bit OPT_LIFT0 of opt_vals and "level 2" at the bit above it
enum { OPT_LIFT0_HI = OPT_LIFT0 + 1 };
int option(int which);

// The pyramid and reparametrisation of a projective lookup as the kernels take them (api_model_ops.hip; the ray network reads them too)
int make_lookup_args(const GeccoReparam* rp, const GeccoPyramid* pyr, LookupArgs* a);

// The operands every GEMM on contiguous rows has; everything else is absent unless the caller names it
inline GemmArgs gemm_args(const float* A, const float* W, const float* bias, float* C, int B, int rows, int K, int Nout) {
    GemmArgs g{};
    g.A = A; g.W = W; g.bias = bias; g.C = C; g.B = B; g.rows = rows; g.K = K; g.Nout = Nout; g.lda = K; g.ldw = K; g.ldc = Nout; g.ldr = Nout;
    return g;
}
// ... of an image-fed GEMM (no W) whose Nout1 + Nout2 columns go to C1 and, the last Nout2, to C2 (null: no second tensor; Nout2 still counts as given)
inline GemmArgs gemm_args_pair(const float* A, const float* bias1, float* C1, int Nout1, const float* bias2, float* C2, int Nout2, int B, int rows, int K) {
    GemmArgs g = gemm_args(A, nullptr, bias1, C1, B, rows, K, Nout1 + Nout2);
    g.ldc = Nout1; g.ldr = Nout1;
    if (C2) { g.C2 = C2; g.bias2 = bias2; g.n_split = Nout1; g.ldc2 = Nout2; }
    return g;
}

// "a finite fp32 number > 0": false for zero, negatives, NaN and +inf
inline bool finite_positive(float x) { return x > 0.f && x <= 3.402823466e38f; }

// The checks the unit entry points repeat.  `who` is the entry point's name in its messages; return codes and texts are part of the ABI's
// contract (tests/golden/api_errors.json), so an entry point keeps its own spelling (`spaced`: "pro_a / pro_o") and its own code (`rc`).
inline int check_pro_pair(const char* who, const float* pro_a, const float* pro_o, bool spaced = false) {
    if ((pro_a == nullptr) == (pro_o == nullptr)) return 0;
    return fail(-1, spaced ? "%s: pro_a / pro_o must both be set" : "%s: pro_a/pro_o must both be set", who);
}
inline int check_alpha(const char* who, int act, const float* alpha, int rc) {
    return ((act == 1 || act == 2) && !alpha) ? fail(rc, "%s: GaussianActivation needs alpha", who) : 0;
}
// precision 0 / 1 / 2, the scratch that 1 and 2 build the image of W in
inline int check_precision(const char* who, int precision, const void* wsplit) {
    if (precision < 0 || precision > 2) return fail(-2, "%s: precision must be 0 (fp32), 1 (split-bf16) or 2 (fp16)", who);
    if (precision >= 1 && !wsplit) return fail(-1, "%s: precision 1 / 2 need the wsplit scratch", who);
    return 0;
}
// the epilogue forms that only the LDS-DMA kernels have: a shape and precision they take (`dma_ok`), wsplit, and W == NULL (image ready) only where an image is read
inline int check_dma_linear(const char* who, bool dma_ok, const float* W, int precision, const void* wsplit) {
    if (!dma_ok) return fail(-2, "%s: shape / precision outside the LDS-DMA kernels' reach", who);
    if (precision >= 1 && !wsplit) return fail(-1, "%s: precision 1 / 2 need wsplit", who);
    if (!W && precision == 0) return fail(-2, "%s: W == NULL (image ready) needs precision 1 / 2", who);
    return 0;
}

}  // namespace gecco_api
