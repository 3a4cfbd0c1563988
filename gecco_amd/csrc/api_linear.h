// The linear plumbing that the network's orchestration (api_network.hip, which defines the functions declared here) and the unit
// entry points (api_linear.hip) share, and the weight-image helpers of the latter.  Internal, like api_common.h.
#pragma once
#include "api_common.h"

#include <optional>

namespace gecco_api {

// One linear, C = act(A' W^T + bias) (+ residual, + statistics): its operands (g; linear() decides g.precision and g.w_img) and where its weight image comes from
struct Lin {
    GemmArgs g;
    int prec = 0;                       // 1 (split-bf16) / 2 (fp16) apply to the N-token GEMMs the LDS-DMA kernels take ...
    float* wsplit = nullptr;            // ... `wsplit` receives the tiled image of W first (a ~3 us pass over <= 1.2 MB: weights may change between calls) ...
    const float* img_ready = nullptr;   // ... unless the image was already converted this forward
    Lin(const float* A, const float* W, const float* bias, float* C, int B, int rows, int K, int Nout) : g(gemm_args(A, W, bias, C, B, rows, K, Nout)) {}
    Lin& pro(const float* a, const float* o) { g.pro_a = a; g.pro_o = o; return *this; }   // AdaGN apply on A
    Lin& activation(int kind, const float* al) { g.act = kind; g.alpha = al; return *this; }
    Lin& plus(const float* r) { g.residual = r; return *this; }
    Lin& with_stats(float* st) { g.stats = st; return *this; }
    Lin& weights(int p, float* scratch, const float* ready = nullptr) { prec = p; wsplit = scratch; img_ready = ready; return *this; }
    // the unit entry points: with W == NULL, `ws` already holds the image of W
    Lin& weights_or_image(int p, void* ws) { return weights(p, g.W ? static_cast<float*>(ws) : nullptr, g.W ? nullptr : static_cast<const float*>(ws)); }
    Lin& f16(int a, int c) { g.a_f16 = a; g.c_f16 = c; return *this; }   // fp16 tensors exist only between the fp16 kernels (st_route checks support)
    Lin& image(int a, int c) { g.a_img = a; g.c_img = c; return *this; } // activation handed over as a tiled split image (kernels.h); callers check act_image_ok
};

int linear(Lin& a, hipStream_t s);   // works on a.g in place: no copy of the operands on the eager path
// Two linears over the same (AdaGN-modulated) A in one launch: `a` is the first, C1 = A' W1^T + b1 (Nout1 columns), and C2 = A' W2^T + b2.
// Returns 1 when the fused form does not apply (caller issues the two linears), 0 on success, <0 on error.
int linear_pair(const Lin& a, const float* W2, const float* b2, int Nout2, float* C2, hipStream_t s);

typedef int (*ImageLaunch)(const SplitJobs&, hipStream_t);   // an image kernel that takes a table of jobs ...
template <int (*One)(const float*, void*, int, int, int, hipStream_t)>
int launch_each(const SplitJobs& jobs, hipStream_t s) {   // ... and a single-image kernel as one: a launch per job
    for (int i = 0; i < jobs.n; ++i)
        if (const int rc = One(jobs.job[i].W, jobs.job[i].img, jobs.job[i].Nout, jobs.job[i].K, jobs.job[i].ldw, s)) return rc;
    return 0;
}

// The images of one weight, or of two that share K, built into `wsplit` by one call of `launch`: the second (W null: there is none) starts
// `second_offset_bytes` behind the first.  format: of the builder `launch` is (weight_images.h)
struct ImageOf { const float* W; int Nout, ldw; ImageFormat format; };
inline int build_images(ImageLaunch launch, void* wsplit, int K, hipStream_t s, ImageOf first, ImageOf second = {}, size_t second_offset_bytes = 0) {
    SplitJobs jobs;
    float* img = static_cast<float*>(wsplit);
    jobs.n = 0;
    jobs.job[jobs.n++] = SplitJob{first.W, img, first.Nout, K, first.ldw, first.format};
    if (second.W) jobs.job[jobs.n++] = SplitJob{second.W, img + second_offset_bytes / sizeof(float), second.Nout, K, second.ldw, second.format};
    return launch(jobs, s);
}

// A caller's batch of image jobs (the gecco_*_images_f32 entry points), a full table per launch.  format_of(job) gives the job's format
// (std::optional<ImageFormat>), or nothing where the builder does not take the job: the call then fails with "<who>: job <i> needs <needs>"
template <class FormatOf>
int image_batch(const char* who, const char* needs, const GeccoSplitJob* jobs, int n, FormatOf format_of, ImageLaunch launch, hipStream_t s) {
    if (n < 0 || (n > 0 && !jobs)) return fail(-1, "%s: null argument", who);
    SplitJobs sj;
    sj.n = 0;
    for (int i = 0; i < n; ++i) {
        const GeccoSplitJob& j = jobs[i];
        const std::optional<ImageFormat> format = (j.W && j.img && j.Nout > 0 && j.K > 0) ? format_of(j) : std::nullopt;
        if (!format) return fail(-2, "%s: job %d needs %s", who, i, needs);
        sj.job[sj.n++] = SplitJob{j.W, static_cast<float*>(j.img), j.Nout, j.K, j.ldw, *format};
        if (sj.n == (int)(sizeof sj.job / sizeof sj.job[0])) {
            TRY(launch(sj, s), who);
            sj.n = 0;
        }
    }
    TRY(launch(sj, s), who);
    return 0;
}

// The jobs of one layer's mlp_fused_f16.hip stream at `stream`, in the order the kernel consumes it: per 128-wide hidden chunk j the fp16 image
// of W0's tile j (128 x C), then W2[:, chunk j] (C x 128) as two 64-k halves.  push(W, img, Nout, K, ldw, F16Image, what) appends one job
// (returns != 0 to stop; `what` names the job in the network's error texts).  The stream is as large as the two images it replaces: split_f16_image_bytes(width, C) + split_f16_image_bytes(C, width)
template <class Push>
int mlp_fused_f16_stream_jobs(const float* W0, const float* W2, int C, int width, float* stream, Push push) {
    const size_t w0_tile = split_f16_image_bytes(128, C) / sizeof(float), w2_half = split_f16_image_bytes(C, 64) / sizeof(float);
    for (int jc = 0; jc < width / 128; ++jc) {
        float* chunk = stream + (size_t)jc * (w0_tile + 2 * w2_half);
        if (const int rc = push(W0 + (size_t)jc * 128 * C, chunk, 128, C, C, F16_PLAIN, "split(mlp.0 tile)")) return rc;
        for (int hf = 0; hf < 2; ++hf)
            if (const int rc = push(W2 + (size_t)jc * 128 + hf * 64, chunk + w0_tile + hf * w2_half, C, 64, width, F16_PLAIN, "split(mlp.2 K-slice)")) return rc;
    }
    return 0;
}

}  // namespace gecco_api
