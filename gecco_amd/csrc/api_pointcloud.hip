// C ABI of libgecco_hip.so, part 4 of 4: point-cloud operators and metrics (distance matrix, Chamfer, set metrics, EMD,
// Sinkhorn, farthest-point sampling, kNN, normals, ICP, FPFH and feature matching, RANSAC registration, voxel grid, DBSCAN, radius search
// and its grid index, ISS keypoints).
#include "api_common.h"

using namespace gecco_api;

extern "C" {

int gecco_distance_matrix_f32(const float* a, const float* b, float* D, int B, int N, int M, int squared, void* stream) {
    if (!a || !b || !D) return fail(-1, "distance_matrix: null argument");
    TRY(dist_matrix_launch(a, b, D, B, N, M, squared, (hipStream_t)stream), "distance_matrix");
    return 0;
}
int gecco_set_chamfer_f32(const float* a, const float* b, float* out, int S, int T, int N, int M, int squared, void* stream) {
    if (!a || !b || !out) return fail(-1, "set_chamfer: null argument");
    if (S <= 0 || T <= 0 || N <= 0 || M <= 0) return fail(-2, "set_chamfer: empty set or cloud");
    hipStream_t s = (hipStream_t)stream;
    TRY(set_nearest_mean_launch(a, b, out, S, T, N, M, squared, T, 1, 0.5f, 0, s), "set_chamfer(a -> b)");
    TRY(set_nearest_mean_launch(b, a, out, T, S, M, N, squared, 1, T, 0.5f, 1, s), "set_chamfer(b -> a)");
    return 0;
}

int gecco_set_metrics_f32(const float* ss, const float* sd, const float* dd, int n, float* out3, int* flags, void* stream) {
    if (!ss || !sd || !dd || !out3 || !flags) return fail(-1, "set_metrics: null argument");
    if (n <= 0) return fail(-2, "set_metrics: empty set");
    TRY(set_metrics_launch(ss, sd, dd, n, out3, flags, (hipStream_t)stream), "set_metrics");
    return 0;
}

int gecco_chamfer_f32(const float* a, const float* b, float* out, float* ws, int B, int N, int M, int squared, void* stream) {
    if (!a || !b || !out || !ws) return fail(-1, "chamfer: null argument");
    hipStream_t s = (hipStream_t)stream;
    float* min_ab = ws;                       // (B, N): nearest b of every a
    float* min_ba = ws + (size_t)B * N;       // (B, M): nearest a of every b
    TRY(nearest_dist_launch(a, b, min_ab, B, N, M, squared, s), "chamfer(a -> b)");
    TRY(nearest_dist_launch(b, a, min_ba, B, M, N, squared, s), "chamfer(b -> a)");
    TRY(row_mean_launch(min_ab, out, B, N, 0.5f, 0, s), "chamfer(mean a)");
    TRY(row_mean_launch(min_ba, out, B, M, 0.5f, 1, s), "chamfer(mean b)");
    return 0;
}
int gecco_chamfer_idx_f32(const float* a, const float* b, float* out, float* ws, int* ia, int* ib, int B, int N, int M, int squared,
                          void* stream) {
    if (!a || !b || !out || !ws || !ia || !ib) return fail(-1, "chamfer_idx: null argument");
    if (B < 1 || N < 1 || M < 1) return fail(-2, "chamfer_idx: B = %d, N = %d, M = %d must all be >= 1", B, N, M);
    if (B > 65535) return fail(-2, "chamfer_idx: B = %d above 65535 (one grid row per sample)", B);
    if (squared != 0 && squared != 1) return fail(-2, "chamfer_idx: squared = %d is not 0 / 1", squared);
    hipStream_t s = (hipStream_t)stream;
    float* min_ab = ws;                       // the layout and the launch order of gecco_chamfer_f32
    float* min_ba = ws + (size_t)B * N;
    TRY(nearest_idx_launch(a, b, min_ab, ia, B, N, M, squared, s), "chamfer_idx(a -> b)");
    TRY(nearest_idx_launch(b, a, min_ba, ib, B, M, N, squared, s), "chamfer_idx(b -> a)");
    TRY(row_mean_launch(min_ab, out, B, N, 0.5f, 0, s), "chamfer_idx(mean a)");
    TRY(row_mean_launch(min_ba, out, B, M, 0.5f, 1, s), "chamfer_idx(mean b)");
    return 0;
}
int gecco_chamfer_bwd_f32(const float* a, const float* b, const int* ia, const int* ib, const float* gout, float* da, float* db, int B,
                          int N, int M, int squared, void* stream) {
    if (!a || !b || !ia || !ib || !gout || (!da && !db)) return fail(-1, "chamfer_bwd: null argument");
    if (B < 1 || N < 1 || M < 1) return fail(-2, "chamfer_bwd: B = %d, N = %d, M = %d must all be >= 1", B, N, M);
    if (B > 65535) return fail(-2, "chamfer_bwd: B = %d above 65535 (one grid row per sample)", B);
    if (squared != 0 && squared != 1) return fail(-2, "chamfer_bwd: squared = %d is not 0 / 1", squared);
    hipStream_t s = (hipStream_t)stream;
    if (da) TRY(chamfer_bwd_launch(a, b, ia, ib, gout, da, B, N, M, squared, s), "chamfer_bwd(da)");
    if (db) TRY(chamfer_bwd_launch(b, a, ib, ia, gout, db, B, M, N, squared, s), "chamfer_bwd(db)");
    return 0;
}
int gecco_emd_bwd_f32(const float* a, const float* b, const int* cols, const float* gout, float* da, float* db, int B, int N,
                      int average_squared, void* stream) {
    if (!a || !b || !cols || !gout || (!da && !db)) return fail(-1, "emd_bwd: null argument");
    if (B < 1 || N < 1) return fail(-2, "emd_bwd: B = %d, N = %d must both be >= 1", B, N);
    if (B > 65535) return fail(-2, "emd_bwd: B = %d above 65535 (one grid row per sample)", B);
    if (average_squared != 0 && average_squared != 1) return fail(-2, "emd_bwd: average_squared = %d is not 0 / 1", average_squared);
    TRY(emd_bwd_launch(a, b, cols, gout, da, db, B, N, average_squared, (hipStream_t)stream), "emd_bwd");
    return 0;
}
int gecco_sinkhorn_f32(const float* C, float* f, float* g, float* rowcost, float* out, int B, int N, int M, float epsilon,
                       int iterations, void* stream) {
    if (!C || !f || !g || !rowcost || !out) return fail(-1, "sinkhorn: null argument");
    if (epsilon <= 0.f || iterations < 1) return fail(-2, "sinkhorn: epsilon > 0 and iterations >= 1");
    hipStream_t s = (hipStream_t)stream;
    TRY((int)hipMemsetAsync(g, 0, (size_t)B * M * sizeof(float), s), "sinkhorn(g = 0)");
    for (int it = 0; it < iterations; ++it) TRY(sinkhorn_step_launch(C, f, g, B, N, M, epsilon, s), "sinkhorn(step)");
    TRY(sinkhorn_cost_launch(C, f, g, rowcost, out, B, N, M, epsilon, s), "sinkhorn(cost)");
    return 0;
}

int gecco_emd_f32(const float* a, const float* b, int B, int N, int match_squared, int average_squared, float* out, int* assign,
                  int* status, int max_rounds, void* stream) {
    if (!a || !b || !out || !status) return fail(-1, "emd: null argument");
    if (B <= 0) return fail(-2, "emd: empty batch");
    if (N < 1 || N > GECCO_EMD_MAX_POINTS) return fail(-2, "emd: N = %d outside 1 .. %d (the LDS-resident limit)", N, GECCO_EMD_MAX_POINTS);
    if (max_rounds < 0) return fail(-2, "emd: max_rounds %d < 0", max_rounds);
    TRY(emd_auction_launch(a, b, out, assign, status, B, 1, 0, N, match_squared != 0, average_squared != 0,
                           max_rounds ? max_rounds : GECCO_EMD_DEFAULT_ROUNDS, (hipStream_t)stream), "emd");
    return 0;
}
int gecco_set_emd_f32(const float* a, const float* b, int S, int T, int N, int match_squared, int average_squared, float* out,
                      int* status, int max_rounds, void* stream) {
    if (!a || !b || !out || !status) return fail(-1, "set_emd: null argument");
    if (S <= 0 || T <= 0) return fail(-2, "set_emd: empty set");
    if ((long long)S * T > 0x7fffffffLL) return fail(-2, "set_emd: S * T = %lld pairs above 2^31 - 1", (long long)S * T);
    if (N < 1 || N > GECCO_EMD_MAX_POINTS) return fail(-2, "set_emd: N = %d outside 1 .. %d (the LDS-resident limit)", N, GECCO_EMD_MAX_POINTS);
    if (max_rounds < 0) return fail(-2, "set_emd: max_rounds %d < 0", max_rounds);
    TRY(emd_auction_launch(a, b, out, nullptr, status, S * T, T, 1, N, match_squared != 0, average_squared != 0,
                           max_rounds ? max_rounds : GECCO_EMD_DEFAULT_ROUNDS, (hipStream_t)stream), "set_emd");
    return 0;
}

// matrix-free Sinkhorn (sinkhorn.hip).  form: 0 auto (resident within GECCO_SINKHORN_RESIDENT_MAX_POINTS), 1 resident, 2 streaming
static int sinkhorn_common_checks(const char* who, int N, int M, float epsilon) {
    if (N < 1 || M < 1) return fail(-2, "%s: N = %d, M = %d must both be >= 1", who, N, M);
    if (!(epsilon > 0.f)) return fail(-2, "%s: epsilon = %g must be > 0", who, (double)epsilon);
    return 0;
}
int gecco_sinkhorn_cloud_f32(const float* a, const float* b, float* f, float* g, float* ws, float* out, int B, int N, int M, float epsilon,
                             int iterations, int form, void* stream) {
    if (!a || !b || !out) return fail(-1, "sinkhorn_cloud: null argument");
    if (B < 1) return fail(-2, "sinkhorn_cloud: empty batch");
    if (int rc = sinkhorn_common_checks("sinkhorn_cloud", N, M, epsilon)) return rc;
    if (iterations < 1) return fail(-2, "sinkhorn_cloud: iterations = %d must be >= 1", iterations);
    if (form < 0 || form > 2) return fail(-2, "sinkhorn_cloud: form = %d is not 0 (auto), 1 (resident) or 2 (streaming)", form);
    const bool fits = (long long)N + M <= GECCO_SINKHORN_RESIDENT_MAX_POINTS;
    if (form == 1 && !fits)
        return fail(-2, "sinkhorn_cloud: the resident form takes N + M <= %d (got %d + %d)", GECCO_SINKHORN_RESIDENT_MAX_POINTS, N, M);
    if (form == 1 || (form == 0 && fits)) {
        TRY(sinkhorn_resident_launch(a, b, f, g, out, B, 1, 0, N, M, epsilon, iterations, (hipStream_t)stream), "sinkhorn_cloud(resident)");
        return 0;
    }
    if (!f || !g || !ws) return fail(-1, "sinkhorn_cloud: the streaming form needs f, g and ws");
    if (B > 65535) return fail(-2, "sinkhorn_cloud: B = %d above 65535 (one grid row per sample)", B);
    TRY(sinkhorn_stream_launch(a, b, f, g, ws, out, B, N, M, epsilon, iterations, (hipStream_t)stream), "sinkhorn_cloud(streaming)");
    return 0;
}
int gecco_set_sinkhorn_f32(const float* a, const float* b, float* out, int S, int T, int N, int M, float epsilon, int iterations,
                           void* stream) {
    if (!a || !b || !out) return fail(-1, "set_sinkhorn: null argument");
    if (S <= 0 || T <= 0) return fail(-2, "set_sinkhorn: empty set");
    if ((long long)S * T > 0x7fffffffLL) return fail(-2, "set_sinkhorn: S * T = %lld pairs above 2^31 - 1", (long long)S * T);
    if (int rc = sinkhorn_common_checks("set_sinkhorn", N, M, epsilon)) return rc;
    if (iterations < 1) return fail(-2, "set_sinkhorn: iterations = %d must be >= 1", iterations);
    if ((long long)N + M > GECCO_SINKHORN_RESIDENT_MAX_POINTS)
        return fail(-2, "set_sinkhorn: the resident form takes N + M <= %d (got %d + %d)", GECCO_SINKHORN_RESIDENT_MAX_POINTS, N, M);
    TRY(sinkhorn_resident_launch(a, b, nullptr, nullptr, out, S * T, T, 1, N, M, epsilon, iterations, (hipStream_t)stream), "set_sinkhorn");
    return 0;
}
int gecco_sinkhorn_cloud_bwd_f32(const float* a, const float* b, const float* f, const float* g, const float* gout, float* da, float* db,
                                 int B, int N, int M, float epsilon, void* stream) {
    if (!a || !b || !f || !g || !gout || (!da && !db)) return fail(-1, "sinkhorn_cloud_bwd: null argument");
    if (B < 1) return fail(-2, "sinkhorn_cloud_bwd: empty batch");
    if (B > 65535) return fail(-2, "sinkhorn_cloud_bwd: B = %d above 65535 (one grid row per sample)", B);
    if (int rc = sinkhorn_common_checks("sinkhorn_cloud_bwd", N, M, epsilon)) return rc;
    TRY(sinkhorn_bwd_launch(a, b, f, g, gout, da, db, B, N, M, epsilon, (hipStream_t)stream), "sinkhorn_cloud_bwd");
    return 0;
}

// farthest-point sampling (fps.hip).  form: 0 auto (resident within GECCO_FPS_RESIDENT_MAX_POINTS), 1 resident, 2 streaming
int gecco_fps_f32(const float* points, const int* start, int* idx, float* sel2, void* ws, int B, int N, int k, int form, void* stream) {
    if (!points || !idx) return fail(-1, "fps: null argument");
    if (B < 1 || N < 1 || k < 1) return fail(-2, "fps: B = %d, N = %d, k = %d must all be >= 1", B, N, k);
    if (k > N) return fail(-2, "fps: k = %d above N = %d", k, N);
    if (form < 0 || form > 2) return fail(-2, "fps: form = %d is not 0 (auto), 1 (resident) or 2 (streaming)", form);
    const bool fits = N <= GECCO_FPS_RESIDENT_MAX_POINTS;
    if (form == 1 && !fits) return fail(-2, "fps: the resident form takes N <= %d (got %d)", GECCO_FPS_RESIDENT_MAX_POINTS, N);
    if (form == 1 || (form == 0 && fits)) {
        TRY(fps_resident_launch(points, start, idx, sel2, B, N, k, (hipStream_t)stream), "fps(resident)");
        return 0;
    }
    if (!ws) return fail(-1, "fps: the streaming form needs ws");
    if ((long long)B * ((N + GECCO_FPS_STREAM_SLICE - 1) / GECCO_FPS_STREAM_SLICE) > 0x7fffffffLL)
        return fail(-2, "fps: B * ceil(N / %d) workgroups above 2^31 - 1", GECCO_FPS_STREAM_SLICE);
    TRY(fps_stream_launch(points, start, idx, sel2, ws, B, N, k, (hipStream_t)stream), "fps(streaming)");
    return 0;
}

// k-nearest neighbours (knn.hip).  form: 0 auto (knn_launch's rule; without ws it is the direct form), 1 direct, 2 split
size_t gecco_knn_workspace_bytes(int B, int M, int N, int k) {
    if (B < 1 || M < 1 || N < 1 || k < 1) return 0;
    return GECCO_KNN_WORKSPACE_BYTES(B, M, N, k);
}
int gecco_knn_f32(const float* query, const float* ref, int32_t* idx, float* d2, void* ws, int B, int M, int N, int k, int exclude_self,
                  int form, void* stream) {
    if (!query || !ref || !idx) return fail(-1, "knn: null argument");
    if (B < 1 || M < 1 || N < 1) return fail(-2, "knn: B = %d, M = %d, N = %d must all be >= 1", B, M, N);
    if (k < 1 || k > GECCO_KNN_MAX_K) return fail(-2, "knn: k = %d is not in 1 .. %d", k, GECCO_KNN_MAX_K);
    if (exclude_self && M != N) return fail(-2, "knn: exclude_self needs the query cloud to be the reference cloud (M = %d, N = %d)", M, N);
    if (k > N - (exclude_self ? 1 : 0))
        return fail(-2, "knn: k = %d above the %d candidates of a query (N = %d%s)", k, N - (exclude_self ? 1 : 0), N,
                    exclude_self ? ", itself excluded" : "");
    if (form < 0 || form > 2) return fail(-2, "knn: form = %d is not 0 (auto), 1 (direct) or 2 (split)", form);
    if (form == 2 && !ws) return fail(-1, "knn: the split form needs ws");
    const int rc = knn_launch(query, ref, idx, d2, ws, B, M, N, k, exclude_self ? 1 : 0, form, (hipStream_t)stream);
    if (rc == -3) return fail(-2, "knn: the grid for B = %d, M = %d, N = %d passes 2^31 - 1 workgroups", B, M, N);
    TRY(rc, "knn");
    return 0;
}

// normals and curvature from kNN lists (normals.hip).  d2 null: the distances a radius needs are recomputed from the coordinates
int gecco_normals_f32(const float* ref, const float* query, const int32_t* idx, const float* d2, const float* viewpoint, float radius2,
                      float* normal, float* eigenvalues, float* curvature, int32_t* count, int B, int M, int N, int k, void* stream) {
    if (!ref || !query || !idx || !normal) return fail(-1, "normals: null argument");
    if (B < 1 || M < 1 || N < 1) return fail(-2, "normals: B = %d, M = %d, N = %d must all be >= 1", B, M, N);
    if (k < 1 || k > GECCO_KNN_MAX_K) return fail(-2, "normals: k = %d is not in 1 .. %d", k, GECCO_KNN_MAX_K);
    const int rc = normals_launch(ref, query, idx, d2, viewpoint, radius2, normal, eigenvalues, curvature, count, B, M, N, k,
                                  (hipStream_t)stream);
    if (rc == -3) return fail(-2, "normals: the grid for B = %d, M = %d passes 2^31 - 1 workgroups", B, M);
    TRY(rc, "normals");
    return 0;
}

// ICP registration (icp.hip).  method 0 point-to-point / 1 point-to-plane; form as gecco_knn_f32; normals, init, correspondence nullable
size_t gecco_icp_workspace_bytes(int B, int M, int N) {
    if (B < 1 || M < 1 || N < 1) return 0;
    return GECCO_ICP_WORKSPACE_BYTES(B, M, N);
}
int gecco_icp_f32(const float* source, const float* target, const float* normals, const double* init, float r, int method,
                  int max_iterations, double relative_fitness, double relative_rmse, double* transformation, float* fitness,
                  float* inlier_rmse, int32_t* iterations, int32_t* status, int32_t* correspondence, void* ws, int B, int M, int N, int form,
                  void* stream) {
    if (!source || !target || !transformation || !fitness || !inlier_rmse || !iterations || !status || !ws)
        return fail(-1, "icp: null argument");
    if (B < 1 || M < 1 || N < 1) return fail(-2, "icp: B = %d, M = %d, N = %d must all be >= 1", B, M, N);
    if (method != 0 && method != 1) return fail(-2, "icp: method = %d is not 0 (point-to-point) or 1 (point-to-plane)", method);
    if (method == 1 && !normals) return fail(-1, "icp: the point-to-plane method needs normals");
    if (form < 0 || form > 2) return fail(-2, "icp: form = %d is not 0 (auto), 1 (direct) or 2 (split)", form);
    if (max_iterations < 0 || max_iterations > GECCO_ICP_MAX_ITERATIONS)
        return fail(-2, "icp: max_iterations = %d is not in 0 .. %d", max_iterations, GECCO_ICP_MAX_ITERATIONS);
    if (!finite_positive(r)) return fail(-2, "icp: r = %g must be a finite number > 0", (double)r);
    if (!(relative_fitness >= 0.0) || !(relative_rmse >= 0.0))
        return fail(-2, "icp: relative_fitness = %g and relative_rmse = %g must both be >= 0", relative_fitness, relative_rmse);
    const float r2 = (float)((double)r * (double)r);
    const int rc = icp_launch(source, target, normals, init, r2, method, max_iterations, relative_fitness, relative_rmse, transformation,
                              fitness, inlier_rmse, iterations, status, correspondence, ws, B, M, N, form, (hipStream_t)stream);
    if (rc == -3) return fail(-2, "icp: the grid for B = %d, M = %d, N = %d passes 2^31 - 1 workgroups", B, M, N);
    TRY(rc, "icp");
    return 0;
}

// FPFH descriptors (fpfh.hip).  radius2 0: no radius; spfh and count are required (the first launch's outputs, read by the second)
int gecco_fpfh_f32(const float* points, const float* normals, const int32_t* idx, float radius2, float* fpfh, float* spfh, int32_t* count,
                   int B, int N, int k, void* stream) {
    if (!points || !normals || !idx || !fpfh || !spfh || !count) return fail(-1, "fpfh: null argument");
    if (B < 1 || N < 1) return fail(-2, "fpfh: B = %d, N = %d must both be >= 1", B, N);
    if (k < 1 || k > GECCO_KNN_MAX_K) return fail(-2, "fpfh: k = %d is not in 1 .. %d", k, GECCO_KNN_MAX_K);
    if (k > N) return fail(-2, "fpfh: k = %d above N = %d", k, N);
    if (!(radius2 >= 0.f)) return fail(-2, "fpfh: radius2 = %g must be >= 0 (0: no radius)", (double)radius2);
    const int rc = fpfh_launch(points, normals, idx, radius2, fpfh, spfh, count, B, N, k, (hipStream_t)stream);
    if (rc == -3) return fail(-2, "fpfh: the grid for B = %d, N = %d passes 2^31 - 1 workgroups", B, N);
    TRY(rc, "fpfh");
    return 0;
}

// nearest neighbour in feature space (fpfh.hip).  form as gecco_knn_f32; d2 nullable
size_t gecco_feature_nn_workspace_bytes(int B, int M, int N) {
    if (B < 1 || M < 1 || N < 1) return 0;
    return GECCO_FEATURE_NN_WORKSPACE_BYTES(B, M, N);
}
int gecco_feature_nn_f32(const float* a, const float* b, int32_t* idx, float* d2, void* ws, int B, int M, int N, int C, int form,
                         void* stream) {
    if (!a || !b || !idx) return fail(-1, "feature_nn: null argument");
    if (B < 1 || M < 1 || N < 1) return fail(-2, "feature_nn: B = %d, M = %d, N = %d must all be >= 1", B, M, N);
    if (C < 1 || C > GECCO_FEATURE_MAX_DIM) return fail(-2, "feature_nn: C = %d is not in 1 .. %d", C, GECCO_FEATURE_MAX_DIM);
    if (form < 0 || form > 2) return fail(-2, "feature_nn: form = %d is not 0 (auto), 1 (direct) or 2 (split)", form);
    if (form == 2 && !ws) return fail(-1, "feature_nn: the split form needs ws");
    const int rc = feature_nn_launch(a, b, idx, d2, ws, B, M, N, C, form, (hipStream_t)stream);
    if (rc == -3) return fail(-2, "feature_nn: the grid for B = %d, M = %d, N = %d passes 2^31 - 1 workgroups", B, M, N);
    TRY(rc, "feature_nn");
    return 0;
}

// RANSAC registration from correspondences (ransac.hip).  inliers, hyp_triple, hyp_count, hyp_sum, candidates nullable
size_t gecco_ransac_workspace_bytes(int B, int M, int hypotheses) {
    if (B < 1 || M < 1 || hypotheses < 1 || hypotheses > GECCO_RANSAC_MAX_HYPOTHESES) return 0;
    return GECCO_RANSAC_WORKSPACE_BYTES(B, M, hypotheses);
}
int gecco_ransac_f32(const float* source, const float* target, const int32_t* corr, float r, double edge_similarity, int hypotheses,
                     int refine_passes, uint64_t seed, double* transformation, float* fitness, float* inlier_rmse, int32_t* n_pairs,
                     int32_t* best, int32_t* status, int32_t* inliers, int32_t* hyp_triple, int32_t* hyp_count, double* hyp_sum,
                     const double* candidates, void* ws, int B, int M, int N, void* stream) {
    if (!source || !target || !corr || !transformation || !fitness || !inlier_rmse || !n_pairs || !best || !status || !ws)
        return fail(-1, "ransac: null argument");
    if (B < 1 || M < 1 || N < 1) return fail(-2, "ransac: B = %d, M = %d, N = %d must all be >= 1", B, M, N);
    if (hypotheses < 1 || hypotheses > GECCO_RANSAC_MAX_HYPOTHESES)
        return fail(-2, "ransac: hypotheses = %d is not in 1 .. %d", hypotheses, GECCO_RANSAC_MAX_HYPOTHESES);
    if (refine_passes < 0 || refine_passes > GECCO_RANSAC_MAX_REFINE)
        return fail(-2, "ransac: refine_passes = %d is not in 0 .. %d", refine_passes, GECCO_RANSAC_MAX_REFINE);
    if (!finite_positive(r)) return fail(-2, "ransac: r = %g must be a finite number > 0", (double)r);
    if (!(edge_similarity >= 0.0) || !(edge_similarity <= 1.0))
        return fail(-2, "ransac: edge_similarity = %g is not in 0 .. 1", edge_similarity);
    const float r2 = (float)((double)r * (double)r);
    const int rc = ransac_launch(source, target, corr, r2, edge_similarity * edge_similarity, hypotheses, refine_passes,
                                 (unsigned long long)seed, transformation, fitness, inlier_rmse, n_pairs, best, status, inliers, hyp_triple,
                                 hyp_count, hyp_sum, candidates, ws, B, M, N, (hipStream_t)stream);
    if (rc == -3) return fail(-2, "ransac: the grid for B = %d, hypotheses = %d passes 2^31 - 1 workgroups", B, hypotheses);
    TRY(rc, "ransac");
    return 0;
}

// RANSAC plane segmentation (plane.hip).  mask, axis, viewpoint, candidates, inliers and the four hyp_ outputs nullable
size_t gecco_plane_ransac_workspace_bytes(int B, int N, int hypotheses) {
    if (B < 1 || N < 1 || hypotheses < 1 || hypotheses > GECCO_PLANE_RANSAC_MAX_HYPOTHESES) return 0;
    return GECCO_PLANE_RANSAC_WORKSPACE_BYTES(B, N, hypotheses);
}
int gecco_plane_ransac_f32(const float* points, const uint8_t* mask, float r, int hypotheses, int refine_passes, uint64_t seed,
                           const double* axis, double cos2, int min_inliers, const float* viewpoint, const double* candidates,
                           double* plane, float* fitness, float* inlier_rmse, int32_t* n_points, int32_t* n_inliers, int32_t* best,
                           int32_t* status, uint8_t* inliers, int32_t* hyp_triple, float* hyp_plane, int32_t* hyp_count, double* hyp_sum,
                           void* ws, int B, int N, void* stream) {
    if (!points || !plane || !fitness || !inlier_rmse || !n_points || !n_inliers || !best || !status || !ws)
        return fail(-1, "plane_ransac: null argument");
    if (B < 1 || N < 1) return fail(-2, "plane_ransac: B = %d, N = %d must both be >= 1", B, N);
    if (hypotheses < 1 || hypotheses > GECCO_PLANE_RANSAC_MAX_HYPOTHESES)
        return fail(-2, "plane_ransac: hypotheses = %d is not in 1 .. %d", hypotheses, GECCO_PLANE_RANSAC_MAX_HYPOTHESES);
    if (refine_passes < 0 || refine_passes > GECCO_PLANE_RANSAC_MAX_REFINE)
        return fail(-2, "plane_ransac: refine_passes = %d is not in 0 .. %d", refine_passes, GECCO_PLANE_RANSAC_MAX_REFINE);
    if (!finite_positive(r)) return fail(-2, "plane_ransac: r = %g must be a finite number > 0", (double)r);
    if (min_inliers < 0) return fail(-2, "plane_ransac: min_inliers = %d must be >= 0", min_inliers);
    if (axis && (!(cos2 >= 0.0) || !(cos2 <= 1.0))) return fail(-2, "plane_ransac: cos2 = %g is not in 0 .. 1", cos2);
    const int rc = plane_ransac_launch(points, mask, r, hypotheses, refine_passes, (unsigned long long)seed, axis, cos2, min_inliers, viewpoint,
                                       candidates, plane, fitness, inlier_rmse, n_points, n_inliers, best, status, inliers, hyp_triple,
                                       hyp_plane, hyp_count, hyp_sum, ws, B, N, (hipStream_t)stream);
    if (rc == -3) return fail(-2, "plane_ransac: the grid for B = %d, hypotheses = %d passes 2^31 - 1 workgroups", B, hypotheses);
    TRY(rc, "plane_ransac");
    return 0;
}

// voxel-grid downsampling (voxel.hip).  origin null: 0; first, count, inverse nullable
size_t gecco_voxel_workspace_bytes(int B, int N) {
    if (B < 1 || N < 1 || N > GECCO_VOXEL_MAX_POINTS) return 0;
    return GECCO_VOXEL_WORKSPACE_BYTES(B, N);
}
int gecco_voxel_downsample_f32(const float* points, const float* origin, float voxel_size, float* centroids, int32_t* first, int32_t* count,
                               int32_t* inverse, int32_t* n_voxels, void* workspace, int B, int N, int max_voxels, void* stream) {
    if (!points || !centroids || !n_voxels || !workspace) return fail(-1, "voxel_downsample: null argument");
    if (B < 1 || N < 1) return fail(-2, "voxel_downsample: B = %d, N = %d must both be >= 1", B, N);
    if (N > GECCO_VOXEL_MAX_POINTS) return fail(-2, "voxel_downsample: N = %d above %d", N, GECCO_VOXEL_MAX_POINTS);
    if (max_voxels < 1 || max_voxels > N) return fail(-2, "voxel_downsample: max_voxels = %d is not in 1 .. N = %d", max_voxels, N);
    if (!finite_positive(voxel_size))
        return fail(-2, "voxel_downsample: voxel_size = %g must be a finite number > 0", (double)voxel_size);
    const int rc = voxel_launch(points, origin, voxel_size, centroids, first, count, inverse, n_voxels, workspace, B, N, max_voxels,
                                (hipStream_t)stream);
    if (rc == -3) return fail(-2, "voxel_downsample: the grid for B = %d, N = %d passes 2^31 - 1 workgroups", B, N);
    TRY(rc, "voxel_downsample");
    return 0;
}

// DBSCAN clustering (dbscan.hip).  eps2 = fp32(eps * eps) from the caller; count, rounds nullable
size_t gecco_dbscan_workspace_bytes(int B, int N, int max_rounds) {
    if (B < 1 || N < 1 || max_rounds < 0 || max_rounds > GECCO_DBSCAN_MAX_ROUNDS) return 0;
    return GECCO_DBSCAN_WORKSPACE_BYTES(B, N, max_rounds);
}
int gecco_dbscan_f32(const float* points, int32_t* labels, int32_t* n_clusters, int32_t* count, int32_t* rounds, int32_t* status, void* ws,
                     int B, int N, float eps2, int min_points, int max_rounds, void* stream) {
    if (!points || !labels || !n_clusters || !status || !ws) return fail(-1, "dbscan: null argument");
    if (B < 1 || N < 1) return fail(-2, "dbscan: B = %d, N = %d must both be >= 1", B, N);
    if (!finite_positive(eps2)) return fail(-2, "dbscan: eps2 = %g must be a finite number > 0", (double)eps2);
    if (min_points < 1) return fail(-2, "dbscan: min_points = %d must be >= 1", min_points);
    if (max_rounds < 0 || max_rounds > GECCO_DBSCAN_MAX_ROUNDS)
        return fail(-2, "dbscan: max_rounds = %d is not in 0 .. %d", max_rounds, GECCO_DBSCAN_MAX_ROUNDS);
    const int rc = dbscan_launch(points, labels, n_clusters, count, rounds, status, ws, B, N, eps2, min_points, max_rounds, (hipStream_t)stream);
    if (rc == -3) return fail(-2, "dbscan: the grid for B = %d, N = %d passes 2^31 - 1 workgroups", B, N);
    TRY(rc, "dbscan");
    return 0;
}

// fixed-radius neighbour search (radius.hip).  radius2 = fp32(r * r) from the caller.  Every refusal is -2, null pointers included
static int radius_common(const char* who, int B, int M, int N, float radius2, int exclude_self) {
    if (B < 1 || M < 1 || N < 1) return fail(-2, "%s: B = %d, M = %d, N = %d must all be >= 1", who, B, M, N);
    if (!finite_positive(radius2)) return fail(-2, "%s: radius2 = %g must be a finite number > 0", who, (double)radius2);
    if (exclude_self && M != N)
        return fail(-2, "%s: exclude_self needs the query cloud to be the reference cloud (M = %d, N = %d)", who, M, N);
    return 0;
}
int gecco_radius_count_f32(const float* query, const float* ref, int32_t* count, int B, int M, int N, float radius2, int exclude_self,
                           void* stream) {
    if (!query || !ref || !count) return fail(-2, "radius_count: null argument");
    if (const int bad = radius_common("radius_count", B, M, N, radius2, exclude_self)) return bad;
    const int rc = radius_launch(query, ref, nullptr, nullptr, nullptr, count, B, M, N, radius2, exclude_self ? 1 : 0, 0, (hipStream_t)stream);
    if (rc == -3) return fail(-3, "radius_count: the grid for B = %d, M = %d, N = %d passes 2^31 - 1 workgroups", B, M, N);
    TRY(rc, "radius_count");
    return 0;
}
int gecco_radius_search_f32(const float* query, const float* ref, const int64_t* row_start, int32_t* idx, float* d2, int32_t* count, int B, int M,
                            int N, float radius2, int exclude_self, int max_neighbors, void* stream) {
    if (!query || !ref || !idx) return fail(-2, "radius_search: null argument");
    if (const int bad = radius_common("radius_search", B, M, N, radius2, exclude_self)) return bad;
    if (row_start ? max_neighbors != 0 : max_neighbors < 1)
        return fail(-2, "radius_search: max_neighbors = %d must be 0 with row_start (the CSR form) and >= 1 without (the fixed-width form)",
                    max_neighbors);
    static_assert(sizeof(long long) == sizeof(int64_t), "row_start is read as long long");
    const int rc = radius_launch(query, ref, reinterpret_cast<const long long*>(row_start), idx, d2, row_start ? nullptr : count, B, M, N,
                                 radius2, exclude_self ? 1 : 0, max_neighbors, (hipStream_t)stream);
    if (rc == -3) return fail(-3, "radius_search: the grid for B = %d, M = %d, N = %d passes 2^31 - 1 workgroups", B, M, N);
    TRY(rc, "radius_search");
    return 0;
}

// the uniform-grid index of the fixed-radius search (grid.hip).  Every refusal is -2, null pointers included
static int grid_cell_size(const char* who, float cell_size) {
    if (!finite_positive(cell_size) || !finite_positive(1.0f / cell_size))
        return fail(-2, "%s: cell_size = %g must be a finite number > 0 with a finite reciprocal", who, (double)cell_size);
    return 0;
}
static int grid_points(const char* who, int B, int N) {
    if (B < 1 || N < 1) return fail(-2, "%s: B = %d, N = %d must both be >= 1", who, B, N);
    if (N > GECCO_VOXEL_MAX_POINTS) return fail(-2, "%s: N = %d above %d", who, N, GECCO_VOXEL_MAX_POINTS);
    return 0;
}
int gecco_grid_keys_f32(const float* points, const float* origin, float cell_size, int64_t* keys, int B, int N, void* stream) {
    if (!points || !keys) return fail(-2, "grid_keys: null argument");
    if (const int bad = grid_points("grid_keys", B, N)) return bad;
    if (const int bad = grid_cell_size("grid_keys", cell_size)) return bad;
    static_assert(sizeof(long long) == sizeof(int64_t), "keys are written as long long");
    const int rc = grid_keys_launch(points, origin, cell_size, reinterpret_cast<long long*>(keys), B, N, (hipStream_t)stream);
    if (rc == -3) return fail(-3, "grid_keys: the grid for B = %d, N = %d passes 2^31 - 1 workgroups", B, N);
    TRY(rc, "grid_keys");
    return 0;
}
int gecco_grid_build_f32(const float* points, const int64_t* sorted_keys, const int32_t* perm, float* sorted, int64_t* table_keys,
                         int32_t* table_range, int32_t* n_in_grid, int B, int N, void* stream) {
    if (!points || !sorted_keys || !perm || !sorted || !table_keys || !table_range || !n_in_grid) return fail(-2, "grid_build: null argument");
    if (const int bad = grid_points("grid_build", B, N)) return bad;
    const int rc = grid_build_launch(points, reinterpret_cast<const long long*>(sorted_keys), perm, sorted,
                                     reinterpret_cast<long long*>(table_keys), table_range, n_in_grid, B, N, (hipStream_t)stream);
    if (rc == -3) return fail(-3, "grid_build: the grid for B = %d, N = %d passes 2^31 - 1 workgroups", B, N);
    TRY(rc, "grid_build");
    return 0;
}
// a radius2 (finite and > 0: checked by the caller) the index's cells serve: not above fp32(cell_size^2), grid_walk.h's grid_radius2_ok
static int grid_radius2_fits(const char* who, const char* name, float cell_size, float radius2) {
    if (!(radius2 <= cell_size * cell_size))
        return fail(-2, "%s: %s = %g is above cell_size^2 = %g: build an index with a larger cell", who, name, (double)radius2,
                    (double)(cell_size * cell_size));
    return 0;
}
// The built index of an entry point that reads one, as the launchers take it (kernels.h's GridIndexArgs), behind the checks every such
// entry makes of it: the four required pointers, grid_points and grid_cell_size.  The two radius entries call radius_common first, which
// leaves grid_points only N's upper bound to refuse
static int grid_index(const char* who, const float* sorted, const int64_t* table_keys, const int32_t* table_range, const int32_t* n_in_grid,
                      const float* origin, float cell_size, int B, int N, GridIndexArgs& index) {
    if (!sorted || !table_keys || !table_range || !n_in_grid) return fail(-2, "%s: null argument", who);
    if (const int bad = grid_points(who, B, N)) return bad;
    if (const int bad = grid_cell_size(who, cell_size)) return bad;
    static_assert(sizeof(long long) == sizeof(int64_t), "table_keys are read as long long");
    index = GridIndexArgs{sorted, reinterpret_cast<const long long*>(table_keys), table_range, n_in_grid, origin, cell_size};
    return 0;
}
int gecco_grid_radius_count_f32(const float* query, const int32_t* qorder, const float* sorted, const int64_t* table_keys,
                                const int32_t* table_range, const int32_t* n_in_grid, const float* origin, float cell_size, int32_t* count,
                                int B, int M, int N, float radius2, int exclude_self, void* stream) {
    if (!query || !count) return fail(-2, "grid_radius_count: null argument");
    if (const int bad = radius_common("grid_radius_count", B, M, N, radius2, exclude_self)) return bad;
    GridIndexArgs index;
    if (const int bad = grid_index("grid_radius_count", sorted, table_keys, table_range, n_in_grid, origin, cell_size, B, N, index)) return bad;
    if (const int bad = grid_radius2_fits("grid_radius_count", "radius2", cell_size, radius2)) return bad;
    const int rc = grid_radius_launch(query, qorder, index, nullptr, nullptr, nullptr, count, B, M, N, radius2, exclude_self ? 1 : 0,
                                      (hipStream_t)stream);
    if (rc == -3) return fail(-3, "grid_radius_count: the grid for B = %d, M = %d passes 2^31 - 1 workgroups", B, M);
    TRY(rc, "grid_radius_count");
    return 0;
}
int gecco_grid_radius_search_f32(const float* query, const int32_t* qorder, const float* sorted, const int64_t* table_keys,
                                 const int32_t* table_range, const int32_t* n_in_grid, const float* origin, float cell_size,
                                 const int64_t* row_start, int32_t* idx, float* d2, int B, int M, int N, float radius2, int exclude_self,
                                 void* stream) {
    if (!query || !row_start || !idx) return fail(-2, "grid_radius_search: null argument");
    if (const int bad = radius_common("grid_radius_search", B, M, N, radius2, exclude_self)) return bad;
    GridIndexArgs index;
    if (const int bad = grid_index("grid_radius_search", sorted, table_keys, table_range, n_in_grid, origin, cell_size, B, N, index)) return bad;
    if (const int bad = grid_radius2_fits("grid_radius_search", "radius2", cell_size, radius2)) return bad;
    const int rc = grid_radius_launch(query, qorder, index, reinterpret_cast<const long long*>(row_start), idx, d2, nullptr, B, M, N, radius2,
                                      exclude_self ? 1 : 0, (hipStream_t)stream);
    if (rc == -3) return fail(-3, "grid_radius_search: the grid for B = %d, M = %d passes 2^31 - 1 workgroups", B, M);
    TRY(rc, "grid_radius_search");
    return 0;
}

// ISS keypoints on the grid index (iss.hip).  Every refusal is -2, null pointers included; eigenvalues, counts and origin nullable
static int iss_radius2(const char* name, float cell_size, float radius2) {
    if (!finite_positive(radius2)) return fail(-2, "iss_keypoints: %s = %g must be a finite number > 0", name, (double)radius2);
    return grid_radius2_fits("iss_keypoints", name, cell_size, radius2);
}
int gecco_iss_keypoints_f32(const float* sorted, const int64_t* table_keys, const int32_t* table_range, const int32_t* n_in_grid,
                            const float* origin, float cell_size, double* saliency, double* eigenvalues, int32_t* counts, uint8_t* mask, int B,
                            int N, float salient_radius2, float non_max_radius2, double gamma_21, double gamma_32, int min_neighbors,
                            void* stream) {
    if (!saliency || !mask) return fail(-2, "iss_keypoints: null argument");
    GridIndexArgs index;
    if (const int bad = grid_index("iss_keypoints", sorted, table_keys, table_range, n_in_grid, origin, cell_size, B, N, index)) return bad;
    if (const int bad = iss_radius2("salient_radius2", cell_size, salient_radius2)) return bad;
    if (const int bad = iss_radius2("non_max_radius2", cell_size, non_max_radius2)) return bad;
    if (!(gamma_21 > 0.0) || !(gamma_21 <= 1.7976931348623157e308) || !(gamma_32 > 0.0) || !(gamma_32 <= 1.7976931348623157e308))
        return fail(-2, "iss_keypoints: gamma_21 = %g and gamma_32 = %g must be finite numbers > 0", gamma_21, gamma_32);
    if (min_neighbors < 1) return fail(-2, "iss_keypoints: min_neighbors = %d must be >= 1", min_neighbors);
    const int rc = iss_launch(index, saliency, eigenvalues, counts, mask, B, N, salient_radius2, non_max_radius2, gamma_21, gamma_32,
                              min_neighbors, (hipStream_t)stream);
    if (rc == -3) return fail(-3, "iss_keypoints: the grid for B = %d, N = %d passes 2^31 - 1 workgroups", B, N);
    TRY(rc, "iss_keypoints");
    return 0;
}

// Normals from radius neighbourhoods on the grid index (normals_grid.hip).  Every refusal is -2, null pointers included; qorder, origin,
// viewpoint, eigenvalues, curvature and counts nullable
int gecco_normals_grid_f32(const float* query, const int32_t* qorder, const float* sorted, const int64_t* table_keys,
                           const int32_t* table_range, const int32_t* n_in_grid, const float* origin, float cell_size, const float* viewpoint,
                           float radius2, int min_neighbors, float* normals, double* eigenvalues, double* curvature, int32_t* counts, int B,
                           int M, int N, void* stream) {
    if (!query || !normals) return fail(-2, "normals_grid: null argument");
    if (const int bad = radius_common("normals_grid", B, M, N, radius2, 0)) return bad;
    GridIndexArgs index;
    if (const int bad = grid_index("normals_grid", sorted, table_keys, table_range, n_in_grid, origin, cell_size, B, N, index)) return bad;
    if (const int bad = grid_radius2_fits("normals_grid", "radius2", cell_size, radius2)) return bad;
    if (min_neighbors < 1) return fail(-2, "normals_grid: min_neighbors = %d must be >= 1", min_neighbors);
    const int rc = normals_grid_launch(query, qorder, index, viewpoint, radius2, min_neighbors, normals, eigenvalues, curvature, counts, B, M, N,
                                       (hipStream_t)stream);
    if (rc == -3) return fail(-3, "normals_grid: the grid for B = %d, M = %d passes 2^31 - 1 workgroups", B, M);
    TRY(rc, "normals_grid");
    return 0;
}

// FPFH from radius neighbourhoods on the grid index (fpfh_grid.hip).  Every refusal is -2, null pointers included; origin nullable; spfh
// and count are required (the first launch's outputs, read by the second)
int gecco_fpfh_grid_f32(const float* normals, const float* sorted, const int64_t* table_keys, const int32_t* table_range,
                        const int32_t* n_in_grid, const float* origin, float cell_size, float radius2, float* fpfh, float* spfh, int32_t* count,
                        int B, int N, void* stream) {
    if (!normals || !fpfh || !spfh || !count) return fail(-2, "fpfh_grid: null argument");
    GridIndexArgs index;
    if (const int bad = grid_index("fpfh_grid", sorted, table_keys, table_range, n_in_grid, origin, cell_size, B, N, index)) return bad;
    if (!finite_positive(radius2)) return fail(-2, "fpfh_grid: radius2 = %g must be a finite number > 0", (double)radius2);
    if (const int bad = grid_radius2_fits("fpfh_grid", "radius2", cell_size, radius2)) return bad;
    const int rc = fpfh_grid_launch(normals, index, radius2, fpfh, spfh, count, B, N, (hipStream_t)stream);
    if (rc == -3) return fail(-3, "fpfh_grid: the grid for B = %d, N = %d passes 2^31 - 1 workgroups", B, N);
    TRY(rc, "fpfh_grid");
    return 0;
}

// DBSCAN on the grid index (dbscan.hip's grid form): gecco_dbscan_f32's outputs and workspace, the index through grid_index as every
// entry above.  It stands here, behind the grid entries, for their checks.  Every refusal is -2, null pointers included
int gecco_dbscan_grid_f32(const float* sorted, const int64_t* table_keys, const int32_t* table_range, const int32_t* n_in_grid,
                          const float* origin, float cell_size, int32_t* labels, int32_t* n_clusters, int32_t* count, int32_t* rounds,
                          int32_t* status, void* ws, int B, int N, float eps2, int min_points, int max_rounds, void* stream) {
    if (!labels || !n_clusters || !status || !ws) return fail(-2, "dbscan_grid: null argument");
    GridIndexArgs index;
    if (const int bad = grid_index("dbscan_grid", sorted, table_keys, table_range, n_in_grid, origin, cell_size, B, N, index)) return bad;
    if (!finite_positive(eps2)) return fail(-2, "dbscan_grid: eps2 = %g must be a finite number > 0", (double)eps2);
    if (const int bad = grid_radius2_fits("dbscan_grid", "eps2", cell_size, eps2)) return bad;
    if (min_points < 1) return fail(-2, "dbscan_grid: min_points = %d must be >= 1", min_points);
    if (max_rounds < 0 || max_rounds > GECCO_DBSCAN_MAX_ROUNDS)
        return fail(-2, "dbscan_grid: max_rounds = %d is not in 0 .. %d", max_rounds, GECCO_DBSCAN_MAX_ROUNDS);
    const int rc = dbscan_grid_launch(index, labels, n_clusters, count, rounds, status, ws, B, N, eps2, min_points, max_rounds,
                                      (hipStream_t)stream);
    if (rc == -3) return fail(-3, "dbscan_grid: the grid for B = %d, N = %d passes 2^31 - 1 workgroups", B, N);
    TRY(rc, "dbscan_grid");
    return 0;
}

}  // extern "C"
