// k-nearest-neighbour search between 3-D clouds on the device (gfx950): for every query q_i of (B, M, 3) the k points of the reference
// cloud (B, N, 3) of the same batch element that are nearest to it.  The reference has no neighbourhood query at all; the only route
// without this file is a materialised M x N distance matrix and a top-k over it.
//
// Definition (gecco_knn_f32, include/gecco_hip.h; tests/_knn_ref.py restates it in numpy float32).  dist2(q, p) = (dx dx + dy dy) + dz dz
// on the coordinate differences, every operation rounded to fp32 and none contracted into an FMA (cloud_dist2 of cloud_nn.h spells the
// roundings out); a NaN dist2 is replaced by +inf; the pairs of query i are ordered by (dist2, j) ascending — equal distances go to
// the LOWEST index — and the first k of them are the result.  Self mode skips the pair j == i by index.
//
// One 64-bit key per pair: dist2's bits in the high word (dist2 >= 0 or +inf, so they order as unsigned integers) and j in the low
// word.  The k smallest keys of a set do not depend on the order the set is visited in, so both forms give the same bits, run to run
// and in any batch position: no float atomics, no atomics at all, and no workgroup waits on another.
//
// The list.  A thread owns one query and keeps its k best keys UNSORTED in LDS, slot t of thread tid at list[t * T + tid] (consecutive
// lanes on consecutive 8-byte words: no bank conflicts), and in registers the largest key of the list (`worst`) and its slot.  A
// candidate no better than `worst` costs one compare and touches nothing.  A better one overwrites the worst slot and the list is
// re-scanned for the new worst: k independent LDS reads, no shifting.  Empty slots hold KNN_EMPTY = ~0, above every key.  In a scan j
// ascends, so a candidate with dist2 equal to the worst's has the higher index and loses: the compare is on dist2's 32 bits alone.
// At the end slot t goes to output position rank(t) = the number of keys below it (keys are distinct: k * k compares, no sort).
//
// Scan kernel.  A workgroup of T = 64, 128 or 256 threads (T queries) walks the points [lo, hi) of the reference cloud in tiles of
// CLOUD_TILE = 512 points staged in LDS as (x, y, z, 0); the next tile is fetched into registers while this one is scanned.  Every lane
// reads the same tile entry (a broadcast read), four candidates per step: eight subtractions / products / sums and one min (NaN ->
// +inf) each, one min over the four and ONE branch; only a step that holds a winner for some lane looks at its four candidates singly.
// "direct" form: one launch, [lo, hi) = the whole cloud, results written from the list.
// "split" form: the cloud is cut into S slices of GECCO_KNN_SPLIT_SLICE points, the grid is (cloud, query tile, slice), every list goes
// as it is (k keys, empty slots included) to the workspace ws[((b * S + s) * k + t) * M + i]; a second launch (knn_merge_kernel) pushes
// the S * k keys of a query through the same list (full 64-bit compare: slices arrive unsorted) and writes the results.  Both launches
// are ordinary grids; every workspace word the merge reads was written by the first launch.
#include "cloud_nn.h"
#include "kernels.h"
#include "launch_state.h"

namespace {

typedef unsigned long long knn_key;
constexpr knn_key KNN_EMPTY = ~0ull;
static_assert(8 * 256 * 16 <= 32 * 1024 && 8 * 128 * 32 <= 32 * 1024 && 8 * 64 * GECCO_KNN_MAX_K <= 32 * 1024,
              "the lists of a workgroup take at most 32 KiB of LDS (cloud_max_threads)");

// the running k-best list of one thread: `list` points at slot 0 of this thread, slots are T words apart
template <int T>
struct KnnList {
    knn_key* list;
    knn_key worst;
    int slot, k;
    __device__ __forceinline__ void init(knn_key* l, int kk) {
        list = l;
        k = kk;
        for (int t = 0; t < k; ++t) list[t * T] = KNN_EMPTY;
        worst = KNN_EMPTY;
        slot = 0;
    }
    __device__ __forceinline__ unsigned worst_bits() const { return (unsigned)(worst >> 32); }
    // key < worst: replace the worst and find the new one
    __device__ __forceinline__ void push(knn_key key) {
        list[slot * T] = key;
        knn_key w = 0;
        int s = 0;
#pragma unroll 4
        for (int t = 0; t < k; ++t) {
            const knn_key v = list[t * T];
            if (v > w) {
                w = v;
                s = t;
            }
        }
        worst = w;
        slot = s;
    }
    // slot t -> output position = the number of keys below it (distinct keys: a permutation of 0 .. k-1)
    __device__ __forceinline__ void emit(int* __restrict__ idx, float* __restrict__ d2) const {
        for (int t = 0; t < k; ++t) {
            const knn_key v = list[t * T];
            int rank = 0;
#pragma unroll 4
            for (int u = 0; u < k; ++u) rank += list[u * T] < v ? 1 : 0;
            idx[rank] = (int)(unsigned)(v & 0xffffffffu);
            if (d2) d2[rank] = __uint_as_float((unsigned)(v >> 32));
        }
    }
};

// grid: B * tiles * S blocks, block (b, tile, s) scans points [s * slice, min(N, (s + 1) * slice)) for queries tile * T .. + T - 1.
// ws == null: S == 1, results to idx / d2.  ws != null: the raw lists to ws.
template <int T>
__global__ __launch_bounds__(T) void knn_scan_kernel(const float* __restrict__ query, const float* __restrict__ ref, int* __restrict__ idx,
                                                     float* __restrict__ d2, knn_key* __restrict__ ws, int M, int N, int k, int exclude_self,
                                                     int tiles, int S, unsigned slice) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
    __shared__ __attribute__((aligned(16))) f32x4 tile[CLOUD_TILE];

    const int tid = threadIdx.x;
    const unsigned bid = blockIdx.x;
    const int s = (int)(bid % (unsigned)S), qt = (int)((bid / (unsigned)S) % (unsigned)tiles), b = (int)(bid / (unsigned)S / (unsigned)tiles);
    const unsigned lo = (unsigned)s * slice, hi = min((unsigned)N, lo + slice);
    const float* rb = ref + (size_t)b * N * 3;
    const int i = qt * T + tid;
    const bool valid = i < M;
    const float* qp = query + ((size_t)b * M + (valid ? i : 0)) * 3;
    const float qx = qp[0], qy = qp[1], qz = qp[2];
    const unsigned self = exclude_self ? (unsigned)i : 0xffffffffu;   // no j reaches 2^32 - 1

    KnnList<T> best;
    best.init(reinterpret_cast<knn_key*>(knn_lds) + tid, k);

    // (icp_match_kernel has the same loop; cloud_nn.h says why it is written out in both)
    constexpr int PPT = CLOUD_TILE / T;
    float rx[PPT], ry[PPT], rz[PPT];
    auto fetch = [&](unsigned base) {
#pragma unroll
        for (int p = 0; p < PPT; ++p) {
            const unsigned j = base + (unsigned)(tid + p * T);
            const bool in = j < hi;
            rx[p] = in ? rb[3 * (size_t)j] : 0.f;
            ry[p] = in ? rb[3 * (size_t)j + 1] : 0.f;
            rz[p] = in ? rb[3 * (size_t)j + 2] : 0.f;
        }
    };
    auto single = [&](unsigned u, unsigned j) {
        if (u < best.worst_bits() && j != self) best.push(((knn_key)u << 32) | (knn_key)j);
    };

    fetch(lo);
    for (unsigned base = lo; base < hi; base += CLOUD_TILE) {
        __syncthreads();   // the scan of the previous tile is over
#pragma unroll
        for (int p = 0; p < PPT; ++p) tile[tid + p * T] = f32x4{rx[p], ry[p], rz[p], 0.f};
        __syncthreads();
        if (base + CLOUD_TILE < hi) fetch(base + CLOUD_TILE);
        if (!valid) continue;
        const int cnt = (int)min((unsigned)CLOUD_TILE, hi - base);   // entries past cnt are never candidates
        int g = 0;
        for (; g + 4 <= cnt; g += 4) {
            const unsigned u0 = cloud_dist2_bits(qx, qy, qz, tile[g]), u1 = cloud_dist2_bits(qx, qy, qz, tile[g + 1]);
            const unsigned u2 = cloud_dist2_bits(qx, qy, qz, tile[g + 2]), u3 = cloud_dist2_bits(qx, qy, qz, tile[g + 3]);
            if (min(min(u0, u1), min(u2, u3)) < best.worst_bits()) {   // ascending j inside the step
                single(u0, base + g);
                single(u1, base + g + 1);
                single(u2, base + g + 2);
                single(u3, base + g + 3);
            }
        }
        for (; g < cnt; ++g) single(cloud_dist2_bits(qx, qy, qz, tile[g]), base + g);
    }
    if (!valid) return;
    if (ws) {
        knn_key* out = ws + ((size_t)b * S + s) * k * (size_t)M + i;
        for (int t = 0; t < k; ++t) out[(size_t)t * M] = best.list[t * T];
    } else {
        const size_t o = ((size_t)b * M + i) * k;
        best.emit(idx + o, d2 ? d2 + o : nullptr);
    }
}

// grid: B * tiles blocks; a thread merges the S raw lists of its query
template <int T>
__global__ __launch_bounds__(T) void knn_merge_kernel(const knn_key* __restrict__ ws, int* __restrict__ idx, float* __restrict__ d2, int M, int k,
                                                      int tiles, int S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
    const int tid = threadIdx.x;
    const int qt = (int)(blockIdx.x % (unsigned)tiles), b = (int)(blockIdx.x / (unsigned)tiles);
    const int i = qt * T + tid;
    if (i >= M) return;   // (no barrier below)
    KnnList<T> best;
    best.init(reinterpret_cast<knn_key*>(knn_lds) + tid, k);
    const knn_key* in = ws + (size_t)b * S * k * (size_t)M + i;
    const size_t n = (size_t)S * k;
    for (size_t e = 0; e < n; ++e) {
        const knn_key key = in[e * M];
        if (key < best.worst) best.push(key);
    }
    const size_t o = ((size_t)b * M + i) * k;
    best.emit(idx + o, d2 ? d2 + o : nullptr);
}

}  // namespace

// form 0: split when a workspace is there and cloud_plan's rule takes it; 1: direct; 2: split (ws required).  T: the most threads whose
// lists fit 32 KiB, halved by the plan.  Returns -3 when the grid would pass 2^31 - 1 workgroups.
int knn_launch(const float* query, const float* ref, int* idx, float* d2, void* ws, int B, int M, int N, int k, int exclude_self, int form,
               hipStream_t st) {
    if (B < 1 || M < 1 || N < 1 || k < 1 || k > GECCO_KNN_MAX_K || form < 0 || form > 2 || (form == 2 && !ws)) return -2;
    const CloudPlan p = cloud_plan(B, M, N, form, ws != nullptr, cloud_max_threads(k), device_cus());
    if (!p.fits()) return -3;
    knn_key* w = p.split ? static_cast<knn_key*>(ws) : nullptr;
    const size_t lds = (size_t)8 * p.T * k;
    dispatch_T(p.T, [&](auto t) {
        constexpr int T = decltype(t)::value;
        hipLaunchKernelGGL(knn_scan_kernel<T>, dim3((unsigned)p.blocks), dim3(T), lds, st, query, ref, idx, d2, w, M, N, k, exclude_self, p.tiles,
                           p.S, p.S == 1 ? (unsigned)N : (unsigned)GECCO_KNN_SPLIT_SLICE);
        if (w) hipLaunchKernelGGL(knn_merge_kernel<T>, dim3((unsigned)(B * p.tiles)), dim3(T), lds, st, w, idx, d2, M, k, p.tiles, p.S);
    });
    return (int)hipGetLastError();
}
