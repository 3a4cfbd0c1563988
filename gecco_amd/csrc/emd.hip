// Exact earth mover's distance between two clouds of N points each, on the device (gfx950): an epsilon-scaling auction
// (Bertsekas) for the square assignment problem, one workgroup per pair of clouds.
//
// Reference: gecco-jax/src/gecco_jax/metrics.py:114-142 (`_scipy_lsa`, `scipy_emd`): scipy's linear_sum_assignment on the
// (N, N) distance matrix, then the mean of a second distance along the assignment ("match with one cost, average another").
//
// Costs.  c_ij = pair_dist(a_i, b_j) (pair_dist.h: the formula gecco_distance_matrix_f32 writes), l1 or squared (l2).  They
// are never stored: every one is recomputed from the coordinates in LDS when it is needed.
//
// Exactness.  The match cost is quantised to integers k_ij = rint(c_ij * s), s = 2^Q / c_max, Q = EMD_Q = 24, where
//     c_max = 2^e with e = the frexp exponent of max_ij c_ij (max c < c_max <= 2 max c), and e >= -100 (also when max c = 0).
// s is then a power of two: c * s is exact in fp32 and 0 <= k_ij <= 2^24.  The integer problem is solved exactly: the costs
// are scaled by N + 1 (K = k (N + 1)) and the epsilon-scaling ends at epsilon = 1, where epsilon-complementary slackness
// puts the assignment within N < N + 1 of the optimum of K, i.e. at the optimum of k.  Since |c - k / s| <= 1 / (2 s), the
// returned assignment's true match cost exceeds the fp32-cost optimum by at most
//     N * c_max * 2^-Q   in total   (a mean gap of at most c_max * 2^-24 per row).
// Prices are int64.  A bid is the new price of its object, p_j + (second best - best) + epsilon > p_j >= 0; every price
// stays below the phase-start maximum + K range + epsilon per phase (an object nobody has bid on yet in the phase bounds
// the second best), so after the ~12 phases every price is below 2^41 and a bid fits the 53 high bits of a bid word.
//
// Determinism.  Synchronous (Jacobi) bidding rounds: every unassigned person bids against the same prices (one wave per
// person, its lanes over the objects), the bids meet in an LDS 64-bit max on (bid << 11 | 2047 - person) per object — the
// highest bid wins, ties go to the lower person — then a barrier, the winners take their objects, the previous owners
// become unassigned, a barrier, the next round.  The outcome of a round depends on the set of unassigned persons and on the
// prices alone, not on the order in which waves ran or appended to the list, so value and assignment are the same bits run to
// run and in any batch position.
//
// Termination.  Every loop is bounded: a non-finite coordinate (or a cloud whose |p|^2 or costs overflow fp32) ends the
// pair with status 1 before any bidding; more than `max_rounds` bidding rounds in all phases end it with status 2.  Both
// write NaN and an assignment of -1.  Only workgroup barriers and LDS are used: no workgroup waits on another.
//
// Value.  out = mean_i d_avg(a_i, b_assign(i)) with d_avg = pair_dist (l1 or squared), summed in fp64 in a fixed order
// (per-thread strides, a fixed butterfly, the waves in order) and rounded to fp32.
#include "../../include/gecco_hip.h"
#include "common.h"
#include "kernels.h"
#include "launch_state.h"
#include "pair_dist.h"

namespace {

constexpr int EMD_MAX_N = GECCO_EMD_MAX_POINTS;     // 11 bits of person index in a bid word
constexpr int EMD_Q = GECCO_EMD_Q;
constexpr int EMD_THREADS = 1024;
constexpr int EMD_WAVES = EMD_THREADS / 64;
constexpr long long EMD_ALPHA = 8;                  // epsilon divisor between phases
constexpr size_t EMD_LDS_PER_POINT = 2 * 8 + 2 * 16 + 3 * 4;   // price, bid word, a and b (x, y, z, |p|^2), owner, assignment, list
static_assert(EMD_MAX_N == 2048, "bid words carry 11 bits of person index");

__global__ __launch_bounds__(EMD_THREADS) void emd_auction_kernel(const float* __restrict__ A, const float* __restrict__ Bc, float* __restrict__ out,
                                                                  int* __restrict__ assign, int* __restrict__ status, int N, int T, int set_mode,
                                                                  int match_sq, int avg_sq, int max_rounds) {
    extern __shared__ __attribute__((aligned(16))) unsigned char emd_lds[];
    long long* price = reinterpret_cast<long long*>(emd_lds);
    unsigned long long* bidw = reinterpret_cast<unsigned long long*>(price + N);
    f32x4* pa = reinterpret_cast<f32x4*>(bidw + N);
    f32x4* pb = pa + N;
    int* owner = reinterpret_cast<int*>(pb + N);   // object -> person (-1: free)
    int* asg = owner + N;                          // person -> object (-1: unassigned)
    int* list = asg + N;                           // the unassigned persons of the round
    __shared__ int s_bad, s_cnt;
    __shared__ unsigned s_maxc;
    __shared__ double s_red[EMD_WAVES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pair = blockIdx.x;                   // = s * T + t in set mode
    const int sa = set_mode ? pair / T : pair, sb = set_mode ? pair % T : pair;
    const float* a = A + (size_t)sa * N * 3;
    const float* b = Bc + (size_t)sb * N * 3;
    if (tid == 0) { s_bad = 0; s_maxc = 0u; }
    __syncthreads();
    for (int i = tid; i < N; i += EMD_THREADS) {
        const float ax = a[3 * i], ay = a[3 * i + 1], az = a[3 * i + 2], aa = sq_norm(ax, ay, az);
        const float bx = b[3 * i], by = b[3 * i + 1], bz = b[3 * i + 2], bb = sq_norm(bx, by, bz);
        if (!__builtin_isfinite(aa) || !__builtin_isfinite(bb) || !__builtin_isfinite(ax + ay + az) || !__builtin_isfinite(bx + by + bz))
            s_bad = 1;
        pa[i] = f32x4{ax, ay, az, aa};
        pb[i] = f32x4{bx, by, bz, bb};
        asg[i] = N == 1 ? 0 : -1;
    }
    __syncthreads();
    int st = s_bad;
    // max_ij c_ij: non-negative floats order like their bit patterns, so an unsigned LDS max is exact and order-free
    if (!st) {
        float mx = 0.f;
        for (int i = wave; i < N; i += EMD_WAVES) {
            const f32x4 p = pa[i];
            for (int j = lane; j < N; j += 64) {
                const f32x4 o = pb[j];
                mx = fmaxf(mx, pair_dist(p[0], p[1], p[2], p[3], o[0], o[1], o[2], o[3], match_sq != 0));
            }
        }
        for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        if (lane == 0) atomicMax(&s_maxc, __float_as_uint(mx));
    }
    __syncthreads();
    const float maxc = __uint_as_float(s_maxc);
    if (!st && !__builtin_isfinite(maxc)) st = 1;
    int e = 0;
    (void)frexpf(maxc, &e);
    e = max(e, -100);
    const float sc = ldexpf(1.f, EMD_Q - e);       // 2^Q / c_max, a power of two
    const long long NP1 = N + 1;

    if (!st && N > 1) {
        const long long kmax = (long long)rintf(maxc * sc) * NP1;
        long long eps = max(1LL, kmax / EMD_ALPHA);
        int rounds = 0;
        for (int j = tid; j < N; j += EMD_THREADS) price[j] = 0;
        for (;;) {                                 // epsilon phases: at most ~12 (Q + log2(N + 1) bits, 3 per phase)
            for (int i = tid; i < N; i += EMD_THREADS) { asg[i] = -1; owner[i] = -1; bidw[i] = 0ull; list[i] = i; }
            __syncthreads();
            int u = N;
            while (u > 0) {                        // bidding rounds: u, rounds and st are the same in every thread
                if (++rounds > max_rounds) { st = 2; break; }
                for (int q = wave; q < u; q += EMD_WAVES) {
                    const int i = list[q];
                    const f32x4 p = pa[i];
                    long long m1 = __LONG_LONG_MAX__, m2 = __LONG_LONG_MAX__;
                    int j1 = 0;
                    for (int j = lane; j < N; j += 64) {
                        const f32x4 o = pb[j];
                        const float c = pair_dist(p[0], p[1], p[2], p[3], o[0], o[1], o[2], o[3], match_sq != 0);
                        const long long v = (long long)(int)rintf(c * sc) * NP1 + price[j];
                        if (v < m1) { m2 = m1; m1 = v; j1 = j; }
                        else if (v < m2) m2 = v;
                    }
                    for (int off = 32; off > 0; off >>= 1) {
                        const long long o1 = __shfl_xor(m1, off, 64), o2 = __shfl_xor(m2, off, 64);
                        const int oj = __shfl_xor(j1, off, 64);
                        m2 = min(min(m2, o2), max(m1, o1));
                        if (o1 < m1 || (o1 == m1 && oj < j1)) { m1 = o1; j1 = oj; }
                    }
                    if (lane == 0) {
                        const long long bid = price[j1] + (m2 - m1) + eps;
                        atomicMax(&bidw[j1], ((unsigned long long)bid << 11) | (unsigned long long)(EMD_MAX_N - 1 - i));
                    }
                }
                __syncthreads();
                if (tid == 0) s_cnt = 0;           // every thread read the previous count before the barrier above
                for (int j = tid; j < N; j += EMD_THREADS) {
                    const unsigned long long w = bidw[j];
                    if (w) {
                        const int i = EMD_MAX_N - 1 - (int)(w & (EMD_MAX_N - 1)), o = owner[j];
                        if (o >= 0) asg[o] = -1;   // an owner never bids: o is no winner of this round
                        owner[j] = i;
                        asg[i] = j;
                        price[j] = (long long)(w >> 11);
                        bidw[j] = 0ull;
                    }
                }
                __syncthreads();
                for (int i = tid; i < N; i += EMD_THREADS)
                    if (asg[i] < 0) list[atomicAdd(&s_cnt, 1)] = i;
                __syncthreads();
                u = s_cnt;
            }
            if (st || eps == 1) break;
            eps = max(1LL, eps / EMD_ALPHA);
        }
    }

    double acc = 0.0;
    if (!st)
        for (int i = tid; i < N; i += EMD_THREADS) {
            const f32x4 p = pa[i], o = pb[asg[i]];
            acc += (double)pair_dist(p[0], p[1], p[2], p[3], o[0], o[1], o[2], o[3], avg_sq != 0);
        }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) s_red[wave] = acc;
    if (assign)
        for (int i = tid; i < N; i += EMD_THREADS) assign[(size_t)pair * N + i] = st ? -1 : asg[i];
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int w = 0; w < EMD_WAVES; ++w) total += s_red[w];
        out[pair] = st ? __builtin_nanf("") : (float)(total / N);
        status[pair] = st;
    }
}

}  // namespace

// pairs workgroups; set_mode == 0: pair p is (A[p], B[p]); set_mode != 0: pair p = s * T + t is (A[s], B[t])
int emd_auction_launch(const float* A, const float* Bc, float* out, int* assign, int* status, int pairs, int T, int set_mode, int N,
                       int match_sq, int avg_sq, int max_rounds, hipStream_t st) {
    if (pairs <= 0 || N < 1 || N > EMD_MAX_N || (set_mode && T <= 0) || max_rounds < 1) return -2;
    if (const hipError_t e = lds_opt_in<emd_auction_kernel>(EMD_LDS_PER_POINT * EMD_MAX_N)) return (int)e;
    hipLaunchKernelGGL(emd_auction_kernel, dim3(pairs), dim3(EMD_THREADS), EMD_LDS_PER_POINT * N, st, A, Bc, out, assign, status, N, T,
                       set_mode, match_sq, avg_sq, max_rounds);
    return (int)hipGetLastError();
}
