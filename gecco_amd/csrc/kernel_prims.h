// Device primitives the gfx950 kernels share: vector types, compile-time loops, counted waits, the LDS-DMA piece, lane exchanges and
// whole-wave reductions, fp16 / fp8 / bf16 packing, the E8M0 block scale, and the no-MFMA stand-ins of the diagnostic builds.  ONE
// definition each: several of them are bit-level contracts between kernels (which value is rounded, and how often), and a private copy
// that drifts from its twin is a silent numeric bug.  Everything here is __forceinline__ and lives outside the kernel files' anonymous
// namespaces, so a translation unit that includes two kernel files (tools/probe) still sees each name once.
//
// Kept apart on purpose (similar, not the same function):
//   * split8 (gemm_f32_dma.hip), cvt8 (gemm_f16_dma.hip), cvt4 (gemm_tn_f16.hip): 8-wide / one-plane forms with their own signatures;
//   * w_absmax32 (mlp_fused_w.hip) takes one f16x32 and calls absmax32 on its four quarters;
//   * w_keep6 (mlp_fused_w.hip) also pins the two scale registers, keep8 does not;
//   * wait_lgkm0 (mlp_fused_w.hip) and wait_ahead (gemm_f16_dma.hip) are built on waitcnt_imm for one kernel each;
//   * max_halves / sum_halves (unpool_outproj_h8.hip) reduce over lane ^ 32 only; lanes_sum takes a runtime width, wave_sum is the
//     fixed 64-lane form (fully unrolled, other order of the partial sums);
//   * dma::dma16 (gemm_dma_common.h) is the global_load ... lds form, dma16_buf the buffer_load ... lds form;
//   * tn_off (gemm_tn_x3.hip), toff<NCB> (gemm_tn_f16.hip), blk_off<NB> (attention_bwd_x3.hip), vt_off<DT> (attention_x3.hip) are LDS
//     layouts of their kernels, not primitives;
//   * the *_STAMPS macros differ in table size and slot count and stay in their files.
#pragma once
#include "common.h"

#include <type_traits>
#include <utility>

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x32 __attribute__((ext_vector_type(32)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x6 __attribute__((ext_vector_type(6)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16;

// ---- compile-time loops: f(std::integral_constant<int, I>{}) for I = 0 .. N - 1, so every index inside f is a constant (register
// arrays stay registers, ring slots are static addresses)
template <int... I, class F>
__device__ __forceinline__ void static_for(std::integer_sequence<int, I...>, F&& f) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for(std::make_integer_sequence<int, N>{}, f);
}
// the same with a second compile-time tag handed through (no wrapper lambda around f: the accumulators stay in registers)
template <int TAG, int... I, class F>
__device__ __forceinline__ void static_for_tag(std::integer_sequence<int, I...>, F&& f) {
    (f(std::integral_constant<int, I>{}, std::integral_constant<int, TAG>{}), ...);
}

// ---- counted waits as the s_waitcnt BUILTIN, not inline asm: the compiler's own wait-count scoreboard understands the
// builtin, so after wait_vm_lgkm0 it knows every earlier LDS read has returned and does not put a second
// s_waitcnt lgkmcnt(0) in front of the first MFMA that uses last step's fragments — which would also wait for the
// fragment reads just issued for the NEXT step and expose their whole latency every K-step (it did, with asm).
// gfx9 encoding: vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] | vmcnt[5:4] << 14.
constexpr int waitcnt_imm(int vm, int lgkm) { return (vm & 0xF) | (0x7 << 4) | ((lgkm & 0xF) << 8) | ((vm >> 4) << 14); }
template <int N>
__device__ __forceinline__ void wait_vm() { __builtin_amdgcn_s_waitcnt(waitcnt_imm(N, 0xF)); }
template <int N>
__device__ __forceinline__ void wait_vm_lgkm0() { __builtin_amdgcn_s_waitcnt(waitcnt_imm(N, 0)); }

// this wave's LDS operations have completed (wave-private LDS tiles need no barrier, only this)
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// LDS writes of this wave have landed, then the block barrier (no vmcnt wait: a weight ring stays in flight)
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// ---- one 16-byte-per-lane piece global -> LDS by buffer_load ... lds: the per-lane offset is a register computed once, the stage
// offset a scalar.  (A non-template device function: inside a kernel template the host pass would have to accept the 16-byte form of
// the builtin, which only the gfx950 target has, and drops the whole instantiation without a word.)
__device__ __forceinline__ void dma16_buf(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff, void* lds_wave_base) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds_wave_base, 16, voff, soff, 0, 0);
}
// a 16-byte MFMA fragment out of a u16 plane in LDS
__device__ __forceinline__ u32x4 frag(const u16* p) { return *reinterpret_cast<const u32x4*>(p); }

// ---- lanes
// value of the neighbouring lane (lane ^ 1): one DPP move (quad_perm [1, 0, 3, 2])
__device__ __forceinline__ unsigned swap_pair(unsigned v) {
    return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);
}
// over the 64 lanes of the wave: every lane gets the result
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// over `width` consecutive lanes (power of two <= 64), nearest lanes first
__device__ __forceinline__ float lanes_sum(float v, int width) {
    for (int o = 1; o < width; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- packing
// two fp32 -> one dword of two fp16, each rounded on its own (the asm keeps the compiler from folding a preceding
// fma into v_fma_mixlo_f16, which would round once where every other kernel of the path rounds twice)
__device__ __forceinline__ unsigned pack2(float v0, float v1) {
    asm volatile("" : "+v"(v0), "+v"(v1));
    f16x2 p;
    p[0] = (_Float16)v0;
    p[1] = (_Float16)v1;
    return __builtin_bit_cast(unsigned, p);
}
// the fp8 (e4m3) range
__device__ __forceinline__ float clamp448(float v) { return __builtin_fminf(__builtin_fmaxf(v, -448.f), 448.f); }
// four floats -> four fp8 (e4m3) bytes, k order
__device__ __forceinline__ unsigned pack_fp8x4(float a, float b, float c, float d) {
    int pk = 0;
    pk = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, pk, false);
    pk = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, pk, true);
    return (unsigned)pk;
}

// ---- the split-bf16 ("x3") operand form of the attention kernels and, with F16, their one-plane fp16 form
// 4 fp32 -> 4 bf16 hi (top 16 bits) and 4 bf16 lo = rne(x - hi), each packed in two dwords
// (F16: hi = the 4 values rounded to fp16, lo unused)
template <bool F16>
__device__ __forceinline__ void split4(const f32x4& x, u32x2& hi, u32x2& lo) {
    if (F16) {
        f16x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (_Float16)x[e];
        hi = __builtin_bit_cast(u32x2, v);
        lo = hi;
        return;
    }
    bf16x4 l;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const unsigned ua = __float_as_uint(x[2 * p]), uc = __float_as_uint(x[2 * p + 1]);
        hi[p] = __builtin_amdgcn_perm(uc, ua, 0x07060302u);  // {hi16(x[2p+1]), hi16(x[2p])}
        l[2 * p] = (__bf16)(x[2 * p] - __uint_as_float(ua & 0xFFFF0000u));
        l[2 * p + 1] = (__bf16)(x[2 * p + 1] - __uint_as_float(uc & 0xFFFF0000u));
    }
    lo = __builtin_bit_cast(u32x2, l);
}
// accumulator registers e0 .. e0+7 -> the hi / lo fragments of one 16-key (16-row) chunk (F16: one fp16 fragment)
template <bool F16>
__device__ __forceinline__ void split_acc8(const f32x16& s, int e0, u32x4& hi, u32x4& lo) {
    if (F16) {
        f16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (_Float16)s[e0 + e];
        hi = __builtin_bit_cast(u32x4, v);
        lo = hi;
        return;
    }
    u32x4 hb;
    bf16x8 l;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const float a = s[e0 + 2 * p], c = s[e0 + 2 * p + 1];
        const unsigned ua = __float_as_uint(a), uc = __float_as_uint(c);
        hb[p] = __builtin_amdgcn_perm(uc, ua, 0x07060302u);
        l[2 * p] = (__bf16)(a - __uint_as_float(ua & 0xFFFF0000u));
        l[2 * p + 1] = (__bf16)(c - __uint_as_float(uc & 0xFFFF0000u));
    }
    hi = hb;
    lo = __builtin_bit_cast(u32x4, l);
}
// acc += a b with a = ahi + alo, b = bhi + blo, smallest terms first (alo blo dropped); F16: one v_mfma_f32_32x32x16_f16 on the hi
// fragments (the lo fragments are dead code)
template <bool F16>
__device__ __forceinline__ f32x16 mfma3(const u32x4& ahi, const u32x4& alo, const u32x4& bhi, const u32x4& blo, f32x16 acc) {
    if (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, ahi), __builtin_bit_cast(f16x8, bhi), acc, 0, 0, 0);
    const bf16x8 ah = __builtin_bit_cast(bf16x8, ahi), al = __builtin_bit_cast(bf16x8, alo);
    const bf16x8 bh = __builtin_bit_cast(bf16x8, bhi), bl = __builtin_bit_cast(bf16x8, blo);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}

// ---- OCP-MX block scaling of the fp6 (e2m3) operands: a lane's 32 values are one scale block of v_mfma_scale_f32_32x32x64_f8f6f4
// E8M0 byte of the block scale for a block whose largest magnitude is m: m / 2^(byte - 127) in (3.75, 7.5] (e2m3's top binades)
__device__ __forceinline__ int e8m0_scale_byte(float m) {
    const int e = (int)(__float_as_uint(m * (16.0f / 15.0f)) >> 23) - 2;
    return m > 0.f ? (e < 1 ? 1 : e) : 127;
}
__device__ __forceinline__ float e8m0_scale_of(int byte) { return __uint_as_float((unsigned)byte << 23); }
// largest magnitude of four fp16 fragments (32 values): sign bits masked, packed fp16 maxima
__device__ __forceinline__ float absmax32(f16x8 a, f16x8 b, f16x8 c, f16x8 d) {
    auto ab = [](f16x8 v) {
        u32x4 u = __builtin_bit_cast(u32x4, v);
        u &= 0x7fff7fffu;
        return __builtin_bit_cast(f16x8, u);
    };
    f16x8 m = __builtin_elementwise_max(__builtin_elementwise_max(ab(a), ab(b)), __builtin_elementwise_max(ab(c), ab(d)));
    const f16x2 m2 = __builtin_elementwise_max(__builtin_elementwise_max(f16x2{m[0], m[1]}, f16x2{m[2], m[3]}),
                                               __builtin_elementwise_max(f16x2{m[4], m[5]}, f16x2{m[6], m[7]}));
    return fmaxf((float)m2[0], (float)m2[1]);
}

// ---- diagnostic builds (*_DIAG_NOMFMA, tools/probe): stand-ins that keep a matrix instruction's operands alive and return the
// accumulator unchanged (results are then garbage; only the time is of interest)
__device__ __forceinline__ f32x16 keep16(f16x8 a, f16x8 b, f32x16 c) {
    asm volatile("" ::"v"(a), "v"(b));
    return c;
}
__device__ __forceinline__ f32x16 keep8(i32x8 a, i32x8 b, f32x16 c) {
    asm volatile("" ::"v"(a), "v"(b));
    return c;
}
