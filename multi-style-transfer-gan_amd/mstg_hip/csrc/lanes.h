// Lane-level device helpers shared by the kernel files: cross-lane reductions of the MFMA accumulator layout, the fp16 vector
// types and the fp16 MFMA wrappers.  Lane l = (i = l & 15, g = l >> 4); accumulator register r of a 16x16 MFMA is D[4g + r][i].
// A new kernel file includes this header and does not re-declare any of it ("Shared kernel helpers").
#pragma once
#include "common.h"

typedef _Float16 h16;
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 b16;
typedef __bf16 b16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 b16x8 __attribute__((ext_vector_type(8)));

namespace mstg {

// Reductions over the 16 lanes that share lane >> 4 (one accumulator row lives in 16 lanes).  Written with DPP row operations
// (quad_perm, row_half_mirror, row_mirror: VALU-speed cross-lane moves inside a row of 16): __shfl_xor compiles to
// ds_bpermute_b32 here, a ~100-cycle LDS round trip per step, and the softmax / normalisation chains are four dependent
// steps deep -- time stamps showed them to be 60 % of a 32-channel window's forward cycles.  Every lane ends with the result.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp_mov<0x141>(v);  // row_half_mirror
    v += dpp_mov<0x140>(v);  // row_mirror
    return v;
}
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, dpp_mov<0xB1>(v));
    v = fmaxf(v, dpp_mov<0x4E>(v));
    v = fmaxf(v, dpp_mov<0x141>(v));
    v = fmaxf(v, dpp_mov<0x140>(v));
    return v;
}

// Reductions over the 4 lanes sharing i = lane & 15 (lanes l, l ^ 16, l ^ 32, l ^ 48: the four accumulator row groups of one
// column); every lane ends with the result.  v_permlane16_swap exchanges the odd rows of its first operand with the even rows of
// its second, v_permlane32_swap the upper half of the first with the lower half of the second: with both operands holding v,
// first (+ or max) second is the xor-16 / xor-32 step.  Inline asm: the builtins' two results of one input get folded into one by
// the compiler.  The s_nop covers the "VALU write -> v_permlane read" hazard (2 wait states).
__device__ __forceinline__ void permlane16_swap(float& a, float& b) {
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void permlane32_swap(float& a, float& b) {
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ float col4_sum(float v) {
    float a = v, b = v;
    permlane16_swap(a, b);
    v = a + b;
    a = b = v;
    permlane32_swap(a, b);
    return a + b;
}
__device__ __forceinline__ float col4_max(float v) {
    float a = v, b = v;
    permlane16_swap(a, b);
    v = fmaxf(a, b);
    a = b = v;
    permlane32_swap(a, b);
    return fmaxf(a, b);
}

// fp16-in / fp32-accumulate MFMA, 16x16 tile (v_mfma_f32_16x16x16_f16, v_mfma_f32_16x16x32_f16): lane (i, g) supplies
// A[m = i][k = 4g .. 4g+3] (K = 16) or A[m = i][k = 8g .. 8g+7] (K = 32), B likewise with n = i; the accumulator as above.
__device__ __forceinline__ f32x4 mfma16x16x16_f16(h16x4 a, h16x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16x16x32_f16(h16x8 a, h16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ h16x4 cvt4(f32x4 v) { return h16x4{(h16)v[0], (h16)v[1], (h16)v[2], (h16)v[3]}; }

// bf16-in / fp32-accumulate MFMA (v_mfma_f32_16x16x32_bf16): the operand and accumulator layouts of the fp16 form.  A float -> b16
// cast rounds to nearest even (v_cvt_pk_bf16_f32).
__device__ __forceinline__ f32x4 mfma16x16x32_bf16(b16x8 a, b16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

}  // namespace mstg
