// Wide-channel fp16 inference (csrc/infer_f16_wide.hip): the layers of EnhancedGenerator(channels=32 / 64) whose input or output
// has more than 64 channels.  The C-ABI entry points of csrc/infer_f16.hip dispatch here; the channels=16 kernels stay as they are.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "mstg_hip.h"

namespace mstg {

// a layer that takes the wide convolution kernel (more than 64 input or output channels)
inline bool f16w_conv_is_wide(const mstg_f16_conv_desc* d) { return d->Cin > 64 || d->Cout > 64; }

size_t f16w_conv_plan_bytes(const mstg_f16_conv_desc* d);     // 0 (and the error message) for an unsupported geometry
size_t f16w_conv_partial_bytes(const mstg_f16_conv_desc* d);
int f16w_conv_pack(const mstg_f16_conv_desc* d, const float* const w[4], const float* const b[4], void* blob, size_t blob_bytes,
                   hipStream_t st);
int f16w_conv_fwd(const mstg_f16_conv_desc* d, const void* blob, const void* x, const float* in_stats, const void* residual, void* y,
                  float* out_stats, void* workspace, size_t workspace_bytes, hipStream_t st);

// LocalAttention at C = 128 / 256 (blob layout of mstg_f16_attn_pack)
int f16w_attn_fwd(const void* x, const float* in_stats, const void* blob, void* y, int N, int H, int W, int C, hipStream_t st);

// partial rows [N][rows][2][CP] -> stats [N][C][2] (f16_norm_finalize_kernel of csrc/infer_f16.hip; CP divides 256)
int f16_norm_finalize(const float* partial, float* stats, int N, int rows, int CP, int C, float count, hipStream_t st);

}  // namespace mstg
