// Route of the fused LocalAttention passes (qkv conv -> window attention -> proj conv in one kernel per direction), shared by
// attention.hip (entry points, LDS-tile kernels, reductions) and attention_reg.hip (register-resident kernels).
#pragma once
#include "common.h"

namespace mstg {

enum AttnFusedKind { AF_NONE, AF_REG, AF_BIG, AF_FUSED };  // no fused path at this width / attn_reg_* / attn_big_* / attn_fused_*
struct AttnFusedRoute {
    AttnFusedKind kind;
    int C;
    int bwd_waves, bwd_wgs_per_cu;  // backward of the attention_reg.hip kernels: waves per workgroup, workgroups (= slabs) per CU
    char name[48];                  // symbol of the pass's kernel, as the per-launch profiler reports it
};
// attention_reg.hip; the only reader of MSTG_ATTN_REG and MSTG_ATTN_BIG32
AttnFusedRoute attn_fused_route(bool bwd, int C, bool norm);
int attn_reg_fwd(const AttnFusedRoute& r, const float* x, const float* in_stats, const float* wqkv, const float* bqkv, const float* wp,
                 const float* bp, float* y, int N, int H, int W, hipStream_t st);
int attn_reg_bwd(const AttnFusedRoute& r, const float* x, const float* in_stats, const float* wqkv, const float* bqkv, const float* wp,
                 const float* dy, float* dx, float* partial, float* nsum, int kblk, int nblocks, int N, int H, int W, hipStream_t st);
// most workgroups the backward uses (grid sizing: the only thing here that looks at the device)
inline int attn_reg_bwd_blocks(const AttnFusedRoute& r) { return cu_count() * r.bwd_wgs_per_cu; }

}  // namespace mstg
