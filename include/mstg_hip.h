/*
 * mstg_hip.h -- C ABI of the MI355X (gfx950) hot-path library for multi-style-transfer-gan.
 *
 * The reference has no FFI / operator boundary of its own: its hot path is torch.nn layers called from
 * enhanced_generator.py.  This header is the boundary the reference would bind instead of
 * those layers; every entry point names the reference call site it replaces.  Conventions:
 *
 *   - plain C, device pointers + explicit sizes + a hipStream_t passed as void*; no torch types;
 *   - every function returns 0 on success or a negative MSTG_E_* code (the Python shim raises RuntimeError);
 *   - the caller owns every buffer, workspaces included (sizes from the *_workspace_bytes queries);
 *   - the library keeps no mutable global state; calls are asynchronous on `stream`;
 *   - activations are fp32 NHWC ("channels last") unless a descriptor flag says NCHW (only the 3-channel
 *     image tensors at the module boundary are NCHW); weights stay in PyTorch's own layouts
 *     (Conv2d OIHW, ConvTranspose2d IOHW) so reference state_dicts are consumed as they are.
 *
 * Memory contract of every entry point (tests/test_gpu_memory_contract.py runs the hot path under it):
 *
 *   - it writes only its declared outputs, and at most workspace_bytes -- what the matching *_workspace_bytes query returned -- of
 *     the workspace; not one byte in front of or behind either;
 *   - it reads nothing that neither it nor the caller wrote: no element past the end of an input, nothing from an output or from
 *     the workspace before the call itself has filled it (with workspace_packed != 0: before the earlier call has);
 *   - it leaves every argument declared `const` unchanged;
 *   - it needs no more than 16-byte alignment of any device pointer (less where an entry says so: a slice `x_coff` / `y_coff`
 *     floats into a row, byte images, the scalar fall-backs of the element-wise kernels).
 *
 *   Written in place, by contract: the power-iteration vectors u and v of mstg_spectral_norm* (training != 0); running_mean /
 *   running_var of the BatchNorm forwards in training mode; p, m and v of the Adam steps, and the step state of the mixed-precision
 *   train step; the gradient buffer of the clip-by-norm entry; every gradient output of an entry called with accumulate != 0
 *   (mstg_conv_desc.accumulate: y or dx; dw / dbias; the attention, multi-scale, spectral-norm and LayerNorm parameter gradients),
 *   which is then read as well as written.
 */
#ifndef MSTG_HIP_H
#define MSTG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSTG_OK 0
#define MSTG_E_BADARG (-1)      /* inconsistent sizes / unsupported geometry */
#define MSTG_E_ALIGN (-2)       /* channel counts / offsets violate the alignment the kernels need */
#define MSTG_E_LAUNCH (-3)      /* hipLaunch failed; see mstg_last_error() */
#define MSTG_E_WORKSPACE (-4)   /* workspace too small */
#define MSTG_E_UNSUPPORTED (-5) /* valid request outside what this build implements */

/* activation codes shared by conv epilogues and the norm kernels */
#define MSTG_ACT_NONE 0
#define MSTG_ACT_RELU 1
#define MSTG_ACT_LEAKY02 2 /* LeakyReLU(0.2), enhanced_generator.py:238-251, pretrain.py:67-76 */
#define MSTG_ACT_TANH 3    /* nn.Tanh, enhanced_generator.py:138 */
#define MSTG_ACT_GELU 4    /* nn.GELU() (erf form): build-defined StructuralTransformerBlock only */

const char* mstg_version(void);    /* "mstg-hip <semver> gfx950" */
const char* mstg_arch(void);       /* "gfx950" */
const char* mstg_last_error(void); /* text of the last failing HIP call on this thread, "" if none */
/* The MSTG_* environment switches are read when the library is loaded; call this after changing one. */
void mstg_env_refresh(void);

/* Per-launch profiler (measurement only; bench.py's `roofline` object).  While enabled, every kernel the library launches is
 * bracketed by two HIP events on the stream it is launched on.  mstg_prof_enable(1) clears earlier records; mstg_prof_get
 * waits for record i and returns its kernel symbol (as rocprofv3 --kernel-trace prints it, without return type, namespace and
 * parameter list) and its duration in milliseconds.  Off by default: no events are created on the product path. */
int mstg_prof_enable(int on);
int mstg_prof_count(void);
int mstg_prof_get(int i, char* name, size_t name_cap, float* ms);

/* ------------------------------------------------------------------------------------------------
 * Convolutions.  One descriptor describes the MODULE (nn.Conv2d or nn.ConvTranspose2d); the three
 * entry points are its forward, its input gradient and its weight/bias gradient.
 * Replaces: nn.Conv2d / nn.ConvTranspose2d at enhanced_generator.py:10-11,53-73,92,99,106,121,128,137,
 * 237-265 and pretrain.py:65-91 (their ATen convolution / convolution_backward dispatch).
 * ---------------------------------------------------------------------------------------------- */
typedef struct mstg_conv_desc {
    int32_t N, H, W, Cin;   /* module input  (N,H,W,Cin)  */
    int32_t Ho, Wo, Cout;   /* module output (N,Ho,Wo,Cout) */
    int32_t KH, KW, stride, pad, dil;
    int32_t transposed;     /* 0: Conv2d (weight OIHW); 1: ConvTranspose2d k4 s2 p1 (weight IOHW) */
    int32_t x_nchw, y_nchw; /* 1: that tensor is NCHW (3-channel image boundary), else NHWC */
    int32_t x_ctot, x_coff; /* module input  = channels [x_coff, x_coff+Cin)  of an NHWC tensor with x_ctot channels */
    int32_t y_ctot, y_coff; /* module output = channels [y_coff, y_coff+Cout) of an NHWC tensor with y_ctot channels */
    int32_t act;            /* forward epilogue activation applied after bias: MSTG_ACT_NONE / _RELU / _LEAKY02 / _TANH */
    int32_t accumulate;     /* fwd: y += result; dgrad: dx += result (branches that share an input) */
} mstg_conv_desc;

/* Input gradient of a convolution whose INPUT was y = ReLU(InstanceNorm2d(x_raw)) (enhanced_generator.py:93-94, 72-75 + 84: the
 * stem norm in front of down1, a MultiScaleBlock's concat norm in front of its fusion convolution, a block's fusion norm in front
 * of the next stage's convolution): besides dx = dL/dy the launch emits sums[n][0][c] = sum_p dx [x^ > 0] and sums[n][1][c] =
 * sum_p dx [x^ > 0] x^ (x^ = (x_raw - mean) * rstd from x_stats [N][Cin][2]) from its epilogue -- the two reductions of that norm's
 * backward, which mstg_norm_bwd_apply(..., sums, 1, ...) consumes; the statistics pass over (x_raw, dx) is not needed.  Supported
 * where the persistent kernel runs the input gradient (mstg_conv2d_dgrad_bsums_supported); workspace_packed as for the *_cached
 * entry points below. */
int mstg_conv2d_dgrad_bsums_supported(const mstg_conv_desc* d);
size_t mstg_conv2d_dgrad_bsums_workspace_bytes(const mstg_conv_desc* d);
int mstg_conv2d_dgrad_bsums(const mstg_conv_desc* d, const float* dy, const float* w, float* dx, const float* x_raw, const float* x_stats,
                            float* sums, void* workspace, size_t workspace_bytes, int workspace_packed, void* stream);

/* Filter-pack caching.  mstg_conv2d_fwd / _fwd_norm / _dgrad and mstg_msblock_fwd / _dgrad begin by re-packing the filter into the
 * caller's workspace (a ~5 us launch, ~170 of them per CycleGAN step).  The *_cached twins take workspace_packed: non-zero = "this
 * workspace still holds what the SAME call (same descriptor, same pass, same weight VALUES) packed into it", and the pack launch is
 * skipped.  Whether that is true is the caller's knowledge (weights change at optimizer.step(); mstg_hip/ops.py keeps one workspace
 * per (layer, pass, stream) and a stamp of the weights' version); with workspace_packed = 0 they are the plain entry points. */
int mstg_conv2d_fwd_cached(const mstg_conv_desc* d, const float* x, const float* w, const float* bias, float* y, void* workspace,
                           size_t workspace_bytes, int workspace_packed, void* stream);
int mstg_conv2d_fwd_norm_cached(const mstg_conv_desc* d, const float* x, const float* in_stats, const float* w, const float* bias,
                                float* y, float* out_stats, void* workspace, size_t workspace_bytes, int workspace_packed, void* stream);
int mstg_conv2d_dgrad_cached(const mstg_conv_desc* d, const float* dy, const float* w, float* dx, void* workspace, size_t workspace_bytes,
                             int workspace_packed, void* stream);
int mstg_msblock_fwd_cached(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                            const float* b3, const float* w4, const float* b4, float* y, int N, int H, int W, int CH, void* workspace,
                            size_t workspace_bytes, int workspace_packed, void* stream);
int mstg_msblock_dgrad_cached(const float* dy, const float* w1, const float* w2, const float* w3, const float* w4, const float* dres,
                              float* dx, int N, int H, int W, int CH, void* workspace, size_t workspace_bytes, int workspace_packed,
                              void* stream);

/* Grouped launches.  G <= mstg_conv2d_group_max() (4) forwards -- or input gradients -- of ONE descriptor, each with its own source,
 * destination, filter and bias, as one launch chain: one pack launch for the G filters, one main launch whose grid is G copies of the
 * single launch's (the persistent kernels split their occupancy-sized grid among the groups).  d describes one group (d->N images);
 * route, tile shape, pack layout and per-image summation order are the single launch's, so group k's result is bit for bit what
 * mstg_conv2d_fwd / _dgrad gives for (x[k], w[k], bias[k]).  The pointer tables live on the host; bias: NULL, or G pointers all
 * null or all non-null.  d->accumulate is not supported.  Workspace: mstg_conv2d_grouped_workspace_bytes(d, G) = G times the
 * per-group query (rounded up to 16 bytes), never cached.  Taught: igemm_light / igemm_heavy, conv_p32_kernel without an epilogue,
 * conv_co1_kernel, conv_img_dgrad_kernel and the two pack kernels; every other route (the stream kernel, the 7x7 image stem, the packed
 * <= 4-channel heads) returns MSTG_E_UNSUPPORTED and launches nothing -- the caller then makes G plain calls.
 * mstg_conv2d_grouped_kernel_name: the main kernel of pass 0 (forward) / 1 (dgrad) as a profiler prints it, "" where unsupported. */
int mstg_conv2d_group_max(void);
size_t mstg_conv2d_grouped_workspace_bytes(const mstg_conv_desc* d, int G);
int mstg_conv2d_fwd_grouped(const mstg_conv_desc* d, int G, const float* const* x, const float* const* w, const float* const* bias,
                            float* const* y, void* workspace, size_t workspace_bytes, void* stream);
int mstg_conv2d_dgrad_grouped(const mstg_conv_desc* d, int G, const float* const* dy, const float* const* w, float* const* dx,
                              void* workspace, size_t workspace_bytes, void* stream);
const char* mstg_conv2d_grouped_kernel_name(const mstg_conv_desc* d, int pass);

/* name of the kernel a pass (0 forward, 1 dgrad, 2 wgrad; 3 forward with the statistics epilogue of mstg_conv2d_fwd_norm, 4 dgrad with
 * the backward-sums epilogue of mstg_conv2d_dgrad_bsums) of this layer launches, as a profiler prints it (for reports and pack keys) */
const char* mstg_conv2d_kernel_name(const mstg_conv_desc* d, int pass);
/* workspace of fwd and dgrad: room for the filter re-packed into the order the kernel stages it (a few 100 KB at most) */
size_t mstg_conv2d_workspace_bytes(const mstg_conv_desc* d);
int mstg_conv2d_fwd(const mstg_conv_desc* d, const float* x, const float* w, const float* bias /*nullable*/,
                    float* y, void* workspace, size_t workspace_bytes, void* stream);
/* dx = d(loss)/d(module input), from dy = d(loss)/d(module output) */
/* Weight gradient of a 1x1 Conv2d whose input is ReLU(InstanceNorm2d(x_raw)) (the MultiScaleBlock's fusion convolution behind the
 * branch concat's norm, enhanced_generator.py:72-75, 83): x_raw is normalised with in_stats[n][c] = (mean, rstd) while the kernel
 * stages it, so the normalised tensor need not exist.  Supported where a staged pixel run stays inside one image. */
int mstg_conv2d_wgrad_norm_supported(const mstg_conv_desc* d);
int mstg_conv2d_wgrad_norm(const mstg_conv_desc* d, const float* x_raw, const float* in_stats, const float* dy, float* dw, float* dbias,
                           void* workspace, size_t workspace_bytes, void* stream);
/* Forward with InstanceNorm folded in on either side, for the layers the persistent kernel covers (4x4 stride-2 Conv2d /
 * ConvTranspose2d and 1x1 Conv2d at 16 / 32 / 64 channels, unsliced NHWC, no fused activation): in_stats (nullable) = (mean, rstd)
 * [N][Cin][2] of the RAW source -- it is normalised and ReLU'd while staged, i.e. x is what stands in front of
 * nn.InstanceNorm2d + nn.ReLU (enhanced_generator.py:54-75) and the normalised tensor is never written; out_stats (nullable) =
 * (mean, rstd) [N][Cout][2] of y, summed in the epilogue (same layout as mstg_norm_stats; sums of squares instead of pivoted
 * sums, combined in double).  Backward: mstg_conv2d_dgrad / _wgrad as for mstg_conv2d_fwd. */
int mstg_conv2d_fwd_norm_supported(const mstg_conv_desc* d);
/* 1 where the epilogue statistics also cost less than a statistics pass over the output (the callers' default routing) */
int mstg_conv2d_fwd_stats_pays(const mstg_conv_desc* d);
size_t mstg_conv2d_fwd_norm_workspace_bytes(const mstg_conv_desc* d);
int mstg_conv2d_fwd_norm(const mstg_conv_desc* d, const float* x, const float* in_stats, const float* w, const float* bias, float* y,
                         float* out_stats, void* workspace, size_t workspace_bytes, void* stream);
int mstg_conv2d_dgrad(const mstg_conv_desc* d, const float* dy, const float* w, float* dx, void* workspace,
                      size_t workspace_bytes, void* stream);
/* dw (same layout as w) and dbias (nullable) ; workspace holds per-split partial sums (deterministic, no atomics);
 * d->accumulate != 0: dw += and dbias += (gradients accumulated straight into an optimizer's flat gradient buffer) */
size_t mstg_conv2d_wgrad_workspace_bytes(const mstg_conv_desc* d);
int mstg_conv2d_wgrad(const mstg_conv_desc* d, const float* x, const float* dy, float* dw, float* dbias /*nullable*/,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * InstanceNorm2d(affine=False, eps=1e-5, biased variance) fused with the activation that follows it and an
 * optional residual add.  Replaces nn.InstanceNorm2d + nn.ReLU / nn.LeakyReLU(0.2) pairs at
 * enhanced_generator.py:54-75,93-94,100-101,107-108,122-123,129-130,242-251,263-264 and the `+ x` of :84.
 *   y = act((x - mean) * rstd) [+ residual]      stats[n][c] = {mean, rstd} is saved for the backward.
 * batch_stats=1 turns it into BatchNorm2d (training: statistics over N,H,W; pretrain.py:69-89) with affine
 * gamma/beta and running-stat update (momentum 0.1, unbiased running_var); batch_stats=2 = BatchNorm eval.
 * ---------------------------------------------------------------------------------------------- */
size_t mstg_norm_workspace_bytes(int N, int HW, int C);
int mstg_norm_act_fwd(const float* x, const float* residual /*nullable*/, float* y, float* stats /* [N][C][2] */,
                      int N, int HW, int C, int act, int batch_stats, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, void* workspace, size_t workspace_bytes, void* stream);
/* dx from dy (gradient w.r.t. y); the residual's gradient is dy itself.  dgamma/dbeta only for batch_stats=1. */
int mstg_norm_act_bwd(const float* x, const float* stats, const float* dy, float* dx, int N, int HW, int C, int act,
                      int batch_stats, const float* gamma, const float* beta, float* dgamma, float* dbeta,
                      void* workspace, size_t workspace_bytes, void* stream);
/* InstanceNorm (batch_stats = 0) over N = G * plan_N images with the plan of a batch of plan_N: the row split per image is a function
 * of the batch size, so a pass over G groups at once would split every image differently from the G passes it replaces.  These run all
 * N images with the launch geometry, partial rows and summation order of a plan_N-image call (both branches: split <= 32, and the
 * statistics / sums launch above it); per image the results are bit for bit those of mstg_norm_act_fwd / _bwd on its own group. */
size_t mstg_norm_workspace_bytes_plan(int N, int plan_N, int HW, int C);
int mstg_norm_act_fwd_plan(const float* x, const float* residual /*nullable*/, float* y, float* stats /* [N][C][2] */, int N, int plan_N,
                           int HW, int C, int act, void* workspace, size_t workspace_bytes, void* stream);
int mstg_norm_act_bwd_plan(const float* x, const float* stats, const float* dy, float* dx, int N, int plan_N, int HW, int C, int act,
                           void* workspace, size_t workspace_bytes, void* stream);
/* The two halves on their own, for a norm whose neighbours do the other half (mstg_window_attn_norm_*): statistics only
 * (stats[n][c] = {mean, rstd}, bit-identical to what mstg_norm_act_fwd stores), and the backward's apply pass given
 * sums[n][s][2][C]: rows that add up, per (image, channel), to sum(dy * act') and sum(dy * act' * x^) (InstanceNorm only). */
int mstg_norm_apply_fwd(const float* x, const float* stats, const float* residual /*nullable*/, float* y, int N, int HW, int C, int act,
                        void* stream);  /* y = act((x - mean) * rstd) [+ residual] with the statistics given */
int mstg_norm_stats(const float* x, float* stats, int N, int HW, int C, void* workspace, size_t workspace_bytes, void* stream);
int mstg_norm_bwd_apply(const float* x, const float* stats, const float* dy, const float* sums /* [N][sums_split][2][C] */,
                        int sums_split, float* dx, int N, int HW, int C, int act, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LocalAttention core (enhanced_generator.py:22-35,39-42), window 4x4.  The qkv and proj 1x1 convolutions
 * (:28, :36) run through mstg_conv2d_*; this is everything between them, per window, with the reference's
 * window partition / un-partition permutes reduced to index arithmetic on NHWC:
 *   q,k L2-normalised per pixel over channels (F.normalize, eps 1e-12) ; attn = softmax_c2(sum_p q^[p,c1] k^[p,c2])
 *   (C x C per window, no scale) ; o[p,c1] = sum_c2 attn[c1,c2] v[p,c2].
 * qkv: NHWC (N,H,W,3C) with q|k|v channel blocks (= qkv.chunk(3, dim=1)); o: NHWC (N,H,W,C).
 * H, W multiples of 4 (anything else raises in the reference too); C a multiple of 4, <= 256 (row-blocked above 64).
 * ---------------------------------------------------------------------------------------------- */
int mstg_window_attn_core_fwd(const float* qkv, float* o, int N, int H, int W, int C, void* stream);
/* dqkv from d_o; the attention matrix is recomputed from qkv, nothing but qkv is saved by the forward */
int mstg_window_attn_core_bwd(const float* qkv, const float* d_o, float* dqkv, int N, int H, int W, int C, void* stream);

/* The same core for any window size (enhanced_generator.py:7: the constructor default is window_size=8; every caller passes 4,
 * which the entry points above serve): qkv NHWC (N,H,W,3C) -> o NHWC (N,H,W,C), one workgroup per ws x ws window, plain fp32 loops.
 * Supported while a window's q|k|v (+ dO, dS in the backward) fits one CU's LDS (mstg_window_attn_ws_supported). */
int mstg_window_attn_ws_supported(int C, int ws);
int mstg_window_attn_ws_fwd(const float* qkv, float* o, int N, int H, int W, int C, int ws, void* stream);
int mstg_window_attn_ws_bwd(const float* qkv, const float* d_o, float* dqkv, int N, int H, int W, int C, int ws, void* stream);

/* Fully fused LocalAttention for C = 16 and 32 (enhanced_generator.py:13-47 in one kernel per direction): the qkv and proj
 * 1x1 convolutions (:28, :36) and the window attention between them; x is read once, y written once.  wqkv (3C,C) and
 * wproj (C,C) are the 1x1 conv weights exactly as stored (OIHW with 1x1 taps).  The backward returns dx and ONE flat
 * gradient vector dparams = [dWqkv (3C*C) | dWproj (C*C) | dbqkv (3C) | dbproj (C)]. */
int mstg_window_attn_fused_supported(int C);
int mstg_window_attn_fwd(const float* x, const float* wqkv, const float* bqkv, const float* wproj, const float* bproj,
                         float* y, int N, int H, int W, int C, void* stream);
/* The stage's first InstanceNorm + ReLU (enhanced_generator.py:93-94, 100-101, 122-123, 129-130) folded into LocalAttention, its
 * only consumer: x_raw is the convolution output in front of the norm, in_stats[n][c] = (mean, rstd) from mstg_norm_stats; the
 * normalised tensor never exists in memory.  The backward also returns norm_sums[n][S][2][C], S = mstg_window_attn_norm_sums_split():
 * rows adding up to the per (image, channel) sums of dz * [z > 0] and dz * [z > 0] * z for mstg_norm_bwd_apply (the norm backward's
 * reduction pass, done in this kernel's epilogue). */
/* mstg_window_attn_bwd / mstg_window_attn_norm_bwd with the four parameter gradients written -- or, accumulate != 0, added -- straight
 * into the caller's gradient tensors (dwqkv (3C,C), dbqkv (3C), dwproj (C,C), dbproj (C)) by the fixed-order slab reduce, instead of
 * into one flat vector: the caller's framework then launches no per-parameter accumulation kernels. */
int mstg_window_attn_bwd_direct(const float* x, const float* wqkv, const float* bqkv, const float* wproj, const float* bproj, const float* dy,
                                float* dx, float* dwqkv, float* dbqkv, float* dwproj, float* dbproj, int accumulate, int N, int H, int W, int C,
                                void* workspace, size_t workspace_bytes, void* stream);
int mstg_window_attn_norm_bwd_direct(const float* x_raw, const float* in_stats, const float* wqkv, const float* bqkv, const float* wproj,
                                     const float* bproj, const float* dy, float* dz, float* dwqkv, float* dbqkv, float* dwproj,
                                     float* dbproj, int accumulate, float* norm_sums, int N, int H, int W, int C, void* workspace,
                                     size_t workspace_bytes, void* stream);
int mstg_window_attn_norm_sums_split(void);
int mstg_window_attn_norm_fwd(const float* x_raw, const float* in_stats, const float* wqkv, const float* bqkv, const float* wproj,
                              const float* bproj, float* y, int N, int H, int W, int C, void* stream);
size_t mstg_window_attn_norm_bwd_workspace_bytes(int N, int H, int W, int C);
int mstg_window_attn_norm_bwd(const float* x_raw, const float* in_stats, const float* wqkv, const float* bqkv, const float* wproj,
                              const float* bproj, const float* dy, float* dz, float* dparams, float* norm_sums, int N, int H, int W,
                              int C, void* workspace, size_t workspace_bytes, void* stream);
size_t mstg_window_attn_bwd_workspace_bytes(int N, int H, int W, int C);
int mstg_window_attn_bwd(const float* x, const float* wqkv, const float* bqkv, const float* wproj, const float* bproj,
                         const float* dy, float* dx, float* dparams, int N, int H, int W, int C, void* workspace,
                         size_t workspace_bytes, void* stream);
/* name of the kernel that does the arithmetic of a pass (0 forward, 1 backward) of the window-attention core (fused == 0; norm is
 * ignored) or of the fused LocalAttention (fused != 0; norm != 0: the mstg_window_attn_norm_* forms) at width C, as a profiler
 * prints it and under the switches as last read, e.g. "attn_core_bwd_blk4_kernel<256>", "attn_reg_bwd_kernel<16, true, 4>";
 * "" for a width without such a path. */
const char* mstg_window_attn_kernel_name(int fused, int pass, int C, int norm);

/* ------------------------------------------------------------------------------------------------
 * Element-wise / reduction helpers of the training step (enhanced_train.py:49-52,72-115,36-43).
 * ---------------------------------------------------------------------------------------------- */
/* y = act(x) ; dx = dy * act'(x)  (LeakyReLU(0.2) of the discriminator stem; Tanh backward uses y) */
int mstg_act_fwd(const float* x, float* y, size_t n, int act, void* stream);
int mstg_act_bwd(const float* x_or_y, const float* dy, float* dx, size_t n, int act, void* stream);
/* mean losses: out[0] = mean(|a-b|) (kind 0, nn.L1Loss) or mean((a-b)^2) (kind 1, nn.MSELoss);
 * b == NULL means the constant `bconst`.  Deterministic two-stage reduction; workspace >= 4 KiB + 8 B per 4096 elems */
size_t mstg_loss_workspace_bytes(size_t n);
int mstg_loss_mean_fwd(const float* a, const float* b, float bconst, size_t n, int kind, float* out, void* workspace,
                       size_t workspace_bytes, void* stream);
/* da = gscale[0]*scale * d(mean loss)/da ; db (nullable) = -da */
int mstg_loss_mean_bwd(const float* a, const float* b, float bconst, size_t n, int kind, const float* gscale, float scale,
                       float* da, float* db, void* stream);
/* y = a + b, n floats (residual connections; 16-byte aligned pointers) */
int mstg_add(const float* a, const float* b, float* y, size_t n, void* stream);
/* out[j] = sum_i weights[j * n + i] * terms[i][0] for 1..8 scalar loss terms and 1..6 outputs (terms: HOST array of device pointers,
 * weights: host matrix, row 0 = the differentiable total), and the backward of output 0, dterms[i] = g[0] * weights[i]: the weighted
 * loss sums of enhanced_train.py:72-81, 95-131 (total + the reported components) in one launch each way */
int mstg_weighted_sum_fwd(const float* const* terms, const float* weights, int n, int nout, float* out, void* stream);
int mstg_weighted_sum_bwd(const float* g, const float* weights, int n, float* dterms, void* stream);
/* masked-image pre-training loss (pretrain.py:160-162): out[0] = mean(|a * (1 - m) - b * (1 - m)|) and da = gscale[0] * d/da;
 * a, b, m same shape (m = the 0/1 mask of MonetPhotoDataset).  Workspace as for mstg_loss_mean_fwd. */
int mstg_masked_l1_mean_fwd(const float* a, const float* b, const float* m, size_t n, float* out, void* workspace,
                            size_t workspace_bytes, void* stream);
int mstg_masked_l1_mean_bwd(const float* a, const float* b, const float* m, size_t n, const float* gscale, float* da, void* stream);
/* torch.nn.utils.clip_grad_norm_(params, max_norm) on ONE flat gradient buffer (pretrain.py:165): g *= min(1, max_norm /
 * (||g||_2 + 1e-6)); norm_out (nullable) receives ||g||_2 before clipping.  Workspace as for mstg_loss_mean_fwd. */
int mstg_clip_grad_norm(float* g, size_t n, float max_norm, float* norm_out, void* workspace, size_t workspace_bytes, void* stream);
/* per-channel sum over pixels of an NHWC tensor slice: out[c] = sum_p x[p][coff+c]  (bias gradients, pooling) */
size_t mstg_channel_sum_workspace_bytes(size_t P, int C);
int mstg_channel_sum(const float* x, size_t P, int ctot, int coff, int C, float scale, float* out, void* workspace,
                     size_t workspace_bytes, void* stream);
/* same for a planar NCHW tensor (the 3-channel image tensors): out[c] = scale * sum_{n,i} x[n][c][i] */
size_t mstg_plane_sum_workspace_bytes(int N, int C, size_t HW);
int mstg_plane_sum(const float* x, int N, int C, size_t HW, float scale, float* out, void* workspace,
                   size_t workspace_bytes, void* stream);
/* nn.AdaptiveAvgPool2d(1) on NHWC (enhanced_generator.py:143,257): x (S,P,C) -> out (S,C) = mean over P; and its
 * gradient dx[s][p][c] = dy[s][c] / P */
int mstg_segment_mean_fwd(const float* x, int S, size_t P, int C, float* out, void* stream);
int mstg_segment_mean_bwd(const float* dy, int S, size_t P, int C, float* dx, void* stream);
/* torch.optim.Adam step over one flat fp32 buffer (enhanced_train.py:36-43: betas (0.5,0.999), eps 1e-8) */
int mstg_adam_step_flat(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                        float eps, int step, const unsigned char* mask /*nullable: 0 = skip element*/, void* stream);

/* MultiScaleBlock (enhanced_generator.py:52-71,79-83): weight and bias gradients of the four branch convolutions
 * (1x1, 3x3 d1, 3x3 d2, 3x3 d4; each CH -> CH/4) in ONE pass over x (N,H,W,CH) and dy (N,H,W,CH = the four branch outputs
 * concatenated).  dw1 (CH/4,CH,1,1), dw2..4 (CH/4,CH,3,3), db1..4 (CH/4), PyTorch layouts.  CH in {16, 32, 64}
 * (mstg_msblock_fused_supported); other widths use mstg_conv2d_wgrad per branch. */
int mstg_msblock_fused_supported(int CH);
/* forward of the four branches: x (N,H,W,CH) -> y (N,H,W,CH) = [1x1 | 3x3 d1 | 3x3 d2 | 3x3 d4] + biases, one staging of x */
size_t mstg_msblock_fwd_workspace_bytes(int CH);
int mstg_msblock_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                     const float* b3, const float* w4, const float* b4, float* y, int N, int H, int W, int CH, void* workspace,
                     size_t workspace_bytes, void* stream);
/* input gradient of the four branches: dy (N,H,W,CH) -> dx (N,H,W,CH), written once (no accumulation passes);
 * dres (nullable, (N,H,W,CH)) = gradient arriving over the block's residual connection (`+ x`, :84), added in the epilogue */
size_t mstg_msblock_dgrad_workspace_bytes(int CH);
int mstg_msblock_dgrad(const float* dy, const float* w1, const float* w2, const float* w3, const float* w4, const float* dres,
                       float* dx, int N, int H, int W, int CH, void* workspace, size_t workspace_bytes, void* stream);
size_t mstg_msblock_wgrad_workspace_bytes(int N, int H, int W, int CH);
int mstg_msblock_wgrad(const float* x, const float* dy, float* dw1, float* db1, float* dw2, float* db2, float* dw3, float* db3,
                       float* dw4, float* db4, int accumulate /* != 0: add to what the eight buffers hold */, int N, int H, int W,
                       int CH, void* workspace, size_t workspace_bytes, void* stream);
/* name of the kernel that does the arithmetic of a pass (0 forward, 1 dgrad, 2 wgrad) of the block, as a profiler prints it and
 * under the switches as last read, e.g. "ms_fwd4b_kernel<32>", "wgrad_msp_sync_kernel<16>"; "" for a width without fused path.
 * bias_aligned: whether b1..b4 of the forward call all lie on 16-byte boundaries (the forward's route depends on it, and on H;
 * a filter pack kept in the workspace belongs to the kernel named here). */
const char* mstg_msblock_kernel_name(int pass, int N, int H, int W, int CH, int bias_aligned);

/* torch.nn.utils.spectral_norm on a conv weight seen as an (M = Cout, K = Cin*kh*kw) matrix (enhanced_generator.py:269-271).
 * fwd: training != 0 runs the one power iteration in place on u (M) and v (K); always sigma = u.(W v), w_out = w / sigma.
 * bwd: dw = dwn / sigma - (sum(dwn * w) / sigma^2) u v^T with the u, v, sigma of that forward (the caller keeps copies:
 * the next forward moves u and v on). */
size_t mstg_spectral_norm_workspace_bytes(int M, int K); /* scratch of the multi-workgroup path (matrices >= 32768 elements) */
/* u_save / v_save (nullable): copies of the u, v this call ends with, for that call's backward */
int mstg_spectral_norm_fwd(const float* w, float* u, float* v, float* w_out, float* sigma, float* u_save, float* v_save, int M,
                           int K, float eps, int training, void* workspace, size_t workspace_bytes, void* stream);
int mstg_spectral_norm_bwd(const float* dwn, const float* w, const float* u, const float* v, const float* sigma, float* dw,
                           int accumulate /* != 0: dw += */, int M, int K, void* workspace, size_t workspace_bytes, void* stream);
/* The same for up to mstg_spectral_norm_group_max() weights at once -- every convolution of one EnhancedDiscriminator forward
 * (enhanced_generator.py:236-271: seven weights, each normalised by its own hook before its convolution runs) in three launches
 * (two in the backward) instead of thirteen.  Arrays hold `count` entries; per weight the semantics are those of the calls above.
 * u_save / v_save may be null as a whole; sigma (fwd) is `count` floats, sigma (bwd) `count` pointers to them. */
int mstg_spectral_norm_group_max(void);
size_t mstg_spectral_norm_group_workspace_bytes(int count, const int* M, const int* K);
int mstg_spectral_norm_group_fwd(int count, const float* const* w, float* const* u, float* const* v, float* const* w_out, float* sigma,
                                 float* const* u_save, float* const* v_save, const int* M, const int* K, float eps, int training,
                                 void* workspace, size_t workspace_bytes, void* stream);
int mstg_spectral_norm_group_bwd(int count, const float* const* dwn, const float* const* w, const float* const* u,
                                 const float* const* v, const float* const* sigma, float* const* dw, const int* accumulate, const int* M,
                                 const int* K, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Build-defined multi-style perceptual loss pieces.  The reference has NO implementation of them (the
 * north star's "VGG-feature Gram-matrix / perceptual style loss" is a README bullet only) -- parity unpinned.
 * The VGG-topology 3x3 convolutions go through mstg_conv2d_* (ReLU = epilogue activation MSTG_ACT_RELU).
 *   max-pool 2x2/2 on NHWC with the arg-max slot (0..3, row-major window order, first maximum wins like torch) per element;
 *   Gram: g[n] = scale * F[n]^T F[n], F[n] = NHWC features viewed (HW, C), C a multiple of 16;
 *   Gram backward: df[n] = scale * F[n] (dg[n] + dg[n]^T).
 * ---------------------------------------------------------------------------------------------- */
int mstg_maxpool2x2_fwd(const float* x, float* y, unsigned char* idx, int N, int H, int W, int C, void* stream);
int mstg_maxpool2x2_bwd(const float* dy, const unsigned char* idx, float* dx, int N, int H, int W, int C, void* stream);
size_t mstg_gram_workspace_bytes(int N, int HW, int C);
int mstg_gram_fwd(const float* f, float* g, int N, int HW, int C, float scale, void* workspace, size_t workspace_bytes,
                  void* stream);
int mstg_gram_bwd(const float* f, const float* dg, float* df, int N, int HW, int C, float scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Inference-only forward in fp16 storage / fp16 MFMA / fp32 accumulation (BASELINE config #5).  Replaces
 * EnhancedGenerator.forward as the reference's inference scripts call it under torch.no_grad()
 * (direct_transform.py:62-63, batch_process_images.py:210-211, advanced_transform.py:99-100).
 * Activations between calls are NHWC fp16; statistics, softmax and every accumulation are fp32.
 * InstanceNorm is split: a convolution that feeds a norm also returns that norm's (mean, rstd) per
 * (image, channel) in `out_stats` [N][Cout][2]; the consumer of the normalised tensor takes them as
 * `in_stats` and applies (x - mean) * rstd -> ReLU while staging its input (nn.InstanceNorm2d + nn.ReLU
 * at enhanced_generator.py:54-75,93-94,100-101,107-108,122-123,129-130 never touch HBM on this path).
 * Filters are packed ONCE per weight set (inference: weights are frozen) into an opaque device blob.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mstg_f16_conv_desc {
    int32_t kind;         /* 0: nn.Conv2d; 1: nn.ConvTranspose2d(k4,s2,p1); 2: the four MultiScaleBlock branch convs (:52-71) as one */
    int32_t N, H, W, Cin; /* source (N,H,W,Cin) NHWC fp16 with Cin in {16,32,64}, or (N,Cin,H,W) NCHW fp32 with Cin <= 4 */
    int32_t Ho, Wo, Cout; /* destination (N,Ho,Wo,Cout) NHWC fp16 (Cout <= 64, multiple of 4) or (N,Cout,Ho,Wo) NCHW fp16 (Cout <= 4) */
    int32_t K, stride, pad, dil;
    int32_t src_nchw_f32; /* 1: the 3-channel fp32 image at the module boundary (stem) */
    int32_t dst_nchw;     /* 1: the 3-channel output image (head) */
    int32_t act;          /* MSTG_ACT_NONE or MSTG_ACT_TANH (dst_nchw only) */
} mstg_f16_conv_desc;
size_t mstg_f16_conv_plan_bytes(const mstg_f16_conv_desc* d); /* size of the packed-filter blob; 0 = unsupported geometry */
/* w0/b0: the layer's fp32 weight (OIHW, or IOHW for kind 1) and bias (nullable); kind 2: w0..w3 / b0..b3 = branch1..branch4 */
int mstg_f16_conv_pack(const mstg_f16_conv_desc* d, const float* w0, const float* b0, const float* w1, const float* b1,
                       const float* w2, const float* b2, const float* w3, const float* b3, void* blob, size_t blob_bytes,
                       void* stream);
size_t mstg_f16_conv_partial_bytes(const mstg_f16_conv_desc* d); /* workspace needed when out_stats != NULL */
int mstg_f16_conv_fwd(const mstg_f16_conv_desc* d, const void* blob, const void* x, const float* in_stats /*nullable*/, void* y,
                      float* out_stats /*nullable*/, void* workspace, size_t workspace_bytes, void* stream);
/* The same layer reading relu((x - mean) * rstd) + residual instead of x: a MultiScaleBlock's closing norm + ReLU + `+ x`
 * (enhanced_generator.py:84) formed while the NEXT layer (:106, :121, :128, :137) stages its input, bit for bit the values
 * mstg_f16_norm_residual would have written.  residual (nullable: then exactly mstg_f16_conv_fwd) needs in_stats and an NHWC source. */
int mstg_f16_conv_fwd_res(const mstg_f16_conv_desc* d, const void* blob, const void* x, const float* in_stats,
                          const void* residual /*nullable*/, void* y, float* out_stats /*nullable*/, void* workspace,
                          size_t workspace_bytes, void* stream);
/* y = relu((x - mean) * rstd) + residual (nullable): the fusion conv's norm and the block's `+ x` (:84); NHWC fp16 */
int mstg_f16_norm_residual(const void* x, const void* residual, const float* stats, void* y, int N, int HW, int C, void* stream);
/* whole LocalAttention module (:13-47) on NHWC fp16, C in {16,32,64}; in_stats (nullable) = normalise + ReLU on load of x;
 * params = blob from mstg_f16_attn_pack (qkv and proj 1x1 filters as fp16 MFMA fragments + fp32 biases) */
size_t mstg_f16_attn_plan_bytes(int C);
int mstg_f16_attn_pack(const float* wqkv, const float* bqkv, const float* wproj, const float* bproj, int C, void* blob,
                       size_t blob_bytes, void* stream);
int mstg_f16_attn_fwd(const void* x, const float* in_stats /*nullable*/, const void* blob, void* y, int N, int H, int W, int C,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * fp16 inference of the plain CycleGAN Generator in eval mode (csrc/infer_f16_plain.hip).  Replaces Generator.forward
 * (pretrain.py:60-97 == batch_process_images.py:20-58) as batch_process_images.py:210-211 calls it under torch.no_grad():
 * eight 4x4 stride-2 convolutions, fp16 NHWC activations between them, fp16 MFMA with fp32 accumulation, and every
 * nn.BatchNorm2d (running statistics) folded by the caller into a per-channel fp32 scale / shift that the epilogue applies:
 *     y = act(acc * scale[co] + shift[co]), rounded once to fp16
 *     scale = gamma * rsqrt(running_var + eps), shift = beta + (conv_bias - running_mean) * scale   (no norm: 1, conv_bias)
 * The scale is NOT multiplied into the fp16 filter.  Pixels are flattened over the batch: no per-image work, no workspace.
 * Filters are packed ONCE per weight set into an opaque device blob.  Deterministic: fixed summation order, no atomics.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mstg_f16_plain_desc {
    int32_t kind;         /* 0: nn.Conv2d(k4,s2,p1); 1: nn.ConvTranspose2d(k4,s2,p1) */
    int32_t N, H, W, Cin; /* source (N,H,W,Cin) NHWC fp16 with Cin a multiple of 8 up to 512, or (N,3,H,W) NCHW fp32 (stem) */
    int32_t Ho, Wo, Cout; /* destination (N,Ho,Wo,Cout) NHWC fp16 with Cout a multiple of 8 up to 512, or (N,Cout,Ho,Wo) NCHW fp16, Cout <= 4 (head) */
    int32_t K;            /* 4 */
    int32_t src_nchw_f32; /* 1: the 3-channel fp32 image at the module boundary (kind 0 only) */
    int32_t dst_nchw;     /* 1: the output image */
    int32_t act;          /* MSTG_ACT_NONE / _RELU / _LEAKY02 / _TANH */
} mstg_f16_plain_desc;
size_t mstg_f16_plain_plan_bytes(const mstg_f16_plain_desc* d); /* size of the blob (N, H, W, Ho, Wo are not read); 0 = unsupported */
/* w: the layer's fp32 weight (OIHW, or IOHW for kind 1); scale / shift: fp32 [Cout] (nullable: 1 / 0) */
int mstg_f16_plain_pack(const mstg_f16_plain_desc* d, const float* w, const float* scale, const float* shift, void* blob,
                        size_t blob_bytes, void* stream);
int mstg_f16_plain_fwd(const mstg_f16_plain_desc* d, const void* blob, const void* x, void* y, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mixed-precision training step of the plain Generator (csrc/train_f16_plain.hip): what pretrain.py:159-166 runs under
 * torch.cuda.amp.autocast() on the layers of pretrain.py:60-97.  fp16 NHWC activations and activation gradients, fp16 MFMA,
 * fp32 accumulation and statistics, fp32 master parameters and parameter gradients.  The forward convolutions and all input
 * gradients are mstg_f16_plain_fwd launches (the input gradient of a k4 s2 p1 layer is the layer of the other kind on the same
 * weight tensor); the entry points below are the rest.  Fixed summation order, no atomics.
 * fstate: 2 floats on the device, {loss scale, 1 / loss scale}; istate: 3 ints, {skipped steps, good steps, last step ok}.
 * Activation gradients carry the loss scale; every parameter gradient is written multiplied by fstate[1].
 * P = N * H * W pixels of an NHWC fp16 tensor with C channels (a multiple of 8 up to 512).
 * ---------------------------------------------------------------------------------------------- */
/* (N,3,H,W) fp32 -> (N,H,W,8) fp16, channels 3..7 zero: the stem's input as its weight gradient reads it */
int mstg_f16_train_image_nhwc8(const float* img, void* out, int N, int H, int W, void* stream);
size_t mstg_f16_train_bn_workspace_bytes(size_t P, int C); /* for _bn_fwd, _bn_bwd and _bias_grad; 0 = unsupported */
/* nn.BatchNorm2d in training mode + activation: mean / rstd [C] out (biased variance of z as stored, two-pass), running statistics
 * (nullable) updated with the unbiased variance, y = act(gamma (z - mean) rstd + beta) rounded once to fp16 */
int mstg_f16_train_bn_fwd(const void* z, const float* gamma, const float* beta, size_t P, int C, int act, float eps, float momentum,
                          float* running_mean, float* running_var, float* mean, float* rstd, void* y, void* workspace,
                          size_t workspace_bytes, void* stream);
/* its backward: the activation mask is recomputed from z; dgamma / dbeta fp32 (times fstate[1]), dz fp16 */
int mstg_f16_train_bn_bwd(const void* z, const void* dy, const float* gamma, const float* beta, const float* mean, const float* rstd,
                          size_t P, int C, int act, const float* fstate, float* dgamma, float* dbeta, void* dz, void* workspace,
                          size_t workspace_bytes, void* stream);
/* dz = da * act'(a) from the OUTPUT a of a ReLU / LeakyReLU(0.2) (the stem has no norm); n fp16 elements, a multiple of 8 */
int mstg_f16_train_act_bwd(const void* a, const void* da, void* dz, size_t n, int act, void* stream);
size_t mstg_f16_train_loss_workspace_bytes(int N, int H, int W);
/* y: the head's fp16 image (N,3,H,W); real, mask: fp32 (N,3,H,W); k = 1 - mask.  loss = mean |y k - real k| (unscaled, fp32);
 * dz (N,H,W,8) fp16 = fstate[0] / numel * sign(y k - real k) * k * (1 - y^2), channels 3..7 zero */
int mstg_f16_train_head_loss_bwd(const void* y, const float* real, const float* mask, int N, int H, int W, const float* fstate,
                                 float* loss, void* dz, void* workspace, size_t workspace_bytes, void* stream);
/* Weight gradient of a k4 s2 p1 layer of either kind.  S: the layer's small map (N,h,w,Cs), B: its big map (N,2h,2w,Cb), NHWC fp16;
 * dW (Cs, CbOut, 4, 4) fp32 = fstate[1] * sum S[n][y][x][s] * B[n][2y+ky-1][2x+kx-1][b].  nn.Conv2d: S = dZ, B = X (dW is OIHW);
 * nn.ConvTranspose2d: S = X, B = dZ (dW is IOHW).  CbOut <= Cb: channels of B that are padding (image / head: 3 of 8). */
size_t mstg_f16_train_wgrad_workspace_bytes(int N, int h, int w, int Cs, int Cb, int CbOut); /* 0 = unsupported */
int mstg_f16_train_wgrad(const void* S, const void* B, int N, int h, int w, int Cs, int Cb, int CbOut, const float* fstate, float* dW,
                         void* workspace, size_t workspace_bytes, void* stream);
/* out[c] = fstate[1] * sum over pixels of dz[p][c], c < Cvalid: the bias gradients of the stem and the head */
int mstg_f16_train_bias_grad(const void* dz, size_t P, int C, int Cvalid, const float* fstate, float* out, void* workspace,
                             size_t workspace_bytes, void* stream);
/* norm: pre-clip gradient norm (device).  Finite: istate = {., +1, 1}.  Else istate = {+1, ., 0} and the loss scale is halved. */
int mstg_f16_train_scale_update(const float* norm, float* fstate, int* istate, void* stream);
/* mstg_adam_step_flat at step = step_base + istate[1]; does nothing when istate[2] == 0 */
int mstg_f16_train_adam(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                        int step_base, const int* istate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mixed-precision multi-style loss (csrc/style_f16.hip; style_loss.py precision="mixed"): the frozen VGG-topology stack, its
 * max-pools and the Gram matrices with fp16 features in the forward and bf16 gradients in the backward, fp32 accumulation
 * everywhere.  bf16 has fp32's exponent range, so the gradients (1e-7 and below) need no loss scale.  NHWC activations, 64-bit
 * offsets, fixed summation order, no atomics, no split-K: two launches give the same bits, and image i of a batch equals the same
 * image run alone.
 * ---------------------------------------------------------------------------------------------- */
#define MSTG_STYLE16_F16 0
#define MSTG_STYLE16_BF16 1
typedef struct mstg_style16_conv_desc {
    int32_t dtype;        /* MSTG_STYLE16_F16 / _BF16: operands, the NHWC source and the NHWC destination */
    int32_t N, H, W;      /* 3x3, stride 1, padding 1: the destination has the source's H and W; any N, H, W >= 1 */
    int32_t Cin;          /* a multiple of 16 up to 512; 3 with src_nchw_f32 */
    int32_t Cout;         /* a multiple of 16 up to 512; 3 with dst_nchw_f32 */
    int32_t src_nchw_f32; /* 1: the stem reads the (N,3,H,W) fp32 image and rounds it to `dtype` while staging */
    int32_t dst_nchw_f32; /* 1: the image gradient, written as (N,3,H,W) fp32 */
    int32_t flip;         /* pack only. 0: w is this convolution's filter (Cout,Cin,3,3).  1: w is the filter (Cin,Cout,3,3) of the
                           * layer whose INPUT gradient this convolution computes: read flipped and transposed */
    int32_t relu;         /* 1: ReLU behind the bias */
} mstg_style16_conv_desc;
/* size of the packed filter (N, H, W are not read); 0 = unsupported, mstg_last_error() names the reason */
size_t mstg_style16_conv_plan_bytes(const mstg_style16_conv_desc* d);
/* the kernel variant (tile shape) a launch of d takes, e.g. "style_conv16_kernel<f16,2,4,0>" = <dtype, 64-pixel fragments rows per
 * block / 64, 16-channel fragments per block, stem>; the launch reads the same choice.  nullptr = unsupported. */
const char* mstg_style16_conv_kernel_name(const mstg_style16_conv_desc* d);
/* w: fp32 (see flip), rounded once to `dtype`; bias: fp32 [Cout], nullable (zero) */
int mstg_style16_conv_pack(const mstg_style16_conv_desc* d, const float* w, const float* bias, void* blob, size_t blob_bytes,
                           void* stream);
/* y = [mask > 0] * relu?(conv(x) + bias), rounded once.  mask (nullable): fp16 NHWC of the destination's shape -- the saved input
 * activation of the layer whose input gradient this is; -0.0 and +0.0 both count as not > 0.  No mask with dst_nchw_f32. */
int mstg_style16_conv_fwd(const mstg_style16_conv_desc* d, const void* blob, const void* x, const void* mask, void* y, void* stream);
/* F.max_pool2d(x, 2) on fp16 NHWC, H and W even, C a multiple of 8; window order and first-maximum rule of mstg_maxpool2x2_fwd */
int mstg_style16_maxpool_fwd(const void* x, void* y, unsigned char* idx, int N, int H, int W, int C, void* stream);
/* dx (N,H,W,C) bf16 = dy (N,H/2,W/2,C) bf16 routed through idx; mask (nullable): fp16 (N,H,W,C), dx = 0 where mask is not > 0 */
int mstg_style16_maxpool_bwd(const void* dy, const unsigned char* idx, const void* mask, void* dx, int N, int H, int W, int C,
                             void* stream);
/* G[n] = scale * F[n]^T F[n], F fp16 (N,HW,C), C a multiple of 16 up to 512, G fp32 (N,C,C); fixed-order slab reduction */
size_t mstg_style16_gram_workspace_bytes(int N, int HW, int C);
int mstg_style16_gram_fwd(const void* f, float* g, int N, int HW, int C, float scale, void* workspace, size_t workspace_bytes,
                          void* stream);
/* dF = [F > 0] * (scale * F (dG + dG^T) + incoming), rounded once to bf16.  F fp16, dG fp32, incoming (nullable) bf16 (N,HW,C).
 * No fp16 intermediate: F is split exactly into two bf16 terms, dG + dG^T into a bf16 head and tail (three bf16 MFMA products). */
size_t mstg_style16_gram_bwd_workspace_bytes(int N, int C);
int mstg_style16_gram_bwd(const void* f, const float* dg, const void* incoming, void* df, int N, int HW, int C, float scale,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * fp16 inference of StructuralTransformerBlock (structural_transformer.py:55-74), csrc/infer_f16_block.hip: fp16 storage and MFMA
 * operands, fp32 accumulation / statistics / softmax, tokens (N, L, C) token-major.  Fixed summation order, no atomics: image i
 * of a batch equals the same image run alone.
 * ---------------------------------------------------------------------------------------------- */
/* token GEMM, nn.Linear over N * L tokens (qkv :69, proj :71, fc1 :73, fc2 :74): y = epi(x W^T + b), x fp16 (N, L, Cin) with Cin in
 * {64, 128, 256, 512}, Cout a multiple of 64 up to 768.  act: MSTG_ACT_NONE or MSTG_ACT_GELU (exact erf); residual (nullable):
 * fp32 (N, L, Cout) added behind the activation; y fp16 (out_f16) or fp32.  The blob (fp32 bias + fp16 filter) is packed once. */
size_t mstg_f16_linear_plan_bytes(int Cin, int Cout); /* 0 = unsupported (mstg_last_error says why) */
int mstg_f16_linear_pack(const float* w /* (Cout, Cin) */, const float* b /*nullable*/, int Cin, int Cout, void* blob,
                         size_t blob_bytes, void* stream);
int mstg_f16_linear_fwd(const void* blob, const void* x, const float* residual /*nullable*/, void* y, int N, int L, int Cin,
                        int Cout, int act, int out_f16, void* stream);
/* u = (LayerNorm(h) * gamma + beta) * (1 + g[n]) + b[n] as fp16 (N, L, dim), dim in {64, 128, 256}, statistics in fp32 (:68, :72).
 * h = x (fp16 if x_f16, else fp32), or with smap (N, L, 4) fp32: h = x + (sp_b + sp_w s) (struct_proj, :65), written to h_out
 * (fp32, nullable).  gb (nullable): style_mod's fp32 output (N, 2 dim) = g | b. */
int mstg_f16_ln_mod_fwd(const void* x, int x_f16, const float* smap /*nullable*/, const float* sp_w, const float* sp_b,
                        const float* gamma, const float* beta, const float* gb /*nullable*/, float* h_out /*nullable*/, void* u,
                        int N, int L, int dim, float eps, void* stream);
/* out (N, dim) fp32 = mean over the L tokens of x fp16 (N, L, dim) (AdaptiveAvgPool2d(1) of the style encoder) */
size_t mstg_f16_token_mean_workspace_bytes(int N, int L, int dim);
int mstg_f16_token_mean(const void* x, float* out, int N, int L, int dim, void* workspace, size_t workspace_bytes, void* stream);
/* softmax(q k^T / sqrt(D)) v per head over all L tokens (:70): qkv fp16 (N, L, 3 heads D) q | k | v, out fp16 (N, L, heads D);
 * D in {16, 32, 64}; inference only (no log-sum-exp) */
int mstg_f16_flash_attn_fwd(const void* qkv, void* out, int N, int L, int heads, int D, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mixed-precision attention of StructuralTransformerBlock for TRAINING (structural_transformer.py:70), csrc/flash_f16_train.hip;
 * ops.flash_attention(qkv, heads, precision="mixed").  16-bit MFMA operands, fp32 accumulation, fp32 softmax, fp32 results.
 * qkv fp32 (N, L, 3 heads D) q | k | v, scale = 1 / sqrt(D), D in {16, 32, 64}: D = 8 is refused by name (MSTG_E_UNSUPPORTED,
 * the width in mstg_last_error()) -- mstg_flash_attn_fwd/bwd serve it.  Contract:
 *   cast      qh = fp16(qkv), qb = bf16(qkv), round-to-nearest-even from the fp32 values; the caller keeps these, not qkv
 *   forward   S = q_h k_h^T (fp32 accumulation); p = exp(scale (S - m)) in fp32; l sums the fp32 p; P is rounded to fp16 once for
 *             P v_h; out = O / l (fp32); lse = scale m + ln l (fp32, (N, heads, L))
 *   backward  dO_b = bf16(dO); S recomputed from qh, P = exp(scale S - lse) in fp32; dP = dO_b v_b^T; dV = bf16(P)^T dO_b;
 *             delta = sum_keys P dP in fp32, from the same P and dP that dS is made of (a first sweep of the dQ kernel) -- NOT
 *             sum_d dO out of the fp32 tensors: that sum sees other roundings of the operands than dP does, so a row of dS would
 *             not sum to zero (with one token dq and dk come out at 3e-3 instead of 0), and the saved out is not needed;
 *             dS = bf16(P (dP - delta)), the product in fp32, rounded once; dQ = scale dS k_b; dK = scale dS^T q_b; dqkv fp32.
 *             bf16 has fp32's range: no loss scale, no state.
 * Fixed summation order, no atomics: image i of a batch gives the bits of the same image run alone.
 * Not built: 16-bit training forms of the block's Linear layers, LayerNorm and GELU (they stay on the fp32 kernels); D = 8.
 * ---------------------------------------------------------------------------------------------- */
/* (:70) qh fp16 and qb bf16 (N, L, 3 heads D), both from the fp32 qkv in one pass */
int mstg_f16_attn_cast_qkv(const float* qkv, void* qh, void* qb, int N, int L, int heads, int D, void* stream);
/* (:70) forward of the contract above from qh: out fp32 (N, L, heads D), lse fp32 (N, heads, L) */
int mstg_f16_flash_attn_train_fwd(const void* qh, float* out, float* lse, int N, int L, int heads, int D, void* stream);
/* (:70) backward of the contract above: dqkv fp32 (N, L, 3 heads D) = dq | dk | dv, every element written.  The caller-owned
 * workspace holds delta (N, heads, L) fp32 and dO_b (N, L, heads D) bf16; launches: cast of dO, delta + dQ, dK/dV. */
size_t mstg_f16_flash_attn_train_bwd_workspace_bytes(int N, int L, int heads, int D);
int mstg_f16_flash_attn_train_bwd(const void* qh, const void* qb, const float* lse, const float* d_out, float* dqkv,
                                  void* workspace, size_t workspace_bytes, int N, int L, int heads, int D, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Image pre/post-processing of the callers either side of the generator, on the device (8-bit RGB, HWC, 3 bytes per pixel).
 * Replaces PIL / torchvision / numpy work in MonetPhotoDataset (pretrain.py:32-57) and process_cyclegan
 * (batch_process_images.py:183-233).  Integer work: bit-exact against Pillow.
 *   filter 0 = BILINEAR (torchvision Resize on a PIL image), 1 = LANCZOS; ksize / coefficient tables follow Pillow's
 *   Resample.c (precompute_coeffs + normalize_coeffs_8bpc) and are computed on the HOST: kk and bounds are HOST pointers,
 *   the caller copies the tables to the device and passes the device copies to the two passes below.
 * ---------------------------------------------------------------------------------------------- */
int mstg_resample_ksize(int in_size, int out_size, int filter);
int mstg_resample_coeffs(int in_size, int out_size, int filter, int* kk /* host [out_size][ksize] */, int* bounds /* host [out_size][2] */);
/* horizontal pass over source rows [y0, y0 + rows): dst (rows, out_w, 3); vertical pass: dst (out_h, w, 3) */
int mstg_resample_h_u8(const unsigned char* src, unsigned char* dst, int src_w, int y0, int rows, int out_w, int ksize,
                       const int* kk, const int* bounds, void* stream);
int mstg_resample_v_u8(const unsigned char* src, unsigned char* dst, int w, int out_h, int ksize, const int* kk, const int* bounds,
                       void* stream);
/* dst (dh, dw): filled with `fill` (if >= 0), then the (ch, cw) window of src at (sy0, sx0) pasted at (dy0, dx0): Image.new +
 * Image.paste (batch_process_images.py:196-199) and Image.crop (:221-233) */
int mstg_paste_u8(const unsigned char* src, int sh, int sw, int sy0, int sx0, int ch, int cw, unsigned char* dst, int dh, int dw,
                  int dy0, int dx0, int fill, void* stream);
/* ToTensor + Normalize(0.5, 0.5) of the (H, W) window at (y0, x0) -> out (3, H, W) fp32, times the 8x8-grid mask (bit i*8+j of
 * `grid` set = cell kept) when use_mask (pretrain.py:44-57); image_out / mask_out (nullable): unmasked image / the mask */
int mstg_u8_to_tensor(const unsigned char* src, int sh, int sw, int y0, int x0, int H, int W, float* out, float* image_out,
                      float* mask_out, unsigned long long grid, int use_mask, void* stream);
/* (y + 1) / 2 -> clamp(0, 1) -> * 255 -> uint8: y (3, H, W) fp32 -> dst (H, W, 3) (batch_process_images.py:213-217) */
int mstg_tensor_to_u8(const float* y, int H, int W, unsigned char* dst, void* stream);
/* Per-pixel blend of the letterboxed original with the styled image (uint8 HWC both), bit-exact with numpy's float64 evaluation:
 * out = clip(orig * (1 - w) + styled * w, 0, 255).astype(uint8).  weight_map == NULL: w = strength everywhere and
 * one_minus_strength is the caller's double 1 - strength (process_local_style mode 'simple', batch_process_images.py:304-312);
 * else w = weight_map[y][x] (float64, H x W: the 'enhanced' / 'advanced' weight-map blend of :340-342 / :386-387 followed by the
 * clip + cast of :352 -- the caller's own map, or the one mstg_local_style_weight_map builds from the canvas). */
int mstg_blend_u8(const unsigned char* orig, const unsigned char* styled, double one_minus_strength, double strength,
                  const double* weight_map /*nullable*/, unsigned char* out, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Batched image pipeline (csrc/image_batch.hip): the steps above for N images of different sizes per launch, byte-identical to
 * the one-image entry points.  Folder inference (batch_process_images.py:176-236, :255-441) and MonetPhotoDataset batches.
 *
 * One descriptor per image and per direction (pre: image -> T x T canvas; post: canvas -> image), built on the host:
 *   box     the part of `src` that is resampled (pre: the whole image; post: the crop box of the canvas);
 *   rs      the size the box is resampled to with `filter`; a pass whose size does not change copies (ks_* = 0);
 *   win     the window of the resampled image that is wanted (letterbox: all of it; dataset item: the centre crop);
 *   dst     where the window lands in the T x T canvas (tensor output only), `fill` = the byte outside it;
 *   tables  kk [rs][ks] and bounds [rs][2] of mstg_resample_coeffs(box, rs, filter) per direction, as int32 indices into ONE
 *           packed table buffer (host copy for validation, device copy for the kernels);
 *   inter   the horizontal pass writes columns [win_x, win_x + win_w) of box rows [y_first, y_first + irows) -- the rows the
 *           vertical pass reads for the window -- as 8-bit rows of `ipitch` bytes (multiple of 4, >= 3 win_w) at byte
 *           `inter_off` (multiple of 4) of one ragged intermediate buffer;
 *   out_off byte offset of the (win_h, win_w, 3) result in the ragged output buffer (u8 output only).
 * Work is distributed by a host-built tile list, four int32 per tile: {image, y0, x0, extent}.  mstg_img_batch_tiles sizes each
 * image's tiles so that a tile's source segment and coefficient window fit the kernel's LDS, and refuses (UNSUPPORTED, naming
 * the image) a reduction factor for which no tile does.  The kernels check every tile against its descriptor before they touch
 * memory.  Integer sums with the 2^21 rounding term, fixed order, no atomics.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mstg_img_desc {
    const unsigned char* src; /* device: (src_h, src_w, 3) */
    int32_t src_h, src_w;
    int32_t box_y, box_x, box_h, box_w;
    int32_t rs_h, rs_w, filter;
    int32_t win_y, win_x, win_h, win_w;
    int32_t dst_y, dst_x, fill;
    int32_t ks_h, ks_v;
    int32_t y_first, irows, ipitch;
    int64_t kk_h, bounds_h, kk_v, bounds_v;
    int64_t inter_off, out_off;
    uint64_t grid; /* 8x8 keep-mask of this image (tensor output with use_mask) */
} mstg_img_desc;
#define MSTG_IMG_PASS_H 0        /* tiles of the intermediate: 4 rows x extent columns */
#define MSTG_IMG_PASS_V_TENSOR 1 /* tiles of the canvas: extent rows x 64 columns */
#define MSTG_IMG_PASS_V_U8 2     /* tiles of the window: extent rows x 64 columns */
/* Host only, touches no device: windows inside their images, positive sizes, table / intermediate / output extents inside the
 * buffers given, every bounds entry inside its source, non-null pointers.  canvas = T for the tensor output, 0 for the ragged
 * uint8 output of `out_bytes`.  A refusal names the image index in mstg_last_error.  Every launch entry below calls it first. */
int mstg_img_batch_validate(const mstg_img_desc* descs, int n, const int32_t* table, size_t table_len, size_t inter_bytes, int canvas,
                            size_t out_bytes);
/* number of tiles of `pass` (negative: error); writes them when tiles != NULL (cap = tiles the buffer holds) */
int mstg_img_batch_tiles(const mstg_img_desc* descs, int n, const int32_t* table, size_t table_len, int pass, int canvas,
                         int32_t* tiles, size_t cap);
/* descs / table: host copies; descs_dev / tiles_dev / table_dev: the same bytes on the device */
int mstg_img_batch_resample_h(const mstg_img_desc* descs, int n, const int32_t* table, size_t table_len, const void* descs_dev,
                              const int32_t* tiles_dev, int ntiles, const int32_t* table_dev, unsigned char* inter, size_t inter_bytes,
                              void* stream);
/* vertical pass + placement + fill + ToTensor / Normalize: out (n, 3, T, T) fp32; use_mask: out is the masked image and
 * image_out / mask_out (nullable) the unmasked image / the mask; canvas_u8 (nullable): the (n, T, T, 3) uint8 canvas */
int mstg_img_batch_resample_v_tensor(const mstg_img_desc* descs, int n, const int32_t* table, size_t table_len, const void* descs_dev,
                                     const int32_t* tiles_dev, int ntiles, const int32_t* table_dev, const unsigned char* inter,
                                     size_t inter_bytes, int T, float* out, float* image_out, float* mask_out, unsigned char* canvas_u8,
                                     int use_mask, void* stream);
/* vertical pass into the ragged uint8 output */
int mstg_img_batch_resample_v_u8(const mstg_img_desc* descs, int n, const int32_t* table, size_t table_len, const void* descs_dev,
                                 const int32_t* tiles_dev, int ntiles, const int32_t* table_dev, const unsigned char* inter,
                                 size_t inter_bytes, unsigned char* out, size_t out_bytes, void* stream);
/* mstg_tensor_to_u8 for a batch: y (N, 3, H, W) fp32 or fp16 (is_f16; widened exactly) -> dst (N, H, W, 3) */
int mstg_img_batch_tensor_to_u8(const void* y, int is_f16, int N, int H, int W, unsigned char* dst, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Image-quality metrics of the reference's evaluation scripts (compare_image_quality.py:14-33, image_quality_comparison.py:11-34,
 * complete_comparison.py:13-32, improved_image_compare.py:8-27), on the device: a, b = two batches of 8-bit RGB images
 * (N, H, W, 3), contiguous; out[n] = {mse, psnr, ssim, ssim_c0, ssim_c1, ssim_c2} (fp64) of pair n on the images / 255:
 *   mse  = np.mean((a - b) ** 2) = SSD / (255^2 H W 3) from the exact integer sum of squared byte differences;
 *   psnr = skimage peak_signal_noise_ratio(data_range=1) = 10 log10(1 / mse), +inf for equal images;
 *   ssim = skimage structural_similarity(channel_axis=2, data_range=1): uniform 7x7 window, sample covariance (49 / 48),
 *          K1 = 0.01, K2 = 0.03, mean over the (H - 6)(W - 6) windows inside the image per channel, ((c0 + c1) + c2) / 3.
 * Window sums are exact integers, S is formed in fp64, sums run in a fixed order without atomics: results are bit-identical from
 * run to run and do not depend on N.  H, W >= 7 (BADARG names the window otherwise); H * W * 3 < 2^31 (else UNSUPPORTED).
 * A workgroup takes MSTG_METRICS_TILE_H x MSTG_METRICS_TILE_W windows; the workspace holds four 8-byte words per tile.
 * ---------------------------------------------------------------------------------------------- */
#define MSTG_METRICS_TILE_H 16
#define MSTG_METRICS_TILE_W 64
size_t mstg_image_metrics_workspace_bytes(int N, int H, int W); /* 0 for an invalid shape */
int mstg_image_metrics_u8(const unsigned char* a, const unsigned char* b, int N, int H, int W, double* out /* [N][6] */,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mixed-size image comparison (csrc/compare.hip).  When the processed image and the original differ in shape, the reference's
 * four folder-comparison scripts resize the processed one with cv2.resize(img, (W, H)) -- the 8-bit INTER_LINEAR -- and only then
 * measure (compare_image_quality.py:100-106, :299-301, image_quality_comparison.py:17-18, complete_comparison.py:16-17,
 * improved_image_compare.py:11-12).  The resize is restated from its definition below, as recalled, not compared with an OpenCV
 * binary (tests/cv_resize_ref.py is the same restatement in numpy).
 *
 * cv2.resize(src, (Wd, Hd)) of an 8-bit image, INTER_LINEAR, per channel.
 *   Per axis, source extent s >= 1, destination extent d >= 1:
 *        scale = 1.0 / ((double)d / (double)s)   (both divisions in double: OpenCV forms inv_scale and then its reciprocal);
 *        for i = 0 .. d-1: f = (float)((i + 0.5) * scale - 0.5) (double arithmetic, a product and a difference, ONE rounding to
 *        float); p = floor(f); f = f - (float)p (a float subtraction);
 *        HORIZONTAL axis only: p < 0 -> p = 0, f = 0; p >= s - 1 -> p = s - 1, f = 0;
 *        w0 = (short)rint((1.f - f) * 2048.f), w1 = (short)rint(f * 2048.f): float operations, each rounded, ties to even,
 *        saturated to int16.
 *   Horizontal pass on a source row S: q = min(p + 1, s - 1); T[x] = S[p] * w0 + S[q] * w1 in int32.
 *   Vertical pass: the rows are clamp(p, 0, s-1) and clamp(p + 1, 0, s-1); the weights b0, b1 come from the UNCLAMPED fraction and
 *        are not reset at the borders (that asymmetry is the library's);
 *        out = (uchar)((((b0 * (T0 >> 4)) >> 16) + ((b1 * (T1 >> 4)) >> 16) + 2) >> 2).
 *   The result is a pure function of four source bytes and four weights: nothing separable has to be stored.  Equal extents give
 *   the identity, an exact 2x reduction gives (a + b + c + d + 2) >> 2 (what OpenCV's switch to its area path computes at that
 *   ratio, so there is no special case).
 *   w0 + w1 == 2048 whenever d <= 4096: f * 2048 is exact; 1 - f is exact unless p == 0, and there the unrounded position lies
 *   either on a point (k + 0.5) / 2048 or at least 1 / (4096 d) >= 2^-24 from it, so f (rounded by at most 2^-26) stays more than
 *   2^-25 from it, which is the most 1 - f can lose: the two rint never disagree.  With both sums 2048 the value before the cast
 *   lies in 0..255 and the cast changes nothing (tests/test_compare_cpu.py holds both).  For larger d a sum of 2049 is conceivable;
 *   the cast is C's conversion of an int to unsigned char, the low 8 bits, and that is what the kernels store (the value stays
 *   below 256 there too: 255 * (2049 / 2048)^2 < 255.3).
 *
 * mstg_cv_resize_coeffs: HOST only, touches no device; the table above for one axis, index[dst] and weights[dst][2] = {w0, w1}.
 * It is the one place where the double and float steps are evaluated: the tables are built on the host and uploaded.
 * DEVICE TABLE of an axis: int32 [2 dst] = index[dst] followed by the bytes of weights[dst][2] (one int32 per pair, w0 low).
 * The kernels clamp every index to its source before they use it.
 *
 * mstg_cv_resize_linear_u8: src (N, Hs, Ws, 3) -> dst (N, Hd, Wd, 3), contiguous, one launch, 64-bit offsets; table_v / table_h =
 * device tables of (Hs -> Hd, vertical) and (Ws -> Wd, horizontal).  H * W * 3 < 2^31 for both shapes, N <= 65535; the output
 * must not overlap the input (BADARG).
 *
 * mstg_pair_metrics_u8: out[P][6] (fp64, the meaning of mstg_image_metrics_u8's rows) for P pairs (a_i, b_i) of ANY shapes, where
 * b_i is resized to a_i's shape by the definition above while its patch is staged -- the resized image is never written to
 * memory; a pair of equal shape is staged as mstg_image_metrics_u8 stages it.  TWO launches whatever P and however many distinct
 * shapes: MSTG_PAIR_METRICS_LAUNCHES = tiles, finish.  One descriptor per pair; one host-built tile list, four int32 per tile
 * {pair, ty, tx, 0}, pair after pair, each pair's tiles in the row-major order of mstg_image_metrics_u8 on a_i; the workspace holds
 * four 8-byte words per tile; `table` = the device tables of the resized pairs packed in one int32 buffer (host copy for
 * validation, device copy for the kernels).  The kernels check every tile against its descriptor before they touch memory.
 * Row i is BIT FOR BIT mstg_image_metrics_u8(a_i, mstg_cv_resize_linear_u8(b_i)): the same tile decomposition of a_i, every sum
 * in the same fixed order, no atomics; it does not depend on P or on the order of the pairs.  The same image may appear in any
 * number of pairs.
 * Refused, naming the pair index and the value in mstg_last_error: an extent below 1 (BADARG); a smaller than the 7x7 SSIM window
 * (BADARG); H * W * 3 >= 2^31 for either image (UNSUPPORTED); a total tile count above 2^24 - 1, the workgroups of one launch --
 * which covers every count that does not fit int32 (UNSUPPORTED).
 * ---------------------------------------------------------------------------------------------- */
#define MSTG_PAIR_METRICS_LAUNCHES 2
typedef struct mstg_pair_desc {
    const unsigned char* a; /* device: (ha, wa, 3), contiguous */
    const unsigned char* b; /* device: (hb, wb, 3), contiguous */
    int32_t ha, wa, hb, wb;
    int32_t tile0, ntiles;    /* first tile of the pair in the tile list and its tile count (mstg_pair_metrics_tiles fills them) */
    int64_t table_v, table_h; /* int32 index of the device tables (hb -> ha, vertical) and (wb -> wa, horizontal) in the packed
                                 table buffer; not read for a pair of equal shape */
} mstg_pair_desc;
int mstg_cv_resize_coeffs(int src, int dst, int horizontal, int32_t* index, int16_t* weights /* [dst][2] */);
int mstg_cv_resize_linear_u8(const unsigned char* src, int N, int Hs, int Ws, int Hd, int Wd, const int32_t* table_v,
                             const int32_t* table_h, unsigned char* dst, void* stream);
/* Host only, touches no device: the refusals above, non-null image pointers, tile0 / ntiles as mstg_pair_metrics_tiles fills
 * them, table offsets inside `table_len` words and (table != NULL) every index inside its source.  A refusal names the pair
 * index.  mstg_pair_metrics_u8 calls it first. */
int mstg_pair_metrics_validate(const mstg_pair_desc* descs, int P, const int32_t* table, size_t table_len);
size_t mstg_pair_metrics_workspace_bytes(const mstg_pair_desc* descs, int P); /* from the shapes alone; 0 for a refused set */
/* fills tile0 / ntiles of every descriptor and returns the number of tiles (negative: error); writes the tile list when
 * tiles != NULL (cap = tiles the buffer holds) */
int mstg_pair_metrics_tiles(mstg_pair_desc* descs, int P, int32_t* tiles, size_t cap);
/* descs / table: host copies; descs_dev / tiles_dev / table_dev: the same bytes on the device (8 / 16 / 4-byte aligned) */
int mstg_pair_metrics_u8(const mstg_pair_desc* descs, int P, const int32_t* table, size_t table_len, const void* descs_dev,
                         const int32_t* tiles_dev, int ntiles, const int32_t* table_dev, double* out /* [P][6] */, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The per-pixel weight map of process_local_style(mode='enhanced') (batch_process_images.py:312-342, detect_sky :126-150; the same
 * map with coefficient 0.4 in mode 'advanced', :355-384), built on the device for N canvases (N, H, W, 3) uint8 in three launches
 * whatever N.  OpenCV's 8-bit integer algorithms are restated from their definitions (not compared with an OpenCV binary):
 *   gray  = cv2.cvtColor(COLOR_RGB2GRAY) (:321)        = (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14;
 *   sky   = detect_sky's mask (:134-144)               = (v > 150) & (s < 100) with v = max(R, G, B), diff = v - min(R, G, B),
 *           s = (diff * sdiv[v] + 2048) >> 12, sdiv[0] = 0, sdiv[i] = round-half-even(1044480 / i) (8-bit COLOR_RGB2HSV);
 *   state = cv2.Canny(gray, 50, 150) before hysteresis (:322): 3x3 Sobel with replicated borders, m = |dx| + |dy| (0 outside the
 *           image); for m > 50 with x = |dx|, y = |dy| << 15, t = x * 13573: y < t keeps m > m[left] && m >= m[right];
 *           y > t + (x << 16) keeps m > m[up] && m >= m[down]; else s = (dx ^ dy) < 0 ? -1 : 1 keeps m > m[y-1][x-s] && m > m[y+1][x+s];
 *           state byte 2 = kept and m > 150, 0 = kept (a candidate), 1 = everything else;
 *   edge  = the hysteresis of Canny: 1 where a 2 is reached from the pixel through 8-connected states != 1;
 *   detail = scipy.ndimage.gaussian_filter(edge.astype(float), sigma=2) > 0.1 (:327): float64, radius 8, 'reflect', axis 0 then 1;
 *   has_sky = (double)count / (double)(H * W) > 0.7 (:147), read on the device;
 *   weight = w_base; = w_sky where has_sky && sky (:333-334); = w_detail where detail (:337-338, assigned last).
 * The caller computes the three weights as the reference does: strength, min(strength + 0.2, 1.0), max(strength - 0.3 * detail, 0.0).
 * All masks are (N, H, W) bytes holding 0 / 1.  Integer arithmetic up to the Gaussian, a fixed summation order, no
 * floating-point atomics: bit-reproducible.  The hysteresis keeps one byte per pixel of an image in LDS: H * W <=
 * MSTG_LOCAL_STYLE_MAX_PIXELS, else MSTG_E_UNSUPPORTED (the message names the size); prepare and weights take any H, W >= 1.
 *
 * The finish of the mode (:342-352), one more launch: the blend with that map and the two optional steps.  Per image: orig, styled
 * uint8 (H, W, 3), weight float64 (H, W), detail bytes 0 / 1 (H, W), flags enhance_colors and smooth.
 *   x   = orig * (1 - w) + styled * w in float64 exactly as mstg_blend_u8 forms it: two rounded products, one rounded sum, no
 *         fused multiply-add.  Without enhance_colors the result is mstg_blend_u8's clip and truncation, byte for byte.
 *   e   = cv2.convertScaleAbs(x, alpha=1.1, beta=5) (:346) = sat_u8(rint_half_even(|fmaf((float)x, 1.1f, 5.0f)|)) per channel:
 *         the double narrowed to float32 (round to nearest), ONE fused multiply-add with the float32 constants, absolute value,
 *         round half to even, saturation to 0..255.  This restates OpenCV 4.x's cvtabs for CV_64F -> CV_8U on a build with FMA
 *         lanes (not compared with an OpenCV binary); plain float64 or unfused float32 evaluation differs on a fraction of a
 *         percent of the bytes, never by more than one grey level (tests/test_local_style_finish_cpu.py measures it).
 *   smooth_transitions(e, detail, radius=3) (:152-174, :350), only together with enhance_colors, so e is uint8:
 *         dil = max, ero = min of detail over the 9 x 9 window clipped to the image (cv2.dilate / cv2.erode with a 5 x 5 box,
 *         two iterations, default border: neutral); boundary = dil != ero;
 *         blur = cv2.GaussianBlur(e, (7, 7), 0), OpenCV's bit-exact 8-bit path: integer taps {8, 28, 56, 72, 56, 28, 8} (the
 *         sigma <= 0 table of size 7 in 8.8 fixed point, sum 256) along x, then along y; BORDER_REFLECT_101 (index p outside
 *         [0, len) mirrored without repeating the edge pixel, repeatedly if need be; len == 1 gives 0); the horizontal sums stay
 *         exact in 16 bits (<= 65280); blur = (sum + 32768) >> 16;
 *         out = boundary ? (e + blur) >> 1 : e for all three channels (the reference assigns the float64 0.5 * a + 0.5 * b into a
 *         uint8 array, which truncates; its final clip + cast changes nothing).
 * mstg_local_style_finish takes any H, W >= 1; out must not overlap an input (MSTG_E_BADARG).  Still not built:
 *   - smooth without enhance_colors: there cv2.GaussianBlur runs on the float64 blend and is truncated right at integers that flat
 *     regions hit exactly (the sky weight 1.0), so OpenCV's float64 summation order decides bytes: MSTG_E_UNSUPPORTED, by name;
 *   - mode 'advanced' (the reference itself raises there: cv2.cvtColor on a float64 array, :391);
 *   - a comparison of any of these restatements with an OpenCV binary.
 * ---------------------------------------------------------------------------------------------- */
#define MSTG_LOCAL_STYLE_MAX_PIXELS 147456 /* 144 KiB of the 160 KiB of LDS of a CU: 256 x 256, up to 384 x 384 */
/* bytes mstg_local_style_weight_map needs for (N, H, W); 0 for an invalid or unsupported shape (mstg_last_error says which) */
size_t mstg_local_style_workspace_bytes(int N, int H, int W);
/* stage A: state map, sky mask, sky_count[n] = number of sky pixels of image n (zeroed here, then integer atomics), and the gray
 * plane where gray != NULL */
int mstg_local_style_prepare(const unsigned char* canvas, int N, int H, int W, unsigned char* state, unsigned char* sky, int* sky_count,
                             unsigned char* gray /*nullable*/, void* stream);
/* stage B: state map in (any byte other than 0 and 2 counts as 1), edge mask out; one workgroup per image */
int mstg_local_style_hysteresis(const unsigned char* state, int N, int H, int W, unsigned char* edge, void* stream);
/* stage C: weight_map (N, H, W) float64 as mstg_blend_u8 consumes it, and the detail mask where detail != NULL */
int mstg_local_style_weights(const unsigned char* edge, const unsigned char* sky, const int* sky_count, int N, int H, int W, double w_base,
                             double w_sky, double w_detail, double* weight_map, unsigned char* detail /*nullable*/, void* stream);
/* the three stages on the caller's workspace (16-byte aligned, mstg_local_style_workspace_bytes) */
int mstg_local_style_weight_map(const unsigned char* canvas, int N, int H, int W, double w_base, double w_sky, double w_detail,
                                double* weight_map, void* workspace, size_t workspace_bytes, void* stream);
/* stage D: blend + enhance_colors + smooth as defined above; detail may be NULL when smooth == 0 */
int mstg_local_style_finish(const unsigned char* canvas, const unsigned char* styled, const double* weight_map,
                            const unsigned char* detail /*nullable iff !smooth*/, int N, int H, int W, int enhance_colors, int smooth,
                            unsigned char* out, void* stream);
/* bytes mstg_local_style_enhanced needs for (N, H, W); 0 for an invalid or unsupported shape (mstg_last_error says which) */
size_t mstg_local_style_enhanced_workspace_bytes(int N, int H, int W);
/* process_local_style(mode='enhanced') from the canvas: stages A-C and the finish on the caller's workspace (16-byte aligned; it
 * holds the map and the detail mask), four launches whatever N; same MSTG_LOCAL_STYLE_MAX_PIXELS limit as the weight map */
int mstg_local_style_enhanced(const unsigned char* canvas, const unsigned char* styled, int N, int H, int W, double w_base, double w_sky,
                              double w_detail, int enhance_colors, int smooth, unsigned char* out, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The finish of the STANDARD mode of the reference's application (gan_login_gui.py:817-868, standard_process_thread; every option
 * of that tab is on by default, :542, :554, :594, :612, :616), on the device for N images (N, H, W, 3) uint8, any H, W >= 1, N
 * images per launch, 64-bit offsets.  The OpenCV steps are restated from the definitions below (tests/standard_mode_ref.py is the
 * same restatement in numpy); NONE OF THEM HAS BEEN COMPARED WITH AN OPENCV BINARY.  For every neighbourhood stage (median,
 * bilateral, blur) `out` must not overlap an input: MSTG_E_BADARG.
 *
 *   blend (:820-828)     x = clip(styled * (1 - r) + canvas * r, 0, 255) truncated, in float64 with two rounded products and one
 *         rounded sum: mstg_blend_u8 with the operands swapped (orig = styled, styled = canvas, strength = r), byte for byte.  The
 *         caller passes 1 - r as its own double; r <= 0 skips the step, as the reference does.
 *   median (:835)        cv2.medianBlur(x, 3): per channel the median of the 9 samples of the 3 x 3 window, BORDER_REPLICATE
 *         (coordinates clamped to the image), integers; H or W of 1 follows from the same rule.
 *   bilateral (:838)     cv2.bilateralFilter(x, d, sigmaColor, sigmaSpace), OpenCV 4.x bilateralFilter_8u for three channels as
 *         recalled from its source:
 *           radius = max(d / 2, 1); d must be 3, 5, 7 or 9 (else MSTG_E_UNSUPPORTED, the message names d: d <= 0 would derive the
 *           radius from sigmaSpace, and improved_smooth.py:106 would need radius 90); a sigma <= 0 counts as 1;
 *           border: BORDER_REFLECT_101 (index p outside [0, len) mirrored without repeating the edge pixel, repeatedly for sides
 *           shorter than the radius; len == 1 gives 0);
 *           taps: (i, j) for i, then j, in -radius .. radius with sqrt(i * i + j * j) <= radius (49 taps at d = 9), sample
 *           (y + i, x + j); space[k] = (float)exp((i * i + j * j) * (-0.5 / sigmaSpace^2)) and
 *           color[t] = (float)exp(t * t * (-0.5 / sigmaColor^2)) for t = 0 .. 767, both evaluated in double on the HOST with
 *           std::exp (mstg_bilateral_tables) and uploaded by the caller: the device never evaluates exp;
 *           per pixel, in float32 and in tap order, with (b0, g0, r0) the centre sample: t = |b - b0| + |g - g0| + |r - r0|,
 *           w = space[k] * color[t] (one rounded product), wsum += w, sum_c = fmaf((float)c, w, sum_c) for the three channels;
 *           then inv = 1.0f / wsum (IEEE division) and out_c = sat_u8(rint_half_even(sum_c * inv)).
 *         This is the SIMD path of an OpenCV build with FMA lanes (the stance taken for convertScaleAbs above); an unfused sum, a
 *         division by wsum or a float64 evaluation differ on a fraction of the bytes, never by more than one grey level
 *         (tests/test_standard_mode_cpu.py measures the shares).
 *   colour step (:843-857) one 256-entry table per channel, lut[256 * channel + v], built on the host by mstg_standard_color_lut:
 *           photo_to_monet: channel 0 = (u8)clip(v * 1.1, 0, 255), channel 1 = (u8)clip(v * 1.05, 0, 255) in float64, truncated,
 *           channel 2 = v (the indices of the reference's code, not its comments);
 *           monet_to_photo: cv2.convertScaleAbs(alpha=1.1, beta=5) = sat_u8(rint_half_even(|fmaf((float)v, 1.1f, 5.0f)|)) on all
 *           three channels: the definition mstg_local_style_finish uses, here on uint8 input.
 *   blur (:859-868)      cv2.GaussianBlur(x, (k, k), 0) with k = 2 * smooth_level + 1, OpenCV's bit-exact 8-bit path: taps in 8.8
 *         fixed point, k = 3: {64, 128, 64}; k = 5: {16, 64, 96, 64, 16}; k = 7: {8, 28, 56, 72, 56, 28, 8}; along x, then along
 *         y; BORDER_REFLECT_101 as above; the row sums stay exact in 16 bits; out = (sum + 32768) >> 16.  smooth_level 4 .. 7
 *         (k = 9 .. 15) needs the taps of OpenCV's softfloat kernel generator, which are not restated: MSTG_E_UNSUPPORTED, the
 *         message names the level; the blur is never approximated.  Level 0 skips the step.
 * ---------------------------------------------------------------------------------------------- */
#define MSTG_BILATERAL_COLOR_WEIGHTS 768
#define MSTG_BILATERAL_MAX_TAPS 49
#define MSTG_BILATERAL_TABLE_FLOATS (MSTG_BILATERAL_COLOR_WEIGHTS + MSTG_BILATERAL_MAX_TAPS)
#define MSTG_STANDARD_PHOTO_TO_MONET 0
#define MSTG_STANDARD_MONET_TO_PHOTO 1
/* Host only: table[0 .. 767] = color[t], table[768 + k] = space[k] in tap order (entries past the last tap 0).  Returns the number of
 * taps (5, 13, 29, 49 for d = 3, 5, 7, 9) or a negative code. */
int mstg_bilateral_tables(int d, double sigma_color, double sigma_space, float* table /* [MSTG_BILATERAL_TABLE_FLOATS] */);
/* Host only: the colour step's three tables for MSTG_STANDARD_PHOTO_TO_MONET / MSTG_STANDARD_MONET_TO_PHOTO; anything else BADARG */
int mstg_standard_color_lut(int model_type, unsigned char* lut /* [768] */);
int mstg_median3_u8(const unsigned char* in, int N, int H, int W, unsigned char* out, void* stream);
/* table: the MSTG_BILATERAL_TABLE_FLOATS floats of mstg_bilateral_tables(d, sigmaColor, sigmaSpace) on the device.  Any other d,
 * d <= 0 and radii up to 90 (improved_smooth.py:106): mstg_bilateral_wide_u8 below, the same definition */
int mstg_bilateral_u8(const unsigned char* in, int N, int H, int W, int d, const float* table, unsigned char* out, void* stream);
/* out = lut[256 * channel + in]; lut: 768 bytes on the device; out must not overlap in */
int mstg_lut_u8(const unsigned char* in, int N, int H, int W, const unsigned char* lut, unsigned char* out, void* stream);
/* ksize 3, 5 or 7; 9 .. 15 MSTG_E_UNSUPPORTED (names smooth_level = ksize / 2) */
int mstg_gaussian_u8(const unsigned char* in, int N, int H, int W, int ksize, unsigned char* out, void* stream);
/* bytes mstg_standard_finish needs for (N, H, W): two image batches; 0 for an invalid shape (mstg_last_error says which) */
size_t mstg_standard_finish_workspace_bytes(int N, int H, int W);
/* The enabled steps in the reference's order on the caller's workspace (16-byte aligned), byte for byte the composition of the
 * stage entries, in at most three launches whatever N: with fix_blocks the median (the blend fused into its load), the bilateral
 * filter (the colour table fused into its store) and the blur; without fix_blocks the blend and the table in one point-wise launch
 * and the blur.  canvas may be NULL when blend_ratio <= 0; bilateral_table and d are read with fix_blocks only; color_lut NULL =
 * no colour step; smooth_level 0 = no blur (the reference's adaptive_smooth=False).  out must not overlap anything else. */
int mstg_standard_finish(const unsigned char* canvas, const unsigned char* styled, int N, int H, int W, double one_minus_ratio,
                         double blend_ratio, int fix_blocks, int d, const float* bilateral_table /*nullable iff !fix_blocks*/,
                         const unsigned char* color_lut /*nullable*/, int smooth_level, unsigned char* out, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The LOCAL-STYLE tab and the COMPARE tab of the reference's application (gan_login_gui.py:1259-1530 local_style_process_thread,
 * :2423-2638 compare_process_thread; the tab's defaults :1051-1116) between the forward pass and the crop, on the device for N
 * images (N, H, W, 3) uint8, any H, W >= 1 unless stated, 64-bit offsets.  This is NOT the chain of mstg_local_style_enhanced,
 * which restates batch_process_images.py (another sky rule, another edge weight, another finish).  The OpenCV steps are restated
 * from the definitions below (tests/app_local_style_ref.py is the same restatement in numpy); NONE OF THEM HAS BEEN COMPARED WITH
 * AN OPENCV BINARY.  No floating-point atomics, a fixed summation order: bit-reproducible and independent of N.
 *
 *   1. sky mask m (:1337-1355, :2483-2501), uint8 (N, H, W).  The 8-bit COLOR_RGB2HSV of the canvas: v, diff and s as defined for
 *        the weight map above (sdiv, (diff * sdiv[v] + 2048) >> 12); hue: hdiv[0] = 0, hdiv[i] = round-half-even(122880 / i)
 *        (= (180 << 12) / (6 i)); h0 = (v == R) ? G - B : (v == G) ? B - R + 2 * diff : R - G + 4 * diff (the test on R first);
 *        h = (h0 * hdiv[diff] + 2048) >> 12 with an arithmetic shift of the signed product; h < 0: h += 180.
 *        blue = 90 <= h <= 130 && s >= 30 && v >= 140 (cv2.inRange [90, 30, 140] .. [130, 255, 255]) and only for rows y < H / 2;
 *        dil  = 255 where any blue lies in the 9 x 9 window clipped to the image, else 0 (cv2.dilate with a 5 x 5 box, two
 *        iterations, default border: neutral);
 *        m    = cv2.GaussianBlur(dil, (15, 15), 0), OpenCV's bit-exact 8-bit path: taps in 8.8 fixed point
 *        {1, 3, 6, 12, 20, 30, 36, 40, 36, 30, 20, 12, 6, 3, 1} (sum 256) along x, then along y; BORDER_REFLECT_101 of dil (index p
 *        outside [0, len) mirrored without repeating the edge pixel, repeatedly for sides shorter than 7; len == 1 gives 0); the
 *        row sums are exact in 16 bits; m = (sum + 32768) >> 16.  The taps are OpenCV's generator as recalled: sigma =
 *        ((15 - 1) * 0.5 - 1) * 0.3 + 0.8, t_i = exp(-0.5 x_i^2 / sigma^2) normalised by the left-to-right sum, then for the first
 *        seven taps error diffusion a = t_i * 256 + err, q = round(a), err = a - q, and the centre = 256 - 2 * their sum.  The
 *        smallest distance of any a from a rounding tie is 0.158 (tests/test_app_local_style_cpu.py regenerates the table and
 *        asserts the margin), so a last-bit difference in exp cannot change a tap.  mstg_gaussian_u8 still refuses ksize 9 .. 15.
 *   2. sky blend (:1358-1367): w = (double)m / 255.0; x = img * (1 - w) + orig * w in float64, two rounded products and one rounded
 *        sum, no fused multiply-add; clip to [0, 255], truncate: the form of mstg_blend_u8 with orig := img (the styled image so
 *        far) and styled := the canvas.
 *   3. edge weight a (:1375-1391, :2520-2537), float64 (N, H, W).  edge = cv2.Canny(gray, 50, 150) of the canvas as
 *        mstg_local_style_prepare and mstg_local_style_hysteresis compute it; ed = 1.0 where any edge lies in the 3 x 3 window
 *        clipped to the image, else 0.0 (255 / 255.0 is exactly 1.0); ew = cv2.GaussianBlur(ed, (21, 21), 0) in float64, sigma 3.5,
 *        BORDER_REFLECT_101 of ed, with OpenCV's generic row filter and symmetric column filter for CV_64F as recalled:
 *          kernel k[0 .. 20] from the HOST (mstg_gaussian_kernel_f64): std::exp(x * x * (-0.5 / sigma^2)), x = i - 10, summed left
 *          to right, every tap multiplied by 1 / sum; the caller uploads it, the device never evaluates exp;
 *          row pass    r = k[0] * S[0]; r += k[j] * S[j] for j = 1 .. 20, left to right (the products are exact: S is 0 or 1);
 *          column pass c = k[10] * R[0]; c += k[10 + j] * (R[+j] + R[-j]) for j = 1 .. 10, the nearest pair first;
 *          every operation rounded, no fused multiply-add.
 *        a = ew * detail (one rounded product); the blend is the form of 2 with w = a.  On images whose styled part equals the
 *        canvas (where truncation is sensitive) a fused column pass changes 0.35 % of the bytes after this blend, the
 *        outermost-pair-first order 0.85 %, scipy.ndimage.correlate1d(mode="mirror") 0.95 %, never by more than one level
 *        (tests/test_app_local_style_cpu.py measures the shares).
 *   4. strength blend (:1404-1408), only when strength < 0.3: bf = strength / 0.3; x = img * bf + orig * (1 - bf), clip, truncate;
 *        the caller passes bf and 1 - bf as its own doubles (w_styled, w_canvas).
 *   5. colour step (:1411-1418): the table of mstg_standard_color_lut for the direction.
 *   6. smoothing (:1423): cv2.bilateralFilter(d=9, 75, 75) = mstg_bilateral_u8.
 *   modes of the tab (:1315, :1328, :1428; named here simple, enhanced, advanced in the tab's order).  simple:
 *        r = max(0.05, min(1.0 - strength, 0.95)), styled * (1 - r) + canvas * r, clip, truncate = step 4's form with
 *        w_styled = 1 - r, w_canvas = r.  enhanced: 2 if ignore_sky and photo_to_monet, 3 if auto_select, 4, 5 if enhance_colors,
 *        6 if smooth_transitions.  advanced (checked with a search of the file for the four helper names): every
 *        helper it calls is guarded by hasattr(self, ...) and the class defines none of them, so it is step 4 alone.  Any other
 *        name: the styled image.  The compare tab (:2475-2560) is the enhanced chain with auto_select, enhance_colors and
 *        smooth_transitions on and detail = 0.6, beside the plain generator's output.
 * ---------------------------------------------------------------------------------------------- */
#define MSTG_APP_EDGE_KSIZE 21
/* Host only: cv2.getGaussianKernel(ksize, sigma, CV_64F) as defined in 3 (sigma <= 0: ((ksize - 1) * 0.5 - 1) * 0.3 + 0.8);
 * ksize odd, 1 .. 255 */
int mstg_gaussian_kernel_f64(int ksize, double sigma, double* out /* [ksize] */);
/* step 1: mask (N, H, W) bytes; one launch whatever N */
int mstg_app_sky_mask(const unsigned char* canvas, int N, int H, int W, unsigned char* mask, void* stream);
/* step 3 after Canny: edge = the (N, H, W) 0 / 1 mask of mstg_local_style_hysteresis, kernel_f64 = the MSTG_APP_EDGE_KSIZE doubles of
 * mstg_gaussian_kernel_f64(21, 0) on the device, weight = a, float64 (N, H, W); one launch whatever N */
int mstg_app_edge_weight(const unsigned char* edge, int N, int H, int W, const double* kernel_f64, double detail, double* weight,
                         void* stream);
/* the point-wise part, one launch: blend 2 with sky_mask (NULL: off), blend 3 with edge_weight (NULL: off), blend 4 with
 * (w_styled, w_canvas) if use_strength, each clipped and truncated to a byte before the next, then the table (NULL: off).  canvas
 * may be NULL when no blend is on; out must not overlap an input */
int mstg_app_chain(const unsigned char* canvas, const unsigned char* styled, int N, int H, int W, const unsigned char* sky_mask /*nullable*/,
                   const double* edge_weight /*nullable*/, int use_strength, double w_styled, double w_canvas,
                   const unsigned char* color_lut /*nullable*/, unsigned char* out, void* stream);
/* bytes mstg_app_local_style_finish needs for (N, H, W); 0 for an invalid shape (mstg_last_error says which) */
size_t mstg_app_local_style_workspace_bytes(int N, int H, int W);
/* The enabled steps in the reference's order on the caller's workspace (16-byte aligned), byte for byte the composition of the stage
 * entries, in at most six launches whatever N: prepare, hysteresis, edge weight (auto_select), sky mask (ignore_sky: the caller
 * passes ignore_sky && photo_to_monet), the point-wise chain, the bilateral filter (smooth).  With auto_select H * W <=
 * MSTG_LOCAL_STYLE_MAX_PIXELS, else MSTG_E_UNSUPPORTED (the message names the size); without it any size.  kernel_f64 is read with
 * auto_select only, bilateral_table (d = 9) with smooth only, color_lut NULL = no colour step.  out must not overlap an input, a
 * table or the workspace: MSTG_E_BADARG. */
int mstg_app_local_style_finish(const unsigned char* canvas, const unsigned char* styled, int N, int H, int W, int ignore_sky,
                                int auto_select, int use_strength, int smooth, double detail, double w_styled, double w_canvas,
                                const double* kernel_f64 /*nullable iff !auto_select*/, const unsigned char* color_lut /*nullable*/,
                                const float* bilateral_table /*nullable iff !smooth*/, unsigned char* out, void* workspace,
                                size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The COLOUR-BLOCK REPAIR of the reference (improved_smooth.py:137-164 fix_color_blocks_improved), on the device for N images
 * (N, H, W, 3) uint8 RGB, any H, W >= 1, N images per launch, 64-bit offsets.  The OpenCV steps are restated from the definitions
 * below, as recalled (tests/color_blocks_ref.py is the same restatement in numpy); NONE OF THEM HAS BEEN COMPARED WITH AN OPENCV
 * BINARY.  No floating-point atomics, a fixed summation order: bit-reproducible and independent of N.  `out` (and a workspace) must
 * not overlap an input: MSTG_E_BADARG.  The device never evaluates exp, pow or cbrt: the tables come from host-only entries.  A
 * parameter outside what is built is refused with MSTG_E_UNSUPPORTED and a message naming it, never approximated.
 *
 *   1. block mask (:53-95 detect_color_blocks; threshold 30, kernel_size 11), bytes 0 / 1 (N, H, W).
 *        a, b of the 8-bit COLOR_RGB2LAB (L is never used), OpenCV's integer path as recalled.  Tables, built on the host in
 *        double (mstg_lab_tables):
 *          gamma[v] = round(2040 * lin(v / 255)), v = 0 .. 255, lin(x) = x <= 0.04045 ? x / 12.92 : ((x + 0.055) / 1.055)^2.4;
 *          cbrt[i]  = round(32768 * f(i / 2040)), i = 0 .. 3071, f(x) = x < 0.008856 ? 7.787 x + 16 / 116 : cbrt(x);
 *          C[r][k]  = round(4096 * M[r][k] / white[r]), M = {0.412453, 0.357580, 0.180423; 0.212671, 0.715160, 0.072169;
 *          0.019334, 0.119193, 0.950227}, white = {0.950456, 1, 1.088754}: C = {1777, 1541, 778; 871, 2929, 296; 73, 448, 3575},
 *          every row sums to 4096; max gamma = 2040, max cbrt = 37555 (16 bits), the index below stays <= 2040.
 *        Per pixel, with R' = gamma[R] and so on: fX = cbrt[(R' C00 + G' C01 + B' C02 + 2048) >> 12], fY, fZ from rows 1 and 2;
 *          a = sat_u8((500 (fX - fY) + 128 * 32768 + 16384) >> 15), b = sat_u8((200 (fY - fZ) + 128 * 32768 + 16384) >> 15),
 *          arithmetic shifts.  White and black give (128, 128), (255, 0, 0) gives (208, 195), (0, 255, 0) (42, 211), (0, 0, 255)
 *          (207, 20).  Over all 2^24 colours a lies within 2.67 and b within 1.70 of float64 CIE Lab.  The smallest distance of
 *          an unrounded gamma or cbrt entry from a rounding tie is 4.7e-6 (asserted above 1e-9: a last-bit difference of pow or
 *          cbrt cannot change an entry).  OpenCV 4 builds these tables in 32-bit soft-float: evaluated in float32 instead of
 *          double, 0 of the 256 gamma entries and 2 of the 3072 cbrt entries change, by one unit
 *          (tests/test_color_blocks_cpu.py measures both).
 *        gradient: on the a and b planes as float32, cv2.Sobel(ksize=3) in x and in y, BORDER_REFLECT_101 (all values are integers
 *          of at most 1020, any summation order is exact); m = sqrt_rn_f32(gx^2 + gy^2) (the argument is an integer below 2^24);
 *          c = fl32(m_a + m_b) * 0.5f; edge = c > threshold (float32).
 *        dilation: mask = 1 where any edge lies in the k x k window clipped to the image (cv2.dilate with a box, default border:
 *          neutral); k odd, 1 .. MSTG_COLOR_BLOCK_MAX_KERNEL, anything else refused (the message names kernel_size).
 *   2. correction (:10-51 adaptive_color_correction; radius 50).  For a flagged pixel and every channel: sum and count over the
 *        (2 r + 1)^2 window of the INPUT clipped to the image (exact integers; uint32, so H * W * 255 < 2^32, else refused by
 *        name); mean = (double)sum / (double)count (one IEEE division); v = 0.5 * px + 0.5 * mean (both products exact, one
 *        rounded sum); the byte is v truncated (the reference assigns float64 into a uint8 array).  Unflagged pixels are copied;
 *        with no flagged pixel the stage is the identity, which is the reference's blocks_detected.any() branch.
 *   3. wide bilateral (:97-112 edge_preserving_smoothing; cv2.bilateralFilter(img, 0, 0.4 * 255, 60)): the definition of
 *        mstg_bilateral_u8 above word for word (tap order i, then j, with sqrt(i^2 + j^2) <= radius; float32, contraction off;
 *        w = space * color[t] one rounded product; wsum += w; three fmaf channel sums; inv = 1.0f / wsum; rint, saturate;
 *        BORDER_REFLECT_101 repeated for sides shorter than the radius; a sigma <= 0 counts as 1), extended in two ways:
 *          radius: d <= 0: radius = cvRound(sigmaSpace * 1.5) (round half to even), at least 1; d > 0: radius = max(d / 2, 1);
 *          radii 1 .. MSTG_BILATERAL_WIDE_MAX_RADIUS are built, above that refused (the message names the radius).  sigmaSpace 60
 *          gives radius 90: 25 445 taps;
 *          space weights: space(i, j) = (float)exp((i^2 + j^2) * (-0.5 / sigmaSpace^2)) in double on the host, a function of
 *          i^2 + j^2 alone, so the device table is indexed by it (8101 floats at radius 90).
 *        At d = 3, 5, 7, 9 the result equals mstg_bilateral_u8 byte for byte.
 *   4. detail blend (:114-135 detail_enhancing_blend; alpha 0.1, beta 0.5 in the chain), on float64: blurred =
 *        cv2.GaussianBlur(orig, (0, 0), 3): for a depth other than 8 bits ksize = cvRound(sigma * 4 * 2 + 1) | 1 = 25; the kernel is
 *        mstg_gaussian_kernel_f64(25, 3); row pass and column pass exactly as defined for step 3 of the application's local-style
 *        chain above (row pass left to right; column pass centre first, then the nearest pair; every operation rounded, no fused
 *        multiply-add; BORDER_REFLECT_101 repeated for sides shorter than 12), here per channel on byte-valued input;
 *        detail = orig - blurred; x = ((img * w_img) + (orig * alpha)) + (detail * beta), every operation rounded; the caller
 *        passes w_img = 1 - alpha as its own double; clip to [0, 255], truncate.  ksize odd, 1 .. MSTG_DETAIL_BLEND_MAX_KSIZE,
 *        anything else refused (the message names ksize).  A caller resizes an original of another size first (Lanczos,
 *        mstg_resample_*).
 * ---------------------------------------------------------------------------------------------- */
#define MSTG_LAB_TABLE_U16 3340 /* gamma[256], cbrt[3072], C[9] row by row, 3 entries of padding */
#define MSTG_COLOR_BLOCK_MAX_KERNEL 31
#define MSTG_BILATERAL_WIDE_MAX_RADIUS 90
#define MSTG_BILATERAL_WIDE_TABLE_FLOATS (MSTG_BILATERAL_COLOR_WEIGHTS + MSTG_BILATERAL_WIDE_MAX_RADIUS * MSTG_BILATERAL_WIDE_MAX_RADIUS + 1)
#define MSTG_DETAIL_BLEND_MAX_KSIZE 31
/* Host only: the tables of step 1 */
int mstg_lab_tables(unsigned short* table /* [MSTG_LAB_TABLE_U16] */);
/* Host only: table[0 .. 767] = color[t], table[768 + q] = space weight of i^2 + j^2 = q for q <= radius^2 (0 beyond).  Returns the
 * radius (1 .. 90) that d and sigma_space give, or a negative code. */
int mstg_bilateral_wide_tables(int d, double sigma_color, double sigma_space, float* table /* [MSTG_BILATERAL_WIDE_TABLE_FLOATS] */);
/* step 1: lab_table = the MSTG_LAB_TABLE_U16 entries of mstg_lab_tables on the device; mask (N, H, W) bytes; workspace: N * H * W
 * bytes (the undilated edges); two launches whatever N */
int mstg_color_block_mask(const unsigned char* in, int N, int H, int W, const unsigned short* lab_table, float threshold, int kernel_size,
                          unsigned char* mask, void* workspace, size_t workspace_bytes, void* stream);
/* step 2: mask (N, H, W) bytes, nonzero = flagged; workspace: N * H * W * 12 bytes, 4-byte aligned (the window's row sums); two
 * launches whatever N */
int mstg_color_correct_u8(const unsigned char* in, const unsigned char* mask, int N, int H, int W, int radius, unsigned char* out,
                          void* workspace, size_t workspace_bytes, void* stream);
/* step 3: radius and table (on the device) from mstg_bilateral_wide_tables; one launch whatever N */
int mstg_bilateral_wide_u8(const unsigned char* in, int N, int H, int W, int radius, const float* table, unsigned char* out, void* stream);
/* step 4: kernel_f64 = the ksize doubles of mstg_gaussian_kernel_f64 on the device; workspace: N * H * W * 24 bytes, 8-byte aligned
 * (the row pass); two launches whatever N, the blend fused into the column pass */
int mstg_detail_blend_u8(const unsigned char* img, const unsigned char* orig, int N, int H, int W, const double* kernel_f64, int ksize,
                         double w_img, double alpha, double beta, unsigned char* out, void* workspace, size_t workspace_bytes, void* stream);
/* bytes mstg_color_block_fix needs for (N, H, W), with or without an original; 0 for an invalid shape (mstg_last_error says which) */
size_t mstg_color_block_fix_workspace_bytes(int N, int H, int W, int with_orig);
/* Steps 1 to 3, and step 4 when orig != NULL, on the caller's workspace (16-byte aligned), byte for byte the composition of the
 * stage entries: five launches without an original, seven with one, whatever N.  kernel_f64, ksize, w_img, alpha and beta are
 * read with an original only. */
int mstg_color_block_fix(const unsigned char* in, const unsigned char* orig /*nullable*/, int N, int H, int W,
                         const unsigned short* lab_table, float threshold, int kernel_size, int correct_radius, int bilateral_radius,
                         const float* bilateral_table, const double* kernel_f64 /*nullable iff !orig*/, int ksize, double w_img,
                         double alpha, double beta, unsigned char* out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The SEGMENTATION-DRIVEN LOCAL STYLE of the reference (enhanced_local_style.py:76-292) between the forward pass and the crop, on
 * the device for N images (N, H, W, 3) uint8 RGB, N images per launch, 64-bit offsets; the segmentation itself (:68) on the host.
 * The OpenCV, scipy and scikit-image steps are restated from the definitions below, as recalled
 * (tests/enhanced_local_style_ref.py is the same restatement in numpy); NONE OF THEM HAS BEEN COMPARED WITH AN OPENCV OR
 * SCIKIT-IMAGE BINARY; the Gaussian of step 2 is compared with scipy itself, bit for bit (tests/test_enhanced_local_style_cpu.py).
 * No floating-point atomics: the statistics are integer sums (64-bit integer atomics, any order gives the same bits), everything
 * else has a fixed order: bit-reproducible and independent of N.  A parameter outside what is built is refused with
 * MSTG_E_UNSUPPORTED / MSTG_E_BADARG and a message naming it, never approximated.  `out` and a workspace must not overlap an input.
 *
 *   1. segment statistics and blend ratios (:76-171 analyze_segments, determine_blend_ratios).  labels (N, H, W) int32 and
 *        num_segments S: a pixel whose label lies outside [0, S) belongs to no segment, contributes to nothing and gets map 0;
 *        labels need be neither contiguous nor connected; a label with no pixel is skipped (ratio 0, sums 0).  2 <= H, W and
 *        H * W <= MSTG_SEGMENT_MAX_PIXELS (the edge sum fits 64 bits while H * W * 1443 < 2^31), else refused by name.
 *        Per image and label s, MSTG_SEGMENT_SUMS exact 64-bit integers, in this order: n; sum R, G, B; sum R^2, G^2, B^2; sum S
 *        (the saturation of the 8-bit COLOR_RGB2HSV as defined above: sdiv, (diff * sdiv[v] + 2048) >> 12); sum y; sum x; E.
 *        E: g_s = the 8-bit grey (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14 where the label is s, 0 elsewhere (cvtColor of the
 *          zeroed copy); gx, gy = the 3 x 3 Sobel of g_s, BORDER_REFLECT_101 (labels and greys mirrored alike); m = sqrt of the
 *          integer gx^2 + gy^2, correctly rounded in float64; E = the sum over ALL pixels of the image of rint(m * 2^32) (round
 *          half to even) as unsigned 64-bit integers.  Only a pixel with an s in its reflected 3 x 3 neighbourhood contributes (at
 *          most nine labels per pixel).  The fixed point is what makes the sum independent of its order.
 *        ratio, float64, every operation rounded, no fused multiply-add, in this order: std_c = sqrt((double)(n * sum c^2 -
 *          (sum c)^2)) / n with the integer formed exactly; mstd = ((std_R + std_G) + std_B) / 3.0; ed = (double)E / 2^32 /
 *          (double)(H * W); py = (double)sum y / n, px likewise; cy = H / 2, cx = W / 2 (integers); md = sqrt((double)(cx^2 + cy^2));
 *          dist = sqrt((py - cy)^2 + (px - cx)^2); sm = (double)sum S / n; adj = (((0.3 * (ed / 30) + 0.2 * (mstd / 50)) - 0.1 *
 *          (dist / md)) + (-0.1 * (n / (H * W / 100.0)))) + 0.2 * (sm / 255); ratio = max(0.3, min(0.9, 0.7 + adj)) rounded to
 *          float32.  This is not numpy's literal evaluation (np.std sums squared deviations in mask order, np.mean of the
 *          magnitudes is a pairwise float64 sum); tests/test_enhanced_local_style_cpu.py compares the float32 ratios of the two.
 *        map[p] = ratio[label[p]], float32 (N, H, W).
 *   2. smoothed map (:174): scipy.ndimage.gaussian_filter(map, sigma=3) on float32: radius 12, the float64 weights of
 *        _gaussian_kernel1d(3, 0, 12) to the bit (constants), mode 'reflect' (d c b a | a b c d | d c b a) for any extent, axis 0
 *        then axis 1, per line t = in[i] * w[0]; t += (in[i - k] + in[i + k]) * w[k] for k = 12 .. 1 in float64, every operation
 *        rounded; the result of each axis pass is stored as float32.
 *   3. blend (:232-240), float32 as numpy forms it from uint8 and float32 arrays: x = fl(fl(styled * m) + fl(canvas * fl(1 - m))),
 *        clipped to [0, 255] and truncated (a NaN gives 0).  The clip is this build's: it matters only for a map outside [0, 1].
 *        NOT mstg_blend_u8, which is float64.
 *   4. colour and contrast (:243-257).  (a) h, s, v of the 8-bit COLOR_RGB2HSV as defined above.  (b) s' = min(rint(s * 1.2), 255):
 *        the fractions are multiples of 0.2, never near a tie, so float32 (used here) and float64 give the same byte for all 256
 *        values (asserted in the CPU test).  (c) v' = CLAHE(clipLimit 2.0, tiles 8 x 8) of the v plane, OpenCV's clahe.cpp as
 *        recalled: tile = (W / 8, H / 8); H and W must be multiples of 8 (OpenCV pads otherwise: refused by name); per tile a
 *        256-bin histogram; clip = max((int)(2.0 * area / 256), 1); the excess above clip is summed and every bin capped; batch =
 *        excess / 256 goes to every bin; residual = excess - batch * 256; if nonzero, step = max(256 / residual, 1) and
 *        for (i = 0; i < 256 && residual > 0; i += step, --residual) ++hist[i]; lut[i] = sat_u8(rint((float)cumsum_i * lutScale)),
 *        lutScale = 255.0f / area.  Per pixel txf = x * (1.0f / tw) - 0.5f; tx1 = floor(txf); xa = txf - tx1; xa1 = 1.0f - xa;
 *        tx1 clamped to >= 0; tx2 = tx1 + 1 (formed before the clamp) clamped to <= 7; the same in y; res = (L11 * xa1 + L12 * xa) *
 *        ya1 + (L21 * xa1 + L22 * xa) * ya in float32, every operation rounded; v' = sat_u8(rint(res)).  For tile sides that are
 *        powers of two up to 64 every product and sum is exact.  (d) the 8-bit COLOR_HSV2RGB of (h, s', v'), OpenCV's float path
 *        as recalled: hf = h, sf = s' * (1.f / 255.f), vf = v' * (1.f / 255.f); sf == 0: r = g = b = vf; else hf *= 6.f / 180.f,
 *        sector = floor(hf), hf -= sector, a sector outside 0 .. 5 becomes sector 0 with hf = 0; tab = {vf, vf * (1 - sf),
 *        vf * (1 - sf * hf), vf * (1 - sf * (1 - hf))}; (b, g, r) = tab indexed by {{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}}
 *        [sector]; every operation rounded in float32, no fused multiply-add; each byte sat_u8(rint(c * 255.f)).  Over all
 *        180 * 256 * 256 (h, s, v) a fused evaluation (1 - sf * hf and 1 - sf * (1 - hf) as one fused operation each)
 *        changes 0.001 % of the bytes and a float64 evaluation 0.020 %, never by more than one level
 *        (tests/test_enhanced_local_style_cpu.py measures both shares).
 *   5. sharpen and denoise (:260-264): cv2.filter2D with [[-1,-1,-1],[-1,9,-1],[-1,-1,-1]] per channel = 9 * centre - the eight
 *        neighbours, BORDER_REFLECT_101, exact integers, saturated; then cv2.bilateralFilter(5, 50, 50) = mstg_bilateral_u8.
 *   segmentation (:68), HOST: skimage.segmentation.felzenszwalb(img, scale, sigma=0.5, min_size) as recalled: the image as float64
 *        divided by 255, scale / 255; scipy's Gaussian per channel (sigma 0.5, radius 2, 'reflect', the weights of
 *        _gaussian_kernel1d(0.5, 0, 2) to the bit, axis 0 then axis 1, the accumulation order of step 2; another sigma is refused
 *        by name); the four 8-neighbour edge sets in the order right, down, down-right, up-right, each in row-major order of its
 *        first pixel; cost = the rounded sqrt of ((d0^2 + d1^2) + d2^2); a STABLE sort by cost; union-find with the merge rule
 *        cost < min(int_0 + scale / size_0, int_1 + scale / size_1), the merged internal cost = the edge's cost; a second pass in
 *        the same edge order that merges any two components of which one is smaller than min_size; labels numbered in ascending
 *        order of the root's pixel index, where the root of a component is its smallest pixel index.  scikit-image orders equal
 *        costs however numpy's unstable sort leaves them: the stable order is THIS BUILD'S definition.
 * ---------------------------------------------------------------------------------------------- */
#define MSTG_SEGMENT_SUMS 11
#define MSTG_SEGMENT_MAX_PIXELS 1048576
#define MSTG_SEGMENT_TILE_SLOTS 128 /* distinct labels a 16 x 64 tile combines in LDS; more go straight to the global sums */
#define MSTG_CLAHE_TILES 8
/* bytes mstg_segment_blend_map needs; 0 for an invalid shape (mstg_last_error says which) */
size_t mstg_segment_blend_map_workspace_bytes(int N, int H, int W, int num_segments, int smooth);
/* step 1, and step 2 when smooth != 0: map float32 (N, H, W); sums (N, S, MSTG_SEGMENT_SUMS) unsigned 64-bit and ratio float32
 * (N, S): the per-segment record; workspace 16-byte aligned (read with smooth only).  Four launches, six with smooth, whatever N
 * and S */
int mstg_segment_blend_map(const unsigned char* canvas, const int* labels, int N, int H, int W, int num_segments, int smooth, float* map,
                           unsigned long long* sums, float* ratio, void* workspace, size_t workspace_bytes, void* stream);
/* step 2 alone on any float32 (N, H, W), any H, W >= 1; workspace: N * H * W * 4 bytes; two launches */
int mstg_gaussian_reflect_f32(const float* in, int N, int H, int W, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* step 3; one launch */
int mstg_blend_map_f32_u8(const unsigned char* canvas, const unsigned char* styled, const float* map, int N, int H, int W, unsigned char* out,
                          void* stream);
/* bytes of the CLAHE tables for N images (mstg_clahe_u8, mstg_hsv_enhance_u8); 0 for an invalid shape */
size_t mstg_clahe_workspace_bytes(int N, int H, int W);
/* step 4c on a plane (N, H, W): the tables, then the application; two launches */
int mstg_clahe_u8(const unsigned char* in, int N, int H, int W, unsigned char* out, void* workspace, size_t workspace_bytes, void* stream);
/* steps 4a-d on an RGB batch; two launches */
int mstg_hsv_enhance_u8(const unsigned char* in, int N, int H, int W, unsigned char* out, void* workspace, size_t workspace_bytes, void* stream);
/* the filter of step 5; one launch */
int mstg_sharpen3_u8(const unsigned char* in, int N, int H, int W, unsigned char* out, void* stream);
/* bytes mstg_enhanced_style_finish needs for (N, H, W); 0 for an invalid shape (mstg_last_error says which) */
size_t mstg_enhanced_style_finish_workspace_bytes(int N, int H, int W);
/* Steps 3, 4 and 5 from canvas, styled and map on the caller's workspace (16-byte aligned), byte for byte the composition of
 * mstg_blend_map_f32_u8, mstg_hsv_enhance_u8, mstg_sharpen3_u8 and mstg_bilateral_u8(d = 5), in FIVE launches whatever N.
 * bilateral_table: the MSTG_BILATERAL_TABLE_FLOATS floats of mstg_bilateral_tables(5, 50, 50) on the device. */
int mstg_enhanced_style_finish(const unsigned char* canvas, const unsigned char* styled, const float* map, int N, int H, int W,
                               const float* bilateral_table, unsigned char* out, void* workspace, size_t workspace_bytes, void* stream);
/* Host only (host pointers, no stream): the segmentation above of one (H, W, 3) image into labels (H, W) int32.  Returns the number
 * of segments (>= 1) or a negative code. */
int mstg_felzenszwalb_u8(const unsigned char* img, int H, int W, double scale, double sigma, int min_size, int* labels);

/* ------------------------------------------------------------------------------------------------
 * SLIC SUPERPIXELS, the DEVICE segmentation for the local style above: the `slic` method that the reference's get_segmentation_mask
 * names (enhanced_local_style.py:65-66: skimage.segmentation.slic(img, n_segments=100, compactness=10)), per image for N images
 * (N, H, W, 3) uint8 RGB, N images per launch, 64-bit offsets, no host step and no host synchronisation.  The algorithm is restated
 * from its definition as recalled (tests/slic_ref.py is the same restatement in numpy); every place where the definition is THIS
 * BUILD'S OWN says so; IT HAS NOT BEEN COMPARED WITH A SCIKIT-IMAGE BINARY.  No floating-point atomics: the updates are exact integer
 * sums, everything else has a fixed order: bit-reproducible and independent of N.  A parameter outside what is built is refused with
 * MSTG_E_UNSUPPORTED and a message naming it, never approximated.  An output or the workspace must not overlap an input.
 *
 *   1. features.  Per pixel the integers (y, x, L, a, b); L, a, b are the bytes of the 8-bit Lab of step 1 of the advanced settings
 *        below (mstg_lab_u8; lab_table = the entries of mstg_lab_tables on the device).  THIS BUILD'S OWN: scikit-image converts
 *        with a float64 rgb2lab.  The 8-bit form keeps every sum an exact integer, evaluates no cbrt or pow on the device and makes
 *        the result bit-reproducible.
 *   2. grid.  s = sqrt((double)(H * W) / n_segments); step = rint(s) (ties to even); start = floor(s / 2).  The centres are the pixels
 *        (start + i * step, start + j * step) for all i, j >= 0 inside the image, row-major: K = ny * nx.  The initial centre is
 *        (y, x, L, a, b) of its pixel as float32.  Refused by name: n_segments < 1; H * W <= n_segments; a side smaller than step
 *        (scikit-image re-grids there; not built); K above MSTG_SLIC_MAX_CENTRES; H * W above MSTG_SEGMENT_MAX_PIXELS;
 *        compactness <= 0 (or one whose square is not a finite float32).
 *   3. ten rounds of assignment and update (max_num_iter = 10, ALWAYS ten: a round that changes nothing is a fixed point, so
 *        scikit-image's early exit gives the same labels).  Every label starts as 0.
 *        candidates: centre k is a candidate for pixel (y, x) iff |y - (int)cy_k| <= 2 * step and |x - (int)cx_k| <= 2 * step.
 *        distance, float32, every operation rounded, no fused multiply-add, in exactly this order:
 *          d = ((dy * dy + dx * dx) * ws) + ((((dL * kL) * (dL * kL) + da * da) + db * db) * wc),
 *          ws = 1.f / (float)(step * step), wc = 1.f / (m * m) with m = (float)compactness, kL = 100.f / 255.f (the 8-bit L back on
 *          the scale of a and b); every difference is (float)feature - centre.
 *        choice: the pixel takes the candidate of the smallest d, among equal d the lowest k; a pixel with no candidate keeps its
 *          label (in round 1 every pixel has one: the nearest grid row and column are at most step away).
 *        update: per centre the exact integers n and the sums of y, x, L, a, b over its pixels; centre = (float)((double)sum /
 *          (double)n) per feature; a centre without pixels keeps its values.
 *        The labels are those of the tenth assignment, 0 .. K - 1; the centres (N, K, 5) float32 those of the tenth update.
 *   4. connectivity.  THIS BUILD'S OWN: scikit-image's pass is a raster-order flood fill whose merge target and whose max_size split
 *        depend on the visiting order; here every decision is a function of the labels alone.
 *        Components are the 4-connected sets of equal label; a component's root is its smallest raster index r, its size n.
 *        min_size = (int)(0.5 * ((double)(H * W) / K)) (mstg_connect_labels takes it from the caller).
 *        A component with n < min_size and r > 0 is SMALL.  Its parent is the component of pixel r - 1, or of pixel r - W when
 *        r % W == 0: that pixel is a 4-neighbour of r with a smaller index, so it belongs to another component with a smaller
 *        root, and the links cannot cycle.  The owner of a component is the first component along its parent links that is not
 *        small (the component of pixel 0 never is); sizes are not updated by merging.  The owners are numbered 1, 2, ... in
 *        ascending order of their roots (scikit-image's start_label = 1) and every pixel gets its owner's number; count = the
 *        number of owners <= H * W / max(min_size, 1) + 1 (integer division; every owner but that of pixel 0 has min_size pixels),
 *        a bound the host can compute, so a caller sizes its per-segment buffers without reading count back.
 *        Components above max_size are NOT split: not built.
 *   Still not built: the max_size split; a comparison with a scikit-image binary.  (`quickshift` is the next block.)
 * ---------------------------------------------------------------------------------------------- */
#define MSTG_SLIC_MAX_CENTRES 4096
#define MSTG_SLIC_SUMS 6 /* per centre: n, sum y, x, L, a, b */
/* Host only: step, ny and nx of step 2 (K = ny * nx); a refused shape returns its code (mstg_last_error names the value) */
int mstg_slic_grid(int H, int W, int n_segments, int* step, int* ny, int* nx);
/* bytes mstg_slic_u8 needs (mstg_slic_assign_u8 needs no more); 0 for a refused shape (mstg_last_error says which) */
size_t mstg_slic_workspace_bytes(int N, int H, int W, int n_segments);
/* steps 1 to 4: labels (N, H, W) int32 in 1 .. count, count (N) int32, both on the device; workspace 16-byte aligned.
 * 22 launches for steps 1 to 3 and 9 + max(ceil(log16(H * W)), 1) for step 4 (13 at 256 x 256), whatever N and the image */
int mstg_slic_u8(const unsigned char* img, int N, int H, int W, int n_segments, double compactness, const unsigned short* lab_table,
                 int* labels, int* count, void* workspace, size_t workspace_bytes, void* stream);
/* steps 1 to 3 only: the raw labels (N, H, W) int32 in 0 .. K - 1 and the final centres (N, K, 5) float32: y, x, L, a, b */
int mstg_slic_assign_u8(const unsigned char* img, int N, int H, int W, int n_segments, double compactness, const unsigned short* lab_table,
                        int* labels, float* centres, void* workspace, size_t workspace_bytes, void* stream);
/* bytes mstg_connect_labels needs; 0 for a refused shape */
size_t mstg_connect_labels_workspace_bytes(int N, int H, int W);
/* step 4 on any int32 labels (N, H, W), any H, W >= 1 with H * W <= MSTG_SEGMENT_MAX_PIXELS; min_size <= 1: nothing is small */
int mstg_connect_labels(const int* labels_in, int N, int H, int W, int min_size, int* labels_out, int* count, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * QUICKSHIFT, the second DEVICE segmentation for the local style above: the `quickshift` method that the reference's
 * get_segmentation_mask names (enhanced_local_style.py:69-70: skimage.segmentation.quickshift(img, kernel_size=3, max_dist=6,
 * ratio=0.5)), per image for N images (N, H, W, 3) uint8 RGB, N images per launch, 64-bit offsets, no host step and no host
 * synchronisation.  The definition is RESTATED AS RECALLED, NOT COMPARED WITH A SCIKIT-IMAGE BINARY (tests/quickshift_ref.py is the
 * same restatement in numpy); every place where it is THIS BUILD'S OWN says so.  No floating-point atomics and no floating-point
 * sum at all: the density is an exact integer, so it does not depend on how a window is split over lanes; everything else has a
 * fixed order: bit-reproducible and independent of N.  A parameter outside what is built is refused with MSTG_E_UNSUPPORTED or
 * MSTG_E_BADARG and a message naming it, on the host before any launch, never approximated.  An output or the workspace must not
 * overlap an input.  idx = r * W + c is a pixel's raster index.
 *
 *   1. features.  (L, a, b) are the bytes of mstg_lab_u8 (lab_table = the entries of mstg_lab_tables on the device, as for
 *        mstg_slic_u8).  THIS BUILD'S OWN: scikit-image converts with a float64 rgb2lab.
 *   2. window and distance.  w = (int)ceil(3 * kernel_size); the window of pixel p is |dr| <= w, |dc| <= w, clipped to the image.
 *        For p and a tap p': q = (100 * dL)^2 + 65025 * (da^2 + db^2), an exact integer (up to 9.1e9: above 2^32, exact in int64
 *        and in a double); s = dr^2 + dc^2; D = (double)q * kc + (double)s, two roundings, no fused multiply-add;
 *        kc = (ratio * ratio) / 65025.0 in double on the host.  That is ratio^2 * |dLab|^2 with L on the scale 0 .. 100 (the byte
 *        times 100 / 255) and a, b free of their offset, plus the squared pixel distance.
 *   3. density.  THIS BUILD'S OWN (fixed point; scikit-image sums float64):
 *        T(p) = sum over the clipped window, p itself included, of rint_half_even(exp(D * inv) * 2^32),
 *        inv = -0.5 / (kernel_size * kernel_size) in double on the host, exp in float64; int64 (N, H, W), at most 961 * 2^32.
 *        Two pixels whose windows hold the same terms tie EXACTLY; a float64 sum leaves mirror-image windows 1 ulp apart, and
 *        such near-ties decide parents.  Two float64 exp that differ by a few ulp move a term by at most one unit.
 *   4. parent.  p' is HIGHER than p iff T(p') > T(p), or T(p') == T(p) and idx' < idx.  THE TIE RULE IS THIS BUILD'S OWN:
 *        scikit-image adds normal(scale = 1e-5) noise from a seeded generator to the densities, which shatters every flat region
 *        (the bars of a letterboxed image) into random specks.  The parent of p is the higher tap of the smallest D, among equal D
 *        the lowest idx' (scikit-image's row-major scan with a strict <).  p is a root (its own parent) if no tap is higher or if
 *        that D > max_dist * max_dist (the product a double from the host; scikit-image compares sqrt(D) > max_dist).
 *        Since D >= s the search needs only |dr|, |dc| <= min(w, floor(max_dist)): a parent with D <= max_dist^2 lies inside that
 *        square and so does every tap that ties with it.
 *   5. labels.  Every pixel follows its parents to a root (no cycle: HIGHER is a strict total order).  The roots are numbered
 *        0, 1, ... in ascending idx (np.unique(..., return_inverse=True)); labels (N, H, W) int32 in 0 .. count - 1, count (N)
 *        int32.  Segments need not be connected, as in scikit-image.  count <= H * W is the only bound the host can know.
 *   Refused by name: kernel_size < 1 or not finite; w above MSTG_QUICKSHIFT_MAX_RADIUS; max_dist <= 0 or not finite; ratio outside
 *   [0, 1]; H * W above MSTG_SEGMENT_MAX_PIXELS; H or W < 1; a workspace that is too small; an output or workspace that overlaps
 *   an input.  Not built: sigma != 0, convert2lab=False, return_tree, scikit-image's noise.
 * ---------------------------------------------------------------------------------------------- */
#define MSTG_QUICKSHIFT_MAX_RADIUS 15
/* bytes mstg_quickshift_u8 needs; 0 for a refused shape or kernel_size (mstg_last_error says which) */
size_t mstg_quickshift_workspace_bytes(int N, int H, int W, double kernel_size);
/* steps 1 to 3: density (N, H, W) int64 on the device, 8-byte aligned; one launch */
int mstg_quickshift_density_u8(const unsigned char* img, int N, int H, int W, double ratio, double kernel_size,
                               const unsigned short* lab_table, long long* density_i64, void* stream);
/* step 4 on a GIVEN density (an input: any int64 (N, H, W)): parent (N, H, W) int32, raster indices inside the pixel's image, a
 * root its own parent; one launch */
int mstg_quickshift_parents_u8(const unsigned char* img, const long long* density_i64, int N, int H, int W, double ratio, double kernel_size,
                               double max_dist, const unsigned short* lab_table, int* parent_i32, void* stream);
/* steps 1 to 5: labels (N, H, W) int32 in 0 .. count - 1, count (N) int32, both on the device; workspace 16-byte aligned.
 * 6 + max(ceil(log16(H * W)), 1) launches (10 at 256 x 256), whatever N and the image: density, parents, the rounds of pointer
 * jumping and the four launches of the numbering that mstg_connect_labels uses too */
int mstg_quickshift_u8(const unsigned char* img, int N, int H, int W, double ratio, double kernel_size, double max_dist,
                       const unsigned short* lab_table, int* labels, int* count, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The FIVE SETTINGS of the reference's advanced_transform.py (:129-311: standard, contrast, multi-scale fusion, detail, K-means
 * regions) between the forward pass and the encoder, on the device for N images (N, H, W, 3) uint8 RGB, any H, W >= 1 unless
 * stated, N images per launch, 64-bit offsets.  The OpenCV steps are restated from the definitions below, as recalled, not
 * compared with an OpenCV binary (tests/advanced_transform_ref.py is the same restatement in numpy); where OpenCV's path could not be
 * recalled or cannot be pinned the step is THIS BUILD'S and says so.  No floating-point atomics, every summation order fixed:
 * bit-reproducible and independent of N.  `out` and a workspace must not overlap an input (MSTG_E_BADARG).  A parameter outside
 * what is built is refused with MSTG_E_UNSUPPORTED and a message naming it, never approximated.  The device evaluates no exp, pow
 * or cbrt: the tables come from host-only entries.
 *
 *   1. Lab (:145, :234), the 8-bit COLOR_RGB2LAB, bytes (L, a, b) in the place of (R, G, B).  fX, fY, fZ, a and b exactly as step 1
 *        of the colour-block repair above defines them (mstg_lab_tables: gamma, cbrt, C), completed with OpenCV's L as recalled:
 *        L = sat_u8((296 fY - 1336934 + 16384) >> 15), 296 = (116 * 255 + 50) / 100 and 1336934 = (16 * 255 * 32768 + 50) / 100 in
 *        integer division, arithmetic shift.  Black gives L 0, white 255, (255, 0, 0) 136, (0, 255, 0) 224, (0, 0, 255) 82.
 *   2. Lab -> RGB (:156, :246), the 8-bit COLOR_LAB2RGB.  The STRUCTURE is OpenCV's integer path as recalled (a table from L to fY,
 *        fX and fZ by adding scaled a and b, a table back from f to the linear value, an integer matrix, an inverse-gamma table);
 *        its table sizes, scales and rounding could not be recalled, so the CONSTANTS AND THE ROUNDING ARE THIS BUILD'S.  Tables,
 *        built on the host in double (mstg_lab_inverse_tables), 16-bit entries:
 *          fy[L]   = round(32768 * f), L* = L * 100 / 255, f = L* <= 8 ? 7.787 (L* / 903.3) + 16 / 116 : (L* + 16) / 116;
 *          da[a]   = round(32768 * (a - 128) / 500), db[b] = round(32768 * (b - 128) / 200) (signed);
 *          cube[i] = round(8192 * max(g(8 i / 32768), 0)), i = 0 .. MSTG_LAB_INV_CUBE - 1, g(t) = t > 6 / 29 ? t^3 : (t - 16 / 116) / 7.787
 *          (at most 36160);
 *          D[r][k] = round(4096 * Minv[r][k] * white[k]) (signed), Minv = {3.240479, -1.53715, -0.498535; -0.969256, 1.875991,
 *          0.041556; 0.055648, -0.204043, 1.057311}, white as above;
 *          enc[i]  = round(255 * e(i / 8192)), i = 0 .. 8192, e(x) = x <= 0.0031308 ? 12.92 x : 1.055 x^(1 / 2.4) - 0.055.
 *        Per pixel: fY = fy[L], fX = fY + da[a], fZ = fY - db[b]; for q = X, Y, Z: f = clamp(f_q, 0, 8 * (MSTG_LAB_INV_CUBE - 1) - 1),
 *        i = f >> 3, G_q = cube[i] + (((cube[i + 1] - cube[i]) * (f & 7) + 4) >> 3) (linear interpolation between two entries; a
 *        negative f gives 0); lin_c = (D[c][0] G_X + D[c][1] G_Y + D[c][2] G_Z + 2048) >> 12 (arithmetic shift; fits 32 bits),
 *        byte_c = enc[clamp(lin_c, 0, 8192)].  Defined for every byte triple, out-of-gamut ones included (they clamp).
 *        Measured over all 2^24 colours (tests/test_advanced_transform_cpu.py): the inverse lies within 2.07 levels of a float64
 *        CIE inverse (the same constants, clipped to [0, 255], unrounded) of the same Lab bytes; RGB -> Lab -> RGB is off by at
 *        most 27 levels in a channel, 0.702 on average, and by more than one level in 9.8 % of the channels.  That is the 8-bit
 *        Lab's own quantisation (dark and saturated blues): the float64 inverse, rounded, is off by at most 27 and by 0.699 on
 *        average as well.  The smallest distance of an unrounded table entry from a rounding tie is 3.1e-5 (asserted above 1e-9).
 *   3. Gaussian (:230): cv2.GaussianBlur(plane, (0, 0), sigma) on 8 bits: ksize = cvRound(sigma * 6 + 1) | 1 (round half to even; 19
 *        at sigma 3); the bit-exact 8.8 fixed-point path defined for the application's 15 x 15 blur above, with the generator as
 *        recalled there run for this sigma (mstg_gaussian_sigma_taps, host): t_i = exp(-0.5 x_i^2 / sigma^2) normalised by the
 *        left-to-right sum, for the first ksize / 2 taps a = t_i * 256 + err, q = round half to even(a), err = a - q, the
 *        centre = 256 - 2 * their sum.  Sigma 3: {0, 1, 3, 4, 9, 14, 20, 28, 32, 34, 32, ...} (sum 256); the smallest distance of
 *        any a from a tie is returned (0.0935 at sigma 3, asserted above 0.09 in the CPU test).  Along x, then along y; BORDER_REFLECT_101
 *        repeated for sides shorter than the radius; the row sums are exact in 16 bits; out = (sum + 32768) >> 16.  ksize above
 *        MSTG_GAUSSIAN_SIGMA_MAX_KSIZE is refused (the message names ksize).
 *   4. HSV gains (:159-164, :249-256, :304-309): h, s, v of the 8-bit COLOR_RGB2HSV as defined above; s' = min(rint(s * s_gain),
 *        255) and v' = min(rint(v * v_gain), 255) in float32 with the gain rounded to float32, round half to even (cv2.multiply
 *        as step 4b of the segmentation-driven local style defines it: OpenCV, as recalled, narrows a double scalar to float32
 *        for 8-bit sources).  At 1.2 float64 gives the same byte for all 256 values; at 1.1 it gives the next byte for the six
 *        values 55, 95, 115, 175, 195, 215 (x.5 in float32, just above it in float64; both asserted in the CPU test).  Then the
 *        8-bit COLOR_HSV2RGB of step 4d there.  With v_gain = 1 and CLAHE put on v it is
 *        mstg_hsv_enhance_u8.
 *   5. K-means (:271-276).  cv2.kmeans(..., KMEANS_RANDOM_CENTERS) draws from OpenCV's generator and cannot be pinned: THIS BUILD'S
 *        definition.  A problem is one attempt of one image; K in 1 .. MSTG_KMEANS_MAX_K, attempts in 1 .. MSTG_KMEANS_MAX_ATTEMPTS,
 *        iters in 1 .. MSTG_KMEANS_MAX_ITERS, else refused by name.
 *          initial centres: c[a][k][ch] = lo[ch] + u[a][k][ch] * (hi[ch] - lo[ch]) in float32, every operation rounded; lo, hi = the
 *          image's per-channel minimum and maximum, found on the device; u = attempts * K * 3 float32 uniforms from the caller (the
 *          Python side draws them from numpy.random.RandomState(seed)), the same for every image.  centers0 (N, K, 3) replaces
 *          them for attempts = 1.
 *          assignment: d_k = ((dx * dx + dy * dy) + dz * dz) in float32, every operation rounded, dx = (float)R - c[k][0] and so
 *          on; the label is the k of the smallest d, the lowest k wins a tie.
 *          update: per cluster the exact integers n, sum c and sum c^2 per channel (64-bit); the new centre is (float)((double)sum /
 *          (double)n); an empty cluster keeps its centre.  shift = max over k of ((e0 * e0 + e1 * e1) + e2 * e2) in float64 with
 *          e = (double)new - (double)old.  A problem whose shift <= eps * eps is frozen (a flag on the device) and skipped from
 *          then on.  At most `iters` rounds of assignment and update.
 *          result: one more assignment of every problem under its final centres gives its sums; compactness = the sum over k
 *          ascending, then ch ascending, of (((double)sum c^2 - (2.0 * c) * (double)sum c) + ((double)n * c) * c) with c the
 *          float32 centre as double, every operation rounded; the attempt of the smallest compactness wins, the lowest attempt
 *          wins a tie.  labels (N, H, W) int32 are the winner's assignment, in the order of its initial centres (no
 *          renumbering); centers (N, K, 3) float32; compactness (N) float64; best (N) int32 = the winning attempt.
 *        6 + 2 * iters launches whatever N and attempts, no host synchronisation.
 *   6. region blend (:281-301): r = ratios[min(label, count - 1)] (the reference: 0.8, 0.4, then 0.6); per byte styled * r + orig *
 *        (1 - r) in float64, two rounded products, one rounded sum, 1 - r a double subtraction; clip, truncate.  A negative label
 *        belongs to no region and gives 0, as the reference's sum over the regions does.
 *   7. fusion of scales (:206-215), float32, every operation rounded: x_s = (float)byte / 255.0f; f = 0; f = f + x_s * w_s in the
 *        order given; f = f * gain; clip to [0, 1]; byte = (u8)(f * 255.0f) truncated.  1 .. MSTG_FUSE_MAX_SCALES scales.
 *   chains, each byte for byte the composition of its stages:
 *        contrast (:137-166): Lab, CLAHE(2.0, 8 x 8) of L (step 4c of the segmentation-driven local style; H and W multiples of 8,
 *        else refused by name), Lab -> RGB, the gains: TWO launches (the histograms and tables of L; one point-wise kernel).
 *        detail (:218-258): g = the 8-bit grey of orig; blurred = step 3 of g; d = (g - blurred) mod 256 (uint8 arithmetic wraps);
 *        L' = (u8)clip((float)L + (float)d * 0.5f, 0, 255) truncated; Lab -> RGB of (L', a, b); the gains: TWO launches (the row
 *        pass of the grey; the column pass with everything else).
 *        regions (:261-311): K-means of orig, then the region blend and the gains in ONE launch (mstg_region_blend_gain_u8).
 *   Still not built: a comparison with an OpenCV binary; OpenCV's own random K-means centres; the random ColorJitter of the
 *   contrast setting's input; the matplotlib chart.
 * ---------------------------------------------------------------------------------------------- */
#define MSTG_LAB_INV_CUBE 6720
#define MSTG_LAB_INV_TABLE_U16 15696 /* fy[256], da[256], db[256], cube[6720], D[9] row by row, enc[8193], 6 entries of padding */
#define MSTG_GAUSSIAN_SIGMA_MAX_KSIZE 31
#define MSTG_KMEANS_MAX_K 16
#define MSTG_KMEANS_MAX_ATTEMPTS 16
#define MSTG_KMEANS_MAX_ITERS 100
#define MSTG_FUSE_MAX_SCALES 8
/* Host only: the tables of step 2 */
int mstg_lab_inverse_tables(unsigned short* table /* [MSTG_LAB_INV_TABLE_U16] */);
/* Host only: the taps of step 3 (entries past ksize 0) and, where margin != NULL, the smallest distance from a rounding tie.
 * Returns ksize or a negative code. */
int mstg_gaussian_sigma_taps(double sigma, int* taps /* [MSTG_GAUSSIAN_SIGMA_MAX_KSIZE] */, double* margin /*nullable*/);
/* step 1: lab_table = the entries of mstg_lab_tables on the device; one launch */
int mstg_lab_u8(const unsigned char* in, int N, int H, int W, const unsigned short* lab_table, unsigned char* out, void* stream);
/* step 2: inv_table = the entries of mstg_lab_inverse_tables on the device; one launch */
int mstg_lab2rgb_u8(const unsigned char* in, int N, int H, int W, const unsigned short* inv_table, unsigned char* out, void* stream);
/* step 3 on a plane (N, H, W): taps on the HOST (non-negative, sum 256); workspace N * H * W * 2 bytes; two launches */
int mstg_gaussian_sigma_u8(const unsigned char* in, int N, int H, int W, const int* taps, int ksize, unsigned char* out, void* workspace,
                           size_t workspace_bytes, void* stream);
/* step 4; one launch */
int mstg_hsv_gain_u8(const unsigned char* in, int N, int H, int W, float s_gain, float v_gain, unsigned char* out, void* stream);
/* bytes mstg_kmeans_u8 needs; 0 for a parameter outside what is built (mstg_last_error says which) */
size_t mstg_kmeans_workspace_bytes(int N, int K, int attempts);
/* step 5: exactly one of uniforms (attempts * K * 3) and centers0 (N * K * 3, attempts = 1), on the device; workspace 16-byte aligned */
int mstg_kmeans_u8(const unsigned char* img, int N, int H, int W, int K, int attempts, int iters, double eps, const float* uniforms,
                   const float* centers0, int* labels, float* centers, double* compactness, int* best, void* workspace,
                   size_t workspace_bytes, void* stream);
/* step 6: ratios on the HOST, count in 1 .. MSTG_KMEANS_MAX_K; one launch */
int mstg_region_blend_u8(const unsigned char* styled, const unsigned char* orig, const int* labels, int N, int H, int W, const double* ratios,
                         int count, unsigned char* out, void* stream);
/* steps 6 and 4 in one launch */
int mstg_region_blend_gain_u8(const unsigned char* styled, const unsigned char* orig, const int* labels, int N, int H, int W,
                              const double* ratios, int count, float s_gain, float v_gain, unsigned char* out, void* stream);
/* step 7: outputs (S, N, H, W, 3), weights (S floats) on the HOST; one launch */
int mstg_fuse_scales_u8(const unsigned char* outputs, int S, int N, int H, int W, const float* weights, float gain, unsigned char* out,
                        void* stream);
/* bytes of the CLAHE tables mstg_contrast_enhanced_finish needs; 0 for an invalid shape (mstg_last_error says which) */
size_t mstg_contrast_enhanced_finish_workspace_bytes(int N, int H, int W);
int mstg_contrast_enhanced_finish(const unsigned char* styled, int N, int H, int W, const unsigned short* lab_table,
                                  const unsigned short* inv_table, float s_gain, float v_gain, unsigned char* out, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* workspace: N * H * W * 2 bytes, 2-byte aligned (the row pass) */
int mstg_detail_enhanced_finish(const unsigned char* styled, const unsigned char* orig, int N, int H, int W, const unsigned short* lab_table,
                                const unsigned short* inv_table, const int* taps, int ksize, float s_gain, float v_gain, unsigned char* out,
                                void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * FRECHET DISTANCE of two feature sets: calculate_fid of the reference's m_test.py (:37-50), its only evaluation of a trained model,
 * without the InceptionV3 that feeds it.  X1 (n1, d) and X2 (n2, d), float32 or float64, row-major on the device.  Everything below is
 * float64 on the device, every operation rounded (no contraction outside the MFMA), every order fixed: two runs give the same bits.
 * No floating-point atomics, no host synchronisation, no workgroup waits on another.
 *
 *   1. x = (double)X.  Converting float32 features BEFORE the mean is THIS BUILD'S: the reference's mean(0) of float32 features stays
 *        in float32 (np.cov converts first, as here).
 *   2. mu[c] = (s0 + s1 + s2 + s3) / n, s_g = the sum of x[r][c] over the rows r = g, g + 4, g + 8, ... in ascending order, the four
 *        added left to right.
 *   3. A[r][c] = (x1[r][c] - mu1[c]) * (1 / sqrt(n1 - 1)), B likewise from X2: A^T A and B^T B are np.cov(rowvar=False).
 *   4. per column: e[c] = (mu1[c] - mu2[c])^2, a[c] = sum of A[r][c]^2, b[c] = sum of B[r][c]^2, both in the row order of step 2.
 *        ssdiff, tr1, tr2 = the sums of e, a, b over the columns: thread t of 256 adds the columns t, t + 256, ..., a butterfly over
 *        each wave of 64, the four waves left to right.  tr1 = tr S1 and tr2 = tr S2.
 *   5. M = A B^T (n1 x n2) on v_mfma_f64_16x16x4_f64: a 16 x 16 tile of M per workgroup; wave w of 4 runs the K steps k0 = 4 w,
 *        4 w + 16, ... in ascending order (each step is one instruction over the features k0 .. k0 + 3, zeros past d and past the last
 *        row), the four partial tiles are added left to right.
 *   6. The nuclear norm of M.  tr sqrtm(S1 S2) of the reference equals it: S1 S2 = A^T (A B^T) B has the nonzero eigenvalues of
 *        M M^T, and the trace of the square root is the sum of their square roots.  (The d x d product is never formed; for
 *        d = 2048 and 100 samples it has rank 99 at most, and sqrtm's result on it is noise above that.)  One-sided (Hestenes) Jacobi,
 *        THIS BUILD'S choice, on G = M if n2 <= n1, else M^T: p rows, q = min(n1, n2) columns.
 *          pairing: cyclic round robin of q' = q rounded up to even players, q' - 1 rounds a sweep; slot 0 of round r pairs q' - 1
 *          with r, slot i > 0 pairs (r + i) mod (q' - 1) with (r - i) mod (q' - 1); the lower index is a, the higher b; a pair with
 *          the phantom column q (odd q) is a bye.  The pairs of a round touch disjoint columns and run side by side.
 *          pair: alpha = g_a . g_a, beta = g_b . g_b, gamma = g_a . g_b (lane l of 16 adds the rows l, l + 16, ..., then a butterfly);
 *          bar = tol * (sqrt(alpha) * sqrt(beta)), tol = DBL_EPSILON * sqrt(p); |gamma| <= bar: the pair is settled; a NaN on either
 *          side: the pair is UNDECIDED and does not rotate; else
 *          zeta = (beta - alpha) / (2 gamma), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)) (0 for a non-finite zeta),
 *          c = 1 / sqrt(1 + t^2), s = c t, g_a' = c g_a - s g_b, g_b' = s g_a + c g_b.
 *          end: after the first sweep without a rotation (converged if that sweep met no undecided pair, else not), or after
 *          MSTG_FRECHET_MAX_SWEEPS sweeps (not converged).
 *          sigma_j = sqrt(g_j . g_j), sorted descending; nuclear = their sum from the largest down.
 *        One workgroup runs a problem; G lives in LDS when p * q <= 16384 doubles, else in the workspace.
 *        MSTG_FRECHET_MAX_SWEEPS is MEASURED: tests/fid_ref.py runs this Jacobi in numpy; over the shapes of tests/test_m_test_cpu.py
 *        (up to (256, 256, 32), float32 and float64 draws, identical sets, a constant column) the largest count is 22 sweeps; the
 *        bound is twice that.  M of centred factors always has a null space, which is what takes the sweeps.  Non-finite features
 *        give non-finite outputs and converged = 0 after at most that many sweeps, never a hang.
 *   7. fid = ((ssdiff + tr1) + tr2) - 2 nuclear.
 *   out = {ssdiff, tr1, tr2, nuclear, fid}; info = {sweeps used, converged (1 / 0)}.  Four launches.
 *   Refused by name before any launch: n1 or n2 below 2, d below 1 (MSTG_E_BADARG); min(n1, n2) above MSTG_FRECHET_MAX_SAMPLES
 *   (MSTG_E_UNSUPPORTED: the d x d form, which more samples than that need, is not built; the reference uses 100); a product
 *   n1 d, n2 d or n1 n2 that does not fit 31 bits; null pointers; a workspace that is null or too small (MSTG_E_WORKSPACE).
 *   Not built: InceptionV3 (its weights come from the network), so run_model needs the caller's feature extractor.
 * ---------------------------------------------------------------------------------------------- */
#define MSTG_FRECHET_MAX_SAMPLES 256
#define MSTG_FRECHET_MAX_SWEEPS 44
/* bytes mstg_frechet_distance needs: (n1 d + n2 d + 3 d + 2 n1 n2 + min(n1, n2) + 1) doubles; 0 for a refused shape (mstg_last_error
 * says which) */
size_t mstg_frechet_workspace_bytes(int n1, int n2, int d);
/* x1, x2: float64 if is_f64 != 0, else float32; out[5], info[2], workspace 8-byte aligned */
int mstg_frechet_distance(const void* x1, const void* x2, int is_f64, int n1, int n2, int d, double* out, int* info, void* workspace,
                          size_t workspace_bytes, void* stream);
/* bytes mstg_singular_values needs: (m n + 1) doubles; 0 for a refused shape */
size_t mstg_singular_values_workspace_bytes(int m, int n);
/* step 6 alone on M (m, n) float64 row-major, min(m, n) <= MSTG_FRECHET_MAX_SAMPLES: sigma[min(m, n)] descending, info[2]; one launch */
int mstg_singular_values(const double* M, int m, int n, double* sigma, int* info, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * DISPLAY FINISH: process_image of the reference's m_test.py (:52-78), which runs twice per test image: gamma 1.1, the cast to bytes,
 * the 8-bit COLOR_RGB2YUV, equalizeHist of Y, the 8-bit COLOR_YUV2RGB.  N images per launch, any H, W >= 1, H * W * 3 below 2^31,
 * 64-bit offsets.  The OpenCV steps are restated as recalled, not compared with an OpenCV binary (tests/display_finish_ref.py is
 * the same restatement in numpy).  `out` and the workspace must not overlap an input (MSTG_E_BADARG).
 *
 *   1. gamma (:58-71): y (N, 3, H, W) float32 or float16, the generator's output -> bytes (N, H, W, 3).
 *        v = (float)y * 0.5f + 0.5f in float32;
 *        v = v > 0 ? (v < 1 ? v : 1) : 0: the clamp to [0, 1] is THIS BUILD'S (a NaN gives 0); the reference raises a negative v to
 *        the power, gets a NaN and casts that to a byte, which C leaves undefined;
 *        p = (float)pow((double)v, gamma), gamma a double in (0, 16] (the reference: 1.1);
 *        byte = (uint8)(p * 255.f), one float32 product, truncated.
 *        pow is the device library's; the GPU test asserts first that no input of it lies within 64 double ulps of a float32
 *        rounding midpoint, four times OpenCL's bound for pow.
 *   2. the 8-bit COLOR_RGB2YUV (:71), 14-bit fixed point, arithmetic shifts, constants as recalled:
 *        Y = (4899 R + 9617 G + 1868 B + 8192) >> 14;
 *        U = sat_u8((8061 (B - Y) + (128 << 14) + 8192) >> 14);  V = sat_u8((14369 (R - Y) + (128 << 14) + 8192) >> 14).
 *   3. equalizeHist of Y (:72), per image: hist = the 256-bin histogram (integer atomics in LDS; the chunks of an image are added
 *        in ascending order); i0 = the first non-empty bin; if hist[i0] = H W the plane is constant and stays as it is; else
 *        scale = 255.f / (float)(H W - hist[i0]) (one float32 division), lut[i] = 0 for i <= i0 and
 *        lut[i] = sat_u8(cvRound((float)(hist[i0 + 1] + ... + hist[i]) * scale)) above it (one float32 product, round half to even).
 *   4. the 8-bit COLOR_YUV2RGB (:73) of (lut[Y], U, V), constants as recalled, u = U - 128, v = V - 128:
 *        B = sat_u8(Y + ((33292 u + 8192) >> 14));  G = sat_u8(Y + ((-6472 u - 9519 v + 8192) >> 14));
 *        R = sat_u8(Y + ((18678 v + 8192) >> 14)).
 *   Steps 2 to 4 take three launches whatever N (the histograms; the tables; one point-wise kernel).  The reference's / 255.0 and
 *   clip to [0, 1] are the Python side's (m_test.py's process_image here).
 *   Steps 2 to 4 are also the colour step of the reference's `advanced` local-style mode (batch_process_images.py:391-393), which is
 *   broken there and stays refused here: nothing calls them from that mode.
 *   Not built: a comparison with an OpenCV binary; the matplotlib figures.
 * ---------------------------------------------------------------------------------------------- */
/* step 1; one launch */
int mstg_gamma_u8(const void* y, int is_half, int N, int H, int W, double gamma, unsigned char* out, void* stream);
/* bytes mstg_equalize_luma_u8 needs: N * chunks * 256 ints and N * 256 bytes, chunks = min(ceil(H W / 4096), 256); 0 for an invalid shape */
size_t mstg_equalize_luma_workspace_bytes(int N, int H, int W);
/* steps 2 to 4 on (N, H, W, 3) bytes; workspace 4-byte aligned; three launches */
int mstg_equalize_luma_u8(const unsigned char* in, int N, int H, int W, unsigned char* out, void* workspace, size_t workspace_bytes,
                          void* stream);

/* ------------------------------------------------------------------------------------------------
 * BUILD-DEFINED StructuralTransformerBlock pieces. The reference imports the class from a file its snapshot does not contain
 * (enhanced_generator.py:4; call shape :115, :218-225) -- parity unpinned; definition in structural_transformer.py.
 * The block's Linear layers go through mstg_conv2d_* (a Linear over tokens (N, L, dim) is a 1x1 convolution on NHWC).
 * ---------------------------------------------------------------------------------------------- */
/* img (N,3,H,W) fp32 -> out (N, H/4, W/4, 4): per 4x4 cell mean R, G, B and mean |dx| + |dy| of the luminance */
int mstg_structure_map(const float* img, float* out, int N, int H, int W, void* stream);
/* y = (LayerNorm(x; gamma, beta, eps) ) * (1 + gmod[n]) + bmod[n] over tokens x (N, L, dim); gmod / bmod (N, dim) nullable (plain
 * LayerNorm); stats (N*L, 2) = (mean, rstd) for the backward.  dim multiple of 4, <= 256. */
int mstg_ln_mod_fwd(const float* x, const float* gamma, const float* beta, const float* gmod, const float* bmod, float* y,
                    float* stats, int N, int L, int dim, float eps, void* stream);
size_t mstg_ln_mod_bwd_workspace_bytes(int N, int L, int dim);
/* dx, dgamma / dbeta (dim; accumulate != 0: +=), dgmod / dbmod (N, dim; nullable with gmod) */
int mstg_ln_mod_bwd(const float* x, const float* stats, const float* gamma, const float* beta, const float* gmod, const float* dy,
                    float* dx, float* dgamma, float* dbeta, float* dgmod, float* dbmod, int accumulate, int N, int L, int dim,
                    void* workspace, size_t workspace_bytes, void* stream);
/* softmax(q k^T / sqrt(D)) v over all L tokens per image and head: qkv (N, L, 3*heads*D) with q | k | v channel blocks,
 * out (N, L, heads*D), lse (N, heads, L) = log-sum-exp of the scaled scores (kept for the backward).  D in {8, 16, 32, 64}. */
int mstg_flash_attn_fwd(const float* qkv, float* out, float* lse, int N, int L, int heads, int D, void* stream);
/* dqkv from d_out; delta_ws: scratch of N*heads*L floats */
int mstg_flash_attn_bwd(const float* qkv, const float* out, const float* lse, const float* d_out, float* dqkv, float* delta_ws, int N,
                        int L, int heads, int D, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSTG_HIP_H */
