// Gather description shared by the implicit-GEMM convolution kernels (conv_igemm.hip, conv_p32.hip): forward passes and input
// gradients of Conv2d / ConvTranspose2d are all "destination pixel = sum over taps and reduction channels of a source pixel".
#pragma once
#include "common.h"

namespace mstg {

struct IGemmArgs {
    const float* x;
    float* y;
    const float* w;
    const float* bias;
    int N;
    int H, W, x_ctot, x_coff, x_nchw;   // source tensor
    int Cr;                             // reduction channels
    int Ho, Wo, y_ctot, y_coff, y_nchw; // destination tensor
    int Co;                             // output channels
    int Gh, Gw;                         // grid walked by the tiles (Ho x Wo, or the source grid in phase mode)
    int tiles_x, tiles_y;
    int KH, KW, stride, pad, dil, flip, phase;
    int w_so, w_sr;                     // weight strides of the output / reduction channel (taps are innermost)
    int PH, PW;                         // LDS patch extent
    int TG;                             // taps per weight-staging group
    int ntaps;
    int act, accumulate;
    int dbg;
    int psz;           // stream kernel: floats reserved for the LDS patch (>= the dpack exchange tiles)
    int wglob;         // light kernel: filter fragments straight from the packed filter in L2 (no LDS filter slice)
    int TH;            // tile height in grid rows: 8, or 16 where the light kernel gives each wave four rows
    int dpack, tapsx;  // <= 4 output channels: rows of the MFMA tile = (pixel shift delta, channel), see igemm_light_kernel
};

// Grouped launch (mstg_conv2d_fwd_grouped / _dgrad_grouped): G copies of one planned launch in one grid, each with its own source,
// destination, filter and bias.  Workgroup bx of the grid's x dimension belongs to group bx / bpg and is workgroup bx % bpg of that
// group's copy; everything else (tiles, channel blocks, parity classes) is the single-group plan.
constexpr int CONV_GROUP_MAX = 4;
struct ConvGroups {
    const float* x[CONV_GROUP_MAX];
    float* y[CONV_GROUP_MAX];
    const float* w[CONV_GROUP_MAX];     // the module's filter (pack kernels) or the group's packed filter (main kernels)
    const float* bias[CONV_GROUP_MAX];
    int G, bpg;
};
// pointer of group g: a select chain over direct kernel arguments (an indexed load would hide the address space from the compiler)
template <typename T>
__host__ __device__ __forceinline__ T group_pick(const T (&p)[CONV_GROUP_MAX], int g) {
    return g == 0 ? p[0] : (g == 1 ? p[1] : (g == 2 ? p[2] : p[3]));
}

// conv_p32.hip: persistent, software-pipelined kernel for the 4x4 stride-2 family (Conv2d k4 s2 p1, ConvTranspose2d k4 s2 p1 and
// their input gradients) and 1x1 convolutions at 16 / 32 / 64 channels, plus three special-case kernels
constexpr int P32_MAX_STEPS = 64;
constexpr int P32_MAX_SEG = 4;

struct P32Plan {
    int nsteps, nseg;
    struct Seg { int s0, s1, oy, ox; } seg[P32_MAX_SEG];  // one segment per output-parity class (one in all for the stride-2 gather)
    unsigned koff[P32_MAX_STEPS];                          // byte offset of the step's tap / channel chunk from the lane's pixel base
    int8_t tky[P32_MAX_STEPS], tkx[P32_MAX_STEPS];         // filter tap of the step
    int16_t tcb[P32_MAX_STEPS];                            // first source channel of the step
    int PH, PW, pixstride, oy0, ox0, stride, up, NF, TH, npf, wlds, KW;
    unsigned m_pw, m_ntile, m_tx;
};

// Which kernel of conv_p32.hip runs a gather, decided ONCE by p32_route(); the launch, the workspace queries, the fusion probes and
// the kernel name all read this struct.
enum P32Kind {
    P32_NONE,     // not a shape of this file (or MSTG_P32=0)
    P32_CO1,      // one output channel: conv_co1_kernel
    P32_IMG,      // 7x7-style stem on an NCHW image source: conv_p32i_kernel
    P32_HEAD,     // <= 4 output channels packed four taps to an MFMA tile: conv_p32d_kernel
    P32_GENERIC   // conv_p32_kernel; the only kind that folds InstanceNorm in (statistics / backward-sums epilogues)
};
struct P32Route {
    P32Kind kind;
    P32Plan plan;        // P32_GENERIC
    int head_th;         // P32_HEAD: tile height in output rows (16 from 16 output rows on, else 8)
    size_t pack_bytes;   // packed filter + bias in the workspace: what a launch without an epilogue needs
    size_t stats_bytes;  // P32_GENERIC: the same + the epilogue's partial sums [N][<= 1024 workgroups][2][Cout]
    // Where the statistics epilogue of a forward launch is worth its price: it costs 20-25 % on the 12-register variants (32 -> 64 and
    // 64 -> 32 channel 4x4 layers: 88 and 120 us a launch at batch 64, against 35 and 60 us for the statistics pass over their
    // output), a few per cent elsewhere.
    bool stats_pays() const { return kind == P32_GENERIC && plan.npf <= 8; }
    // ... and the backward-sums epilogue.  Measured per layer (profiles/r03_bench_b32_256_kernel_table.txt): it costs the launch
    // 7-30 % where the output has <= 32 channels and the patch <= 8 prefetch registers (then it is cheaper than the two-read statistics
    // pass it replaces: 1x1 fusion convolutions, the 16 <-> 32 channel 4x4 layers), but 45-55 % on the 64-channel / 12-register
    // variants, whose 256 VGPRs it fills -- more than norm_partial_kernel<true> takes on their (small) tensors.
    bool bsums_pays() const { return kind == P32_GENERIC && plan.NF <= 2 && plan.npf <= 8; }
};
P32Route p32_route(const IGemmArgs& a);
// InstanceNorm folded in on either side (P32_GENERIC only): in_stats (nullable) = (mean, rstd) of the raw source, normalised + ReLU'd
// while staged; out_stats (nullable) = (mean, rstd) of the output, summed in the epilogue -- or, with aux / aux_stats (an input-gradient
// launch whose output dz feeds the backward of ReLU(InstanceNorm(aux))), sums [N][2][Cout] = per (image, channel) sum of
// dz [aux^ > 0] and of dz [aux^ > 0] aux^.  Either epilogue needs r.stats_bytes of workspace.
int launch_p32(const IGemmArgs& a, const P32Route& r, const float* in_stats, float* out_stats, const float* aux, const float* aux_stats,
               void* workspace, size_t workspace_bytes, hipStream_t st);
const char* p32_kernel_name(const P32Route& r, int stats);  // stats: the generic kernel's STATS argument (0 = no epilogue)
// Grouped launch of P32_CO1 / P32_GENERIC (no epilogue): a = one group's gather, gs = the groups' pointers (w, bias: the modules' own),
// group k's workspace = ws_stride bytes at workspace + k * ws_stride.  MSTG_E_UNSUPPORTED for the other kinds.
int launch_p32_grouped(const IGemmArgs& a, const P32Route& r, ConvGroups gs, void* workspace, size_t ws_stride, hipStream_t st);
const char* p32_grouped_kernel_name(const P32Route& r);  // "" where launch_p32_grouped does not run

// conv_img.hip: input gradient of the discriminator's image-side layer, Conv2d(3, C, 4, 2, 1) on the NCHW image, on the vector pipe
bool img_dgrad_eligible(const IGemmArgs& a);
int launch_img_dgrad(const IGemmArgs& a, hipStream_t st);
int launch_img_dgrad_grouped(const IGemmArgs& a, ConvGroups gs, hipStream_t st);  // gs.x = dy, gs.y = dx, gs.w = the modules' filters

}  // namespace mstg
