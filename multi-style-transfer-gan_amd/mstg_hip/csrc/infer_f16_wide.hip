// Wide-channel layers of the fp16 inference forward: EnhancedGenerator(channels=32 / 64), stage widths up to 256 channels.
// csrc/infer_f16.hip keeps the channels=16 kernels (a tile's whole input patch in LDS, every output fragment of a pixel in registers);
// at 128 / 256 channels neither fits, so the layers with more than 64 input or output channels run here:
//
//   conv_f16w_kernel  implicit GEMM.  M = 256 output pixels of ONE image per workgroup (a 16 x 16 tile of the compute grid, four rows
//                     per wave), N = 16 * NF output channels per workgroup (64; a MultiScaleBlock branch at 128 channels: 32),
//                     K = taps x Cin walked in K-steps of 32 input channels of one tap on v_mfma_f32_16x16x32_f16.  For an NHWC source
//                     the MFMA's B fragment IS the memory layout (lane (pixel, group g) = 8 consecutive channels = 16 bytes), so a
//                     K-step is one 16-byte load per row and lane straight from global memory -- the neighbouring taps and channel
//                     blocks of a tile hit L1 / L2 -- issued one K-step ahead of the MFMAs.  InstanceNorm + ReLU of the producer
//                     (and the residual add of mode 2) are applied in registers, zero padding after normalisation.  Filter packed
//                     once in fragment order, read from L2.  Epilogue: bias as the first C operand, fp16 NHWC stores, per-tile
//                     sum / sum of squares as fixed-order partial rows (no atomics) finished by f16_norm_finalize_kernel.
//                     Kinds: 0 Conv2d (k x k, stride 1 / 2), 1 ConvTranspose2d k4 s2 p1 (one parity class per workgroup: a dense
//                     2 x 2 filter), 2 MultiScaleBlock (one branch per workgroup: a dense 1x1 or dilated 3x3 writing its slice of
//                     the concat).
//   attn_f16w_kernel  LocalAttention at 128 / 256 channels, one 4 x 4 window per wave: attn_f16r_kernel's MFMA chains, but q^, k^
//                     and v^T (C x 16 each) go to wave-private LDS tiles and the C x C score matrix is walked one 16-column
//                     block at a time (each block's softmax and its rows of O^T are complete in registers); filters streamed
//                     from L2.
//
// Every offset into an activation is 64-bit: at batch 64, 1024 x 1024 and 64 channels one tensor holds 2^32 elements.
#include <hip/hip_fp16.h>

#include "lanes.h"
#include "infer_f16_wide.h"

namespace mstg {

// (named kernels in namespace mstg, not an anonymous one: the per-launch profiler and bench.py attribute work by these symbols)
constexpr int FW_TILE = 16;      // tile edge in compute-grid pixels
constexpr int FW_MAXC = 256;     // widest input / output
constexpr int FW_BIAS_BYTES = 1024;

// the geometry of a wide layer, shared by the host planner, the pack kernel and the convolution kernel
struct WGeom {
    int kind, Cin, Cout, K, stride, pad;
    int NF;        // output fragments per workgroup (16 channels each)
    int nblk_c;    // channel blocks per parity class (kind 0 / 1); kind 2: 4 branches
    int ncls;      // 4 for ConvTranspose, else 1
    int nblk;      // workgroups per tile
    int T;         // tap slots per block in the packed filter
    int chunks;    // Cin / 32
};

// taps of block `blk`: how many, and the source offset (dy, dx) of tap t relative to (gy * stride, gx * stride)
static __host__ __device__ __forceinline__ int wtaps(const WGeom& g, int blk) {
    if (g.kind == 0) return g.K * g.K;
    if (g.kind == 1) return 4;
    return blk == 0 ? 1 : 9;
}
static __host__ __device__ __forceinline__ void wtap_off(const WGeom& g, int blk, int t, int& dy, int& dx) {
    if (g.kind == 0) {
        dy = t / g.K - g.pad;
        dx = t % g.K - g.pad;
    } else if (g.kind == 1) {  // class (py, px) reads source rows y + {-1, 0} (py = 0) or y + {0, 1} (py = 1)
        const int cls = blk / g.nblk_c, py = cls >> 1, px = cls & 1, a = t >> 1, b = t & 1;
        dy = py == 0 ? a - 1 : a;
        dx = px == 0 ? b - 1 : b;
    } else {
        const int d = blk == 0 ? 0 : 1 << (blk - 1);
        dy = blk == 0 ? 0 : (t / 3 - 1) * d;
        dx = blk == 0 ? 0 : (t % 3 - 1) * d;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// filter packing: fp32 PyTorch layouts -> [blk][chunk * T + tap][frag][lane][8] fp16: lane (m = lane & 15, g = lane >> 4) holds
// W[co = co0 + 16 frag + m][ci = 32 chunk + 8 g + j] of the tap; + the fp32 bias vector [Cout]
// ---------------------------------------------------------------------------------------------------------------------------
struct WPackSrc { const float* w[4]; const float* b[4]; };

__global__ void f16w_pack_kernel(WGeom g, WPackSrc s, h16* __restrict__ wpk, float* __restrict__ bias) {
    const long total = (long)g.nblk * g.T * g.chunks * g.NF * 64 * 8;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int j = (int)(e & 7), lane = (int)((e >> 3) & 63);
        long rest = e >> 9;
        const int f = (int)(rest % g.NF);
        rest /= g.NF;
        const int st = (int)(rest % (g.T * g.chunks)), blk = (int)(rest / (g.T * g.chunks));
        const int chunk = st / g.T, t = st % g.T;
        const int m = lane & 15, ci = 32 * chunk + 8 * (lane >> 4) + j;
        float v = 0.f;
        if (g.kind == 0) {
            const int co = (blk % g.nblk_c) * 16 * g.NF + 16 * f + m, ky = t / g.K, kx = t % g.K;
            v = s.w[0][((size_t)(co * g.Cin + ci) * g.K + ky) * g.K + kx];
        } else if (g.kind == 1) {
            // py = 0: source row y-1 <-> ky = 3, row y <-> ky = 1 ; py = 1: row y <-> ky = 2, row y+1 <-> ky = 0
            const int cls = blk / g.nblk_c, py = cls >> 1, px = cls & 1, a = t >> 1, b = t & 1;
            const int co = (blk % g.nblk_c) * 16 * g.NF + 16 * f + m;
            const int ky = py == 0 ? (a == 0 ? 3 : 1) : (a == 0 ? 2 : 0), kx = px == 0 ? (b == 0 ? 3 : 1) : (b == 0 ? 2 : 0);
            v = s.w[0][((size_t)(ci * g.Cout + co) * 4 + ky) * 4 + kx];
        } else {
            const int cb = 16 * f + m;  // channel within the branch
            if (blk == 0) v = t == 0 ? s.w[0][(size_t)cb * g.Cin + ci] : 0.f;
            else if (t < 9) v = s.w[blk][((size_t)(cb * g.Cin + ci) * 3 + t / 3) * 3 + t % 3];
        }
        wpk[e] = (h16)v;
    }
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < g.Cout; c += gridDim.x * blockDim.x) {
        if (g.kind == 2) {
            const int c4 = g.Cout / 4, br = c / c4;
            bias[c] = s.b[br] ? s.b[br][c - br * c4] : 0.f;
        } else {
            bias[c] = s.b[0] ? s.b[0][c] : 0.f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// the convolution kernel
// ---------------------------------------------------------------------------------------------------------------------------
struct F16WArgs {
    const h16* x;           // NHWC fp16 (N, H, W, Cin)
    const h16* res;         // SRC 2: the input is relu((x - mean) * rstd) + res (NHWC fp16 like x)
    h16* y;                 // NHWC fp16 (N, Ho, Wo, Cout)
    const h16* wpk;
    const float* bias;      // [Cout]
    const float* in_stats;  // nullable [N][Cin][2] (mean, rstd): normalise + ReLU on load
    float* partial;         // nullable [N][ncls * tiles][2][Cout]
    WGeom g;
    int N, H, W, Ho, Wo;
    int Gh, Gw, tiles_x, tpi;  // compute grid (Ho x Wo, or H x W for ConvTranspose), tiles per row / per image
    int nblocks;               // grid size = N * tpi * nblk
};

template <int NF, int SRC>
__global__ __launch_bounds__(256, 2) void conv_f16w_kernel(const F16WArgs a) {
    constexpr int RPW = 4;  // rows per wave
    __shared__ float s_sc[FW_MAXC], s_nb[FW_MAXC];
    __shared__ float red[4][2][16 * NF];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nl = lane & 15, g = lane >> 4;
    const WGeom& G = a.g;
    // consecutive logical blocks (the channel blocks / classes of one tile, then the next tile) stay on one XCD's L2
    const int lb = xcd_swizzle(blockIdx.x, a.nblocks);
    const int blk = lb % G.nblk, tile = lb / G.nblk;
    const int n = tile / a.tpi, tt = tile - n * a.tpi, ty = tt / a.tiles_x, tx = tt - ty * a.tiles_x;
    const int cls = G.kind == 1 ? blk / G.nblk_c : 0;
    const int co0 = G.kind == 2 ? blk * 16 * NF : (blk % G.nblk_c) * 16 * NF;
    const int ntap = wtaps(G, blk), nsteps = ntap * G.chunks;
    const int str = G.kind == 0 ? G.stride : 1;
    const bool norm = SRC == 2 || a.in_stats != nullptr;
    if (norm) {  // (x - mean) * rstd = x * sc + nb: the form (and the bits) of f16_norm_residual_kernel
        for (int c = tid; c < G.Cin; c += 256) {
            const float* st = a.in_stats + ((size_t)n * G.Cin + c) * 2;
            s_sc[c] = st[1];
            s_nb[c] = -st[0] * st[1];
        }
    }
    __syncthreads();

    const int gy0 = ty * FW_TILE + RPW * wv, gx = tx * FW_TILE + nl;
    const size_t img = (size_t)n * a.H * a.W * G.Cin;
    const h16* xi = a.x + img;
    const h16* ri = SRC == 2 ? a.res + img : nullptr;
    const h16x8* wp = reinterpret_cast<const h16x8*>(a.wpk) + (size_t)blk * G.T * G.chunks * NF * 64 + lane;

    struct Ops { h16x8 af[NF]; h16x8 v[RPW]; h16x8 r[SRC == 2 ? RPW : 1]; unsigned ok; };
    // operands of K-step s: the filter fragments and this lane's 8 channels of the 4 pixels; out-of-image pixels read offset 0
    auto fetch = [&](int s, Ops& o) {
        const int chunk = s / ntap, t = s - chunk * ntap;
        int dy, dx;
        wtap_off(G, blk, t, dy, dx);
        const h16x8* w = wp + (size_t)(chunk * G.T + t) * NF * 64;
#pragma unroll
        for (int f = 0; f < NF; ++f) o.af[f] = w[f * 64];
        const int ix = gx * str + dx, cofs = 32 * chunk + 8 * g;
        o.ok = 0;
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const int iy = (gy0 + r) * str + dy;
            const bool ok = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            o.ok |= (unsigned)ok << r;
            const size_t off = ok ? ((size_t)iy * a.W + ix) * G.Cin + cofs : 0;
            o.v[r] = *reinterpret_cast<const h16x8*>(xi + off);
            if (SRC == 2) o.r[r] = *reinterpret_cast<const h16x8*>(ri + off);
        }
    };
    f32x4 acc[RPW][NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(a.bias + co0 + 16 * f + 4 * g);
#pragma unroll
        for (int r = 0; r < RPW; ++r) acc[r][f] = b;
    }
    Ops cur, nxt;
    fetch(0, cur);
    for (int s = 0; s < nsteps; ++s) {
        if (s + 1 < nsteps) fetch(s + 1, nxt);
        h16x8 bf[RPW];
        if (norm) {
            const int c0 = 32 * (s / ntap) + 8 * g;
            float sc[8], nb[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) { sc[c] = s_sc[c0 + c]; nb[c] = s_nb[c0 + c]; }
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                h16x8 w = cur.v[r];
                if (SRC == 2) {  // the arithmetic of f16_norm_residual_kernel, so that folding the pass changes no bit
#pragma unroll
                    for (int c = 0; c < 8; ++c) w[c] = (h16)(fmaxf(fmaf((float)w[c], sc[c], nb[c]), 0.f) + (float)cur.r[r][c]);
                } else {
#pragma unroll
                    for (int c = 0; c < 8; ++c) w[c] = (h16)fmaxf(fmaf((float)w[c], sc[c], nb[c]), 0.f);
                }
                bf[r] = ((cur.ok >> r) & 1) ? w : h16x8{0, 0, 0, 0, 0, 0, 0, 0};  // zero padding of the NORMALISED activation
            }
        } else {
#pragma unroll
            for (int r = 0; r < RPW; ++r) bf[r] = ((cur.ok >> r) & 1) ? cur.v[r] : h16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int r = 0; r < RPW; ++r) acc[r][f] = mfma16x16x32_f16(cur.af[f], bf[r], acc[r][f]);
        if (s + 1 < nsteps) cur = nxt;
    }

    // ---- epilogue: lane holds output channels co0 + 16 f + 4 g + {0..3} of compute-grid pixel (gy0 + r, gx) ---------------------
    const int py = cls >> 1, px = cls & 1, mul = G.kind == 1 ? 2 : 1;
    float ssum[NF][4], ssq[NF][4];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int q = 0; q < 4; ++q) ssum[f][q] = ssq[f][q] = 0.f;
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const int gy = gy0 + r;
        if (gy >= a.Gh || gx >= a.Gw) continue;
        const int oy = gy * mul + (G.kind == 1 ? py : 0), ox = gx * mul + (G.kind == 1 ? px : 0);
        h16* yp = a.y + (((size_t)n * a.Ho + oy) * a.Wo + ox) * G.Cout + co0 + 4 * g;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const f32x4 v = acc[r][f];
#pragma unroll
            for (int q = 0; q < 4; ++q) { ssum[f][q] += v[q]; ssq[f][q] += v[q] * v[q]; }
            *reinterpret_cast<h16x4*>(yp + 16 * f) = h16x4{(h16)v[0], (h16)v[1], (h16)v[2], (h16)v[3]};
        }
    }
    if (a.partial) {  // fixed order: 16 lanes of a row by DPP, then the four waves in order
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float s1 = row16_sum(ssum[f][q]), s2 = row16_sum(ssq[f][q]);
                if (nl == 0) {
                    red[wv][0][16 * f + 4 * g + q] = s1;
                    red[wv][1][16 * f + 4 * g + q] = s2;
                }
            }
        __syncthreads();
        if (tid < 2 * 16 * NF) {
            const int k = tid / (16 * NF), c = tid - k * 16 * NF;
            const float sm = red[0][k][c] + red[1][k][c] + red[2][k][c] + red[3][k][c];
            const size_t row = (size_t)n * G.ncls * a.tpi + (size_t)cls * a.tpi + tt;
            a.partial[(row * 2 + k) * G.Cout + co0 + c] = sm;
        }
    }
}

static int wgeom(const mstg_f16_conv_desc* d, WGeom& g) {
    memset(&g, 0, sizeof(g));
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Cin <= 0 || d->Cout <= 0) return fail_arg(MSTG_E_BADARG, "f16 conv: empty tensor");
    if (d->src_nchw_f32 || d->dst_nchw) return fail_arg(MSTG_E_UNSUPPORTED, "f16 wide conv: NHWC fp16 source and destination only");
    if (d->Cin > FW_MAXC || d->Cout > FW_MAXC) return fail_arg(MSTG_E_UNSUPPORTED, "f16 conv: more than 256 input or output channels");
    if (d->Cin % 32) return fail_arg(MSTG_E_ALIGN, "f16 wide conv: NHWC source needs a multiple of 32 channels");
    if (d->act != MSTG_ACT_NONE) return fail_arg(MSTG_E_UNSUPPORTED, "f16 wide conv: no output activation");
    g.kind = d->kind; g.Cin = d->Cin; g.Cout = d->Cout; g.K = d->K; g.stride = d->stride; g.pad = d->pad;
    g.chunks = d->Cin / 32;
    g.NF = 4;
    g.ncls = 1;
    if (d->kind == 0) {
        if (d->Cout % 64) return fail_arg(MSTG_E_ALIGN, "f16 wide conv: output channels must be a multiple of 64");
        if (d->dil != 1 || (d->stride != 1 && d->stride != 2) || d->K < 1 || d->K > 7 || d->pad < 0)
            return fail_arg(MSTG_E_UNSUPPORTED, "f16 wide conv: k <= 7, stride 1 or 2, no dilation");
        if (d->Ho != (d->H + 2 * d->pad - (d->K - 1) - 1) / d->stride + 1 || d->Wo != (d->W + 2 * d->pad - (d->K - 1) - 1) / d->stride + 1)
            return fail_arg(MSTG_E_BADARG, "f16 conv: Ho / Wo do not match the geometry");
        g.nblk_c = d->Cout / 64;
        g.nblk = g.nblk_c;
        g.T = d->K * d->K;
    } else if (d->kind == 1) {
        if (d->Cout % 64) return fail_arg(MSTG_E_ALIGN, "f16 wide convT: output channels must be a multiple of 64");
        if (d->K != 4 || d->stride != 2 || d->pad != 1 || d->Ho != 2 * d->H || d->Wo != 2 * d->W)
            return fail_arg(MSTG_E_UNSUPPORTED, "f16 convT: only k4 s2 p1");
        g.nblk_c = d->Cout / 64;
        g.ncls = 4;
        g.nblk = 4 * g.nblk_c;
        g.T = 4;
    } else if (d->kind == 2) {
        if (d->Cout != d->Cin || d->Ho != d->H || d->Wo != d->W) return fail_arg(MSTG_E_BADARG, "f16 msblock: output must match the input");
        if (d->Cin != 128 && d->Cin != 256) return fail_arg(MSTG_E_UNSUPPORTED, "f16 wide msblock: 128 or 256 channels");
        g.NF = d->Cin / 64;  // one branch (Cin / 4 channels) per workgroup
        g.nblk_c = 4;
        g.nblk = 4;
        g.T = 9;
    } else {
        return fail_arg(MSTG_E_BADARG, "f16 conv: unknown kind");
    }
    return MSTG_OK;
}

static size_t wblob_bytes(const WGeom& g) { return FW_BIAS_BYTES + (size_t)g.nblk * g.T * g.chunks * g.NF * 64 * 16; }

// ---------------------------------------------------------------------------------------------------------------------------
// LocalAttention, C = 128 / 256.  Lane (i = lane & 15, g = lane >> 4); accumulator register r of an MFMA = D[4g + r][i].
// ---------------------------------------------------------------------------------------------------------------------------
// keeps the compiler from hoisting the next fragment row's filter loads (NB^2 of them per product) into registers it does not have
static __device__ __forceinline__ void fence_loads() { asm volatile("" ::: "memory"); }

template <int C>
__global__ __launch_bounds__(256) void attn_f16w_kernel(const h16* __restrict__ x, const float* __restrict__ in_stats,
                                                        const h16* __restrict__ wfrag, const float* __restrict__ bias,
                                                        h16* __restrict__ y, int N, int H, int W) {
    constexpr int NB = C / 16;
    const int tid = threadIdx.x, l = tid & 63, i = l & 15, g = l >> 4;
    // lane (i, g): W[part * C + 16 f + i][16 ks + 4 g + j]
    const h16x4* wl = reinterpret_cast<const h16x4*>(wfrag) + l;
    auto wget = [&](int part, int f, int ks) -> h16x4 { return wl[(size_t)((part * NB + f) * NB + ks) * 64]; };
    const int nwx = W / 4, nwy = H / 4;
    const long nwin = (long)N * nwx * nwy;
    const long wv = blockIdx.x * 4L + (tid >> 6), nwv = gridDim.x * 4L;
    const long per = (nwin + nwv - 1) / nwv, w0 = wv * per, w1 = w0 + per < nwin ? w0 + per : nwin;
    const unsigned lane_off = (unsigned)(((i >> 2) * W + (i & 3)) * C + 4 * g);
    // wave-private LDS tiles of q^ (later O^T), k^ and v^T, fragment-major: [f][lane] 8 bytes (conflict-free)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    h16x4* qh = reinterpret_cast<h16x4*>(smem) + (size_t)(tid >> 6) * 3 * NB * 64 + l;
    h16x4* kh = qh + NB * 64;
    h16x4* vh = kh + NB * 64;
    for (long win = w0; win < w1; ++win) {
        const int cn = (int)(win / ((long)nwx * nwy)), rem = (int)(win - (long)cn * nwx * nwy), cwy = rem / nwx, cwx = rem - cwy * nwx;
        const size_t woff = (((size_t)cn * H + 4 * cwy) * W + 4 * cwx) * C + lane_off;
        h16x4 xa[NB];
#pragma unroll
        for (int h = 0; h < NB; ++h) {
            xa[h] = *reinterpret_cast<const h16x4*>(x + woff + 16 * h);
            if (in_stats) {  // (x - mean) * rstd, ReLU: fp32 arithmetic, one rounding to fp16 (attn_f16r_kernel's form)
                const float* st = in_stats + ((size_t)cn * C + 16 * h + 4 * g) * 2;
                const f32x4 s0 = *reinterpret_cast<const f32x4*>(st), s1 = *reinterpret_cast<const f32x4*>(st + 4);
                const f32x4 sc = f32x4{s0[1], s0[3], s1[1], s1[3]};
                const f32x4 nb = f32x4{-s0[0] * s0[1], -s0[2] * s0[3], -s1[0] * s1[1], -s1[2] * s1[3]};
#pragma unroll
                for (int c = 0; c < 4; ++c) xa[h][c] = (h16)fmaxf(fmaf((float)xa[h][c], sc[c], nb[c]), 0.f);
            }
        }
        // q^ | k^ = F.normalize(X W^T + b) over channels: a row (g, r) is a pixel, its channels lie across 16 lanes and NB fragments
#pragma unroll 1
        for (int part = 0; part < 2; ++part) {
            f32x4 q[NB];
            f32x4 ss = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int f = 0; f < NB; ++f) {
                const float b = bias[part * C + 16 * f + i];
                q[f] = f32x4{b, b, b, b};
#pragma unroll
                for (int h = 0; h < NB; ++h) q[f] = mfma16x16x16_f16(xa[h], wget(part, f, h), q[f]);
                ss += q[f] * q[f];
                fence_loads();
            }
            f32x4 iv;
#pragma unroll
            for (int r = 0; r < 4; ++r) iv[r] = fminf(__builtin_amdgcn_rsqf(row16_sum(ss[r])), 1e12f);  // 1 / max(||.||, 1e-12)
            h16x4* dst = part == 0 ? qh : kh;
#pragma unroll
            for (int f = 0; f < NB; ++f) dst[64 * f] = cvt4(q[f] * iv);
        }
        // v^T = Wv X^T + b: D[channel][pixel]
#pragma unroll 1
        for (int f = 0; f < NB; ++f) {
            f32x4 v = *reinterpret_cast<const f32x4*>(bias + 2 * C + 16 * f + 4 * g);
#pragma unroll
            for (int h = 0; h < NB; ++h) v = mfma16x16x16_f16(wget(2, f, h), xa[h], v);
            vh[64 * f] = cvt4(v);
        }
        // per 16-column block nn of S^T[c2][c1] = sum_p k^[p][c2] q^[p][c1]: softmax over c2 (|S| <= 1: no max subtraction), then
        // O^T[c1 in nn][p] = sum_c2 P^T[c2][c1] v^T[c2][p], written over q^'s block nn (read for the last time just before)
#pragma unroll 1
        for (int nn = 0; nn < NB; ++nn) {
            const h16x4 qb = qh[64 * nn];
            f32x4 st[NB];
            float z = 0.f;
#pragma unroll
            for (int m = 0; m < NB; ++m) {
                st[m] = mfma16x16x16_f16(kh[64 * m], qb, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
                for (int r = 0; r < 4; ++r) { st[m][r] = __expf(st[m][r]); z += st[m][r]; }
            }
            z += __shfl_xor(z, 16, 64);
            z += __shfl_xor(z, 32, 64);
            const float inv = __builtin_amdgcn_rcpf(z);
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int m = 0; m < NB; ++m) o = mfma16x16x16_f16(cvt4(st[m] * f32x4{inv, inv, inv, inv}), vh[64 * m], o);
            qh[64 * nn] = cvt4(o);
        }
        // Y^T[co][p] = bp[co] + sum_c1 Wp[co][c1] O^T[c1][p] -> 8-byte NHWC stores
        h16* yp = y + woff;
#pragma unroll 1
        for (int cf = 0; cf < NB; ++cf) {
            f32x4 acc = *reinterpret_cast<const f32x4*>(bias + 3 * C + 16 * cf + 4 * g);
#pragma unroll
            for (int n1 = 0; n1 < NB; ++n1) acc = mfma16x16x16_f16(wget(3, cf, n1), qh[64 * n1], acc);
            *reinterpret_cast<h16x4*>(yp + 16 * cf) = cvt4(acc);
        }
    }
}

size_t f16w_conv_plan_bytes(const mstg_f16_conv_desc* d) {
    WGeom g;
    if (wgeom(d, g)) return 0;
    return wblob_bytes(g);
}

size_t f16w_conv_partial_bytes(const mstg_f16_conv_desc* d) {
    WGeom g;
    if (wgeom(d, g)) return 0;
    const int gh = d->kind == 1 ? d->H : d->Ho, gw = d->kind == 1 ? d->W : d->Wo;
    const size_t tpi = (size_t)((gh + FW_TILE - 1) / FW_TILE) * ((gw + FW_TILE - 1) / FW_TILE);
    return (size_t)d->N * g.ncls * tpi * 2 * d->Cout * sizeof(float);
}

int f16w_conv_pack(const mstg_f16_conv_desc* d, const float* const w[4], const float* const b[4], void* blob, size_t blob_bytes,
                   hipStream_t st) {
    WGeom g;
    if (int rc = wgeom(d, g)) return rc;
    if (blob_bytes < wblob_bytes(g)) return fail_arg(MSTG_E_WORKSPACE, "f16 conv pack: blob too small");
    if (d->kind == 2 && (!w[1] || !w[2] || !w[3])) return fail_arg(MSTG_E_BADARG, "f16 msblock pack: four weight tensors needed");
    WPackSrc s;
    for (int k = 0; k < 4; ++k) { s.w[k] = w[k]; s.b[k] = b[k]; }
    MSTG_LAUNCH(f16w_pack_kernel, dim3(256), dim3(256), 0, st, g, s, (h16*)((char*)blob + FW_BIAS_BYTES), (float*)blob);
    MSTG_CHECK_LAUNCH("f16w_pack_kernel");
    return MSTG_OK;
}

int f16w_conv_fwd(const mstg_f16_conv_desc* d, const void* blob, const void* x, const float* in_stats, const void* residual, void* y,
                  float* out_stats, void* workspace, size_t workspace_bytes, hipStream_t st) {
    WGeom g;
    if (int rc = wgeom(d, g)) return rc;
    F16WArgs a;
    a.x = (const h16*)x; a.res = (const h16*)residual; a.y = (h16*)y;
    a.bias = (const float*)blob;
    a.wpk = (const h16*)((const char*)blob + FW_BIAS_BYTES);
    a.in_stats = in_stats;
    a.g = g;
    a.N = d->N; a.H = d->H; a.W = d->W; a.Ho = d->Ho; a.Wo = d->Wo;
    a.Gh = d->kind == 1 ? d->H : d->Ho;
    a.Gw = d->kind == 1 ? d->W : d->Wo;
    a.tiles_x = (a.Gw + FW_TILE - 1) / FW_TILE;
    a.tpi = a.tiles_x * ((a.Gh + FW_TILE - 1) / FW_TILE);
    const long blocks = (long)d->N * a.tpi * g.nblk;
    if (blocks > 0x7fffffffL) return fail_arg(MSTG_E_UNSUPPORTED, "f16 wide conv: too many tiles");
    a.nblocks = (int)blocks;
    a.partial = nullptr;
    if (out_stats) {
        if (!workspace || workspace_bytes < f16w_conv_partial_bytes(d))
            return fail_arg(MSTG_E_WORKSPACE, "f16 conv: workspace too small for the statistics partials");
        a.partial = (float*)workspace;
    }
    const int src = residual ? 2 : 0;
    if (g.NF == 4 && src == 0) MSTG_LAUNCH((conv_f16w_kernel<4, 0>), dim3((unsigned)blocks), dim3(256), 0, st, a);
    else if (g.NF == 4) MSTG_LAUNCH((conv_f16w_kernel<4, 2>), dim3((unsigned)blocks), dim3(256), 0, st, a);
    else if (src == 0) MSTG_LAUNCH((conv_f16w_kernel<2, 0>), dim3((unsigned)blocks), dim3(256), 0, st, a);
    else MSTG_LAUNCH((conv_f16w_kernel<2, 2>), dim3((unsigned)blocks), dim3(256), 0, st, a);
    MSTG_CHECK_LAUNCH("conv_f16w_kernel");
    if (out_stats) return f16_norm_finalize(a.partial, out_stats, d->N, g.ncls * a.tpi, d->Cout, d->Cout, (float)((size_t)d->Ho * d->Wo), st);
    return MSTG_OK;
}

int f16w_attn_fwd(const void* x, const float* in_stats, const void* blob, void* y, int N, int H, int W, int C, hipStream_t st) {
    const float* bias = (const float*)blob;
    const h16* wfrag = (const h16*)((const char*)blob + (size_t)4 * C * sizeof(float));
    const long nwin = (long)N * (H / 4) * (W / 4);
    long nb = (long)cu_count() * 2;  // persistent workgroups, each wave a contiguous run of windows
    if (nb * 4 > nwin) nb = (nwin + 3) / 4;
    const size_t lds = (size_t)4 * 3 * C * 16 * sizeof(h16);  // 48 KiB at C = 128, 96 KiB at C = 256
    if (C == 256) {
        static bool attr = false;
        if (!attr) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_f16w_kernel<256>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            attr = true;
        }
    }
    if (C == 128) MSTG_LAUNCH((attn_f16w_kernel<128>), dim3((unsigned)nb), dim3(256), lds, st, (const h16*)x, in_stats, wfrag, bias, (h16*)y, N, H, W);
    else if (C == 256) MSTG_LAUNCH((attn_f16w_kernel<256>), dim3((unsigned)nb), dim3(256), lds, st, (const h16*)x, in_stats, wfrag, bias, (h16*)y, N, H, W);
    else return fail_arg(MSTG_E_UNSUPPORTED, "f16 attn: C must be 16, 32, 64, 128 or 256");
    MSTG_CHECK_LAUNCH("attn_f16w_kernel");
    return MSTG_OK;
}

}  // namespace mstg
