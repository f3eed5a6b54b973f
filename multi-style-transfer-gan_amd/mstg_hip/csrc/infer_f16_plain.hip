// fp16 inference of the plain CycleGAN Generator (pretrain.py:60-97 == batch_process_images.py:20-58) in eval mode: eight
// convolutions, every BatchNorm2d folded into the epilogue of the convolution in front of it (mstg_f16_plain_*, include/mstg_hip.h).
//
// One implicit-GEMM kernel, D[cout][pixel] = sum_k W[cout][k] * X[k][pixel], on v_mfma_f32_16x16x32_f16:
//   * nn.Conv2d(k4,s2,p1):          K = 16 taps x Cin, one GEMM;
//   * nn.ConvTranspose2d(k4,s2,p1): four output-parity classes (py, px), each a dense 2x2 filter with K = 4 x Cin:
//                                   output (2y+py, 2x+px) reads input (y + py - ty, x + px - tx) through filter tap
//                                   (1 - py + 2 ty, 1 - px + 2 tx), ty, tx in {0, 1}.
// The filter is the A operand (rows = output channels) and the activations the B operand (columns = pixels), so that a lane's four
// accumulator registers are four CONSECUTIVE output channels of one pixel: the NHWC store is one 8-byte write per fragment and
// scale / shift come in as one 16-byte load each.
//
// Pixels are flattened over the batch (there are no per-image statistics on this path), so a tile may span images; a row of the
// tile decodes its own (image, y, x) and every activation offset is 64-bit.  Each output's sum walks K in the same order whatever
// its neighbours are: results do not depend on the batch or on the tile a pixel falls in.
//
// K runs in (tap, channel) order in groups of 8 channels (one 16-byte piece of an NHWC pixel, one B-fragment lane), so Cin = 8 and
// 16 put several taps into one K-step.  A K-chunk is 64 = two MFMA K-steps; a stage is KC chunks.  Per stage a block puts into LDS
//   * the activation gather [64 * MT pixels][64 KC k] as rows of 128 KC + 16 bytes (the ds_read_b128 of a fragment, 16 rows at
//     one 16-byte column, then lands on 16 distinct bank quads), and
//   * the filter chunks [16 * NT couts][64 KC k], which the pack kernel laid out in fragment order (LDS image = linear copy,
//     fragment read = lane * 16 bytes, conflict-free),
// double-buffered: the global loads of stage c + 1 are issued before the MFMAs of stage c and written to the other buffer behind
// them, one barrier per stage.  Both operands are staged because the four waves of a block split the pixels and share the whole
// filter chunk: read from L2 each wave would fetch the same 2 KB x NT per chunk.
// Two shapes of the same loop: 128 or 64 pixels with KC = 1 (52 KB or less: three blocks per CU hide each other's loads) where the
// pixels fill the machine, and 64 pixels with KC = 4 (130 KB, 16 loads in flight per thread) where they do not (the 16x16 and
// 32x32 maps at small batch): there a block is alone on its CU and the K loop is a chain of global-memory round trips.
//
// Stem (encoder.0): the (N,3,H,W) fp32 image, K order (tap, 4 channels) = 64 with the fourth channel zero: one chunk.
// Head (decoder.9): Cout = 3 padded to one fragment, tanh, (N,3,2H,2W) fp16 NCHW.
// Fixed summation order, no atomics, no split-K.
#include "lanes.h"

namespace mstg {

constexpr int PL_BK = 64;        // K elements per chunk
constexpr int PL_MAXC = 512;

struct PlainArgs {
    const void* x;
    void* y;
    const h16* wpk;
    const float* scale;
    const float* shift;
    long long M;          // GEMM columns: N * Hm * Wm
    int H, W, Cin;        // source
    int Hm, Wm;           // pixel grid of one GEMM: (Ho, Wo) for the convolution, (H, W) for a parity class
    int Cout, kind, act, dst_nchw;
    int nchunks, ntn, cg, kgroups;  // K chunks, filter tiles, Cin / 8, valid 8-groups of K
    int cg_magic;                   // ceil(2^20 / cg): g / cg == (g * cg_magic) >> 20 for g < 2048, cg <= 64
    int classes;
};

// ---- packed filter -----------------------------------------------------------------------------------------------------
// blob: scale[CoutP] | shift[CoutP] | halves [class][ntile][chunk][kstep 2][frag NT][lane 64][8]
//   element j of lane l = W[cout = ntile * 16 NT + 16 frag + (l & 15)][k = 64 chunk + 32 kstep + 8 (l >> 4) + j]
static inline int plain_nt(int Cout) { return Cout > 32 ? 4 : (Cout > 16 ? 2 : 1); }
static inline int plain_coutp(int Cout) { const int bn = 16 * plain_nt(Cout); return (Cout + bn - 1) / bn * bn; }
static inline int plain_ktot(const mstg_f16_plain_desc* d) { return (d->kind == 1 ? 4 : 16) * (d->src_nchw_f32 ? 4 : d->Cin); }
static inline int plain_nchunks(const mstg_f16_plain_desc* d) { return (plain_ktot(d) + PL_BK - 1) / PL_BK; }

__global__ void plain_pack_kernel(const float* __restrict__ w, const float* __restrict__ scale, const float* __restrict__ shift,
                                  float* __restrict__ bscale, float* __restrict__ bshift, h16* __restrict__ out, int kind, int Cin,
                                  int Cout, int CoutP, int cinp, int NT, int ntn, int nchunks, long long total) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < CoutP) {
        bscale[e] = e < Cout ? (scale ? scale[e] : 1.f) : 0.f;
        bshift[e] = e < Cout ? (shift ? shift[e] : 0.f) : 0.f;
    }
    if (e >= total) return;
    long long r = e;
    const int j = (int)(r & 7); r >>= 3;
    const int l = (int)(r & 63); r >>= 6;
    const int f = (int)(r % NT); r /= NT;
    const int s = (int)(r & 1); r >>= 1;
    const int ch = (int)(r % nchunks); r /= nchunks;
    const int nt = (int)(r % ntn); r /= ntn;
    const int cls = (int)r;
    const int co = nt * 16 * NT + 16 * f + (l & 15);
    const int k = ch * PL_BK + 32 * s + 8 * (l >> 4) + j;
    const int tap = k / cinp, ci = k - tap * cinp;
    const int ntaps = kind == 1 ? 4 : 16;
    float v = 0.f;
    if (co < Cout && tap < ntaps && ci < Cin) {
        if (kind == 1) {  // ConvTranspose2d weight (Cin, Cout, 4, 4)
            const int py = cls >> 1, px = cls & 1, ty = tap >> 1, tx = tap & 1;
            const int ky = 1 - py + 2 * ty, kx = 1 - px + 2 * tx;
            v = w[(((size_t)ci * Cout + co) * 4 + ky) * 4 + kx];
        } else {          // Conv2d weight (Cout, Cin, 4, 4)
            v = w[(((size_t)co * Cin + ci) * 4 + (tap >> 2)) * 4 + (tap & 3)];
        }
    }
    out[e] = (h16)v;
}

// ---- the convolution -----------------------------------------------------------------------------------------------------
// LDS bytes of a block: two stages of (activation rows + filter chunks)
constexpr int plain_arow(int KC) { return 128 * KC + 16; }
constexpr int plain_lds_bytes(int MT, int NT, int KC) { return 2 * (64 * MT * plain_arow(KC) + KC * NT * 2048); }

template <int MT, int NT, bool STEM, int KC>
__global__ __launch_bounds__(256) void plain_conv_f16_kernel(PlainArgs a) {
    constexpr int BM = 64 * MT;          // pixels per block: 4 waves x MT fragments
    constexpr int QN = 8 * KC;           // 16-byte pieces per pixel row of a stage (KC chunks of 64 k)
    constexpr int RP = 256 / QN;         // rows staged per pass of the block
    constexpr int NA = BM / RP;          // 16-byte activation pieces per thread and stage
    constexpr int AROW = plain_arow(KC); // bytes per pixel row in LDS: 4 (mod 64) dwords, conflict-free fragment reads
    constexpr int WCH = NT * 2048;       // bytes of one filter chunk
    constexpr int WST = KC * WCH;        // ... of one stage
    constexpr int NW = (WST / 16 + 255) / 256;
    extern __shared__ __attribute__((aligned(16))) unsigned char plain_smem[];
    unsigned char* const As = plain_smem;                  // [2][BM * AROW]
    unsigned char* const Ws = plain_smem + 2 * BM * AROW;  // [2][WST]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // tiles in (pixel tile, filter tile, class) order, one contiguous run of them per XCD: the blocks that share an activation
    // tile (every filter tile and class of it) then meet in ONE L2 instead of fetching it into eight
    int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int cls = bid % a.classes; bid /= a.classes;
    const int nt = bid % a.ntn;
    const long long m0 = (long long)(bid / a.ntn) * BM;
    const int py = cls >> 1, px = cls & 1;
    const int S = a.kind == 1 ? 1 : 2;

    // this thread's rows of the gather: piece q of rows tid / QN + RP i
    const int q = tid % QN, r0 = tid / QN;
    // Per row, once: the image, the window origin, the element offset of the origin pixel and one validity bit per filter row /
    // column, so that a stage costs one 64-bit add, one bit test and one load per piece (an invalid piece reads element 0 and is
    // zeroed) instead of a 64-bit multiply chain per piece.
    long long nbase[NA], rowoff[NA];
    int by[NA], bx[NA], ymask[NA], xmask[NA];
    const int hw = a.Hm * a.Wm;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const long long m = m0 + r0 + RP * i;
        nbase[i] = -1;
        by[i] = bx[i] = ymask[i] = xmask[i] = 0;
        rowoff[i] = 0;
        if (m < a.M) {
            const long long n = m / hw;
            const int rem = (int)(m - n * hw);
            const int oy = rem / a.Wm, ox = rem - oy * a.Wm;
            nbase[i] = n;
            by[i] = oy * S;
            bx[i] = ox * S;
            rowoff[i] = ((n * a.H + by[i]) * (long long)a.W + bx[i]) * a.Cin;
            for (int t = 0; t < 4; ++t) {  // filter row / column t reads source row by + dy(t): dy = t - 1, or py - t for a parity class
                const int dy = a.kind == 1 ? py - t : t - 1, dx = a.kind == 1 ? px - t : t - 1;
                const bool tv = a.kind != 1 || t < 2;
                ymask[i] |= (int)(tv && (unsigned)(by[i] + dy) < (unsigned)a.H) << t;
                xmask[i] |= (int)(tv && (unsigned)(bx[i] + dx) < (unsigned)a.W) << t;
            }
        }
    }

    const unsigned char* wsrc = reinterpret_cast<const unsigned char*>(a.wpk) + ((size_t)(cls * a.ntn + nt) * a.nchunks) * WCH;

    uint4 areg[NA], wreg[NW];
    auto load_chunk = [&](int ch) {  // ch: stage = chunks KC ch .. KC ch + KC - 1 (contiguous in the blob)
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int p = tid + 256 * i;
            bool ok = p * 16 < WST;
            if constexpr (KC > 1) ok = ok && ch * KC + p * 16 / WCH < a.nchunks;  // the last stage may be short
            const uint4 v = *reinterpret_cast<const uint4*>(wsrc + (ok ? (size_t)ch * WST + (size_t)p * 16 : (size_t)0));
            wreg[i] = ok ? v : uint4{0, 0, 0, 0};
        }
        if constexpr (STEM) {
            // group q = taps (ty, tx0) and (ty, tx0 + 1) x channels 0..2 (+ a zero) of the fp32 NCHW image
            const float* img = reinterpret_cast<const float*>(a.x);
            const int ty = q >> 1, tx0 = (q & 1) * 2;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                h16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                const int iy = by[i] + ty - 1;
                if (nbase[i] >= 0 && (unsigned)iy < (unsigned)a.H) {
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const int ix = bx[i] + tx0 + t - 1;
                        if ((unsigned)ix < (unsigned)a.W) {
#pragma unroll
                            for (int c = 0; c < 3; ++c)
                                v[4 * t + c] = (h16)img[((nbase[i] * 3 + c) * a.H + iy) * (long long)a.W + ix];
                        }
                    }
                }
                areg[i] = *reinterpret_cast<uint4*>(&v);
            }
        } else {
            const h16* src = reinterpret_cast<const h16*>(a.x);
            const int g = ch * QN + q;
            const bool gok = g < a.kgroups;
            const int tap = (int)(((unsigned)g * (unsigned)a.cg_magic) >> 20), c = (g - tap * a.cg) * 8;  // g / cg, g < 2048
            const int ty = a.kind == 1 ? tap >> 1 : tap >> 2, tx = a.kind == 1 ? tap & 1 : tap & 3;
            const int dy = a.kind == 1 ? py - ty : ty - 1, dx = a.kind == 1 ? px - tx : tx - 1;
            const long long delta = ((long long)dy * a.W + dx) * a.Cin + c;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const bool ok = gok && ((ymask[i] >> ty) & (xmask[i] >> tx) & 1);
                const uint4 v = *reinterpret_cast<const uint4*>(src + (ok ? rowoff[i] + delta : 0ll));
                areg[i] = ok ? v : uint4{0, 0, 0, 0};
            }
        }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int p = tid + 256 * i;
            if (p * 16 < WST) *reinterpret_cast<uint4*>(&Ws[buf * WST + p * 16]) = wreg[i];
        }
#pragma unroll
        for (int i = 0; i < NA; ++i)
            *reinterpret_cast<uint4*>(&As[buf * BM * AROW + (r0 + RP * i) * AROW + q * 16]) = areg[i];
    };

    f32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int f = 0; f < NT; ++f) acc[m][f] = f32x4{0.f, 0.f, 0.f, 0.f};

    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    const int nstages = (a.nchunks + KC - 1) / KC;
    for (int ch = 0; ch < nstages; ++ch) {
        const int buf = ch & 1;
        const bool more = ch + 1 < nstages;
        if (more) load_chunk(ch + 1);  // in flight under the MFMAs below
#pragma unroll
        for (int s = 0; s < 2 * KC; ++s) {  // K-steps of 32 in k order
            h16x8 wf[NT], xf[MT];
#pragma unroll
            for (int f = 0; f < NT; ++f) wf[f] = *reinterpret_cast<const h16x8*>(&Ws[buf * WST + ((s * NT + f) * 64 + lane) * 16]);
#pragma unroll
            for (int m = 0; m < MT; ++m)
                xf[m] = *reinterpret_cast<const h16x8*>(&As[buf * BM * AROW + (wave * 16 * MT + 16 * m + (lane & 15)) * AROW + 64 * s + 16 * (lane >> 4)]);
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int f = 0; f < NT; ++f) acc[m][f] = mfma16x16x32_f16(wf[f], xf[m], acc[m][f]);
        }
        if (more) store_chunk(buf ^ 1);  // last read before the barrier that closed chunk ch - 1
        __syncthreads();
    }

    // epilogue: acc[m][f][r] = D[cout = 16 NT nt + 16 f + 4 (lane >> 4) + r][pixel = m0 + 16 MT wave + 16 m + (lane & 15)]
    h16* y = reinterpret_cast<h16*>(a.y);
    const int Ho = a.kind == 1 ? 2 * a.Hm : a.Hm, Wo = a.kind == 1 ? 2 * a.Wm : a.Wm;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const long long pm = m0 + wave * 16 * MT + 16 * m + (lane & 15);
        if (pm >= a.M) continue;
        const long long n = pm / hw;
        const int rem = (int)(pm - n * hw);
        int oy = rem / a.Wm, ox = rem - oy * a.Wm;
        if (a.kind == 1) {
            oy = 2 * oy + py;
            ox = 2 * ox + px;
        }
#pragma unroll
        for (int f = 0; f < NT; ++f) {
            const int co = nt * 16 * NT + 16 * f + 4 * (lane >> 4);
            if (co >= a.Cout) continue;
            const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scale + co), sh = *reinterpret_cast<const f32x4*>(a.shift + co);
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = apply_act(acc[m][f][r] * sc[r] + sh[r], a.act);
            if (a.dst_nchw) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (co + r < a.Cout) y[((n * a.Cout + co + r) * Ho + oy) * (long long)Wo + ox] = (h16)v[r];
            } else {
                const h16x4 o = {(h16)v[0], (h16)v[1], (h16)v[2], (h16)v[3]};
                *reinterpret_cast<h16x4*>(y + ((n * Ho + oy) * (long long)Wo + ox) * a.Cout + co) = o;
            }
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static const char* plain_validate(const mstg_f16_plain_desc* d) {
    if (!d) return "mstg_f16_plain: null descriptor";
    if (d->kind != 0 && d->kind != 1) return "mstg_f16_plain: kind must be 0 (Conv2d k4 s2 p1) or 1 (ConvTranspose2d k4 s2 p1)";
    if (d->K != 4) return "mstg_f16_plain: only 4x4 stride-2 padding-1 filters (K must be 4)";
    if (d->Cin > PL_MAXC || d->Cout > PL_MAXC || d->Cin < 1 || d->Cout < 1) return "mstg_f16_plain: Cin and Cout must be in 1..512";
    if (d->src_nchw_f32) {
        if (d->kind != 0 || d->Cin != 3) return "mstg_f16_plain: the fp32 NCHW source is the 3-channel stem of a Conv2d";
    } else if (d->Cin % 8) {
        return "mstg_f16_plain: Cin must be a multiple of 8 (or the 3-channel fp32 stem)";
    }
    if (d->dst_nchw) {
        if (d->Cout > 4) return "mstg_f16_plain: the NCHW destination is the image head (Cout <= 4)";
    } else if (d->Cout % 8) {
        return "mstg_f16_plain: Cout must be a multiple of 8 (or the NCHW image head)";
    }
    if (d->act != MSTG_ACT_NONE && d->act != MSTG_ACT_RELU && d->act != MSTG_ACT_LEAKY02 && d->act != MSTG_ACT_TANH)
        return "mstg_f16_plain: act must be none, ReLU, LeakyReLU(0.2) or tanh";
    return nullptr;
}

static size_t plain_filter_halves(const mstg_f16_plain_desc* d) {
    return (size_t)(d->kind == 1 ? 4 : 1) * plain_coutp(d->Cout) * plain_nchunks(d) * PL_BK;
}

template <int MT, int NT, bool STEM, int KC>
static int plain_launch1(const PlainArgs& a, unsigned grid, hipStream_t st) {
    constexpr int lds = plain_lds_bytes(MT, NT, KC);
    if constexpr (lds > 64 * 1024) {
        static hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&plain_conv_f16_kernel<MT, NT, STEM, KC>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return fail_launch(e, "hipFuncSetAttribute(plain_conv_f16_kernel)");
    }
    MSTG_LAUNCH((plain_conv_f16_kernel<MT, NT, STEM, KC>), dim3(grid), dim3(256), lds, st, a);
    return MSTG_OK;
}
template <int NT>
static int plain_launch(const PlainArgs& a, int MT, int KC, bool stem, unsigned grid, hipStream_t st) {
    if (stem) return MT == 2 ? plain_launch1<2, NT, true, 1>(a, grid, st) : plain_launch1<1, NT, true, 1>(a, grid, st);
    if (MT == 2) return plain_launch1<2, NT, false, 1>(a, grid, st);
    return KC == 4 ? plain_launch1<1, NT, false, 4>(a, grid, st) : plain_launch1<1, NT, false, 1>(a, grid, st);
}

}  // namespace mstg

using namespace mstg;

extern "C" size_t mstg_f16_plain_plan_bytes(const mstg_f16_plain_desc* d) {
    if (const char* e = plain_validate(d)) {
        fail_arg(MSTG_E_UNSUPPORTED, e);
        return 0;
    }
    return (size_t)plain_coutp(d->Cout) * 8 + plain_filter_halves(d) * 2;
}

extern "C" int mstg_f16_plain_pack(const mstg_f16_plain_desc* d, const float* w, const float* scale, const float* shift, void* blob,
                                   size_t blob_bytes, void* stream) {
    if (const char* e = plain_validate(d)) return fail_arg(MSTG_E_UNSUPPORTED, e);
    if (!w || !blob) return fail_arg(MSTG_E_BADARG, "mstg_f16_plain_pack: null pointer");
    if (blob_bytes < mstg_f16_plain_plan_bytes(d)) return fail_arg(MSTG_E_BADARG, "mstg_f16_plain_pack: blob smaller than mstg_f16_plain_plan_bytes");
    const int CoutP = plain_coutp(d->Cout), NT = plain_nt(d->Cout);
    float* bscale = reinterpret_cast<float*>(blob);
    float* bshift = bscale + CoutP;
    h16* out = reinterpret_cast<h16*>(bshift + CoutP);
    const long long total = (long long)plain_filter_halves(d);
    const unsigned grid = (unsigned)((total + 255) / 256);
    MSTG_LAUNCH(plain_pack_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, scale, shift, bscale, bshift, out, d->kind, d->Cin,
                d->Cout, CoutP, d->src_nchw_f32 ? 4 : d->Cin, NT, CoutP / (16 * NT), plain_nchunks(d), total);
    MSTG_CHECK_LAUNCH("mstg_f16_plain_pack");
    return MSTG_OK;
}

extern "C" int mstg_f16_plain_fwd(const mstg_f16_plain_desc* d, const void* blob, const void* x, void* y, void* stream) {
    if (const char* e = plain_validate(d)) return fail_arg(MSTG_E_UNSUPPORTED, e);
    if (!blob || !x || !y) return fail_arg(MSTG_E_BADARG, "mstg_f16_plain_fwd: null pointer");
    if (d->N < 1 || d->H < 1 || d->W < 1) return fail_arg(MSTG_E_BADARG, "mstg_f16_plain_fwd: N, H, W must be positive");
    if (d->kind == 0 && ((d->H | d->W) & 1)) return fail_arg(MSTG_E_BADARG, "mstg_f16_plain_fwd: a k4 s2 p1 convolution needs even H and W");
    const int Hm = d->kind == 1 ? d->H : d->H / 2, Wm = d->kind == 1 ? d->W : d->W / 2;
    const int Ho = d->kind == 1 ? 2 * d->H : Hm, Wo = d->kind == 1 ? 2 * d->W : Wm;
    if (d->Ho != Ho || d->Wo != Wo) return fail_arg(MSTG_E_BADARG, "mstg_f16_plain_fwd: Ho / Wo do not match the layer (H / 2 or 2 H)");
    const long long M = (long long)d->N * Hm * Wm;
    if ((long long)Hm * Wm >= (1ll << 30)) return fail_arg(MSTG_E_BADARG, "mstg_f16_plain_fwd: image too large");
    const int CoutP = plain_coutp(d->Cout), NT = plain_nt(d->Cout), classes = d->kind == 1 ? 4 : 1;
    PlainArgs a;
    a.x = x;
    a.y = y;
    a.scale = reinterpret_cast<const float*>(blob);
    a.shift = a.scale + CoutP;
    a.wpk = reinterpret_cast<const h16*>(a.shift + CoutP);
    a.M = M;
    a.H = d->H; a.W = d->W; a.Cin = d->Cin;
    a.Hm = Hm; a.Wm = Wm;
    a.Cout = d->Cout; a.kind = d->kind; a.act = d->act; a.dst_nchw = d->dst_nchw;
    a.nchunks = plain_nchunks(d);
    a.ntn = CoutP / (16 * NT);
    a.cg = d->src_nchw_f32 ? 1 : d->Cin / 8;
    a.kgroups = plain_ktot(d) / 8;
    a.cg_magic = ((1 << 20) + a.cg - 1) / a.cg;
    a.classes = classes;
    // 128-pixel tiles when they still give every CU two blocks.  Else (the 16x16 and 32x32 maps at small batch) 64-pixel tiles, and
    // where K is deep and there is at most one block per CU, stages of four chunks: a block is then alone on its CU and its K loop
    // is a chain of global-memory round trips, one per stage, with four times the bytes in flight each.  The k order of every sum
    // is the same in all variants.
    const long long per = (long long)classes * a.ntn;
    const long long blocks128 = (M + 127) / 128 * per;
    const int MT = blocks128 >= 512 ? 2 : 1;
    const int KC = MT == 1 && a.nchunks >= 4 && (M + 63) / 64 * per <= 256 ? 4 : 1;
    const long long blocks = (M + 64 * MT - 1) / (64 * MT) * per;
    if (blocks >= (1ll << 31)) return fail_arg(MSTG_E_BADARG, "mstg_f16_plain_fwd: too many tiles");
    const bool stem = d->src_nchw_f32 != 0;
    const int rc = NT == 4   ? plain_launch<4>(a, MT, KC, stem, (unsigned)blocks, (hipStream_t)stream)
                   : NT == 2 ? plain_launch<2>(a, MT, KC, stem, (unsigned)blocks, (hipStream_t)stream)
                             : plain_launch<1>(a, MT, KC, stem, (unsigned)blocks, (hipStream_t)stream);
    if (rc != MSTG_OK) return rc;
    MSTG_CHECK_LAUNCH("mstg_f16_plain_fwd");
    return MSTG_OK;
}
