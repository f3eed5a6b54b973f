// Mixed-precision multi-style loss (mstg_style16_*, include/mstg_hip.h; mstg_hip/style_f16.py): the frozen VGG-topology stack up to
// relu4_3, its 2x2 max-pools and the Gram matrices with fp16 features in the forward and bf16 gradients in the backward.
//
// Why two formats: the gradients of this loss are 1e-7 and below and shrink with 1 / (C H W); fp16 would flush them without a loss
// scale.  bf16 has fp32's exponent range, so the backward needs no scale, no overflow bookkeeping and no state.  The forward keeps
// fp16's three extra mantissa bits because the loss is a difference of Gram matrices.
//
// Convolution (3x3, stride 1, pad 1): one implicit-GEMM kernel for both formats, D[cout][pixel] = sum_k W[cout][k] X[k][pixel] on
// v_mfma_f32_16x16x32_f16 / _bf16, the loop of plain_conv_f16_kernel (infer_f16_plain.hip): the filter is the A operand, so a lane's
// four accumulators are four consecutive channels of one pixel; both operands are staged in LDS, double-buffered, one barrier per
// K chunk of 64; pixels are flattened over the batch and every row decodes its own (image, y, x); K runs in (tap, channel) order in
// groups of 8 channels; every output's sum walks K in the same order whatever tile it falls in.  The input gradient of a layer is
// the same kernel in bf16 on that layer's filter packed flipped and transposed, and its epilogue multiplies by the ReLU mask of the
// layer's input activation (the saved fp16 feature at the same pixel and channels): what it stores is the gradient in front of
// that ReLU.
// Boundary forms: the stem reads the (N,3,H,W) fp32 image, K order (tap, 4 channels) = 36 of one chunk; the image gradient has
// Cout = 3 padded to one fragment and writes (N,3,H,W) fp32.
// Fixed summation order, no atomics, no split-K.
#include "lanes.h"

namespace mstg {

constexpr int SC_BK = 64;  // K elements per chunk
constexpr int SC_MAXC = 512;

template <typename T> struct vec8;
template <> struct vec8<h16> { typedef h16x8 type; };
template <> struct vec8<b16> { typedef b16x8 type; };
template <typename T> struct vec4;
template <> struct vec4<h16> { typedef h16x4 type; };
template <> struct vec4<b16> { typedef b16x4 type; };

template <typename T>
__device__ __forceinline__ f32x4 mfma16x16x32(typename vec8<T>::type a, typename vec8<T>::type b, f32x4 c) {
    if constexpr (std::is_same<T, h16>::value) return mfma16x16x32_f16(a, b, c);
    else return mfma16x16x32_bf16(a, b, c);
}

struct SConvArgs {
    const void* x;
    void* y;
    const h16* mask;
    const unsigned char* wpk;
    const float* bias;
    long long M;  // GEMM columns: N * H * W
    int H, W, Cin, Cout, relu, dst_nchw;
    int nchunks, ntn, cg, kgroups;  // K chunks, filter tiles, Cin / 8, valid 8-groups of K
    int cg_magic;                   // ceil(2^20 / cg): g / cg == (g * cg_magic) >> 20 for g < 2048, cg <= 64
};

// ---- packed filter -------------------------------------------------------------------------------------------------------------
// blob: bias[CoutP] fp32 | T [ntile][chunk][kstep 2][frag NT][lane 64][8]
//   element j of lane l = W[cout = ntile * 16 NT + 16 frag + (l & 15)][k = 64 chunk + 32 kstep + 8 (l >> 4) + j], k = tap * cinp + ci
static inline int sconv_nt(int Cout) { return Cout > 32 ? 4 : (Cout > 16 ? 2 : 1); }
static inline int sconv_coutp(int Cout) { const int bn = 16 * sconv_nt(Cout); return (Cout + bn - 1) / bn * bn; }
static inline int sconv_cinp(const mstg_style16_conv_desc* d) { return d->src_nchw_f32 ? 4 : d->Cin; }
static inline int sconv_nchunks(const mstg_style16_conv_desc* d) { return (9 * sconv_cinp(d) + SC_BK - 1) / SC_BK; }

template <typename T>
__global__ void style_conv16_pack_kernel(const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ bbias,
                                         T* __restrict__ out, int flip, int Cin, int Cout, int CoutP, int cinp, int NT, int nchunks,
                                         long long total) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < CoutP) bbias[e] = (e < Cout && bias) ? bias[e] : 0.f;
    if (e >= total) return;
    long long r = e;
    const int j = (int)(r & 7); r >>= 3;
    const int l = (int)(r & 63); r >>= 6;
    const int f = (int)(r % NT); r /= NT;
    const int s = (int)(r & 1); r >>= 1;
    const int ch = (int)(r % nchunks); r /= nchunks;
    const int nt = (int)r;
    const int co = nt * 16 * NT + 16 * f + (l & 15);
    const int k = ch * SC_BK + 32 * s + 8 * (l >> 4) + j;
    const int tap = k / cinp, ci = k - tap * cinp;
    float v = 0.f;
    if (co < Cout && tap < 9 && ci < Cin)
        v = flip ? w[((size_t)ci * Cout + co) * 9 + (8 - tap)]  // layer filter (Cin, Cout, 3, 3) read flipped and transposed
                 : w[((size_t)co * Cin + ci) * 9 + tap];
    out[e] = (T)v;
}

// ---- the convolution -------------------------------------------------------------------------------------------------------------
constexpr int SC_AROW = 144;  // bytes per pixel row of a chunk in LDS: 128 + 16, 4 (mod 64) dwords, conflict-free fragment reads
constexpr int sconv_lds_bytes(int MT, int NT) { return 2 * (64 * MT * SC_AROW + NT * 2048); }

template <typename T, int MT, int NT, bool STEM>
__global__ __launch_bounds__(256) void style_conv16_kernel(SConvArgs a) {
    typedef typename vec8<T>::type T8;
    typedef typename vec4<T>::type T4;
    constexpr int BM = 64 * MT;    // pixels per block: 4 waves x MT fragments
    constexpr int RP = 32;         // rows staged per pass of the block (8 pieces of 16 bytes per row)
    constexpr int NA = BM / RP;    // 16-byte activation pieces per thread and chunk
    constexpr int WCH = NT * 2048; // bytes of one filter chunk
    constexpr int NW = (WCH / 16 + 255) / 256;
    extern __shared__ __attribute__((aligned(16))) unsigned char sconv_smem[];
    unsigned char* const As = sconv_smem;                     // [2][BM * SC_AROW]
    unsigned char* const Ws = sconv_smem + 2 * BM * SC_AROW;  // [2][WCH]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // tiles in (pixel tile, filter tile) order, one contiguous run per XCD: the filter tiles of one pixel tile meet in one L2
    int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int nt = bid % a.ntn;
    const long long m0 = (long long)(bid / a.ntn) * BM;

    const int q = tid & 7, r0 = tid >> 3;
    long long nbase[NA], rowoff[NA];
    int by[NA], bx[NA], ymask[NA], xmask[NA];
    const int hw = a.H * a.W;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const long long m = m0 + r0 + RP * i;
        nbase[i] = -1;
        by[i] = bx[i] = ymask[i] = xmask[i] = 0;
        rowoff[i] = 0;
        if (m < a.M) {
            const long long n = m / hw;
            const int rem = (int)(m - n * hw);
            const int oy = rem / a.W, ox = rem - oy * a.W;
            nbase[i] = n;
            by[i] = oy;
            bx[i] = ox;
            rowoff[i] = m * a.Cin;  // NHWC: the flat pixel index is the pixel's position
#pragma unroll
            for (int t = 0; t < 3; ++t) {  // filter row / column t reads source row oy + t - 1
                ymask[i] |= (int)((unsigned)(oy + t - 1) < (unsigned)a.H) << t;
                xmask[i] |= (int)((unsigned)(ox + t - 1) < (unsigned)a.W) << t;
            }
        }
    }

    const unsigned char* wsrc = a.wpk + ((size_t)nt * a.nchunks) * WCH;

    uint4 areg[NA], wreg[NW];
    auto load_chunk = [&](int ch) {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int p = tid + 256 * i;
            const bool ok = p * 16 < WCH;
            const uint4 v = *reinterpret_cast<const uint4*>(wsrc + (ok ? (size_t)ch * WCH + (size_t)p * 16 : (size_t)0));
            wreg[i] = ok ? v : uint4{0, 0, 0, 0};
        }
        if constexpr (STEM) {
            // group q = taps 2q and 2q + 1 (tap = 3 ty + tx) x channels 0..2 (+ a zero) of the fp32 NCHW image
            const float* img = reinterpret_cast<const float*>(a.x);
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                T8 v;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = (T)0.f;
                if (nbase[i] >= 0) {
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const int tap = 2 * q + t, ty = tap / 3, tx = tap - 3 * ty;
                        const int iy = by[i] + ty - 1, ix = bx[i] + tx - 1;
                        if (tap < 9 && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) v[4 * t + c] = (T)img[((nbase[i] * 3 + c) * a.H + iy) * (long long)a.W + ix];
                        }
                    }
                }
                areg[i] = *reinterpret_cast<uint4*>(&v);
            }
        } else {
            const T* src = reinterpret_cast<const T*>(a.x);
            const int g = ch * 8 + q;
            const bool gok = g < a.kgroups;
            const int tap = gok ? (int)(((unsigned)g * (unsigned)a.cg_magic) >> 20) : 0, c = gok ? (g - tap * a.cg) * 8 : 0;  // g / cg
            const int ty = tap / 3, tx = tap - 3 * ty;
            const long long delta = ((long long)(ty - 1) * a.W + (tx - 1)) * a.Cin + c;
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
            if (p * 16 < WCH) *reinterpret_cast<uint4*>(&Ws[buf * WCH + p * 16]) = wreg[i];
        }
#pragma unroll
        for (int i = 0; i < NA; ++i) *reinterpret_cast<uint4*>(&As[buf * BM * SC_AROW + (r0 + RP * i) * SC_AROW + q * 16]) = areg[i];
    };

    f32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int f = 0; f < NT; ++f) acc[m][f] = f32x4{0.f, 0.f, 0.f, 0.f};

    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    for (int ch = 0; ch < a.nchunks; ++ch) {
        const int buf = ch & 1;
        const bool more = ch + 1 < a.nchunks;
        if (more) load_chunk(ch + 1);  // in flight under the MFMAs below
#pragma unroll
        for (int s = 0; s < 2; ++s) {  // K-steps of 32 in k order
            T8 wf[NT], xf[MT];
#pragma unroll
            for (int f = 0; f < NT; ++f) wf[f] = *reinterpret_cast<const T8*>(&Ws[buf * WCH + ((s * NT + f) * 64 + lane) * 16]);
#pragma unroll
            for (int m = 0; m < MT; ++m)
                xf[m] = *reinterpret_cast<const T8*>(&As[buf * BM * SC_AROW + (wave * 16 * MT + 16 * m + (lane & 15)) * SC_AROW + 64 * s + 16 * (lane >> 4)]);
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int f = 0; f < NT; ++f) acc[m][f] = mfma16x16x32<T>(wf[f], xf[m], acc[m][f]);
        }
        if (more) store_chunk(buf ^ 1);  // last read before the barrier that closed chunk ch - 1
        __syncthreads();
    }

    // epilogue: acc[m][f][r] = D[cout = 16 NT nt + 16 f + 4 (lane >> 4) + r][pixel = m0 + 16 MT wave + 16 m + (lane & 15)]
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const long long pm = m0 + wave * 16 * MT + 16 * m + (lane & 15);
        if (pm >= a.M) continue;
#pragma unroll
        for (int f = 0; f < NT; ++f) {
            const int co = nt * 16 * NT + 16 * f + 4 * (lane >> 4);
            if (co >= a.Cout) continue;
            const f32x4 b = *reinterpret_cast<const f32x4*>(a.bias + co);
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = acc[m][f][r] + b[r];
                if (a.relu) v[r] = v[r] > 0.f ? v[r] : 0.f;
            }
            if (a.dst_nchw) {  // the image gradient: Cout = 3, fp32
                float* y = reinterpret_cast<float*>(a.y);
                const long long n = pm / hw;
                const int rem = (int)(pm - n * hw);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (co + r < a.Cout) y[(n * a.Cout + co + r) * (long long)hw + rem] = v[r];
            } else {
                const long long off = pm * a.Cout + co;
                if (a.mask) {
                    const h16x4 mk = *reinterpret_cast<const h16x4*>(a.mask + off);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = mk[r] > (h16)0.f ? v[r] : 0.f;
                }
                const T4 o = {(T)v[0], (T)v[1], (T)v[2], (T)v[3]};
                *reinterpret_cast<T4*>(reinterpret_cast<T*>(a.y) + off) = o;
            }
        }
    }
}

// ---- 2x2 / stride 2 max-pool on fp16, its backward on bf16 -----------------------------------------------------------------------
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

__global__ void style16_pool_fwd_kernel(const h16* __restrict__ x, h16* __restrict__ y, unsigned char* __restrict__ idx, int N, int H,
                                        int W, int C8) {
    const int Ho = H / 2, Wo = W / 2;
    const size_t total = (size_t)N * Ho * Wo * C8, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int q = e % C8;
        size_t r = e / C8;
        const int ox = r % Wo; r /= Wo;
        const int oy = r % Ho;
        const size_t n = r / Ho;
        const h16x8* src = reinterpret_cast<const h16x8*>(x) + ((n * H + 2 * oy) * W + 2 * ox) * C8 + q;
        const h16x8 v0 = src[0], v1 = src[C8], v2 = src[(size_t)W * C8], v3 = src[(size_t)W * C8 + C8];
        h16x8 m;
        unsigned long long code = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {  // first maximum in row-major window order; a NaN wins (mstg_maxpool2x2_fwd)
            float best = (float)v0[k];
            unsigned long long bi = 0;
            const float f1 = (float)v1[k], f2 = (float)v2[k], f3 = (float)v3[k];
            if (f1 > best || f1 != f1) { best = f1; bi = 1; }
            if (f2 > best || f2 != f2) { best = f2; bi = 2; }
            if (f3 > best || f3 != f3) { best = f3; bi = 3; }
            m[k] = bi == 0 ? v0[k] : (bi == 1 ? v1[k] : (bi == 2 ? v2[k] : v3[k]));
            code |= bi << (8 * k);
        }
        reinterpret_cast<h16x8*>(y)[e] = m;
        reinterpret_cast<unsigned long long*>(idx)[e] = code;
    }
}

__global__ void style16_pool_bwd_kernel(const u16x8* __restrict__ dy, const unsigned char* __restrict__ idx, const h16* __restrict__ mask,
                                        u16x8* __restrict__ dx, int N, int H, int W, int C8) {
    const int Ho = H / 2, Wo = W / 2;
    const size_t total = (size_t)N * Ho * Wo * C8, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int q = e % C8;
        size_t r = e / C8;
        const int ox = r % Wo; r /= Wo;
        const int oy = r % Ho;
        const size_t n = r / Ho;
        const u16x8 g = dy[e];
        const unsigned long long code = reinterpret_cast<const unsigned long long*>(idx)[e];
        const size_t base = ((n * H + 2 * oy) * W + 2 * ox) * C8 + q;
        const size_t offs[4] = {base, base + C8, base + (size_t)W * C8, base + (size_t)W * C8 + C8};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            u16x8 o;
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = ((code >> (8 * k)) & 255ull) == (unsigned long long)s ? g[k] : (unsigned short)0;
            if (mask) {
                const h16x8 mk = reinterpret_cast<const h16x8*>(mask)[offs[s]];
#pragma unroll
                for (int k = 0; k < 8; ++k) o[k] = mk[k] > (h16)0.f ? o[k] : (unsigned short)0;
            }
            dx[offs[s]] = o;
        }
    }
}

// ---- Gram forward: partial[n][split][c1][c2] = sum over the split's pixels of F[p][c1] * F[p][c2] --------------------------------
// workgroup = (64 x 64 tile of G, pixel split, image); wave w owns rows c1 + 16 w .. + 15 and all four 16-column fragments, so no
// sum crosses waves.  The MFMA's K index is the pixel, so both operands are staged TRANSPOSED, [channel][64 pixels] as rows of
// 128 + 16 bytes: a thread loads 8 channels of two neighbouring pixels and writes 8 dwords (one pixel pair of one channel each),
// conflict-free; a fragment is then 16 bytes of one channel row.
constexpr int GF_P = 64;
constexpr int GF_ROW = 144;
__global__ __launch_bounds__(256) void style16_gram_fwd_kernel(const h16* __restrict__ f, float* __restrict__ partial, int HW, int C,
                                                               int S, int pps) {
    __shared__ __attribute__((aligned(16))) unsigned char At[64 * GF_ROW];
    __shared__ __attribute__((aligned(16))) unsigned char Bt[64 * GF_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
    const int ntc = (C + 63) / 64;
    const int c1 = (blockIdx.x % ntc) * 64, c2 = (blockIdx.x / ntc) * 64;
    const int sp = blockIdx.y, n = blockIdx.z;
    const int p0 = sp * pps, p1 = min(HW, p0 + pps);
    const h16* fn = f + (size_t)n * HW * C;
    const int pp = tid & 31, cq = tid >> 5;  // pixel pair, 8-channel group
    f32x4 acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    uint4 ra[2], rb[2];
    auto load_stage = [&](int pt) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int p = pt + 2 * pp + t;
            const bool oka = p < p1 && c1 + 8 * cq < C, okb = p < p1 && c2 + 8 * cq < C;
            const uint4 va = *reinterpret_cast<const uint4*>(fn + (oka ? (size_t)p * C + c1 + 8 * cq : (size_t)0));
            const uint4 vb = *reinterpret_cast<const uint4*>(fn + (okb ? (size_t)p * C + c2 + 8 * cq : (size_t)0));
            ra[t] = oka ? va : uint4{0, 0, 0, 0};
            rb[t] = okb ? vb : uint4{0, 0, 0, 0};
        }
    };
    auto store_stage = [&]() {
        const unsigned short* a0 = reinterpret_cast<const unsigned short*>(&ra[0]);
        const unsigned short* a1 = reinterpret_cast<const unsigned short*>(&ra[1]);
        const unsigned short* b0 = reinterpret_cast<const unsigned short*>(&rb[0]);
        const unsigned short* b1 = reinterpret_cast<const unsigned short*>(&rb[1]);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            *reinterpret_cast<unsigned*>(&At[(8 * cq + j) * GF_ROW + 4 * pp]) = (unsigned)a0[j] | ((unsigned)a1[j] << 16);
            *reinterpret_cast<unsigned*>(&Bt[(8 * cq + j) * GF_ROW + 4 * pp]) = (unsigned)b0[j] | ((unsigned)b1[j] << 16);
        }
    };
    if (p0 < p1) load_stage(p0);
    for (int pt = p0; pt < p1; pt += GF_P) {
        __syncthreads();  // the fragments of the stage before have been read
        store_stage();
        __syncthreads();
        if (pt + GF_P < p1) load_stage(pt + GF_P);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const h16x8 af = *reinterpret_cast<const h16x8*>(&At[(16 * wave + i) * GF_ROW + 64 * s + 16 * g]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const h16x8 bf = *reinterpret_cast<const h16x8*>(&Bt[(16 * k + i) * GF_ROW + 64 * s + 16 * g]);
                acc[k] = mfma16x16x32_f16(af, bf, acc[k]);
            }
        }
    }
    float* out = partial + ((size_t)n * S + sp) * C * C;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = c1 + 16 * wave + 4 * g + e, c = c2 + 16 * k + i;
            if (r < C && c < C) out[(size_t)r * C + c] = acc[k][e];
        }
}

// G[n][e] = scale * sum_s partial[n][s][e], s in order
__global__ void style16_gram_reduce_kernel(const float* __restrict__ partial, float* __restrict__ gm, int S, int CC, float scale) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
    if (e >= CC) return;
    float s = 0.f;
    for (int k = 0; k < S; ++k) s += partial[((size_t)n * S + k) * CC + e];
    gm[(size_t)n * CC + e] = s * scale;
}

// ---- Gram backward: dF[n][p][c] = [F > 0] (scale * sum_c2 (dG[n][c][c2] + dG[n][c2][c]) F[n][p][c2] + incoming) -------------------
// No fp16 intermediate.  S = dG + dG^T is written once as a bf16 head and tail, Sh = bf16(S), Sl = bf16(S - Sh); an fp16 F is the
// sum of two bf16 numbers EXACTLY (11 significant bits = 8 + at most 3 behind them, and bf16 reaches below fp16's subnormals):
// Fh = bf16(F), Fl = F - Fh.  The product is Sh Fh + Sh Fl + Sl Fh in fp32 (Sl Fl, 2^-16 relative, is dropped).  Every term scales
// exactly with a power of two on dG as long as nothing leaves the normal range of fp32 / bf16.
__global__ void style16_gram_sym_kernel(const float* __restrict__ dg, b16* __restrict__ sh, b16* __restrict__ sl, int C) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
    if (e >= C * C) return;
    const int r = e / C, c = e - r * C;
    const float* d = dg + (size_t)n * C * C;
    const float s = d[(size_t)r * C + c] + d[(size_t)c * C + r];
    const b16 hi = (b16)s;
    sh[(size_t)n * C * C + e] = hi;
    sl[(size_t)n * C * C + e] = (b16)(s - (float)hi);
}

// workgroup = 64 PT pixels x 64 output channels of one image; wave w owns PT fragments of 16 pixels.  S rows are the A operand (a
// lane's four accumulators are four consecutive channels of one pixel), F the B operand: both fragments are 16 contiguous bytes of
// a row in global memory (S is C x C per image, cache resident), so nothing is staged.  The S fragments of a K-step -- four
// channel fragments, head and tail, four times the bytes of one F fragment -- are loaded once and used for all PT pixel fragments.
// Every output's sum walks K in the same order for every PT.
template <int PT>
__global__ __launch_bounds__(256) void style16_gram_bwd_kernel(const h16* __restrict__ f, const b16* __restrict__ sh,
                                                               const b16* __restrict__ sl, const b16* __restrict__ incoming,
                                                               b16* __restrict__ df, int HW, int C, float scale) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
    const int n = blockIdx.z, co0 = blockIdx.y * 64;
    const long long p0 = (long long)blockIdx.x * (64 * PT) + wave * (16 * PT) + i;  // pixel of fragment t: p0 + 16 t
    const h16* fn = f + (size_t)n * HW * C;
    const b16* shn = sh + (size_t)n * C * C;
    const b16* sln = sl + (size_t)n * C * C;
    f32x4 acc[PT][4];
#pragma unroll
    for (int t = 0; t < PT; ++t)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[t][k] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < C; k0 += 32) {
        const int kc = k0 + 8 * g;
        const bool kok = kc < C;
        uint4 raw[PT];
#pragma unroll
        for (int t = 0; t < PT; ++t) {
            const long long p = p0 + 16 * t;
            const bool fok = kok && p < HW;
            const uint4 v = *reinterpret_cast<const uint4*>(fn + (fok ? (size_t)p * C + kc : (size_t)0));
            raw[t] = fok ? v : uint4{0, 0, 0, 0};
        }
        b16x8 ah[4], al[4];
#pragma unroll
        for (int mf = 0; mf < 4; ++mf) {
            const int c = co0 + 16 * mf + i;
            const bool ok = kok && c < C;
            const size_t off = ok ? (size_t)c * C + kc : (size_t)0;
            const uint4 h = *reinterpret_cast<const uint4*>(shn + off), l = *reinterpret_cast<const uint4*>(sln + off);
            const uint4 hz = ok ? h : uint4{0, 0, 0, 0}, lz = ok ? l : uint4{0, 0, 0, 0};
            ah[mf] = *reinterpret_cast<const b16x8*>(&hz);
            al[mf] = *reinterpret_cast<const b16x8*>(&lz);
        }
#pragma unroll
        for (int t = 0; t < PT; ++t) {
            const h16x8 fv = *reinterpret_cast<const h16x8*>(&raw[t]);
            b16x8 fh, fl;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = (float)fv[j];
                fh[j] = (b16)v;
                fl[j] = (b16)(v - (float)fh[j]);
            }
#pragma unroll
            for (int mf = 0; mf < 4; ++mf) {
                acc[t][mf] = mfma16x16x32_bf16(ah[mf], fh, acc[t][mf]);
                acc[t][mf] = mfma16x16x32_bf16(ah[mf], fl, acc[t][mf]);
                acc[t][mf] = mfma16x16x32_bf16(al[mf], fh, acc[t][mf]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < PT; ++t) {
        const long long p = p0 + 16 * t;
        if (p >= HW) continue;
#pragma unroll
        for (int mf = 0; mf < 4; ++mf) {
            const int c = co0 + 16 * mf + 4 * g;
            if (c >= C) continue;
            const size_t off = ((size_t)n * HW + p) * C + c;
            const h16x4 fm = *reinterpret_cast<const h16x4*>(f + off);
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = acc[t][mf][r] * scale;
            if (incoming) {
                const b16x4 in = *reinterpret_cast<const b16x4*>(incoming + off);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += (float)in[r];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = fm[r] > (h16)0.f ? v[r] : 0.f;
            const b16x4 o = {(b16)v[0], (b16)v[1], (b16)v[2], (b16)v[3]};
            *reinterpret_cast<b16x4*>(df + off) = o;
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
static const char* sconv_validate(const mstg_style16_conv_desc* d) {
    if (!d) return "mstg_style16_conv: null descriptor";
    if (d->dtype != MSTG_STYLE16_F16 && d->dtype != MSTG_STYLE16_BF16) return "mstg_style16_conv: dtype must be MSTG_STYLE16_F16 or MSTG_STYLE16_BF16";
    if (d->src_nchw_f32 && d->dst_nchw_f32) return "mstg_style16_conv: the fp32 stem and the fp32 image gradient are different layers";
    if (d->src_nchw_f32) {
        if (d->Cin != 3) return "mstg_style16_conv: the fp32 NCHW source is the 3-channel stem (Cin must be 3)";
    } else if (d->Cin < 16 || d->Cin % 16 || d->Cin > SC_MAXC) {
        return "mstg_style16_conv: Cin must be a multiple of 16 up to 512 (or the 3-channel fp32 stem)";
    }
    if (d->dst_nchw_f32) {
        if (d->Cout != 3) return "mstg_style16_conv: the fp32 NCHW destination is the 3-channel image gradient (Cout must be 3)";
    } else if (d->Cout < 16 || d->Cout % 16 || d->Cout > SC_MAXC) {
        return "mstg_style16_conv: Cout must be a multiple of 16 up to 512 (or the 3-channel fp32 image gradient)";
    }
    return nullptr;
}

static size_t sconv_filter_elems(const mstg_style16_conv_desc* d) { return (size_t)sconv_coutp(d->Cout) * sconv_nchunks(d) * SC_BK; }

// The tile shape of a launch: 16 NT output channels per block by the layer's width; 128-pixel tiles when they still give every CU
// two blocks, else 64-pixel tiles.  The k order of every sum is the same in all variants.
struct SConvRoute {
    int MT, NT;
    bool stem;
    long long blocks;
};
static bool sconv_route(const mstg_style16_conv_desc* d, SConvRoute* r) {
    if (sconv_validate(d) || d->N < 1 || d->H < 1 || d->W < 1) return false;
    const long long M = (long long)d->N * d->H * d->W;
    r->NT = sconv_nt(d->Cout);
    const long long ntn = sconv_coutp(d->Cout) / (16 * r->NT);
    r->MT = (M + 127) / 128 * ntn >= 512 ? 2 : 1;
    r->stem = d->src_nchw_f32 != 0;
    r->blocks = (M + 64 * r->MT - 1) / (64 * r->MT) * ntn;
    return true;
}

template <typename T, int MT, int NT, bool STEM>
static int sconv_launch1(const SConvArgs& a, unsigned grid, hipStream_t st) {
    constexpr int lds = sconv_lds_bytes(MT, NT);
    static_assert(lds <= 64 * 1024, "the default dynamic LDS limit");
    MSTG_LAUNCH((style_conv16_kernel<T, MT, NT, STEM>), dim3(grid), dim3(256), lds, st, a);
    return MSTG_OK;
}
template <typename T, int NT>
static int sconv_launch_nt(const SConvArgs& a, const SConvRoute& r, hipStream_t st) {
    const unsigned grid = (unsigned)r.blocks;
    if (r.stem) return r.MT == 2 ? sconv_launch1<T, 2, NT, true>(a, grid, st) : sconv_launch1<T, 1, NT, true>(a, grid, st);
    return r.MT == 2 ? sconv_launch1<T, 2, NT, false>(a, grid, st) : sconv_launch1<T, 1, NT, false>(a, grid, st);
}
template <typename T>
static int sconv_launch(const SConvArgs& a, const SConvRoute& r, hipStream_t st) {
    return r.NT == 4 ? sconv_launch_nt<T, 4>(a, r, st) : r.NT == 2 ? sconv_launch_nt<T, 2>(a, r, st) : sconv_launch_nt<T, 1>(a, r, st);
}

static int s16_gram_splits(int HW) {
    const int s = HW / 4096;
    return s < 1 ? 1 : (s > 16 ? 16 : s);
}

}  // namespace mstg

using namespace mstg;

extern "C" size_t mstg_style16_conv_plan_bytes(const mstg_style16_conv_desc* d) {
    if (const char* e = sconv_validate(d)) {
        fail_arg(MSTG_E_UNSUPPORTED, e);
        return 0;
    }
    return (size_t)sconv_coutp(d->Cout) * 4 + sconv_filter_elems(d) * 2;
}

extern "C" const char* mstg_style16_conv_kernel_name(const mstg_style16_conv_desc* d) {
    static thread_local char name[64];
    SConvRoute r;
    if (!sconv_route(d, &r)) {
        const char* e = sconv_validate(d);
        fail_arg(e ? MSTG_E_UNSUPPORTED : MSTG_E_BADARG, e ? e : "mstg_style16_conv: N, H, W must be positive");
        return nullptr;
    }
    snprintf(name, sizeof(name), "style_conv16_kernel<%s,%d,%d,%d>", d->dtype == MSTG_STYLE16_BF16 ? "bf16" : "f16", r.MT, r.NT, (int)r.stem);
    return name;
}

extern "C" int mstg_style16_conv_pack(const mstg_style16_conv_desc* d, const float* w, const float* bias, void* blob, size_t blob_bytes,
                                      void* stream) {
    if (const char* e = sconv_validate(d)) return fail_arg(MSTG_E_UNSUPPORTED, e);
    if (!w || !blob) return fail_arg(MSTG_E_BADARG, "mstg_style16_conv_pack: null pointer");
    if (blob_bytes < mstg_style16_conv_plan_bytes(d)) return fail_arg(MSTG_E_BADARG, "mstg_style16_conv_pack: blob smaller than mstg_style16_conv_plan_bytes");
    const int CoutP = sconv_coutp(d->Cout), NT = sconv_nt(d->Cout);
    float* bbias = reinterpret_cast<float*>(blob);
    void* out = bbias + CoutP;
    const long long total = (long long)sconv_filter_elems(d);
    const unsigned grid = (unsigned)((total + 255) / 256);
    if (d->dtype == MSTG_STYLE16_BF16)
        MSTG_LAUNCH(style_conv16_pack_kernel<b16>, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, bias, bbias, (b16*)out, d->flip, d->Cin,
                    d->Cout, CoutP, sconv_cinp(d), NT, sconv_nchunks(d), total);
    else
        MSTG_LAUNCH(style_conv16_pack_kernel<h16>, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, bias, bbias, (h16*)out, d->flip, d->Cin,
                    d->Cout, CoutP, sconv_cinp(d), NT, sconv_nchunks(d), total);
    MSTG_CHECK_LAUNCH("mstg_style16_conv_pack");
    return MSTG_OK;
}

extern "C" int mstg_style16_conv_fwd(const mstg_style16_conv_desc* d, const void* blob, const void* x, const void* mask, void* y,
                                     void* stream) {
    if (const char* e = sconv_validate(d)) return fail_arg(MSTG_E_UNSUPPORTED, e);
    if (!blob || !x || !y) return fail_arg(MSTG_E_BADARG, "mstg_style16_conv_fwd: null pointer");
    if (d->N < 1 || d->H < 1 || d->W < 1) return fail_arg(MSTG_E_BADARG, "mstg_style16_conv_fwd: N, H, W must be positive");
    if ((long long)d->H * d->W >= (1ll << 30)) return fail_arg(MSTG_E_BADARG, "mstg_style16_conv_fwd: image too large");
    if (mask && d->dst_nchw_f32) return fail_arg(MSTG_E_BADARG, "mstg_style16_conv_fwd: the fp32 image gradient takes no ReLU mask");
    SConvRoute r;
    if (!sconv_route(d, &r)) return fail_arg(MSTG_E_BADARG, "mstg_style16_conv_fwd: no route");
    if (r.blocks >= (1ll << 31)) return fail_arg(MSTG_E_BADARG, "mstg_style16_conv_fwd: too many tiles");
    const int CoutP = sconv_coutp(d->Cout);
    SConvArgs a;
    a.x = x;
    a.y = y;
    a.mask = reinterpret_cast<const h16*>(mask);
    a.bias = reinterpret_cast<const float*>(blob);
    a.wpk = reinterpret_cast<const unsigned char*>(a.bias + CoutP);
    a.M = (long long)d->N * d->H * d->W;
    a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Cout = d->Cout;
    a.relu = d->relu; a.dst_nchw = d->dst_nchw_f32;
    a.nchunks = sconv_nchunks(d);
    a.ntn = CoutP / (16 * r.NT);
    a.cg = d->src_nchw_f32 ? 1 : d->Cin / 8;
    a.kgroups = 9 * sconv_cinp(d) / 8;
    a.cg_magic = ((1 << 20) + a.cg - 1) / a.cg;
    const int rc = d->dtype == MSTG_STYLE16_BF16 ? sconv_launch<b16>(a, r, (hipStream_t)stream) : sconv_launch<h16>(a, r, (hipStream_t)stream);
    if (rc != MSTG_OK) return rc;
    MSTG_CHECK_LAUNCH("mstg_style16_conv_fwd");
    return MSTG_OK;
}

static int pool16_check(const char* who, const void* a, const void* b, const void* c, int N, int H, int W, int C) {
    static thread_local char msg[128];
    const char* what = nullptr;
    int code = MSTG_E_BADARG;
    if (!a || !b || !c) what = "null pointer";
    else if (N <= 0 || H < 2 || W < 2 || (H & 1) || (W & 1) || C <= 0) what = "H and W must be even and >= 2";
    else if (C & 7) { what = "C must be a multiple of 8"; code = MSTG_E_ALIGN; }
    if (!what) return MSTG_OK;
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return fail_arg(code, msg);
}

extern "C" int mstg_style16_maxpool_fwd(const void* x, void* y, unsigned char* idx, int N, int H, int W, int C, void* stream) {
    if (const int rc = pool16_check("mstg_style16_maxpool_fwd", x, y, idx, N, H, W, C)) return rc;
    const size_t total = (size_t)N * (H / 2) * (W / 2) * (C / 8);
    const int nb = (int)(cdivz(total, 256) > 8192 ? 8192 : cdivz(total, 256));
    MSTG_LAUNCH(style16_pool_fwd_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const h16*)x, (h16*)y, idx, N, H, W, C / 8);
    MSTG_CHECK_LAUNCH("style16_pool_fwd_kernel");
    return MSTG_OK;
}

extern "C" int mstg_style16_maxpool_bwd(const void* dy, const unsigned char* idx, const void* mask, void* dx, int N, int H, int W, int C,
                                        void* stream) {
    if (const int rc = pool16_check("mstg_style16_maxpool_bwd", dy, dx, idx, N, H, W, C)) return rc;
    const size_t total = (size_t)N * (H / 2) * (W / 2) * (C / 8);
    const int nb = (int)(cdivz(total, 256) > 8192 ? 8192 : cdivz(total, 256));
    MSTG_LAUNCH(style16_pool_bwd_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const u16x8*)dy, idx, (const h16*)mask, (u16x8*)dx, N,
                H, W, C / 8);
    MSTG_CHECK_LAUNCH("style16_pool_bwd_kernel");
    return MSTG_OK;
}

static const char* gram16_validate(int N, long long HW, int C) {
    if (N <= 0 || HW <= 0 || C <= 0) return "mstg_style16_gram: empty tensor";
    if (C % 16 || C > SC_MAXC) return "mstg_style16_gram: C must be a multiple of 16 up to 512";
    if (HW >= (1ll << 30)) return "mstg_style16_gram: image too large";
    return nullptr;
}

extern "C" size_t mstg_style16_gram_workspace_bytes(int N, int HW, int C) {
    if (const char* e = gram16_validate(N, HW, C)) {
        fail_arg(MSTG_E_UNSUPPORTED, e);
        return 0;
    }
    return (size_t)N * s16_gram_splits(HW) * C * C * sizeof(float);
}

extern "C" int mstg_style16_gram_fwd(const void* f, float* g, int N, int HW, int C, float scale, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    if (const char* e = gram16_validate(N, HW, C)) return fail_arg(MSTG_E_UNSUPPORTED, e);
    if (!f || !g || !workspace) return fail_arg(MSTG_E_BADARG, "mstg_style16_gram_fwd: null pointer");
    if (workspace_bytes < mstg_style16_gram_workspace_bytes(N, HW, C)) return fail_arg(MSTG_E_WORKSPACE, "mstg_style16_gram_fwd: workspace too small");
    const int S = s16_gram_splits(HW);
    const int pps = cdiv(cdiv(HW, S), GF_P) * GF_P;
    const int ntc = cdiv(C, 64);
    hipStream_t st = (hipStream_t)stream;
    MSTG_LAUNCH(style16_gram_fwd_kernel, dim3(ntc * ntc, S, N), dim3(256), 0, st, (const h16*)f, (float*)workspace, HW, C, S, pps);
    MSTG_CHECK_LAUNCH("style16_gram_fwd_kernel");
    MSTG_LAUNCH(style16_gram_reduce_kernel, dim3(cdiv(C * C, 256), N), dim3(256), 0, st, (const float*)workspace, g, S, C * C, scale);
    MSTG_CHECK_LAUNCH("style16_gram_reduce_kernel");
    return MSTG_OK;
}

extern "C" size_t mstg_style16_gram_bwd_workspace_bytes(int N, int C) {
    if (const char* e = gram16_validate(N, 1, C)) {
        fail_arg(MSTG_E_UNSUPPORTED, e);
        return 0;
    }
    return (size_t)N * C * C * 2 * 2;  // Sh | Sl, bf16
}

extern "C" int mstg_style16_gram_bwd(const void* f, const float* dg, const void* incoming, void* df, int N, int HW, int C, float scale,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    if (const char* e = gram16_validate(N, HW, C)) return fail_arg(MSTG_E_UNSUPPORTED, e);
    if (!f || !dg || !df || !workspace) return fail_arg(MSTG_E_BADARG, "mstg_style16_gram_bwd: null pointer");
    if (workspace_bytes < mstg_style16_gram_bwd_workspace_bytes(N, C)) return fail_arg(MSTG_E_WORKSPACE, "mstg_style16_gram_bwd: workspace too small");
    b16* sh = reinterpret_cast<b16*>(workspace);
    b16* sl = sh + (size_t)N * C * C;
    hipStream_t st = (hipStream_t)stream;
    MSTG_LAUNCH(style16_gram_sym_kernel, dim3(cdiv(C * C, 256), N), dim3(256), 0, st, dg, sh, sl, C);
    MSTG_CHECK_LAUNCH("style16_gram_sym_kernel");
    // 256 pixels per block (the S fragments of a K-step serve four pixel fragments) when that still gives 512 blocks, else 64
    if ((long long)cdiv(HW, 256) * cdiv(C, 64) * N >= 512)
        MSTG_LAUNCH(style16_gram_bwd_kernel<4>, dim3(cdiv(HW, 256), cdiv(C, 64), N), dim3(256), 0, st, (const h16*)f, (const b16*)sh,
                    (const b16*)sl, (const b16*)incoming, (b16*)df, HW, C, scale);
    else
        MSTG_LAUNCH(style16_gram_bwd_kernel<1>, dim3(cdiv(HW, 64), cdiv(C, 64), N), dim3(256), 0, st, (const h16*)f, (const b16*)sh,
                    (const b16*)sl, (const b16*)incoming, (b16*)df, HW, C, scale);
    MSTG_CHECK_LAUNCH("style16_gram_bwd_kernel");
    return MSTG_OK;
}
