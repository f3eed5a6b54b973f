// fp16 inference of StructuralTransformerBlock (structural_transformer.py:55-74; CPU restatement
// oracle/restatement.py::structural_transformer_block): fp16 storage and MFMA operands, fp32 accumulation, statistics and softmax
// (mstg_f16_linear_*, mstg_f16_ln_mod_fwd, mstg_f16_token_mean, mstg_f16_flash_attn_fwd; include/mstg_hip.h).
//
//   token GEMM      the block's nn.Linear layers over N * L tokens (qkv :69, proj :71, fc1 :73, fc2 :74) on
//                   v_mfma_f32_16x16x32_f16; epilogues none / exact-erf GELU / + fp32 residual
//   ln_mod          u = LayerNorm(h) * (1 + g) + b in fp32, fp16 out (:68, :72), optionally h = x + struct_proj(s) first (:65)
//   token mean      AdaptiveAvgPool2d(1) of the fp16 tokens for the style vector (enhanced_generator.py:144-146)
//   flash attention softmax(q k^T / sqrt(D)) v over all L tokens of an image (:70), fp16 operands, fp32 online softmax
//
// Every sum runs in a fixed order that does not depend on the batch: image i of a batch equals the same image run alone.
#include "lanes.h"

namespace mstg {

// ---- token GEMM (nn.Linear over tokens) --------------------------------------------------------------------------------------
// y[t][co] = epi(sum_k x[t][k] W[co][k] + b[co]).  A = the filter (rows = output channels), B = the tokens (columns), so that a
// lane's four accumulator registers are four consecutive output channels of one token.  A wave owns 16 tokens: it loads their
// whole rows once (Cin / 32 fragments) and walks every output channel, reading the filter from L2 (<= 256 KB, shared by all).
// blob: bias fp32 [Cout] | W fp16 [Cout][Cin] (row-major, nn.Linear's layout).
struct LinArgs {
    const h16* x;
    const h16* w;
    const float* bias;
    const float* res;  // fp32 [T][Cout] or null
    void* y;           // fp16 or fp32 [T][Cout]
    long long T;
    int Cout, act, out_f16;
};

__global__ void blk_linear_pack_kernel(const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ bias,
                                       h16* __restrict__ wh, int Cout, long long total) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < Cout) bias[e] = b ? b[e] : 0.f;
    if (e < total) wh[e] = (h16)w[e];
}

template <int KS>  // Cin = 32 KS
__global__ __launch_bounds__(256) void blk_linear_f16_kernel(LinArgs a) {
    constexpr int CIN = 32 * KS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    const long long tok = ((long long)blockIdx.x * 4 + wave) * 16 + i;
    const bool tv = tok < a.T;
    h16x8 xf[KS];
    const h16* xp = a.x + (tv ? tok : 0ll) * CIN + 8 * g;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const h16x8 v = *reinterpret_cast<const h16x8*>(xp + 32 * ks);
        xf[ks] = tv ? v : h16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    const int nf = a.Cout >> 4;  // a multiple of 4
    for (int f0 = 0; f0 < nf; f0 += 4) {
        f32x4 acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const h16x8 wf = *reinterpret_cast<const h16x8*>(a.w + (size_t)(16 * (f0 + u) + i) * CIN + 32 * ks + 8 * g);
                acc[u] = mfma16x16x32_f16(wf, xf[ks], acc[u]);
            }
        if (!tv) continue;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int co = 16 * (f0 + u) + 4 * g;
            const f32x4 bb = *reinterpret_cast<const f32x4*>(a.bias + co);
            f32x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = apply_act(acc[u][r] + bb[r], a.act);
            const long long off = tok * a.Cout + co;
            if (a.res) v = *reinterpret_cast<const f32x4*>(a.res + off) + v;
            if (a.out_f16) {
                const h16x4 o = {(h16)v[0], (h16)v[1], (h16)v[2], (h16)v[3]};
                *reinterpret_cast<h16x4*>(reinterpret_cast<h16*>(a.y) + off) = o;
            } else {
                *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.y) + off) = v;
            }
        }
    }
}

// ---- LayerNorm + style modulation -----------------------------------------------------------------------------------------
// A group of 16 lanes owns a token; lane j holds channels 64c + 4j.  With smap: h = x + (b_sp + W_sp s) (Linear(4 -> dim), :65),
// written to h_out when given.  u = (LN(h) * gamma + beta) * (1 + g[n]) + b[n], gb = (N, 2 dim) = style_mod's output (g | b).
constexpr int BLN_MAXC = 4;
template <bool XF16>
__global__ __launch_bounds__(256) void blk_ln_mod_f16_kernel(const void* __restrict__ xv, const float* __restrict__ smap,
                                                             const float* __restrict__ spw, const float* __restrict__ spb,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ gb, float* __restrict__ h_out,
                                                             h16* __restrict__ u, long long T, int L, int dim, float eps) {
    const int j = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const long long tok = (long long)blockIdx.x * 16 + grp;
    if (tok >= T) return;
    const long long n = tok / L;
    const int nc = dim >> 6;
    f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
    if (smap) s4 = *reinterpret_cast<const f32x4*>(smap + tok * 4);
    f32x4 v[BLN_MAXC];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < BLN_MAXC; ++c) {
        v[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < nc) {
            const int ch = 64 * c + 4 * j;
            if constexpr (XF16) {
                const h16x4 x4 = *reinterpret_cast<const h16x4*>(reinterpret_cast<const h16*>(xv) + tok * dim + ch);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[c][e] = (float)x4[e];
            } else {
                v[c] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(xv) + tok * dim + ch);
            }
            if (smap) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const f32x4 w4 = *reinterpret_cast<const f32x4*>(spw + (size_t)(ch + e) * 4);
                    float lin = spb[ch + e];
#pragma unroll
                    for (int k = 0; k < 4; ++k) lin = fmaf(w4[k], s4[k], lin);
                    v[c][e] += lin;
                }
                if (h_out) *reinterpret_cast<f32x4*>(h_out + tok * dim + ch) = v[c];
            }
            s += v[c][0] + v[c][1] + v[c][2] + v[c][3];
        }
    }
    const float mean = row16_sum(s) / (float)dim;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < BLN_MAXC; ++c)
        if (c < nc)
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float d = v[c][e] - mean; q += d * d; }
    const float rstd = rsqrtf(row16_sum(q) / (float)dim + eps);
#pragma unroll
    for (int c = 0; c < BLN_MAXC; ++c) {
        if (c >= nc) continue;
        const int ch = 64 * c + 4 * j;
        const f32x4 ga = *reinterpret_cast<const f32x4*>(gamma + ch), be = *reinterpret_cast<const f32x4*>(beta + ch);
        f32x4 gm = {0.f, 0.f, 0.f, 0.f}, bm = {0.f, 0.f, 0.f, 0.f};
        if (gb) {
            gm = *reinterpret_cast<const f32x4*>(gb + n * 2 * dim + ch);
            bm = *reinterpret_cast<const f32x4*>(gb + n * 2 * dim + dim + ch);
        }
        h16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (h16)(((v[c][e] - mean) * rstd * ga[e] + be[e]) * (1.f + gm[e]) + bm[e]);
        *reinterpret_cast<h16x4*>(u + tok * dim + ch) = o;
    }
}

// ---- token mean ------------------------------------------------------------------------------------------------------------
// Workgroup (chunk ck, image n): thread (c = t % dim, part p = t / dim) sums tokens p, p + parts, ... of the chunk in order; the
// parts are added in order 0, 1, ...; the reduce kernel adds the chunks in order and divides by L.
static int tmean_chunks(int L, int* chunk) {
    int nchunk = cdiv(L, 256);
    if (nchunk > 64) nchunk = 64;
    *chunk = cdiv(L, nchunk);
    return cdiv(L, *chunk);
}

__global__ __launch_bounds__(256) void blk_token_mean_partial_kernel(const h16* __restrict__ x, float* __restrict__ part, int L,
                                                                     int dim, int chunk, int nchunk) {
    __shared__ float red[256];
    const int t = threadIdx.x, n = blockIdx.y, ck = blockIdx.x;
    const int parts = 256 / dim, c = t % dim, p = t / dim;
    const int t0 = ck * chunk, t1 = min(L, t0 + chunk);
    float acc = 0.f;
    if (p < parts)
        for (int k = t0 + p; k < t1; k += parts) acc += (float)x[((long long)n * L + k) * dim + c];
    red[t] = acc;
    __syncthreads();
    if (t < dim) {
        float s = 0.f;
        for (int q = 0; q < parts; ++q) s += red[q * dim + t];
        part[((size_t)n * nchunk + ck) * dim + t] = s;
    }
}

__global__ void blk_token_mean_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, int L, int dim, int nchunk) {
    const int c = threadIdx.x, n = blockIdx.x;
    if (c >= dim) return;
    float s = 0.f;
    for (int k = 0; k < nchunk; ++k) s += part[((size_t)n * nchunk + k) * dim + c];
    out[(size_t)n * dim + c] = s / (float)L;
}

// ---- flash attention, fp16 -------------------------------------------------------------------------------------------------
// qkv (N, L, 3 heads D) fp16 token-major, q | k | v blocks, head h = channels [h D, (h + 1) D); out (N, L, heads D) fp16.
// Workgroup = 64 queries of one (image, head), 16 per wave; key tiles of 64 staged in LDS (K row-major, V transposed), shared by
// the four waves, the next tile's global loads in flight under the current tile's arithmetic.
// Per tile and wave:
//   S^T = K Q^T: four 16-key blocks, keys on the accumulator rows (key 16c + 4g + r in register r of lane group g = lane >> 4),
//   the lane's query on the column.  So the tile's scores of a query sit in the 16 registers of the four lanes i, i + 16, i + 32,
//   i + 48: the row maximum is a local max and two permlane swaps.
//   p = exp2(s * c - m * c), c = log2(e) / sqrt(D), fp32 (the argument s - m is formed in fp32 by the fma), rounded to fp16 ONCE.
//   O^T += V^T P^T on 16x16x32: k-slot 8g + j of lane group g holds keys 4g + j (block 2kb) and 16 + 4g + j - 4 (block 2kb + 1),
//   exactly the registers of the two S^T blocks, so P goes from the accumulator to the next MFMA's operand without LDS; V^T is read
//   in the same key order.
//   The rescale of O and l by exp2((m_old - m_new) c) runs on every tile (no deferred rescale).
constexpr int BF_TQ = 64, BF_TK = 64;

template <int D>
struct BfCfg {
    static constexpr int KST = D + 8;       // halves per staged key row (16-byte pieces; conflict-free fragment reads)
    static constexpr int VST = BF_TK + 8;   // halves per staged channel row of V^T
    static constexpr int NDF = D / 16;      // 16-channel output fragments
    static constexpr int NQ = D >= 32 ? D / 32 : 1;  // K-steps of S^T (one 16x16x16 at D = 16)
    static constexpr int KP = BF_TK * D / 8;         // 16-byte pieces of a K tile
    static constexpr int NKR = (KP + 255) / 256;     // ... per thread
    static constexpr int VP = BF_TK / 2 * D / 8;     // (key pair, 8 channels) pieces of a V tile: <= 256
};

template <int D>
__global__ __launch_bounds__(256) void blk_flash_f16_kernel(const h16* __restrict__ qkv, h16* __restrict__ out, int L, int heads,
                                                            float cexp) {
    typedef BfCfg<D> CF;
    __shared__ __attribute__((aligned(16))) h16 Ks[BF_TK * CF::KST];
    __shared__ __attribute__((aligned(16))) h16 Vt[D * CF::VST];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i = lane & 15, g = lane >> 4;
    const int h = blockIdx.y, dim = heads * D;
    const long long ld = 3ll * dim, img = (long long)blockIdx.z * L;
    const int qi = blockIdx.x * BF_TQ + 16 * wv + i;
    const bool qv = qi < L;

    // Q as the B operand: Q[qi][channels of k-slot]
    h16x8 qf8[CF::NQ];
    h16x4 qf4 = {0, 0, 0, 0};
    {
        const h16* qp = qkv + (img + (qv ? qi : 0)) * ld + h * D;
        if constexpr (D == 16) {
            const h16x4 t = *reinterpret_cast<const h16x4*>(qp + 4 * g);
            qf4 = qv ? t : h16x4{0, 0, 0, 0};
        } else {
#pragma unroll
            for (int s = 0; s < CF::NQ; ++s) {
                const h16x8 t = *reinterpret_cast<const h16x8*>(qp + 32 * s + 8 * g);
                qf8[s] = qv ? t : h16x8{0, 0, 0, 0, 0, 0, 0, 0};
            }
        }
    }

    uint4 kreg[CF::NKR], vreg0 = {0, 0, 0, 0}, vreg1 = {0, 0, 0, 0};
    auto load_tile = [&](int k0) {
#pragma unroll
        for (int r = 0; r < CF::NKR; ++r) {
            const int p = tid + 256 * r;
            const int kr = p / (D / 8), q = p - kr * (D / 8);
            const bool ok = p < CF::KP && k0 + kr < L;
            const uint4 v = *reinterpret_cast<const uint4*>(qkv + (ok ? (img + k0 + kr) * ld + dim + h * D + 8 * q : 0ll));
            kreg[r] = ok ? v : uint4{0, 0, 0, 0};
        }
        if (tid < CF::VP) {
            const int kp = tid & 31, q = tid >> 5;
            const int key = k0 + 2 * kp;
            const bool ok0 = key < L, ok1 = key + 1 < L;
            const uint4 a = *reinterpret_cast<const uint4*>(qkv + (ok0 ? (img + key) * ld + 2 * dim + h * D + 8 * q : 0ll));
            const uint4 b = *reinterpret_cast<const uint4*>(qkv + (ok1 ? (img + key + 1) * ld + 2 * dim + h * D + 8 * q : 0ll));
            vreg0 = ok0 ? a : uint4{0, 0, 0, 0};
            vreg1 = ok1 ? b : uint4{0, 0, 0, 0};
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int r = 0; r < CF::NKR; ++r) {
            const int p = tid + 256 * r;
            const int kr = p / (D / 8), q = p - kr * (D / 8);
            if (p < CF::KP) *reinterpret_cast<uint4*>(&Ks[kr * CF::KST + 8 * q]) = kreg[r];
        }
        if (tid < CF::VP) {
            const int kp = tid & 31, q = tid >> 5;
            const h16x8 a = __builtin_bit_cast(h16x8, vreg0), b = __builtin_bit_cast(h16x8, vreg1);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const h16x2 pr = {a[e], b[e]};
                *reinterpret_cast<h16x2*>(&Vt[(8 * q + e) * CF::VST + 2 * kp]) = pr;
            }
        }
    };

    f32x4 o[CF::NDF];
#pragma unroll
    for (int df = 0; df < CF::NDF; ++df) o[df] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, lsum = 0.f;

    load_tile(0);
    store_tile();
    __syncthreads();
    for (int k0 = 0; k0 < L; k0 += BF_TK) {
        const bool more = k0 + BF_TK < L;
        if (more) load_tile(k0 + BF_TK);
        f32x4 s[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            s[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            const h16* kp = &Ks[(16 * c + i) * CF::KST];
            if constexpr (D == 16) {
                s[c] = mfma16x16x16_f16(*reinterpret_cast<const h16x4*>(kp + 4 * g), qf4, s[c]);
            } else {
#pragma unroll
                for (int st = 0; st < CF::NQ; ++st) s[c] = mfma16x16x32_f16(*reinterpret_cast<const h16x8*>(kp + 32 * st + 8 * g), qf8[st], s[c]);
            }
        }
        if (k0 + BF_TK > L) {  // ragged last tile
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (k0 + 16 * c + 4 * g + r >= L) s[c][r] = -INFINITY;
        }
        float tmax = s[0][0];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) tmax = fmaxf(tmax, s[c][r]);
        tmax = col4_max(tmax);
        const float mnew = fmaxf(m, tmax);                       // finite: every tile holds a valid key
        const float alpha = __builtin_amdgcn_exp2f((m - mnew) * cexp);  // m = -inf on the first tile: 0
        lsum *= alpha;
#pragma unroll
        for (int df = 0; df < CF::NDF; ++df) o[df] *= alpha;
        m = mnew;
        const float mc = m * cexp;
        h16x4 ph[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(fmaf(s[c][r], cexp, -mc));
                lsum += p;
                ph[c][r] = (h16)p;
            }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const h16x8 pb = {ph[2 * kb][0], ph[2 * kb][1], ph[2 * kb][2], ph[2 * kb][3],
                               ph[2 * kb + 1][0], ph[2 * kb + 1][1], ph[2 * kb + 1][2], ph[2 * kb + 1][3]};
#pragma unroll
            for (int df = 0; df < CF::NDF; ++df) {
                const h16* vp = &Vt[(16 * df + i) * CF::VST + 32 * kb + 4 * g];
                const h16x4 lo = *reinterpret_cast<const h16x4*>(vp), hi = *reinterpret_cast<const h16x4*>(vp + 16);
                const h16x8 va = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                o[df] = mfma16x16x32_f16(va, pb, o[df]);
            }
        }
        __syncthreads();
        if (more) {
            store_tile();
            __syncthreads();
        }
    }
    lsum = col4_sum(lsum);
    if (qv) {
        const float inv = 1.f / lsum;
        h16* op = out + (img + qi) * dim + h * D;
#pragma unroll
        for (int df = 0; df < CF::NDF; ++df) {
            const h16x4 v = {(h16)(o[df][0] * inv), (h16)(o[df][1] * inv), (h16)(o[df][2] * inv), (h16)(o[df][3] * inv)};
            *reinterpret_cast<h16x4*>(op + 16 * df + 4 * g) = v;
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static const char* linear_validate(int Cin, int Cout) {
    if (Cin != 64 && Cin != 128 && Cin != 256 && Cin != 512) return "mstg_f16_linear: Cin must be 64, 128, 256 or 512";
    if (Cout < 64 || Cout > 768 || Cout % 64) return "mstg_f16_linear: Cout must be a multiple of 64 in 64..768";
    return nullptr;
}

template <int KS>
static void linear_launch(const LinArgs& a, unsigned grid, hipStream_t st) {
    MSTG_LAUNCH((blk_linear_f16_kernel<KS>), dim3(grid), dim3(256), 0, st, a);
}

template <int D>
static void flash_launch(const void* qkv, void* out, int N, int L, int heads, hipStream_t st) {
    const float cexp = 1.4426950408889634f / sqrtf((float)D);
    MSTG_LAUNCH((blk_flash_f16_kernel<D>), dim3(cdiv(L, BF_TQ), heads, N), dim3(256), 0, st, reinterpret_cast<const h16*>(qkv),
                reinterpret_cast<h16*>(out), L, heads, cexp);
}

}  // namespace mstg

using namespace mstg;

extern "C" size_t mstg_f16_linear_plan_bytes(int Cin, int Cout) {
    if (const char* e = linear_validate(Cin, Cout)) {
        fail_arg(MSTG_E_UNSUPPORTED, e);
        return 0;
    }
    return (size_t)Cout * 4 + (size_t)Cout * Cin * 2;
}

extern "C" int mstg_f16_linear_pack(const float* w, const float* b, int Cin, int Cout, void* blob, size_t blob_bytes, void* stream) {
    if (const char* e = linear_validate(Cin, Cout)) return fail_arg(MSTG_E_UNSUPPORTED, e);
    if (!w || !blob) return fail_arg(MSTG_E_BADARG, "mstg_f16_linear_pack: null pointer");
    if (blob_bytes < mstg_f16_linear_plan_bytes(Cin, Cout)) return fail_arg(MSTG_E_BADARG, "mstg_f16_linear_pack: blob smaller than mstg_f16_linear_plan_bytes");
    float* bias = reinterpret_cast<float*>(blob);
    h16* wh = reinterpret_cast<h16*>(bias + Cout);
    const long long total = (long long)Cout * Cin;
    MSTG_LAUNCH(blk_linear_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, b, bias, wh, Cout, total);
    MSTG_CHECK_LAUNCH("mstg_f16_linear_pack");
    return MSTG_OK;
}

extern "C" int mstg_f16_linear_fwd(const void* blob, const void* x, const float* residual, void* y, int N, int L, int Cin, int Cout,
                                   int act, int out_f16, void* stream) {
    if (const char* e = linear_validate(Cin, Cout)) return fail_arg(MSTG_E_UNSUPPORTED, e);
    if (!blob || !x || !y) return fail_arg(MSTG_E_BADARG, "mstg_f16_linear_fwd: null pointer");
    if (N < 1 || L < 1) return fail_arg(MSTG_E_BADARG, "mstg_f16_linear_fwd: N and L must be positive");
    if (act != MSTG_ACT_NONE && act != MSTG_ACT_GELU) return fail_arg(MSTG_E_UNSUPPORTED, "mstg_f16_linear_fwd: act must be none or GELU");
    const long long T = (long long)N * L;
    if ((T + 63) / 64 >= (1ll << 31)) return fail_arg(MSTG_E_BADARG, "mstg_f16_linear_fwd: too many tokens");
    LinArgs a;
    a.x = reinterpret_cast<const h16*>(x);
    a.bias = reinterpret_cast<const float*>(blob);
    a.w = reinterpret_cast<const h16*>(a.bias + Cout);
    a.res = residual;
    a.y = y;
    a.T = T;
    a.Cout = Cout;
    a.act = act;
    a.out_f16 = out_f16 ? 1 : 0;
    const unsigned grid = (unsigned)((T + 63) / 64);
    hipStream_t st = (hipStream_t)stream;
    switch (Cin) {
        case 64: linear_launch<2>(a, grid, st); break;
        case 128: linear_launch<4>(a, grid, st); break;
        case 256: linear_launch<8>(a, grid, st); break;
        default: linear_launch<16>(a, grid, st); break;
    }
    MSTG_CHECK_LAUNCH("mstg_f16_linear_fwd");
    return MSTG_OK;
}

extern "C" int mstg_f16_ln_mod_fwd(const void* x, int x_f16, const float* smap, const float* sp_w, const float* sp_b,
                                   const float* gamma, const float* beta, const float* gb, float* h_out, void* u, int N, int L, int dim,
                                   float eps, void* stream) {
    if (!x || !gamma || !beta || !u) return fail_arg(MSTG_E_BADARG, "mstg_f16_ln_mod_fwd: null pointer");
    if (smap && (!sp_w || !sp_b)) return fail_arg(MSTG_E_BADARG, "mstg_f16_ln_mod_fwd: the structure map comes with struct_proj's weight and bias");
    if (h_out && !smap) return fail_arg(MSTG_E_BADARG, "mstg_f16_ln_mod_fwd: h_out is the sum x + struct_proj(s): it needs the structure map");
    if (dim != 64 && dim != 128 && dim != 256) return fail_arg(MSTG_E_UNSUPPORTED, "mstg_f16_ln_mod_fwd: dim must be 64, 128 or 256");
    if (N < 1 || L < 1) return fail_arg(MSTG_E_BADARG, "mstg_f16_ln_mod_fwd: N and L must be positive");
    const long long T = (long long)N * L;
    const unsigned grid = (unsigned)((T + 15) / 16);
    hipStream_t st = (hipStream_t)stream;
    if (x_f16)
        MSTG_LAUNCH(blk_ln_mod_f16_kernel<true>, dim3(grid), dim3(256), 0, st, x, smap, sp_w, sp_b, gamma, beta, gb, h_out,
                    reinterpret_cast<h16*>(u), T, L, dim, eps);
    else
        MSTG_LAUNCH(blk_ln_mod_f16_kernel<false>, dim3(grid), dim3(256), 0, st, x, smap, sp_w, sp_b, gamma, beta, gb, h_out,
                    reinterpret_cast<h16*>(u), T, L, dim, eps);
    MSTG_CHECK_LAUNCH("mstg_f16_ln_mod_fwd");
    return MSTG_OK;
}

extern "C" size_t mstg_f16_token_mean_workspace_bytes(int N, int L, int dim) {
    if (N < 1 || L < 1 || dim < 1) return 0;
    int chunk;
    return (size_t)N * tmean_chunks(L, &chunk) * dim * sizeof(float);
}

extern "C" int mstg_f16_token_mean(const void* x, float* out, int N, int L, int dim, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    if (!x || !out || !workspace) return fail_arg(MSTG_E_BADARG, "mstg_f16_token_mean: null pointer");
    if (dim != 64 && dim != 128 && dim != 256) return fail_arg(MSTG_E_UNSUPPORTED, "mstg_f16_token_mean: dim must be 64, 128 or 256");
    if (N < 1 || L < 1 || N > 65535) return fail_arg(MSTG_E_BADARG, "mstg_f16_token_mean: N must be in 1..65535 and L positive");
    if (workspace_bytes < mstg_f16_token_mean_workspace_bytes(N, L, dim)) return fail_arg(MSTG_E_WORKSPACE, "mstg_f16_token_mean: workspace too small");
    int chunk;
    const int nchunk = tmean_chunks(L, &chunk);
    hipStream_t st = (hipStream_t)stream;
    MSTG_LAUNCH(blk_token_mean_partial_kernel, dim3(nchunk, N), dim3(256), 0, st, reinterpret_cast<const h16*>(x), (float*)workspace, L,
                dim, chunk, nchunk);
    MSTG_CHECK_LAUNCH("blk_token_mean_partial_kernel");
    MSTG_LAUNCH(blk_token_mean_reduce_kernel, dim3(N), dim3(256), 0, st, (const float*)workspace, out, L, dim, nchunk);
    MSTG_CHECK_LAUNCH("blk_token_mean_reduce_kernel");
    return MSTG_OK;
}

extern "C" int mstg_f16_flash_attn_fwd(const void* qkv, void* out, int N, int L, int heads, int D, void* stream) {
    if (!qkv || !out) return fail_arg(MSTG_E_BADARG, "mstg_f16_flash_attn_fwd: null pointer");
    if (N < 1 || L < 1 || heads < 1) return fail_arg(MSTG_E_BADARG, "mstg_f16_flash_attn_fwd: empty tensor");
    if (D != 16 && D != 32 && D != 64) {
        snprintf(g_last_error, sizeof(g_last_error), "mstg_f16_flash_attn_fwd: head width %d is not served (16, 32 or 64)", D);
        return MSTG_E_UNSUPPORTED;
    }
    if (N > 65535 || heads > 65535) return fail_arg(MSTG_E_UNSUPPORTED, "mstg_f16_flash_attn_fwd: grid too large");
    hipStream_t st = (hipStream_t)stream;
    switch (D) {
        case 16: flash_launch<16>(qkv, out, N, L, heads, st); break;
        case 32: flash_launch<32>(qkv, out, N, L, heads, st); break;
        default: flash_launch<64>(qkv, out, N, L, heads, st); break;
    }
    MSTG_CHECK_LAUNCH("mstg_f16_flash_attn_fwd");
    return MSTG_OK;
}
