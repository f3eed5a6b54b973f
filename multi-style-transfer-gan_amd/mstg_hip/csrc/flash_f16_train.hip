// Mixed-precision attention of StructuralTransformerBlock for TRAINING (structural_transformer.py:70): forward with log-sum-exp and
// backward on the 16-bit MFMA of gfx950, fp32 accumulation, fp32 softmax, fp32 results (mstg_f16_attn_cast_qkv,
// mstg_f16_flash_attn_train_fwd / _bwd; include/mstg_hip.h states the arithmetic contract).
//
//   cast      qh = fp16(qkv), qb = bf16(qkv), both round-to-nearest-even from the fp32 values; these two are what autograd saves
//   forward   the arithmetic of blk_flash_f16_kernel (infer_f16_block.hip) on qh, fp32 out, lse = scale m + ln l
//   prep      dO_b = bf16(dO)
//   dQ        workgroup = 64 queries, two sweeps over key tiles: S^T = K_h Q_h^T, dP^T = V_b dO_b^T; delta = sum_keys P dP, then
//             dQ^T += K_b^T dS^T
//   dK / dV   workgroup = 64 keys, loops over query tiles:    S = Q_h K_h^T, dP = dO_b V_b^T, dV^T += dO_b^T P, dK^T += Q_b^T dS
//
// Gradient-side operands are bf16 (fp32's range): no loss scale.  P = exp(scale S - lse) in fp32, rounded to bf16 once for dV;
// dS = bf16(P (dP - delta)), the product formed in fp32.  In all three MFMA kernels the lane's own token is the accumulator COLUMN, so
// the score / P / dS blocks a lane holds are directly the B operand (k-slots = the other side's tokens) of the next MFMA, without
// LDS.  The other side's tiles of 64 tokens are staged in LDS row-major (for S, dP) and transposed (for the second contraction); the
// next tile's global loads are in flight under the current tile's arithmetic.  Every sum runs in a fixed order, no atomics: image
// i of a batch gives the bits of the same image run alone.
#include "lanes.h"

namespace mstg {

typedef unsigned short u16;
typedef short s16x4 __attribute__((ext_vector_type(4)));
constexpr int FT_T = 64;  // tokens per workgroup and per staged tile
constexpr float FT_LOG2E = 1.4426950408889634f;

__device__ __forceinline__ f32x4 mfma16x16x16_bf16(b16x4 a, b16x4 b, f32x4 c) {  // v_mfma_f32_16x16x16_bf16
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a), __builtin_bit_cast(s16x4, b), c, 0, 0, 0);
}

template <int D>
struct FtCfg {
    static constexpr int KST = D + 8;       // 16-bit elements per staged token row (16-byte pieces; conflict-free fragment reads)
    static constexpr int VST = FT_T + 8;    // ... per staged channel row of a transposed tile
    static constexpr int NDF = D / 16;      // 16-channel output fragments
    static constexpr int NQ = D >= 32 ? D / 32 : 1;  // K-steps of a contraction over the channels (one 16x16x16 at D = 16)
    static constexpr int KP = FT_T * D / 8;          // 16-byte pieces of a row-major tile
    static constexpr int NKR = (KP + 255) / 256;     // ... per thread
    static constexpr int VP = FT_T / 2 * D / 8;      // (token pair, 8 channels) pieces of a transposed tile: <= 256
};

// Register image of a tile of 64 tokens x D channels (16-bit elements), stored row-major.  base = channel 0 of the head in token 0
// of the image, ld = elements per token; tokens >= L read token 0 and are stored as zeros.
template <int D>
struct FtRowTile {
    uint4 r[FtCfg<D>::NKR];
    __device__ __forceinline__ void load(const u16* __restrict__ base, long long ld, int t0, int L, int tid) {
#pragma unroll
        for (int k = 0; k < FtCfg<D>::NKR; ++k) {
            const int p = tid + 256 * k;
            const int t = p / (D / 8), q = p - t * (D / 8);
            const bool ok = p < FtCfg<D>::KP && t0 + t < L;
            const uint4 v = *reinterpret_cast<const uint4*>(base + (ok ? (long long)(t0 + t) * ld + 8 * q : 0ll));
            r[k] = ok ? v : uint4{0, 0, 0, 0};
        }
    }
    __device__ __forceinline__ void store(u16* lds, int tid) const {
#pragma unroll
        for (int k = 0; k < FtCfg<D>::NKR; ++k) {
            const int p = tid + 256 * k;
            const int t = p / (D / 8), q = p - t * (D / 8);
            if (p < FtCfg<D>::KP) *reinterpret_cast<uint4*>(&lds[t * FtCfg<D>::KST + 8 * q]) = r[k];
        }
    }
};

// The same tile stored transposed, lds[channel][token]: a thread takes two neighbouring tokens x 8 channels and writes 8 pairs.
template <int D>
struct FtColTile {
    uint4 a = {0, 0, 0, 0}, b = {0, 0, 0, 0};
    __device__ __forceinline__ void load(const u16* __restrict__ base, long long ld, int t0, int L, int tid) {
        if (tid < FtCfg<D>::VP) {
            const int tp = tid & 31, q = tid >> 5;
            const int t = t0 + 2 * tp;
            const bool ok0 = t < L, ok1 = t + 1 < L;
            const uint4 v0 = *reinterpret_cast<const uint4*>(base + (ok0 ? (long long)t * ld + 8 * q : 0ll));
            const uint4 v1 = *reinterpret_cast<const uint4*>(base + (ok1 ? (long long)(t + 1) * ld + 8 * q : 0ll));
            a = ok0 ? v0 : uint4{0, 0, 0, 0};
            b = ok1 ? v1 : uint4{0, 0, 0, 0};
        }
    }
    __device__ __forceinline__ void store(u16* lds, int tid) const {
        if (tid < FtCfg<D>::VP) {
            const int tp = tid & 31, q = tid >> 5;
            const unsigned wa[4] = {a.x, a.y, a.z, a.w}, wb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                *reinterpret_cast<unsigned*>(&lds[(8 * q + 2 * e) * FtCfg<D>::VST + 2 * tp]) = (wa[e] & 0xFFFFu) | (wb[e] << 16);
                *reinterpret_cast<unsigned*>(&lds[(8 * q + 2 * e + 1) * FtCfg<D>::VST + 2 * tp]) = (wa[e] >> 16) | (wb[e] & 0xFFFF0000u);
            }
        }
    }
};

// A operand of a contraction over 32 tokens of a transposed tile: k-slot 8g + j = token 32 kb + 4g + j (j < 4) and
// 32 kb + 16 + 4g + j - 4 -- the registers of accumulator blocks 2 kb and 2 kb + 1 of the lane group.
template <typename V8, typename V4>
__device__ __forceinline__ V8 ft_tr_frag(const u16* row, int kb, int g) {
    const V4 lo = *reinterpret_cast<const V4*>(row + 32 * kb + 4 * g), hi = *reinterpret_cast<const V4*>(row + 32 * kb + 16 + 4 * g);
    return V8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// ---- cast ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ft_cast_kernel(const float* __restrict__ x, u16* __restrict__ xh, u16* __restrict__ xb,
                                                      long long n8) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n8; e += (long long)gridDim.x * 256) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(x + 8 * e), b = *reinterpret_cast<const f32x4*>(x + 8 * e + 4);
        const h16x8 vh = {(h16)a[0], (h16)a[1], (h16)a[2], (h16)a[3], (h16)b[0], (h16)b[1], (h16)b[2], (h16)b[3]};
        const b16x8 vb = {(b16)a[0], (b16)a[1], (b16)a[2], (b16)a[3], (b16)b[0], (b16)b[1], (b16)b[2], (b16)b[3]};
        *reinterpret_cast<h16x8*>(xh + 8 * e) = vh;
        *reinterpret_cast<b16x8*>(xb + 8 * e) = vb;
    }
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
// blk_flash_f16_kernel with fp32 out and the log-sum-exp: S^T = K Q^T (keys on the accumulator rows, the lane's query on the
// column), row maximum by two permlane swaps, p = exp2(s c - m c) in fp32 summed into l in fp32 and rounded to fp16 once,
// O^T += V^T P^T with the S^T registers as the B operand.
template <int D>
__global__ __launch_bounds__(256) void ft_fwd_kernel(const u16* __restrict__ qh, float* __restrict__ out, float* __restrict__ lse,
                                                     int L, int heads, float cexp, float scale) {
    typedef FtCfg<D> CF;
    __shared__ __attribute__((aligned(16))) u16 Ks[FT_T * CF::KST];
    __shared__ __attribute__((aligned(16))) u16 Vt[D * CF::VST];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i = lane & 15, g = lane >> 4;
    const int h = blockIdx.y, dim = heads * D;
    const long long ld = 3ll * dim, img = (long long)blockIdx.z * L;
    const int qi = blockIdx.x * FT_T + 16 * wv + i;
    const bool qv = qi < L;
    const u16* hp = qh + img * ld + h * D;  // q block of the head, token 0 of the image

    h16x8 qf8[CF::NQ];
    h16x4 qf4 = {0, 0, 0, 0};
    {
        const u16* qp = hp + (long long)(qv ? qi : 0) * ld;
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
    FtRowTile<D> kr;
    FtColTile<D> vt;
    f32x4 o[CF::NDF];
#pragma unroll
    for (int df = 0; df < CF::NDF; ++df) o[df] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, lsum = 0.f;

    kr.load(hp + dim, ld, 0, L, tid);
    vt.load(hp + 2 * dim, ld, 0, L, tid);
    kr.store(Ks, tid);
    vt.store(Vt, tid);
    __syncthreads();
    for (int k0 = 0; k0 < L; k0 += FT_T) {
        const bool more = k0 + FT_T < L;
        if (more) {
            kr.load(hp + dim, ld, k0 + FT_T, L, tid);
            vt.load(hp + 2 * dim, ld, k0 + FT_T, L, tid);
        }
        f32x4 s[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            s[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            const u16* kp = &Ks[(16 * c + i) * CF::KST];
            if constexpr (D == 16) {
                s[c] = mfma16x16x16_f16(*reinterpret_cast<const h16x4*>(kp + 4 * g), qf4, s[c]);
            } else {
#pragma unroll
                for (int st = 0; st < CF::NQ; ++st) s[c] = mfma16x16x32_f16(*reinterpret_cast<const h16x8*>(kp + 32 * st + 8 * g), qf8[st], s[c]);
            }
        }
        if (k0 + FT_T > L) {  // ragged last tile
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
        const float mnew = fmaxf(m, tmax);                              // finite: every tile holds a valid key
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
            for (int df = 0; df < CF::NDF; ++df)
                o[df] = mfma16x16x32_f16(ft_tr_frag<h16x8, h16x4>(&Vt[(16 * df + i) * CF::VST], kb, g), pb, o[df]);
        }
        __syncthreads();
        if (more) {
            kr.store(Ks, tid);
            vt.store(Vt, tid);
            __syncthreads();
        }
    }
    lsum = col4_sum(lsum);
    if (qv) {
        const float inv = 1.f / lsum;
        float* op = out + (img + qi) * dim + h * D;
#pragma unroll
        for (int df = 0; df < CF::NDF; ++df) *reinterpret_cast<f32x4*>(op + 16 * df + 4 * g) = o[df] * inv;
        if (g == 0) lse[((long long)blockIdx.z * heads + h) * L + qi] = fmaf(m, scale, __logf(lsum));
    }
}

// ---- backward: the bf16 copy of dO ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ft_cast_bf16_kernel(const float* __restrict__ x, u16* __restrict__ xb, long long n8) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n8; e += (long long)gridDim.x * 256) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(x + 8 * e), b = *reinterpret_cast<const f32x4*>(x + 8 * e + 4);
        const b16x8 vb = {(b16)a[0], (b16)a[1], (b16)a[2], (b16)a[3], (b16)b[0], (b16)b[1], (b16)b[2], (b16)b[3]};
        *reinterpret_cast<b16x8*>(xb + 8 * e) = vb;
    }
}

// ---- backward: delta and dQ -------------------------------------------------------------------------------------------------
// Two sweeps over the key tiles.  Per tile and wave, both form the S^T and dP^T blocks (keys on the rows, the lane's query on the
// column) from the row-major K_h and V_b tiles and P = exp2(s c - lse log2 e) in fp32.
//   sweep 1   delta = sum_keys P dP, fp32, from the very P and dP that dS is made of: a row of dS then sums to zero up to its own
//             bf16 rounding (a single token gives dS = 0 exactly), which sum_d dO O from other roundings of the operands does not;
//             each lane adds its 16 keys of a tile in order, tile after tile, and the four lane groups are added at the end;
//             written for the dK / dV kernel
//   sweep 2   dS^T = bf16(P (dP - delta)) stays in registers as the B operand of dQ^T += K_b^T dS^T (K_b transposed in LDS)
template <int D>
__global__ __launch_bounds__(256) void ft_bwd_dq_kernel(const u16* __restrict__ qh, const u16* __restrict__ qb, const u16* __restrict__ dob,
                                                        const float* __restrict__ lse, float* __restrict__ delta,
                                                        float* __restrict__ dqkv, int L, int heads, float cexp, float scale) {
    typedef FtCfg<D> CF;
    __shared__ __attribute__((aligned(16))) u16 Ks[FT_T * CF::KST];  // K fp16, row-major
    __shared__ __attribute__((aligned(16))) u16 Vs[FT_T * CF::KST];  // V bf16, row-major
    __shared__ __attribute__((aligned(16))) u16 Kt[D * CF::VST];     // K bf16, transposed
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i = lane & 15, g = lane >> 4;
    const int h = blockIdx.y, dim = heads * D;
    const long long ld = 3ll * dim, img = (long long)blockIdx.z * L;
    const int qi = blockIdx.x * FT_T + 16 * wv + i;
    const bool qv = qi < L;
    const u16* hp = qh + img * ld + h * D;
    const u16* bp = qb + img * ld + h * D;

    h16x8 qf8[CF::NQ];
    b16x8 of8[CF::NQ];
    h16x4 qf4 = {0, 0, 0, 0};
    b16x4 of4 = {0, 0, 0, 0};
    {
        const u16* qp = hp + (long long)(qv ? qi : 0) * ld;
        const u16* op = dob + (img + (qv ? qi : 0)) * dim + h * D;
        if constexpr (D == 16) {
            const h16x4 t = *reinterpret_cast<const h16x4*>(qp + 4 * g);
            const b16x4 u = *reinterpret_cast<const b16x4*>(op + 4 * g);
            qf4 = qv ? t : h16x4{0, 0, 0, 0};
            of4 = qv ? u : b16x4{0, 0, 0, 0};
        } else {
#pragma unroll
            for (int s = 0; s < CF::NQ; ++s) {
                const h16x8 t = *reinterpret_cast<const h16x8*>(qp + 32 * s + 8 * g);
                const b16x8 u = *reinterpret_cast<const b16x8*>(op + 32 * s + 8 * g);
                qf8[s] = qv ? t : h16x8{0, 0, 0, 0, 0, 0, 0, 0};
                of8[s] = qv ? u : b16x8{0, 0, 0, 0, 0, 0, 0, 0};
            }
        }
    }
    const long long row = ((long long)blockIdx.z * heads + h) * L + (qv ? qi : 0);
    const float nl = qv ? -lse[row] * FT_LOG2E : 0.f;
    float dl = 0.f;  // sweep 1: this lane's part of delta; sweep 2: delta

    FtRowTile<D> kr, vr;
    FtColTile<D> kt;
    f32x4 dq[CF::NDF];
#pragma unroll
    for (int df = 0; df < CF::NDF; ++df) dq[df] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto sweep = [&](auto second) {  // std::false_type: delta; std::true_type: dQ.  Leaves behind a barrier after its last LDS read.
        constexpr bool DQ = decltype(second)::value;
        kr.load(hp + dim, ld, 0, L, tid);
        vr.load(bp + 2 * dim, ld, 0, L, tid);
        if constexpr (DQ) kt.load(bp + dim, ld, 0, L, tid);
        kr.store(Ks, tid);
        vr.store(Vs, tid);
        if constexpr (DQ) kt.store(Kt, tid);
        __syncthreads();
        for (int k0 = 0; k0 < L; k0 += FT_T) {
            const bool more = k0 + FT_T < L;
            if (more) {
                kr.load(hp + dim, ld, k0 + FT_T, L, tid);
                vr.load(bp + 2 * dim, ld, k0 + FT_T, L, tid);
                if constexpr (DQ) kt.load(bp + dim, ld, k0 + FT_T, L, tid);
            }
            f32x4 s[4], dp[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                s[c] = dp[c] = f32x4{0.f, 0.f, 0.f, 0.f};
                const u16* kp = &Ks[(16 * c + i) * CF::KST];
                const u16* vp = &Vs[(16 * c + i) * CF::KST];
                if constexpr (D == 16) {
                    s[c] = mfma16x16x16_f16(*reinterpret_cast<const h16x4*>(kp + 4 * g), qf4, s[c]);
                    dp[c] = mfma16x16x16_bf16(*reinterpret_cast<const b16x4*>(vp + 4 * g), of4, dp[c]);
                } else {
#pragma unroll
                    for (int st = 0; st < CF::NQ; ++st) {
                        s[c] = mfma16x16x32_f16(*reinterpret_cast<const h16x8*>(kp + 32 * st + 8 * g), qf8[st], s[c]);
                        dp[c] = mfma16x16x32_bf16(*reinterpret_cast<const b16x8*>(vp + 32 * st + 8 * g), of8[st], dp[c]);
                    }
                }
            }
            if (k0 + FT_T > L) {  // ragged last tile: p = exp2(-inf) = 0, and dp = 0 there (zero rows of V)
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (k0 + 16 * c + 4 * g + r >= L) s[c][r] = -INFINITY;
            }
            if constexpr (!DQ) {
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dl = fmaf(__builtin_amdgcn_exp2f(fmaf(s[c][r], cexp, nl)), dp[c][r], dl);
            } else {
                b16x4 dsb[4];
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float p = __builtin_amdgcn_exp2f(fmaf(s[c][r], cexp, nl));
                        dsb[c][r] = (b16)(p * (dp[c][r] - dl));
                    }
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
                    const b16x8 db = {dsb[2 * kb][0], dsb[2 * kb][1], dsb[2 * kb][2], dsb[2 * kb][3],
                                       dsb[2 * kb + 1][0], dsb[2 * kb + 1][1], dsb[2 * kb + 1][2], dsb[2 * kb + 1][3]};
#pragma unroll
                    for (int df = 0; df < CF::NDF; ++df)
                        dq[df] = mfma16x16x32_bf16(ft_tr_frag<b16x8, b16x4>(&Kt[(16 * df + i) * CF::VST], kb, g), db, dq[df]);
                }
            }
            __syncthreads();
            if (more) {
                kr.store(Ks, tid);
                vr.store(Vs, tid);
                if constexpr (DQ) kt.store(Kt, tid);
                __syncthreads();
            }
        }
    };
    sweep(std::false_type{});
    dl = col4_sum(dl);
    if (qv && g == 0) delta[row] = dl;
    sweep(std::true_type{});
    if (qv) {
        float* op = dqkv + (img + qi) * ld + h * D;
#pragma unroll
        for (int df = 0; df < CF::NDF; ++df) *reinterpret_cast<f32x4*>(op + 16 * df + 4 * g) = dq[df] * scale;
    }
}

// ---- backward: dK and dV ------------------------------------------------------------------------------------------------------
// Per query tile and wave: S and dP blocks (queries on the rows, the lane's key on the column) from the row-major Q_h and dO_b
// tiles; P and dS go to bf16 in registers and are the B operands of dV^T += dO_b^T P and dK^T += Q_b^T dS (both transposed in
// LDS).  -lse log2(e) and delta of the tile's queries sit in LDS; a query past L carries -inf there, so its P and dS are 0.
template <int D>
__global__ __launch_bounds__(256) void ft_bwd_dkv_kernel(const u16* __restrict__ qh, const u16* __restrict__ qb, const u16* __restrict__ dob,
                                                         const float* __restrict__ lse, const float* __restrict__ delta,
                                                         float* __restrict__ dqkv, int L, int heads, float cexp, float scale) {
    typedef FtCfg<D> CF;
    __shared__ __attribute__((aligned(16))) u16 Qs[FT_T * CF::KST];  // Q fp16, row-major
    __shared__ __attribute__((aligned(16))) u16 Os[FT_T * CF::KST];  // dO bf16, row-major
    __shared__ __attribute__((aligned(16))) u16 Qt[D * CF::VST];     // Q bf16, transposed
    __shared__ __attribute__((aligned(16))) u16 Ot[D * CF::VST];     // dO bf16, transposed
    __shared__ __attribute__((aligned(16))) float Ls[FT_T];
    __shared__ __attribute__((aligned(16))) float Ds[FT_T];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i = lane & 15, g = lane >> 4;
    const int h = blockIdx.y, dim = heads * D;
    const long long ld = 3ll * dim, img = (long long)blockIdx.z * L;
    const int ki = blockIdx.x * FT_T + 16 * wv + i;  // this lane's key (column)
    const bool kv = ki < L;
    const u16* hp = qh + img * ld + h * D;
    const u16* bp = qb + img * ld + h * D;
    const u16* gp = dob + img * dim + h * D;
    const float* lp = lse + ((long long)blockIdx.z * heads + h) * L;
    const float* dlp = delta + ((long long)blockIdx.z * heads + h) * L;

    h16x8 kf8[CF::NQ];
    b16x8 vf8[CF::NQ];
    h16x4 kf4 = {0, 0, 0, 0};
    b16x4 vf4 = {0, 0, 0, 0};
    {
        const u16* kp = hp + (long long)(kv ? ki : 0) * ld + dim;
        const u16* vp = bp + (long long)(kv ? ki : 0) * ld + 2 * dim;
        if constexpr (D == 16) {
            const h16x4 t = *reinterpret_cast<const h16x4*>(kp + 4 * g);
            const b16x4 u = *reinterpret_cast<const b16x4*>(vp + 4 * g);
            kf4 = kv ? t : h16x4{0, 0, 0, 0};
            vf4 = kv ? u : b16x4{0, 0, 0, 0};
        } else {
#pragma unroll
            for (int s = 0; s < CF::NQ; ++s) {
                const h16x8 t = *reinterpret_cast<const h16x8*>(kp + 32 * s + 8 * g);
                const b16x8 u = *reinterpret_cast<const b16x8*>(vp + 32 * s + 8 * g);
                kf8[s] = kv ? t : h16x8{0, 0, 0, 0, 0, 0, 0, 0};
                vf8[s] = kv ? u : b16x8{0, 0, 0, 0, 0, 0, 0, 0};
            }
        }
    }
    FtRowTile<D> qr, orr;
    FtColTile<D> qt, ot;
    float lreg = 0.f, dreg = 0.f;
    auto load_tile = [&](int q0) {
        qr.load(hp, ld, q0, L, tid);
        orr.load(gp, dim, q0, L, tid);
        qt.load(bp, ld, q0, L, tid);
        ot.load(gp, dim, q0, L, tid);
        if (tid < FT_T) {
            const bool ok = q0 + tid < L;
            const float a = lp[ok ? q0 + tid : 0], b = dlp[ok ? q0 + tid : 0];
            lreg = ok ? -a * FT_LOG2E : -INFINITY;
            dreg = ok ? b : 0.f;
        }
    };
    auto store_tile = [&]() {
        qr.store(Qs, tid);
        orr.store(Os, tid);
        qt.store(Qt, tid);
        ot.store(Ot, tid);
        if (tid < FT_T) {
            Ls[tid] = lreg;
            Ds[tid] = dreg;
        }
    };
    f32x4 dk[CF::NDF], dv[CF::NDF];
#pragma unroll
    for (int df = 0; df < CF::NDF; ++df) dk[df] = dv[df] = f32x4{0.f, 0.f, 0.f, 0.f};

    load_tile(0);
    store_tile();
    __syncthreads();
    for (int q0 = 0; q0 < L; q0 += FT_T) {
        const bool more = q0 + FT_T < L;
        if (more) load_tile(q0 + FT_T);
        b16x4 pb[4], dsb[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
            const u16* qp = &Qs[(16 * c + i) * CF::KST];
            const u16* op = &Os[(16 * c + i) * CF::KST];
            if constexpr (D == 16) {
                s = mfma16x16x16_f16(*reinterpret_cast<const h16x4*>(qp + 4 * g), kf4, s);
                dp = mfma16x16x16_bf16(*reinterpret_cast<const b16x4*>(op + 4 * g), vf4, dp);
            } else {
#pragma unroll
                for (int st = 0; st < CF::NQ; ++st) {
                    s = mfma16x16x32_f16(*reinterpret_cast<const h16x8*>(qp + 32 * st + 8 * g), kf8[st], s);
                    dp = mfma16x16x32_bf16(*reinterpret_cast<const b16x8*>(op + 32 * st + 8 * g), vf8[st], dp);
                }
            }
            const f32x4 nl = *reinterpret_cast<const f32x4*>(&Ls[16 * c + 4 * g]);
            const f32x4 dl = *reinterpret_cast<const f32x4*>(&Ds[16 * c + 4 * g]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(fmaf(s[r], cexp, nl[r]));
                pb[c][r] = (b16)p;
                dsb[c][r] = (b16)(p * (dp[r] - dl[r]));
            }
        }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const b16x8 pk = {pb[2 * kb][0], pb[2 * kb][1], pb[2 * kb][2], pb[2 * kb][3],
                               pb[2 * kb + 1][0], pb[2 * kb + 1][1], pb[2 * kb + 1][2], pb[2 * kb + 1][3]};
            const b16x8 dk8 = {dsb[2 * kb][0], dsb[2 * kb][1], dsb[2 * kb][2], dsb[2 * kb][3],
                                dsb[2 * kb + 1][0], dsb[2 * kb + 1][1], dsb[2 * kb + 1][2], dsb[2 * kb + 1][3]};
#pragma unroll
            for (int df = 0; df < CF::NDF; ++df) {
                dv[df] = mfma16x16x32_bf16(ft_tr_frag<b16x8, b16x4>(&Ot[(16 * df + i) * CF::VST], kb, g), pk, dv[df]);
                dk[df] = mfma16x16x32_bf16(ft_tr_frag<b16x8, b16x4>(&Qt[(16 * df + i) * CF::VST], kb, g), dk8, dk[df]);
            }
        }
        __syncthreads();
        if (more) {
            store_tile();
            __syncthreads();
        }
    }
    if (kv) {
        float* kp = dqkv + (img + ki) * ld + dim + h * D;
#pragma unroll
        for (int df = 0; df < CF::NDF; ++df) {
            *reinterpret_cast<f32x4*>(kp + 16 * df + 4 * g) = dk[df] * scale;
            *reinterpret_cast<f32x4*>(kp + dim + 16 * df + 4 * g) = dv[df];
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static int ft_check(const char* who, int N, int L, int heads, int D) {
    if (N < 1 || L < 1 || heads < 1) {
        snprintf(g_last_error, sizeof(g_last_error), "%s: empty tensor", who);
        return MSTG_E_BADARG;
    }
    if (D != 16 && D != 32 && D != 64) {
        snprintf(g_last_error, sizeof(g_last_error), "%s: head width %d is not served (16, 32 or 64; mstg_flash_attn_* serves 8)", who, D);
        return MSTG_E_UNSUPPORTED;
    }
    if (N > 65535 || heads > 65535) {  // the grid limits of the fp32 path's flash_check
        snprintf(g_last_error, sizeof(g_last_error), "%s: grid too large", who);
        return MSTG_E_UNSUPPORTED;
    }
    return MSTG_OK;
}

static size_t ft_delta_bytes(int N, int L, int heads) { return ((size_t)N * heads * L * sizeof(float) + 15) & ~(size_t)15; }

static unsigned ft_flat_grid(long long work) {
    const long long blocks = (work + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : blocks > 8192 ? 8192 : blocks);
}

template <int D>
static void ft_launch_fwd(const u16* qh, float* out, float* lse, int N, int L, int heads, hipStream_t st) {
    const float scale = 1.f / sqrtf((float)D);
    MSTG_LAUNCH((ft_fwd_kernel<D>), dim3(cdiv(L, FT_T), heads, N), dim3(256), 0, st, qh, out, lse, L, heads, FT_LOG2E * scale, scale);
}

template <int D>
static void ft_launch_bwd(const u16* qh, const u16* qb, const u16* dob, const float* lse, float* delta, float* dqkv, int N, int L,
                          int heads, hipStream_t st) {
    const float scale = 1.f / sqrtf((float)D);
    const dim3 grid(cdiv(L, FT_T), heads, N);
    MSTG_LAUNCH((ft_bwd_dq_kernel<D>), grid, dim3(256), 0, st, qh, qb, dob, lse, delta, dqkv, L, heads, FT_LOG2E * scale, scale);
    MSTG_LAUNCH((ft_bwd_dkv_kernel<D>), grid, dim3(256), 0, st, qh, qb, dob, lse, (const float*)delta, dqkv, L, heads, FT_LOG2E * scale, scale);
}

}  // namespace mstg

using namespace mstg;

extern "C" int mstg_f16_attn_cast_qkv(const float* qkv, void* qh, void* qb, int N, int L, int heads, int D, void* stream) {
    if (!qkv || !qh || !qb) return fail_arg(MSTG_E_BADARG, "mstg_f16_attn_cast_qkv: null pointer");
    if (int rc = ft_check("mstg_f16_attn_cast_qkv", N, L, heads, D)) return rc;
    const long long n8 = (long long)N * L * 3 * heads * D / 8;  // D is a multiple of 16
    MSTG_LAUNCH(ft_cast_kernel, dim3(ft_flat_grid(n8)), dim3(256), 0, (hipStream_t)stream, qkv, reinterpret_cast<u16*>(qh),
                reinterpret_cast<u16*>(qb), n8);
    MSTG_CHECK_LAUNCH("mstg_f16_attn_cast_qkv");
    return MSTG_OK;
}

extern "C" int mstg_f16_flash_attn_train_fwd(const void* qh, float* out, float* lse, int N, int L, int heads, int D, void* stream) {
    if (!qh || !out || !lse) return fail_arg(MSTG_E_BADARG, "mstg_f16_flash_attn_train_fwd: null pointer");
    if (int rc = ft_check("mstg_f16_flash_attn_train_fwd", N, L, heads, D)) return rc;
    for_width<16, 32, 64>(D, [&](auto w) { ft_launch_fwd<w()>(reinterpret_cast<const u16*>(qh), out, lse, N, L, heads, (hipStream_t)stream); });
    MSTG_CHECK_LAUNCH("mstg_f16_flash_attn_train_fwd");
    return MSTG_OK;
}

extern "C" size_t mstg_f16_flash_attn_train_bwd_workspace_bytes(int N, int L, int heads, int D) {
    if (N < 1 || L < 1 || heads < 1 || D < 1) return 0;
    return ft_delta_bytes(N, L, heads) + (size_t)N * L * heads * D * sizeof(u16);
}

extern "C" int mstg_f16_flash_attn_train_bwd(const void* qh, const void* qb, const float* lse, const float* d_out,
                                             float* dqkv, void* workspace, size_t workspace_bytes, int N, int L, int heads, int D,
                                             void* stream) {
    if (!qh || !qb || !lse || !d_out || !dqkv || !workspace)
        return fail_arg(MSTG_E_BADARG, "mstg_f16_flash_attn_train_bwd: null pointer");
    if (int rc = ft_check("mstg_f16_flash_attn_train_bwd", N, L, heads, D)) return rc;
    if (workspace_bytes < mstg_f16_flash_attn_train_bwd_workspace_bytes(N, L, heads, D))
        return fail_arg(MSTG_E_WORKSPACE, "mstg_f16_flash_attn_train_bwd: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float* delta = reinterpret_cast<float*>(workspace);
    u16* dob = reinterpret_cast<u16*>(reinterpret_cast<char*>(workspace) + ft_delta_bytes(N, L, heads));
    const long long n8 = (long long)N * L * heads * D / 8;  // D is a multiple of 16
    MSTG_LAUNCH(ft_cast_bf16_kernel, dim3(ft_flat_grid(n8)), dim3(256), 0, st, d_out, dob, n8);
    MSTG_CHECK_LAUNCH("mstg_f16_flash_attn_train_bwd (cast)");
    for_width<16, 32, 64>(D, [&](auto w) {
        ft_launch_bwd<w()>(reinterpret_cast<const u16*>(qh), reinterpret_cast<const u16*>(qb), dob, lse, delta, dqkv, N, L, heads, st);
    });
    MSTG_CHECK_LAUNCH("mstg_f16_flash_attn_train_bwd");
    return MSTG_OK;
}
