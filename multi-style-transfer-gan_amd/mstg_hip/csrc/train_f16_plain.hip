// Mixed-precision (fp16 storage / fp16 MFMA / fp32 accumulation) training step of the plain CycleGAN Generator: what
// pretrain.py:159-166 runs under torch.cuda.amp.autocast() on the layer stack of pretrain.py:60-97 (mstg_f16_train_*,
// include/mstg_hip.h).  The forward convolutions and every input gradient are launches of plain_conv_f16_kernel
// (csrc/infer_f16_plain.hip); this file holds what a training step needs beside them:
//   * BatchNorm2d in TRAINING mode on NHWC fp16 activations, forward (batch statistics, running statistics) and backward;
//   * the masked-L1 loss with the tanh backward that starts the chain, times a loss scale read from device memory;
//   * the weight gradient of a k4 s2 p1 layer on v_mfma_f32_16x16x32_f16, operands read through ds_read_b64_tr_b16;
//   * the step's bookkeeping: non-finite check / scale halving and an Adam launch that a device flag turns into a no-op.
// Everything sums in a fixed order (no atomics): two runs of a step give the same bits.
//
// Weight gradient.  Both layer kinds are ONE product.  With S the layer's small map (N,h,w,Cs) and B its big map (N,2h,2w,Cb),
//   G[s][b][ky][kx] = sum over (n,y,x) of S[n][y][x][s] * B[n][2y+ky-1][2x+kx-1][b]
// is dW (Cout=s, Cin=b, 4, 4) of nn.Conv2d(k4,s2,p1) with S = dZ, B = X, and dW (Cin=s, Cout=b, 4, 4) of nn.ConvTranspose2d(k4,s2,p1)
// with S = X, B = dZ: the same memory layout (s, b, 4, 4) both times.  Per filter tap it is a GEMM with M = Cs, N = Cb and the
// PIXEL index as K, the strided index of both NHWC operands.  A workgroup owns a 16 MS x 16 NB tile of (s, b), all 16 taps and a
// contiguous range ("slab") of chunks of 32 small pixels, flattened over the batch.  Per chunk it stages to LDS, as they come
// from memory, [32 pixels][16 MS channels] of S and, per tap, [32 pixels][16 NB channels] of B (pixels outside the map: zeros),
// and each of the four waves runs four taps.  The MFMA wants, per lane, 8 consecutive K of ONE channel: a column of the staged
// tile, which ds_read_b64_tr_b16 delivers (4 pixel rows x 16 channels per 16-lane group, two reads per operand).  K index
// 8 g + j of the MFMA is pixel row 4 g + j (j < 4) or 16 + 4 g + (j - 4) of the chunk, for both operands alike, so that a
// 32-lane half reads the 8 CONSECUTIVE rows 8 (g >> 1) .. + 7 (+ 16): with a row stride of 8 x odd dwords (WG_ROW) the eight rows
// start 8 banks apart and the half's 64 dwords cover the 64 banks once, conflict-free.
// Slabs are fp32 [slab][tap][s][b]; wgrad_reduce_kernel adds them in slab order, multiplies by 1 / loss scale and writes (s, b, 4, 4).
#include "lanes.h"

namespace mstg {

constexpr int TR_MAXC = 512;
constexpr int TR_MAX_PART = 256;  // partial rows of a per-channel reduction

// device state of the step: fstate = {loss scale, 1 / loss scale}, istate = {skipped steps, good steps, last step ok}

// ---- fixed-order reductions ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float train_block_sum(float v, float* sh4) {  // 256 threads, every thread gets the sum
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- image -> NHWC fp16, 3 channels padded to 8 (the stem's weight gradient reads it as its big map) --------------------------
__global__ void train_img_nhwc8_kernel(const float* __restrict__ img, h16* __restrict__ out, long long npix, long long HW) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const long long n = p / HW, i = p - n * HW;
    h16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (h16)img[(n * 3 + c) * HW + i];
    *reinterpret_cast<h16x8*>(out + p * 8) = v;
}

// ---- per-channel sums over the pixels of an NHWC fp16 tensor -----------------------------------------------------------------
// Thread t of a block owns the 8 channels 8 (t % cg) .. + 7 of the pixels p0 + t / cg + k (256 / cg) of the block's range; the
// rows of a block are then added in row order and the blocks by the *_final kernels in block order.
// MODE 0: batch statistics, two passes over the block's range: its mean, then the squares about that mean (pmean, pm2).
// MODE 1: BatchNorm backward: sum(dyh), sum(dyh * xhat) with dyh = dy * act'(gamma xhat + beta)  (pa, pb).
// MODE 2: plain sum (bias gradients)  (pa).
struct ChanArgs {
    const h16* z;
    const h16* dy;
    const float *mean, *rstd, *gamma, *beta;
    float *pa, *pb;
    long long P, ppb;
    int C, act;
};

__device__ __forceinline__ void train_rows_sum(const float (&acc)[8], float* sh, int C, int cg, int rows, float* out, float mul) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) sh[threadIdx.x * 8 + j] = acc[j];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float s = 0.f;
        for (int r = 0; r < rows; ++r) s += sh[(r * cg + (c >> 3)) * 8 + (c & 7)];
        out[c] = s * mul;
    }
    __syncthreads();
}

template <int MODE>
__global__ __launch_bounds__(256) void train_chan_partial_kernel(ChanArgs a) {
    __shared__ float sh[256 * 8];
    __shared__ float red[TR_MAXC];
    const int cg = a.C >> 3, rows = 256 / cg;
    const int g = threadIdx.x % cg, row = threadIdx.x / cg;
    const bool active = row < rows;
    const long long p0 = (long long)blockIdx.x * a.ppb, p1 = p0 + a.ppb < a.P ? p0 + a.ppb : a.P;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float* const outa = a.pa + (size_t)blockIdx.x * a.C;
    if constexpr (MODE == 0) {
        if (active)
            for (long long p = p0 + row; p < p1; p += rows) {
                const h16x8 v = *reinterpret_cast<const h16x8*>(a.z + p * a.C + 8 * g);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += (float)v[j];
            }
        train_rows_sum(acc, sh, a.C, cg, rows, red, 1.f / (float)(p1 - p0));
        float m[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            m[j] = red[8 * g + j];
            acc[j] = 0.f;
        }
        if (active)
            for (long long p = p0 + row; p < p1; p += rows) {
                const h16x8 v = *reinterpret_cast<const h16x8*>(a.z + p * a.C + 8 * g);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float d = (float)v[j] - m[j];
                    acc[j] += d * d;
                }
            }
        for (int c = threadIdx.x; c < a.C; c += 256) outa[c] = red[c];
        train_rows_sum(acc, sh, a.C, cg, rows, a.pb + (size_t)blockIdx.x * a.C, 1.f);
    } else if constexpr (MODE == 1) {
        float acc2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (active) {
            float mean[8], rstd[8], gam[8], bet[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                mean[j] = a.mean[8 * g + j];
                rstd[j] = a.rstd[8 * g + j];
                gam[j] = a.gamma[8 * g + j];
                bet[j] = a.beta[8 * g + j];
            }
            for (long long p = p0 + row; p < p1; p += rows) {
                const h16x8 v = *reinterpret_cast<const h16x8*>(a.z + p * a.C + 8 * g);
                const h16x8 d = *reinterpret_cast<const h16x8*>(a.dy + p * a.C + 8 * g);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float xh = ((float)v[j] - mean[j]) * rstd[j];
                    const float dh = (float)d[j] * act_grad(gam[j] * xh + bet[j], a.act);
                    acc[j] += dh;
                    acc2[j] += dh * xh;
                }
            }
        }
        train_rows_sum(acc, sh, a.C, cg, rows, outa, 1.f);
        train_rows_sum(acc2, sh, a.C, cg, rows, a.pb + (size_t)blockIdx.x * a.C, 1.f);
    } else {
        if (active)
            for (long long p = p0 + row; p < p1; p += rows) {
                const h16x8 v = *reinterpret_cast<const h16x8*>(a.z + p * a.C + 8 * g);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += (float)v[j];
            }
        train_rows_sum(acc, sh, a.C, cg, rows, outa, 1.f);
    }
}

// one wave per channel.  mean = sum n_b mean_b / P, M2 = sum (M2_b + n_b (mean_b - mean)^2): the parallel form of the two-pass
// variance, in double (a few hundred terms per channel).  Running statistics as nn.BatchNorm2d: momentum, unbiased variance.
__global__ __launch_bounds__(64) void train_bn_stats_final_kernel(const float* __restrict__ pmean, const float* __restrict__ pm2, int nb,
                                                                  long long P, long long ppb, int C, float eps, float momentum,
                                                                  float* __restrict__ mean, float* __restrict__ rstd,
                                                                  float* __restrict__ running_mean, float* __restrict__ running_var) {
    const int c = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += 64) {
        const long long n = (b + 1) * ppb <= P ? ppb : P - b * ppb;
        s += (double)n * (double)pmean[(size_t)b * C + c];
    }
    const double mu = wave_sum_d(s) / (double)P;
    double q = 0.0;
    for (int b = threadIdx.x; b < nb; b += 64) {
        const long long n = (b + 1) * ppb <= P ? ppb : P - b * ppb;
        const double d = (double)pmean[(size_t)b * C + c] - mu;
        q += (double)pm2[(size_t)b * C + c] + (double)n * d * d;
    }
    const double var = wave_sum_d(q) / (double)P;
    if (threadIdx.x == 0) {
        mean[c] = (float)mu;
        rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
        if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mu;
        if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)(var * (double)P / (double)(P > 1 ? P - 1 : 1));
    }
}

__global__ __launch_bounds__(64) void train_bn_bwd_final_kernel(const float* __restrict__ pa, const float* __restrict__ pb, int nb, int C,
                                                                const float* __restrict__ fstate, float* __restrict__ sums,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int b = threadIdx.x; b < nb; b += 64) {
        s1 += (double)pa[(size_t)b * C + c];
        s2 += (double)pb[(size_t)b * C + c];
    }
    s1 = wave_sum_d(s1);
    s2 = wave_sum_d(s2);
    if (threadIdx.x == 0) {
        const float inv = fstate[1];
        sums[c] = (float)s1;
        sums[C + c] = (float)s2;
        dbeta[c] = (float)s1 * inv;
        dgamma[c] = (float)s2 * inv;
    }
}

__global__ __launch_bounds__(64) void train_bias_final_kernel(const float* __restrict__ pa, int nb, int C, int Cvalid,
                                                              const float* __restrict__ fstate, float* __restrict__ out) {
    const int c = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += 64) s += (double)pa[(size_t)b * C + c];
    s = wave_sum_d(s);
    if (threadIdx.x == 0 && c < Cvalid) out[c] = (float)s * fstate[1];
}

// y = act(gamma (z - mean) rstd + beta), one rounding to fp16.  The grid's thread count is a multiple of cg = C / 8 (bn_ew_blocks),
// so a thread stays on one group of 8 channels: its 32 per-channel constants are loaded once, the loop only streams.
__global__ void train_bn_apply_kernel(const h16* __restrict__ z, const float* __restrict__ mean, const float* __restrict__ rstd,
                                      const float* __restrict__ gamma, const float* __restrict__ beta, h16* __restrict__ y,
                                      long long pieces, int cg, int act) {
    const long long stride = (long long)gridDim.x * blockDim.x, i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = (int)(i0 % cg) * 8;
    float mu[8], rs[8], ga[8], be[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        mu[j] = mean[c + j];
        rs[j] = rstd[c + j];
        ga[j] = gamma[c + j];
        be[j] = beta[c + j];
    }
    for (long long i = i0; i < pieces; i += stride) {
        const h16x8 v = reinterpret_cast<const h16x8*>(z)[i];
        h16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (h16)apply_act(ga[j] * (((float)v[j] - mu[j]) * rs[j]) + be[j], act);
        reinterpret_cast<h16x8*>(y)[i] = o;
    }
}

// dz = gamma rstd (dyh - mean(dyh) - xhat mean(dyh xhat)), one rounding to fp16; sums = {sum dyh [C], sum dyh xhat [C]}
__global__ void train_bn_bwd_apply_kernel(const h16* __restrict__ z, const h16* __restrict__ dy, const float* __restrict__ mean,
                                          const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                          const float* __restrict__ sums, h16* __restrict__ dz, long long pieces, int cg, int act,
                                          float invP) {
    const int C = cg * 8;
    const long long stride = (long long)gridDim.x * blockDim.x, i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = (int)(i0 % cg) * 8;
    float mu[8], rs[8], ga[8], be[8], gr[8], m1[8], m2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        mu[j] = mean[c + j];
        rs[j] = rstd[c + j];
        ga[j] = gamma[c + j];
        be[j] = beta[c + j];
        gr[j] = ga[j] * rs[j];
        m1[j] = sums[c + j] * invP;
        m2[j] = sums[C + c + j] * invP;
    }
    for (long long i = i0; i < pieces; i += stride) {
        const h16x8 v = reinterpret_cast<const h16x8*>(z)[i];
        const h16x8 d = reinterpret_cast<const h16x8*>(dy)[i];
        h16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float xh = ((float)v[j] - mu[j]) * rs[j];
            const float dh = (float)d[j] * act_grad(ga[j] * xh + be[j], act);
            o[j] = (h16)(gr[j] * (dh - m1[j] - xh * m2[j]));
        }
        reinterpret_cast<h16x8*>(dz)[i] = o;
    }
}

// backward of LeakyReLU(0.2) / ReLU from the activation's OUTPUT a (both keep the sign of their input): dz = da * act'(a)
__global__ void train_act_bwd_kernel(const h16* __restrict__ a, const h16* __restrict__ da, h16* __restrict__ dz, long long pieces, int act) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < pieces; i += stride) {
        const h16x8 v = reinterpret_cast<const h16x8*>(a)[i];
        const h16x8 d = reinterpret_cast<const h16x8*>(da)[i];
        h16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (h16)((float)d[j] * act_grad((float)v[j], act));
        reinterpret_cast<h16x8*>(dz)[i] = o;
    }
}

// ---- loss and the gradient that enters the chain -------------------------------------------------------------------------------
// y: the head's fp16 image (N,3,H,W); real, mask: fp32 (N,3,H,W).  With k = 1 - mask and d = y k - real k (products first, as the
// reference forms them): partial[block] = sum |d|, dz[pixel][c] = scale / numel * sign(d) * k * (1 - y^2) as NHWC fp16 with the 3
// channels padded to 8 (the layout the head's input and weight gradients read).
__global__ __launch_bounds__(256) void train_head_loss_bwd_kernel(const h16* __restrict__ y, const float* __restrict__ real,
                                                                  const float* __restrict__ mask, long long npix, long long HW,
                                                                  const float* __restrict__ fstate, float inv_numel,
                                                                  float* __restrict__ partial, h16* __restrict__ dz) {
    __shared__ float sh4[4];
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    float acc = 0.f;
    if (p < npix) {
        const float gs = fstate[0] * inv_numel;
        const long long n = p / HW, i = p - n * HW;
        h16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long long e = (n * 3 + c) * HW + i;
            const float yv = (float)y[e], k = 1.f - mask[e];
            const float d = yv * k - real[e] * k;
            acc += fabsf(d);
            o[c] = (h16)((d > 0.f ? gs : (d < 0.f ? -gs : 0.f)) * k * (1.f - yv * yv));
        }
        *reinterpret_cast<h16x8*>(dz + p * 8) = o;
    }
    const float r = train_block_sum(acc, sh4);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}
__global__ __launch_bounds__(256) void train_loss_final_kernel(const float* __restrict__ partial, long long nb, float inv_numel,
                                                               float* __restrict__ loss) {
    __shared__ float sh4[4];
    float acc = 0.f;
    for (long long i = threadIdx.x; i < nb; i += 256) acc += partial[i];
    const float r = train_block_sum(acc, sh4);
    if (threadIdx.x == 0) loss[0] = r * inv_numel;
}

// ---- weight gradient -----------------------------------------------------------------------------------------------------------
constexpr int WG_PX = 32;  // small pixels per chunk = one MFMA K-step
constexpr int wg_row(int frags) { return frags == 1 ? 32 : (frags == 2 ? 96 : 160); }  // bytes per staged pixel row: 8 x odd dwords
constexpr int wg_lds_bytes(int MS, int NB) { return WG_PX * wg_row(MS) + 16 * WG_PX * wg_row(NB); }

struct WgradArgs {
    const h16* S;
    const h16* B;
    float* part;      // [slab][16][Cs][CbOut]
    long long P;      // small pixels N h w
    int h, w, Cs, Cb, CbOut;
    int nts, ntb;     // tiles over s and b
    int nchunks, cps; // chunks of 32 pixels, chunks per slab
};

__device__ __forceinline__ h16x8 wg_tr_read(const unsigned char* base, int off_lo, int off_hi) {
    typedef __fp16 trv4 __attribute__((__vector_size__(8)));
    typedef __attribute__((address_space(3))) trv4 lds_trv4;
    const trv4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_trv4*)(base + off_lo));
    const trv4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_trv4*)(base + off_hi));
    union {
        trv4 h[2];
        h16x8 v;
    } u;
    u.h[0] = lo;
    u.h[1] = hi;
    return u.v;
}

template <int MS, int NB>
__global__ __launch_bounds__(256) void wgrad_f16_kernel(WgradArgs a) {
    constexpr int SROW = wg_row(MS), BROW = wg_row(NB);
    constexpr int SP = 2 * MS, BP = 2 * NB;       // 16-byte pieces per pixel row
    constexpr int TSTEP = 256 / (WG_PX * BP);     // taps between two pieces of a thread
    constexpr int NI = 16 / TSTEP;                // B pieces per thread and chunk
    constexpr int BTAP = WG_PX * BROW;            // bytes of one tap's tile
    extern __shared__ __attribute__((aligned(16))) unsigned char wg_smem[];
    unsigned char* const Ss = wg_smem;                  // [32][SROW]
    unsigned char* const Bs = wg_smem + WG_PX * SROW;   // [16][32][BROW]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bid = blockIdx.x;
    const int tb = bid % a.ntb; bid /= a.ntb;
    const int ts = bid % a.nts;
    const int slab = bid / a.nts;
    const int s0 = ts * 16 * MS, b0 = tb * 16 * NB;
    const int c_begin = slab * a.cps, c_end = c_begin + a.cps < a.nchunks ? c_begin + a.cps : a.nchunks;

    // staging roles: B piece (bpx, bq) of taps btap0 + TSTEP i; S piece (spx, sq) for tid < 32 SP
    const int bq = tid % BP, bpx = (tid / BP) % WG_PX, btap0 = tid / (BP * WG_PX);
    const int sq = tid % SP, spx = (tid / SP) % WG_PX;
    const bool s_thread = tid < WG_PX * SP;
    const bool bch_ok = b0 + 8 * bq < a.Cb, sch_ok = s0 + 8 * sq < a.Cs;
    const int hw = a.h * a.w, H2 = 2 * a.h, W2 = 2 * a.w;

    uint4 breg[NI], sreg;
    auto load_chunk = [&](int ch) {
        const long long pb = (long long)ch * WG_PX + bpx;
        int y2 = 0, x2 = 0;
        long long nimg = 0;
        const bool pok = pb < a.P;
        if (pok) {
            nimg = pb / hw;
            const int rem = (int)(pb - nimg * hw);
            const int y = rem / a.w;
            y2 = 2 * y - 1;
            x2 = 2 * (rem - y * a.w) - 1;
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int tap = btap0 + TSTEP * i;
            const int Y = y2 + (tap >> 2), X = x2 + (tap & 3);
            const bool ok = pok && bch_ok && (unsigned)Y < (unsigned)H2 && (unsigned)X < (unsigned)W2;
            const long long off = ok ? ((nimg * H2 + Y) * (long long)W2 + X) * a.Cb + b0 + 8 * bq : 0ll;
            const uint4 v = *reinterpret_cast<const uint4*>(a.B + off);
            breg[i] = ok ? v : uint4{0, 0, 0, 0};
        }
        const long long ps = (long long)ch * WG_PX + spx;
        const bool ok = s_thread && sch_ok && ps < a.P;
        const uint4 v = *reinterpret_cast<const uint4*>(a.S + (ok ? ps * a.Cs + s0 + 8 * sq : 0ll));
        sreg = ok ? v : uint4{0, 0, 0, 0};
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < NI; ++i) *reinterpret_cast<uint4*>(&Bs[(btap0 + TSTEP * i) * BTAP + bpx * BROW + bq * 16]) = breg[i];
        if (s_thread) *reinterpret_cast<uint4*>(&Ss[spx * SROW + sq * 16]) = sreg;
    };

    f32x4 acc[4][MS][NB];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int m = 0; m < MS; ++m)
#pragma unroll
            for (int n = 0; n < NB; ++n) acc[t][m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    // transposed-read address of this lane (T10): group g = lane >> 4 reads pixel rows 4 g + q (and + 16), lane 4 q + p of the
    // group supplies row q, channels 4 p .. 4 p + 3 of the fragment
    const int g = lane >> 4, qrow = (lane >> 2) & 3, pcol = lane & 3;
    const int s_lo = (4 * g + qrow) * SROW + pcol * 8, b_lo = (4 * g + qrow) * BROW + pcol * 8;

    load_chunk(c_begin);
    store_chunk();
    __syncthreads();
    for (int ch = c_begin; ch < c_end; ++ch) {
        const bool more = ch + 1 < c_end;
        if (more) load_chunk(ch + 1);
        h16x8 sf[MS];
#pragma unroll
        for (int m = 0; m < MS; ++m) sf[m] = wg_tr_read(Ss, s_lo + 32 * m, s_lo + 32 * m + 16 * SROW);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const unsigned char* bt = Bs + (wave * 4 + t) * BTAP;
#pragma unroll
            for (int n = 0; n < NB; ++n) {
                const h16x8 bf = wg_tr_read(bt, b_lo + 32 * n, b_lo + 32 * n + 16 * BROW);
#pragma unroll
                for (int m = 0; m < MS; ++m) acc[t][m][n] = mfma16x16x32_f16(sf[m], bf, acc[t][m][n]);
            }
        }
        __syncthreads();  // every wave has read chunk ch
        if (more) store_chunk();
        __syncthreads();
    }

    // acc[t][m][n][r] = G[s = s0 + 16 m + 4 (lane >> 4) + r][b = b0 + 16 n + (lane & 15)][tap = 4 wave + t]
    float* const part = a.part + (size_t)slab * 16 * a.Cs * a.CbOut;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int m = 0; m < MS; ++m)
#pragma unroll
            for (int n = 0; n < NB; ++n) {
                const int b = b0 + 16 * n + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int s = s0 + 16 * m + 4 * (lane >> 4) + r;
                    if (s < a.Cs && b < a.CbOut) part[((size_t)(wave * 4 + t) * a.Cs + s) * a.CbOut + b] = acc[t][m][n][r];
                }
            }
}

// dW[(s CbOut + b) 16 + tap] = (1 / loss scale) * sum over slabs, in slab order
__global__ void wgrad_reduce_kernel(const float* __restrict__ part, int nslabs, int Cs, int CbOut, const float* __restrict__ fstate,
                                    float* __restrict__ dW) {
    const size_t per = (size_t)16 * Cs * CbOut;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // (tap, s, b), b fastest
    if (e >= per) return;
    float s = 0.f;
    for (int k = 0; k < nslabs; ++k) s += part[(size_t)k * per + e];
    const int b = (int)(e % CbOut);
    const size_t r = e / CbOut;
    const int sc = (int)(r % Cs), tap = (int)(r / Cs);
    dW[((size_t)sc * CbOut + b) * 16 + tap] = s * fstate[1];
}

// ---- step bookkeeping ------------------------------------------------------------------------------------------------------------
// norm: the pre-clip gradient norm.  Finite: one more good step.  Not finite: one more skipped step, the loss scale is halved.
__global__ void train_scale_update_kernel(const float* __restrict__ norm, float* __restrict__ fstate, int* __restrict__ istate) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float v = norm[0];
    const bool ok = v == v && fabsf(v) <= 3.402823466e38f;
    if (ok) {
        istate[1] += 1;
    } else {
        istate[0] += 1;
        fstate[0] *= 0.5f;
        fstate[1] *= 2.f;
    }
    istate[2] = ok ? 1 : 0;
}

// torch.optim.Adam as adam_kernel (csrc/elementwise.hip) computes it, at step = step_base + the good steps counted on the device;
// a no-op when the step that has just been checked was not ok
__global__ void train_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, size_t n,
                                  float lr, float b1, float b2, float eps, int step_base, const int* __restrict__ istate) {
    if (!istate[2]) return;
    const int step = step_base + istate[1];
    const float bc1 = (float)(1.0 - pow((double)b1, (double)step));
    const float bc2_sqrt = (float)sqrt(1.0 - pow((double)b2, (double)step));
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float gi = g[i];
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        p[i] -= (lr / bc1) * (mi / denom);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
static const char* chan_validate(long long P, int C) {
    if (P < 1) return "mstg_f16_train: the tensor has no pixels";
    if (C < 8 || C > TR_MAXC || C % 8) return "mstg_f16_train: channels must be a multiple of 8 up to 512";
    return nullptr;
}
static int chan_blocks(long long P, int C, long long* ppb) {
    const int rows = 256 / (C / 8);
    long long nb = (P + rows - 1) / rows;  // at least one pixel per thread row
    if (nb > TR_MAX_PART) nb = TR_MAX_PART;
    *ppb = (P + nb - 1) / nb;
    return (int)((P + *ppb - 1) / *ppb);
}
static size_t chan_ws_bytes(int C) { return (size_t)(2 * TR_MAX_PART + 2) * C * sizeof(float); }
static unsigned ew_blocks(long long pieces) {
    const long long nb = (pieces + 255) / 256;
    return (unsigned)(nb < 1 ? 1 : (nb > 8192 ? 8192 : nb));
}

// grid of the BatchNorm apply kernels: a multiple of cg blocks, so that blocks * 256 threads is a multiple of cg
static unsigned bn_ew_blocks(long long pieces, int cg) {
    const unsigned nb = ew_blocks(pieces);
    return (nb + cg - 1) / cg * cg;
}

static const char* wgrad_validate(int N, int h, int w, int Cs, int Cb, int CbOut) {
    if (N < 1 || h < 1 || w < 1) return "mstg_f16_train_wgrad: N, h, w must be positive";
    if (Cs < 8 || Cs > TR_MAXC || Cs % 8) return "mstg_f16_train_wgrad: Cs must be a multiple of 8 up to 512";
    if (Cb < 8 || Cb > TR_MAXC || Cb % 8) return "mstg_f16_train_wgrad: Cb must be a multiple of 8 up to 512 (pad a 3-channel image to 8)";
    if (CbOut < 1 || CbOut > Cb) return "mstg_f16_train_wgrad: CbOut must be in 1..Cb";
    if ((long long)N * h * w >= (1ll << 31) - WG_PX) return "mstg_f16_train_wgrad: too many pixels";
    return nullptr;
}
struct WgradPlan {
    int MS, NB, nts, ntb, nchunks, cps, nslabs;
};
static WgradPlan wgrad_plan(int N, int h, int w, int Cs, int Cb) {
    WgradPlan p;
    p.MS = Cs > 32 ? 4 : (Cs > 16 ? 2 : 1);
    p.NB = Cb > 16 ? 2 : 1;
    p.nts = cdiv(Cs, 16 * p.MS);
    p.ntb = cdiv(Cb, 16 * p.NB);
    p.nchunks = (int)(((long long)N * h * w + WG_PX - 1) / WG_PX);
    // about two workgroups per CU, a slab no shorter than four chunks; the split depends on the shape alone
    int want = cdiv(512, p.nts * p.ntb);
    const int most = cdiv(p.nchunks, 4);
    if (want > most) want = most;
    if (want < 1) want = 1;
    p.cps = cdiv(p.nchunks, want);
    p.nslabs = cdiv(p.nchunks, p.cps);
    return p;
}

template <int MS, int NB>
static int wgrad_launch(const WgradArgs& a, unsigned grid, hipStream_t st) {
    constexpr int lds = wg_lds_bytes(MS, NB);
    MSTG_LAUNCH((wgrad_f16_kernel<MS, NB>), dim3(grid), dim3(256), lds, st, a);
    return MSTG_OK;
}

}  // namespace mstg

using namespace mstg;

extern "C" int mstg_f16_train_image_nhwc8(const float* img, void* out, int N, int H, int W, void* stream) {
    if (!img || !out) return fail_arg(MSTG_E_BADARG, "mstg_f16_train_image_nhwc8: null pointer");
    if (N < 1 || H < 1 || W < 1) return fail_arg(MSTG_E_BADARG, "mstg_f16_train_image_nhwc8: N, H, W must be positive");
    const long long HW = (long long)H * W, npix = HW * N;
    MSTG_LAUNCH(train_img_nhwc8_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, img,
                reinterpret_cast<h16*>(out), npix, HW);
    MSTG_CHECK_LAUNCH("train_img_nhwc8_kernel");
    return MSTG_OK;
}

extern "C" size_t mstg_f16_train_bn_workspace_bytes(size_t P, int C) {
    if (const char* e = chan_validate((long long)P, C)) {
        fail_arg(MSTG_E_UNSUPPORTED, e);
        return 0;
    }
    return chan_ws_bytes(C);
}

extern "C" int mstg_f16_train_bn_fwd(const void* z, const float* gamma, const float* beta, size_t P, int C, int act, float eps,
                                     float momentum, float* running_mean, float* running_var, float* mean, float* rstd, void* y,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    if (const char* e = chan_validate((long long)P, C)) return fail_arg(MSTG_E_UNSUPPORTED, e);
    if (!z || !gamma || !beta || !mean || !rstd || !y || !workspace) return fail_arg(MSTG_E_BADARG, "mstg_f16_train_bn_fwd: null pointer");
    if (P < 2) return fail_arg(MSTG_E_BADARG, "mstg_f16_train_bn_fwd: batch statistics need more than one value per channel");
    if (act != MSTG_ACT_NONE && act != MSTG_ACT_RELU && act != MSTG_ACT_LEAKY02)
        return fail_arg(MSTG_E_UNSUPPORTED, "mstg_f16_train_bn_fwd: act must be none, ReLU or LeakyReLU(0.2)");
    if (workspace_bytes < chan_ws_bytes(C)) return fail_arg(MSTG_E_WORKSPACE, "mstg_f16_train_bn_fwd: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    ChanArgs a{};
    a.z = reinterpret_cast<const h16*>(z);
    a.P = (long long)P;
    a.C = C;
    a.pa = reinterpret_cast<float*>(workspace);
    a.pb = a.pa + (size_t)TR_MAX_PART * C;
    const int nb = chan_blocks(a.P, C, &a.ppb);
    MSTG_LAUNCH(train_chan_partial_kernel<0>, dim3(nb), dim3(256), 0, st, a);
    MSTG_CHECK_LAUNCH("train_chan_partial_kernel<0>");
    MSTG_LAUNCH(train_bn_stats_final_kernel, dim3(C), dim3(64), 0, st, a.pa, a.pb, nb, a.P, a.ppb, C, eps, momentum, mean, rstd,
                running_mean, running_var);
    MSTG_CHECK_LAUNCH("train_bn_stats_final_kernel");
    const long long pieces = a.P * (C / 8);
    MSTG_LAUNCH(train_bn_apply_kernel, dim3(bn_ew_blocks(pieces, C / 8)), dim3(256), 0, st, a.z, mean, rstd, gamma, beta, reinterpret_cast<h16*>(y),
                pieces, C / 8, act);
    MSTG_CHECK_LAUNCH("train_bn_apply_kernel");
    return MSTG_OK;
}

extern "C" int mstg_f16_train_bn_bwd(const void* z, const void* dy, const float* gamma, const float* beta, const float* mean,
                                     const float* rstd, size_t P, int C, int act, const float* fstate, float* dgamma, float* dbeta,
                                     void* dz, void* workspace, size_t workspace_bytes, void* stream) {
    if (const char* e = chan_validate((long long)P, C)) return fail_arg(MSTG_E_UNSUPPORTED, e);
    if (!z || !dy || !gamma || !beta || !mean || !rstd || !fstate || !dgamma || !dbeta || !dz || !workspace)
        return fail_arg(MSTG_E_BADARG, "mstg_f16_train_bn_bwd: null pointer");
    if (act != MSTG_ACT_NONE && act != MSTG_ACT_RELU && act != MSTG_ACT_LEAKY02)
        return fail_arg(MSTG_E_UNSUPPORTED, "mstg_f16_train_bn_bwd: act must be none, ReLU or LeakyReLU(0.2)");
    if (workspace_bytes < chan_ws_bytes(C)) return fail_arg(MSTG_E_WORKSPACE, "mstg_f16_train_bn_bwd: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    ChanArgs a{};
    a.z = reinterpret_cast<const h16*>(z);
    a.dy = reinterpret_cast<const h16*>(dy);
    a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta;
    a.P = (long long)P;
    a.C = C;
    a.act = act;
    a.pa = reinterpret_cast<float*>(workspace);
    a.pb = a.pa + (size_t)TR_MAX_PART * C;
    float* sums = a.pb + (size_t)TR_MAX_PART * C;
    const int nb = chan_blocks(a.P, C, &a.ppb);
    MSTG_LAUNCH(train_chan_partial_kernel<1>, dim3(nb), dim3(256), 0, st, a);
    MSTG_CHECK_LAUNCH("train_chan_partial_kernel<1>");
    MSTG_LAUNCH(train_bn_bwd_final_kernel, dim3(C), dim3(64), 0, st, a.pa, a.pb, nb, C, fstate, sums, dgamma, dbeta);
    MSTG_CHECK_LAUNCH("train_bn_bwd_final_kernel");
    const long long pieces = a.P * (C / 8);
    MSTG_LAUNCH(train_bn_bwd_apply_kernel, dim3(bn_ew_blocks(pieces, C / 8)), dim3(256), 0, st, a.z, a.dy, mean, rstd, gamma, beta, sums,
                reinterpret_cast<h16*>(dz), pieces, C / 8, act, (float)(1.0 / (double)P));
    MSTG_CHECK_LAUNCH("train_bn_bwd_apply_kernel");
    return MSTG_OK;
}

extern "C" int mstg_f16_train_act_bwd(const void* a, const void* da, void* dz, size_t n, int act, void* stream) {
    if (!a || !da || !dz) return fail_arg(MSTG_E_BADARG, "mstg_f16_train_act_bwd: null pointer");
    if (n == 0 || n % 8) return fail_arg(MSTG_E_BADARG, "mstg_f16_train_act_bwd: the element count must be a positive multiple of 8");
    if (act != MSTG_ACT_RELU && act != MSTG_ACT_LEAKY02)
        return fail_arg(MSTG_E_UNSUPPORTED, "mstg_f16_train_act_bwd: act must be ReLU or LeakyReLU(0.2) (their outputs keep the input's sign)");
    const long long pieces = (long long)(n / 8);
    MSTG_LAUNCH(train_act_bwd_kernel, dim3(ew_blocks(pieces)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const h16*>(a),
                reinterpret_cast<const h16*>(da), reinterpret_cast<h16*>(dz), pieces, act);
    MSTG_CHECK_LAUNCH("train_act_bwd_kernel");
    return MSTG_OK;
}

extern "C" size_t mstg_f16_train_loss_workspace_bytes(int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1) {
        fail_arg(MSTG_E_UNSUPPORTED, "mstg_f16_train_loss: N, H, W must be positive");
        return 0;
    }
    return (size_t)(((long long)N * H * W + 255) / 256) * sizeof(float);
}

extern "C" int mstg_f16_train_head_loss_bwd(const void* y, const float* real, const float* mask, int N, int H, int W, const float* fstate,
                                            float* loss, void* dz, void* workspace, size_t workspace_bytes, void* stream) {
    if (!y || !real || !mask || !fstate || !loss || !dz || !workspace) return fail_arg(MSTG_E_BADARG, "mstg_f16_train_head_loss_bwd: null pointer");
    if (N < 1 || H < 1 || W < 1) return fail_arg(MSTG_E_BADARG, "mstg_f16_train_head_loss_bwd: N, H, W must be positive");
    const long long HW = (long long)H * W, npix = HW * N, nb = (npix + 255) / 256;
    if (nb >= (1ll << 31)) return fail_arg(MSTG_E_BADARG, "mstg_f16_train_head_loss_bwd: image too large");
    if (workspace_bytes < (size_t)nb * sizeof(float)) return fail_arg(MSTG_E_WORKSPACE, "mstg_f16_train_head_loss_bwd: workspace too small");
    const float inv_numel = (float)(1.0 / (3.0 * (double)npix));
    hipStream_t st = (hipStream_t)stream;
    MSTG_LAUNCH(train_head_loss_bwd_kernel, dim3((unsigned)nb), dim3(256), 0, st, reinterpret_cast<const h16*>(y), real, mask, npix, HW,
                fstate, inv_numel, reinterpret_cast<float*>(workspace), reinterpret_cast<h16*>(dz));
    MSTG_CHECK_LAUNCH("train_head_loss_bwd_kernel");
    MSTG_LAUNCH(train_loss_final_kernel, dim3(1), dim3(256), 0, st, reinterpret_cast<const float*>(workspace), nb, inv_numel, loss);
    MSTG_CHECK_LAUNCH("train_loss_final_kernel");
    return MSTG_OK;
}

extern "C" size_t mstg_f16_train_wgrad_workspace_bytes(int N, int h, int w, int Cs, int Cb, int CbOut) {
    if (const char* e = wgrad_validate(N, h, w, Cs, Cb, CbOut)) {
        fail_arg(MSTG_E_UNSUPPORTED, e);
        return 0;
    }
    const WgradPlan p = wgrad_plan(N, h, w, Cs, Cb);
    return (size_t)p.nslabs * 16 * Cs * CbOut * sizeof(float);
}

extern "C" int mstg_f16_train_wgrad(const void* S, const void* B, int N, int h, int w, int Cs, int Cb, int CbOut, const float* fstate,
                                    float* dW, void* workspace, size_t workspace_bytes, void* stream) {
    if (const char* e = wgrad_validate(N, h, w, Cs, Cb, CbOut)) return fail_arg(MSTG_E_UNSUPPORTED, e);
    if (!S || !B || !fstate || !dW || !workspace) return fail_arg(MSTG_E_BADARG, "mstg_f16_train_wgrad: null pointer");
    const WgradPlan p = wgrad_plan(N, h, w, Cs, Cb);
    if (workspace_bytes < (size_t)p.nslabs * 16 * Cs * CbOut * sizeof(float))
        return fail_arg(MSTG_E_WORKSPACE, "mstg_f16_train_wgrad: workspace smaller than mstg_f16_train_wgrad_workspace_bytes");
    WgradArgs a;
    a.S = reinterpret_cast<const h16*>(S);
    a.B = reinterpret_cast<const h16*>(B);
    a.part = reinterpret_cast<float*>(workspace);
    a.P = (long long)N * h * w;
    a.h = h; a.w = w; a.Cs = Cs; a.Cb = Cb; a.CbOut = CbOut;
    a.nts = p.nts; a.ntb = p.ntb; a.nchunks = p.nchunks; a.cps = p.cps;
    const unsigned grid = (unsigned)(p.nslabs * p.nts * p.ntb);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (p.NB == 2) rc = p.MS == 4 ? wgrad_launch<4, 2>(a, grid, st) : (p.MS == 2 ? wgrad_launch<2, 2>(a, grid, st) : wgrad_launch<1, 2>(a, grid, st));
    else rc = p.MS == 4 ? wgrad_launch<4, 1>(a, grid, st) : (p.MS == 2 ? wgrad_launch<2, 1>(a, grid, st) : wgrad_launch<1, 1>(a, grid, st));
    if (rc != MSTG_OK) return rc;
    MSTG_CHECK_LAUNCH("wgrad_f16_kernel");
    const size_t per = (size_t)16 * Cs * CbOut;
    MSTG_LAUNCH(wgrad_reduce_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, st, a.part, p.nslabs, Cs, CbOut, fstate, dW);
    MSTG_CHECK_LAUNCH("wgrad_reduce_kernel");
    return MSTG_OK;
}

extern "C" int mstg_f16_train_bias_grad(const void* dz, size_t P, int C, int Cvalid, const float* fstate, float* out, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    if (const char* e = chan_validate((long long)P, C)) return fail_arg(MSTG_E_UNSUPPORTED, e);
    if (!dz || !fstate || !out || !workspace) return fail_arg(MSTG_E_BADARG, "mstg_f16_train_bias_grad: null pointer");
    if (Cvalid < 1 || Cvalid > C) return fail_arg(MSTG_E_BADARG, "mstg_f16_train_bias_grad: Cvalid must be in 1..C");
    if (workspace_bytes < chan_ws_bytes(C)) return fail_arg(MSTG_E_WORKSPACE, "mstg_f16_train_bias_grad: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    ChanArgs a{};
    a.z = reinterpret_cast<const h16*>(dz);
    a.P = (long long)P;
    a.C = C;
    a.pa = reinterpret_cast<float*>(workspace);
    const int nb = chan_blocks(a.P, C, &a.ppb);
    MSTG_LAUNCH(train_chan_partial_kernel<2>, dim3(nb), dim3(256), 0, st, a);
    MSTG_CHECK_LAUNCH("train_chan_partial_kernel<2>");
    MSTG_LAUNCH(train_bias_final_kernel, dim3(C), dim3(64), 0, st, a.pa, nb, C, Cvalid, fstate, out);
    MSTG_CHECK_LAUNCH("train_bias_final_kernel");
    return MSTG_OK;
}

extern "C" int mstg_f16_train_scale_update(const float* norm, float* fstate, int* istate, void* stream) {
    if (!norm || !fstate || !istate) return fail_arg(MSTG_E_BADARG, "mstg_f16_train_scale_update: null pointer");
    MSTG_LAUNCH(train_scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, norm, fstate, istate);
    MSTG_CHECK_LAUNCH("train_scale_update_kernel");
    return MSTG_OK;
}

extern "C" int mstg_f16_train_adam(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                                   int step_base, const int* istate, void* stream) {
    if (!p || !g || !m || !v || !istate) return fail_arg(MSTG_E_BADARG, "mstg_f16_train_adam: null pointer");
    if (n == 0) return fail_arg(MSTG_E_BADARG, "mstg_f16_train_adam: empty buffer");
    if (step_base < 0) return fail_arg(MSTG_E_BADARG, "mstg_f16_train_adam: step_base must not be negative");
    const size_t nb = (n + 255) / 256;
    MSTG_LAUNCH(train_adam_kernel, dim3((unsigned)(nb > 4096 ? 4096 : nb)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1,
                beta2, eps, step_base, istate);
    MSTG_CHECK_LAUNCH("train_adam_kernel");
    return MSTG_OK;
}
