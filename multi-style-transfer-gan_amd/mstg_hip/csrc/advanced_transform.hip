// The five settings of the reference's advanced_transform.py (:129-311) between the forward pass and the encoder, on the device for a
// batch of (N, H, W, 3) uint8 RGB images: the 8-bit RGB <-> Lab round trip, OpenCV's 8-bit Gaussian for sigma > 0, the HSV gains,
// a deterministic K-means, the region blend and the multi-scale fusion, and the three chains built from them.  Every step is
// restated from the definition in include/mstg_hip.h (tests/advanced_transform_ref.py is the same restatement in numpy -- neither
// has been compared with an OpenCV binary).  Every kernel takes N images per launch:
//
// P  at_point_kernel<MODE>   one thread per pixel, all point-wise work of the file: RGB -> Lab, Lab -> RGB, the HSV gains, the region
//    blend (alone, or followed by the gains), and the two chain kernels: CONTRAST (Lab, the CLAHE interpolation of L, Lab -> RGB, the
//    gains) and DETAIL (the Gaussian's column pass, grey - blurred wrapping in 8 bits, L + 0.5 * detail, Lab -> RGB, the gains).
//    The Lab tables (16-bit, from the host) are read from global memory: 38 KB that every workgroup gathers from, resident in L2.
// T  at_clahe_lut_kernel     one workgroup per CLAHE tile: the histogram of L in LDS, then the shared tail (u8_image.h).
// H  at_gauss_row_kernel<RGB> one thread per pixel: the row pass in 8.8 fixed point, exact 16-bit sums; RGB: of the 8-bit grey.
// V  at_gauss_col_kernel     one thread per pixel: the column pass, (sum + 32768) >> 16.
// F  at_fuse_kernel          one thread per pixel: the float32 weighted sum of S scales.
// K-means (every launch covers all attempts of all images: a "problem" is one attempt of one image):
// I  km_init_kernel          clears the sums and flags, sets min = 255, max = 0.
// M  km_minmax_kernel        per image and channel min and max: a wave reduction, LDS, then six integer atomics a workgroup.
// C  km_centers_kernel       the initial centres lo + u * (hi - lo), or centers0.
// A  km_assign_kernel        the hot one: a workgroup takes 1024 pixels of one problem, a thread four of them; the centres are scalar
//    loads; per cluster n, sum c and sum c^2 are combined in registers (a run of equal labels), across a wave (when all lanes hold
//    one label), in LDS (32-bit integer atomics: 1024 pixels fit) and then go to the problem's sums with 64-bit integer atomics.
//    A frozen problem returns at once.
// U  km_update_kernel        one workgroup per problem: the new centres, the largest squared shift, the flag; clears the sums.
// S  km_select_kernel        one workgroup per image: the compactness of every attempt in float64, the smallest wins.
// L  km_label_kernel         one thread per pixel: the label under the winner's centres.
//
// No floating-point atomics; the device evaluates no exp, pow or cbrt.
#include <cmath>

#include "lanes.h"
#include "u8_image.h"

namespace mstg {

constexpr int AT_THREADS = 256;
constexpr int LI_FY = 0, LI_A = 256, LI_B = 512, LI_CUBE = 768, LI_CUBE_N = MSTG_LAB_INV_CUBE, LI_COEF = LI_CUBE + LI_CUBE_N;
constexpr int LI_GAMMA = LI_COEF + 9, LI_GAMMA_N = 8193;  // the inverse table (mstg_lab_inverse_tables)
static_assert(LI_GAMMA + LI_GAMMA_N <= MSTG_LAB_INV_TABLE_U16, "the inverse table holds fy, a, b, cube, the coefficients and the gamma");
constexpr int GS_MAX = MSTG_GAUSSIAN_SIGMA_MAX_KSIZE;
constexpr int KM_MAX = MSTG_KMEANS_MAX_K, KM_F = 7;  // sums per cluster: n, sum R, G, B, sum R^2, G^2, B^2
constexpr int KM_PX = 4, KM_TILE = AT_THREADS * KM_PX;
constexpr int FS_MAX = MSTG_FUSE_MAX_SCALES;

typedef unsigned long long u64;

struct Q8Taps {
    int k[GS_MAX];
};
struct Ratios {
    double r[KM_MAX], r1[KM_MAX];
    int count;
};
struct FuseWeights {
    float w[FS_MAX];
};

// ---- Lab ------------------------------------------------------------------------------------------------------------------------
// (lab_px, RGB -> Lab, is in u8_image.h: quickshift.hip uses it too)
// f (scale 32768) -> the linear value (scale 8192): two neighbouring entries of the table, interpolated linearly
__device__ __forceinline__ int lab_cube(int f, const unsigned short* __restrict__ cube) {
    f = min(max(f, 0), 8 * (LI_CUBE_N - 1) - 1);
    const int i = f >> 3, lo = cube[i], hi = cube[i + 1];
    return lo + (((hi - lo) * (f & 7) + 4) >> 3);
}

// L, a, b (packed) -> RGB (packed): this build's integer path, defined for every byte triple
__device__ __forceinline__ unsigned lab2rgb_px(unsigned q, const unsigned short* __restrict__ t) {
    const int fy = t[LI_FY + (q & 0xffu)];
    const int fx = fy + (short)t[LI_A + ((q >> 8) & 0xffu)];
    const int fz = fy - (short)t[LI_B + (q >> 16)];
    const int gx = lab_cube(fx, t + LI_CUBE), gy = lab_cube(fy, t + LI_CUBE), gz = lab_cube(fz, t + LI_CUBE);
    unsigned out = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int c0 = (short)t[LI_COEF + 3 * ch], c1 = (short)t[LI_COEF + 3 * ch + 1], c2 = (short)t[LI_COEF + 3 * ch + 2];
        const int lin = (c0 * gx + c1 * gy + c2 * gz + 2048) >> 12;  // below 2^31: |c| <= 13273, g <= 36160
        out |= (unsigned)t[LI_GAMMA + min(max(lin, 0), LI_GAMMA_N - 1)] << (8 * ch);
    }
    return out;
}

// the HSV gains on a packed pixel: 8-bit RGB -> HSV, cv2.multiply of s and of v, HSV -> RGB
__device__ __forceinline__ unsigned hsv_gain_px(unsigned q, const int* sdiv, const int* hdiv, float s_gain, float v_gain) {
    int h, s, v;
    hsv_px(q, sdiv, hdiv, h, s, v);
    return hsv2rgb_px(h, gain_u8(s, s_gain), gain_u8(v, v_gain));
}

enum PointMode { PM_LAB, PM_LAB2RGB, PM_GAIN, PM_BLEND, PM_BLEND_GAIN, PM_CONTRAST, PM_DETAIL };

struct PointArgs {
    const unsigned char* a;      // the image (styled)
    const unsigned char* b;      // the original (BLEND*, DETAIL)
    const int* labels;           // BLEND*
    const unsigned short* lab;   // forward table
    const unsigned short* inv;   // inverse table
    const unsigned char* luts;   // CONTRAST: the CLAHE tables of L
    const unsigned short* rows;  // DETAIL: the row pass of the grey of b
    float s_gain, v_gain;
    int H, W, ksize;
    size_t total;
    unsigned char* out;
};

template <int MODE>
__global__ __launch_bounds__(AT_THREADS) void at_point_kernel(const PointArgs p, const Ratios ratios, const Q8Taps taps) {
#pragma clang fp contract(off)
    constexpr bool GAIN = MODE == PM_GAIN || MODE == PM_BLEND_GAIN || MODE == PM_CONTRAST || MODE == PM_DETAIL;
    __shared__ int sdiv[256], hdiv[256];
    const int tid = threadIdx.x;
    if (GAIN) {
        sdiv[tid] = div_rhe(255 << 12, tid);
        hdiv[tid] = div_rhe(122880, tid);
        __syncthreads();
    }
    const size_t idx = (size_t)blockIdx.x * AT_THREADS + tid;
    if (idx >= p.total) return;
    unsigned q = load_px(p.a + idx * 3);
    if (MODE == PM_LAB) q = lab_px(q, p.lab);
    if (MODE == PM_LAB2RGB) q = lab2rgb_px(q, p.inv);
    if (MODE == PM_BLEND || MODE == PM_BLEND_GAIN) {
        const int l = p.labels[idx];
        if (l < 0) {
            q = 0;  // no region: the reference's sum over the regions leaves 0
        } else {
            const int k = min(l, ratios.count - 1);
            const unsigned o = load_px(p.b + idx * 3);
            const double r = ratios.r[k], r1 = ratios.r1[k];
            q = blend_byte(q & 0xffu, o & 0xffu, r, r1) | blend_byte((q >> 8) & 0xffu, (o >> 8) & 0xffu, r, r1) << 8 |
                blend_byte(q >> 16, o >> 16, r, r1) << 16;
        }
    }
    if (MODE == PM_CONTRAST || MODE == PM_DETAIL) {
        const size_t hw = (size_t)p.H * p.W;
        const size_t n = idx / hw;
        const int rem = (int)(idx - n * hw), y = rem / p.W, x = rem - y * p.W;
        q = lab_px(q, p.lab);
        int L = q & 0xffu;
        if (MODE == PM_CONTRAST) {
            const float inv_th = __fdiv_rn(1.0f, (float)(p.H / MSTG_CLAHE_TILES)), inv_tw = __fdiv_rn(1.0f, (float)(p.W / MSTG_CLAHE_TILES));
            L = clahe_px(p.luts + n * MSTG_CLAHE_TILES * MSTG_CLAHE_TILES * 256, L, y, x, inv_th, inv_tw);
        } else {
            const unsigned short* col = p.rows + n * hw + x;
            const int r = p.ksize >> 1;
            unsigned sum = 0;
            for (int k = 0; k < p.ksize; ++k) sum += (unsigned)taps.k[k] * col[(size_t)reflect101(y + k - r, p.H) * p.W];
            const int blurred = (int)((sum + 32768u) >> 16);
            const int detail = (gray_px(load_px(p.b + idx * 3)) - blurred) & 0xff;  // uint8 - uint8 wraps
            float f = (float)L + (float)detail * 0.5f;                             // both exact
            f = f < 0.f ? 0.f : (f > 255.f ? 255.f : f);
            L = (int)f;  // truncated
        }
        q = lab2rgb_px((q & 0xffff00u) | (unsigned)L, p.inv);
    }
    if (GAIN) q = hsv_gain_px(q, sdiv, hdiv, p.s_gain, p.v_gain);
    p.out[idx * 3] = (unsigned char)(q & 0xffu);
    p.out[idx * 3 + 1] = (unsigned char)((q >> 8) & 0xffu);
    p.out[idx * 3 + 2] = (unsigned char)(q >> 16);
}

// ---- T: the CLAHE tables of L ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AT_THREADS) void at_clahe_lut_kernel(const unsigned char* __restrict__ in, const unsigned short* __restrict__ lab, int H,
                                                                  int W, unsigned char* __restrict__ luts) {
    __shared__ int hist[256], scan[256];
    __shared__ int excess;
    const int tid = threadIdx.x;
    constexpr int T = MSTG_CLAHE_TILES;
    const int n = blockIdx.x / (T * T), tile = blockIdx.x - n * T * T;
    const int ty = tile / T, tx = tile - ty * T;
    const int th = H / T, tw = W / T, area = th * tw;
    const unsigned char* img = in + (size_t)n * H * W * 3;
    hist[tid] = 0;
    if (tid == 0) excess = 0;
    __syncthreads();
    for (int e = tid; e < area; e += AT_THREADS) {
        const int r = e / tw, c = e - r * tw;
        const size_t at = (size_t)(ty * th + r) * W + tx * tw + c;
        atomicAdd(&hist[lab_px(load_px(img + at * 3), lab) & 0xffu], 1);
    }
    __syncthreads();
    clahe_tile_lut(tid, area, hist, scan, &excess, luts + (size_t)blockIdx.x * 256);
}

// ---- H, V: the 8-bit Gaussian ---------------------------------------------------------------------------------------------------------
template <bool RGB>
__global__ __launch_bounds__(AT_THREADS) void at_gauss_row_kernel(const unsigned char* __restrict__ in, const Q8Taps taps, int ksize, int H, int W,
                                                                  size_t total, unsigned short* __restrict__ rows) {
    const size_t idx = (size_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t line = idx / W;  // n * H + y
    const int x = (int)(idx - line * W), r = ksize >> 1;
    const unsigned char* src = in + line * W * (RGB ? 3 : 1);
    unsigned sum = 0;  // at most 256 * 255
    for (int k = 0; k < ksize; ++k) {
        const int sx = reflect101(x + k - r, W);
        const unsigned v = RGB ? (unsigned)gray_px(load_px(src + (size_t)sx * 3)) : (unsigned)src[sx];
        sum += (unsigned)taps.k[k] * v;
    }
    rows[idx] = (unsigned short)sum;
}

__global__ __launch_bounds__(AT_THREADS) void at_gauss_col_kernel(const unsigned short* __restrict__ rows, const Q8Taps taps, int ksize, int H,
                                                                  int W, size_t total, unsigned char* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t hw = (size_t)H * W;
    const size_t n = idx / hw;
    const int rem = (int)(idx - n * hw), y = rem / W, x = rem - y * W, r = ksize >> 1;
    const unsigned short* col = rows + n * hw + x;
    unsigned sum = 0;  // at most 256 * 65280
    for (int k = 0; k < ksize; ++k) sum += (unsigned)taps.k[k] * col[(size_t)reflect101(y + k - r, H) * W];
    out[idx] = (unsigned char)((sum + 32768u) >> 16);
}

// ---- F: the fusion of scales ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AT_THREADS) void at_fuse_kernel(const unsigned char* __restrict__ in, int S, size_t bytes, const FuseWeights w,
                                                             float gain, unsigned char* __restrict__ out) {
#pragma clang fp contract(off)  // numpy rounds every operation
    const size_t idx = (size_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (idx >= bytes) return;
    float f = 0.f;
    for (int s = 0; s < S; ++s) {
        const float x = __fdiv_rn((float)in[(size_t)s * bytes + idx], 255.0f);
        f = f + x * w.w[s];
    }
    f = f * gain;
    f = f < 0.f ? 0.f : (f > 1.f ? 1.f : f);
    if (!(f == f)) f = 0.f;  // a NaN weight: keep the byte defined
    out[idx] = (unsigned char)(f * 255.0f);
}

// ---- K-means ----------------------------------------------------------------------------------------------------------------------
// workspace of P = N * attempts problems: centres float [P][KM_MAX][3], sums u64 [P][KM_MAX][KM_F], flag int [P], range int [N][6]
struct KmWorkspace {
    size_t sums, centres, flags, range, total;
};
static KmWorkspace km_workspace(int N, int attempts) {
    const size_t P = (size_t)N * attempts;
    KmWorkspace w;
    w.sums = 0;
    w.centres = align16(P * KM_MAX * KM_F * sizeof(u64));
    w.flags = w.centres + align16(P * KM_MAX * 3 * sizeof(float));
    w.range = w.flags + align16(P * sizeof(int));
    w.total = w.range + align16((size_t)N * 6 * sizeof(int));
    return w;
}

__global__ __launch_bounds__(AT_THREADS) void km_init_kernel(u64* __restrict__ sums, size_t n_sums, int* __restrict__ flags, size_t n_flags,
                                                             int* __restrict__ range, size_t n_range) {
    const size_t idx = (size_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (idx < n_sums) sums[idx] = 0;
    if (idx < n_flags) flags[idx] = 0;
    if (idx < n_range) range[idx] = (idx % 6) < 3 ? 255 : 0;  // min R, G, B, then max R, G, B
}

__global__ __launch_bounds__(AT_THREADS) void km_minmax_kernel(const unsigned char* __restrict__ img, size_t hw, int tiles, int* __restrict__ range) {
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    const unsigned char* src = img + (size_t)n * hw * 3;
    __shared__ int wg[6];
    if (threadIdx.x < 6) wg[threadIdx.x] = threadIdx.x < 3 ? 255 : 0;
    __syncthreads();
    int lo[3] = {255, 255, 255}, hi[3] = {0, 0, 0};
#pragma unroll
    for (int j = 0; j < KM_PX; ++j) {
        const size_t at = (size_t)tile * KM_TILE + j * AT_THREADS + threadIdx.x;
        if (at < hw) {
            const unsigned q = load_px(src + at * 3);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int v = (q >> (8 * c)) & 0xff;
                lo[c] = min(lo[c], v);
                hi[c] = max(hi[c], v);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo[c] = min(lo[c], __shfl_xor(lo[c], o, WAVE));
            hi[c] = max(hi[c], __shfl_xor(hi[c], o, WAVE));
        }
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {  // the four waves meet in LDS
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            atomicMin(&wg[c], lo[c]);
            atomicMax(&wg[3 + c], hi[c]);
        }
    }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&range[n * 6 + threadIdx.x], wg[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(&range[n * 6 + threadIdx.x], wg[threadIdx.x]);
}

__global__ __launch_bounds__(AT_THREADS) void km_centers_kernel(const int* __restrict__ range, const float* __restrict__ uniforms,
                                                                const float* __restrict__ centers0, int K, int attempts, size_t total,
                                                                float* __restrict__ centres) {
#pragma clang fp contract(off)
    const size_t idx = (size_t)blockIdx.x * AT_THREADS + threadIdx.x;  // (problem, k, channel)
    if (idx >= total) return;
    const int c = (int)(idx % 3), k = (int)(idx / 3 % K);
    const size_t prob = idx / 3 / K;
    const size_t n = prob / attempts;
    const int a = (int)(prob - n * attempts);
    float v;
    if (centers0) {
        v = centers0[(n * K + k) * 3 + c];  // attempts == 1
    } else {
        const float lo = (float)range[n * 6 + c], hi = (float)range[n * 6 + 3 + c];
        const float span = hi - lo;
        const float step = uniforms[((size_t)a * K + k) * 3 + c] * span;
        v = lo + step;
    }
    centres[(prob * KM_MAX + k) * 3 + c] = v;
}

// the label of a pixel: the nearest centre in float32, ((dx^2 + dy^2) + dz^2), the lowest index wins a tie
__device__ __forceinline__ int km_nearest(unsigned q, const float* __restrict__ cen, int K) {
#pragma clang fp contract(off)
    const float R = (float)(q & 0xffu), G = (float)((q >> 8) & 0xffu), B = (float)(q >> 16);
    int best = 0;
    float bd = 0.f;
    for (int k = 0; k < K; ++k) {
        const float dx = R - cen[3 * k], dy = G - cen[3 * k + 1], dz = B - cen[3 * k + 2];
        const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
        const float d = (xx + yy) + zz;
        if (k == 0 || d < bd) {
            bd = d;
            best = k;
        }
    }
    return best;
}

struct KmRun {
    int label;
    unsigned f[KM_F];
};

__device__ __forceinline__ void km_flush(const KmRun& r, unsigned* acc) {
    if (r.label < 0) return;
#pragma unroll
    for (int k = 0; k < KM_F; ++k)
        if (r.f[k]) atomicAdd(&acc[r.label * KM_F + k], r.f[k]);
}

// final: every problem is assigned (the sums of the compactness); otherwise a frozen problem is skipped
__global__ __launch_bounds__(AT_THREADS) void km_assign_kernel(const unsigned char* __restrict__ img, size_t hw, int tiles, int K, int attempts,
                                                               int final, const float* __restrict__ centres, const int* __restrict__ flags,
                                                               u64* __restrict__ sums) {
    __shared__ unsigned acc[KM_MAX * KM_F];
    const int tid = threadIdx.x;
    const int prob = blockIdx.x / tiles, tile = blockIdx.x - prob * tiles;
    if (!final && flags[prob]) return;  // uniform: the whole workgroup leaves
    const int n = prob / attempts;
    const unsigned char* src = img + (size_t)n * hw * 3;
    const float* cen = centres + (size_t)prob * KM_MAX * 3;  // uniform address: scalar loads
    if (tid < KM_MAX * KM_F) acc[tid] = 0;
    __syncthreads();
    KmRun run;
    run.label = -1;
#pragma unroll
    for (int k = 0; k < KM_F; ++k) run.f[k] = 0;
    bool clean = true;  // one run of four existing pixels
#pragma unroll
    for (int j = 0; j < KM_PX; ++j) {
        const size_t at = (size_t)tile * KM_TILE + (size_t)tid * KM_PX + j;
        if (at >= hw) {
            clean = false;
            continue;
        }
        const unsigned q = load_px(src + at * 3);
        const int l = km_nearest(q, cen, K);
        if (l != run.label) {
            if (j > 0) clean = false;
            km_flush(run, acc);
            run.label = l;
#pragma unroll
            for (int k = 0; k < KM_F; ++k) run.f[k] = 0;
        }
        const unsigned R = q & 0xffu, G = (q >> 8) & 0xffu, B = q >> 16;
        run.f[0] += 1;
        run.f[1] += R;
        run.f[2] += G;
        run.f[3] += B;
        run.f[4] += R * R;
        run.f[5] += G * G;
        run.f[6] += B * B;
    }
    const int first = __builtin_amdgcn_readfirstlane(run.label);
    if (__all(clean && run.label == first)) {  // the interior of a cluster: the wave adds its lanes up, one lane goes on
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int k = 0; k < KM_F; ++k) run.f[k] += __shfl_xor(run.f[k], o, WAVE);  // 256 pixels: every sum fits 32 bits
        if ((tid & (WAVE - 1)) == 0) km_flush(run, acc);
    } else {
        km_flush(run, acc);
    }
    __syncthreads();
    if (tid < K * KM_F) {  // 1024 pixels: every sum fits 32 bits (at most 1024 * 255^2)
        const unsigned v = acc[tid];
        if (v) atomicAdd(&sums[(size_t)prob * KM_MAX * KM_F + tid], (u64)v);
    }
}

__global__ __launch_bounds__(WAVE) void km_update_kernel(u64* __restrict__ sums, float* __restrict__ centres, int* __restrict__ flags, int K,
                                                         double eps2) {
#pragma clang fp contract(off)
    __shared__ double shift[KM_MAX];
    const int prob = blockIdx.x, k = threadIdx.x;
    if (flags[prob]) return;  // uniform
    if (k < K) {
        u64* s = sums + ((size_t)prob * KM_MAX + k) * KM_F;
        float* c = centres + ((size_t)prob * KM_MAX + k) * 3;
        const u64 n = s[0];
        double sh = 0.0;
        if (n != 0) {  // an empty cluster keeps its centre
            double d[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float nc = (float)((double)s[1 + ch] / (double)n);
                d[ch] = (double)nc - (double)c[ch];
                c[ch] = nc;
            }
            const double xx = d[0] * d[0], yy = d[1] * d[1], zz = d[2] * d[2];
            sh = (xx + yy) + zz;
        }
        shift[k] = sh;
#pragma unroll
        for (int f = 0; f < KM_F; ++f) s[f] = 0;
    }
    __syncthreads();
    if (k == 0) {
        double m = 0.0;
        for (int i = 0; i < K; ++i) m = shift[i] > m ? shift[i] : m;
        if (m <= eps2) flags[prob] = 1;
    }
}

__global__ __launch_bounds__(WAVE) void km_select_kernel(const u64* __restrict__ sums, const float* __restrict__ centres, int K, int attempts,
                                                         float* __restrict__ out_centres, double* __restrict__ compactness,
                                                         int* __restrict__ best) {
#pragma clang fp contract(off)
    __shared__ double comp[MSTG_KMEANS_MAX_ATTEMPTS];
    __shared__ int winner;
    const int n = blockIdx.x, a = threadIdx.x;
    if (a < attempts) {
        const size_t prob = (size_t)n * attempts + a;
        double total = 0.0;
        for (int k = 0; k < K; ++k) {
            const u64* s = sums + (prob * KM_MAX + k) * KM_F;
            const double cnt = (double)s[0];
            for (int ch = 0; ch < 3; ++ch) {
                const double c = (double)centres[(prob * KM_MAX + k) * 3 + ch];
                const double twice = 2.0 * c;
                const double cross = twice * (double)s[1 + ch];
                const double nc = cnt * c;
                const double sq = nc * c;
                const double t = ((double)s[4 + ch] - cross) + sq;
                total = total + t;
            }
        }
        comp[a] = total;
    }
    __syncthreads();
    if (a == 0) {
        int w = 0;
        for (int i = 1; i < attempts; ++i)
            if (comp[i] < comp[w]) w = i;  // the lowest attempt wins a tie
        winner = w;
        best[n] = w;
        compactness[n] = comp[w];
    }
    __syncthreads();
    if (a < K * 3) out_centres[(size_t)n * K * 3 + a] = centres[((size_t)n * attempts + winner) * KM_MAX * 3 + a];
}

__global__ __launch_bounds__(AT_THREADS) void km_label_kernel(const unsigned char* __restrict__ img, size_t hw, size_t total, int K, int attempts,
                                                              const float* __restrict__ centres, const int* __restrict__ best,
                                                              int* __restrict__ labels) {
    const size_t idx = (size_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t n = idx / hw;
    const float* cen = centres + (n * attempts + best[n]) * KM_MAX * 3;
    labels[idx] = km_nearest(load_px(img + idx * 3), cen, K);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static dim3 at_grid(size_t items) { return dim3((unsigned)cdivz(items, (size_t)AT_THREADS)); }

static int at_shape(const char* who, int N, int H, int W) {
    const int rc = check_extent(who, N, H, W);
    if (rc != MSTG_OK) return rc;
    const long long px = (long long)N * H * W;  // the finest grid: a thread per byte of the fusion, else per pixel
    return check_grid(who, (px * 3 + AT_THREADS - 1) / AT_THREADS, 31, "N * H * W * 3", px * 3);
}

static int at_clahe_shape(const char* who, int N, int H, int W) {
    const int rc = at_shape(who, N, H, W);
    if (rc != MSTG_OK) return rc;
    if (H % MSTG_CLAHE_TILES == 0 && W % MSTG_CLAHE_TILES == 0) return MSTG_OK;
    char msg[220];
    snprintf(msg, sizeof(msg), "%s: H = %d, W = %d: CLAHE with %d x %d tiles is built for sizes that are multiples of %d (OpenCV pads others)", who,
             H, W, MSTG_CLAHE_TILES, MSTG_CLAHE_TILES, MSTG_CLAHE_TILES);
    return fail_arg(MSTG_E_UNSUPPORTED, msg);
}

static int at_ksize(const char* who, int ksize) {
    if (ksize >= 1 && ksize <= GS_MAX && (ksize & 1)) return MSTG_OK;
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: ksize = %d is not built: the 8.8 fixed-point Gaussian takes the odd sizes 1 to %d (sigma up to 5)", who, ksize,
             GS_MAX);
    return fail_arg(MSTG_E_UNSUPPORTED, msg);
}

static int at_taps(const char* who, const int* taps, int ksize, Q8Taps& t) {
    int sum = 0;
    for (int k = 0; k < GS_MAX; ++k) {
        t.k[k] = k < ksize ? taps[k] : 0;
        if (t.k[k] < 0) return fail_arg(MSTG_E_BADARG, "gaussian taps: a negative tap (the 16-bit row sums would not be exact)");
        sum += t.k[k];
    }
    if (sum == 256) return MSTG_OK;
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: the taps sum to %d, not to 256", who, sum);
    return fail_arg(MSTG_E_BADARG, msg);
}

static int at_ratios(const char* who, const double* ratios, int count, Ratios& r) {
#pragma clang fp contract(off)
    if (!ratios || count < 1 || count > KM_MAX) {
        char msg[160];
        snprintf(msg, sizeof(msg), "%s: ratios = %s, count = %d: need 1 to %d ratios", who, ratios ? "set" : "null", count, KM_MAX);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    r.count = count;
    for (int k = 0; k < KM_MAX; ++k) {
        r.r[k] = ratios[k < count ? k : count - 1];
        r.r1[k] = 1.0 - r.r[k];  // the reference's (1 - blend_ratio), a double subtraction
    }
    return MSTG_OK;
}

static PointArgs at_args(const unsigned char* a, int N, int H, int W, unsigned char* out) {
    PointArgs p;
    memset(&p, 0, sizeof(p));
    p.a = a;
    p.H = H;
    p.W = W;
    p.total = (size_t)N * H * W;
    p.s_gain = p.v_gain = 1.f;
    p.out = out;
    return p;
}

template <int MODE>
static int at_point(const PointArgs& p, const Ratios& r, const Q8Taps& t, hipStream_t st) {
    MSTG_LAUNCH(at_point_kernel<MODE>, at_grid(p.total), dim3(AT_THREADS), 0, st, p, r, t);
    MSTG_CHECK_LAUNCH("at_point_kernel");
    return MSTG_OK;
}

static int at_gauss_rows(const unsigned char* in, bool rgb, const Q8Taps& t, int ksize, int N, int H, int W, unsigned short* rows, hipStream_t st) {
    const size_t px = (size_t)N * H * W;
    if (rgb)
        MSTG_LAUNCH(at_gauss_row_kernel<true>, at_grid(px), dim3(AT_THREADS), 0, st, in, t, ksize, H, W, px, rows);
    else
        MSTG_LAUNCH(at_gauss_row_kernel<false>, at_grid(px), dim3(AT_THREADS), 0, st, in, t, ksize, H, W, px, rows);
    MSTG_CHECK_LAUNCH("at_gauss_row_kernel");
    return MSTG_OK;
}

static int km_params(const char* who, int K, int attempts, int iters) {
    char msg[200];
    if (K < 1 || K > KM_MAX) {
        snprintf(msg, sizeof(msg), "%s: K = %d is not built: this build takes K from 1 to %d", who, K, KM_MAX);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    if (attempts < 1 || attempts > MSTG_KMEANS_MAX_ATTEMPTS) {
        snprintf(msg, sizeof(msg), "%s: attempts = %d is not built: this build takes 1 to %d attempts", who, attempts, MSTG_KMEANS_MAX_ATTEMPTS);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    if (iters < 1 || iters > MSTG_KMEANS_MAX_ITERS) {
        snprintf(msg, sizeof(msg), "%s: iters = %d is not built: this build takes 1 to %d iterations", who, iters, MSTG_KMEANS_MAX_ITERS);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    return MSTG_OK;
}

static int km_shape(const char* who, int N, int H, int W, int attempts) {
    const int rc = at_shape(who, N, H, W);
    if (rc != MSTG_OK) return rc;
    const long long tiles = ((long long)H * W + KM_TILE - 1) / KM_TILE;
    return check_grid(who, (long long)N * attempts * tiles, 31, "N * attempts * tiles", (long long)N * attempts * tiles);
}

}  // namespace mstg

using namespace mstg;

extern "C" int mstg_lab_inverse_tables(unsigned short* table) {
    if (!table) return fail_arg(MSTG_E_BADARG, "lab_inverse_tables: null table pointer");
    for (int e = 0; e < MSTG_LAB_INV_TABLE_U16; ++e) table[e] = 0;
    for (int v = 0; v < 256; ++v) {
        const double L = v * 100.0 / 255.0;
        const double fy = L <= 8.0 ? 7.787 * (L / 903.3) + 16.0 / 116.0 : (L + 16.0) / 116.0;
        table[LI_FY + v] = (unsigned short)std::lrint(32768.0 * fy);
        table[LI_A + v] = (unsigned short)(short)std::lrint(32768.0 * (v - 128) / 500.0);
        table[LI_B + v] = (unsigned short)(short)std::lrint(32768.0 * (v - 128) / 200.0);
    }
    for (int i = 0; i < LI_CUBE_N; ++i) {
        const double t = i * 8.0 / 32768.0;
        const double g = t > 6.0 / 29.0 ? t * t * t : (t - 16.0 / 116.0) / 7.787;
        table[LI_CUBE + i] = (unsigned short)std::lrint(8192.0 * (g > 0.0 ? g : 0.0));
    }
    const double m[3][3] = {{3.240479, -1.53715, -0.498535}, {-0.969256, 1.875991, 0.041556}, {0.055648, -0.204043, 1.057311}};
    const double white[3] = {0.950456, 1.0, 1.088754};
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) table[LI_COEF + 3 * r + k] = (unsigned short)(short)std::lrint(4096.0 * m[r][k] * white[k]);
    for (int i = 0; i < LI_GAMMA_N; ++i) {
        const double x = i / 8192.0;
        const double enc = x <= 0.0031308 ? 12.92 * x : 1.055 * std::pow(x, 1.0 / 2.4) - 0.055;
        table[LI_GAMMA + i] = (unsigned short)std::lrint(255.0 * enc);
    }
    return MSTG_OK;
}

extern "C" int mstg_gaussian_sigma_taps(double sigma, int* taps, double* margin) {
#pragma clang fp contract(off)
    if (!taps) return fail_arg(MSTG_E_BADARG, "gaussian_sigma_taps: null taps pointer");
    if (!(sigma > 0) || !(sigma < 1e6)) {
        char msg[160];
        snprintf(msg, sizeof(msg), "gaussian_sigma_taps: sigma = %g: need sigma > 0 (sigma <= 0 with a given size is mstg_gaussian_u8)", sigma);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    const int ksize = (int)std::nearbyint(sigma * 6 + 1) | 1;  // cvRound: round half to even
    const int rc = at_ksize("gaussian_sigma_taps", ksize);
    if (rc != MSTG_OK) return rc;
    const int r = ksize / 2;
    double t[GS_MAX], total = 0.0;
    for (int i = 0; i < ksize; ++i) {
        const double x = (double)(i - r);
        t[i] = std::exp(-0.5 * (x * x) / (sigma * sigma));
        total += t[i];  // left to right
    }
    double err = 0.0, worst = 1.0;
    int sum = 0;
    for (int i = 0; i < GS_MAX; ++i) taps[i] = 0;
    for (int i = 0; i < r; ++i) {
        const double a = t[i] / total * 256 + err;
        const double q = std::nearbyint(a);
        const double dist = std::fabs(std::fabs(a - std::floor(a)) - 0.5);
        worst = dist < worst ? dist : worst;
        err = a - q;
        taps[i] = taps[ksize - 1 - i] = (int)q;
        sum += (int)q;
    }
    taps[r] = 256 - 2 * sum;
    if (margin) *margin = worst;
    return ksize;
}

extern "C" int mstg_lab_u8(const unsigned char* in, int N, int H, int W, const unsigned short* lab_table, unsigned char* out, void* stream) {
    if (!in || !lab_table || !out) return fail_arg(MSTG_E_BADARG, "lab_u8: null in, table or out pointer");
    const int rc = at_shape("lab_u8", N, H, W);
    if (rc != MSTG_OK) return rc;
    if ((uintptr_t)lab_table & 1) return fail_arg(MSTG_E_ALIGN, "lab_u8: table not 2-byte aligned");
    const size_t nb = (size_t)N * H * W * 3;
    if (overlaps(out, nb, in, nb) || overlaps(out, nb, lab_table, 2 * MSTG_LAB_TABLE_U16)) return fail_arg(MSTG_E_BADARG, "lab_u8: out overlaps the input or the table");
    PointArgs p = at_args(in, N, H, W, out);
    p.lab = lab_table;
    return at_point<PM_LAB>(p, Ratios{}, Q8Taps{}, (hipStream_t)stream);
}

extern "C" int mstg_lab2rgb_u8(const unsigned char* in, int N, int H, int W, const unsigned short* inv_table, unsigned char* out, void* stream) {
    if (!in || !inv_table || !out) return fail_arg(MSTG_E_BADARG, "lab2rgb_u8: null in, table or out pointer");
    const int rc = at_shape("lab2rgb_u8", N, H, W);
    if (rc != MSTG_OK) return rc;
    if ((uintptr_t)inv_table & 1) return fail_arg(MSTG_E_ALIGN, "lab2rgb_u8: table not 2-byte aligned");
    const size_t nb = (size_t)N * H * W * 3;
    if (overlaps(out, nb, in, nb) || overlaps(out, nb, inv_table, 2 * MSTG_LAB_INV_TABLE_U16))
        return fail_arg(MSTG_E_BADARG, "lab2rgb_u8: out overlaps the input or the table");
    PointArgs p = at_args(in, N, H, W, out);
    p.inv = inv_table;
    return at_point<PM_LAB2RGB>(p, Ratios{}, Q8Taps{}, (hipStream_t)stream);
}

extern "C" int mstg_gaussian_sigma_u8(const unsigned char* in, int N, int H, int W, const int* taps, int ksize, unsigned char* out, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    int rc = at_ksize("gaussian_sigma_u8", ksize);  // first: the refusal does not depend on the buffers
    if (rc != MSTG_OK) return rc;
    if (!in || !taps || !out) return fail_arg(MSTG_E_BADARG, "gaussian_sigma_u8: null in, taps or out pointer");
    rc = at_shape("gaussian_sigma_u8", N, H, W);
    if (rc != MSTG_OK) return rc;
    Q8Taps t;
    rc = at_taps("gaussian_sigma_u8", taps, ksize, t);
    if (rc != MSTG_OK) return rc;
    const size_t px = (size_t)N * H * W, need = px * 2;
    if (!workspace || workspace_bytes < need) return fail_arg(MSTG_E_WORKSPACE, "gaussian_sigma_u8: workspace too small (N * H * W * 2 bytes)");
    if ((uintptr_t)workspace & 1) return fail_arg(MSTG_E_ALIGN, "gaussian_sigma_u8: workspace not 2-byte aligned");
    if (overlaps(out, px, in, px) || overlaps(out, px, workspace, need) || overlaps(workspace, need, in, px))
        return fail_arg(MSTG_E_BADARG, "gaussian_sigma_u8: out or workspace overlaps the input or each other");
    hipStream_t st = (hipStream_t)stream;
    rc = at_gauss_rows(in, false, t, ksize, N, H, W, (unsigned short*)workspace, st);
    if (rc != MSTG_OK) return rc;
    MSTG_LAUNCH(at_gauss_col_kernel, at_grid(px), dim3(AT_THREADS), 0, st, (const unsigned short*)workspace, t, ksize, H, W, px, out);
    MSTG_CHECK_LAUNCH("at_gauss_col_kernel");
    return MSTG_OK;
}

extern "C" int mstg_hsv_gain_u8(const unsigned char* in, int N, int H, int W, float s_gain, float v_gain, unsigned char* out, void* stream) {
    if (!in || !out) return fail_arg(MSTG_E_BADARG, "hsv_gain_u8: null in or out pointer");
    const int rc = at_shape("hsv_gain_u8", N, H, W);
    if (rc != MSTG_OK) return rc;
    if (!(s_gain >= 0.f) || !(v_gain >= 0.f)) {
        char msg[160];
        snprintf(msg, sizeof(msg), "hsv_gain_u8: s_gain = %g, v_gain = %g: a gain must be a number >= 0", (double)s_gain, (double)v_gain);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    const size_t nb = (size_t)N * H * W * 3;
    if (overlaps(out, nb, in, nb)) return fail_arg(MSTG_E_BADARG, "hsv_gain_u8: out overlaps the input");
    PointArgs p = at_args(in, N, H, W, out);
    p.s_gain = s_gain;
    p.v_gain = v_gain;
    return at_point<PM_GAIN>(p, Ratios{}, Q8Taps{}, (hipStream_t)stream);
}

extern "C" size_t mstg_kmeans_workspace_bytes(int N, int K, int attempts) {
    if (N < 1) {
        fail_arg(MSTG_E_BADARG, "kmeans_workspace_bytes: N < 1");
        return 0;
    }
    if (km_params("kmeans_workspace_bytes", K, attempts, 1) != MSTG_OK) return 0;
    return km_workspace(N, attempts).total;
}

extern "C" int mstg_kmeans_u8(const unsigned char* img, int N, int H, int W, int K, int attempts, int iters, double eps, const float* uniforms,
                              const float* centers0, int* labels, float* centers, double* compactness, int* best, void* workspace,
                              size_t workspace_bytes, void* stream) {
    int rc = km_params("kmeans_u8", K, attempts, iters);  // first: the refusal does not depend on the buffers
    if (rc != MSTG_OK) return rc;
    if (!img || !labels || !centers || !compactness || !best) return fail_arg(MSTG_E_BADARG, "kmeans_u8: null img, labels, centers, compactness or best pointer");
    if ((uniforms == nullptr) == (centers0 == nullptr)) return fail_arg(MSTG_E_BADARG, "kmeans_u8: give either uniforms or centers0");
    if (centers0 && attempts != 1) return fail_arg(MSTG_E_BADARG, "kmeans_u8: centers0 goes with attempts = 1");
    if (!(eps >= 0)) return fail_arg(MSTG_E_BADARG, "kmeans_u8: eps must be a number >= 0");
    rc = km_shape("kmeans_u8", N, H, W, attempts);
    if (rc != MSTG_OK) return rc;
    const KmWorkspace ws = km_workspace(N, attempts);
    if (!workspace || workspace_bytes < ws.total) return fail_arg(MSTG_E_WORKSPACE, "kmeans_u8: workspace too small");
    if (((uintptr_t)workspace & 15) || ((uintptr_t)labels & 3) || ((uintptr_t)centers & 3) || ((uintptr_t)compactness & 7) || ((uintptr_t)best & 3) ||
        ((uintptr_t)uniforms & 3) || ((uintptr_t)centers0 & 3))
        return fail_arg(MSTG_E_ALIGN, "kmeans_u8: workspace not 16-byte, compactness not 8-byte or another array not 4-byte aligned");
    const size_t hw = (size_t)H * W, px = (size_t)N * hw, P = (size_t)N * attempts;
    const size_t tb = (size_t)(uniforms ? attempts : N) * K * 3 * sizeof(float);
    const void* bufs[7] = {img, uniforms ? (const void*)uniforms : (const void*)centers0, labels, centers, compactness, best, workspace};
    const size_t lens[7] = {px * 3, tb, px * 4, (size_t)N * K * 3 * 4, (size_t)N * 8, (size_t)N * 4, ws.total};
    for (int a = 2; a < 7; ++a)
        for (int b = 0; b < a; ++b)
            if (overlaps(bufs[a], lens[a], bufs[b], lens[b])) return fail_arg(MSTG_E_BADARG, "kmeans_u8: an output or the workspace overlaps an input or another output");
    unsigned char* base = (unsigned char*)workspace;
    u64* sums = (u64*)(base + ws.sums);
    float* cen = (float*)(base + ws.centres);
    int* flags = (int*)(base + ws.flags);
    int* range = (int*)(base + ws.range);
    hipStream_t st = (hipStream_t)stream;
    const size_t n_sums = P * KM_MAX * KM_F;
    const int tiles = (int)cdivz(hw, (size_t)KM_TILE);
    MSTG_LAUNCH(km_init_kernel, at_grid(n_sums), dim3(AT_THREADS), 0, st, sums, n_sums, flags, P, range, (size_t)N * 6);
    MSTG_CHECK_LAUNCH("km_init_kernel");
    MSTG_LAUNCH(km_minmax_kernel, dim3((unsigned)(N * tiles)), dim3(AT_THREADS), 0, st, img, hw, tiles, range);
    MSTG_CHECK_LAUNCH("km_minmax_kernel");
    MSTG_LAUNCH(km_centers_kernel, at_grid(P * K * 3), dim3(AT_THREADS), 0, st, (const int*)range, uniforms, centers0, K, attempts, P * K * 3, cen);
    MSTG_CHECK_LAUNCH("km_centers_kernel");
    const dim3 agrid((unsigned)(P * tiles));
    for (int it = 0; it <= iters; ++it) {  // iters rounds of assignment and update, then the assignment that the result reports
        const int final = it == iters;
        MSTG_LAUNCH(km_assign_kernel, agrid, dim3(AT_THREADS), 0, st, img, hw, tiles, K, attempts, final, (const float*)cen, (const int*)flags, sums);
        MSTG_CHECK_LAUNCH("km_assign_kernel");
        if (final) break;
        MSTG_LAUNCH(km_update_kernel, dim3((unsigned)P), dim3(WAVE), 0, st, sums, cen, flags, K, eps * eps);
        MSTG_CHECK_LAUNCH("km_update_kernel");
    }
    MSTG_LAUNCH(km_select_kernel, dim3((unsigned)N), dim3(WAVE), 0, st, (const u64*)sums, (const float*)cen, K, attempts, centers, compactness, best);
    MSTG_CHECK_LAUNCH("km_select_kernel");
    MSTG_LAUNCH(km_label_kernel, at_grid(px), dim3(AT_THREADS), 0, st, img, hw, px, K, attempts, (const float*)cen, (const int*)best, labels);
    MSTG_CHECK_LAUNCH("km_label_kernel");
    return MSTG_OK;
}

static int region_blend(const char* who, int mode_gain, const unsigned char* styled, const unsigned char* orig, const int* labels, int N, int H, int W,
                        const double* ratios, int count, float s_gain, float v_gain, unsigned char* out, void* stream) {
    char msg[200];
    Ratios r;
    int rc = at_ratios(who, ratios, count, r);
    if (rc != MSTG_OK) return rc;
    if (!styled || !orig || !labels || !out) {
        snprintf(msg, sizeof(msg), "%s: null styled, orig, labels or out pointer", who);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    rc = at_shape(who, N, H, W);
    if (rc != MSTG_OK) return rc;
    if ((uintptr_t)labels & 3) {
        snprintf(msg, sizeof(msg), "%s: labels not 4-byte aligned", who);
        return fail_arg(MSTG_E_ALIGN, msg);
    }
    const size_t px = (size_t)N * H * W, nb = px * 3;
    if (overlaps(out, nb, styled, nb) || overlaps(out, nb, orig, nb) || overlaps(out, nb, labels, px * 4)) {
        snprintf(msg, sizeof(msg), "%s: out overlaps an input", who);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    PointArgs p = at_args(styled, N, H, W, out);
    p.b = orig;
    p.labels = labels;
    p.s_gain = s_gain;
    p.v_gain = v_gain;
    return mode_gain ? at_point<PM_BLEND_GAIN>(p, r, Q8Taps{}, (hipStream_t)stream) : at_point<PM_BLEND>(p, r, Q8Taps{}, (hipStream_t)stream);
}

extern "C" int mstg_region_blend_u8(const unsigned char* styled, const unsigned char* orig, const int* labels, int N, int H, int W,
                                    const double* ratios, int count, unsigned char* out, void* stream) {
    return region_blend("region_blend_u8", 0, styled, orig, labels, N, H, W, ratios, count, 1.f, 1.f, out, stream);
}

extern "C" int mstg_region_blend_gain_u8(const unsigned char* styled, const unsigned char* orig, const int* labels, int N, int H, int W,
                                         const double* ratios, int count, float s_gain, float v_gain, unsigned char* out, void* stream) {
    if (!(s_gain >= 0.f) || !(v_gain >= 0.f)) return fail_arg(MSTG_E_BADARG, "region_blend_gain_u8: a gain must be a number >= 0");
    return region_blend("region_blend_gain_u8", 1, styled, orig, labels, N, H, W, ratios, count, s_gain, v_gain, out, stream);
}

extern "C" int mstg_fuse_scales_u8(const unsigned char* outputs, int S, int N, int H, int W, const float* weights, float gain, unsigned char* out,
                                   void* stream) {
    char msg[160];
    if (S < 1 || S > FS_MAX) {
        snprintf(msg, sizeof(msg), "fuse_scales_u8: S = %d scales is not built: this build takes 1 to %d", S, FS_MAX);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    if (!outputs || !weights || !out) return fail_arg(MSTG_E_BADARG, "fuse_scales_u8: null outputs, weights or out pointer");
    const int rc = at_shape("fuse_scales_u8", N, H, W);
    if (rc != MSTG_OK) return rc;
    const size_t nb = (size_t)N * H * W * 3;
    if (overlaps(out, nb, outputs, nb * S)) return fail_arg(MSTG_E_BADARG, "fuse_scales_u8: out overlaps the input");
    FuseWeights w;
    for (int s = 0; s < FS_MAX; ++s) w.w[s] = s < S ? weights[s] : 0.f;
    MSTG_LAUNCH(at_fuse_kernel, at_grid(nb), dim3(AT_THREADS), 0, (hipStream_t)stream, outputs, S, nb, w, gain, out);
    MSTG_CHECK_LAUNCH("at_fuse_kernel");
    return MSTG_OK;
}

extern "C" size_t mstg_contrast_enhanced_finish_workspace_bytes(int N, int H, int W) {
    if (at_clahe_shape("contrast_enhanced_finish_workspace_bytes", N, H, W) != MSTG_OK) return 0;
    return align16((size_t)N * MSTG_CLAHE_TILES * MSTG_CLAHE_TILES * 256);
}

extern "C" int mstg_contrast_enhanced_finish(const unsigned char* styled, int N, int H, int W, const unsigned short* lab_table,
                                             const unsigned short* inv_table, float s_gain, float v_gain, unsigned char* out, void* workspace,
                                             size_t workspace_bytes, void* stream) {
    const int rc = at_clahe_shape("contrast_enhanced_finish", N, H, W);  // first: the refusal does not depend on the buffers
    if (rc != MSTG_OK) return rc;
    if (!styled || !lab_table || !inv_table || !out) return fail_arg(MSTG_E_BADARG, "contrast_enhanced_finish: null styled, table or out pointer");
    if (!(s_gain >= 0.f) || !(v_gain >= 0.f)) return fail_arg(MSTG_E_BADARG, "contrast_enhanced_finish: a gain must be a number >= 0");
    const size_t nb = (size_t)N * H * W * 3, need = align16((size_t)N * MSTG_CLAHE_TILES * MSTG_CLAHE_TILES * 256);
    if (!workspace || workspace_bytes < need) return fail_arg(MSTG_E_WORKSPACE, "contrast_enhanced_finish: workspace too small (N * 64 * 256 bytes)");
    if (((uintptr_t)lab_table & 1) || ((uintptr_t)inv_table & 1)) return fail_arg(MSTG_E_ALIGN, "contrast_enhanced_finish: a table not 2-byte aligned");
    if (overlaps(out, nb, styled, nb) || overlaps(out, nb, workspace, need) || overlaps(workspace, need, styled, nb) ||
        overlaps(out, nb, lab_table, 2 * MSTG_LAB_TABLE_U16) || overlaps(out, nb, inv_table, 2 * MSTG_LAB_INV_TABLE_U16) ||
        overlaps(workspace, need, lab_table, 2 * MSTG_LAB_TABLE_U16) || overlaps(workspace, need, inv_table, 2 * MSTG_LAB_INV_TABLE_U16))
        return fail_arg(MSTG_E_BADARG, "contrast_enhanced_finish: out or workspace overlaps an input, a table or each other");
    hipStream_t st = (hipStream_t)stream;
    unsigned char* luts = (unsigned char*)workspace;
    MSTG_LAUNCH(at_clahe_lut_kernel, dim3((unsigned)(N * MSTG_CLAHE_TILES * MSTG_CLAHE_TILES)), dim3(AT_THREADS), 0, st, styled, lab_table, H, W, luts);
    MSTG_CHECK_LAUNCH("at_clahe_lut_kernel");
    PointArgs p = at_args(styled, N, H, W, out);
    p.lab = lab_table;
    p.inv = inv_table;
    p.luts = luts;
    p.s_gain = s_gain;
    p.v_gain = v_gain;
    return at_point<PM_CONTRAST>(p, Ratios{}, Q8Taps{}, st);
}

extern "C" int mstg_detail_enhanced_finish(const unsigned char* styled, const unsigned char* orig, int N, int H, int W,
                                           const unsigned short* lab_table, const unsigned short* inv_table, const int* taps, int ksize,
                                           float s_gain, float v_gain, unsigned char* out, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = at_ksize("detail_enhanced_finish", ksize);
    if (rc != MSTG_OK) return rc;
    if (!styled || !orig || !lab_table || !inv_table || !taps || !out)
        return fail_arg(MSTG_E_BADARG, "detail_enhanced_finish: null styled, orig, table, taps or out pointer");
    if (!(s_gain >= 0.f) || !(v_gain >= 0.f)) return fail_arg(MSTG_E_BADARG, "detail_enhanced_finish: a gain must be a number >= 0");
    rc = at_shape("detail_enhanced_finish", N, H, W);
    if (rc != MSTG_OK) return rc;
    Q8Taps t;
    rc = at_taps("detail_enhanced_finish", taps, ksize, t);
    if (rc != MSTG_OK) return rc;
    const size_t px = (size_t)N * H * W, nb = px * 3, need = px * 2;
    if (!workspace || workspace_bytes < need) return fail_arg(MSTG_E_WORKSPACE, "detail_enhanced_finish: workspace too small (N * H * W * 2 bytes)");
    if (((uintptr_t)lab_table & 1) || ((uintptr_t)inv_table & 1) || ((uintptr_t)workspace & 1))
        return fail_arg(MSTG_E_ALIGN, "detail_enhanced_finish: a table or the workspace not 2-byte aligned");
    if (overlaps(out, nb, styled, nb) || overlaps(out, nb, orig, nb) || overlaps(out, nb, workspace, need) || overlaps(workspace, need, styled, nb) ||
        overlaps(workspace, need, orig, nb) || overlaps(out, nb, lab_table, 2 * MSTG_LAB_TABLE_U16) ||
        overlaps(out, nb, inv_table, 2 * MSTG_LAB_INV_TABLE_U16) || overlaps(workspace, need, lab_table, 2 * MSTG_LAB_TABLE_U16) ||
        overlaps(workspace, need, inv_table, 2 * MSTG_LAB_INV_TABLE_U16))
        return fail_arg(MSTG_E_BADARG, "detail_enhanced_finish: out or workspace overlaps an input, a table or each other");
    hipStream_t st = (hipStream_t)stream;
    rc = at_gauss_rows(orig, true, t, ksize, N, H, W, (unsigned short*)workspace, st);
    if (rc != MSTG_OK) return rc;
    PointArgs p = at_args(styled, N, H, W, out);
    p.b = orig;
    p.lab = lab_table;
    p.inv = inv_table;
    p.rows = (const unsigned short*)workspace;
    p.ksize = ksize;
    p.s_gain = s_gain;
    p.v_gain = v_gain;
    return at_point<PM_DETAIL>(p, Ratios{}, t, st);
}
