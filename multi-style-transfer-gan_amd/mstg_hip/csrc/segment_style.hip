// The segmentation-driven local style of the reference (enhanced_local_style.py:76-292) on the device, for a batch of (N, H, W, 3)
// uint8 canvases: the per-segment statistics and blend ratios (:76-171 analyze_segments, determine_blend_ratios), the smoothed blend
// map (:174 scipy.ndimage.gaussian_filter(sigma=3)), the float32 blend (:232-240), the colour / contrast step (:243-257: 8-bit
// COLOR_RGB2HSV, saturation * 1.2, CLAHE(2.0, 8 x 8) of v, COLOR_HSV2RGB), the 3 x 3 sharpening filter (:260-261) and
// cv2.bilateralFilter(5, 50, 50) (:264, the existing mstg_bilateral_u8), and on the HOST the Felzenszwalb segmentation (:68).  Every
// OpenCV, scipy and scikit-image step is restated from the definition in include/mstg_hip.h (tests/enhanced_local_style_ref.py is
// the same restatement in numpy -- neither has been compared with an OpenCV or scikit-image binary).  Every kernel takes N images per
// launch:
//
// Z  seg_zero_kernel        clears the per-segment sums.
// S  seg_stats_kernel       the hot one: a segmented reduction keyed by label, one pass over the image instead of the reference's
//    masked copy, grey conversion and two Sobel filters PER SEGMENT.  One workgroup of 256 threads per 16 x 64 tile, a thread four
//    neighbouring pixels of a row.  The packed pixels and the labels of the tile + 1 pixel of halo (BORDER_REFLECT_101) go to LDS.
//    A pixel adds its ten sums (n, R, G, B, R^2, G^2, B^2, S, y, x) to its own label, and for every DISTINCT label s of its reflected
//    3 x 3 neighbourhood the fixed-point Sobel magnitude of the grey image masked to s (at most nine labels).  Combining, before any
//    global atomic: (1) a thread keeps a run of equal labels in registers; (2) where every lane of a wave ends with one run of the
//    same label (the interior of a segment) the wave adds its lanes up with cross-lane moves and one lane goes on; (3) a
//    workgroup keeps SS_SLOTS label slots (open addressing, LDS atomics on 64-bit integers) and writes every used slot once at
//    the end, with 64-bit integer global atomics.  A tile with more than SS_SLOTS distinct labels sends what does not fit straight
//    to the global sums.  All sums are integers, so the result does not depend on the order: bit-reproducible, independent of N.
// R  seg_ratio_kernel       one thread per (image, label): the ratio in float64, contraction off, every operation in the header's order.
// M  seg_map_kernel         one thread per pixel: map = ratio[label], 0 for a label outside [0, S).
// G  seg_gauss_kernel<AXIS> one thread per pixel: scipy's correlate1d on a float32 plane, float64 weights (SS_K), mode 'reflect',
//    the symmetric accumulation order (outermost pair first), the result stored as float32.
// B  es_blend_kernel        point-wise float32 blend with a map.
// L  es_clahe_lut_kernel    one workgroup per CLAHE tile: histogram in LDS (integer atomics), clip, redistribution, prefix sum, table
//    (the tail, the interpolation and the HSV -> RGB conversion are in u8_image.h: advanced_transform.hip uses them too).
// A  es_clahe_apply_kernel  / es_hsv_apply_kernel: per pixel the bilinear interpolation of the four tables; the RGB form also converts
//    to HSV, scales s and converts back.
// F  es_sharpen_kernel      one thread per pixel: 9 * centre - the eight neighbours, BORDER_REFLECT_101, saturated.
//
// No floating-point atomics anywhere; the device never evaluates exp.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "u8_image.h"

namespace mstg {

constexpr int SS_THREADS = 256;
constexpr int SS_TH = 16, SS_TW = 64, SS_PX = 4;    // tile of the statistics kernel; pixels of a row per thread
constexpr int SS_PH = SS_TH + 2, SS_PW = SS_TW + 2;  // patch with 1 pixel of halo
constexpr int SS_SLOTS = MSTG_SEGMENT_TILE_SLOTS;    // label slots of a workgroup in LDS
constexpr int SS_F = MSTG_SEGMENT_SUMS;              // sums per label: n, R, G, B, R^2, G^2, B^2, S, y, x, E
constexpr int SS_E = SS_F - 1;
constexpr int SS_R = 12;                             // radius of the map smoothing: int(4 * 3 + 0.5)
constexpr int ES_TILES = MSTG_CLAHE_TILES;
static_assert(SS_TH * SS_TW == SS_THREADS * SS_PX && SS_TW / SS_PX == 16, "four pixels per thread, sixteen threads per row");
static_assert((SS_SLOTS & (SS_SLOTS - 1)) == 0 && SS_SLOTS == 128 && SS_F == 11, "the hash takes the top seven bits");
// scipy.ndimage._filters._gaussian_kernel1d(3, 0, 12): exp(-x^2 / 18) / sum, x = 0..12 (numpy's exp and pairwise sum, to the bit)
constexpr double SS_K[SS_R + 1] = {0x1.105a329f98197p-3, 0x1.01a25f86eb137p-3, 0x1.b42a57d56c0bep-4, 0x1.4a614d1afd337p-4, 0x1.bfde9c12bec92p-5,
                                   0x1.0fa58939b528fp-5, 0x1.26defcaeb0202p-6, 0x1.1e6bccad344bap-7, 0x1.f1e9915139406p-9, 0x1.8345966f69518p-10,
                                   0x1.0d8a5ad43c165p-11, 0x1.4fbe39149e277p-13, 0x1.763a210dfb306p-15};
// _gaussian_kernel1d(0.5, 0, 2), for the host segmentation
constexpr double FZ_K[3] = {0x1.92b965ef5aaeep-1, 0x1.b405b9842b206p-4, 0x1.14aebe6a24088p-12};

typedef unsigned long long u64;

// ---- Z, S: the segmented reduction ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SS_THREADS) void seg_zero_kernel(u64* __restrict__ sums, size_t total) {
    const size_t idx = (size_t)blockIdx.x * SS_THREADS + threadIdx.x;
    if (idx < total) sums[idx] = 0;
}

// the slot of `label` in the workgroup's table, -1 when the table is full (the caller then adds to the global sums)
__device__ __forceinline__ int ss_slot(int* keys, int* full, int label) {
    if (*(volatile int*)full) return -1;
    unsigned h = ((unsigned)label * 2654435761u) >> 25;
    for (int i = 0; i < SS_SLOTS; ++i) {
        const int old = atomicCAS(&keys[h], -1, label);
        if (old == -1 || old == label) return (int)h;
        h = (h + 1) & (SS_SLOTS - 1);
    }
    *(volatile int*)full = 1;
    return -1;
}

__device__ __forceinline__ void ss_add(u64* vals, u64* gsum, int slot, int label, int field, u64 v) {
    if (v == 0) return;
    if (slot >= 0)
        atomicAdd(&vals[slot * SS_F + field], v);
    else
        atomicAdd(&gsum[(size_t)label * SS_F + field], v);
}

struct SegRun {
    int label;
    unsigned f[SS_E];
    u64 e;
};

__device__ __forceinline__ void ss_clear(SegRun& r, int label) {
    r.label = label;
#pragma unroll
    for (int k = 0; k < SS_E; ++k) r.f[k] = 0;
    r.e = 0;
}

__device__ __forceinline__ void ss_flush(const SegRun& r, int* keys, int* full, u64* vals, u64* gsum) {
    if (r.label < 0) return;
    const int slot = ss_slot(keys, full, r.label);
#pragma unroll
    for (int k = 0; k < SS_E; ++k) ss_add(vals, gsum, slot, r.label, k, r.f[k]);
    ss_add(vals, gsum, slot, r.label, SS_E, r.e);
}

__global__ __launch_bounds__(SS_THREADS) void seg_stats_kernel(const unsigned char* __restrict__ canvas, const int* __restrict__ labels, int S,
                                                               int H, int W, int tiles_x, int tiles, u64* __restrict__ sums) {
    __shared__ int sdiv[256];
    __shared__ unsigned rgb[SS_PH * SS_PW];
    __shared__ int lab[SS_PH * SS_PW];
    __shared__ int keys[SS_SLOTS];
    __shared__ u64 vals[SS_SLOTS * SS_F];
    __shared__ int full;
    const int tid = threadIdx.x;
    const auto [n, y0, x0] = tile_of<SS_TH, SS_TW>(tiles, tiles_x);
    const size_t plane = (size_t)n * H * W;
    const unsigned char* img = canvas + plane * 3;
    const int* l_img = labels + plane;
    u64* gsum = sums + (size_t)n * S * SS_F;
    sdiv[tid] = div_rhe(255 << 12, tid);  // 256 threads, 256 entries
    if (tid < SS_SLOTS) keys[tid] = -1;
    if (tid == 0) full = 0;
    for (int e = tid; e < SS_SLOTS * SS_F; e += SS_THREADS) vals[e] = 0;
    for (int e = tid; e < SS_PH * SS_PW; e += SS_THREADS) {
        const int r = e / SS_PW, c = e - r * SS_PW;
        const int sy = reflect101(y0 - 1 + r, H), sx = reflect101(x0 - 1 + c, W);  // a position past the image's last tile mirrors too
        const size_t at = (size_t)sy * W + sx;
        const int l = l_img[at];
        rgb[e] = load_px(img + at * 3);
        lab[e] = (unsigned)l < (unsigned)S ? l : -1;  // outside [0, S): belongs to no segment
    }
    __syncthreads();
    const int row = tid >> 4, col = (tid & 15) * SS_PX;
    const int py = y0 + row;
    SegRun run;
    ss_clear(run, -1);
    bool clean = true;  // one run, four pixels of the image, nothing sent elsewhere
#pragma unroll
    for (int j = 0; j < SS_PX; ++j) {
        const int px = x0 + col + j;
        if (py >= H || px >= W) {
            clean = false;
            continue;
        }
        const int c = (row + 1) * SS_PW + col + j + 1;
        const int L = lab[c];
        if (L != run.label) {
            if (j > 0) clean = false;
            ss_flush(run, keys, &full, vals, gsum);
            ss_clear(run, L);
        }
        if (L >= 0) {
            const unsigned q = rgb[c];
            const unsigned R = q & 0xffu, G = (q >> 8) & 0xffu, B = q >> 16;
            int h, s, v;
            hsv_px(q, sdiv, nullptr, h, s, v);
            run.f[0] += 1;
            run.f[1] += R;
            run.f[2] += G;
            run.f[3] += B;
            run.f[4] += R * R;
            run.f[5] += G * G;
            run.f[6] += B * B;
            run.f[7] += (unsigned)s;
            run.f[8] += (unsigned)py;
            run.f[9] += (unsigned)px;
        } else {
            clean = false;
        }
        int l9[9], g9[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int at = c + (k / 3 - 1) * SS_PW + (k % 3 - 1);
            l9[k] = lab[at];
            g9[k] = gray_px(rgb[at]);
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int s = l9[k];
            bool first = s >= 0;
#pragma unroll
            for (int i = 0; i < k; ++i) first = first && l9[i] != s;
            if (!first) continue;
            int m[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) m[i] = l9[i] == s ? g9[i] : 0;
            const int gx = (m[2] + 2 * m[5] + m[8]) - (m[0] + 2 * m[3] + m[6]);
            const int gy = (m[6] + 2 * m[7] + m[8]) - (m[0] + 2 * m[1] + m[2]);
            const int q2 = gx * gx + gy * gy;  // at most 2 * 1020^2
            if (q2 == 0) continue;
            const u64 e = (u64)__builtin_rint(__dsqrt_rn((double)q2) * 4294967296.0);  // below 2^43; the scaling is exact
            if (s == run.label) {
                run.e += e;
            } else {
                clean = false;
                ss_add(vals, gsum, ss_slot(keys, &full, s), s, SS_E, e);
            }
        }
    }
    // the interior of a segment: every lane of the wave holds one run of one label
    const int first_label = __builtin_amdgcn_readfirstlane(run.label);
    if (__all(clean && run.label == first_label)) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int k = 0; k < SS_E; ++k) run.f[k] += __shfl_xor(run.f[k], o, WAVE);  // 256 pixels: every sum fits 32 bits
            run.e += __shfl_xor(run.e, o, WAVE);
        }
        if ((tid & (WAVE - 1)) == 0) ss_flush(run, keys, &full, vals, gsum);
    } else {
        ss_flush(run, keys, &full, vals, gsum);
    }
    __syncthreads();
    for (int e = tid; e < SS_SLOTS * SS_F; e += SS_THREADS) {
        const int slot = e / SS_F, f = e - slot * SS_F;
        const int key = keys[slot];
        const u64 v = vals[e];
        if (key >= 0 && v != 0) atomicAdd(&gsum[(size_t)key * SS_F + f], v);
    }
}

// ---- R, M: the ratio and the map -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SS_THREADS) void seg_ratio_kernel(const u64* __restrict__ sums, int H, int W, size_t total,
                                                               float* __restrict__ ratio) {
#pragma clang fp contract(off)  // numpy rounds every operation
    const size_t idx = (size_t)blockIdx.x * SS_THREADS + threadIdx.x;
    if (idx >= total) return;
    const u64* s = sums + idx * SS_F;
    const u64 n = s[0];
    if (n == 0) {  // a label with no pixel is skipped
        ratio[idx] = 0.f;
        return;
    }
    const double dn = (double)n, hw = (double)((long long)H * W);
    double sd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const u64 var = n * s[4 + c] - s[1 + c] * s[1 + c];  // exact: n <= 2^20, the sums below 2^36 and 2^28
        sd[c] = __dsqrt_rn((double)var) / dn;
    }
    const double mstd = ((sd[0] + sd[1]) + sd[2]) / 3.0;
    const double ed = (double)s[SS_E] / 4294967296.0 / hw;
    const double py = (double)s[8] / dn, px = (double)s[9] / dn;
    const int cy = H / 2, cx = W / 2;
    const double md = __dsqrt_rn((double)(cx * cx + cy * cy));
    const double dy = py - (double)cy, dx = px - (double)cx;
    const double dist = __dsqrt_rn(dy * dy + dx * dx);
    const double sm = (double)s[7] / dn;
    const double t_edge = 0.3 * (ed / 30.0);
    const double t_var = 0.2 * (mstd / 50.0);
    const double t_dist = 0.1 * (dist / md);
    const double t_size = -0.1 * (dn / (hw / 100.0));
    const double t_sat = 0.2 * (sm / 255.0);
    const double adj = (((t_edge + t_var) - t_dist) + t_size) + t_sat;
    double r = 0.7 + adj;
    r = r < 0.9 ? r : 0.9;  // min(0.9, r)
    r = r > 0.3 ? r : 0.3;  // max(0.3, .)
    ratio[idx] = (float)r;
}

__global__ __launch_bounds__(SS_THREADS) void seg_map_kernel(const int* __restrict__ labels, const float* __restrict__ ratio, int S, size_t hw,
                                                             size_t total, float* __restrict__ map) {
    const size_t idx = (size_t)blockIdx.x * SS_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t n = idx / hw;
    const int l = labels[idx];
    map[idx] = (unsigned)l < (unsigned)S ? ratio[n * S + l] : 0.f;
}

// ---- G: scipy.ndimage.gaussian_filter(sigma=3) on float32 ---------------------------------------------------------------------------
template <int AXIS>
__global__ __launch_bounds__(SS_THREADS) void seg_gauss_kernel(const float* __restrict__ in, int H, int W, size_t total, float* __restrict__ out) {
#pragma clang fp contract(off)  // scipy rounds every product and every sum
    const size_t idx = (size_t)blockIdx.x * SS_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t hw = (size_t)H * W;
    const size_t n = idx / hw;
    const int rem = (int)(idx - n * hw), y = rem / W, x = rem - y * W;
    const float* plane = in + n * hw;
    const int len = AXIS == 0 ? H : W, pos = AXIS == 0 ? y : x;
    const size_t stride = AXIS == 0 ? (size_t)W : 1, base = AXIS == 0 ? (size_t)x : (size_t)y * W;
    double t = (double)plane[base + pos * stride] * SS_K[0];
    for (int k = SS_R; k >= 1; --k) {  // the outermost pair first
        int a = pos - k, b = pos + k;
        if (a < 0) a = reflect_sym(a, len);
        if (b >= len) b = reflect_sym(b, len);
        t += ((double)plane[base + a * stride] + (double)plane[base + b * stride]) * SS_K[k];
    }
    out[idx] = (float)t;
}

// ---- B: the float32 blend ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SS_THREADS) void es_blend_kernel(const unsigned char* __restrict__ canvas, const unsigned char* __restrict__ styled,
                                                              const float* __restrict__ map, size_t total, unsigned char* __restrict__ out) {
#pragma clang fp contract(off)  // numpy rounds each product and the sum
    const size_t idx = (size_t)blockIdx.x * SS_THREADS + threadIdx.x;
    if (idx >= total) return;
    const float m = map[idx], m1 = 1.0f - m;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = (float)styled[idx * 3 + c] * m;
        const float b = (float)canvas[idx * 3 + c] * m1;
        float x = a + b;
        x = x < 0.f ? 0.f : (x > 255.f ? 255.f : x);
        if (!(x == x)) x = 0.f;  // a NaN weight: keep the byte defined
        out[idx * 3 + c] = (unsigned char)x;
    }
}

// ---- L, A: CLAHE and the colour step -------------------------------------------------------------------------------------------------
// in: a plane (RGB == false) or an interleaved RGB image whose v = max(R, G, B) is the plane (RGB == true)
template <bool RGB>
__global__ __launch_bounds__(SS_THREADS) void es_clahe_lut_kernel(const unsigned char* __restrict__ in, int H, int W, unsigned char* __restrict__ luts) {
#pragma clang fp contract(off)
    __shared__ int hist[256], scan[256];
    __shared__ int excess;
    const int tid = threadIdx.x;
    const int n = blockIdx.x / (ES_TILES * ES_TILES), tile = blockIdx.x - n * ES_TILES * ES_TILES;
    const int ty = tile / ES_TILES, tx = tile - ty * ES_TILES;
    const int th = H / ES_TILES, tw = W / ES_TILES, area = th * tw;
    const unsigned char* img = in + (size_t)n * H * W * (RGB ? 3 : 1);
    hist[tid] = 0;
    if (tid == 0) excess = 0;
    __syncthreads();
    for (int e = tid; e < area; e += SS_THREADS) {
        const int r = e / tw, c = e - r * tw;
        const size_t at = (size_t)(ty * th + r) * W + tx * tw + c;
        int v;
        if (RGB) {
            const unsigned q = load_px(img + at * 3);
            v = max((int)(q & 0xffu), max((int)((q >> 8) & 0xffu), (int)(q >> 16)));
        } else {
            v = img[at];
        }
        atomicAdd(&hist[v], 1);
    }
    __syncthreads();
    clahe_tile_lut(tid, area, hist, scan, &excess, luts + (size_t)blockIdx.x * 256);  // u8_image.h
}

__global__ __launch_bounds__(SS_THREADS) void es_clahe_apply_kernel(const unsigned char* __restrict__ in, const unsigned char* __restrict__ luts,
                                                                    int H, int W, size_t total, unsigned char* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * SS_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t hw = (size_t)H * W;
    const size_t n = idx / hw;
    const int rem = (int)(idx - n * hw), y = rem / W, x = rem - y * W;
    const float inv_th = __fdiv_rn(1.0f, (float)(H / ES_TILES)), inv_tw = __fdiv_rn(1.0f, (float)(W / ES_TILES));
    out[idx] = (unsigned char)clahe_px(luts + n * ES_TILES * ES_TILES * 256, in[idx], y, x, inv_th, inv_tw);
}

__global__ __launch_bounds__(SS_THREADS) void es_hsv_apply_kernel(const unsigned char* __restrict__ in, const unsigned char* __restrict__ luts, int H,
                                                                  int W, size_t total, unsigned char* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ int sdiv[256], hdiv[256];
    const int tid = threadIdx.x;
    sdiv[tid] = div_rhe(255 << 12, tid);
    hdiv[tid] = div_rhe(122880, tid);
    __syncthreads();
    const size_t idx = (size_t)blockIdx.x * SS_THREADS + tid;
    if (idx >= total) return;
    const size_t hw = (size_t)H * W;
    const size_t n = idx / hw;
    const int rem = (int)(idx - n * hw), y = rem / W, x = rem - y * W;
    int h, s, v;
    hsv_px(load_px(in + idx * 3), sdiv, hdiv, h, s, v);
    const int s2 = (int)fminf(__builtin_rintf((float)s * 1.2f), 255.f);
    const float inv_th = __fdiv_rn(1.0f, (float)(H / ES_TILES)), inv_tw = __fdiv_rn(1.0f, (float)(W / ES_TILES));
    const int v2 = clahe_px(luts + n * ES_TILES * ES_TILES * 256, v, y, x, inv_th, inv_tw);
    const unsigned o = hsv2rgb_px(h, s2, v2);
    out[idx * 3] = (unsigned char)(o & 0xffu);
    out[idx * 3 + 1] = (unsigned char)((o >> 8) & 0xffu);
    out[idx * 3 + 2] = (unsigned char)(o >> 16);
}

// ---- F: the sharpening filter --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SS_THREADS) void es_sharpen_kernel(const unsigned char* __restrict__ in, int H, int W, size_t total,
                                                                unsigned char* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * SS_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t hw = (size_t)H * W;
    const size_t n = idx / hw;
    const int rem = (int)(idx - n * hw), y = rem / W, x = rem - y * W;
    const unsigned char* img = in + n * hw * 3;
    int ys[3], xs[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ys[k] = reflect101(y + k - 1, H);
        xs[k] = reflect101(x + k - 1, W);
    }
    int sum[3] = {0, 0, 0};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned q = load_px(img + ((size_t)ys[r] * W + xs[c]) * 3);
            const int wgt = (r == 1 && c == 1) ? 9 : -1;
            sum[0] += wgt * (int)(q & 0xffu);
            sum[1] += wgt * (int)((q >> 8) & 0xffu);
            sum[2] += wgt * (int)(q >> 16);
        }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[idx * 3 + c] = (unsigned char)min(max(sum[c], 0), 255);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static dim3 ss_grid(size_t items) { return dim3((unsigned)cdivz(items, (size_t)SS_THREADS)); }

// 0 = fine, else the error code (message set)
static int ss_shape(const char* who, int N, int H, int W) {
    const int rc = check_extent(who, N, H, W);
    if (rc != MSTG_OK) return rc;
    const long long px = (long long)N * H * W;  // the finest grid: a thread per pixel
    return check_grid(who, (px + SS_THREADS - 1) / SS_THREADS, 31, "N * H * W", px);
}

static int ss_stats_shape(const char* who, int N, int H, int W, int S) {
    int rc = ss_shape(who, N, H, W);
    if (rc != MSTG_OK) return rc;
    char msg[220];
    if (H < 2 || W < 2) {
        snprintf(msg, sizeof(msg), "%s: H = %d, W = %d: the Sobel filter of the edge sum needs at least 2 x 2 pixels", who, H, W);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    if ((long long)H * W > MSTG_SEGMENT_MAX_PIXELS) {
        snprintf(msg, sizeof(msg), "%s: H * W = %lld is more than %d: the fixed-point edge sum would not fit 64 bits", who, (long long)H * W,
                 MSTG_SEGMENT_MAX_PIXELS);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    if (S < 1) {
        snprintf(msg, sizeof(msg), "%s: num_segments = %d", who, S);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    if ((long long)N * S * SS_F >= (1ll << 31)) {
        snprintf(msg, sizeof(msg), "%s: N * num_segments = %lld: the per-segment sums do not fit one launch", who, (long long)N * S);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    return MSTG_OK;
}

static int es_clahe_shape(const char* who, int N, int H, int W) {
    const int rc = ss_shape(who, N, H, W);
    if (rc != MSTG_OK) return rc;
    if (H % ES_TILES == 0 && W % ES_TILES == 0) return MSTG_OK;
    char msg[220];
    snprintf(msg, sizeof(msg), "%s: H = %d, W = %d: CLAHE with %d x %d tiles is built for sizes that are multiples of %d (OpenCV pads others)", who,
             H, W, ES_TILES, ES_TILES, ES_TILES);
    return fail_arg(MSTG_E_UNSUPPORTED, msg);
}

static int ss_gauss(const float* in, int N, int H, int W, float* tmp, float* out, hipStream_t st) {
    const size_t px = (size_t)N * H * W;
    MSTG_LAUNCH(seg_gauss_kernel<0>, ss_grid(px), dim3(SS_THREADS), 0, st, in, H, W, px, tmp);
    MSTG_CHECK_LAUNCH("seg_gauss_kernel<0>");
    MSTG_LAUNCH(seg_gauss_kernel<1>, ss_grid(px), dim3(SS_THREADS), 0, st, (const float*)tmp, H, W, px, out);
    MSTG_CHECK_LAUNCH("seg_gauss_kernel<1>");
    return MSTG_OK;
}

static int es_blend(const unsigned char* canvas, const unsigned char* styled, const float* map, int N, int H, int W, unsigned char* out,
                    hipStream_t st) {
    const size_t px = (size_t)N * H * W;
    MSTG_LAUNCH(es_blend_kernel, ss_grid(px), dim3(SS_THREADS), 0, st, canvas, styled, map, px, out);
    MSTG_CHECK_LAUNCH("es_blend_kernel");
    return MSTG_OK;
}

static int es_hsv(const unsigned char* in, int N, int H, int W, unsigned char* luts, unsigned char* out, hipStream_t st) {
    const size_t px = (size_t)N * H * W;
    MSTG_LAUNCH(es_clahe_lut_kernel<true>, dim3((unsigned)(N * ES_TILES * ES_TILES)), dim3(SS_THREADS), 0, st, in, H, W, luts);
    MSTG_CHECK_LAUNCH("es_clahe_lut_kernel<true>");
    MSTG_LAUNCH(es_hsv_apply_kernel, ss_grid(px), dim3(SS_THREADS), 0, st, in, (const unsigned char*)luts, H, W, px, out);
    MSTG_CHECK_LAUNCH("es_hsv_apply_kernel");
    return MSTG_OK;
}

static int es_sharpen(const unsigned char* in, int N, int H, int W, unsigned char* out, hipStream_t st) {
    const size_t px = (size_t)N * H * W;
    MSTG_LAUNCH(es_sharpen_kernel, ss_grid(px), dim3(SS_THREADS), 0, st, in, H, W, px, out);
    MSTG_CHECK_LAUNCH("es_sharpen_kernel");
    return MSTG_OK;
}

static size_t es_lut_bytes(int N) { return align16((size_t)N * ES_TILES * ES_TILES * 256); }

// the layout of mstg_enhanced_style_finish's workspace: the CLAHE tables and two image batches used in turn
struct EsWorkspace {
    size_t luts, a, b, total;
};
static EsWorkspace es_workspace(int N, int H, int W) {
    const size_t img = align16((size_t)N * H * W * 3);
    EsWorkspace w;
    w.luts = 0;
    w.a = es_lut_bytes(N);
    w.b = w.a + img;
    w.total = w.b + img;
    return w;
}

// scipy's correlate1d of one line (stride st, length n) with the symmetric weights k[0 .. r], mode 'reflect'
static void fz_line(const double* in, double* out, int n, size_t st, const double* k, int r) {
#pragma clang fp contract(off)
    auto idx = [n](int i) {
        const int p = 2 * n;
        i %= p;
        if (i < 0) i += p;
        return i < n ? i : p - 1 - i;
    };
    for (int i = 0; i < n; ++i) {
        double t = in[(size_t)i * st] * k[0];
        for (int j = r; j >= 1; --j) t += (in[(size_t)idx(i - j) * st] + in[(size_t)idx(i + j) * st]) * k[j];
        out[(size_t)i * st] = t;
    }
}

}  // namespace mstg

using namespace mstg;

extern "C" size_t mstg_segment_blend_map_workspace_bytes(int N, int H, int W, int num_segments, int smooth) {
    if (ss_stats_shape("segment_blend_map_workspace_bytes", N, H, W, num_segments) != MSTG_OK) return 0;
    return smooth ? 2 * align16((size_t)N * H * W * sizeof(float)) : 16;
}

extern "C" int mstg_segment_blend_map(const unsigned char* canvas, const int* labels, int N, int H, int W, int num_segments, int smooth,
                                      float* map, unsigned long long* sums, float* ratio, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    int rc = ss_stats_shape("segment_blend_map", N, H, W, num_segments);
    if (rc != MSTG_OK) return rc;
    if (!canvas || !labels || !map || !sums || !ratio) return fail_arg(MSTG_E_BADARG, "segment_blend_map: null canvas, labels, map, sums or ratio pointer");
    const size_t px = (size_t)N * H * W, mb = px * sizeof(float), plane = align16(mb);
    const size_t need = smooth ? 2 * plane : 0;
    if (smooth && (!workspace || workspace_bytes < need)) return fail_arg(MSTG_E_WORKSPACE, "segment_blend_map: workspace too small");
    if (((uintptr_t)labels & 3) || ((uintptr_t)map & 3) || ((uintptr_t)ratio & 3) || ((uintptr_t)sums & 7) || (smooth && ((uintptr_t)workspace & 15)))
        return fail_arg(MSTG_E_ALIGN, "segment_blend_map: labels, map or ratio not 4-byte, sums not 8-byte or workspace not 16-byte aligned");
    const size_t ns = (size_t)N * num_segments, sb = ns * SS_F * sizeof(u64), rb = ns * sizeof(float);
    const void* bufs[6] = {canvas, labels, map, sums, ratio, smooth ? workspace : nullptr};
    const size_t lens[6] = {px * 3, px * 4, mb, sb, rb, need};
    for (int a = 2; a < 6; ++a)
        for (int b = 0; b < a; ++b)
            if (bufs[a] && overlaps(bufs[a], lens[a], bufs[b], lens[b]))
                return fail_arg(MSTG_E_BADARG, "segment_blend_map: an output or the workspace overlaps an input or another output");
    hipStream_t st = (hipStream_t)stream;
    MSTG_LAUNCH(seg_zero_kernel, ss_grid(ns * SS_F), dim3(SS_THREADS), 0, st, sums, ns * SS_F);
    MSTG_CHECK_LAUNCH("seg_zero_kernel");
    const int tx = cdiv(W, SS_TW), tiles = tx * cdiv(H, SS_TH);
    MSTG_LAUNCH(seg_stats_kernel, dim3((unsigned)(N * tiles)), dim3(SS_THREADS), 0, st, canvas, labels, num_segments, H, W, tx, tiles, sums);
    MSTG_CHECK_LAUNCH("seg_stats_kernel");
    MSTG_LAUNCH(seg_ratio_kernel, ss_grid(ns), dim3(SS_THREADS), 0, st, (const u64*)sums, H, W, ns, ratio);
    MSTG_CHECK_LAUNCH("seg_ratio_kernel");
    float* raw = smooth ? (float*)workspace : map;
    MSTG_LAUNCH(seg_map_kernel, ss_grid(px), dim3(SS_THREADS), 0, st, labels, (const float*)ratio, num_segments, (size_t)H * W, px, raw);
    MSTG_CHECK_LAUNCH("seg_map_kernel");
    if (!smooth) return MSTG_OK;
    return ss_gauss(raw, N, H, W, (float*)((unsigned char*)workspace + plane), map, st);
}

extern "C" int mstg_gaussian_reflect_f32(const float* in, int N, int H, int W, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!in || !out) return fail_arg(MSTG_E_BADARG, "gaussian_reflect_f32: null in or out pointer");
    const int rc = ss_shape("gaussian_reflect_f32", N, H, W);
    if (rc != MSTG_OK) return rc;
    const size_t mb = (size_t)N * H * W * sizeof(float);
    if (!workspace || workspace_bytes < mb) return fail_arg(MSTG_E_WORKSPACE, "gaussian_reflect_f32: workspace too small (N * H * W * 4 bytes)");
    if (((uintptr_t)in & 3) || ((uintptr_t)out & 3) || ((uintptr_t)workspace & 3))
        return fail_arg(MSTG_E_ALIGN, "gaussian_reflect_f32: in, out or workspace not 4-byte aligned");
    if (overlaps(out, mb, in, mb) || overlaps(out, mb, workspace, mb) || overlaps(workspace, mb, in, mb))
        return fail_arg(MSTG_E_BADARG, "gaussian_reflect_f32: out or workspace overlaps the input or each other");
    return ss_gauss(in, N, H, W, (float*)workspace, out, (hipStream_t)stream);
}

extern "C" int mstg_blend_map_f32_u8(const unsigned char* canvas, const unsigned char* styled, const float* map, int N, int H, int W,
                                     unsigned char* out, void* stream) {
    if (!canvas || !styled || !map || !out) return fail_arg(MSTG_E_BADARG, "blend_map_f32_u8: null canvas, styled, map or out pointer");
    const int rc = ss_shape("blend_map_f32_u8", N, H, W);
    if (rc != MSTG_OK) return rc;
    if ((uintptr_t)map & 3) return fail_arg(MSTG_E_ALIGN, "blend_map_f32_u8: map not 4-byte aligned");
    const size_t px = (size_t)N * H * W, nb = px * 3;
    if (overlaps(out, nb, canvas, nb) || overlaps(out, nb, styled, nb) || overlaps(out, nb, map, px * 4))
        return fail_arg(MSTG_E_BADARG, "blend_map_f32_u8: out overlaps an input");
    return es_blend(canvas, styled, map, N, H, W, out, (hipStream_t)stream);
}

extern "C" size_t mstg_clahe_workspace_bytes(int N, int H, int W) {
    if (es_clahe_shape("clahe_workspace_bytes", N, H, W) != MSTG_OK) return 0;
    return es_lut_bytes(N);
}

extern "C" int mstg_clahe_u8(const unsigned char* in, int N, int H, int W, unsigned char* out, void* workspace, size_t workspace_bytes,
                             void* stream) {
    const int rc = es_clahe_shape("clahe_u8", N, H, W);  // first: the refusal does not depend on the buffers
    if (rc != MSTG_OK) return rc;
    if (!in || !out) return fail_arg(MSTG_E_BADARG, "clahe_u8: null in or out pointer");
    const size_t px = (size_t)N * H * W, need = es_lut_bytes(N);
    if (!workspace || workspace_bytes < need) return fail_arg(MSTG_E_WORKSPACE, "clahe_u8: workspace too small (N * 64 * 256 bytes)");
    if (overlaps(out, px, in, px) || overlaps(out, px, workspace, need) || overlaps(workspace, need, in, px))
        return fail_arg(MSTG_E_BADARG, "clahe_u8: out or workspace overlaps the input or each other");
    hipStream_t st = (hipStream_t)stream;
    unsigned char* luts = (unsigned char*)workspace;
    MSTG_LAUNCH(es_clahe_lut_kernel<false>, dim3((unsigned)(N * ES_TILES * ES_TILES)), dim3(SS_THREADS), 0, st, in, H, W, luts);
    MSTG_CHECK_LAUNCH("es_clahe_lut_kernel<false>");
    MSTG_LAUNCH(es_clahe_apply_kernel, ss_grid(px), dim3(SS_THREADS), 0, st, in, (const unsigned char*)luts, H, W, px, out);
    MSTG_CHECK_LAUNCH("es_clahe_apply_kernel");
    return MSTG_OK;
}

extern "C" int mstg_hsv_enhance_u8(const unsigned char* in, int N, int H, int W, unsigned char* out, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    const int rc = es_clahe_shape("hsv_enhance_u8", N, H, W);
    if (rc != MSTG_OK) return rc;
    if (!in || !out) return fail_arg(MSTG_E_BADARG, "hsv_enhance_u8: null in or out pointer");
    const size_t nb = (size_t)N * H * W * 3, need = es_lut_bytes(N);
    if (!workspace || workspace_bytes < need) return fail_arg(MSTG_E_WORKSPACE, "hsv_enhance_u8: workspace too small (N * 64 * 256 bytes)");
    if (overlaps(out, nb, in, nb) || overlaps(out, nb, workspace, need) || overlaps(workspace, need, in, nb))
        return fail_arg(MSTG_E_BADARG, "hsv_enhance_u8: out or workspace overlaps the input or each other");
    return es_hsv(in, N, H, W, (unsigned char*)workspace, out, (hipStream_t)stream);
}

extern "C" int mstg_sharpen3_u8(const unsigned char* in, int N, int H, int W, unsigned char* out, void* stream) {
    if (!in || !out) return fail_arg(MSTG_E_BADARG, "sharpen3_u8: null in or out pointer");
    const int rc = ss_shape("sharpen3_u8", N, H, W);
    if (rc != MSTG_OK) return rc;
    const size_t nb = (size_t)N * H * W * 3;
    if (overlaps(out, nb, in, nb)) return fail_arg(MSTG_E_BADARG, "sharpen3_u8: out overlaps the input (the filter reads neighbours of every pixel)");
    return es_sharpen(in, N, H, W, out, (hipStream_t)stream);
}

extern "C" size_t mstg_enhanced_style_finish_workspace_bytes(int N, int H, int W) {
    if (es_clahe_shape("enhanced_style_finish_workspace_bytes", N, H, W) != MSTG_OK) return 0;
    return es_workspace(N, H, W).total;
}

extern "C" int mstg_enhanced_style_finish(const unsigned char* canvas, const unsigned char* styled, const float* map, int N, int H, int W,
                                          const float* bilateral_table, unsigned char* out, void* workspace, size_t workspace_bytes,
                                          void* stream) {
    int rc = es_clahe_shape("enhanced_style_finish", N, H, W);
    if (rc == MSTG_OK) rc = check_shape_16x64("enhanced_style_finish", N, H, W);  // the bilateral filter's grid
    if (rc != MSTG_OK) return rc;
    if (!canvas || !styled || !map || !bilateral_table || !out)
        return fail_arg(MSTG_E_BADARG, "enhanced_style_finish: null canvas, styled, map, table or out pointer");
    const EsWorkspace ws = es_workspace(N, H, W);
    const size_t px = (size_t)N * H * W, nb = px * 3, need = ws.total;
    if (!workspace || workspace_bytes < need) return fail_arg(MSTG_E_WORKSPACE, "enhanced_style_finish: workspace too small");
    if (((uintptr_t)workspace & 15) || ((uintptr_t)map & 3) || ((uintptr_t)bilateral_table & 3))
        return fail_arg(MSTG_E_ALIGN, "enhanced_style_finish: workspace not 16-byte, map or table not 4-byte aligned");
    const size_t tb = sizeof(float) * MSTG_BILATERAL_TABLE_FLOATS;
    if (overlaps(out, nb, canvas, nb) || overlaps(out, nb, styled, nb) || overlaps(out, nb, map, px * 4) || overlaps(out, nb, workspace, need) ||
        overlaps(out, nb, bilateral_table, tb) || overlaps(workspace, need, canvas, nb) || overlaps(workspace, need, styled, nb) ||
        overlaps(workspace, need, map, px * 4) || overlaps(workspace, need, bilateral_table, tb))
        return fail_arg(MSTG_E_BADARG, "enhanced_style_finish: out or the workspace overlaps an input or the table");
    unsigned char* base = (unsigned char*)workspace;
    unsigned char* luts = base + ws.luts;
    unsigned char* a = base + ws.a;
    unsigned char* b = base + ws.b;
    hipStream_t st = (hipStream_t)stream;
    rc = es_blend(canvas, styled, map, N, H, W, a, st);
    if (rc == MSTG_OK) rc = es_hsv(a, N, H, W, luts, b, st);
    if (rc == MSTG_OK) rc = es_sharpen(b, N, H, W, a, st);
    if (rc != MSTG_OK) return rc;
    return mstg_bilateral_u8(a, N, H, W, 5, bilateral_table, out, stream);
}

extern "C" int mstg_felzenszwalb_u8(const unsigned char* img, int H, int W, double scale, double sigma, int min_size, int* labels) {
#pragma clang fp contract(off)
    char msg[200];
    if (!img || !labels) return fail_arg(MSTG_E_BADARG, "felzenszwalb_u8: null img or labels pointer");
    if (H < 1 || W < 1 || (long long)H * W > MSTG_SEGMENT_MAX_PIXELS) {
        snprintf(msg, sizeof(msg), "felzenszwalb_u8: H = %d, W = %d: need 1 to %d pixels", H, W, MSTG_SEGMENT_MAX_PIXELS);
        return fail_arg(H < 1 || W < 1 ? MSTG_E_BADARG : MSTG_E_UNSUPPORTED, msg);
    }
    if (sigma != 0.5) {
        snprintf(msg, sizeof(msg), "felzenszwalb_u8: sigma = %g is not built: the Gaussian's weights are restated for sigma = 0.5 only", sigma);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    if (!(scale > 0) || min_size < 0) {
        snprintf(msg, sizeof(msg), "felzenszwalb_u8: scale = %g, min_size = %d", scale, min_size);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    const size_t hw = (size_t)H * W;
    std::vector<double> a(hw * 3), b(hw * 3);
    for (size_t i = 0; i < hw * 3; ++i) a[i] = (double)img[i] / 255.0;
    for (int c = 0; c < 3; ++c) {
        for (int x = 0; x < W; ++x) fz_line(&a[(size_t)x * 3 + c], &b[(size_t)x * 3 + c], H, (size_t)W * 3, FZ_K, 2);  // axis 0
        for (int y = 0; y < H; ++y) fz_line(&b[(size_t)y * W * 3 + c], &a[(size_t)y * W * 3 + c], W, 3, FZ_K, 2);    // axis 1
    }
    const double sc = scale / 255.0;
    std::vector<int> e0, e1;
    std::vector<double> cost;
    const int dys[4] = {0, 1, 1, -1}, dxs[4] = {1, 0, 1, 1};  // right, down, down-right, up-right
    for (int k = 0; k < 4; ++k)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const int y2 = y + dys[k], x2 = x + dxs[k];
                if (y2 < 0 || y2 >= H || x2 >= W) continue;
                const size_t p = (size_t)y * W + x, q = (size_t)y2 * W + x2;
                const double d0 = a[p * 3] - a[q * 3], d1 = a[p * 3 + 1] - a[q * 3 + 1], d2 = a[p * 3 + 2] - a[q * 3 + 2];
                const double s0 = d0 * d0, s1 = d1 * d1, s2 = d2 * d2;
                e0.push_back((int)p);
                e1.push_back((int)q);
                cost.push_back(std::sqrt((s0 + s1) + s2));
            }
    std::vector<int> order(cost.size());
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&cost](int i, int j) { return cost[i] < cost[j]; });
    std::vector<int> parent(hw), size(hw, 1);
    std::vector<double> cint(hw, 0.0);
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&parent](int i) {
        int r = i;
        while (parent[r] != r) r = parent[r];
        while (parent[i] != r) {
            const int nx = parent[i];
            parent[i] = r;
            i = nx;
        }
        return r;
    };
    auto join = [&](int r0, int r1) {  // the smaller pixel index stays the root
        const int keep = r0 < r1 ? r0 : r1, gone = r0 < r1 ? r1 : r0;
        parent[gone] = keep;
        size[keep] += size[gone];
        return keep;
    };
    for (int i : order) {
        const int r0 = find(e0[i]), r1 = find(e1[i]);
        if (r0 == r1) continue;
        const double t0 = cint[r0] + sc / (double)size[r0], t1 = cint[r1] + sc / (double)size[r1];
        if (cost[i] < (t0 < t1 ? t0 : t1)) cint[join(r0, r1)] = cost[i];
    }
    for (int i : order) {
        const int r0 = find(e0[i]), r1 = find(e1[i]);
        if (r0 != r1 && (size[r0] < min_size || size[r1] < min_size)) join(r0, r1);
    }
    int count = 0;
    for (size_t p = 0; p < hw; ++p)  // a root is the smallest pixel of its component: it is numbered before any other pixel reads it
        labels[p] = find((int)p) == (int)p ? count++ : labels[find((int)p)];
    return count;
}
