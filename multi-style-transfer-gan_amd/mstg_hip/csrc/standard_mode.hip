// The finish of the standard mode of the reference's application (gan_login_gui.py:817-868 standard_process_thread) on the device, for a
// batch of 256 x 256 canvases (any H, W >= 1): the blend with the canvas (:820-828), cv2.medianBlur(3) (:835),
// cv2.bilateralFilter(d=9, 75, 75) (:838), the colour step of the direction (:843-857) and cv2.GaussianBlur((k, k), 0) (:859-868).
// Every OpenCV step is restated from the definition in include/mstg_hip.h (tests/standard_mode_ref.py is the same restatement in
// numpy -- neither has been compared with an OpenCV binary).  Four kernels, every one takes N images per launch:
//
// M  standard_median3_kernel     one workgroup of 256 threads per 16 x 64 tile, four pixels of a row per thread.  The tile + 1 pixel
//    of halo (BORDER_REPLICATE) goes to LDS as one packed word per pixel; with BLEND the word is formed from the styled image and
//    the canvas as blend_byte (u8_image.h) forms it (float64, two rounded products, one rounded sum, clip, truncate), halo pixels from
//    their own replicated source coordinates.  Per channel the median of the 9 samples through a 19-exchange network: integers.
// B  standard_bilateral_kernel   the hot one: same tiling, halo = radius (4 at d = 9) with BORDER_REFLECT_101 source coordinates,
//    the 768 colour weights in LDS (a gather per tap), the space weights read at compile-time indices of the table (scalar loads).
//    A thread walks the taps in the definition's order (i, then j) for its four pixels at once, so a row of 4 + 2 * radius LDS
//    words serves 4 * (2 * radius + 1) taps.  float32, contraction off, the three channel sums through __fmaf_rn, one IEEE
//    division 1 / wsum, round half to even.  With LUT the colour step's table lookup is applied to the byte before the store.
// P  standard_pointwise_kernel   the blend and / or the table lookup on the flat byte stream, 12 bytes per thread.
// G  standard_gaussian_kernel    OpenCV's bit-exact 8-bit blur for ksize 3, 5, 7 (sigma 0): 8.8 fixed-point taps along x into exact
//    16-bit row sums in LDS, then along y, (sum + 32768) >> 16; BORDER_REFLECT_101; one workgroup per 32 x 64 tile.
//
// The device never evaluates exp: the bilateral tables come from the host (mstg_bilateral_tables) and are uploaded by the caller.
// No atomics, no floating-point reduction across threads: every output is a function of the inputs alone, bit-reproducible.
#include <cmath>

#include "u8_image.h"

namespace mstg {

constexpr int SM_THREADS = 256;
constexpr int SM_TH = 16, SM_TW = 64;  // tile of the median and the bilateral kernel: 16 rows of 16 threads x 4 pixels
constexpr int SG_TH = 32, SG_TW = 64;  // tile of the blur
constexpr int SM_COLOR = MSTG_BILATERAL_COLOR_WEIGHTS, SM_TAPS = MSTG_BILATERAL_MAX_TAPS;
static_assert(SM_TW == 64 && SM_TH * (SM_TW / 4) == SM_THREADS, "one item of four pixels per thread");

// a packed pixel of styled * (1 - r) + canvas * r, every byte through blend_byte
__device__ __forceinline__ unsigned sm_blend_px(unsigned s, unsigned c, double w0, double w1) {
    return blend_byte(s & 0xffu, c & 0xffu, w0, w1) | blend_byte((s >> 8) & 0xffu, (c >> 8) & 0xffu, w0, w1) << 8 |
           blend_byte((s >> 16) & 0xffu, (c >> 16) & 0xffu, w0, w1) << 16;
}

__device__ __forceinline__ void sm_sort2(int& a, int& b) {
    const int lo = min(a, b);
    b = max(a, b);
    a = lo;
}

// median of nine through the 19-exchange network
__device__ __forceinline__ int sm_median9(int p0, int p1, int p2, int p3, int p4, int p5, int p6, int p7, int p8) {
    sm_sort2(p1, p2); sm_sort2(p4, p5); sm_sort2(p7, p8);
    sm_sort2(p0, p1); sm_sort2(p3, p4); sm_sort2(p6, p7);
    sm_sort2(p1, p2); sm_sort2(p4, p5); sm_sort2(p7, p8);
    sm_sort2(p0, p3); sm_sort2(p5, p8); sm_sort2(p4, p7);
    sm_sort2(p3, p6); sm_sort2(p1, p4); sm_sort2(p2, p5);
    sm_sort2(p4, p7); sm_sort2(p4, p2); sm_sort2(p6, p4);
    sm_sort2(p4, p2);
    return p4;
}

template <bool BLEND>
__global__ __launch_bounds__(SM_THREADS) void standard_median3_kernel(const unsigned char* __restrict__ in,
                                                                      const unsigned char* __restrict__ canvas, double w0, double w1, int H,
                                                                      int W, int tiles_x, int tiles, unsigned char* __restrict__ out) {
    constexpr int PH = SM_TH + 2, PW = SM_TW + 2;
    __shared__ unsigned px[PH * PW];
    const int tid = threadIdx.x;
    const auto [n, y0, x0] = tile_of<SM_TH, SM_TW>(tiles, tiles_x);
    const size_t base = (size_t)n * H * W * 3;
    for (int e = tid; e < PH * PW; e += SM_THREADS) {
        const int r = e / PW, c = e - r * PW;
        const int sy = min(max(y0 - 1 + r, 0), H - 1), sx = min(max(x0 - 1 + c, 0), W - 1);  // BORDER_REPLICATE
        const size_t i = base + ((size_t)sy * W + sx) * 3;
        unsigned v = load_px(in + i);
        if (BLEND) v = sm_blend_px(v, load_px(canvas + i), w0, w1);
        px[e] = v;
    }
    __syncthreads();
    const int r = tid >> 4, c = (tid & 15) * 4;
    const int py = y0 + r, pxx = x0 + c;
    if (py >= H || pxx >= W) return;
    unsigned o[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        unsigned q[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) q[k] = px[(r + k / 3) * PW + c + p + k % 3];
        unsigned v = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int s = 8 * ch;
            v |= (unsigned)sm_median9((q[0] >> s) & 0xff, (q[1] >> s) & 0xff, (q[2] >> s) & 0xff, (q[3] >> s) & 0xff, (q[4] >> s) & 0xff,
                                      (q[5] >> s) & 0xff, (q[6] >> s) & 0xff, (q[7] >> s) & 0xff, (q[8] >> s) & 0xff)
                 << s;
        }
        o[p] = v;
    }
    store_px4(out + base + ((size_t)py * W + pxx) * 3, o, W - pxx);
}

template <int R, bool LUT>
__global__ __launch_bounds__(SM_THREADS) void standard_bilateral_kernel(const unsigned char* __restrict__ in, const float* __restrict__ table,
                                                                        const unsigned char* __restrict__ lut, int H, int W, int tiles_x,
                                                                        int tiles, unsigned char* __restrict__ out) {
#pragma clang fp contract(off)  // the definition rounds the weight product; the only fused operations are the explicit __fmaf_rn
    constexpr int PH = SM_TH + 2 * R, PW = SM_TW + 2 * R, ROW = 4 + 2 * R;
    __shared__ __align__(16) unsigned px[PH * PW];
    __shared__ float color[SM_COLOR];
    __shared__ unsigned char slut[LUT ? 768 : 4];
    const int tid = threadIdx.x;
    const auto [n, y0, x0] = tile_of<SM_TH, SM_TW>(tiles, tiles_x);
    const size_t base = (size_t)n * H * W * 3;
    for (int e = tid; e < SM_COLOR; e += SM_THREADS) {
        color[e] = table[e];
        if (LUT) slut[e] = lut[e];  // the two tables have the same length: one loop stages both (stage_lut768 would be a second one)
    }
    for (int e = tid; e < PH * PW; e += SM_THREADS) {
        const int r = e / PW, c = e - r * PW;
        int sy = y0 - R + r, sx = x0 - R + c;
        if ((unsigned)sy >= (unsigned)H) sy = reflect101(sy, H);  // also for rows of the tile below the image: any valid pixel
        if ((unsigned)sx >= (unsigned)W) sx = reflect101(sx, W);
        px[e] = load_px(in + base + ((size_t)sy * W + sx) * 3);
    }
    __syncthreads();
    const int r = tid >> 4, c = (tid & 15) * 4;
    const int py = y0 + r, pxx = x0 + c;
    if (py >= H || pxx >= W) return;
    float wsum[4], s0[4], s1[4], s2[4];
    unsigned ctr[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        wsum[p] = s0[p] = s1[p] = s2[p] = 0.f;
        ctr[p] = px[(r + R) * PW + c + R + p];
    }
    int k = 0;  // index of the tap in the definition's list; a constant after unrolling
#pragma unroll
    for (int i = -R; i <= R; ++i) {
        unsigned row[ROW];
#pragma unroll
        for (int q = 0; q < ROW; ++q) row[q] = px[(r + R + i) * PW + c + q];
#pragma unroll
        for (int j = -R; j <= R; ++j) {
            if (i * i + j * j > R * R) continue;
            const float sp = table[SM_COLOR + k];
            ++k;
#pragma unroll
            for (int p = 0; p < 4; ++p) bilateral_tap(row[p + R + j], ctr[p], sp, color, wsum[p], s0[p], s1[p], s2[p]);
        }
    }
    unsigned o[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        unsigned b0, b1, b2;
        bilateral_bytes(wsum[p], s0[p], s1[p], s2[p], b0, b1, b2);
        if (LUT) {
            b0 = slut[b0];
            b1 = slut[256 + b1];
            b2 = slut[512 + b2];
        }
        o[p] = b0 | b1 << 8 | b2 << 16;
    }
    store_px4(out + base + ((size_t)py * W + pxx) * 3, o, W - pxx);
}

// a and canvas: flat byte streams of nbytes (a multiple of 3: byte b belongs to channel b % 3); 12 bytes per thread
template <bool BLEND, bool LUT>
__global__ __launch_bounds__(SM_THREADS) void standard_pointwise_kernel(const unsigned char* __restrict__ a,
                                                                        const unsigned char* __restrict__ canvas, double w0, double w1,
                                                                        const unsigned char* __restrict__ lut, size_t nbytes, int aligned,
                                                                        unsigned char* __restrict__ out) {
    __shared__ unsigned char slut[LUT ? 768 : 4];
    const int tid = threadIdx.x;
    if (LUT) {
        stage_lut768<SM_THREADS>(lut, slut, tid);
        __syncthreads();
    }
    const size_t b0 = ((size_t)blockIdx.x * SM_THREADS + tid) * 12;
    if (b0 >= nbytes) return;
    if (aligned && b0 + 12 <= nbytes) {
        unsigned va[3], vc[3] = {0u, 0u, 0u}, vo[3] = {0u, 0u, 0u};
#pragma unroll
        for (int w = 0; w < 3; ++w) va[w] = reinterpret_cast<const unsigned*>(a + b0)[w];
        if (BLEND) {
#pragma unroll
            for (int w = 0; w < 3; ++w) vc[w] = reinterpret_cast<const unsigned*>(canvas + b0)[w];
        }
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            unsigned v = (va[k >> 2] >> (8 * (k & 3))) & 0xffu;
            if (BLEND) v = blend_byte(v, (vc[k >> 2] >> (8 * (k & 3))) & 0xffu, w0, w1);
            if (LUT) v = slut[256 * (k % 3) + v];
            vo[k >> 2] |= v << (8 * (k & 3));
        }
#pragma unroll
        for (int w = 0; w < 3; ++w) reinterpret_cast<unsigned*>(out + b0)[w] = vo[w];
        return;
    }
    const int cnt = (int)(nbytes - b0 < 12 ? nbytes - b0 : 12);
    for (int k = 0; k < cnt; ++k) {
        unsigned v = a[b0 + k];
        if (BLEND) v = blend_byte(v, canvas[b0 + k], w0, w1);
        if (LUT) v = slut[256 * (k % 3) + v];
        out[b0 + k] = (unsigned char)v;
    }
}

template <int R>
__global__ __launch_bounds__(SM_THREADS) void standard_gaussian_kernel(const unsigned char* __restrict__ in, int H, int W, int tiles_x,
                                                                       int tiles, unsigned char* __restrict__ out) {
    constexpr int EH = SG_TH + 2 * R, EW = SG_TW + 2 * R, EWP = SG_TW + 8;  // the patch and its row pitch in LDS
    static_assert(EWP >= EW, "pitch of the blur's patch");
    __shared__ unsigned char en[3 * EH * EWP];
    __shared__ unsigned short hz[3 * EH * SG_TW];  // the horizontally filtered rows, exact (<= 65280)
    const int tid = threadIdx.x;
    const auto [n, y0, x0] = tile_of<SG_TH, SG_TW>(tiles, tiles_x);
    const size_t base = (size_t)n * H * W * 3;
    for (int e = tid; e < EH * EW; e += SM_THREADS) {
        const int r = e / EW, c = e - r * EW;
        int sy = y0 - R + r, sx = x0 - R + c;
        if ((unsigned)sy >= (unsigned)H) sy = reflect101(sy, H);
        if ((unsigned)sx >= (unsigned)W) sx = reflect101(sx, W);
        const unsigned v = load_px(in + base + ((size_t)sy * W + sx) * 3);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) en[(ch * EH + r) * EWP + c] = (unsigned char)((v >> (8 * ch)) & 0xffu);
    }
    __syncthreads();
    for (int e = tid; e < 3 * EH * SG_TW; e += SM_THREADS) {
        const int row = e / SG_TW, c = e - row * SG_TW;  // row = channel * EH + patch row
        const unsigned char* p = &en[row * EWP + c];
        int sum = 0;
#pragma unroll
        for (int k = 0; k <= 2 * R; ++k) sum += gauss_q8_tap<2 * R + 1>(k) * (int)p[k];
        hz[e] = (unsigned short)sum;
    }
    __syncthreads();
    for (int it = tid; it < SG_TH * (SG_TW / 4); it += SM_THREADS) {
        const int r = it >> 4, c = (it & 15) * 4;
        const int py = y0 + r, pxx = x0 + c;
        if (py >= H || pxx >= W) continue;
        unsigned o[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            unsigned v = 0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const unsigned short* hp = &hz[(ch * EH + r) * SG_TW + c + p];
                int sum = 0;
#pragma unroll
                for (int k = 0; k <= 2 * R; ++k) sum += gauss_q8_tap<2 * R + 1>(k) * (int)hp[k * SG_TW];
                v |= (unsigned)((sum + 32768) >> 16) << (8 * ch);
            }
            o[p] = v;
        }
        store_px4(out + base + ((size_t)py * W + pxx) * 3, o, W - pxx);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// every check returns 0 = fine, else the error code (message set); the shape check is check_shape_16x64 (SM_TH x SM_TW)
static int sm_d(const char* who, int d) {
    if (d == 3 || d == 5 || d == 7 || d == 9) return MSTG_OK;
    char msg[240];
    snprintf(msg, sizeof(msg),
             "%s: d = %d is not built: this build takes the odd diameters 3 to 9 (d <= 0 derives the radius from sigma_space, "
             "d > 9 needs a halo of more than 4 pixels)",
             who, d);
    return fail_arg(MSTG_E_UNSUPPORTED, msg);
}

// smooth_level 0 = no blur; 1 .. 3 = ksize 3, 5, 7
static int sm_level(const char* who, int level) {
    if (level >= 0 && level <= 3) return MSTG_OK;
    char msg[256];
    if (level < 0) {
        snprintf(msg, sizeof(msg), "%s: smooth_level = %d", who, level);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    snprintf(msg, sizeof(msg),
             "%s: smooth_level = %d (ksize %d) is not built: above ksize 7 OpenCV generates the fixed-point taps with its softfloat "
             "code, which is not restated here, and the blur is never approximated",
             who, level, 2 * level + 1);
    return fail_arg(MSTG_E_UNSUPPORTED, msg);
}

static int sm_median(const unsigned char* in, const unsigned char* canvas, double w0, double w1, int N, int H, int W, unsigned char* out,
                     hipStream_t st) {
    const int tx = cdiv(W, SM_TW), tiles = tx * cdiv(H, SM_TH);
    const dim3 grid((unsigned)(N * tiles)), block(SM_THREADS);
    if (canvas)
        MSTG_LAUNCH((standard_median3_kernel<true>), grid, block, 0, st, in, canvas, w0, w1, H, W, tx, tiles, out);
    else
        MSTG_LAUNCH((standard_median3_kernel<false>), grid, block, 0, st, in, canvas, w0, w1, H, W, tx, tiles, out);
    MSTG_CHECK_LAUNCH("standard_median3_kernel");
    return MSTG_OK;
}

template <int R>
static void sm_bilateral_r(const unsigned char* in, const float* table, const unsigned char* lut, int N, int H, int W, unsigned char* out,
                           hipStream_t st) {
    const int tx = cdiv(W, SM_TW), tiles = tx * cdiv(H, SM_TH);
    const dim3 grid((unsigned)(N * tiles)), block(SM_THREADS);
    if (lut)
        MSTG_LAUNCH((standard_bilateral_kernel<R, true>), grid, block, 0, st, in, table, lut, H, W, tx, tiles, out);
    else
        MSTG_LAUNCH((standard_bilateral_kernel<R, false>), grid, block, 0, st, in, table, lut, H, W, tx, tiles, out);
}

static int sm_bilateral(const unsigned char* in, int d, const float* table, const unsigned char* lut, int N, int H, int W, unsigned char* out,
                        hipStream_t st) {
    switch (d / 2) {
        case 1: sm_bilateral_r<1>(in, table, lut, N, H, W, out, st); break;
        case 2: sm_bilateral_r<2>(in, table, lut, N, H, W, out, st); break;
        case 3: sm_bilateral_r<3>(in, table, lut, N, H, W, out, st); break;
        default: sm_bilateral_r<4>(in, table, lut, N, H, W, out, st); break;
    }
    MSTG_CHECK_LAUNCH("standard_bilateral_kernel");
    return MSTG_OK;
}

// the blend (canvas != NULL) and / or the lookup (lut != NULL) on N * H * W * 3 bytes; neither = a copy
static int sm_pointwise(const unsigned char* a, const unsigned char* canvas, double w0, double w1, const unsigned char* lut, size_t nbytes,
                        unsigned char* out, hipStream_t st) {
    const dim3 grid((unsigned)cdivz(nbytes, (size_t)SM_THREADS * 12)), block(SM_THREADS);
    const int aligned = aligned4(a) && aligned4(out) && (!canvas || aligned4(canvas));
    if (canvas && lut)
        MSTG_LAUNCH((standard_pointwise_kernel<true, true>), grid, block, 0, st, a, canvas, w0, w1, lut, nbytes, aligned, out);
    else if (canvas)
        MSTG_LAUNCH((standard_pointwise_kernel<true, false>), grid, block, 0, st, a, canvas, w0, w1, lut, nbytes, aligned, out);
    else if (lut)
        MSTG_LAUNCH((standard_pointwise_kernel<false, true>), grid, block, 0, st, a, canvas, w0, w1, lut, nbytes, aligned, out);
    else
        MSTG_LAUNCH((standard_pointwise_kernel<false, false>), grid, block, 0, st, a, canvas, w0, w1, lut, nbytes, aligned, out);
    MSTG_CHECK_LAUNCH("standard_pointwise_kernel");
    return MSTG_OK;
}

static int sm_gaussian(const unsigned char* in, int N, int H, int W, int level, unsigned char* out, hipStream_t st) {
    const int tx = cdiv(W, SG_TW), tiles = tx * cdiv(H, SG_TH);
    const dim3 grid((unsigned)(N * tiles)), block(SM_THREADS);
    if (level == 1)
        MSTG_LAUNCH((standard_gaussian_kernel<1>), grid, block, 0, st, in, H, W, tx, tiles, out);
    else if (level == 2)
        MSTG_LAUNCH((standard_gaussian_kernel<2>), grid, block, 0, st, in, H, W, tx, tiles, out);
    else
        MSTG_LAUNCH((standard_gaussian_kernel<3>), grid, block, 0, st, in, H, W, tx, tiles, out);
    MSTG_CHECK_LAUNCH("standard_gaussian_kernel");
    return MSTG_OK;
}

}  // namespace mstg

using namespace mstg;

extern "C" int mstg_bilateral_tables(int d, double sigma_color, double sigma_space, float* table) {
    if (!table) return fail_arg(MSTG_E_BADARG, "bilateral_tables: null table pointer");
    const int rc = sm_d("bilateral_tables", d);
    if (rc != MSTG_OK) return rc;
    if (sigma_color <= 0) sigma_color = 1;
    if (sigma_space <= 0) sigma_space = 1;
    const int radius = d / 2 > 1 ? d / 2 : 1;
    const double gauss_color = -0.5 / (sigma_color * sigma_color), gauss_space = -0.5 / (sigma_space * sigma_space);
    for (int t = 0; t < SM_COLOR; ++t) table[t] = (float)std::exp((double)(t * t) * gauss_color);
    int k = 0;
    for (int i = -radius; i <= radius; ++i)
        for (int j = -radius; j <= radius; ++j) {
            if (std::sqrt((double)i * i + (double)j * j) > radius) continue;
            table[SM_COLOR + k++] = (float)std::exp((double)(i * i + j * j) * gauss_space);
        }
    for (int e = k; e < SM_TAPS; ++e) table[SM_COLOR + e] = 0.f;
    return k;
}

extern "C" int mstg_standard_color_lut(int model_type, unsigned char* lut) {
    if (!lut) return fail_arg(MSTG_E_BADARG, "standard_color_lut: null table pointer");
    if (model_type == MSTG_STANDARD_PHOTO_TO_MONET) {
        for (int v = 0; v < 256; ++v) {  // the indices of the reference's code: channel 0 * 1.1, channel 1 * 1.05, float64, truncated
            const double a = (double)v * 1.1, b = (double)v * 1.05;
            lut[v] = (unsigned char)(a < 0.0 ? 0.0 : (a > 255.0 ? 255.0 : a));
            lut[256 + v] = (unsigned char)(b < 0.0 ? 0.0 : (b > 255.0 ? 255.0 : b));
            lut[512 + v] = (unsigned char)v;
        }
        return MSTG_OK;
    }
    if (model_type == MSTG_STANDARD_MONET_TO_PHOTO) {
        for (int v = 0; v < 256; ++v) {  // convertScaleAbs(alpha=1.1, beta=5) as local_style_finish_kernel defines it
            float t = std::fabs(std::fmaf((float)v, 1.1f, 5.0f));
            t = std::nearbyint(t);  // round half to even (the default rounding mode)
            const unsigned char b = (unsigned char)(t > 255.f ? 255.f : t);
            lut[v] = lut[256 + v] = lut[512 + v] = b;
        }
        return MSTG_OK;
    }
    char msg[160];
    snprintf(msg, sizeof(msg), "standard_color_lut: model_type = %d is neither photo_to_monet (0) nor monet_to_photo (1)", model_type);
    return fail_arg(MSTG_E_BADARG, msg);
}

extern "C" int mstg_median3_u8(const unsigned char* in, int N, int H, int W, unsigned char* out, void* stream) {
    if (!in || !out) return fail_arg(MSTG_E_BADARG, "median3_u8: null in or out pointer");
    const int rc = check_shape_16x64("median3_u8", N, H, W);
    if (rc != MSTG_OK) return rc;
    const size_t nb = (size_t)N * H * W * 3;
    if (overlaps(out, nb, in, nb)) return fail_arg(MSTG_E_BADARG, "median3_u8: out overlaps the input (the filter reads neighbours of every pixel)");
    return sm_median(in, nullptr, 0.0, 0.0, N, H, W, out, (hipStream_t)stream);
}

extern "C" int mstg_bilateral_u8(const unsigned char* in, int N, int H, int W, int d, const float* table, unsigned char* out, void* stream) {
    int rc = sm_d("bilateral_u8", d);  // first: the refusal does not depend on the buffers
    if (rc != MSTG_OK) return rc;
    if (!in || !out || !table) return fail_arg(MSTG_E_BADARG, "bilateral_u8: null in, table or out pointer");
    rc = check_shape_16x64("bilateral_u8", N, H, W);
    if (rc != MSTG_OK) return rc;
    if ((uintptr_t)table & 3) return fail_arg(MSTG_E_ALIGN, "bilateral_u8: table not 4-byte aligned");
    const size_t nb = (size_t)N * H * W * 3;
    if (overlaps(out, nb, in, nb) || overlaps(out, nb, table, sizeof(float) * MSTG_BILATERAL_TABLE_FLOATS))
        return fail_arg(MSTG_E_BADARG, "bilateral_u8: out overlaps the input or the table (the filter reads neighbours of every pixel)");
    return sm_bilateral(in, d, table, nullptr, N, H, W, out, (hipStream_t)stream);
}

extern "C" int mstg_lut_u8(const unsigned char* in, int N, int H, int W, const unsigned char* lut, unsigned char* out, void* stream) {
    if (!in || !out || !lut) return fail_arg(MSTG_E_BADARG, "lut_u8: null in, lut or out pointer");
    const int rc = check_shape_16x64("lut_u8", N, H, W);
    if (rc != MSTG_OK) return rc;
    const size_t nb = (size_t)N * H * W * 3;
    if (overlaps(out, nb, lut, 768) || overlaps(out, nb, in, nb)) return fail_arg(MSTG_E_BADARG, "lut_u8: out overlaps the input or the table");
    return sm_pointwise(in, nullptr, 0.0, 0.0, lut, nb, out, (hipStream_t)stream);
}

extern "C" int mstg_gaussian_u8(const unsigned char* in, int N, int H, int W, int ksize, unsigned char* out, void* stream) {
    if (ksize < 3 || !(ksize & 1)) {
        char msg[120];
        snprintf(msg, sizeof(msg), "gaussian_u8: ksize = %d: need an odd size of at least 3 (ksize = 2 * smooth_level + 1)", ksize);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    int rc = sm_level("gaussian_u8", ksize / 2);
    if (rc != MSTG_OK) return rc;
    if (!in || !out) return fail_arg(MSTG_E_BADARG, "gaussian_u8: null in or out pointer");
    rc = check_shape_16x64("gaussian_u8", N, H, W);
    if (rc != MSTG_OK) return rc;
    const size_t nb = (size_t)N * H * W * 3;
    if (overlaps(out, nb, in, nb)) return fail_arg(MSTG_E_BADARG, "gaussian_u8: out overlaps the input (the filter reads neighbours of every pixel)");
    return sm_gaussian(in, N, H, W, ksize / 2, out, (hipStream_t)stream);
}

extern "C" size_t mstg_standard_finish_workspace_bytes(int N, int H, int W) {
    if (check_shape_16x64("standard_finish_workspace_bytes", N, H, W) != MSTG_OK) return 0;
    return 2 * align16((size_t)N * H * W * 3);
}

extern "C" int mstg_standard_finish(const unsigned char* canvas, const unsigned char* styled, int N, int H, int W, double one_minus_ratio,
                                    double blend_ratio, int fix_blocks, int d, const float* bilateral_table, const unsigned char* color_lut,
                                    int smooth_level, unsigned char* out, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = fix_blocks ? sm_d("standard_finish", d) : MSTG_OK;
    if (rc == MSTG_OK) rc = sm_level("standard_finish", smooth_level);
    if (rc != MSTG_OK) return rc;
    const bool blend = blend_ratio > 0;  // the reference skips the step otherwise (:820)
    if (!styled || !out || (blend && !canvas)) return fail_arg(MSTG_E_BADARG, "standard_finish: null styled, out or (with a blend) canvas pointer");
    if (fix_blocks && !bilateral_table) return fail_arg(MSTG_E_BADARG, "standard_finish: fix_blocks needs the bilateral table");
    rc = check_shape_16x64("standard_finish", N, H, W);
    if (rc != MSTG_OK) return rc;
    const size_t nb = (size_t)N * H * W * 3, plane = align16(nb);
    if (!workspace || workspace_bytes < 2 * plane) return fail_arg(MSTG_E_WORKSPACE, "standard_finish: workspace too small");
    if (((uintptr_t)workspace & 15) || ((uintptr_t)bilateral_table & 3))
        return fail_arg(MSTG_E_ALIGN, "standard_finish: workspace not 16-byte or bilateral table not 4-byte aligned");
    if (overlaps(out, nb, styled, nb) || (blend && overlaps(out, nb, canvas, nb)) || overlaps(out, nb, workspace, 2 * plane) ||
        (fix_blocks && overlaps(out, nb, bilateral_table, sizeof(float) * MSTG_BILATERAL_TABLE_FLOATS)) ||
        (color_lut && overlaps(out, nb, color_lut, 768)))
        return fail_arg(MSTG_E_BADARG, "standard_finish: out overlaps an input, a table or the workspace");
    unsigned char* wa = (unsigned char*)workspace;
    unsigned char* wb = wa + plane;
    const unsigned char* cv = blend ? canvas : nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (fix_blocks) {  // median (blend at its load) -> bilateral (lookup at its store) -> blur
        rc = sm_median(styled, cv, one_minus_ratio, blend_ratio, N, H, W, wa, st);
        if (rc == MSTG_OK) rc = sm_bilateral(wa, d, bilateral_table, color_lut, N, H, W, smooth_level ? wb : out, st);
        if (rc == MSTG_OK && smooth_level) rc = sm_gaussian(wb, N, H, W, smooth_level, out, st);
        return rc;
    }
    if (!smooth_level) return sm_pointwise(styled, cv, one_minus_ratio, blend_ratio, color_lut, nb, out, st);
    const unsigned char* src = styled;
    if (cv || color_lut) {  // blend and lookup in one point-wise launch
        rc = sm_pointwise(styled, cv, one_minus_ratio, blend_ratio, color_lut, nb, wa, st);
        if (rc != MSTG_OK) return rc;
        src = wa;
    }
    return sm_gaussian(src, N, H, W, smooth_level, out, st);
}
