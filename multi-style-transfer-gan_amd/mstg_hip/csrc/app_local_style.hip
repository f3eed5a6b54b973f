// The local-style tab and the compare tab of the reference's application (gan_login_gui.py:1328-1426 local_style_process_thread,
// :2475-2560 compare_process_thread) on the device, for a batch of canvases (any H, W >= 1): the sky mask (cv2.cvtColor(COLOR_RGB2HSV)
// -> cv2.inRange -> upper half -> cv2.dilate(5 x 5, 2 iterations) -> cv2.GaussianBlur((15, 15), 0)), the edge weight (cv2.Canny ->
// cv2.dilate(3 x 3) -> cv2.GaussianBlur((21, 21), 0) in float64 -> * detail), the three truncating float64 blends, the colour step
// and cv2.bilateralFilter(9, 75, 75).  Canny (csrc/local_style.hip), the bilateral filter and the colour tables
// (csrc/standard_mode.hip) exist; this file adds three kernels and the chain entry.  Every OpenCV step is restated from the
// definition in include/mstg_hip.h (tests/app_local_style_ref.py is the same restatement in numpy -- neither has been compared with
// an OpenCV binary).
//
// S  app_sky_mask_kernel     one workgroup of 256 threads per 32 x 64 tile.  The `blue` bits of the tile + 11 pixels of halo (4 for
//    the 9 x 9 maximum, 7 for the blur; 0 outside the image and below the upper half) go to LDS; the hue and saturation divisor
//    tables are built in LDS with integer round-half-even; the dilation runs as a row OR and a column OR; the 15-tap blur in 8.8
//    fixed point along x into exact 16-bit sums, then along y, (sum + 32768) >> 16, both as dword passes with four outputs per
//    item.  BORDER_REFLECT_101 applies to the DILATED mask: a patch position outside the image is filled with the mirrored pixel's
//    own value, which the patch holds (a pixel of the tile lies at most 7 from the tap and the mirror at most 7 beyond it on the
//    inner side, its 9 x 9 window 4 further: 11).  A tile whose patch lies below the upper half writes zeros and is done.
// E  app_edge_weight_kernel  one workgroup of 256 threads per 16 x 64 tile (the tiling of local_style_weights_kernel).  The edge bytes
//    of the tile + 11 pixels of halo (1 for the 3 x 3 maximum, 10 for the blur) go to LDS, the dilation to a second patch; the
//    float64 row pass (21 taps left to right, four outputs per item from six dwords) writes LDS, the column pass (centre, then the
//    symmetric pairs from the nearest outwards; one column and four rows per thread, 24 LDS values for 84 taps) reads it;
//    contraction off; a patch position outside the image holds the 3 x 3 maximum around the mirrored pixel.  The taps come from
//    the host (mstg_gaussian_kernel_f64) and are read with scalar loads: the device never evaluates exp.
// C  app_chain_kernel        point-wise, no LDS but the colour table: the enabled blends (sky, edge, strength), each clipped and
//    truncated to a byte before the next, then the table; four pixels per thread, dword loads and stores; a disabled stage is
//    compiled out.
//
// Integer arithmetic or a fixed float64 order everywhere, no atomics in these kernels: bit-reproducible and independent of N.
#include <cmath>

#include "u8_image.h"

namespace mstg {

constexpr int AP_THREADS = 256;
constexpr int AS_TH = 32, AS_TW = 64;                   // tile of the sky mask
constexpr int AS_RD = 4, AS_RB = 7, AS_HALO = AS_RD + AS_RB;  // 9 x 9 maximum, 15-tap blur
constexpr int AS_BH = AS_TH + 2 * AS_HALO, AS_BW = AS_TW + 2 * AS_HALO;  // blue patch
constexpr int AS_DH = AS_TH + 2 * AS_RB, AS_DW = AS_TW + 2 * AS_RB;      // dilated patch
constexpr int AS_DWP = AS_TW + 2 * 8;  // its row pitch in LDS: the item of the last four columns reads five whole dwords
constexpr int AE_TH = 16, AE_TW = 64;                   // tile of the edge weight (LC_TH, LC_TW of local_style.hip)
constexpr int AE_RB = 10, AE_HALO = AE_RB + 1;          // 21-tap blur, 3 x 3 maximum
constexpr int AE_EH = AE_TH + 2 * AE_HALO, AE_EW = AE_TW + 2 * AE_HALO;  // edge patch
constexpr int AE_DH = AE_TH + 2 * AE_RB, AE_DW = AE_TW + 2 * AE_RB;      // dilated patch
constexpr int AE_TAPS = MSTG_APP_EDGE_KSIZE;
static_assert(AE_TAPS == 2 * AE_RB + 1, "the edge blur has 21 taps");
static_assert(AS_DWP >= AS_DW && AS_DWP % 4 == 0 && AS_TW % 4 == 0 && AE_DW % 4 == 0 && AE_TW == 64 && AE_TH == 16 && AP_THREADS == 256,
              "dword passes; one column and four rows per thread in the edge weight's column pass");

// round-half-even(num / i) in integers, 0 for i == 0
__device__ __forceinline__ int ap_div_rhe(int num, int i) {
    if (i == 0) return 0;
    const int q = num / i, r = num - q * i;
    return q + ((2 * r > i || (2 * r == i && (q & 1))) ? 1 : 0);
}

__global__ __launch_bounds__(AP_THREADS) void app_sky_mask_kernel(const unsigned char* __restrict__ canvas, int H, int W, int tiles_x,
                                                                  int tiles, unsigned char* __restrict__ mask) {
    __shared__ int sdiv[256], hdiv[256];
    __shared__ unsigned char bl[AS_BH * AS_BW];   // blue: 0 / 1, 0 outside the image (the dilation's neutral border)
    __shared__ unsigned char ro[AS_BH * AS_DW];   // OR of bl over the 9 columns of the window
    __shared__ __align__(16) unsigned char dl[AS_DH * AS_DWP];  // the dilated mask, 0 / 255, mirrored outside the image
    __shared__ __align__(16) unsigned short hz[AS_DH * AS_TW];  // the horizontally filtered rows, exact (<= 65280)
    const int tid = threadIdx.x;
    const auto [n, y0, x0] = tile_of<AS_TH, AS_TW>(tiles, tiles_x);
    const size_t plane = (size_t)n * H * W;
    const unsigned char* img = canvas + plane * 3;
    unsigned char* m_img = mask + plane;
    const int half = H / 2;
    if (y0 - AS_HALO >= half) {  // no row of the patch lies in the upper half: the mask is 0 on the whole tile (the workgroup agrees)
        for (int e = tid; e < AS_TH * AS_TW; e += AP_THREADS) {
            const int py = y0 + e / AS_TW, px = x0 + (e & (AS_TW - 1));
            if (py < H && px < W) m_img[(size_t)py * W + px] = 0;
        }
        return;
    }
    sdiv[tid] = ap_div_rhe(255 << 12, tid);  // 256 threads, 256 entries
    hdiv[tid] = ap_div_rhe(122880, tid);     // (180 << 12) / (6 i)
    __syncthreads();
    // staged in batches of unconditional loads (a position outside the upper half reads pixel 0 and counts as 0), so a wave waits
    // out one memory round trip per batch, not per element
    constexpr int NB = 5;
    for (int e0 = 0; e0 < AS_BH * AS_BW; e0 += NB * AP_THREADS) {
        unsigned rgb[NB];
        bool ok[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int e = e0 + k * AP_THREADS + tid;
            const int r = e / AS_BW, c = e - r * AS_BW;
            const int py = y0 - AS_HALO + r, px = x0 - AS_HALO + c;
            ok[k] = e < AS_BH * AS_BW && (unsigned)py < (unsigned)half && (unsigned)px < (unsigned)W;  // only the upper half can be sky
            const unsigned char* p = img + (ok[k] ? ((size_t)py * W + px) * 3 : 0);
            rgb[k] = load_px(p);
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int e = e0 + k * AP_THREADS + tid;
            const int R = rgb[k] & 0xff, G = (rgb[k] >> 8) & 0xff, B = rgb[k] >> 16;
            const int v = max(R, max(G, B)), diff = v - min(R, min(G, B));
            const int s = (diff * sdiv[v] + 2048) >> 12;
            const int h0 = v == R ? G - B : (v == G ? B - R + 2 * diff : R - G + 4 * diff);
            int h = (h0 * hdiv[diff] + 2048) >> 12;  // arithmetic shift of the signed product
            if (h < 0) h += 180;
            if (e < AS_BH * AS_BW) bl[e] = (ok[k] && h >= 90 && h <= 130 && s >= 30 && v >= 140) ? 1 : 0;
        }
    }
    __syncthreads();
    for (int e = tid; e < AS_BH * AS_DW; e += AP_THREADS) {
        const int r = e / AS_DW, c = e - r * AS_DW;
        const unsigned char* p = &bl[r * AS_BW + c];
        unsigned v = 0;
#pragma unroll
        for (int k = 0; k <= 2 * AS_RD; ++k) v |= p[k];
        ro[e] = (unsigned char)v;
    }
    __syncthreads();
    for (int e = tid; e < AS_DH * AS_DW; e += AP_THREADS) {
        const int r = e / AS_DW, c = e - r * AS_DW;
        unsigned v = 0;
#pragma unroll
        for (int k = 0; k <= 2 * AS_RD; ++k) v |= ro[(r + k) * AS_DW + c];
        dl[r * AS_DWP + c] = v ? 255 : 0;
    }
    __syncthreads();
    // BORDER_REFLECT_101 of the dilated mask: a position outside the image takes the value of the mirrored pixel (positions inside
    // the image are read, positions outside are written).  The clamp only moves positions no pixel of the image needs.
    for (int e = tid; e < AS_DH * AS_DW; e += AP_THREADS) {
        const int r = e / AS_DW, c = e - r * AS_DW;
        const int py = y0 - AS_RB + r, px = x0 - AS_RB + c;
        if ((unsigned)py < (unsigned)H && (unsigned)px < (unsigned)W) continue;
        const int my = reflect101(py, H), mx = reflect101(px, W);
        const int mr = min(max(my - (y0 - AS_RB), 0), AS_DH - 1), mc = min(max(mx - (x0 - AS_RB), 0), AS_DW - 1);
        dl[r * AS_DWP + c] = dl[mr * AS_DWP + mc];
    }
    __syncthreads();
    for (int it = tid; it < AS_DH * (AS_TW / 4); it += AP_THREADS) {  // four columns per item: bytes c .. c + 17 of the row
        const int r = it / (AS_TW / 4), c = 4 * (it - r * (AS_TW / 4));
        const unsigned* p = reinterpret_cast<const unsigned*>(&dl[r * AS_DWP + c]);
        const unsigned w[5] = {p[0], p[1], p[2], p[3], p[4]};
        int px[18];
#pragma unroll
        for (int k = 0; k < 18; ++k) px[k] = (int)((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
        unsigned o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int sum = 0;
#pragma unroll
            for (int k = 0; k <= 2 * AS_RB; ++k) sum += gauss_q8_tap<2 * AS_RB + 1>(k) * px[j + k];
            o[j] = (unsigned)sum;  // <= 65280
        }
        *reinterpret_cast<uint2*>(&hz[r * AS_TW + c]) = make_uint2(o[0] | o[1] << 16, o[2] | o[3] << 16);
    }
    __syncthreads();
    for (int it = tid; it < AS_TH * (AS_TW / 4); it += AP_THREADS) {
        const int r = it / (AS_TW / 4), c = 4 * (it - r * (AS_TW / 4));
        const int py = y0 + r, px = x0 + c;
        if (py >= H || px >= W) continue;
        int sum[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k <= 2 * AS_RB; ++k) {
            const uint2 h = *reinterpret_cast<const uint2*>(&hz[(r + k) * AS_TW + c]);
            sum[0] += gauss_q8_tap<2 * AS_RB + 1>(k) * (int)(h.x & 0xffffu);
            sum[1] += gauss_q8_tap<2 * AS_RB + 1>(k) * (int)(h.x >> 16);
            sum[2] += gauss_q8_tap<2 * AS_RB + 1>(k) * (int)(h.y & 0xffffu);
            sum[3] += gauss_q8_tap<2 * AS_RB + 1>(k) * (int)(h.y >> 16);
        }
        unsigned o[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) o[p] = (unsigned)((sum[p] + 32768) >> 16);
        unsigned char* dst = m_img + (size_t)py * W + px;
        if (px + 4 <= W && ((uintptr_t)dst & 3) == 0) {
            *reinterpret_cast<unsigned*>(dst) = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
        } else {
            for (int p = 0; p < 4; ++p)
                if (px + p < W) dst[p] = (unsigned char)o[p];
        }
    }
}

__global__ __launch_bounds__(AP_THREADS) void app_edge_weight_kernel(const unsigned char* __restrict__ edge,
                                                                     const double* __restrict__ taps, double detail, int H, int W,
                                                                     int tiles_x, int tiles, double* __restrict__ weight) {
#pragma clang fp contract(off)  // OpenCV's generic filters round every product and every sum
    __shared__ unsigned char eg[AE_EH * AE_EW];                // edge: 0 / 1, 0 outside the image (the dilation's neutral border)
    __shared__ __align__(16) unsigned char ed[AE_DH * AE_DW];  // the dilated mask, 0 / 1, mirrored outside the image
    __shared__ __align__(16) double rw[AE_DH * AE_TW];         // the row pass
    const int tid = threadIdx.x;
    const auto [n, y0, x0] = tile_of<AE_TH, AE_TW>(tiles, tiles_x);
    const size_t plane = (size_t)n * H * W;
    const unsigned char* e_img = edge + plane;
    constexpr int NB = 7;  // batches of unconditional loads, as in the sky mask: a position outside the image reads pixel 0, counts as 0
    for (int e0 = 0; e0 < AE_EH * AE_EW; e0 += NB * AP_THREADS) {
        unsigned char v[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int e = e0 + k * AP_THREADS + tid;
            const int r = e / AE_EW, c = e - r * AE_EW;
            const int py = y0 - AE_HALO + r, px = x0 - AE_HALO + c;
            const bool ok = e < AE_EH * AE_EW && (unsigned)py < (unsigned)H && (unsigned)px < (unsigned)W;
            const unsigned char b = e_img[ok ? (size_t)py * W + px : 0];
            v[k] = ok && b != 0 ? 1 : 0;
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int e = e0 + k * AP_THREADS + tid;
            if (e < AE_EH * AE_EW) eg[e] = v[k];
        }
    }
    __syncthreads();
    // The dilation at every position of the patch; BORDER_REFLECT_101 applies to the DILATED mask, so a position outside the image
    // takes the 3 x 3 maximum around the mirrored pixel.  The clamp only moves positions no pixel of the image needs.
    for (int e = tid; e < AE_DH * AE_DW; e += AP_THREADS) {
        const int r = e / AE_DW, c = e - r * AE_DW;
        int py = y0 - AE_RB + r, px = x0 - AE_RB + c;
        if ((unsigned)py >= (unsigned)H) py = reflect101(py, H);
        if ((unsigned)px >= (unsigned)W) px = reflect101(px, W);
        const int mr = min(max(py - (y0 - AE_HALO), 1), AE_EH - 2), mc = min(max(px - (x0 - AE_HALO), 1), AE_EW - 2);
        const unsigned char* p = &eg[(mr - 1) * AE_EW + mc - 1];
        ed[e] = p[0] | p[1] | p[2] | p[AE_EW] | p[AE_EW + 1] | p[AE_EW + 2] | p[2 * AE_EW] | p[2 * AE_EW + 1] | p[2 * AE_EW + 2];
    }
    __syncthreads();
    for (int it = tid; it < AE_DH * (AE_TW / 4); it += AP_THREADS) {  // four columns per item: bytes c .. c + 23 of the row
        const int r = it / (AE_TW / 4), c = 4 * (it - r * (AE_TW / 4));
        const unsigned* p = reinterpret_cast<const unsigned*>(&ed[r * AE_DW + c]);
        const unsigned w[6] = {p[0], p[1], p[2], p[3], p[4], p[5]};
        double t[4];
#pragma unroll
        for (int j = 0; j < AE_TAPS; ++j) {
            const double kj = taps[j];  // the same for every lane: a scalar load
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double v = (w[(q + j) >> 2] >> (8 * ((q + j) & 3))) & 1u ? kj : 0.0;  // k[j] * S: exact, S is 0 or 1
                t[q] = j == 0 ? v : t[q] + v;
            }
        }
        double* dst = &rw[r * AE_TW + c];
        *reinterpret_cast<double2*>(dst) = make_double2(t[0], t[1]);
        *reinterpret_cast<double2*>(dst + 2) = make_double2(t[2], t[3]);
    }
    __syncthreads();
    // one column and four rows per thread: 24 values of the row pass serve 4 x 21 taps
    const int c = tid & (AE_TW - 1), r0 = 4 * (tid / AE_TW);
    const int px = x0 + c;
    if (px >= W) return;
    double v[AE_TAPS + 3];
#pragma unroll
    for (int i = 0; i < AE_TAPS + 3; ++i) v[i] = rw[(r0 + i) * AE_TW + c];
    double* w_img = weight + plane;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int py = y0 + r0 + q;
        if (py >= H) break;
        double t = taps[AE_RB] * v[q + AE_RB];
#pragma unroll
        for (int j = 1; j <= AE_RB; ++j) t += taps[AE_RB + j] * (v[q + AE_RB + j] + v[q + AE_RB - j]);
        w_img[(size_t)py * W + px] = t * detail;
    }
}

// flat pixel streams of npix pixels; four pixels (12 bytes) per thread
template <bool SKY, bool EDGE, bool STRENGTH, bool LUT>
__global__ __launch_bounds__(AP_THREADS) void app_chain_kernel(const unsigned char* __restrict__ canvas,
                                                               const unsigned char* __restrict__ styled,
                                                               const unsigned char* __restrict__ sky, const double* __restrict__ edge_w,
                                                               double w_img, double w_orig, const unsigned char* __restrict__ lut,
                                                               size_t npix, int aligned, unsigned char* __restrict__ out) {
#pragma clang fp contract(off)
    constexpr bool BLEND = SKY || EDGE || STRENGTH;
    __shared__ unsigned char slut[LUT ? 768 : 4];
    const int tid = threadIdx.x;
    if (LUT) {
        stage_lut768<AP_THREADS>(lut, slut, tid);
        __syncthreads();
    }
    const size_t p0 = ((size_t)blockIdx.x * AP_THREADS + tid) * 4;
    if (p0 >= npix) return;
    const int cnt = (int)(npix - p0 < 4 ? npix - p0 : 4);
    const bool vec = aligned && cnt == 4;
    unsigned vs[3] = {0u, 0u, 0u}, vc[3] = {0u, 0u, 0u}, vo[3] = {0u, 0u, 0u}, vm = 0u;
    double wa[4] = {0.0, 0.0, 0.0, 0.0};
    if (vec) {
#pragma unroll
        for (int w = 0; w < 3; ++w) vs[w] = reinterpret_cast<const unsigned*>(styled + p0 * 3)[w];
        if (BLEND) {
#pragma unroll
            for (int w = 0; w < 3; ++w) vc[w] = reinterpret_cast<const unsigned*>(canvas + p0 * 3)[w];
        }
        if (SKY) vm = *reinterpret_cast<const unsigned*>(sky + p0);
    } else {
        for (int b = 0; b < 3 * cnt; ++b) {
            vs[b >> 2] |= (unsigned)styled[p0 * 3 + b] << (8 * (b & 3));
            if (BLEND) vc[b >> 2] |= (unsigned)canvas[p0 * 3 + b] << (8 * (b & 3));
        }
        if (SKY)
            for (int k = 0; k < cnt; ++k) vm |= (unsigned)sky[p0 + k] << (8 * k);
    }
    if (EDGE) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) wa[k] = edge_w[p0 + k];
    }
#pragma unroll
    for (int b = 0; b < 12; ++b) {
        const int k = b / 3, ch = b - 3 * k;
        unsigned v = (vs[b >> 2] >> (8 * (b & 3))) & 0xffu;
        const unsigned c = (vc[b >> 2] >> (8 * (b & 3))) & 0xffu;
        if (SKY) {
            const double w = (double)((vm >> (8 * k)) & 0xffu) / 255.0;  // IEEE division, as numpy's
            v = blend_byte(v, c, 1.0 - w, w);
        }
        if (EDGE) v = blend_byte(v, c, 1.0 - wa[k], wa[k]);
        if (STRENGTH) v = blend_byte(v, c, w_img, w_orig);
        if (LUT) v = slut[256 * ch + v];
        vo[b >> 2] |= v << (8 * (b & 3));
    }
    if (vec) {
#pragma unroll
        for (int w = 0; w < 3; ++w) reinterpret_cast<unsigned*>(out + p0 * 3)[w] = vo[w];
    } else {
        for (int b = 0; b < 3 * cnt; ++b) out[p0 * 3 + b] = (unsigned char)((vo[b >> 2] >> (8 * (b & 3))) & 0xffu);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// the shape check is check_shape_16x64: the edge weight's tiling (AE_TH x AE_TW, asserted above) is the finest, the point-wise grid
// is no finer
static int ap_sky_mask(const unsigned char* canvas, int N, int H, int W, unsigned char* mask, hipStream_t st) {
    const int tx = cdiv(W, AS_TW), tiles = tx * cdiv(H, AS_TH);
    MSTG_LAUNCH(app_sky_mask_kernel, dim3((unsigned)(N * tiles)), dim3(AP_THREADS), 0, st, canvas, H, W, tx, tiles, mask);
    MSTG_CHECK_LAUNCH("app_sky_mask_kernel");
    return MSTG_OK;
}

static int ap_edge_weight(const unsigned char* edge, const double* taps, double detail, int N, int H, int W, double* weight,
                          hipStream_t st) {
    const int tx = cdiv(W, AE_TW), tiles = tx * cdiv(H, AE_TH);
    MSTG_LAUNCH(app_edge_weight_kernel, dim3((unsigned)(N * tiles)), dim3(AP_THREADS), 0, st, edge, taps, detail, H, W, tx, tiles, weight);
    MSTG_CHECK_LAUNCH("app_edge_weight_kernel");
    return MSTG_OK;
}

template <bool SKY, bool EDGE>
static void ap_chain_se(bool strength, bool lut, dim3 grid, hipStream_t st, const unsigned char* canvas, const unsigned char* styled,
                        const unsigned char* sky, const double* edge_w, double w_img, double w_orig, const unsigned char* color_lut,
                        size_t npix, int aligned, unsigned char* out) {
    const dim3 block(AP_THREADS);
    if (strength && lut)
        MSTG_LAUNCH((app_chain_kernel<SKY, EDGE, true, true>), grid, block, 0, st, canvas, styled, sky, edge_w, w_img, w_orig, color_lut, npix,
                    aligned, out);
    else if (strength)
        MSTG_LAUNCH((app_chain_kernel<SKY, EDGE, true, false>), grid, block, 0, st, canvas, styled, sky, edge_w, w_img, w_orig, color_lut, npix,
                    aligned, out);
    else if (lut)
        MSTG_LAUNCH((app_chain_kernel<SKY, EDGE, false, true>), grid, block, 0, st, canvas, styled, sky, edge_w, w_img, w_orig, color_lut, npix,
                    aligned, out);
    else
        MSTG_LAUNCH((app_chain_kernel<SKY, EDGE, false, false>), grid, block, 0, st, canvas, styled, sky, edge_w, w_img, w_orig, color_lut,
                    npix, aligned, out);
}

// sky / edge_w / color_lut NULL = that stage off; none of the stages = a copy
static int ap_chain(const unsigned char* canvas, const unsigned char* styled, const unsigned char* sky, const double* edge_w, bool strength,
                    double w_img, double w_orig, const unsigned char* color_lut, size_t npix, unsigned char* out, hipStream_t st) {
    const dim3 grid((unsigned)cdivz(npix, (size_t)AP_THREADS * 4));
    const bool blend = sky || edge_w || strength;
    const int aligned = aligned4(styled) && aligned4(out) && (!blend || aligned4(canvas)) && (!sky || aligned4(sky));
    const bool lut = color_lut != nullptr;
    if (sky && edge_w)
        ap_chain_se<true, true>(strength, lut, grid, st, canvas, styled, sky, edge_w, w_img, w_orig, color_lut, npix, aligned, out);
    else if (sky)
        ap_chain_se<true, false>(strength, lut, grid, st, canvas, styled, sky, edge_w, w_img, w_orig, color_lut, npix, aligned, out);
    else if (edge_w)
        ap_chain_se<false, true>(strength, lut, grid, st, canvas, styled, sky, edge_w, w_img, w_orig, color_lut, npix, aligned, out);
    else
        ap_chain_se<false, false>(strength, lut, grid, st, canvas, styled, sky, edge_w, w_img, w_orig, color_lut, npix, aligned, out);
    MSTG_CHECK_LAUNCH("app_chain_kernel");
    return MSTG_OK;
}

// the layout of mstg_app_local_style_finish's workspace
struct ApWorkspace {
    size_t weight, state, sky_bits, edge, mask, count, image, total;
};
static ApWorkspace ap_workspace(int N, int H, int W) {
    const size_t px = (size_t)N * H * W, plane = align16(px);
    ApWorkspace w;
    w.weight = 0;
    w.state = align16(px * sizeof(double));
    w.sky_bits = w.state + plane;
    w.edge = w.sky_bits + plane;
    w.mask = w.edge + plane;
    w.count = w.mask + plane;
    w.image = w.count + align16((size_t)N * sizeof(int));
    w.total = w.image + align16(px * 3);
    return w;
}

}  // namespace mstg

using namespace mstg;

extern "C" int mstg_gaussian_kernel_f64(int ksize, double sigma, double* out) {
    if (!out) return fail_arg(MSTG_E_BADARG, "gaussian_kernel_f64: null out pointer");
    if (ksize < 1 || !(ksize & 1) || ksize > 255) {
        char msg[120];
        snprintf(msg, sizeof(msg), "gaussian_kernel_f64: ksize = %d: need an odd size from 1 to 255", ksize);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    if (!(sigma > 0)) sigma = ((ksize - 1) * 0.5 - 1) * 0.3 + 0.8;  // cv2.getGaussianKernel's rule for sigma <= 0
    const double scale = -0.5 / (sigma * sigma);
    double sum = 0;
    for (int i = 0; i < ksize; ++i) {
        const double x = i - (ksize - 1) / 2;
        out[i] = std::exp(x * x * scale);
        sum += out[i];
    }
    const double inv = 1.0 / sum;
    for (int i = 0; i < ksize; ++i) out[i] *= inv;
    return MSTG_OK;
}

extern "C" int mstg_app_sky_mask(const unsigned char* canvas, int N, int H, int W, unsigned char* mask, void* stream) {
    if (!canvas || !mask) return fail_arg(MSTG_E_BADARG, "app_sky_mask: null canvas or mask pointer");
    const int rc = check_shape_16x64("app_sky_mask", N, H, W);
    if (rc != MSTG_OK) return rc;
    const size_t px = (size_t)N * H * W;
    if (overlaps(mask, px, canvas, px * 3)) return fail_arg(MSTG_E_BADARG, "app_sky_mask: mask overlaps the canvas");
    return ap_sky_mask(canvas, N, H, W, mask, (hipStream_t)stream);
}

extern "C" int mstg_app_edge_weight(const unsigned char* edge, int N, int H, int W, const double* kernel_f64, double detail, double* weight,
                                    void* stream) {
    if (!edge || !kernel_f64 || !weight) return fail_arg(MSTG_E_BADARG, "app_edge_weight: null edge, kernel or weight pointer");
    const int rc = check_shape_16x64("app_edge_weight", N, H, W);
    if (rc != MSTG_OK) return rc;
    if (((uintptr_t)weight & 7) || ((uintptr_t)kernel_f64 & 7))
        return fail_arg(MSTG_E_ALIGN, "app_edge_weight: weight or kernel not 8-byte aligned");
    const size_t px = (size_t)N * H * W;
    if (overlaps(weight, px * 8, edge, px) || overlaps(weight, px * 8, kernel_f64, sizeof(double) * AE_TAPS))
        return fail_arg(MSTG_E_BADARG, "app_edge_weight: weight overlaps the edge mask or the kernel");
    return ap_edge_weight(edge, kernel_f64, detail, N, H, W, weight, (hipStream_t)stream);
}

extern "C" int mstg_app_chain(const unsigned char* canvas, const unsigned char* styled, int N, int H, int W, const unsigned char* sky_mask,
                              const double* edge_weight, int use_strength, double w_styled, double w_canvas, const unsigned char* color_lut,
                              unsigned char* out, void* stream) {
    const bool blend = sky_mask || edge_weight || use_strength;
    if (!styled || !out || (blend && !canvas)) return fail_arg(MSTG_E_BADARG, "app_chain: null styled, out or (with a blend) canvas pointer");
    const int rc = check_shape_16x64("app_chain", N, H, W);
    if (rc != MSTG_OK) return rc;
    if ((uintptr_t)edge_weight & 7) return fail_arg(MSTG_E_ALIGN, "app_chain: edge_weight not 8-byte aligned");
    const size_t px = (size_t)N * H * W, nb = px * 3;
    if (overlaps(out, nb, styled, nb) || (blend && overlaps(out, nb, canvas, nb)) || (sky_mask && overlaps(out, nb, sky_mask, px)) ||
        (edge_weight && overlaps(out, nb, edge_weight, px * 8)) || (color_lut && overlaps(out, nb, color_lut, 768)))
        return fail_arg(MSTG_E_BADARG, "app_chain: out overlaps an input, a mask or the table");
    return ap_chain(canvas, styled, sky_mask, edge_weight, use_strength != 0, w_styled, w_canvas, color_lut, px, out, (hipStream_t)stream);
}

extern "C" size_t mstg_app_local_style_workspace_bytes(int N, int H, int W) {
    if (check_shape_16x64("app_local_style_workspace_bytes", N, H, W) != MSTG_OK) return 0;
    return ap_workspace(N, H, W).total;
}

extern "C" int mstg_app_local_style_finish(const unsigned char* canvas, const unsigned char* styled, int N, int H, int W, int ignore_sky,
                                           int auto_select, int use_strength, int smooth, double detail, double w_styled, double w_canvas,
                                           const double* kernel_f64, const unsigned char* color_lut, const float* bilateral_table,
                                           unsigned char* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!canvas || !styled || !out) return fail_arg(MSTG_E_BADARG, "app_local_style_finish: null canvas, styled or out pointer");
    int rc = check_shape_16x64("app_local_style_finish", N, H, W);
    if (rc == MSTG_OK && auto_select) rc = fits_hysteresis_lds("app_local_style_finish", H, W, "with auto_select ");
    if (rc != MSTG_OK) return rc;
    if (auto_select && !kernel_f64) return fail_arg(MSTG_E_BADARG, "app_local_style_finish: auto_select needs the 21-tap kernel");
    if (smooth && !bilateral_table) return fail_arg(MSTG_E_BADARG, "app_local_style_finish: smooth needs the bilateral table");
    const ApWorkspace ws = ap_workspace(N, H, W);
    if (!workspace || workspace_bytes < ws.total) return fail_arg(MSTG_E_WORKSPACE, "app_local_style_finish: workspace too small");
    if (((uintptr_t)workspace & 15) || ((uintptr_t)kernel_f64 & 7) || ((uintptr_t)bilateral_table & 3))
        return fail_arg(MSTG_E_ALIGN, "app_local_style_finish: workspace not 16-byte, kernel not 8-byte or bilateral table not 4-byte aligned");
    const size_t px = (size_t)N * H * W, nb = px * 3;
    if (overlaps(out, nb, canvas, nb) || overlaps(out, nb, styled, nb) || overlaps(out, nb, workspace, ws.total) ||
        (auto_select && overlaps(out, nb, kernel_f64, sizeof(double) * AE_TAPS)) || (color_lut && overlaps(out, nb, color_lut, 768)) ||
        (smooth && overlaps(out, nb, bilateral_table, sizeof(float) * MSTG_BILATERAL_TABLE_FLOATS)))
        return fail_arg(MSTG_E_BADARG, "app_local_style_finish: out overlaps an input, a table or the workspace");
    unsigned char* base = (unsigned char*)workspace;
    double* weight = (double*)(base + ws.weight);
    unsigned char* mask = base + ws.mask;
    unsigned char* tmp = base + ws.image;
    if (auto_select) {  // Canny of the canvas (csrc/local_style.hip), then the dilation, the float64 blur and * detail
        unsigned char* state = base + ws.state;
        unsigned char* edge = base + ws.edge;
        rc = mstg_local_style_prepare(canvas, N, H, W, state, base + ws.sky_bits, (int*)(base + ws.count), nullptr, stream);
        if (rc == MSTG_OK) rc = mstg_local_style_hysteresis(state, N, H, W, edge, stream);
        if (rc == MSTG_OK) rc = ap_edge_weight(edge, kernel_f64, detail, N, H, W, weight, (hipStream_t)stream);
        if (rc != MSTG_OK) return rc;
    }
    if (ignore_sky) {
        rc = ap_sky_mask(canvas, N, H, W, mask, (hipStream_t)stream);
        if (rc != MSTG_OK) return rc;
    }
    const bool pointwise = ignore_sky || auto_select || use_strength || color_lut;
    if (!smooth || pointwise) {
        rc = ap_chain(canvas, styled, ignore_sky ? mask : nullptr, auto_select ? weight : nullptr, use_strength != 0, w_styled, w_canvas,
                      color_lut, px, smooth ? tmp : out, (hipStream_t)stream);
        if (rc != MSTG_OK) return rc;
    }
    if (smooth) return mstg_bilateral_u8(pointwise ? tmp : styled, N, H, W, 9, bilateral_table, out, stream);
    return MSTG_OK;
}
