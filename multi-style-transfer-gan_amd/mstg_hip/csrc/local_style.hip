// The per-pixel weight map of the reference's process_local_style(mode='enhanced') on the device, for a batch of canvases
// (batch_process_images.py:126-150 detect_sky, :312-342): cv2.cvtColor(COLOR_RGB2HSV) -> sky mask, cv2.cvtColor(COLOR_RGB2GRAY)
// -> cv2.Canny(gray, 50, 150) -> scipy.ndimage.gaussian_filter(edges, sigma=2) > 0.1 -> three weight levels.  OpenCV's 8-bit
// colour conversions and Canny (aperture 3, L1 gradient) are integer algorithms and are restated here from their definitions
// (include/mstg_hip.h spells them out; tests/local_style_ref.py is the same restatement in numpy -- neither has been compared with
// an OpenCV binary).  Three kernels, whatever the batch:
//
// A  local_style_prepare_kernel   one workgroup of 256 threads per 32 x 64 tile.  Gray of the tile + 2 pixels of halo (replicated
//    borders) goes to LDS, the tile's own pixels also get their sky bit (S and V of RGB2HSV; the saturation divisor table is
//    built in LDS with integer round-half-even); the L1 Sobel magnitude of the tile + 1 pixel of halo (0 outside the image) goes
//    to LDS as 16-bit values; each pixel then redoes its own dx, dy, applies the non-maximum suppression and writes the state
//    byte (2 strong, 0 candidate, 1 nothing).  The sky pixels of a tile are summed over the workgroup and added to the image's count
//    by ONE integer atomic per tile (order-free; the host entry zeroes the counts with a memset node before the launch).
// B  local_style_hysteresis_kernel   one workgroup of 1024 threads per image, the whole state map in LDS (one byte per pixel:
//    H * W <= 147456 = 144 KiB of the CU's 160 KiB).  A pass = every thread sweeps its own contiguous run of the flat map (a
//    word at a time: words without a candidate byte are skipped) and promotes each candidate that has a strong 8-neighbour;
//    the promoting thread then WALKS on from that pixel -- promote the first candidate among the 8 neighbours, step onto it,
//    repeat until there is none -- so a thin path of any length and shape is consumed in the pass that first touches it, and a
//    side branch left behind has a strong neighbour for the next pass: the number of passes follows the branching depth of the
//    edge graph, not its length.  States only ever go 0 -> 2, a byte store does not touch its neighbours, and a pass in which
//    no sweep promoted anything read one constant map and checked every candidate in it: that is the fixed point, and it does
//    not depend on the order in which strength spread.  Passes end at a workgroup-wide OR.
// C  local_style_weights_kernel   one workgroup of 256 threads per 16 x 64 tile.  The edge bytes of the tile + 8 pixels of halo
//    (scipy's 'reflect' boundary, for any extent) go to LDS; the fp64 Gaussian (radius 8, sigma 2) runs along axis 0, then
//    along axis 1 over the LDS result, each tap sum in scipy's own order (centre tap, then the symmetric pairs from the
//    outermost inwards, no fused multiply-add); detail = g > 0.1; has_sky is formed from the image's count on the device.
//
// Everything before the Gaussian is integer, nothing uses floating-point atomics, so the three outputs are bit-reproducible.
//
// D  local_style_finish_kernel   the blend with that map and the two finishing steps of the mode (:342-352), one workgroup of 256
//    threads per 32 x 64 tile: x = orig * (1 - w) + styled * w as blend_byte (u8_image.h) forms it (float64, products and sum
//    rounded); enhance_colors = cv2.convertScaleAbs(x, alpha=1.1, beta=5) restated as narrow to float32, ONE fused multiply-add,
//    |.|, round half to even, saturate; smooth = smooth_transitions(radius=3): boundary = dilate != erode of the detail mask over
//    the 9 x 9 window clipped to the image (two iterations of a 5 x 5 box), the 8-bit GaussianBlur 7 x 7 (sigma 0) in OpenCV's
//    8.8 fixed point with BORDER_REFLECT_101, and (e + blur) >> 1 on the boundary.  The smoothing variant keeps the enhanced
//    patch with 3 pixels of halo (recomputed from the mirrored source pixels), the detail patch with 4 (outside the image a pixel
//    is neutral) and the 16-bit horizontally filtered rows in LDS; without smooth the kernel is the per-pixel blend and uses no
//    LDS.  Integer after the colour step, no atomics: bit-reproducible.  Restated from the definitions (include/mstg_hip.h),
//    not compared with an OpenCV binary.
#include "u8_image.h"

namespace mstg {

constexpr int LS_MAX_PIXELS = MSTG_LOCAL_STYLE_MAX_PIXELS;

constexpr int LA_TH = 32, LA_TW = 64, LA_THREADS = 256;
constexpr int LA_GH = LA_TH + 4, LA_GW = LA_TW + 4;  // gray patch: halo 2
constexpr int LA_MH = LA_TH + 2, LA_MW = LA_TW + 2;  // magnitude patch: halo 1
constexpr int LS_LOW = 50, LS_HIGH = 150;            // cv2.Canny(gray, 50, 150)
constexpr int LS_TG22 = 13573;                       // tan(22.5 deg) * 2^15, OpenCV's constant

constexpr int LB_THREADS = 1024;

constexpr int LC_TH = 16, LC_TW = 64, LC_THREADS = 256, LC_R = 8;  // radius = int(4 * sigma + 0.5)
constexpr int LC_EH = LC_TH + 2 * LC_R, LC_EW = LC_TW + 2 * LC_R;
// scipy.ndimage._filters._gaussian_kernel1d(2, 0, 8): exp(-x^2 / 8) / sum, x = 0..8 (numpy's exp and pairwise sum, to the bit)
constexpr double LC_K[LC_R + 1] = {0x1.98862a07ae7b4p-3, 0x1.68856f9ab1982p-3, 0x1.ef9093fc46e5ap-4, 0x1.0941b71ceef37p-4, 0x1.ba4d4125ffd2ap-6,
                                   0x1.1f30504e20207p-7, 0x1.227362b5fc92dp-9, 0x1.c98b8c5d0dda5p-12, 0x1.18aad19e4159bp-14};

__device__ __forceinline__ int sobel_dx(const unsigned char* g) {  // g = the pixel in the gray patch
    return ((int)g[-LA_GW + 1] + 2 * (int)g[1] + (int)g[LA_GW + 1]) - ((int)g[-LA_GW - 1] + 2 * (int)g[-1] + (int)g[LA_GW - 1]);
}
__device__ __forceinline__ int sobel_dy(const unsigned char* g) {
    return ((int)g[LA_GW - 1] + 2 * (int)g[LA_GW] + (int)g[LA_GW + 1]) - ((int)g[-LA_GW - 1] + 2 * (int)g[-LA_GW] + (int)g[-LA_GW + 1]);
}

__global__ __launch_bounds__(LA_THREADS) void local_style_prepare_kernel(const unsigned char* __restrict__ canvas, int H, int W, int tiles_x,
                                                                         int tiles, unsigned char* __restrict__ state,
                                                                         unsigned char* __restrict__ sky, int* __restrict__ sky_count,
                                                                         unsigned char* __restrict__ gray_out) {
    __shared__ int sdiv[256];
    __shared__ unsigned char g[LA_GH * LA_GW];
    __shared__ unsigned short mag[LA_MH * LA_MW];
    __shared__ int wave_cnt[LA_THREADS / WAVE];
    const int tid = threadIdx.x;
    // tile_of (u8_image.h) written out: with the call the compiler schedules this kernel's third loop differently
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * LA_TH, x0 = tx * LA_TW;
    {  // sdiv[i] = cvRound((255 << 12) / i): round half to even, in integers
        int v = 0;
        if (tid > 0) {
            const int q = 1044480 / tid, r = 1044480 - q * tid;
            v = q + ((2 * r > tid || (2 * r == tid && (q & 1))) ? 1 : 0);
        }
        sdiv[tid] = v;
    }
    __syncthreads();
    const size_t plane = (size_t)n * H * W;
    const unsigned char* img = canvas + plane * 3;
    int cnt = 0;
    for (int e = tid; e < LA_GH * LA_GW; e += LA_THREADS) {
        const int r = e / LA_GW, c = e - r * LA_GW;
        const int py = y0 - 2 + r, px = x0 - 2 + c;
        const int cy = min(max(py, 0), H - 1), cx = min(max(px, 0), W - 1);  // BORDER_REPLICATE
        const unsigned char* p = img + ((size_t)cy * W + cx) * 3;
        const int R = p[0], G = p[1], B = p[2];
        const int gr = (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14;
        g[e] = (unsigned char)gr;
        if (r >= 2 && r < LA_TH + 2 && c >= 2 && c < LA_TW + 2 && py < H && px < W) {  // a pixel this tile owns
            const int v = max(R, max(G, B)), diff = v - min(R, min(G, B));
            const int s = (diff * sdiv[v] + 2048) >> 12;
            const int is_sky = (v > 150 && s < 100) ? 1 : 0;
            const size_t idx = plane + (size_t)py * W + px;
            sky[idx] = (unsigned char)is_sky;
            if (gray_out) gray_out[idx] = (unsigned char)gr;
            cnt += is_sky;
        }
    }
    __syncthreads();
    for (int e = tid; e < LA_MH * LA_MW; e += LA_THREADS) {
        const int r = e / LA_MW, c = e - r * LA_MW;
        const int py = y0 - 1 + r, px = x0 - 1 + c;
        int m = 0;  // the magnitude counts as 0 outside the image
        if ((unsigned)py < (unsigned)H && (unsigned)px < (unsigned)W) {
            const unsigned char* gp = &g[(r + 1) * LA_GW + (c + 1)];
            m = abs(sobel_dx(gp)) + abs(sobel_dy(gp));
        }
        mag[e] = (unsigned short)m;  // <= 2040
    }
    __syncthreads();
    for (int e = tid; e < LA_TH * LA_TW; e += LA_THREADS) {
        const int r = e / LA_TW, c = e - r * LA_TW;
        const int py = y0 + r, px = x0 + c;
        if (py >= H || px >= W) continue;
        const unsigned char* gp = &g[(r + 2) * LA_GW + (c + 2)];
        const unsigned short* mp = &mag[(r + 1) * LA_MW + (c + 1)];
        const int dx = sobel_dx(gp), dy = sobel_dy(gp);
        const int m = mp[0];
        int st = 1;
        if (m > LS_LOW) {
            const int x = abs(dx), y = abs(dy) << 15, t = x * LS_TG22;
            bool keep;
            if (y < t) {
                keep = m > mp[-1] && m >= mp[1];
            } else if (y > t + (x << 16)) {
                keep = m > mp[-LA_MW] && m >= mp[LA_MW];
            } else {
                const int s = (dx ^ dy) < 0 ? -1 : 1;
                keep = m > mp[-LA_MW - s] && m > mp[LA_MW + s];
            }
            if (keep) st = m > LS_HIGH ? 2 : 0;
        }
        state[plane + (size_t)py * W + px] = (unsigned char)st;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((tid & 63) == 0) wave_cnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        const int total = (wave_cnt[0] + wave_cnt[1]) + (wave_cnt[2] + wave_cnt[3]);
        if (total) atomicAdd(&sky_count[n], total);
    }
}

// Bit k set where neighbour k of pixel i = (y, x) exists and holds `what`; k: 0 left, 1 right, 2 up, 3 down, 4 up-left, 5 up-right,
// 6 down-left, 7 down-right.  Eight independent LDS reads (a missing neighbour reads the pixel itself and is masked out).
__device__ __forceinline__ unsigned neighbours_holding(const unsigned char* st, int i, int y, int x, int H, int W, unsigned what) {
    const bool l = x > 0, r = x < W - 1, u = y > 0, d = y < H - 1;
    const unsigned a0 = st[l ? i - 1 : i], a1 = st[r ? i + 1 : i], a2 = st[u ? i - W : i], a3 = st[d ? i + W : i];
    const unsigned a4 = st[u && l ? i - W - 1 : i], a5 = st[u && r ? i - W + 1 : i];
    const unsigned a6 = st[d && l ? i + W - 1 : i], a7 = st[d && r ? i + W + 1 : i];
    return (unsigned)(l && a0 == what) | (unsigned)(r && a1 == what) << 1 | (unsigned)(u && a2 == what) << 2 |
           (unsigned)(d && a3 == what) << 3 | (unsigned)(u && l && a4 == what) << 4 | (unsigned)(u && r && a5 == what) << 5 |
           (unsigned)(d && l && a6 == what) << 6 | (unsigned)(d && r && a7 == what) << 7;
}

__device__ __forceinline__ bool has_zero_byte(unsigned v) { return ((v - 0x01010101u) & ~v & 0x80808080u) != 0; }

__global__ __launch_bounds__(LB_THREADS) void local_style_hysteresis_kernel(const unsigned char* __restrict__ state, int H, int W,
                                                                            unsigned char* __restrict__ edge) {
    extern __shared__ __align__(16) unsigned char st[];  // 4 * words bytes; the bytes past H * W hold 1
    unsigned* sw = reinterpret_cast<unsigned*>(st);
    const int tid = threadIdx.x;
    const int HW = H * W, words = (HW + 3) >> 2;
    const unsigned char* src = state + (size_t)blockIdx.x * HW;
    unsigned char* dst = edge + (size_t)blockIdx.x * HW;
    const bool src_al = ((uintptr_t)src & 3) == 0, dst_al = ((uintptr_t)dst & 3) == 0;
    for (int w = tid; w < words; w += LB_THREADS) {
        unsigned v;
        if (src_al && 4 * w + 4 <= HW) {
            v = *reinterpret_cast<const unsigned*>(src + 4 * w);
        } else {
            v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) v |= (4 * w + b < HW ? (unsigned)src[4 * w + b] : 1u) << (8 * b);
        }
        sw[w] = v;
    }
    __syncthreads();

    // this thread's run of the flat map (an odd number of words per thread: the lanes of a wave then start in different banks)
    const int wpt = ((words + LB_THREADS - 1) / LB_THREADS) | 1;
    const int w0 = min(tid * wpt, words), w1 = min(w0 + wpt, words);

    int any;
    do {
        int changed = 0;
        if (w0 < w1) {
            int y = (4 * w0) / W, rs = y * W;  // row of the pixel under the cursor and its first flat index
            for (int w = w0; w < w1; ++w) {
                if (!has_zero_byte(sw[w])) continue;
                for (int b = 0; b < 4; ++b) {
                    const int i = 4 * w + b;
                    if (st[i] != 0) continue;  // re-read: a walk may have promoted it meanwhile; the padding holds 1
                    while (i >= rs + W) {
                        rs += W;
                        ++y;
                    }
                    if (neighbours_holding(st, i, y, i - rs, H, W, 2u) == 0) continue;
                    st[i] = 2;
                    changed = 1;
                    // follow the path from here: promote the first candidate among the neighbours, step onto it, repeat
                    int ci = i, cy = y, cx = i - rs;
                    for (;;) {
                        const unsigned m = neighbours_holding(st, ci, cy, cx, H, W, 0u);
                        if (m == 0) break;
                        const unsigned k = (unsigned)__ffs((int)m) - 1u;
                        cy += (int)((0xC8u >> k) & 1u) - (int)((0x34u >> k) & 1u);  // down: k = 3, 6, 7; up: k = 2, 4, 5
                        cx += (int)((0xA2u >> k) & 1u) - (int)((0x51u >> k) & 1u);  // right: k = 1, 5, 7; left: k = 0, 4, 6
                        ci = cy * W + cx;
                        st[ci] = 2;
                    }
                }
            }
        }
        any = __syncthreads_or(changed);
    } while (any);

    for (int w = tid; w < words; w += LB_THREADS) {
        const unsigned v = sw[w];
        unsigned o = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) o |= (((v >> (8 * b)) & 0xffu) == 2u ? 1u : 0u) << (8 * b);
        if (dst_al && 4 * w + 4 <= HW) {
            *reinterpret_cast<unsigned*>(dst + 4 * w) = o;
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (4 * w + b < HW) dst[4 * w + b] = (unsigned char)((o >> (8 * b)) & 0xffu);
        }
    }
}

// scipy.ndimage 'reflect' (d c b a | a b c d | d c b a), for any distance from the array
__device__ __forceinline__ int reflect_index(int i, int n) {
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

__global__ __launch_bounds__(LC_THREADS) void local_style_weights_kernel(const unsigned char* __restrict__ edge,
                                                                         const unsigned char* __restrict__ sky,
                                                                         const int* __restrict__ sky_count, int H, int W, int tiles_x,
                                                                         int tiles, double w_base, double w_sky, double w_detail,
                                                                         double* __restrict__ wmap, unsigned char* __restrict__ detail) {
#pragma clang fp contract(off)  // scipy rounds every product and every sum; g is compared with 0.1, the ratio with 0.7
    __shared__ unsigned char ed[LC_EH * LC_EW];
    __shared__ double col[LC_TH * LC_EW];
    const int tid = threadIdx.x;
    const auto [n, y0, x0] = tile_of<LC_TH, LC_TW>(tiles, tiles_x);
    const size_t plane = (size_t)n * H * W;
    const unsigned char* e_img = edge + plane;
    for (int e = tid; e < LC_EH * LC_EW; e += LC_THREADS) {
        const int r = e / LC_EW, c = e - r * LC_EW;
        const int sy = reflect_index(y0 - LC_R + r, H), sx = reflect_index(x0 - LC_R + c, W);
        ed[e] = e_img[(size_t)sy * W + sx] != 0 ? 1 : 0;
    }
    __syncthreads();
    for (int e = tid; e < LC_TH * LC_EW; e += LC_THREADS) {  // axis 0 first
        const int r = e / LC_EW, c = e - r * LC_EW;
        const unsigned char* p = &ed[(r + LC_R) * LC_EW + c];
        double t = (double)p[0] * LC_K[0];
#pragma unroll
        for (int k = LC_R; k >= 1; --k) t += ((double)p[-k * LC_EW] + (double)p[k * LC_EW]) * LC_K[k];
        col[e] = t;
    }
    __syncthreads();
    const double ratio = (double)sky_count[n] / (double)((long long)H * W);
    const bool has_sky = ratio > 0.7;
    for (int e = tid; e < LC_TH * LC_TW; e += LC_THREADS) {
        const int r = e / LC_TW, c = e - r * LC_TW;
        const int py = y0 + r, px = x0 + c;
        if (py >= H || px >= W) continue;
        const double* p = &col[r * LC_EW + c + LC_R];
        double t = p[0] * LC_K[0];
#pragma unroll
        for (int k = LC_R; k >= 1; --k) t += (p[-k] + p[k]) * LC_K[k];
        const bool det = t > 0.1;
        const size_t idx = plane + (size_t)py * W + px;
        double w = w_base;
        if (has_sky && sky[idx]) w = w_sky;
        if (det) w = w_detail;  // the detail weight is assigned last in the reference and overrides the sky weight
        wmap[idx] = w;
        if (detail) detail[idx] = det ? 1 : 0;
    }
}

constexpr int LD_TH = LA_TH, LD_TW = LA_TW, LD_THREADS = 256;
constexpr int LD_RB = 3, LD_RM = 4;                              // blur radius (7 taps), morphology radius (9 x 9)
constexpr int LD_EH = LD_TH + 2 * LD_RB, LD_EW = LD_TW + 2 * LD_RB;  // enhanced patch
constexpr int LD_EWP = LD_TW + 8;  // its row pitch in LDS: the item of the last four columns reads three whole dwords
constexpr int LD_DH = LD_TH + 2 * LD_RM, LD_DW = LD_TW + 2 * LD_RM;  // detail patch
static_assert(LD_EWP >= LD_EW && LD_EWP % 4 == 0 && LD_DW == LD_TW + 8 && LD_TW % 4 == 0, "dword passes of the finish kernel");

// One channel of one pixel: the blend in float64, then either its clip and truncation (blend_byte, u8_image.h) or the
// convertScaleAbs restatement on the unclipped sum.
template <bool ENHANCE>
__device__ __forceinline__ unsigned char finish_channel(unsigned char o, unsigned char s, double w0, double w1) {
#pragma clang fp contract(off)  // numpy rounds each product and the sum
    if (!ENHANCE) return (unsigned char)blend_byte(o, s, w0, w1);
    const double a = (double)o * w0;
    const double b = (double)s * w1;
    const double r = a + b;
    float t = fabsf(__builtin_fmaf((float)r, 1.1f, 5.0f));  // the one fused multiply-add of the definition
    if (!(t == t)) t = 0.f;                                 // a NaN weight: keep the byte defined here too
    t = fminf(__builtin_rintf(t), 255.f);                   // round half to even, saturate (t >= 0)
    return (unsigned char)t;
}

template <bool ENHANCE, bool SMOOTH>
__global__ __launch_bounds__(LD_THREADS) void local_style_finish_kernel(const unsigned char* __restrict__ canvas,
                                                                        const unsigned char* __restrict__ styled,
                                                                        const double* __restrict__ wmap,
                                                                        const unsigned char* __restrict__ detail, int H, int W, int tiles_x,
                                                                        int tiles, unsigned char* __restrict__ out) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const auto [n, y0, x0] = tile_of<LD_TH, LD_TW>(tiles, tiles_x);
    const size_t plane = (size_t)n * H * W;
    const unsigned char* c_img = canvas + plane * 3;
    const unsigned char* s_img = styled + plane * 3;
    const double* w_img = wmap + plane;
    unsigned char* o_img = out + plane * 3;
    if (!SMOOTH) {
        for (int e = tid; e < LD_TH * LD_TW; e += LD_THREADS) {
            const int r = e / LD_TW, c = e - r * LD_TW;
            const int py = y0 + r, px = x0 + c;
            if (py >= H || px >= W) continue;
            const size_t i = (size_t)py * W + px;
            const double w1 = w_img[i], w0 = 1.0 - w1;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) o_img[i * 3 + ch] = finish_channel<ENHANCE>(c_img[i * 3 + ch], s_img[i * 3 + ch], w0, w1);
        }
        return;
    }
    // LDS: planes per channel, rows padded to whole dwords, so the two horizontal passes read dwords and make four outputs each
    __shared__ __align__(16) unsigned char en[3 * LD_EH * LD_EWP];    // the enhanced image, halo 3
    __shared__ __align__(16) unsigned char dm[LD_DH * LD_DW];         // detail: 1 = set, 2 = clear, 0 = outside the image (neutral)
    __shared__ __align__(16) unsigned char dh[LD_DH * LD_TW];         // OR of dm over the 9 columns of the window
    __shared__ __align__(16) unsigned short hz[3 * LD_EH * LD_TW];    // the horizontally filtered rows, exact (<= 65280)
    const unsigned char* d_img = detail + plane;
    for (int e = tid; e < LD_EH * LD_EW; e += LD_THREADS) {
        const int r = e / LD_EW, c = e - r * LD_EW;
        int sy = y0 - LD_RB + r, sx = x0 - LD_RB + c;
        if ((unsigned)sy >= (unsigned)H) sy = reflect101(sy, H);
        if ((unsigned)sx >= (unsigned)W) sx = reflect101(sx, W);
        const size_t i = (size_t)sy * W + sx;
        const double w1 = w_img[i], w0 = 1.0 - w1;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            en[(ch * LD_EH + r) * LD_EWP + c] = finish_channel<true>(c_img[i * 3 + ch], s_img[i * 3 + ch], w0, w1);
    }
    for (int e = tid; e < LD_DH * LD_DW; e += LD_THREADS) {
        const int r = e / LD_DW, c = e - r * LD_DW;
        const int py = y0 - LD_RM + r, px = x0 - LD_RM + c;
        unsigned char v = 0;
        if ((unsigned)py < (unsigned)H && (unsigned)px < (unsigned)W) v = d_img[(size_t)py * W + px] != 0 ? 1 : 2;
        dm[e] = v;
    }
    __syncthreads();
    for (int e = tid; e < LD_DH * (LD_TW / 4); e += LD_THREADS) {  // four columns per item: bytes c .. c + 11 of the row
        const int r = e / (LD_TW / 4), c = 4 * (e - r * (LD_TW / 4));
        const unsigned* p = reinterpret_cast<const unsigned*>(&dm[r * LD_DW + c]);
        const unsigned a = p[0], b = p[1], d = p[2];
        const unsigned mid = (a >> 24) | b | (b >> 8) | (b >> 16) | (b >> 24) | d;  // bytes 3 .. 8 (in the low byte)
        const unsigned o0 = a | (a >> 8) | (a >> 16) | mid;                          // 0 .. 8
        const unsigned o1 = (a >> 8) | (a >> 16) | mid | (d >> 8);                   // 1 .. 9
        const unsigned o2 = (a >> 16) | mid | (d >> 8) | (d >> 16);                  // 2 .. 10
        const unsigned o3 = mid | (d >> 8) | (d >> 16) | (d >> 24);                  // 3 .. 11
        *reinterpret_cast<unsigned*>(&dh[r * LD_TW + c]) = (o0 & 3u) | (o1 & 3u) << 8 | (o2 & 3u) << 16 | (o3 & 3u) << 24;
    }
    for (int e = tid; e < 3 * LD_EH * (LD_TW / 4); e += LD_THREADS) {  // four columns per item: bytes c .. c + 9 of the plane row
        const int row = e / (LD_TW / 4), c = 4 * (e - row * (LD_TW / 4));  // row = channel * LD_EH + patch row
        const unsigned* p = reinterpret_cast<const unsigned*>(&en[row * LD_EWP + c]);
        const unsigned w[3] = {p[0], p[1], p[2]};
        int px[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) px[k] = (int)((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
        unsigned short o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int sum = 0;
#pragma unroll
            for (int k = 0; k <= 2 * LD_RB; ++k) sum += gauss_q8_tap<2 * LD_RB + 1>(k) * px[j + k];
            o[j] = (unsigned short)sum;
        }
        *reinterpret_cast<uint2*>(&hz[row * LD_TW + c]) = make_uint2((unsigned)o[0] | (unsigned)o[1] << 16, (unsigned)o[2] | (unsigned)o[3] << 16);
    }
    __syncthreads();
    for (int e = tid; e < LD_TH * LD_TW; e += LD_THREADS) {
        const int r = e / LD_TW, c = e - r * LD_TW;
        const int py = y0 + r, px = x0 + c;
        if (py >= H || px >= W) continue;
        unsigned v = 0;
#pragma unroll
        for (int k = 0; k <= 2 * LD_RM; ++k) v |= dh[(r + k) * LD_TW + c];
        const bool boundary = v == 3u;  // the window holds a set and a clear pixel: dilate != erode
        const size_t i = ((size_t)py * W + px) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            int o = en[(ch * LD_EH + r + LD_RB) * LD_EWP + c + LD_RB];
            if (boundary) {
                const unsigned short* hp = &hz[(ch * LD_EH + r) * LD_TW + c];
                int sum = 0;
#pragma unroll
                for (int k = 0; k <= 2 * LD_RB; ++k) sum += gauss_q8_tap<2 * LD_RB + 1>(k) * (int)hp[k * LD_TW];
                o = (o + ((sum + 32768) >> 16)) >> 1;
            }
            o_img[i + ch] = (unsigned char)o;
        }
    }
}

// ---- host side: every check returns 0 = fine, else the error code (message set) -----------------------------------------------
static_assert(LC_TH == 16 && LC_TW == 64, "check_shape_16x64 counts the tiles of the weights kernel, the finer of the two tilings");

static int ls_prepare(const unsigned char* canvas, int N, int H, int W, unsigned char* state, unsigned char* sky, int* sky_count,
                      unsigned char* gray, hipStream_t st) {
    hipError_t e = hipMemsetAsync(sky_count, 0, (size_t)N * sizeof(int), st);
    if (e != hipSuccess) return fail_launch(e, "local_style_prepare: hipMemsetAsync(sky_count)");
    const int tx = cdiv(W, LA_TW), tiles = tx * cdiv(H, LA_TH);
    MSTG_LAUNCH(local_style_prepare_kernel, dim3((unsigned)(N * tiles)), dim3(LA_THREADS), 0, st, canvas, H, W, tx, tiles, state, sky,
                sky_count, gray);
    MSTG_CHECK_LAUNCH("local_style_prepare_kernel");
    return MSTG_OK;
}

static int ls_hysteresis(const unsigned char* state, int N, int H, int W, unsigned char* edge, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&local_style_hysteresis_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, LS_MAX_PIXELS);
        if (e != hipSuccess) return fail_launch(e, "hipFuncSetAttribute(local_style_hysteresis_kernel)");
        attr_set = true;
    }
    const size_t lds = (size_t)(((H * W + 3) >> 2) << 2);
    MSTG_LAUNCH(local_style_hysteresis_kernel, dim3((unsigned)N), dim3(LB_THREADS), lds, st, state, H, W, edge);
    MSTG_CHECK_LAUNCH("local_style_hysteresis_kernel");
    return MSTG_OK;
}

static int ls_weights(const unsigned char* edge, const unsigned char* sky, const int* sky_count, int N, int H, int W, double w_base,
                      double w_sky, double w_detail, double* weight_map, unsigned char* detail, hipStream_t st) {
    const int tx = cdiv(W, LC_TW), tiles = tx * cdiv(H, LC_TH);
    MSTG_LAUNCH(local_style_weights_kernel, dim3((unsigned)(N * tiles)), dim3(LC_THREADS), 0, st, edge, sky, sky_count, H, W, tx, tiles,
                w_base, w_sky, w_detail, weight_map, detail);
    MSTG_CHECK_LAUNCH("local_style_weights_kernel");
    return MSTG_OK;
}

static int ls_finish(const unsigned char* canvas, const unsigned char* styled, const double* weight_map, const unsigned char* detail, int N,
                     int H, int W, int enhance, int smooth, unsigned char* out, hipStream_t st) {
    const int tx = cdiv(W, LD_TW), tiles = tx * cdiv(H, LD_TH);
    const dim3 grid((unsigned)(N * tiles)), block(LD_THREADS);
    if (smooth)
        MSTG_LAUNCH((local_style_finish_kernel<true, true>), grid, block, 0, st, canvas, styled, weight_map, detail, H, W, tx, tiles, out);
    else if (enhance)
        MSTG_LAUNCH((local_style_finish_kernel<true, false>), grid, block, 0, st, canvas, styled, weight_map, detail, H, W, tx, tiles, out);
    else
        MSTG_LAUNCH((local_style_finish_kernel<false, false>), grid, block, 0, st, canvas, styled, weight_map, detail, H, W, tx, tiles, out);
    MSTG_CHECK_LAUNCH("local_style_finish_kernel");
    return MSTG_OK;
}

// smooth without enhance_colors is refused by name; 0 = fine
static int ls_flags(const char* who, int enhance, int smooth) {
    if (smooth && !enhance) {
        char msg[256];
        snprintf(msg, sizeof(msg),
                 "%s: smooth without enhance_colors is not built: there cv2.GaussianBlur runs on the float64 blend and OpenCV's "
                 "summation order decides bytes",
                 who);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    return MSTG_OK;
}

// the layout of the workspace of mstg_local_style_weight_map and, with the weight map and the detail mask, mstg_local_style_enhanced
struct LsWorkspace {
    size_t weight, state, sky, edge, detail, count, total;
};
static LsWorkspace ls_workspace(int N, int H, int W, bool enhanced) {
    const size_t px = (size_t)N * H * W, plane = align16(px);
    LsWorkspace w;
    w.weight = 0;
    w.state = enhanced ? align16(px * sizeof(double)) : 0;
    w.sky = w.state + plane;
    w.edge = w.sky + plane;
    w.detail = w.edge + plane;
    w.count = w.detail + (enhanced ? plane : 0);
    w.total = w.count + align16((size_t)N * sizeof(int));
    return w;
}

// shape and hysteresis limit of an entry that runs, or sizes the workspace of, the whole chain
static int ls_chain_shape(const char* who, int N, int H, int W) {
    const int rc = check_shape_16x64(who, N, H, W);
    return rc != MSTG_OK ? rc : fits_hysteresis_lds(who, H, W, "");
}

}  // namespace mstg

using namespace mstg;

extern "C" size_t mstg_local_style_workspace_bytes(int N, int H, int W) {
    if (ls_chain_shape("local_style_workspace_bytes", N, H, W) != MSTG_OK) return 0;
    return ls_workspace(N, H, W, false).total;
}

extern "C" int mstg_local_style_prepare(const unsigned char* canvas, int N, int H, int W, unsigned char* state, unsigned char* sky,
                                        int* sky_count, unsigned char* gray, void* stream) {
    if (!canvas || !state || !sky || !sky_count) return fail_arg(MSTG_E_BADARG, "local_style_prepare: null canvas, state, sky or count pointer");
    const int rc = check_shape_16x64("local_style_prepare", N, H, W);
    if (rc != MSTG_OK) return rc;
    if ((uintptr_t)sky_count & 3) return fail_arg(MSTG_E_ALIGN, "local_style_prepare: sky_count not 4-byte aligned");
    return ls_prepare(canvas, N, H, W, state, sky, sky_count, gray, (hipStream_t)stream);
}

extern "C" int mstg_local_style_hysteresis(const unsigned char* state, int N, int H, int W, unsigned char* edge, void* stream) {
    if (!state || !edge) return fail_arg(MSTG_E_BADARG, "local_style_hysteresis: null state or edge pointer");
    const int rc = ls_chain_shape("local_style_hysteresis", N, H, W);
    if (rc != MSTG_OK) return rc;
    return ls_hysteresis(state, N, H, W, edge, (hipStream_t)stream);
}

extern "C" int mstg_local_style_weights(const unsigned char* edge, const unsigned char* sky, const int* sky_count, int N, int H, int W,
                                        double w_base, double w_sky, double w_detail, double* weight_map, unsigned char* detail,
                                        void* stream) {
    if (!edge || !sky || !sky_count || !weight_map) return fail_arg(MSTG_E_BADARG, "local_style_weights: null edge, sky, count or map pointer");
    const int rc = check_shape_16x64("local_style_weights", N, H, W);
    if (rc != MSTG_OK) return rc;
    if (((uintptr_t)weight_map & 7) || ((uintptr_t)sky_count & 3))
        return fail_arg(MSTG_E_ALIGN, "local_style_weights: weight_map not 8-byte or sky_count not 4-byte aligned");
    return ls_weights(edge, sky, sky_count, N, H, W, w_base, w_sky, w_detail, weight_map, detail, (hipStream_t)stream);
}

extern "C" int mstg_local_style_weight_map(const unsigned char* canvas, int N, int H, int W, double w_base, double w_sky, double w_detail,
                                           double* weight_map, void* workspace, size_t workspace_bytes, void* stream) {
    if (!canvas || !weight_map) return fail_arg(MSTG_E_BADARG, "local_style_weight_map: null canvas or map pointer");
    int rc = ls_chain_shape("local_style_weight_map", N, H, W);
    if (rc != MSTG_OK) return rc;
    const LsWorkspace ws = ls_workspace(N, H, W, false);
    if (!workspace || workspace_bytes < ws.total) return fail_arg(MSTG_E_WORKSPACE, "local_style_weight_map: workspace too small");
    if (((uintptr_t)workspace & 15) || ((uintptr_t)weight_map & 7))
        return fail_arg(MSTG_E_ALIGN, "local_style_weight_map: workspace not 16-byte or weight_map not 8-byte aligned");
    unsigned char* base = (unsigned char*)workspace;
    unsigned char *state = base + ws.state, *sky = base + ws.sky, *edge = base + ws.edge;
    int* count = (int*)(base + ws.count);
    hipStream_t st = (hipStream_t)stream;
    rc = ls_prepare(canvas, N, H, W, state, sky, count, nullptr, st);
    if (rc == MSTG_OK) rc = ls_hysteresis(state, N, H, W, edge, st);
    if (rc == MSTG_OK) rc = ls_weights(edge, sky, count, N, H, W, w_base, w_sky, w_detail, weight_map, nullptr, st);
    return rc;
}

extern "C" int mstg_local_style_finish(const unsigned char* canvas, const unsigned char* styled, const double* weight_map,
                                       const unsigned char* detail, int N, int H, int W, int enhance_colors, int smooth, unsigned char* out,
                                       void* stream) {
    if (!canvas || !styled || !weight_map || !out) return fail_arg(MSTG_E_BADARG, "local_style_finish: null canvas, styled, map or out pointer");
    int rc = check_shape_16x64("local_style_finish", N, H, W);
    if (rc == MSTG_OK) rc = ls_flags("local_style_finish", enhance_colors, smooth);
    if (rc != MSTG_OK) return rc;
    if (smooth && !detail) return fail_arg(MSTG_E_BADARG, "local_style_finish: smooth needs the detail mask");
    if ((uintptr_t)weight_map & 7) return fail_arg(MSTG_E_ALIGN, "local_style_finish: weight_map not 8-byte aligned");
    const size_t px = (size_t)N * H * W;
    if (overlaps(out, px * 3, canvas, px * 3) || overlaps(out, px * 3, styled, px * 3) || overlaps(out, px * 3, weight_map, px * 8) ||
        (smooth && overlaps(out, px * 3, detail, px)))
        return fail_arg(MSTG_E_BADARG, "local_style_finish: out overlaps an input (the smoothing reads neighbours of every pixel)");
    return ls_finish(canvas, styled, weight_map, detail, N, H, W, enhance_colors, smooth, out, (hipStream_t)stream);
}

extern "C" size_t mstg_local_style_enhanced_workspace_bytes(int N, int H, int W) {
    if (ls_chain_shape("local_style_enhanced_workspace_bytes", N, H, W) != MSTG_OK) return 0;
    return ls_workspace(N, H, W, true).total;
}

extern "C" int mstg_local_style_enhanced(const unsigned char* canvas, const unsigned char* styled, int N, int H, int W, double w_base,
                                         double w_sky, double w_detail, int enhance_colors, int smooth, unsigned char* out, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    if (!canvas || !styled || !out) return fail_arg(MSTG_E_BADARG, "local_style_enhanced: null canvas, styled or out pointer");
    int rc = ls_chain_shape("local_style_enhanced", N, H, W);
    if (rc == MSTG_OK) rc = ls_flags("local_style_enhanced", enhance_colors, smooth);
    if (rc != MSTG_OK) return rc;
    const LsWorkspace ws = ls_workspace(N, H, W, true);
    if (!workspace || workspace_bytes < ws.total) return fail_arg(MSTG_E_WORKSPACE, "local_style_enhanced: workspace too small");
    if ((uintptr_t)workspace & 15) return fail_arg(MSTG_E_ALIGN, "local_style_enhanced: workspace not 16-byte aligned");
    const size_t px = (size_t)N * H * W;
    if (overlaps(out, px * 3, canvas, px * 3) || overlaps(out, px * 3, styled, px * 3) || overlaps(out, px * 3, workspace, ws.total))
        return fail_arg(MSTG_E_BADARG, "local_style_enhanced: out overlaps an input or the workspace");
    unsigned char* base = (unsigned char*)workspace;
    double* wm = (double*)(base + ws.weight);
    unsigned char *state = base + ws.state, *sky = base + ws.sky, *edge = base + ws.edge, *det = base + ws.detail;
    int* count = (int*)(base + ws.count);
    hipStream_t st = (hipStream_t)stream;
    rc = ls_prepare(canvas, N, H, W, state, sky, count, nullptr, st);
    if (rc == MSTG_OK) rc = ls_hysteresis(state, N, H, W, edge, st);
    if (rc == MSTG_OK) rc = ls_weights(edge, sky, count, N, H, W, w_base, w_sky, w_detail, wm, det, st);
    if (rc == MSTG_OK) rc = ls_finish(canvas, styled, wm, det, N, H, W, enhance_colors, smooth, out, st);
    return rc;
}
