// The colour-block repair of the reference (improved_smooth.py:137-164 fix_color_blocks_improved) on the device, for a batch of
// (N, H, W, 3) uint8 images (any H, W >= 1): the block mask (:53-95: the a and b planes of the 8-bit COLOR_RGB2LAB, Sobel, magnitude,
// threshold, box dilation), the correction towards the window mean (:10-51), cv2.bilateralFilter(img, 0, 0.4 * 255, 60) (:97-112,
// radius 90: 25 445 taps per pixel) and the detail blend (:114-135: a float64 GaussianBlur of the original).  Every OpenCV step is
// restated from the definition in include/mstg_hip.h (tests/color_blocks_ref.py is the same restatement in numpy -- neither has
// been compared with an OpenCV binary).  Seven kernels, every one takes N images per launch:
//
// E  cb_edge_kernel        one thread per pixel; the gamma and cube-root tables (16-bit, from the host: mstg_lab_tables) in LDS; a
//    and b of the 3 x 3 neighbourhood (BORDER_REFLECT_101), the two Sobel pairs (integers in float32: exact), two correctly
//    rounded square roots, (m_a + m_b) * 0.5f > threshold.
// D  cb_dilate_kernel      one thread per pixel: any edge in the k x k window clipped to the image.
// R  cb_rowsum_kernel      one thread per pixel: the three channel sums over the 2 r + 1 columns of the window clipped to the
//    image, exact in uint32.
// C  cb_correct_kernel     one thread per pixel: an unflagged pixel is copied; a flagged one sums the row sums over the rows of
//    its window, divides once in float64 and blends 0.5 / 0.5, truncated.
// W  cb_bilateral_wide_kernel   the hot one.  A workgroup of four waves covers a band of 4 rows x 256 columns, a wave one row of
//    it, a lane four neighbouring pixels (its 16 accumulators live in registers).  Skewed schedule: at step s the workgroup holds
//    input row y0 - radius + s in LDS and wave w processes tap row i = s - radius - w, so all four waves read the same row; the
//    rows are double-buffered (the next one is loaded from global memory while this one is used; one barrier per step), and a
//    wave idles for 3 of the 2 * radius + 4 steps.  Within a row a lane slides along j = -jmax(i) .. jmax(i): one LDS read of a
//    packed pixel serves four taps.  The row is stored de-interleaved (column e at (e & 3) * pitch + (e >> 2)) so that the lanes of
//    a wave, which read columns 4 apart, hit consecutive banks.  i and j are the same for the whole wave: the space weight,
//    indexed by i * i + j * j, is a scalar load and the loop does not diverge.  Per tap bilateral_tap (u8_image.h), as in
//    standard_bilateral_kernel: v_sad_u8, one LDS gather of the colour weight, one rounded product, wsum, three __fmaf_rn; the tap
//    order per pixel is the definition's (i, then j).
// H  cb_blur_row_kernel    one thread per pixel: the float64 row pass of cv2.GaussianBlur on the three channels, left to right.
// B  cb_detail_blend_kernel one thread per pixel: the column pass (centre, then the nearest pair first), detail = orig - blurred,
//    ((img * w_img) + (orig * alpha)) + (detail * beta), clip, truncate.  Contraction off in both.
//
// The device never evaluates exp, pow or cbrt: every table comes from a host-only entry.  Integer arithmetic or a fixed
// floating-point order everywhere, no atomics: bit-reproducible and independent of N.
#include <cmath>

#include "u8_image.h"

namespace mstg {

constexpr int CB_THREADS = 256;
constexpr int CB_GAMMA = 256, CB_CBRT = 3072, CB_COEF = CB_GAMMA + CB_CBRT;  // layout of the Lab table (16-bit entries)
static_assert(CB_COEF + 9 <= MSTG_LAB_TABLE_U16, "the Lab table holds gamma, cbrt and the nine coefficients");
constexpr int BW_TH = 4, BW_PX = 4, BW_TW = WAVE * BW_PX;  // band of the wide bilateral: a wave per row, four pixels per lane
constexpr int BW_RMAX = MSTG_BILATERAL_WIDE_MAX_RADIUS;
constexpr int BW_ROW = BW_TW + 2 * BW_RMAX;  // columns of a row in LDS at the largest radius
constexpr int BW_PITCH = (BW_ROW + 3) / 4;   // de-interleaved: four runs of this many words
constexpr int BW_COLOR = MSTG_BILATERAL_COLOR_WEIGHTS;
static_assert(BW_TH * WAVE == CB_THREADS && 2 * CB_THREADS >= BW_ROW, "a wave per band row; two columns of the LDS row per thread");
static_assert(MSTG_BILATERAL_WIDE_TABLE_FLOATS == BW_COLOR + BW_RMAX * BW_RMAX + 1, "colour weights, then space weights by i*i + j*j");

// ---- E: the block edges ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CB_THREADS) void cb_edge_kernel(const unsigned char* __restrict__ in, const unsigned short* __restrict__ tab,
                                                             float threshold, int H, int W, size_t total, unsigned char* __restrict__ edge) {
    __shared__ unsigned short gam[CB_GAMMA], cbr[CB_CBRT];
    __shared__ int coef[9];
    const int tid = threadIdx.x;
    gam[tid] = tab[tid];
    for (int e = tid; e < CB_CBRT; e += CB_THREADS) cbr[e] = tab[CB_GAMMA + e];
    if (tid < 9) coef[tid] = tab[CB_COEF + tid];
    __syncthreads();
    const size_t idx = (size_t)blockIdx.x * CB_THREADS + tid;
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
    float a[3][3], b[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned char* p = img + ((size_t)ys[r] * W + xs[c]) * 3;
            const int R = gam[p[0]], G = gam[p[1]], B = gam[p[2]];
            const int fx = cbr[(R * coef[0] + G * coef[1] + B * coef[2] + 2048) >> 12];
            const int fy = cbr[(R * coef[3] + G * coef[4] + B * coef[5] + 2048) >> 12];
            const int fz = cbr[(R * coef[6] + G * coef[7] + B * coef[8] + 2048) >> 12];
            const int av = (500 * (fx - fy) + 128 * 32768 + 16384) >> 15;  // arithmetic shift of the signed sum
            const int bv = (200 * (fy - fz) + 128 * 32768 + 16384) >> 15;
            a[r][c] = (float)min(max(av, 0), 255);
            b[r][c] = (float)min(max(bv, 0), 255);
        }
    // integers of at most 1020 in float32: every sum is exact, in any order
    const float agx = (a[0][2] + 2.f * a[1][2] + a[2][2]) - (a[0][0] + 2.f * a[1][0] + a[2][0]);
    const float agy = (a[2][0] + 2.f * a[2][1] + a[2][2]) - (a[0][0] + 2.f * a[0][1] + a[0][2]);
    const float bgx = (b[0][2] + 2.f * b[1][2] + b[2][2]) - (b[0][0] + 2.f * b[1][0] + b[2][0]);
    const float bgy = (b[2][0] + 2.f * b[2][1] + b[2][2]) - (b[0][0] + 2.f * b[0][1] + b[0][2]);
    const float ma = __fsqrt_rn(agx * agx + agy * agy);  // the argument is an integer below 2^24
    const float mb = __fsqrt_rn(bgx * bgx + bgy * bgy);
    const float c = (ma + mb) * 0.5f;
    edge[idx] = c > threshold ? 1 : 0;
}

// ---- D: the dilation ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CB_THREADS) void cb_dilate_kernel(const unsigned char* __restrict__ edge, int H, int W, int radius, size_t total,
                                                               unsigned char* __restrict__ mask) {
    const size_t idx = (size_t)blockIdx.x * CB_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t hw = (size_t)H * W;
    const size_t n = idx / hw;
    const int rem = (int)(idx - n * hw), y = rem / W, x = rem - y * W;
    const unsigned char* e = edge + n * hw;
    const int y0 = max(y - radius, 0), y1 = min(y + radius, H - 1), x0 = max(x - radius, 0), x1 = min(x + radius, W - 1);
    unsigned v = 0;
    for (int yy = y0; yy <= y1 && !v; ++yy)
        for (int xx = x0; xx <= x1; ++xx) v |= e[(size_t)yy * W + xx];
    mask[idx] = v ? 1 : 0;
}

// ---- R, C: the correction -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CB_THREADS) void cb_rowsum_kernel(const unsigned char* __restrict__ in, int H, int W, int radius, size_t total,
                                                               unsigned* __restrict__ rows) {
    const size_t idx = (size_t)blockIdx.x * CB_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t hw = (size_t)H * W;
    const size_t n = idx / hw;
    const int rem = (int)(idx - n * hw), y = rem / W, x = rem - y * W;
    const int x0 = max(x - radius, 0), x1 = min(x + radius, W - 1);
    const unsigned char* p = in + (n * hw + (size_t)y * W + x0) * 3;
    unsigned s0 = 0, s1 = 0, s2 = 0;
    for (int xx = x0; xx <= x1; ++xx, p += 3) {
        s0 += p[0];
        s1 += p[1];
        s2 += p[2];
    }
    rows[idx * 3] = s0;
    rows[idx * 3 + 1] = s1;
    rows[idx * 3 + 2] = s2;
}

__global__ __launch_bounds__(CB_THREADS) void cb_correct_kernel(const unsigned char* __restrict__ in, const unsigned char* __restrict__ mask,
                                                                const unsigned* __restrict__ rows, int H, int W, int radius, size_t total,
                                                                unsigned char* __restrict__ out) {
#pragma clang fp contract(off)  // numpy rounds each product and the sum
    const size_t idx = (size_t)blockIdx.x * CB_THREADS + threadIdx.x;
    if (idx >= total) return;
    const unsigned char* p = in + idx * 3;
    unsigned char* o = out + idx * 3;
    if (!mask[idx]) {
        o[0] = p[0];
        o[1] = p[1];
        o[2] = p[2];
        return;
    }
    const size_t hw = (size_t)H * W;
    const size_t n = idx / hw;
    const int rem = (int)(idx - n * hw), y = rem / W, x = rem - y * W;
    const int y0 = max(y - radius, 0), y1 = min(y + radius, H - 1), x0 = max(x - radius, 0), x1 = min(x + radius, W - 1);
    const unsigned* r = rows + (n * hw + (size_t)y0 * W + x) * 3;
    unsigned s[3] = {0, 0, 0};
    for (int yy = y0; yy <= y1; ++yy, r += (size_t)W * 3) {
        s[0] += r[0];
        s[1] += r[1];
        s[2] += r[2];
    }
    const double count = (double)((y1 - y0 + 1) * (x1 - x0 + 1));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double mean = (double)s[c] / count;  // one IEEE division
        const double a = 0.5 * (double)p[c];
        const double b = 0.5 * mean;
        o[c] = (unsigned char)(a + b);  // within [0, 255]: truncated
    }
}

// ---- W: the wide bilateral filter -----------------------------------------------------------------------------------------------
__device__ __forceinline__ int bw_index(int e) { return (e & 3) * BW_PITCH + (e >> 2); }

__global__ __launch_bounds__(CB_THREADS) void cb_bilateral_wide_kernel(const unsigned char* __restrict__ in, const float* __restrict__ table,
                                                                       int radius, int H, int W, int tiles_x, int tiles,
                                                                       unsigned char* __restrict__ out) {
#pragma clang fp contract(off)  // the definition rounds the weight product; the only fused operations are the explicit __fmaf_rn
    __shared__ unsigned rowbuf[2][4 * BW_PITCH];
    __shared__ float color[BW_COLOR];
    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & (WAVE - 1);
    const auto [n, y0, x0] = tile_of<BW_TH, BW_TW>(tiles, tiles_x);
    const unsigned char* img = in + (size_t)n * H * W * 3;
    const int R = radius, rowlen = BW_TW + 2 * R;
    for (int e = tid; e < BW_COLOR; e += CB_THREADS) color[e] = table[e];
    const float* __restrict__ space = table + BW_COLOR;
    // the two columns of the LDS row this thread stages at every step: byte offsets of their mirrored source columns
    int soff[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) soff[k] = reflect101(x0 - R + min(tid + k * CB_THREADS, rowlen - 1), W) * 3;
    const int d0 = bw_index(tid), d1 = bw_index(tid + CB_THREADS);
    const bool two = tid + CB_THREADS < rowlen;  // tid < rowlen always: rowlen >= 258
    const int py = y0 + wv, pxx = x0 + lane * BW_PX;
    const bool active = py < H && pxx < W;
    float wsum[BW_PX], s0[BW_PX], s1[BW_PX], s2[BW_PX];
    unsigned ctr[BW_PX];
#pragma unroll
    for (int p = 0; p < BW_PX; ++p) {
        wsum[p] = s0[p] = s1[p] = s2[p] = 0.f;
        ctr[p] = active ? load_px(img + ((size_t)py * W + min(pxx + p, W - 1)) * 3) : 0u;
    }
    const int steps = 2 * R + min(BW_TH, H - y0);  // the last row of the band that exists needs input rows up to its own + R
    {
        const unsigned char* src = img + (size_t)reflect101(y0 - R, H) * W * 3;
        rowbuf[0][d0] = load_px(src + soff[0]);
        if (two) rowbuf[0][d1] = load_px(src + soff[1]);
    }
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        const bool more = s + 1 < steps;
        unsigned nxt0 = 0, nxt1 = 0;
        if (more) {  // the next input row: in flight while this one is used
            const unsigned char* src = img + (size_t)reflect101(y0 - R + s + 1, H) * W * 3;
            nxt0 = load_px(src + soff[0]);
            nxt1 = load_px(src + soff[1]);
        }
        const int i = s - R - wv;  // the tap row of this wave: the same for all its lanes
        if (active && i >= -R && i <= R) {
            const unsigned* row = rowbuf[s & 1] + lane;
            const int i2 = i * i, rem = R * R - i2;
            int jmax = (int)__fsqrt_rn((float)rem);  // the largest j with i * i + j * j <= R * R
            while (jmax * jmax > rem) --jmax;
            while ((jmax + 1) * (jmax + 1) <= rem) ++jmax;
            unsigned q0 = row[bw_index(R - jmax)], q1 = row[bw_index(R - jmax + 1)], q2 = row[bw_index(R - jmax + 2)];
#pragma unroll 4
            for (int j = -jmax; j <= jmax; ++j) {
                const unsigned q3 = row[bw_index(R + j + 3)];  // column 4 * lane + R + j + 3 <= rowlen - 1
                const float sp = space[i2 + j * j];
                const unsigned q[BW_PX] = {q0, q1, q2, q3};
#pragma unroll
                for (int p = 0; p < BW_PX; ++p) bilateral_tap(q[p], ctr[p], sp, color, wsum[p], s0[p], s1[p], s2[p]);
                q0 = q1;
                q1 = q2;
                q2 = q3;
            }
        }
        if (more) {
            unsigned* dst = rowbuf[(s + 1) & 1];  // last read at step s - 1, before the barrier that ended it
            dst[d0] = nxt0;
            if (two) dst[d1] = nxt1;
        }
        __syncthreads();
    }
    if (!active) return;
    unsigned o[BW_PX];
#pragma unroll
    for (int p = 0; p < BW_PX; ++p) {
        unsigned b0, b1, b2;
        bilateral_bytes(wsum[p], s0[p], s1[p], s2[p], b0, b1, b2);
        o[p] = b0 | b1 << 8 | b2 << 16;
    }
    store_px4(out + (size_t)n * H * W * 3 + ((size_t)py * W + pxx) * 3, o, W - pxx);
}

// ---- H, B: the detail blend -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CB_THREADS) void cb_blur_row_kernel(const unsigned char* __restrict__ orig, const double* __restrict__ taps,
                                                                 int ksize, int H, int W, size_t total, double* __restrict__ rows) {
#pragma clang fp contract(off)  // OpenCV's generic filters round every product and every sum
    const size_t idx = (size_t)blockIdx.x * CB_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t hw = (size_t)H * W;
    const size_t n = idx / hw;
    const int rem = (int)(idx - n * hw), y = rem / W, x = rem - y * W;
    const unsigned char* line = orig + (n * hw + (size_t)y * W) * 3;
    const int r = ksize / 2;
    double t[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < ksize; ++j) {  // left to right
        int sx = x + j - r;
        if ((unsigned)sx >= (unsigned)W) sx = reflect101(sx, W);
        const unsigned char* p = line + (size_t)sx * 3;
        const double kj = taps[j];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = kj * (double)p[c];
            t[c] = j == 0 ? v : t[c] + v;
        }
    }
    rows[idx * 3] = t[0];
    rows[idx * 3 + 1] = t[1];
    rows[idx * 3 + 2] = t[2];
}

__global__ __launch_bounds__(CB_THREADS) void cb_detail_blend_kernel(const unsigned char* __restrict__ img,
                                                                     const unsigned char* __restrict__ orig,
                                                                     const double* __restrict__ rows, const double* __restrict__ taps,
                                                                     int ksize, double w_img, double alpha, double beta, int H, int W,
                                                                     size_t total, unsigned char* __restrict__ out) {
#pragma clang fp contract(off)
    const size_t idx = (size_t)blockIdx.x * CB_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t hw = (size_t)H * W;
    const size_t n = idx / hw;
    const int rem = (int)(idx - n * hw), y = rem / W, x = rem - y * W;
    const double* plane = rows + n * hw * 3;
    const int r = ksize / 2;
    const double* c0 = plane + ((size_t)y * W + x) * 3;
    const double kc = taps[r];
    double t[3] = {kc * c0[0], kc * c0[1], kc * c0[2]};
    for (int j = 1; j <= r; ++j) {  // the nearest pair first
        int ya = y + j, yb = y - j;
        if (ya >= H) ya = reflect101(ya, H);
        if (yb < 0) yb = reflect101(yb, H);
        const double* pa = plane + ((size_t)ya * W + x) * 3;
        const double* pb = plane + ((size_t)yb * W + x) * 3;
        const double kj = taps[r + j];
#pragma unroll
        for (int c = 0; c < 3; ++c) t[c] = t[c] + kj * (pa[c] + pb[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double o = (double)orig[idx * 3 + c];
        const double detail = o - t[c];
        const double u = (double)img[idx * 3 + c] * w_img;
        const double v = o * alpha;
        const double w = detail * beta;
        double xv = (u + v) + w;
        xv = xv < 0.0 ? 0.0 : (xv > 255.0 ? 255.0 : xv);
        if (!(xv == xv)) xv = 0.0;  // a NaN weight: keep the byte defined, as blend_u8_kernel does
        out[idx * 3 + c] = (unsigned char)xv;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// 0 = fine, else the error code (message set)
static int cb_shape(const char* who, int N, int H, int W) {
    const int rc = check_extent(who, N, H, W);
    if (rc != MSTG_OK) return rc;
    const long long px = (long long)N * H * W;  // the finest grid: a thread per pixel
    return check_grid(who, (px + CB_THREADS - 1) / CB_THREADS, 31, "N * H * W", px);
}

static int cb_kernel_size(const char* who, int k) {
    if (k >= 1 && (k & 1) && k <= MSTG_COLOR_BLOCK_MAX_KERNEL) return MSTG_OK;
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: kernel_size = %d is not built: this build takes the odd sizes 1 to %d (an even box has no centre)", who,
             k, MSTG_COLOR_BLOCK_MAX_KERNEL);
    return fail_arg(MSTG_E_UNSUPPORTED, msg);
}

static int cb_correct_args(const char* who, int H, int W, int radius) {
    char msg[200];
    if (radius < 0) {
        snprintf(msg, sizeof(msg), "%s: radius = %d", who, radius);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    if ((unsigned long long)H * W * 255ull >= (1ull << 32)) {
        snprintf(msg, sizeof(msg), "%s: H * W * 255 = %llu does not fit the 32-bit window sums", who, (unsigned long long)H * W * 255ull);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    return MSTG_OK;
}

static int cb_wide_radius(const char* who, int radius) {
    if (radius >= 1 && radius <= BW_RMAX) return MSTG_OK;
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: radius = %d is not built: this build takes the radii 1 to %d", who, radius, BW_RMAX);
    return fail_arg(radius < 1 ? MSTG_E_BADARG : MSTG_E_UNSUPPORTED, msg);
}

static int cb_ksize(const char* who, int ksize) {
    if (ksize >= 1 && (ksize & 1) && ksize <= MSTG_DETAIL_BLEND_MAX_KSIZE) return MSTG_OK;
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: ksize = %d is not built: this build takes the odd sizes 1 to %d", who, ksize, MSTG_DETAIL_BLEND_MAX_KSIZE);
    return fail_arg(MSTG_E_UNSUPPORTED, msg);
}

static dim3 cb_grid(size_t px) { return dim3((unsigned)cdivz(px, (size_t)CB_THREADS)); }

static int cb_mask(const unsigned char* in, int N, int H, int W, const unsigned short* lab, float threshold, int k, unsigned char* edge,
                   unsigned char* mask, hipStream_t st) {
    const size_t px = (size_t)N * H * W;
    MSTG_LAUNCH(cb_edge_kernel, cb_grid(px), dim3(CB_THREADS), 0, st, in, lab, threshold, H, W, px, edge);
    MSTG_CHECK_LAUNCH("cb_edge_kernel");
    MSTG_LAUNCH(cb_dilate_kernel, cb_grid(px), dim3(CB_THREADS), 0, st, edge, H, W, k / 2, px, mask);
    MSTG_CHECK_LAUNCH("cb_dilate_kernel");
    return MSTG_OK;
}

static int cb_correct(const unsigned char* in, const unsigned char* mask, int N, int H, int W, int radius, unsigned* rows, unsigned char* out,
                      hipStream_t st) {
    const size_t px = (size_t)N * H * W;
    MSTG_LAUNCH(cb_rowsum_kernel, cb_grid(px), dim3(CB_THREADS), 0, st, in, H, W, radius, px, rows);
    MSTG_CHECK_LAUNCH("cb_rowsum_kernel");
    MSTG_LAUNCH(cb_correct_kernel, cb_grid(px), dim3(CB_THREADS), 0, st, in, mask, rows, H, W, radius, px, out);
    MSTG_CHECK_LAUNCH("cb_correct_kernel");
    return MSTG_OK;
}

static int cb_wide(const unsigned char* in, int N, int H, int W, int radius, const float* table, unsigned char* out, hipStream_t st) {
    const int tx = cdiv(W, BW_TW), tiles = tx * cdiv(H, BW_TH);
    MSTG_LAUNCH(cb_bilateral_wide_kernel, dim3((unsigned)(N * tiles)), dim3(CB_THREADS), 0, st, in, table, radius, H, W, tx, tiles, out);
    MSTG_CHECK_LAUNCH("cb_bilateral_wide_kernel");
    return MSTG_OK;
}

static int cb_wide_grid(const char* who, int N, int H, int W) {
    const long long blocks = (long long)N * cdiv(H, BW_TH) * cdiv(W, BW_TW);
    if (blocks < (1ll << 31)) return MSTG_OK;
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: N * bands = %lld, more than 2^31 - 1 workgroups in one launch", who, blocks);
    return fail_arg(MSTG_E_UNSUPPORTED, msg);
}

static int cb_blend(const unsigned char* img, const unsigned char* orig, int N, int H, int W, const double* taps, int ksize, double w_img,
                    double alpha, double beta, double* rows, unsigned char* out, hipStream_t st) {
    const size_t px = (size_t)N * H * W;
    MSTG_LAUNCH(cb_blur_row_kernel, cb_grid(px), dim3(CB_THREADS), 0, st, orig, taps, ksize, H, W, px, rows);
    MSTG_CHECK_LAUNCH("cb_blur_row_kernel");
    MSTG_LAUNCH(cb_detail_blend_kernel, cb_grid(px), dim3(CB_THREADS), 0, st, img, orig, rows, taps, ksize, w_img, alpha, beta, H, W, px, out);
    MSTG_CHECK_LAUNCH("cb_detail_blend_kernel");
    return MSTG_OK;
}

// the layout of mstg_color_block_fix's workspace
struct CbWorkspace {
    size_t edge, mask, sums, corrected, smoothed, total;
};
static CbWorkspace cb_workspace(int N, int H, int W, bool with_orig) {
    const size_t px = (size_t)N * H * W;
    CbWorkspace w;
    w.edge = 0;
    w.mask = align16(px);
    w.sums = w.mask + align16(px);  // the window's row sums (12 bytes a pixel), then the blur's row pass (24 bytes a pixel)
    w.corrected = w.sums + align16(px * 3 * (with_orig ? sizeof(double) : sizeof(unsigned)));
    w.smoothed = w.corrected + align16(px * 3);
    w.total = w.smoothed + (with_orig ? align16(px * 3) : 0);
    return w;
}

}  // namespace mstg

using namespace mstg;

extern "C" int mstg_lab_tables(unsigned short* table) {
    if (!table) return fail_arg(MSTG_E_BADARG, "lab_tables: null table pointer");
    for (int v = 0; v < CB_GAMMA; ++v) {
        const double x = v / 255.0;
        const double lin = x <= 0.04045 ? x / 12.92 : std::pow((x + 0.055) / 1.055, 2.4);
        table[v] = (unsigned short)std::lrint(2040.0 * lin);
    }
    for (int i = 0; i < CB_CBRT; ++i) {
        const double x = i / 2040.0;
        const double f = x < 0.008856 ? 7.787 * x + 16.0 / 116.0 : std::cbrt(x);
        table[CB_GAMMA + i] = (unsigned short)std::lrint(32768.0 * f);
    }
    const double m[3][3] = {{0.412453, 0.357580, 0.180423}, {0.212671, 0.715160, 0.072169}, {0.019334, 0.119193, 0.950227}};
    const double white[3] = {0.950456, 1.0, 1.088754};
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) table[CB_COEF + 3 * r + k] = (unsigned short)std::lrint(4096.0 * m[r][k] / white[r]);
    for (int e = CB_COEF + 9; e < MSTG_LAB_TABLE_U16; ++e) table[e] = 0;
    return MSTG_OK;
}

extern "C" int mstg_bilateral_wide_tables(int d, double sigma_color, double sigma_space, float* table) {
    if (!table) return fail_arg(MSTG_E_BADARG, "bilateral_wide_tables: null table pointer");
    if (!(sigma_color > 0)) sigma_color = 1;
    if (!(sigma_space > 0)) sigma_space = 1;
    int radius;
    if (d <= 0) {
        const double r = std::nearbyint(sigma_space * 1.5);  // cvRound: round half to even (the default rounding mode)
        radius = r > 1e6 ? 1000000 : (int)r;
    } else {
        radius = d / 2;
    }
    if (radius < 1) radius = 1;
    if (radius > BW_RMAX) {
        char msg[220];
        snprintf(msg, sizeof(msg), "bilateral_wide_tables: radius = %d (d = %d, sigma_space = %g) is not built: this build takes the radii 1 to %d",
                 radius, d, sigma_space, BW_RMAX);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    const double gauss_color = -0.5 / (sigma_color * sigma_color), gauss_space = -0.5 / (sigma_space * sigma_space);
    for (int t = 0; t < BW_COLOR; ++t) table[t] = (float)std::exp((double)(t * t) * gauss_color);
    for (int q = 0; q <= BW_RMAX * BW_RMAX; ++q) table[BW_COLOR + q] = q <= radius * radius ? (float)std::exp((double)q * gauss_space) : 0.f;
    return radius;
}

extern "C" int mstg_color_block_mask(const unsigned char* in, int N, int H, int W, const unsigned short* lab_table, float threshold,
                                     int kernel_size, unsigned char* mask, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = cb_kernel_size("color_block_mask", kernel_size);
    if (rc != MSTG_OK) return rc;
    if (!in || !lab_table || !mask) return fail_arg(MSTG_E_BADARG, "color_block_mask: null in, table or mask pointer");
    rc = cb_shape("color_block_mask", N, H, W);
    if (rc != MSTG_OK) return rc;
    const size_t px = (size_t)N * H * W;
    if (!workspace || workspace_bytes < px) return fail_arg(MSTG_E_WORKSPACE, "color_block_mask: workspace too small (N * H * W bytes)");
    if ((uintptr_t)lab_table & 1) return fail_arg(MSTG_E_ALIGN, "color_block_mask: table not 2-byte aligned");
    if (overlaps(mask, px, in, px * 3) || overlaps(mask, px, workspace, px) || overlaps(mask, px, lab_table, 2 * MSTG_LAB_TABLE_U16) ||
        overlaps(workspace, px, in, px * 3) || overlaps(workspace, px, lab_table, 2 * MSTG_LAB_TABLE_U16))
        return fail_arg(MSTG_E_BADARG, "color_block_mask: mask or workspace overlaps an input, the table or each other");
    return cb_mask(in, N, H, W, lab_table, threshold, kernel_size, (unsigned char*)workspace, mask, (hipStream_t)stream);
}

extern "C" int mstg_color_correct_u8(const unsigned char* in, const unsigned char* mask, int N, int H, int W, int radius, unsigned char* out,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    if (!in || !mask || !out) return fail_arg(MSTG_E_BADARG, "color_correct_u8: null in, mask or out pointer");
    int rc = cb_shape("color_correct_u8", N, H, W);
    if (rc == MSTG_OK) rc = cb_correct_args("color_correct_u8", H, W, radius);
    if (rc != MSTG_OK) return rc;
    const size_t px = (size_t)N * H * W, nb = px * 3, need = nb * sizeof(unsigned);
    if (!workspace || workspace_bytes < need) return fail_arg(MSTG_E_WORKSPACE, "color_correct_u8: workspace too small (N * H * W * 12 bytes)");
    if ((uintptr_t)workspace & 3) return fail_arg(MSTG_E_ALIGN, "color_correct_u8: workspace not 4-byte aligned");
    if (overlaps(out, nb, in, nb) || overlaps(out, nb, mask, px) || overlaps(out, nb, workspace, need) ||
        overlaps(workspace, need, in, nb) || overlaps(workspace, need, mask, px))
        return fail_arg(MSTG_E_BADARG, "color_correct_u8: out or workspace overlaps an input or each other");
    return cb_correct(in, mask, N, H, W, radius, (unsigned*)workspace, out, (hipStream_t)stream);
}

extern "C" int mstg_bilateral_wide_u8(const unsigned char* in, int N, int H, int W, int radius, const float* table, unsigned char* out,
                                      void* stream) {
    int rc = cb_wide_radius("bilateral_wide_u8", radius);  // first: the refusal does not depend on the buffers
    if (rc != MSTG_OK) return rc;
    if (!in || !out || !table) return fail_arg(MSTG_E_BADARG, "bilateral_wide_u8: null in, table or out pointer");
    rc = cb_shape("bilateral_wide_u8", N, H, W);
    if (rc == MSTG_OK) rc = cb_wide_grid("bilateral_wide_u8", N, H, W);
    if (rc != MSTG_OK) return rc;
    if ((uintptr_t)table & 3) return fail_arg(MSTG_E_ALIGN, "bilateral_wide_u8: table not 4-byte aligned");
    const size_t nb = (size_t)N * H * W * 3;
    if (overlaps(out, nb, in, nb) || overlaps(out, nb, table, sizeof(float) * MSTG_BILATERAL_WIDE_TABLE_FLOATS))
        return fail_arg(MSTG_E_BADARG, "bilateral_wide_u8: out overlaps the input or the table (the filter reads neighbours of every pixel)");
    return cb_wide(in, N, H, W, radius, table, out, (hipStream_t)stream);
}

extern "C" int mstg_detail_blend_u8(const unsigned char* img, const unsigned char* orig, int N, int H, int W, const double* kernel_f64,
                                    int ksize, double w_img, double alpha, double beta, unsigned char* out, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    int rc = cb_ksize("detail_blend_u8", ksize);
    if (rc != MSTG_OK) return rc;
    if (!img || !orig || !kernel_f64 || !out) return fail_arg(MSTG_E_BADARG, "detail_blend_u8: null img, orig, kernel or out pointer");
    rc = cb_shape("detail_blend_u8", N, H, W);
    if (rc != MSTG_OK) return rc;
    const size_t nb = (size_t)N * H * W * 3, need = nb * sizeof(double);
    if (!workspace || workspace_bytes < need) return fail_arg(MSTG_E_WORKSPACE, "detail_blend_u8: workspace too small (N * H * W * 24 bytes)");
    if (((uintptr_t)workspace & 7) || ((uintptr_t)kernel_f64 & 7))
        return fail_arg(MSTG_E_ALIGN, "detail_blend_u8: workspace or kernel not 8-byte aligned");
    if (overlaps(out, nb, img, nb) || overlaps(out, nb, orig, nb) || overlaps(out, nb, workspace, need) ||
        overlaps(out, nb, kernel_f64, sizeof(double) * ksize) || overlaps(workspace, need, img, nb) || overlaps(workspace, need, orig, nb) ||
        overlaps(workspace, need, kernel_f64, sizeof(double) * ksize))
        return fail_arg(MSTG_E_BADARG, "detail_blend_u8: out or workspace overlaps an input, the kernel or each other");
    return cb_blend(img, orig, N, H, W, kernel_f64, ksize, w_img, alpha, beta, (double*)workspace, out, (hipStream_t)stream);
}

extern "C" size_t mstg_color_block_fix_workspace_bytes(int N, int H, int W, int with_orig) {
    if (cb_shape("color_block_fix_workspace_bytes", N, H, W) != MSTG_OK) return 0;
    return cb_workspace(N, H, W, with_orig != 0).total;
}

extern "C" int mstg_color_block_fix(const unsigned char* in, const unsigned char* orig, int N, int H, int W, const unsigned short* lab_table,
                                    float threshold, int kernel_size, int correct_radius, int bilateral_radius, const float* bilateral_table,
                                    const double* kernel_f64, int ksize, double w_img, double alpha, double beta, unsigned char* out,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    int rc = cb_kernel_size("color_block_fix", kernel_size);
    if (rc == MSTG_OK) rc = cb_wide_radius("color_block_fix", bilateral_radius);
    if (rc == MSTG_OK && orig) rc = cb_ksize("color_block_fix", ksize);
    if (rc != MSTG_OK) return rc;
    if (!in || !out || !lab_table || !bilateral_table || (orig && !kernel_f64))
        return fail_arg(MSTG_E_BADARG, "color_block_fix: null in, out, table or (with orig) kernel pointer");
    rc = cb_shape("color_block_fix", N, H, W);
    if (rc == MSTG_OK) rc = cb_wide_grid("color_block_fix", N, H, W);
    if (rc == MSTG_OK) rc = cb_correct_args("color_block_fix", H, W, correct_radius);
    if (rc != MSTG_OK) return rc;
    const CbWorkspace ws = cb_workspace(N, H, W, orig != nullptr);
    if (!workspace || workspace_bytes < ws.total) return fail_arg(MSTG_E_WORKSPACE, "color_block_fix: workspace too small");
    if (((uintptr_t)workspace & 15) || ((uintptr_t)bilateral_table & 3) || ((uintptr_t)kernel_f64 & 7) || ((uintptr_t)lab_table & 1))
        return fail_arg(MSTG_E_ALIGN, "color_block_fix: workspace not 16-byte, bilateral table not 4-byte, kernel not 8-byte or Lab table not 2-byte aligned");
    const size_t nb = (size_t)N * H * W * 3;
    if (overlaps(out, nb, in, nb) || (orig && overlaps(out, nb, orig, nb)) || overlaps(out, nb, workspace, ws.total) ||
        overlaps(out, nb, lab_table, 2 * MSTG_LAB_TABLE_U16) ||
        overlaps(out, nb, bilateral_table, sizeof(float) * MSTG_BILATERAL_WIDE_TABLE_FLOATS) ||
        (orig && overlaps(out, nb, kernel_f64, sizeof(double) * ksize)) || overlaps(workspace, ws.total, in, nb) ||
        (orig && overlaps(workspace, ws.total, orig, nb)))
        return fail_arg(MSTG_E_BADARG, "color_block_fix: out or the workspace overlaps an input or a table");
    unsigned char* base = (unsigned char*)workspace;
    unsigned char* mask = base + ws.mask;
    unsigned char* corrected = base + ws.corrected;
    hipStream_t st = (hipStream_t)stream;
    rc = cb_mask(in, N, H, W, lab_table, threshold, kernel_size, base + ws.edge, mask, st);
    if (rc == MSTG_OK) rc = cb_correct(in, mask, N, H, W, correct_radius, (unsigned*)(base + ws.sums), corrected, st);
    if (rc != MSTG_OK) return rc;
    if (!orig) return cb_wide(corrected, N, H, W, bilateral_radius, bilateral_table, out, st);
    unsigned char* smoothed = base + ws.smoothed;
    rc = cb_wide(corrected, N, H, W, bilateral_radius, bilateral_table, smoothed, st);
    if (rc == MSTG_OK) rc = cb_blend(smoothed, orig, N, H, W, kernel_f64, ksize, w_img, alpha, beta, (double*)(base + ws.sums), out, st);
    return rc;
}
