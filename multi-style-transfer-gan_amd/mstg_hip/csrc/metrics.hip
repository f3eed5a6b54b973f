// Image-quality metrics of the reference's evaluation scripts on the device: MSE, PSNR and SSIM of two batches of 8-bit RGB
// images (N, H, W, 3) (compare_image_quality.py:14-33, image_quality_comparison.py:11-34, complete_comparison.py:13-32,
// improved_image_compare.py:8-27: astype(float) / 255, np.mean((a - b) ** 2), peak_signal_noise_ratio(data_range=1) and
// structural_similarity(channel_axis=2, data_range=1) = uniform 7x7 window, sample covariance, K1 = 0.01, K2 = 0.03, mean over
// the windows that lie inside the image, per channel).
//
// The inputs are bytes, so every window statistic is an exact integer: with Sx = sum x, Sy = sum y, Sq = sum (x^2 + y^2),
// Sxy = sum x y over the 49 pixels of a window (x, y in 0..255)
//   2 ux uy   = 2 Sx Sy / D1                      ux^2 + uy^2 = (Sx^2 + Sy^2) / D1             D1 = (49 * 255)^2
//   2 vxy     = 2 (49 Sxy - Sx Sy) / D2           vx + vy     = (49 Sq - Sx^2 - Sy^2) / D2     D2 = 49 * 48 * 255^2
// and all four numerators fit int32 (<= 3.2e8).  Only the last step is fp64: numerator and denominator of S are scaled by D1 D2,
//   S = (2 Sx Sy + C1 D1) (2 (49 Sxy - Sx Sy) + C2 D2) / ((Sx^2 + Sy^2 + C1 D1) (49 Sq - Sx^2 - Sy^2 + C2 D2)),
// four int -> double conversions, four additions, two products and ONE division per window, with no cancellation anywhere, and
// exactly 1.0 where the two windows are equal (both brackets of the numerator are then the same doubles as the denominator's).
//
// ssim_tile_kernel: one workgroup of 256 threads per tile of MT_H x MT_W windows, all three channels (3 MT_W "columns" of the
// interleaved rows).  The two (MT_H + 6) x (MT_W + 6) x 3 byte patches are staged in LDS with aligned dword loads (bytes outside the
// image are zero); horizontal 7-sums of (Sx | Sy << 16), Sq, Sxy go to int32 LDS rows; each thread then slides vertical 7-sums down
// 4 rows of 3 columns (one column of each channel), forms S in fp64 and the tile's three channel sums are reduced in a fixed
// order (wave butterfly, then the four waves in index order).  The tile also owns a disjoint set of PIXELS for the squared
// difference sum (its MT_H x MT_W block, edge tiles take the 6-pixel rest): int32 per thread, int64 per tile.  Each tile writes
// {sum S c0, sum S c1, sum S c2 (fp64), SSD (int64)} to the workspace; metrics_finish_kernel adds an image's tiles in a fixed
// order and writes {mse, psnr, ssim, ssim_c0, ssim_c1, ssim_c2}.  No atomics: results are bit-reproducible and independent of N.
// LDS- and VALU-bound (2 bytes read per pixel-channel), not HBM-bound.
#include <math.h>

#include "common.h"

namespace mstg {

constexpr int MT_H = MSTG_METRICS_TILE_H, MT_W = MSTG_METRICS_TILE_W;  // windows per tile
constexpr int MT_ROWS = MT_H + 6;                                      // patch rows
constexpr int MT_COLS = 3 * MT_W;                                      // output columns (x, c) of the interleaved rows
constexpr int MT_PBYTES = 3 * (MT_W + 6);                              // patch bytes per row
constexpr int MT_ROW_DW = (MT_PBYTES + 3 + 3) / 4;                     // + up to 3 bytes of alignment shift, in dwords
constexpr int MT_SEG = 4;                                              // output rows a thread slides over
constexpr int MT_THREADS = 256;
static_assert(MT_COLS * (MT_H / MT_SEG) == 3 * MT_THREADS, "three (column, row segment) items per thread, one of each channel");
static_assert(MT_COLS % 3 == 0 && MT_THREADS % 3 == 1, "item k of thread t has channel (t + k) % 3");

constexpr double SSIM_D1 = 12495.0 * 12495.0;           // (49 * 255)^2
constexpr double SSIM_D2 = 49.0 * 48.0 * 65025.0;       // 49 * 48 * 255^2
constexpr double SSIM_C1D1 = 1e-4 * SSIM_D1, SSIM_C2D2 = 9e-4 * SSIM_D2;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// rows of `len` valid bytes starting at p (row r of the patch: p + r * pitch, valid while r < rows) -> lds[r][MT_ROW_DW] dwords so
// that patch byte j of row r sits at byte (shift(r) + j) of the LDS row, shift(r) = address of the row start & 3.  Whole dwords
// inside the row are loaded as dwords (their address is aligned by construction), the rest byte by byte; nothing outside
// [row start, row start + len) is read, and everything outside is stored as zero.
__device__ __forceinline__ void stage_patch(const unsigned char* __restrict__ p, size_t pitch, int rows, int len,
                                            unsigned* __restrict__ lds, int tid) {
    for (int e = tid; e < MT_ROWS * MT_ROW_DW; e += MT_THREADS) {
        const int r = e / MT_ROW_DW, k = e - r * MT_ROW_DW;
        const unsigned char* row = p + (size_t)r * pitch;
        const int lo = 4 * k - (int)((uintptr_t)row & 3);  // patch byte of this dword's first byte
        unsigned v = 0;
        if (r < rows) {
            if (lo >= 0 && lo + 4 <= len) {
                v = *reinterpret_cast<const unsigned*>(row + lo);
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (lo + b >= 0 && lo + b < len) v |= (unsigned)row[lo + b] << (8 * b);
            }
        }
        lds[e] = v;
    }
}

__global__ __launch_bounds__(MT_THREADS) void ssim_tile_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b,
                                                               int H, int W, int tiles_x, int tiles, double* __restrict__ ws) {
    __shared__ unsigned pa[MT_ROWS * MT_ROW_DW], pb[MT_ROWS * MT_ROW_DW];
    __shared__ int h_p[MT_ROWS * MT_COLS], h_q[MT_ROWS * MT_COLS], h_xy[MT_ROWS * MT_COLS];
    __shared__ double red_s[4][3];
    __shared__ long long red_d[4];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * MT_H, x0 = tx * MT_W;                  // first window = first pixel of the tile
    const int rows = min(MT_ROWS, H - y0);                     // patch rows / bytes per row inside the image
    const int len = 3 * min(MT_W + 6, W - x0);
    const size_t pitch = (size_t)W * 3;
    const size_t off = ((size_t)n * H + y0) * pitch + (size_t)x0 * 3;
    stage_patch(a + off, pitch, rows, len, pa, tid);
    stage_patch(b + off, pitch, rows, len, pb, tid);
    __syncthreads();

    const unsigned char* ba = reinterpret_cast<const unsigned char*>(pa);
    const unsigned char* bb = reinterpret_cast<const unsigned char*>(pb);
    const int sh_a0 = (int)((uintptr_t)(a + off) & 3), sh_b0 = (int)((uintptr_t)(b + off) & 3), sh_step = (int)(pitch & 3);

    // squared differences of the pixels this tile owns: its MT_H x MT_W block, the last tile of a row / column up to the edge
    const int own_rows = ty == tiles / tiles_x - 1 ? rows : MT_H;
    const int own_len = tx == tiles_x - 1 ? len : 3 * MT_W;
    int ssd = 0;
    for (int e = tid; e < own_rows * MT_PBYTES; e += MT_THREADS) {
        const int r = e / MT_PBYTES, j = e - r * MT_PBYTES;
        if (j < own_len) {
            const int d = (int)ba[r * (4 * MT_ROW_DW) + ((sh_a0 + r * sh_step) & 3) + j] -
                          (int)bb[r * (4 * MT_ROW_DW) + ((sh_b0 + r * sh_step) & 3) + j];
            ssd += d * d;
        }
    }

    // horizontal 7-sums: column (x, c) of patch row r sums the bytes j = 3 x + c + 3 k, k = 0..6
    for (int e = tid; e < MT_ROWS * MT_COLS; e += MT_THREADS) {
        const int r = e / MT_COLS, col = e - r * MT_COLS;
        const unsigned char* ra = ba + r * (4 * MT_ROW_DW) + ((sh_a0 + r * sh_step) & 3) + col;
        const unsigned char* rb = bb + r * (4 * MT_ROW_DW) + ((sh_b0 + r * sh_step) & 3) + col;
        int sx = 0, sy = 0, sq = 0, sxy = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const int x = ra[3 * k], y = rb[3 * k];
            sx += x;
            sy += y;
            sq += x * x + y * y;
            sxy += x * y;
        }
        h_p[e] = sx | (sy << 16);  // each <= 7 * 255; their 7-row sums <= 12495 < 2^16: the fields never carry
        h_q[e] = sq;
        h_xy[e] = sxy;
    }
    __syncthreads();

    // vertical 7-sums by sliding add / subtract, S in fp64; item k of this thread: column (tid + 256 k) % 192 -> channel (tid + k) % 3
    const int win_rows = H - 6 - y0, win_cols = W - 6 - x0;  // windows of the image from the tile's origin (> 0)
    double part[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int it = tid + MT_THREADS * k;
        const int seg = it / MT_COLS, col = it - seg * MT_COLS;
        const int r0 = seg * MT_SEG;
        const bool col_ok = col / 3 < win_cols;
        int p = 0, q = 0, xy = 0;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            p += h_p[(r0 + i) * MT_COLS + col];
            q += h_q[(r0 + i) * MT_COLS + col];
            xy += h_xy[(r0 + i) * MT_COLS + col];
        }
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < MT_SEG; ++i) {
            if (i > 0) {
                p += h_p[(r0 + i + 6) * MT_COLS + col] - h_p[(r0 + i - 1) * MT_COLS + col];
                q += h_q[(r0 + i + 6) * MT_COLS + col] - h_q[(r0 + i - 1) * MT_COLS + col];
                xy += h_xy[(r0 + i + 6) * MT_COLS + col] - h_xy[(r0 + i - 1) * MT_COLS + col];
            }
            const int sx = p & 0xffff, sy = (int)((unsigned)p >> 16);
            const int mxy = sx * sy, mm = sx * sx + sy * sy;  // <= 1.57e8, <= 3.13e8
            const double a1 = (double)(2 * mxy) + SSIM_C1D1, b1 = (double)mm + SSIM_C1D1;
            const double a2 = (double)(2 * (49 * xy - mxy)) + SSIM_C2D2, b2 = (double)(49 * q - mm) + SSIM_C2D2;
            const double s = (a1 * a2) / (b1 * b2);
            if (col_ok && r0 + i < win_rows) acc += s;
        }
        part[k] = acc;
    }
    // channel c's item of this thread is k = (c - tid) mod 3
    const int c0 = tid % 3;
    double s0 = c0 == 0 ? part[0] : (c0 == 2 ? part[1] : part[2]);
    double s1 = c0 == 1 ? part[0] : (c0 == 0 ? part[1] : part[2]);
    double s2 = c0 == 2 ? part[0] : (c0 == 1 ? part[1] : part[2]);
    s0 = wave_sum_f64(s0);
    s1 = wave_sum_f64(s1);
    s2 = wave_sum_f64(s2);
    const long long d = wave_sum_i64((long long)ssd);
    if ((tid & 63) == 0) {
        red_s[tid >> 6][0] = s0;
        red_s[tid >> 6][1] = s1;
        red_s[tid >> 6][2] = s2;
        red_d[tid >> 6] = d;
    }
    __syncthreads();
    if (tid < 4) {
        double* o = ws + (size_t)blockIdx.x * 4;
        if (tid < 3)
            o[tid] = ((red_s[0][tid] + red_s[1][tid]) + red_s[2][tid]) + red_s[3][tid];
        else
            *reinterpret_cast<long long*>(o + 3) = ((red_d[0] + red_d[1]) + red_d[2]) + red_d[3];
    }
}

// one workgroup per image: thread t adds tiles t, t + 256, ... in that order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(MT_THREADS) void metrics_finish_kernel(const double* __restrict__ ws, int H, int W, int tiles,
                                                                    double* __restrict__ out) {
    __shared__ double red_s[4][3];
    __shared__ long long red_d[4];
    const int tid = threadIdx.x, n = blockIdx.x;
    const double* w = ws + (size_t)n * tiles * 4;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    long long d = 0;
    for (int t = tid; t < tiles; t += MT_THREADS) {
        s0 += w[(size_t)t * 4];
        s1 += w[(size_t)t * 4 + 1];
        s2 += w[(size_t)t * 4 + 2];
        d += *reinterpret_cast<const long long*>(w + (size_t)t * 4 + 3);
    }
    s0 = wave_sum_f64(s0);
    s1 = wave_sum_f64(s1);
    s2 = wave_sum_f64(s2);
    d = wave_sum_i64(d);
    if ((tid & 63) == 0) {
        red_s[tid >> 6][0] = s0;
        red_s[tid >> 6][1] = s1;
        red_s[tid >> 6][2] = s2;
        red_d[tid >> 6] = d;
    }
    __syncthreads();
    if (tid == 0) {
        const double windows = (double)(H - 6) * (double)(W - 6);
        double c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = (((red_s[0][k] + red_s[1][k]) + red_s[2][k]) + red_s[3][k]) / windows;
        const long long ssd = ((red_d[0] + red_d[1]) + red_d[2]) + red_d[3];
        const double mse = (double)ssd / (65025.0 * (double)H * (double)W * 3.0);
        double* o = out + (size_t)n * 6;
        o[0] = mse;
        o[1] = ssd == 0 ? (double)INFINITY : 10.0 * log10(1.0 / mse);
        o[2] = ((c[0] + c[1]) + c[2]) / 3.0;
        o[3] = c[0];
        o[4] = c[1];
        o[5] = c[2];
    }
}

// 0 = fine, else the error code (message set)
static int metrics_shape(const char* who, int N, int H, int W, int* tiles_x, int* tiles_y) {
    char msg[160];
    if (N < 1) {
        snprintf(msg, sizeof(msg), "%s: N = %d, need at least one image pair", who, N);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    if (H < 7 || W < 7) {
        snprintf(msg, sizeof(msg), "%s: image %d x %d is smaller than the 7x7 SSIM window", who, H, W);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    if ((long long)H * W * 3 >= (1ll << 31)) {
        snprintf(msg, sizeof(msg), "%s: H * W * 3 = %lld does not fit 31 bits", who, (long long)H * W * 3);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    *tiles_x = cdiv(W - 6, MT_W);
    *tiles_y = cdiv(H - 6, MT_H);
    if ((long long)N * *tiles_x * *tiles_y >= (1ll << 24)) {  // workgroups of 256 threads: below 2^32 threads per launch
        snprintf(msg, sizeof(msg), "%s: N * tiles = %lld, more than 2^24 - 1 workgroups in one launch", who,
                 (long long)N * *tiles_x * *tiles_y);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    return MSTG_OK;
}

}  // namespace mstg

using namespace mstg;

extern "C" size_t mstg_image_metrics_workspace_bytes(int N, int H, int W) {
    int tx, ty;
    if (metrics_shape("image_metrics_workspace_bytes", N, H, W, &tx, &ty) != MSTG_OK) return 0;
    return (size_t)N * tx * ty * 4 * sizeof(double);
}

extern "C" int mstg_image_metrics_u8(const unsigned char* a, const unsigned char* b, int N, int H, int W, double* out, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    if (!a || !b || !out) return fail_arg(MSTG_E_BADARG, "image_metrics_u8: null image or output pointer");
    int tx, ty;
    const int rc = metrics_shape("image_metrics_u8", N, H, W, &tx, &ty);
    if (rc != MSTG_OK) return rc;
    const size_t need = (size_t)N * tx * ty * 4 * sizeof(double);
    if (!workspace || workspace_bytes < need) return fail_arg(MSTG_E_WORKSPACE, "image_metrics_u8: workspace too small");
    if (((uintptr_t)workspace & 7) || ((uintptr_t)out & 7)) return fail_arg(MSTG_E_ALIGN, "image_metrics_u8: out / workspace not 8-byte aligned");
    const int tiles = tx * ty;
    MSTG_LAUNCH(ssim_tile_kernel, dim3((unsigned)(N * tiles)), dim3(MT_THREADS), 0, (hipStream_t)stream, a, b, H, W, tx, tiles,
                (double*)workspace);
    MSTG_CHECK_LAUNCH("ssim_tile_kernel");
    MSTG_LAUNCH(metrics_finish_kernel, dim3((unsigned)N), dim3(MT_THREADS), 0, (hipStream_t)stream, (const double*)workspace, H, W, tiles,
                out);
    MSTG_CHECK_LAUNCH("metrics_finish_kernel");
    return MSTG_OK;
}
