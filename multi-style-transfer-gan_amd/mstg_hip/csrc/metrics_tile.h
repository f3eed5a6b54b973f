// The tile arithmetic of the image-quality metrics, shared by csrc/metrics.hip (batches of one shape) and csrc/compare.hip (ragged
// pairs, the second image resized while it is staged): patch staging, the window sums and S of one tile, the tile's fixed-order
// reduction, and the finish of one image pair.  Both files run exactly these operations in exactly this order, which is what makes
// a row of mstg_pair_metrics_u8 bit-identical to mstg_image_metrics_u8 on the resized image.  See csrc/metrics.hip for the
// formulation (exact integer window sums, one fp64 division per window, no atomics).
#pragma once
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

// What a tile of an H x W image covers: tile (ty, tx) of tiles_x x tiles_y starts at window = pixel (ty MT_H, tx MT_W).
struct MetricsTile {
    int y0, x0;
    int rows, len;          // patch rows / bytes per row inside the image
    int own_rows, own_len;  // the pixels whose squared differences this tile owns: its MT_H x MT_W block, the last tile of a row /
                            // column up to the edge
    int win_rows, win_cols; // windows of the image from the tile's origin (> 0)
};
__device__ __forceinline__ MetricsTile metrics_tile(int H, int W, int ty, int tx, int tiles_x, int tiles_y) {
    MetricsTile g;
    g.y0 = ty * MT_H;
    g.x0 = tx * MT_W;
    g.rows = min(MT_ROWS, H - g.y0);
    g.len = 3 * min(MT_W + 6, W - g.x0);
    g.own_rows = ty == tiles_y - 1 ? g.rows : MT_H;
    g.own_len = tx == tiles_x - 1 ? g.len : 3 * MT_W;
    g.win_rows = H - 6 - g.y0;
    g.win_cols = W - 6 - g.x0;
    return g;
}

// The tile's work once both patches are staged (pa, pb: [MT_ROWS][MT_ROW_DW] dwords, patch byte j of row r at byte
// ((sh0 + r * step) & 3) + j of LDS row r) and the workgroup has synchronised: o[0..2] = the tile's three channel sums of S (fp64),
// o[3] = its sum of squared differences (int64).  Called by all MT_THREADS threads.
__device__ __forceinline__ void ssim_tile_sums(const unsigned* pa, const unsigned* pb, int sh_a0, int sh_a_step, int sh_b0, int sh_b_step,
                                               const MetricsTile& g, double* __restrict__ o) {
    __shared__ int h_p[MT_ROWS * MT_COLS], h_q[MT_ROWS * MT_COLS], h_xy[MT_ROWS * MT_COLS];
    __shared__ double red_s[4][3];
    __shared__ long long red_d[4];
    const int tid = threadIdx.x;
    const unsigned char* ba = reinterpret_cast<const unsigned char*>(pa);
    const unsigned char* bb = reinterpret_cast<const unsigned char*>(pb);

    // squared differences of the pixels this tile owns
    int ssd = 0;
    for (int e = tid; e < g.own_rows * MT_PBYTES; e += MT_THREADS) {
        const int r = e / MT_PBYTES, j = e - r * MT_PBYTES;
        if (j < g.own_len) {
            const int d = (int)ba[r * (4 * MT_ROW_DW) + ((sh_a0 + r * sh_a_step) & 3) + j] -
                          (int)bb[r * (4 * MT_ROW_DW) + ((sh_b0 + r * sh_b_step) & 3) + j];
            ssd += d * d;
        }
    }

    // horizontal 7-sums: column (x, c) of patch row r sums the bytes j = 3 x + c + 3 k, k = 0..6
    for (int e = tid; e < MT_ROWS * MT_COLS; e += MT_THREADS) {
        const int r = e / MT_COLS, col = e - r * MT_COLS;
        const unsigned char* ra = ba + r * (4 * MT_ROW_DW) + ((sh_a0 + r * sh_a_step) & 3) + col;
        const unsigned char* rb = bb + r * (4 * MT_ROW_DW) + ((sh_b0 + r * sh_b_step) & 3) + col;
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
    double part[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int it = tid + MT_THREADS * k;
        const int seg = it / MT_COLS, col = it - seg * MT_COLS;
        const int r0 = seg * MT_SEG;
        const bool col_ok = col / 3 < g.win_cols;
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
            if (col_ok && r0 + i < g.win_rows) acc += s;
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
        if (tid < 3)
            o[tid] = ((red_s[0][tid] + red_s[1][tid]) + red_s[2][tid]) + red_s[3][tid];
        else
            *reinterpret_cast<long long*>(o + 3) = ((red_d[0] + red_d[1]) + red_d[2]) + red_d[3];
    }
}

// One workgroup adds the `tiles` four-word records at w of one H x W pair: thread t adds tiles t, t + 256, ... in that order, then
// a fixed tree over the 256 threads; thread 0 writes o[0..5] = {mse, psnr, ssim, ssim_c0, ssim_c1, ssim_c2}.
__device__ __forceinline__ void metrics_finish_pair(const double* __restrict__ w, int H, int W, int tiles, double* __restrict__ o) {
    __shared__ double red_s[4][3];
    __shared__ long long red_d[4];
    const int tid = threadIdx.x;
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
        o[0] = mse;
        o[1] = ssd == 0 ? (double)INFINITY : 10.0 * log10(1.0 / mse);
        o[2] = ((c[0] + c[1]) + c[2]) / 3.0;
        o[3] = c[0];
        o[4] = c[1];
        o[5] = c[2];
    }
}

}  // namespace mstg
