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
#include "metrics_tile.h"  // the tile arithmetic and the finish, shared with csrc/compare.hip

namespace mstg {

__global__ __launch_bounds__(MT_THREADS) void ssim_tile_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b,
                                                               int H, int W, int tiles_x, int tiles, double* __restrict__ ws) {
    __shared__ unsigned pa[MT_ROWS * MT_ROW_DW], pb[MT_ROWS * MT_ROW_DW];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const MetricsTile g = metrics_tile(H, W, ty, tx, tiles_x, tiles / tiles_x);
    const size_t pitch = (size_t)W * 3;
    const size_t off = ((size_t)n * H + g.y0) * pitch + (size_t)g.x0 * 3;
    stage_patch(a + off, pitch, g.rows, g.len, pa, tid);
    stage_patch(b + off, pitch, g.rows, g.len, pb, tid);
    __syncthreads();
    const int sh_step = (int)(pitch & 3);
    ssim_tile_sums(pa, pb, (int)((uintptr_t)(a + off) & 3), sh_step, (int)((uintptr_t)(b + off) & 3), sh_step, g, ws + (size_t)blockIdx.x * 4);
}

// one workgroup per image
__global__ __launch_bounds__(MT_THREADS) void metrics_finish_kernel(const double* __restrict__ ws, int H, int W, int tiles,
                                                                    double* __restrict__ out) {
    const int n = blockIdx.x;
    metrics_finish_pair(ws + (size_t)n * tiles * 4, H, W, tiles, out + (size_t)n * 6);
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
