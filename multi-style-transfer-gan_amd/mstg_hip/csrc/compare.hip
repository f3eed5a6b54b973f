// Mixed-size image comparison (include/mstg_hip.h, "Mixed-size image comparison"): what the reference's four folder-comparison
// scripts do when the processed image and the original differ in shape -- cv2.resize(img, (W, H)), the 8-bit INTER_LINEAR, and then
// MSE / PSNR / SSIM (compare_image_quality.py:100-106, :299-301, image_quality_comparison.py:17-18, complete_comparison.py:16-17,
// improved_image_compare.py:11-12).
//   mstg_cv_resize_coeffs      host only: index and the two 11-bit weights per destination position of one axis, the ONE place
//                              where the definition's double and float steps are evaluated;
//   cv_resize_linear_kernel    the resize alone, N images of one shape per launch, one thread per destination pixel;
//   pair_tile_kernel           P pairs of any shapes per launch, one workgroup per tile of a host-built tile list {pair, ty, tx, 0}:
//                              the tile of csrc/metrics.hip (csrc/metrics_tile.h) with b's patch staged by EVALUATING the resize
//                              from b's own pixels and the pair's tables -- four byte loads per staged byte, and the resized image
//                              is never written to memory.  A pair of equal shape stages b as a is staged;
//   pair_finish_kernel         one workgroup per pair adds that pair's tiles in their fixed order.
// A resized byte is a pure function of four source bytes and four weights, and the tile decomposition of a, the order of every sum
// and the finish are those of mstg_image_metrics_u8: row i is bit for bit mstg_image_metrics_u8(a_i, mstg_cv_resize_linear_u8(b_i)),
// whatever P and the order of the pairs.  No atomics.  A tile is checked against its descriptor before any access, and the
// kernels clamp every table index to its source, so a table of any content reads inside b.
#include <stdarg.h>

#include "metrics_tile.h"

namespace mstg {

constexpr int CV_ONE = 2048;  // INTER_RESIZE_COEF_SCALE: 11 bits

// the vertical pass' result byte from the two horizontal sums (int32) and the two vertical weights
__device__ __forceinline__ unsigned cv_linear_byte(int s00, int s01, int s10, int s11, int w0, int w1, int b0, int b1) {
    const int t0 = s00 * w0 + s01 * w1, t1 = s10 * w0 + s11 * w1;
    return (unsigned)((((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2) & 0xffu;  // the (uchar) cast: low 8 bits
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// device table of an axis with destination extent d: int32 [2 d] = index[d], then the d int16 weight pairs {w0, w1}
__device__ __forceinline__ void cv_axis(const int* __restrict__ table, int d, int i, int s, int* p0, int* p1, int* w0, int* w1) {
    const int p = table[i], w = table[d + i];
    *p0 = clampi(p, 0, s - 1);
    *p1 = clampi(p + 1, 0, s - 1);
    *w0 = (int)(short)(w & 0xffff);
    *w1 = w >> 16;
}

// src (N, Hs, Ws, 3) -> dst (N, Hd, Wd, 3); grid (pixels of one image / 256, N)
__global__ __launch_bounds__(256) void cv_resize_linear_kernel(const unsigned char* __restrict__ src, int Hs, int Ws, int Hd, int Wd,
                                                               const int* __restrict__ table_v, const int* __restrict__ table_h,
                                                               unsigned char* __restrict__ dst) {
    const int e = blockIdx.x * 256 + threadIdx.x;  // Hd * Wd < 2^31 / 3
    if (e >= Hd * Wd) return;
    const int y = e / Wd, x = e - y * Wd;
    int r0, r1, b0, b1, p, q, w0, w1;
    cv_axis(table_v, Hd, y, Hs, &r0, &r1, &b0, &b1);
    cv_axis(table_h, Wd, x, Ws, &p, &q, &w0, &w1);
    const unsigned char* img = src + (size_t)blockIdx.y * Hs * Ws * 3;
    const unsigned char* s0 = img + (size_t)r0 * Ws * 3;
    const unsigned char* s1 = img + (size_t)r1 * Ws * 3;
    unsigned char* o = dst + ((size_t)blockIdx.y * Hd * Wd + (size_t)e) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (unsigned char)cv_linear_byte(s0[3 * p + c], s0[3 * q + c], s1[3 * p + c], s1[3 * q + c], w0, w1, b0, b1);
}

__global__ __launch_bounds__(MT_THREADS) void pair_tile_kernel(const mstg_pair_desc* __restrict__ descs, int P, const int4* __restrict__ tiles,
                                                               int ntiles, const int* __restrict__ table, double* __restrict__ ws) {
    __shared__ unsigned pa[MT_ROWS * MT_ROW_DW], pb[MT_ROWS * MT_ROW_DW];
    __shared__ int row_t[MT_ROWS][4];   // {row offset 0, row offset 1 (bytes of b), b0, b1} per patch row
    __shared__ int col_t[MT_W + 6][4];  // {3 p, 3 q, w0, w1} per patch pixel column
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= ntiles) return;
    const int4 t = tiles[blockIdx.x];
    if ((unsigned)t.x >= (unsigned)P) return;
    const mstg_pair_desc d = descs[t.x];
    if (d.ha < 7 || d.wa < 7 || d.hb < 1 || d.wb < 1) return;
    const int tiles_x = (d.wa - 6 + MT_W - 1) / MT_W, tiles_y = (d.ha - 6 + MT_H - 1) / MT_H;
    // the tile belongs to the pair and is the one whose workspace record this workgroup writes
    if (t.y < 0 || t.y >= tiles_y || t.z < 0 || t.z >= tiles_x || d.ntiles != tiles_x * tiles_y ||
        (long long)d.tile0 + t.y * tiles_x + t.z != (long long)blockIdx.x)
        return;
    const MetricsTile g = metrics_tile(d.ha, d.wa, t.y, t.z, tiles_x, tiles_y);
    const size_t pitch = (size_t)d.wa * 3;
    const unsigned char* a0 = d.a + (size_t)g.y0 * pitch + (size_t)g.x0 * 3;
    stage_patch(a0, pitch, g.rows, g.len, pa, tid);
    int sh_b0 = 0, sh_b_step = 0;
    if (d.hb == d.ha && d.wb == d.wa) {
        const unsigned char* b0p = d.b + (size_t)g.y0 * pitch + (size_t)g.x0 * 3;
        stage_patch(b0p, pitch, g.rows, g.len, pb, tid);
        sh_b0 = (int)((uintptr_t)b0p & 3);
        sh_b_step = (int)(pitch & 3);
    } else {
        // the pair's tables for this tile's rows and pixel columns, indices clamped to b
        if (tid < g.rows) {
            int r0, r1, b0, b1;
            cv_axis(table + d.table_v, d.ha, g.y0 + tid, d.hb, &r0, &r1, &b0, &b1);
            row_t[tid][0] = r0 * d.wb * 3;  // < hb * wb * 3 < 2^31
            row_t[tid][1] = r1 * d.wb * 3;
            row_t[tid][2] = b0;
            row_t[tid][3] = b1;
        } else if (tid >= 64 && 3 * (tid - 64) < g.len) {
            int p, q, w0, w1;
            cv_axis(table + d.table_h, d.wa, g.x0 + tid - 64, d.wb, &p, &q, &w0, &w1);
            col_t[tid - 64][0] = 3 * p;
            col_t[tid - 64][1] = 3 * q;
            col_t[tid - 64][2] = w0;
            col_t[tid - 64][3] = w1;
        }
        __syncthreads();
        // patch byte j of row r at byte j of LDS row r (no shift): each staged byte from four bytes of b
        // (a pointer read from a descriptor is generic to the compiler; typed as global memory the 16 byte loads per dword are
        // global loads, not flat ones)
        typedef const __attribute__((address_space(1))) unsigned char* gbytes;
        const gbytes b = (gbytes)d.b;
        for (int e = tid; e < MT_ROWS * MT_ROW_DW; e += MT_THREADS) {
            const int r = e / MT_ROW_DW, k = e - r * MT_ROW_DW;
            unsigned v = 0;
            if (r < g.rows && 4 * k < g.len) {
                const gbytes s0 = b + (size_t)row_t[r][0];
                const gbytes s1 = b + (size_t)row_t[r][1];
                const int b0 = row_t[r][2], b1 = row_t[r][3];
#pragma unroll
                for (int bb = 0; bb < 4; ++bb) {
                    const int j = 4 * k + bb;
                    if (j < g.len) {
                        const int x = j / 3, c = j - 3 * x;
                        const int p = col_t[x][0] + c, q = col_t[x][1] + c;
                        v |= cv_linear_byte(s0[p], s0[q], s1[p], s1[q], col_t[x][2], col_t[x][3], b0, b1) << (8 * bb);
                    }
                }
            }
            pb[e] = v;
        }
    }
    __syncthreads();
    ssim_tile_sums(pa, pb, (int)((uintptr_t)a0 & 3), (int)(pitch & 3), sh_b0, sh_b_step, g, ws + (size_t)blockIdx.x * 4);
}

// one workgroup per pair; its tiles are records [tile0, tile0 + ntiles) of the workspace
__global__ __launch_bounds__(MT_THREADS) void pair_finish_kernel(const mstg_pair_desc* __restrict__ descs, int ntiles, const double* __restrict__ ws,
                                                                 double* __restrict__ out) {
    const mstg_pair_desc d = descs[blockIdx.x];
    if (d.ha < 7 || d.wa < 7 || d.tile0 < 0 || d.ntiles < 1 || (long long)d.tile0 + d.ntiles > (long long)ntiles) return;
    metrics_finish_pair(ws + (size_t)d.tile0 * 4, d.ha, d.wa, d.ntiles, out + (size_t)blockIdx.x * 6);
}

// ---- host: the coefficient table, validation, the tile list ---------------------------------------------------------------------
static int pair_fail(int code, int i, const char* fmt, ...) {
    char what[192];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(what, sizeof(what), fmt, ap);
    va_end(ap);
    snprintf(g_last_error, sizeof(g_last_error), "pair_metrics: pair %d: %s", i, what);
    return code;
}

constexpr long long PAIR_MAX_TILES = (1ll << 24) - 1;  // workgroups of 256 threads: below 2^32 threads per launch

// shapes of pair i; adds its tiles to *total.  0 = fine, else the error code (message set)
static int pair_shape(const mstg_pair_desc& d, int i, long long* total, int* tiles_out) {
    if (d.ha < 1 || d.wa < 1 || d.hb < 1 || d.wb < 1)
        return pair_fail(MSTG_E_BADARG, i, "an extent is below 1: a is %d x %d, b is %d x %d", d.ha, d.wa, d.hb, d.wb);
    if (d.ha < 7 || d.wa < 7) return pair_fail(MSTG_E_BADARG, i, "image a %d x %d is smaller than the 7x7 SSIM window", d.ha, d.wa);
    if ((long long)d.ha * d.wa * 3 >= (1ll << 31))
        return pair_fail(MSTG_E_UNSUPPORTED, i, "H * W * 3 = %lld of image a does not fit 31 bits", (long long)d.ha * d.wa * 3);
    if ((long long)d.hb * d.wb * 3 >= (1ll << 31))
        return pair_fail(MSTG_E_UNSUPPORTED, i, "H * W * 3 = %lld of image b does not fit 31 bits", (long long)d.hb * d.wb * 3);
    const int n = cdiv(d.wa - 6, MT_W) * cdiv(d.ha - 6, MT_H);
    *total += n;
    if (*total > PAIR_MAX_TILES)
        return pair_fail(MSTG_E_UNSUPPORTED, i, "the total tile count reaches %lld, more than 2^24 - 1 workgroups in one launch (and int32 beyond)",
                         *total);
    *tiles_out = n;
    return MSTG_OK;
}

static int pair_shapes(const char* who, const mstg_pair_desc* descs, int P, long long* total) {
    if (!descs || P < 1) {
        snprintf(g_last_error, sizeof(g_last_error), "%s: null descriptors or P = %d, need at least one pair", who, P);
        return MSTG_E_BADARG;
    }
    *total = 0;
    for (int i = 0; i < P; ++i) {
        int n;
        if (int rc = pair_shape(descs[i], i, total, &n)) return rc;
    }
    return MSTG_OK;
}

}  // namespace mstg

using namespace mstg;

extern "C" int mstg_cv_resize_coeffs(int src, int dst, int horizontal, int32_t* index, int16_t* weights) {
#pragma clang fp contract(off)  // (i + 0.5) * scale - 0.5 below is a product and a difference, each rounded
    if (src < 1 || dst < 1) {
        snprintf(g_last_error, sizeof(g_last_error), "cv_resize_coeffs: extents %d -> %d, both must be at least 1", src, dst);
        return MSTG_E_BADARG;
    }
    if (!index || !weights) return fail_arg(MSTG_E_BADARG, "cv_resize_coeffs: null table pointer");
    const double inv_scale = (double)dst / (double)src;
    const double scale = 1.0 / inv_scale;
    for (int i = 0; i < dst; ++i) {
        const double pos = (i + 0.5) * scale;
        float f = (float)(pos - 0.5);
        int p = (int)floorf(f);
        f = f - (float)p;
        if (horizontal) {
            if (p < 0) p = 0, f = 0.f;
            if (p >= src - 1) p = src - 1, f = 0.f;
        }
        const float u0 = (1.f - f) * 2048.f, u1 = f * 2048.f;
        long w0 = lrintf(u0), w1 = lrintf(u1);  // ties to even (the default rounding mode)
        w0 = w0 < -32768 ? -32768 : (w0 > 32767 ? 32767 : w0);
        w1 = w1 < -32768 ? -32768 : (w1 > 32767 ? 32767 : w1);
        index[i] = p;
        weights[2 * i] = (int16_t)w0;
        weights[2 * i + 1] = (int16_t)w1;
    }
    return MSTG_OK;
}

extern "C" int mstg_cv_resize_linear_u8(const unsigned char* src, int N, int Hs, int Ws, int Hd, int Wd, const int32_t* table_v,
                                        const int32_t* table_h, unsigned char* dst, void* stream) {
    if (!src || !dst || !table_v || !table_h) return fail_arg(MSTG_E_BADARG, "cv_resize_linear_u8: null image, table or output pointer");
    char msg[200];
    if (N < 1 || Hs < 1 || Ws < 1 || Hd < 1 || Wd < 1) {
        snprintf(msg, sizeof(msg), "cv_resize_linear_u8: N = %d, %d x %d -> %d x %d: every extent must be at least 1", N, Hs, Ws, Hd, Wd);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    const long long sb = (long long)Hs * Ws * 3, db = (long long)Hd * Wd * 3;
    if (sb >= (1ll << 31) || db >= (1ll << 31)) {
        snprintf(msg, sizeof(msg), "cv_resize_linear_u8: H * W * 3 = %lld (source) / %lld (destination) does not fit 31 bits", sb, db);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    const long long blocks = ((long long)Hd * Wd + 255) / 256;
    if (N > 65535 || blocks * N > PAIR_MAX_TILES) {
        snprintf(msg, sizeof(msg), "cv_resize_linear_u8: N = %d images of %lld workgroups, more than 65535 images or 2^24 - 1 workgroups", N, blocks);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    if (((uintptr_t)table_v & 3) || ((uintptr_t)table_h & 3)) return fail_arg(MSTG_E_ALIGN, "cv_resize_linear_u8: tables not 4-byte aligned");
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)(sb * N), d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)(db * N);
    if (s0 < d1 && d0 < s1) return fail_arg(MSTG_E_BADARG, "cv_resize_linear_u8: the output overlaps the input");
    MSTG_LAUNCH(cv_resize_linear_kernel, dim3((unsigned)blocks, (unsigned)N), dim3(256), 0, (hipStream_t)stream, src, Hs, Ws, Hd, Wd,
                (const int*)table_v, (const int*)table_h, dst);
    MSTG_CHECK_LAUNCH("cv_resize_linear_kernel");
    return MSTG_OK;
}

extern "C" int mstg_pair_metrics_validate(const mstg_pair_desc* descs, int P, const int32_t* table, size_t table_len) {
    long long total;
    if (int rc = pair_shapes("pair_metrics", descs, P, &total)) return rc;
    long long run = 0;
    for (int i = 0; i < P; ++i) {
        const mstg_pair_desc& d = descs[i];
        if (!d.a || !d.b) return pair_fail(MSTG_E_BADARG, i, "null image pointer");
        const int n = cdiv(d.wa - 6, MT_W) * cdiv(d.ha - 6, MT_H);
        if (d.tile0 != run || d.ntiles != n)
            return pair_fail(MSTG_E_BADARG, i, "tile0 = %d, ntiles = %d do not belong to the shapes (%lld, %d)", d.tile0, d.ntiles, run, n);
        run += n;
        if (d.ha == d.hb && d.wa == d.wb) continue;
        const int64_t tl = (int64_t)table_len;
        if (d.table_v < 0 || d.table_v > tl || 2 * (int64_t)d.ha > tl - d.table_v || d.table_h < 0 || d.table_h > tl ||
            2 * (int64_t)d.wa > tl - d.table_h)
            return pair_fail(MSTG_E_BADARG, i, "table offset %lld / %lld past the table buffer of %lld words", (long long)d.table_v,
                             (long long)d.table_h, (long long)tl);
        if (table) {
            for (int y = 0; y < d.ha; ++y)
                if (table[d.table_v + y] < -1 || table[d.table_v + y] > d.hb - 1)
                    return pair_fail(MSTG_E_BADARG, i, "vertical index %d at row %d lies outside b's %d rows", table[d.table_v + y], y, d.hb);
            for (int x = 0; x < d.wa; ++x)
                if (table[d.table_h + x] < 0 || table[d.table_h + x] > d.wb - 1)
                    return pair_fail(MSTG_E_BADARG, i, "horizontal index %d at column %d lies outside b's %d columns", table[d.table_h + x], x,
                                     d.wb);
        }
    }
    return MSTG_OK;
}

extern "C" size_t mstg_pair_metrics_workspace_bytes(const mstg_pair_desc* descs, int P) {
    long long total;
    if (pair_shapes("pair_metrics_workspace_bytes", descs, P, &total) != MSTG_OK) return 0;
    return (size_t)total * 4 * sizeof(double);
}

extern "C" int mstg_pair_metrics_tiles(mstg_pair_desc* descs, int P, int32_t* tiles, size_t cap) {
    long long total;
    if (int rc = pair_shapes("pair_metrics_tiles", descs, P, &total)) return rc;
    if (tiles && (size_t)total > cap) return fail_arg(MSTG_E_WORKSPACE, "pair_metrics_tiles: tile buffer too small");
    int run = 0;
    for (int i = 0; i < P; ++i) {
        mstg_pair_desc& d = descs[i];
        const int tx = cdiv(d.wa - 6, MT_W), ty = cdiv(d.ha - 6, MT_H);
        d.tile0 = run;
        d.ntiles = tx * ty;
        if (tiles)
            for (int y = 0; y < ty; ++y)
                for (int x = 0; x < tx; ++x) {
                    int32_t* t = tiles + 4 * ((size_t)run + (size_t)y * tx + x);
                    t[0] = i; t[1] = y; t[2] = x; t[3] = 0;
                }
        run += tx * ty;
    }
    return (int)total;
}

extern "C" int mstg_pair_metrics_u8(const mstg_pair_desc* descs, int P, const int32_t* table, size_t table_len, const void* descs_dev,
                                    const int32_t* tiles_dev, int ntiles, const int32_t* table_dev, double* out, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    if (int rc = mstg_pair_metrics_validate(descs, P, table, table_len)) return rc;
    const long long total = (long long)descs[P - 1].tile0 + descs[P - 1].ntiles;
    if (!descs_dev || !tiles_dev || !out || ntiles != total) return fail_arg(MSTG_E_BADARG, "pair_metrics_u8: null pointer, or ntiles is not the pairs' tile count");
    bool resized = false;
    for (int i = 0; i < P; ++i) resized = resized || descs[i].ha != descs[i].hb || descs[i].wa != descs[i].wb;
    if (resized && (!table || !table_dev)) return fail_arg(MSTG_E_BADARG, "pair_metrics_u8: a pair needs a resize and there is no table");
    if (!workspace || workspace_bytes < (size_t)total * 4 * sizeof(double)) return fail_arg(MSTG_E_WORKSPACE, "pair_metrics_u8: workspace too small");
    if (((uintptr_t)workspace & 7) || ((uintptr_t)out & 7) || ((uintptr_t)descs_dev & 7) || ((uintptr_t)tiles_dev & 15) || ((uintptr_t)table_dev & 3))
        return fail_arg(MSTG_E_ALIGN, "pair_metrics_u8: out / workspace / descriptors / tiles / table not aligned (8 / 8 / 8 / 16 / 4 bytes)");
    MSTG_LAUNCH(pair_tile_kernel, dim3((unsigned)ntiles), dim3(MT_THREADS), 0, (hipStream_t)stream, (const mstg_pair_desc*)descs_dev, P,
                (const int4*)tiles_dev, ntiles, (const int*)table_dev, (double*)workspace);
    MSTG_CHECK_LAUNCH("pair_tile_kernel");
    MSTG_LAUNCH(pair_finish_kernel, dim3((unsigned)P), dim3(MT_THREADS), 0, (hipStream_t)stream, (const mstg_pair_desc*)descs_dev, ntiles,
                (const double*)workspace, out);
    MSTG_CHECK_LAUNCH("pair_finish_kernel");
    return MSTG_OK;
}
