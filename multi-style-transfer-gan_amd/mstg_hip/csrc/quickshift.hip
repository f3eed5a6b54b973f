// Quickshift (the `quickshift` method of the reference's get_segmentation_mask, enhanced_local_style.py:69-70) on the device, for a
// batch of (N, H, W, 3) uint8 canvases, as include/mstg_hip.h defines it: 8-bit Lab features, a fixed-point density, the parent of
// every pixel, labels numbered by ascending root.  tests/quickshift_ref.py is the same definition in numpy; neither has been compared
// with a scikit-image binary.  Every kernel takes N images per launch, offsets are 64-bit, the number of launches depends on H * W
// alone (the rounds of the pointer jumping), never on N or on the data:
//
// D  qs_density_kernel<SPLIT>  the hot one: (2 w + 1)^2 float64 exponentials per pixel (361 at kernel_size 3).  One workgroup of 256
//    threads per tile of 16 columns; the Lab words of the tile and a halo of w (one dword per pixel, 0xffffffff outside the image)
//    are computed from the SOURCE pixels into LDS, so a tap is one LDS read and nothing is read from a neighbour's output.  A term
//    is rint(exp(D * inv) * 2^32) as an integer and the density their integer sum: any split of a window gives the same bits.
//    SPLIT = 1: a thread per pixel, 16 x 16 tiles.  SPLIT = 4: four neighbouring lanes per pixel, lane k takes the window rows
//    -w + k, -w + k + 4, ..., 16 x 4 tiles, the four partial sums joined with two DPP quad moves (lanes.h).  A single 256 x 256
//    image is 1024 waves with SPLIT = 1, one per SIMD, and the chain of float64 operations of one exponential after the other is
//    then bound by latency; SPLIT = 4 gives the same image 4096 waves.  The host takes SPLIT = 4 below QS_SPLIT_BELOW pixels per
//    launch and SPLIT = 1 from there on, where the pixels alone fill the device and the narrower tiles would only stage more halo.
// P  qs_parents_kernel     a thread per pixel, 16 x 16 tiles, the Lab words and the int64 densities of the tile and a halo of
//    reach = min(w, floor(max_dist)) in LDS; row-major scan of the square with a strict <, so the lowest index wins among equal D.
// then the tail that slic.hip's connectivity step has (cc_resolve_number, u8_image.h): the rounds of pointer jumping over the
// parents in place and the numbering of the roots from 0.
//
// No floating-point atomics and no floating-point sum: bit-reproducible, independent of N and of SPLIT.
#include <cmath>
#include <cstdlib>

#include "lanes.h"
#include "u8_image.h"

namespace mstg {

constexpr int QS_THREADS = 256;
constexpr int QS_TW = 16, QS_TH = 16;  // the tile of a thread per pixel; SPLIT lanes per pixel: QS_TH / SPLIT rows
constexpr int QS_R = MSTG_QUICKSHIFT_MAX_RADIUS;
constexpr int QS_HALO = (QS_TH + 2 * QS_R) * (QS_TW + 2 * QS_R);  // dwords of the largest staged window
constexpr unsigned QS_OUTSIDE = 0xffffffffu;                      // a Lab word has 24 bits
constexpr long long QS_SPLIT_BELOW = 1 << 19;                     // pixels per launch below which four lanes share a pixel
static_assert(QS_TW * QS_TH == QS_THREADS, "a thread per pixel of the tile");

typedef unsigned long long u64;

// The Lab words (and, with dens, the densities) of rows y0 - r .. y0 + th - 1 + r and columns x0 - r .. x0 + QS_TW - 1 + r of an
// image into LDS, row length QS_TW + 2 r; th <= QS_TH and r <= QS_R: at most QS_HALO entries.  The caller places the barrier.
__device__ __forceinline__ void qs_stage(const unsigned char* __restrict__ img, const long long* __restrict__ dens,
                                         const unsigned short* __restrict__ lab, int H, int W, int y0, int x0, int th, int r, unsigned* s,
                                         long long* sd, int tid) {
    const int cols = QS_TW + 2 * r, total = (th + 2 * r) * cols;
    for (int e = tid; e < total; e += QS_THREADS) {
        const int rr = e / cols, cc = e - rr * cols;
        const int y = y0 - r + rr, x = x0 - r + cc;
        const bool in = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
        const size_t at = in ? (size_t)y * W + x : 0;
        s[e] = in ? lab_px(load_px(img + at * 3), lab) : QS_OUTSIDE;
        if (dens) sd[e] = in ? dens[at] : 0;
    }
}

// D of the header for a pixel p and a tap t (Lab words), s = dr^2 + dc^2
__device__ __forceinline__ double qs_dist(unsigned p, unsigned t, int s, double kc) {
#pragma clang fp contract(off)  // the definition rounds the product and the sum
    const int dL = 100 * ((int)(t & 0xffu) - (int)(p & 0xffu));
    const int da = (int)((t >> 8) & 0xffu) - (int)((p >> 8) & 0xffu), db = (int)(t >> 16) - (int)(p >> 16);
    // q = dL^2 + 65025 (da^2 + db^2) < 2^34: the two parts fit an int, and they and their sum are exact in doubles
    const double q = (double)(dL * dL) + 65025.0 * (double)(da * da + db * db);
    return q * kc + (double)s;
}

template <int CTRL>
__device__ __forceinline__ u64 dpp_mov_u64(u64 v) {
    const unsigned lo = __builtin_bit_cast(unsigned, dpp_mov<CTRL>(__builtin_bit_cast(float, (unsigned)v)));
    const unsigned hi = __builtin_bit_cast(unsigned, dpp_mov<CTRL>(__builtin_bit_cast(float, (unsigned)(v >> 32))));
    return (u64)hi << 32 | lo;
}

template <int SPLIT>
__global__ __launch_bounds__(QS_THREADS) void qs_density_kernel(const unsigned char* __restrict__ img, const unsigned short* __restrict__ lab,
                                                                int H, int W, int w, double kc, double inv, int tiles_x, int tiles,
                                                                long long* __restrict__ dens) {
    static_assert(SPLIT == 1 || SPLIT == 4, "a pixel is one lane or one quad of lanes");
    constexpr int TH = QS_TH / SPLIT;
    __shared__ unsigned s[QS_HALO];
    const int tid = threadIdx.x;
    const auto [n, y0, x0] = tile_of<TH, QS_TW>(tiles, tiles_x);
    const size_t plane = (size_t)n * H * W;
    qs_stage(img + plane * 3, nullptr, lab, H, W, y0, x0, TH, w, s, nullptr, tid);
    __syncthreads();
    const int part = tid % SPLIT, pix = tid / SPLIT, ly = pix / QS_TW, lx = pix - ly * QS_TW;
    const int cols = QS_TW + 2 * w;
    const unsigned p = s[(ly + w) * cols + lx + w];
    u64 sum = 0;
    if (p != QS_OUTSIDE) {
        for (int dr = -w + part; dr <= w; dr += SPLIT) {
            const unsigned* row = s + (ly + w + dr) * cols + lx;  // columns lx - w .. lx + w of the image row
            for (int j = 0; j <= 2 * w; ++j) {
                const unsigned t = row[j];
                if (t == QS_OUTSIDE) continue;
                const int dc = j - w;
                const double D = qs_dist(p, t, dr * dr + dc * dc, kc);
                sum += (u64)(long long)__builtin_rint(exp(D * inv) * 4294967296.0);  // 0 .. 2^32, ties to even
            }
        }
    }
    if (SPLIT == 4) {  // every lane of the wave is here: the quads are whole
        sum += dpp_mov_u64<0xB1>(sum);  // quad_perm [1,0,3,2]
        sum += dpp_mov_u64<0x4E>(sum);  // quad_perm [2,3,0,1]
    }
    if (part == 0 && p != QS_OUTSIDE) dens[plane + (size_t)(y0 + ly) * W + x0 + lx] = (long long)sum;
}

__global__ __launch_bounds__(QS_THREADS) void qs_parents_kernel(const unsigned char* __restrict__ img, const long long* __restrict__ dens,
                                                                const unsigned short* __restrict__ lab, int H, int W, int reach, double kc,
                                                                double max2, int tiles_x, int tiles, int* __restrict__ parent) {
    __shared__ unsigned s[QS_HALO];
    __shared__ long long sd[QS_HALO];
    const int tid = threadIdx.x;
    const auto [n, y0, x0] = tile_of<QS_TH, QS_TW>(tiles, tiles_x);
    const size_t plane = (size_t)n * H * W;
    qs_stage(img + plane * 3, dens + plane, lab, H, W, y0, x0, QS_TH, reach, s, sd, tid);
    __syncthreads();
    const int ly = tid / QS_TW, lx = tid - ly * QS_TW;
    const int cols = QS_TW + 2 * reach, at = (ly + reach) * cols + lx + reach;
    const unsigned p = s[at];
    if (p == QS_OUTSIDE) return;
    const long long T = sd[at];
    const int idx = (y0 + ly) * W + x0 + lx;  // H * W <= MSTG_SEGMENT_MAX_PIXELS
    double best = __builtin_inf();
    int bp = idx;
    for (int dr = -reach; dr <= reach; ++dr) {
        const int base = at + dr * cols - reach;
        for (int j = 0; j <= 2 * reach; ++j) {
            const unsigned t = s[base + j];
            if (t == QS_OUTSIDE) continue;
            const int dc = j - reach, tidx = idx + dr * W + dc;
            const long long Tt = sd[base + j];
            if (!(Tt > T || (Tt == T && tidx < idx))) continue;  // not higher than p
            const double D = qs_dist(p, t, dr * dr + dc * dc, kc);
            if (D < best) {  // strict: among equal D the first of the row-major scan, the lowest index
                best = D;
                bp = tidx;
            }
        }
    }
    parent[plane + idx] = best > max2 ? idx : bp;  // nothing higher (best = inf) or too far: a root
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
struct QsPlan {
    int w, reach;
    double kc, inv, max2;
};

// the shape and kernel_size; 0 = fine, else the error code (message set)
static int qs_shape(const char* who, int N, int H, int W, double kernel_size, QsPlan& q) {
    char msg[240];
    int rc = check_extent(who, N, H, W);
    if (rc != MSTG_OK) return rc;
    const long long hw = (long long)H * W;
    if (hw > MSTG_SEGMENT_MAX_PIXELS) {
        snprintf(msg, sizeof(msg), "%s: H * W = %lld is more than %d", who, hw, MSTG_SEGMENT_MAX_PIXELS);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    if (!std::isfinite(kernel_size) || kernel_size < 1) {
        snprintf(msg, sizeof(msg), "%s: kernel_size = %g: need a finite value of at least 1", who, kernel_size);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    const double wd = std::ceil(3.0 * kernel_size);
    if (wd > MSTG_QUICKSHIFT_MAX_RADIUS) {
        snprintf(msg, sizeof(msg), "%s: kernel_size = %g gives the window radius w = %g, more than %d", who, kernel_size, wd,
                 MSTG_QUICKSHIFT_MAX_RADIUS);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    q.w = (int)wd;
    q.inv = -0.5 / (kernel_size * kernel_size);
    // the finest grid: 16 x 4 tiles (SPLIT = 4); the point-wise kernels of the tail take 256 pixels a workgroup
    const long long blocks = (long long)N * cdiv(H, QS_TH / 4) * cdiv(W, QS_TW);
    return check_grid(who, blocks, 31, "N * tiles", blocks);
}

// ratio and, with has_dist, max_dist
static int qs_params(const char* who, double ratio, bool has_dist, double max_dist, QsPlan& q) {
    char msg[200];
    if (!(ratio >= 0 && ratio <= 1)) {
        snprintf(msg, sizeof(msg), "%s: ratio = %g: need a value in [0, 1]", who, ratio);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    q.kc = (ratio * ratio) / 65025.0;
    q.reach = 0, q.max2 = 0;
    if (!has_dist) return MSTG_OK;
    if (!std::isfinite(max_dist) || max_dist <= 0) {
        snprintf(msg, sizeof(msg), "%s: max_dist = %g: need a finite value above 0", who, max_dist);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    q.max2 = max_dist * max_dist;
    q.reach = (int)std::fmin((double)q.w, std::floor(max_dist));
    return MSTG_OK;
}

// dens: N * H * W int64; jump, num: N * H * W ints each; the blocks' counts of the numbering
struct QsWorkspace {
    size_t dens, jump, num, bsum, total;
};
static QsWorkspace qs_workspace(int N, int H, int W) {
    const size_t px = (size_t)N * H * W, plane = align16(px * sizeof(int));
    QsWorkspace w;
    w.dens = 0;
    w.jump = align16(px * sizeof(long long));
    w.num = w.jump + plane;
    w.bsum = w.num + plane;
    w.total = w.bsum + align16((size_t)N * cc_blocks((size_t)H * W) * sizeof(int));
    return w;
}

static int qs_density(const unsigned char* img, int N, int H, int W, const QsPlan& q, const unsigned short* lab, long long* dens, hipStream_t st) {
    int split = (long long)N * H * W < QS_SPLIT_BELOW ? 4 : 1;
    if (const char* e = getenv("MSTG_QUICKSHIFT_SPLIT")) {  // experiments (tools/bench_quickshift.py): the same bits either way
        const int v = atoi(e);
        if (v == 1 || v == 4) split = v;
    }
    const int tx = cdiv(W, QS_TW);
    if (split == 4) {
        const int tiles = tx * cdiv(H, QS_TH / 4);
        MSTG_LAUNCH(qs_density_kernel<4>, dim3((unsigned)((size_t)N * tiles)), dim3(QS_THREADS), 0, st, img, lab, H, W, q.w, q.kc, q.inv, tx, tiles, dens);
    } else {
        const int tiles = tx * cdiv(H, QS_TH);
        MSTG_LAUNCH(qs_density_kernel<1>, dim3((unsigned)((size_t)N * tiles)), dim3(QS_THREADS), 0, st, img, lab, H, W, q.w, q.kc, q.inv, tx, tiles, dens);
    }
    MSTG_CHECK_LAUNCH("qs_density_kernel");
    return MSTG_OK;
}

static int qs_parents(const unsigned char* img, const long long* dens, int N, int H, int W, const QsPlan& q, const unsigned short* lab, int* parent,
                      hipStream_t st) {
    const int tx = cdiv(W, QS_TW), tiles = tx * cdiv(H, QS_TH);
    MSTG_LAUNCH(qs_parents_kernel, dim3((unsigned)((size_t)N * tiles)), dim3(QS_THREADS), 0, st, img, dens, lab, H, W, q.reach, q.kc, q.max2, tx, tiles,
                parent);
    MSTG_CHECK_LAUNCH("qs_parents_kernel");
    return MSTG_OK;
}

// nulls, alignment and overlaps of an entry: in[] are read, out[] written (the workspace among them); every out against every
// in and every other out
struct QsBuf {
    const void* p;
    size_t bytes, align;
};
static int qs_buffers(const char* who, const QsBuf* in, int n_in, const QsBuf* out, int n_out) {
    char msg[200];
    for (int i = 0; i < n_in + n_out; ++i) {
        const QsBuf& b = i < n_in ? in[i] : out[i - n_in];
        if (!b.p) {
            snprintf(msg, sizeof(msg), "%s: null image, table, density, parent, labels or count pointer", who);
            return fail_arg(MSTG_E_BADARG, msg);
        }
        if ((uintptr_t)b.p & (b.align - 1)) {
            snprintf(msg, sizeof(msg), "%s: table not 2-byte, labels, parent or count not 4-byte, density not 8-byte or workspace not 16-byte aligned", who);
            return fail_arg(MSTG_E_ALIGN, msg);
        }
    }
    for (int a = 0; a < n_out; ++a) {
        bool bad = false;
        for (int b = 0; b < n_in; ++b) bad = bad || overlaps(out[a].p, out[a].bytes, in[b].p, in[b].bytes);
        for (int b = 0; b < a; ++b) bad = bad || overlaps(out[a].p, out[a].bytes, out[b].p, out[b].bytes);
        if (bad) {
            snprintf(msg, sizeof(msg), "%s: an output or the workspace overlaps an input or another output", who);
            return fail_arg(MSTG_E_BADARG, msg);
        }
    }
    return MSTG_OK;
}

}  // namespace mstg

using namespace mstg;

extern "C" size_t mstg_quickshift_workspace_bytes(int N, int H, int W, double kernel_size) {
    QsPlan q;
    if (qs_shape("quickshift_workspace_bytes", N, H, W, kernel_size, q) != MSTG_OK) return 0;
    return qs_workspace(N, H, W).total;
}

extern "C" int mstg_quickshift_density_u8(const unsigned char* img, int N, int H, int W, double ratio, double kernel_size,
                                          const unsigned short* lab_table, long long* density_i64, void* stream) {
    QsPlan q;
    int rc = qs_shape("quickshift_density_u8", N, H, W, kernel_size, q);  // first: the refusals do not depend on the buffers
    if (rc == MSTG_OK) rc = qs_params("quickshift_density_u8", ratio, false, 0, q);
    if (rc != MSTG_OK) return rc;
    const size_t px = (size_t)N * H * W;
    const QsBuf in[2] = {{img, px * 3, 1}, {lab_table, 2 * MSTG_LAB_TABLE_U16, 2}}, out[1] = {{density_i64, px * 8, 8}};
    rc = qs_buffers("quickshift_density_u8", in, 2, out, 1);
    if (rc != MSTG_OK) return rc;
    return qs_density(img, N, H, W, q, lab_table, density_i64, (hipStream_t)stream);
}

extern "C" int mstg_quickshift_parents_u8(const unsigned char* img, const long long* density_i64, int N, int H, int W, double ratio,
                                          double kernel_size, double max_dist, const unsigned short* lab_table, int* parent_i32, void* stream) {
    QsPlan q;
    int rc = qs_shape("quickshift_parents_u8", N, H, W, kernel_size, q);
    if (rc == MSTG_OK) rc = qs_params("quickshift_parents_u8", ratio, true, max_dist, q);
    if (rc != MSTG_OK) return rc;
    const size_t px = (size_t)N * H * W;
    const QsBuf in[3] = {{img, px * 3, 1}, {lab_table, 2 * MSTG_LAB_TABLE_U16, 2}, {density_i64, px * 8, 8}}, out[1] = {{parent_i32, px * 4, 4}};
    rc = qs_buffers("quickshift_parents_u8", in, 3, out, 1);
    if (rc != MSTG_OK) return rc;
    return qs_parents(img, density_i64, N, H, W, q, lab_table, parent_i32, (hipStream_t)stream);
}

extern "C" int mstg_quickshift_u8(const unsigned char* img, int N, int H, int W, double ratio, double kernel_size, double max_dist,
                                  const unsigned short* lab_table, int* labels, int* count, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    QsPlan q;
    int rc = qs_shape("quickshift_u8", N, H, W, kernel_size, q);
    if (rc == MSTG_OK) rc = qs_params("quickshift_u8", ratio, true, max_dist, q);
    if (rc != MSTG_OK) return rc;
    const QsWorkspace ws = qs_workspace(N, H, W);
    if (!workspace || workspace_bytes < ws.total) return fail_arg(MSTG_E_WORKSPACE, "quickshift_u8: workspace too small");
    const size_t px = (size_t)N * H * W;
    const QsBuf in[2] = {{img, px * 3, 1}, {lab_table, 2 * MSTG_LAB_TABLE_U16, 2}};
    const QsBuf out[3] = {{labels, px * 4, 4}, {count, (size_t)N * 4, 4}, {workspace, ws.total, 16}};
    rc = qs_buffers("quickshift_u8", in, 2, out, 3);
    if (rc != MSTG_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* base = (unsigned char*)workspace;
    long long* dens = (long long*)(base + ws.dens);
    int* jump = (int*)(base + ws.jump);
    rc = qs_density(img, N, H, W, q, lab_table, dens, st);
    if (rc == MSTG_OK) rc = qs_parents(img, dens, N, H, W, q, lab_table, jump, st);
    if (rc != MSTG_OK) return rc;
    return cc_resolve_number(jump, N, H, W, 0, (int*)(base + ws.num), (int*)(base + ws.bsum), labels, count, st);
}
