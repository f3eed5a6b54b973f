// Batched image pipeline: the steps of image.hip for N images of different sizes per launch (include/mstg_hip.h, "Batched image
// pipeline").  Folder inference (batch_process_images.py:176-236, :255-441) and MonetPhotoDataset batches (pretrain.py:32-57) make
// eight one-image launches per image around a forward that is only fast at batch size; here the number of launches does not
// depend on N:
//   pre   img_batch_resample_h_kernel   all images, only the rows / columns the vertical pass reads -> 8-bit intermediates
//         img_batch_resample_v_kernel   vertical pass + placement on the T x T canvas + fill + ToTensor / Normalize (+ grid mask)
//   post  img_batch_tensor_to_u8_kernel (N,3,T,T) fp32 / fp16 -> (N,T,T,3) uint8
//         (mstg_blend_u8 on the (N*T, T, 3) view)
//         img_batch_resample_h_kernel   reads each image's crop box from its canvas
//         img_batch_resample_v_kernel   -> ragged uint8 output
// Same integer arithmetic as image.hip (22-bit coefficients, 2^21 rounding term, clip8 after each pass), so every byte equals the
// one-image path.  Byte movers, HBM / latency bound: a workgroup takes one tile of a host-built tile list {image, y0, x0, extent},
// stages the tile's source segment and coefficient window in LDS with aligned dword loads, and writes whole dwords (the ragged
// ends of a row as bytes).  A tile is checked against its (host-validated) descriptor before any access; integer sums in a fixed
// order, no atomics.
#include "common.h"

namespace mstg {

constexpr int RS_BITS = 32 - 8 - 2;
constexpr int H_ROWS = 4, H_COLS = 64;      // horizontal tile: 4 intermediate rows (one wave each) x up to 64 columns
constexpr int H_SEG_BYTES = 4096;           // LDS per staged source row
constexpr int H_COEF_INTS = 4096;           // LDS for the tile's coefficient rows (extent * ksize)
constexpr int V_ROWS = 4, V_COLS = 64;      // vertical tile: up to 4 output rows (one wave each) x 64 columns
constexpr int V_PITCH = 200;                // LDS bytes per staged intermediate row: 192 + alignment slack
constexpr int V_SEG_ROWS = 200;             // intermediate rows a tile can stage
constexpr int V_COEF_INTS = 1024;

__device__ __forceinline__ unsigned char rs_clip8(int v) {
    v >>= RS_BITS;
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// global bytes [g, g + n) -> lds[(g & 3) ..]: aligned dword loads (the first / last dword may hold up to 3 neighbouring bytes)
__device__ __forceinline__ void stage_bytes(const unsigned char* g, int n, unsigned* lds, int lane, int nlanes) {
    const uintptr_t a = (uintptr_t)g;
    const unsigned* g4 = (const unsigned*)(a & ~(uintptr_t)3);
    const int nd = (int)((a & 3) + n + 3) >> 2;
    for (int i = lane; i < nd; i += nlanes) lds[i] = g4[i];
}

// LDS bytes [l, l + n) -> global [g, g + n): the aligned dwords of the destination as dword stores, its ragged ends as bytes
__device__ __forceinline__ void store_bytes(const unsigned char* l, unsigned char* g, int n, int lane, int nlanes) {
    int head = (int)((4 - ((uintptr_t)g & 3)) & 3);
    if (head > n) head = n;
    const int nd = (n - head) >> 2, tail = n - head - 4 * nd;
    unsigned* g4 = (unsigned*)(g + head);
    for (int i = lane; i < nd; i += nlanes) {
        const unsigned char* s = l + head + 4 * i;
        g4[i] = (unsigned)s[0] | ((unsigned)s[1] << 8) | ((unsigned)s[2] << 16) | ((unsigned)s[3] << 24);
    }
    if (lane < head) g[lane] = l[lane];
    if (lane < tail) g[head + 4 * nd + lane] = l[head + 4 * nd + lane];
}

// intermediate[y0 + r][x0 + c] = rs_clip8(2^21 + sum_x box[y_first + y0 + r][xmin + x] * k[win_x + x0 + c][x])   (ks_h = 0: a copy)
__global__ __launch_bounds__(256) void img_batch_resample_h_kernel(const mstg_img_desc* __restrict__ descs, int n, const int4* __restrict__ tiles,
                                                                   const int* __restrict__ table, unsigned char* __restrict__ inter) {
    __shared__ unsigned seg[H_ROWS][H_SEG_BYTES / 4];
    __shared__ int coef[H_COEF_INTS];
    __shared__ unsigned outt[H_ROWS][H_COLS * 3 / 4];
    const int4 t = tiles[blockIdx.x];
    if ((unsigned)t.x >= (unsigned)n) return;
    const mstg_img_desc& d = descs[t.x];
    const int y0 = t.y, x0 = t.z, tw = t.w;
    if (y0 < 0 || x0 < 0 || tw < 1 || tw > H_COLS || y0 >= d.irows || x0 + tw > d.win_w) return;
    const int rows = min(H_ROWS, d.irows - y0), ks = d.ks_h, c_first = d.win_x + x0;
    const int* bounds = table + d.bounds_h;
    int sx0, sx1;  // columns of the box this tile reads
    if (ks) {
        if (tw * ks > H_COEF_INTS) return;
        sx0 = bounds[2 * c_first];
        sx1 = bounds[2 * (c_first + tw - 1)] + bounds[2 * (c_first + tw - 1) + 1];
    } else {
        sx0 = c_first;
        sx1 = c_first + tw;
    }
    const int span = sx1 - sx0;
    if (sx0 < 0 || span <= 0 || sx1 > d.box_w || span * 3 + 6 > H_SEG_BYTES) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned char* g = d.src + ((size_t)(d.box_y + d.y_first + y0 + wave) * d.src_w + d.box_x + sx0) * 3;
    if (wave < rows) stage_bytes(g, span * 3, seg[wave], lane, 64);
    if (ks) {
        const int* kk = table + d.kk_h + (size_t)c_first * ks;
        for (int i = tid; i < tw * ks; i += 256) coef[i] = kk[i];
    }
    __syncthreads();
    if (wave < rows && lane < tw) {
        const unsigned char* s = (const unsigned char*)seg[wave] + ((uintptr_t)g & 3);
        unsigned char* o = (unsigned char*)outt[wave] + 3 * lane;
        if (ks) {
            int xmin = bounds[2 * (c_first + lane)] - sx0, xmax = bounds[2 * (c_first + lane) + 1];
            xmin = max(xmin, 0);
            xmax = min(min(xmax, ks), span - xmin);
            const int* k = coef + lane * ks;  // ks is odd: the lanes' rows start on different banks
            s += 3 * xmin;
            int s0 = 1 << (RS_BITS - 1), s1 = s0, s2 = s0;
            for (int x = 0; x < xmax; ++x) {
                const int w = k[x];
                s0 += s[3 * x] * w;
                s1 += s[3 * x + 1] * w;
                s2 += s[3 * x + 2] * w;
            }
            o[0] = rs_clip8(s0); o[1] = rs_clip8(s1); o[2] = rs_clip8(s2);
        } else {
            o[0] = s[3 * lane]; o[1] = s[3 * lane + 1]; o[2] = s[3 * lane + 2];
        }
    }
    __syncthreads();
    if (wave < rows)
        store_bytes((const unsigned char*)outt[wave], inter + d.inter_off + (size_t)(y0 + wave) * d.ipitch + (size_t)x0 * 3, tw * 3, lane, 64);
}

// TENSOR: tiles of the T x T canvas.  Pixel (y, x) inside the placed window = the vertical pass over the intermediate
//   rs_clip8(2^21 + sum_y inter[ymin - y_first + y][x - dst_x] * k[win_y + y - dst_y][y])   (ks_v = 0: a copy),
// outside it the fill byte; then ToTensor / Normalize in the two fp32 operations of u8_to_tensor_kernel, times the 8x8-grid mask
// when use_mask; out / image_out / mask_out (n, 3, T, T), out_u8 (nullable) = the (n, T, T, 3) canvas.
// !TENSOR: tiles of the window, bytes to out_u8 + out_off (win_h, win_w, 3).
template <bool TENSOR>
__global__ __launch_bounds__(256) void img_batch_resample_v_kernel(const mstg_img_desc* __restrict__ descs, int n, const int4* __restrict__ tiles,
                                                                   const int* __restrict__ table, const unsigned char* __restrict__ inter, int T,
                                                                   float* __restrict__ out, float* __restrict__ image_out,
                                                                   float* __restrict__ mask_out, unsigned char* __restrict__ out_u8, int use_mask) {
    __shared__ unsigned seg[V_SEG_ROWS * V_PITCH / 4];
    __shared__ int coef[V_COEF_INTS];
    __shared__ unsigned outt[V_ROWS][V_COLS * 3 / 4];
    const int4 t = tiles[blockIdx.x];
    if ((unsigned)t.x >= (unsigned)n) return;
    const mstg_img_desc& d = descs[t.x];
    const int y0 = t.y, x0 = t.z, th = t.w;
    const int OH = TENSOR ? T : d.win_h, OW = TENSOR ? T : d.win_w;
    if (y0 < 0 || x0 < 0 || th < 1 || th > V_ROWS || y0 >= OH || x0 >= OW) return;
    const int rows = min(th, OH - y0), cols = min(V_COLS, OW - x0);
    const int oy = TENSOR ? d.dst_y : 0, ox = TENSOR ? d.dst_x : 0, ks = d.ks_v;
    const int wy_lo = max(y0 - oy, 0), wy_hi = min(y0 + rows - oy, d.win_h);  // rows / columns of the window under this tile
    const int wx_lo = max(x0 - ox, 0), wx_hi = min(x0 + cols - ox, d.win_w);
    const int* bounds = table + d.bounds_v;
    const int tid = threadIdx.x, row = tid >> 6, col = tid & 63;
    int rlo = 0, nrows = 0, mis = 0;
    if (wy_lo < wy_hi && wx_lo < wx_hi) {
        int rhi;
        if (ks) {
            if ((wy_hi - wy_lo) * ks > V_COEF_INTS) return;
            const int last = d.win_y + wy_hi - 1;
            rlo = bounds[2 * (d.win_y + wy_lo)] - d.y_first;
            rhi = bounds[2 * last] + bounds[2 * last + 1] - d.y_first;
        } else {
            rlo = d.win_y + wy_lo - d.y_first;
            rhi = d.win_y + wy_hi - d.y_first;
        }
        nrows = rhi - rlo;
        if (rlo < 0 || rhi > d.irows || nrows <= 0 || nrows > V_SEG_ROWS) return;
        const unsigned char* base = inter + d.inter_off + (size_t)rlo * d.ipitch + (size_t)wx_lo * 3;
        mis = (int)((uintptr_t)base & 3);  // the same for every row: inter_off and ipitch are multiples of 4
        const int nd = (mis + (wx_hi - wx_lo) * 3 + 3) >> 2;
        for (int i = tid; i < nrows * nd; i += 256) {
            const int r = i / nd, j = i - r * nd;
            seg[r * (V_PITCH / 4) + j] = ((const unsigned*)(base - mis + (size_t)r * d.ipitch))[j];
        }
        if (ks) {
            const int* kk = table + d.kk_v + (size_t)(d.win_y + wy_lo) * ks;
            for (int i = tid; i < (wy_hi - wy_lo) * ks; i += 256) coef[i] = kk[i];
        }
    }
    __syncthreads();
    if (row < rows && col < cols) {
        const int y = y0 + row, x = x0 + col, wy = y - oy, wx = x - ox;
        unsigned char b0, b1, b2;
        if (wy >= 0 && wy < d.win_h && wx >= 0 && wx < d.win_w) {
            const unsigned char* s = (const unsigned char*)seg + mis + (wx - wx_lo) * 3;
            if (ks) {
                int ymin = bounds[2 * (d.win_y + wy)] - d.y_first - rlo, ymax = bounds[2 * (d.win_y + wy) + 1];
                ymin = max(ymin, 0);
                ymax = min(min(ymax, ks), nrows - ymin);
                const int* k = coef + (wy - wy_lo) * ks;
                s += ymin * V_PITCH;
                int s0 = 1 << (RS_BITS - 1), s1 = s0, s2 = s0;
                for (int yy = 0; yy < ymax; ++yy) {
                    const int w = k[yy];
                    s0 += s[yy * V_PITCH] * w;
                    s1 += s[yy * V_PITCH + 1] * w;
                    s2 += s[yy * V_PITCH + 2] * w;
                }
                b0 = rs_clip8(s0); b1 = rs_clip8(s1); b2 = rs_clip8(s2);
            } else {
                s += (d.win_y + wy - d.y_first - rlo) * V_PITCH;
                b0 = s[0]; b1 = s[1]; b2 = s[2];
            }
        } else {
            b0 = b1 = b2 = (unsigned char)d.fill;
        }
        if (TENSOR) {
            float m = 1.f;
            if (use_mask) {
                const int ps = T / 8;  // patch_size = img_size // 8 (pretrain.py:46)
                const int i = ps ? y / ps : 8, j = ps ? x / ps : 8;
                if (i < 8 && j < 8) m = ((d.grid >> (i * 8 + j)) & 1ull) ? 1.f : 0.f;
            }
            const size_t plane = (size_t)T * T, o = (size_t)t.x * 3 * plane + (size_t)y * T + x;
            const unsigned char b[3] = {b0, b1, b2};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float tt = (float)b[c] / 255.f;  // ToTensor: byte -> float32, div(255)
                const float v = (tt - 0.5f) / 0.5f;    // Normalize: sub_(mean).div_(std)
                out[o + c * plane] = v * m;
                if (image_out) image_out[o + c * plane] = v;
                if (mask_out) mask_out[o + c * plane] = m;
            }
        }
        if (!TENSOR || out_u8) {
            unsigned char* q = (unsigned char*)outt[row] + 3 * col;
            q[0] = b0; q[1] = b1; q[2] = b2;
        }
    }
    if (!TENSOR || out_u8) {
        __syncthreads();
        if (row < rows) {
            unsigned char* g = TENSOR ? out_u8 + (((size_t)t.x * T + y0 + row) * T + x0) * 3
                                      : out_u8 + d.out_off + ((size_t)(y0 + row) * d.win_w + x0) * 3;
            store_bytes((const unsigned char*)outt[row], g, cols * 3, col, 64);
        }
    }
}

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned char out_byte(float y) {  // tensor_to_u8_kernel's arithmetic
    float t = (y + 1.0f) / 2.0f;
    t = fminf(fmaxf(t, 0.f), 1.f);
    if (!(t == t)) t = 0.f;
    return (unsigned char)(t * 255.0f);
}

// y (N, 3, plane) -> dst (N, plane, 3): four pixels per thread, 16- / 8-byte plane loads when `vec` (plane % 4 == 0, y aligned),
// three dword stores
template <typename Tin, typename Vec4>
__global__ void img_batch_tensor_to_u8_kernel(const Tin* __restrict__ y, size_t plane, size_t total, unsigned char* __restrict__ dst, int vec) {
    const size_t g = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (g >= total) return;
    float v[3][4];
    if (vec) {
        const size_t img = g / plane, p = g - img * plane;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const Vec4 q = *reinterpret_cast<const Vec4*>(y + (img * 3 + c) * plane + p);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[c][j] = (float)q[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t gj = g + j < total ? g + j : total - 1, img = gj / plane, p = gj - img * plane;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][j] = (float)y[(img * 3 + c) * plane + p];
        }
    }
    unsigned char b[12];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) b[3 * j + c] = out_byte(v[c][j]);
    if (g + 4 <= total) {
        unsigned* o = reinterpret_cast<unsigned*>(dst + g * 3);
#pragma unroll
        for (int i = 0; i < 3; ++i)
            o[i] = (unsigned)b[4 * i] | ((unsigned)b[4 * i + 1] << 8) | ((unsigned)b[4 * i + 2] << 16) | ((unsigned)b[4 * i + 3] << 24);
    } else {
        for (size_t i = 0; i < (total - g) * 3; ++i) dst[g * 3 + i] = b[i];
    }
}

// ---- host: validation and tile lists ------------------------------------------------------------------------------------------
static int img_fail(int code, int i, const char* what) {
    snprintf(g_last_error, sizeof(g_last_error), "img_batch: image %d: %s", i, what);
    return code;
}

// bounds rows [first, first + count) of a table: inside [0, in_size), at most ks taps, both ends non-decreasing
static const char* check_bounds(const int32_t* b, int first, int count, int ks, int in_size) {
    int pmin = 0, pend = 0;
    for (int r = first; r < first + count; ++r) {
        const int mn = b[2 * r], ln = b[2 * r + 1];
        if (mn < 0 || ln < 1 || ln > ks || (int64_t)mn + ln > in_size) return "a bounds entry lies outside its source";
        if (r > first && (mn < pmin || mn + ln < pend)) return "bounds are not monotonic";
        pmin = mn;
        pend = mn + ln;
    }
    return nullptr;
}

static int validate_one(const mstg_img_desc& d, int i, const int32_t* table, size_t table_len, size_t inter_bytes, int canvas, size_t out_bytes) {
    const int64_t tl = (int64_t)table_len;
    if (!d.src) return img_fail(MSTG_E_BADARG, i, "null source pointer");
    if (d.src_h <= 0 || d.src_w <= 0 || d.box_h <= 0 || d.box_w <= 0 || d.rs_h <= 0 || d.rs_w <= 0 || d.win_h <= 0 || d.win_w <= 0 || d.irows <= 0)
        return img_fail(MSTG_E_BADARG, i, "a size is not positive");
    if (d.box_y < 0 || d.box_x < 0 || (int64_t)d.box_y + d.box_h > d.src_h || (int64_t)d.box_x + d.box_w > d.src_w)
        return img_fail(MSTG_E_BADARG, i, "source box outside the image");
    if (d.win_y < 0 || d.win_x < 0 || (int64_t)d.win_y + d.win_h > d.rs_h || (int64_t)d.win_x + d.win_w > d.rs_w)
        return img_fail(MSTG_E_BADARG, i, "window outside the resized image");
    if ((d.filter != 0 && d.filter != 1) || d.fill < 0 || d.fill > 255) return img_fail(MSTG_E_BADARG, i, "bad filter or fill byte");
    if (d.ks_h != (d.rs_w == d.box_w ? 0 : mstg_resample_ksize(d.box_w, d.rs_w, d.filter)) ||
        d.ks_v != (d.rs_h == d.box_h ? 0 : mstg_resample_ksize(d.box_h, d.rs_h, d.filter)))
        return img_fail(MSTG_E_BADARG, i, "ks_h / ks_v do not belong to the sizes");
    if (d.y_first < 0 || (int64_t)d.y_first + d.irows > d.box_h) return img_fail(MSTG_E_BADARG, i, "intermediate rows outside the source box");
    if (d.ipitch % 4 || (int64_t)d.ipitch < 3 * (int64_t)d.win_w || d.inter_off < 0 || d.inter_off % 4 ||
        d.inter_off > (int64_t)inter_bytes || (int64_t)d.irows * d.ipitch > (int64_t)inter_bytes - d.inter_off)
        return img_fail(MSTG_E_BADARG, i, "intermediate extent outside its buffer (or not dword aligned)");
    if (d.ks_h) {
        if (d.kk_h < 0 || d.bounds_h < 0 || d.kk_h > tl || (int64_t)d.rs_w * d.ks_h > tl - d.kk_h || d.bounds_h > tl || 2 * (int64_t)d.rs_w > tl - d.bounds_h)
            return img_fail(MSTG_E_BADARG, i, "horizontal table offset past the table buffer");
        if (table)
            if (const char* e = check_bounds(table + d.bounds_h, d.win_x, d.win_w, d.ks_h, d.box_w)) return img_fail(MSTG_E_BADARG, i, e);
    }
    if (d.ks_v) {
        if (d.kk_v < 0 || d.bounds_v < 0 || d.kk_v > tl || (int64_t)d.rs_h * d.ks_v > tl - d.kk_v || d.bounds_v > tl || 2 * (int64_t)d.rs_h > tl - d.bounds_v)
            return img_fail(MSTG_E_BADARG, i, "vertical table offset past the table buffer");
        if (table) {
            const int32_t* b = table + d.bounds_v;
            if (const char* e = check_bounds(b, d.win_y, d.win_h, d.ks_v, d.box_h)) return img_fail(MSTG_E_BADARG, i, e);
            const int last = d.win_y + d.win_h - 1;
            if (b[2 * d.win_y] < d.y_first || b[2 * last] + b[2 * last + 1] > d.y_first + d.irows)
                return img_fail(MSTG_E_BADARG, i, "the vertical pass reads rows the intermediate does not hold");
        }
    } else if (d.win_y < d.y_first || (int64_t)d.win_y + d.win_h > (int64_t)d.y_first + d.irows) {
        return img_fail(MSTG_E_BADARG, i, "the vertical pass reads rows the intermediate does not hold");
    }
    if (canvas > 0) {
        if (d.dst_y < 0 || d.dst_x < 0 || (int64_t)d.dst_y + d.win_h > canvas || (int64_t)d.dst_x + d.win_w > canvas)
            return img_fail(MSTG_E_BADARG, i, "window placed outside the canvas");
    } else if (d.out_off < 0 || d.out_off > (int64_t)out_bytes || 3 * (int64_t)d.win_h * d.win_w > (int64_t)out_bytes - d.out_off) {
        return img_fail(MSTG_E_BADARG, i, "output extent outside its buffer");
    }
    return MSTG_OK;
}

static int launch_args_ok(const void* descs_dev, const void* tiles_dev, int ntiles, const void* table_dev, const void* inter, const char* what) {
    if (!descs_dev || !tiles_dev || !table_dev || !inter || ntiles <= 0) return fail_arg(MSTG_E_BADARG, what);
    if (((uintptr_t)descs_dev & 7) || ((uintptr_t)tiles_dev & 15) || ((uintptr_t)table_dev & 3) || ((uintptr_t)inter & 3))
        return fail_arg(MSTG_E_ALIGN, "img_batch: descriptors / tiles / table / intermediate are not aligned (8 / 16 / 4 / 4 bytes)");
    return MSTG_OK;
}

}  // namespace mstg

using namespace mstg;

extern "C" int mstg_img_batch_validate(const mstg_img_desc* descs, int n, const int32_t* table, size_t table_len, size_t inter_bytes,
                                       int canvas, size_t out_bytes) {
    if (!descs || n <= 0 || canvas < 0 || canvas > 32768) return fail_arg(MSTG_E_BADARG, "img_batch: null descriptors, no images or a bad canvas size");
    for (int i = 0; i < n; ++i)
        if (int rc = validate_one(descs[i], i, table, table_len, inter_bytes, canvas, out_bytes)) return rc;
    return MSTG_OK;
}

extern "C" int mstg_img_batch_tiles(const mstg_img_desc* descs, int n, const int32_t* table, size_t table_len, int pass, int canvas,
                                    int32_t* tiles, size_t cap) {
    if (pass != MSTG_IMG_PASS_H && pass != MSTG_IMG_PASS_V_TENSOR && pass != MSTG_IMG_PASS_V_U8) return fail_arg(MSTG_E_BADARG, "img_batch_tiles: bad pass");
    if (!table || (pass == MSTG_IMG_PASS_V_TENSOR) != (canvas > 0)) return fail_arg(MSTG_E_BADARG, "img_batch_tiles: null table or canvas does not fit the pass");
    // extents are checked here only as far as the tile sizes need them: buffers are not known yet (pass the largest sizes)
    if (int rc = mstg_img_batch_validate(descs, n, table, table_len, (size_t)INT64_MAX, canvas, (size_t)INT64_MAX)) return rc;
    size_t count = 0;
    auto emit = [&](int i, int y0, int x0, int ext) {
        if (tiles && count < cap) {
            int32_t* t = tiles + 4 * count;
            t[0] = i; t[1] = y0; t[2] = x0; t[3] = ext;
        }
        ++count;
    };
    for (int i = 0; i < n; ++i) {
        const mstg_img_desc& d = descs[i];
        if (pass == MSTG_IMG_PASS_H) {
            int tw = H_COLS;
            if (d.ks_h) {
                const int32_t* b = table + d.bounds_h;
                for (; tw >= 1; tw >>= 1) {  // the widest tile whose source segment and coefficient rows fit the LDS
                    bool fits = (int64_t)tw * d.ks_h <= H_COEF_INTS;
                    for (int x0 = 0; fits && x0 < d.win_w; x0 += tw) {
                        const int c0 = d.win_x + x0, c1 = d.win_x + (x0 + tw < d.win_w ? x0 + tw : d.win_w) - 1;
                        fits = ((int64_t)b[2 * c1] + b[2 * c1 + 1] - b[2 * c0]) * 3 + 6 <= H_SEG_BYTES;
                    }
                    if (fits) break;
                }
                if (tw < 1) return img_fail(MSTG_E_UNSUPPORTED, i, "horizontal reduction factor too large for the batched kernels");
            }
            for (int y0 = 0; y0 < d.irows; y0 += H_ROWS)
                for (int x0 = 0; x0 < d.win_w; x0 += tw) emit(i, y0, x0, x0 + tw < d.win_w ? tw : d.win_w - x0);
        } else {
            const int OH = canvas > 0 ? canvas : d.win_h, OW = canvas > 0 ? canvas : d.win_w, oy = canvas > 0 ? d.dst_y : 0;
            int th = V_ROWS;
            if (d.ks_v) {
                const int32_t* b = table + d.bounds_v;
                for (; th >= 1; th >>= 1) {
                    bool fits = (int64_t)th * d.ks_v <= V_COEF_INTS;
                    for (int y0 = 0; fits && y0 < OH; y0 += th) {
                        const int lo = y0 - oy > 0 ? y0 - oy : 0, hi = y0 + th - oy < d.win_h ? y0 + th - oy : d.win_h;
                        if (lo >= hi) continue;
                        const int r0 = d.win_y + lo, r1 = d.win_y + hi - 1;
                        fits = (int64_t)b[2 * r1] + b[2 * r1 + 1] - b[2 * r0] <= V_SEG_ROWS;
                    }
                    if (fits) break;
                }
                if (th < 1) return img_fail(MSTG_E_UNSUPPORTED, i, "vertical reduction factor too large for the batched kernels");
            }
            for (int y0 = 0; y0 < OH; y0 += th)
                for (int x0 = 0; x0 < OW; x0 += V_COLS) emit(i, y0, x0, th);
        }
    }
    if (count > (size_t)INT32_MAX) return fail_arg(MSTG_E_UNSUPPORTED, "img_batch_tiles: more than 2^31 tiles");
    if (tiles && count > cap) return fail_arg(MSTG_E_WORKSPACE, "img_batch_tiles: tile buffer too small");
    return (int)count;
}

extern "C" int mstg_img_batch_resample_h(const mstg_img_desc* descs, int n, const int32_t* table, size_t table_len, const void* descs_dev,
                                         const int32_t* tiles_dev, int ntiles, const int32_t* table_dev, unsigned char* inter,
                                         size_t inter_bytes, void* stream) {
    // the horizontal pass itself places nothing: canvas / output extents belong to the vertical entries
    if (int rc = mstg_img_batch_validate(descs, n, table, table_len, inter_bytes, 0, (size_t)INT64_MAX)) return rc;
    if (int rc = launch_args_ok(descs_dev, tiles_dev, ntiles, table_dev, inter, "img_batch_resample_h: null pointer or no tiles")) return rc;
    MSTG_LAUNCH(img_batch_resample_h_kernel, dim3((unsigned)ntiles), dim3(256), 0, (hipStream_t)stream, (const mstg_img_desc*)descs_dev, n,
                (const int4*)tiles_dev, table_dev, inter);
    MSTG_CHECK_LAUNCH("img_batch_resample_h_kernel");
    return MSTG_OK;
}

extern "C" int mstg_img_batch_resample_v_tensor(const mstg_img_desc* descs, int n, const int32_t* table, size_t table_len,
                                                const void* descs_dev, const int32_t* tiles_dev, int ntiles, const int32_t* table_dev,
                                                const unsigned char* inter, size_t inter_bytes, int T, float* out, float* image_out,
                                                float* mask_out, unsigned char* canvas_u8, int use_mask, void* stream) {
    if (T <= 0) return fail_arg(MSTG_E_BADARG, "img_batch_resample_v_tensor: bad canvas size");
    if (int rc = mstg_img_batch_validate(descs, n, table, table_len, inter_bytes, T, 0)) return rc;
    if (int rc = launch_args_ok(descs_dev, tiles_dev, ntiles, table_dev, inter, "img_batch_resample_v_tensor: null pointer or no tiles")) return rc;
    if (!out) return fail_arg(MSTG_E_BADARG, "img_batch_resample_v_tensor: null output");
    MSTG_LAUNCH(img_batch_resample_v_kernel<true>, dim3((unsigned)ntiles), dim3(256), 0, (hipStream_t)stream, (const mstg_img_desc*)descs_dev, n,
                (const int4*)tiles_dev, table_dev, inter, T, out, image_out, mask_out, canvas_u8, use_mask);
    MSTG_CHECK_LAUNCH("img_batch_resample_v_kernel<true>");
    return MSTG_OK;
}

extern "C" int mstg_img_batch_resample_v_u8(const mstg_img_desc* descs, int n, const int32_t* table, size_t table_len, const void* descs_dev,
                                            const int32_t* tiles_dev, int ntiles, const int32_t* table_dev, const unsigned char* inter,
                                            size_t inter_bytes, unsigned char* out, size_t out_bytes, void* stream) {
    if (int rc = mstg_img_batch_validate(descs, n, table, table_len, inter_bytes, 0, out_bytes)) return rc;
    if (int rc = launch_args_ok(descs_dev, tiles_dev, ntiles, table_dev, inter, "img_batch_resample_v_u8: null pointer or no tiles")) return rc;
    if (!out) return fail_arg(MSTG_E_BADARG, "img_batch_resample_v_u8: null output");
    MSTG_LAUNCH(img_batch_resample_v_kernel<false>, dim3((unsigned)ntiles), dim3(256), 0, (hipStream_t)stream, (const mstg_img_desc*)descs_dev, n,
                (const int4*)tiles_dev, table_dev, inter, 0, (float*)nullptr, (float*)nullptr, (float*)nullptr, out, 0);
    MSTG_CHECK_LAUNCH("img_batch_resample_v_kernel<false>");
    return MSTG_OK;
}

extern "C" int mstg_img_batch_tensor_to_u8(const void* y, int is_f16, int N, int H, int W, unsigned char* dst, void* stream) {
    if (!y || !dst || N <= 0 || H <= 0 || W <= 0) return fail_arg(MSTG_E_BADARG, "img_batch_tensor_to_u8: bad argument");
    if ((uintptr_t)dst & 3) return fail_arg(MSTG_E_ALIGN, "img_batch_tensor_to_u8: dst is not dword aligned");
    const size_t plane = (size_t)H * W, total = plane * N;
    const int vec = plane % 4 == 0 && ((uintptr_t)y & 15) == 0;
    const unsigned grid = (unsigned)cdivz(cdivz(total, 4), 256);
    if (is_f16) {
        MSTG_LAUNCH((img_batch_tensor_to_u8_kernel<_Float16, f16x4>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const _Float16*)y, plane, total,
                    dst, vec);
    } else {
        MSTG_LAUNCH((img_batch_tensor_to_u8_kernel<float, f32x4>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)y, plane, total, dst,
                    vec);
    }
    MSTG_CHECK_LAUNCH("img_batch_tensor_to_u8_kernel");
    return MSTG_OK;
}
