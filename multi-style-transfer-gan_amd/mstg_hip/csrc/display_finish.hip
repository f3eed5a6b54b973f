// The display finish of the reference's process_image (m_test.py:52-78) on the device (include/mstg_hip.h, "DISPLAY FINISH"):
// gamma 1.1 on the generator's output and its cast to bytes, the 8-bit COLOR_RGB2YUV, equalizeHist of Y, the 8-bit COLOR_YUV2RGB.
//
// gamma_u8_kernel        point-wise: (N, 3, H, W) float32 / float16 -> (N, H, W, 3) bytes; four pixels a thread.
// luma_hist_kernel       a workgroup per chunk of an image: a 256-bin histogram of Y in LDS (integer atomics), written whole to the
//                        workspace (no global atomics, nothing to zero).
// luma_lut_kernel        a workgroup per image, thread = bin: the chunks added in ascending order, the first non-empty bin, an
//                        inclusive prefix sum, the table.
// luma_apply_kernel      point-wise: Y, U, V again, the table, YUV -> RGB; four pixels a thread.
// Three launches for the equalisation whatever N.  The integer steps are exact; the float steps are single operations.
#include <hip/hip_fp16.h>
#include <math.h>

#include "u8_image.h"

namespace mstg {

constexpr int DF_THREADS = 256;
constexpr int DF_CHUNK = DF_THREADS * 16;  // pixels of a histogram chunk at the finest split
constexpr int DF_MAX_CHUNKS = 256;         // chunks of an image at most; a larger image gives each chunk more pixels

__device__ __forceinline__ int sat_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// the 8-bit COLOR_RGB2YUV of a packed pixel: 14-bit fixed point, arithmetic shifts
__device__ __forceinline__ void yuv_px(unsigned q, int& Y, int& U, int& V) {
    const int R = q & 0xff, B = q >> 16;
    Y = gray_px(q);
    U = sat_u8(((B - Y) * 8061 + (128 << 14) + 8192) >> 14);
    V = sat_u8(((R - Y) * 14369 + (128 << 14) + 8192) >> 14);
}

// the 8-bit COLOR_YUV2RGB
__device__ __forceinline__ unsigned rgb_of_yuv(int Y, int U, int V) {
    const int u = U - 128, v = V - 128;
    const int b = sat_u8(Y + ((u * 33292 + 8192) >> 14));
    const int g = sat_u8(Y + ((u * -6472 + v * -9519 + 8192) >> 14));
    const int r = sat_u8(Y + ((v * 18678 + 8192) >> 14));
    return (unsigned)r | (unsigned)g << 8 | (unsigned)b << 16;
}

__device__ __forceinline__ float df_load(const float* p) { return *p; }
__device__ __forceinline__ float df_load(const __half* p) { return __half2float(*p); }

template <typename T>
__global__ __launch_bounds__(DF_THREADS) void gamma_u8_kernel(const T* __restrict__ y, int HW, int groups, double gamma,
                                                              unsigned char* __restrict__ out) {
#pragma clang fp contract(off)
    const int n = blockIdx.x / groups, grp = blockIdx.x - n * groups;
    const int p0 = (grp * DF_THREADS + threadIdx.x) * 4;  // first of this thread's four pixels
    if (p0 >= HW) return;
    const int cnt = min(4, HW - p0);
    const T* src = y + (size_t)n * 3 * HW;
    unsigned px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < cnt)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float v = df_load(src + (size_t)ch * HW + p0 + k) * 0.5f + 0.5f;
                v = v > 0.f ? (v < 1.f ? v : 1.f) : 0.f;  // a NaN gives 0
                const float pw = (float)pow((double)v, gamma);
                px[k] |= (unsigned)(unsigned char)(pw * 255.f) << (8 * ch);
            }
    store_px4(out + ((size_t)n * HW + p0) * 3, px, cnt);
}

// hists: [N][chunks][256] ints
__global__ __launch_bounds__(DF_THREADS) void luma_hist_kernel(const unsigned char* __restrict__ img, int HW, int chunks, int chunk_px,
                                                               int* __restrict__ hists) {
    __shared__ int hist[256];
    const int n = blockIdx.x / chunks, c = blockIdx.x - n * chunks;
    hist[threadIdx.x] = 0;
    __syncthreads();
    const unsigned char* src = img + (size_t)n * HW * 3;
    const long long lo = (long long)c * chunk_px;
    const int hi = (int)min((long long)HW, lo + chunk_px);
    for (int p = (int)lo + threadIdx.x; p < hi; p += DF_THREADS) atomicAdd(&hist[gray_px(load_px(src + (size_t)p * 3))], 1);
    __syncthreads();
    hists[(size_t)blockIdx.x * 256 + threadIdx.x] = hist[threadIdx.x];
}

// luts: [N][256] bytes
__global__ __launch_bounds__(DF_THREADS) void luma_lut_kernel(const int* __restrict__ hists, int HW, int chunks, unsigned char* __restrict__ luts) {
#pragma clang fp contract(off)
    __shared__ int scan[256];
    __shared__ int first;
    const int n = blockIdx.x, tid = threadIdx.x;
    int h = 0;
    for (int c = 0; c < chunks; ++c) h += hists[((size_t)n * chunks + c) * 256 + tid];
    if (tid == 0) first = 256;
    __syncthreads();
    if (h != 0) atomicMin(&first, tid);
    scan[tid] = h;
    __syncthreads();
    const int i0 = first;
    const int h0 = scan[i0];  // HW >= 1: some bin is not empty
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // inclusive prefix sum
        const int add = tid >= o ? scan[tid - o] : 0;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    int v = tid;  // a constant plane stays as it is
    if (h0 != HW) {
        const float scale = __fdiv_rn(255.0f, (float)(HW - h0));
        v = tid <= i0 ? 0 : (int)fminf(fmaxf(__builtin_rintf((float)(scan[tid] - h0) * scale), 0.f), 255.f);
    }
    luts[(size_t)n * 256 + tid] = (unsigned char)v;
}

__global__ __launch_bounds__(DF_THREADS) void luma_apply_kernel(const unsigned char* __restrict__ img, int HW, int groups,
                                                                const unsigned char* __restrict__ luts, unsigned char* __restrict__ out) {
    __shared__ unsigned char lut[256];
    const int n = blockIdx.x / groups, grp = blockIdx.x - n * groups;
    lut[threadIdx.x] = luts[(size_t)n * 256 + threadIdx.x];
    __syncthreads();
    const int p0 = (grp * DF_THREADS + threadIdx.x) * 4;
    if (p0 >= HW) return;
    const int cnt = min(4, HW - p0);
    const unsigned char* src = img + ((size_t)n * HW + p0) * 3;
    unsigned px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < cnt) {
            int Y, U, V;
            yuv_px(load_px(src + 3 * k), Y, U, V);
            px[k] = rgb_of_yuv(lut[Y], U, V);
        }
    store_px4(out + ((size_t)n * HW + p0) * 3, px, cnt);
}

static int df_chunks(int HW) { return min(cdiv(HW, DF_CHUNK), DF_MAX_CHUNKS); }

// 0 = fine, else the error code (message set); *groups = workgroups of four pixels a thread per image
static int df_shape(const char* who, int N, int H, int W, int* groups) {
    const int rc = check_extent(who, N, H, W);
    if (rc != MSTG_OK) return rc;
    *groups = cdiv(H * W, 4 * DF_THREADS);
    return check_grid(who, (long long)N * *groups, 31, "N * groups of 1024 pixels", (long long)N * *groups);
}

}  // namespace mstg

using namespace mstg;

extern "C" int mstg_gamma_u8(const void* y, int is_half, int N, int H, int W, double gamma, unsigned char* out, void* stream) {
    if (!y || !out) return fail_arg(MSTG_E_BADARG, "gamma_u8: null input or output pointer");
    int groups;
    const int rc = df_shape("gamma_u8", N, H, W, &groups);
    if (rc != MSTG_OK) return rc;
    if (!(gamma > 0.0) || !(gamma <= 16.0)) {
        char msg[120];
        snprintf(msg, sizeof(msg), "gamma_u8: gamma = %g is outside (0, 16]", gamma);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    if ((uintptr_t)y & (is_half ? 1 : 3)) return fail_arg(MSTG_E_ALIGN, "gamma_u8: input not aligned to its element");
    const size_t in_bytes = (size_t)N * 3 * H * W * (is_half ? 2 : 4), out_bytes = (size_t)N * H * W * 3;
    if (overlaps(y, in_bytes, out, out_bytes)) return fail_arg(MSTG_E_BADARG, "gamma_u8: out overlaps the input");
    const dim3 grid((unsigned)(N * groups));
    if (is_half)
        MSTG_LAUNCH(gamma_u8_kernel<__half>, grid, dim3(DF_THREADS), 0, (hipStream_t)stream, (const __half*)y, H * W, groups, gamma, out);
    else
        MSTG_LAUNCH(gamma_u8_kernel<float>, grid, dim3(DF_THREADS), 0, (hipStream_t)stream, (const float*)y, H * W, groups, gamma, out);
    MSTG_CHECK_LAUNCH("gamma_u8_kernel");
    return MSTG_OK;
}

extern "C" size_t mstg_equalize_luma_workspace_bytes(int N, int H, int W) {
    int groups;
    if (df_shape("equalize_luma_workspace_bytes", N, H, W, &groups) != MSTG_OK) return 0;
    return (size_t)N * df_chunks(H * W) * 256 * sizeof(int) + (size_t)N * 256;
}

extern "C" int mstg_equalize_luma_u8(const unsigned char* in, int N, int H, int W, unsigned char* out, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    if (!in || !out) return fail_arg(MSTG_E_BADARG, "equalize_luma_u8: null image or output pointer");
    int groups;
    const int rc = df_shape("equalize_luma_u8", N, H, W, &groups);
    if (rc != MSTG_OK) return rc;
    const int HW = H * W, chunks = df_chunks(HW);
    const size_t hist_bytes = (size_t)N * chunks * 256 * sizeof(int), need = hist_bytes + (size_t)N * 256;
    if (!workspace || workspace_bytes < need) {
        char msg[160];
        snprintf(msg, sizeof(msg), "equalize_luma_u8: workspace of %zu bytes, need %zu", workspace ? workspace_bytes : (size_t)0, need);
        return fail_arg(MSTG_E_WORKSPACE, msg);
    }
    if (!aligned4(workspace)) return fail_arg(MSTG_E_ALIGN, "equalize_luma_u8: workspace not 4-byte aligned");
    const size_t img_bytes = (size_t)N * HW * 3;
    if (overlaps(in, img_bytes, out, img_bytes) || overlaps(in, img_bytes, workspace, need) || overlaps(out, img_bytes, workspace, need))
        return fail_arg(MSTG_E_BADARG, "equalize_luma_u8: out or the workspace overlaps another buffer");
    if ((long long)N * chunks >= (1ll << 31)) return check_grid("equalize_luma_u8", (long long)N * chunks, 31, "N * chunks", (long long)N * chunks);
    hipStream_t st = (hipStream_t)stream;
    int* hists = (int*)workspace;
    unsigned char* luts = (unsigned char*)workspace + hist_bytes;
    const int chunk_px = cdiv(cdiv(HW, chunks), DF_THREADS) * DF_THREADS;
    MSTG_LAUNCH(luma_hist_kernel, dim3((unsigned)(N * chunks)), dim3(DF_THREADS), 0, st, in, HW, chunks, chunk_px, hists);
    MSTG_CHECK_LAUNCH("luma_hist_kernel");
    MSTG_LAUNCH(luma_lut_kernel, dim3((unsigned)N), dim3(DF_THREADS), 0, st, (const int*)hists, HW, chunks, luts);
    MSTG_CHECK_LAUNCH("luma_lut_kernel");
    MSTG_LAUNCH(luma_apply_kernel, dim3((unsigned)(N * groups)), dim3(DF_THREADS), 0, st, in, HW, groups, (const unsigned char*)luts, out);
    MSTG_CHECK_LAUNCH("luma_apply_kernel");
    return MSTG_OK;
}
