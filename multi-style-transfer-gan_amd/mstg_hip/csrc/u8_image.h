// Device and host helpers shared by the 8-bit image filters (local_style.hip, standard_mode.hip, app_local_style.hip,
// color_blocks.hip, segment_style.hip, advanced_transform.hip, slic.hip, quickshift.hip).  Every device helper is a bit-exact restatement of an OpenCV / numpy
// definition; a primitive that more than one of those files uses is defined HERE, once, so that a fix reaches every user (DESIGN.md,
// "Shared 8-bit image helpers").  All __forceinline__: a kernel compiles to the code it had with the body written out in place.
#pragma once
#include "common.h"

namespace mstg {

// ---- device side ----------------------------------------------------------------------------------------------------------------
// cv2.BORDER_REFLECT_101 (d c b | a b c d | c b a), for any distance from the array; n == 1 gives 0
__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

// one pixel of an interleaved 3-channel image as a packed word: channel ch in bits 8 ch .. 8 ch + 7
__device__ __forceinline__ unsigned load_px(const unsigned char* p) { return (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16; }

// four pixels (packed words, 24 bits each) -> the 12 bytes at p; n = how many of the four exist
__device__ __forceinline__ void store_px4(unsigned char* p, const unsigned* v, int n) {
    if (n >= 4 && ((uintptr_t)p & 3) == 0) {
        unsigned* q = reinterpret_cast<unsigned*>(p);
        q[0] = v[0] | v[1] << 24;
        q[1] = v[1] >> 8 | v[2] << 16;
        q[2] = v[2] >> 16 | v[3] << 8;
        return;
    }
    for (int k = 0; k < 4; ++k)
        if (k < n) {
            p[3 * k] = (unsigned char)(v[k] & 0xffu);
            p[3 * k + 1] = (unsigned char)((v[k] >> 8) & 0xffu);
            p[3 * k + 2] = (unsigned char)((v[k] >> 16) & 0xffu);
        }
}

// One byte of a * wa + b * wb as numpy forms it on float64 arrays and as blend_u8_kernel (image.hip) restates it: two rounded
// products, one rounded sum, clip to [0, 255], truncate (astype(uint8)).
__device__ __forceinline__ unsigned blend_byte(unsigned a, unsigned b, double wa, double wb) {
#pragma clang fp contract(off)  // numpy rounds each product and the sum (the pragma is lexical: it does not follow an inlined call)
    const double x = (double)a * wa;
    const double y = (double)b * wb;
    double r = x + y;
    r = r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r);
    if (!(r == r)) r = 0.0;  // a NaN weight: keep the byte defined, as blend_u8_kernel does
    return (unsigned)(unsigned char)r;
}

// One tap of cv2.bilateralFilter on 8-bit, 3-channel pixels (packed words): q = the neighbour, ctr = the centre, sp = the space
// weight of the tap, color = the colour weights in LDS.  float32; the definition rounds the weight product, the three channel
// sums go through __fmaf_rn (the only fused operations).
__device__ __forceinline__ void bilateral_tap(unsigned q, unsigned ctr, float sp, const float* color, float& wsum, float& s0, float& s1,
                                              float& s2) {
#pragma clang fp contract(off)
    const unsigned t = __builtin_amdgcn_sad_u8(q, ctr, 0u);  // |b - b0| + |g - g0| + |r - r0| <= 765
    const float w = sp * color[t];
    wsum += w;
    s0 = __fmaf_rn((float)(q & 0xffu), w, s0);
    s1 = __fmaf_rn((float)((q >> 8) & 0xffu), w, s1);
    s2 = __fmaf_rn((float)((q >> 16) & 0xffu), w, s2);
}

// The tail of cv2.bilateralFilter: one IEEE division 1 / wsum, the three products, round half to even, saturate.
__device__ __forceinline__ void bilateral_bytes(float wsum, float s0, float s1, float s2, unsigned& b0, unsigned& b1, unsigned& b2) {
#pragma clang fp contract(off)
    const float inv = __fdiv_rn(1.0f, wsum);  // wsum >= 1: the centre tap weighs 1
    b0 = (unsigned)fminf(fmaxf(__builtin_rintf(s0 * inv), 0.f), 255.f);
    b1 = (unsigned)fminf(fmaxf(__builtin_rintf(s1 * inv), 0.f), 255.f);
    b2 = (unsigned)fminf(fmaxf(__builtin_rintf(s2 * inv), 0.f), 255.f);
}

// OpenCV's table for getGaussianKernel(KSIZE, sigma <= 0) in 8.8 fixed point, as its bit-exact 8-bit GaussianBlur uses it; every
// row sums to 256.  Sizes 3, 5, 7 ({0.25, 0.5, 0.25}, {0.0625, 0.25, 0.375, ...}, {0.03125, 0.109375, 0.21875, 0.28125, ...}) are
// exact; 15 comes from OpenCV's softfloat generator with error diffusion (include/mstg_hip.h).  The row pass (exact 16-bit sums) and
// the column pass ((sum + 32768) >> 16) that loop over these taps stay in their kernels: a loop inside a shared function is
// unrolled before the function is inlined, and the kernels then compile to other code than with the loop in place.
template <int KSIZE>
__device__ __forceinline__ int gauss_q8_tap(int k) {
    static_assert(KSIZE == 3 || KSIZE == 5 || KSIZE == 7 || KSIZE == 15, "the sizes whose 8.8 taps are restated");
    constexpr int t[4][15] = {{64, 128, 64}, {16, 64, 96, 64, 16}, {8, 28, 56, 72, 56, 28, 8},
                              {1, 3, 6, 12, 20, 30, 36, 40, 36, 30, 20, 12, 6, 3, 1}};
    return t[KSIZE == 15 ? 3 : KSIZE / 2 - 1][k];
}

// Workgroup -> (image, first row, first column of its TH x TW tile); the grid is N * tiles workgroups, tiles_x of them per tile row.
struct TileOrigin {
    int n, y0, x0;
};
template <int TH, int TW>
__device__ __forceinline__ TileOrigin tile_of(int tiles, int tiles_x) {
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    return {n, ty * TH, tx * TW};
}

// The colour step's table (three runs of 256 bytes, one per channel) into LDS; the caller places the barrier.
template <int THREADS>
__device__ __forceinline__ void stage_lut768(const unsigned char* __restrict__ lut, unsigned char* slut, int tid) {
    for (int e = tid; e < 768; e += THREADS) slut[e] = lut[e];
}

// ---- shared by the kernels of segment_style.hip ------------------------------------------------------------------------------------
// round-half-even(num / i) in integers, 0 for i == 0: OpenCV's cvRound of the divisor tables (sdiv: num = 255 << 12, hdiv: 122880)
__device__ __forceinline__ int div_rhe(int num, int i) {
    if (i == 0) return 0;
    const int q = num / i, r = num - q * i;
    return q + ((2 * r > i || (2 * r == i && (q & 1))) ? 1 : 0);
}

// the 8-bit COLOR_RGB2GRAY of a packed pixel
__device__ __forceinline__ int gray_px(unsigned q) {
    return (int)((q & 0xffu) * 4899u + ((q >> 8) & 0xffu) * 9617u + (q >> 16) * 1868u + 8192u) >> 14;
}

// the 8-bit COLOR_RGB2HSV of a packed pixel (include/mstg_hip.h); sdiv, hdiv = the two divisor tables (hdiv may be null: h = 0)
__device__ __forceinline__ void hsv_px(unsigned q, const int* sdiv, const int* hdiv, int& h, int& s, int& v) {
    const int R = q & 0xff, G = (q >> 8) & 0xff, B = q >> 16;
    v = max(R, max(G, B));
    const int diff = v - min(R, min(G, B));
    s = (diff * sdiv[v] + 2048) >> 12;
    h = 0;
    if (hdiv) {
        const int h0 = v == R ? G - B : (v == G ? B - R + 2 * diff : R - G + 4 * diff);
        h = (h0 * hdiv[diff] + 2048) >> 12;  // arithmetic shift of the signed product
        if (h < 0) h += 180;
    }
}

// scipy.ndimage 'reflect' (d c b a | a b c d | d c b a), for any distance from the array
__device__ __forceinline__ int reflect_sym(int i, int n) {
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

// ---- shared by segment_style.hip and advanced_transform.hip: CLAHE(2.0, 8 x 8) and the 8-bit COLOR_HSV2RGB -------------------------
// The tail of a CLAHE tile's table after its 256-bin histogram is filled (a workgroup of 256 threads, thread = bin; the caller has
// zeroed *excess and placed a barrier after the fill): clip, redistribution, inclusive prefix sum, lut[tid] (include/mstg_hip.h).
__device__ __forceinline__ void clahe_tile_lut(int tid, int area, int* hist, int* scan, int* excess, unsigned char* lut) {
#pragma clang fp contract(off)
    const int clip = max((int)(2.0 * (double)area / 256.0), 1);
    int h = hist[tid];
    if (h > clip) {
        atomicAdd(excess, h - clip);
        h = clip;
    }
    __syncthreads();
    const int ex = *excess, batch = ex / 256;
    int residual = ex - batch * 256;
    h += batch;
    if (residual != 0) {
        const int step = max(256 / residual, 1);
        if (tid % step == 0 && tid / step < residual) ++h;
    }
    scan[tid] = h;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // inclusive prefix sum
        const int add = tid >= o ? scan[tid - o] : 0;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    const float scale = __fdiv_rn(255.0f, (float)area);
    const float f = __builtin_rintf((float)scan[tid] * scale);
    lut[tid] = (unsigned char)fminf(fmaxf(f, 0.f), 255.f);
}

// one axis of the interpolation: the two tiles and the two float32 weights
__device__ __forceinline__ void clahe_axis(int p, float inv, int& t1, int& t2, float& a, float& a1) {
#pragma clang fp contract(off)
    const float tf = (float)p * inv - 0.5f;
    const float fl = floorf(tf);
    t1 = (int)fl;
    t2 = t1 + 1;
    a = tf - fl;
    a1 = 1.0f - a;
    t1 = max(t1, 0);
    t2 = min(t2, MSTG_CLAHE_TILES - 1);
}

__device__ __forceinline__ int clahe_px(const unsigned char* luts_img, int v, int y, int x, float inv_th, float inv_tw) {
#pragma clang fp contract(off)
    int tx1, tx2, ty1, ty2;
    float xa, xa1, ya, ya1;
    clahe_axis(x, inv_tw, tx1, tx2, xa, xa1);
    clahe_axis(y, inv_th, ty1, ty2, ya, ya1);
    const float l11 = (float)luts_img[(ty1 * MSTG_CLAHE_TILES + tx1) * 256 + v], l12 = (float)luts_img[(ty1 * MSTG_CLAHE_TILES + tx2) * 256 + v];
    const float l21 = (float)luts_img[(ty2 * MSTG_CLAHE_TILES + tx1) * 256 + v], l22 = (float)luts_img[(ty2 * MSTG_CLAHE_TILES + tx2) * 256 + v];
    const float p0 = l11 * xa1, p1 = l12 * xa, p2 = l21 * xa1, p3 = l22 * xa;
    const float top = (p0 + p1) * ya1, bot = (p2 + p3) * ya;
    const float res = top + bot;
    return (int)fminf(fmaxf(__builtin_rintf(res), 0.f), 255.f);
}

// 8-bit COLOR_HSV2RGB, OpenCV's float path: float32, every operation rounded
__device__ __forceinline__ unsigned hsv2rgb_px(int h, int s, int v) {
#pragma clang fp contract(off)
    constexpr float k255 = 1.f / 255.f, hscale = 6.f / 180.f;
    float hf = (float)h;
    const float sf = (float)s * k255, vf = (float)v * k255;
    float b, g, r;
    if (sf == 0.f) {
        b = g = r = vf;
    } else {
        hf = hf * hscale;
        const float fl = floorf(hf);
        int sector = (int)fl;
        hf = hf - fl;
        if ((unsigned)sector >= 6u) {
            sector = 0;
            hf = 0.f;
        }
        float tab[4];
        tab[0] = vf;
        tab[1] = vf * (1.f - sf);
        const float sh = sf * hf;
        tab[2] = vf * (1.f - sh);
        const float sh1 = sf * (1.f - hf);
        tab[3] = vf * (1.f - sh1);
        // (b, g, r) = tab[idx[sector]] with idx = {{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}}, packed two bits each
        const unsigned bi = (0x835u >> (2 * sector)) & 3u, gi = (0x583u >> (2 * sector)) & 3u, ri = (0x358u >> (2 * sector)) & 3u;
        b = tab[bi];
        g = tab[gi];
        r = tab[ri];
    }
    const unsigned rb = (unsigned)fminf(fmaxf(__builtin_rintf(r * 255.f), 0.f), 255.f);
    const unsigned gb = (unsigned)fminf(fmaxf(__builtin_rintf(g * 255.f), 0.f), 255.f);
    const unsigned bb = (unsigned)fminf(fmaxf(__builtin_rintf(b * 255.f), 0.f), 255.f);
    return rb | gb << 8 | bb << 16;
}

// cv2.multiply(plane, gain) on a byte as the colour steps define it: min(rint((float)v * gain), 255) in float32
__device__ __forceinline__ int gain_u8(int v, float gain) {
#pragma clang fp contract(off)
    return (int)fminf(fmaxf(__builtin_rintf((float)v * gain), 0.f), 255.f);
}

// ---- shared by advanced_transform.hip and quickshift.hip: the 8-bit COLOR_RGB2LAB ------------------------------------------------
constexpr int LT_GAMMA = 256, LT_CBRT = 3072, LT_COEF = LT_GAMMA + LT_CBRT;  // the forward table (mstg_lab_tables)
// RGB (packed) -> L, a, b (packed): the integer path of mstg_color_block_mask completed with L
__device__ __forceinline__ unsigned lab_px(unsigned q, const unsigned short* __restrict__ t) {
    const int R = t[q & 0xffu], G = t[(q >> 8) & 0xffu], B = t[q >> 16];
    const unsigned short* cbr = t + LT_GAMMA;
    const unsigned short* c = t + LT_COEF;
    const int fx = cbr[(R * c[0] + G * c[1] + B * c[2] + 2048) >> 12];
    const int fy = cbr[(R * c[3] + G * c[4] + B * c[5] + 2048) >> 12];
    const int fz = cbr[(R * c[6] + G * c[7] + B * c[8] + 2048) >> 12];
    const int L = (296 * fy - 1336934 + 16384) >> 15;  // arithmetic shifts of the signed sums
    const int a = (500 * (fx - fy) + 128 * 32768 + 16384) >> 15;
    const int b = (200 * (fy - fz) + 128 * 32768 + 16384) >> 15;
    // The compiler packs the two saturated shifts of L and a with v_ashr_pk_u8_i32, which writes 16 bits and LEAVES the upper half
    // of its destination as it was, and then ors b in as if that half were zero: in quickshift.hip's staging the destination was the
    // register of the unshifted L, whose upper half ended up in b (measured on an MI355X: densities equal to a restatement with
    // exactly that word).  The empty asm hides the value from the compiler, so the mask that follows is really executed.
    unsigned la = (unsigned)min(max(L, 0), 255) | (unsigned)min(max(a, 0), 255) << 8;
    asm("" : "+v"(la));
    return (la & 0xffffu) | (unsigned)min(max(b, 0), 255) << 16;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
inline bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}
inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

// (N, H, W) of a batch of 8-bit images and the launch limit; 0 = fine, else the error code (message set).  blocks = workgroups of
// the finest grid that any kernel of the entry launches; it must stay below 2^limit_bits.  grid_what / grid_count = how the
// message names that grid.  The caller forms blocks only after check_extent passed (H * W * 3 < 2^31: no overflow in it).
inline int check_extent(const char* who, int N, int H, int W) {
    char msg[200];
    if (N < 1 || H < 1 || W < 1) {
        snprintf(msg, sizeof(msg), "%s: N = %d, H = %d, W = %d: need at least one image of at least one pixel", who, N, H, W);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    if ((long long)H * W * 3 >= (1ll << 31)) {
        snprintf(msg, sizeof(msg), "%s: H * W * 3 = %lld does not fit 31 bits", who, (long long)H * W * 3);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    return MSTG_OK;
}
inline int check_grid(const char* who, long long blocks, int limit_bits, const char* grid_what, long long grid_count) {
    if (blocks < (1ll << limit_bits)) return MSTG_OK;
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: %s = %lld, more than 2^%d - 1 workgroups in one launch", who, grid_what, grid_count, limit_bits);
    return fail_arg(MSTG_E_UNSUPPORTED, msg);
}
// the shape check of the files whose finest tiling is 16 x 64 pixels a workgroup (a point-wise grid is coarser)
inline int check_shape_16x64(const char* who, int N, int H, int W) {
    const int rc = check_extent(who, N, H, W);
    if (rc != MSTG_OK) return rc;
    const long long blocks = (long long)N * cdiv(H, 16) * cdiv(W, 64);
    return check_grid(who, blocks, 24, "N * tiles", blocks);
}

// ---- shared by slic.hip and quickshift.hip (defined in slic.hip): the tail of a segmentation whose pixels point at an owner ------------
// jump (N, H, W): per pixel an index inside its image; an owner points at itself, and following the pointers from any pixel ends
// at an owner after fewer than H * W links.  cc_resolve_number launches cc_rounds(H * W) rounds of pointer jumping in place, then
// numbers the owners first, first + 1, ... in ascending index: out (N, H, W) = the number of each pixel's owner, count (N) = the
// owners.  num: N * H * W ints, bsum: N * cc_blocks(H * W) ints of workspace.  cc_rounds(H * W) + 4 launches whatever N.
constexpr int CC_BLOCK = 1024;  // pixels per workgroup of the numbering: four per thread
inline int cc_blocks(size_t hw) { return (int)((hw + CC_BLOCK - 1) / CC_BLOCK); }
int cc_rounds(size_t hw);
int cc_resolve_number(int* jump, int N, int H, int W, int first, int* num, int* bsum, int* out, int* count, hipStream_t st);

// cv2.Canny's hysteresis (local_style_hysteresis_kernel) keeps one byte per pixel of an image in LDS; extra = words for the
// message between "pixels; " and "the hysteresis" (with their trailing blank), or "".
inline int fits_hysteresis_lds(const char* who, int H, int W, const char* extra) {
    if ((long long)H * W <= MSTG_LOCAL_STYLE_MAX_PIXELS) return MSTG_OK;
    char msg[220];
    snprintf(msg, sizeof(msg), "%s: a %d x %d image has %lld pixels; %sthe hysteresis keeps one byte per pixel in LDS and takes at most %d", who,
             H, W, (long long)H * W, extra, MSTG_LOCAL_STYLE_MAX_PIXELS);
    return fail_arg(MSTG_E_UNSUPPORTED, msg);
}

}  // namespace mstg
