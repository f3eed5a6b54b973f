// SLIC superpixels (the `slic` method of the reference's get_segmentation_mask, enhanced_local_style.py:65-66) on the device, for a
// batch of (N, H, W, 3) uint8 canvases, as include/mstg_hip.h defines it: the 8-bit Lab features, the grid of centres, ten rounds of
// assignment and update, and this build's own connectivity step.  tests/slic_ref.py is the same definition in numpy; neither has
// been compared with a scikit-image binary.  Every kernel takes N images per launch, offsets are 64-bit, the number of launches
// depends on H * W alone (the rounds of the pointer doubling), never on N or on the data:
//
// L  mstg_lab_u8 (advanced_transform.hip)  the Lab bytes, once.
// I  slic_init_kernel      one thread per (image, centre): the centre's pixel, its Lab; clears the sums.
// A  slic_assign_kernel    the hot one, once per round.  One workgroup of 256 threads per 16 x 64 tile, a thread four neighbouring
//    pixels of a row.  The centres are taken 256 at a time: a thread tests one centre's window against the tile, and the ones that
//    meet it go to LDS IN ASCENDING k by an ordered compaction (a ballot per wave, the waves' counts through LDS) -- an atomic
//    append would lose the order that the tie rule needs.  Every thread then walks that list for its four pixels (all lanes read
//    the same entry: the LDS reads broadcast), strict `<`, so among equal distances the lowest k stays.  The six integer sums of a
//    pixel (n, y, x, L, a, b) go to its centre: (1) a thread keeps a run of equal labels in registers; (2) where every lane of a
//    wave ends with one run of one label the wave adds its lanes up with cross-lane moves; (3) the workgroup keeps SL_SLOTS label
//    slots in LDS (open addressing, 32-bit LDS atomics: a tile has 1024 pixels and y, x < 2^20) and writes every used slot once,
//    with 64-bit integer global atomics; what does not fit a slot goes straight to the global sums.
//    The global sums are 64 bits: n <= H * W <= 2^20 and L, a, b <= 255 would fit 32, but sum y < n * H fits 32 bits only while
//    H <= 2^12, and a strip of 65536 x 16 pixels with a centre that owns a long run of it is inside what is built.
// F  slic_final_kernel     one thread per (image, centre): (float)((double)sum / (double)n) into the other centre buffer, clears the sums.
// C  the connectivity: cc_init_kernel (a pixel starts below the first pixel of its row's run as far as the run lies in its wave: a
//    ballot, no atomic; sizes 0), cc_merge_kernel (union-find: a pixel joins the tree of its lower neighbour of equal label unless
//    their left neighbours already imply it, and a run that crosses a wave is joined there; integer atomicMin on the parent of
//    the larger root, so a root is the smallest raster index of its tree), cc_flatten_kernel, cc_size_kernel (integer atomics, one
//    per distinct root of a wave), cc_link_kernel (a small component points at the component of the pixel before its root,
//    everything else at its root), cc_jump_kernel x R (pointer jumping, a thread follows CC_HOPS = 16 pointers per launch, so the
//    shortest pointer grows 16-fold: R = ceil(log16(H * W)); a chain of small components is up to H * W - 1 links long and a
//    per-thread walk to its end would not finish in time; in place: a pointer only ever moves along its chain and stops at its end,
//    so reading a neighbour's newer value only shortens the work), then the numbering: cc_count_kernel (owners per block of 1024 pixels), cc_scan_kernel (one
//    workgroup per image: the blocks' offsets and the count), cc_number_kernel (the owners' numbers), cc_gather_kernel.
//    Every loop of the union-find is capped by H * W (a parent is always a smaller index, so no path is longer).
//    The pointer jumping and the numbering are cc_resolve_number (declared in u8_image.h): quickshift.hip ends with the same tail,
//    its roots numbered from 0.
//
// No floating-point atomics; all sums are integers, so the result does not depend on the order: bit-reproducible, independent of N.
#include <cmath>

#include "u8_image.h"

namespace mstg {

constexpr int SL_THREADS = 256;
constexpr int SL_TH = 16, SL_TW = 64, SL_PX = 4;  // tile of the assignment; pixels of a row per thread
constexpr int SL_CHUNK = SL_THREADS;              // centres tested per pass: one per thread
constexpr int SL_SLOTS = 64;                      // label slots of a workgroup in LDS
constexpr int SL_F = MSTG_SLIC_SUMS;              // n, y, x, L, a, b
constexpr int SL_C = 5;                           // floats of a centre: y, x, L, a, b
constexpr int SL_ROUNDS = 10;
constexpr int CC_HOPS = 16;                       // pointers a thread follows per launch of the pointer jumping
static_assert(SL_TH * SL_TW == SL_THREADS * SL_PX && SL_TW / SL_PX == 16, "four pixels per thread, sixteen threads per row");
static_assert((SL_SLOTS & (SL_SLOTS - 1)) == 0 && SL_F == 6, "the hash takes the top bits");

typedef unsigned long long u64;

struct SlicCentre {  // 32 bytes: two 16-byte LDS reads
    float y, x, L, a, b;
    int iy, ix, k;
};

// ---- I, A, F: assignment and update --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SL_THREADS) void slic_init_kernel(const unsigned char* __restrict__ lab, int H, int W, int K, int nx, int step,
                                                               int start, size_t total, float* __restrict__ cen, u64* __restrict__ sums) {
    const size_t idx = (size_t)blockIdx.x * SL_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t n = idx / K;
    const int k = (int)(idx - n * K), i = k / nx, j = k - i * nx;
    const int cy = start + i * step, cx = start + j * step;  // inside the image: the host counted ny and nx so
    const unsigned q = load_px(lab + (n * H * W + (size_t)cy * W + cx) * 3);
    float* c = cen + idx * SL_C;
    c[0] = (float)cy;
    c[1] = (float)cx;
    c[2] = (float)(q & 0xffu);
    c[3] = (float)((q >> 8) & 0xffu);
    c[4] = (float)(q >> 16);
    for (int f = 0; f < SL_F; ++f) sums[idx * SL_F + f] = 0;
}

// the slot of `label` in the workgroup's table, -1 when the table is full (the caller then adds to the global sums)
__device__ __forceinline__ int sl_slot(int* keys, int* full, int label) {
    if (*(volatile int*)full) return -1;
    unsigned h = ((unsigned)label * 2654435761u) >> 26;
    for (int i = 0; i < SL_SLOTS; ++i) {
        const int old = atomicCAS(&keys[h], -1, label);
        if (old == -1 || old == label) return (int)h;
        h = (h + 1) & (SL_SLOTS - 1);
    }
    *(volatile int*)full = 1;
    return -1;
}

struct SlicRun {
    int label;
    unsigned f[SL_F];
};

__device__ __forceinline__ void sl_flush(const SlicRun& r, int* keys, int* full, unsigned* vals, u64* gsum) {
    if (r.label < 0) return;
    const int slot = sl_slot(keys, full, r.label);
#pragma unroll
    for (int f = 0; f < SL_F; ++f) {
        if (r.f[f] == 0) continue;
        if (slot >= 0)
            atomicAdd(&vals[slot * SL_F + f], r.f[f]);
        else
            atomicAdd(&gsum[(size_t)r.label * SL_F + f], (u64)r.f[f]);
    }
}

__global__ __launch_bounds__(SL_THREADS) void slic_assign_kernel(const unsigned char* __restrict__ lab, const float* __restrict__ cen, int K, int H,
                                                                 int W, int step, float ws, float wc, float kL, int first, int tiles_x, int tiles,
                                                                 int* __restrict__ labels, u64* __restrict__ sums) {
#pragma clang fp contract(off)  // the definition rounds every operation
    __shared__ SlicCentre list[SL_CHUNK];
    __shared__ int wcount[SL_THREADS / WAVE];
    __shared__ int keys[SL_SLOTS];
    __shared__ unsigned vals[SL_SLOTS * SL_F];
    __shared__ int full;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const auto [n, y0, x0] = tile_of<SL_TH, SL_TW>(tiles, tiles_x);
    const size_t plane = (size_t)n * H * W;
    const unsigned char* img = lab + plane * 3;
    const float* c_img = cen + (size_t)n * K * SL_C;
    int* l_img = labels + plane;
    u64* gsum = sums + (size_t)n * K * SL_F;
    if (tid < SL_SLOTS) keys[tid] = -1;
    if (tid == 0) full = 0;
    for (int e = tid; e < SL_SLOTS * SL_F; e += SL_THREADS) vals[e] = 0;
    const int row = tid >> 4, col = (tid & 15) * SL_PX;
    const int py = y0 + row, px0 = x0 + col;
    const int y1 = min(y0 + SL_TH, H) - 1, x1 = min(x0 + SL_TW, W) - 1;  // the tile's last row and column inside the image
    const int reach = 2 * step;
    unsigned q[SL_PX];
    float best[SL_PX];
    int bk[SL_PX];
    bool ok[SL_PX];
#pragma unroll
    for (int j = 0; j < SL_PX; ++j) {
        ok[j] = py < H && px0 + j < W;
        q[j] = ok[j] ? load_px(img + ((size_t)py * W + px0 + j) * 3) : 0u;
        best[j] = __builtin_inff();
        bk[j] = -1;
    }
    const float fy = (float)py;
    for (int base = 0; base < K; base += SL_CHUNK) {  // K is the host's: at most MSTG_SLIC_MAX_CENTRES / SL_CHUNK passes
        const int k = base + tid;
        SlicCentre c;
        bool meets = false;
        if (k < K) {
            const float* p = c_img + (size_t)k * SL_C;
            c.y = p[0], c.x = p[1], c.L = p[2], c.a = p[3], c.b = p[4];
            c.iy = (int)c.y, c.ix = (int)c.x, c.k = k;
            meets = c.iy - reach <= y1 && c.iy + reach >= y0 && c.ix - reach <= x1 && c.ix + reach >= x0;
        }
        const u64 m = __ballot(meets);
        if (lane == 0) wcount[wave] = __popcll(m);
        __syncthreads();
        int at = __popcll(m & ((1ull << lane) - 1ull)), count = 0;
#pragma unroll
        for (int w = 0; w < SL_THREADS / WAVE; ++w) {
            const int cw = wcount[w];
            if (w < wave) at += cw;
            count += cw;
        }
        if (meets) list[at] = c;  // ascending k: lanes, then waves, then passes
        __syncthreads();
        for (int e = 0; e < count; ++e) {
            const SlicCentre ce = list[e];
            const bool row_in = abs(py - ce.iy) <= reach;
            const float dy = fy - ce.y;
            const float dy2 = dy * dy;
#pragma unroll
            for (int j = 0; j < SL_PX; ++j) {
                const int px = px0 + j;
                const float dx = (float)px - ce.x;
                const float dL = (float)(q[j] & 0xffu) - ce.L, da = (float)((q[j] >> 8) & 0xffu) - ce.a, db = (float)(q[j] >> 16) - ce.b;
                const float sp = (dy2 + dx * dx) * ws;
                const float t = dL * kL;
                const float co = ((t * t + da * da) + db * db) * wc;
                const float d = sp + co;
                if (row_in && abs(px - ce.ix) <= reach && d < best[j]) {
                    best[j] = d;
                    bk[j] = ce.k;
                }
            }
        }
        // the next pass writes wcount before its first barrier and list after it: every thread has read both by then
    }
    SlicRun run;
    run.label = -1;
    bool clean = true;  // one run, four pixels of the image
#pragma unroll
    for (int j = 0; j < SL_PX; ++j) {
        if (!ok[j]) {
            clean = false;
            continue;
        }
        const size_t p = (size_t)py * W + px0 + j;
        int L = bk[j];
        if (L < 0)
            L = first ? 0 : l_img[p];  // no candidate: the pixel keeps its label (0 before the first round)
        else
            l_img[p] = L;
        if (first && bk[j] < 0) l_img[p] = 0;
        if (L != run.label) {
            if (j > 0) clean = false;
            sl_flush(run, keys, &full, vals, gsum);
            run.label = L;
#pragma unroll
            for (int f = 0; f < SL_F; ++f) run.f[f] = 0;
        }
        run.f[0] += 1;
        run.f[1] += (unsigned)py;
        run.f[2] += (unsigned)(px0 + j);
        run.f[3] += q[j] & 0xffu;
        run.f[4] += (q[j] >> 8) & 0xffu;
        run.f[5] += q[j] >> 16;
    }
    // (the slot table was cleared before the barriers of the passes above: K >= 1, so there was at least one)
    const int first_label = __builtin_amdgcn_readfirstlane(run.label);
    if (__all(clean && run.label == first_label)) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int f = 0; f < SL_F; ++f) run.f[f] += __shfl_xor(run.f[f], o, WAVE);  // 256 pixels, y and x below 2^20: 32 bits hold it
        if (lane == 0) sl_flush(run, keys, &full, vals, gsum);
    } else {
        sl_flush(run, keys, &full, vals, gsum);
    }
    __syncthreads();
    for (int e = tid; e < SL_SLOTS * SL_F; e += SL_THREADS) {
        const int slot = e / SL_F, f = e - slot * SL_F;
        const int key = keys[slot];
        const unsigned v = vals[e];
        if (key >= 0 && v != 0) atomicAdd(&gsum[(size_t)key * SL_F + f], (u64)v);
    }
}

__global__ __launch_bounds__(SL_THREADS) void slic_final_kernel(const float* __restrict__ cen, u64* __restrict__ sums, size_t total,
                                                                float* __restrict__ next) {
    const size_t idx = (size_t)blockIdx.x * SL_THREADS + threadIdx.x;
    if (idx >= total) return;
    u64* s = sums + idx * SL_F;
    const u64 n = s[0];
#pragma unroll
    for (int f = 0; f < SL_C; ++f)  // a centre without pixels keeps its values
        next[idx * SL_C + f] = n ? (float)__ddiv_rn((double)s[1 + f], (double)n) : cen[idx * SL_C + f];
#pragma unroll
    for (int f = 0; f < SL_F; ++f) s[f] = 0;
}

// ---- C: connectivity -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int cc_load(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

__device__ __forceinline__ int cc_find(const int* par, int x, int cap) {
    for (int i = 0; i < cap; ++i) {  // a parent is a smaller index: at most cap - 1 steps
        const int p = cc_load(par + x);
        if (p == x) break;
        x = p;
    }
    return x;
}

__device__ __forceinline__ void cc_union(int* par, int a, int b, int cap) {
    for (int i = 0; i < cap; ++i) {  // every retry moves a to a smaller index
        a = cc_find(par, a, cap);
        b = cc_find(par, b, cap);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(par + a, b);  // a was a root: it now hangs below the smaller root
        if (old == a) return;
        a = old;  // another thread linked a first: join what it linked to
    }
}

struct CcPixel {
    size_t n;
    int p;
};
__device__ __forceinline__ CcPixel cc_pixel(size_t idx, size_t hw) {
    const size_t n = idx / hw;
    return {n, (int)(idx - n * hw)};
}

// does pixel p (column x > 0 of its row) continue the run of its left neighbour?
__device__ __forceinline__ bool cc_left_same(const int* l, int p, int x) { return x > 0 && l[p - 1] == l[p]; }

// Every pixel starts below the first pixel of its row's run of equal labels as far as the run lies inside the pixel's wave (the
// lanes of a wave are 64 consecutive pixels): most horizontal joins are made here, without an atomic.
__global__ __launch_bounds__(SL_THREADS) void cc_init_kernel(const int* __restrict__ labels, int W, size_t hw, size_t total, int* __restrict__ par,
                                                             int* __restrict__ size) {
    const size_t idx = (size_t)blockIdx.x * SL_THREADS + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1);
    const bool live = idx < total;
    int p = 0;
    bool starts = true;
    if (live) {
        const CcPixel c = cc_pixel(idx, hw);
        p = c.p;
        starts = !cc_left_same(labels + c.n * hw, p, p % W);
    }
    const u64 upto = __ballot(starts) & ((2ull << lane) - 1ull);  // the starts at or before this lane
    const int first = upto ? 63 - __clzll((long long)upto) : 0;   // none: the run comes in from the wave before, lane 0 leads here
    if (!live) return;
    par[idx] = p - (lane - first);
    size[idx] = 0;
}

__global__ __launch_bounds__(SL_THREADS) void cc_merge_kernel(const int* __restrict__ labels, int H, int W, size_t total, int* __restrict__ par) {
    const size_t idx = (size_t)blockIdx.x * SL_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t hw = (size_t)H * W;
    const auto [n, p] = cc_pixel(idx, hw);
    const int* l = labels + n * hw;
    int* pr = par + n * hw;
    const int y = p / W, x = p - y * W, v = l[p];
    const bool left = cc_left_same(l, p, x);
    // cc_init_kernel joined a run inside a wave; a run that comes in from the wave before is joined to it here
    if (left && (threadIdx.x & (WAVE - 1)) == 0) cc_union(pr, p, p - 1, (int)hw);
    // the join with the pixel below is implied where the left neighbours are joined to both and to each other
    if (y + 1 < H && l[p + W] == v && !(left && l[p + W - 1] == v)) cc_union(pr, p, p + W, (int)hw);
}

__global__ __launch_bounds__(SL_THREADS) void cc_flatten_kernel(size_t hw, size_t total, int* __restrict__ par) {
    const size_t idx = (size_t)blockIdx.x * SL_THREADS + threadIdx.x;
    if (idx >= total) return;
    const auto [n, p] = cc_pixel(idx, hw);
    int* pr = par + n * hw;
    const int r = cc_find(pr, p, (int)hw);
    if (r != p) __atomic_store_n(pr + p, r, __ATOMIC_RELAXED);  // a root is never written: a concurrent find still ends at it
}

__global__ __launch_bounds__(SL_THREADS) void cc_size_kernel(size_t hw, size_t total, const int* __restrict__ par, int* __restrict__ size) {
    const size_t idx = (size_t)blockIdx.x * SL_THREADS + threadIdx.x;
    const bool live = idx < total;
    size_t at = 0;
    if (live) at = cc_pixel(idx, hw).n * hw + par[idx];
    bool todo = live;
    for (int i = 0; i < WAVE; ++i) {  // one addition per distinct root of the wave: at most 64 passes, one or two inside a component
        const u64 m = __ballot(todo);
        if (m == 0) break;
        const int leader = __ffsll((long long)m) - 1;
        const size_t lead = ((size_t)__shfl((int)(at >> 32), leader, WAVE) << 32) | (unsigned)__shfl((int)at, leader, WAVE);
        const bool mine = todo && at == lead;
        const int cnt = __popcll(__ballot(mine));
        if (mine && (int)(threadIdx.x & (WAVE - 1)) == leader) atomicAdd(size + at, cnt);
        if (mine) todo = false;
    }
}

// jump[p]: a root that is small -> the root of the pixel before it; any other root -> itself; any other pixel -> its root
__global__ __launch_bounds__(SL_THREADS) void cc_link_kernel(int W, size_t hw, size_t total, int min_size, const int* __restrict__ par,
                                                             const int* __restrict__ size, int* __restrict__ jump) {
    const size_t idx = (size_t)blockIdx.x * SL_THREADS + threadIdx.x;
    if (idx >= total) return;
    const auto [n, p] = cc_pixel(idx, hw);
    const int r = par[idx];
    int to = r;
    if (r == p && p > 0 && size[idx] < min_size) to = par[n * hw + (p % W == 0 ? p - W : p - 1)];  // p > 0 and p % W == 0: p >= W
    jump[idx] = to;
}

__global__ __launch_bounds__(SL_THREADS) void cc_jump_kernel(size_t hw, size_t total, int* __restrict__ jump) {
    const size_t idx = (size_t)blockIdx.x * SL_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int* img = jump + cc_pixel(idx, hw).n * hw;
    const int j0 = cc_load(jump + idx);
    int j = j0;
    for (int s = 1; s < CC_HOPS; ++s) {  // CC_HOPS pointers in a row, each at least as long as any was before this launch
        const int jj = cc_load(img + j);
        if (jj == j) break;
        j = jj;
    }
    if (j != j0) __atomic_store_n(jump + idx, j, __ATOMIC_RELAXED);
}

// the owners (jump[p] == p) of each block of CC_BLOCK pixels of an image
__global__ __launch_bounds__(SL_THREADS) void cc_count_kernel(size_t hw, int blocks, const int* __restrict__ jump, int* __restrict__ bsum) {
    __shared__ int wsum[SL_THREADS / WAVE];
    const int tid = threadIdx.x;
    const size_t n = blockIdx.x / blocks;
    const int b = blockIdx.x - (int)n * blocks;
    int c = 0;
#pragma unroll
    for (int j = 0; j < CC_BLOCK / SL_THREADS; ++j) {
        const size_t p = (size_t)b * CC_BLOCK + (size_t)tid * (CC_BLOCK / SL_THREADS) + j;
        if (p < hw && jump[n * hw + p] == (int)p) ++c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, WAVE);
    if ((tid & (WAVE - 1)) == 0) wsum[tid / WAVE] = c;
    __syncthreads();
    if (tid == 0) bsum[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// exclusive prefix sum of 256 values, one per thread; *total = their sum.  Two barriers; tmp: SL_THREADS / WAVE + 1 ints of LDS
__device__ __forceinline__ int cc_scan256(int v, int tid, int* tmp, int* total) {
    const int lane = tid & (WAVE - 1), wave = tid / WAVE;
    int inc = v;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int t = __shfl_up(inc, o, WAVE);
        if (lane >= o) inc += t;
    }
    __syncthreads();  // tmp may still be read from the call before
    if (lane == WAVE - 1) tmp[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SL_THREADS / WAVE; ++w) {
        const int t = tmp[w];
        if (w < wave) before += t;
        all += t;
    }
    *total = all;
    return before + inc - v;
}

// one workgroup per image: the blocks' counts become their offsets; count[n] = the number of owners
__global__ __launch_bounds__(SL_THREADS) void cc_scan_kernel(int blocks, int* __restrict__ bsum, int* __restrict__ count) {
    __shared__ int tmp[SL_THREADS / WAVE];
    const int tid = threadIdx.x;
    int* b = bsum + (size_t)blockIdx.x * blocks;
    int carry = 0;
    for (int base = 0; base < blocks; base += SL_THREADS) {  // blocks <= MSTG_SEGMENT_MAX_PIXELS / CC_BLOCK: at most four passes
        const int i = base + tid;
        const int v = i < blocks ? b[i] : 0;
        int all;
        const int ex = cc_scan256(v, tid, tmp, &all);
        if (i < blocks) b[i] = carry + ex;
        carry += all;
    }
    if (tid == 0) count[blockIdx.x] = carry;
}

// num[p] = the number (from `first`, ascending p) of owner p
__global__ __launch_bounds__(SL_THREADS) void cc_number_kernel(size_t hw, int blocks, const int* __restrict__ jump, const int* __restrict__ bsum,
                                                               int first, int* __restrict__ num) {
    __shared__ int tmp[SL_THREADS / WAVE];
    const int tid = threadIdx.x;
    const size_t n = blockIdx.x / blocks;
    const int b = blockIdx.x - (int)n * blocks;
    constexpr int PER = CC_BLOCK / SL_THREADS;
    bool own[PER];
    int c = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const size_t p = (size_t)b * CC_BLOCK + (size_t)tid * PER + j;
        own[j] = p < hw && jump[n * hw + p] == (int)p;
        c += own[j];
    }
    int all;
    int at = first + bsum[blockIdx.x] + cc_scan256(c, tid, tmp, &all);
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const size_t p = (size_t)b * CC_BLOCK + (size_t)tid * PER + j;
        if (own[j]) num[n * hw + p] = at++;
    }
}

__global__ __launch_bounds__(SL_THREADS) void cc_gather_kernel(size_t hw, size_t total, const int* __restrict__ jump, const int* __restrict__ num,
                                                               int* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * SL_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t n = idx / hw;
    out[idx] = num[n * hw + jump[idx]];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static dim3 sl_grid(size_t items) { return dim3((unsigned)cdivz(items, (size_t)SL_THREADS)); }

struct SlicGrid {
    int step, ny, nx, start;
};

// 0 = fine, else the error code (message set)
static int sl_grid_of(const char* who, int H, int W, int n_segments, SlicGrid& g) {
    char msg[240];
    if (H < 1 || W < 1) {
        snprintf(msg, sizeof(msg), "%s: H = %d, W = %d", who, H, W);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    const long long hw = (long long)H * W;
    if (n_segments < 1) {
        snprintf(msg, sizeof(msg), "%s: n_segments = %d: need at least 1", who, n_segments);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    if (hw > MSTG_SEGMENT_MAX_PIXELS) {
        snprintf(msg, sizeof(msg), "%s: H * W = %lld is more than %d", who, hw, MSTG_SEGMENT_MAX_PIXELS);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    if (hw <= n_segments) {
        snprintf(msg, sizeof(msg), "%s: n_segments = %d is not below H * W = %lld", who, n_segments, hw);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    const double s = std::sqrt((double)hw / (double)n_segments);
    g.step = (int)std::nearbyint(s);  // ties to even
    g.start = (int)std::floor(s / 2);
    if (H < g.step || W < g.step) {
        snprintf(msg, sizeof(msg), "%s: H = %d, W = %d with n_segments = %d: a side is smaller than step = %d (scikit-image re-grids there; not built)",
                 who, H, W, n_segments, g.step);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    g.ny = (H - 1 - g.start) / g.step + 1;  // start <= step / 2 < H
    g.nx = (W - 1 - g.start) / g.step + 1;
    if ((long long)g.ny * g.nx > MSTG_SLIC_MAX_CENTRES) {
        snprintf(msg, sizeof(msg), "%s: K = %lld centres (n_segments = %d) is more than %d", who, (long long)g.ny * g.nx, n_segments,
                 MSTG_SLIC_MAX_CENTRES);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    return MSTG_OK;
}

static int sl_batch(const char* who, int N, int H, int W) {
    const int rc = check_extent(who, N, H, W);
    if (rc != MSTG_OK) return rc;
    const long long px = (long long)N * H * W;  // the finest grid: a thread per pixel
    return check_grid(who, (px + SL_THREADS - 1) / SL_THREADS, 31, "N * H * W", px);
}

static int cc_shape(const char* who, int N, int H, int W) {
    const int rc = sl_batch(who, N, H, W);
    if (rc != MSTG_OK) return rc;
    if ((long long)H * W <= MSTG_SEGMENT_MAX_PIXELS) return MSTG_OK;
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: H * W = %lld is more than %d", who, (long long)H * W, MSTG_SEGMENT_MAX_PIXELS);
    return fail_arg(MSTG_E_UNSUPPORTED, msg);
}

// the workspace of the connectivity step: par, size (later num), jump: N * H * W ints each; the blocks' counts
struct CcWorkspace {
    size_t par, size, jump, bsum, total;
    int blocks;
};
static CcWorkspace cc_workspace(int N, int H, int W) {
    const size_t plane = align16((size_t)N * H * W * sizeof(int));
    CcWorkspace w;
    w.blocks = cc_blocks((size_t)H * W);
    w.par = 0;
    w.size = plane;
    w.jump = 2 * plane;
    w.bsum = 3 * plane;
    w.total = w.bsum + align16((size_t)N * w.blocks * sizeof(int));
    return w;
}

// launches of cc_jump_kernel: a path (a pixel, its root, the chain of small components) has fewer than H * W links, and the
// shortest pointer grows CC_HOPS-fold per launch: the smallest r with CC_HOPS^r >= H * W, at least 1
int cc_rounds(size_t hw) {
    int r = 1;
    for (size_t reach = CC_HOPS; reach < hw; reach *= CC_HOPS) ++r;
    return r;
}

int cc_resolve_number(int* jump, int N, int H, int W, int first, int* num, int* bsum, int* out, int* count, hipStream_t st) {
    const size_t hw = (size_t)H * W, px = (size_t)N * hw;
    const int blocks = cc_blocks(hw);
    const int rounds = cc_rounds(hw);
    for (int r = 0; r < rounds; ++r) {
        MSTG_LAUNCH(cc_jump_kernel, sl_grid(px), dim3(SL_THREADS), 0, st, hw, px, jump);
        MSTG_CHECK_LAUNCH("cc_jump_kernel");
    }
    const dim3 per_block((unsigned)((size_t)N * blocks));
    MSTG_LAUNCH(cc_count_kernel, per_block, dim3(SL_THREADS), 0, st, hw, blocks, (const int*)jump, bsum);
    MSTG_CHECK_LAUNCH("cc_count_kernel");
    MSTG_LAUNCH(cc_scan_kernel, dim3((unsigned)N), dim3(SL_THREADS), 0, st, blocks, bsum, count);
    MSTG_CHECK_LAUNCH("cc_scan_kernel");
    MSTG_LAUNCH(cc_number_kernel, per_block, dim3(SL_THREADS), 0, st, hw, blocks, (const int*)jump, (const int*)bsum, first, num);
    MSTG_CHECK_LAUNCH("cc_number_kernel");
    MSTG_LAUNCH(cc_gather_kernel, sl_grid(px), dim3(SL_THREADS), 0, st, hw, px, (const int*)jump, (const int*)num, out);
    MSTG_CHECK_LAUNCH("cc_gather_kernel");
    return MSTG_OK;
}

static int cc_run(const int* labels, int N, int H, int W, int min_size, int* out, int* count, unsigned char* base, hipStream_t st) {
    const CcWorkspace ws = cc_workspace(N, H, W);
    const size_t hw = (size_t)H * W, px = (size_t)N * hw;
    int* par = (int*)(base + ws.par);
    int* size = (int*)(base + ws.size);
    int* jump = (int*)(base + ws.jump);
    int* bsum = (int*)(base + ws.bsum);
    MSTG_LAUNCH(cc_init_kernel, sl_grid(px), dim3(SL_THREADS), 0, st, labels, W, hw, px, par, size);
    MSTG_CHECK_LAUNCH("cc_init_kernel");
    MSTG_LAUNCH(cc_merge_kernel, sl_grid(px), dim3(SL_THREADS), 0, st, labels, H, W, px, par);
    MSTG_CHECK_LAUNCH("cc_merge_kernel");
    MSTG_LAUNCH(cc_flatten_kernel, sl_grid(px), dim3(SL_THREADS), 0, st, hw, px, par);
    MSTG_CHECK_LAUNCH("cc_flatten_kernel");
    MSTG_LAUNCH(cc_size_kernel, sl_grid(px), dim3(SL_THREADS), 0, st, hw, px, (const int*)par, size);
    MSTG_CHECK_LAUNCH("cc_size_kernel");
    MSTG_LAUNCH(cc_link_kernel, sl_grid(px), dim3(SL_THREADS), 0, st, W, hw, px, min_size, (const int*)par, (const int*)size, jump);
    MSTG_CHECK_LAUNCH("cc_link_kernel");
    return cc_resolve_number(jump, N, H, W, 1, size, bsum, out, count, st);  // scikit-image's start_label = 1
}

// the workspace of the assignment: the Lab bytes, two centre buffers, the sums; for mstg_slic_u8 also the raw labels and the
// connectivity step's workspace
struct SlicWorkspace {
    size_t lab, cen_a, cen_b, sums, raw, cc, assign_total, total;
};
static SlicWorkspace sl_workspace(int N, int H, int W, int K) {
    SlicWorkspace w;
    const size_t cen = align16((size_t)N * K * SL_C * sizeof(float));
    w.lab = 0;
    w.cen_a = align16((size_t)N * H * W * 3);
    w.cen_b = w.cen_a + cen;
    w.sums = w.cen_b + cen;
    w.assign_total = w.sums + align16((size_t)N * K * SL_F * sizeof(u64));
    w.raw = w.assign_total;
    w.cc = w.raw + align16((size_t)N * H * W * sizeof(int));
    w.total = w.cc + cc_workspace(N, H, W).total;
    return w;
}

static int sl_shape(const char* who, int N, int H, int W, int n_segments, SlicGrid& g) {
    int rc = sl_grid_of(who, H, W, n_segments, g);
    if (rc == MSTG_OK) rc = sl_batch(who, N, H, W);
    return rc;
}

static int sl_compactness(const char* who, double compactness) {
    if (compactness > 0 && (float)compactness > 0.f && std::isfinite((float)compactness * (float)compactness)) return MSTG_OK;
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: compactness = %g: need a positive value whose square is a finite float32", who, compactness);
    return fail_arg(MSTG_E_UNSUPPORTED, msg);
}

// steps 1 to 3 into `labels` (raw) and `centres` (nullable); base: the workspace, at least assign_total bytes
static int sl_assign(const unsigned char* img, int N, int H, int W, const SlicGrid& g, double compactness, const unsigned short* lab_table,
                     int* labels, float* centres, unsigned char* base, const SlicWorkspace& ws, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int K = g.ny * g.nx;
    unsigned char* lab = base + ws.lab;
    float* cen[2] = {(float*)(base + ws.cen_a), (float*)(base + ws.cen_b)};
    u64* sums = (u64*)(base + ws.sums);
    int rc = mstg_lab_u8(img, N, H, W, lab_table, lab, stream);
    if (rc != MSTG_OK) return rc;
    const size_t nk = (size_t)N * K;
    MSTG_LAUNCH(slic_init_kernel, sl_grid(nk), dim3(SL_THREADS), 0, st, (const unsigned char*)lab, H, W, K, g.nx, g.step, g.start, nk, cen[0], sums);
    MSTG_CHECK_LAUNCH("slic_init_kernel");
    const float m = (float)compactness;
    const float ws_f = 1.f / (float)(g.step * g.step), wc_f = 1.f / (m * m), kL = 100.f / 255.f;
    const int tx = cdiv(W, SL_TW), tiles = tx * cdiv(H, SL_TH);
    for (int r = 0; r < SL_ROUNDS; ++r) {
        float* next = (r == SL_ROUNDS - 1 && centres) ? centres : cen[(r + 1) & 1];
        MSTG_LAUNCH(slic_assign_kernel, dim3((unsigned)(N * tiles)), dim3(SL_THREADS), 0, st, (const unsigned char*)lab, (const float*)cen[r & 1], K, H,
                    W, g.step, ws_f, wc_f, kL, r == 0 ? 1 : 0, tx, tiles, labels, sums);
        MSTG_CHECK_LAUNCH("slic_assign_kernel");
        MSTG_LAUNCH(slic_final_kernel, sl_grid(nk), dim3(SL_THREADS), 0, st, (const float*)cen[r & 1], sums, nk, next);
        MSTG_CHECK_LAUNCH("slic_final_kernel");
    }
    return MSTG_OK;
}

}  // namespace mstg

using namespace mstg;

extern "C" int mstg_slic_grid(int H, int W, int n_segments, int* step, int* ny, int* nx) {
    if (!step || !ny || !nx) return fail_arg(MSTG_E_BADARG, "slic_grid: null step, ny or nx pointer");
    SlicGrid g;
    const int rc = sl_grid_of("slic_grid", H, W, n_segments, g);
    if (rc != MSTG_OK) return rc;
    *step = g.step, *ny = g.ny, *nx = g.nx;
    return MSTG_OK;
}

extern "C" size_t mstg_slic_workspace_bytes(int N, int H, int W, int n_segments) {
    SlicGrid g;
    if (sl_shape("slic_workspace_bytes", N, H, W, n_segments, g) != MSTG_OK) return 0;
    return sl_workspace(N, H, W, g.ny * g.nx).total;
}

extern "C" size_t mstg_connect_labels_workspace_bytes(int N, int H, int W) {
    if (cc_shape("connect_labels_workspace_bytes", N, H, W) != MSTG_OK) return 0;
    return cc_workspace(N, H, W).total;
}

extern "C" int mstg_connect_labels(const int* labels_in, int N, int H, int W, int min_size, int* labels_out, int* count, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    const int rc = cc_shape("connect_labels", N, H, W);  // first: the refusal does not depend on the buffers
    if (rc != MSTG_OK) return rc;
    if (!labels_in || !labels_out || !count) return fail_arg(MSTG_E_BADARG, "connect_labels: null labels_in, labels_out or count pointer");
    const size_t nb = (size_t)N * H * W * sizeof(int), need = cc_workspace(N, H, W).total, cb = (size_t)N * sizeof(int);
    if (!workspace || workspace_bytes < need) return fail_arg(MSTG_E_WORKSPACE, "connect_labels: workspace too small");
    if (((uintptr_t)labels_in & 3) || ((uintptr_t)labels_out & 3) || ((uintptr_t)count & 3) || ((uintptr_t)workspace & 15))
        return fail_arg(MSTG_E_ALIGN, "connect_labels: labels or count not 4-byte or workspace not 16-byte aligned");
    if (overlaps(labels_out, nb, labels_in, nb) || overlaps(workspace, need, labels_in, nb) || overlaps(workspace, need, labels_out, nb) ||
        overlaps(count, cb, labels_in, nb) || overlaps(count, cb, labels_out, nb) || overlaps(count, cb, workspace, need))
        return fail_arg(MSTG_E_BADARG, "connect_labels: an output or the workspace overlaps the input or another output");
    return cc_run(labels_in, N, H, W, min_size, labels_out, count, (unsigned char*)workspace, (hipStream_t)stream);
}

// the checks the two SLIC entries share; centres and count are nullable here, the callers test theirs
static int sl_check(const char* who, const unsigned char* img, int N, int H, int W, const unsigned short* lab_table, const int* labels,
                    const void* extra, size_t extra_bytes, const void* workspace, size_t workspace_bytes, size_t need) {
    char msg[200];
    if (!img || !lab_table || !labels || !extra) {
        snprintf(msg, sizeof(msg), "%s: null image, table, labels, centres or count pointer", who);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    if (!workspace || workspace_bytes < need) {
        snprintf(msg, sizeof(msg), "%s: workspace too small", who);
        return fail_arg(MSTG_E_WORKSPACE, msg);
    }
    if (((uintptr_t)lab_table & 1) || ((uintptr_t)labels & 3) || ((uintptr_t)extra & 3) || ((uintptr_t)workspace & 15)) {
        snprintf(msg, sizeof(msg), "%s: table not 2-byte, labels, centres or count not 4-byte or workspace not 16-byte aligned", who);
        return fail_arg(MSTG_E_ALIGN, msg);
    }
    const size_t px = (size_t)N * H * W;
    const void* bufs[5] = {img, lab_table, labels, extra, workspace};
    const size_t lens[5] = {px * 3, 2 * MSTG_LAB_TABLE_U16, px * 4, extra_bytes, need};
    for (int a = 2; a < 5; ++a)
        for (int b = 0; b < a; ++b)
            if (overlaps(bufs[a], lens[a], bufs[b], lens[b])) {
                snprintf(msg, sizeof(msg), "%s: an output or the workspace overlaps an input or another output", who);
                return fail_arg(MSTG_E_BADARG, msg);
            }
    return MSTG_OK;
}

extern "C" int mstg_slic_assign_u8(const unsigned char* img, int N, int H, int W, int n_segments, double compactness,
                                   const unsigned short* lab_table, int* labels, float* centres, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    SlicGrid g;
    int rc = sl_shape("slic_assign_u8", N, H, W, n_segments, g);  // first: the refusals do not depend on the buffers
    if (rc == MSTG_OK) rc = sl_compactness("slic_assign_u8", compactness);
    if (rc != MSTG_OK) return rc;
    const int K = g.ny * g.nx;
    const SlicWorkspace ws = sl_workspace(N, H, W, K);
    rc = sl_check("slic_assign_u8", img, N, H, W, lab_table, labels, centres, (size_t)N * K * SL_C * sizeof(float), workspace, workspace_bytes,
                  ws.assign_total);
    if (rc != MSTG_OK) return rc;
    return sl_assign(img, N, H, W, g, compactness, lab_table, labels, centres, (unsigned char*)workspace, ws, stream);
}

extern "C" int mstg_slic_u8(const unsigned char* img, int N, int H, int W, int n_segments, double compactness, const unsigned short* lab_table,
                            int* labels, int* count, void* workspace, size_t workspace_bytes, void* stream) {
    SlicGrid g;
    int rc = sl_shape("slic_u8", N, H, W, n_segments, g);
    if (rc == MSTG_OK) rc = sl_compactness("slic_u8", compactness);
    if (rc != MSTG_OK) return rc;
    const int K = g.ny * g.nx;
    const SlicWorkspace ws = sl_workspace(N, H, W, K);
    rc = sl_check("slic_u8", img, N, H, W, lab_table, labels, count, (size_t)N * sizeof(int), workspace, workspace_bytes, ws.total);
    if (rc != MSTG_OK) return rc;
    unsigned char* base = (unsigned char*)workspace;
    int* raw = (int*)(base + ws.raw);
    rc = sl_assign(img, N, H, W, g, compactness, lab_table, raw, nullptr, base, ws, stream);
    if (rc != MSTG_OK) return rc;
    const int min_size = (int)(0.5 * ((double)((long long)H * W) / (double)K));
    return cc_run(raw, N, H, W, min_size, labels, count, base + ws.cc, (hipStream_t)stream);
}
