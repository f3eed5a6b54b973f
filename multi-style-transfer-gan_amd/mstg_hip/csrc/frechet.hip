// The Frechet distance of two feature sets (the reference's calculate_fid, m_test.py:37-50) on the device, all in float64
// (include/mstg_hip.h, "FRECHET DISTANCE"):
//   fid = |mu1 - mu2|^2 + ||A||_F^2 + ||B||_F^2 - 2 ||A B^T||_*,   A = (X1 - mu1) / sqrt(n1 - 1),   B = (X2 - mu2) / sqrt(n2 - 1).
// The d x d product S1 S2 of the reference is never formed: its nonzero eigenvalues are those of M M^T with M = A B^T (n1 x n2), so
// tr sqrtm(S1 S2) is the sum of the singular values of M.
//
// frechet_center_kernel   one workgroup per 64 columns, 4 row groups: column means (rows in ascending order inside a group, the groups
//                         added 0..3), A and B, and per column (mu1 - mu2)^2, sum A^2, sum B^2.
// frechet_gemm_kernel     M = A B^T on v_mfma_f64_16x16x4_f64: one workgroup per 16 x 16 tile of M, wave w takes the K steps
//                         w, w + 4, ... in ascending order, the four partial tiles are added 0..3.  Ragged n1, n2 and d load zeros.
// frechet_jacobi_kernel   one-sided (Hestenes) Jacobi on G = whichever of M, M^T has fewer columns: ONE workgroup of 1024 threads, the
//                         matrix in LDS when it fits (else in the workspace), 16 lanes per column pair of the round (64 pairs side by
//                         side: the 50 of the reference's 100 samples in one pass), a workgroup barrier per round.  Nothing waits on another workgroup; the sweep loop ends at MSTG_FRECHET_MAX_SWEEPS.
// frechet_finish_kernel   the per-column sums in a fixed order and the five outputs.
// No floating-point atomics, no host synchronisation, every order fixed: two runs give the same bits.
#include <math.h>

#include "common.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace mstg {

constexpr int FC_COLS = 64, FC_GROUPS = 4;             // frechet_center_kernel: 256 threads
constexpr int FJ_THREADS = 1024, FJ_LANES = 16, FJ_GROUPS = FJ_THREADS / FJ_LANES;  // 16 lanes (a DPP row) per column pair
constexpr int FJ_LDS_DOUBLES = 16384;                  // 128 KiB of the CU's 160: a 128 x 128 matrix, or 100 x 100
constexpr double FJ_EPS = 2.220446049250313e-16;       // DBL_EPSILON

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// over the aligned group of FJ_LANES lanes: every lane of the group ends with the same bits
__device__ __forceinline__ double group_sum_d(double v) {
#pragma unroll
    for (int o = FJ_LANES / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <typename T>
__device__ __forceinline__ void center_one(const T* __restrict__ x, int n, int d, int col, int g, double* __restrict__ a, double (*red)[FC_COLS],
                                           int c, double& mu, double& ss) {
    const bool ok = col < d;
    double s = 0.0;
    if (ok)
        for (int r = g; r < n; r += FC_GROUPS) s += (double)x[(size_t)r * d + col];
    red[g][c] = s;
    __syncthreads();
    mu = (((red[0][c] + red[1][c]) + red[2][c]) + red[3][c]) / (double)n;
    __syncthreads();
    const double inv = 1.0 / sqrt((double)(n - 1));
    double q = 0.0;
    if (ok)
        for (int r = g; r < n; r += FC_GROUPS) {
            const double v = ((double)x[(size_t)r * d + col] - mu) * inv;
            a[(size_t)r * d + col] = v;
            q += v * v;
        }
    red[g][c] = q;
    __syncthreads();
    ss = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
    __syncthreads();
}

// part: [3][d] = (mu1 - mu2)^2, sum A^2, sum B^2 of each column
template <typename T>
__global__ __launch_bounds__(FC_COLS* FC_GROUPS) void frechet_center_kernel(const T* __restrict__ x1, const T* __restrict__ x2, int n1, int n2,
                                                                            int d, double* __restrict__ A, double* __restrict__ B,
                                                                            double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double red[FC_GROUPS][FC_COLS];
    const int c = threadIdx.x & (FC_COLS - 1), g = threadIdx.x / FC_COLS;
    const int col = blockIdx.x * FC_COLS + c;
    double mu1, mu2, s1, s2;
    center_one(x1, n1, d, col, g, A, red, c, mu1, s1);
    center_one(x2, n2, d, col, g, B, red, c, mu2, s2);
    if (g == 0 && col < d) {
        const double dm = mu1 - mu2;
        part[col] = dm * dm;
        part[(size_t)d + col] = s1;
        part[2 * (size_t)d + col] = s2;
    }
}

// M[i][j] = sum_k A[i][k] B[j][k], row-major n1 x n2.  The f64 MFMA: lane l supplies A[m = l & 15][k = l >> 4] and B[k = l >> 4][n = l & 15];
// register r of lane l is D[row (l >> 4) + 4 r][col l & 15] (NOT the f32 map).
__global__ __launch_bounds__(256) void frechet_gemm_kernel(const double* __restrict__ A, const double* __restrict__ B, int n1, int n2, int d,
                                                           double* __restrict__ M) {
    __shared__ double red[4][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
    const int mi = i0 + (lane & 15), nj = j0 + (lane & 15), kq = lane >> 4;
    const bool a_ok = mi < n1, b_ok = nj < n2;
    const double* ap = A + (size_t)(a_ok ? mi : 0) * d;
    const double* bp = B + (size_t)(b_ok ? nj : 0) * d;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 4 * w; k0 < d; k0 += 16) {
        const int k = k0 + kq;
        const bool k_ok = k < d;
        const double a = a_ok && k_ok ? ap[k] : 0.0;
        const double b = b_ok && k_ok ? bp[k] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[w][((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc[r];
    __syncthreads();
    const int e = threadIdx.x, i = i0 + (e >> 4), j = j0 + (e & 15);
    if (i < n1 && j < n2) M[(size_t)i * n2 + j] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
}

// slot i of round r of the cyclic pairing of qe = q rounded up to even players (tests/fid_ref.py round_robin)
__device__ __forceinline__ void rr_pair(int r, int i, int qe, int& a, int& b) {
    if (i == 0) {
        a = qe - 1;
        b = r;
    } else {
        a = (r + i) % (qe - 1);
        b = (r - i + qe - 1) % (qe - 1);
    }
    if (a > b) {
        const int t = a;
        a = b;
        b = t;
    }
}

// G (p rows, q <= p columns, column j at G + j * p) = src[i * si + j * sj]; sigma[q] descending; *nuclear = their sum in that order;
// info = {sweeps used, converged}
template <bool IN_LDS>
__global__ __launch_bounds__(FJ_THREADS) void frechet_jacobi_kernel(const double* __restrict__ src, long long si, long long sj, int p, int q,
                                                                    double* gwork, double* __restrict__ sigma, double* __restrict__ nuclear,
                                                                    int* __restrict__ info) {
#pragma clang fp contract(off)
    extern __shared__ double g_lds[];
    __shared__ int rot[FJ_GROUPS], nan_pairs[FJ_GROUPS];
    __shared__ double sv[MSTG_FRECHET_MAX_SAMPLES];
    double* G = IN_LDS ? g_lds : gwork;
    const int tid = threadIdx.x, lane = tid & (FJ_LANES - 1), grp = tid / FJ_LANES;
    for (long long e = tid; e < (long long)p * q; e += FJ_THREADS) {
        const int j = (int)(e / p), i = (int)(e - (long long)j * p);
        G[e] = src[i * si + j * sj];
    }
    __syncthreads();
    const int qe = q + (q & 1);
    const double tol = FJ_EPS * sqrt((double)p);
    int sweeps = 0, converged = q < 2 ? 1 : 0;
    bool done = q < 2;
    while (!done && sweeps < MSTG_FRECHET_MAX_SWEEPS) {
        int mine = 0, undecided = 0;  // rotations and NaN pairs of this group in the sweep (the same in all its lanes)
        for (int r = 0; r < qe - 1; ++r) {
            for (int slot = grp; slot < qe / 2; slot += FJ_GROUPS) {
                int a, b;
                rr_pair(r, slot, qe, a, b);
                if (b >= q) continue;  // the bye of an odd q
                double* ga = G + (size_t)a * p;
                double* gb = G + (size_t)b * p;
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int i = lane; i < p; i += FJ_LANES) {
                    const double x = ga[i], y = gb[i];
                    alpha += x * x;
                    beta += y * y;
                    gamma += x * y;
                }
                alpha = group_sum_d(alpha);
                beta = group_sum_d(beta);
                gamma = group_sum_d(gamma);
                const double bar = tol * (sqrt(alpha) * sqrt(beta));
                if (fabs(gamma) <= bar) continue;
                if (!(fabs(gamma) > bar)) {  // a NaN: no rotation can settle this pair
                    ++undecided;
                    continue;
                }
                ++mine;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = isfinite(zeta) ? copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta)) : 0.0;
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int i = lane; i < p; i += FJ_LANES) {
                    const double x = ga[i], y = gb[i];
                    ga[i] = c * x - s * y;
                    gb[i] = s * x + c * y;
                }
            }
            __syncthreads();  // the columns of a round are disjoint; the next round pairs them anew
        }
        if (lane == 0) {
            rot[grp] = mine;
            nan_pairs[grp] = undecided;
        }
        __syncthreads();
        int total = 0, bad = 0;
        for (int k = 0; k < FJ_GROUPS; ++k) {
            total += rot[k];
            bad += nan_pairs[k];
        }
        __syncthreads();
        ++sweeps;
        done = total == 0;  // nothing moved: another sweep would see the same pairs
        converged = done && bad == 0 ? 1 : 0;
    }
    for (int j = grp; j < q; j += FJ_GROUPS) {
        const double* gj = G + (size_t)j * p;
        double s = 0.0;
        for (int i = lane; i < p; i += FJ_LANES) s += gj[i] * gj[i];
        s = group_sum_d(s);
        if (lane == 0) sv[j] = sqrt(s);
    }
    __syncthreads();
    // descending by counting: the key orders every bit pattern (a NaN above the infinity), the lower column wins a tie
    if (tid < q) {
        const double mine = sv[tid];
        const long long key = __double_as_longlong(mine) & 0x7fffffffffffffffll;
        int rank = 0;
        for (int k = 0; k < q; ++k) {
            const long long other = __double_as_longlong(sv[k]) & 0x7fffffffffffffffll;
            rank += (other > key || (other == key && k < tid)) ? 1 : 0;
        }
        sigma[rank] = mine;
    }
    __syncthreads();  // sigma is global memory written and read by this workgroup only
    if (tid == 0) {
        double s = 0.0;
        for (int k = 0; k < q; ++k) s += sigma[k];
        *nuclear = s;
        info[0] = sweeps;
        info[1] = converged;
    }
}

// out = {ssdiff, tr1, tr2, nuclear, fid}
__global__ __launch_bounds__(256) void frechet_finish_kernel(const double* __restrict__ part, int d, const double* __restrict__ nuclear,
                                                             double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double red[4][3];
    const int tid = threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    for (int c = tid; c < d; c += 256) {
        s[0] += part[c];
        s[1] += part[(size_t)d + c];
        s[2] += part[2 * (size_t)d + c];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = wave_sum_d(s[k]);
    if ((tid & 63) == 0)
        for (int k = 0; k < 3; ++k) red[tid >> 6][k] = s[k];
    __syncthreads();
    if (tid == 0) {
        double t[3];
        for (int k = 0; k < 3; ++k) t[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
        const double nuc = *nuclear;
        out[0] = t[0];
        out[1] = t[1];
        out[2] = t[2];
        out[3] = nuc;
        out[4] = ((t[0] + t[1]) + t[2]) - 2.0 * nuc;
    }
}

// 0 = fine, else the error code (message set)
static int frechet_shape(const char* who, int n1, int n2, int d) {
    char msg[220];
    if (n1 < 2 || n2 < 2) {
        snprintf(msg, sizeof(msg), "%s: n1 = %d, n2 = %d: a covariance needs at least two samples in each set", who, n1, n2);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    if (d < 1) {
        snprintf(msg, sizeof(msg), "%s: d = %d: need at least one feature", who, d);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    if ((n1 < n2 ? n1 : n2) > MSTG_FRECHET_MAX_SAMPLES) {
        snprintf(msg, sizeof(msg), "%s: min(n1, n2) = %d is above MSTG_FRECHET_MAX_SAMPLES = %d; the d x d form for more samples is not built", who,
                 n1 < n2 ? n1 : n2, MSTG_FRECHET_MAX_SAMPLES);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    if ((long long)n1 * d >= (1ll << 31) || (long long)n2 * d >= (1ll << 31) || (long long)n1 * n2 >= (1ll << 31)) {
        snprintf(msg, sizeof(msg), "%s: n1 * d = %lld, n2 * d = %lld, n1 * n2 = %lld: one of them does not fit 31 bits", who, (long long)n1 * d,
                 (long long)n2 * d, (long long)n1 * n2);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    if ((n1 + 15) / 16 > 65535) {
        snprintf(msg, sizeof(msg), "%s: n1 = %d: more than 65535 tile rows in one launch", who, n1);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    return MSTG_OK;
}

static int svd_shape(const char* who, int m, int n) {
    char msg[200];
    if (m < 1 || n < 1) {
        snprintf(msg, sizeof(msg), "%s: m = %d, n = %d: need at least one row and one column", who, m, n);
        return fail_arg(MSTG_E_BADARG, msg);
    }
    if ((m < n ? m : n) > MSTG_FRECHET_MAX_SAMPLES) {
        snprintf(msg, sizeof(msg), "%s: min(m, n) = %d is above MSTG_FRECHET_MAX_SAMPLES = %d", who, m < n ? m : n, MSTG_FRECHET_MAX_SAMPLES);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    if ((long long)m * n >= (1ll << 31)) {
        snprintf(msg, sizeof(msg), "%s: m * n = %lld does not fit 31 bits", who, (long long)m * n);
        return fail_arg(MSTG_E_UNSUPPORTED, msg);
    }
    return MSTG_OK;
}

// src (m x n, element (i, j) at src[i * n + j]) -> sigma, nuclear, info; gwork: m * n doubles
static int launch_jacobi(const double* src, int m, int n, double* gwork, double* sigma, double* nuclear, int* info, hipStream_t st) {
    const bool keep = n <= m;  // G = src, else its transpose
    const int p = keep ? m : n, q = keep ? n : m;
    const long long si = keep ? n : 1, sj = keep ? 1 : n;
    if ((long long)p * q <= FJ_LDS_DOUBLES) {
        static hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&frechet_jacobi_kernel<true>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, FJ_LDS_DOUBLES * (int)sizeof(double));
        if (e != hipSuccess) return fail_launch(e, "hipFuncSetAttribute(frechet_jacobi_kernel)");
        MSTG_LAUNCH(frechet_jacobi_kernel<true>, dim3(1), dim3(FJ_THREADS), (size_t)p * q * sizeof(double), st, src, si, sj, p, q, gwork, sigma,
                    nuclear, info);
    } else {
        MSTG_LAUNCH(frechet_jacobi_kernel<false>, dim3(1), dim3(FJ_THREADS), 0, st, src, si, sj, p, q, gwork, sigma, nuclear, info);
    }
    MSTG_CHECK_LAUNCH("frechet_jacobi_kernel");
    return MSTG_OK;
}

}  // namespace mstg

using namespace mstg;

extern "C" size_t mstg_frechet_workspace_bytes(int n1, int n2, int d) {
    if (frechet_shape("frechet_workspace_bytes", n1, n2, d) != MSTG_OK) return 0;
    const size_t q = (size_t)(n1 < n2 ? n1 : n2);
    return ((size_t)n1 * d + (size_t)n2 * d + 3 * (size_t)d + 2 * (size_t)n1 * n2 + q + 1) * sizeof(double);
}

extern "C" int mstg_frechet_distance(const void* x1, const void* x2, int is_f64, int n1, int n2, int d, double* out, int* info, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    if (!x1 || !x2 || !out || !info) return fail_arg(MSTG_E_BADARG, "frechet_distance: null feature, output or info pointer");
    const int rc = frechet_shape("frechet_distance", n1, n2, d);
    if (rc != MSTG_OK) return rc;
    const size_t need = mstg_frechet_workspace_bytes(n1, n2, d);
    if (!workspace || workspace_bytes < need) {
        char msg[160];
        snprintf(msg, sizeof(msg), "frechet_distance: workspace of %zu bytes, need %zu", workspace ? workspace_bytes : (size_t)0, need);
        return fail_arg(MSTG_E_WORKSPACE, msg);
    }
    if (((uintptr_t)workspace & 7) || ((uintptr_t)out & 7) || ((uintptr_t)x1 & (is_f64 ? 7 : 3)) || ((uintptr_t)x2 & (is_f64 ? 7 : 3)))
        return fail_arg(MSTG_E_ALIGN, "frechet_distance: features, out or workspace not aligned to their element");
    hipStream_t st = (hipStream_t)stream;
    double* A = (double*)workspace;
    double* B = A + (size_t)n1 * d;
    double* part = B + (size_t)n2 * d;
    double* M = part + 3 * (size_t)d;
    double* gwork = M + (size_t)n1 * n2;
    double* sigma = gwork + (size_t)n1 * n2;
    double* nuclear = sigma + (n1 < n2 ? n1 : n2);
    const dim3 cgrid((unsigned)cdiv(d, FC_COLS));
    if (is_f64)
        MSTG_LAUNCH(frechet_center_kernel<double>, cgrid, dim3(FC_COLS * FC_GROUPS), 0, st, (const double*)x1, (const double*)x2, n1, n2, d, A, B,
                    part);
    else
        MSTG_LAUNCH(frechet_center_kernel<float>, cgrid, dim3(FC_COLS * FC_GROUPS), 0, st, (const float*)x1, (const float*)x2, n1, n2, d, A, B,
                    part);
    MSTG_CHECK_LAUNCH("frechet_center_kernel");
    MSTG_LAUNCH(frechet_gemm_kernel, dim3((unsigned)cdiv(n2, 16), (unsigned)cdiv(n1, 16)), dim3(256), 0, st, (const double*)A, (const double*)B, n1,
                n2, d, M);
    MSTG_CHECK_LAUNCH("frechet_gemm_kernel");
    const int jr = launch_jacobi(M, n1, n2, gwork, sigma, nuclear, info, st);
    if (jr != MSTG_OK) return jr;
    MSTG_LAUNCH(frechet_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)part, d, (const double*)nuclear, out);
    MSTG_CHECK_LAUNCH("frechet_finish_kernel");
    return MSTG_OK;
}

extern "C" size_t mstg_singular_values_workspace_bytes(int m, int n) {
    if (svd_shape("singular_values_workspace_bytes", m, n) != MSTG_OK) return 0;
    return ((size_t)m * n + 1) * sizeof(double);
}

extern "C" int mstg_singular_values(const double* M, int m, int n, double* sigma, int* info, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    if (!M || !sigma || !info) return fail_arg(MSTG_E_BADARG, "singular_values: null matrix, output or info pointer");
    const int rc = svd_shape("singular_values", m, n);
    if (rc != MSTG_OK) return rc;
    const size_t need = mstg_singular_values_workspace_bytes(m, n);
    if (!workspace || workspace_bytes < need) {
        char msg[160];
        snprintf(msg, sizeof(msg), "singular_values: workspace of %zu bytes, need %zu", workspace ? workspace_bytes : (size_t)0, need);
        return fail_arg(MSTG_E_WORKSPACE, msg);
    }
    if (((uintptr_t)workspace & 7) || ((uintptr_t)sigma & 7) || ((uintptr_t)M & 7))
        return fail_arg(MSTG_E_ALIGN, "singular_values: matrix, sigma or workspace not 8-byte aligned");
    double* gwork = (double*)workspace;
    return launch_jacobi(M, m, n, gwork, sigma, gwork + (size_t)m * n, info, (hipStream_t)stream);
}
