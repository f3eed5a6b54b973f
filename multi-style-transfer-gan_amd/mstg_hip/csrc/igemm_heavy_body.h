// Body of igemm_heavy_kernel and igemm_heavy_grouped_kernel (conv_igemm.hip), included once into each: the kernels differ only in
// where a workgroup's x index and the x extent of its launch come from (IG_BX, IG_NBX) and in whose pointers `a` / `wp` hold.
// Included text, not a shared function, so that the single-launch kernel compiles to exactly the code it had on its own.
// In scope: a (IGemmArgs), wp, CoP, the template arguments V, NFW, SRC.
    constexpr int CK = 4 * V, CKP = ckp_heavy_of<V>(), BN = 16 * NFW;
    typedef typename Frag<V>::T frag_t;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int PSZ = (a.PH * a.PW * CKP + 3) & ~3, WSZ = a.TG * BN * CKP;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
    const int co0 = blockIdx.y * BN;
    const int cls = blockIdx.z, pa = cls >> 1, pb = cls & 1;
    const int s = a.phase ? 1 : a.stride;
    const int nchunks = (a.Cr + CK - 1) / CK;
    const int ngroups = (a.ntaps + a.TG - 1) / a.TG;
    const int ntiles = a.N * a.tiles_x * a.tiles_y;
    const int my_tiles = (ntiles - (int)IG_BX + (int)IG_NBX - 1) / (int)IG_NBX;
    const int total = my_tiles * nchunks * ngroups;
    const int npatch = a.PH * a.PW * V;

    // per-thread slot descriptors (tile independent).  patch: LDS float offset, row, col, quad; unused slots read pixel 0.
    int p_lds[NPQ], p_rc[NPQ];
#pragma unroll
    for (int j = 0; j < NPQ; ++j) {
        const int e = tid + 256 * j;
        const bool used = e < npatch;
        const int ee = used ? e : 0;
        const int pr = ee / (a.PW * V), rem = ee % (a.PW * V), pc = rem / V, q = rem % V;
        p_lds[j] = used ? (pr * a.PW + pc) * CKP + 4 * q : -1;
        p_rc[j] = pr | (pc << 8) | (q << 16);
    }
    int w_src[NWQ], w_lds[NWQ];  // filter: offset inside the stage's packed slice (tap-local), LDS float offset, or -1
#pragma unroll
    for (int j = 0; j < NWQ; ++j) {
        const int e = tid + 256 * j, row = e / V, q = e % V, tl = row / BN, col = row % BN;
        const bool used = tl < a.TG;
        w_src[j] = used ? (tl * CoP + col) * CK + 4 * q : 0;
        w_lds[j] = used ? row * CKP + 4 * q : -1;
    }

    // two cursors over (tile sequence number, chunk, tap group): cur = stage being computed, nxt = stage being loaded
    int c_seq = 0, c_chunk = 0, c_tg = 0, c_tx0, c_ty0, c_n;
    int n_seq = 0, n_chunk = 0, n_tg = 0, n_tx0, n_ty0, n_n;
    {
        const int tile = xcd_swizzle((int)IG_BX, ntiles);
        c_tx0 = n_tx0 = tile % a.tiles_x;
        c_ty0 = n_ty0 = (tile / a.tiles_x) % a.tiles_y;
        c_n = n_n = tile / (a.tiles_x * a.tiles_y);
    }

    f32x4 preg[NPQ], wreg[NWQ];

#define IG_LOAD_STAGE()                                                                                                     \
    {                                                                                                                       \
        if (n_tg == 0) {                                                                                                    \
            const int y0 = a.phase ? n_ty0 * TILE_H - 1 : n_ty0 * TILE_H * s - a.pad;                                       \
            const int x0 = a.phase ? n_tx0 * TILE_W - 1 : n_tx0 * TILE_W * s - a.pad;                                       \
            _Pragma("unroll") for (int j = 0; j < NPQ; ++j) {                                                               \
                const int iy = min(max(y0 + (p_rc[j] & 255), 0), a.H - 1), ix = min(max(x0 + ((p_rc[j] >> 8) & 255), 0), a.W - 1); \
                if (SRC == 2) {                                                                                             \
                    const size_t cs = (size_t)a.H * a.W;                                                                    \
                    const float* src = a.x + (((size_t)n_n * a.x_ctot + a.x_coff) * a.H + iy) * a.W + ix;                   \
                    preg[j][0] = src[0];                                                                                    \
                    preg[j][1] = src[(a.Cr > 1 ? 1 : 0) * cs];                                                              \
                    preg[j][2] = src[(a.Cr > 2 ? 2 : 0) * cs];                                                              \
                    preg[j][3] = src[(a.Cr > 3 ? 3 : 0) * cs];                                                              \
                } else if (SRC == 0) {                                                                                      \
                    const int c0 = min(n_chunk * CK + 4 * (p_rc[j] >> 16), a.Cr - 4);                                       \
                    preg[j] = *reinterpret_cast<const f32x4*>(a.x + (((size_t)n_n * a.H + iy) * a.W + ix) * a.x_ctot + a.x_coff + c0); \
                } else {                                                                                                    \
                    const int c0 = min(n_chunk * CK + 4 * (p_rc[j] >> 16), a.Cr - 1), rem = a.Cr - 1 - c0;                  \
                    const float* src = a.x + (((size_t)n_n * a.H + iy) * a.W + ix) * a.x_ctot + a.x_coff + c0;              \
                    preg[j][0] = src[0];                                                                                    \
                    preg[j][1] = src[min(1, rem)];                                                                          \
                    preg[j][2] = src[min(2, rem)];                                                                          \
                    preg[j][3] = src[min(3, rem)];                                                                          \
                }                                                                                                           \
            }                                                                                                               \
        }                                                                                                                   \
        {                                                                                                                   \
            const int t0 = n_tg * a.TG, tlast = a.ntaps - 1 - t0;                                                           \
            const float* base = wp + ((size_t)((cls * nchunks + n_chunk) * a.ntaps + t0) * CoP + co0) * CK;                 \
            const int lim = tlast * CoP * CK;  /* rows of taps beyond the filter are clamped to its last tap */             \
            _Pragma("unroll") for (int j = 0; j < NWQ; ++j) {                                                               \
                const int off = w_src[j] > lim + (CoP - 1) * CK + CK - 4 ? 0 : w_src[j];                                    \
                wreg[j] = *reinterpret_cast<const f32x4*>(base + off);                                                      \
            }                                                                                                               \
        }                                                                                                                   \
    }

#define IG_STORE_STAGE(KBUF)                                                                                                \
    {                                                                                                                       \
        if (n_tg == 0) {                                                                                                    \
            float* patch = smem + ((n_seq * nchunks + n_chunk) & 1) * PSZ;                                                  \
            const int y0 = a.phase ? n_ty0 * TILE_H - 1 : n_ty0 * TILE_H * s - a.pad;                                       \
            const int x0 = a.phase ? n_tx0 * TILE_W - 1 : n_tx0 * TILE_W * s - a.pad;                                       \
            _Pragma("unroll") for (int j = 0; j < NPQ; ++j) {                                                               \
                if (p_lds[j] >= 0) {                                                                                        \
                    const int iy = y0 + (p_rc[j] & 255), ix = x0 + ((p_rc[j] >> 8) & 255);                                  \
                    const bool inb = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;                          \
                    const int c0 = SRC == 2 ? 0 : n_chunk * CK + 4 * (p_rc[j] >> 16);                                       \
                    const int nreal = inb ? a.Cr - c0 : 0;                                                                  \
                    f32x4 v = preg[j];                                                                                      \
                    v[0] = nreal > 0 ? v[0] : 0.f;                                                                          \
                    v[1] = nreal > 1 ? v[1] : 0.f;                                                                          \
                    v[2] = nreal > 2 ? v[2] : 0.f;                                                                          \
                    v[3] = nreal > 3 ? v[3] : 0.f;                                                                          \
                    *reinterpret_cast<f32x4*>(&patch[p_lds[j]]) = v;                                                        \
                }                                                                                                           \
            }                                                                                                               \
        }                                                                                                                   \
        {                                                                                                                   \
            float* wl = smem + 2 * PSZ + (KBUF)*WSZ;                                                                        \
            const int tn = min(a.TG, a.ntaps - n_tg * a.TG);                                                                \
            _Pragma("unroll") for (int j = 0; j < NWQ; ++j) {                                                               \
                if (w_lds[j] >= 0 && w_lds[j] < tn * BN * CKP) *reinterpret_cast<f32x4*>(&wl[w_lds[j]]) = wreg[j];          \
            }                                                                                                               \
        }                                                                                                                   \
    }

#define IG_ADVANCE(P)                                                                                                       \
    {                                                                                                                       \
        if (++P##_tg == ngroups) {                                                                                          \
            P##_tg = 0;                                                                                                     \
            if (++P##_chunk == nchunks) {                                                                                   \
                P##_chunk = 0;                                                                                              \
                ++P##_seq;                                                                                                  \
                if (P##_seq < my_tiles) {                                                                                   \
                    const int tile = xcd_swizzle((int)IG_BX + P##_seq * (int)IG_NBX, ntiles);                               \
                    P##_tx0 = tile % a.tiles_x;                                                                             \
                    P##_ty0 = (tile / a.tiles_x) % a.tiles_y;                                                               \
                    P##_n = tile / (a.tiles_x * a.tiles_y);                                                                 \
                }                                                                                                           \
            }                                                                                                               \
        }                                                                                                                   \
    }

    if (total > 0) {
        IG_LOAD_STAGE();
        IG_STORE_STAGE(0);
        IG_ADVANCE(n);
    }
    __syncthreads();

    f32x4 acc[NFW][2];
    for (int k = 0; k < total; ++k) {
        const bool more = k + 1 < total;
        if (more) IG_LOAD_STAGE();  // in flight during the MFMAs below
        const float* wl = smem + 2 * PSZ + (k & 1) * WSZ;
        const float* patch = smem + ((c_seq * nchunks + c_chunk) & 1) * PSZ;
        if (c_chunk == 0 && c_tg == 0) {
#pragma unroll
            for (int wf = 0; wf < NFW; ++wf)
#pragma unroll
                for (int pf = 0; pf < 2; ++pf) acc[wf][pf] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        // ---- MFMA over the group's taps; the fragments of tap t+1 are read from LDS while tap t's MFMAs issue ------
        const int t0 = c_tg * a.TG, tn = min(a.TG, a.ntaps - t0);
        const int brow0 = ((2 * wave) * s * a.PW + i * s) * CKP + V * g, brow1 = brow0 + s * a.PW * CKP;
        const int arow = i * CKP + V * g;
        frag_t af[NFW], bf[2], afn[NFW], bfn[2];
        {
            const int po = tap_patch_offset(a, t0, pa, pb, CKP);
#pragma unroll
            for (int wf = 0; wf < NFW; ++wf) af[wf] = *reinterpret_cast<const frag_t*>(&wl[16 * wf * CKP + arow]);
            bf[0] = *reinterpret_cast<const frag_t*>(&patch[brow0 + po]);
            bf[1] = *reinterpret_cast<const frag_t*>(&patch[brow1 + po]);
        }
        for (int tl = 0; tl < tn; ++tl) {
            const int tnext = min(tl + 1, tn - 1);
            const int po = tap_patch_offset(a, t0 + tnext, pa, pb, CKP);
#pragma unroll
            for (int wf = 0; wf < NFW; ++wf) afn[wf] = *reinterpret_cast<const frag_t*>(&wl[(tnext * BN + 16 * wf) * CKP + arow]);
            bfn[0] = *reinterpret_cast<const frag_t*>(&patch[brow0 + po]);
            bfn[1] = *reinterpret_cast<const frag_t*>(&patch[brow1 + po]);
#pragma unroll
            for (int j = 0; j < V; ++j)
#pragma unroll
                for (int wf = 0; wf < NFW; ++wf)
#pragma unroll
                    for (int pf = 0; pf < 2; ++pf)
                        acc[wf][pf] = mfma16(frag_get<V>(af[wf], j), frag_get<V>(bf[pf], j), acc[wf][pf]);
#pragma unroll
            for (int wf = 0; wf < NFW; ++wf) af[wf] = afn[wf];
            bf[0] = bfn[0];
            bf[1] = bfn[1];
        }
        if (c_chunk == nchunks - 1 && c_tg == ngroups - 1) igemm_epilogue<NFW>(a, acc, c_n, c_ty0, c_tx0, co0, pa, pb, wave, i, g);
        if (more) {
            IG_STORE_STAGE((k + 1) & 1);
            IG_ADVANCE(n);
        }
        IG_ADVANCE(c);
        __syncthreads();
    }
#undef IG_LOAD_STAGE
#undef IG_STORE_STAGE
#undef IG_ADVANCE
