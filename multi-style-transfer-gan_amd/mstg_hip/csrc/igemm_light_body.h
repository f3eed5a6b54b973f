// Body of igemm_light_kernel and igemm_light_grouped_kernel (conv_igemm.hip), included once into each: the kernels differ only in
// where a workgroup's x index and the x extent of its launch come from (IG_BX, IG_NBX) and in whose pointers `a` / `wp` hold.
// Included text, not a shared function, so that the single-launch kernel compiles to exactly the code it had on its own.
// In scope: a (IGemmArgs), wp, CoP, the template arguments V, NFW, PF.
    constexpr int CK = 4 * V, CKP = ckp_of<V>(), BN = 16 * NFW, TH = 4 * PF;
    typedef typename Frag<V>::T frag_t;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* patch = smem;
    float* wl = smem + ((a.PH * a.PW * CKP + 3) & ~3);
    int* tapo = reinterpret_cast<int*>(wl + (a.wglob ? 0 : a.TG * BN * CKP));  // LDS offset of every tap inside the patch

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
    const int tile = xcd_swizzle(IG_BX, IG_NBX);
    const int tx0 = tile % a.tiles_x, ty0 = (tile / a.tiles_x) % a.tiles_y, n = tile / (a.tiles_x * a.tiles_y);
    const int co0 = blockIdx.y * BN;
    const int cls = blockIdx.z, pa = cls >> 1, pb = cls & 1;
    const int s = a.phase ? 1 : a.stride;
    const int y0 = a.phase ? ty0 * TH - 1 : ty0 * TH * s - a.pad;
    // dpack: tiles advance by 13 output columns; the 16 accumulator columns start 3 pixels to their left
    const int x0 = a.phase ? tx0 * TILE_W - 1 : (a.dpack ? tx0 * 13 - 3 - a.pad : tx0 * TILE_W * s - a.pad);
    const int nchunks = (a.Cr + CK - 1) / CK;
    const unsigned m_pw = magic_u32(a.PW);
    MSTG_STAMP(0)
    if (tid < a.ntaps) tapo[tid] = tap_patch_offset(a, tid, pa, pb, CKP);  // visible after the first barrier below

    f32x4 acc[NFW][PF];
#pragma unroll
    for (int wf = 0; wf < NFW; ++wf)
#pragma unroll
        for (int pf = 0; pf < PF; ++pf) acc[wf][pf] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int chunk = 0; chunk < nchunks; ++chunk) {
        if (chunk) __syncthreads();
        // ---- stage the source patch (halo included, zero outside the image) -------------------------------------
        if (a.x_nchw) {  // 3-channel image tensor, V == 1: channel 3 of the k-slot group is zero
            stage_window_c4(a.x + ((size_t)n * a.x_ctot + a.x_coff) * a.H * a.W, patch, a.PH, a.PW, m_pw, y0, x0, a.H, a.W, (unsigned)a.W, 1u,
                            (unsigned)(a.H * a.W), a.Cr, tid);
        } else if (((a.x_ctot | a.x_coff | a.Cr) & 3) == 0) {
            stage_window(a.x + (size_t)n * a.H * a.W * a.x_ctot + a.x_coff + chunk * CK, patch, a.PH, a.PW, V, m_pw, 0xFFFFFFFFu / V + 1u, y0,
                         x0, a.H, a.W, a.x_ctot, min(V, (a.Cr - chunk * CK) >> 2), CKP, tid);
        } else {
            for (int pr = wave; pr < a.PH; pr += 4) {
                const int iy = y0 + pr;
                for (int e = lane; e < a.PW * V; e += 64) {
                    const int pc = e / V, q = e % V;
                    const int ix = x0 + pc;
                    const bool inb = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                    f32x4 v = {0.f, 0.f, 0.f, 0.f};
                    const int c0 = chunk * CK + 4 * q;
                    if (inb && c0 < a.Cr) {
                        const float* src = a.x + (((size_t)n * a.H + iy) * a.W + ix) * a.x_ctot + a.x_coff + c0;
#pragma unroll
                        for (int c = 0; c < 4; ++c)
                            if (c0 + c < a.Cr) v[c] = src[c];
                    }
                    *reinterpret_cast<f32x4*>(&patch[(pr * a.PW + pc) * CKP + 4 * q]) = v;
                }
            }
        }
        MSTG_STAMP(1)
        if (a.wglob) {
            // ---- filter fragments from L2: no filter slice in LDS, no second barrier; tap t+2's fragment is in flight --------------
            __syncthreads();
            const float* wb = wp + ((size_t)((cls * nchunks + chunk) * a.ntaps) * CoP + co0 + i) * CK + V * g;
            const int wts = CoP * CK;  // floats between consecutive taps
            const int bbase0 = ((PF * wave) * s * a.PW + i * s) * CKP + V * g, bstep = s * a.PW * CKP;
            frag_t a0[NFW], a1[NFW], a2[NFW], bf[PF], bfn[PF];
#pragma unroll
            for (int wf = 0; wf < NFW; ++wf) {
                a0[wf] = *reinterpret_cast<const frag_t*>(wb + 16 * wf * CK);
                a1[wf] = *reinterpret_cast<const frag_t*>(wb + min(1, a.ntaps - 1) * wts + 16 * wf * CK);
            }
            {
                const int po = tapo[0];
#pragma unroll
                for (int pf = 0; pf < PF; ++pf) bf[pf] = *reinterpret_cast<const frag_t*>(&patch[bbase0 + pf * bstep + po]);
            }
            for (int tl = 0; tl < a.ntaps; ++tl) {
                const int t2 = min(tl + 2, a.ntaps - 1), t1 = min(tl + 1, a.ntaps - 1);
#pragma unroll
                for (int wf = 0; wf < NFW; ++wf) a2[wf] = *reinterpret_cast<const frag_t*>(wb + t2 * wts + 16 * wf * CK);
                const int po = tapo[t1];
#pragma unroll
                for (int pf = 0; pf < PF; ++pf) bfn[pf] = *reinterpret_cast<const frag_t*>(&patch[bbase0 + pf * bstep + po]);
#pragma unroll
                for (int j = 0; j < V; ++j)
#pragma unroll
                    for (int wf = 0; wf < NFW; ++wf)
#pragma unroll
                        for (int pf = 0; pf < PF; ++pf)
                            acc[wf][pf] = mfma16(frag_get<V>(a0[wf], j), frag_get<V>(bf[pf], j), acc[wf][pf]);
#pragma unroll
                for (int wf = 0; wf < NFW; ++wf) { a0[wf] = a1[wf]; a1[wf] = a2[wf]; }
#pragma unroll
                for (int pf = 0; pf < PF; ++pf) bf[pf] = bfn[pf];
            }
            continue;
        }
        for (int t0 = 0; t0 < a.ntaps; t0 += a.TG) {
            __syncthreads();  // patch staged / previous tap group consumed
            MSTG_STAMP(2)
            const int tn = min(a.TG, a.ntaps - t0);
            // ---- stage this tap group's filter slice: 16-byte copies out of the packed filter ---------------------
            const float* base = wp + ((size_t)((cls * nchunks + chunk) * a.ntaps + t0) * CoP + co0) * CK;
            for (int e0 = 0; e0 < tn * BN * V; e0 += 1024) {
                f32x4 wv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int e = min(e0 + 256 * k + tid, tn * BN * V - 1);
                    const int row = e / V, q = e % V, tl = row / BN, col = row % BN;
                    wv[k] = *reinterpret_cast<const f32x4*>(base + (unsigned)((tl * CoP + col) * CK + 4 * q));
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int e = e0 + 256 * k + tid;
                    if (e < tn * BN * V) *reinterpret_cast<f32x4*>(&wl[(e / V) * CKP + 4 * (e % V)]) = wv[k];
                }
            }
            MSTG_STAMP(3)
            __syncthreads();
            MSTG_STAMP(4)
            // ---- MFMA over the group's taps -------------------------------------------------------------------------
            // fragments of tap tl+1 are read while the MFMAs of tap tl run
            const int bbase0 = ((PF * wave) * s * a.PW + i * s) * CKP + V * g, bstep = s * a.PW * CKP;
            frag_t af[NFW], bf[PF], afn[NFW], bfn[PF];
            {
                const int po = tapo[t0];
#pragma unroll
                for (int wf = 0; wf < NFW; ++wf) af[wf] = *reinterpret_cast<const frag_t*>(&wl[(16 * wf + i) * CKP + V * g]);
#pragma unroll
                for (int pf = 0; pf < PF; ++pf) bf[pf] = *reinterpret_cast<const frag_t*>(&patch[bbase0 + pf * bstep + po]);
            }
            for (int tl = 0; tl < ((a.dbg & 1) ? 1 : tn); ++tl) {
                const int tnx = min(tl + 1, tn - 1);
                const int po = tapo[t0 + tnx];
#pragma unroll
                for (int wf = 0; wf < NFW; ++wf) afn[wf] = *reinterpret_cast<const frag_t*>(&wl[(tnx * BN + 16 * wf + i) * CKP + V * g]);
#pragma unroll
                for (int pf = 0; pf < PF; ++pf) bfn[pf] = *reinterpret_cast<const frag_t*>(&patch[bbase0 + pf * bstep + po]);
#pragma unroll
                for (int j = 0; j < V; ++j)
#pragma unroll
                    for (int wf = 0; wf < NFW; ++wf)
#pragma unroll
                        for (int pf = 0; pf < PF; ++pf)
                            acc[wf][pf] = mfma16(frag_get<V>(af[wf], j), frag_get<V>(bf[pf], j), acc[wf][pf]);
#pragma unroll
                for (int wf = 0; wf < NFW; ++wf) af[wf] = afn[wf];
#pragma unroll
                for (int pf = 0; pf < PF; ++pf) bf[pf] = bfn[pf];
            }
        }
    }
    MSTG_STAMP(5)
    if (!a.dpack) {
        igemm_epilogue<NFW, PF>(a, acc, n, ty0, tx0, co0, pa, pb, wave, i, g);
        MSTG_STAMP(6)
        return;
    }
    // ---- dpack epilogue.  Accumulator row 4*delta + c of pixel column p is a partial sum of output column p + delta:
    //      y[q][c] = sum_delta D[delta][q - delta].  Exchange through LDS, then lanes (q < 13, pf) finish 13 columns. ---------
    __syncthreads();  // everybody is done with the filter / patch tiles: reuse the front of LDS
    float* comb = smem + wave * (256 * PF);  // [pf][delta][p][4]
#pragma unroll
    for (int pf = 0; pf < PF; ++pf) *reinterpret_cast<f32x4*>(&comb[((pf * 4 + g) * 16 + i) * 4]) = acc[0][pf];
    __syncthreads();
    if (g < PF && i < 13) {
        const int pf = g;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int d = 0; d < 4; ++d) v += *reinterpret_cast<const f32x4*>(&comb[((pf * 4 + d) * 16 + i + 3 - d) * 4]);
        const int oy = ty0 * TH + PF * wave + pf, ox = tx0 * 13 + i;
        if (oy < a.Gh && ox < a.Gw) {
            if (!a.y_nchw && a.Co == 4 && ((a.y_ctot | a.y_coff) & 3) == 0) {  // a whole 4-channel slice: one 16-byte store
                float* p = a.y + (((size_t)n * a.Ho + oy) * a.Wo + ox) * a.y_ctot + a.y_coff;
                if (a.bias) v += *reinterpret_cast<const f32x4*>(a.bias);
                if (a.accumulate) v += *reinterpret_cast<const f32x4*>(p);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = apply_act(v[e], a.act);
                *reinterpret_cast<f32x4*>(p) = v;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (e >= a.Co) continue;
                    float* p = a.y_nchw ? a.y + (((size_t)n * a.y_ctot + a.y_coff + e) * a.Ho + oy) * a.Wo + ox
                                        : a.y + (((size_t)n * a.Ho + oy) * a.Wo + ox) * a.y_ctot + a.y_coff + e;
                    float val = v[e] + (a.bias ? a.bias[e] : 0.f);
                    if (a.accumulate) val += *p;
                    *p = apply_act(val, a.act);
                }
            }
        }
    }
    MSTG_STAMP(6)
