// Body of conv_p32_kernel and conv_p32_grouped_kernel (conv_p32.hip), included once into each: the two kernels differ only in where a
// workgroup's index and the number of workgroups that share its tiles come from (P32_BX, P32_NWG) and in whose pointers `a` holds.
// Included text, not a shared function, so that the single-launch kernel compiles to exactly the code it had on its own.
// In scope: a (P32Args), p (P32Plan), the template arguments RPW, NF, NPF, WLDS, STATS.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int TH = 4 * RPW;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nl = lane & 15, g = lane >> 4;
    const int ntile = a.tiles_x * a.tiles_y, total_tiles = a.N * ntile, G = P32_NWG;
    unsigned char* wl = smem + P32_TABLE_BYTES;
    unsigned char* patch = wl + (WLDS ? (size_t)p.nsteps * NF * 1024 : 0);
    if (tid < P32_MAX_STEPS) {
        reinterpret_cast<unsigned*>(smem)[tid] = p.koff[tid];
    } else if (tid < P32_MAX_STEPS + P32_MAX_SEG) {
        const int c = tid - P32_MAX_STEPS;
        int* e = reinterpret_cast<int*>(smem + 4 * P32_MAX_STEPS + 16 * c);
        e[0] = p.seg[c].s0; e[1] = p.seg[c].s1; e[2] = p.seg[c].oy; e[3] = p.seg[c].ox;
    }
    if (WLDS) {
        const int nchunk = p.nsteps * NF * 64;
        for (int e = tid; e < nchunk; e += 256) reinterpret_cast<f32x4*>(wl)[e] = reinterpret_cast<const f32x4*>(a.wpk)[e];
    }
    const f32x4* wglob = reinterpret_cast<const f32x4*>(a.wpk) + lane;  // static address spaces: no flat loads
    const unsigned char* wlds_lane = wl + 16 * lane;
    const int nseg = p.nseg, up = p.up;
    unsigned base[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) base[r] = (unsigned)(((RPW * wv + r) * p.stride * p.PW + nl * p.stride) * p.pixstride + 16 * g);
    f32x4 b4[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) b4[f] = *reinterpret_cast<const f32x4*>(a.bias + 16 * f + 4 * g);

    // what a thread stages is the same for every tile: element k of thread tid = channel quad o of patch pixel (r, c)
    const int quads = a.Cin >> 2, o = tid & (quads - 1), sh = quads == 4 ? 2 : (quads == 8 ? 3 : 4);
    unsigned rel[NPF], vmask = 0;
    {
        const int total = p.PH * p.PW * quads;
#pragma unroll
        for (int k = 0; k < NPF; ++k) {
            const int e = 256 * k + tid, pix = e >> sh;
            const int r = (int)__umulhi((unsigned)pix, p.m_pw), c = pix - r * p.PW;
            if (e < total) vmask |= 1u << k;
            rel[k] = (unsigned)(((r * a.W + c) * a.Cin + 4 * o) * 4);
        }
    }
    float ssum[STATS ? NF : 1][4], ssq[STATS ? NF : 1][4];
#pragma unroll
    for (int f = 0; f < (STATS ? NF : 1); ++f)
#pragma unroll
        for (int q = 0; q < 4; ++q) ssum[f][q] = ssq[f][q] = 0.f;
    const int lb = STATS ? xcd_swizzle((int)P32_BX, G) : (int)P32_BX;  // logical index of this workgroup's tile range (below)
    auto flush_stats = [&](int n_img) {  // between tiles only (the scratch aliases the patch); ends with a barrier
        float* red = reinterpret_cast<float*>(patch);  // [4 waves][2][16 * NF]
#pragma unroll
        for (int f = 0; f < (STATS ? NF : 1); ++f)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float s1 = row16_sum(ssum[f][q]), s2 = row16_sum(ssq[f][q]);
                if (nl == 0) {
                    red[(wv * 2 + 0) * 16 * NF + 16 * f + 4 * g + q] = s1;
                    red[(wv * 2 + 1) * 16 * NF + 16 * f + 4 * g + q] = s2;
                }
                ssum[f][q] = ssq[f][q] = 0.f;
            }
        __syncthreads();
        if (tid < 2 * 16 * NF)
            a.partial[((size_t)n_img * G + lb) * 2 * 16 * NF + tid] = red[tid] + red[2 * 16 * NF + tid] + red[4 * 16 * NF + tid] + red[6 * 16 * NF + tid];
        __syncthreads();
    };
    int cur_n = -1;
    f32x4 amu[STATS == 2 ? NF : 1], ars[STATS == 2 ? NF : 1];  // STATS == 2: (mean, rstd) of the lane's output channels, image cur_n
    float nsc[4], nnb[4];  // in_stats: (rstd, mean) of this thread's channel quad of image cur_in
    int cur_in = -1;
    const size_t out_row = (size_t)(up ? 2 : 1) * a.Wo * a.Cout * 4;  // bytes between this wave's consecutive rows
    P32Regs<NPF> R;
    int it = 0;
    // STATS: a workgroup takes a CONTIGUOUS range of tiles, so that an image is covered by a few workgroups and the statistics
    // finalize reads a few rows per image (with the strided order every workgroup touches every image: a row per pair, a memset and a
    // finalize that cost what the statistics pass they replace costs); otherwise the strided, XCD-contiguous order
    // ... and the ranges are dealt XCD-aware: workgroups b and b + 8 share an XCD (and its L2), so the logical range index is the
    // XCD-contiguous renumbering of the block index -- the ranges one L2 serves at a time are then neighbours (shared halo rows)
    const int chunk = STATS ? (total_tiles + G - 1) / G : 0;
    const int t_end = STATS ? min(total_tiles, (lb + 1) * chunk) : total_tiles;
    auto tile_of = [&](int i) { return STATS ? lb * chunk + i : p32_tile(i, P32_BX, G); };
    int t = tile_of(it);
    if (t < t_end) p32_fetch<NPF>(a, p, t, TH, tid, rel, vmask, R);
    while (t < t_end) {
        const int n = ntile == 1 ? t : (int)__umulhi((unsigned)t, p.m_ntile), tt = t - n * ntile;
        const int ty = a.tiles_x == 1 ? tt : (int)__umulhi((unsigned)tt, p.m_tx), tx = tt - ty * a.tiles_x;
        const int gy0 = ty * TH, gx0 = tx * P32_TW;
        if (STATS && n != cur_n) {
            if (cur_n >= 0) flush_stats(cur_n);
            cur_n = n;
            if (STATS == 2) {
#pragma unroll
                for (int f = 0; f < (STATS == 2 ? NF : 1); ++f) {
                    const float* st = a.aux_stats + ((size_t)n * a.Cout + 16 * f + 4 * g) * 2;
                    const f32x4 s0 = *reinterpret_cast<const f32x4*>(st), s1_ = *reinterpret_cast<const f32x4*>(st + 4);
                    amu[f] = f32x4{s0[0], s0[2], s1_[0], s1_[2]};
                    ars[f] = f32x4{s0[1], s0[3], s1_[1], s1_[3]};
                }
            }
        }
        if (a.in_stats && n != cur_in) {
            const float* st = a.in_stats + ((size_t)n * a.Cin + 4 * o) * 2;
#pragma unroll
            for (int c = 0; c < 4; ++c) { nsc[c] = st[2 * c + 1]; nnb[c] = st[2 * c]; }
            cur_in = n;
        }
#pragma unroll
        for (int k = 0; k < NPF; ++k)
            if (((vmask >> k) & 1) && !(a.dbg & 8)) {
                f32x4 w = R.v[k];
                if (a.in_stats) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) w[c] = fmaxf((w[c] - nnb[c]) * nsc[c], 0.f);  // norm_apply_kernel's arithmetic, bit for bit
                }
                if (!((R.okmask >> k) & 1)) w = f32x4{0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(patch + (unsigned)(((256 * k + tid) >> sh) * p.pixstride + 16 * o)) = w;
            }
        __syncthreads();
        const int tnext = tile_of(it + 1);
        if (tnext < t_end && !(a.dbg & 4)) p32_fetch<NPF>(a, p, tnext, TH, tid, rel, vmask, R);

        for (int sg = 0; sg < nseg; ++sg) {
            const int4 ci = *reinterpret_cast<const int4*>(smem + 4 * P32_MAX_STEPS + 16 * sg);
            const int s0 = __builtin_amdgcn_readfirstlane(ci.x), s1 = __builtin_amdgcn_readfirstlane(ci.y);
            const int oyc = __builtin_amdgcn_readfirstlane(ci.z), oxc = __builtin_amdgcn_readfirstlane(ci.w);
            f32x4 acc[RPW][NF];
            // STATS == 2: the raw tensor at the pixels this segment will store, in flight behind the whole K loop
            const int mul = up ? 2 : 1;
            const bool full_tile = gy0 + TH <= a.Gh && gx0 + P32_TW <= a.Gw && (a.Cout & 15) == 0;
            const size_t ybyte = ((((size_t)n * a.Ho + gy0 * mul + oyc) * a.Wo + gx0 * mul + oxc) * a.Cout) * 4;
            const unsigned out_off0 = (unsigned)(((RPW * wv * mul) * a.Wo + nl * mul) * a.Cout + 4 * g) * 4u;
            f32x4 av[STATS == 2 ? RPW : 1][STATS == 2 ? NF : 1];
            if (STATS == 2 && full_tile && !(a.dbg & 2)) {
                const char* abase = reinterpret_cast<const char*>(a.aux) + ybyte;
#pragma unroll
                for (int r = 0; r < RPW; ++r)
#pragma unroll
                    for (int f = 0; f < NF; ++f) av[STATS == 2 ? r : 0][STATS == 2 ? f : 0] = *reinterpret_cast<const f32x4*>(abase + r * out_row + out_off0 + 64 * f);
            }
            auto load_ko = [&](int s) -> unsigned { return reinterpret_cast<const unsigned*>(smem)[s]; };
            auto load_ops = [&](unsigned ko, int s, f32x4 (&bf)[RPW], f32x4 (&af)[NF]) {
#pragma unroll
                for (int r = 0; r < RPW; ++r) bf[r] = *reinterpret_cast<const f32x4*>(patch + base[r] + ko);
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    if (WLDS) af[f] = *reinterpret_cast<const f32x4*>(wlds_lane + (size_t)(s * NF + f) * 1024);
                    else af[f] = wglob[(size_t)(s * NF + f) * 64];
                }
            };
            auto mma_step = [&](const f32x4 (&bf)[RPW], const f32x4 (&af)[NF], auto from_bias) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int f = 0; f < NF; ++f)
#pragma unroll
                        for (int r = 0; r < RPW; ++r)
                            acc[r][f] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[f][j], bf[r][j],
                                                                             (decltype(from_bias)::value && j == 0) ? b4[f] : acc[r][f], 0, 0, 0);
            };
            auto clip = [&](int s) { return s < s1 ? s : s1 - 1; };  // past the end: re-read the last step (loaded, never used)
            f32x4 bA[RPW], aA[NF], bB[RPW], aB[NF];
            unsigned k0 = load_ko(s0), k1 = load_ko(clip(s0 + 1));
            load_ops(k0, s0, bA, aA);
            k0 = load_ko(clip(s0 + 2));
            load_ops(k1, clip(s0 + 1), bB, aB);
            mma_step(bA, aA, P32True{});  // accumulators start from the bias (the MFMA's C operand)
            int s = s0 + 1;  // invariant: B holds the operands of step s (if s < s1), k0 the offset of step s + 1
            if (a.dbg & 1) s = s1;  // experiments (MSTG_P32_DBG): 1 one K-step only, 2 no stores, 4 no patch fetch, 8 no patch commit
            for (; s + 1 < s1; s += 2) {
                k1 = load_ko(clip(s + 2));
                load_ops(k0, s + 1, bA, aA);
                mma_step(bB, aB, P32False{});
                k0 = load_ko(clip(s + 3));
                load_ops(k1, clip(s + 2), bB, aB);
                mma_step(bA, aA, P32False{});
            }
            if (s < s1) mma_step(bB, aB, P32False{});
            // ---- epilogue of this class: lane holds output channels 16f + 4g + {0..3} of compute-grid pixel (gy, gx0 + nl) --------
            if (a.dbg & 2) continue;
            if (full_tile) {
                char* ybase = reinterpret_cast<char*>(a.y) + ybyte;
#pragma unroll
                for (int r = 0; r < RPW; ++r)
#pragma unroll
                    for (int f = 0; f < NF; ++f) {
                        if (STATS == 1) {
#pragma unroll
                            for (int q = 0; q < 4; ++q) { const float dv = acc[r][f][q] - b4[f][q]; ssum[f][q] += dv; ssq[f][q] += dv * dv; }  // pivot = the channel's bias
                        }
                        *reinterpret_cast<f32x4*>(ybase + r * out_row + out_off0 + 64 * f) = acc[r][f];
                    }
                if (STATS == 2) {
#pragma unroll
                    for (int r = 0; r < RPW; ++r)
#pragma unroll
                        for (int f = 0; f < NF; ++f) {
                            const f32x4 xh = (av[STATS == 2 ? r : 0][STATS == 2 ? f : 0] - amu[STATS == 2 ? f : 0]) * ars[STATS == 2 ? f : 0];  // norm_partial_kernel<true>'s arithmetic
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const float gg = xh[q] > 0.f ? acc[r][f][q] : 0.f;
                                ssum[f][q] += gg;
                                ssq[f][q] += gg * xh[q];
                            }
                        }
                }
            } else {
#pragma unroll
                for (int r = 0; r < RPW; ++r) {
                    const int gy = gy0 + RPW * wv + r, gx = gx0 + nl;
                    if (gy < a.Gh && gx < a.Gw) {
                        const int oy = gy * mul + oyc, ox = gx * mul + oxc;
#pragma unroll
                        for (int f = 0; f < NF; ++f)
                            if (16 * f + 4 * g < a.Cout) {
                                const size_t oe = (((size_t)n * a.Ho + oy) * a.Wo + ox) * a.Cout + 16 * f + 4 * g;
                                if (STATS == 1) {
#pragma unroll
                                    for (int q = 0; q < 4; ++q) { const float dv = acc[r][f][q] - b4[f][q]; ssum[f][q] += dv; ssq[f][q] += dv * dv; }  // pivot = the channel's bias
                                }
                                if (STATS == 2) {
                                    const f32x4 xh = (*reinterpret_cast<const f32x4*>(a.aux + oe) - amu[STATS == 2 ? f : 0]) * ars[STATS == 2 ? f : 0];
#pragma unroll
                                    for (int q = 0; q < 4; ++q) {
                                        const float gg = xh[q] > 0.f ? acc[r][f][q] : 0.f;
                                        ssum[f][q] += gg;
                                        ssq[f][q] += gg * xh[q];
                                    }
                                }
                                *reinterpret_cast<f32x4*>(a.y + oe) = acc[r][f];
                            }
                    }
                }
            }
        }
        __syncthreads();  // every wave is done with the patch
        ++it;
        t = tnext;
    }
    if (STATS && cur_n >= 0) flush_stats(cur_n);
