// sf_icp_fused_body.inc -- the body of k_icp_fused<MODE, WINDOW, REUSE> and of its robust twin k_icp_fused_rob<WINDOW, REUSE>
// (sf_icp.hip), included inside both kernels for the reason given in sf_nn_red_body.inc.  In scope: the kernel's parameters,
// MODE, WINDOW, REUSE, `constexpr bool ROBUST` and the RobustArg `rk`.
    constexpr int NREC = MODE == 2 ? NREC_PLANE : NREC_P2P;
    const int b = blockIdx.y, bx = blockIdx.x;
    __shared__ IcpState S;
    __shared__ double rec[REC_STRIDE];
    __shared__ sf::WaveNN nn_ws[BLK / 64];
    __shared__ double stage[BLK / 64][32];
    __shared__ int bar_ok;
    for (int k = threadIdx.x; k < (int)(sizeof(IcpState) / 4); k += BLK) reinterpret_cast<uint32_t *>(&S)[k] = reinterpret_cast<const uint32_t *>(st + b)[k];
    __syncthreads();
    uint32_t *ctr = bar + 2 * b, *fin = bar + 2 * b + 1;
    double *const slab_even = partials + (size_t)b * nblocks * REC_STRIDE, *const slab_odd = partials + ((size_t)gridDim.y + b) * nblocks * REC_STRIDE; // used in turn: see k_ref_fused
    const int slot = bx * BLK + (int)threadIdx.x;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool have = slot < n;
    double x0 = 0.0, y0 = 0.0, z0 = 0.0;
    if (have) {
        const size_t o = (size_t)b * n + (size_t)slot;
        x0 = X0x[o]; y0 = X0y[o]; z0 = X0z[o];
    }
    float4 c0 = make_float4(0.f, 0.f, 0.f, 0.f), c1 = c0, c2 = c0; // the lane's neighbour cache (k_nn_red keeps it in memory)
    uint32_t passed = 0;
    bool alive = true;
    const int launches = MODE == 1 ? K + 1 : K; // what the launch list enqueues
    for (int it = 0; it < launches && !S.done; ++it) {
        double sx = 0, sy = 0, sz = 0;
        float qx = 0.f, qy = 0.f, qz = 0.f;
        if (have) {
            sx = S.T[0] * x0 + S.T[1] * y0 + S.T[2] * z0 + S.T[3];
            sy = S.T[4] * x0 + S.T[5] * y0 + S.T[6] * z0 + S.T[7];
            sz = S.T[8] * x0 + S.T[9] * y0 + S.T[10] * z0 + S.T[11];
            qx = (float)sx; qy = (float)sy; qz = (float)sz;
        }
        sf::NNHit hit;
        float4 tn;
        sf::NNHit seed;
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool live = REUSE && S.n_research > 0;
        const bool need = reuse_certificate_pos(have, qx, qy, qz, thr, live ? c0 : z4, live ? c1 : z4, live ? c2 : z4, hit, tn, seed);
        if (__ballot(need) != 0ull) {
            const sf::NNHit h = sf::nn_search_wave<WINDOW>(g, w, need, qx, qy, qz, thr, &nn_ws[wv], seed);
            if (need) {
                hit = h;
                if (MODE == 2 && h.j >= 0) tn = g.nrm[h.j];
                if (REUSE) {
                    c0 = make_float4(qx, qy, qz, sqrtf(h.lb2));
                    c1 = make_float4(h.px, h.py, h.pz, __int_as_float(h.j));
                    c2 = tn;
                }
            }
        }
        LanePair P;
        P.sx = sx; P.sy = sy; P.sz = sz;
        P.px = hit.px; P.py = hit.py; P.pz = hit.pz;
        P.tn = tn;
        P.ok = hit.j >= 0;
        const PairTerms T = pair_terms<MODE>(P);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            double v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = 0.0;
            if constexpr (ROBUST) add_half_robust(T, h, v, robust_weight(rk, T.r));
            else add_half<MODE>(T, h, v);
            if (MODE == 1 && h == 1) {
                const double t1 = wave_reduce_1(v[0]);
                if (lane == 0) stage[wv][16] = t1;
            } else {
                const double t0 = wave_reduce_16(v);
                if ((lane & 3) == 0) stage[wv][16 * h + (lane >> 2)] = t0;
            }
        }
        __syncthreads();
        double *slab = (passed & 1u) ? slab_odd : slab_even;
        if (threadIdx.x < NREC) {
            const int c = threadIdx.x;
            slab[(size_t)bx * REC_STRIDE + c] = ((stage[0][c] + stage[1][c]) + stage[2][c]) + stage[3][c];
        }
        ++passed;
        alive = ref_grid_barrier(ctr, passed * (uint32_t)nblocks, &bar_ok);
        if (!alive) break;
        reduce_partials<NREC, BLK>(slab, nblocks, rec);
        if (threadIdx.x == 0) {
            for (int c = 0; c < NREC; ++c) S.rec[c] = rec[c];
            if (MODE == 1) solve_o3d(&S, rec, n, 0, K);
            else solve_plane(&S, rec, n, K);
        }
        __syncthreads();
    }
    __syncthreads();
    if (!alive) {
        if (threadIdx.x == 0) {
            atomicOr(&st[b].flags, SF_ICP_FLAG_BARRIER_TIMEOUT);
            if (host_out) host_out[b].flags = SF_ICP_FLAG_BARRIER_TIMEOUT;
        }
        return;
    }
    if (bx == 0)
        for (int k = threadIdx.x; k < (int)(sizeof(IcpState) / 4); k += BLK) {
            const uint32_t v = reinterpret_cast<const uint32_t *>(&S)[k];
            reinterpret_cast<uint32_t *>(st + b)[k] = v;
            if (host_out) reinterpret_cast<uint32_t *>(host_out + b)[k] = v;
        }
    if (threadIdx.x == 0) {
        const uint32_t left = __hip_atomic_fetch_add(fin, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (left == (uint32_t)nblocks - 1u) {
            __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(fin, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
