// sf_nn_red_body.inc -- the body of k_nn_red<MODE, WINDOW, SHARD, Q> and of its robust twin k_nn_red_rob<WINDOW, SHARD, Q>
// (sf_icp.hip), included inside both kernels so that the plain kernel compiles to exactly the code it had before the twin
// existed (a shared __device__ body changes its instruction schedule).  In scope: the kernel's parameters, MODE, WINDOW,
// SHARD, Q, `constexpr bool ROBUST` and the RobustArg `rk` (the plain kernel discards every branch that names it).
    constexpr int NREC = MODE == 2 ? NREC_PLANE : NREC_P2P;
    // XCD-aware placement: workgroups are dealt round-robin to the 8 XCDs in launch order, so
    // linear id L runs on XCD L % 8.  Each XCD sweeps its own CONTIGUOUS eighth of the chunks
    // (chunk = 256 * Q consecutive queries of a scan), all scans of the batch adjacent in time:
    // with cell-ordered queries, chunk c of every scan covers about the same stretch of the map (to
    // within a chunk or so), so neighbouring chunks must meet in the same L2.  grid.x is padded
    // to a multiple of 8.
    const int L = blockIdx.y * gridDim.x + blockIdx.x;
    const int kk = L >> 3;
    const int b = kk % (int)gridDim.y;
    const int bx = (L & 7) * ((int)gridDim.x >> 3) + kk / (int)gridDim.y;
    if (bx >= nblocks) return;
    const IcpState *S = st + b;
    if (S->done) return;
    // sharded: X0x/y/z are this rank's compact arrays of owned-query candidates (slab widened by
    // the margin at the pose the arrays were built at, cell-ordered, scan b at [own_off[b], own_off[b+1]));
    // the exact slab predicate is still applied per lane
    const int n_live = SHARD ? (int)(own_off[b + 1] - own_off[b]) : n;
    if (SHARD && bx * (BLK * Q) >= n_live) return; // k_reduce_only reads only the rows that exist
    __shared__ sf::WaveNN nn_ws[BLK / 64];
    __shared__ double stage[BLK / 64][32];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // the pairs are kept, not their terms (13 against 36 registers per query across the next search); the terms are
    // formed once per half below
#ifdef SF_PHASE_TRACE
    sf::PhaseClock pclk, *pc = &pclk;
    pclk.start();
#else
    sf::PhaseClock *pc = nullptr;
#endif
    LanePair P[Q];
    // Q > 1, from the launch on in which most waves only verify: the loads of ALL the lane's queries go out together (one
    // round trip per wave, Q times the bytes in flight) and, if every lane of the wave certifies every one of its
    // queries, the pairs come straight from them.  A wave with anything left to search drops what it loaded and takes the
    // queries one after the other as always -- the same pairs either way, so which path a wave takes changes no bit.
    bool fast = false;
    if (Q > 1 && qcache != nullptr && S->cache_live != 0 && S->n_research >= VERIFY_FROM_SEARCH) {
        const float m_now = (float)S->motion;
        bool any_need = false;
#pragma unroll
        for (int u = 0; u < Q; ++u) {
            const int slot = bx * (BLK * Q) + u * BLK + (int)threadIdx.x;
            const QueryIn q = query_in<MODE, SHARD>(X0x, X0y, X0z, n, b, S, xlo, xhi, own_off, qcache, cache_n, true, slot, n_live);
            sf::NNHit hit, seed;
            float4 tn;
            any_need = reuse_certificate(q.valid, q.qx, q.qy, q.qz, thr, m_now, q.e, q.c1, q.c2, hit, tn, seed) || any_need;
            P[u] = make_pair(q, hit, tn);
        }
        fast = __ballot(any_need) == 0ull;
    }
    if (!fast) {
        asm volatile("" ::: "memory"); // nothing loaded above stays live across the searches below
#pragma unroll
        for (int u = 0; u < Q; ++u) {
            const int slot = bx * (BLK * Q) + u * BLK + (int)threadIdx.x;
            P[u] = nn_pair<MODE, WINDOW, SHARD>(g, w, X0x, X0y, X0z, n, b, S, thr, xlo, xhi, own_off, qcache, cache_n, slot, n_live, &nn_ws[wv], stats, pc);
        }
    }
    // the lane's pairs added, reduced over the wave in two halves of 16 values (keeps the live
    // registers low enough for 4+ waves per SIMD), staged per wave in LDS
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        double v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = 0.0;
#pragma unroll
        for (int u = 0; u < Q; ++u) {
            const PairTerms t = pair_terms<MODE>(P[u]);
            if constexpr (ROBUST) add_half_robust(t, h, v, robust_weight(rk, t.r));
            else add_half<MODE>(t, h, v);
        }
        if (MODE == 1 && h == 1) {
            const double t1 = wave_reduce_1(v[0]);
            if (lane == 0) stage[wv][16] = t1;
        } else {
            const double t0 = wave_reduce_16(v);
            if ((lane & 3) == 0) stage[wv][16 * h + (lane >> 2)] = t0;
        }
    }
    SF_PH(pc, 7);
    __syncthreads();
    if (threadIdx.x < NREC) {
        const int c = threadIdx.x;
        double *dst = partials + ((size_t)b * nblocks + bx) * REC_STRIDE;
        dst[c] = ((stage[0][c] + stage[1][c]) + stage[2][c]) + stage[3][c];
    }
#ifdef SF_PHASE_TRACE
    SF_PH(pc, 8);
    pclk.count(14, 1u);
    if (lane == 0) {
        unsigned long long *dstp = g_phase_trace + (size_t)(L & (sf::PH_SHARDS - 1)) * sf::PH_SLOTS;
        for (int i = 0; i < sf::PH_SLOTS; ++i) atomicAdd(&dstp[i], (unsigned long long)pclk.acc[i]);
    }
#endif
