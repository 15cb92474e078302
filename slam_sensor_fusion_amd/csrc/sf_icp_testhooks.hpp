// sf_icp_testhooks.hpp -- test hooks of the float64 numerical core (sf_test_linalg, sf_test_wave_reduce, sf_test_block_reduce,
// sf_test_reduce_partials; include/slamfusion.h).  Included by sf_icp.hip inside its anonymous namespace,
// after every other kernel (sf_cov.hpp included), so that none of them changes.  The kernels below CALL sf_linalg.hpp's svd3,
// kabsch_from_record, ldlt6 and vec6_to_mat4, sf_reduce.hpp's wave_reduce_*, block_reduce_store and reduce_partials, sf_jacobi.hpp's
// rsqrt_nr / jacobi_sym, sf_cov.hpp's recip_nr and that file's robust_weight as they are: no copy of a routine, no second implementation.  They
// stay in the ICP unit because robust_weight and the instantiations they pin (NREC_COV_*, SBLK) are ICP's.  Not part
// of the drop-in boundary and no reference counterpart (the reference calls Eigen::JacobiSVD and Open3D's solvers).
// At the end of the file, host code alone: test_download_cache_run, the read-only copy of the launch list's neighbour cache behind
// sf_icp_test_download_cache.
//
// sf_test_linalg runs one case per thread in workgroups of 64: one lane working on its own little matrix is how production
// runs these routines.  The reductions run in ONE workgroup of BLK (wave and block forms) or NT (reduce_partials) threads.

constexpr int TEST_LBLK = 64;
constexpr int64_t TEST_MAX_CASES = (int64_t)1 << 20;
constexpr int TEST_MAX_ROWS = 1 << 16;

enum { TEST_OP_RSQRT = 0, TEST_OP_SVD3, TEST_OP_KABSCH, TEST_OP_LDLT6, TEST_OP_VEC6, TEST_OP_JACOBI3, TEST_OP_JACOBI6, TEST_OP_ROBUST, TEST_OP_EIGVEC, TEST_OP_COUNT };
// doubles a case reads / writes, by op (TEST_OP_EIGVEC runs in sf_map.hip)
constexpr int TEST_OP_IN[TEST_OP_COUNT] = {1, 9, REC_STRIDE, 42, 6, 9, 36, 3, 9};
constexpr int TEST_OP_OUT[TEST_OP_COUNT] = {2, 21, 16, 7, 16, 13, 43, 1, 3};

template <int N>
__device__ __forceinline__ void test_jacobi_case(const double *__restrict__ a, double *__restrict__ o)
{
    double A[N * N], V[N * N];
#pragma unroll
    for (int i = 0; i < N * N; ++i) A[i] = a[i];
    const int sweeps = jacobi_sym<N>(A, V);
#pragma unroll
    for (int k = 0; k < N; ++k) o[k] = A[(N + 1) * k];
#pragma unroll
    for (int i = 0; i < N * N; ++i) o[N + i] = V[i];
    o[N + N * N] = (double)sweeps;
}

template <int OP>
__global__ __launch_bounds__(TEST_LBLK) void k_test_linalg(const double *__restrict__ in, int in_stride, int64_t cases, double *__restrict__ out, int out_stride)
{
    const int64_t i = (int64_t)blockIdx.x * TEST_LBLK + threadIdx.x;
    if (i >= cases) return;
    const double *a = in + (size_t)i * in_stride;
    double *o = out + (size_t)i * out_stride;
    if constexpr (OP == TEST_OP_RSQRT) {
        o[0] = rsqrt_nr(a[0]);
        o[1] = recip_nr(a[0]);
    } else if constexpr (OP == TEST_OP_SVD3) {
        double A[9], U[9], S[3], V[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) A[k] = a[k];
        svd3(A, U, S, V);
#pragma unroll
        for (int k = 0; k < 9; ++k) { o[k] = U[k]; o[12 + k] = V[k]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) o[9 + k] = S[k];
    } else if constexpr (OP == TEST_OP_KABSCH) {
        double T[16];
        kabsch_from_record(a, T);
#pragma unroll
        for (int k = 0; k < 16; ++k) o[k] = T[k];
    } else if constexpr (OP == TEST_OP_LDLT6) {
        double A[36], b[6], x[6] = {0, 0, 0, 0, 0, 0}; // (ldlt6 leaves x alone when it refuses)
#pragma unroll
        for (int k = 0; k < 36; ++k) A[k] = a[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) b[k] = a[36 + k];
        const int rc = ldlt6(A, b, x);
        o[0] = (double)rc;
#pragma unroll
        for (int k = 0; k < 6; ++k) o[1 + k] = x[k];
    } else if constexpr (OP == TEST_OP_VEC6) {
        double v[6], T[16];
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = a[k];
        vec6_to_mat4(v, T);
#pragma unroll
        for (int k = 0; k < 16; ++k) o[k] = T[k];
    } else if constexpr (OP == TEST_OP_JACOBI3) {
        test_jacobi_case<3>(a, o);
    } else if constexpr (OP == TEST_OP_JACOBI6) {
        test_jacobi_case<6>(a, o);
    } else {
        const RobustArg rk = {(int)a[0], a[1]};
        o[0] = robust_weight(rk, a[2]);
    }
}

// every lane's return value of wave_reduce_<WIDTH>: in[BLK][WIDTH] -> out[BLK]
template <int WIDTH>
__global__ __launch_bounds__(BLK) void k_test_wave_reduce(const double *__restrict__ in, double *__restrict__ out)
{
    const double *a = in + (size_t)threadIdx.x * WIDTH;
    if constexpr (WIDTH == 1) {
        out[threadIdx.x] = wave_reduce_1(a[0]);
    } else {
        double v[WIDTH];
#pragma unroll
        for (int k = 0; k < WIDTH; ++k) v[k] = a[k];
        if constexpr (WIDTH == 16) out[threadIdx.x] = wave_reduce_16(v);
        else out[threadIdx.x] = wave_reduce_32(v);
    }
}

template <int NREC>
__global__ __launch_bounds__(BLK) void k_test_block_reduce(const double *__restrict__ in, double *__restrict__ out)
{
    double acc[NREC];
#pragma unroll
    for (int k = 0; k < NREC; ++k) acc[k] = in[(size_t)threadIdx.x * NREC + k];
    block_reduce_store<NREC>(acc, out);
}

template <int NREC, int NT>
__global__ __launch_bounds__(NT) void k_test_reduce_partials(const double *__restrict__ part, int nblocks, double *__restrict__ out)
{
    __shared__ double rec[REC_STRIDE];
    reduce_partials<NREC, NT>(part, nblocks, rec);
    if (threadIdx.x < REC_STRIDE) out[threadIdx.x] = rec[threadIdx.x];
}

// host array -> device, launch(d_in, d_out), device -> host array; out_init: the device result starts as the caller's array
template <class Launch>
int test_round_trip(sf_ctx *ctx, const double *in, size_t n_in, double *out, size_t n_out, bool out_init, Launch launch)
{
    SF_HIP(hipSetDevice(ctx->device));
    sf::DevBuf din, dout; // freed on every path
    SF_TRY(din.reserve(sizeof(double) * (n_in ? n_in : 1)));
    SF_TRY(dout.reserve(sizeof(double) * (n_out ? n_out : 1)));
    hipStream_t st = ctx->stream;
    if (n_in) SF_TRY(sf::upload_staged(ctx, din.p, in, sizeof(double) * n_in));
    if (n_out && out_init) SF_TRY(sf::upload_staged(ctx, dout.p, out, sizeof(double) * n_out));
    launch(din.as<double>(), dout.as<double>(), st);
    SF_HIP(hipGetLastError());
    if (n_out) SF_HIP(hipMemcpyAsync(out, dout.p, sizeof(double) * n_out, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    return SF_OK;
}

template <int OP>
void test_launch_linalg(const double *in, int in_stride, int64_t cases, double *out, int out_stride, hipStream_t st)
{
    hipLaunchKernelGGL(k_test_linalg<OP>, dim3(nblk(cases, TEST_LBLK)), dim3(TEST_LBLK), 0, st, in, in_stride, cases, out, out_stride);
}

int test_linalg_run(sf_ctx *ctx, int op, const double *in, int in_stride, int64_t cases, double *out, int out_stride)
{
    if (cases == 0) return SF_OK;
    return test_round_trip(ctx, in, (size_t)cases * in_stride, out, (size_t)cases * out_stride, true, [&](const double *di, double *dd, hipStream_t st) {
        switch (op) {
        case TEST_OP_RSQRT: test_launch_linalg<TEST_OP_RSQRT>(di, in_stride, cases, dd, out_stride, st); break;
        case TEST_OP_SVD3: test_launch_linalg<TEST_OP_SVD3>(di, in_stride, cases, dd, out_stride, st); break;
        case TEST_OP_KABSCH: test_launch_linalg<TEST_OP_KABSCH>(di, in_stride, cases, dd, out_stride, st); break;
        case TEST_OP_LDLT6: test_launch_linalg<TEST_OP_LDLT6>(di, in_stride, cases, dd, out_stride, st); break;
        case TEST_OP_VEC6: test_launch_linalg<TEST_OP_VEC6>(di, in_stride, cases, dd, out_stride, st); break;
        case TEST_OP_JACOBI3: test_launch_linalg<TEST_OP_JACOBI3>(di, in_stride, cases, dd, out_stride, st); break;
        case TEST_OP_JACOBI6: test_launch_linalg<TEST_OP_JACOBI6>(di, in_stride, cases, dd, out_stride, st); break;
        default: test_launch_linalg<TEST_OP_ROBUST>(di, in_stride, cases, dd, out_stride, st); break;
        }
    });
}

int test_wave_reduce_run(sf_ctx *ctx, int width, const double *in, double *out)
{
    return test_round_trip(ctx, in, (size_t)BLK * width, out, BLK, false, [&](const double *di, double *dd, hipStream_t st) {
        if (width == 1) hipLaunchKernelGGL(k_test_wave_reduce<1>, dim3(1), dim3(BLK), 0, st, di, dd);
        else if (width == 16) hipLaunchKernelGGL(k_test_wave_reduce<16>, dim3(1), dim3(BLK), 0, st, di, dd);
        else hipLaunchKernelGGL(k_test_wave_reduce<32>, dim3(1), dim3(BLK), 0, st, di, dd);
    });
}

int test_block_reduce_run(sf_ctx *ctx, int nrec, const double *in, double *out)
{
    // out goes to the device first: what block_reduce_store leaves alone (components >= nrec) comes back as it went in
    return test_round_trip(ctx, in, (size_t)BLK * nrec, out, REC_STRIDE, true, [&](const double *di, double *dd, hipStream_t st) {
        if (nrec == NREC_P2P) hipLaunchKernelGGL(k_test_block_reduce<NREC_P2P>, dim3(1), dim3(BLK), 0, st, di, dd);
        else hipLaunchKernelGGL(k_test_block_reduce<NREC_PLANE>, dim3(1), dim3(BLK), 0, st, di, dd);
    });
}

// the instantiations the library itself uses: <17 | 30, 1024> (k_reduce_solve, k_p2p_*), <17 | 30, 256> (the single-launch
// forms, the frozen solve) and <11 | 24, 256> (k_cov_solve)
inline bool test_reduce_partials_known(int nrec, int nt)
{
    if (nt == SBLK) return nrec == NREC_COV_P2P || nrec == NREC_P2P || nrec == NREC_COV_PLANE || nrec == NREC_PLANE;
    return nt == RBLK && (nrec == NREC_P2P || nrec == NREC_PLANE);
}

int test_reduce_partials_run(sf_ctx *ctx, int nrec, int nt, const double *part, int nblocks, double *out)
{
    return test_round_trip(ctx, part, (size_t)nblocks * REC_STRIDE, out, REC_STRIDE, false, [&](const double *di, double *dd, hipStream_t st) {
#define SF_TEST_RP(NREC, NT)                                                                                              \
    if (nrec == NREC && nt == NT) hipLaunchKernelGGL((k_test_reduce_partials<NREC, NT>), dim3(1), dim3(NT), 0, st, di, nblocks, dd)
        SF_TEST_RP(NREC_COV_P2P, SBLK);
        SF_TEST_RP(NREC_P2P, SBLK);
        SF_TEST_RP(NREC_COV_PLANE, SBLK);
        SF_TEST_RP(NREC_PLANE, SBLK);
        SF_TEST_RP(NREC_P2P, RBLK);
        SF_TEST_RP(NREC_PLANE, RBLK);
#undef SF_TEST_RP
    });
}

// ------------------------------------------------------------------ the neighbour cache of the last alignment, read back
// sf_icp_test_download_cache (include/slamfusion.h): host code alone.  What the launch list's kernels left in
// the lane of the latest alignment -- per entry the query it belongs to, the cached neighbour, its index position and E, and the
// scan's pose, motion bound and counters -- copied out after a stream synchronise.  No launch, no write on the device, no member
// of the object changed (the object comes in const).  A template because struct sf_icp (sf_icp_object.hpp) is declared behind this
// file; it is instantiated once, by the entry point at the end of sf_icp.hip.
template <class Icp>
int test_download_cache_run(const Icp *icp, int b, int64_t cap, float *x0, int32_t *orig, float *nbr, int32_t *j, float *e, sf_icp_cache_info *info)
{
    const auto &ln = icp->cur();
    const auto &M = ln.meta;
    // the launch list, enqueued whole, with the neighbour reuse on: the single launch (its cache lives in registers) and REF_CPP
    // leave the schedule of the lane undescribed (zeros)
    SF_CHECK(M.valid && M.batch > 0 && !icp->last_fused && !icp->shard && (M.mode == SF_ICP_O3D_P2P || M.mode == SF_ICP_P2PLANE) && M.sched.mode == M.mode && M.sched.whole &&
                 M.sched.reuse,
             SF_ERR_STATE, "sf_icp_test_download_cache: the latest alignment of this object is no O3D_P2P / P2PLANE launch list with neighbour reuse (none yet, REF_CPP, the single launch, sharded, stepped or reuse off)");
    const auto &ss = icp->srcs[M.src_set];
    SF_CHECK(ss.have_source && ss.batch == M.batch && ss.n > 0 && ln.qcache.p && ln.state.p && icp->cache_n >= ss.n * ss.batch, SF_ERR_STATE,
             "sf_icp_test_download_cache: the source or the cache of the latest alignment is gone");
    SF_CHECK(b >= 0 && b < M.batch, SF_ERR_INVALID, "sf_icp_test_download_cache: scan %d outside [0, %d)", b, M.batch);
    const int64_t n = ss.n;
    const bool sized = cap == 0 && !x0 && !orig && !nbr && !j && !e; // the size query: info alone
    SF_CHECK(sized || (cap >= n && x0 && nbr && j && e), SF_ERR_INVALID, "sf_icp_test_download_cache: buffers of %lld entries (or NULL) for a scan of %lld", (long long)cap, (long long)n);
    SF_CHECK(!icp->ordered || ln.Xq.p, SF_ERR_STATE, "sf_icp_test_download_cache: the ordered queries are gone");
    SF_HIP(hipSetDevice(icp->ctx->device));
    hipStream_t st = icp->ctx->stream; // (waits for every lane's alignment: LaneScope)
    SF_HIP(hipStreamSynchronize(st));
    IcpState S;
    SF_HIP(hipMemcpyAsync(static_cast<void *>(&S), static_cast<const IcpState *>(ln.state.p) + b, sizeof(IcpState), hipMemcpyDeviceToHost, st));
    const size_t first = (size_t)b * (size_t)n, cn = (size_t)icp->cache_n;
    const bool tiled = icp->ordered && icp->tile_on && ln.qidx.p; // the tile sort keeps the ids of its ordered queries; the move kernel of the plain order keeps none
    std::vector<float> xs, es;
    std::vector<float4> c1, c2;
    std::vector<uint32_t> ids;
    if (!sized) {
        xs.resize(3 * (size_t)n);
        c1.resize((size_t)n);
        const float *X = static_cast<const float *>(icp->ordered ? ln.Xq.p : ss.X0.p);
        for (int a = 0; a < 3; ++a)
            SF_HIP(hipMemcpyAsync(xs.data() + (size_t)a * n, X + (size_t)a * (size_t)ss.plane + first, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, st));
        const float4 *qc = static_cast<const float4 *>(ln.qcache.p);
        SF_HIP(hipMemcpyAsync(c1.data(), qc + first, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, st));
        if (M.mode == SF_ICP_P2PLANE) { // (neighbour's normal, E)
            c2.resize((size_t)n);
            SF_HIP(hipMemcpyAsync(c2.data(), qc + cn + first, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, st));
        } else { // E alone, as floats
            es.resize((size_t)n);
            SF_HIP(hipMemcpyAsync(es.data(), reinterpret_cast<const float *>(qc + cn) + first, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, st));
        }
        if (tiled && orig) {
            ids.resize((size_t)n);
            SF_HIP(hipMemcpyAsync(ids.data(), static_cast<const uint32_t *>(ln.qidx.p) + first, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
        }
    }
    SF_HIP(hipStreamSynchronize(st));
    for (int64_t i = 0; i < (sized ? 0 : n); ++i) {
        for (int a = 0; a < 3; ++a) x0[3 * i + a] = xs[(size_t)a * n + i];
        nbr[3 * i] = c1[i].x; nbr[3 * i + 1] = c1[i].y; nbr[3 * i + 2] = c1[i].z;
        std::memcpy(&j[i], &c1[i].w, sizeof(int32_t));
        e[i] = M.mode == SF_ICP_P2PLANE ? c2[i].w : es[i];
        if (orig) orig[i] = !icp->ordered ? (int32_t)i : tiled ? (int32_t)((int64_t)ids[i] - (int64_t)first) : -1;
    }
    if (info) {
        std::memcpy(info->T, S.T, sizeof(double) * 16);
        info->motion = S.motion;
        info->n = n;
        info->batch = M.batch; info->mode = M.mode;
        info->cache_live = S.cache_live; info->n_research = S.n_research; info->iterations = S.iterations;
        info->ordered = !icp->ordered ? 0 : tiled ? 2 : 1;
    }
    return SF_OK;
}
