// sf_icp_testhooks.hpp -- test hooks of the float64 numerical core (sf_test_linalg, sf_test_wave_reduce, sf_test_block_reduce,
// sf_test_reduce_partials; include/slamfusion.h).  Included by sf_icp.hip inside its anonymous namespace,
// after every other kernel (sf_cov.hpp included), so that none of them changes.  The kernels below CALL sf_linalg.hpp's svd3,
// kabsch_from_record, ldlt6 and vec6_to_mat4, sf_reduce.hpp's wave_reduce_*, block_reduce_store and reduce_partials, sf_jacobi.hpp's
// rsqrt_nr / jacobi_sym, sf_cov.hpp's recip_nr and that file's robust_weight as they are: no copy of a routine, no second implementation.  They
// stay in the ICP unit because robust_weight and the instantiations they pin (NREC_COV_*, SBLK) are ICP's.  Not part
// of the drop-in boundary and no reference counterpart (the reference calls Eigen::JacobiSVD and Open3D's solvers).
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
