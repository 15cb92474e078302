// sf_cov.hpp -- pose covariance and degeneracy of a finished alignment (sf_icp_set_covariance, include/slamfusion.h).
// Included by sf_icp.hip inside its anonymous namespace, after every other kernel, so that none of them changes: it uses
// that file's IcpState, query_in and robust_weight, sf_reduce.hpp's wave_reduce_16 and reduce_partials and sf_jacobi.hpp's rsqrt_nr
// and jacobi_sym as they are.  The first three are ICP's own, which is why this stays a fragment of that unit.
//
// Two launches behind the last iteration of an alignment, on its stream:
//   k_nn_cov<MODE, WINDOW>  one lane per source point: s = T x (float64) at the FINAL pose read from IcpState, the exact
//                           wave-cooperative search of sf_nn.hpp on the float32 rounding of s, the mode's own acceptance
//                           predicate, then the pair's terms in float64; wave butterfly, one 32-double row per workgroup.
//                           P2PLANE: the 21 unique entries of w J^T J, w r^2, w and the count (24 sums).  REF_CPP / O3D_P2P:
//                           n, sum s, the 6 unique entries of sum s s^T and sum |r|^2 (11 sums) -- H follows in closed form.
//   k_cov_solve<MODE>       one workgroup per scan: the rows summed in reduce_partials' fixed order (the same bits run to
//                           run, and whichever path produced the pose -- both walk the same query arrays), then on one lane
//                           H, the 6x6 Jacobi eigen-solve, cov, the two 3x3 solves of the marginals, the flags.
// One query per lane for every scan size: rows of 256 queries (SrcSet::nblocks of them), wide scans included.

constexpr int NREC_COV_PLANE = 24;
constexpr int NREC_COV_P2P = 11;
constexpr int COV_SBLK = 256; // k_cov_solve: one wave per SIMD may use the whole register file (the 6x6 solve keeps ~100 doubles live)

struct CovArg { double sensor_sigma, thr_t, thr_r, infl_t, infl_r; };

template <int MODE, bool WINDOW>
__global__ __launch_bounds__(BLK, NN_RED_WAVES) void k_nn_cov(SfGrid g, SfWindow w, const SfWindow *__restrict__ wdev, const float *__restrict__ X0x, const float *__restrict__ X0y,
                                                              const float *__restrict__ X0z, int n, const int *__restrict__ n_dev, const IcpState *__restrict__ st, float thr,
                                                              double *__restrict__ part, int nblocks, RobustArg rk)
{
    constexpr int NREC = MODE == 2 ? NREC_COV_PLANE : NREC_COV_P2P;
    if (WINDOW && wdev) w = *wdev; // REF_CPP on the launch list: the map crop lives in device memory (a captured graph does not bake it in)
    if (n_dev) n = *n_dev;         // single scan, REF_CPP: the point count in device memory
    // the XCD placement of k_nn_red: chunk c of every scan of the batch on one XCD (grid.x is padded to a multiple of 8)
    const int L = blockIdx.y * gridDim.x + blockIdx.x;
    const int kk = L >> 3;
    const int b = kk % (int)gridDim.y;
    const int bx = (L & 7) * ((int)gridDim.x >> 3) + kk / (int)gridDim.y;
    if (bx >= nblocks) return;
    const IcpState *S = st + b; // (a scan that stopped early is evaluated like any other: at the pose it stopped at)
    __shared__ sf::WaveNN nn_ws[BLK / 64];
    __shared__ double stage[BLK / 64][32];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int slot = bx * BLK + (int)threadIdx.x;
    const QueryIn q = query_in<1, false>(X0x, X0y, X0z, n, b, S, 0.0f, 0.0f, nullptr, nullptr, 0, false, slot, n);
    // every lane takes part in the search (lanes without a query still execute other lanes' tasks)
    const sf::NNHit hit = sf::nn_search_wave<WINDOW>(g, w, q.valid, q.qx, q.qy, q.qz, thr, &nn_ws[wv]);
    const bool ok = q.valid && hit.j >= 0;
    // lanes without a pair contribute exact zeros (a non-finite dead query must not turn 0 * s into NaN)
    const double cnt = ok ? 1.0 : 0.0;
    const double sx = ok ? q.sx : 0.0, sy = ok ? q.sy : 0.0, sz = ok ? q.sz : 0.0;
    const double ex = sx - (double)(ok ? hit.px : 0.0f), ey = sy - (double)(ok ? hit.py : 0.0f), ez = sz - (double)(ok ? hit.pz : 0.0f);
    if (MODE == 2) {
        float4 tn = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok) tn = g.nrm[hit.j];
        const double nx = (double)tn.x, ny = (double)tn.y, nz = (double)tn.z;
        const double r = fma(ex, nx, fma(ey, ny, ez * nz));
        const double wgt = ok ? robust_weight(rk, r) : 0.0;
        double J[6], Jw[6];
        J[0] = fma(sy, nz, -(sz * ny)); J[1] = fma(sz, nx, -(sx * nz)); J[2] = fma(sx, ny, -(sy * nx));
        J[3] = nx; J[4] = ny; J[5] = nz;
#pragma unroll
        for (int a = 0; a < 6; ++a) Jw[a] = wgt * J[a];
        // row[0..20] = w J^T J (0,0) (0,1) .. (0,5) (1,1) .. (5,5), row[21] = w r^2, row[22] = w, row[23] = 1; reduced over the
        // wave in two halves of 16 values, as k_nn_red does
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            double v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = 0.0;
            int k = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
#pragma unroll
                for (int c = a; c < 6; ++c) {
                    if ((k >> 4) == h) v[k & 15] = Jw[a] * J[c];
                    ++k;
                }
            }
            if (h == 1) { v[5] = wgt * r * r; v[6] = wgt; v[7] = cnt; }
            const double t0 = wave_reduce_16(v);
            if ((lane & 3) == 0) stage[wv][16 * h + (lane >> 2)] = t0;
        }
    } else {
        double v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = 0.0;
        v[0] = cnt;
        v[1] = sx; v[2] = sy; v[3] = sz;
        v[4] = sx * sx; v[5] = sx * sy; v[6] = sx * sz; v[7] = sy * sy; v[8] = sy * sz; v[9] = sz * sz;
        v[10] = fma(ex, ex, fma(ey, ey, ez * ez));
        const double t0 = wave_reduce_16(v);
        if ((lane & 3) == 0) stage[wv][lane >> 2] = t0;
    }
    __syncthreads();
    if (threadIdx.x < NREC) {
        const int c = threadIdx.x;
        part[((size_t)b * nblocks + bx) * REC_STRIDE + c] = ((stage[0][c] + stage[1][c]) + stage[2][c]) + stage[3][c];
    }
}

// (jacobi_sym<N>: sf_jacobi.hpp, included by sf_icp.hip beside rsqrt_nr)

__device__ __forceinline__ double recip_nr(double x) // 1 / x within 5 ulp for x in rsqrt_nr's domain (normal, positive, finite): no divide expansion on the one working lane
{
    const double y = rsqrt_nr(x);
    return y * y;
}

template <int A, int B>
__device__ __forceinline__ void order3(double (&val)[3], double (&vec)[9])
{
    if (val[B] < val[A]) {
        double t = val[A]; val[A] = val[B]; val[B] = t;
#pragma unroll
        for (int i = 0; i < 3; ++i) { t = vec[3 * A + i]; vec[3 * A + i] = vec[3 * B + i]; vec[3 * B + i] = t; }
    }
}

// eigen-pairs of the inverse of a marginal (a 3x3 diagonal block C of cov / sigma2) -> the marginal information's eigenvalues
// ascending, divided by W, and its eigenvectors as rows; flagged directions inflate the block of cov at offset O
template <int O>
__device__ __forceinline__ bool marginal_info(const double (&C)[36], double inv_w, double thr, double infl, double *__restrict__ info_out, double *__restrict__ dir_out,
                                              double (&cov)[36])
{
    double M[9], U[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[3 * i + j] = C[6 * (O + i) + O + j];
    jacobi_sym<3>(M, U);
    double val[3], vec[9]; // vec: eigenvectors as rows
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        val[k] = recip_nr(M[4 * k]) * inv_w; // (C is positive definite: every eigenvalue of H was clamped from below)
#pragma unroll
        for (int i = 0; i < 3; ++i) vec[3 * k + i] = U[3 * i + k];
    }
    order3<0, 1>(val, vec);
    order3<1, 2>(val, vec);
    order3<0, 1>(val, vec);
    bool flagged = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        info_out[k] = val[k];
#pragma unroll
        for (int i = 0; i < 3; ++i) dir_out[3 * k + i] = vec[3 * k + i];
        if (val[k] < thr) {
            flagged = true;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) cov[6 * (O + i) + O + j] = fma(infl, vec[3 * k + i] * vec[3 * k + j], cov[6 * (O + i) + O + j]); // (v_i v_j commutes: cov stays symmetric to the bit)
        }
    }
    return flagged;
}

template <int MODE>
__global__ __launch_bounds__(COV_SBLK) void k_cov_solve(const double *__restrict__ part, int nblocks, CovArg ca, sf_icp_covariance *__restrict__ out)
{
    constexpr int NREC = MODE == 2 ? NREC_COV_PLANE : NREC_COV_P2P;
    const int b = blockIdx.x;
    __shared__ double rec[REC_STRIDE];
    reduce_partials<NREC, COV_SBLK>(part + (size_t)b * nblocks * REC_STRIDE, nblocks, rec);
    if (threadIdx.x != 0) return;
    sf_icp_covariance *o = out + b;
    double H[36], chi2, W, cnt, dof;
    if (MODE == 2) {
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = a; c < 6; ++c) {
                H[6 * a + c] = rec[k];
                H[6 * c + a] = rec[k];
                ++k;
            }
        chi2 = rec[21]; W = rec[22]; cnt = rec[23];
        dof = W - 6.0;
    } else {
        // J_i = [-[s_i]x, I]:  H_rr = sum (|s|^2 I - s s^T),  H_rt = [sum s]x,  H_tr = H_rt^T,  H_tt = n I
        cnt = rec[0];
        const double mx = rec[1], my = rec[2], mz = rec[3];
        const double xx = rec[4], xy = rec[5], xz = rec[6], yy = rec[7], yz = rec[8], zz = rec[9];
#pragma unroll
        for (int i = 0; i < 36; ++i) H[i] = 0.0;
        H[0] = yy + zz; H[7] = xx + zz; H[14] = xx + yy;
        H[1] = H[6] = -xy; H[2] = H[12] = -xz; H[8] = H[13] = -yz;
        H[4] = -mz; H[5] = my; H[9] = mz; H[11] = -mx; H[15] = -my; H[16] = mx; // rows 0..2, columns 3..5: [m]x
        H[19] = mz; H[20] = -my; H[24] = -mz; H[26] = mx; H[30] = my; H[31] = -mx; // its transpose
        H[21] = H[28] = H[35] = cnt;
        chi2 = rec[10]; W = cnt;
        dof = 3.0 * cnt - 6.0;
    }
    int flags = 0;
    double cov[36], C[36];
#pragma unroll
    for (int i = 0; i < 36; ++i) cov[i] = C[i] = 0.0;
    double s2hat = 0.0, s2 = 0.0, lmax = 0.0;
    if (cnt < 10.0) { // the reference's own floor
        flags |= SF_COV_FEW_CORR;
#pragma unroll
        for (int i = 0; i < 36; ++i) H[i] = 0.0;
    } else {
        s2hat = dof > 0.0 ? chi2 / dof : 0.0;
        s2 = ca.sensor_sigma > 0.0 ? ca.sensor_sigma * ca.sensor_sigma : s2hat;
    }
#pragma unroll
    for (int i = 0; i < 36; ++i) o->info[i] = H[i];
    o->sigma2 = s2; o->sigma2_hat = s2hat; o->weight_sum = W;
    o->n_corr = (int64_t)cnt;
    double V[36];
    if (!(flags & SF_COV_FEW_CORR)) {
        jacobi_sym<6>(H, V);
#pragma unroll
        for (int k = 0; k < 6; ++k) lmax = fmax(lmax, H[7 * k]);
    }
    const bool solved = lmax > 0.0 && W > 0.0; // (a kernel that zeroed every weight leaves nothing to invert)
    if (solved) {
        const double floor_l = SF_COV_EIG_EPS * lmax;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            if (H[7 * k] <= floor_l) flags |= SF_COV_SINGULAR;
            const double il = recip_nr(fmax(H[7 * k], floor_l));
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = i; j < 6; ++j) C[6 * i + j] = fma(il * V[6 * i + k], V[6 * j + k], C[6 * i + j]);
        }
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) {
                C[6 * j + i] = C[6 * i + j];
                cov[6 * i + j] = cov[6 * j + i] = s2 * C[6 * i + j];
            }
        const double inv_w = recip_nr(W);
        if (marginal_info<0>(C, inv_w, ca.thr_r, ca.infl_r, o->rot_info, o->rot_dir, cov)) flags |= SF_COV_DEGENERATE_ROT;
        if (marginal_info<3>(C, inv_w, ca.thr_t, ca.infl_t, o->trans_info, o->trans_dir, cov)) flags |= SF_COV_DEGENERATE_TRANS;
    } else {
        if (!(flags & SF_COV_FEW_CORR)) flags |= SF_COV_SINGULAR;
#pragma unroll
        for (int k = 0; k < 3; ++k) { o->trans_info[k] = 0.0; o->rot_info[k] = 0.0; }
#pragma unroll
        for (int k = 0; k < 9; ++k) { o->trans_dir[k] = 0.0; o->rot_dir[k] = 0.0; }
    }
#pragma unroll
    for (int i = 0; i < 36; ++i) o->cov[i] = cov[i];
    o->flags = flags;
}
