// sf_ndt.hip -- Normal Distributions Transform scan-to-map registration (sf_ndt_*, include/slamfusion.h; extension, no reference
// code: the rule is in DESIGN sections 24 and 25 and restated in tests/ndt_ref_np.py and tests/ndt_ls_ref_np.py).  gfx950 only, wave64.
// A translation unit of its own over the float64 numerical core: it uses sf_reduce.hpp's block_reduce_store, reduce_partials and
// wave_reduce_1, sf_linalg.hpp's vec6_to_mat4 and mat4_mul and sf_jacobi.hpp's jacobi_sym as they are, the scans of sf_sort.hpp,
// and nothing of ICP.
//
// Target (once per target, on the grid index sf_map_build makes at cell = resolution):
//   k_ndt_cell_flags   one lane per cell: 1 when the cell holds a point; an exclusive scan ranks the occupied cells
//   k_ndt_occupied     the occupied cells in ascending cell id
//   k_ndt_voxels       one WAVE per occupied cell over the cell's contiguous run: the mean, then the centred second moments,
//                      float64, lanes strided by 64 and the fixed butterfly of wave_reduce_1 -- the same bits every build;
//                      then on every lane alike the 3 x 3 Jacobi solve, the eigenvalue floor, cov = V L V^T and B = V L^-1 V^T
//   k_ndt_compact      the voxels in ascending cell id (an exclusive scan of the voxel flags) and the dense cell -> voxel table
// Alignment (per iteration, no host synchronisation in between):
//   k_ndt_derivs<NB>   one lane per source point, blockIdx.y the batch entry: y = T x, the home cell, 1 or 7 voxel records of
//                      80 bytes, the 30-double record (score, gradient 6, upper Hessian 21, points that met a voxel, terms) in
//                      registers; block_reduce_store<30> into partials[b][block][32]
//   k_ndt_step         one workgroup per batch entry: reduce_partials<30, 256>, then on one lane the modified Newton step
//                      (jacobi_sym<6>), the pose update, the done flag and the trace row; as the last launch of an alignment
//                      (final_pass) it only records score, gradient and Hessian at the final pose
#include "sf_common.hpp"
#include "sf_sort.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

namespace {

#include "sf_linalg.hpp"
#include "sf_reduce.hpp"

constexpr int NREC_NDT = 30;
constexpr int NDT_VOX_STRIDE = 10; // doubles per voxel record: mean[3], B xx xy xz yy yz zz, count -- five 16-byte loads
constexpr int NDT_TMP_STRIDE = 16; // per occupied cell before the compaction: mean[3], cov[6], B[6], count
constexpr int NDT_SBLK = 256;

struct NdtGrid {
    double org[3], inv_h;          // the index's float32 origin and 1 / cell, widened
    int dim[3];
    const int32_t *cell_voxel;     // [ncell]: voxel id or -1
    const double *vox;             // [n_voxels][NDT_VOX_STRIDE]
};

struct NdtConst { double d1, half_d2, d2, neg_d1d2; };
struct NdtStepArg { double step_size, eps, hessian_floor; };

struct NdtState {
    double T[16];
    double score, g[6], H[36];
    long long n_inside, n_terms;
    int iterations, converged, modified, flags, done, pad;
};

__global__ __launch_bounds__(256) void k_ndt_cell_flags(const uint32_t *__restrict__ cell_start, int64_t ncell, uint32_t *__restrict__ flag)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < ncell) flag[c] = cell_start[c + 1] > cell_start[c] ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_ndt_occupied(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos, int64_t ncell, uint32_t *__restrict__ occ)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < ncell && flag[c]) occ[pos[c]] = (uint32_t)c;
}

__global__ __launch_bounds__(BLK) void k_ndt_voxels(const float4 *__restrict__ pts, const uint32_t *__restrict__ cell_start, const uint32_t *__restrict__ occ, int64_t n_occ,
                                                    int min_points, double min_eig_ratio, double *__restrict__ tmp, uint32_t *__restrict__ is_voxel)
{
    const int64_t o = (int64_t)blockIdx.x * (BLK / 64) + (threadIdx.x >> 6);
    if (o >= n_occ) return; // (the whole wave leaves together)
    const int lane = threadIdx.x & 63;
    const uint32_t c = occ[o];
    const uint32_t a = cell_start[c], b = cell_start[c + 1];
    const int m = (int)(b - a);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (uint32_t k = a + lane; k < b; k += 64) {
        const float4 p = pts[k];
        sx = sx + (double)p.x; sy = sy + (double)p.y; sz = sz + (double)p.z;
    }
    sx = wave_reduce_1(sx); sy = wave_reduce_1(sy); sz = wave_reduce_1(sz);
    const double mx = sx / (double)m, my = sy / (double)m, mz = sz / (double)m;
    bool voxel = m >= min_points; // (min_points >= 3: m - 1 > 0 below)
    double cov[6] = {0, 0, 0, 0, 0, 0}, B[6] = {0, 0, 0, 0, 0, 0};
    if (voxel) { // wave-uniform
        double qxx = 0.0, qxy = 0.0, qxz = 0.0, qyy = 0.0, qyz = 0.0, qzz = 0.0;
        for (uint32_t k = a + lane; k < b; k += 64) {
            const float4 p = pts[k];
            const double dx = (double)p.x - mx, dy = (double)p.y - my, dz = (double)p.z - mz;
            qxx = qxx + dx * dx; qxy = qxy + dx * dy; qxz = qxz + dx * dz;
            qyy = qyy + dy * dy; qyz = qyz + dy * dz; qzz = qzz + dz * dz;
        }
        qxx = wave_reduce_1(qxx); qxy = wave_reduce_1(qxy); qxz = wave_reduce_1(qxz);
        qyy = wave_reduce_1(qyy); qyz = wave_reduce_1(qyz); qzz = wave_reduce_1(qzz);
        const double dof = (double)(m - 1);
        double A[9], V[9];
        A[0] = qxx / dof;
        A[1] = A[3] = qxy / dof;
        A[2] = A[6] = qxz / dof;
        A[4] = qyy / dof;
        A[5] = A[7] = qyz / dof;
        A[8] = qzz / dof;
        jacobi_sym<3>(A, V);
        const double lmax = fmax(A[0], fmax(A[4], A[8]));
        voxel = lmax > 0.0 && lmax < INFINITY; // (NaN compares false)
        if (voxel) {
            const double fl = min_eig_ratio * lmax;
            double l[3], il[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                l[k] = fmax(A[4 * k], fl);
                il[k] = 1.0 / l[k];
            }
            int e = 0;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = i; j < 3; ++j) {
                    cov[e] = (l[0] * V[3 * i] * V[3 * j] + l[1] * V[3 * i + 1] * V[3 * j + 1]) + l[2] * V[3 * i + 2] * V[3 * j + 2];
                    B[e] = (il[0] * V[3 * i] * V[3 * j] + il[1] * V[3 * i + 1] * V[3 * j + 1]) + il[2] * V[3 * i + 2] * V[3 * j + 2];
                    ++e;
                }
        }
    }
    if (lane == 0) {
        double *t = tmp + (size_t)o * NDT_TMP_STRIDE;
        t[0] = mx; t[1] = my; t[2] = mz;
#pragma unroll
        for (int e = 0; e < 6; ++e) { t[3 + e] = cov[e]; t[9 + e] = B[e]; }
        t[15] = (double)m;
        is_voxel[o] = voxel ? 1u : 0u;
    }
}

__global__ __launch_bounds__(256) void k_ndt_compact(const uint32_t *__restrict__ occ, const uint32_t *__restrict__ is_voxel, const uint32_t *__restrict__ vpos, int64_t n_occ,
                                                     const double *__restrict__ tmp, double *__restrict__ vox, double *__restrict__ cov, int64_t *__restrict__ vcell,
                                                     int32_t *__restrict__ vcount, int32_t *__restrict__ cell_voxel)
{
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_occ || !is_voxel[o]) return;
    const uint32_t v = vpos[o], c = occ[o];
    const double *t = tmp + (size_t)o * NDT_TMP_STRIDE;
    double *r = vox + (size_t)v * NDT_VOX_STRIDE;
    r[0] = t[0]; r[1] = t[1]; r[2] = t[2];
#pragma unroll
    for (int e = 0; e < 6; ++e) { r[3 + e] = t[9 + e]; cov[(size_t)v * 6 + e] = t[3 + e]; }
    r[9] = t[15];
    vcell[v] = (int64_t)c;
    vcount[v] = (int32_t)t[15];
    cell_voxel[c] = (int32_t)v;
}

// the map's points back in their original order (sf_ndt_set_target_map: the NDT index is built from them like from a cloud)
__global__ __launch_bounds__(256) void k_ndt_unsort(const float4 *__restrict__ pts, int64_t n, float *__restrict__ xyz)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const float4 p = pts[j];
    const size_t id = __float_as_uint(p.w);
    if (id >= (size_t)n) return;
    xyz[3 * id] = p.x; xyz[3 * id + 1] = p.y; xyz[3 * id + 2] = p.z;
}

// J_j . v for the pose parameters (rx, ry, rz, tx, ty, tz): J_i = e_i x y for i < 3, e_(i-3) beyond
template <int J>
__device__ __forceinline__ double ndt_jdot(const double (&y)[3], double v0, double v1, double v2)
{
    if constexpr (J == 0) return v2 * y[1] - v1 * y[2];
    else if constexpr (J == 1) return v0 * y[2] - v2 * y[0];
    else if constexpr (J == 2) return v1 * y[0] - v0 * y[1];
    else if constexpr (J == 3) return v0;
    else if constexpr (J == 4) return v1;
    else return v2;
}

template <int I, int J>
__device__ __forceinline__ void ndt_hessian_entries(double (&acc)[NREC_NDT], const double (&y)[3], const double (&c)[3], const double (&a)[6], const double (&BJ)[18], double cy,
                                                    double w, double d2)
{
    constexpr int K = 7 + (I * (13 - I)) / 2 + (J - I); // the upper triangle row by row: (0,0) (0,1) .. (0,5) (1,1) .. (5,5)
    double t = ndt_jdot<J>(y, BJ[3 * I], BJ[3 * I + 1], BJ[3 * I + 2]) - d2 * a[I] * a[J];
    if constexpr (J < 3) { // the second derivative of y: e_I y_J - y delta_IJ
        t = t + c[I] * y[J];
        if constexpr (I == J) t = t - cy;
    }
    acc[K] = acc[K] + w * t;
    if constexpr (J + 1 < 6) ndt_hessian_entries<I, J + 1>(acc, y, c, a, BJ, cy, w, d2);
    else if constexpr (I + 1 < 6) ndt_hessian_entries<I + 1, I + 1>(acc, y, c, a, BJ, cy, w, d2);
}

template <int NB>
__global__ __launch_bounds__(BLK) void k_ndt_derivs(NdtGrid g, NdtConst cn, const float *__restrict__ src, int n, size_t src_stride, const NdtState *__restrict__ st, int force,
                                                    double *__restrict__ partials, int nblocks)
{
    const int b = blockIdx.y;
    const NdtState *S = st + b;
    if (!force && S->done) return;
    double acc[NREC_NDT];
#pragma unroll
    for (int k = 0; k < NREC_NDT; ++k) acc[k] = 0.0;
    const int i = blockIdx.x * BLK + (int)threadIdx.x;
    if (i < n) {
        const float *p = src + (size_t)b * src_stride + 3 * (size_t)i;
        const double x0 = (double)p[0], x1 = (double)p[1], x2 = (double)p[2];
        double y[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) y[d] = ((S->T[4 * d] * x0 + S->T[4 * d + 1] * x1) + S->T[4 * d + 2] * x2) + S->T[4 * d + 3];
        const double gx = (y[0] - g.org[0]) * g.inv_h, gy = (y[1] - g.org[1]) * g.inv_h, gz = (y[2] - g.org[2]) * g.inv_h;
        // a point outside the grid has no home cell (NaN compares false): this is not the index's clamp
        if (gx >= 0.0 && gx < (double)g.dim[0] && gy >= 0.0 && gy < (double)g.dim[1] && gz >= 0.0 && gz < (double)g.dim[2]) {
            const int cx = (int)floor(gx), cy_ = (int)floor(gy), cz = (int)floor(gz);
            int terms = 0;
            for (int nb = 0; nb < NB; ++nb) { // the home cell, then +x -x +y -y +z -z
                const int ax = (nb + 1) >> 1, sg = (nb & 1) ? 1 : -1;
                const int ox = cx + (ax == 1 ? sg : 0), oy = cy_ + (ax == 2 ? sg : 0), oz = cz + (ax == 3 ? sg : 0);
                if (ox < 0 || ox >= g.dim[0] || oy < 0 || oy >= g.dim[1] || oz < 0 || oz >= g.dim[2]) continue;
                const int32_t v = g.cell_voxel[((size_t)oz * (size_t)g.dim[1] + (size_t)oy) * (size_t)g.dim[0] + (size_t)ox];
                if (v < 0) continue;
                const double2 *r = reinterpret_cast<const double2 *>(g.vox + (size_t)v * NDT_VOX_STRIDE);
                const double2 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
                const double r4 = r[4].x;
                const double q0 = y[0] - r0.x, q1 = y[1] - r0.y, q2 = y[2] - r1.x;
                const double bxx = r1.y, bxy = r2.x, bxz = r2.y, byy = r3.x, byz = r3.y, bzz = r4;
                double c[3];
                c[0] = (bxx * q0 + bxy * q1) + bxz * q2;
                c[1] = (bxy * q0 + byy * q1) + byz * q2;
                c[2] = (bxz * q0 + byz * q1) + bzz * q2;
                const double s = (q0 * c[0] + q1 * c[1]) + q2 * c[2];
                const double e = exp(-(cn.half_d2 * s));
                const double w = cn.neg_d1d2 * e;
                acc[0] = acc[0] + cn.d1 * e;
                double a[6];
                a[0] = ndt_jdot<0>(y, c[0], c[1], c[2]);
                a[1] = ndt_jdot<1>(y, c[0], c[1], c[2]);
                a[2] = ndt_jdot<2>(y, c[0], c[1], c[2]);
                a[3] = c[0]; a[4] = c[1]; a[5] = c[2];
#pragma unroll
                for (int k = 0; k < 6; ++k) acc[1 + k] = acc[1 + k] + w * a[k];
                // B J_i: J_0 = (0, -y2, y1), J_1 = (y2, 0, -y0), J_2 = (-y1, y0, 0), J_3.. = the unit vectors
                double BJ[18];
                BJ[0] = bxz * y[1] - bxy * y[2]; BJ[1] = byz * y[1] - byy * y[2]; BJ[2] = bzz * y[1] - byz * y[2];
                BJ[3] = bxx * y[2] - bxz * y[0]; BJ[4] = bxy * y[2] - byz * y[0]; BJ[5] = bxz * y[2] - bzz * y[0];
                BJ[6] = bxy * y[0] - bxx * y[1]; BJ[7] = byy * y[0] - bxy * y[1]; BJ[8] = byz * y[0] - bxz * y[1];
                BJ[9] = bxx; BJ[10] = bxy; BJ[11] = bxz;
                BJ[12] = bxy; BJ[13] = byy; BJ[14] = byz;
                BJ[15] = bxz; BJ[16] = byz; BJ[17] = bzz;
                const double cy = (c[0] * y[0] + c[1] * y[1]) + c[2] * y[2];
                ndt_hessian_entries<0, 0>(acc, y, c, a, BJ, cy, w, cn.d2);
                ++terms;
            }
            acc[28] = terms > 0 ? 1.0 : 0.0;
            acc[29] = (double)terms;
        }
    }
    block_reduce_store<NREC_NDT>(acc, partials + ((size_t)b * nblocks + blockIdx.x) * REC_STRIDE);
}

__global__ __launch_bounds__(NDT_SBLK) void k_ndt_step(NdtState *__restrict__ st, const double *__restrict__ partials, int nblocks, NdtStepArg sa, int it, int final_pass,
                                                       double *__restrict__ trace)
{
    const int b = blockIdx.x;
    NdtState *S = st + b;
    if (!final_pass && S->done) return;
    __shared__ double rec[REC_STRIDE];
    reduce_partials<NREC_NDT, NDT_SBLK>(partials + (size_t)b * nblocks * REC_STRIDE, nblocks, rec);
    if (threadIdx.x != 0) return;
    double g[6], H[36];
#pragma unroll
    for (int k = 0; k < 6; ++k) g[k] = rec[1 + k];
    {
        int k = 7;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = a; c < 6; ++c) { H[6 * a + c] = rec[k]; H[6 * c + a] = rec[k]; ++k; }
    }
    // usable: a term exists, everything is finite and H is not all zero
    double hsum = 0.0, gsum = 0.0;
#pragma unroll
    for (int k = 0; k < 36; ++k) hsum = hsum + fabs(H[k]);
#pragma unroll
    for (int k = 0; k < 6; ++k) gsum = gsum + fabs(g[k]);
    const bool usable = rec[29] > 0.0 && hsum > 0.0 && hsum < INFINITY && gsum < INFINITY && fabs(rec[0]) < INFINITY;
    if (final_pass) {
        S->score = usable ? rec[0] : 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) S->g[k] = usable ? g[k] : 0.0;
#pragma unroll
        for (int k = 0; k < 36; ++k) S->H[k] = usable ? H[k] : 0.0;
        S->n_inside = (long long)rec[28];
        S->n_terms = (long long)rec[29];
        if (!usable) S->flags |= SF_NDT_FLAG_NO_OVERLAP;
        if (!S->done) { S->iterations = it; S->done = 1; }
        return;
    }
    if (!usable) { // the pose stays as it is
        S->flags |= SF_NDT_FLAG_NO_OVERLAP;
        S->iterations = it;
        S->done = 1;
        return;
    }
    double V[36];
    jacobi_sym<6>(H, V);
    double amax = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) amax = fmax(amax, fabs(H[7 * k]));
    const double fl = sa.hessian_floor * amax;
    bool modified = false;
    double pk[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double l = H[7 * k];
        if (l < 0.0 || fabs(l) < fl) modified = true;
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) t = t + V[6 * i + k] * g[i];
        pk[k] = t / fmax(fabs(l), fl);
    }
    double d[6], n2 = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) t = t + V[6 * i + k] * pk[k];
        d[i] = -t;
        n2 = n2 + d[i] * d[i];
    }
    double len = sqrt(n2);
    if (!(len < INFINITY)) { // (an overflow of the solve: treated like a Hessian that is not finite)
        S->flags |= SF_NDT_FLAG_NO_OVERLAP;
        S->iterations = it;
        S->done = 1;
        return;
    }
    if (len > sa.step_size) {
        const double sc = sa.step_size / len;
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = d[i] * sc;
        len = sa.step_size;
    }
    double upd[16], Tc[16];
    vec6_to_mat4(d, upd);
#pragma unroll
    for (int i = 0; i < 16; ++i) Tc[i] = S->T[i];
    mat4_mul(upd, Tc, Tc);
#pragma unroll
    for (int i = 0; i < 16; ++i) S->T[i] = Tc[i];
    if (trace && b == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) trace[(size_t)(it + 1) * 16 + i] = Tc[i];
    }
    S->iterations = it + 1;
    if (modified) S->modified += 1;
    if (len < sa.eps) { S->converged = 1; S->done = 1; }
}

// ------------------------------------------------------------------ line search (sf_ndt_set_line_search)
// Per iteration, after k_ndt_derivs as above:
//   k_ndt_step_ls      one workgroup per batch entry: the reduction and the 6 x 6 solve of k_ndt_step up to d (the same expressions
//                      in the same order), then alpha_max, the slope and the `trials` poses T_k = M(ldexp(alpha_max, -k) d) T
//   k_ndt_scores<NB>   one lane per source point with k_ndt_derivs' mapping, blockIdx.y the entry, blockIdx.z the trial: the score
//                      in slot 0 and the terms in slot 1 of the same block_reduce_store (its butterfly pairs the same lanes whatever
//                      the slot), so that the sums are bit for bit k_ndt_derivs' acc[0] and acc[29] at that pose
//   k_ndt_pick         one workgroup per entry: reduce_partials over each trial's rows, then on one lane the smallest k that meets
//                      the Armijo condition, the pose, the counters, the flags and the rows of entry 0
constexpr int NREC_NDT_SCORE = 2;

struct NdtLsArg { double step_max, armijo, eps, hessian_floor; int trials; };

struct NdtLsEntry {
    double Tk[SF_NDT_MAX_TRIALS][16];
    double alpha_max, raw, phi0, slope;
    int modified, pad;
};

// pose p = blockIdx.y * gridDim.z + blockIdx.z reads poses[p][16] and the scan blockIdx.y (src_stride 0: every pose the same
// scan); done: the states whose done flag lets an entry leave at once, or nullptr
template <int NB>
__global__ __launch_bounds__(BLK) void k_ndt_scores(NdtGrid g, NdtConst cn, const float *__restrict__ src, int n, size_t src_stride, const NdtState *__restrict__ done,
                                                    const double *__restrict__ poses, size_t pose_stride, double *__restrict__ partials, int nblocks)
{
    const int b = blockIdx.y;
    if (done && done[b].done) return;
    const size_t p = (size_t)b * gridDim.z + blockIdx.z;
    const double *T = poses + (size_t)b * pose_stride + (size_t)blockIdx.z * 16;
    double acc[NREC_NDT_SCORE] = {0.0, 0.0};
    const int i = blockIdx.x * BLK + (int)threadIdx.x;
    if (i < n) {
        const float *q = src + (size_t)b * src_stride + 3 * (size_t)i;
        const double x0 = (double)q[0], x1 = (double)q[1], x2 = (double)q[2];
        double y[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) y[d] = ((T[4 * d] * x0 + T[4 * d + 1] * x1) + T[4 * d + 2] * x2) + T[4 * d + 3];
        const double gx = (y[0] - g.org[0]) * g.inv_h, gy = (y[1] - g.org[1]) * g.inv_h, gz = (y[2] - g.org[2]) * g.inv_h;
        if (gx >= 0.0 && gx < (double)g.dim[0] && gy >= 0.0 && gy < (double)g.dim[1] && gz >= 0.0 && gz < (double)g.dim[2]) {
            const int cx = (int)floor(gx), cy_ = (int)floor(gy), cz = (int)floor(gz);
            int terms = 0;
            for (int nb = 0; nb < NB; ++nb) { // the home cell, then +x -x +y -y +z -z
                const int ax = (nb + 1) >> 1, sg = (nb & 1) ? 1 : -1;
                const int ox = cx + (ax == 1 ? sg : 0), oy = cy_ + (ax == 2 ? sg : 0), oz = cz + (ax == 3 ? sg : 0);
                if (ox < 0 || ox >= g.dim[0] || oy < 0 || oy >= g.dim[1] || oz < 0 || oz >= g.dim[2]) continue;
                const int32_t v = g.cell_voxel[((size_t)oz * (size_t)g.dim[1] + (size_t)oy) * (size_t)g.dim[0] + (size_t)ox];
                if (v < 0) continue;
                const double2 *r = reinterpret_cast<const double2 *>(g.vox + (size_t)v * NDT_VOX_STRIDE);
                const double2 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
                const double r4 = r[4].x;
                const double q0 = y[0] - r0.x, q1 = y[1] - r0.y, q2 = y[2] - r1.x;
                const double bxx = r1.y, bxy = r2.x, bxz = r2.y, byy = r3.x, byz = r3.y, bzz = r4;
                const double c0 = (bxx * q0 + bxy * q1) + bxz * q2;
                const double c1 = (bxy * q0 + byy * q1) + byz * q2;
                const double c2 = (bxz * q0 + byz * q1) + bzz * q2;
                const double s = (q0 * c0 + q1 * c1) + q2 * c2;
                const double e = exp(-(cn.half_d2 * s));
                acc[0] = acc[0] + cn.d1 * e;
                ++terms;
            }
            acc[1] = (double)terms;
        }
    }
    block_reduce_store<NREC_NDT_SCORE>(acc, partials + (p * (size_t)nblocks + blockIdx.x) * REC_STRIDE);
}

// sf_ndt_scores: one workgroup per pose
__global__ __launch_bounds__(NDT_SBLK) void k_ndt_scores_out(const double *__restrict__ partials, int nblocks, double *__restrict__ out)
{
    __shared__ double rec[REC_STRIDE];
    reduce_partials<NREC_NDT_SCORE, NDT_SBLK>(partials + (size_t)blockIdx.x * nblocks * REC_STRIDE, nblocks, rec);
    if (threadIdx.x != 0) return;
    const bool finite = fabs(rec[0]) < INFINITY; // (NaN compares false)
    out[2 * (size_t)blockIdx.x] = finite ? rec[0] : 0.0;
    out[2 * (size_t)blockIdx.x + 1] = finite ? rec[1] : 0.0;
}

__global__ __launch_bounds__(NDT_SBLK) void k_ndt_step_ls(NdtState *__restrict__ st, const double *__restrict__ partials, int nblocks, NdtLsArg la, int it,
                                                          NdtLsEntry *__restrict__ ls, sf_ndt_ls_row *__restrict__ rows)
{
    const int b = blockIdx.x;
    NdtState *S = st + b;
    if (S->done) return;
    __shared__ double rec[REC_STRIDE];
    reduce_partials<NREC_NDT, NDT_SBLK>(partials + (size_t)b * nblocks * REC_STRIDE, nblocks, rec);
    if (threadIdx.x != 0) return;
    double g[6], H[36];
#pragma unroll
    for (int k = 0; k < 6; ++k) g[k] = rec[1 + k];
    {
        int k = 7;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = a; c < 6; ++c) { H[6 * a + c] = rec[k]; H[6 * c + a] = rec[k]; ++k; }
    }
    double hsum = 0.0, gsum = 0.0;
#pragma unroll
    for (int k = 0; k < 36; ++k) hsum = hsum + fabs(H[k]);
#pragma unroll
    for (int k = 0; k < 6; ++k) gsum = gsum + fabs(g[k]);
    const bool usable = rec[29] > 0.0 && hsum > 0.0 && hsum < INFINITY && gsum < INFINITY && fabs(rec[0]) < INFINITY;
    if (!usable) { // the pose stays as it is
        S->flags |= SF_NDT_FLAG_NO_OVERLAP;
        S->iterations = it;
        S->done = 1;
        return;
    }
    double V[36];
    jacobi_sym<6>(H, V);
    double amax = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) amax = fmax(amax, fabs(H[7 * k]));
    const double fl = la.hessian_floor * amax;
    bool modified = false;
    double pk[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double l = H[7 * k];
        if (l < 0.0 || fabs(l) < fl) modified = true;
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) t = t + V[6 * i + k] * g[i];
        pk[k] = t / fmax(fabs(l), fl);
    }
    double d[6], n2 = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) t = t + V[6 * i + k] * pk[k];
        d[i] = -t;
        n2 = n2 + d[i] * d[i];
    }
    const double raw = sqrt(n2);
    if (!(raw < INFINITY)) {
        S->flags |= SF_NDT_FLAG_NO_OVERLAP;
        S->iterations = it;
        S->done = 1;
        return;
    }
    const double alpha_max = raw > la.step_max ? la.step_max / raw : 1.0;
    const double slope = ((((g[0] * d[0] + g[1] * d[1]) + g[2] * d[2]) + g[3] * d[3]) + g[4] * d[4]) + g[5] * d[5];
    NdtLsEntry *L = ls + b;
    double Tc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) Tc[i] = S->T[i];
    for (int k = 0; k < la.trials; ++k) {
        const double alpha = ldexp(alpha_max, -k);
        double dk[6], upd[16], Tk[16];
#pragma unroll
        for (int i = 0; i < 6; ++i) dk[i] = alpha * d[i];
        vec6_to_mat4(dk, upd);
        mat4_mul(upd, Tc, Tk);
#pragma unroll
        for (int i = 0; i < 16; ++i) L->Tk[k][i] = Tk[i];
    }
    L->alpha_max = alpha_max;
    L->raw = raw;
    L->phi0 = rec[0];
    L->slope = slope;
    L->modified = modified ? 1 : 0;
    if (rows && b == 0) {
        sf_ndt_ls_row *R = rows + it;
        R->alpha_max = alpha_max;
        R->raw_length = raw;
        R->phi0 = rec[0];
        R->slope = slope;
#pragma unroll
        for (int i = 0; i < 6; ++i) R->delta[i] = d[i];
        R->trials = la.trials;
    }
}

__global__ __launch_bounds__(NDT_SBLK) void k_ndt_pick(NdtState *__restrict__ st, const double *__restrict__ tpart, int nblocks, NdtLsArg la, int it,
                                                       const NdtLsEntry *__restrict__ ls, double *__restrict__ trace, sf_ndt_ls_row *__restrict__ rows)
{
    const int b = blockIdx.x;
    NdtState *S = st + b;
    if (S->done) return; // (also an entry that k_ndt_step_ls has just ended)
    __shared__ double rec[REC_STRIDE];
    __shared__ double phi[SF_NDT_MAX_TRIALS], terms[SF_NDT_MAX_TRIALS];
    for (int k = 0; k < la.trials; ++k) {
        reduce_partials<NREC_NDT_SCORE, NDT_SBLK>(tpart + ((size_t)b * la.trials + k) * nblocks * REC_STRIDE, nblocks, rec);
        if (threadIdx.x == 0) { phi[k] = rec[0]; terms[k] = rec[1]; }
    }
    if (threadIdx.x != 0) return;
    const NdtLsEntry *L = ls + b;
    int chosen = -1;
    double alpha_chosen = 0.0;
    for (int k = 0; k < la.trials && chosen < 0; ++k) {
        const double alpha = ldexp(L->alpha_max, -k);
        if (terms[k] > 0.0 && fabs(phi[k]) < INFINITY && phi[k] <= L->phi0 + (la.armijo * alpha) * L->slope) { chosen = k; alpha_chosen = alpha; }
    }
    if (rows && b == 0) {
        sf_ndt_ls_row *R = rows + it;
        for (int k = 0; k < SF_NDT_MAX_TRIALS; ++k) {
            R->phi[k] = k < la.trials ? phi[k] : 0.0;
            R->n_terms[k] = k < la.trials ? (int64_t)terms[k] : 0;
        }
        R->chosen = chosen;
    }
    if (chosen < 0) { // the pose stays as it is
        S->flags |= SF_NDT_FLAG_LINE_SEARCH_STALLED;
        S->iterations = it;
        S->done = 1;
        return;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) S->T[i] = L->Tk[chosen][i];
    if (trace && b == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) trace[(size_t)(it + 1) * 16 + i] = L->Tk[chosen][i];
    }
    S->iterations = it + 1;
    if (L->modified) S->modified += 1;
    if (alpha_chosen * L->raw < la.eps) { S->converged = 1; S->done = 1; }
}

} // namespace

// ==================================================================== the host side
// The object, the voxel build on an index of its own and the launch list of an alignment.  An alignment enqueues max_iterations
// pairs (k_ndt_derivs, k_ndt_step), one more derivative pass at the final pose and the copy of the states, and waits once.  With
// the line search on (sf_ndt_set_line_search) an iteration is four launches (k_ndt_derivs, k_ndt_step_ls, k_ndt_scores over every
// entry's trials, k_ndt_pick), still without a wait in between; sf_ndt_align_levels runs one such alignment per level.

struct sf_ndt {
    sf_ctx *ctx = nullptr;
    sf_ndt_params prm{};
    sf_map *index = nullptr;    // the grid index at cell = resolution (its own, also for a map target)
    sf_cloud *points = nullptr; // sf_ndt_set_target_map: the map's points in original order
    sf::DevBuf flag, pos, occ, is_voxel, vpos, tmp, vox, cov, vcell, vcount, cell_voxel;
    sf::DevBuf src, state, partials, trace;
    sf_ndt_line_search ls{0, 0, 1.0, 1e-4};            // trials 0: off
    sf::DevBuf ls_entry, ls_partials, ls_rows, poses, scores;
    std::vector<sf_ndt_ls_row> rows;                   // entry 0 of the last sf_ndt_align with the search on
    bool has_rows = false;
    int64_t n_points = 0, n_cells = 0, n_occupied = 0, n_voxels = 0, n_src = 0;
    int batch = 0;
    bool has_target = false, has_source = false;
    float build_ms = -1.0f, align_ms = -1.0f;
    hipEvent_t ev[2] = {nullptr, nullptr};
};

namespace {

constexpr int NDT_MAX_BATCH = 64;

int ndt_check_params(const sf_ndt_params *p)
{
    SF_CHECK(p, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(std::isfinite(p->resolution) && p->resolution > 0.0, SF_ERR_INVALID, "bad arguments: ndt resolution must be positive and finite (got %g)", p->resolution);
    SF_CHECK(p->outlier_ratio > 0.0 && p->outlier_ratio < 1.0, SF_ERR_INVALID, "bad arguments: ndt outlier_ratio must lie in (0, 1) (got %g)", p->outlier_ratio);
    SF_CHECK(p->min_points >= 3, SF_ERR_INVALID, "bad arguments: ndt min_points must be >= 3 (got %d)", (int)p->min_points);
    SF_CHECK(p->neighbours == SF_NDT_DIRECT1 || p->neighbours == SF_NDT_DIRECT7, SF_ERR_INVALID, "bad arguments: ndt neighbours must be 1 or 7 (got %d)", (int)p->neighbours);
    SF_CHECK(p->max_iterations >= 0 && p->max_iterations <= 1024, SF_ERR_INVALID, "bad arguments: ndt max_iterations must be 0 .. 1024 (got %d)", (int)p->max_iterations);
    SF_CHECK(p->step_size > 0.0, SF_ERR_INVALID, "bad arguments: ndt step_size must be positive (got %g)", p->step_size);
    return SF_OK;
}

NdtConst ndt_constants(const sf_ndt_params &p)
{
    const double r = p.resolution, c1 = 10.0 * (1.0 - p.outlier_ratio), c2 = p.outlier_ratio / (r * r * r);
    const double d3 = -std::log(c2), d1 = -std::log(c1 + c2) - d3;
    const double d2 = -2.0 * std::log((-std::log(c1 * std::exp(-0.5) + c2) - d3) / d1);
    return NdtConst{d1, 0.5 * d2, d2, -(d1 * d2)};
}

inline unsigned ndt_blocks(int64_t n, int per) { return (unsigned)std::max<int64_t>(sf::div_up(n, per), 1); }

int ndt_event_ms(sf_ndt *ndt, float *ms)
{
    *ms = -1.0f;
    if (ndt->prm.profile) SF_HIP(hipEventElapsedTime(ms, ndt->ev[0], ndt->ev[1]));
    return SF_OK;
}

int ndt_mark(sf_ndt *ndt, int k)
{
    if (!ndt->prm.profile) return SF_OK;
    if (!ndt->ev[k]) SF_HIP(hipEventCreate(&ndt->ev[k]));
    SF_HIP(hipEventRecord(ndt->ev[k], ndt->ctx->stream));
    return SF_OK;
}

// the index of `cloud` at cell = resolution, then the voxels
int ndt_build(sf_ndt *ndt, sf_cloud *cloud)
{
    sf_ctx *ctx = ndt->ctx;
    ndt->has_target = false;
    ndt->build_ms = -1.0f;
    if (!ndt->index) SF_TRY(sf_map_create(ctx, &ndt->index));
    SF_TRY(sf_map_build(ndt->index, cloud, (float)ndt->prm.resolution)); // (refuses a table that does not fit: SF_ERR_OVERFLOW)
    const SfGrid &G = ndt->index->grid;
    const uint64_t ncell = (uint64_t)G.dim[0] * (uint64_t)G.dim[1] * (uint64_t)G.dim[2];
    SF_CHECK(ncell < (1ull << 31), SF_ERR_OVERFLOW, "ndt: %.3g cells at resolution %g: the cell -> voxel table holds fewer than 2^31", (double)ncell, ndt->prm.resolution);
    hipStream_t s = ctx->stream;
    const int64_t nc = (int64_t)ncell;
    SF_TRY(ndt->flag.reserve(sizeof(uint32_t) * (size_t)nc));
    SF_TRY(ndt->pos.reserve(sizeof(uint32_t) * (size_t)nc));
    SF_TRY(ndt->cell_voxel.reserve(sizeof(int32_t) * (size_t)nc));
    SF_TRY(ndt_mark(ndt, 0));
    SF_HIP(hipMemsetAsync(ndt->cell_voxel.p, 0xff, sizeof(int32_t) * (size_t)nc, s));
    hipLaunchKernelGGL(k_ndt_cell_flags, dim3(ndt_blocks(nc, 256)), dim3(256), 0, s, G.cell_start, nc, ndt->flag.as<uint32_t>());
    SF_TRY(sf::scan_u32<0>(ctx, ndt->flag.as<uint32_t>(), ndt->pos.as<uint32_t>(), nc));
    uint32_t last[2] = {0, 0};
    SF_HIP(hipMemcpyAsync(&last[0], ndt->pos.as<uint32_t>() + (nc - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    SF_HIP(hipMemcpyAsync(&last[1], ndt->flag.as<uint32_t>() + (nc - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    SF_HIP(hipStreamSynchronize(s));
    const int64_t n_occ = (int64_t)last[0] + (int64_t)last[1];
    int64_t n_vox = 0;
    if (n_occ > 0) {
        SF_TRY(ndt->occ.reserve(sizeof(uint32_t) * (size_t)n_occ));
        SF_TRY(ndt->is_voxel.reserve(sizeof(uint32_t) * (size_t)n_occ));
        SF_TRY(ndt->vpos.reserve(sizeof(uint32_t) * (size_t)n_occ));
        SF_TRY(ndt->tmp.reserve(sizeof(double) * NDT_TMP_STRIDE * (size_t)n_occ));
        SF_TRY(ndt->vox.reserve(sizeof(double) * NDT_VOX_STRIDE * (size_t)n_occ));
        SF_TRY(ndt->cov.reserve(sizeof(double) * 6 * (size_t)n_occ));
        SF_TRY(ndt->vcell.reserve(sizeof(int64_t) * (size_t)n_occ));
        SF_TRY(ndt->vcount.reserve(sizeof(int32_t) * (size_t)n_occ));
        hipLaunchKernelGGL(k_ndt_occupied, dim3(ndt_blocks(nc, 256)), dim3(256), 0, s, ndt->flag.as<uint32_t>(), ndt->pos.as<uint32_t>(), nc, ndt->occ.as<uint32_t>());
        hipLaunchKernelGGL(k_ndt_voxels, dim3(ndt_blocks(n_occ, BLK / 64)), dim3(BLK), 0, s, G.pts, G.cell_start, ndt->occ.as<uint32_t>(), n_occ, (int)ndt->prm.min_points,
                           ndt->prm.min_eig_ratio, ndt->tmp.as<double>(), ndt->is_voxel.as<uint32_t>());
        SF_TRY(sf::scan_u32<0>(ctx, ndt->is_voxel.as<uint32_t>(), ndt->vpos.as<uint32_t>(), n_occ));
        hipLaunchKernelGGL(k_ndt_compact, dim3(ndt_blocks(n_occ, 256)), dim3(256), 0, s, ndt->occ.as<uint32_t>(), ndt->is_voxel.as<uint32_t>(), ndt->vpos.as<uint32_t>(), n_occ,
                           ndt->tmp.as<double>(), ndt->vox.as<double>(), ndt->cov.as<double>(), ndt->vcell.as<int64_t>(), ndt->vcount.as<int32_t>(),
                           ndt->cell_voxel.as<int32_t>());
        SF_HIP(hipGetLastError());
        SF_TRY(ndt_mark(ndt, 1));
        SF_HIP(hipMemcpyAsync(&last[0], ndt->vpos.as<uint32_t>() + (n_occ - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        SF_HIP(hipMemcpyAsync(&last[1], ndt->is_voxel.as<uint32_t>() + (n_occ - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        SF_HIP(hipStreamSynchronize(s));
        n_vox = (int64_t)last[0] + (int64_t)last[1];
    } else {
        SF_HIP(hipGetLastError());
        SF_TRY(ndt_mark(ndt, 1));
        SF_HIP(hipStreamSynchronize(s));
    }
    SF_TRY(ndt_event_ms(ndt, &ndt->build_ms));
    ndt->n_points = cloud->n;
    ndt->n_cells = nc;
    ndt->n_occupied = n_occ;
    ndt->n_voxels = n_vox;
    ndt->has_target = true;
    return SF_OK;
}

NdtGrid ndt_grid(const sf_ndt *ndt)
{
    const SfGrid &G = ndt->index->grid;
    NdtGrid g;
    for (int d = 0; d < 3; ++d) { g.org[d] = (double)G.org[d]; g.dim[d] = G.dim[d]; }
    g.inv_h = (double)G.inv_h;
    g.cell_voxel = ndt->cell_voxel.as<int32_t>();
    g.vox = ndt->vox.as<double>();
    return g;
}

void ndt_launch_derivs(sf_ndt *ndt, const NdtGrid &g, const NdtConst &cn, int entries, size_t src_stride, int force, int nblocks)
{
    hipStream_t s = ndt->ctx->stream;
    const dim3 grid((unsigned)nblocks, (unsigned)entries);
    if (ndt->prm.neighbours == SF_NDT_DIRECT7)
        hipLaunchKernelGGL(k_ndt_derivs<7>, grid, dim3(BLK), 0, s, g, cn, ndt->src.as<float>(), (int)ndt->n_src, src_stride, ndt->state.as<NdtState>(), force,
                           ndt->partials.as<double>(), nblocks);
    else
        hipLaunchKernelGGL(k_ndt_derivs<1>, grid, dim3(BLK), 0, s, g, cn, ndt->src.as<float>(), (int)ndt->n_src, src_stride, ndt->state.as<NdtState>(), force,
                           ndt->partials.as<double>(), nblocks);
}

void ndt_result(const NdtState &S, sf_ndt_result *o)
{
    for (int i = 0; i < 16; ++i) o->T[i] = S.T[i];
    o->score = S.score;
    for (int i = 0; i < 6; ++i) o->gradient[i] = S.g[i];
    for (int i = 0; i < 36; ++i) o->hessian[i] = S.H[i];
    o->n_inside = (int64_t)S.n_inside;
    o->n_terms = (int64_t)S.n_terms;
    o->iterations = S.iterations;
    o->converged = S.converged;
    o->modified = S.modified;
    o->flags = S.flags;
}

int ndt_reserve_run(sf_ndt *ndt, int entries, int nblocks)
{
    SF_TRY(ndt->state.reserve(sizeof(NdtState) * (size_t)entries));
    SF_TRY(ndt->partials.reserve(sizeof(double) * REC_STRIDE * (size_t)nblocks * (size_t)entries));
    return SF_OK;
}

// the scores of gridDim.y * gridDim.z poses in one launch: pose (y, z) at poses + y * pose_stride + 16 z, its rows at slab y * nz + z
void ndt_launch_scores(sf_ndt *ndt, const NdtGrid &g, const NdtConst &cn, int ny, int nz, size_t src_stride, const NdtState *done, const double *poses, size_t pose_stride,
                       double *partials, int nblocks)
{
    hipStream_t s = ndt->ctx->stream;
    const dim3 grid((unsigned)nblocks, (unsigned)ny, (unsigned)nz);
    if (ndt->prm.neighbours == SF_NDT_DIRECT7)
        hipLaunchKernelGGL(k_ndt_scores<7>, grid, dim3(BLK), 0, s, g, cn, ndt->src.as<float>(), (int)ndt->n_src, src_stride, done, poses, pose_stride, partials, nblocks);
    else
        hipLaunchKernelGGL(k_ndt_scores<1>, grid, dim3(BLK), 0, s, g, cn, ndt->src.as<float>(), (int)ndt->n_src, src_stride, done, poses, pose_stride, partials, nblocks);
}

// entries states start at `poses` [entries][16]; iterations > 0: the Newton loop first; then the derivatives at the final poses
// with the line search on, an iteration is (k_ndt_derivs, k_ndt_step_ls, k_ndt_scores, k_ndt_pick); want_rows: the rows of entry 0
int ndt_run(sf_ndt *ndt, const double *poses, int entries, size_t src_stride, int iterations, bool timed, sf_ndt_result *out, double *trace, bool want_rows = false)
{
    sf_ctx *ctx = ndt->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int nblocks = (int)ndt_blocks(ndt->n_src, BLK);
    SF_TRY(ndt_reserve_run(ndt, entries, nblocks));
    std::vector<NdtState> h((size_t)entries);
    for (int b = 0; b < entries; ++b) {
        std::memset(&h[(size_t)b], 0, sizeof(NdtState));
        for (int i = 0; i < 16; ++i) h[(size_t)b].T[i] = poses[16 * (size_t)b + i];
    }
    double *d_trace = nullptr;
    if (trace) {
        SF_TRY(ndt->trace.reserve(sizeof(double) * 16 * (size_t)(iterations + 1)));
        d_trace = ndt->trace.as<double>();
    }
    const int trials = iterations > 0 ? (int)ndt->ls.trials : 0;
    sf_ndt_ls_row *d_rows = nullptr;
    if (want_rows) ndt->has_rows = false;
    if (trials > 0) {
        SF_TRY(ndt->ls_entry.reserve(sizeof(NdtLsEntry) * (size_t)entries));
        SF_TRY(ndt->ls_partials.reserve(sizeof(double) * REC_STRIDE * (size_t)nblocks * (size_t)trials * (size_t)entries));
        if (want_rows) {
            SF_TRY(ndt->ls_rows.reserve(sizeof(sf_ndt_ls_row) * (size_t)iterations));
            d_rows = ndt->ls_rows.as<sf_ndt_ls_row>();
        }
    }
    SF_TRY(sf::upload_staged(ctx, ndt->state.p, h.data(), sizeof(NdtState) * (size_t)entries));
    const NdtGrid g = ndt_grid(ndt);
    const NdtConst cn = ndt_constants(ndt->prm);
    const NdtStepArg sa{ndt->prm.step_size, ndt->prm.transformation_epsilon, ndt->prm.hessian_floor};
    SF_TRY(ndt_mark(ndt, 0));
    const NdtLsArg la{ndt->ls.step_max, ndt->ls.armijo, ndt->prm.transformation_epsilon, ndt->prm.hessian_floor, trials};
    for (int it = 0; it < iterations; ++it) {
        ndt_launch_derivs(ndt, g, cn, entries, src_stride, 0, nblocks);
        if (trials == 0) {
            hipLaunchKernelGGL(k_ndt_step, dim3((unsigned)entries), dim3(NDT_SBLK), 0, s, ndt->state.as<NdtState>(), ndt->partials.as<double>(), nblocks, sa, it, 0, d_trace);
            continue;
        }
        hipLaunchKernelGGL(k_ndt_step_ls, dim3((unsigned)entries), dim3(NDT_SBLK), 0, s, ndt->state.as<NdtState>(), ndt->partials.as<double>(), nblocks, la, it,
                           ndt->ls_entry.as<NdtLsEntry>(), d_rows);
        ndt_launch_scores(ndt, g, cn, entries, trials, src_stride, ndt->state.as<NdtState>(), reinterpret_cast<const double *>(ndt->ls_entry.p), sizeof(NdtLsEntry) / sizeof(double),
                          ndt->ls_partials.as<double>(), nblocks);
        hipLaunchKernelGGL(k_ndt_pick, dim3((unsigned)entries), dim3(NDT_SBLK), 0, s, ndt->state.as<NdtState>(), ndt->ls_partials.as<double>(), nblocks, la, it,
                           ndt->ls_entry.as<NdtLsEntry>(), d_trace, d_rows);
    }
    ndt_launch_derivs(ndt, g, cn, entries, src_stride, 1, nblocks);
    hipLaunchKernelGGL(k_ndt_step, dim3((unsigned)entries), dim3(NDT_SBLK), 0, s, ndt->state.as<NdtState>(), ndt->partials.as<double>(), nblocks, sa, iterations, 1, d_trace);
    SF_HIP(hipGetLastError());
    SF_TRY(ndt_mark(ndt, 1));
    SF_HIP(hipMemcpyAsync(h.data(), ndt->state.p, sizeof(NdtState) * (size_t)entries, hipMemcpyDeviceToHost, s));
    SF_HIP(hipStreamSynchronize(s));
    if (timed) SF_TRY(ndt_event_ms(ndt, &ndt->align_ms));
    for (int b = 0; b < entries; ++b) ndt_result(h[(size_t)b], out + b);
    if (trace) {
        for (int i = 0; i < 16; ++i) trace[i] = poses[i];
        const int rows = out[0].iterations;
        if (rows > 0) SF_HIP(hipMemcpy(trace + 16, d_trace + 16, sizeof(double) * 16 * (size_t)rows, hipMemcpyDeviceToHost));
    }
    if (d_rows) { // one row per iteration whose trials were evaluated: the steps taken and the stalled one
        const int rows = out[0].iterations + ((out[0].flags & SF_NDT_FLAG_LINE_SEARCH_STALLED) ? 1 : 0);
        ndt->rows.resize((size_t)rows);
        if (rows > 0) SF_HIP(hipMemcpy(ndt->rows.data(), d_rows, sizeof(sf_ndt_ls_row) * (size_t)rows, hipMemcpyDeviceToHost));
        ndt->has_rows = true;
    }
    return SF_OK;
}

int ndt_check_line_search(const sf_ndt_line_search *p)
{
    SF_CHECK(p->trials >= 0 && p->trials <= SF_NDT_MAX_TRIALS, SF_ERR_INVALID, "bad arguments: ndt line search trials must be 0 .. 16 (got %d)", (int)p->trials);
    SF_CHECK(std::isfinite(p->step_max) && p->step_max > 0.0, SF_ERR_INVALID, "bad arguments: ndt line search step_max must be positive and finite (got %g)", p->step_max);
    SF_CHECK(p->armijo > 0.0 && p->armijo < 1.0, SF_ERR_INVALID, "bad arguments: ndt line search armijo must lie in (0, 1) (got %g)", p->armijo);
    return SF_OK;
}

} // namespace

extern "C" void sf_ndt_default_params(sf_ndt_params *p)
{
    if (!p) return;
    *p = sf_ndt_params{1.0, 0.55, 0.1, 1e-4, 0.01, 1e-6, 6, SF_NDT_DIRECT7, 30, 0};
}

extern "C" int sf_ndt_create(sf_ctx *ctx, const sf_ndt_params *p, sf_ndt **out)
{
    SF_CHECK(ctx && p && out, SF_ERR_INVALID, "bad arguments");
    SF_TRY(ndt_check_params(p));
    sf_ndt *ndt = new (std::nothrow) sf_ndt();
    SF_CHECK(ndt, SF_ERR_NOMEM, "out of host memory");
    ndt->ctx = ctx;
    ndt->prm = *p;
    sf::ctx_retain(ctx);
    *out = ndt;
    return SF_OK;
}

extern "C" void sf_ndt_destroy(sf_ndt *ndt)
{
    if (!ndt) return;
    hipError_t e = hipStreamSynchronize(ndt->ctx->stream);
    (void)e;
    if (ndt->index) sf_map_destroy(ndt->index);
    if (ndt->points) sf_cloud_destroy(ndt->points);
    for (hipEvent_t ev : ndt->ev)
        if (ev) { hipError_t e2 = hipEventDestroy(ev); (void)e2; }
    sf_ctx *ctx = ndt->ctx;
    delete ndt;
    sf::ctx_release(ctx);
}

extern "C" int sf_ndt_set_target_cloud(sf_ndt *ndt, sf_cloud *cloud)
{
    SF_CHECK(ndt && cloud, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(cloud->ctx == ndt->ctx, SF_ERR_INVALID, "bad arguments: the cloud belongs to another context");
    SF_HIP(hipSetDevice(ndt->ctx->device));
    return ndt_build(ndt, cloud);
}

extern "C" int sf_ndt_set_target_map(sf_ndt *ndt, sf_map *map)
{
    SF_CHECK(ndt && map, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(map->ctx == ndt->ctx, SF_ERR_INVALID, "bad arguments: the map belongs to another context");
    SF_CHECK(map->built, SF_ERR_STATE, "map not built");
    sf_ctx *ctx = ndt->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    if (ndt->points) { sf_cloud_destroy(ndt->points); ndt->points = nullptr; }
    SF_TRY(sf_cloud_create(ctx, &ndt->points));
    sf_cloud *c = ndt->points;
    const int64_t n = map->n;
    SF_TRY(c->xyz.reserve(sizeof(float) * 3 * (size_t)std::max<int64_t>(n, 1)));
    if (n > 0) {
        hipLaunchKernelGGL(k_ndt_unsort, dim3(ndt_blocks(n, 256)), dim3(256), 0, ctx->stream, map->grid.pts, n, c->xyz.as<float>());
        SF_HIP(hipGetLastError());
    }
    c->n = n;
    sf::cloud_touch(c);
    return ndt_build(ndt, c);
}

extern "C" int sf_ndt_download_voxels(sf_ndt *ndt, int64_t *cell, int32_t *count, double *mean, double *cov, double *icov, int64_t cap, int64_t *n)
{
    SF_CHECK(ndt, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(ndt->has_target, SF_ERR_INVALID, "bad arguments: ndt has no target");
    const int64_t nv = ndt->n_voxels;
    if (n) *n = nv;
    SF_CHECK(cap >= nv || !(cell || count || mean || cov || icov), SF_ERR_INVALID, "bad arguments: cap %lld is below the %lld voxels", (long long)cap, (long long)nv);
    if (nv == 0) return SF_OK;
    sf_ctx *ctx = ndt->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    if (cell) SF_HIP(hipMemcpy(cell, ndt->vcell.p, sizeof(int64_t) * (size_t)nv, hipMemcpyDeviceToHost));
    if (count) SF_HIP(hipMemcpy(count, ndt->vcount.p, sizeof(int32_t) * (size_t)nv, hipMemcpyDeviceToHost));
    if (cov) SF_HIP(hipMemcpy(cov, ndt->cov.p, sizeof(double) * 6 * (size_t)nv, hipMemcpyDeviceToHost));
    if (mean || icov) {
        std::vector<double> rec((size_t)nv * NDT_VOX_STRIDE);
        SF_HIP(hipMemcpy(rec.data(), ndt->vox.p, sizeof(double) * rec.size(), hipMemcpyDeviceToHost));
        for (int64_t v = 0; v < nv; ++v) {
            const double *r = rec.data() + (size_t)v * NDT_VOX_STRIDE;
            if (mean) for (int d = 0; d < 3; ++d) mean[3 * v + d] = r[d];
            if (icov) for (int e = 0; e < 6; ++e) icov[6 * v + e] = r[3 + e];
        }
    }
    return SF_OK;
}

extern "C" int sf_ndt_set_source_batch(sf_ndt *ndt, const float *xyz, int64_t n_per_scan, int batch)
{
    SF_CHECK(ndt && n_per_scan >= 0 && (xyz || n_per_scan == 0), SF_ERR_INVALID, "bad arguments");
    SF_CHECK(batch >= 1 && batch <= NDT_MAX_BATCH, SF_ERR_INVALID, "bad arguments: ndt batch must be 1 .. 64 (got %d)", batch);
    SF_CHECK(n_per_scan < (int64_t)1 << 30, SF_ERR_INVALID, "bad arguments: ndt source of %lld points", (long long)n_per_scan);
    sf_ctx *ctx = ndt->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    const size_t bytes = sizeof(float) * 3 * (size_t)n_per_scan * (size_t)batch;
    SF_TRY(ndt->src.reserve(std::max<size_t>(bytes, 16)));
    SF_TRY(sf::upload_staged(ctx, ndt->src.p, xyz, bytes));
    ndt->n_src = n_per_scan;
    ndt->batch = batch;
    ndt->has_source = true;
    return SF_OK;
}

extern "C" int sf_ndt_set_source_cloud(sf_ndt *ndt, sf_cloud *cloud)
{
    SF_CHECK(ndt && cloud, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(cloud->ctx == ndt->ctx, SF_ERR_INVALID, "bad arguments: the cloud belongs to another context");
    SF_CHECK(cloud->n < (int64_t)1 << 30, SF_ERR_INVALID, "bad arguments: ndt source of %lld points", (long long)cloud->n);
    sf_ctx *ctx = ndt->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    const size_t bytes = sizeof(float) * 3 * (size_t)cloud->n;
    SF_TRY(ndt->src.reserve(std::max<size_t>(bytes, 16)));
    if (bytes) SF_HIP(hipMemcpyAsync(ndt->src.p, cloud->xyz.p, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    ndt->n_src = cloud->n;
    ndt->batch = 1;
    ndt->has_source = true;
    return SF_OK;
}

extern "C" int sf_ndt_derivatives(sf_ndt *ndt, const double *poses, int64_t k, sf_ndt_result *out)
{
    SF_CHECK(ndt && k >= 0 && ((poses && out) || k == 0), SF_ERR_INVALID, "bad arguments");
    SF_CHECK(ndt->has_target && ndt->has_source, SF_ERR_INVALID, "bad arguments: ndt needs a target and a source first");
    for (int64_t at = 0; at < k; at += NDT_MAX_BATCH) {
        const int chunk = (int)std::min<int64_t>(NDT_MAX_BATCH, k - at);
        SF_TRY(ndt_run(ndt, poses + 16 * at, chunk, 0, 0, true, out + at, nullptr)); // every pose reads entry 0 of the source
    }
    return SF_OK;
}

extern "C" int sf_ndt_align_batch(sf_ndt *ndt, const double *inits, sf_ndt_result *out)
{
    SF_CHECK(ndt && inits && out, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(ndt->has_target && ndt->has_source, SF_ERR_INVALID, "bad arguments: ndt needs a target and a source first");
    return ndt_run(ndt, inits, ndt->batch, 3 * (size_t)ndt->n_src, (int)ndt->prm.max_iterations, true, out, nullptr);
}

extern "C" int sf_ndt_align(sf_ndt *ndt, const double init[16], sf_ndt_result *out, double *trace)
{
    SF_CHECK(ndt && init && out, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(ndt->has_target && ndt->has_source, SF_ERR_INVALID, "bad arguments: ndt needs a target and a source first");
    return ndt_run(ndt, init, 1, 3 * (size_t)ndt->n_src, (int)ndt->prm.max_iterations, true, out, trace, true);
}

extern "C" int sf_ndt_stats_read(sf_ndt *ndt, sf_ndt_stats *out)
{
    SF_CHECK(ndt && out, SF_ERR_INVALID, "bad arguments");
    *out = sf_ndt_stats{ndt->n_points, ndt->n_cells, ndt->n_occupied, ndt->n_voxels, {0, 0, 0}, ndt->build_ms, ndt->align_ms};
    if (ndt->has_target)
        for (int d = 0; d < 3; ++d) out->dims[d] = ndt->index->grid.dim[d];
    return SF_OK;
}

extern "C" void sf_ndt_default_line_search(sf_ndt_line_search *p)
{
    if (!p) return;
    *p = sf_ndt_line_search{8, 0, 1.0, 1e-4};
}

extern "C" int sf_ndt_set_line_search(sf_ndt *ndt, const sf_ndt_line_search *p)
{
    SF_CHECK(ndt, SF_ERR_INVALID, "bad arguments");
    if (p) SF_TRY(ndt_check_line_search(p));
    if (p && p->trials > 0) ndt->ls = sf_ndt_line_search{p->trials, 0, p->step_max, p->armijo};
    else ndt->ls.trials = 0;
    return SF_OK;
}

extern "C" int sf_ndt_scores(sf_ndt *ndt, const double *poses, int64_t k, double *score, int64_t *n_terms)
{
    SF_CHECK(ndt && k >= 0 && ((poses && score && n_terms) || k == 0), SF_ERR_INVALID, "bad arguments");
    SF_CHECK(ndt->has_target && ndt->has_source, SF_ERR_INVALID, "bad arguments: ndt needs a target and a source first");
    if (k == 0) return SF_OK;
    sf_ctx *ctx = ndt->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int nblocks = (int)ndt_blocks(ndt->n_src, BLK);
    const int64_t cap = std::min<int64_t>(k, NDT_MAX_BATCH * SF_NDT_MAX_TRIALS); // poses per launch
    SF_TRY(ndt->poses.reserve(sizeof(double) * 16 * (size_t)cap));
    SF_TRY(ndt->scores.reserve(sizeof(double) * 2 * (size_t)cap));
    SF_TRY(ndt->ls_partials.reserve(sizeof(double) * REC_STRIDE * (size_t)nblocks * (size_t)cap));
    const NdtGrid g = ndt_grid(ndt);
    const NdtConst cn = ndt_constants(ndt->prm);
    std::vector<double> h(2 * (size_t)cap);
    for (int64_t at = 0; at < k; at += cap) {
        const int chunk = (int)std::min<int64_t>(cap, k - at);
        SF_TRY(sf::upload_staged(ctx, ndt->poses.p, poses + 16 * at, sizeof(double) * 16 * (size_t)chunk));
        SF_TRY(ndt_mark(ndt, 0));
        ndt_launch_scores(ndt, g, cn, chunk, 1, 0, nullptr, ndt->poses.as<double>(), 16, ndt->ls_partials.as<double>(), nblocks); // every pose reads entry 0 of the source
        hipLaunchKernelGGL(k_ndt_scores_out, dim3((unsigned)chunk), dim3(NDT_SBLK), 0, s, ndt->ls_partials.as<double>(), nblocks, ndt->scores.as<double>());
        SF_HIP(hipGetLastError());
        SF_TRY(ndt_mark(ndt, 1));
        SF_HIP(hipMemcpyAsync(h.data(), ndt->scores.p, sizeof(double) * 2 * (size_t)chunk, hipMemcpyDeviceToHost, s));
        SF_HIP(hipStreamSynchronize(s));
        SF_TRY(ndt_event_ms(ndt, &ndt->align_ms));
        for (int i = 0; i < chunk; ++i) {
            score[at + i] = h[2 * (size_t)i];
            n_terms[at + i] = (int64_t)h[2 * (size_t)i + 1];
        }
    }
    return SF_OK;
}

extern "C" int sf_ndt_line_search_read(sf_ndt *ndt, sf_ndt_ls_row *rows, int64_t cap, int64_t *n)
{
    SF_CHECK(ndt, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(ndt->has_rows, SF_ERR_STATE, "ndt: no sf_ndt_align with the line search on has run");
    const int64_t have = (int64_t)ndt->rows.size();
    if (n) *n = have;
    SF_CHECK(!rows || cap >= have, SF_ERR_INVALID, "bad arguments: cap %lld is below the %lld rows", (long long)cap, (long long)have);
    if (rows) std::copy(ndt->rows.begin(), ndt->rows.end(), rows);
    return SF_OK;
}

extern "C" int sf_ndt_align_levels(sf_ndt *const *levels, int n_levels, const double *inits, sf_ndt_result *out, sf_ndt_result *per_level)
{
    SF_CHECK(levels && inits && out, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(n_levels >= 1, SF_ERR_INVALID, "bad arguments: ndt needs at least one level (got %d)", n_levels);
    for (int l = 0; l < n_levels; ++l) {
        const sf_ndt *a = levels[l], *f = levels[0];
        SF_CHECK(a, SF_ERR_INVALID, "bad arguments");
        SF_CHECK(a->has_target && a->has_source, SF_ERR_INVALID, "bad arguments: ndt level %d needs a target and a source first", l);
        SF_CHECK(a->ctx == f->ctx, SF_ERR_INVALID, "bad arguments: ndt level %d belongs to another context", l);
        SF_CHECK(a->batch == f->batch && a->n_src == f->n_src, SF_ERR_INVALID, "bad arguments: ndt level %d holds %d scans of %lld points, level 0 %d of %lld", l, a->batch,
                 (long long)a->n_src, f->batch, (long long)f->n_src);
    }
    const int batch = levels[0]->batch;
    std::vector<double> poses(inits, inits + 16 * (size_t)batch);
    std::vector<sf_ndt_result> res((size_t)batch);
    for (int l = 0; l < n_levels; ++l) {
        sf_ndt *ndt = levels[l];
        SF_TRY(ndt_run(ndt, poses.data(), batch, 3 * (size_t)ndt->n_src, (int)ndt->prm.max_iterations, true, res.data(), nullptr));
        for (int b = 0; b < batch; ++b) {
            for (int i = 0; i < 16; ++i) poses[16 * (size_t)b + i] = res[(size_t)b].T[i];
            if (per_level) per_level[(size_t)l * batch + b] = res[(size_t)b];
        }
    }
    for (int b = 0; b < batch; ++b) out[b] = res[(size_t)b];
    return SF_OK;
}
