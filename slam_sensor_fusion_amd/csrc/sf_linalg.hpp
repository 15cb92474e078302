// sf_linalg.hpp -- the small float64 linear algebra of the numerical core, each routine on ONE lane with its little matrices in
// registers: mat4_mul, the one-sided Jacobi SVD of a 3 x 3 (jacobi_pair, swap_cols_if_less, svd3), kabsch_from_record, ldlt6 and
// vec6_to_mat4; rsqrt_nr and jacobi_sym come with it through sf_jacobi.hpp.  Like sf_jacobi.hpp it is included INSIDE the anonymous
// namespace of the translation unit that uses it, so the routines keep internal linkage: sf_icp.hip (the solves of an iteration,
// sf_cov.hpp, the hooks of sf_icp_testhooks.hpp, which pin every routine: tests/test_gpu_linalg_direct.py) and sf_ndt.hip (the pose
// update of a Newton step).  It needs nothing of either; a unit that includes it has included <cfloat> and <cmath> before it opens
// its namespace.  The fixed-order reductions are sf_reduce.hpp.
#pragma once

// ------------------------------------------------------------------ small device linear algebra (one lane)
// Every loop below has compile-time bounds and is fully unrolled so the little matrices
// live in registers (runtime-indexed arrays would go to scratch memory).
__device__ __forceinline__ void mat4_mul(const double A[16], const double B[16], double C[16])
{
    double R[16];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            R[4 * r + c] = A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c] + A[4 * r + 2] * B[8 + c] + A[4 * r + 3] * B[12 + c];
#pragma unroll
    for (int i = 0; i < 16; ++i) C[i] = R[i];
}

// rsqrt_nr (and the symmetric Jacobi of k_cov_solve, sf_cov.hpp): shared with sf_map.hip
#include "sf_jacobi.hpp"

// One Hestenes rotation of columns P, Q (the smaller angle): with al = |u_P|^2, be = |u_Q|^2, ga = u_P . u_Q,
// cos 2t = |be - al| / w, sin 2t = 2 ga sgn(be - al) / w, w = sqrt((be - al)^2 + 4 ga^2); c = sqrt((1 + cos 2t) / 2),
// s = sin 2t / (2 c) -- two reciprocal square roots, no divide.
template <int P, int Q>
__device__ __forceinline__ bool jacobi_pair(double (&u)[9], double (&v)[9])
{
    double al = 0, be = 0, ga = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        al += u[3 * i + P] * u[3 * i + P];
        be += u[3 * i + Q] * u[3 * i + Q];
        ga += u[3 * i + P] * u[3 * i + Q];
    }
    if (ga * ga <= (DBL_EPSILON * DBL_EPSILON) * (al * be) || fabs(ga) < 1e-150) return false;
    const double tau = be - al;
    const double r = rsqrt_nr(tau * tau + 4.0 * ga * ga);
    const double c2 = 0.5 + 0.5 * fabs(tau) * r;
    const double rc = rsqrt_nr(c2);
    const double c = c2 * rc, s = (tau >= 0 ? ga : -ga) * r * rc;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double a = u[3 * i + P], b = u[3 * i + Q];
        u[3 * i + P] = c * a - s * b;
        u[3 * i + Q] = s * a + c * b;
        a = v[3 * i + P]; b = v[3 * i + Q];
        v[3 * i + P] = c * a - s * b;
        v[3 * i + Q] = s * a + c * b;
    }
    return true;
}

template <int A, int B>
__device__ __forceinline__ void swap_cols_if_less(double (&s)[3], double (&u)[9], double (&v)[9], double (&inv)[3])
{
    if (s[B] > s[A]) {
        double t = s[A]; s[A] = s[B]; s[B] = t;
        t = inv[A]; inv[A] = inv[B]; inv[B] = t;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            t = u[3 * i + A]; u[3 * i + A] = u[3 * i + B]; u[3 * i + B] = t;
            t = v[3 * i + A]; v[3 * i + A] = v[3 * i + B]; v[3 * i + B] = t;
        }
    }
}

// one-sided Jacobi SVD of a 3x3 (row-major), S descending — stands in for
// Eigen::JacobiSVD<Matrix3f> at icp_point_to_point.cpp:137 (float64 here).
// Domain: |A| = 0 or 1e-60 <= |A| <= 1e60 (tests/test_gpu_linalg_direct.py::test_svd3_supported_scale_range).  jacobi_pair
// works on SQUARED column norms: below |A| ~ 1e-67 its |ga| < 1e-150 guard ends the sweeps before the columns are orthogonal
// to eps (from 1e-75 down nothing rotates: V = I, S = the column norms, and n2 > 1e-300 zeroes S below 1e-150); above
// |A| ~ 1e77 the product al * be overflows, inf <= inf skips every rotation and the result is finite and WRONG.  H of a Kabsch
// step is a sum of products of metres and never comes near either end.  Columns whose singular value is below 8 eps S0 are
// completed, not normalised: rank 0 gives U = I, rank 1 a unit vector orthogonal to the first column and then the cross
// product, rank 2 the cross product -- U is orthonormal with det +1 whenever the rank is below 3.
__device__ __forceinline__ void svd3(const double (&A)[9], double (&U)[9], double (&S)[3], double (&V)[9])
{
#pragma unroll
    for (int i = 0; i < 9; ++i) { U[i] = A[i]; V[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = jacobi_pair<0, 1>(U, V);
        rotated = jacobi_pair<0, 2>(U, V) || rotated;
        rotated = jacobi_pair<1, 2>(U, V) || rotated;
        if (!rotated) break;
    }
    double invS[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double n2 = U[j] * U[j] + U[3 + j] * U[3 + j] + U[6 + j] * U[6 + j];
        invS[j] = n2 > 1e-300 ? rsqrt_nr(n2) : 0.0;
        S[j] = n2 * invS[j];
    }
    swap_cols_if_less<0, 1>(S, U, V, invS);
    swap_cols_if_less<0, 2>(S, U, V, invS);
    swap_cols_if_less<1, 2>(S, U, V, invS);
    const double thr = S[0] * DBL_EPSILON * 8;
    int rank = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (S[j] > thr && S[j] > 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) U[3 * i + j] *= invS[j];
            ++rank;
        }
    if (rank == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) U[i] = (i % 4 == 0) ? 1.0 : 0.0;
    }
    if (rank == 1) {
        const double a0 = U[0], a1 = U[3], a2 = U[6];
        double b0, b1, b2;
        if (fabs(a0) <= fabs(a1) && fabs(a0) <= fabs(a2)) { b0 = 0; b1 = -a2; b2 = a1; }
        else if (fabs(a1) <= fabs(a2)) { b0 = -a2; b1 = 0; b2 = a0; }
        else { b0 = -a1; b1 = a0; b2 = 0; }
        const double nb = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
        U[1] = b0 / nb; U[4] = b1 / nb; U[7] = b2 / nb;
        rank = 2;
    }
    if (rank == 2) {
        U[2] = U[3] * U[7] - U[6] * U[4];
        U[5] = U[6] * U[1] - U[0] * U[7];
        U[8] = U[0] * U[4] - U[3] * U[1];
    }
}

// Kabsch step (icp_point_to_point.cpp:112-159) from the uncentred sums of the record:
// rec[0]=n, [1..3]=sum s, [4..6]=sum t, [7..15]=sum s t^T.  H = sum s t^T - n cs ct^T.
__device__ __forceinline__ void kabsch_from_record(const double *rec, double (&T)[16])
{
    const double n = rec[0];
    double cs[3], ct[3], H[9];
    const double inv_n = 1.0 / n;
#pragma unroll
    for (int d = 0; d < 3; ++d) { cs[d] = rec[1 + d] * inv_n; ct[d] = rec[4 + d] * inv_n; }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) H[3 * r + c] = rec[7 + 3 * r + c] - n * cs[r] * ct[c];
    double U[9], S[3], V[9], R[9];
    svd3(H, U, S, V);
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                R[3 * r + c] = V[3 * r] * U[3 * c] + V[3 * r + 1] * U[3 * c + 1] + V[3 * r + 2] * U[3 * c + 2];
        const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
        if (pass == 1 || !(det < 0)) break;
        V[2] = -V[2]; V[5] = -V[5]; V[8] = -V[8];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) T[i] = 0;
    T[15] = 1;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) T[4 * r + c] = R[3 * r + c];
        T[4 * r + 3] = ct[r] - (R[3 * r] * cs[0] + R[3 * r + 1] * cs[1] + R[3 * r + 2] * cs[2]);
    }
}

__device__ __forceinline__ int ldlt6(const double (&A)[36], const double (&b)[6], double (&x)[6])
{
    double L[36], D[6], y[6];
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 36; ++i) L[i] = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = A[6 * j + j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[6 * j + k] * L[6 * j + k] * D[k];
        if (!(fabs(d) > 0) || !isfinite(d)) bad = true;
        D[j] = d;
        L[6 * j + j] = 1;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = A[6 * i + j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[6 * i + k] * L[6 * j + k] * D[k];
            L[6 * i + j] = v / d;
        }
    }
    if (bad) return -1;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= L[6 * i + k] * y[k];
        y[i] = v;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) y[i] /= D[i];
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v -= L[6 * k + i] * x[k];
        x[i] = v;
    }
    return 0;
}

// R = Rz(v2) Ry(v1) Rx(v0), t = v[3:6] (Open3D TransformVector6dToMatrix4d)
__device__ __forceinline__ void vec6_to_mat4(const double (&v)[6], double (&T)[16])
{
    double ca, sa, cb, sb, cg, sg; // one range reduction per angle
    sincos(v[0], &sa, &ca);
    sincos(v[1], &sb, &cb);
    sincos(v[2], &sg, &cg);
    const double R[9] = {cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa,
                         sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa,
                         -sb, cb * sa, cb * ca};
#pragma unroll
    for (int i = 0; i < 16; ++i) T[i] = 0;
    T[15] = 1;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) T[4 * r + c] = R[3 * r + c];
        T[4 * r + 3] = v[3 + r];
    }
}
