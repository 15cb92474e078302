// sf_jacobi.hpp -- rsqrt_nr and the symmetric Jacobi eigen-solve, N x N in registers.  Included inside the anonymous namespace of
// the translation units that use them: through sf_linalg.hpp (svd3) sf_icp.hip (also k_cov_solve of sf_cov.hpp and the hooks of
// sf_icp_testhooks.hpp) and sf_ndt.hip (the voxel and Newton-step solves); directly sf_map.hip (the per-label boxes of sf_box.hpp),
// sf_register.hip and sf_keypoint.hip.  One implementation; tests/test_gpu_linalg_direct.py pins it through sf_icp.hip.
#pragma once
#include <cfloat>

// 1 / sqrt(x) for NORMAL x in [DBL_MIN, 1e300]: the hardware estimate and two Newton steps, within 2 ulp of the exact
// value over that whole range (measured 2.0 ulp; recip_nr = its square: within 5 ulp, measured 4.0).  Outside the
// domain -- 0, subnormals, inf, negative x, NaN -- the estimate is inf / 0 / NaN and the Newton steps make NaN of inf * 0:
// every caller guards (svd3 by n2 > 1e-300, jacobi_pair / jacobi_sym_pair by their skip tests, k_cov_solve by its eigenvalue
// floor and by W > 0).
// The solve runs on ONE lane while the rest of its workgroup -- on the per-scan path the whole grid -- waits, so the
// float64 divide / sqrt expansions (a few dozen dependent instructions each) are what an iteration's controller costs:
// measured 6.2 us per controller step with divides and square roots, 3.2-4.0 us with this.
__device__ __forceinline__ double rsqrt_nr(double x)
{
    double y = __builtin_amdgcn_rsq(x);
    y = y * fma(-0.5 * x * y, y, 1.5);
    y = y * fma(-0.5 * x * y, y, 1.5);
    return y;
}

// ------------------------------------------------------------------ symmetric Jacobi, N x N in registers
// One two-sided rotation of the pair (P, Q): A <- G^T A G with G's column P = c e_P - s e_Q and column Q = s e_P + c e_Q, the
// smaller angle of tan 2t = 2 a_PQ / (a_QQ - a_PP) -- the rotation of sf_icp.hip's jacobi_pair, from two reciprocal square roots.
// Everything is indexed at compile time (P, Q template parameters, loops unrolled): the matrices stay in registers.
template <int N, int P, int Q>
__device__ __forceinline__ bool jacobi_sym_pair(double (&A)[N * N], double (&V)[N * N])
{
    const double al = A[P * N + P], be = A[Q * N + Q], ga = A[P * N + Q];
    if (ga * ga <= (DBL_EPSILON * DBL_EPSILON) * fabs(al * be) || fabs(ga) < 1e-150) return false;
    const double tau = be - al;
    const double r = rsqrt_nr(fma(tau, tau, 4.0 * ga * ga));
    const double c2 = 0.5 + 0.5 * fabs(tau) * r;
    const double rc = rsqrt_nr(c2);
    const double c = c2 * rc, s = (tau >= 0 ? ga : -ga) * r * rc;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (k != P && k != Q) {
            const double a = A[k * N + P], b = A[k * N + Q];
            const double na = fma(c, a, -(s * b)), nb = fma(s, a, c * b);
            A[k * N + P] = na; A[P * N + k] = na;
            A[k * N + Q] = nb; A[Q * N + k] = nb;
        }
        const double va = V[k * N + P], vb = V[k * N + Q];
        V[k * N + P] = fma(c, va, -(s * vb));
        V[k * N + Q] = fma(s, va, c * vb);
    }
    const double cs2 = 2.0 * c * s * ga;
    A[P * N + P] = fma(c * c, al, fma(s * s, be, -cs2));
    A[Q * N + Q] = fma(s * s, al, fma(c * c, be, cs2));
    A[P * N + Q] = 0.0; A[Q * N + P] = 0.0;
    return true;
}

template <int N, int P, int Q>
__device__ __forceinline__ bool jacobi_sym_sweep(double (&A)[N * N], double (&V)[N * N])
{
    bool any = jacobi_sym_pair<N, P, Q>(A, V);
    if constexpr (Q + 1 < N) any = jacobi_sym_sweep<N, P, Q + 1>(A, V) || any;
    else if constexpr (P + 2 < N) any = jacobi_sym_sweep<N, P + 1, P + 2>(A, V) || any;
    return any;
}

// A = V diag(A_kk) V^T on return (A symmetric on entry; its off-diagonal is rotated away).  Converges quadratically: 6 x 6
// takes 5-7 sweeps (8 with clustered eigenvalues, 4 for 3 x 3: tests/test_gpu_linalg_direct.py asserts <= 12), the cap is never
// the reason to stop.  Returns the number of sweeps that rotated.
template <int N>
__device__ __forceinline__ int jacobi_sym(double (&A)[N * N], double (&V)[N * N])
{
#pragma unroll
    for (int i = 0; i < N * N; ++i) V[i] = (i / N == i % N) ? 1.0 : 0.0;
    int sweep = 0;
    for (; sweep < 24; ++sweep)
        if (!jacobi_sym_sweep<N, 0, 1>(A, V)) break;
    return sweep; // (24: the cap stopped it)
}
