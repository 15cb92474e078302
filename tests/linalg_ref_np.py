"""Plain numpy references and seeded case sets for the float64 numerical core (tests/test_gpu_linalg_direct.py runs the device
routines through the sf_test_* hooks; tests/test_linalg_ref.py checks this file against itself; tools/linalg_errors.py prints
the worst errors).  Nothing here shares code with the library or with oracle/: numpy.linalg.svd / eigh in float64, a centred
Kabsch and a pivoted 6x6 elimination in np.longdouble, math.fsum for sums, Rz Ry Rx written from the definition of Open3D's
TransformVector6dToMatrix4d, and the four robust weights written from the SF_ROBUST_* text of include/slamfusion.h."""
import math

import numpy as np

EPS = 2.0 ** -52
LD = np.longdouble
DBL_MIN = 2.2250738585072014e-308


# ------------------------------------------------------------------ small tools
def ulps(got, want_ld):
    """|got - want| in units of the float64 spacing at want (want: np.longdouble)"""
    want_ld = np.asarray(want_ld, dtype=LD)
    return np.abs((np.asarray(got, dtype=LD) - want_ld) / np.spacing(np.abs(want_ld).astype(np.float64)).astype(LD)).astype(np.float64)


def random_rotations(rng, n):
    """n proper rotations (QR of Gaussian matrices, sign-fixed)"""
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 2] *= np.linalg.det(q)[:, None]
    return q


def random_orthogonal(rng, n, d):
    q, r = np.linalg.qr(rng.normal(size=(n, d, d)))
    return q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]


def fsum_columns(a):
    """exactly rounded column sums of a 2-D array"""
    a = np.asarray(a, dtype=np.float64)
    return np.array([math.fsum(a[:, c]) for c in range(a.shape[1])])


# ------------------------------------------------------------------ rsqrt / recip
def rsqrt_cases(rng):
    """the domain of rsqrt_nr / recip_nr: normal, finite, positive doubles in [DBL_MIN, 1e300]"""
    k = np.arange(-1020, 997, 7)
    p2 = np.ldexp(1.0, k)
    return np.concatenate([
        10.0 ** rng.uniform(-300, 300, 4000),
        p2, p2 * (1 + EPS), p2 * (1 - EPS / 2),
        DBL_MIN * (1 + EPS * np.arange(0, 9)), DBL_MIN * np.array([1.5, 2.0, 3.0, 4.0]),
        np.array([1.0, 2.0, 3.0, 4.0, 0.25, 1e300])])


def rsqrt_ref(x):
    x = np.asarray(x, dtype=LD)
    return 1 / np.sqrt(x), 1 / x


# ------------------------------------------------------------------ svd3
def svd3_cases(rng):
    """name -> (A[n, 3, 3], rank[n]); the rank is the exact (or, for 'rank2_noise', the numerical) rank"""
    out = {}
    n = 1500
    scale = 10.0 ** rng.uniform(-6, 6, n)
    out["random"] = (rng.normal(size=(n, 3, 3)) * scale[:, None, None], np.full(n, 3))
    d = rng.normal(size=(200, 3)) * 10.0 ** rng.uniform(-3, 3, (200, 1))
    out["diagonal"] = (np.einsum("ni,ij->nij", d, np.eye(3)), np.full(200, 3))
    out["identity"] = (np.stack([np.eye(3), -np.eye(3), 2 * np.eye(3)]), np.full(3, 3))
    rep = []
    for s in ((2.0, 2.0, 1.0), (1.0, 1.0, 1.0), (3.0, 1.0, 1.0)):
        q1, q2 = random_rotations(rng, 100), random_rotations(rng, 100)
        rep.append(q1 @ np.diag(s) @ np.swapaxes(q2, 1, 2))
    out["repeated"] = (np.concatenate(rep), np.full(300, 3))
    out["rank0"] = (np.zeros((2, 3, 3)), np.zeros(2, int))
    u = rng.integers(-4, 5, (400, 3)).astype(float)
    v = rng.integers(-4, 5, (400, 3)).astype(float)
    keep = (np.abs(u).sum(1) > 0) & (np.abs(v).sum(1) > 0)
    out["rank1"] = (np.einsum("ni,nj->nij", u[keep], v[keep]), np.ones(keep.sum(), int))
    u2 = rng.integers(-4, 5, (400, 3)).astype(float)
    v2 = rng.integers(-4, 5, (400, 3)).astype(float)
    keep = (np.abs(np.cross(u, u2)).sum(1) > 0) & (np.abs(np.cross(v, v2)).sum(1) > 0)
    r2 = np.einsum("ni,nj->nij", u[keep], v[keep]) + np.einsum("ni,nj->nij", u2[keep], v2[keep])
    out["rank2"] = (r2, np.full(len(r2), 2))
    out["rank2_noise"] = (r2 + 1e-17 * rng.normal(size=r2.shape), np.full(len(r2), 2))
    neg = rng.normal(size=(300, 3, 3))
    neg[:, :, 0] *= -np.sign(np.linalg.det(neg))[:, None]
    out["det_negative"] = (neg, np.full(300, 3))
    perms = []
    for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        for sg in ((1, 1, 1), (1, -1, 1), (-1, -1, -1)):
            perms.append(np.eye(3)[list(p)] * np.array(sg, float))
    out["permutation"] = (np.stack(perms), np.full(len(perms), 3))
    return out


# ------------------------------------------------------------------ Kabsch
def kabsch_record(src, tgt):
    """the 32-double record k_nn_red sums for point-to-point pairs: n, sum s, sum t, sum s t^T (row-major); float64, every
    product rounded once"""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    rec = np.zeros(32)
    rec[0] = len(src)
    rec[1:4] = src.sum(0)
    rec[4:7] = tgt.sum(0)
    rec[7:16] = (src[:, :, None] * tgt[:, None, :]).sum(0).ravel()
    return rec


def rodrigues_ld(w):
    w = np.asarray(w, dtype=LD)
    th = np.sqrt((w * w).sum())
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=LD)
    if th == 0:
        return np.eye(3, dtype=LD)
    return np.eye(3, dtype=LD) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / (th * th)) * (K @ K)


def polish_rotation_ld(R0, H):
    """R0 (float64, from numpy's SVD: good to a few eps) -> the stationary rotation of tr(R H) next to it, in np.longdouble.
    Newton-Schulz makes R0 orthonormal to long-double precision; then R H must be symmetric: for a small rotation vector w,
    skew((I + [w]x) B) = 0 with B = R H ~ S symmetric gives (tr(S) I - S) w = -vee(B - B^T)."""
    R = np.asarray(R0, dtype=LD)
    I = np.eye(3, dtype=LD)
    for _ in range(3):
        R = R @ (3 * I - R.T @ R) / 2
    for _ in range(3):
        B = R @ H
        S = (B + B.T) / 2
        D = B - B.T
        M = np.trace(S) * I - S
        if abs(float(np.linalg.det(M.astype(np.float64)))) < 1e-12 * max(float(np.abs(M).max()), 1e-300) ** 3:
            break                                               # R is not unique here: nothing to polish towards
        w = -solve6_ld(M, np.array([D[2, 1], D[0, 2], D[1, 0]], dtype=LD))
        R = rodrigues_ld(w) @ R
    return R


def kabsch_ld(src, tgt):
    """centred Kabsch in np.longdouble: centroids, H and the translation directly; the rotation from numpy's float64 SVD of H
    (numpy has no wider one) with the det < 0 flip, then polished in long double (polish_rotation_ld).  Returns (T as float64
    4x4, unique): R is unique when the two largest singular values of H are non-zero (the flip decides the third axis)."""
    s, t = np.asarray(src, dtype=LD), np.asarray(tgt, dtype=LD)
    cs, ct = s.sum(0) / len(s), t.sum(0) / len(t)
    H = (s - cs).T @ (t - ct)
    U, S, Vt = np.linalg.svd(H.astype(np.float64))
    V = Vt.T.copy()
    R = V @ U.T
    if np.linalg.det(R) < 0:
        V[:, 2] *= -1
        R = V @ U.T
    unique = bool(S[1] > 1e-9 * max(S[0], 1e-300))
    R = polish_rotation_ld(R, H) if unique else np.asarray(R, dtype=LD)
    T = np.eye(4)
    T[:3, :3] = R.astype(np.float64)
    T[:3, 3] = (ct - R @ cs).astype(np.float64)
    return T, unique


def residual_ld(T, src, tgt):
    """root of the summed squared distances of T src to tgt, in np.longdouble"""
    s, t = np.asarray(src, dtype=LD), np.asarray(tgt, dtype=LD)
    d = s @ T[:3, :3].astype(LD).T + T[:3, 3].astype(LD) - t
    return float(np.sqrt((d * d).sum()))


RIGID_COND = 8.0


def scatter_cond(src):
    """S0 / (S1 + S2) of the centred scatter: by how much the Kabsch rotation amplifies a relative perturbation of H (a needle
    of three points has S1 << S0 and a rotation about the needle that the data barely holds)"""
    d = np.asarray(src, float) - np.mean(src, axis=0)
    sv = np.linalg.svd(d.T @ d, compute_uv=False)
    return sv[0] / max(sv[1] + sv[2], 1e-300)


def rigid_sets(rng, sizes=(3, 4, 5, 7, 10, 33, 100, 500, 2000), sigma=5.0, offset=0.0, reps=4):
    """exact rigid motions of clouds with spread sigma: list of (src, tgt, R, t); src is centred `offset` metres from the origin
    (in a random direction) and well spread (scatter_cond <= RIGID_COND), the motion is a rotation of up to ~0.2 rad about the cloud's centre plus a shift of up to 1 m, as an
    ICP step sees it"""
    sets = []
    for n in sizes:
        for _ in range(reps):
            c = rng.normal(size=3)
            c *= offset / np.linalg.norm(c)
            while True:                                         # the rotation's condition number S0 / (S1 + S2) stays below RIGID_COND
                src = rng.normal(size=(n, 3)) * sigma
                if scatter_cond(src) <= RIGID_COND:
                    break
            src = src + c
            w = rng.normal(size=3) * 0.1
            R = rodrigues(w)
            t = c - R @ c + rng.uniform(-1, 1, 3)
            tgt = src @ R.T + t
            sets.append((src, tgt, R, t))
    return sets


def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def rotation_angle(Ra, Rb):
    """angle of Ra Rb^T in radians (from the skew part: accurate near zero)"""
    D = Ra @ Rb.T
    return float(np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]]) / 2)


def offset_law_bound(c, sigma=5.0):
    """the Kabsch offset law: error of the uncentred H = sum s t^T - n cs ct^T at distance c from the origin"""
    return 16 * EPS * c ** 3 / sigma ** 2 + 64 * EPS * (1 + c)


# ------------------------------------------------------------------ 6x6 solve
def solve6_ld(A, b):
    """Gaussian elimination with partial pivoting in np.longdouble"""
    n = len(b)
    M = np.concatenate([np.asarray(A, dtype=LD), np.asarray(b, dtype=LD)[:, None]], axis=1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
        for i in range(k + 1, n):
            M[i, k:] -= (M[i, k] / M[k, k]) * M[k, k:]
    x = np.zeros(n, dtype=LD)
    for i in range(n - 1, -1, -1):
        x[i] = (M[i, n] - M[i, i + 1:n] @ x[i + 1:]) / M[i, i]
    return x


def spd_with_cond(rng, cond, n=6):
    """A = Q diag(lambda) Q^T, lambda log-spaced from 1 down to 1 / cond"""
    q = random_orthogonal(rng, 1, n)[0]
    lam = np.logspace(0, -math.log10(cond), n) if cond > 1 else np.ones(n)
    A = (q * lam) @ q.T
    return (A + A.T) / 2


def plane_jacobian(points, normals):
    """point-to-plane Jacobian rows [p x n, n] (the J of sf_icp.hip's pair terms)"""
    return np.concatenate([np.cross(points, normals), normals], axis=1)


def three_walls(rng, n=300, offset=0.0, tilt=0.0):
    """a room corner: points on three orthogonal walls with their normals (tilted by `tilt` rad of noise), moved `offset` along x"""
    pts, nrm = [], []
    for axis in range(3):
        p = rng.uniform(-5, 5, (n // 3, 3))
        p[:, axis] = 5.0
        e = np.zeros(3)
        e[axis] = 1.0
        m = e + tilt * rng.normal(size=(n // 3, 3))
        pts.append(p)
        nrm.append(m / np.linalg.norm(m, axis=1, keepdims=True))
    pts = np.concatenate(pts)
    pts[:, 0] += offset
    return pts, np.concatenate(nrm)


def normal_equations(rng, pts, nrm):
    J = plane_jacobian(pts, nrm)
    r = rng.normal(size=len(J)) * 0.05
    return J.T @ J, J.T @ r


def ldlt6_cond_cases(rng):
    """list of (A, b) with their class name: Q diag Q^T at five condition numbers and the three-wall scenes"""
    cases = []
    for cond in (1.0, 1e3, 1e6, 1e9, 1e12):
        for _ in range(40):
            cases.append(("cond%.0e" % cond, spd_with_cond(rng, cond), rng.normal(size=6)))
    for off in (0.0, 1000.0):
        for _ in range(40):
            A, b = normal_equations(rng, *three_walls(rng, offset=off, tilt=0.02))
            cases.append(("walls%g" % off, A, b))
    return cases


def ldlt6_refused_cases():
    """(name, A) that ldlt6 must answer with rc = -1: exact zero pivots and non-finite entries"""
    rng = np.random.default_rng(5)
    cases = []
    pts, _ = three_walls(rng)
    J = plane_jacobian(pts, np.tile([0.0, 0.0, 1.0], (len(pts), 1)))
    cases.append(("normals_all_z", J.T @ J))
    v = np.array([2.0, 3.0, -5.0, 7.0, 1.0, 6.0])          # v0 a power of two: every L entry and every later pivot is exact
    cases.append(("rank1", np.outer(v, v)))
    cases.append(("zero", np.zeros((6, 6))))
    good = spd_with_cond(rng, 10.0)
    for bad in (np.nan, np.inf, -np.inf):
        for i in range(6):
            for j in range(i + 1):
                A = good.copy()
                A[i, j] = A[j, i] = bad
                cases.append(("%s_%d%d" % (bad, i, j), A))
    return cases


def ldlt6_deficient_cases(rng, n=20000):
    """rank-deficient and badly scaled J^T J, b = J^T r: ranks 1..5 (normals and points confined to subspaces), scales 1e-150 .. 1e150"""
    A = np.zeros((n, 6, 6))
    b = np.zeros((n, 6))
    rank = rng.integers(1, 6, n)
    for i in range(n):
        B = rng.normal(size=(6, rank[i]))                       # J = G B^T: the rows of J live in a rank-dimensional subspace
        G = rng.normal(size=(12, rank[i]))
        J = (G @ B.T) * 10.0 ** rng.uniform(-150, 150)
        with np.errstate(over="ignore", invalid="ignore"):
            A[i] = J.T @ J
            b[i] = J.T @ rng.normal(size=12)
    return A, b, rank


def near_planar_case():
    """one wall whose normals are perturbed by 1e-9: J^T J of condition ~1e22"""
    rng = np.random.default_rng(11)
    p = rng.uniform(-5, 5, (300, 3))
    p[:, 2] = 0.0
    m = np.array([0.0, 0.0, 1.0]) + 1e-9 * rng.normal(size=(300, 3))
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    return normal_equations(rng, p, m)


# ------------------------------------------------------------------ vec6 -> 4x4 (Open3D TransformVector6dToMatrix4d)
def vec6_ref(v):
    """T = [Rz(v2) Ry(v1) Rx(v0) | v3:6] in np.longdouble: Open3D composes AngleAxis(v2, Z) * AngleAxis(v1, Y) * AngleAxis(v0, X)"""
    v = np.asarray(v, dtype=LD)
    ca, sa, cb, sb, cg, sg = np.cos(v[0]), np.sin(v[0]), np.cos(v[1]), np.sin(v[1]), np.cos(v[2]), np.sin(v[2])
    one, zero = LD(1), LD(0)
    Rx = np.array([[one, zero, zero], [zero, ca, -sa], [zero, sa, ca]], dtype=LD)
    Ry = np.array([[cb, zero, sb], [zero, one, zero], [-sb, zero, cb]], dtype=LD)
    Rz = np.array([[cg, -sg, zero], [sg, cg, zero], [zero, zero, one]], dtype=LD)
    T = np.eye(4, dtype=LD)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = v[3:6]
    return T


def vec6_cases(rng):
    special = [0.0, math.pi / 2, -math.pi / 2, 1e-9, -1e-9, math.pi, -math.pi, 1e3, -1e3]
    grid = np.array([[a, b, c] for a in special for b in special for c in special])
    rnd = rng.uniform(-math.pi, math.pi, (2000, 3))
    ang = np.concatenate([grid, rnd])
    return np.concatenate([ang, rng.normal(size=(len(ang), 3)) * 10.0 ** rng.uniform(-3, 4, (len(ang), 1))], axis=1)


# ------------------------------------------------------------------ robust weights (include/slamfusion.h, SF_ROBUST_*)
ROBUST_KINDS = {"none": 0, "huber": 1, "cauchy": 2, "tukey": 3, "gm": 4}


def robust_ref(kind, k, r):
    k, r = LD(k), LD(r)
    if kind == 0:
        return LD(1)
    if kind == 1:
        return LD(1) if abs(r) <= k else k / abs(r)
    if kind == 2:
        return 1 / (1 + (r / k) ** 2)
    if kind == 3:
        return (1 - (r / k) ** 2) ** 2 if abs(r) <= k else LD(0)
    if kind == 4:
        return (k * k / (k * k + r * r)) ** 2
    raise ValueError(kind)


def robust_cases(rng):
    """rows (kind, k, r): r = 0, +-k exactly, the doubles next to +-k, and |r| from 1e-9 k to 1e6 k of both signs"""
    rows = []
    for kind in ROBUST_KINDS.values():
        for k in (0.05, 0.1, 1.0, 0.3, 7.0):
            rs = [0.0, k, -k, np.nextafter(k, 0), np.nextafter(k, 10), -np.nextafter(k, 0), -np.nextafter(k, 10), 1e6 * k, -1e6 * k]
            rs += list(k * 10.0 ** rng.uniform(-9, 6, 150) * rng.choice([-1.0, 1.0], 150))
            rs += list(k * rng.uniform(0.5, 1.5, 50))
            rows += [(kind, k, r) for r in rs]
    return np.array(rows)


# ------------------------------------------------------------------ symmetric eigen-solves
def sym_from_eig(rng, lam):
    lam = np.asarray(lam, float)
    q = random_orthogonal(rng, 1, len(lam))[0]
    A = (q * lam) @ q.T
    return (A + A.T) / 2


def jacobi_cases(rng, n):
    """name -> A[m, n, n] symmetric"""
    out = {}
    g = rng.normal(size=(400, n, n)) * 10.0 ** rng.uniform(-3, 3, (400, 1, 1))
    out["random"] = (g + np.swapaxes(g, 1, 2)) / 2
    out["psd_wide"] = np.stack([sym_from_eig(rng, 10.0 ** np.sort(rng.uniform(-12, 4, n))) for _ in range(300)])
    clustered = []
    for _ in range(100):
        clustered.append(sym_from_eig(rng, 1 + 1e-9 * rng.normal(size=n)))
        lam = np.ones(n)
        lam[: n // 2] = 3.0
        clustered.append(sym_from_eig(rng, lam))
        clustered.append(sym_from_eig(rng, np.full(n, 2.0)))
    out["clustered"] = np.stack(clustered)
    z = rng.normal(size=(200, n, n))
    z = (z + np.swapaxes(z, 1, 2)) / 2
    z[:, np.arange(n), np.arange(n)] = 0.0
    out["zero_diagonal"] = z
    out["diagonal"] = np.stack([np.diag(rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3)) for _ in range(50)] + [np.zeros((n, n)), np.eye(n)])
    out["indefinite"] = np.stack([sym_from_eig(rng, (0.1 + np.abs(rng.normal(size=n))) * np.array([1, -1] * (n // 2) + [1] * (n % 2))) for _ in range(200)])
    return out


# ------------------------------------------------------------------ map normals
def neighbourhood_cov(points):
    """the 3x3 centred sums normals_point forms (two passes in float64: mean, then sum of (q - mean)(q - mean)^T; not divided by
    the count), from float32 coordinates"""
    q = np.asarray(points, np.float32).astype(np.float64)
    d = q - q.sum(0) / len(q)
    C = d.T @ d
    return (C + C.T) / 2


def eigvec_cases(rng):
    """name -> C[m, 3, 3]; neighbourhoods of 12-30 points at scales 1e-4 .. 1e2 m (C from 1e-8 to 1e4 m^2)"""
    out = {}

    def blob(n, sx, sy, sz, R, scale):
        return (rng.normal(size=(n, 3)) * [sx, sy, sz]) @ R.T * scale + rng.uniform(-50, 50, 3) * min(scale, 1.0)

    rots = random_rotations(rng, 200)
    scales = 10.0 ** rng.uniform(-4, 2, 200)
    out["plane"] = np.stack([neighbourhood_cov(blob(rng.integers(12, 31), 1, 0.7, 0.01, rots[i], scales[i])) for i in range(200)])
    ax = []
    for i in range(60):
        p = rng.normal(size=(20, 3)).astype(np.float32).astype(np.float64)
        C = np.zeros((3, 3))
        C[np.arange(3), np.arange(3)] = (p * p).sum(0) * np.roll([1.0, 0.5, 1e-4], i % 3) * scales[i] ** 2
        ax.append(C)
    out["axis_aligned"] = np.stack(ax)
    out["line"] = np.stack([neighbourhood_cov(blob(20, 1, 0.003, 0.002, rots[i], scales[i])) for i in range(100)])
    out["blob"] = np.stack([neighbourhood_cov(blob(25, 1, 1, 1, rots[i], scales[i])) for i in range(100)])
    outl = []
    for i in range(100):
        p = blob(25, 1, 0.8, 0.005, rots[i], 1.0)
        p[0] += rots[i][:, 2] * 0.5
        outl.append(neighbourhood_cov(p))
    out["plane_outlier"] = np.stack(outl)
    out["zero"] = np.zeros((1, 3, 3))
    return out


def sign_rule(v):
    """the library's normal orientation: z > 0, then y, then x"""
    x, y, z = v
    return not (z < 0 or (z == 0 and (y < 0 or (y == 0 and x < 0))))


# ------------------------------------------------------------------ reductions
def reduce_inputs(rng, shape, kind):
    """integer: integer-valued doubles below 2^30 (every partial sum exact); random: 12 decades, mixed signs"""
    if kind == "integer":
        return rng.integers(-(1 << 30) + 1, 1 << 30, shape).astype(np.float64)
    return rng.normal(size=shape) * 10.0 ** rng.uniform(-6, 6, shape)
