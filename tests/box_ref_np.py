"""The per-label box rule and the multi-box predicate restated in numpy (include/slamfusion.h,
sf_cloud_label_boxes / sf_cloud_remove_boxes): membership, lo / hi, pivot, moments, axes, center and extent, stage by stage, so that
the device can be compared with each of them.  Nothing here calls the library.  tests/test_box_rule.py pins this file to independent
code (math.fsum moments, numpy.linalg.eigh, brute-force corner containment); tests/test_gpu_boxes.py compares the device with it.
The sums are numpy's (pairwise): the rule leaves the summation order to the implementation, so moments are compared within the
rounding bound of a sum (moment_bounds), everything that is a minimum, a maximum or a count exactly."""
import math
from fractions import Fraction

import numpy as np

AABB, PCA, UPRIGHT = 0, 1, 2
MODES = {"aabb": AABB, "pca": PCA, "upright": UPRIGHT}
U = 2.0 ** -53   # unit roundoff of float64
BOX_DTYPE = np.dtype([("count", "<i8"), ("lo", "<f4", (3,)), ("hi", "<f4", (3,)), ("mean", "<f8", (3,)), ("cov", "<f8", (6,)), ("center", "<f8", (3,)),
                      ("R", "<f8", (3, 3)), ("extent", "<f8", (3,)), ("eigenvalues", "<f8", (3,)), ("valid", "<i4"), ("pad", "<i4")])
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))   # cov: xx xy xz yy yz zz


def membership(x, labels, n_labels):
    """-> (member bool [n], stats dict without n_valid / device_ms): a label outside 0 .. n_labels - 1 is ignored whatever the point
    holds, a non-finite point with a label in range is counted as such"""
    x = np.asarray(x, np.float32).reshape(-1, 3)
    labels = np.asarray(labels, np.int32).reshape(-1)
    ignored = (labels < 0) | (labels >= n_labels)
    nonfinite = ~ignored & ~np.isfinite(x).all(1)
    member = ~ignored & ~nonfinite
    return member, dict(n_points=len(x), n_labelled=int(member.sum()), n_ignored=int(ignored.sum()), n_nonfinite=int(nonfinite.sum()), n_labels=int(n_labels))


def unit_up(up):
    """up normalised in float64, left to right; None or all zeros: +z"""
    u = np.zeros(3) if up is None else np.asarray(up, np.float64).reshape(3)
    if not u.any():
        u = np.array([0.0, 0.0, 1.0])
    nn = u[0] * u[0]
    nn = nn + u[1] * u[1]
    nn = nn + u[2] * u[2]
    return u / np.sqrt(nn)


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def upright_frame(up):
    """-> (u, e1, e2): e1 = normalize(u x e_k), k the coordinate of smallest |u_k| (the first on a tie), e2 = u x e1"""
    u = unit_up(up)
    k = 0
    for j in (1, 2):
        if abs(u[j]) < abs(u[k]):
            k = j
    v = cross(u, np.eye(3)[k])
    vv = v[0] * v[0]
    vv = vv + v[1] * v[1]
    vv = vv + v[2] * v[2]
    e1 = v / np.sqrt(vv)
    return u, e1, cross(u, e1)


def signed(a):
    """the component of largest magnitude, the first such on a tie, made positive"""
    m = 0
    for j in (1, 2):
        if abs(a[j]) > abs(a[m]):
            m = j
    return -a if a[m] < 0 else a


def jacobi3(C):
    """cyclic Jacobi on a symmetric 3 x 3 -> (eigenvalues [3], eigenvectors as columns), unsorted; plain rotations, no library call"""
    A = np.array(C, np.float64)
    V = np.eye(3)
    for _ in range(30):
        off = abs(A[0, 1]) + abs(A[0, 2]) + abs(A[1, 2])
        if off <= 1e-300 or off <= 1e-17 * (abs(A[0, 0]) + abs(A[1, 1]) + abs(A[2, 2])):
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            if A[p, q] == 0.0:
                continue
            theta = 0.5 * math.atan2(2.0 * A[p, q], A[q, q] - A[p, p])
            c, s = math.cos(theta), math.sin(theta)
            G = np.eye(3)
            G[p, p], G[q, q], G[p, q], G[q, p] = c, c, s, -s
            A = G.T @ A @ G
            A = 0.5 * (A + A.T)
            V = V @ G
    return np.diag(A).copy(), V


def cov_matrix(c6):
    c = np.asarray(c6, np.float64)
    return np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])


def axes_of(cov6, mode, up=None):
    """-> (R [3, 3] with the axes as columns, eigenvalues [3], valid 1 | 2)"""
    C = cov_matrix(cov6)
    if not np.isfinite(C).all():
        return np.eye(3), np.zeros(3), 2
    if mode == AABB:
        return np.eye(3), np.array([C[0, 0], C[1, 1], C[2, 2]]), 1
    if mode == PCA:
        lam, V = jacobi3(C)
        order = sorted(range(3), key=lambda k: -lam[k])          # stable: ties keep index order
        a0, a1 = signed(V[:, order[0]]), signed(V[:, order[1]])
        return np.stack([a0, a1, cross(a0, a1)], axis=1), lam[order], 1
    u, e1, e2 = upright_frame(up)
    c11, c12, c22 = e1 @ C @ e1, e1 @ C @ e2, e2 @ C @ e2
    theta = math.atan2(2.0 * c12, c11 - c22) / 2
    a0 = signed(math.cos(theta) * e1 + math.sin(theta) * e2)
    a1 = cross(u, a0)
    return np.stack([a0, a1, u], axis=1), np.array([a0 @ C @ a0, a1 @ C @ a1, u @ C @ u]), 1


def pivot(lo, hi):
    return (np.asarray(lo, np.float32).astype(np.float64) + np.asarray(hi, np.float32).astype(np.float64)) / 2


def projections(pts, c0, R):
    """d . a_k per member and axis, float64, unfused, left to right -> [m, 3]"""
    d = np.asarray(pts, np.float32).astype(np.float64) - c0
    R = np.asarray(R, np.float64).reshape(3, 3)
    p = d[:, 0:1] * R[0] + d[:, 1:2] * R[1]
    return p + d[:, 2:3] * R[2]


def center_extent(pts, c0, R):
    """the box of the members along the axes R (columns) -> (center [3], extent [3]).  extent_k = pmax_k - pmin_k; center_i is the
    exact value of c0_i + sum_k R[i, k] (pmin_k + pmax_k) / 2 rounded ONCE (rational arithmetic here; the device's double-double
    evaluation returns the same but for rare double roundings): sf_cloud_crop_obb subtracts the rounded center, and every further
    rounding would move the faces against the members that define them"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    p = projections(pts, c0, R)
    pmin, pmax = p.min(0), p.max(0)
    if not (np.isfinite(p).all() and np.isfinite(R).all()):
        return np.full(3, np.nan), pmax - pmin
    h = [(Fraction(float(pmin[k])) + Fraction(float(pmax[k]))) / 2 for k in range(3)]
    center = np.array([float(Fraction(float(c0[i])) + sum(Fraction(float(R[i, k])) * h[k] for k in range(3))) for i in range(3)])
    return center, pmax - pmin


def terms(pts, c0):
    """the summands of the moments: d [m, 3] and d_i d_j [m, 6] (each product rounded once, as on the device)"""
    d = np.asarray(pts, np.float32).astype(np.float64) - c0
    return d, np.stack([d[:, i] * d[:, j] for i, j in PAIRS], axis=1)


def moments(S1, S2, count, c0):
    """sums -> (mean [3], cov [6]) by the rule's two formulas"""
    m = S1 / count
    return c0 + m, np.array([S2[k] / count - m[i] * m[j] for k, (i, j) in enumerate(PAIRS)])


def label_boxes(x, labels, n_labels, mode="pca", up=None):
    """-> (boxes [n_labels] of BOX_DTYPE, stats dict)"""
    mode = MODES.get(mode, mode)
    x = np.asarray(x, np.float32).reshape(-1, 3)
    labels = np.asarray(labels, np.int32).reshape(-1)
    member, st = membership(x, labels, n_labels)
    boxes = np.zeros(n_labels, BOX_DTYPE)
    order = np.flatnonzero(member)
    order = order[np.argsort(labels[order], kind="stable")]
    lab = labels[order]
    starts = np.searchsorted(lab, np.arange(n_labels + 1))
    with np.errstate(all="ignore"):
        for l in range(n_labels):
            ids = order[starts[l]:starts[l + 1]]
            if not len(ids):
                continue
            pts, b = x[ids], boxes[l]
            b["count"], b["lo"], b["hi"] = len(ids), pts.min(0), pts.max(0)
            c0 = pivot(b["lo"], b["hi"])
            d, dd = terms(pts, c0)
            b["mean"], b["cov"] = moments(d.sum(0), dd.sum(0), len(ids), c0)
            R, lam, valid = axes_of(b["cov"], mode, up)
            b["R"], b["eigenvalues"], b["valid"] = R, lam, valid
            b["center"], b["extent"] = center_extent(pts, c0, R)
    st["n_valid"] = int((boxes["count"] > 0).sum())
    return boxes, st


def moment_bounds(pts, c0):
    """What any summation order may differ by from the exact sums, propagated through the rule's two formulas.  For m summands t_i
    every order gives |S - sum t_i| <= (m - 1) u sum |t_i| (u = 2^-53).  math.fsum returns the exact sum rounded once, u |S| more.
    mean = c0 + S1 / m costs one division and one addition, each of relative error u on either side of the comparison; cov_ij =
    S2_ij / m - mu_i mu_j (mu = S1 / m) one division, one product and one subtraction likewise, and carries the error of mu.
    -> (S1, S2 by math.fsum, mean, cov from them, bound on |mean - mean'| [3], bound on |cov - cov'| [6])"""
    d, dd = terms(pts, c0)
    m = len(d)
    S1 = np.array([math.fsum(d[:, k]) for k in range(3)])
    S2 = np.array([math.fsum(dd[:, k]) for k in range(6)])
    e1 = (m - 1) * U * np.abs(d).sum(0) + U * np.abs(S1)
    e2 = (m - 1) * U * np.abs(dd).sum(0) + U * np.abs(S2)
    mean, cov = moments(S1, S2, m, c0)
    mu = S1 / m
    dmu = e1 / m + 2 * U * np.abs(mu)
    bmean = dmu + 2 * U * np.abs(mean)
    bcov = np.array([e2[k] / m + 2 * U * abs(S2[k] / m) + abs(mu[i]) * dmu[j] + abs(mu[j]) * dmu[i] + dmu[i] * dmu[j] + 2 * U * abs(mu[i] * mu[j]) +
                     2 * U * (abs(S2[k] / m) + abs(mu[i] * mu[j])) for k, (i, j) in enumerate(PAIRS)])
    return S1, S2, mean, cov, bmean, bcov


def inside_any(x, center, R, extent, margin=0.0):
    """sf_cloud_remove_boxes' predicate: inside at least one box whose extent is extent_k + 2 margin -- sf_cloud_crop_obb's float64
    expressions in their order; a non-finite point is never inside -> bool [n]"""
    x = np.asarray(x, np.float32).reshape(-1, 3)
    center, R, extent = np.asarray(center, np.float64).reshape(-1, 3), np.asarray(R, np.float64).reshape(-1, 9), np.asarray(extent, np.float64).reshape(-1, 3)
    x64 = x.astype(np.float64)
    inside = np.zeros(len(x), bool)
    with np.errstate(all="ignore"):
        for c, r, e in zip(center, R, extent):
            half = (e + 2 * margin) / 2
            d = x64 - c
            ok = np.ones(len(x), bool)
            for k in range(3):
                proj = d[:, 0] * r[k] + d[:, 1] * r[3 + k]
                proj = proj + d[:, 2] * r[6 + k]
                ok &= np.abs(proj) <= half[k]
            inside |= ok
    return inside & np.isfinite(x).all(1)


# ------------------------------------------------------------------ fixtures
BLOB_SIGMAS = (0.6, 0.25, 0.1)   # adjacent variance ratios 5.8 and 6.3


def random_rotations(rng, count):
    q, _ = np.linalg.qr(rng.normal(size=(count, 3, 3)))
    q[:, :, 2] *= np.sign(np.linalg.det(q))[:, None]
    return q


def aniso_blob_cloud(n=20_000, blobs=25, scatter=0.1, seed=5):
    """`blobs` anisotropic Gaussian blobs (sigmas BLOB_SIGMAS along the axes of a random rotation each) in a 12 m cube plus a share
    `scatter` of uniform points, in shuffled order -> (x float32 [n, 3], labels int32 [n]: the blob, -1 for the scatter)"""
    rng = np.random.default_rng(seed)
    ns = int(round(n * scatter))
    cen, rot = rng.uniform(-5, 5, (blobs, 3)), random_rotations(rng, blobs)
    which = np.concatenate([rng.integers(0, blobs, n - ns), np.full(ns, -1)])[rng.permutation(n)]
    w = np.maximum(which, 0)
    blob = cen[w] + np.einsum("nij,nj->ni", rot[w], rng.normal(size=(n, 3)) * np.array(BLOB_SIGMAS))
    x = np.where((which >= 0)[:, None], blob, rng.uniform(-6, 6, (n, 3))).astype(np.float32)
    return x, which.astype(np.int32)


def grid_labels(x, cell=3.0):
    """a labelling of any cloud for the tests: the 3 m cell a finite point falls in, numbered in order of first appearance, -1 for a
    point that is not finite -> (labels int32 [n], n_labels)"""
    x = np.asarray(x, np.float32).reshape(-1, 3)
    fin = np.isfinite(x).all(1)
    ijk = np.floor(np.where(fin[:, None], x, 0).astype(np.float64) / cell).astype(np.int64)
    _, first, inv = np.unique(ijk[fin], axis=0, return_index=True, return_inverse=True)
    rank = np.argsort(np.argsort(first))
    labels = np.full(len(x), -1, np.int32)
    labels[fin] = rank[inv.reshape(-1)]
    return labels, int(len(first))


def tilted(x, degrees=3.0):
    """x rotated about the x axis by `degrees` (float64, rounded once) -> (x' float32, the rotated +z)"""
    a = math.radians(degrees)
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    return (np.asarray(x, np.float64) @ Rx.T).astype(np.float32), Rx[:, 2].copy()


def random_boxes(rng, count, span=6.0):
    """`count` boxes with random centres in +-span, random rotations and extents 0.3 .. 3 m -> (center, R [count, 3, 3], extent)"""
    return rng.uniform(-span, span, (count, 3)), random_rotations(rng, count), rng.uniform(0.3, 3.0, (count, 3))
