"""numpy restatement of the FPFH and descriptor-matching rules (include/slamfusion.h), brute force.

Neighbours: indexed (finite) points i != j with the float32 `((dx*dx)+dy*dy)+dz*dz` < float32(radius^2).
Normals: float64 of the stored float32 normal; orient 0 as stored, 1 negated when n . toward < 0, 2 negated when n . (toward - x) < 0;
all zeros or not finite: no normal, the point contributes to nothing and gets no descriptor.
Pair (i, j), float64, every product and sum written out left to right over x, y, z (no dot(), which may fuse):
  d = x_j - x_i, L = sqrt(d.d), L == 0 skips; a_i = (n_i.d) / L, a_j = (n_j.d) / L; |a_i| < |a_j|: source j, target i, d = -d,
  phi = -a_j, else source i, target j, phi = a_i; v = d x n_src, |v| == 0 skips, v = v / |v|, w = n_src x v; alpha = v . n_tgt;
  theta = atan2(w . n_tgt, n_src . n_tgt).
Bins: floor(11 (theta + pi) / (2 pi)), floor(11 (alpha + 1) / 2), floor(11 (phi + 1) / 2), clamped to 0 .. 10; row = theta | alpha | phi.
SPFH_i[b] = cnt_i[b] * (100.0 / P_i) over the P_i pairs that were not skipped; P_i == 0: none.
FPFH: W[b] = sum over the neighbours j with an SPFH and d2_ij > 0 of SPFH_j[b] / float64(d2_ij) (the float32 d2 of the neighbour rule);
  per group of 11 S = sum W[b]; F_i[b] = (S > 0 ? W[b] * (100.0 / S) : 0) + SPFH_i[b], rounded to float32 once.  The order of the sum
  W is the index's on the device and numpy's here: the two differ by float64 roundings.
Matching: D = float32, ascending k: acc = 0; t = a[k] - b[k]; t = t * t; acc = acc + t.  Best = smallest (D, index) over the valid rows
  of dst, runner-up = the smallest D over the others."""
import numpy as np

DIM, BINS = 33, 11
ORIENT = {"none": 0, "direction": 1, "viewpoint": 2}


def d2_rows(Q, P):
    """[len(Q), len(P)] float32"""
    dx, dy, dz = (Q[:, None, d] - P[None, :, d] for d in range(3))
    d = ((dx * dx) + dy * dy) + dz * dz
    assert d.dtype == np.float32
    return d


def neighbour_pairs(P, radius):
    """P float32 [m, 3], all finite -> (i, j, d2 float32) of every ordered pair i != j with d2 < float32(radius^2)"""
    r2 = np.float32(float(radius) * float(radius))
    I, J, D = [], [], []
    for s in range(0, len(P), 512):
        d2 = d2_rows(P[s:s + 512], P)
        i, j = np.nonzero(d2 < r2)
        keep = (i + s) != j
        I.append(i[keep] + s)
        J.append(j[keep])
        D.append(d2[i[keep], j[keep]])
    if not I:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    return np.concatenate(I), np.concatenate(J), np.concatenate(D)


def oriented_normals(points, normals, orient=0, toward=(0.0, 0.0, 1.0)):
    """-> (float64 [n, 3], has_normal bool [n]); points only matter for orient 2"""
    orient = ORIENT.get(orient, orient)
    nf = np.asarray(normals, np.float32).reshape(-1, 3)
    has = np.isfinite(nf).all(1) & ~(nf == 0).all(1)
    n = nf.astype(np.float64)
    t = np.asarray(toward, np.float64).reshape(3)
    if orient != 0:
        a = np.broadcast_to(t, n.shape)
        if orient == 2:
            a = t[None, :] - np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            s = (n[:, 0] * a[:, 0] + n[:, 1] * a[:, 1]) + n[:, 2] * a[:, 2]
            n = np.where((s < 0)[:, None], -n, n)
    return n, has


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _edge_margin(x):
    """distance of the binned values x (bin = floor(x)) from the nearest INNER edge 1 .. 10"""
    if len(x) == 0:
        return np.inf
    return float(np.abs(x[:, None] - np.arange(1, BINS)[None, :]).min())


def pair_features(xi, ni, xj, nj):
    """float64 [m, 3] each -> (used bool [m], bins int [m, 3] (theta, alpha, phi), margin of the used pairs)"""
    d = xj - xi
    L = np.sqrt(_dot(d, d))
    used = L != 0
    with np.errstate(invalid="ignore", divide="ignore"):
        ai, aj = _dot(ni, d) / L, _dot(nj, d) / L
        swap = np.abs(ai) < np.abs(aj)
        src, tgt = np.where(swap[:, None], nj, ni), np.where(swap[:, None], ni, nj)
        d = np.where(swap[:, None], -d, d)
        phi = np.where(swap, -aj, ai)
        v = _cross(d, src)
        vn = np.sqrt(_dot(v, v))
        used &= vn != 0
        v = v / vn[:, None]
        w = _cross(src, v)
        alpha = _dot(v, tgt)
        theta = np.arctan2(_dot(w, tgt), _dot(src, tgt))
        x = np.stack([11.0 * (theta + np.pi) / (2.0 * np.pi), 11.0 * (alpha + 1.0) / 2.0, 11.0 * (phi + 1.0) / 2.0], 1)
    bins = np.clip(np.floor(np.where(used[:, None], x, 0.0)), 0, BINS - 1).astype(np.int64)
    return used, bins, _edge_margin(x[used].reshape(-1))


def spfh(points, normals, radius, orient=0, toward=(0.0, 0.0, 1.0)):
    """-> dict(counts uint32 [n, 33], n_pairs int32 [n], margin, and for fpfh(): ok, i, j, d2 in positions of points[ok])"""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    n = len(pts)
    ok = np.isfinite(pts).all(1)
    P = np.ascontiguousarray(pts[ok])
    nrm, has = oriented_normals(pts, normals, orient, toward)
    nrm, has = nrm[ok], has[ok]
    i, j, d2 = neighbour_pairs(P, radius)
    both = has[i] & has[j]
    P64 = P.astype(np.float64)
    used, bins, margin = pair_features(P64[i[both]], nrm[i[both]], P64[j[both]], nrm[j[both]])
    cnt = np.zeros((len(P), DIM), np.int64)
    iu, bu = i[both][used], bins[used]
    for g in range(3):
        np.add.at(cnt, (iu, g * BINS + bu[:, g]), 1)
    pairs = np.bincount(iu, minlength=len(P)).astype(np.int32)
    counts, n_pairs = np.zeros((n, DIM), np.uint32), np.zeros(n, np.int32)
    counts[ok], n_pairs[ok] = cnt.astype(np.uint32), pairs
    return dict(counts=counts, n_pairs=n_pairs, margin=margin, ok=ok, i=i, j=j, d2=d2)


def fpfh(points, normals, radius, orient=0, toward=(0.0, 0.0, 1.0)):
    """-> dict(rows float32 [n, 33], valid bool [n], counts, n_pairs, margin, stats)"""
    s = spfh(points, normals, radius, orient, toward)
    ok, i, j, d2 = s["ok"], s["i"], s["j"], s["d2"]
    n = len(ok)
    cnt, P = s["counts"][ok].astype(np.float64), s["n_pairs"][ok].astype(np.float64)
    has = P > 0
    with np.errstate(divide="ignore"):
        S = cnt * np.where(has, 100.0 / P, 0.0)[:, None]
    take = has[j] & (d2 > 0)
    W = np.zeros_like(S)
    np.add.at(W, i[take], S[j[take]] / d2[take].astype(np.float64)[:, None])
    F = np.zeros_like(S)
    for g in range(3):
        Wg = W[:, g * BINS:(g + 1) * BINS]
        Sg = np.zeros(len(W))
        for b in range(BINS):
            Sg = Sg + Wg[:, b]
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(Sg > 0, 100.0 / Sg, 0.0)
        F[:, g * BINS:(g + 1) * BINS] = np.where((Sg > 0)[:, None], Wg * f[:, None], 0.0) + S[:, g * BINS:(g + 1) * BINS]
    F[~has] = 0.0
    rows, valid = np.zeros((n, DIM), np.float32), np.zeros(n, bool)
    rows[ok], valid[ok] = F.astype(np.float32), has
    F64 = np.zeros((n, DIM))
    F64[ok] = F
    stats = dict(n_points=n, n_valid=int(ok.sum()), n_featured=int(valid.sum()), n_pairs=int(s["n_pairs"].sum()),
                 max_pairs=int(s["n_pairs"].max()) if n else 0)
    return dict(rows=rows, rows64=F64, valid=valid, counts=s["counts"], n_pairs=s["n_pairs"], margin=s["margin"], stats=stats)


def normalise_valid(rows, valid=None):
    rows = np.asarray(rows, np.float32).reshape(-1, DIM)
    v = np.ones(len(rows), bool) if valid is None else np.asarray(valid).reshape(-1) != 0
    return rows, v & np.isfinite(rows).all(1)


def distances(A, B):
    """float32 [len(A), len(B)]: the loop over k on float32 arrays"""
    acc = np.zeros((len(A), len(B)), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(DIM):
            t = A[:, None, k] - B[None, :, k]
            t = t * t
            acc = acc + t
    assert acc.dtype == np.float32
    return acc


def best_two(A, va, B, vb):
    """-> idx int32 [len(A)], dist2, second2 float32"""
    na = len(A)
    idx, d2, s2 = np.full(na, -1, np.int32), np.full(na, np.inf, np.float32), np.full(na, np.inf, np.float32)
    cand = np.nonzero(vb)[0]
    if len(cand) == 0 or na == 0:
        return idx, d2, s2
    Bc = np.ascontiguousarray(B[cand])
    for s in range(0, na, 256):
        D = distances(np.where(va[s:s + 256, None], A[s:s + 256], np.float32(0)), Bc)
        first = np.argmin(D, axis=1)                         # the first of equal minima: the smallest index
        rows = np.arange(len(D))
        best = D[rows, first]
        D2 = D.copy()
        D2[rows, first] = np.inf
        second = D2.min(axis=1) if len(cand) > 1 else np.full(len(D), np.inf, np.float32)
        q = va[s:s + 256]
        idx[s:s + 256] = np.where(q, cand[first], -1)
        d2[s:s + 256] = np.where(q, best, np.float32(np.inf))
        s2[s:s + 256] = np.where(q, second, np.float32(np.inf))
    return idx, d2, s2


def match(src_rows, src_valid, dst_rows, dst_valid, ratio=0.0, mutual=False, cap_pairs=None):
    """-> dict(idx, dist2, second2, pairs int32 [m, 2], stats)"""
    A, va = normalise_valid(src_rows, src_valid)
    B, vb = normalise_valid(dst_rows, dst_valid)
    idx, d2, s2 = best_two(A, va, B, vb)
    acc = idx >= 0
    if 0.0 < ratio < 1.0:
        rr = np.float32(float(ratio) * float(ratio))
        with np.errstate(invalid="ignore"):
            acc &= d2 < rr * s2
    if mutual and len(B):
        back, _, _ = best_two(B, vb, A, va)
        acc &= back[np.maximum(idx, 0)] == np.arange(len(A))
    i = np.nonzero(acc)[0]
    pairs = np.stack([i, idx[i]], 1).astype(np.int32).reshape(-1, 2)
    n_matched = len(pairs)
    if cap_pairs is not None:
        pairs = pairs[:cap_pairs]
    stats = dict(n_src=len(A), n_dst=len(B), n_src_valid=int(va.sum()), n_dst_valid=int(vb.sum()), n_matched=n_matched)
    return dict(idx=idx, dist2=d2, second2=s2, pairs=pairs, stats=stats)


# ---------------------------------------------------------------- fixtures shared by the rule test and the GPU tests
def sphere_cloud(n, seed, radius=1.0, centre=(0.2, -0.1, 0.3)):
    """n points on a sphere, outward analytic normals -> (float32 [n, 3], float32 [n, 3])"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    pts = (np.asarray(centre) + radius * u).astype(np.float32)
    return pts, u.astype(np.float32)


def scene_cloud(n, seed):
    """A sphere (half the points), three tilted planes and a dozen isolated points, analytic normals; shuffled."""
    rng = np.random.default_rng(seed)
    ns = n // 2
    pts, nrm = [], []
    p, u = sphere_cloud(ns, seed + 1, 0.8)
    pts.append(p.astype(np.float64)), nrm.append(u.astype(np.float64))
    rest = n - ns - min(12, n // 8)
    for k, (normal, off) in enumerate((((0.1, 0.2, 1.0), -1.0), ((1.0, 0.3, 0.2), 1.3), ((-0.2, 1.0, 0.4), -1.4))):
        m = rest // 3 + (1 if k < rest % 3 else 0)
        nn = np.asarray(normal) / np.linalg.norm(normal)
        e1 = np.cross(nn, (0.0, 0.0, 1.0) if abs(nn[2]) < 0.9 else (1.0, 0.0, 0.0))
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(nn, e1)
        ab = rng.uniform(-1.2, 1.2, (m, 2))
        pts.append(off * nn + ab[:, :1] * e1 + ab[:, 1:] * e2)
        nrm.append(np.broadcast_to(nn, (m, 3)).copy())
    lone = n - sum(len(p) for p in pts)
    pts.append(rng.uniform(4.0, 9.0, (lone, 3)))
    v = rng.normal(size=(lone, 3))
    nrm.append(v / np.linalg.norm(v, axis=1)[:, None])
    pts, nrm = np.concatenate(pts), np.concatenate(nrm)
    order = rng.permutation(len(pts))
    return pts[order].astype(np.float32), nrm[order].astype(np.float32)


def descriptor_rows(n, seed, duplicates=0):
    """n rows of 33 float32 like FPFH rows (three groups that sum to about 200); the last `duplicates` rows repeat earlier ones"""
    rng = np.random.default_rng(seed)
    r = rng.gamma(0.7, 1.0, (n, 3, BINS))
    r = (200.0 * r / r.sum(2, keepdims=True)).reshape(n, DIM).astype(np.float32)
    if duplicates:
        r[n - duplicates:] = r[rng.integers(0, n - duplicates, duplicates)]
    return r


def _special_cloud(seed):
    """The scene with the edge cases planted: duplicated points (L = 0), a pair whose offset is parallel to both normals (|v| = 0),
    non-finite points, zero and non-finite normals."""
    pts, nrm = scene_cloud(600, seed)
    pts, nrm = pts.copy(), nrm.copy()
    pts = np.concatenate([pts, pts[:10], np.float32([[20, 20, 20], [20, 20, 20.125]]), np.float32([[np.nan, 0, 0], [0, np.inf, 0], [1, 1, -np.inf]])])
    nrm = np.concatenate([nrm, nrm[:10], np.float32([[0, 0, 1], [0, 0, 1]]), np.float32([[0, 0, 1]] * 3)])
    nrm[20:30] = 0.0
    nrm[30] = (np.nan, 0.0, 1.0)
    nrm[31] = (0.0, np.inf, 0.0)
    return pts, nrm


def _flipped_sphere(n, seed):
    pts, nrm = sphere_cloud(n, seed, 0.8)
    sign = np.where(np.random.default_rng(seed + 100).random(n) < 0.5, -1.0, 1.0).astype(np.float32)
    return pts, nrm * sign[:, None]


def fixtures():
    """name -> dict(points, normals, radius, orient, toward, cell): every cloud the GPU test compares exactly; the rule test asserts
    the bin-edge margin of each on the CPU."""
    fx = {}
    for n in (1, 2, 63, 64, 65, 257):
        p, u = sphere_cloud(n, 10 + n, 0.5)
        fx["sphere%d" % n] = dict(points=p, normals=u, radius=0.45, orient=0, toward=(0, 0, 1), cell=0.3)
    p, u = scene_cloud(3000, 3)
    fx["scene_below_cell"] = dict(points=p, normals=u, radius=0.15, orient=0, toward=(0, 0, 1), cell=0.2)
    fx["scene_reach3"] = dict(points=p, normals=u, radius=0.25, orient=0, toward=(0, 0, 1), cell=0.1)
    p, u = _special_cloud(5)
    fx["special"] = dict(points=p, normals=u, radius=0.3, orient=0, toward=(0, 0, 1), cell=0.25)
    p, u = _flipped_sphere(700, 7)
    fx["orient_none"] = dict(points=p, normals=u, radius=0.2, orient=0, toward=(0, 0, 1), cell=0.15)
    fx["orient_direction"] = dict(points=p, normals=u, radius=0.2, orient=1, toward=(0.1, -0.2, 1.0), cell=0.15)
    fx["orient_viewpoint"] = dict(points=p, normals=u, radius=0.2, orient=2, toward=(3.0, 1.0, 2.0), cell=0.15)
    p, u = sphere_cloud(700, 8, 0.8)
    fx["orient_inside"] = dict(points=p, normals=u, radius=0.2, orient=2, toward=(0.2, -0.1, 0.3), cell=0.15)
    return fx


_REFERENCES = {}


def reference(name):
    """fpfh() of a fixture, computed once and shared (do not modify the result)"""
    if name not in _REFERENCES:
        f = fixtures()[name]
        _REFERENCES[name] = fpfh(f["points"], f["normals"], f["radius"], f["orient"], f["toward"])
    return _REFERENCES[name]
