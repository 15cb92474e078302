"""numpy restatement of the outlier-removal rules (include/slamfusion.h), brute force.

Distances are float32 `((dx*dx)+dy*dy)+dz*dz` between the finite ("indexed") points.  Statistical: the K smallest d2 of a point
(its own zero included) in ascending order are list positions 0 .. K-1, position p contributes sqrt(float64(d2_p)), absent positions
+0.0, summed in the pairwise tree over 64 positions; the global sums run over the points in original order (points that are not
indexed +0.0) in the pairwise tree over the array padded with +0.0 to a power of two.  Radius: a strict float32 count."""
import numpy as np


def d2_rows(Q, P):
    """[len(Q), len(P)] float32"""
    dx, dy, dz = (Q[:, None, d] - P[None, :, d] for d in range(3))
    d = ((dx * dx) + dy * dy) + dz * dz
    assert d.dtype == np.float32
    return d


def tree64(v):
    """[n, 64] -> [n]: ((v0 + v1) + (v2 + v3)) + ..."""
    assert v.shape[1] == 64
    while v.shape[1] > 1:
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def tree_sum(v):
    """float64 [n] -> the pairwise tree over v padded with +0.0 to the next power of two"""
    v = np.asarray(v, np.float64)
    size = 1
    while size < max(len(v), 1):
        size *= 2
    v = np.concatenate([v, np.zeros(size - len(v))])
    while len(v) > 1:
        v = v[0::2] + v[1::2]
    return float(v[0])


def list_length(k, flavour):
    return k + 1 if flavour == "pcl" else k


def mean_distances(points, k, flavour):
    """-> d float64 [n] (NaN where the point is not finite), n_valid"""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    ok = np.isfinite(pts).all(1)
    P = np.ascontiguousarray(pts[ok])
    nv = len(P)
    K = list_length(k, flavour)
    cnt = min(K, nv)
    out = np.full(len(pts), np.nan)
    if nv == 0:
        return out, 0
    d = np.empty(nv)
    for s in range(0, nv, 512):
        d2 = np.sort(d2_rows(P[s:s + 512], P), axis=1)[:, :cnt]                  # equal values may swap places: equal terms
        lst = np.zeros((len(d2), 64))
        lst[:, :cnt] = np.sqrt(d2.astype(np.float64))
        total = tree64(lst)
        if flavour == "pcl":
            d[s:s + 512] = total / (cnt - 1) if cnt >= 2 else 0.0
        else:
            d[s:s + 512] = total / cnt
    out[ok] = d
    return out, nv


def statistical(points, k, std_ratio=2.0, flavour="pcl"):
    """-> keep bool [n], d float64 [n], stats dict"""
    d, nv = mean_distances(points, k, flavour)
    ok = ~np.isnan(d)
    mean = stddev = 0.0
    if nv > 0:
        mean = tree_sum(np.where(ok, d, 0.0)) / nv
    if nv >= 2:
        dev = np.where(ok, d - mean, 0.0)
        stddev = float(np.sqrt(tree_sum(dev * dev) / (nv - 1)))
    thr = mean + std_ratio * stddev
    with np.errstate(invalid="ignore"):
        keep = (d <= thr) if flavour == "pcl" else (d < thr)
    keep &= ok
    return keep, d, dict(n_points=len(d), n_valid=nv, n_kept=int(keep.sum()), mean=mean, stddev=stddev, threshold=thr)


def radius_counts(points, radius):
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    ok = np.isfinite(pts).all(1)
    P = np.ascontiguousarray(pts[ok])
    r2 = np.float32(float(radius) * float(radius))
    cnt = np.zeros(len(pts), np.int32)
    c = np.empty(len(P), np.int32)
    for s in range(0, len(P), 512):
        c[s:s + 512] = (d2_rows(P[s:s + 512], P) < r2).sum(1)
    cnt[ok] = c
    return cnt


def radius(points, radius, min_neighbors):
    """-> keep bool [n], n_neighbors int32 [n] (the point itself included), stats dict"""
    cnt = radius_counts(points, radius)
    ok = np.isfinite(np.asarray(points, np.float32).reshape(-1, 3)).all(1)
    keep = (cnt > min_neighbors) & ok
    return keep, cnt, dict(n_points=len(cnt), n_valid=int(ok.sum()), n_kept=int(keep.sum()), mean=0.0, stddev=0.0, threshold=0.0)


N_SURFACE, N_PLANTED = 4000, 40


def planted_cloud():
    """4 000 surface points uniform in +-3 m, half on the plane z = 0 and half on x = 2 (sigma 5 mm), then 40 points uniform in the box
    away from both planes (|z| > 0.5 and |x - 2| > 0.5); seed 7.  -> float32 [4040, 3], the surface points first."""
    rng = np.random.default_rng(7)
    s = rng.uniform(-3, 3, (N_SURFACE, 3))
    s[:N_SURFACE // 2, 2] = rng.normal(0, 0.005, N_SURFACE // 2)
    s[N_SURFACE // 2:, 0] = 2.0 + rng.normal(0, 0.005, N_SURFACE - N_SURFACE // 2)
    lone = np.empty((0, 3))
    while len(lone) < N_PLANTED:
        c = rng.uniform(-3, 3, (4 * N_PLANTED, 3))
        lone = np.concatenate([lone, c[(np.abs(c[:, 2]) > 0.5) & (np.abs(c[:, 0] - 2.0) > 0.5)]])
    return np.concatenate([s, lone[:N_PLANTED]]).astype(np.float32)
