"""The plane segmentation rule restated in numpy (include/slamfusion.h, sf_cloud_segment_plane): samples,
hypotheses, score, choice, refit and final flags, stage by stage, so that the device can be compared with each of them.  Nothing
here calls the library.  tests/test_plane_rule.py pins this file to independent code (numpy.cross, numpy.linalg.norm, a float64
distance count, numpy.linalg.svd); tests/test_gpu_plane.py compares the device with it."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
MAX_HYPOTHESES = 4096


def mix(x):
    """the splitmix64 step on uint64 with wrap-around"""
    z = (x + GOLDEN) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def samples(seed, num_hypotheses, n):
    """int32 [H, 3]: hypothesis h samples the original indices mix(seed + GOLDEN (3h + j + 1)) mod n"""
    out = np.empty((num_hypotheses, 3), np.int32)
    for k in range(3 * num_hypotheses):
        out[k // 3, k % 3] = mix((seed + GOLDEN * (k + 1)) & M64) % n
    return out


def unit_axis(axis):
    """the axis normalised in float64, None for none (all zeros)"""
    if axis is None:
        return None
    a = np.asarray(axis, np.float64).reshape(3)
    if not a.any():
        return None
    return a / np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])


def planes_f64(xyz, idx, axis=None, axis_min_cos=0.0):
    """float64, unfused, left to right -> (planes float64 [H, 4] before the one rounding, ok bool [H]: not degenerate)"""
    xyz = np.asarray(xyz, np.float32)
    ax = unit_axis(axis)
    p0, p1, p2 = (xyz[idx[:, j]].astype(np.float64) for j in range(3))
    with np.errstate(all="ignore"):
        u, v = p1 - p0, p2 - p0
        N = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
        nn = N[:, 0] * N[:, 0]
        nn = nn + N[:, 1] * N[:, 1]
        nn = nn + N[:, 2] * N[:, 2]
        ok = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2]) & np.isfinite(nn) & (nn > 0)
        nh = N / np.sqrt(nn)[:, None]
        if ax is not None:
            dot = nh[:, 0] * ax[0]
            dot = dot + nh[:, 1] * ax[1]
            dot = dot + nh[:, 2] * ax[2]
            ok &= ~(np.abs(dot) < axis_min_cos)
            flip = ~(dot >= 0)
        else:
            x, y, z = nh[:, 0], nh[:, 1], nh[:, 2]
            flip = (z < 0) | ((z == 0) & ((y < 0) | ((y == 0) & (x < 0))))
        nh = np.where(flip[:, None], -nh, nh)
        d = nh[:, 0] * p0[:, 0]
        d = d + nh[:, 1] * p0[:, 1]
        d = d + nh[:, 2] * p0[:, 2]
        return np.concatenate([nh, -d[:, None]], axis=1), ok


def planes_from_samples(xyz, idx, axis=None, axis_min_cos=0.0):
    """-> (planes float32 [H, 4]: planes_f64 rounded once, four NaNs for a degenerate one; the number of those)"""
    planes, ok = planes_f64(xyz, idx, axis, axis_min_cos)
    with np.errstate(all="ignore"):
        planes = planes.astype(np.float32)
    planes[~ok] = np.nan
    return planes, int((~ok).sum())


def hypotheses(xyz, num_hypotheses, seed=0, axis=None, axis_min_cos=0.0):
    """-> (planes float32 [H, 4], samples int32 [H, 3], n_degenerate)"""
    idx = samples(seed, num_hypotheses, len(xyz))
    planes, n_deg = planes_from_samples(xyz, idx, axis, axis_min_cos)
    return planes, idx, n_deg


def inliers(xyz, plane, distance_threshold):
    """bool [n]: fabsf(s) < t with s = a x; s = s + b y; s = s + c z; s = s + d in float32, unfused"""
    xyz = np.asarray(xyz, np.float32)
    a, b, c, d = (np.float32(v) for v in plane)
    t = np.float32(distance_threshold)
    with np.errstate(all="ignore"):
        s = a * xyz[:, 0]
        s = s + b * xyz[:, 1]
        s = s + c * xyz[:, 2]
        s = s + d
        return np.abs(s) < t


def score(xyz, planes, distance_threshold, chunk=64):
    """int64 [H]: the inliers of every plane"""
    xyz = np.asarray(xyz, np.float32)
    planes = np.asarray(planes, np.float32).reshape(-1, 4)
    t = np.float32(distance_threshold)
    x, y, z = xyz[None, :, 0], xyz[None, :, 1], xyz[None, :, 2]
    counts = np.zeros(len(planes), np.int64)
    with np.errstate(all="ignore"):
        for lo in range(0, len(planes), chunk):
            pl = planes[lo:lo + chunk]
            s = pl[:, 0:1] * x
            s = s + pl[:, 1:2] * y
            s = s + pl[:, 2:3] * z
            s = s + pl[:, 3:4]
            assert s.dtype == np.float32
            counts[lo:lo + chunk] = (np.abs(s) < t).sum(axis=1)
    return counts


def choose(counts, min_inliers=3):
    """-> (best index: the largest count, on a tie the smallest h; its count; found)"""
    best = int(np.argmax(counts))      # (numpy returns the first of equal maxima)
    return best, int(counts[best]), int(counts[best] >= min_inliers)


def refit(xyz, plane, distance_threshold):
    """the float64 moments of x - c0 over the inliers of `plane` -> (refitted plane float32 [4], refined)"""
    plane = np.asarray(plane, np.float32)
    sel = inliers(xyz, plane, distance_threshold)
    cnt = int(sel.sum())
    if cnt < 3:
        return plane.copy(), 0
    n0 = plane[:3].astype(np.float64)
    c0 = -np.float64(plane[3]) * n0
    dx = np.asarray(xyz, np.float32)[sel].astype(np.float64) - c0
    m = dx.sum(axis=0) / cnt
    cov = (dx[:, :, None] * dx[:, None, :]).sum(axis=0) / cnt - np.outer(m, m)
    if not (np.isfinite(cov).all() and np.isfinite(m).all()):
        return plane.copy(), 0
    w, V = np.linalg.eigh(cov)
    nrm = V[:, 0]
    if nrm @ n0 < 0:
        nrm = -nrm
    out = np.concatenate([nrm, [-(nrm @ (c0 + m))]]).astype(np.float32)
    if not np.isfinite(out).all():
        return plane.copy(), 0
    return out, 1


def segment(xyz, distance_threshold=0.1, num_hypotheses=1024, refine=True, seed=0, min_inliers=3, axis=None, axis_min_cos=0.0):
    """the whole call -> dict(plane, inlier, counts, planes, stats)"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    st = dict(n_points=n, n_hypotheses=0, n_degenerate=0, best_index=0, best_count=0, n_inliers=0, found=0, refined=0)
    if n == 0:
        return dict(plane=np.zeros(4, np.float32), inlier=np.zeros(0, bool), counts=None, planes=None, stats=st)
    planes, _, n_deg = hypotheses(xyz, num_hypotheses, seed, axis, axis_min_cos)
    counts = score(xyz, planes, distance_threshold)
    best, count, found = choose(counts, min_inliers)
    st.update(n_hypotheses=num_hypotheses, n_degenerate=n_deg, best_index=best, best_count=count, found=found)
    plane, inl = np.zeros(4, np.float32), np.zeros(n, bool)
    if found:
        plane = planes[best].copy()
        if refine:
            plane, st["refined"] = refit(xyz, plane, distance_threshold)
        inl = inliers(xyz, plane, distance_threshold)
    st["n_inliers"] = int(inl.sum())
    return dict(plane=plane, inlier=inl, counts=counts, planes=planes, stats=st)


# ------------------------------------------------------------------ the workhorse cloud of the tests
GROUND = (0.05, -0.03, 1.5)     # z = 0.05 x - 0.03 y + 1.5


def workhorse(n=20_000, seed=2024):
    """half on the plane z = 0.05 x - 0.03 y + 1.5 with sigma = 0.02 noise, a quarter on the wall y = 7, a quarter uniform; shuffled;
    NaN and inf coordinates planted every ~1000 points.  float32 [n, 3]."""
    rng = np.random.default_rng(seed)
    h, q = n // 2, n // 4
    g = rng.uniform(-10, 10, (h, 3))
    g[:, 2] = GROUND[0] * g[:, 0] + GROUND[1] * g[:, 1] + GROUND[2] + rng.normal(0, 0.02, h)
    w = rng.uniform(-10, 10, (q, 3))
    w[:, 1] = 7.0
    w[:, 2] = rng.uniform(0, 6, q)
    u = rng.uniform(-10, 10, (n - h - q, 3))
    pts = np.concatenate([g, w, u])[rng.permutation(n)].astype(np.float32)
    bad = (np.nan, np.inf, -np.inf)
    for k, i in enumerate(range(500, n, 1000)):
        pts[i + k % 7, k % 3] = bad[k % 3]
    return pts
