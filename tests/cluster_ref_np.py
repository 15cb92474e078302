"""The clustering rule of DESIGN §15 (sf_map_cluster_dbscan, sf_map_cluster_euclidean and the two cloud calls) restated in numpy
and scipy; tests/test_cluster_rule.py pins it to scikit-learn's DBSCAN and to scipy's components of the float64 graph.

Edges: the indexed (finite) points i != j with l2_simple(x_i, x_j) < float32(eps * eps), float32, unfused, strict.  Candidates come
from cKDTree.query_pairs at 1.001 eps in float64 (a pair the float32 rule accepts is within eps (1 + 1e-6)), the rule decides.
Core: count_i >= min_points, the point itself counted.  Clusters: scipy's connected components of the core graph, numbered by their
smallest core index.  Border: a point that is not core takes the smallest label among its core neighbours.  Everything else: -1."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

STAT_KEYS = ("n_points", "n_valid", "n_core", "n_border", "n_noise", "n_clusters", "largest_size", "n_kept")


def l2_simple(a, b):
    """float32 (dx*dx + dy*dy) + dz*dz of matching rows, every operation rounded on its own"""
    d = np.asarray(a, np.float32) - np.asarray(b, np.float32)
    r = d[:, 0] * d[:, 0]
    r = r + d[:, 1] * d[:, 1]
    return r + d[:, 2] * d[:, 2]


def r2_of(eps):
    return np.float32(np.float64(eps) * np.float64(eps))


def edges(x, eps):
    """-> (pairs int64 [E, 2] of original indices, i < j; finite bool [n])"""
    x = np.asarray(x, np.float32).reshape(-1, 3)
    finite = np.isfinite(x).all(1)
    ids = np.flatnonzero(finite)
    if len(ids) < 2:
        return np.zeros((0, 2), np.int64), finite
    pts = x[ids]
    pr = cKDTree(pts.astype(np.float64)).query_pairs(float(eps) * 1.001, output_type="ndarray").reshape(-1, 2)
    pr = pr[l2_simple(pts[pr[:, 0]], pts[pr[:, 1]]) < r2_of(eps)]
    return ids[pr].astype(np.int64), finite


def counts(n, pairs, finite):
    cnt = finite.astype(np.int64)
    np.add.at(cnt, pairs[:, 0], 1)
    np.add.at(cnt, pairs[:, 1], 1)
    return cnt


def _stats(labels, finite, core):
    sizes = np.bincount(labels[labels >= 0]).astype(np.int32) if (labels >= 0).any() else np.zeros(0, np.int32)
    kept = int((labels >= 0).sum())
    n_core = int(core.sum())
    st = dict(n_points=len(labels), n_valid=int(finite.sum()), n_core=n_core, n_border=0, n_noise=int(finite.sum()) - kept, n_clusters=len(sizes),
              largest_size=int(sizes.max()) if len(sizes) else 0, n_kept=kept)
    return sizes, st


def dbscan(x, eps, min_points):
    """-> (labels int32 [n], sizes int32 [C], stats dict, core bool [n])"""
    x = np.asarray(x, np.float32).reshape(-1, 3)
    n = len(x)
    pairs, finite = edges(x, eps)
    core = finite & (counts(n, pairs, finite) >= min_points)
    labels = np.full(n, -1, np.int32)
    ci = np.flatnonzero(core)
    if len(ci):
        cc = pairs[core[pairs[:, 0]] & core[pairs[:, 1]]]
        graph = coo_matrix((np.ones(len(cc), np.int8), (cc[:, 0], cc[:, 1])), shape=(n, n))
        comp = connected_components(graph, directed=False)[1][ci]
        _, first, inverse = np.unique(comp, return_index=True, return_inverse=True)   # first: position in ci, ascending with the index
        order = np.empty(len(first), np.int64)
        order[np.argsort(first, kind="stable")] = np.arange(len(first))
        labels[ci] = order[inverse]
        big = np.iinfo(np.int32).max
        best = np.full(n, big, np.int32)
        for a, b in ((0, 1), (1, 0)):
            sel = core[pairs[:, a]] & ~core[pairs[:, b]]
            np.minimum.at(best, pairs[sel, b], labels[pairs[sel, a]])
        border = ~core & (best < big)
        labels[border] = best[border]
    sizes, st = _stats(labels, finite, core)
    st["n_border"] = st["n_kept"] - st["n_core"]
    return labels, sizes, st, core


def euclidean(x, tolerance, min_size=1, max_size=0):
    """-> (labels int32 [n], sizes int32 [C], stats dict): the components, those outside min_size .. max_size dropped, the rest
    renumbered in the same order"""
    labels, sizes, st, core = dbscan(x, tolerance, 1)
    keep = (sizes >= min_size) & ((sizes <= max_size) if max_size > 0 else True)
    new = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    has = labels >= 0
    labels[has] = new[labels[has]]
    sizes, st = _stats(labels, np.isfinite(np.asarray(x, np.float32).reshape(-1, 3)).all(1), core)
    return labels, sizes, st


def filter_clusters(x, tolerance, min_size, max_size=0):
    """-> (mask bool [n] of the points sf_cloud_filter_clusters keeps, stats dict)"""
    labels, _, st = euclidean(x, tolerance, min_size, max_size)
    return labels >= 0, st


def keep_largest_cluster(x, tolerance):
    """-> (mask bool [n], stats dict): the largest cluster, on a tie the one with the smallest label; n_kept and n_noise say what stayed
    and what went"""
    labels, sizes, st = euclidean(x, tolerance)
    if not len(sizes):
        return np.zeros(len(labels), bool), st
    mask = labels == int(np.argmax(sizes))                              # argmax: the first of equals
    st = dict(st, n_kept=int(mask.sum()), n_noise=st["n_valid"] - int(mask.sum()))
    return mask, st


def contested_cloud(eps, a_first=True):
    """Two blobs of 12 points inside spheres of radius eps / 4 whose centres are 1.6 eps apart (no point of one is adjacent to a point
    of the other) and one lone point at the midpoint, the last row.  Three points of each blob lie on the side facing the midpoint,
    0.7 eps from it, the other nine on the far side, more than eps from it: the lone point counts 7 with itself, so at min_points = 8
    it is a border point of both clusters while all 24 blob points are core.  a_first: blob A (around the origin) comes first."""
    rng = np.random.default_rng(12)

    def blob(cx, s):
        far = np.stack([np.full(9, cx - s * 0.23 * eps), *rng.uniform(-0.02 * eps, 0.02 * eps, (2, 9))], 1)
        near = np.stack([np.full(3, cx + s * 0.1 * eps), *rng.uniform(-0.02 * eps, 0.02 * eps, (2, 3))], 1)
        return np.concatenate([far, near])[rng.permutation(12)]

    a, b = blob(0.0, 1.0), blob(1.6 * eps, -1.0)
    mid = np.array([[0.8 * eps, 0.0, 0.0]])
    return np.concatenate([a, b, mid] if a_first else [b, a, mid]).astype(np.float32)


PARITY_EPS = (0.12, 0.2, 0.3)


def near_pairs(x, eps):
    """the pairs whose float64 distance lies within eps (1 +- 1e-5)"""
    P = np.asarray(x, np.float64)
    pr = cKDTree(P).query_pairs(eps * (1 + 1e-5), output_type="ndarray").reshape(-1, 2)
    d = np.linalg.norm(P[pr[:, 0]] - P[pr[:, 1]], axis=1)
    return pr[d >= eps * (1 - 1e-5)]


def blob_cloud(n=20_000, blobs=25, scatter=0.1, seed=3, clear_of=PARITY_EPS):
    """`blobs` Gaussian blobs (sigma 0.25 m) in a 12 m cube plus a share `scatter` of uniform points, in shuffled order.  Among 2e8
    pairs some dozens lie within 1e-5 of one of the radii `clear_of`, whatever the seed: one point of each such pair is drawn again
    (from the same blob, or uniformly) until none is left, so that < in float32 and <= in float64 draw the same graph on this cloud."""
    rng = np.random.default_rng(seed)
    ns = int(round(n * scatter))
    cen = rng.uniform(-5, 5, (blobs, 3))
    which = np.concatenate([rng.integers(0, blobs, n - ns), np.full(ns, -1)])

    def draw(w):
        return np.where((w >= 0)[:, None], cen[np.maximum(w, 0)] + rng.normal(0, 0.25, (len(w), 3)), rng.uniform(-6, 6, (len(w), 3))).astype(np.float32)

    which = which[rng.permutation(n)]
    x = draw(which)
    for _ in range(20):
        bad = np.unique(np.concatenate([near_pairs(x, eps)[:, 0] for eps in clear_of])) if len(clear_of) else []
        if not len(bad):
            return x
        x[bad] = draw(which[bad])
    raise AssertionError("blob_cloud: pairs at a radius remain")


def near_eps_pairs(x, eps):
    """the number of pairs whose float64 distance lies in eps (1 +- 1e-5): with none, < in float32 and <= in float64 draw the same graph"""
    t = cKDTree(np.asarray(x, np.float64))
    return int(t.count_neighbors(t, eps * (1 + 1e-5)) - t.count_neighbors(t, eps * (1 - 1e-5)))
