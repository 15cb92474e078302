"""The neighbour table and its re-search rule (sf_map_build_neighbour_table, sf::nn_research_table) written out in numpy,
float32 operation by float32 operation, for tests/test_neighbour_table_rule.py (against brute force) and
tests/test_gpu_neighbour_table.py (against the device).  Not a test module."""
import numpy as np

F = np.float32
NONE = np.uint32(0xFFFFFFFF)
K = 7
BIG = F(3.0e38)


def l2_simple(a, b):
    """FLANN L2_Simple in float32: ((dx*dx) + dy*dy) + dz*dz, every operation rounded"""
    d = np.asarray(a, F) - np.asarray(b, F)
    r = d[..., 0] * d[..., 0]
    r = r + d[..., 1] * d[..., 1]
    r = r + d[..., 2] * d[..., 2]
    return r.astype(F)


def hit_key(d2, j):
    return (np.asarray(d2, F).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(j).astype(np.uint32).astype(np.uint64)


def cells_of(pts, org, inv_h, dims):
    """the cell of every point, by the expression of the index build (float32, clamped into the grid)"""
    g = np.floor((np.asarray(pts, F) - np.asarray(org, F)) * F(inv_h))
    return np.minimum(np.maximum(g, F(0)), (np.asarray(dims) - 1).astype(F)).astype(np.int64)


def simple_grid(pts, cell):
    """a grid of the test's own (origin at the smallest coordinates): (points sorted by cell, x fastest; org, inv_h, dims, gap_eps)"""
    pts = np.asarray(pts, F)
    org = pts.min(0)
    dims = np.floor((pts.max(0).astype(np.float64) - org.astype(np.float64)) / cell).astype(np.int64) + 1
    inv_h = F(1.0 / cell)
    c = cells_of(pts, org, inv_h, dims)
    key = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    order = np.argsort(key, kind="stable")
    gap_eps = F(1.5) * F(2.384186e-7) * F(dims.max()) * F(cell)
    return pts[order], org, inv_h, dims, gap_eps


def cap_of(h, gap_eps):
    return F(max(F(h) - F(gap_eps), F(0))) * F(0.999)


def build_table(pts, cells, h, gap_eps, chunk=512):
    """(ids [n, 7] uint32 sorted positions, NONE where there is none; r [n] float32) of points in sorted order"""
    pts = np.asarray(pts, F)
    n = len(pts)
    cap = cap_of(h, gap_eps)
    cap2 = F(cap * cap)
    ids = np.full((n, K), NONE, np.uint32)
    r = np.full(n, cap, F)
    pos = np.arange(n, dtype=np.uint32)
    allmax = np.uint64(0xFFFFFFFFFFFFFFFF)
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        d2 = l2_simple(pts[a:b, None, :], pts[None, :, :])
        near = (np.abs(cells[a:b, None, :] - cells[None, :, :]) <= 1).all(-1)
        ok = near & (d2 < cap2) & (pos[None, :] != pos[a:b, None])
        key = np.where(ok, hit_key(d2, np.broadcast_to(pos[None, :], d2.shape)), allmax)
        kk = min(K, n)
        part = np.sort(np.partition(key, kk - 1, axis=1)[:, :kk], axis=1)
        part = np.concatenate([part, np.full((b - a, K - kk), allmax, np.uint64)], axis=1)
        ids[a:b] = (part & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        full = part[:, K - 1] != allmax
        d7 = (part[:, K - 1] >> np.uint64(32)).astype(np.uint32).view(F)
        r[a:b] = np.where(full, np.sqrt(d7, dtype=F) * F(0.9999), cap)
    return ids, r


def research(pts, ids, r, q, seed, thr):
    """The rule for queries q [m, 3] from the cached points seed [m] (sorted positions, all valid).
    -> served [m] bool, winner [m] int64 (-1: nothing under thr), d2 [m] float32 of the best candidate, lb [m] float32: every
    point but the winner -- every point at all when the winner is -1 -- is at least lb from the query"""
    pts, q = np.asarray(pts, F), np.asarray(q, F)
    seed = np.asarray(seed, np.int64)
    cand = np.concatenate([seed[:, None].astype(np.uint32), ids[seed]], axis=1)          # [m, 8]
    valid = cand != NONE
    cp = pts[np.where(valid, cand, 0).astype(np.int64)]
    d2 = l2_simple(q[:, None, :], cp)
    key = np.where(valid, hit_key(d2, cand), np.uint64(0xFFFFFFFFFFFFFFFF))
    rows = np.arange(len(q))
    dp = np.sqrt(d2[:, 0], dtype=F)

    def fold(upto):
        bi = np.argmin(key[:, :upto], axis=1)
        others = np.where(valid[:, :upto], d2[:, :upto], BIG)
        others[rows, bi] = BIG
        return bi, d2[rows, bi], others.min(axis=1)
    # p and the first four first: with a fifth listed, the fourth's distance from p stands in for r (the list is in key order)
    b5, d5, s5 = fold(5)
    r4 = np.sqrt(l2_simple(pts[seed], cp[:, 4]), dtype=F) * F(0.9999)
    early = valid[:, 5] & (((dp + np.sqrt(d5, dtype=F)) * F(1.0001) + F(2.0e-6)) < r4)
    b8, d8, s8 = fold(8)
    bi, d2b, second = np.where(early, b5, b8), np.where(early, d5, d8), np.where(early, s5, s8)
    rr = np.where(early, r4, r[seed]).astype(F)
    served = ((dp + np.sqrt(d2b, dtype=F)) * F(1.0001) + F(2.0e-6)) < rr
    lb = np.maximum(np.minimum(np.sqrt(second, dtype=F) * F(0.9999), rr - dp * F(1.0001) - F(1.0e-6)), F(0))
    # nothing under thr: the bound of a "no neighbour" entry covers EVERY point, the best candidate included
    lb = np.where(d2b < F(thr), lb, np.minimum(lb, np.sqrt(d2b, dtype=F) * F(0.9999)))
    winner = np.where(d2b < F(thr), cand[rows, bi].astype(np.int64), -1)
    return served, winner, d2b, lb.astype(F)


def brute_force(pts, q, thr, chunk=1024):
    """lexicographic (d2, position) minimum over all points -> (winner or -1, d2 of the best, float64 distance to every point [m, n])"""
    pts, q = np.asarray(pts, F), np.asarray(q, F)
    win = np.empty(len(q), np.int64)
    best = np.empty(len(q), F)
    pos = np.arange(len(pts), dtype=np.uint32)
    for a in range(0, len(q), chunk):
        d2 = l2_simple(q[a:a + chunk, None, :], pts[None, :, :])
        j = np.argmin(hit_key(d2, np.broadcast_to(pos[None, :], d2.shape)), axis=1)
        best[a:a + chunk] = d2[np.arange(len(j)), j]
        win[a:a + chunk] = j
    return np.where(best < F(thr), win, -1), best


def min_other_distance(pts, q, exclude, chunk=1024):
    """float64 distance from each query to the nearest point other than exclude[i] (-1: exclude nothing)"""
    p64, q64 = np.asarray(pts, np.float64), np.asarray(q, np.float64)
    out = np.empty(len(q64))
    for a in range(0, len(q64), chunk):
        d = np.sqrt(((q64[a:a + chunk, None, :] - p64[None, :, :]) ** 2).sum(-1))
        ex = exclude[a:a + chunk]
        has = ex >= 0
        d[np.nonzero(has)[0], ex[has]] = np.inf
        out[a:a + chunk] = d.min(1)
    return out
