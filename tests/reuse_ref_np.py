"""The neighbour-reuse certificate of the launch list (csrc/sf_icp.hip: query_in, reuse_certificate) restated in numpy, and a brute
force over the indexed points to hold it against (tests/test_reuse_rule.py, tests/test_gpu_reuse_bound.py).
Nothing here calls the library.  Not a test module.

The device's arithmetic: the library is built with -ffp-contract=off and numpy rounds every float32 operation, so an expression
written here operation by operation, in the device's order, gives the device's bits.

  query32    the scan point under the pose: float64 products summed left to right, rounded to the float32 the search works in
  reach32    what is left of E = D + M_then once the motion so far and the rounding margins are taken off
  certifies  whether the cached neighbour (or "nothing within the acceptance radius") stands without a search
  entry32    E as the writers form it from a runner-up distance D and the motion at write time
  brute      per query the float32 lexicographic nearest (l2_simple, position) -- the rule of sf_map_nn -- and the float64 distance to
             the nearest accepted point other than a given position
  ideal_entries   the cache a perfect search would write: the nearest within the radius and E from the true distance D* of the rest
  sphere_accept / obb_accept   the window's accept rule on the indexed points (csrc/sf_nn.hpp: window_accepts)
  rigid, floor32  a small pose about a centre; the largest float32 not above a float64"""
import numpy as np

F = np.float32


def sphere_accept(P, centre, radius):
    c = np.asarray(centre, np.float32)
    d = c[None, :] - P
    return ((d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] < np.float32(float(radius) * float(radius))


def obb_accept(P, centre, R, extent):
    d = P.astype(np.float64) - np.asarray(centre, np.float64)[None, :]
    R = np.asarray(R, np.float64).reshape(3, 3)
    ok = np.ones(len(P), bool)
    for k in range(3):
        proj = (d[:, 0] * R[0, k] + d[:, 1] * R[1, k]) + d[:, 2] * R[2, k]
        ok &= np.abs(proj) <= np.asarray(extent, np.float64)[k] / 2
    return ok


def query32(T, x0):
    """T: 4x4 float64 (row major), x0: float32 [n, 3] -> float32 [n, 3]; non-finite points come out non-finite."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    x = np.asarray(x0, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = [((T[r, 0] * x[:, 0] + T[r, 1] * x[:, 1]) + T[r, 2] * x[:, 2]) + T[r, 3] for r in range(3)]
        return np.stack(s, axis=1).astype(np.float32)


def l2_simple(q, p):
    """((dx*dx) + dy*dy) + dz*dz in float32, row by row"""
    q, p = np.asarray(q, np.float32), np.asarray(p, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = q - p
        r = d[..., 0] * d[..., 0]
        r = r + d[..., 1] * d[..., 1]
        r = r + d[..., 2] * d[..., 2]
    assert r.dtype == np.float32
    return r


def reach32(e, m_now, q):
    """e - m_now*1.000002f - (|qx|+|qy|+|qz|+1)*1.3e-7f - (e+m_now)*5e-7f - 1e-6f, left to right, in float32.
    m_now: IcpState::motion (a double on the device, converted to float first)."""
    e, q = np.asarray(e, np.float32), np.asarray(q, np.float32)
    m = F(m_now)
    with np.errstate(invalid="ignore", over="ignore"):
        a = ((np.abs(q[:, 0]) + np.abs(q[:, 1])) + np.abs(q[:, 2])) + F(1.0)
        r = e - m * F(1.000002)
        r = r - a * F(1.3e-7)
        r = r - (e + m) * F(5.0e-7)
        r = r - F(1.0e-6)
    assert r.dtype == np.float32
    return r


def certifies(e, j, q, c1, thr, m_now):
    """Whether reuse_certificate lets the query go without a search: e [n] float32, j [n] int32 (negative: nothing cached), q and
    c1 [n, 3] float32 (the query now, the cached neighbour), thr = float32(max_correspondence_dist^2)."""
    e, j = np.asarray(e, np.float32), np.asarray(j)
    reach = reach32(e, m_now, q)
    with np.errstate(invalid="ignore", over="ignore"):
        near = np.sqrt(l2_simple(q, c1)) * F(1.0001) + F(1.0e-6)
        none = np.sqrt(F(thr)) * F(1.0001) + F(1.0e-6)
        assert near.dtype == np.float32 and none.dtype == np.float32
        ok = np.where(j >= 0, near < reach, none < reach)
    return ok & (e > F(0.0)) & np.isfinite(q).all(axis=1)


def entry32(d, m_then):
    """E as every writer forms it: fmaxf(d * 0.9999f + m * 0.999998f - 1e-6f, 1e-30f), d = sqrtf(lb2) float32 [n]"""
    d = np.asarray(d, np.float32)
    e = (d * F(0.9999) + F(m_then) * F(0.999998)) - F(1.0e-6)
    assert e.dtype == np.float32
    return np.maximum(e, F(1.0e-30))


def rigid(t, w, centre=0.0):
    """a rotation by the vector w (Rodrigues) about the point `centre` followed by the translation t, float64 4x4"""
    w = np.asarray(w, np.float64)
    a = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / (a if a > 0 else 1.0)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    c = np.zeros(3) + np.asarray(centre, np.float64)
    T[:3, 3] = np.asarray(t, np.float64) + c - T[:3, :3] @ c
    return T


def floor32(d):
    """the largest float32 not above the float64 d"""
    d = np.asarray(d, np.float64)
    f = d.astype(np.float32)
    return np.where(f.astype(np.float64) > d, np.nextafter(f, F(-np.inf)), f).astype(np.float32)


def ideal_entries(q, P, ok_pt, thr, m_then, inflate=1.0):
    """The cache a perfect search would write for the queries q under the motion bound m_then: the lexicographic nearest within
    thr (or none) and E from D* = the float64 distance to the nearest OTHER accepted point, rounded down to float32 (times
    `inflate`: above 1 the bound is no longer one).  -> (j int32 [n], c1 float32 [n, 3], E float32 [n]; E = 0 for non-finite q)"""
    none = np.full(len(q), -1)
    j, _, _ = brute(q, P, ok_pt, thr, none)
    _, _, other = brute(q, P, ok_pt, np.inf, j)
    E = entry32(floor32(np.minimum(other * inflate, 1.0e30)), m_then)
    E[~np.isfinite(q).all(axis=1)] = 0.0
    c1 = np.where((j >= 0)[:, None], P[np.maximum(j, 0)], 0).astype(np.float32)
    return j.astype(np.int32), c1, E


def brute(q, P, ok_pt, thr, j_excl, chunk=256):
    """q [n, 3] float32 (non-finite rows allowed: no result), P [m, 3] float32 in index order, ok_pt [m] bool (the window),
    thr: float32 acceptance threshold on d2 (strict), j_excl [n]: the position to leave out of `other` (negative: none).
    -> pos [n] int64  position of the lexicographic minimum of (bits of l2_simple, position) over accepted points with d2 < thr, -1 if none
       d2  [n] float32  its l2_simple (inf if none)
       other [n] float64  the distance to the nearest accepted point that is not j_excl (inf if there is none)"""
    q = np.asarray(q, np.float32)
    n, m = len(q), len(P)
    pos = np.full(n, -1, np.int64)
    d2 = np.full(n, np.inf, np.float32)
    other = np.full(n, np.inf)
    fin = np.flatnonzero(np.isfinite(q).all(axis=1))
    if m == 0:
        return pos, d2, other
    P64 = P.astype(np.float64)
    j_excl = np.asarray(j_excl, np.int64)
    big = np.float32(np.inf)
    for s in range(0, len(fin), chunk):
        rows = fin[s:s + chunk]
        c = q[rows]
        r = np.arange(len(c))
        d = c[:, None, 0] - P[None, :, 0]
        d *= d
        for k in (1, 2):
            t = c[:, None, k] - P[None, :, k]
            t *= t
            d += t
        assert d.dtype == np.float32
        d[:, ~ok_pt] = big
        # argmin takes the first of equal values: the lowest position among equal distances, the lexicographic minimum
        best = d.argmin(axis=1)
        dm = d[r, best]
        took = dm < np.float32(thr)
        pos[rows] = np.where(took, best, -1)
        d2[rows] = np.where(took, dm, np.inf)
        # float64 only where it can matter: l2_simple of float32 points is within 4e-7 of the true squared distance (three
        # differences, three squares, two sums, each rounded once), so the true nearest OTHER point is among those whose float32
        # value is within 2e-6 of the smallest
        je = j_excl[rows]
        has = je >= 0
        d[r[has], je[has]] = big
        lim = d.min(axis=1)
        lim = np.where(np.isfinite(lim), lim * np.float32(1.000002) + np.float32(1.0e-37), np.float32(-1.0))
        rr, cc = np.nonzero(d <= lim[:, None])
        e = ((c[rr].astype(np.float64) - P64[cc]) ** 2).sum(axis=1)
        o = np.full(len(c), np.inf)
        np.minimum.at(o, rr, e)
        other[rows] = np.sqrt(o)
    return pos, d2, other
