"""numpy restatement of the radius normals (sf_map_estimate_normals / sf_map_estimate_normals_cov, include/slamfusion.h; k_normals ->
normals_point in csrc/sf_map.hip) and the named fixtures of their tests.  Nothing here knows about cells: every neighbourhood is
found by brute force over all pairs.

The rule.  The neighbourhood of an indexed point p is every indexed point q, p included, with ex^2 + ey^2 + ez^2 <= (double)radius^2,
e = (double)q - (double)p the differences of the float32 coordinates taken in float64 (they are exact there), the sum evaluated
in float64 without fusing, radius the float32 the call receives.  The count goes to .w of the normal.  Below 3 neighbours the normal
is (0, 0, 1) and the covariance is zero.  Otherwise: the float64 mean of the neighbours, the centred sums C = sum (q - mean)(q - mean)^T
as xx xy xz yy yz zz, cov6 = C / count; the normal is the unit eigenvector of the smallest eigenvalue of C, rounded to float32 and
oriented z > 0, then y > 0, then x > 0.  An axis-aligned C (every off-diagonal entry exactly 0) takes the axis of the FIRST smallest
diagonal entry, so a neighbourhood on one spot gives +x.
Points that are not indexed (a non-finite coordinate) are nobody's neighbour; sf_map_download_normals returns normal (0, 0, 0) and
count 0 for them and sf_map_download_covariances six zeros (both clear the host-ordered buffer before the indexed points are written).

Here the sums are taken in long double (64-bit significand) and rounded once; the spectrum is numpy.linalg.eigh's.  No summation order
of the device is copied, so the comparison carries tolerances.  u = 2^-53, m = count, r = radius, X = the largest |coordinate|:

 cov6   The device sums m float64 numbers of size <= X one after another: off by at most (m - 1) u m X, the mean after the division
        by d = m u X.  All neighbours and their mean lie within r of p, so a centred difference is at most 2 r per axis and carries
        one rounding, 2 u r.  Because sum (q - mean) = 0, an error d of the mean enters C only as m d d^T and through the rounded
        differences (4 m u^2 X r, nothing): per entry of C / m that is d^2.  First order, per entry of C: the rounded differences
        2 * 2r * 2ur = 8 u r^2 per term, the rounded product 4 u r^2 per term, the sum of m products of size <= 4 r^2 one after
        another (m - 1) u m 4 r^2; divided by m, with the division's own rounding 4 u r^2 and the one rounding of this restatement
        4 u r^2:  tol_cov = (4 m + 16) u r^2 + 2 (m u X)^2, per entry.  (The second term is what a map far from the origin adds: it
        grows with X^2 but stays second order.)  As a 3 x 3 matrix the error has spectral norm E_cov <= 3 tol_cov.
 normal, separated   The device solves its own C / m + E, |E|_2 <= E_cov, by cyclic Jacobi; tests/test_gpu_linalg_direct.py holds
        that solve to sin <= 64 eps |C| / gap (eps = 2^-52, |C| the largest eigenvalue).  With E = E_cov + 64 eps l2 and the
        reference's gap = l1 - l0 > 2 E, Davis-Kahan gives sin(angle) <= E / (gap - E); the components are then rounded to float32,
        each by at most 2^-25, the vector by sqrt(3) 2^-25 < 2^-24:  tol_sin = E / (gap - E) + 2^-24.  A point counts as separated
        when gap >= max(1e-6 l2, 100 E).
 normal, not separated (collinear, isotropic, one spot)   unit length: | |n| - 1 | <= 2^-24 (the same float32 rounding).  Rayleigh
        excess: the device's float64 vector v has v^T (C/m) v - l0 <= 2 E_cov + 64 eps l2 =: a (its own matrix is within E_cov, twice:
        the value and l0); rounding v to n = v + e, |e| <= 2^-24, adds at most 2 |e| |res| + l2 |e|^2 with the residual
        |res| <= sqrt(a l2):  tol_rayleigh = a + 2^-23 sqrt(a l2) + 2^-48 l2.  The excess is measured on n / |n| in float64.
 Exact rows: where the restatement's off-diagonal sums are exactly 0 and the device's are too (the fixtures that rely on it keep
        every coordinate sum exact: see `exact`), the normal is asserted bit for bit.  The same holds for an exactly flat
        neighbourhood (x = c: xx = xy = xz = 0 exactly) whose other two eigenvalues are positive: no rotation touches that axis, its
        diagonal entry 0 is the only smallest one, the normal is that axis.

The predicate itself carries no tolerance: `ambiguous` counts the pairs whose exact d^2 is within 8 u of r^2 without being equal to
it, and every fixture's precondition is that there are none, so that the float64 evaluation cannot depend on how it is rounded."""
import functools
import math

import numpy as np

U = 2.0 ** -53
EPS = 2.0 ** -52
F = np.float32
LD = np.longdouble
SYM = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))                      # xx xy xz yy yz zz
Z_UP = np.array([0, 0, 1], np.float32)


def sign_rule(n):
    """n [k, 3] -> oriented z > 0, then y > 0, then x > 0"""
    n = np.array(n, copy=True)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    flip = (z < 0) | ((z == 0) & ((y < 0) | ((y == 0) & (x < 0))))
    n[flip] = -n[flip]
    return n


def obeys_sign_rule(n):
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    return (z > 0) | ((z == 0) & ((y > 0) | ((y == 0) & (x > 0))))


def sym3(c6):
    c6 = np.asarray(c6)
    M = np.zeros(c6.shape[:-1] + (3, 3), c6.dtype)
    for d, (i, j) in enumerate(SYM):
        M[..., i, j] = M[..., j, i] = c6[..., d]
    return M


def neighbours(points, radius, chunk=256):
    """-> (lists: per point the ascending ids of its neighbourhood, empty for a point that is not indexed; ambiguous: how many ordered
    pairs have an exact d^2 within 8 u of r^2 without being equal to it; at_r: pairs with d^2 == r^2 exactly)"""
    P = np.asarray(points, np.float32).reshape(-1, 3)
    ok = np.isfinite(P).all(1)
    ids = np.flatnonzero(ok)
    Q = P[ids].astype(np.float64)
    r = float(F(radius))
    r2 = r * r
    r2L = LD(r) * LD(r)
    lists = [np.zeros(0, np.int64) for _ in range(len(P))]
    ambiguous = at_r = 0
    for a in range(0, len(Q), chunk):
        e = Q[None, :, :] - Q[a:a + chunk, None, :]
        d2 = (e[:, :, 0] * e[:, :, 0] + e[:, :, 1] * e[:, :, 1]) + e[:, :, 2] * e[:, :, 2]
        inside = d2 <= r2
        near = np.abs(d2 - r2) <= 64 * U * r2
        if near.any():
            eL = e[near].astype(LD)
            d2L = eL[:, 0] * eL[:, 0] + eL[:, 1] * eL[:, 1] + eL[:, 2] * eL[:, 2]
            ambiguous += int(((np.abs(d2L - r2L) <= 8 * U * r2L) & (d2L != r2L)).sum())
            at_r += int((d2L == r2L).sum())
        for k in range(inside.shape[0]):
            lists[ids[a + k]] = ids[np.flatnonzero(inside[k])]
    return lists, ambiguous, at_r


def estimate(points, radius):
    """The rule by brute force -> dict(count [n] int32, cov6 [n, 6] float64, normal [n, 3] float32, normal64 [n, 3] (before the rounding),
    lam [n, 3] ascending eigenvalues of cov6, indexed [n] bool, exact [n] bool: the axis-aligned rule fixes the normal, ambiguous, at_r)"""
    P = np.asarray(points, np.float32).reshape(-1, 3)
    n = len(P)
    lists, ambiguous, at_r = neighbours(P, radius)
    count = np.array([len(v) for v in lists], np.int32)
    cov6 = np.zeros((n, 6), np.float64)
    for i in np.flatnonzero(count >= 3):
        q = P[lists[i]].astype(LD)
        a = q - q.sum(0) / LD(len(q))
        cov6[i] = [float((a[:, s] * a[:, t]).sum() / LD(len(q))) for s, t in SYM]
    lam, vec = np.linalg.eigh(sym3(cov6))
    normal64 = sign_rule(vec[:, :, 0])
    exact = (count >= 3) & (cov6[:, 1] == 0) & (cov6[:, 2] == 0) & (cov6[:, 4] == 0)
    for i in np.flatnonzero(exact):
        normal64[i] = np.eye(3)[int(np.argmin(cov6[i, [0, 3, 5]]))]      # argmin: the first among equals
    for axis, (d, o1, o2) in enumerate(((0, 1, 2), (3, 1, 4), (5, 2, 4))):   # an exactly flat neighbourhood: that axis, whatever the rest is
        flat = (count >= 3) & ~exact & (cov6[:, d] == 0) & (cov6[:, o1] == 0) & (cov6[:, o2] == 0) & (lam[:, 1] > 1e-6 * lam[:, 2])
        normal64[flat] = np.eye(3)[axis]
        exact |= flat
    few = count < 3
    normal64[few] = Z_UP
    indexed = np.isfinite(P).all(1)
    normal64[~indexed] = 0.0
    lam[few] = 0.0
    return dict(count=count, cov6=cov6, normal=normal64.astype(np.float32), normal64=normal64, lam=lam, indexed=indexed, exact=exact,
                ambiguous=ambiguous, at_r=at_r)


def estimate_fsum(points, radius, rows):
    """the same sums for a few rows through math.fsum (exactly rounded sums of the float64 terms): a check of `estimate` on itself"""
    P = np.asarray(points, np.float32).reshape(-1, 3)
    lists = neighbours(P, radius)[0]
    out = {}
    for i in rows:
        q = P[lists[i]].astype(np.float64)
        m = len(q)
        if m < 3:
            out[i] = np.zeros(6)
            continue
        mean = [math.fsum(q[:, d]) / m for d in range(3)]
        out[i] = np.array([math.fsum((q[:, s] - mean[s]) * (q[:, t] - mean[t])) / m for s, t in SYM])
    return out


def cov_tol(count, coord_max, radius):
    """per entry of cov6 (module docstring)"""
    m = np.asarray(count, np.float64)
    r = float(F(radius))
    return (4.0 * m + 16.0) * U * r * r + 2.0 * (m * U * float(coord_max)) ** 2


def normal_tols(ref, coord_max, radius):
    """-> dict(cov [n], separated [n] bool, sin [n], rayleigh [n]) from a result of `estimate` (module docstring)"""
    tc = cov_tol(ref["count"], coord_max, radius)
    lam = ref["lam"]
    l2 = lam[:, 2]
    E = 3.0 * tc + 64.0 * EPS * l2
    gap = lam[:, 1] - lam[:, 0]
    separated = (ref["count"] >= 3) & (gap >= np.maximum(1e-6 * l2, 100.0 * E)) & (gap > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        tol_sin = np.where(separated, E / (gap - E), np.inf) + 2.0 ** -24
    a = 6.0 * tc + 64.0 * EPS * l2
    return dict(cov=tc, separated=separated, sin=tol_sin, rayleigh=a + 2.0 ** -23 * np.sqrt(a * l2) + 2.0 ** -48 * l2)


# ------------------------------------------------------------------ the index's own binning, simulated in float32
def inv_h_of(cell):
    return F(1.0 / float(F(cell)))


def grid_coord(x, org, inv_h):
    """G(x) = fl(fl(x - org) * inv_h), float32 throughout (k_cell_keys)"""
    return (np.asarray(x, F) - F(org)).astype(F) * F(inv_h)


def reach_old(radius, cell):
    """normals_reach as it was: max(1, ceil(radius / h - 1e-9)) in float64 of the float32 arguments"""
    return max(1, int(math.ceil(float(F(radius)) / float(F(cell)) - 1e-9)))


def find_straddles(cell, ratio, seed, tries=400_000):
    """One-axis pairs (org, q, p), float32, with (double)p - (double)q <= (double)radius whose simulated cells lie reach_old + 1 apart
    -> (radius float32, [tries', 3] float32 rows in the order they were found)"""
    rng = np.random.default_rng(seed)
    h = F(cell)
    radius = F(F(ratio) * h)
    inv_h = inv_h_of(cell)
    org = rng.uniform(-40.0, 40.0, tries).astype(F)
    j = rng.integers(10, 60, tries).astype(F)
    q = (org + j * h).astype(F)
    q = np.nextafter(q, F(-np.inf))                                              # just below a face, by one or two steps
    q = np.where(rng.random(tries) < 0.5, q, np.nextafter(q, F(-np.inf)))
    p = (q + radius).astype(F)
    far = p.astype(np.float64) - q.astype(np.float64) > float(radius)
    p = np.where(far, np.nextafter(p, F(-np.inf)), p)
    assert (p.astype(np.float64) - q.astype(np.float64) <= float(radius)).all()
    cq, cp = np.floor(grid_coord(q, org, inv_h)), np.floor(grid_coord(p, org, inv_h))
    hit = (cp - cq == reach_old(radius, cell) + 1) & (cq >= 0)
    return radius, np.stack([org[hit], q[hit], p[hit]], 1)


# ------------------------------------------------------------------ fixtures
def _case(points, cell, radius, lattice=0, **extra):
    return dict(points=np.ascontiguousarray(points, np.float32).reshape(-1, 3), cell=float(F(cell)), radius=float(F(radius)), lattice=lattice, **extra)


STRADDLE = [(c, k) for c in (0.25, 0.3) for k in (1, 2, 3)]


def straddle_case(cell, ratio):
    """Precondition: one pair per axis whose ends are within the radius by the float64 rule and whose simulated cells lie
    reach_old + 1 apart on that axis; the origin of the grid is the anchor (the minimum on every axis), farther than the radius from
    everything else, and a cap point 70 cells up on every axis keeps every pair clear of the clamp at the upper faces; both ends have 5 companions within 0.3 radius, so their counts are >= 3 and a missed end moves cov6 by about
    radius^2 / 7."""
    rng = np.random.default_rng(int(cell * 1000) * 10 + ratio)
    found = [find_straddles(cell, ratio, 1000 * axis + int(cell * 100) + ratio) for axis in range(3)]
    radius = found[0][0]
    rows = [f[1][0] for f in found]                                              # (org, q, p) of axis 0, 1, 2
    org = np.array([r[0] for r in rows], F)
    pts, pairs = [org.copy()], []
    for axis in range(3):
        # the pair runs along `axis`; on the other axes it sits 12 + 8 axis cells above the origin: the pairs stay apart from each other
        base = (org + F(cell) * F(12 + 8 * axis)).astype(F)
        q, p = base.copy(), base.copy()
        q[axis], p[axis] = rows[axis][1], rows[axis][2]
        pairs.append((len(pts), len(pts) + 1, axis))
        pts += [q, p]
        for end, away in ((q, -1.0), (p, 1.0)):
            for _ in range(5):
                d = rng.uniform(-0.3, 0.3, 3) * float(radius)
                d[axis] = away * abs(d[axis])                                    # (outwards: a companion never lies between the two ends)
                pts.append((end.astype(np.float64) + d).astype(F))
    pts.append((org + F(cell) * F(70)).astype(F))
    return _case(np.stack(pts), cell, radius, pairs=pairs, anchor=0)


def boundary_case(radius, cell):
    """Precondition: at least 20 ordered pairs exactly at d^2 == r^2 (inside: the rule is <=) and at least 20 one float32 step farther
    on the same axis (outside); the differences and their squares are exact in float64."""
    r = F(radius)
    pts = []
    for axis in range(3):
        for k in range(8):
            # a centre near 0.5 on the lattice's own axis: from there both steps of r are exact in float32 (r is a multiple of 2^-24)
            B = np.zeros(3, F)
            c = B[axis] = F(0.5) + F(k) * F(2.0 ** -12)
            B[(axis + 1) % 3], B[(axis + 2) % 3] = F(2.0 * k + 1.0), F(2.0 * axis + 3.0)
            up, dn = F(c + r), F(c - r)
            assert float(up) - float(c) == float(r) and float(c) - float(dn) == float(r)
            for v in (c, up, dn, np.nextafter(up, F(np.inf)), np.nextafter(dn, F(-np.inf))):
                P = B.copy()
                P[axis] = v
                pts.append(P)
            for s in (1, 2):
                P = B.copy()
                P[(axis + s) % 3] += F(0.0625)
                pts.append(P)
    return _case(np.stack(pts), cell, r)


def counts_case():
    """Precondition: the counts are exactly 1, 2, 3 and 4 (an isolated point, a pair, a triple, four)"""
    rng = np.random.default_rng(5)
    pts = [np.array([3.0 * g, 0.0, 0.0]) + rng.uniform(-0.05, 0.05, (g, 3)) for g in (1, 2, 3, 4)]
    return _case(np.concatenate(pts), 0.25, 0.25, groups=(1, 2, 3, 4))


def degenerate_case():
    """Groups 3 m apart, dyadic coordinates where a result is to be exact.  Precondition: every count >= 3; `spot` (300 copies of one
    point), `line_x`, `line_y`, `line_z`, `plane_x`, `plane_y`, `plane_z` are exact rows with the answers +x, +y, +x, +x, +x, +y, +z;
    `line_d` (a diagonal) is not separated."""
    rng = np.random.default_rng(6)
    groups, pts, at = {}, [], 0

    def add(name, g):
        nonlocal at
        g = np.asarray(g, np.float64) + np.array([3.0 * len(groups), 1.0, 2.0])
        groups[name] = (at, at + len(g))
        at += len(g)
        pts.append(g)
    add("spot", np.tile([[0.375, 0.125, 0.25]], (300, 1)))
    t = np.arange(9) / 32.0
    z = np.zeros(9)
    add("line_x", np.stack([t, z, z], 1))
    add("line_y", np.stack([z, t, z], 1))
    add("line_z", np.stack([z, z, t], 1))
    add("line_d", np.stack([t, t, t], 1))
    for name, axis in (("plane_x", 0), ("plane_y", 1), ("plane_z", 2)):
        g = np.round(rng.uniform(0.0, 0.3, (40, 3)) * 1024) / 1024
        g[:, axis] = 0.125
        add(name, g)
    answers = dict(spot=0, line_x=1, line_y=0, line_z=0, plane_x=0, plane_y=1, plane_z=2)
    return _case(np.concatenate(pts), 0.25, 0.25, groups=groups, answers=answers)


def tilted_case():
    """Two dyadic planes of 5 x 5 points, 10 m apart, radius 1 m > their diameter, so that all 25 points of a plane share one
    neighbourhood and every sum is exact.  `xz`: x = z = i / 8, y = j / 8, normal +-(1, 0, -1) / sqrt 2: the first rotation the cyclic
    Jacobi takes leaves the raw vector with z < 0.  `xy`: x = y = i / 8, z = j / 8, normal +-(1, -1, 0) / sqrt 2, raw z == 0 and y < 0.
    Each branch of the sign rule flips once.  Precondition: counts 25, xy's cov6 has xz = yz = 0 exactly, both separated."""
    i, j = [v.ravel() / 8.0 for v in np.meshgrid(np.arange(-2, 3), np.arange(-2, 3), indexing="ij")]
    xz = np.stack([i, j, i], 1) + np.array([1.0, 1.0, 1.0])
    xy = np.stack([i, i, j], 1) + np.array([11.0, 1.0, 1.0])
    return _case(np.concatenate([xz, xy]), 0.25, 1.0, groups=dict(xz=(0, 25), xy=(25, 50)))


SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257)


@functools.lru_cache(None)
def patch_points():
    """257 points of a noisy plane patch, 0.6 m x 0.6 m, sigma 5 mm, tilted"""
    rng = np.random.default_rng(7)
    uv = rng.uniform(0.0, 0.6, (257, 2))
    w = rng.normal(0.0, 0.005, 257)
    e1, e2, e3 = np.array([0.8, 0.0, 0.6]), np.array([0.0, 1.0, 0.0]), np.array([-0.6, 0.0, 0.8])
    return (np.array([2.0, -1.0, 0.5]) + uv[:, :1] * e1 + uv[:, 1:] * e2 + w[:, None] * e3).astype(F)


def size_case(n):
    """Precondition: from n = 63 on at least 90 % of the counts are >= 3"""
    return _case(patch_points()[:n], 0.25, 0.25)


@functools.lru_cache(None)
def scene_points():
    """about 2000 points: a floor, a wall and a standing cylinder, sigma 5 mm along the surface normal"""
    rng = np.random.default_rng(8)
    n1, n2, n3 = 800, 700, 500
    floor = np.stack([rng.uniform(0, 4, n1), rng.uniform(0, 4, n1), rng.normal(0, 0.005, n1)], 1)
    wall = np.stack([rng.normal(0, 0.005, n2), rng.uniform(0, 4, n2), rng.uniform(0, 2.5, n2)], 1)
    a, rr = rng.uniform(0, 2 * np.pi, n3), 0.5 + rng.normal(0, 0.005, n3)
    cyl = np.stack([2.0 + rr * np.cos(a), 2.0 + rr * np.sin(a), rng.uniform(0, 2.0, n3)], 1)
    return (np.concatenate([floor, wall, cyl]) + np.array([-3.1, 5.3, 0.7])).astype(F)


def sheet_case():
    """a sheet one cell thick (z constant: dims[2] == 1), every row exact with the answer +z"""
    rng = np.random.default_rng(9)
    g = np.round(rng.uniform(0.0, 2.0, (400, 3)) * 1024) / 1024
    g[:, 2] = 0.75
    return _case(g, 0.25, 0.25, dims_one=(2,))


def rod_case():
    """a rod along x (dims[1] == dims[2] == 1), every row with count >= 3 exact with the answer +y"""
    rng = np.random.default_rng(10)
    g = np.zeros((120, 3))
    g[:, 0] = np.round(rng.uniform(0.0, 3.0, 120) * 1024) / 1024
    g[:, 1:] = (0.5, -0.25)
    return _case(g, 0.25, 0.25, dims_one=(1, 2))


def nonfinite_case():
    """the first 500 points of the scene with 12 non-finite rows scattered in (NaN, +inf, -inf in each column)"""
    P = scene_points()[:500].copy()
    rows = np.arange(12) * 41 + 3
    bad = [np.nan, np.inf, -np.inf]
    for k, i in enumerate(rows):
        P[i, k % 3] = bad[(k // 3) % 3]
    P[rows[-1]] = np.nan
    return _case(P, 0.25, 0.4, bad_rows=rows)


def scene_shift(metres):
    return (scene_points() + F(metres)).astype(F)


@functools.lru_cache(None)
def cases():
    """name -> case: dict(points [n, 3] float32, cell, radius, lattice, ...)"""
    out = {}
    for cell, k in STRADDLE:
        out["straddle_%g_%d" % (cell, k)] = straddle_case(cell, k)
    out["boundary_0.25"] = boundary_case(0.25, 0.25)
    out["boundary_0.3"] = boundary_case(0.3, 0.3)
    out["boundary_0.3_cell_0.25"] = boundary_case(0.3, 0.25)
    out["counts"] = counts_case()
    out["degenerate"] = degenerate_case()
    out["tilted"] = tilted_case()
    for n in SIZES:
        out["size_%d" % n] = size_case(n)
    out["sheet"] = sheet_case()
    out["rod"] = rod_case()
    out["whole_extent"] = _case(patch_points(), 0.25, 100.0)
    for cells in (0.1, 1.6, 2.5, 3.3):
        out["scene_%g" % cells] = _case(scene_points(), 0.25, F(cells) * F(0.25))
    out["scene_1.6_cell_0.4"] = _case(scene_points(), 0.4, F(1.6) * F(0.25))
    out["scene_1.6_lattice"] = _case(scene_points(), 0.25, F(1.6) * F(0.25), lattice=64)
    out["far_1km"] = _case(scene_shift(1000.0), 0.25, 0.4)
    out["far_3km"] = _case(scene_shift(3000.0), 0.25, 0.4)
    out["nonfinite"] = nonfinite_case()
    return out


SAME_COUNTS = (("scene_1.6", "scene_1.6_cell_0.4"), ("scene_1.6", "scene_1.6_lattice"))     # one cloud, one radius: two indexes

_REF = {}


def reference(name):
    """`estimate` of a case with its tolerances, computed once per process; nobody writes to it"""
    if name not in _REF:
        c = cases()[name]
        ref = estimate(c["points"], c["radius"])
        fin = c["points"][np.isfinite(c["points"]).all(1)]
        ref["coord_max"] = float(np.abs(fin).max()) if len(fin) else 0.0
        ref["tol"] = normal_tols(ref, ref["coord_max"], c["radius"])
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[name] = ref
    return _REF[name]


def compare(name, nrm, cnt, cov):
    """A device result (original point order) against the reference of case `name` -> dict of worst error / bound ratios
    (cov, sin, unit, rayleigh) after asserting what is exact: the counts, the rows below 3 neighbours, the rows that are not
    indexed, the sign rule and the exact rows."""
    ref = reference(name)
    tol = ref["tol"]
    n = len(ref["count"])
    assert nrm.shape == (n, 3) and cnt.shape == (n,) and cov.shape == (n, 6)
    wrong = np.flatnonzero(cnt != ref["count"])
    assert len(wrong) == 0, "%s: %d counts differ, first rows %s: device %s, rule %s" % (name, len(wrong), wrong[:6], cnt[wrong[:6]], ref["count"][wrong[:6]])
    few = ref["indexed"] & (ref["count"] < 3)
    assert (nrm[few] == Z_UP).all() and not cov[few].any()
    assert not nrm[~ref["indexed"]].any() and not cov[~ref["indexed"]].any()
    ok = ref["count"] >= 3
    worst = dict(cov=0.0, sin=0.0, unit=0.0, rayleigh=0.0)
    if not ok.any():
        return worst
    assert np.isfinite(nrm).all() and np.isfinite(cov).all()
    assert obeys_sign_rule(nrm[ok]).all()
    ex = ref["exact"]
    assert np.array_equal(nrm[ex].view(np.uint32), ref["normal"][ex].view(np.uint32)), name
    worst["cov"] = float((np.abs(cov - ref["cov6"]).max(1) / tol["cov"])[ok].max())
    n64 = nrm.astype(np.float64)
    length = np.linalg.norm(n64, axis=1)
    worst["unit"] = float(np.abs(length[ok] - 1.0).max() / 2.0 ** -24)
    unit = n64[ok] / length[ok, None]
    sep = tol["separated"][ok]
    if sep.any():
        sin = np.linalg.norm(np.cross(unit, ref["normal64"][ok]), axis=1)
        worst["sin"] = float((sin / tol["sin"][ok])[sep].max())
    loose = ~sep & ~ex[ok]
    if loose.any():
        M = sym3(ref["cov6"][ok])
        excess = np.einsum("ni,nij,nj->n", unit, M, unit) - ref["lam"][ok, 0]
        worst["rayleigh"] = float(np.maximum(excess / tol["rayleigh"][ok], 0.0)[loose].max())
    return worst
