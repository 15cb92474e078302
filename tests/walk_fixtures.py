"""Seeded clouds that sit on the edges of the grid walks (tests/test_walk_rule.py, tests/test_gpu_walk_edges.py): anchors placed on
the faces of their cells as the device's own binning expression sees them, partners one float32 coordinate step inside and outside
the radius, on narrow and on 20 000-cell-wide grids, near the origin and 65 km out.  Everything is a function of the arguments and the
seed; nothing calls the library.  Not a test module.

One geometry is (cell, offset, base, extent, lattice): two far points, offset + base and offset + base + extent, pin the bounds, so
the grid is walk_ref_np.make_geometry of them whatever else the cloud holds (asserted).  Six face points per side keep those faces
occupied for the queries from outside.

Anchors.  Per radius `anchors` of them; the coordinate of an anchor on an axis is found by bisection over the float32 coordinates
through G(x) = fl(fl(x - org) * inv_h) itself, never by c * h in float64, for one of five classes:
  ZERO   the first coordinate of its cell; where the binning has one, a coordinate with G(x) == c exactly is taken (`zero_exact`)
  TOP    the last coordinate of its cell: the next float32 bins into the cell above.  Where the coordinates are as fine as the grid
         coordinates this is G(x) == nextafter(c + 1, 0) (`top_exact`); 65 km out a 0.1 m cell holds 13 coordinates and no more
  IN_LO / IN_HI   one or two coordinates inside the lower / upper face;  HALF   the first coordinate with G(x) >= c + 0.5
Every anchor has ZERO on one axis and TOP on another.  On a corridor half of the anchors lie in the last 50 cells of the long axis.

Partners.  Per anchor one direction along an axis (both ways over the anchors; upward from a TOP or a ZERO face, downward likewise)
and one seeded diagonal.  At a radius of k whole cells every cell of every axis is scanned for a pair that straddles k + 1 faces
(straddles()); up to 24 per axis get an anchor of their own, classes TOP / HALF / HALF.  From q0 = float32(p + r u) the moving coordinate is stepped one float32 at a time to the place where
l2_simple(p, q) crosses r2: the last two q with d2 < r2 and the first two with d2 >= r2 are kept.  Where the coordinates are fine
(offset 0: `fine`) four diagonals in five are shallow -- nearly along the anchor's axis, the moving coordinate a small one, on a
corridor one of the short axes -- so that one step moves d2 by about its own spacing or less and d2 == nextafter(r2, 0) and
d2 == r2 are both reached; elsewhere one coordinate step moves d2 by 2 r ulp(x), hundreds of its spacings, and "one spacing from
the edge" can only mean one coordinate step.  A direction that leaves the box is turned round, then onto the next axis.

Queries for the device tests, no points of the cloud: fresh_queries (from the anchors along new directions), outside_queries (from
the face points straight out of the grid), face_queries (where the nearest point and the runner-up change places across a face).

Limits: at most 4 000 rows with the duplicates and the non-finite rows; no point has more than 64 neighbours within the largest
radius (tests/test_walk_rule.py asserts both)."""
import functools

import numpy as np

import walk_ref_np as W

F = np.float32
ZERO, TOP, IN_LO, IN_HI, HALF = range(5)
CUBE = (4.0, 4.0, 4.0)
CORRIDOR = (2000.0, 7.9, 1.9)          # 20 000 x 80 x 20 cells at 0.1 m: 32e6 cells, a 128 MB table

# name, cell, offset, base, extent, lattice, anchors per radius, why this one
GEOMETRIES = (
    ("cube_h010", 0.1, 0.0, 0.0, CUBE, 0, 30, "the plain case: 40 cells a side, coordinates as fine as the grid coordinates"),
    ("cube_h015", 0.15, 0.0, 0.0, CUBE, 0, 20, "1 / h is no float32 and 4 m is no whole number of cells"),
    ("cube_h015_1km", 0.15, 1000.0, 0.0, CUBE, 0, 20, "1 km out with an inexact 1 / h: 2 400 coordinates per cell, G rounds both ways"),
    ("cube_h010_1km", 0.1, 1000.0, 0.0, CUBE, 0, 30, "1 km out, 1 / h = 10 exact: the products are exact, the faces can be hit"),
    ("cube_h010_65km", 0.1, 65536.0, 0.0, CUBE, 0, 30, "65 536 m out: a 0.1 m cell is 13 float32 spacings wide"),
    ("cube_h015_65km", 0.15, 65536.0, 0.0, CUBE, 0, 20, "65 536 m out with an inexact 1 / h: 19 spacings per cell, G rounds both ways"),
    ("corridor_h010", 0.1, 0.0, 0.0, CORRIDOR, 0, 30, "20 000 cells on x: gap_eps is 7e-3 of a cell, a grid coordinate has 2^-9 spacing"),
    ("corridor_h010_lattice", 0.1, 0.0, 19.25, (2000.0, 7.85, 1.85), 64, 30, "the corridor on an origin snapped to 64 cells: org is no round number"),
    ("corridor_h025", 0.25, 0.0, 0.0, CORRIDOR, 0, 30, "h, 1 / h and k h exact: on the axes d2 == r2 ties are exact and every face can be hit"),
    ("corridor_h050", 0.5, 0.0, 0.0, CORRIDOR, 0, 20, "a 5-cell z axis under a reach of 4: the block is clamped on both sides"),
    ("corridor_h037_1km", 0.37, 1000.0, 0.0, CORRIDOR, 0, 20, "a wide grid 1 km out with an inexact 1 / h"),
)
STRADDLES = 24                          # at most so many straddle anchors per axis and whole-cell radius
RADII_CELLS = (1.0, 2.0, 3.0, 2.5, 1.0 - 1.0e-6, 1.0 + 1.0e-6)
WHOLE = (True, True, True, False, False, False)


def radii_of(cell):
    """1, 2, 3 and 2.5 cells and one cell (1 -+ 1e-6), as the doubles the library is given"""
    h = float(F(cell))
    return tuple(k * h for k in RADII_CELLS)


def _ord(x):
    """float32 -> int64 that ascends with the value, consecutive floats one apart (-0.0 and 0.0 share the 0)"""
    b = np.asarray(x, F).view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, -(b & 0x7fffffff))


def _flt(o):
    o = np.asarray(o, np.int64)
    return np.where(o >= 0, o, (-o) | 0x80000000).astype(np.uint32).view(F)


def _G1(g, axis, x):
    d = np.asarray(x, F) - g.org[axis]
    return d * g.inv_h


def first_at_least(g, axis, target, lo, hi):
    """the smallest float32 coordinate in [lo, hi] whose grid coordinate on `axis` is >= target, as an ordinal (target: array)"""
    target = np.asarray(target, F)
    a, b = np.full(target.shape, _ord(lo)), np.full(target.shape, _ord(hi))
    assert (_G1(g, axis, _flt(b)) >= target).all()
    while (a < b).any():
        mid = (a + b) // 2
        ok = _G1(g, axis, _flt(mid)) >= target
        b, a = np.where(ok, mid, b), np.where(ok, a, mid + 1)
    return a


def place(g, axis, cells, classes, steps, lo, hi):
    """coordinates (float32) on `axis` in the given cells for the given classes; steps in {1, 2} for IN_LO / IN_HI"""
    cells = np.asarray(cells, np.int64)
    first = first_at_least(g, axis, cells.astype(F), lo, hi)
    last = first_at_least(g, axis, (cells + 1).astype(F), lo, hi) - 1
    half = first_at_least(g, axis, cells.astype(F) + F(0.5), lo, hi)
    assert (last - first >= 4).all()                                   # every class has a coordinate of its own
    o = np.select([classes == ZERO, classes == TOP, classes == IN_LO, classes == IN_HI], [first, last, first + steps, last - steps], half)
    x = _flt(o)
    assert (W.grid_cell(_G1(g, axis, x), g.dim[axis]) == cells).all()
    return x


def exact_face_cells(g, axis, cells, lo, hi, cls):
    """which of `cells` hold a coordinate whose grid coordinate is the cell number itself (ZERO) or the largest float32 below the
    next cell number (TOP)"""
    cells = np.asarray(cells, np.int64)
    if cls == ZERO:
        return _G1(g, axis, _flt(first_at_least(g, axis, cells.astype(F), lo, hi))) == cells.astype(F)
    last = first_at_least(g, axis, (cells + 1).astype(F), lo, hi) - 1
    return _G1(g, axis, _flt(last)) == np.nextafter((cells + 1).astype(F), F(0.0))


def straddles(g, axis, k, radius, lo, hi):
    """The cells c of `axis` from whose last coordinate p the largest coordinate q with fl(fl(q - p)^2) < r2 is binned k + 1 cells up,
    at a radius of k cells: G(p) and G(q) round to either side of two faces k cells apart.  The reach ceil(radius / h) = k misses q."""
    cells = np.arange(1, int(g.dim[axis]) - k - 3, dtype=np.int64)
    if len(cells) == 0:
        return cells
    px = _flt(first_at_least(g, axis, (cells + 1).astype(F), lo, hi) - 1)
    r2 = W.r2_of(radius)
    o = _ord((px.astype(np.float64) + float(radius)).astype(F))
    best = np.full(len(px), -1, np.int64)
    for t in range(-3, 4):
        q = _flt(o + t)
        d = q - px
        best = np.where((d * d < r2) & (q <= hi), o + t, best)
    cq = W.grid_cell(_G1(g, axis, _flt(np.maximum(best, 0))), g.dim[axis])
    return cells[(best >= 0) & (cq - W.grid_cell(_G1(g, axis, px), g.dim[axis]) == k + 1)]


def partners(p, u, mv, radius, lo, hi, window=4096):
    """p float32 [s, 3], u float64 [s, 3] unit directions, mv int [s] the moving axis -> (q float32 [s, 4, 3], ok bool [s]): the two
    last accepted and the two first rejected places of the moving coordinate, inside out; ok: found, and all four inside [lo, hi]"""
    p = np.asarray(p, F).reshape(-1, 3)
    s = len(p)
    rows = np.arange(s)
    r2 = W.r2_of(radius)
    q0 = (p.astype(np.float64) + float(radius) * np.asarray(u, np.float64)).astype(F)
    o0, op = _ord(q0[rows, mv]), _ord(p[rows, mv])
    out = np.where(o0 != op, np.sign(o0 - op), np.where(np.asarray(u)[rows, mv] < 0, -1, 1)).astype(np.int64)   # the way that leads away from p

    def d2_at(t):
        q = q0.copy()
        q[rows, mv] = _flt(o0 + t * out)
        return W.l2_simple(p, q), q

    a = -np.minimum(window, np.abs(o0 - op))                           # inward no further than p's own coordinate
    b = np.full(s, window, np.int64)
    ok = (d2_at(a)[0] < r2) & (d2_at(b)[0] >= r2) & (a <= -2)
    a, b = np.where(ok, a, 0), np.where(ok, b, 0)
    while (a < b).any():
        mid = np.floor_divide(a + b, 2)
        hit = d2_at(mid)[0] >= r2
        b, a = np.where(hit, mid, b), np.where(hit, a, mid + 1)
    q = np.stack([d2_at(a + t)[1] for t in (-2, -1, 0, 1)], 1)
    d2 = np.stack([W.l2_simple(p, q[:, t]) for t in range(4)], 1)
    ok &= (d2[:, 0] < r2) & (d2[:, 1] < r2) & (d2[:, 2] >= r2) & (d2[:, 3] >= r2)
    ok &= ((q >= np.asarray(lo, F)) & (q <= np.asarray(hi, F))).all((1, 2))
    return q, ok


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _anchor_cells(rng, g, n, long_tail):
    """cells [n, 3] anywhere but in the outermost layers; long_tail: half of them in the last 50 cells of axis 0"""
    c = np.empty((n, 3), np.int64)
    for a in range(3):
        top = int(g.dim[a]) - 2                                         # (the last cell is clamped into: the far point's own)
        mrg = min(1, max(top // 2 - 1, 0))
        c[:, a] = rng.integers(mrg, top - mrg + 1, n)
    if long_tail:
        tail = np.arange(n) % 2 == 1
        c[tail, 0] = rng.integers(int(g.dim[0]) - 51, int(g.dim[0]) - 1, int(tail.sum()))
    return c


def build(cell, offset, base, extent, lattice, anchors, seed):
    """-> dict(points float32 [n, 3], geometry, radii, lo, hi, anchors=[per radius dict(p, cls, cells, zero_exact, top_exact)],
    sets=[per radius dict(p, q [s, 4, 3], anchor, shallow)], face float32 [36, 3], fine bool)"""
    rng = np.random.default_rng(seed)
    lo = np.full(3, F(F(offset) + F(base)), F)
    hi = (lo.astype(np.float64) + np.asarray(extent, np.float64)).astype(F)
    g = W.make_geometry(lo, hi, cell, lattice)
    fine = offset == 0.0 and base == 0.0
    radii = radii_of(cell)
    long_tail = extent[0] > 100.0
    others = np.array([IN_LO, IN_HI, HALF])
    rows, per_radius, sets = [lo[None], hi[None]], [], []
    for ri, radius in enumerate(radii):
        n = anchors
        k = np.arange(n)
        axis, up = (k % 6) // 2, (k % 6) % 2 == 0                        # the partner's axis and way
        on_axis = np.where(up == ((k // 6) % 2 == 0), TOP, ZERO)           # upward from a TOP face, downward from a ZERO face; every other round reversed
        cls = np.empty((n, 3), np.int64)
        cls[k, axis] = on_axis
        cls[k, (axis + 1) % 3] = np.where(on_axis == TOP, ZERO, TOP)
        cls[k, (axis + 2) % 3] = others[rng.integers(0, 3, n)]
        cells = _anchor_cells(rng, g, n, long_tail)
        p = np.empty((n, 3), F)
        for a in range(3):
            for i in np.flatnonzero((cls[:, a] == ZERO) | (cls[:, a] == TOP)):   # to a cell whose face the binning can hit, if its neighbourhood has one
                near = np.arange(max(cells[i, a] - 8, 1), min(cells[i, a] + 9, int(g.dim[a]) - 1))
                hit = near[exact_face_cells(g, a, near, lo[a], hi[a], cls[i, a])]
                if len(hit):
                    cells[i, a] = hit[np.argmin(np.abs(hit - cells[i, a]))]
            p[:, a] = place(g, a, cells[:, a], cls[:, a], rng.integers(1, 3, n), lo[a], hi[a])
        gp = W.G(g, p)
        zero_exact = ((cls == ZERO) & (gp == cells.astype(F))).any(1)
        top_exact = ((cls == TOP) & (gp == np.nextafter((cells + 1).astype(F), F(0.0)))).any(1)
        per_radius.append(dict(p=p, cls=cls, cells=cells, zero_exact=zero_exact, top_exact=top_exact))
        # directions: the axis one, and a diagonal
        u_axis = np.zeros((n, 3))
        u_axis[k, axis] = np.where(up, 1.0, -1.0)
        shallow = fine & (k % 5 != 0)
        small = (axis + 1 + rng.integers(0, 2, n)) % 3
        if long_tail:
            small = np.where(axis == 2, 1, 2)                              # on a corridor the moving coordinate is a short axis: fine steps
        u_sh = u_axis.copy()
        u_sh[k, small] = rng.uniform(0.002, 0.02, n) * rng.choice([-1.0, 1.0], n)
        u_sh[k, 3 - axis - small] = rng.uniform(-0.005, 0.005, n)
        u_gen = rng.normal(size=(n, 3))
        u_diag = _unit(np.where(shallow[:, None], u_sh, u_gen))
        mv_diag = np.where(shallow, small, np.abs(u_diag).argmax(1))
        P, Q, A, SH = [], [], [], []
        for u, mv, sh in ((u_axis, axis, np.zeros(n, bool)), (u_diag, mv_diag, shallow)):
            q, ok = partners(p, u, mv, radius, lo, hi)
            ur, mr = np.roll(u, 1, axis=1), (mv + 1) % 3
            for u2, mv2 in ((-u, mv), (ur, mr), (-ur, mr)):              # where it leaves the box: the other way, then the next axis both ways
                q2, ok2 = partners(p, u2, mv2, radius, lo, hi)
                use2 = ~ok & ok2
                q[use2], ok = q2[use2], ok | ok2
            P.append(p[ok])
            Q.append(q[ok])
            A.append(k[ok])
            SH.append(sh[ok])
        if WHOLE[ri]:                                                    # anchors of their own where a pair straddles k + 1 faces
            for a in range(3):
                hit = straddles(g, a, ri + 1, radius, lo[a], hi[a])
                hit = hit[rng.permutation(len(hit))[:STRADDLES]]
                if not len(hit):
                    continue
                m = len(hit)
                sc, scl = _anchor_cells(rng, g, m, False), np.full((m, 3), HALF, np.int64)
                sc[:, a], scl[:, a] = hit, TOP
                sp = np.stack([place(g, b, sc[:, b], scl[:, b], np.ones(m, np.int64), lo[b], hi[b]) for b in range(3)], 1)
                su = np.zeros((m, 3))
                su[:, a] = 1.0
                q, ok = partners(sp, su, np.full(m, a), radius, lo, hi)
                P.append(sp[ok])
                Q.append(q[ok])
                A.append(np.full(int(ok.sum()), -1))                      # (no anchor of the regular ones)
                SH.append(np.zeros(int(ok.sum()), bool))
                rows.append(sp[ok])
        st = dict(p=np.concatenate(P), q=np.concatenate(Q), anchor=np.concatenate(A), shallow=np.concatenate(SH))
        sets.append(st)
        rows += [p, st["q"].reshape(-1, 3)]
    face = rng.uniform(0.0, 1.0, (6, 6, 3)) * (hi.astype(np.float64) - lo) + lo
    face = face.astype(F)
    for a in range(3):
        face[2 * a, :, a], face[2 * a + 1, :, a] = lo[a], hi[a]
    face = np.clip(face.reshape(-1, 3), lo, hi)
    rows.append(face)
    rows.append(np.concatenate([per_radius[ri]["p"][:2] for ri in range(len(radii))]))     # exact duplicates of a few anchors
    x = np.concatenate(rows).astype(F)
    x = x[rng.permutation(len(x))]
    bad = np.array([[np.nan, lo[1], lo[2]], [lo[0], np.inf, lo[2]], [lo[0], lo[1], -np.inf], [np.nan, np.nan, np.nan]], F)
    at = np.sort(rng.integers(0, len(x), len(bad)))
    x = np.insert(x, at, bad, axis=0)
    g2 = W.geometry(x, cell, lattice)
    assert np.array_equal(g2.org, g.org) and np.array_equal(g2.dim, g.dim) and g2.gap_eps == g.gap_eps and g2.inv_h == g.inv_h, (g, g2)
    x.setflags(write=False)
    return dict(points=x, geometry=g, radii=radii, lo=lo, hi=hi, anchors=per_radius, sets=sets, face=face, fine=fine)


def fresh_queries(f, ri, seed=7):
    """Queries that are no points of the cloud: from every anchor of radius `ri` along a new seeded direction, the two last places
    inside and the two first outside of that radius -> float32 [s * 4, 3]"""
    rng = np.random.default_rng(seed + ri)
    p = f["anchors"][ri]["p"]
    u = _unit(rng.normal(size=(len(p), 3)))
    q, ok = partners(p, u, np.abs(u).argmax(1), f["radii"][ri], f["lo"], f["hi"])
    return q[ok].reshape(-1, 3)


def outside_queries(f, ri):
    """From the six points on every face of the bounding box straight outward: the two last places inside the radius and the two
    first outside it, every one of them beyond the grid on that axis -> float32 [s * 4, 3]"""
    face = f["face"]
    u = np.zeros((len(face), 3))
    axis = np.repeat(np.arange(3), 12)
    u[np.arange(len(face)), axis] = np.tile(np.repeat([-1.0, 1.0], 6), 3)
    q, ok = partners(face, u, axis, f["radii"][ri], np.full(3, -np.inf, F), np.full(3, np.inf, F))
    assert ok.all()
    q = q.reshape(-1, 3)
    a = np.repeat(axis, 4)
    rows = np.arange(len(q))
    assert ((q[rows, a] < f["lo"][a]) | (q[rows, a] > f["hi"][a])).all()
    return q


def face_queries(f, ri):
    """Queries on the segment from an anchor p to its axis partner q (the last one inside the radius), at the two places either side
    of where l2_simple(x, q) falls below l2_simple(x, p): the nearest point and the runner-up change places within one float32
    step, and where p and q lie in different cells one of the two is across a face from the query -> float32 [s * 2, 3]"""
    st = f["sets"][ri]
    p, q = st["p"], st["q"][:, 1]
    axial = ((p != q).sum(1) == 1)
    p, q = p[axial], q[axial]
    rows = np.arange(len(p))
    mv = (p != q).argmax(1)
    op, oq = _ord(p[rows, mv]), _ord(q[rows, mv])
    way = np.sign(oq - op)

    def nearer_q(t):
        x = p.copy()
        x[rows, mv] = _flt(op + way * t)
        return W.l2_simple(x, q) < W.l2_simple(x, p), x

    a, b = np.zeros(len(p), np.int64), np.abs(oq - op)
    while (a < b).any():
        mid = (a + b) // 2
        hit = nearer_q(mid)[0]
        b, a = np.where(hit, mid, b), np.where(hit, a, mid + 1)
    return np.concatenate([nearer_q(a)[1], nearer_q(a - 1)[1]])


@functools.lru_cache(maxsize=None)
def fixture(name):
    """build() of one geometry, once per process (do not modify the result)"""
    for i, (nm, cell, offset, base, extent, lattice, anchors, _) in enumerate(GEOMETRIES):
        if nm == name:
            f = build(cell, offset, base, extent, lattice, anchors, 1000 + i)
            f.update(name=name, cell=cell, lattice=lattice, corridor=extent[0] > 100.0)
            return f
    raise KeyError(name)


NAMES = tuple(g[0] for g in GEOMETRIES)
CUBES = tuple(g[0] for g in GEOMETRIES if g[4] == CUBE)
CORRIDORS = tuple(g[0] for g in GEOMETRIES if g[4] != CUBE)


def cases():
    """[(name, points, cell, lattice, radii)] for tests/test_walk_rule.py and tests/test_gpu_walk_edges.py"""
    out = []
    for name in NAMES:
        f = fixture(name)
        out.append((name, f["points"], f["cell"], f["lattice"], f["radii"]))
    return out
