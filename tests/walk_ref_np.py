"""The geometry every fixed-radius walk of the grid index rests on, restated in float32 numpy from the text of sf_map_build (step 2)
and the comments of sf_nn.hpp / sf_walk.hpp: how a point is binned, how far the block of cells around it reaches, and which cells
of that block radius_walk / radius_runs enter.  Every operation is rounded on its own (the library is built without contraction).
tests/test_walk_rule.py holds it to hand-worked values and proves on the clouds of tests/walk_fixtures.py that the rule as written
loses no accepted pair while its weakened forms do; tests/test_gpu_walk_edges.py ties it to the index the kernels walk.  Nothing here
calls the library.  Not a test module.

    h      = float32(cell);  org = the smallest finite coordinate per axis, or float32(floor(mn / (lattice h)) lattice h)
    dim    = floor((mx - org) / h) + 1 in float64;  inv_h = float32(1 / h)
    gap_eps = ((1.5f * 2.384186e-7f) * float(maxdim)) * float(h)
    G(x)   = fl(fl(x - org) * inv_h);  cell = int(min(max(floor(G), 0), float(dim - 1)))
    reach  = ceil((sqrt(r2) (1 + 1e-6) + gap_eps) inv_h) in float64
    a row (y, z) of the block is entered when  (ry ry + rz rz) * 0.998f < r2,  rz alone first, and a cell x of it when it is the
    point's own column or ((ry ry + rz rz) + rx rx) * 0.998f < r2, with r = max(cell_gap * h - gap_eps, 0) per axis.
"""
import numpy as np

from cluster_ref_np import l2_simple, r2_of  # noqa: F401  (re-exported: the rule's distance and the float32 square of a radius)

F = np.float32
FACTOR = F(0.998)
EPS_UNIT = F(1.5) * F(2.384186e-7)          # the compiler folds the two literals in float32


class Geometry:
    """h, org [3], dim [3], inv_h, gap_eps of one build; h, inv_h and gap_eps are float32 scalars, org float32, dim int64"""

    def __init__(self, h, org, dim, inv_h, gap_eps):
        self.h, self.org, self.dim, self.inv_h, self.gap_eps = F(h), np.asarray(org, F), np.asarray(dim, np.int64), F(inv_h), F(gap_eps)

    def __repr__(self):
        return "Geometry(h=%r, org=%r, dim=%r, inv_h=%r, gap_eps=%r)" % (self.h, self.org.tolist(), self.dim.tolist(), self.inv_h, self.gap_eps)


def grid_origin(mn, h, lattice):
    """float32 mn [3], float64 h -> float32 [3]: mn itself, or mn snapped down to a multiple of `lattice` cells"""
    mn = np.asarray(mn, F)
    if lattice <= 0:
        return mn.copy()
    step = np.float64(lattice) * np.float64(h)
    return (np.floor(mn.astype(np.float64) / step) * step).astype(F)


def make_geometry(mn, mx, cell, lattice=0):
    """the geometry of an explicit cell over the finite bounds mn, mx (float32 [3])"""
    h = np.float64(F(cell))
    assert h > 0
    org = grid_origin(mn, h, lattice)
    dim = (np.floor((np.asarray(mx, F).astype(np.float64) - org.astype(np.float64)) / h) + 1).astype(np.int64)
    gap_eps = (EPS_UNIT * F(dim.max())) * F(h)
    return Geometry(F(h), org, dim, F(np.float64(1.0) / h), gap_eps)


def geometry(points, cell, lattice=0):
    """the geometry sf_map_build gives the finite rows of `points` at an explicit cell"""
    x = np.asarray(points, F).reshape(-1, 3)
    x = x[np.isfinite(x).all(1)]
    assert len(x)
    return make_geometry(x.min(0), x.max(0), cell, lattice)


def G(g, x):
    """float32 [..., 3] -> the grid coordinates the device bins by"""
    x = np.asarray(x, F)
    with np.errstate(over="ignore", invalid="ignore"):
        d = x - g.org
        assert d.dtype == F
        return d * g.inv_h


def grid_cell(gc, n):
    """int64 cells of grid coordinates gc on axes of n cells (n scalar or [3]): clamped in float32 before the conversion"""
    gc = np.asarray(gc, F)
    top = (np.asarray(n, np.int64) - 1).astype(F)
    with np.errstate(invalid="ignore"):                                  # (a NaN row is never binned; its cell here means nothing)
        return np.minimum(np.maximum(np.floor(gc), F(0.0)), top).astype(np.int64)


def cell(g, gc):
    return grid_cell(gc, g.dim)


def cell_gap(gc, c, cq):
    """distance in cells (float32, >= 0) from grid coordinate gc, binned in cell cq, to the cell interval [c, c + 1]"""
    gc, c, cq = np.asarray(gc, F), np.asarray(c, np.int64), np.asarray(cq, np.int64)
    below = gc - (c + 1).astype(F)
    above = c.astype(F) - gc
    d = np.where(c < cq, below, above).astype(F)
    return np.where((c == cq) | ~(d > 0), F(0.0), d).astype(F)


def safe_gap(gap, eps):
    return np.maximum(np.asarray(gap, F) - F(eps), F(0.0)).astype(F)


def reach(g, r2, formula="full", radius=None):
    """the R of the host.  "full": radius_reach / feature_reach as written, from r2 alone; "naive": ceil(radius / h) of the radius as
    it was given (sqrt(r2) without one), what the normals once used"""
    r = np.sqrt(np.float64(F(r2)))
    if formula == "naive":
        return int(max(np.ceil((r if radius is None else np.float64(radius)) / np.float64(g.h)), 1.0))
    assert formula == "full", formula
    return int(min(max(np.ceil((r * (1.0 + 1.0e-6) + np.float64(g.gap_eps)) * np.float64(g.inv_h)), 1.0), float(g.dim.max())))


def _passes(g2, r2, factor):
    return (g2 * F(factor)).astype(F) < F(r2)


def walk_visits(g, p, q_cell, r2, slack=True, factor=FACTOR, formula="full", radius=None):
    """p float32 [m, 3], q_cell int64 [m, 3] (cells of the grid) -> bool [m]: radius_walk from p enters that cell.
    slack False: gap_eps taken as 0; factor: what stands in place of 0.998f; formula, radius: reach()'s."""
    p = np.asarray(p, F).reshape(-1, 3)
    qc = np.asarray(q_cell, np.int64).reshape(-1, 3)
    gp = G(g, p)
    cp = cell(g, gp)
    R = reach(g, r2, formula, radius)
    ge = g.gap_eps if slack else F(0.0)
    in_block = (np.abs(qc - cp) <= R).all(1)
    r = [safe_gap(cell_gap(gp[:, a], qc[:, a], cp[:, a]) * g.h, ge) for a in range(3)]
    rz2 = r[2] * r[2]
    z_ok = _passes(rz2, r2, factor)
    g2 = r[1] * r[1] + rz2
    assert g2.dtype == F
    row_ok = _passes(g2, r2, factor)
    x_ok = (qc[:, 0] == cp[:, 0]) | _passes(g2 + r[0] * r[0], r2, factor)
    return in_block & z_ok & row_ok & x_ok


def accepted_pairs(points, r2, chunk=512):
    """(i, j, d2) of every ordered pair i != j of finite rows of `points` (original row numbers) with l2_simple < r2, strict"""
    x = np.asarray(points, F).reshape(-1, 3)
    ids = np.flatnonzero(np.isfinite(x).all(1))
    P = np.ascontiguousarray(x[ids])
    I, J, D = [], [], []
    for s in range(0, len(P), chunk):
        c = P[s:s + chunk]
        dx, dy, dz = (c[:, None, a] - P[None, :, a] for a in range(3))
        d = ((dx * dx) + dy * dy) + dz * dz
        assert d.dtype == F
        i, j = np.nonzero(d < F(r2))
        keep = (i + s) != j
        I.append(ids[i[keep] + s])
        J.append(ids[j[keep]])
        D.append(d[i[keep], j[keep]])
    return np.concatenate(I), np.concatenate(J), np.concatenate(D)


def lost_pairs(g, points, r2, **weaken):
    """-> (the number of accepted ordered pairs (i, j) whose cell of j the walk from i does not enter, the number of pairs)"""
    x = np.asarray(points, F).reshape(-1, 3)
    i, j, _ = accepted_pairs(x, r2)
    seen = walk_visits(g, x[i], cell(g, G(g, x[j])), r2, **weaken)
    return int((~seen).sum()), len(i)
