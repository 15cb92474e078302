"""The argument above radius_walk (sf_walk.hpp, steps (a) - (d)), held to account on this CPU: the float32 restatement of the
binning and the pruning (tests/walk_ref_np.py) loses no accepted pair on the edge clouds of tests/walk_fixtures.py, its weakened forms
do, the clouds sit where they claim to sit, and the restatement gives the values worked out by hand from the library's text.

What "the edge is there" counts, per case and radius (each at least 20 unless said otherwise):
  steps     ordered pairs one float32 coordinate step inside the radius (the next step outward is rejected), and one step outside
  faces     anchors that are the first / the last float32 coordinate of their cell on some axis, by the binning expression itself
  cells     accepted pairs whose cells differ by two or more on an axis, at the radii of two cells and more, and at (1 + 1e-6)
            cells where the coordinates can tell that radius from one cell (offset 0).  At a radius of one cell or less such a
            pair needs G(q) - G(p) > 1 from |q - p| < h: it exists only where the roundings of (b) put p and q on either side of
            two faces, which is the pair the reach ceil(radius / h) loses.  The count is printed there, and
            test_the_fixtures_have_teeth asserts that such pairs exist at whole-cell radii.
  on the cases with fine coordinates (offset 0, walk_fixtures `fine`) also, to the bit:
  d2        pairs with d2 == nextafter(r2, 0) and pairs with d2 == r2
  exact     anchors with G(p) == c and with G(p) == nextafter(c + 1, 0) on some axis
  Elsewhere these cannot be had: one coordinate step moves d2 by 2 r ulp(x) -- 65 km out, 1e-3 m^2 against a spacing of 1e-9 --,
  and a cell holds 13 coordinates, none of which need land on an integer."""
import numpy as np
import pytest

import walk_fixtures as fx
import walk_ref_np as W

F = np.float32
WEAK = dict(none=dict(slack=False, factor=1.0), no_gap_eps=dict(slack=False), no_factor=dict(factor=1.0))


@pytest.fixture(scope="module")
def tallies():
    """per case and radius: the accepted pairs and what each form of the rule loses of them, computed once"""
    out = {}
    for name in fx.NAMES:
        f = fx.fixture(name)
        g, x = f["geometry"], f["points"]
        cells = W.cell(g, W.G(g, x))
        rows = []
        for radius in f["radii"]:
            r2 = W.r2_of(radius)
            i, j, d2 = W.accepted_pairs(x, r2)
            lost = {"written": int((~W.walk_visits(g, x[i], cells[j], r2)).sum()),
                    "naive_reach": int((~W.walk_visits(g, x[i], cells[j], r2, formula="naive", radius=radius)).sum())}
            for key, kw in WEAK.items():
                lost[key] = int((~W.walk_visits(g, x[i], cells[j], r2, **kw)).sum())
            rows.append(dict(radius=radius, r2=r2, i=i, j=j, d2=d2, lost=lost))
        out[name] = rows
    return out


# ------------------------------------------------------------------ 1. nothing lost
@pytest.mark.parametrize("name", fx.NAMES)
def test_nothing_lost(tallies, name):
    for row in tallies[name]:
        assert len(row["i"]) > 1000
        assert row["lost"]["written"] == 0, (name, row["radius"], row["lost"])


# ------------------------------------------------------------------ 2. the fixtures have teeth
def test_the_fixtures_have_teeth(tallies):
    total = {key: {"cube": 0, "corridor": 0} for key in ("none", "no_gap_eps", "no_factor")}
    naive_whole, pairs = 0, 0
    for name in fx.NAMES:
        kind = "corridor" if fx.fixture(name)["corridor"] else "cube"
        for ri, row in enumerate(tallies[name]):
            pairs += len(row["i"])
            for key in total:
                total[key][kind] += row["lost"][key]
            if fx.WHOLE[ri]:
                naive_whole += row["lost"]["naive_reach"]
    print("accepted ordered pairs: %d" % pairs)
    print("lost with no slack at all (gap_eps = 0, factor 1): cubes %d, corridors %d" % (total["none"]["cube"], total["none"]["corridor"]))
    print("lost with reach = ceil(radius / h) at whole-cell radii: %d" % naive_whole)
    print("lost with gap_eps = 0 alone: cubes %d, corridors %d (nothing asserted)" % (total["no_gap_eps"]["cube"], total["no_gap_eps"]["corridor"]))
    print("lost with the factor 1 alone: cubes %d, corridors %d (nothing asserted)" % (total["no_factor"]["cube"], total["no_factor"]["corridor"]))
    assert total["none"]["cube"] >= 1 and total["none"]["corridor"] >= 1
    assert naive_whole >= 1


# ------------------------------------------------------------------ 3. the edge is there
def _step(x, axis, way):
    y = np.array(x, F)
    y[:, axis] = np.nextafter(y[:, axis], F(way * np.inf))
    return y


@pytest.mark.parametrize("name", fx.NAMES)
def test_the_edge_is_there(tallies, name):
    f = fx.fixture(name)
    g, x = f["geometry"], f["points"]
    finite = np.isfinite(x).all(1)
    assert len(x) <= 4000 and 3 <= (~finite).sum() <= 8
    assert len(x) - len(np.unique(x[finite], axis=0)) - (~finite).sum() >= 6                    # exact duplicates
    have = {row.tobytes() for row in x[finite]}
    cells = W.cell(g, W.G(g, x))
    big = max(f["radii"])
    i, _, _ = W.accepted_pairs(x, W.r2_of(big))
    most = int(np.bincount(i).max()) + 1                                                      # the point itself is in its row
    assert most <= 64, most
    for ri, row in enumerate(tallies[name]):
        radius, r2, st, an = row["radius"], row["r2"], f["sets"][ri], f["anchors"][ri]
        # steps: the kept partners are in the cloud, ascend outward one coordinate step at a time and cross r2 in the middle
        p, q = st["p"], st["q"]
        assert all(v.tobytes() in have for v in p) and all(v.tobytes() in have for v in q.reshape(-1, 3))
        d2 = np.stack([W.l2_simple(p, q[:, t]) for t in range(4)], 1)
        assert (d2[:, :2] < r2).all() and (d2[:, 2:] >= r2).all()
        moved = (q[:, 1:] != q[:, :-1])
        assert (moved.sum(2) == 1).all()                                                       # one coordinate ...
        o = q.view(np.uint32).astype(np.int64)
        assert (np.abs(o[:, 1:] - o[:, :-1]).sum(2) == 1).all()                                # ... one spacing
        n_inside, n_outside = 2 * len(p), 2 * len(p)                                           # both directions of (p, q1) and of (p, q2)
        # faces, by the binning itself
        pa = an["p"]
        ca = W.cell(g, W.G(g, pa))
        first = np.zeros(len(pa), bool)
        last = np.zeros(len(pa), bool)
        for a in range(3):
            first |= W.cell(g, W.G(g, _step(pa, a, -1)))[:, a] < ca[:, a]
            last |= W.cell(g, W.G(g, _step(pa, a, +1)))[:, a] > ca[:, a]
        # cells
        far = int((np.abs(cells[row["i"]] - cells[row["j"]]).max(1) >= 2).sum())
        counts = dict(inside=n_inside, outside=n_outside, first=int(first.sum()), last=int(last.sum()), far=far)
        if f["fine"]:
            gp = W.G(g, pa)
            counts.update(below=int((row["d2"] == np.nextafter(r2, F(0.0))).sum()), equal=_equal_pairs(x[finite], r2),
                          zero_exact=int((gp == ca.astype(F)).any(1).sum()), top_exact=int((gp == np.nextafter((ca + 1).astype(F), F(0.0))).any(1).sum()))
        print(name, "radius %.9g" % radius, counts)
        room = fx.RADII_CELLS[ri] >= 2.0 or (f["fine"] and fx.RADII_CELLS[ri] > 1.0)
        for key, v in counts.items():
            if key == "far" and not room:
                continue
            assert v >= 20, (name, radius, key, v)


def _equal_pairs(P, r2):
    n = 0
    for s in range(0, len(P), 512):
        c = P[s:s + 512]
        dx, dy, dz = (c[:, None, a] - P[None, :, a] for a in range(3))
        n += int((((dx * dx) + dy * dy) + dz * dz == r2).sum())
    return n


def test_the_cases_are_what_the_issue_lists():
    cs = fx.cases()
    assert [c[0] for c in cs] == list(fx.NAMES) and 10 <= len(cs) <= 14
    cells = {c[2] for c in cs}
    assert cells == {0.1, 0.15, 0.37, 0.25, 0.5}
    assert {g[2] for g in fx.GEOMETRIES} == {0.0, 1000.0, 65536.0}
    assert any(c[3] == 64 for c in cs)
    for name, pts, cell, lattice, radii in cs:
        h = float(F(cell))
        assert radii == (h, 2 * h, 3 * h, 2.5 * h, h * (1 - 1e-6), h * (1 + 1e-6))
        g = W.geometry(pts, cell, lattice)
        assert int(np.prod(g.dim)) * 4 <= 128_100_000, (name, g)                                 # the table: 128 MB at most
        if name.startswith("corridor_h010"):
            assert g.dim.max() >= 20_000
    f = fx.fixture("cube_h010_65km")                                                            # 65 km out a 0.1 m cell is about 13 float32 spacings
    assert 12 <= F(0.1) / np.spacing(F(65537.0)) <= 13
    assert np.array_equal(fx.build(0.1, 65536.0, 0.0, fx.CUBE, 0, 30, 1000 + fx.NAMES.index("cube_h010_65km"))["points"], f["points"], equal_nan=True)


# ------------------------------------------------------------------ 4. the model is the library's text
def test_grid_cell_by_hand():
    gc = np.array([-0.5, -1e30, 0.0, 0.99999994, 3.0, 9.999999, 10.0, 12.3, 3e38, np.inf, -np.inf], F)
    assert W.grid_cell(gc, 10).tolist() == [0, 0, 0, 0, 3, 9, 9, 9, 9, 9, 0]
    assert W.grid_cell(F(7.0), 1) == 0
    # the clamp is a float32: (float)(n - 1) for n - 1 = 2^24 + 3 is 2^24 + 4 = n, a cell beyond the grid -- why an axis holds 2^24 cells at most
    n = 2 ** 24 + 4
    assert W.grid_cell(F(3e7), n) == n and W.grid_cell(F(3e7), 2 ** 24) == 2 ** 24 - 1


@pytest.mark.parametrize("cell,org,mx,dim", [(0.1, 0.0, 0.5, 5), (0.15, 0.0, 0.75, 5), (0.37, 0.0, 1.8499999, 5), (0.25, 0.12360742, 0.8736074, 3),
                                             (0.5, 0.09484708, 2.594847, 5)])
def test_the_largest_coordinate_rounds_up_to_dim_and_is_clamped(cell, org, mx, dim):
    org, mx = F(org), F(mx)
    g = W.make_geometry(np.full(3, org), np.full(3, mx), cell)
    assert g.dim.tolist() == [dim] * 3                                                          # floor((mx - org) / h) + 1 in float64: mx lies below the face
    assert (np.float64(mx) - np.float64(org)) / np.float64(g.h) < dim
    gc = W.G(g, np.full(3, mx))
    assert (gc == F(dim)).all()                                                                 # ... and its float32 grid coordinate on it
    assert W.cell(g, gc).tolist() == [dim - 1] * 3


def test_cell_gap_and_safe_gap_by_hand():
    assert W.cell_gap(F(5.25), 5, 5) == 0.0
    assert W.cell_gap(F(5.25), 3, 5) == 1.25 and W.cell_gap(F(5.25), 4, 5) == 0.25                # to the upper face of a cell below
    assert W.cell_gap(F(5.25), 7, 5) == 1.75 and W.cell_gap(F(5.25), 6, 5) == 0.75                # to the lower face of a cell above
    assert W.cell_gap(F(5.0), 4, 5) == 0.0                                                      # on the face
    assert W.cell_gap(F(4.75), 4, 5) == 0.0 and W.cell_gap(F(6.5), 6, 5) == 0.0                 # a clamped query: never negative
    assert W.cell_gap(F(20000.998), 20002, 20000) == F(20002.0) - F(20000.998)                   # float32 throughout: 2^-9 spacing out there
    assert W.safe_gap(F(0.5), F(0.125)) == 0.375 and W.safe_gap(F(0.05), F(0.1)) == 0.0 and W.safe_gap(F(0.1), F(0.1)) == 0.0
    assert W.safe_gap(F(0.3), F(1e-9)) == F(0.3)                                                # a slack below half a spacing changes nothing


def test_geometry_and_reach_by_hand():
    g = W.make_geometry(np.zeros(3, F), np.array([4, 2, 1], F), 0.25)
    assert g.dim.tolist() == [17, 9, 5] and g.inv_h == 4.0 and g.h == 0.25
    unit = F(2.384186e-7)
    assert unit == np.nextafter(F(2.0 ** -22), F(1.0))                                          # the literal is one spacing above 2^-22
    assert g.gap_eps == F(F(F(1.5) * unit) * F(17.0)) * F(0.25)
    assert abs(float(g.gap_eps) - 1.5 * 2.0 ** -22 * 17 * 0.25) < 1e-12
    # ceil((r (1 + 1e-6) + gap_eps) * 4): two cells exactly -> 3, and it stays 3 up to just under three cells
    assert W.reach(g, W.r2_of(0.5)) == 3 and W.reach(g, W.r2_of(0.5), "naive", 0.5) == 2
    assert W.reach(g, W.r2_of(0.49)) == 2 and W.reach(g, W.r2_of(0.7499)) == 3 and W.reach(g, W.r2_of(0.75)) == 4
    assert W.reach(g, W.r2_of(1e-4)) == 1 and W.reach(g, W.r2_of(100.0)) == 17                   # at least one ring, at most the grid
    # a snapped origin: the multiple of 64 cells below the smallest coordinate, rounded to float32
    g = W.make_geometry(np.full(3, F(19.25)), np.full(3, F(30.0)), 0.1, 64)
    step = 64 * float(F(0.1))
    assert g.org.tolist() == [float(F(3 * step))] * 3 and g.org[0] < 19.25
    assert g.dim.tolist() == [int(np.floor((30.0 - float(F(3 * step))) / float(F(0.1))) + 1)] * 3 == [108] * 3
    assert g.inv_h == 10.0                                                                      # float32(1 / 0.100000001490116)
    g = W.make_geometry(np.zeros(3, F), np.ones(3, F), 0.15)
    assert g.inv_h == F(1.0 / float(F(0.15))) == F(6.6666665) and float(g.inv_h) * float(F(0.15)) != 1.0   # 1 / h is no float32


def test_walk_visits_by_hand():
    """h = 0.25 on a 17 x 9 x 5 grid, p at grid coordinates (8.5, 4.5, 2.5), radius 0.5 = two cells, R = 3"""
    g = W.make_geometry(np.zeros(3, F), np.array([4, 2, 1], F), 0.25)
    p = np.array([[2.125, 1.125, 0.625]], F)
    r2 = W.r2_of(0.5)
    see = lambda c, **kw: bool(W.walk_visits(g, p, np.array([c]), r2, **kw)[0])
    assert see((8, 4, 2)) and see((6, 4, 2)) and see((10, 4, 2))                                # gap 1.5 cells = 0.375 m < 0.5
    assert not see((5, 4, 2)) and not see((11, 4, 2))                                           # gap 2.5 cells: (0.625^2) * 0.998 >= 0.25, trimmed
    assert not see((4, 4, 2))                                                                   # beyond the reach
    assert see((8, 6, 2)) and not see((8, 7, 2))                                                # the (y, z) skip
    assert see((8, 4, 4)) and see((8, 4, 0))                                                    # z: gap 1.5 cells either way
    assert see((7, 5, 3)) and see((9, 3, 1))                                                    # 0.5 cells on each axis
    assert not see((6, 6, 4))                                                                   # 1.5 cells on each axis: 3 * 0.375^2 = 0.42 >= 0.25
    assert not see((8, 6, 4))                                                                   # 2 * 0.375^2 * 0.998 = 0.2807 >= 0.25: the row is skipped, p's column with it
    assert see((8, 5, 4)) and see((6, 5, 2))                                                    # 0.375^2 + 0.125^2 = 0.156
    assert see((8, 6, 3)) and not see((5, 6, 3))                                                # a row that is entered: p's column stays, the far end is trimmed
    # the weakened forms differ where they should: a reach of 2 leaves (5, ...) out anyway, and drops nothing nearer
    assert see((6, 4, 2), formula="naive", radius=0.5) and not see((5, 4, 2), formula="naive", radius=0.5)
