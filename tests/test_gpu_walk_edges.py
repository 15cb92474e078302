"""Every fixed-radius consumer of the grid index on the edge clouds of tests/walk_fixtures.py, against brute force: anchors on the
faces of their cells, partners one float32 step inside and outside the radius, grids 20 000 cells wide, clouds 65 km out, a snapped
origin.  tests/test_walk_rule.py shows on this CPU that the walk's rule loses nothing on these clouds and that its weakened forms do;
test_geometry here ties that restatement to the index the kernels walk, bit for bit.  Everything is compared with np.array_equal:
the rule is float32 and strict on both sides, nothing is excused.  The radius normals (box_rows / ball_box) have
tests/test_gpu_normals_radius.py."""
import ctypes as C

import numpy as np
import pytest

import cluster_ref_np as cluster_ref
import fpfh_ref_np as fpfh_ref
import iss_ref_np as iss_ref
import outlier_ref_np as outlier_ref
import radius_ref_np as ref
import walk_fixtures as fx
import walk_ref_np as W
from test_gpu_radius_search import FILLS, ORDERS, same

pytestmark = pytest.mark.gpu

F = np.float32
SF_ERR_STATE, SF_ERR_OVERFLOW = -4, -5
SECOND_CELL = 0.37            # what the cube cases are built with a second time
FEATURE_CASES = (("cube_h010", 1), ("corridor_h010_lattice", 0), ("cube_h015_65km", 3))   # (case, index of the radius): two whole cells; a wide snapped grid; 65 km out


class Pts4:
    """the points of an index for radius_ref, without another download of the table"""

    def __init__(self, pts4):
        self.pts4 = pts4

    def index(self):
        return dict(pts4=self.pts4)


@pytest.fixture(scope="module")
def built(api, ctx):
    """name -> (Map, fixture, Pts4 of its index): every case built once"""
    cache = {}

    def get(name):
        if name not in cache:
            f = fx.fixture(name)
            mp = api.Map(ctx)
            if f["lattice"]:
                mp.set_origin_lattice(f["lattice"])
            mp.build(api.Cloud(ctx, f["points"]), f["cell"])
            cache[name] = (mp, f, Pts4(mp.index()["pts4"]))
        return cache[name]

    yield get
    for mp, _, _ in cache.values():
        mp.close()


@pytest.fixture(scope="module")
def rows_ref():
    """(name, radius index, order) -> radius_ref of the cloud's own points, computed once and left unchanged"""
    cache = {}

    def get(name, host, ri, order):
        key = (name, ri, order)
        if key not in cache:
            f = fx.fixture(name)
            out = ref.radius_ref(host, f["points"], f["radii"][ri], order)
            for a in out:
                a.setflags(write=False)
            cache[key] = out
        return cache[key]

    return get


def bits(v):
    return np.asarray(v, F).view(np.uint32)


# ------------------------------------------------------------------ 1. the index is the model's
@pytest.mark.parametrize("name", fx.NAMES)
def test_geometry(built, name):
    mp, f, _ = built(name)
    g = W.geometry(f["points"], f["cell"], f["lattice"])
    ix = mp.index()
    cell, dims = mp.cell_size()
    assert bits(cell) == bits(g.h) and list(dims) == g.dim.tolist()
    assert np.array_equal(bits(ix["org"]), bits(g.org)) and bits(ix["inv_h"]) == bits(g.inv_h) and bits(ix["gap_eps"]) == bits(g.gap_eps)
    pts4, cs = ix["pts4"], ix["cell_start"].astype(np.int64)
    finite = np.isfinite(f["points"]).all(1)
    assert len(pts4) == finite.sum() and len(cs) == int(np.prod(g.dim)) + 1 and cs[0] == 0 and cs[-1] == len(pts4)
    ids = pts4[:, 3].view(np.uint32)
    assert np.array_equal(np.sort(ids), np.flatnonzero(finite)) and np.array_equal(bits(pts4[:, :3]), bits(f["points"][ids]))
    c = W.cell(g, W.G(g, pts4[:, :3]))
    key = (c[:, 2] * g.dim[1] + c[:, 1]) * g.dim[0] + c[:, 0]
    pos = np.arange(len(pts4))
    assert ((cs[key] <= pos) & (pos < cs[key + 1])).all()                                       # every point in the run of the cell the model bins it into
    assert (np.diff(key) >= 0).all() and (np.diff(ids.astype(np.int64))[np.diff(key) == 0] > 0).all()
    occupied, held = np.unique(key, return_counts=True)
    assert np.array_equal(cs[occupied + 1] - cs[occupied], held)                                # ... and nothing else in those runs


# ------------------------------------------------------------------ 2. the radius filter
@pytest.mark.parametrize("name", fx.NAMES)
def test_radius_filter(built, name):
    mp, f, _ = built(name)
    for radius in f["radii"]:
        keep, n_nb, st = mp.radius_outliers(radius, 0)
        want = outlier_ref.radius_counts(f["points"], radius)
        assert np.array_equal(n_nb, want), (name, radius, np.flatnonzero(n_nb != want)[:5])
        assert np.array_equal(keep, want > 0) and st["n_kept"] == int((want > 0).sum())


# ------------------------------------------------------------------ 3. search and graph, every order and fill
@pytest.mark.parametrize("name", fx.NAMES)
def test_search_and_graph(built, rows_ref, name):
    mp, f, host = built(name)
    for ri, radius in enumerate(f["radii"]):
        for order in ORDERS:
            want = rows_ref(name, host, ri, order)
            for fill in FILLS:
                mp.set_radius_fill(fill)
                same(mp.radius_graph(radius, order), want, (name, radius, order, fill, "graph"))
                same(mp.radius_search(f["points"], radius, order), want, (name, radius, order, fill, "search"))
    mp.set_radius_fill("auto")


# ------------------------------------------------------------------ 4. queries binned outside the grid
@pytest.mark.parametrize("name", fx.NAMES)
def test_outside_queries(built, name):
    mp, f, host = built(name)
    for ri, radius in enumerate(f["radii"]):
        q = fx.outside_queries(f, ri)
        hits = None
        for order in ORDERS:
            want = ref.radius_ref(host, q, radius, order)
            for fill in FILLS:
                mp.set_radius_fill(fill)
                same(mp.radius_search(q, radius, order), want, (name, radius, order, fill, "outside"))
            hits = np.diff(want[0]).reshape(-1, 4)
        assert (hits[:, :2] >= 1).all() and hits[:, :2].sum() > hits[:, 2:].sum()               # the two inside hold their face point, which the two outside have lost
    mp.set_radius_fill("auto")


# ------------------------------------------------------------------ 5. k nearest within the radius
@pytest.mark.parametrize("name", fx.NAMES)
def test_knn_and_hybrid(built, rows_ref, name):
    mp, f, host = built(name)
    x = f["points"]
    for ri, radius in enumerate(f["radii"]):
        off, idx, d2 = rows_ref(name, host, ri, "distance")
        assert np.diff(off).max() <= 64                                                         # the whole row fits: nothing is cut
        wi, wd, wc = ref.rows_cut(off, idx, d2, 64)
        for what, (gi, gd, gc) in (("knn", mp.knn(x, 64, W.r2_of(radius))), ("hybrid", mp.hybrid_search(x, radius, 64))):
            assert np.array_equal(gc, wc), (name, radius, what, np.flatnonzero(gc != wc)[:5])
            assert np.array_equal(bits(gd), bits(wd)) and np.array_equal(gi, wi), (name, radius, what)


# ------------------------------------------------------------------ 6. the nearest neighbour
def nn_ref(P, ids, q, thr):
    """brute force -> (hit bool, d2 float32 of the nearest, its id where it is the only one at that distance else -2)"""
    d = outlier_ref.d2_rows(np.ascontiguousarray(q, F), P)
    best = d.min(1)
    unique = (d == best[:, None]).sum(1) == 1
    return best < thr, best, np.where(unique, ids[d.argmin(1)].astype(np.int64), -2)


def check_nn(mp, host, q, thr, what):
    P = np.ascontiguousarray(host.pts4[:, :3])
    ids = host.pts4[:, 3].view(np.uint32)
    hit, best, who = nn_ref(P, ids, q, thr)
    idx, d2 = mp.nn(q, thr)
    assert np.array_equal(idx >= 0, hit), (what, np.flatnonzero((idx >= 0) != hit)[:5])
    assert np.array_equal(bits(d2[hit]), bits(best[hit])) and np.isinf(d2[~hit]).all(), what
    sure = hit & (who >= 0)
    assert np.array_equal(idx[sure], who[sure]), (what, np.flatnonzero(sure & (idx != who))[:5])
    return hit


@pytest.mark.parametrize("name", fx.NAMES)
def test_nearest_neighbour(built, name):
    mp, f, host = built(name)
    g = f["geometry"]
    P = np.ascontiguousarray(host.pts4[:, :3])
    across = 0
    for ri, radius in enumerate(f["radii"]):
        r2 = W.r2_of(radius)
        q = fx.fresh_queries(f, ri)                                                             # no points of the cloud: two inside, two outside of their anchor
        hit = check_nn(mp, host, q, r2, (name, radius, "fresh"))
        assert hit.any() and not hit.all()
        check_nn(mp, host, np.concatenate([f["sets"][ri]["q"].reshape(-1, 3), fx.outside_queries(f, ri)]), r2, (name, radius, "partners"))
        # the nearest point across a face, the runner-up one float32 step behind it in the query's own cell: the rings must not stop early
        q = fx.face_queries(f, ri)
        check_nn(mp, host, q, np.inf, (name, radius, "faces"))
        check_nn(mp, host, q, r2, (name, radius, "faces within r2"))
        d = outlier_ref.d2_rows(q, P)
        two = np.argsort(d, axis=1, kind="stable")[:, :2]
        c, c1, c2 = W.cell(g, W.G(g, q)), W.cell(g, W.G(g, P[two[:, 0]])), W.cell(g, W.G(g, P[two[:, 1]]))
        across += int(((c1 != c).any(1) & (c2 == c).all(1)).sum())
    print(name, "queries whose nearest point lies across a face, the runner-up in their own cell:", across)
    assert across >= 3


# ------------------------------------------------------------------ 7. clustering: the END and AUX forms of the walk
@pytest.mark.parametrize("name", fx.NAMES)
def test_clustering(built, name):
    mp, f, _ = built(name)
    x = f["points"]
    for radius in f["radii"]:
        labels, sizes, st = mp.cluster_euclidean(radius)
        wl, ws, wst = cluster_ref.euclidean(x, radius)
        assert np.array_equal(labels, wl) and np.array_equal(sizes, ws) and st == wst, (name, radius, "euclidean", st, wst)
        labels, sizes, st = mp.cluster_dbscan(radius, 3)
        wl, ws, wst, _ = cluster_ref.dbscan(x, radius, 3)
        assert np.array_equal(labels, wl) and np.array_equal(sizes, ws) and st == wst, (name, radius, "dbscan", st, wst)


# ------------------------------------------------------------------ 8. feature_reach, the copy of the reach
@pytest.mark.parametrize("name,ri", FEATURE_CASES)
def test_feature_counts(built, name, ri):
    mp, f, _ = built(name)
    x, radius = f["points"], f["radii"][ri]
    rng = np.random.default_rng(11)
    nrm = rng.normal(size=(len(x), 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    mp.set_normals(nrm)
    _, pairs = mp.compute_spfh(radius)
    want = fpfh_ref.spfh(x, nrm, radius)["n_pairs"]
    assert want.max() >= 4 and np.array_equal(pairs, want), (name, radius, np.flatnonzero(pairs != want)[:5])
    got = mp.iss_saliency(radius)["n_neighbors"]
    want = iss_ref.saliency(x, radius)["n_neighbors"]
    assert np.array_equal(got, want), (name, radius, np.flatnonzero(got != want)[:5])
    assert np.array_equal(got, outlier_ref.radius_counts(x, radius))


# ------------------------------------------------------------------ 9. another cell size, the same rows
@pytest.mark.parametrize("name", fx.CUBES)
def test_cell_independence(api, ctx, built, rows_ref, name):
    _, f, host = built(name)
    x = f["points"]
    other = api.Map(ctx, api.Cloud(ctx, x), SECOND_CELL)
    assert other.cell_size()[0] != F(f["cell"])
    host2 = Pts4(other.index()["pts4"])
    for ri, radius in enumerate(f["radii"]):
        off, idx, d2 = rows_ref(name, host, ri, "distance")
        for fill in FILLS:
            other.set_radius_fill(fill)
            same(other.radius_search(x, radius, "distance"), ref.radius_ref(host2, x, radius, "distance"), (name, radius, fill, SECOND_CELL))
        g_off, g_idx, g_d2, _ = other.radius_search(x, radius, "distance")
        rows = np.repeat(np.arange(len(x)), np.diff(off))
        assert np.array_equal(g_off, off) and np.array_equal(bits(g_d2), bits(d2))
        assert np.array_equal(g_idx[np.lexsort((g_idx, rows))], idx[np.lexsort((idx, rows))])    # equal d2 may change places, nothing else
        assert np.array_equal(other.radius_outliers(radius, 0)[1], np.diff(off))
    other.close()


# ------------------------------------------------------------------ 10. an axis float32 cannot count
def test_an_axis_of_more_than_2_24_cells_is_refused(api, ctx):
    """17 000 m at a cell of 1 mm is 17e6 cells on x, above 2^24: grid_cell's float32 clamp could name a cell beyond the grid.  The
    refusal only; no such grid is ever walked."""
    x = np.array([[0.0, 0.0, 0.0], [17000.0, 0.0, 0.0]], F)
    lib = api.load_library()
    cloud = api.Cloud(ctx, x)
    mp = api.Map(ctx)
    assert lib.sf_map_build(mp.h, cloud.h, C.c_float(0.001)) == SF_ERR_OVERFLOW
    n = C.c_int64(-1)
    assert lib.sf_map_index_info(mp.h, C.byref(n), None, None, None, None) == SF_ERR_STATE         # the map stays unbuilt
    q = np.zeros((1, 3), F)
    assert lib.sf_map_radius_search(mp.h, q.ctypes.data_as(C.c_void_p), C.c_int64(1), C.c_double(1.0), C.c_int(0), None, None) == SF_ERR_STATE
    with pytest.raises(api.SlamFusionError):
        mp.build(cloud, 0.001)
    mp.build(cloud, 0.0)                                                                        # an automatic cell grows until the axis fits
    cell, dims = mp.cell_size()
    assert max(dims) <= 2 ** 24 and len(mp) == 2
    # a built map that is asked for such a grid is unbuilt afterwards, not left on its old index
    assert lib.sf_map_build(mp.h, cloud.h, C.c_float(0.001)) == SF_ERR_OVERFLOW
    assert lib.sf_map_index_info(mp.h, C.byref(n), None, None, None, None) == SF_ERR_STATE
    mp.close()


def test_a_patch_that_would_grow_an_axis_past_2_24_cells_takes_the_build_which_refuses(api, ctx):
    """16 000 m at 1 mm is 16 000 000 cells on x, which an index may have; a merge that brings a point at 17 000 m makes sf_map_patch
    fall back to the build, and the build refuses.  Nothing searches either grid."""
    lib = api.load_library()
    prev = api.voxel_merge_min_points(0)
    try:
        dev = api.Cloud(ctx, np.array([[0.0, 0.0, 0.0], [8000.0, 0.0, 0.0], [16000.0, 0.0, 0.0]], F))
        dev.voxel_downsample(0.1, "pcl")
        mp = api.Map(ctx).build(dev, 0.001)
        assert mp.cell_size()[1] == (16_000_000, 1, 1) and W.geometry(dev.download(), 0.001).dim.tolist() == [16_000_000, 1, 1]
        _, merged = dev.voxel_merge(api.Cloud(ctx, np.array([[17000.0, 0.0, 0.0]], F)), 0.1)
        assert merged and len(dev.download()) == 4
        done = C.c_int(7)
        assert lib.sf_map_patch(mp.h, dev.h, C.byref(done)) == SF_ERR_OVERFLOW
        n = C.c_int64(-1)
        assert lib.sf_map_index_info(mp.h, C.byref(n), None, None, None, None) == SF_ERR_STATE
        mp.build(dev, 0.0)
        assert len(mp) == 4 and max(mp.cell_size()[1]) <= 2 ** 24
        mp.close()
    finally:
        api.voxel_merge_min_points(prev)
