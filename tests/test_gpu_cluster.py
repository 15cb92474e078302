"""Clustering on the device (sf_map_cluster_dbscan, sf_map_cluster_euclidean, sf_cloud_filter_clusters,
sf_cloud_keep_largest_cluster) against the numpy restatement of the rule (tests/cluster_ref_np.py), which
tests/test_cluster_rule.py pins to scikit-learn.  Everything is integer: labels, sizes and statistics are compared exactly and no
point is excused."""
import numpy as np
import pytest

import cluster_ref_np as ref
from test_gpu_knn import lattice
from test_gpu_knn_normals import noisy_map  # noqa: F401  (the fixture: [1] is 3 000 mixed points plus 20 isolated ones)

pytestmark = pytest.mark.gpu

DBSCAN_PARAMS = ((0.12, 5), (0.2, 3), (0.2, 10), (0.3, 1))
SIZE_FILTERS = ((1, 0), (5, 0), (5, 200))
INVALID, STATE = "error -1:", "error -4:"


@pytest.fixture(scope="module")
def clouds(noisy_map):  # noqa: F811
    return {"mixed": noisy_map[1], "blobs": ref.blob_cloud()}


@pytest.fixture(scope="module")
def refs(clouds):
    """the restatement, computed once per (cloud, call, parameters) and never changed"""
    cache = {}

    def get(name, kind, *args):
        key = (name, kind) + args
        if key not in cache:
            out = (ref.dbscan if kind == "dbscan" else ref.euclidean)(clouds[name], *args)[:3]
            for a in out[:2]:
                a.setflags(write=False)
            cache[key] = out
        return cache[key]
    return get


def same(got, want, what):
    labels, sizes, st = got
    rl, rs, rst = want
    assert labels.dtype == np.int32 and sizes.dtype == np.int32 and labels.shape == rl.shape, what
    assert np.array_equal(labels, rl), (what, np.flatnonzero(labels != rl)[:5])
    assert np.array_equal(sizes, rs), what
    assert st == rst, (what, st, rst)


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", ["mixed", "blobs"])
def test_parity(api, ctx, clouds, refs, name):
    mp = api.Map(ctx, api.Cloud(ctx, clouds[name]), 0.25)
    for eps, min_points in DBSCAN_PARAMS:
        got = mp.cluster_dbscan(eps, min_points)
        print("%s dbscan(%g, %d): %s" % (name, eps, min_points, got[2]))
        same(got, refs(name, "dbscan", eps, min_points), (name, eps, min_points))
    for min_size, max_size in SIZE_FILTERS:
        got = mp.cluster_euclidean(0.2, min_size, max_size)
        print("%s euclidean(0.2, %d, %d): %s" % (name, min_size, max_size, got[2]))
        same(got, refs(name, "euclidean", 0.2, min_size, max_size), (name, min_size, max_size))
    mp.close()


# ------------------------------------------------------------------ 2. a border point two clusters contend for
@pytest.mark.parametrize("a_first", [True, False])
def test_contested_border_point(api, ctx, a_first):
    eps = 0.5
    x = ref.contested_cloud(eps, a_first)
    for cell in (0.0, 0.25):
        mp = api.Map(ctx, api.Cloud(ctx, x), cell)
        labels, sizes, st = mp.cluster_dbscan(eps, 8)
        mp.close()
        assert list(labels) == [0] * 12 + [1] * 12 + [0]            # the blob that comes first in the array, whichever it is
        assert list(sizes) == [13, 12]
        assert st == dict(n_points=25, n_valid=25, n_core=24, n_border=1, n_noise=0, n_clusters=2, largest_size=13, n_kept=25)
        same((labels, sizes, st), ref.dbscan(x, eps, 8)[:3], (a_first, cell))


# ------------------------------------------------------------------ 3. long chains
def serpentine(n=20_000, rows=40, step=0.09):
    """n points `step` apart along a path that runs to and fro through `rows` rows, five steps between the rows: consecutive points
    are the only ones closer than 1.4 steps"""
    per_row = -(-(n + 4) // rows) - 4
    ij = []
    for r in range(rows):
        xs = range(per_row) if r % 2 == 0 else range(per_row - 1, -1, -1)
        ij += [(i, 5 * r) for i in xs]
        ij += [(xs[-1], 5 * r + k) for k in range(1, 5)]
    ij = np.array(ij[:n], np.float64)
    assert len(ij) == n
    return np.concatenate([ij * step, np.zeros((n, 1))], 1).astype(np.float32)


def test_long_chains(api, ctx):
    eps = 0.1
    path = serpentine()
    n = len(path)
    rng = np.random.default_rng(6)
    perm = rng.permutation(n)
    mp = api.Map(ctx, api.Cloud(ctx, path[perm]), 0.25)
    assert mp.cell_size()[1][1] >= 40
    first = None
    for rep in range(5):
        labels, sizes, st = mp.cluster_euclidean(eps)
        assert not labels.any() and list(sizes) == [n]
        assert st == dict(n_points=n, n_valid=n, n_core=n, n_border=0, n_noise=0, n_clusters=1, largest_size=n, n_kept=n)
    mp.close()
    # three points out: four pieces
    cuts = np.array([3_333, 9_000, 9_002])
    piece = np.searchsorted(cuts, np.arange(n), side="right")          # of a path position
    left = np.ones(n, bool)
    left[cuts] = False
    order = perm[left[perm]]                                            # path positions in array order
    pp = piece[order]
    starts = np.array([np.flatnonzero(pp == k)[0] for k in range(4)])   # where each piece first shows in the array
    rank = np.empty(4, np.int64)
    rank[np.argsort(starts)] = np.arange(4)
    want = rank[pp].astype(np.int32)
    want_sizes = np.bincount(want).astype(np.int32)
    assert sorted(want_sizes) == sorted([3_333, 9_000 - 3_334, 1, n - 9_003])
    mp = api.Map(ctx, api.Cloud(ctx, path[order]), 0.25)
    for rep in range(5):
        labels, sizes, st = mp.cluster_euclidean(eps)
        assert np.array_equal(labels, want) and np.array_equal(sizes, want_sizes)
        assert st["n_clusters"] == 4 and st["largest_size"] == n - 9_003 and st["n_kept"] == n - 3
        d = mp.cluster_dbscan(eps, 2)                                   # the single point is noise, the ends of the pieces are core
        assert d[2]["n_clusters"] == 3 and d[2]["n_noise"] == 1 and d[2]["n_border"] == 0 and np.array_equal(d[0] >= 0, want_sizes[want] > 1)
        if first is None:
            first = (labels, d[0])
        assert np.array_equal(labels, first[0]) and np.array_equal(d[0], first[1])
    mp.close()


# ------------------------------------------------------------------ 4. the reach at an exact multiple of the cell
@pytest.mark.parametrize("cell", [0.5, 1.0])
def test_tolerance_at_a_multiple_of_the_cell(api, ctx, cell):
    m = lattice()
    n = len(m)
    mp = api.Map(ctx, api.Cloud(ctx, m), cell)
    labels, sizes, st = mp.cluster_euclidean(1.0)                       # r2 = 1.0: the face neighbours are AT the tolerance
    assert np.array_equal(labels, np.arange(n)) and (sizes == 1).all() and st["n_clusters"] == n and st["largest_size"] == 1
    above = float(np.sqrt(np.float64(np.nextafter(np.float32(1.0), np.float32(2.0)))))
    assert np.float32(above * above) == np.nextafter(np.float32(1.0), np.float32(2.0))
    labels, sizes, st = mp.cluster_euclidean(above)
    assert not labels.any() and list(sizes) == [n] and st["n_clusters"] == 1
    labels, sizes, st = mp.cluster_dbscan(above, 5)                     # corners count 4, edges 5: the corners are border points
    same((labels, sizes, st), ref.dbscan(m, above, 5)[:3], cell)
    assert st["n_core"] == n - 8 and st["n_border"] == 8 and st["n_clusters"] == 1
    mp.close()


# ------------------------------------------------------------------ 5. independence of the cell and of the run
def test_independent_of_cell_and_run(api, ctx, clouds, refs):
    x = clouds["blobs"]
    for cell in (0.25, 0.0, 0.15, 0.5, 1.0, 0.25):
        mp = api.Map(ctx, api.Cloud(ctx, x), cell)
        same(mp.cluster_dbscan(0.2, 5), refs("blobs", "dbscan", 0.2, 5), cell)
        same(mp.cluster_euclidean(0.2), refs("blobs", "euclidean", 0.2, 1, 0), cell)
        mp.close()


# ------------------------------------------------------------------ 6. edges
def test_non_finite_coincident_and_few_points(api, ctx):
    rng = np.random.default_rng(8)
    holes = rng.uniform(-1, 1, (400, 3)).astype(np.float32)
    holes[7] = [np.nan, 0.0, 0.0]
    holes[21] = [0.0, np.inf, 0.0]
    mp = api.Map(ctx, api.Cloud(ctx, holes), 0.25)
    for eps, min_points in ((0.3, 1), (0.3, 4), (0.2, 3)):
        got = mp.cluster_dbscan(eps, min_points)
        same(got, ref.dbscan(holes, eps, min_points)[:3], (eps, min_points))
        assert (got[0][[7, 21]] == -1).all() and got[2]["n_points"] == 400 and got[2]["n_valid"] == 398
        assert got[2]["n_kept"] + got[2]["n_noise"] == 398
    got = mp.cluster_euclidean(0.3, 3, 0)
    same(got, ref.euclidean(holes, 0.3, 3, 0), "holes")
    mp.close()
    # 50 coincident points among others
    twins = np.concatenate([rng.uniform(2, 3, (30, 3)), np.repeat([[1.0, 1.0, 1.0]], 50, axis=0)]).astype(np.float32)[rng.permutation(80)]
    mp = api.Map(ctx, api.Cloud(ctx, twins), 0.0)
    labels, sizes, st = mp.cluster_dbscan(0.05, 50)
    where = (twins == 1.0).all(1)
    assert np.array_equal(labels, np.where(where, 0, -1)) and list(sizes) == [50]
    assert st == dict(n_points=80, n_valid=80, n_core=50, n_border=0, n_noise=30, n_clusters=1, largest_size=50, n_kept=50)
    mp.close()
    # one point; only non-finite points
    mp = api.Map(ctx, api.Cloud(ctx, np.array([[0.5, -1.0, 2.0]], np.float32)), 0.25)
    for got in (mp.cluster_euclidean(0.3), mp.cluster_dbscan(0.3, 1)):
        assert list(got[0]) == [0] and list(got[1]) == [1]
        assert got[2] == dict(n_points=1, n_valid=1, n_core=1, n_border=0, n_noise=0, n_clusters=1, largest_size=1, n_kept=1)
    got = mp.cluster_dbscan(0.3, 2)
    assert list(got[0]) == [-1] and len(got[1]) == 0 and got[2]["n_noise"] == 1 and got[2]["n_clusters"] == 0
    mp.close()
    mp = api.Map(ctx, api.Cloud(ctx, np.full((5, 3), np.nan, np.float32)), 0.25)
    for got in (mp.cluster_euclidean(0.3), mp.cluster_dbscan(0.3, 3)):
        assert (got[0] == -1).all() and len(got[0]) == 5 and len(got[1]) == 0
        assert got[2] == dict(n_points=5, n_valid=0, n_core=0, n_border=0, n_noise=0, n_clusters=0, largest_size=0, n_kept=0)
    mp.close()
    mp = api.Map(ctx, api.Cloud(ctx, np.zeros((0, 3), np.float32)), 0.25)
    got = mp.cluster_euclidean(0.3)
    assert got[0].shape == (0,) and got[1].shape == (0,) and got[2] == dict.fromkeys(ref.STAT_KEYS, 0)
    mp.close()


def test_arguments(api, ctx, clouds, refs):
    import ctypes as C
    x = clouds["mixed"]
    mp = api.Map(ctx, api.Cloud(ctx, x), 0.25)
    cloud = api.Cloud(ctx, x)
    # nothing reaches min_points: all noise
    labels, sizes, st = mp.cluster_dbscan(0.2, 10_000)
    assert (labels == -1).all() and len(sizes) == 0
    assert st == dict(n_points=len(x), n_valid=len(x), n_core=0, n_border=0, n_noise=len(x), n_clusters=0, largest_size=0, n_kept=0)
    # cap_sizes below n_clusters: only that many entries are written; every output may be NULL
    rl, rs, rst = refs("mixed", "euclidean", 0.2, 1, 0)
    assert rst["n_clusters"] > 10
    lib, p = mp.lib, api._p
    buf = np.full(20, -7, np.int32)
    stc = api.ClusterStats()
    api._check(lib.sf_map_cluster_euclidean(mp.h, C.c_double(0.2), C.c_int64(1), C.c_int64(0), None, p(buf), C.c_int64(10), C.byref(stc)))
    assert np.array_equal(buf[:10], rs[:10]) and (buf[10:] == -7).all() and stc.as_dict() == rst
    api._check(lib.sf_map_cluster_euclidean(mp.h, C.c_double(0.2), C.c_int64(1), C.c_int64(0), None, None, C.c_int64(0), None))
    api._check(lib.sf_map_cluster_dbscan(mp.h, C.c_double(0.2), C.c_int(3), None, p(buf), C.c_int64(0), None))
    assert (buf[10:] == -7).all() and np.array_equal(buf[:10], rs[:10])
    for eps, min_points in ((0.0, 3), (-1.0, 3), (np.nan, 3), (np.inf, 3), (0.2, 0), (0.2, -2)):
        with pytest.raises(api.SlamFusionError, match=INVALID):
            mp.cluster_dbscan(eps, min_points)
    for tol, min_size in ((0.0, 1), (-0.2, 1), (np.nan, 1), (np.inf, 1), (0.2, 0), (0.2, -1)):
        with pytest.raises(api.SlamFusionError, match=INVALID):
            mp.cluster_euclidean(tol, min_size)
        with pytest.raises(api.SlamFusionError, match=INVALID):
            cloud.filter_clusters(tol, min_size)
        if min_size == 1:
            with pytest.raises(api.SlamFusionError, match=INVALID):
                cloud.keep_largest_cluster(tol)
        assert len(cloud) == len(x)
    same(mp.cluster_euclidean(0.2), (rl, rs, rst), "after the refusals")
    unbuilt = api.Map(ctx)
    with pytest.raises(api.SlamFusionError, match=STATE):
        api._check(unbuilt.lib.sf_map_cluster_dbscan(unbuilt.h, C.c_double(0.2), C.c_int(3), None, None, C.c_int64(0), None))
    with pytest.raises(api.SlamFusionError):
        unbuilt.cluster_euclidean(0.2)
    assert unbuilt.lib.sf_map_cluster_dbscan(unbuilt.h, C.c_double(0.2), C.c_int(3), None, None, C.c_int64(0), None) == -4
    assert unbuilt.lib.sf_map_cluster_euclidean(unbuilt.h, C.c_double(0.2), C.c_int64(1), C.c_int64(0), None, None, C.c_int64(0), None) == -4
    unbuilt.build(api.Cloud(ctx, x), 0.5)
    same(unbuilt.cluster_euclidean(0.2), (rl, rs, rst), "built later")
    unbuilt.close()
    mp.close()
    cloud.close()


# ------------------------------------------------------------------ 7. the core points are those of the radius filter
def test_core_points_are_the_radius_counts(api, ctx, clouds):
    for name, eps, min_points in (("mixed", 0.3, 3), ("blobs", 0.2, 10), ("blobs", 0.12, 5)):
        mp = api.Map(ctx, api.Cloud(ctx, clouds[name]), 0.25)
        labels, sizes, st = mp.cluster_dbscan(eps, min_points)
        cnt = mp.radius_outliers(eps, 0)[1]
        assert st["n_core"] == int((cnt >= min_points).sum()) and st["n_core"] > 0
        assert (labels[cnt >= min_points] >= 0).all() and (labels[cnt == 1] == -1).all()
        mp.close()


# ------------------------------------------------------------------ 8. nothing else moved
def test_the_map_is_left_as_it_was(api, ctx, clouds, refs):
    x = clouds["mixed"]
    rng = np.random.default_rng(2)
    q = (x[rng.integers(0, len(x), 1000)] + rng.normal(0, 0.1, (1000, 3))).astype(np.float32)
    mp = api.Map(ctx, api.Cloud(ctx, x), 0.25)
    mp.estimate_normals_knn(20, covariance=True)
    mp.build_neighbour_table()

    def state():
        ix = mp.index()
        nrm, cnt = mp.download_normals()
        ids, r = mp.download_neighbour_table()
        idx, d2 = mp.nn(q)
        return [nrm.view(np.uint32), cnt, mp.download_covariances().view(np.uint64), ids, r.view(np.uint32), ix["pts4"].view(np.uint32), ix["cell_start"],
                ix["org"].view(np.uint32), np.float32(ix["inv_h"]).view(np.uint32), np.float32(ix["gap_eps"]).view(np.uint32), idx, d2.view(np.uint32)]

    before = state()
    mp.cluster_dbscan(0.3, 3)
    mp.cluster_euclidean(0.2, 5, 200)
    after = state()
    assert len(before) == len(after)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert mp.neighbour_table_info()["present"]
    # a window stays in force for sf_map_nn and is ignored by the clustering
    mp.window_sphere(x[0], 1.0)
    inside = mp.window_count()
    assert 0 < inside < len(x)
    idx_w, d2_w = mp.nn(q)
    same(mp.cluster_euclidean(0.2), refs("mixed", "euclidean", 0.2, 1, 0), "window")
    same(mp.cluster_dbscan(0.3, 1), refs("mixed", "dbscan", 0.3, 1), "window")
    idx_w2, d2_w2 = mp.nn(q)
    assert mp.window_count() == inside and np.array_equal(idx_w, idx_w2) and np.array_equal(d2_w.view(np.uint32), d2_w2.view(np.uint32))
    assert not np.array_equal(idx_w, before[-2])                       # (the window does change what sf_map_nn answers)
    mp.close()


def test_launch_time_is_recorded(api, ctx, clouds):
    mp = api.Map(ctx, api.Cloud(ctx, clouds["mixed"]), 0.25)
    mp.profile_launches(True)
    with pytest.raises(api.SlamFusionError):
        mp.last_launch_ms()
    mp.cluster_euclidean(0.2)
    a = mp.last_launch_ms()
    mp.cluster_dbscan(0.3, 3)
    b = mp.last_launch_ms()
    assert 0.0 < a < 5000.0 and 0.0 < b < 5000.0
    mp.close()


# ------------------------------------------------------------------ 9. the cloud calls
@pytest.mark.parametrize("cell", [0.0, 0.5])
def test_cloud_calls(api, ctx, clouds, cell):
    x = clouds["blobs"]
    for which in ("filter", "largest"):
        cloud = api.Cloud(ctx, x)
        if which == "filter":
            st = cloud.filter_clusters(0.2, 50, cell=cell)
            mask, rst = ref.filter_clusters(x, 0.2, 50)
        else:
            st = cloud.keep_largest_cluster(0.2, cell=cell)
            mask, rst = ref.keep_largest_cluster(x, 0.2)
        print(which, st)
        assert 0 < mask.sum() < len(x)
        assert st == rst, (which, st, rst)
        assert len(cloud) == int(mask.sum())
        assert np.array_equal(cloud.last_indices(), np.flatnonzero(mask))
        assert np.array_equal(cloud.download().view(np.uint32), x[mask].view(np.uint32))
        if which == "filter":                                           # the cloud is usable afterwards: what is left passes whole
            st2 = cloud.filter_clusters(0.2, 50, 0, cell)
            assert st2["n_kept"] == st2["n_points"] == int(mask.sum()) and st2["n_noise"] == 0 and st2["n_clusters"] == st["n_clusters"]
        cloud.close()


def test_cloud_calls_on_an_empty_cloud(api, ctx):
    zero = dict.fromkeys(ref.STAT_KEYS, 0)
    cloud = api.Cloud(ctx, np.zeros((0, 3), np.float32))
    assert cloud.filter_clusters(0.2, 50) == zero and len(cloud) == 0 and len(cloud.last_indices()) == 0
    assert cloud.keep_largest_cluster(0.2) == zero and len(cloud) == 0
    cloud.close()
    cloud = api.Cloud(ctx, np.array([[0, 0, 0], [np.nan, 0, 0], [0.1, 0, 0], [3, 0, 0]], np.float32))
    st = cloud.keep_largest_cluster(0.2)
    assert st == dict(n_points=4, n_valid=3, n_core=3, n_border=0, n_noise=1, n_clusters=2, largest_size=2, n_kept=2)
    assert list(cloud.last_indices()) == [0, 2]
    cloud.close()
