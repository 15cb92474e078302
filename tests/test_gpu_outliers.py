"""The outlier filters on the device (sf_map_statistical_outliers, sf_map_radius_outliers and the two sf_cloud_remove_* calls)
against the numpy restatement of their rules (tests/outlier_ref_np.py).  Bounds: mean_dist within 1e-13 relative (at most
65 square roots and a 6-level tree: below 8e-15 even with a sqrt that is off by an ulp), the statistics within 1e-12 relative;
flags, neighbour counts and everything said to be independent of the cell or the run are compared exactly."""
import numpy as np
import pytest

import outlier_ref_np as ref
from test_gpu_knn import lattice
from test_gpu_knn_normals import noisy_map  # noqa: F401  (the fixture: [1] is 3 000 mixed points plus 20 isolated ones)

pytestmark = pytest.mark.gpu

STAT_KEYS = ("mean", "stddev", "threshold")
PCL_KS, O3D_KS, RATIOS = (1, 8, 20, 63), (2, 8, 20, 64), (1.0, 2.0)


@pytest.fixture(scope="module")
def parity_cloud(noisy_map):  # noqa: F811
    return noisy_map[1]


@pytest.fixture(scope="module")
def parity_ref(parity_cloud):
    """the restatement for all sixteen parameter sets, computed once: (flavour, k, ratio) -> (keep, d, stats)"""
    out = {}
    for flavour, ks in (("pcl", PCL_KS), ("o3d", O3D_KS)):
        for k in ks:
            for ratio in RATIOS:
                out[flavour, k, ratio] = ref.statistical(parity_cloud, k, ratio, flavour)
    return out


@pytest.fixture(scope="module")
def planted():
    return ref.planted_cloud()


def rel_close(a, b, tol):
    return abs(a - b) <= tol * abs(b)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def stat_bits(st):
    return bits([st[key] for key in STAT_KEYS])


def check_statistical(got, want, what):
    """device result against the restatement; no point may be excused"""
    keep, d, st = got
    rkeep, rd, rst = want
    assert keep.dtype == bool and d.dtype == np.float64 and keep.shape == rd.shape == d.shape, what
    ok = ~np.isnan(rd)
    assert np.array_equal(np.isnan(d), ~ok), what
    err = (np.abs(d[ok] - rd[ok]) / np.where(rd[ok] > 0, rd[ok], 1.0)).max() if ok.any() else 0.0
    print("%s: mean_dist max relative error %.2e" % (what, err))
    assert (np.abs(d[ok] - rd[ok]) <= 1e-13 * rd[ok]).all(), what
    for key in STAT_KEYS:
        print("   %s %.17g (restatement %.17g)" % (key, st[key], rst[key]))
        assert rel_close(st[key], rst[key], 1e-12), (what, key)
    for key in ("n_points", "n_valid"):
        assert st[key] == rst[key], (what, key)
    return keep, d, st


def check_masks(got, want, flavour, what, exact=False):
    """exact: a cloud whose arithmetic is exact (every d equals the threshold): the bits must agree instead of a margin"""
    keep, d, st = got
    rkeep, rd, rst = want
    with np.errstate(invalid="ignore"):
        host = d <= st["threshold"] if flavour == "pcl" else d < st["threshold"]
    assert np.array_equal(keep, host), what                       # the device's compare is the host's compare of what it downloaded
    assert st["n_kept"] == int(keep.sum()), what
    ok = ~np.isnan(rd)
    if exact:
        assert np.array_equal(bits(d), bits(rd)) and np.array_equal(stat_bits(st), stat_bits(rst)), what
    elif ok.any() and rst["threshold"] > 0:
        margin = np.abs(rd[ok] - rst["threshold"]).min() / rst["threshold"]
        print("   the restatement's nearest d is %.2e of the threshold away" % margin)
        assert margin > 1e-9, what
    assert np.array_equal(keep, rkeep), what
    assert st["n_kept"] == rst["n_kept"], what


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("flavour,k", [("pcl", k) for k in PCL_KS] + [("o3d", k) for k in O3D_KS])
def test_parity(api, ctx, parity_cloud, parity_ref, flavour, k):
    mp = api.Map(ctx, api.Cloud(ctx, parity_cloud), 0.25)
    for ratio in RATIOS:
        what = "%s k %d ratio %g" % (flavour, k, ratio)
        got = mp.statistical_outliers(k, ratio, flavour)
        want = parity_ref[flavour, k, ratio]
        check_statistical(got, want, what)
        check_masks(got, want, flavour, what)
        if k >= 8:
            assert not got[0][-20:].any(), what                   # the isolated points go
        assert got[0][:-20].mean() > 0.8, what
    mp.close()


# ------------------------------------------------------------------ 2. independence of the cell and of the run
@pytest.mark.parametrize("flavour,k", [("pcl", 20), ("o3d", 8)])
def test_independent_of_cell_and_run(api, ctx, parity_cloud, flavour, k):
    first = None
    for cell in (0.25, 0.0, 0.15, 0.5, 1.0, 0.25):
        mp = api.Map(ctx, api.Cloud(ctx, parity_cloud), cell)
        keep, d, st = mp.statistical_outliers(k, 2.0, flavour)
        mp.close()
        if first is None:
            first = (keep, d, st)
            continue
        assert np.array_equal(bits(d), bits(first[1])), cell
        assert np.array_equal(stat_bits(st), stat_bits(first[2])), cell
        assert st == first[2] and np.array_equal(keep, first[0]), cell


# ------------------------------------------------------------------ 3. coincident and few points
def test_coincident_points(api, ctx):
    rng = np.random.default_rng(5)
    m = np.repeat(lattice(), 3, axis=0)
    m = m[rng.permutation(len(m))]
    for cell in (0.0, 1.0):
        mp = api.Map(ctx, api.Cloud(ctx, m), cell)
        keep, d, st = mp.statistical_outliers(2, 2.0, "pcl")       # the two nearest others are the two copies
        assert not d.any() and not np.signbit(d).any() and keep.all()
        assert st == dict(n_points=len(m), n_valid=len(m), n_kept=len(m), mean=0.0, stddev=0.0, threshold=0.0)
        for flavour in ("pcl", "o3d"):
            got = mp.statistical_outliers(8, 2.0, flavour)
            want = ref.statistical(m, 8, 2.0, flavour)
            check_statistical(got, want, ("lattice", cell, flavour))
            assert (want[1] == want[2]["threshold"]).all()            # whole numbers and halves throughout: <= keeps all, < none
            check_masks(got, want, flavour, ("lattice", cell, flavour), exact=True)
            assert got[0].all() == (flavour == "pcl") and got[0].any() == (flavour == "pcl")
        mp.close()


def test_few_points(api, ctx):
    rng = np.random.default_rng(8)
    one = np.array([[0.5, -1.0, 2.0]], np.float32)
    five = rng.uniform(-1, 1, (5, 3)).astype(np.float32)
    holes = rng.uniform(-1, 1, (40, 3)).astype(np.float32)
    holes[7] = [np.nan, 0.0, 0.0]
    holes[21] = [0.0, np.inf, 0.0]
    for name, m, k in (("n = 1", one, 3), ("n = 5", five, 8), ("non-finite", holes, 8)):
        mp = api.Map(ctx, api.Cloud(ctx, m), 0.25)
        for flavour in ("pcl", "o3d"):
            got = mp.statistical_outliers(k, 2.0, flavour)
            want = ref.statistical(m, k, 2.0, flavour)
            check_statistical(got, want, (name, flavour))
            check_masks(got, want, flavour, (name, flavour))
        keep, cnt, st = mp.radius_outliers(0.8, 1)
        rkeep, rcnt, rst = ref.radius(m, 0.8, 1)
        assert np.array_equal(cnt, rcnt) and np.array_equal(keep, rkeep) and st == rst, name
        mp.close()
    # what the non-finite rows get
    mp = api.Map(ctx, api.Cloud(ctx, holes), 0.25)
    keep, d, st = mp.statistical_outliers(8, 2.0, "pcl")
    assert np.isnan(d[[7, 21]]).all() and not keep[[7, 21]].any() and st["n_points"] == 40 and st["n_valid"] == 38
    keep, cnt, st = mp.radius_outliers(0.8, 0)
    assert (cnt[[7, 21]] == 0).all() and not keep[[7, 21]].any() and st["n_valid"] == 38 and keep.sum() == 38
    mp.close()
    # n = 1: the point is its own list
    mp = api.Map(ctx, api.Cloud(ctx, one), 0.0)
    keep, d, st = mp.statistical_outliers(3, 2.0, "pcl")
    assert d[0] == 0.0 and keep[0] and st["threshold"] == 0.0
    keep, d, st = mp.statistical_outliers(3, 2.0, "o3d")
    assert d[0] == 0.0 and not keep[0]                            # 0 < 0
    mp.close()


def test_empty_cloud(api, ctx):
    zero = dict(n_points=0, n_valid=0, n_kept=0, mean=0.0, stddev=0.0, threshold=0.0)
    cloud = api.Cloud(ctx, np.zeros((0, 3), np.float32))
    mp = api.Map(ctx, cloud, 0.25)
    keep, d, st = mp.statistical_outliers(20)
    assert keep.shape == (0,) and d.shape == (0,) and st == zero
    keep, cnt, st = mp.radius_outliers(0.3, 3)
    assert keep.shape == (0,) and cnt.shape == (0,) and cnt.dtype == np.int32 and st == zero
    mp.close()
    assert cloud.remove_statistical_outliers() == zero and len(cloud) == 0 and len(cloud.last_indices()) == 0
    assert cloud.remove_radius_outliers(0.3, 3) == zero and len(cloud) == 0
    cloud.close()


# ------------------------------------------------------------------ 4. radius
@pytest.mark.parametrize("cell", [0.0, 0.15, 0.25, 0.5])
def test_radius_counts(api, ctx, parity_cloud, cell):
    mp = api.Map(ctx, api.Cloud(ctx, parity_cloud), cell)
    for radius in (0.25, 0.4, 0.6):
        keep, cnt, st = mp.radius_outliers(radius, 3)
        rkeep, rcnt, rst = ref.radius(parity_cloud, radius, 3)
        assert cnt.dtype == np.int32 and np.array_equal(cnt, rcnt), (cell, radius, np.flatnonzero(cnt != rcnt)[:5])
        assert np.array_equal(keep, rkeep) and st == rst, (cell, radius)
        r2 = np.float32(radius * radius)
        assert np.array_equal(np.minimum(cnt, 64), mp.knn(parity_cloud, 64, r2)[2]), (cell, radius)
    mp.close()


@pytest.mark.parametrize("cell", [0.0, 0.25])
def test_radius_is_strict(api, ctx, parity_cloud, cell):
    """the isolated points are 0.6 m apart: at radius 0.6 some ordered pairs have d2 == r2 in float32 and must not count"""
    lone = parity_cloud[-20:]
    d2 = ref.d2_rows(lone, lone)
    r2 = np.float32(0.6 * 0.6)
    ties = int((d2 == r2).sum())
    print("ordered pairs with d2 == r2:", ties)
    assert ties == 10
    strict, loose = (d2 < r2).sum(1).astype(np.int32), (d2 <= r2).sum(1).astype(np.int32)
    assert (strict != loose).sum() >= 5                           # what a <= on the device would get wrong
    mp = api.Map(ctx, api.Cloud(ctx, parity_cloud), cell)
    keep, cnt, st = mp.radius_outliers(0.6, 1)
    mp.close()
    assert np.array_equal(cnt[-20:], strict)                      # nothing else is within 1.5 m of them
    assert np.array_equal(keep[-20:], strict > 1)


@pytest.mark.parametrize("cell", [0.5, 1.0])
def test_radius_at_a_multiple_of_the_cell(api, ctx, cell):
    m = lattice()
    mp = api.Map(ctx, api.Cloud(ctx, m), cell)
    keep, cnt, st = mp.radius_outliers(1.0, 0)                    # r2 = 1.0: the face neighbours are AT the radius
    assert (cnt == 1).all() and keep.all() and st["n_kept"] == len(m)
    keep, cnt, st = mp.radius_outliers(1.0, 1)
    assert not keep.any() and st["n_kept"] == 0
    above = float(np.sqrt(np.float64(np.nextafter(np.float32(1.0), np.float32(2.0)))))
    assert np.float32(above * above) == np.nextafter(np.float32(1.0), np.float32(2.0))
    keep, cnt, st = mp.radius_outliers(above, 4)
    faces = 1 + ((m > 0).sum(1) + (m < 3).sum(1))                 # itself and its face neighbours inside the 4 x 4 x 4 lattice
    assert np.array_equal(cnt, faces.astype(np.int32)) and np.array_equal(cnt, ref.radius_counts(m, above))
    assert np.array_equal(keep, faces > 4) and 0 < keep.sum() < len(m)
    mp.close()
    # more neighbours than sf_map_knn can list
    m3 = np.repeat(m, 3, axis=0)
    mp = api.Map(ctx, api.Cloud(ctx, m3), cell)
    keep, cnt, st = mp.radius_outliers(2.5, 100)
    rkeep, rcnt, rst = ref.radius(m3, 2.5, 100)
    assert np.array_equal(cnt, rcnt) and np.array_equal(keep, rkeep) and st == rst and cnt.max() > 64 and 0 < keep.sum() < len(m3)
    assert np.array_equal(mp.knn(m3, 64, np.float32(6.25))[2], np.minimum(cnt, 64))
    mp.close()


def test_radius_of_several_cells(api, ctx, parity_cloud):
    mp = api.Map(ctx, api.Cloud(ctx, parity_cloud), 0.25)
    radius = 3.3 * 0.25
    keep, cnt, st = mp.radius_outliers(radius, 10)
    rkeep, rcnt, rst = ref.radius(parity_cloud, radius, 10)
    assert np.array_equal(cnt, rcnt) and np.array_equal(keep, rkeep) and st == rst and cnt.max() > 30
    mp.close()


# ------------------------------------------------------------------ 5. the cloud calls
def brute_nn(m, q):
    d2 = ref.d2_rows(q, m)
    return d2.argmin(1), d2.min(1)


@pytest.mark.parametrize("which", ["statistical", "radius"])
def test_cloud_calls(api, ctx, planted, which):
    rng = np.random.default_rng(4)
    cloud = api.Cloud(ctx, planted)
    mp = api.Map(ctx, api.Cloud(ctx, planted), 0.25)
    if which == "statistical":
        st = cloud.remove_statistical_outliers(20, 2.0)
        keep, _, mst = mp.statistical_outliers(20, 2.0)
        assert stat_bits(st).tolist() == stat_bits(mst).tolist()  # the temporary index has another cell: the same numbers
    else:
        st = cloud.remove_radius_outliers(0.3, 3)
        keep, _, mst = mp.radius_outliers(0.3, 3)
    mp.close()
    assert st == mst and st["n_points"] == st["n_valid"] == len(planted) and st["n_kept"] == ref.N_SURFACE
    assert len(cloud) == ref.N_SURFACE
    assert np.array_equal(cloud.last_indices(), np.arange(ref.N_SURFACE))
    left = cloud.download()
    assert np.array_equal(left, planted[:ref.N_SURFACE]) and np.array_equal(left, planted[keep])
    # the cloud is usable afterwards
    q = (left[rng.integers(0, len(left), 200)] + rng.normal(0, 0.05, (200, 3))).astype(np.float32)
    mp = api.Map(ctx, cloud)
    idx, d2 = mp.nn(q)
    bi, bd = brute_nn(left, q)
    assert np.array_equal(d2, bd) and np.array_equal(ref.d2_rows(q, left)[np.arange(200), idx], bd)
    mp.close()
    if which == "statistical":                                     # the O3D flavour and an explicit cell, on what is left
        st = cloud.remove_statistical_outliers(nb_neighbors=20, std_ratio=2.0, flavour="o3d", cell=0.5)
        rkeep, _, rst = ref.statistical(left, 20, 2.0, "o3d")
        assert st["n_kept"] == rst["n_kept"] == len(cloud) and np.array_equal(cloud.last_indices(), np.flatnonzero(rkeep))
    cloud.close()


# ------------------------------------------------------------------ 6. arguments
def test_arguments(api, ctx, parity_cloud):
    mp = api.Map(ctx, api.Cloud(ctx, parity_cloud), 0.25)
    cloud = api.Cloud(ctx, parity_cloud)
    good = mp.statistical_outliers(8, 2.0, "pcl")
    good_r = mp.radius_outliers(0.4, 3)

    def still_fine():
        again = mp.statistical_outliers(8, 2.0, "pcl")
        assert np.array_equal(again[0], good[0]) and np.array_equal(bits(again[1]), bits(good[1])) and again[2] == good[2]
        assert len(cloud) == len(parity_cloud)

    for k, flavour in ((0, "pcl"), (64, "pcl"), (0, "o3d"), (65, "o3d"), (8, 2), (-3, "pcl")):
        with pytest.raises(api.SlamFusionError):
            mp.statistical_outliers(k, 2.0, flavour)
        with pytest.raises(api.SlamFusionError):
            cloud.remove_statistical_outliers(k, 2.0, flavour)
        still_fine()
    for radius, min_nb in ((0.0, 3), (-1.0, 3), (np.nan, 3), (np.inf, 3), (0.4, -1)):
        with pytest.raises(api.SlamFusionError):
            mp.radius_outliers(radius, min_nb)
        with pytest.raises(api.SlamFusionError):
            cloud.remove_radius_outliers(radius, min_nb)
        still_fine()
    assert mp.statistical_outliers(63, 2.0, "pcl")[2]["n_valid"] == len(parity_cloud)       # the largest k of either flavour
    assert mp.statistical_outliers(64, 2.0, "o3d")[2]["n_valid"] == len(parity_cloud)
    unbuilt = api.Map(ctx)
    with pytest.raises(api.SlamFusionError):
        unbuilt.statistical_outliers(8)
    with pytest.raises(api.SlamFusionError):
        unbuilt.radius_outliers(0.4, 3)
    unbuilt.build(api.Cloud(ctx, parity_cloud), 0.25)
    assert unbuilt.radius_outliers(0.4, 3)[2] == good_r[2]
    unbuilt.close()
    # a window on the map changes nothing
    mp.window_sphere(parity_cloud[0], 1.0)
    assert 0 < mp.window_count() < len(parity_cloud)
    still_fine()
    keep, cnt, st = mp.radius_outliers(0.4, 3)
    assert np.array_equal(keep, good_r[0]) and np.array_equal(cnt, good_r[1]) and st == good_r[2]
    mp.close()
    cloud.close()


# ------------------------------------------------------------------ 7. nothing else moved
def test_the_map_is_left_as_it_was(api, ctx, parity_cloud):
    mp = api.Map(ctx, api.Cloud(ctx, parity_cloud), 0.25)
    mp.estimate_normals_knn(20, covariance=True)
    mp.build_neighbour_table()

    def state():
        ix = mp.index()
        nrm, cnt = mp.download_normals()
        ids, r = mp.download_neighbour_table()
        return [nrm.view(np.uint32), cnt, mp.download_covariances().view(np.uint64), ids, r.view(np.uint32), ix["pts4"].view(np.uint32), ix["cell_start"],
                ix["org"].view(np.uint32), np.float32(ix["inv_h"]).view(np.uint32), np.float32(ix["gap_eps"]).view(np.uint32)]

    before = state()
    mp.statistical_outliers(20, 2.0, "pcl")
    mp.statistical_outliers(20, 1.0, "o3d")
    mp.radius_outliers(0.4, 3)
    after = state()
    assert len(before) == len(after)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert mp.neighbour_table_info()["present"]
    mp.close()


def test_launch_time_is_recorded(api, ctx, parity_cloud):
    mp = api.Map(ctx, api.Cloud(ctx, parity_cloud), 0.25)
    mp.profile_launches(True)
    with pytest.raises(api.SlamFusionError):
        mp.last_launch_ms()
    mp.statistical_outliers(20)
    a = mp.last_launch_ms()
    mp.radius_outliers(0.4, 3)
    b = mp.last_launch_ms()
    assert 0.0 < a < 5000.0 and 0.0 < b < 5000.0
    mp.close()
