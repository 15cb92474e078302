"""sf_map_radius_search / sf_map_radius_graph on the device against the brute-force numpy restatement of their rule
(tests/radius_ref_np.py, pinned to scipy by tests/test_radius_rule.py).  Everything is compared with np.array_equal --
offsets, idx and d2 -- in both orders and in both fill forms: the rule is float32 and strict on both sides, nothing is excused."""
import ctypes as C

import numpy as np
import pytest

import radius_ref_np as ref
from test_gpu_knn import mixed_map, obb_accept, sphere_accept
from test_gpu_knn_normals import noisy_map  # noqa: F401  (the fixture: [1] is 3 000 mixed points plus 20 isolated ones)
from test_radius_rule import parity_world

pytestmark = pytest.mark.gpu

ORDERS = ("index", "distance")
FILLS = ("lane", "wave", "auto")
SF_ERR_INVALID, SF_ERR_STATE, SF_ERR_OVERFLOW = -1, -4, -5


def same(got, want, what):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float32, what
    assert np.array_equal(got[0], want[0]), (what, "offsets", np.flatnonzero(np.diff(got[0]) != np.diff(want[0]))[:5])
    assert np.array_equal(got[1], want[1]), (what, "idx", np.flatnonzero(got[1] != want[1])[:5])
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), (what, "d2", np.flatnonzero(got[2] != want[2])[:5])


def check(mp, q, radius, accept=None, what=None, fills=FILLS, orders=ORDERS):
    """every order in every fill form against the restatement; -> the stats of the last call"""
    st = None
    for order in orders:
        want = ref.radius_ref(mp, q, radius, order, accept)
        counts = np.diff(want[0])
        for fill in fills:
            mp.set_radius_fill(fill)
            got = mp.radius_search(q, radius, order)
            same(got, want, (what, radius, order, fill))
            st = got[3]
            finite = int(np.isfinite(np.asarray(q, np.float32).reshape(-1, 3)).all(1).sum()) if len(mp) else 0
            assert st == dict(n_queries=len(counts), n_searched=finite, n_empty=int((counts == 0).sum()), total=int(want[0][-1]),
                              max_count=int(counts.max()) if len(counts) else 0), (what, radius, order, fill, st)
    mp.set_radius_fill("auto")
    return st


def call(api, fn, *args):
    """a C call's return code, without the wrapper's exception"""
    return getattr(api.load_library(), fn)(*args)


# ------------------------------------------------------------------ 1. parity
@pytest.fixture(scope="module")
def world():
    m, q = parity_world()
    return m, np.concatenate([q, np.array([[np.nan, 0, 0], [0, -np.inf, 1]], np.float32)])


@pytest.mark.parametrize("cell", [0.0, 0.15, 0.25, 0.5])
def test_parity(api, ctx, world, cell):
    m, q = world
    mp = api.Map(ctx, api.Cloud(ctx, m), cell)
    for radius in (0.3, 0.75, 2.0, 5.0):
        st = check(mp, q, radius, what=cell)
        if radius == 5.0:
            off = mp.radius_search(q, radius)[0]
            assert st["total"] == 646973 and (np.diff(off)[:-2] > 64).all() and (np.diff(off)[-2:] == 0).all()
    mp.close()


# ------------------------------------------------------------------ 2. exact row lengths
@pytest.fixture(scope="module")
def clusters():
    """cluster k = k points within 1 mm of each other, k = 0 .. 130, the centres 10 m apart on a 12 x 11 lattice"""
    rng = np.random.default_rng(127)
    k = np.arange(131)
    centres = np.stack([10.0 * (k % 12), 10.0 * (k // 12), np.zeros(131)], 1).astype(np.float32)
    pts = np.concatenate([centres[i] + rng.uniform(-2.5e-4, 2.5e-4, (i, 3)) for i in k]).astype(np.float32)
    return centres, pts[rng.permutation(len(pts))]


@pytest.mark.parametrize("cell", [0.0, 0.5])
def test_exact_row_lengths(api, ctx, clusters, cell):
    centres, pts = clusters
    mp = api.Map(ctx, api.Cloud(ctx, pts), cell)
    for order in ORDERS:
        for fill in FILLS:
            mp.set_radius_fill(fill)
            off, idx, d2, st = mp.radius_search(centres, 0.1, order)
            assert np.array_equal(np.diff(off), np.arange(131)), (cell, order, fill)           # trips of four, a wave's 63 / 64 / 65
            assert st["max_count"] == 130 and st["n_empty"] == 1 and st["total"] == 130 * 131 // 2
    check(mp, centres, 0.1, what=("clusters", cell))
    for n in (1, 63, 64, 65, 257):                                                             # the workgroup edge
        q = np.resize(centres, (n, 3))
        check(mp, q, 0.1, what=("clusters", cell, n))
        assert np.array_equal(np.diff(mp.radius_search(q, 0.1)[0]), np.arange(n) % 131)
    mp.close()


# ------------------------------------------------------------------ 3. queries outside the grid
@pytest.mark.parametrize("cell", [0.0, 0.25])
def test_outside_the_grid(api, ctx, cell):
    rng = np.random.default_rng(3)
    m = rng.uniform(-2, 2, (2000, 3)).astype(np.float32)
    face = rng.uniform(-2, 2, (6, 40, 3)).astype(np.float32)
    for a in range(3):
        face[2 * a, :, a], face[2 * a + 1, :, a] = -2.0, 2.0                                  # points ON all six faces of the bounding box
    m = np.concatenate([m, face.reshape(-1, 3)])
    mp = api.Map(ctx, api.Cloud(ctx, m), cell)
    far = []
    for a in range(3):
        for v in (1e4, -1e4, 3e38, -3e38):
            p = np.zeros(3, np.float32)
            p[a] = v
            far.append(p)
    far = np.array(far, np.float32)
    for radius in (0.3, 2.0):
        near = []
        for f in range(6):
            a, sign = f // 2, (-1.0 if f % 2 == 0 else 1.0)
            for p in face[f, :5]:
                for d in (radius * (1 - 1e-3), radius * (1 + 1e-3)):                          # just inside / just outside of the nearest point
                    x = p.astype(np.float64)
                    x[a] += sign * d
                    near.append(x)
        near = np.array(near, np.float32)
        q = np.concatenate([near, far])
        check(mp, q, radius, what=("outside", cell))
        off = mp.radius_search(q, radius)[0]
        counts = np.diff(off)
        assert (counts[len(near):] == 0).all()
        assert (counts[:len(near):2] >= 1).all() and (counts[:len(near)] > 0).sum() < len(near)   # the inside ones hold their point; some outside ones hold nothing
    mp.close()


# ------------------------------------------------------------------ 4. windows
@pytest.mark.parametrize("window", ["sphere", "obb"])
def test_windows(api, ctx, world, window):
    m, q = world
    mp = api.Map(ctx, api.Cloud(ctx, m), 0.25)
    centre = np.array([1.0, -0.5, 0.25], np.float32)
    if window == "sphere":
        mp.window_sphere(centre, 4.0)
        accept = lambda P: sphere_accept(P, centre, 4.0)
    else:
        R = np.array([[0.9, -0.3, 0.05], [0.35, 0.95, 0.0], [0.0, 0.1, 1.1]])                  # not orthonormal
        ext = (9.0, 7.0, 5.0)
        mp.window_obb(centre.astype(np.float64), R, ext)
        accept = lambda P: obb_accept(P, centre.astype(np.float64), R, ext)
    for radius in (0.75, 2.0):
        st = check(mp, q, radius, accept, what=window)
        assert 0 < st["total"] < ref.radius_ref(mp, q, radius)[0][-1]                          # the window took something away
    # the graph ignores the window
    same(mp.radius_graph(0.75), ref.radius_ref(mp, m, 0.75), (window, "graph"))
    mp.close()


# ------------------------------------------------------------------ 5. hybrid
def test_hybrid_route(api, ctx, world):
    m, q = world
    mp = api.Map(ctx, api.Cloud(ctx, m), 0.25)
    for radius in (0.3, 2.0, 5.0):
        r2 = np.float32(radius * radius)
        off, idx, d2, _ = mp.radius_search(q, radius, "distance")
        ki, kd, kc = mp.knn(q, 64, r2)
        ci, cd, cc = ref.rows_cut(off, idx, d2, 64)
        assert np.array_equal(cc, kc) and np.array_equal(cd, kd) and np.array_equal(ci, ki), radius
        for max_nn in (1, 20, 64):
            hi, hd, hc = mp.hybrid_search(q, radius, max_nn)
            ki, kd, kc = mp.knn(q, max_nn, r2)
            assert np.array_equal(hi, ki) and np.array_equal(hd, kd) and np.array_equal(hc, kc), (radius, max_nn)
    for max_nn in (0, 65, -3):
        with pytest.raises(ValueError):
            mp.hybrid_search(q, 1.0, max_nn)
    mp.close()


# ------------------------------------------------------------------ 6. graph
def test_graph(api, ctx, noisy_map):  # noqa: F811
    x = noisy_map[1].copy()
    x = np.concatenate([x[:1000], np.full((1, 3), np.nan, np.float32), x[1000:], np.array([[0, np.nan, 1]], np.float32), np.repeat(x[17:18], 3, 0)]).astype(np.float32)
    nan_rows = np.flatnonzero(~np.isfinite(x).all(1))
    assert len(nan_rows) == 2
    for cell in (0.0, 0.25):
        mp = api.Map(ctx, api.Cloud(ctx, x), cell)
        for radius in (0.2, 0.6):
            _, n_nb, _ = mp.radius_outliers(radius, 0)
            for order in ORDERS:
                want = ref.radius_ref(mp, x, radius, order)
                for fill in FILLS:
                    mp.set_radius_fill(fill)
                    got = mp.radius_graph(radius, order)
                    what = ("graph", cell, radius, order, fill)
                    same(got, want, what)
                    same(mp.radius_search(x, radius, order), want, what + ("search",))
                    off, idx, d2, st = got
                    assert np.array_equal(np.diff(off), n_nb), what
                    assert st["n_queries"] == len(x) and st["n_searched"] == len(x) - 2 and st["n_empty"] == 2 and st["max_count"] == n_nb.max(), what
                    assert (np.diff(off)[nan_rows] == 0).all() and not np.isin(idx, nan_rows).any(), what
                    rows = np.repeat(np.arange(len(x)), np.diff(off))
                    fwd = np.unique(rows * len(x) + idx)
                    assert len(fwd) == len(idx) and np.array_equal(fwd, np.unique(idx.astype(np.int64) * len(x) + rows)), what   # j in row i exactly when i in row j
                    assert (d2[rows == idx] == 0).all() and (rows == idx).sum() == len(x) - 2, what                             # every indexed point holds itself
        mp.close()


# ------------------------------------------------------------------ 7. limits and state
def test_overflow_leaves_the_map_usable(api, ctx):
    rng = np.random.default_rng(66)
    x = rng.uniform(0, 1, (66000, 3)).astype(np.float32)
    mp = api.Map(ctx, api.Cloud(ctx, x), 0.25)
    off = np.zeros(len(x) + 1, np.int64)
    st = api.RadiusStats()
    for order in (0, 1):
        assert call(api, "sf_map_radius_graph", mp.h, C.c_double(10.0), C.c_int(order), off.ctypes.data_as(C.c_void_p), C.byref(st)) == SF_ERR_OVERFLOW   # 66 000^2 > 2^32
        total = C.c_int64(-7)
        assert call(api, "sf_map_radius_results", mp.h, None, None, C.c_int64(0), C.byref(total)) == SF_ERR_STATE and total.value == 0
    with pytest.raises(api.SlamFusionError):
        mp.radius_graph(10.0)
    check(mp, x[:300], 0.05, what="after the overflow")
    mp.close()


def test_state_and_arguments(api, ctx, world):
    m, q = world
    mp = api.Map(ctx)
    total = C.c_int64(-7)
    none = api.RadiusStats()
    assert call(api, "sf_map_radius_search", mp.h, q.ctypes.data_as(C.c_void_p), C.c_int64(4), C.c_double(1.0), C.c_int(0), None, C.byref(none)) == SF_ERR_STATE   # not built
    assert call(api, "sf_map_radius_graph", mp.h, C.c_double(1.0), C.c_int(0), None, None) == SF_ERR_STATE
    cloud = api.Cloud(ctx, m)
    mp.build(cloud, 0.25)
    assert call(api, "sf_map_radius_results", mp.h, None, None, C.c_int64(0), C.byref(total)) == SF_ERR_STATE and total.value == 0   # no call so far
    off, idx, d2, st = mp.radius_search(q, 0.75)
    assert call(api, "sf_map_radius_results", mp.h, None, None, C.c_int64(0), C.byref(total)) == 0 and total.value == st["total"] > 0
    gi, gd = np.full(st["total"], -9, np.int32), np.full(st["total"], -9, np.float32)
    total = C.c_int64(-7)
    assert call(api, "sf_map_radius_results", mp.h, gi.ctypes.data_as(C.c_void_p), gd.ctypes.data_as(C.c_void_p), C.c_int64(st["total"] - 1), C.byref(total)) == SF_ERR_INVALID
    assert total.value == st["total"] and (gi == -9).all() and (gd == -9).all()              # one short: total set, nothing written
    assert call(api, "sf_map_radius_results", mp.h, gi.ctypes.data_as(C.c_void_p), None, C.c_int64(st["total"]), C.byref(total)) == 0 and np.array_equal(gi, idx)
    assert call(api, "sf_map_radius_results", mp.h, None, gd.ctypes.data_as(C.c_void_p), C.c_int64(st["total"]), C.byref(total)) == 0 and np.array_equal(gd, d2)
    # offsets may be NULL; the lists are there all the same
    assert call(api, "sf_map_radius_search", mp.h, q.ctypes.data_as(C.c_void_p), C.c_int64(len(q)), C.c_double(0.75), C.c_int(1), None, None) == 0
    assert call(api, "sf_map_radius_results", mp.h, None, None, C.c_int64(0), C.byref(total)) == 0 and total.value == st["total"]
    for radius in (0.0, -1.0, np.nan, np.inf, -np.inf, 1e30):                                 # 1e30: its float32 square is not finite
        assert call(api, "sf_map_radius_search", mp.h, q.ctypes.data_as(C.c_void_p), C.c_int64(len(q)), C.c_double(radius), C.c_int(0), None, None) == SF_ERR_INVALID, radius
        assert call(api, "sf_map_radius_graph", mp.h, C.c_double(radius), C.c_int(0), None, None) == SF_ERR_INVALID, radius
    for order in (2, -1, 7):
        assert call(api, "sf_map_radius_search", mp.h, q.ctypes.data_as(C.c_void_p), C.c_int64(len(q)), C.c_double(0.5), C.c_int(order), None, None) == SF_ERR_INVALID, order
        assert call(api, "sf_map_radius_graph", mp.h, C.c_double(0.5), C.c_int(order), None, None) == SF_ERR_INVALID, order
    with pytest.raises(api.SlamFusionError):
        mp.radius_search(q, 0.5, order=3)
    for mode in (-1, 3):
        assert call(api, "sf_map_set_radius_fill", mp.h, C.c_int(mode)) == SF_ERR_INVALID
    # an empty query set
    off, idx, d2, st = mp.radius_search(np.zeros((0, 3), np.float32), 0.5)
    assert np.array_equal(off, [0]) and idx.shape == (0,) and d2.shape == (0,) and st == dict(n_queries=0, n_searched=0, n_empty=0, total=0, max_count=0)
    # build drops the lists
    mp.radius_search(q, 0.75)
    mp.build(cloud, 0.25)
    assert call(api, "sf_map_radius_results", mp.h, None, None, C.c_int64(0), C.byref(total)) == SF_ERR_STATE and total.value == 0
    assert mp.radius_launch_ms() == (0.0, 0.0, 0.0)                                           # nothing timed: profiling is off
    mp.profile_launches(True)
    mp.radius_search(q, 2.0, "distance")
    ms = mp.radius_launch_ms()
    assert all(v > 0 for v in ms) and abs(mp.last_launch_ms() - sum(ms)) < 1e-3
    mp.close()
    # an empty map
    mp = api.Map(ctx, api.Cloud(ctx, np.zeros((0, 3), np.float32)), 0.25)
    for order in ORDERS:
        off, idx, d2, st = mp.radius_search(q, 0.5, order)
        assert np.array_equal(off, np.zeros(len(q) + 1, np.int64)) and len(idx) == 0 and st == dict(n_queries=len(q), n_searched=0, n_empty=len(q), total=0, max_count=0)
        off, idx, d2, st = mp.radius_graph(0.5, order)
        assert np.array_equal(off, [0]) and len(idx) == 0 and st["total"] == 0
    mp.close()


def test_patch_drops_the_lists(api, ctx, synth):
    """both ways sf_map_patch can go -- the index merged over the growth step, and the build it falls back to -- leave no lists"""
    rng = np.random.default_rng(43)
    prev = api.voxel_merge_min_points(0)
    try:
        base = synth.make_map(60_000)
        inner = base[(np.abs(base[:, 0]) < 5.0) & (np.abs(base[:, 1]) < 5.0)]
        dev = api.Cloud(ctx, inner)
        dev.voxel_downsample(0.1, "pcl")
        core = inner[(np.abs(inner[:, 0]) < 4.5) & (np.abs(inner[:, 1]) < 4.5) & (np.abs(inner[:, 2]) < 4.5)]
        near = lambda n: (core[rng.choice(len(core), n, replace=False)] + rng.normal(0, 0.004, (n, 3))).astype(np.float32)
        mp = api.Map(ctx).set_origin_lattice(64).build(dev, 0.25)
        q = near(300)
        total = C.c_int64(-7)
        for merged_path in (True, False):
            _, _, _, st = mp.radius_search(q, 0.3)
            assert call(api, "sf_map_radius_results", mp.h, None, None, C.c_int64(0), C.byref(total)) == 0 and total.value == st["total"] > 0
            _, merged = dev.voxel_merge(api.Cloud(ctx, near(500)), 0.1)
            assert merged
            if not merged_path:
                dev.transform(np.eye(4, dtype=np.float32))                                   # the cloud was touched: the patch takes the build
            assert mp.patch(dev) == merged_path
            assert call(api, "sf_map_radius_results", mp.h, None, None, C.c_int64(0), C.byref(total)) == SF_ERR_STATE and total.value == 0
            check(mp, q, 0.3, what=("after the patch", merged_path))                         # ... and the next call sees the patched index
        mp.close()
    finally:
        api.voxel_merge_min_points(prev)


# ------------------------------------------------------------------ 8. repeatability
def test_repeatable_and_independent_of_the_cell(api, ctx, world):
    m, q = world
    base = None
    for cell in (0.0, 0.15, 0.5):
        mp = api.Map(ctx, api.Cloud(ctx, m), cell)
        a = mp.radius_search(q, 2.0, "distance")
        b = mp.radius_search(q, 2.0, "distance")
        same(a, b, ("twice", cell))
        assert a[3] == b[3]
        g1, g2 = mp.radius_graph(0.75, "index"), mp.radius_graph(0.75, "index")
        same(g1, g2, ("graph twice", cell))
        off, idx, d2, _ = a
        rows = np.repeat(np.arange(len(q)), np.diff(off))
        ids = idx[np.lexsort((idx, rows))]                                                      # the id set of every row
        if base is None:
            base = (off, ids, d2)
        else:                                                                                   # other cells: another position order among equal d2, nothing else
            assert np.array_equal(off, base[0]) and np.array_equal(ids, base[1]) and np.array_equal(d2, base[2]), cell
        mp.close()
