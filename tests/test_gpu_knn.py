"""sf_map_knn against a brute-force numpy restatement of its rule: the candidates of a query are the indexed points the window
accepts with float32 d2 = ((dx*dx)+dy*dy)+dz*dz < max_d2 (strict), ordered by the 64-bit key (bits of d2) << 32 | position in
the index; the first k are the result.  idx, d2 and count are compared with np.array_equal."""
import os

import numpy as np
import pytest

from reuse_ref_np import obb_accept, sphere_accept   # (the window's accept rule: shared with tests/test_gpu_reuse_bound.py)

pytestmark = pytest.mark.gpu


def knn_ref(mp, q, k, max_d2=np.inf, accept=None, positions=False):
    """-> idx [n, k] (original ids, or index positions), d2 [n, k], count [n]; `accept` takes the points in index order."""
    pts4 = mp.index()["pts4"]
    P = np.ascontiguousarray(pts4[:, :3])
    ids = pts4[:, 3].view(np.uint32).astype(np.int64)
    q = np.asarray(q, np.float32).reshape(-1, 3)
    n, m = len(q), len(P)
    idx = np.full((n, k), -1, np.int32)
    d2 = np.full((n, k), np.inf, np.float32)
    cnt = np.zeros(n, np.int32)
    if m == 0 or n == 0:
        return idx, d2, cnt
    ok_pt = np.ones(m, bool) if accept is None else accept(P)
    pos = np.arange(m, dtype=np.uint64)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, n, 256):
            c = q[s:s + 256]
            dx, dy, dz = (c[:, None, d] - P[None, :, d] for d in range(3))
            d = ((dx * dx) + dy * dy) + dz * dz
            assert d.dtype == np.float32
            ok = (d < np.float32(max_d2)) & ok_pt[None, :] & np.isfinite(c).all(1)[:, None]
            key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | pos[None, :]
            key[~ok] = np.uint64(0xFFFFFFFFFFFFFFFF)
            order = np.argsort(key, axis=1, kind="stable")[:, :k]
            kk = order.shape[1]
            took = np.take_along_axis(ok, order, 1)
            cnt[s:s + 256] = took.sum(1)
            idx[s:s + 256, :kk] = np.where(took, order if positions else ids[order], -1)
            d2[s:s + 256, :kk] = np.where(took, np.take_along_axis(d, order, 1), np.inf)
    return idx, d2, cnt


def check(mp, q, k, max_d2=np.inf, accept=None, what=None):
    gi, gd, gc = mp.knn(q, k, max_d2)
    ri, rd, rc = knn_ref(mp, q, k, max_d2, accept)
    assert gi.shape == ri.shape and gi.dtype == np.int32 and gd.dtype == np.float32 and gc.dtype == np.int32, what
    assert np.array_equal(gc, rc), (what, "count", np.flatnonzero(gc != rc)[:5], gc[gc != rc][:5], rc[gc != rc][:5])
    assert np.array_equal(gd, rd), (what, "d2", np.argwhere(gd != rd)[:5])
    assert np.array_equal(gi, ri), (what, "idx", np.argwhere(gi != ri)[:5])
    return gi, gd, gc


def mixed_map(rng, n, sigma=0.0):
    """half uniform in a +-6 m box, half on the planes z = 0 and x = 2 (the planes of the fuzz in test_gpu_parity.py)"""
    m = rng.uniform(-6, 6, (n, 3))
    a, b = n // 2, n // 2 + n // 4
    m[a:b, 2] = rng.normal(0, sigma, b - a) if sigma else 0.0
    m[b:, 0] = 2.0 + (rng.normal(0, sigma, n - b) if sigma else 0.0)
    return m.astype(np.float32)


def queries_near(rng, m, n, noise=0.2):
    return (m[rng.integers(0, len(m), n)] + rng.normal(0, noise, (n, 3))).astype(np.float32)


@pytest.mark.parametrize("window", ["none", "sphere", "obb"])
def test_k1_equals_map_nn_bitwise(api, ctx, small_world, window):
    m, scan = small_world["map"], small_world["scan"]
    mp = api.Map(ctx, api.Cloud(ctx, m), 0.25)
    q = np.concatenate([scan[:600], np.array([[np.nan, 0, 0], [0, np.inf, 0]], np.float32),
                        np.array([[1000, 0, 0], [-1000, 3, 1], [0, 1000, 0], [2, -1000, 0], [1, 2, 1000], [0, 0, -1000]], np.float32), m[::997][:20]]).astype(np.float32)
    centre = scan.mean(0)
    accept = None
    if window == "sphere":
        mp.window_sphere(centre, 6.0)
        accept = lambda P: sphere_accept(P, centre, 6.0)
    elif window == "obb":
        R = np.array([[0.9, -0.3, 0.05], [0.35, 0.95, 0.0], [0.0, 0.1, 1.1]])          # not orthonormal
        ext = (9.0, 7.0, 5.0)
        mp.window_obb(centre.astype(np.float64), R, ext)
        accept = lambda P: obb_accept(P, centre.astype(np.float64), R, ext)
    for max_d2 in (np.inf, 0.25):
        ni, nd = mp.nn(q, max_d2)
        gi, gd, gc = check(mp, q, 1, max_d2, accept, (window, max_d2))
        assert np.array_equal(gi[:, 0], ni) and np.array_equal(gd[:, 0], nd), (window, max_d2)
        assert np.array_equal(gc, (ni >= 0).astype(np.int32))
        assert (gc[600:602] == 0).all() and (0 < gc.sum() < len(q) or max_d2 == np.inf)
    mp.close()


@pytest.mark.parametrize("cell", [0.0, 0.15, 0.25, 0.5])
def test_general_parity(api, ctx, cell):
    rng = np.random.default_rng(11)
    m = mixed_map(rng, 4000)
    mp = api.Map(ctx, api.Cloud(ctx, m), cell)
    q = np.concatenate([queries_near(rng, m, 200), rng.uniform(-7, 7, (57, 3)).astype(np.float32)])
    for k in (1, 2, 7, 20, 63, 64):
        for n in (1, 63, 64, 65, 257):
            check(mp, q[:n], k, what=(cell, k, n))
    mp.close()


def lattice():
    g = np.arange(4, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


@pytest.mark.parametrize("copies", [1, 3])
def test_ties_are_settled_by_the_index_position(api, ctx, copies):
    rng = np.random.default_rng(5)
    m = np.repeat(lattice(), copies, axis=0)
    m = m[rng.permutation(len(m))]
    for cell in (0.0, 0.5, 1.0):
        mp = api.Map(ctx, api.Cloud(ctx, m), cell)
        q = np.array([[1.5, 1.5, 1.5], [1.0, 2.0, 1.0], [0.0, 0.0, 0.0], [3.0, 3.0, 3.0]], np.float32)
        _, rd, _ = knn_ref(mp, q[:1], 32 * copies if 32 * copies <= 64 else 64)
        assert (rd[0, :8 * copies] == 0.75).all() and (copies > 1 or (rd[0, 8:32] == 2.75).all())   # the tie groups the case is about
        for k in (5, 8, 10, 32):
            check(mp, q, k, what=(copies, cell, k))
        mp.close()


@pytest.mark.parametrize("k", [20, 64])
def test_selection_under_pressure(api, ctx, k):
    rng = np.random.default_rng(3)
    dense = (rng.uniform(0.01, 0.24, (600, 3)) + [1.0, 1.0, 1.0]).astype(np.float32)        # inside one 0.25 m cell
    scattered = rng.uniform(-2, 4, (50, 3)).astype(np.float32)
    scattered[0] = -2.0                 # the grid starts at the smallest coordinates: with this corner, 1.0 is the edge of cell 12 on every axis
    m = np.concatenate([dense, scattered])
    mp = api.Map(ctx, api.Cloud(ctx, m), 0.25)
    ix = mp.index()
    assert (ix["org"] == -2.0).all() and ix["inv_h"] == 4.0
    assert np.diff(ix["cell_start"].astype(np.int64)).max() >= 600                          # one range holds them all
    q = np.concatenate([queries_near(rng, dense, 40, 0.05), queries_near(rng, m, 24, 0.5)])
    check(mp, q, k, what=k)
    # candidates arriving in descending order of distance: every trip displaces the whole selection
    far = np.array([[1.125, 1.125, 30.0]], np.float32)
    check(mp, far, k, what=(k, "far"))
    mp.close()


def test_few_points_many_rings(api, ctx):
    rng = np.random.default_rng(8)
    m = rng.uniform(0, 10, (200, 3)).astype(np.float32)
    mp = api.Map(ctx, api.Cloud(ctx, m), 0.25)
    q = queries_near(rng, m, 20, 1.0)
    _, rd, _ = knn_ref(mp, q, 64)
    assert np.sqrt(rd[:, 63]).min() > 10 * 0.25                                             # the k-th neighbour is tens of rings out
    check(mp, q, 64, what="sparse")
    out = np.array([10.0, 5.0, 5.0], np.float32) + np.outer(np.linspace(3, 30, 10), [1.0, 0.2, -0.1]).astype(np.float32)
    check(mp, out, 64, what="outside")
    check(mp, out, 3, 16.0, what="outside, thresholded")
    mp.close()
    # fewer points than k
    m5 = rng.uniform(-1, 1, (5, 3)).astype(np.float32)
    mp = api.Map(ctx, api.Cloud(ctx, m5), 0.25)
    gi, gd, gc = check(mp, queries_near(rng, m5, 9, 0.3), 8, what="m = 5")
    assert (gc == 5).all() and (gi[:, 5:] == -1).all() and np.isinf(gd[:, 5:]).all() and (np.sort(gi[:, :5], 1) == np.arange(5)).all()
    mp.close()
    # a map flat in z
    flat = rng.uniform(-3, 3, (1500, 3)).astype(np.float32)
    flat[:, 2] = 0.5
    mp = api.Map(ctx, api.Cloud(ctx, flat), 0.25)
    assert mp.cell_size()[1][2] == 1
    check(mp, np.concatenate([queries_near(rng, flat, 60, 0.3), queries_near(rng, flat, 20, 3.0)]), 20, what="flat")
    mp.close()


def test_threshold_is_strict(api, ctx):
    rng = np.random.default_rng(21)
    m = mixed_map(rng, 2000)
    mp = api.Map(ctx, api.Cloud(ctx, m), 0.25)
    q = queries_near(rng, m, 50)
    _, rd, _ = knn_ref(mp, q, 4)
    use = np.flatnonzero((rd[:, 1] < rd[:, 2]) & (rd[:, 2] < rd[:, 3]))
    assert len(use) >= 10
    for i in use[:10]:
        gi, gd, gc = check(mp, q[i:i + 1], 8, float(rd[i, 2]), what=int(i))
        assert gc[0] == 2 and gi[0, 2] == -1
        assert mp.knn(q[i:i + 1], 8, float(np.nextafter(rd[i, 2], np.float32(np.inf))))[2][0] == 3
    mp.close()


def test_arguments(api, ctx):
    rng = np.random.default_rng(2)
    m = mixed_map(rng, 500)
    mp = api.Map(ctx, api.Cloud(ctx, m), 0.25)
    q = queries_near(rng, m, 10)
    for k in (0, 65, -1):
        with pytest.raises(api.SlamFusionError):
            mp.knn(q, k)
        check(mp, q, 3, what=("usable after", k))
    gi, gd, gc = mp.knn(np.zeros((0, 3), np.float32), 5)
    assert gi.shape == (0, 5) and gd.shape == (0, 5) and gc.shape == (0,)
    for k in (0, 65, -1):
        with pytest.raises(api.SlamFusionError):
            mp.estimate_normals_knn(k)
    mp.close()


def test_seeded_fuzz(api, ctx):
    seed = int(os.environ.get("SF_FUZZ_SEED", "91"))
    rng = np.random.default_rng(seed)
    for trial in range(int(os.environ.get("SF_FUZZ_TRIALS", "12"))):
        n = int(rng.integers(50, 3001))
        m = mixed_map(rng, n) if trial % 3 else np.round(mixed_map(rng, n) * 8) / np.float32(8)
        cell = float(rng.choice([0.0, 0.15, 0.25, 0.5]))
        k = int(rng.integers(1, 65))
        max_d2 = float(rng.choice([np.inf, 0.05, 0.5]))
        mp = api.Map(ctx, api.Cloud(ctx, m), cell)
        accept = None
        if rng.integers(0, 2):
            c, r = rng.uniform(-3, 3, 3).astype(np.float32), float(rng.uniform(1.0, 6.0))
            mp.window_sphere(c, r)
            accept = lambda P, c=c, r=r: sphere_accept(P, c, r)
        q = np.concatenate([queries_near(rng, m, 150, float(rng.choice([0.001, 0.1, 1.0]))), rng.uniform(-8, 8, (50, 3)).astype(np.float32)])
        check(mp, q, k, max_d2, accept, "trial %d of seed %d: n %d cell %g k %d max_d2 %g window %s" % (trial, seed, n, cell, k, max_d2, accept is not None))
        mp.close()


def test_determinism_and_independence_of_the_batch(api, ctx, small_world):
    m, scan = small_world["map"], small_world["scan"]
    mp = api.Map(ctx, api.Cloud(ctx, m), 0.25)
    q = scan[:600]
    a = mp.knn(q, 20, 0.5)
    b = mp.knn(q, 20, 0.5)
    parts = [mp.knn(q[s:s + 200], 20, 0.5) for s in (0, 200, 400)]
    for x, y, z in zip(a, b, [np.concatenate([p[i] for p in parts]) for i in range(3)]):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert a[2].max() == 20
    mp.close()
