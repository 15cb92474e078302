"""Plane segmentation on the device (sf_cloud_plane_hypotheses, sf_cloud_score_planes, sf_cloud_segment_plane, sf_cloud_remove_plane,
sf_test_plane_score) against the numpy restatement of the rule (tests/plane_ref_np.py), which
tests/test_plane_rule.py pins to independent code.  Hypotheses, samples, counts, the choice and the masks are compared exactly; the
refitted plane, a float64 result that differs from the restatement's in summation order and eigen-solver only, within two float32
ulps of max(1, |value|) per coefficient: one for the float32 rounding on either side.

The workhorse is plane_ref_np.workhorse(): 20 000 points, half on z = 0.05 x - 0.03 y + 1.5 (sigma 0.02), a quarter on the wall
y = 7, a quarter uniform, shuffled, NaN / inf planted every ~1000 points.  On it, at t = 0.1 (tests/test_plane_rule.py asserts the
same of the restatement): seed 1, H = 64 has a tie for the best count between hypotheses 8 and 27 at 10 222 inliers, so 8 must win;
the axis (0, 0, 1) at 15 degrees refuses 179 of 257 hypotheses at seed 1."""
import ctypes
import math

import numpy as np
import pytest

import plane_ref_np as ref

pytestmark = pytest.mark.gpu

T = 0.1
INVALID = "error -1:"
TILE = 1024


@pytest.fixture(scope="module")
def cloud():
    x = ref.workhorse()
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def dev(api, ctx, cloud):
    c = api.Cloud(ctx, cloud)
    yield c
    c.close()


@pytest.fixture(scope="module")
def planes4096(cloud):
    """4096 hypotheses of the workhorse (seed 1) and their counts by the restatement, computed once"""
    planes = ref.hypotheses(cloud, 4096, 1)[0]
    counts = ref.score(cloud, planes, T)
    planes.setflags(write=False)
    counts.setflags(write=False)
    return planes, counts


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ulps(got, want):
    """|got - want| in float32 ulps of max(1, |want|), per coefficient"""
    want = np.asarray(want, np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(want), np.float32(1)))


# ------------------------------------------------------------------ 1. hypotheses
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_plane_hypotheses(dev, cloud, seed):
    for H in (1, 64, 257, 4096):
        for axis, deg in ((None, None), ((0.0, 0.0, 1.0), 15.0), ((0.3, -0.2, -1.0), 40.0)):
            planes, samples, n_deg = dev.plane_hypotheses(H, seed, axis, deg)
            rp, rs, rn = ref.hypotheses(cloud, H, seed, axis, 0.0 if deg is None else math.cos(math.radians(deg)))
            assert planes.shape == (H, 4) and samples.dtype == np.int32
            assert np.array_equal(samples, rs), (H, axis)
            assert n_deg == rn and n_deg == int(np.isnan(planes).all(axis=1).sum()), (H, axis, n_deg, rn)
            assert np.array_equal(bits(planes), bits(rp)), (H, axis, np.flatnonzero((bits(planes) != bits(rp)).any(axis=1))[:5])
    if seed == 1:
        assert dev.plane_hypotheses(2, 1)[1].tolist() == [[8519, 10590, 235], [8761, 10048, 7045]]
        assert dev.plane_hypotheses(257, 1, (0, 0, 1), 15.0)[2] == 179


# ------------------------------------------------------------------ 2. scoring
@pytest.mark.parametrize("H", [1, 2, 63, 64, 65, 257, 4096])
def test_score_planes_hypothesis_counts(api, dev, planes4096, H):
    planes, counts = planes4096
    got = dev.score_planes(planes[:H], T)
    assert got.dtype == np.int64 and np.array_equal(got, counts[:H]), np.flatnonzero(got != counts[:H])[:5]
    for max_blocks in (1, 3, 0):                                 # 20 tiles on 1 and 3 workgroups: several tiles each
        got = api.hook_plane_score(dev, planes[:H], T, max_blocks)
        assert np.array_equal(got, counts[:H]), (max_blocks, np.flatnonzero(got != counts[:H])[:5])


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_score_planes_cloud_sizes(api, ctx, cloud, planes4096, n):
    planes = planes4096[0][:130]
    x = cloud[np.isfinite(cloud).all(axis=1)][:n] if n <= 3 else cloud[max(0, 500 - n // 2):][:n]     # (the larger ones hold a non-finite point)
    c = api.Cloud(ctx, x)
    want = ref.score(x, planes, T)
    assert np.array_equal(c.score_planes(planes, T), want)
    assert np.array_equal(api.hook_plane_score(c, planes, T, 1), want)
    c.close()
    assert len(x) == n and (n <= 3 or not np.isfinite(x).all())


def test_score_planes_special_planes(api, ctx, dev, cloud):
    n_finite = int(np.isfinite(cloud).all(axis=1).sum())
    planes = np.array([[np.nan] * 4, [0, 0, 0, 0], [0, 0, 1, -1000], [0, 0, 1, np.nan], [np.inf, 0, 0, 0], [0, 0, 0, 0.09999], [0, 0, 0, 0.1]], np.float32)
    got = dev.score_planes(planes, T)
    assert got.tolist() == [0, n_finite, 0, 0, 0, n_finite, 0] and np.array_equal(got, ref.score(cloud, planes, T))
    # a cloud of non-finite points only: nothing matches, not even the all-zero plane
    bad = np.full((70, 3), np.nan, np.float32)
    bad[::2, 1] = np.inf
    bad[1::4] = (1.0, -np.inf, 2.0)
    c = api.Cloud(ctx, bad)
    assert not c.score_planes(planes, T).any() and not ref.score(bad, planes, T).any()
    assert c.segment_plane(T, 16)[2]["found"] == 0
    c.close()
    assert api.Cloud(ctx, np.zeros((0, 3), np.float32)).score_planes(planes, T).tolist() == [0] * 7


# ------------------------------------------------------------------ 3. the segmentation
def check_segmentation(cloud, got, want, **kw):
    plane, inlier, st = got
    rst = want["stats"]
    for key in ("n_points", "n_hypotheses", "n_degenerate", "best_index", "best_count", "found", "refined"):
        assert st[key] == rst[key], (kw, key, st, rst)
    assert plane.dtype == np.float32 and inlier.dtype == bool and inlier.shape == (len(cloud),)
    u = ulps(plane, want["plane"])
    print(kw, "plane", plane, "ulps from the restatement", u, "n_inliers", st["n_inliers"], rst["n_inliers"])
    assert (u <= 2).all(), (kw, plane, want["plane"], u)
    # the mask and its count: the score rule applied to the plane the device returned, exactly
    mask = ref.inliers(cloud, plane, T) if st["found"] else np.zeros(len(cloud), bool)
    assert np.array_equal(inlier, mask) and st["n_inliers"] == int(mask.sum()), kw
    assert st["score_ms"] == -1.0 and st["total_ms"] == -1.0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_segment_plane(dev, cloud, seed):
    for H in (1, 64, 257):
        want = ref.segment(cloud, T, H, True, seed)
        check_segmentation(cloud, dev.segment_plane(T, H, True, seed), want, seed=seed, H=H)
        assert want["stats"]["refined"] == 1
    a, b, c = ref.GROUND
    truth = np.array([-a, -b, 1.0, -c]) / np.sqrt(a * a + b * b + 1)
    plane, inlier, st = dev.segment_plane(T, 257, True, seed)
    assert np.abs(plane - truth).max() < 2e-3 and 10_000 < st["n_inliers"] < 10_400       # the ground, whatever the seed


def test_segment_plane_tie_and_axis(dev, cloud):
    want = ref.segment(cloud, T, 64, True, 1)
    c = want["counts"]
    assert np.flatnonzero(c == c.max()).tolist() == [8, 27]     # the tie of the restatement: the smaller index wins
    plane, inlier, st = dev.segment_plane(T, 64, True, 1)
    assert (st["best_index"], st["best_count"]) == (8, 10222)
    # the wall y = 7 is the best plane among those within 15 degrees of the y axis; the ground among those of the z axis
    for axis in ((0.0, 1.0, 0.0), (0.0, 0.0, -2.0)):
        want = ref.segment(cloud, T, 257, True, 1, axis=axis, axis_min_cos=math.cos(math.radians(15.0)))
        got = dev.segment_plane(T, 257, True, 1, axis=axis, max_angle_deg=15.0)
        check_segmentation(cloud, got, want, axis=axis)
        assert got[0][:3] @ np.asarray(axis) > 0 and got[2]["n_degenerate"] > 150
    assert abs(dev.segment_plane(T, 257, True, 1, axis=(0, 1, 0), max_angle_deg=15.0)[0][3] + 7.0) < 1e-2


def test_segment_plane_without_refit_and_repeats(dev, cloud):
    planes = ref.hypotheses(cloud, 257, 2)[0]
    plane, inlier, st = dev.segment_plane(T, 257, False, 2)
    assert st["refined"] == 0 and np.array_equal(bits(plane), bits(planes[st["best_index"]]))
    check_segmentation(cloud, (plane, inlier, st), ref.segment(cloud, T, 257, False, 2), refine=False)
    assert st["n_inliers"] == st["best_count"]
    runs = [dev.segment_plane(T, 257, True, 3) for _ in range(3)]
    for plane, inlier, st in runs[1:]:
        assert np.array_equal(bits(plane), bits(runs[0][0])) and np.array_equal(inlier, runs[0][1]) and st == runs[0][2]


def test_segment_plane_profile(dev):
    st = dev.segment_plane(T, 64, True, 1, profile=True)[2]
    assert 0.0 < st["score_ms"] <= st["total_ms"]


def test_min_inliers_not_reached(dev, cloud):
    plane, inlier, st = dev.segment_plane(T, 64, True, 1, min_inliers=10223)
    assert (st["best_index"], st["best_count"], st["found"], st["refined"], st["n_inliers"]) == (8, 10222, 0, 0, 0)
    assert np.array_equal(bits(plane), np.zeros(4, np.uint32)) and not inlier.any()
    assert dev.segment_plane(T, 64, True, 1, min_inliers=10222)[2]["found"] == 1


def test_tiny_clouds(api, ctx):
    for pts in (np.zeros((0, 3)), [[1, 2, 3]], [[1, 2, 3], [4, 5, 6]], [[0, 0, 0], [1, 1, 1], [2, 2, 2]]):
        pts = np.asarray(pts, np.float32).reshape(-1, 3)
        c = api.Cloud(ctx, pts)
        plane, inlier, st = c.segment_plane(T, 16, True, 5)
        want = ref.segment(pts, T, 16, True, 5)["stats"]
        assert {k: st[k] for k in want} == want, (len(pts), st, want)
        assert st["found"] == 0 and st["n_degenerate"] == (16 if len(pts) else 0) and not plane.any() and inlier.shape == (len(pts),) and not inlier.any()
        planes, samples, n_deg = c.plane_hypotheses(16, 5)
        assert np.isnan(planes).all() and n_deg == 16 and (len(pts) > 0 or (samples == -1).all())
        c.close()
    # three points that span a plane: every hypothesis with three different samples finds all three
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    c = api.Cloud(ctx, pts)
    plane, inlier, st = c.segment_plane(T, 64, True, 5)
    want = ref.segment(pts, T, 64, True, 5)
    assert st["found"] == 1 and st["best_count"] == 3 and st["best_index"] == want["stats"]["best_index"] and inlier.all()
    assert (ulps(plane, want["plane"]) <= 2).all() and np.abs(plane - np.array([0, 0, 1, 0], np.float32)).max() < 1e-6
    c.close()


def test_segment_plane_leaves_the_cloud_alone(api, ctx, cloud):
    c = api.Cloud(ctx, cloud)
    c.crop_aabb((-9.0, -9.0, -9.0), (9.0, 9.0, 9.0))
    before, idx = c.download(), c.last_indices()
    c.segment_plane(T, 64)
    c.plane_hypotheses(64)
    c.score_planes(np.zeros((3, 4), np.float32), T)
    assert np.array_equal(bits(c.download()), bits(before)) and np.array_equal(c.last_indices(), idx) and len(c) == len(before)
    c.close()


# ------------------------------------------------------------------ 4. removal
@pytest.mark.parametrize("keep_inliers", [False, True])
def test_remove_plane(api, ctx, cloud, dev, keep_inliers):
    plane0, inlier, st0 = dev.segment_plane(T, 257, True, 1)
    c = api.Cloud(ctx, cloud)
    plane, st = c.remove_plane(T, 257, True, 1, keep_inliers=keep_inliers)
    assert np.array_equal(bits(plane), bits(plane0)) and st == st0
    keep = np.flatnonzero(inlier == keep_inliers)
    assert len(c) == len(keep) and np.array_equal(c.last_indices(), keep)
    assert np.array_equal(bits(c.download()), bits(cloud[keep]))                # order kept, NaN and inf points among them
    # no plane found: nothing is removed, either way round
    plane, st = c.remove_plane(T, 64, True, 1, min_inliers=len(cloud), keep_inliers=keep_inliers)
    assert st["found"] == 0 and not plane.any() and len(c) == len(keep) and np.array_equal(c.last_indices(), np.arange(len(keep)))
    assert np.array_equal(bits(c.download()), bits(cloud[keep]))
    c.close()


def test_remove_plane_empty_cloud(api, ctx):
    c = api.Cloud(ctx, np.zeros((0, 3), np.float32))
    plane, st = c.remove_plane(T, 64)
    assert st["found"] == 0 and st["n_points"] == 0 and not plane.any() and len(c) == 0 and len(c.last_indices()) == 0
    c.close()


# ------------------------------------------------------------------ 5. refused arguments
def test_refused_arguments(api, ctx, cloud):
    c = api.Cloud(ctx, cloud[:500])
    c.crop_aabb((-9.0, -9.0, -9.0), (9.0, 9.0, 9.0))
    before, idx = c.download(), c.last_indices()
    bad = (dict(num_hypotheses=0), dict(num_hypotheses=4097), dict(distance_threshold=0.0), dict(distance_threshold=-1.0), dict(distance_threshold=float("nan")),
           dict(distance_threshold=float("inf")), dict(min_inliers=2), dict(axis=(0, 0, 1), max_angle_deg=100.0), dict(axis=(0, float("nan"), 1)))
    for kw in bad:
        for call in (c.segment_plane, c.remove_plane):
            with pytest.raises(api.SlamFusionError, match=INVALID):
                call(**kw)
    p = api._plane_params(T, 64, True, 0, 3, (0, 0, 1), None, False)
    p.axis_min_cos = 1.5
    plane = np.zeros(4, np.float32)
    assert api.load_library().sf_cloud_segment_plane(c.h, ctypes.byref(p), plane.ctypes.data, None, None) == -1
    for kw in (dict(num_hypotheses=0), dict(num_hypotheses=4097)):
        with pytest.raises(api.SlamFusionError, match=INVALID):
            c.plane_hypotheses(**kw)
    ok = np.zeros((1, 4), np.float32)
    for planes, t in ((np.zeros((0, 4), np.float32), T), (np.zeros((4097, 4), np.float32), T), (ok, 0.0), (ok, float("nan"))):
        with pytest.raises(api.SlamFusionError, match=INVALID):
            c.score_planes(planes, t)
    with pytest.raises(api.SlamFusionError, match=INVALID):
        api.hook_plane_score(c, ok, T, -1)
    assert np.array_equal(bits(c.download()), bits(before)) and np.array_equal(c.last_indices(), idx)
    c.close()


