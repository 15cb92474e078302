"""Range images on the device (sf_range_image_*) against the numpy restatement of the rule
(tests/visibility_ref_np.py): range, index and the statistics bit for bit.  tests/test_visibility_rule.py pins the restatement to
independent facts and shows that no fixture here has a point on a pixel edge, where the device's atan2 could decide otherwise."""
import numpy as np
import pytest

import visibility_fixtures as fx
import visibility_ref_np as ref

pytestmark = pytest.mark.gpu

INVALID = "error -1:"
STAT_KEYS = ("n_points", "n_projected", "n_outside", "n_nonfinite", "n_filled")


def image_for(api, ctx, prm):
    return api.RangeImage(ctx, prm["width"], prm["height"], prm["el_min"], prm["el_max"], prm["min_range"], prm["max_range"])


def check_build(api, ctx, img, pts, T, prm, what):
    st = img.build(api.Cloud(ctx, pts), T)
    rng, idx = img.download()
    want_rng, want_idx, want_st = ref.build(pts, T, prm)
    assert rng.dtype == np.float32 and idx.dtype == np.int32 and rng.shape == idx.shape == (prm["height"], prm["width"]), what
    assert np.array_equal(rng.view(np.uint32), want_rng.view(np.uint32)), what
    assert np.array_equal(idx, want_idx), what
    assert {k: st[k] for k in STAT_KEYS} == want_st, (what, st, want_st)
    assert st["device_ms"] >= 0.0, what
    return rng, idx, st


@pytest.mark.parametrize("shape", fx.SHAPES, ids=lambda s: "%dx%d" % s)
def test_counts_and_shapes(api, ctx, shape):
    """n = 0 .. 3 000 points into one image of each shape, one build after the other: every build replaces what the image held"""
    img = image_for(api, ctx, fx.count_case(0, shape)[2])
    assert img.params == fx.count_case(0, shape)[2]
    for n in fx.COUNTS[::-1] + fx.COUNTS:                                  # (descending first: a smaller build must clear the larger one)
        pts, T, prm = fx.count_case(n, shape)
        rng, idx, st = check_build(api, ctx, img, pts, T, prm, (shape, n))
        if n == 0:
            assert np.isposinf(rng).all() and (idx == -1).all() and st["n_filled"] == 0


@pytest.mark.parametrize("case", [fx.one_pixel_case, fx.special_case, fx.elevation_case, fx.nonfinite_case], ids=lambda c: c.__name__)
def test_the_edges_of_the_rule(api, ctx, case):
    pts, T, prm = case()
    rng, idx, st = check_build(api, ctx, image_for(api, ctx, prm), pts, T, prm, case.__name__)
    if case is fx.one_pixel_case:
        assert rng[0, 0] == np.float32(5.0) and idx[0, 0] == 1                       # equal ranges: the smallest index
    if case is fx.special_case:
        assert st["n_outside"] == 5 and st["n_projected"] == len(pts) - 5 and st["n_filled"] == 6
    if case is fx.elevation_case:
        assert st["n_projected"] == 24 and st["n_outside"] == 24 and set(np.flatnonzero((idx >= 0).any(axis=1))) == {0, 31}
    if case is fx.nonfinite_case:
        assert st["n_nonfinite"] == int((~np.isfinite(pts).all(axis=1)).sum()) > 3


def test_a_pose_against_the_cloud_taken_back(api, ctx):
    """1 km away under a general rotation: exactly the restatement's image, the pixel of every point that of the cloud taken back into
    the sensor frame beforehand (pose NULL), the ranges within one float32 spacing"""
    world, T, back, prm = fx.posed_case()
    img = image_for(api, ctx, prm)
    rng_a, idx_a, st_a = check_build(api, ctx, img, world, T, prm, "posed")
    rng_b, idx_b, st_b = check_build(api, ctx, img, back, None, prm, "taken back")
    assert np.array_equal(idx_a, idx_b) and {k: st_a[k] for k in STAT_KEYS} == {k: st_b[k] for k in STAT_KEYS}
    filled = idx_a >= 0
    assert filled.sum() > 300
    assert (np.abs(rng_a[filled].astype(np.float64) - rng_b[filled].astype(np.float64)) <= np.spacing(np.maximum(rng_a[filled], rng_b[filled])).astype(np.float64)).all()
    qa, qb = ref.project(world, T, prm), ref.project(back, None, prm)
    assert np.array_equal(qa["inside"], qb["inside"]) and np.array_equal(qa["row"][qa["inside"]], qb["row"][qa["inside"]])
    assert np.array_equal(qa["col"][qa["inside"]], qb["col"][qa["inside"]])


def test_two_runs_are_bitwise_equal(api, ctx):
    pts, T, prm = fx.count_case(3000, (7, 3))                              # 21 pixels for 3 000 points: every pixel is fought over
    cloud, outs = api.Cloud(ctx, pts), []
    for _ in range(2):
        img = image_for(api, ctx, prm)
        img.build(cloud, T)
        outs.append(img.download())
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()


def test_every_refusal_leaves_the_image_untouched(api, ctx):
    pts, T, prm = fx.count_case(257, (64, 16))
    img, cloud = image_for(api, ctx, prm), api.Cloud(ctx, pts)
    img.build(cloud, T)
    before = img.download()
    bad = np.eye(4)
    for value in (np.nan, np.inf):
        bad[1, 2] = value
        with pytest.raises(api.SlamFusionError, match=INVALID):
            img.build(cloud, bad)
    after = img.download()
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes() and img.params == prm
    for over in (dict(width=0), dict(width=16385), dict(height=0), dict(height=4097), dict(el_min=np.nan), dict(el_max=np.inf), dict(el_min=0.5, el_max=0.5),
                 dict(el_min=0.6, el_max=0.5), dict(min_range=-0.1), dict(min_range=np.nan), dict(max_range=np.inf), dict(min_range=3.0, max_range=3.0),
                 dict(min_range=3.0, max_range=2.0)):
        q = dict(prm)
        q.update(over)
        with pytest.raises(api.SlamFusionError, match=INVALID):
            image_for(api, ctx, q)
    ok = image_for(api, ctx, dict(prm, width=16384, height=1, min_range=0.0))   # the bounds themselves are allowed
    assert ok.params["width"] == 16384 and np.isposinf(ok.download()[0]).all()
