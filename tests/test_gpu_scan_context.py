"""Scan Context descriptors on the device (sf_cloud_scan_context, sf_place_db_add_cloud) against the numpy
restatement of the rule (tests/place_ref_np.py): descriptor and statistics bit for bit.  tests/test_place_rule.py pins the restatement
to independent facts and shows that no fixture here has a point on a sector edge, where the device's atan2 could decide otherwise."""
import numpy as np
import pytest

import place_fixtures as fx
import place_ref_np as ref

pytestmark = pytest.mark.gpu

INVALID = "error -1:"


def check_build(api, ctx, pts, T, prm, what):
    desc, st = api.Cloud(ctx, pts).scan_context(T, **prm)
    want, want_st = ref.descriptor(pts, T, prm)
    assert desc.dtype == np.float32 and desc.shape == (prm["num_rings"], prm["num_sectors"]), what
    assert np.array_equal(desc.view(np.uint32), want.view(np.uint32)), what
    assert {k: st[k] for k in ref.STAT_KEYS} == want_st, (what, st, want_st)
    assert st["device_ms"] >= 0.0, what
    return desc, st


@pytest.mark.parametrize("shape", fx.SHAPES, ids=lambda s: "%dx%d" % s)
def test_counts_and_shapes(api, ctx, shape):
    for n in fx.COUNTS:
        pts, T, prm = fx.count_case(n, shape)
        desc, st = check_build(api, ctx, pts, T, prm, (shape, n))
        if n == 0:
            assert not desc.any() and st["n_filled"] == 0
    assert st["n_outside"] > 100 and st["n_below"] > 100 and st["n_binned"] > 1000          # (n = 3 000)


@pytest.mark.parametrize("case", [fx.special_case, fx.min_range_case, fx.nonfinite_case], ids=lambda c: c.__name__)
def test_the_edges_of_the_rule(api, ctx, case):
    pts, T, prm = case()
    desc, st = check_build(api, ctx, pts, T, prm, case.__name__)
    if case is fx.special_case:
        assert desc[0, 30] == 3.0                                   # rho = 0: ring 0, the sector of az = 0; its other point is below
        assert desc[2, 0] == 3.5 and desc[2, 59] == 0.0             # +pi and -pi are one sector
        assert desc[19].max() == 3.0 and st["n_outside"] == 2       # max_range itself and beyond are outside, one float32 inside is ring 19
        assert st["n_below"] == 4 and desc[2, 38] == np.float32(2.0) - np.float32(1.9999999)   # heights of exactly 0 and below; one float32 above
        assert desc[4, 51] == 5.25 and desc[4, 30] == 2.5 and st["n_filled"] == 6                # equal heights in one bin, and a lower one
    if case is fx.min_range_case:
        assert st["n_outside"] == 3 and st["n_binned"] == 3 and desc[0, 38] == 5.0 and desc[0, 8] == 6.0 and st["n_filled"] == 2
    if case is fx.nonfinite_case:
        assert st["n_nonfinite"] == int((~np.isfinite(pts).all(axis=1)).sum()) > 3


def test_a_pose_against_the_cloud_taken_back(api, ctx):
    """1 km away under a general rotation: exactly the restatement's descriptor; the bins are those of the cloud taken back into the
    sensor frame beforehand (pose NULL) and the heights agree within what float32 coordinates 1 km out can carry"""
    world, T, back, prm = fx.posed_case()
    a, st_a = check_build(api, ctx, world, T, prm, "posed")
    b, st_b = check_build(api, ctx, back, None, prm, "taken back")
    assert {k: st_a[k] for k in ref.STAT_KEYS} == {k: st_b[k] for k in ref.STAT_KEYS}
    assert np.array_equal(a != 0, b != 0) and (a != 0).sum() > 200
    assert np.abs(a.astype(np.float64) - b.astype(np.float64)).max() <= 2.0 * float(np.spacing(np.float32(1000.0)))


def test_a_smaller_build_after_a_larger_one_and_the_database_rows(api, ctx):
    """the query slot of a database is reused from one call to the next: a scan of 1 point after one of 3 000 leaves nothing of the
    larger one behind; add followed by download gives the same rows as Cloud.scan_context"""
    shape = (20, 60)
    prm = fx.count_case(0, shape)[2]
    db = api.PlaceDB(ctx, **prm)
    assert db.params == prm and len(db) == 0
    want, poses = [], []
    for k, n in enumerate((3000, 1, 65, 0, 64)):
        pts = fx.count_case(n, shape)[0]
        T = fx.yaw_pose(10.0 * k, (k, -k, 0.5))
        index, st = db.add(api.Cloud(ctx, pts), T)
        ref_desc, ref_st = ref.descriptor(pts, None, prm)
        assert index == k and {k2: st[k2] for k2 in ref.STAT_KEYS} == ref_st
        want.append(ref_desc)
        poses.append(T)
        out = db.query_cloud(api.Cloud(ctx, pts), 1)              # the descriptor built into the query slot is the restatement's too
        d, s = ref.distances(ref_desc[None], np.stack(want))
        best = ref.top_k(d, s, 1)
        assert out["idx"][0, 0] == best["idx"][0, 0] and out["shift"][0, 0] == best["shift"][0, 0] and out["dist"][0, 0] == best["dist"][0, 0]
        assert {k2: out["build_stats"][k2] for k2 in ref.STAT_KEYS} == ref_st
    desc, got_poses = db.download()
    assert np.array_equal(desc.view(np.uint32), np.stack(want).view(np.uint32)) and np.array_equal(got_poses, np.stack(poses))
    db.clear()
    assert len(db) == 0 and db.download()[0].shape == (0, 20, 60)


def test_two_runs_are_bitwise_equal(api, ctx):
    pts, T, prm = fx.count_case(3000, (3, 7))                     # 21 bins for 3 000 points: every bin is fought over
    cloud = api.Cloud(ctx, pts)
    a, b = cloud.scan_context(T, **prm)[0], cloud.scan_context(T, **prm)[0]
    assert a.tobytes() == b.tobytes()


def test_every_refusal(api, ctx):
    pts, T, prm = fx.count_case(65, (20, 60))
    cloud = api.Cloud(ctx, pts)
    bad = np.eye(4)
    for value in (np.nan, np.inf):
        bad[1, 2] = value
        with pytest.raises(api.SlamFusionError, match=INVALID):
            cloud.scan_context(bad, **prm)
    for over in (dict(num_rings=0), dict(num_rings=41), dict(num_sectors=0), dict(num_sectors=121), dict(min_range=-0.1), dict(min_range=np.nan), dict(max_range=np.inf),
                 dict(min_range=3.0, max_range=3.0), dict(min_range=3.0, max_range=2.0), dict(sensor_height=np.nan)):
        q = dict(prm)
        q.update(over)
        with pytest.raises(api.SlamFusionError, match=INVALID):
            cloud.scan_context(None, **q)
        with pytest.raises(api.SlamFusionError, match=INVALID):
            api.PlaceDB(ctx, **q)
    other = api.Context(0)
    db = api.PlaceDB(other, **prm)
    with pytest.raises(api.SlamFusionError, match=INVALID):
        db.add(cloud, np.eye(4))                                   # a cloud of another context
    with pytest.raises(api.SlamFusionError, match=INVALID):
        db.query_cloud(cloud, 1)
    with pytest.raises(api.SlamFusionError, match=INVALID):
        api.PlaceDB(ctx, **prm).add(cloud, bad)
    assert len(db) == 0
    assert api.Cloud(ctx, pts).scan_context(None, **dict(prm, num_rings=40, num_sectors=120, min_range=0.0))[0].shape == (40, 120)   # the bounds themselves are allowed
