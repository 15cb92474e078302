"""The numpy restatement of the range-image and visibility rule (tests/visibility_ref_np.py) held against facts it was not built
from, and every fixture of the GPU tests (tests/visibility_fixtures.py) held against the edge condition that makes an exact comparison
with the device legitimate.  No device call."""
import numpy as np
import pytest

import visibility_fixtures as fx
import visibility_ref_np as ref


def _shell_and_probes():
    """a dense shell of radius 10 with the azimuths 1.0 .. 2.0 missing, probes in seeded directions at a given radius"""
    rng = np.random.default_rng(11)
    d = fx.directions(40_000, rng)
    az = np.arctan2(d[:, 1], d[:, 0])
    shell = (d[(az < 1.0) | (az > 2.0)] * 10.0).astype(np.float32)
    q = fx.directions(6_000, rng, el_lo=-1.4, el_hi=1.4)
    qaz = np.arctan2(q[:, 1], q[:, 0])
    return shell, q[(qaz < 0.7) | (qaz > 2.3)], q[(qaz > 1.45) & (qaz < 1.55)]   # (column 23 of 32: the window's columns 22 .. 24 span 1.18 .. 1.77)


def test_a_sphere_shell_sorts_points_by_their_radius():
    shell, seen_dirs, hole_dirs = _shell_and_probes()
    prm = fx.params(32, 16)
    image = ref.build(shell, None, prm)[:2]
    assert len(seen_dirs) > 500 and len(hole_dirs) > 50
    assert (ref.classify((seen_dirs * 5.0).astype(np.float32), None, prm, image) == ref.SEEN_THROUGH).all()
    assert (ref.classify((seen_dirs * 15.0).astype(np.float32), None, prm, image) == ref.OCCLUDED).all()
    assert (ref.classify(shell, None, prm, image) == ref.WITHIN).all()
    for radius in (5.0, 10.0, 15.0):                                      # an empty window is no evidence, whatever the radius
        assert (ref.classify((hole_dirs * radius).astype(np.float32), None, prm, image) == ref.UNKNOWN).all()
    assert (ref.classify((seen_dirs * 50.0).astype(np.float32), None, prm, image) == ref.OUTSIDE).all()   # beyond max_range


def test_a_quarter_turn_shifts_the_image_by_a_quarter_of_its_columns():
    pts = fx.shell(4_000, 21, 1.0, 30.0)
    prm = fx.params(64, 16)
    turned = np.stack([-pts[:, 1], pts[:, 0], pts[:, 2]], axis=1)         # Rz(+90 deg), exact
    rng0, idx0, st0 = ref.build(pts, None, prm)
    assert min(ref.edge_distance(pts, None, prm)) > 1e-9 and min(ref.edge_distance(turned, None, prm)) > 1e-9
    rng1, idx1, st1 = ref.build(turned, None, prm)
    assert np.array_equal(rng1, np.roll(rng0, 16, axis=1)) and np.array_equal(idx1, np.roll(idx0, 16, axis=1)) and st0 == st1
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    rng2, idx2, st2 = ref.build(turned, fx.pose(Rz, np.zeros(3)), prm)    # cloud and pose turned together: nothing moves
    assert np.array_equal(rng2, rng0) and np.array_equal(idx2, idx0) and st2 == st0


def test_a_dyadic_translation_of_pose_and_cloud_changes_nothing():
    rng = np.random.default_rng(31)
    pts = (rng.integers(-32 * 1024, 32 * 1024, (3_000, 3)) / 1024.0).astype(np.float32)      # multiples of 2^-10 within +-32
    scan = (rng.integers(-32 * 1024, 32 * 1024, (3_000, 3)) / 1024.0).astype(np.float32)
    t = np.array([1024.5, -256.25, 8.0])
    moved, moved_scan = (pts.astype(np.float64) + t).astype(np.float32), (scan.astype(np.float64) + t).astype(np.float32)
    assert np.array_equal(moved.astype(np.float64) - t, pts.astype(np.float64))                 # the sum is exact in float32
    prm, T = fx.params(64, 16), fx.pose(np.eye(3), t)
    a, b = ref.build(scan, None, prm), ref.build(moved_scan, T, prm)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert np.array_equal(ref.classify(pts, None, prm, a[:2]), ref.classify(moved, T, prm, b[:2]))
    assert len(np.unique(ref.classify(pts, None, prm, a[:2]))) >= 4


def test_both_signs_of_zero_fall_into_one_column():
    prm = fx.params(360, 32)
    q = ref.project(np.array([[-5, 0.0, 1], [-5, -0.0, 1], [-0.5, 0.0, -3], [-0.5, -0.0, -3]], np.float32), None, prm)
    assert q["inside"].all() and (q["col"] == 0).all()
    assert set(q["u"]) <= {0.0, 360.0}
    ends = [(az + ref.PI) / (2 * ref.PI) * 360 for az in (np.arctan2(0.0, -1.0), np.arctan2(-0.0, -1.0))]
    assert ends == [360.0, 0.0]                                           # +pi and -pi: the two ends of u, and col - W makes them one column


def test_votes_are_the_summed_single_image_classes():
    specs = fx.image_specs()[:5]
    pts = fx.map_points(3000)
    images = [(prm, ref.build(scan, None, prm)[:2]) for scan, prm, _ in specs]
    poses = [T for _, _, T in specs]
    seen, within, _ = ref.votes(pts, images, poses)
    want_seen, want_within = np.zeros(len(pts), int), np.zeros(len(pts), int)
    for (prm, image), T in zip(images, poses):
        for i in range(0, len(pts), 250):                                  # chunk by chunk: a class is a function of its own point
            cls = ref.classify(pts[i:i + 250], T, prm, image)
            want_seen[i:i + 250] += cls == ref.SEEN_THROUGH
            want_within[i:i + 250] += cls == ref.WITHIN
    assert np.array_equal(seen, want_seen) and np.array_equal(within, want_within)
    assert seen.max() >= 3 and within.max() >= 2 and (seen == 0).any()
    mask = ref.remove_mask(seen, within, 2, 1)
    assert 0 < mask.sum() < len(pts) and np.array_equal(mask, (want_seen >= 2) & (want_within <= 1))


def test_the_key_orders_by_range_then_index():
    pts, _, prm = fx.one_pixel_case()
    rng, idx, st = ref.build(pts, None, prm)
    assert rng.shape == (1, 1) and rng[0, 0] == np.float32(5.0) and idx[0, 0] == 1 and st["n_filled"] == 1 and st["n_projected"] == len(pts)


def test_the_special_points():
    pts, _, prm = fx.special_case()
    q = ref.project(pts, None, prm)
    assert not q["inside"][0]                                               # the sensor itself: r = 0
    assert q["inside"][1] and q["inside"][2] and q["row"][1] == 15 and q["row"][2] == 0   # the z axis: the top and the bottom row
    assert list(q["inside"][9:15]) == [True, False, True, True, True, False]            # at, below, above min_range and max_range
    assert q["r"][9] == 0.625 and q["r"][12] == 40.0 and not q["inside"][15] and not q["inside"][16]


@pytest.mark.parametrize("cases", [fx.build_cases, fx.visibility_cases], ids=["range image", "visibility"])
def test_no_fixture_of_the_gpu_tests_lies_on_a_pixel_edge(cases):
    worst = np.inf
    for name, pts, T, prm in cases():
        du, dv = ref.edge_distance(pts, T, prm)
        assert du > 1e-9 and dv > 1e-9, (name, du, dv)
        worst = min(worst, du, dv)
    print("smallest distance of a u or v from an integer: %.3e" % worst)


def test_the_scene_floor():
    """the sanity floor of the scene test, on the restatement alone: most of the car goes, nothing of the wall does"""
    sc = fx.scene()
    images = [(sc["prm"], ref.build(s, None, sc["prm"])[:2]) for s in sc["scans"]]
    seen, within, _ = ref.votes(sc["map"], images, sc["poses"])
    assert 18_000 < len(sc["map"]) <= 20_000 and sc["car"].sum() > 200 and sc["wall"].sum() > 1_000
    assert (seen[sc["car"]] >= 2).mean() > 0.5
    assert not (seen[sc["wall"]] >= 2).any()
