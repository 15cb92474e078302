"""Visibility classes, votes and the removal of seen-through points on the device (sf_map_visibility, sf_map_visibility_votes,
sf_cloud_remove_seen_through) against the numpy restatement of the rule (tests/visibility_ref_np.py): classes, both
vote arrays and the statistics bit for bit.  tests/test_visibility_rule.py pins the restatement to independent facts and shows that no
fixture here has a point on a pixel edge."""
import functools

import numpy as np
import pytest

import visibility_fixtures as fx
import visibility_ref_np as ref
from test_gpu_range_image import image_for

pytestmark = pytest.mark.gpu

INVALID, STATE = "error -1:", "error -4:"
COUNT_KEYS = ("n_points", "n_valid", "n_outside", "n_unknown", "n_within", "n_occluded", "n_seen_through")
WINDOWS = ((0, 0), (1, 1), (2, 0), (0, 2))
MARGINS = ((0.0, 0.0), (0.2, 0.01))


@functools.lru_cache(maxsize=None)
def ref_image(b):
    """image b of fx.image_specs() by the restatement, computed once: (prm, (range, index))"""
    scan, prm, _ = fx.image_specs()[b]
    return prm, ref.build(scan, None, prm)[:2]


@pytest.fixture(scope="module")
def images(api, ctx):
    """the 64 images of fx.image_specs() on the device, each exactly the restatement's"""
    out = []
    for b, (scan, prm, _) in enumerate(fx.image_specs()):
        img = image_for(api, ctx, prm)
        img.build(api.Cloud(ctx, scan))
        if b < 8:
            rng, idx = img.download()
            assert np.array_equal(rng, ref_image(b)[1][0]) and np.array_equal(idx, ref_image(b)[1][1]), b
        out.append(img)
    return out


def poses_of(bs):
    return np.stack([np.eye(4) if fx.image_specs()[b][2] is None else fx.image_specs()[b][2] for b in bs])


def n_finite(pts):
    return int(np.isfinite(pts).all(axis=1).sum())


def check_stats(st, all_cls, pts, n_removed, what):
    want = ref.class_stats(all_cls, n_finite(pts))
    assert {k: st[k] for k in COUNT_KEYS} == want and st["n_removed"] == n_removed, (what, st, want)
    assert st["device_ms"] == -1.0, what


@pytest.mark.parametrize("n", fx.MAP_SIZES)
def test_map_sizes_at_two_cells(api, ctx, images, n):
    pts = fx.map_points(n)
    answers = []
    for cell in (0.5, 2.0):
        m = api.Map(ctx, api.Cloud(ctx, pts), cell)
        for b in (0, 1):
            T = fx.image_specs()[b][2]
            cls, st = m.visibility(images[b], T)
            want = ref.classify(pts, T, *ref_image(b))
            assert cls.dtype == np.uint8 and np.array_equal(cls, want), (n, cell, b)
            check_stats(st, [want], pts, 0, (n, cell, b))
            assert (cls[~np.isfinite(pts).all(axis=1)] == ref.OUTSIDE).all()
            answers.append(cls)
    assert np.array_equal(answers[0], answers[2]) and np.array_equal(answers[1], answers[3])   # the cell does not matter
    if n == 3000:
        assert set(np.unique(answers[0])) == {0, 1, 2, 3, 4}                                     # every class occurs


@pytest.mark.parametrize("margins", MARGINS, ids=lambda m: "margin %g ratio %g" % m)
@pytest.mark.parametrize("full", (False, True), ids=("min_hits 1", "min_hits full"))
@pytest.mark.parametrize("window", WINDOWS + ((3, 1), (3, 2)), ids=lambda w: "window %d %d" % w)
def test_windows_hits_and_margins(api, ctx, images, window, full, margins):
    """the windows of the issue on the 64 x 16 image; (3, 1) and (3, 2) on the 7 x 3 one: as wide as W, and rows cut off at both ends"""
    pts = fx.map_points(3000)
    m = api.Map(ctx, api.Cloud(ctx, pts))
    hc, hr = window
    win = ref.window(half_cols=hc, half_rows=hr, min_hits=(2 * hc + 1) * (2 * hr + 1) if full else 1, range_margin=margins[0], range_ratio=margins[1])
    if hc == 3:
        prm = fx.params(7, 3)
        img = image_for(api, ctx, prm)
        img.build(api.Cloud(ctx, fx.scan_shell()))
        image, T = ref.build(fx.scan_shell(), None, prm)[:2], None
    else:
        (prm, image), img, T = ref_image(1), images[1], fx.image_specs()[1][2]
    cls, st = m.visibility(img, T, **win)
    want = ref.classify(pts, T, prm, image, win)
    assert np.array_equal(cls, want), (window, full, margins)
    check_stats(st, [want], pts, 0, (window, full, margins))
    assert len(np.unique(cls)) >= 4 or full                                 # (a full window over the scan's holes leaves fewer classes)


def test_the_wrap_across_the_seam(api, ctx):
    scan, pts, prm = fx.wrap_case()
    img = image_for(api, ctx, prm)
    img.build(api.Cloud(ctx, scan))
    image = ref.build(scan, None, prm)[:2]
    assert image[1][:, 359].max() == 0 and (image[1][:, :359] == -1).all()                       # the one hit lies in the last column
    m = api.Map(ctx, api.Cloud(ctx, pts))
    for hc, expect in ((1, [ref.SEEN_THROUGH, ref.OCCLUDED, ref.WITHIN, ref.SEEN_THROUGH]), (0, [ref.UNKNOWN, ref.UNKNOWN, ref.UNKNOWN, ref.SEEN_THROUGH])):
        win = ref.window(half_cols=hc, half_rows=0)
        cls, _ = m.visibility(img, None, **win)
        assert list(ref.classify(pts, None, prm, image, win)) == expect and list(cls) == expect, hc


def test_points_exactly_on_the_margins(api, ctx):
    near, far, pts, prm, win = fx.dyadic_case()
    m = api.Map(ctx, api.Cloud(ctx, pts))
    for scan, expect in ((near, [ref.WITHIN, ref.SEEN_THROUGH, ref.WITHIN]), (far, [ref.WITHIN, ref.WITHIN, ref.OCCLUDED])):
        img = image_for(api, ctx, prm)
        img.build(api.Cloud(ctx, scan))
        cls, _ = m.visibility(img, None, **win)
        assert list(ref.classify(pts, None, prm, ref.build(scan, None, prm)[:2], win)) == expect and list(cls) == expect


@pytest.mark.parametrize("count", (1, 2, 5, 64))
def test_votes_of_many_images(api, ctx, images, count):
    pts = fx.map_points(3000)
    m = api.Map(ctx, api.Cloud(ctx, pts))
    bs = list(range(count))
    seen, within, st = m.visibility_votes([images[b] for b in bs], poses_of(bs))
    want_seen, want_within, all_cls = ref.votes(pts, [ref_image(b) for b in bs], [fx.image_specs()[b][2] for b in bs])
    assert seen.dtype == within.dtype == np.uint16 and np.array_equal(seen, want_seen) and np.array_equal(within, want_within), count
    check_stats(st, all_cls, pts, 0, count)
    if count == 5:                                                          # the sum of the single calls, on the device too
        s, w = np.zeros(len(pts), np.uint16), np.zeros(len(pts), np.uint16)
        for b in bs:
            cls, _ = m.visibility(images[b], fx.image_specs()[b][2])
            s += cls == ref.SEEN_THROUGH
            w += cls == ref.WITHIN
        assert np.array_equal(seen, s) and np.array_equal(within, w)
    if count == 64:
        assert seen.max() > 32 and within.max() > 8


@pytest.mark.parametrize("rule", ((1, 0), (2, 1), (1, 64), (6, 0)), ids=lambda r: "min_seen %d max_within %d" % r)
def test_the_cloud_form(api, ctx, images, rule):
    pts = fx.map_points(3000)
    bs = list(range(5))
    want_seen, want_within, all_cls = ref.votes(pts, [ref_image(b) for b in bs], [fx.image_specs()[b][2] for b in bs])
    mask = ref.remove_mask(want_seen, want_within, *rule)
    cloud = api.Cloud(ctx, pts)
    st = cloud.remove_seen_through([images[b] for b in bs], poses_of(bs), *rule)
    check_stats(st, all_cls, pts, int(mask.sum()), rule)
    kept = cloud.download()
    assert np.array_equal(kept.view(np.uint32), pts[~mask].view(np.uint32)) and np.array_equal(cloud.last_indices(), np.flatnonzero(~mask))
    if rule == (6, 0):
        assert not mask.any() and len(cloud) == len(pts)                    # five images cannot give six votes: nothing goes
    else:
        assert 0 < mask.sum() < len(pts)
    empty = api.Cloud(ctx, np.zeros((0, 3), np.float32))
    st = empty.remove_seen_through([images[0]], None)
    assert {k: st[k] for k in COUNT_KEYS + ("n_removed",)} == dict.fromkeys(COUNT_KEYS + ("n_removed",), 0) and len(empty) == 0


def test_the_map_is_left_alone_and_two_runs_agree(api, ctx, images):
    pts = fx.map_points(3000)
    m = api.Map(ctx, api.Cloud(ctx, pts), 0.5)
    m.estimate_normals(1.0)
    queries = fx.shell(500, 9, 2.0, 18.0)
    nn0, nrm0, index0 = m.nn(queries), m.download_normals(), m.index()
    bs = list(range(5))
    runs = [m.visibility_votes([images[b] for b in bs], poses_of(bs)) for _ in range(2)]
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    a, b = m.visibility(images[2], fx.image_specs()[2][2])[0], m.visibility(images[2], fx.image_specs()[2][2])[0]
    assert a.tobytes() == b.tobytes()
    nn1, nrm1, index1 = m.nn(queries), m.download_normals(), m.index()
    assert nn0[0].tobytes() == nn1[0].tobytes() and nn0[1].tobytes() == nn1[1].tobytes() and nrm0[0].tobytes() == nrm1[0].tobytes()
    assert index0["pts4"].tobytes() == index1["pts4"].tobytes() and index0["cell_start"].tobytes() == index1["cell_start"].tobytes()
    m.profile_launches(True)                                                # the measurement switch times the map forms
    assert m.visibility(images[0], None)[1]["device_ms"] > 0.0
    m.profile_launches(False)
    assert m.visibility(images[0], None, profile=True)[1]["device_ms"] > 0.0


def test_every_refusal_touches_nothing(api, ctx, images):
    pts = fx.map_points(257)
    cloud = api.Cloud(ctx, pts)
    m = api.Map(ctx, cloud)
    wide, small = images[0], images[3]                                      # 64 x 16 and 7 x 3
    bad_pose = np.eye(4)
    bad_pose[0, 3] = np.nan
    refusals = [dict(half_cols=-1), dict(half_rows=-1), dict(half_cols=32), dict(min_hits=0), dict(min_hits=10), dict(range_margin=-0.1), dict(range_margin=np.nan),
                dict(range_ratio=-1.0), dict(range_ratio=np.inf)]
    for kw in refusals:
        with pytest.raises(api.SlamFusionError, match=INVALID):
            m.visibility(wide, None, **kw)
        with pytest.raises(api.SlamFusionError, match=INVALID):
            cloud.remove_seen_through([wide], None, **kw)
    with pytest.raises(api.SlamFusionError, match=INVALID):
        m.visibility_votes([wide, small], None, half_cols=4)                # fits the first image, not the second
    with pytest.raises(api.SlamFusionError, match=INVALID):
        m.visibility(wide, bad_pose)
    with pytest.raises(api.SlamFusionError, match=INVALID):
        m.visibility_votes([], None)
    with pytest.raises(api.SlamFusionError, match=INVALID):
        m.visibility_votes([wide] * 65, None)
    for rule in ((0, 0), (1, -1)):
        with pytest.raises(api.SlamFusionError, match=INVALID):
            cloud.remove_seen_through([wide], None, *rule)
    with pytest.raises(api.SlamFusionError, match=INVALID):
        cloud.remove_seen_through([wide], bad_pose[None])
    closed = image_for(api, ctx, fx.params(7, 3))
    closed.close()                                                          # its handle is NULL now
    with pytest.raises(api.SlamFusionError, match=INVALID):
        m.visibility_votes([wide, closed], None)
    with pytest.raises(api.SlamFusionError, match=STATE):
        api.Map(ctx).visibility(wide, None)
    assert np.array_equal(cloud.download().view(np.uint32), pts.view(np.uint32)) and len(cloud) == len(pts)
    rng, idx = wide.download()
    assert np.array_equal(rng, ref_image(0)[1][0]) and np.array_equal(idx, ref_image(0)[1][1])
    cls, _ = m.visibility(wide, None)
    assert np.array_equal(cls, ref.classify(pts, None, *ref_image(0)))


def test_a_parked_car_leaves_the_map(api, ctx):
    """About 20 k map points of a ground patch, a wall and a car; four scans of the same world without the car.  The flags are the
    restatement's exactly.  The floor (tests/test_visibility_rule.py runs it on the restatement alone: 0.92 of the car's points get
    seen_through >= 2, no wall point does): more than half of the car goes, nothing of the wall."""
    sc = fx.scene()
    prm = sc["prm"]
    imgs, ref_images = [], []
    for scan in sc["scans"]:
        img = image_for(api, ctx, prm)
        img.build(api.Cloud(ctx, scan))
        imgs.append(img)
        ref_images.append((prm, ref.build(scan, None, prm)[:2]))
        rng, idx = img.download()
        assert np.array_equal(rng, ref_images[-1][1][0]) and np.array_equal(idx, ref_images[-1][1][1])
    m = api.Map(ctx, api.Cloud(ctx, sc["map"]))
    seen, within, st = m.visibility_votes(imgs, np.stack(sc["poses"]))
    want_seen, want_within, all_cls = ref.votes(sc["map"], ref_images, sc["poses"])
    assert np.array_equal(seen, want_seen) and np.array_equal(within, want_within)
    check_stats(st, all_cls, sc["map"], 0, "scene")
    assert (seen[sc["car"]] >= 2).mean() > 0.5 and not (seen[sc["wall"]] >= 2).any()
    cloud = api.Cloud(ctx, sc["map"])
    st = cloud.remove_seen_through(imgs, np.stack(sc["poses"]), 2, 4)
    mask = ref.remove_mask(want_seen, want_within, 2, 4)
    assert st["n_removed"] == mask.sum() and np.array_equal(cloud.last_indices(), np.flatnonzero(~mask))
    assert mask[sc["car"]].mean() > 0.5 and not mask[sc["wall"]].any()
