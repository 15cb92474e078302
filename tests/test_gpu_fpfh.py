"""sf_map_compute_fpfh / sf_map_compute_spfh / sf_cloud_compute_fpfh on the device against the numpy restatement of the rule
(tests/fpfh_ref_np.py).  Normals are analytic and given through sf_map_set_normals, so nothing depends on PCA signs.
Bounds: counts, pair counts, validity and stats are integers and equal; every descriptor value lies within one float32 spacing of the
reference value -- both round a float64 whose relative difference (another summation order, a few ulp in 100 / S) is a few hundred
2^-53.  Every fixture's binned values keep 1e-9 from the inner bin edges (tests/test_fpfh_rule.py asserts it on the CPU), so the few
ulp between the device's and numpy's atan2 cannot move a bin."""
import ctypes as C

import numpy as np
import pytest

import fpfh_ref_np as ref

pytestmark = pytest.mark.gpu

STAT_KEYS = ("n_points", "n_valid", "n_featured", "n_pairs", "max_pairs")


def spacing_ok(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.maximum(np.abs(got), np.abs(want))).astype(np.float64)


def build(api, ctx, f, cell=None):
    mp = api.Map(ctx, api.Cloud(ctx, f["points"]), f["cell"] if cell is None else cell)
    mp.set_normals(f["normals"])
    return mp


def check_against_reference(api, ctx, name, cell=None):
    f, r = ref.fixtures()[name], ref.reference(name)
    mp = build(api, ctx, f, cell)
    counts, pairs = mp.compute_spfh(f["radius"], f["orient"], f["toward"])
    assert np.array_equal(pairs, r["n_pairs"]), name
    assert np.array_equal(counts, r["counts"]), name
    feat, st = mp.compute_fpfh(f["radius"], f["orient"], f["toward"])
    rows, valid = feat.download()
    assert len(feat) == len(f["points"]) and np.array_equal(valid, r["valid"]), name
    assert {k: st[k] for k in STAT_KEYS} == r["stats"] and st["spfh_ms"] == -1.0 and st["fpfh_ms"] == -1.0, (name, st, r["stats"])
    ok = spacing_ok(rows, r["rows"])
    assert ok.all(), (name, int((~ok).sum()), float(np.abs(rows - r["rows"]).max()))
    assert np.all(rows[~valid] == 0)
    return counts, pairs, rows, valid


@pytest.mark.parametrize("name", ["sphere1", "sphere2", "sphere63", "sphere64", "sphere65", "sphere257"])
def test_wave_and_block_edges(api, ctx, name):
    _, pairs, _, valid = check_against_reference(api, ctx, name)
    if name not in ("sphere1", "sphere2"):
        assert valid.sum() > len(valid) // 2 and pairs.max() >= 3


def test_empty_map(api, ctx):
    mp = api.Map(ctx, api.Cloud(ctx, np.zeros((0, 3), np.float32)), 0.5)
    feat, st = mp.compute_fpfh(0.5)                                  # no normals either: an empty map is SF_OK before that matters
    assert len(feat) == 0 and {k: st[k] for k in STAT_KEYS} == dict.fromkeys(STAT_KEYS, 0)
    rows, valid = feat.download()
    assert rows.shape == (0, 33) and valid.shape == (0,)
    counts, pairs = mp.compute_spfh(0.5)
    assert counts.shape == (0, 33) and pairs.shape == (0,)
    feat2, st2 = api.Cloud(ctx, np.zeros((0, 3), np.float32)).compute_fpfh(0.3, 0.5)
    assert len(feat2) == 0 and st2["n_points"] == 0


def test_radius_below_one_cell(api, ctx):
    _, pairs, _, valid = check_against_reference(api, ctx, "scene_below_cell")
    assert valid.sum() > 2500 and not valid.all()                   # the isolated points have no pair


def test_radius_of_two_and_a_half_cells(api, ctx):
    _, pairs, _, _ = check_against_reference(api, ctx, "scene_reach3")
    assert pairs.max() > 40


def test_two_cell_sizes_on_one_cloud(api, ctx):
    a = check_against_reference(api, ctx, "scene_reach3", cell=0.1)
    b = check_against_reference(api, ctx, "scene_reach3", cell=0.37)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    assert spacing_ok(a[2], b[2]).mean() > 0.99                     # both within a spacing of the reference, hence within two of each other


def test_duplicates_parallel_offsets_nonfinite_points_and_missing_normals(api, ctx):
    counts, pairs, rows, valid = check_against_reference(api, ctx, "special")
    n = len(pairs)
    assert np.all(pairs[n - 5:] == 0) and np.all(pairs[20:32] == 0) and not valid[n - 5:].any() and not valid[20:32].any()
    assert np.array_equal(counts[n - 15:n - 5], counts[:10]) and valid[:10].all()


@pytest.mark.parametrize("name", ["orient_none", "orient_direction", "orient_viewpoint", "orient_inside"])
def test_orientation_modes(api, ctx, name):
    _, _, rows, valid = check_against_reference(api, ctx, name)
    assert valid.sum() > 600
    if name == "orient_inside":                                      # the viewpoint inside the sphere flips every outward normal
        f = ref.fixtures()[name]
        mp = api.Map(ctx, api.Cloud(ctx, f["points"]), f["cell"])
        mp.set_normals(-f["normals"])
        flipped, _ = mp.compute_fpfh(f["radius"])
        assert np.array_equal(flipped.download()[0], rows)
        assert np.array_equal(mp.download_normals()[0], -f["normals"])    # the stored normals stay as they are


def test_two_runs_are_bitwise_equal_and_timed_when_asked(api, ctx):
    f = ref.fixtures()["scene_reach3"]
    mp = build(api, ctx, f)
    index_before = mp.index()
    a, sa = mp.compute_fpfh(f["radius"], profile=True)
    b, sb = mp.compute_fpfh(f["radius"])
    ra, rb = a.download(), b.download()
    assert np.array_equal(ra[0].view(np.uint32), rb[0].view(np.uint32)) and np.array_equal(ra[1], rb[1])
    assert sa["spfh_ms"] > 0 and sa["fpfh_ms"] > 0 and sb["spfh_ms"] == -1.0
    assert {k: sa[k] for k in STAT_KEYS} == {k: sb[k] for k in STAT_KEYS}
    after = mp.index()
    assert np.array_equal(index_before["pts4"].view(np.uint32), after["pts4"].view(np.uint32)) and np.array_equal(index_before["cell_start"], after["cell_start"])
    assert np.array_equal(mp.download_normals()[0], f["normals"])


def test_cloud_form_equals_the_three_map_calls(api, ctx):
    pts, _ = ref.scene_cloud(1500, 9)
    pts = np.concatenate([pts, np.float32([[np.nan, 0, 0]])])
    cloud = api.Cloud(ctx, pts)
    feat, st = cloud.compute_fpfh(0.3, 0.25, "direction", (0, 0, 1), cell=0.2)
    assert np.array_equal(cloud.download().view(np.uint32), pts.view(np.uint32))      # not modified
    mp = api.Map(ctx, api.Cloud(ctx, pts), 0.2)
    mp.estimate_normals(0.3)
    want, wst = mp.compute_fpfh(0.25, "direction", (0, 0, 1))
    got_rows, got_valid = feat.download()
    want_rows, want_valid = want.download()
    assert np.array_equal(got_rows.view(np.uint32), want_rows.view(np.uint32)) and np.array_equal(got_valid, want_valid)
    assert st == wst and st["n_featured"] > 1000 and st["n_valid"] == 1500 and not got_valid[-1]


def test_a_map_without_normals_is_a_state_error(api, ctx):
    mp = api.Map(ctx, api.Cloud(ctx, ref.sphere_cloud(50, 1)[0]), 0.3)
    with pytest.raises(api.SlamFusionError, match="error -4"):
        mp.compute_fpfh(0.3)
    with pytest.raises(api.SlamFusionError, match="error -4"):
        mp.compute_spfh(0.3)
    with pytest.raises(api.SlamFusionError, match="error -4"):
        api.Map(ctx).compute_fpfh(0.3)                               # not built


def test_invalid_arguments_touch_nothing(api, ctx):
    f = ref.fixtures()["sphere65"]
    mp = build(api, ctx, f)
    lib = api.load_library()
    seed_rows = ref.descriptor_rows(5, 4)
    out = api.Features(ctx, seed_rows)
    counts, pairs = np.full((65, 33), 7, np.uint32), np.full(65, 7, np.int32)
    st = api.FpfhStats(9, 9, 9, 9, 9, 9.0, 9.0)
    nan, inf = float("nan"), float("inf")
    bad = [(0.0, 0, (0, 0, 1)), (-1.0, 0, (0, 0, 1)), (nan, 0, (0, 0, 1)), (inf, 0, (0, 0, 1)), (0.3, 3, (0, 0, 1)), (0.3, -1, (0, 0, 1)),
           (0.3, 1, (nan, 0, 1)), (0.3, 2, (0, inf, 1))]
    for radius, orient, toward in bad:
        p = api._fpfh_params(radius, orient, toward, False)
        assert lib.sf_map_compute_fpfh(mp.h, C.byref(p), out.h, C.byref(st)) == -1, (radius, orient, toward)
        assert lib.sf_map_compute_spfh(mp.h, C.byref(p), counts.ctypes.data_as(C.c_void_p), pairs.ctypes.data_as(C.c_void_p)) == -1
        cloud = api.Cloud(ctx, f["points"])
        assert lib.sf_cloud_compute_fpfh(cloud.h, C.c_double(0.3), C.byref(p), C.c_float(0), out.h, C.byref(st)) == -1
    good = api._fpfh_params(0.3, 0, (0, 0, 1), False)
    cloud = api.Cloud(ctx, f["points"])
    for normal_radius in (0.0, -1.0, nan, inf):
        assert lib.sf_cloud_compute_fpfh(cloud.h, C.c_double(normal_radius), C.byref(good), C.c_float(0), out.h, C.byref(st)) == -1
    assert lib.sf_map_compute_fpfh(mp.h, None, out.h, C.byref(st)) == -1 and lib.sf_map_compute_fpfh(mp.h, C.byref(good), None, C.byref(st)) == -1
    rows, valid = out.download()
    assert len(out) == 5 and np.array_equal(rows, seed_rows) and valid.all()
    assert np.all(counts == 7) and np.all(pairs == 7) and st.n_points == 9 and st.spfh_ms == 9.0
    assert np.array_equal(cloud.download(), f["points"])
    other = api.Context(0)                                           # a feature set of another context
    foreign = api.Features(other)
    assert lib.sf_map_compute_fpfh(mp.h, C.byref(good), foreign.h, C.byref(st)) == -1
    foreign.close()
    other.close()
