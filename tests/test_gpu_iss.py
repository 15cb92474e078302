"""sf_map_iss_saliency / sf_map_iss_keypoints / sf_cloud_iss_keypoints / sf_features_gather on the device against the numpy
restatement (tests/iss_ref_np.py).

Counts: equal.  lambda: within iss_ref_np.tol(count, salient_radius) per eigenvalue (the derivation is in that file).  Salient
flags: equal to the restatement's on every fixture (tests/test_iss_rule.py asserts on the CPU that none hangs on a rounding), and
equal bit for bit to the rule applied to the device's OWN lambda and counts.  Keypoint flags and indices: equal to the rule applied
to the device's own lambda3 and salient flags on every fixture, and to the restatement's where the fixture allows (exact_nms).
Every fixture finishes in well under a second on the device; the restatement of each is computed once per session."""
import ctypes as C

import numpy as np
import pytest

import fpfh_ref_np as fp
import iss_ref_np as ref

pytestmark = pytest.mark.gpu

WORST = {"ratio": 0.0}      # the largest |lambda_device - lambda_numpy| / tol seen in this session (printed by the last test)


def run(api, ctx, f, cell):
    mp = api.Map(ctx, api.Cloud(ctx, f["points"]), cell)
    p = ref.params(f)
    sal = mp.iss_saliency(p["salient_radius"], p["non_max_radius"], p["gamma_21"], p["gamma_32"], p["min_neighbors"], p["min_lambda3"])
    kp = mp.iss_keypoints(**p)
    mp.close()
    return sal, kp


def check(api, ctx, name, cell=None):
    f, want = ref.fixture(name), ref.reference(name)
    p, pts = ref.params(f), f["points"]
    for c in (f["cells"] if cell is None else (cell,)):
        sal, kp = run(api, ctx, f, c)
        lam, cnt = sal["lambda"], sal["n_neighbors"]
        assert np.array_equal(cnt, want["n_neighbors"]), (name, c)
        t = ref.tol(cnt, p["salient_radius"])[:, None]
        err = np.abs(lam - want["lambda"])
        if len(pts):
            WORST["ratio"] = max(WORST["ratio"], float((err / t).max()))
            print("%s cell %g: keypoints %d of %d salient, largest |lambda - numpy| / tol %.3g" % (name, c, kp["stats"]["n_keypoints"], kp["stats"]["n_salient"], (err / t).max()))
        assert np.all(err <= t), (name, c, float((err / t).max()))
        assert np.all(lam[:, 0] >= lam[:, 1]) and np.all(lam[:, 1] >= lam[:, 2]) and np.all(lam[:, 2] >= 0)
        # the device's own rule, bit for bit
        own = ref.salient_rule(lam, cnt, p["gamma_21"], p["gamma_32"], p["min_neighbors"], p["min_lambda3"])
        assert np.array_equal(sal["salient"], own), (name, c)
        own_flags, nms_count = ref.nms_rule(pts, lam[:, 2], sal["salient"], p["non_max_radius"], p["min_neighbors"])
        assert np.array_equal(kp["flags"], own_flags), (name, c)
        assert np.array_equal(kp["indices"], np.flatnonzero(own_flags).astype(np.int32)) and kp["indices"].dtype == np.int32
        assert np.array_equal(nms_count, want["nms_count"])
        # the restatement
        assert np.array_equal(sal["salient"], want["salient"]), (name, c)
        st = kp["stats"]
        assert (st["n_points"], st["n_valid"], st["n_salient"], st["max_neighbors"]) == tuple(want["stats"][k] for k in ("n_points", "n_valid", "n_salient", "max_neighbors"))
        assert st["n_keypoints"] == int(kp["flags"].sum()) and st["saliency_ms"] == -1.0 and st["nms_ms"] == -1.0
        if f["exact_nms"]:
            assert np.array_equal(kp["flags"], want["flags"]) and np.array_equal(kp["indices"], want["indices"]), (name, c)
    return sal, kp


@pytest.mark.parametrize("name", ["all%d" % n for n in (0, 1, 2, 4, 5, 6)] + ["sphere%d" % n for n in (63, 64, 65, 257)])
def test_wave_and_block_edges(api, ctx, name):
    sal, kp = check(api, ctx, name)
    n = len(ref.fixture(name)["points"])
    if name.startswith("all"):
        assert kp["stats"]["n_keypoints"] == (1 if n >= 5 else 0) and kp["stats"]["n_salient"] == (n if n >= 5 else 0)     # min_neighbors = 5 turns at n = 5
    else:
        assert kp["stats"]["n_keypoints"] >= 1


def test_radius_below_one_cell(api, ctx):
    _, kp = check(api, ctx, "scene_below_cell")
    assert kp["stats"]["n_keypoints"] > 100


def test_radius_of_two_and_a_half_cells_and_other_parameters(api, ctx):
    _, kp = check(api, ctx, "scene_reach3")
    assert kp["stats"]["max_neighbors"] > 40 and kp["stats"]["n_keypoints"] > 50
    check(api, ctx, "scene_loose")


def test_two_cell_sizes_move_lambda_by_rounding_only(api, ctx):
    f = ref.fixture("scene_reach3")
    (sa, ka), (sb, kb) = run(api, ctx, f, 0.1), run(api, ctx, f, 0.37)
    assert np.array_equal(sa["n_neighbors"], sb["n_neighbors"]) and np.array_equal(sa["salient"], sb["salient"]) and np.array_equal(ka["indices"], kb["indices"])
    assert np.all(np.abs(sa["lambda"] - sb["lambda"]) <= ref.tol(sa["n_neighbors"], f["salient_radius"])[:, None])


def test_the_lattice_has_its_closed_form_and_one_keypoint(api, ctx):
    sal, kp = check(api, ctx, "lattice")
    want = 0.25 ** 2 * np.array([2.0, 1.25, 2.0 / 3.0])
    assert np.all(np.abs(sal["lambda"] - want) <= ref.tol(60, 2.0)) and sal["salient"].all()
    assert kp["stats"]["n_keypoints"] == 1 and kp["flags"].sum() == 1 and len(kp["indices"]) == 1


def test_coincident_points_keep_the_smaller_index(api, ctx):
    sal, kp = check(api, ctx, "ties")
    first, second = np.arange(100, 140), np.arange(800, 840)
    assert np.array_equal(sal["lambda"][first].view(np.uint64), sal["lambda"][second].view(np.uint64))       # the same neighbours in the same order
    assert kp["flags"][first].sum() >= 1 and not kp["flags"][second].any()


def test_nonfinite_points_get_zeros_and_are_never_neighbours(api, ctx):
    sal, kp = check(api, ctx, "nonfinite")
    bad = ~np.isfinite(ref.fixture("nonfinite")["points"]).all(1)
    assert bad.sum() == 4 and np.all(sal["lambda"][bad] == 0) and np.all(sal["n_neighbors"][bad] == 0) and not sal["salient"][bad].any() and not kp["flags"][bad].any()
    assert kp["stats"]["n_points"] == 604 and kp["stats"]["n_valid"] == 600


def test_the_1024_m_offset(api, ctx):
    _, kp = check(api, ctx, "offset1024")
    assert kp["stats"]["n_keypoints"] > 30


def test_cap_truncates_and_two_runs_are_bitwise_equal(api, ctx):
    f, want = ref.fixture("scene_reach3"), ref.reference("scene_reach3")
    mp = api.Map(ctx, api.Cloud(ctx, f["points"]), 0.1)
    index_before = mp.index()
    lib, p, n = api.load_library(), api._iss_params(profile=True, **ref.params(f)), len(f["points"])
    total = want["stats"]["n_keypoints"]
    outs = []
    for cap in (total + 5, 7, 0, total + 5):
        idx, flags, nk, st = np.full(max(cap, 1), -9, np.int32), np.full(n, 9, np.uint8), C.c_int64(-1), api.IssStats()
        assert lib.sf_map_iss_keypoints(mp.h, C.byref(p), idx.ctypes.data_as(C.c_void_p) if cap else None, C.c_int64(cap), C.byref(nk), flags.ctypes.data_as(C.c_void_p),
                                        C.byref(st)) == 0
        assert nk.value == total == st.n_keypoints
        assert np.array_equal(idx[:min(cap, total)], want["indices"][:min(cap, total)]) and np.all(idx[min(cap, total):] == -9)        # nothing beyond is written
        assert np.array_equal(flags.astype(bool), want["flags"])
        assert st.saliency_ms > 0 and st.nms_ms > 0
        outs.append((idx.copy(), flags.copy()))
    assert np.array_equal(outs[0][0], outs[3][0]) and np.array_equal(outs[0][1], outs[3][1])
    a = mp.iss_saliency(f["salient_radius"], min_lambda3=f["min_lambda3"])
    b = mp.iss_saliency(f["salient_radius"], min_lambda3=f["min_lambda3"])
    assert a["lambda"].tobytes() == b["lambda"].tobytes() and np.array_equal(a["n_neighbors"], b["n_neighbors"]) and np.array_equal(a["salient"], b["salient"])
    # any output may be NULL
    assert lib.sf_map_iss_saliency(mp.h, C.byref(p), None, None, None) == 0
    assert lib.sf_map_iss_keypoints(mp.h, C.byref(p), None, C.c_int64(0), None, None, None) == 0
    after = mp.index()
    assert all(np.array_equal(index_before[k], after[k]) for k in index_before if isinstance(index_before[k], np.ndarray))       # the index is not modified
    # the radius filter's count is this call's count
    assert np.array_equal(mp.radius_outliers(f["salient_radius"], 0)[1], a["n_neighbors"])
    mp.close()


def test_cloud_form_equals_the_two_map_calls(api, ctx):
    f = ref.fixture("nonfinite")
    pts, p = f["points"], ref.params(f)
    cloud = api.Cloud(ctx, pts)
    cloud.subsample(1)
    last_before = cloud.last_indices()
    got = cloud.iss_keypoints(cell=0.16, **p)
    assert np.array_equal(cloud.download().view(np.uint32), pts.view(np.uint32)) and np.array_equal(cloud.last_indices(), last_before)      # not modified
    mp = api.Map(ctx, api.Cloud(ctx, pts), 0.16)
    want = mp.iss_keypoints(**p)
    assert np.array_equal(got["indices"], want["indices"]) and got["stats"] == want["stats"] and len(got["indices"]) > 0
    auto = cloud.iss_keypoints(**p)                                      # cell 0 = automatic
    assert np.array_equal(auto["indices"], want["indices"])
    empty = api.Cloud(ctx, np.zeros((0, 3), np.float32)).iss_keypoints(0.3, 0.2)
    assert len(empty["indices"]) == 0 and empty["stats"] == dict(n_points=0, n_valid=0, n_salient=0, n_keypoints=0, max_neighbors=0, saliency_ms=-1.0, nms_ms=-1.0)
    mp.close()


def test_state_errors_and_an_empty_map(api, ctx):
    with pytest.raises(api.SlamFusionError, match="error -4"):
        api.Map(ctx).iss_keypoints(0.3, 0.2)                             # not built
    with pytest.raises(api.SlamFusionError, match="error -4"):
        api.Map(ctx).iss_saliency(0.3)
    mp = api.Map(ctx, api.Cloud(ctx, np.zeros((0, 3), np.float32)), 0.5)
    kp = mp.iss_keypoints(0.3, 0.2, profile=True)
    assert len(kp["indices"]) == 0 and len(kp["flags"]) == 0 and kp["stats"]["n_points"] == 0 and kp["stats"]["n_keypoints"] == 0
    assert len(mp.iss_saliency(0.3)["lambda"]) == 0


def test_every_refusal_leaves_its_outputs_untouched(api, ctx):
    f = ref.fixture("sphere65")
    pts = f["points"]
    mp, cloud = api.Map(ctx, api.Cloud(ctx, pts), 0.3), api.Cloud(ctx, pts)
    lib, n = api.load_library(), len(pts)
    nan, inf = float("nan"), float("inf")
    good = dict(salient_radius=0.45, non_max_radius=0.3, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, min_lambda3=0.0)
    bad = [dict(salient_radius=v) for v in (0.0, -1.0, nan, inf)] + [dict(non_max_radius=v) for v in (0.0, -1.0, nan, inf)] + \
          [dict(gamma_21=v) for v in (0.0, -0.5, 1.0000001, nan)] + [dict(gamma_32=v) for v in (0.0, 1.5, nan)] + [dict(min_lambda3=v) for v in (-1e-30, nan)] + \
          [dict(min_neighbors=v) for v in (0, -3)]
    idx, flags, nk, st = np.full(n, -9, np.int32), np.full(n, 9, np.uint8), C.c_int64(-7), api.IssStats(-1, -1, -1, -1, -1, 5.0, 5.0)
    lam, cnt, sal = np.full((n, 3), 7.0), np.full(n, -9, np.int32), np.full(n, 9, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def untouched():
        return np.all(idx == -9) and np.all(flags == 9) and nk.value == -7 and st.n_points == -1 and st.saliency_ms == 5.0 and np.all(lam == 7.0) and \
            np.all(cnt == -9) and np.all(sal == 9)

    for change in bad:
        p = api._iss_params(profile=False, **dict(good, **change))
        assert lib.sf_map_iss_keypoints(mp.h, C.byref(p), vp(idx), C.c_int64(n), C.byref(nk), vp(flags), C.byref(st)) == -1, change
        assert lib.sf_cloud_iss_keypoints(cloud.h, C.byref(p), C.c_float(0), vp(idx), C.c_int64(n), C.byref(nk), C.byref(st)) == -1, change
        assert lib.sf_map_iss_saliency(mp.h, C.byref(p), vp(lam), vp(cnt), vp(sal)) == -1, change
        assert untouched(), change
    p = api._iss_params(profile=False, **good)
    assert lib.sf_map_iss_keypoints(mp.h, C.byref(p), vp(idx), C.c_int64(-1), C.byref(nk), vp(flags), C.byref(st)) == -1            # cap < 0
    assert lib.sf_map_iss_keypoints(mp.h, C.byref(p), None, C.c_int64(4), C.byref(nk), vp(flags), C.byref(st)) == -1              # indices NULL, cap > 0
    assert lib.sf_cloud_iss_keypoints(cloud.h, C.byref(p), C.c_float(0), vp(idx), C.c_int64(-1), C.byref(nk), C.byref(st)) == -1
    assert lib.sf_cloud_iss_keypoints(cloud.h, C.byref(p), C.c_float(0), None, C.c_int64(4), C.byref(nk), C.byref(st)) == -1
    assert lib.sf_map_iss_keypoints(mp.h, None, vp(idx), C.c_int64(n), C.byref(nk), vp(flags), C.byref(st)) == -1
    unbuilt = api.Map(ctx)
    assert lib.sf_map_iss_keypoints(unbuilt.h, C.byref(p), vp(idx), C.c_int64(n), C.byref(nk), vp(flags), C.byref(st)) == -4        # SF_ERR_STATE
    assert lib.sf_map_iss_saliency(unbuilt.h, C.byref(p), vp(lam), vp(cnt), vp(sal)) == -4
    assert untouched()
    assert np.array_equal(cloud.download().view(np.uint32), pts.view(np.uint32))
    for obj in (unbuilt, mp, cloud):
        obj.close()


@pytest.mark.parametrize("k", [0, 1, 64, 65, 1000])
def test_features_gather(api, ctx, k):
    rows = fp.descriptor_rows(300, 17)
    valid = np.random.default_rng(18).random(300) < 0.8
    rows[5, 3] = np.nan                                                  # invalid whatever flag came with it
    src = api.Features(ctx, rows, valid)
    src_rows, src_valid = src.download()
    rng = np.random.default_rng(100 + k)
    pick = rng.integers(0, 300, k).astype(np.int64)                      # with repeats once k is large
    if k == 65:
        pick = rng.permutation(300)[:65]
    if k == 1000:
        pick[:300] = rng.permutation(300)                                # a whole permutation, then repeats
    out = src.gather(pick)
    got_rows, got_valid = out.download()
    assert len(out) == k and got_rows.shape == (k, 33)
    assert np.array_equal(got_rows.view(np.uint32), src_rows[pick].view(np.uint32)) and np.array_equal(got_valid, src_valid[pick])
    if k >= 64:
        m = out.match(src)                                               # n_valid travels with the rows
        assert m["stats"]["n_src_valid"] == int(src_valid[pick].sum())
        assert np.all(m["dist2"][got_valid] == 0)
    assert np.array_equal(src.download()[0].view(np.uint32), src_rows.view(np.uint32))      # the source is as it was
    for obj in (out, src):
        obj.close()


def test_features_gather_refusals_leave_out_untouched(api, ctx):
    rows = fp.descriptor_rows(50, 19)
    src, out, other = api.Features(ctx, rows), api.Features(ctx, rows[:7]), api.Context(0)
    foreign = api.Features(other, rows[:3])
    lib = api.load_library()
    before = out.download()

    def gather(src_, picks, out_, k=None):
        a = np.ascontiguousarray(picks, np.int32)
        return lib.sf_features_gather(src_.h, a.ctypes.data_as(C.c_void_p), C.c_int64(len(a) if k is None else k), out_.h)

    for picks in ([0, 50], [-1], [3, 4, 2 ** 31 - 1], list(range(50)) + [50]):
        assert gather(src, picks, out) == -1, picks
        assert b"outside" in lib.sf_last_error()
    assert gather(src, [1, 2], src) == -1                                # out == src
    assert gather(src, [1, 2], foreign) == -1                            # different contexts
    assert gather(src, [1, 2], out, k=-1) == -1                          # k < 0
    assert lib.sf_features_gather(src.h, None, C.c_int64(2), out.h) == -1
    after = out.download()
    assert len(out) == 7 and np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)) and np.array_equal(before[1], after[1])
    assert gather(src, [], out) == 0 and len(out) == 0                   # k = 0 empties out
    empty_src = api.Features(ctx)
    assert gather(empty_src, [0], out) == -1 and len(empty_src.gather([])) == 0
    for obj in (foreign, empty_src, out, src, other):
        obj.close()


def test_the_largest_lambda_ratio_of_this_session():
    """Not a check of its own: prints the largest |lambda_device - lambda_numpy| / tol over everything compared above (DESIGN.md
    section 23 records it); every comparison asserted its own ratio <= 1."""
    print("largest lambda ratio over the session: %.3g" % WORST["ratio"])
    assert WORST["ratio"] <= 1.0
