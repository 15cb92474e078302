"""Per-label boxes and multi-box removal on the device (sf_cloud_label_boxes, sf_cloud_cluster_boxes, sf_cloud_remove_boxes; DESIGN
section 19) against the numpy restatement of the rule (tests/box_ref_np.py), which tests/test_box_rule.py pins to independent code.
Counts, minima, maxima, flags and statistics are compared exactly.  Sums are compared within the bound of a sum in any order,
computed from the data (box_ref_np.moment_bounds); what follows from the returned axes is recomputed from the returned axes."""
import ctypes

import numpy as np
import pytest

import box_ref_np as ref
from test_gpu_knn_normals import noisy_map  # noqa: F401  (the fixture: [1] is 3 000 mixed points plus 20 isolated ones)

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
INVALID = "error -1:"
STAT_KEYS = ("n_points", "n_labelled", "n_ignored", "n_nonfinite", "n_labels", "n_valid")


@pytest.fixture(scope="module")
def blobs():
    x, labels = ref.aniso_blob_cloud()
    x.setflags(write=False)
    labels.setflags(write=False)
    return x, labels


@pytest.fixture(scope="module")
def mixed(noisy_map):  # noqa: F811
    x = noisy_map[1]
    labels, n_labels = ref.grid_labels(x)
    return x, labels, n_labels


def check_exact(boxes, st, x, labels, n_labels, what):
    """count, lo, hi, valid and the stats against the restatement, exactly; an empty label is zeros throughout"""
    want, wst = ref.label_boxes(x, labels, n_labels, "aabb")
    assert boxes.dtype == ref.BOX_DTYPE and boxes.shape == (n_labels,), what
    for key in ("count", "lo", "hi"):
        assert np.array_equal(boxes[key], want[key]), (what, key)
    assert np.array_equal(boxes["valid"] != 0, want["valid"] != 0), what
    assert {k: st[k] for k in STAT_KEYS} == wst, (what, st, wst)
    empty = boxes[boxes["count"] == 0]
    assert not np.frombuffer(empty.tobytes(), np.uint8).any(), what
    return want


def check_moments(boxes, x, labels, what):
    """mean and cov within the bound of their sums (any order), propagated through the two formulas -> worst |error| / bound"""
    worst = 0.0
    for l in np.flatnonzero(boxes["count"] > 0):
        pts = x[(labels == l) & np.isfinite(x).all(1)]
        _, _, mean, cov, bmean, bcov = ref.moment_bounds(pts, ref.pivot(boxes["lo"][l], boxes["hi"][l]))
        em, ec = np.abs(boxes["mean"][l] - mean), np.abs(boxes["cov"][l] - cov)
        assert (em <= bmean).all() and (ec <= bcov).all(), (what, l, em, bmean, ec, bcov)
        worst = max(worst, (em / np.maximum(bmean, 1e-300)).max(), (ec / np.maximum(bcov, 1e-300)).max())
    return worst


def check_axes(boxes, mode, up, what):
    """R orthonormal (32 eps, jacobi3's limit) and right-handed, the sign rule, R^T C R diagonal with descending values.
    jacobi3 is held to V diag V^T = C within 64 eps |C| and V^T V = I within 32 eps (tests/test_gpu_linalg_direct.py), so
    v_i^T C v_j = (V^T V L V^T V)_ij + v_i^T E v_j: at most 2 x 32 eps |C| + |E|_2 <= 3 x 64 eps |C|, 256 eps |C| in all; a2 = a0 x a1
    lies within the same 32 eps of the third eigenvector, 128 eps |C| more: 384 eps |C|_2 for the off-diagonal, and the diagonal equals
    the eigenvalues within 64 + 64 eps |C|.  UPRIGHT: one closed-form rotation, asserted at the same limit."""
    u = ref.unit_up(up)
    for l in np.flatnonzero(boxes["count"] > 0):
        R, C, lam = boxes["R"][l], ref.cov_matrix(boxes["cov"][l]), boxes["eigenvalues"][l]
        norm = np.linalg.norm(C, 2)
        if mode == "aabb" or boxes["valid"][l] == 2:
            assert np.array_equal(R, np.eye(3)), (what, l)
            continue
        assert np.abs(R.T @ R - np.eye(3)).max() <= 32 * EPS and np.linalg.det(R) > 0, (what, l)
        D = R.T @ C @ R
        if mode == "pca":
            for k in range(2):
                col = R[:, k]
                m = int(np.argmax(np.abs(col)))                                   # (argmax: the first of equal magnitudes)
                assert col[m] > 0 or not col.any(), (what, l, k)
            assert lam[0] >= lam[1] >= lam[2], (what, l)
            assert np.abs(D - np.diag(np.diag(D))).max() <= 384 * EPS * norm, (what, l, D)
        else:
            assert np.array_equal(R[:, 2], u), (what, l)
            assert R[int(np.argmax(np.abs(R[:, 0]))), 0] > 0, (what, l)
            assert abs(D[0, 1]) <= 384 * EPS * norm, (what, l, D)
        assert np.abs(np.diag(D) - lam).max() <= 128 * EPS * norm, (what, l)


def check_extent(boxes, x, labels, what):
    """center and extent against the numpy min / max of d . a_k along the RETURNED axes, to 4 float64 ulps of the half-diagonal"""
    for l in np.flatnonzero(boxes["count"] > 0):
        pts = x[(labels == l) & np.isfinite(x).all(1)]
        b = boxes[l]
        center, extent = ref.center_extent(pts, ref.pivot(b["lo"], b["hi"]), b["R"])
        tol = 4 * np.spacing(np.linalg.norm(b["hi"].astype(np.float64) - b["lo"].astype(np.float64)) / 2)
        assert np.abs(b["center"] - center).max() <= tol and np.abs(b["extent"] - extent).max() <= tol, (what, l, b["center"] - center, b["extent"] - extent, tol)


def run(api, ctx, x, labels, n_labels, mode="pca", up=None, what=None):
    cloud = api.Cloud(ctx, x)
    boxes, st = cloud.label_boxes(labels, n_labels, mode, up)
    assert np.array_equal(cloud.download(), x, equal_nan=True)                    # the cloud is not modified
    cloud.close()
    check_exact(boxes, st, x, labels, n_labels, what)
    worst = check_moments(boxes, x, labels, what)
    check_axes(boxes, mode, up, what)
    check_extent(boxes, x, labels, what)
    print("%s: %d labels, %d valid, worst moment error / bound %.3f" % (what, n_labels, st["n_valid"], worst))
    return boxes, st


# ------------------------------------------------------------------ 1. the two clouds, the three modes
@pytest.mark.parametrize("mode", ["aabb", "pca", "upright"])
def test_blobs(api, ctx, blobs, mode):
    x, labels = blobs
    boxes, st = run(api, ctx, x, labels, 25, mode, None, "blobs " + mode)
    assert st["n_valid"] == 25 and st["n_ignored"] == 2000 and st["device_ms"] == -1.0


@pytest.mark.parametrize("mode", ["aabb", "pca", "upright"])
def test_mixed(api, ctx, mixed, mode):
    x, labels, n_labels = mixed
    run(api, ctx, x, labels, n_labels, mode, None, "mixed " + mode)


def test_pca_axes_agree_with_eigh_within_davis_kahan(api, ctx, blobs):
    """On the well-separated fixture (adjacent eigenvalue ratios >= 2: tests/test_box_rule.py) axis k agrees with eigh's up to
    sin(angle) <= 2 |dC|_2 / gap_k (Davis-Kahan).  dC: the covariance bound of check_moments (Frobenius norm of the bound matrix),
    plus what the two solvers are held to themselves, 64 eps |C| each (jacobi3's reconstruction limit; LAPACK's backward error is
    below it)."""
    x, labels = blobs
    for data, what in ((x, "blobs"), ((x.astype(np.float64) + 1000.0).astype(np.float32), "blobs + 1 km")):
        cloud = api.Cloud(ctx, data)
        boxes, _ = cloud.label_boxes(labels, 25, "pca")
        cloud.close()
        worst = 0.0
        for l in range(25):
            pts = data[labels == l]
            _, _, _, cov, _, bcov = ref.moment_bounds(pts, ref.pivot(boxes["lo"][l], boxes["hi"][l]))
            C = ref.cov_matrix(cov)
            lam, V = np.linalg.eigh(C)
            lam, V = lam[::-1], V[:, ::-1]
            dC = np.linalg.norm(ref.cov_matrix(bcov), "fro") + 128 * EPS * lam[0]
            gaps = (lam[0] - lam[1], min(lam[0] - lam[1], lam[1] - lam[2]), lam[1] - lam[2])
            for k in range(3):
                sin = np.linalg.norm(np.cross(boxes["R"][l][:, k], V[:, k]))
                assert sin <= 2 * dC / gaps[k], (what, l, k, sin, 2 * dC / gaps[k])
                worst = max(worst, sin / (2 * dC / gaps[k]))
        print("%s: worst sin(angle to eigh) / Davis-Kahan bound %.3f" % (what, worst))


# ------------------------------------------------------------------ 2. shapes
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_small_sizes(api, ctx, blobs, n):
    x, labels = blobs
    boxes, st = run(api, ctx, x[:n].copy(), labels[:n].copy(), 25, "pca", None, "n = %d" % n)
    if n == 0:
        assert st["n_valid"] == 0 and not boxes["valid"].any()


def test_every_point_its_own_label(api, ctx, mixed):
    x = mixed[0]
    labels = np.random.default_rng(2).permutation(len(x)).astype(np.int32)
    boxes, st = run(api, ctx, x, labels, len(x), "pca", None, "n_labels = n")
    assert st["n_valid"] == len(x) and (boxes["count"] == 1).all() and not boxes["extent"].any() and not boxes["cov"].any()
    assert np.array_equal(boxes["center"][labels], x.astype(np.float64)) and np.array_equal(boxes["mean"][labels], x.astype(np.float64))


def test_one_label_holds_every_point(api, ctx, blobs):
    x, _ = blobs
    boxes, st = run(api, ctx, x, np.zeros(len(x), np.int32), 1, "pca", None, "one label")   # 79 workgroups, 158 partial rows, one run
    assert boxes["count"][0] == len(x)


def test_empty_labels_out_of_range_and_non_finite(api, ctx, blobs):
    x, labels = blobs
    x, labels = x.copy(), labels.copy()
    labels = np.where(labels >= 0, 2 * labels + 1, -1).astype(np.int32)              # every even label is empty
    labels[100:140] = 51 + 3                                                         # beyond n_labels
    labels[140:150] = -5
    labels[150:160] = np.iinfo(np.int32).max
    x[200:220, 0], x[220:230, 1], x[230:235, 2] = np.nan, np.inf, -np.inf            # members and ignored points alike
    boxes, st = run(api, ctx, x, labels, 51, "pca", None, "gaps")
    assert not boxes["valid"][::2].any() and boxes["valid"][1::2].all() and st["n_nonfinite"] > 0
    boxes, st = run(api, ctx, x, labels, 0, "pca", None, "no label at all")
    assert st["n_ignored"] == len(x) and st["n_labelled"] == 0


def test_coincident_points(api, ctx):
    x = np.concatenate([np.tile(np.float32([1.5, -2.25, 0.125]), (300, 1)), np.tile(np.float32([7, 7, 7]), (2, 1)), np.float32([[0, 0, 0], [0, 0, 1]])])
    labels = np.array([0] * 300 + [1] * 2 + [2] * 2, np.int32)
    for mode in ("aabb", "pca", "upright"):
        boxes, st = run(api, ctx, x, labels, 3, mode, None, "coincident " + mode)
        assert not boxes["cov"][:2].any() and not boxes["extent"][:2].any() and (mode == "upright" or np.array_equal(boxes["R"][0], np.eye(3)))
        assert np.array_equal(boxes["center"][0], [1.5, -2.25, 0.125]) and np.array_equal(boxes["mean"][1], [7, 7, 7])
        assert sorted(boxes["extent"][2]) == [0, 0, 1]


def test_a_cloud_one_kilometre_out(api, ctx, blobs):
    x, labels = blobs
    far = (x.astype(np.float64) + np.array([1000.0, -1000.0, 1000.0])).astype(np.float32)
    boxes, _ = run(api, ctx, far, labels, 25, "pca", None, "1 km")
    near, _ = ref.label_boxes(x, labels, 25, "pca")
    assert np.abs(boxes["extent"] - near["extent"]).max() <= 1e-3                    # float32 coordinates at 1 km: 6e-5 m each


def test_the_pass_that_walks_several_tiles(api, ctx, blobs):
    """the hook caps the grid of the segmented passes: one workgroup carries the open run from tile to tile (max_blocks 1), three
    workgroups take 27 tiles each -- the path production takes from 262 145 points on"""
    x, labels = blobs
    cloud = api.Cloud(ctx, x)
    base, bst = cloud.label_boxes(labels, 25, "pca")
    for lab, n_labels in ((labels, 25), (np.zeros(len(x), np.int32), 1)):
        for max_blocks in (1, 3, 50):
            boxes, st = api.hook_label_boxes(cloud, lab, n_labels, "pca", None, max_blocks)
            what = "max_blocks %d, %d labels" % (max_blocks, n_labels)
            check_exact(boxes, st, x, lab, n_labels, what)
            check_moments(boxes, x, lab, what)
            check_axes(boxes, "pca", None, what)
            check_extent(boxes, x, lab, what)
    boxes, st = api.hook_label_boxes(cloud, labels, 25, "pca", None, 0)
    assert boxes.tobytes() == base.tobytes()
    cloud.close()


# ------------------------------------------------------------------ 3. upright
def test_upright_about_a_segmented_ground_normal(api, ctx, blobs):
    x, labels = blobs
    rng = np.random.default_rng(12)
    ground = np.stack([rng.uniform(-8, 8, 12000), rng.uniform(-8, 8, 12000), np.full(12000, -6.5)], 1)
    scene, up_true = ref.tilted(np.concatenate([x.astype(np.float64), ground]), 3.0)
    lab = np.concatenate([labels, np.full(12000, -1, np.int32)])
    cloud = api.Cloud(ctx, scene)
    plane, inlier, pst = cloud.segment_plane(0.05, 1024, seed=4)        # a third of the points lie on the ground: ~38 of the samples do
    cloud.close()
    assert pst["found"] and inlier[-12000:].all() and abs(float(plane[:3] @ up_true)) > 0.9999
    up = plane[:3].astype(np.float64)
    boxes, _ = run(api, ctx, scene, lab, 25, "upright", up, "upright about the ground normal")
    flat, _ = run(api, ctx, x, labels, 25, "upright", (0, 0, 1), "upright about +z")
    # the tilt turns the scene rigidly and the normal with it: the boxes keep their sizes within the float32 rounding of the turned
    # points (1e-6 m) and of the fitted normal (1e-7 of a 4 m blob)
    assert np.abs(boxes["extent"] - flat["extent"]).max() <= 1e-4
    assert np.array_equal(boxes["R"][:, :, 2], np.tile(ref.unit_up(up), (25, 1)))


# ------------------------------------------------------------------ 4. the same bits every time
def test_five_calls_give_equal_bits(api, ctx, blobs, mixed):
    for x, labels, n_labels in ((blobs[0], blobs[1], 25), mixed, (blobs[0], np.zeros(len(blobs[0]), np.int32), 1)):
        cloud = api.Cloud(ctx, x)
        for mode in ("pca", "upright"):
            first = cloud.label_boxes(labels, n_labels, mode)[0].tobytes()
            for _ in range(4):
                assert cloud.label_boxes(labels, n_labels, mode)[0].tobytes() == first
        cloud.close()


def test_profile_reports_a_device_time(api, ctx, blobs):
    cloud = api.Cloud(ctx, blobs[0])
    plain = cloud.label_boxes(blobs[1], 25)
    timed = cloud.label_boxes(blobs[1], 25, profile=True)
    cloud.close()
    assert plain[1]["device_ms"] == -1.0 and 0.0 < timed[1]["device_ms"] < 1000.0 and plain[0].tobytes() == timed[0].tobytes()


# ------------------------------------------------------------------ 5. members against the crop
def test_members_pass_crop_obb(api, ctx, blobs):
    """Every member passes sf_cloud_crop_obb with its label's (center, R, extent).  tests/test_box_rule.py::
    test_center_rounding_needs_a_margin shows on the restatement that the rounding of center needs a margin (53 of 18 000 members lie
    outside at margin 0), so the margin is one float64 ulp of the (largest) extent, through sf_cloud_remove_boxes, whose predicate at
    margin 0 is the crop's (test_one_box_equals_crop_obb).  The restatement loses no member at that margin -- its worst excess is
    exactly that ulp -- because center is the rule's exact value rounded once; evaluated with three roundings it lost 4 and the device 5."""
    x, labels = blobs
    cloud = api.Cloud(ctx, x)
    boxes, _ = cloud.label_boxes(labels, 25, "pca")
    cloud.close()
    outside = 0
    for l in range(25):
        pts = x[labels == l]
        b = boxes[l]
        margin = np.spacing(b["extent"].max())
        cloud = api.Cloud(ctx, pts)
        inside = cloud.remove_boxes((b["center"], b["R"], b["extent"]), margin=margin, keep_inside=True)
        cloud.close()
        want = int(ref.inside_any(pts, b["center"], b["R"], b["extent"], margin).sum())
        assert inside == want, (l, inside, want)                                   # the device's predicate is the restatement's
        outside += len(pts) - inside
    print("members outside their own box at one ulp of the extent: %d" % outside)
    assert outside == 0


# ------------------------------------------------------------------ 6. cluster_boxes
def test_cluster_boxes_equal_label_boxes_of_the_cluster_labels(api, ctx, blobs):
    x, _ = blobs
    src = api.Cloud(ctx, x)
    mp = api.Map(ctx, src, 0.25)
    labels, sizes, cst = mp.cluster_euclidean(0.2, 5, 0)
    mp.close()
    want, wst = src.label_boxes(labels, len(sizes), "pca")
    assert len(sizes) >= 2 and np.array_equal(want["count"], sizes)
    for cell in (0.0, 0.2, 0.7):
        boxes, gcst, bst = src.cluster_boxes(0.2, 5, 0, cell, "pca")
        assert boxes.tobytes() == want.tobytes(), cell
        assert gcst == cst and {k: bst[k] for k in STAT_KEYS} == {k: wst[k] for k in STAT_KEYS}, cell
        assert len(src) == len(x) and np.array_equal(src.download(), x)            # the cloud is left alone
    for mode, up in (("aabb", None), ("upright", (0.1, 0.0, 1.0))):
        assert src.cluster_boxes(0.2, 5, 0, 0.0, mode, up)[0].tobytes() == src.label_boxes(labels, len(sizes), mode, up)[0].tobytes()
    # cap_boxes: the first cap boxes in label order, nothing beyond them
    cap = 7
    out = np.zeros(cap + 2, api.LABEL_BOX_DTYPE)
    out["pad"][cap:] = 77
    p, cs, bs = api.BoxParams(mode=1), api.ClusterStats(), api.BoxStats()
    rc = src.lib.sf_cloud_cluster_boxes(src.h, 0.2, 5, 0, 0.0, ctypes.byref(p), out.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(cs), ctypes.byref(bs))
    assert rc == 0 and out[:cap].tobytes() == want[:cap].tobytes() and (out["pad"][cap:] == 77).all() and not out["count"][cap:].any()
    assert cs.n_clusters == len(sizes) and bs.n_valid == len(sizes)
    src.close()
    empty = api.Cloud(ctx, np.zeros((0, 3), np.float32))
    boxes, gcst, bst = empty.cluster_boxes(0.2)
    assert len(boxes) == 0 and gcst["n_clusters"] == 0 and bst["n_points"] == 0
    empty.close()


# ------------------------------------------------------------------ 7. remove_boxes
@pytest.fixture(scope="module")
def box_sets():
    rng = np.random.default_rng(21)
    return {count: ref.random_boxes(rng, count) for count in (1, 40, 1024)}


@pytest.mark.parametrize("count", [1, 40, 1024])
@pytest.mark.parametrize("keep_inside", [False, True])
def test_remove_boxes_equals_the_restatement(api, ctx, blobs, box_sets, count, keep_inside):
    x = blobs[0].copy()
    x[7], x[8], x[9] = (np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)
    center, R, extent = box_sets[count]
    if count == 1024:
        extent = extent * 0.2                                                        # (so that the boxes do not cover everything)
    for margin in (0.0, 0.1):
        inside = ref.inside_any(x, center, R, extent, margin)
        keep = inside if keep_inside else ~inside
        cloud = api.Cloud(ctx, x)
        n_inside = cloud.remove_boxes((center, R, extent), margin, keep_inside)
        assert n_inside == inside.sum() and n_inside < len(x) and (count == 1 or n_inside > 0), (count, margin)
        assert np.array_equal(cloud.last_indices(), np.flatnonzero(keep)) and np.array_equal(cloud.download(), x[keep], equal_nan=True)
        cloud.close()
    assert not inside[7:10].any()


def test_one_box_equals_crop_obb(api, ctx, blobs, box_sets):
    x, total = blobs[0], 0
    for k in range(10):
        center, R, extent = (a[k] for a in box_sets[40])
        extent = extent * 3
        a, b = api.Cloud(ctx, x), api.Cloud(ctx, x)
        a.crop_obb(center, R, extent)
        n_inside = b.remove_boxes((center[None], R[None], extent[None]), 0.0, True)
        assert n_inside == len(a) == len(b) and np.array_equal(a.last_indices(), b.last_indices()) and np.array_equal(a.download(), b.download())
        total += n_inside
        a.close()
        b.close()
    assert total > 0


def test_remove_boxes_takes_label_boxes_and_no_boxes(api, ctx, blobs):
    x, labels = blobs
    cloud = api.Cloud(ctx, x)
    boxes, _ = cloud.label_boxes(np.where(labels >= 0, 2 * labels, -1), 50, "pca")   # half of the entries are invalid and skipped
    n_inside = cloud.remove_boxes(boxes, margin=0.05)
    want = ref.inside_any(x, boxes["center"][::2], boxes["R"][::2], boxes["extent"][::2], 0.05)
    assert n_inside == want.sum() >= 18_000 and np.array_equal(cloud.last_indices(), np.flatnonzero(~want))
    none = (np.zeros((0, 3)), np.zeros((0, 3, 3)), np.zeros((0, 3)))
    n = len(cloud)
    assert cloud.remove_boxes(none) == 0 and len(cloud) == n and np.array_equal(cloud.last_indices(), np.arange(n))
    assert cloud.remove_boxes(none, keep_inside=True) == 0 and len(cloud) == 0 and len(cloud.last_indices()) == 0
    assert cloud.remove_boxes(boxes) == 0 and len(cloud) == 0                       # an empty cloud
    cloud.close()


def test_refused_arguments(api, ctx, blobs):
    x, labels = blobs
    cloud = api.Cloud(ctx, x[:500].copy())
    lab = labels[:500]
    for kwargs in (dict(n_labels=-1), dict(n_labels=(1 << 24) + 1), dict(n_labels=25, mode=7), dict(n_labels=25, mode="upright", up=(0, np.nan, 1)),
                   dict(n_labels=25, up=(np.inf, 0, 0))):
        with pytest.raises(api.SlamFusionError, match=INVALID):
            cloud.label_boxes(lab, **kwargs)
    with pytest.raises(api.SlamFusionError, match=INVALID):
        api.hook_label_boxes(cloud, lab, 25, max_blocks=-1)
    for args in ((0.0, 1), (0.2, 0), (np.nan, 1)):
        with pytest.raises(api.SlamFusionError, match=INVALID):
            cloud.cluster_boxes(*args)
    with pytest.raises(api.SlamFusionError, match=INVALID):
        cloud.cluster_boxes(0.2, mode=9)
    rng = np.random.default_rng(1)
    with pytest.raises(api.SlamFusionError, match=INVALID):
        cloud.remove_boxes(ref.random_boxes(rng, 1025))
    with pytest.raises(api.SlamFusionError, match=INVALID):
        cloud.remove_boxes(ref.random_boxes(rng, 2), margin=np.nan)
    assert len(cloud) == 500 and np.array_equal(cloud.download(), x[:500])          # nothing touched
    cloud.close()
