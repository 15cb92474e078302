"""tests/box_ref_np.py, the numpy restatement of the per-label box rule, against independent code: math.fsum
moments, numpy.linalg.eigh, brute-force corner containment.  No device call.  Also pins the properties of the fixtures that
tests/test_gpu_boxes.py relies on."""
import itertools
import math

import numpy as np
import pytest

import box_ref_np as ref

EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def blobs():
    x, labels = ref.aniso_blob_cloud()
    return x, labels, ref.label_boxes(x, labels, 25, "pca")[0]


def test_membership_and_stats():
    x = np.array([[0, 0, 0], [1, 1, 1], [np.nan, 0, 0], [2, 2, 2], [np.inf, 0, 0], [3, 3, 3]], np.float32)
    labels = np.array([0, 2, 2, -1, 7, 3], np.int32)
    member, st = ref.membership(x, labels, 3)
    assert list(member) == [True, True, False, False, False, False]
    assert st == dict(n_points=6, n_labelled=2, n_ignored=3, n_nonfinite=1, n_labels=3)
    boxes, st = ref.label_boxes(x, labels, 3)
    assert st["n_valid"] == 2 and list(boxes["count"]) == [1, 0, 1] and list(boxes["valid"]) == [1, 0, 1]
    assert not np.frombuffer(boxes[1:2].tobytes(), np.uint8).any()                  # an empty label: zeros throughout
    assert np.array_equal(boxes["center"][2], [1, 1, 1]) and np.array_equal(boxes["extent"][2], [0, 0, 0])


def test_moments_against_fsum(blobs):
    x, labels, boxes = blobs
    worst = 0.0
    for l in range(25):
        pts = x[labels == l].astype(np.float64)
        m = len(pts)
        mean = np.array([math.fsum(pts[:, k]) / m for k in range(3)])               # about the origin, not the pivot
        cov = np.array([math.fsum((pts[:, i] - mean[i]) * (pts[:, j] - mean[j])) / m for i, j in ref.PAIRS])
        _, _, _, _, bmean, bcov = ref.moment_bounds(x[labels == l], ref.pivot(boxes["lo"][l], boxes["hi"][l]))
        assert boxes["count"][l] == m
        assert (np.abs(boxes["mean"][l] - mean) <= bmean + 8 * EPS * np.abs(mean)).all()
        # the two-pass form is exact to a few eps of the variances; the one-pass form about the pivot within its own bound
        assert (np.abs(boxes["cov"][l] - cov) <= bcov + 8 * EPS * np.abs(cov).max()).all()
        worst = max(worst, (np.abs(boxes["cov"][l] - cov) / bcov).max())
    print("cov: worst |restatement - two-pass fsum| / bound = %.3f" % worst)
    assert np.array_equal(boxes["lo"], np.stack([x[labels == l].min(0) for l in range(25)]))
    assert np.array_equal(boxes["hi"], np.stack([x[labels == l].max(0) for l in range(25)]))


def test_the_gpu_axis_fixtures_are_well_separated(blobs):
    """test_gpu_boxes.py compares axes with eigh on these labels: adjacent eigenvalue ratios >= 2"""
    x, labels, boxes = blobs
    for data, lab in ((x, labels), (ref.tilted(x)[0], labels), ((x.astype(np.float64) + 1000.0).astype(np.float32), labels)):
        for l in range(25):
            lam = np.linalg.eigvalsh(np.cov(data[lab == l].astype(np.float64).T, bias=True))[::-1]
            assert lam[0] >= 2 * lam[1] >= 4 * lam[2] > 0, (l, lam)


def test_pca_axes_against_eigh(blobs):
    x, labels, boxes = blobs
    for l in range(25):
        C = ref.cov_matrix(boxes["cov"][l])
        lam, V = np.linalg.eigh(C)
        lam, V = lam[::-1], V[:, ::-1]
        R = boxes["R"][l]
        assert np.abs(boxes["eigenvalues"][l] - lam).max() <= 64 * EPS * lam[0]
        gap = min(lam[0] - lam[1], lam[1] - lam[2])
        for k in range(3):
            assert np.linalg.norm(np.cross(R[:, k], V[:, k])) <= 64 * EPS * lam[0] / gap
        assert np.abs(R.T @ R - np.eye(3)).max() <= 32 * EPS and np.linalg.det(R) > 0
        for k in range(2):                                                           # the sign rule
            assert R[np.argmax(np.abs(R[:, k])), k] > 0
        assert np.array_equal(R[:, 2], ref.cross(R[:, 0], R[:, 1]))


def test_ties_and_signs():
    R, lam, valid = ref.axes_of([2.0, 0, 0, 2.0, 0, 5.0], ref.PCA)                  # xx = yy: index order among the equal ones
    assert valid == 1 and list(lam) == [5.0, 2.0, 2.0]
    assert np.array_equal(R, np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0.0]]))
    assert np.array_equal(ref.signed(np.array([-0.5, 0.5, 0.1])), [0.5, -0.5, -0.1])    # a tie in magnitude: the first component decides
    R, lam, valid = ref.axes_of([np.inf, 0, 0, 1, 0, 1], ref.PCA)
    assert valid == 2 and np.array_equal(R, np.eye(3)) and not lam.any()
    R, lam, valid = ref.axes_of([3.0, 1, 0, 2.0, 0, 1.0], ref.AABB)
    assert np.array_equal(R, np.eye(3)) and list(lam) == [3.0, 2.0, 1.0]


@pytest.mark.parametrize("up", [None, (0, 0, 2.0), (0.1, -0.2, 1.0), (1.0, 0, 0), (1.0, 1.0, 1.0)])
def test_upright_axes(blobs, up):
    x, labels, _ = blobs
    boxes, _ = ref.label_boxes(x, labels, 25, "upright", up)
    u = ref.unit_up(up)
    if up is None or up == (0, 0, 2.0):
        assert np.array_equal(u, [0, 0, 1])
    uu, e1, e2 = ref.upright_frame(up)
    assert abs(e1 @ u) <= 4 * EPS and abs(e2 @ u) <= 4 * EPS and abs(e1 @ e2) <= 4 * EPS and np.linalg.det(np.stack([e1, e2, u], 1)) > 0
    for l in range(25):
        R, C = boxes["R"][l], ref.cov_matrix(boxes["cov"][l])
        assert np.array_equal(R[:, 2], u)
        assert np.abs(R.T @ R - np.eye(3)).max() <= 32 * EPS and np.linalg.det(R) > 0
        assert R[np.argmax(np.abs(R[:, 0])), 0] > 0
        # a0 is the major axis of the covariance projected on the plane across u: numpy.linalg.eigh of the 2 x 2
        P = np.stack([e1, e2], 1)
        lam, V = np.linalg.eigh(P.T @ C @ P)
        major = P @ V[:, 1]
        assert np.linalg.norm(np.cross(R[:, 0], major)) <= 64 * EPS * lam[1] / (lam[1] - lam[0])
        assert np.abs(boxes["eigenvalues"][l] - np.diag(R.T @ C @ R)).max() <= 16 * EPS * np.abs(C).max()
        assert abs((R.T @ C @ R)[0, 1]) <= 16 * EPS * np.abs(C).max()


@pytest.mark.parametrize("mode", ["aabb", "pca", "upright"])
def test_boxes_hold_their_members_brute_force(blobs, mode):
    """corner containment: every member lies inside the convex hull of the 8 corners grown by a few ulps, and each of the six faces
    is touched -- the box is the tightest along its axes"""
    x, labels, _ = blobs
    boxes, _ = ref.label_boxes(x, labels, 25, mode)
    for l in range(25):
        b = boxes[l]
        pts = x[labels == l].astype(np.float64)
        R, c, e = b["R"], b["center"], b["extent"]
        corners = np.array([c + R @ (np.array(s) * e / 2) for s in itertools.product((-1, 1), repeat=3)])
        tol = 16 * EPS * (np.abs(c).max() + e.max())
        for k in range(3):
            lo, hi = (corners @ R[:, k]).min(), (corners @ R[:, k]).max()
            p = pts @ R[:, k]
            assert p.min() >= lo - tol and p.max() <= hi + tol
            assert abs(p.min() - lo) <= tol and abs(p.max() - hi) <= tol
        if mode == "aabb":
            assert np.abs(c - (b["lo"].astype(np.float64) + b["hi"].astype(np.float64)) / 2).max() <= tol
            assert np.abs(e - (b["hi"].astype(np.float64) - b["lo"].astype(np.float64))).max() <= tol


def test_center_rounding_needs_a_margin(blobs):
    """Does sf_cloud_crop_obb(center, R, extent) keep every member at margin 0?  The crop subtracts the ROUNDED center, the rule
    measures from the pivot: the six extreme members sit on the faces, and a face moves by the rounding of center.  Counted here on
    the restatement, so that tests/test_gpu_boxes.py knows what it may ask for: margin 0 loses members even with center rounded once,
    one ulp of the (largest) extent keeps them all on this fixture.  Evaluated left to right in float64 (three roundings) the same
    center loses members at that margin too, which is why the rule asks for one rounding."""
    x, labels, boxes = blobs
    out0 = out1 = plain1 = 0
    need = 0.0
    for l in range(25):
        b, pts = boxes[l], x[labels == l]
        margin = np.spacing(b["extent"].max())
        out0 += int((~ref.inside_any(pts, b["center"], b["R"], b["extent"], 0.0)).sum())
        out1 += int((~ref.inside_any(pts, b["center"], b["R"], b["extent"], margin)).sum())
        d = pts.astype(np.float64) - b["center"]
        p = d[:, 0:1] * b["R"][0] + d[:, 1:2] * b["R"][1]
        p = p + d[:, 2:3] * b["R"][2]
        need = max(need, ((np.abs(p) - b["extent"] / 2).max(0) / margin).max())
        c0 = ref.pivot(b["lo"], b["hi"])
        q = ref.projections(pts, c0, b["R"])
        h = (q.min(0) + q.max(0)) / 2
        plain = c0 + b["R"][:, 0] * h[0]
        plain = plain + b["R"][:, 1] * h[1]
        plain = plain + b["R"][:, 2] * h[2]
        plain1 += int((~ref.inside_any(pts, plain, b["R"], b["extent"], margin)).sum())
    print("members outside their own box: %d at margin 0, %d at one ulp of the extent (worst excess %.2f of that margin); "
          "with center evaluated in plain float64: %d at one ulp" % (out0, out1, need, plain1))
    assert out0 > 0                                              # the rounding of center does need a margin
    assert out1 == 0 and need <= 1.0
    assert plain1 > 0


def test_inside_any_against_brute_force():
    rng = np.random.default_rng(8)
    x = rng.uniform(-7, 7, (4000, 3)).astype(np.float32)
    x[5], x[6] = (np.nan, 0, 0), (0, np.inf, 0)
    center, R, extent = ref.random_boxes(rng, 12)
    want = np.zeros(len(x), bool)
    for c, r, e in zip(center, R, extent):
        with np.errstate(invalid="ignore"):
            local = (x.astype(np.float64) - c) @ r                                   # coordinates along the columns of R
            want |= (np.abs(local) <= e / 2 + 0.05).all(1)
    got = ref.inside_any(x, center, R, extent, 0.05)
    assert np.array_equal(got, want & np.isfinite(x).all(1))                         # (nobody lies within rounding of a face in this draw)
    assert not got[5] and not got[6] and 0 < got.sum() < len(x)
    assert not ref.inside_any(x, center[:0], R[:0], extent[:0]).any()


def test_grid_labels_and_tilt():
    x = np.array([[0.5, 0.5, 0.5], [10, 0, 0], [np.nan, 0, 0], [1, 1, 1], [10.5, 0.2, 0.1]], np.float32)
    labels, n = ref.grid_labels(x)
    assert list(labels) == [0, 1, -1, 0, 1] and n == 2
    y, up = ref.tilted(np.array([[0, 0, 1.0]]), 3.0)
    assert np.allclose(y[0], up) and abs(math.degrees(math.acos(up[2])) - 3.0) < 1e-9
