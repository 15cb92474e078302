"""The numpy restatement of the plane segmentation rule (tests/plane_ref_np.py) against independent code:
known answers of the generator, numpy.cross / numpy.linalg.norm for the hypotheses, a float64 distance count for the score,
numpy.linalg.svd for the refit.  No device call."""
import numpy as np
import pytest

import plane_ref_np as ref

T = 0.1


@pytest.fixture(scope="module")
def cloud():
    x = ref.workhorse()
    x.setflags(write=False)
    return x


def test_mix_and_samples_known_answers():
    assert ref.mix(0) == 0xE220A8397B1DCDAF
    s = ref.samples(1, 2, 20000)
    assert s.dtype == np.int32 and s.tolist() == [[8519, 10590, 235], [8761, 10048, 7045]]
    assert ref.samples((1 << 64) - 1, 3, 7).max() < 7            # the seed wraps around


@pytest.mark.parametrize("axis", [None, (0.0, 0.0, 2.0), (0.3, -0.2, -1.0)])
def test_hypotheses_against_cross_and_norm(cloud, axis):
    planes, idx, n_deg = ref.hypotheses(cloud, 257, 1, axis, 0.0)
    raw, ok = ref.planes_f64(cloud, idx, axis, 0.0)
    assert n_deg == int((~ok).sum()) == int(np.isnan(planes).any(axis=1).sum()) and ok.sum() > 200
    assert np.array_equal(planes[ok], raw[ok].astype(np.float32)) and np.isnan(planes[~ok]).all()        # rounded once
    ax = None if axis is None else np.asarray(axis) / np.linalg.norm(axis)
    p0, p1, p2 = (cloud[idx[ok][:, j]].astype(np.float64) for j in range(3))
    N = np.cross(p1 - p0, p2 - p0)
    N /= np.linalg.norm(N, axis=1)[:, None]
    if ax is not None:
        N *= np.where(N @ ax >= 0, 1.0, -1.0)[:, None]
    else:                                                       # the first non-zero of (z, y, x) is positive (three wall points: z = 0)
        zyx = N[:, ::-1]
        N *= np.sign(zyx[np.arange(len(N)), (zyx != 0).argmax(axis=1)])[:, None]
    d = -(N * p0).sum(axis=1)
    assert np.abs(raw[ok][:, :3] - N).max() <= 1e-15
    assert (np.abs(raw[ok][:, 3] - d) / np.maximum(1.0, np.abs(d))).max() <= 1e-15
    assert (planes[ok][:, 2] >= 0).all() and (planes[ok][:, 2] == 0).any() if ax is None else (planes[ok][:, :3].astype(np.float64) @ ax >= 0).all()


def test_counts_against_float64_distances(cloud):
    planes, _, _ = ref.hypotheses(cloud, 64, 1)
    planes = planes[~np.isnan(planes).any(axis=1)]
    fin = cloud[np.isfinite(cloud).all(axis=1)]
    dist = np.abs(fin.astype(np.float64) @ planes[:, :3].astype(np.float64).T + planes[:, 3].astype(np.float64))     # [n, H]
    t = np.float64(np.float32(T))
    x = fin[(np.abs(dist - t) >= 1e-4).all(axis=1)]            # no point within 1e-4 of a threshold ...
    dist = np.abs(x.astype(np.float64) @ planes[:, :3].astype(np.float64).T + planes[:, 3].astype(np.float64))
    assert len(x) > 15000 and not (np.abs(dist - t) < 1e-4).any()   # ... and none was left
    assert np.array_equal(ref.score(x, planes, T), (dist < t).sum(axis=0))
    # non-finite points match nothing, whatever the plane
    bad = cloud[~np.isfinite(cloud).all(axis=1)]
    assert len(bad) == 20 and not ref.score(bad, np.concatenate([planes, np.zeros((1, 4), np.float32)]), T).any()
    assert ref.score(fin, np.zeros((1, 4), np.float32), T)[0] == len(fin)        # the all-zero plane: every finite point
    assert ref.score(fin, np.full((1, 4), np.nan, np.float32), T)[0] == 0


def test_refit_against_svd(cloud):
    r = ref.segment(cloud, T, 64, True, 1)
    best = r["planes"][r["stats"]["best_index"]]
    sel = ref.inliers(cloud, best, T)
    pts = cloud[sel].astype(np.float64)
    mean = pts.mean(axis=0)
    nrm = np.linalg.svd(pts - mean, full_matrices=False)[2][2]
    nrm = nrm if nrm @ best[:3] >= 0 else -nrm
    want = np.concatenate([nrm, [-(nrm @ mean)]])
    got, refined = ref.refit(cloud, best, T)
    assert refined == 1 and r["stats"]["refined"] == 1 and np.array_equal(got, r["plane"])
    assert np.abs(got.astype(np.float64) - want).max() < 2e-7, (got, want)       # float32 of a float64 result
    # the fitted plane is the ground: z = 0.05 x - 0.03 y + 1.5
    a, b, c = ref.GROUND
    truth = np.array([-a, -b, 1.0, -c]) / np.sqrt(a * a + b * b + 1)
    assert np.abs(got - truth).max() < 2e-3
    assert r["stats"]["n_inliers"] == int(ref.inliers(cloud, got, T).sum()) and np.array_equal(r["inlier"], ref.inliers(cloud, got, T))
    # fewer than 3 inliers: the hypothesis stands
    far = np.array([0, 0, 1, -100], np.float32)
    assert ref.refit(cloud, far, T) == (pytest.approx(far), 0)


def test_tie_rule(cloud):
    assert ref.choose(np.array([3, 7, 7, 1])) == (1, 7, 1)
    assert ref.choose(np.array([0, 0])) == (0, 0, 0)
    r = ref.segment(cloud, T, 64, True, 1)                       # on this cloud seed 1, H = 64 has a tie for the best count
    c = r["counts"]
    assert np.flatnonzero(c == c.max()).tolist() == [8, 27] and r["stats"]["best_index"] == 8 and r["stats"]["best_count"] == 10222


def test_degenerate_cases(cloud):
    x = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [np.nan, 0, 0], [0, np.inf, 1]], np.float32)
    idx = np.array([[0, 1, 1], [0, 0, 3], [3, 1, 3],           # a repeated index
                    [0, 1, 2],                                  # collinear
                    [0, 1, 4], [5, 1, 3],                       # a NaN / an inf sample
                    [0, 1, 3], [0, 3, 1]], np.int32)            # fine: +z both ways round
    planes, n_deg = ref.planes_from_samples(x, idx)
    assert n_deg == 6 and np.isnan(planes[:6]).all()
    assert planes[6:].tolist() == [[0, 0, 1, 0], [0, 0, 1, 0]]
    # an axis that refuses: the plane z = 0 against the axis x at 15 degrees; one that takes it, and orients it
    planes, n_deg = ref.planes_from_samples(x, idx[6:], (1, 0, 0), np.cos(np.radians(15)))
    assert n_deg == 2 and np.isnan(planes).all()
    planes, n_deg = ref.planes_from_samples(x, idx[6:], (0, 0, -3), np.cos(np.radians(15)))
    assert n_deg == 0 and planes[:, 2].tolist() == [-1, -1]
    assert ref.hypotheses(cloud, 257, 1, (0, 0, 1), np.cos(np.radians(15)))[2] == 179      # of 257 on the workhorse cloud
    # three collinear points, and clouds too small to sample from: no plane
    for pts in (x[:3], x[:2], x[:1]):
        r = ref.segment(pts, T, 16)
        assert r["stats"]["n_degenerate"] == 16 and r["stats"]["found"] == 0 and not r["plane"].any() and not r["inlier"].any()
    assert ref.segment(np.zeros((0, 3)), T, 16)["stats"]["found"] == 0


def test_min_inliers_not_reached(cloud):
    r = ref.segment(cloud, T, 64, True, 1, min_inliers=10223)
    assert r["stats"]["best_count"] == 10222 and r["stats"]["found"] == 0 and r["stats"]["n_inliers"] == 0
    assert not r["plane"].any() and not r["inlier"].any()
    assert ref.segment(cloud, T, 64, True, 1, min_inliers=10222)["stats"]["found"] == 1
