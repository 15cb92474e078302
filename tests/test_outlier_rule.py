"""The numpy restatement of the outlier rules (tests/outlier_ref_np.py, what the GPU tests compare against) checked against an
independent float64 calculation with scipy's cKDTree on the planted-outlier cloud, and the filters doing their job on it.  No device."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import outlier_ref_np as ref


@pytest.fixture(scope="module")
def cloud():
    return ref.planted_cloud()


@pytest.fixture(scope="module")
def tree(cloud):
    return cKDTree(cloud.astype(np.float64))


def test_the_planted_cloud_is_what_it_says(cloud):
    s, lone = cloud[:ref.N_SURFACE], cloud[ref.N_SURFACE:]
    assert cloud.shape == (ref.N_SURFACE + ref.N_PLANTED, 3) and cloud.dtype == np.float32 and np.abs(cloud).max() <= 3.1
    assert np.abs(s[:2000, 2]).max() < 0.03 and np.abs(s[2000:, 0] - 2.0).max() < 0.03
    assert (np.abs(lone[:, 2]) > 0.5).all() and (np.abs(lone[:, 0] - 2.0) > 0.5).all()


@pytest.mark.parametrize("flavour", ["pcl", "o3d"])
def test_statistical_against_kdtree(cloud, tree, flavour):
    k, ratio = 20, 2.0
    keep, d, st = ref.statistical(cloud, k, ratio, flavour)
    dist = tree.query(cloud.astype(np.float64), k + 1 if flavour == "pcl" else k)[0]
    d64 = dist[:, 1:].sum(1) / k if flavour == "pcl" else dist.sum(1) / k
    rel = np.abs(d - d64).max() / d64.min()
    print("%s: max |d - d64| / min d64 = %.2e" % (flavour, rel))
    assert np.abs(d - d64).max() <= 1e-6 * d64.min()
    mean, std = d64.mean(), d64.std(ddof=1)
    thr = mean + ratio * std
    assert abs(st["mean"] - mean) <= 1e-6 * mean and abs(st["stddev"] - std) <= 1e-6 * std and abs(st["threshold"] - thr) <= 1e-6 * thr
    keep64 = d64 <= thr if flavour == "pcl" else d64 < thr
    margin = np.abs(d64 - thr).min() / thr
    print("%s: threshold %.4f, the nearest d is %.1f %% away" % (flavour, thr, 100 * margin))
    assert margin > 1e-3                                                                     # no point decides on a rounding
    assert np.array_equal(keep, keep64)
    # the filter does its job: the planted points go, every surface point stays
    assert keep[:ref.N_SURFACE].all() and not keep[ref.N_SURFACE:].any()
    assert st["n_points"] == st["n_valid"] == len(cloud) and st["n_kept"] == ref.N_SURFACE


def test_radius_against_kdtree(cloud, tree):
    r, min_nb = 0.3, 3
    keep, cnt, st = ref.radius(cloud, r, min_nb)
    P = cloud.astype(np.float64)
    near = tree.query_pairs(r * 1.001, output_type="ndarray")
    dd = np.linalg.norm(P[near[:, 0]] - P[near[:, 1]], axis=1)
    assert np.abs(dd - r).min() > 1e-6 * r                                                   # no pair decides on a rounding
    cnt64 = tree.query_ball_point(P, r, return_length=True)
    assert np.array_equal(cnt, cnt64)
    assert np.array_equal(keep, cnt64 > min_nb)
    assert keep[:ref.N_SURFACE].all() and not keep[ref.N_SURFACE:].any()
    assert st["n_kept"] == ref.N_SURFACE and st["mean"] == st["stddev"] == st["threshold"] == 0.0


def test_the_tree_sum_is_the_padded_pairwise_tree():
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 255, 256, 257, 1000, 65537):
        v = rng.uniform(0, 1, n)
        # the same tree built the way the device builds it: blocks of 256 leaves, then the same again over the block sums
        w = v
        while len(w) > 1:
            pad = np.concatenate([w, np.zeros(-len(w) % 256)]).reshape(-1, 256)
            while pad.shape[1] > 1:
                pad = pad[:, 0::2] + pad[:, 1::2]
            w = pad[:, 0]
        assert ref.tree_sum(v) == w[0], n
    assert ref.tree_sum([]) == 0.0


def test_few_and_non_finite_points():
    p = np.array([[0, 0, 0], [np.nan, 0, 0], [1, 0, 0], [0, np.inf, 0], [0, 2, 0]], np.float32)
    keep, d, st = ref.statistical(p, 8, 2.0, "pcl")                                          # three indexed points: the two others, / 2
    assert st["n_points"] == 5 and st["n_valid"] == 3 and np.isnan(d[[1, 3]]).all() and not keep[[1, 3]].any()
    assert np.allclose(d[[0, 2, 4]], [(1 + 2) / 2, (1 + np.sqrt(5)) / 2, (2 + np.sqrt(5)) / 2], rtol=1e-7, atol=0)
    keep, d, st = ref.statistical(p[:1], 3, 2.0, "pcl")
    assert d[0] == 0.0 and keep[0] and st["stddev"] == 0.0 and st["threshold"] == 0.0
    keep, d, st = ref.statistical(p[:1], 3, 2.0, "o3d")                                      # 0 < 0 is false
    assert d[0] == 0.0 and not keep[0]
    keep, cnt, st = ref.radius(p, 1.5, 1)                                                    # at least one neighbour besides itself
    assert list(cnt) == [2, 0, 2, 0, 1] and list(keep) == [True, False, True, False, False]
