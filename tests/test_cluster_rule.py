"""The numpy restatement of the clustering rule (tests/cluster_ref_np.py, what tests/test_gpu_cluster.py compares against) pinned to
scikit-learn's DBSCAN -- labels, core set and border points alike -- and to scipy's connected components of the float64 graph, on
the clouds and parameters of the GPU parity test.  The rule has < in float32 where the libraries have <= in float64: every case first
asserts that no pair lies within eps (1 +- 1e-5) of the threshold, so a mismatch cannot be put down to that.  No device."""
import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree
from sklearn.cluster import DBSCAN

import cluster_ref_np as ref
from test_gpu_knn_normals import noisy_map  # noqa: F401  (the fixture: [1] is 3 000 mixed points plus 20 isolated ones; no device)

DBSCAN_PARAMS = ((0.12, 5), (0.2, 3), (0.2, 10), (0.3, 1))


@pytest.fixture(scope="module")
def clouds(noisy_map):  # noqa: F811
    return {"mixed": noisy_map[1], "blobs": ref.blob_cloud()}


@pytest.mark.parametrize("name", ["mixed", "blobs"])
@pytest.mark.parametrize("eps,min_points", DBSCAN_PARAMS)
def test_dbscan_equals_scikit_learn(clouds, name, eps, min_points):
    x = clouds[name]
    assert ref.near_eps_pairs(x, eps) == 0
    labels, sizes, st, core = ref.dbscan(x, eps, min_points)
    sk = DBSCAN(eps=eps, min_samples=min_points, algorithm="kd_tree").fit(x.astype(np.float64))
    print("%s eps %g min_points %d: %d clusters, %d core, %d border, %d noise" % (name, eps, min_points, st["n_clusters"], st["n_core"], st["n_border"], st["n_noise"]))
    assert np.array_equal(np.flatnonzero(core), sk.core_sample_indices_)
    assert np.array_equal(labels, sk.labels_)
    assert np.array_equal(sizes, np.bincount(sk.labels_[sk.labels_ >= 0], minlength=st["n_clusters"]))
    assert st["n_core"] + st["n_border"] == st["n_kept"] == int((labels >= 0).sum()) and st["n_kept"] + st["n_noise"] == st["n_valid"] == len(x)
    assert min_points > 1 or (st["n_border"] == 0 and st["n_noise"] == 0)


@pytest.mark.parametrize("name", ["mixed", "blobs"])
def test_euclidean_equals_the_float64_components(clouds, name):
    x, tol = clouds[name], 0.2
    assert ref.near_eps_pairs(x, tol) == 0
    P = x.astype(np.float64)
    pr = cKDTree(P).query_pairs(tol, output_type="ndarray")
    n = len(x)
    nc, comp = connected_components(coo_matrix((np.ones(len(pr), np.int8), (pr[:, 0], pr[:, 1])), shape=(n, n)), directed=False)
    labels, sizes, st = ref.euclidean(x, tol)
    assert st["n_clusters"] == nc and st["n_kept"] == n and st["n_noise"] == 0 and st["largest_size"] == np.bincount(comp).max()
    # the same partition, numbered by smallest member
    first = np.full(nc, n)
    np.minimum.at(first, comp, np.arange(n))
    rank = np.empty(nc, np.int64)
    rank[np.argsort(first)] = np.arange(nc)
    assert np.array_equal(labels, rank[comp])
    assert np.array_equal(sizes, np.bincount(rank[comp]))
    for min_size, max_size in ((5, 0), (5, 200)):
        fl, fs, fst = ref.euclidean(x, tol, min_size, max_size)
        ok = (sizes >= min_size) & ((sizes <= max_size) if max_size > 0 else True)
        assert ok.sum() < nc                                                 # (blobs, (5, 200): nothing passes -- every blob is larger, the rest smaller)
        assert np.array_equal(fl >= 0, ok[labels]) and np.array_equal(fs, sizes[ok]) and fst["n_clusters"] == ok.sum()
        assert np.array_equal(fl[fl >= 0], (np.cumsum(ok) - 1)[labels[fl >= 0]])
        assert fst["n_noise"] == n - sizes[ok].sum() and fst["n_kept"] == sizes[ok].sum() and fst["largest_size"] == (sizes[ok].max() if ok.any() else 0)


def test_contested_border_point_and_non_finite_points():
    eps = 0.5
    for a_first in (True, False):
        x = ref.contested_cloud(eps, a_first)
        d = np.linalg.norm(x[:24, None].astype(np.float64) - x[None, :24].astype(np.float64), axis=2)
        assert d[:12, :12].max() < 0.5 * eps and d[12:, 12:].max() < 0.5 * eps and d[:12, 12:].min() > 1.05 * eps
        dm = np.linalg.norm(x[:24].astype(np.float64) - x[24].astype(np.float64), axis=1)
        assert (dm[:12] < 0.75 * eps).sum() == 3 and (dm[12:] < 0.75 * eps).sum() == 3 and (dm > 1.02 * eps).sum() == 18
        labels, sizes, st, core = ref.dbscan(x, eps, 8)
        assert list(labels) == [0] * 12 + [1] * 12 + [0] and core[:24].all() and not core[24] and list(sizes) == [13, 12]
        assert st == dict(n_points=25, n_valid=25, n_core=24, n_border=1, n_noise=0, n_clusters=2, largest_size=13, n_kept=25)
        sk = DBSCAN(eps=eps, min_samples=8).fit(x.astype(np.float64))
        assert np.array_equal(sk.labels_, labels) and np.array_equal(sk.core_sample_indices_, np.arange(24))
        # points that are not indexed: -1, counted nowhere but in n_points
        y = np.concatenate([x[:5], [[np.nan, 0, 0]], x[5:], [[0, np.inf, 0]]]).astype(np.float32)
        labels, sizes, st, core = ref.dbscan(y, eps, 8)
        fin = np.isfinite(y).all(1)
        assert np.array_equal(labels[fin], sk.labels_) and (labels[~fin] == -1).all() and not core[~fin].any()
        assert st == dict(n_points=27, n_valid=25, n_core=24, n_border=1, n_noise=0, n_clusters=2, largest_size=13, n_kept=25)


def test_cloud_masks():
    x = ref.blob_cloud(4000, 6, 0.1, seed=9)
    labels, sizes, st = ref.euclidean(x, 0.2)
    mask, fst = ref.filter_clusters(x, 0.2, 50)
    assert np.array_equal(mask, (sizes >= 50)[labels]) and fst["n_kept"] == mask.sum() and 0 < mask.sum() < len(x)
    mask, lst = ref.keep_largest_cluster(x, 0.2)
    assert mask.sum() == sizes.max() == lst["n_kept"] == lst["largest_size"] and lst["n_clusters"] == st["n_clusters"]
    assert lst["n_noise"] == len(x) - sizes.max() and len(set(labels[mask])) == 1
    two = np.array([[0, 0, 0], [5, 0, 0], [5.1, 0, 0], [0.1, 0, 0]], np.float32)          # a tie: the cluster of point 0 stays
    mask, lst = ref.keep_largest_cluster(two, 0.2)
    assert list(mask) == [True, False, False, True] and lst["n_kept"] == 2
    assert ref.keep_largest_cluster(np.zeros((0, 3), np.float32), 0.2)[1] == dict.fromkeys(ref.STAT_KEYS, 0)
