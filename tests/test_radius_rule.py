"""The numpy restatement of the radius-search rule (tests/radius_ref_np.py, what tests/test_gpu_radius_search.py compares against)
pinned to scipy's cKDTree.query_ball_point in float64 by a sandwich: the rule has < in float32 where the tree has <= in float64, so
ball(r (1 - 1e-5)) is contained in the row and the row in ball(r (1 + 1e-5)) -- 1e-5 is a hundred float32 roundings of the
squared distance -- and the two balls may differ in at most 1 % of the rows, or the sandwich would say little.  The cloud and the
queries are those of the GPU parity test.  No device."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import radius_ref_np as ref
from test_gpu_knn import knn_ref, mixed_map, queries_near

RADII = (0.3, 0.75, 2.0)
TOTALS = {0.3: 1401, 0.75: 7116, 2.0: 67472}


def parity_world():
    rng = np.random.default_rng(27)
    m = mixed_map(rng, 3000)
    q = np.concatenate([queries_near(rng, m, 500), m[::7]]).astype(np.float32)
    return m, q


@pytest.fixture(scope="module")
def world():
    m, q = parity_world()
    assert len(q) == 929
    return m, q, ref.HostIndex(m), cKDTree(m.astype(np.float64))


@pytest.mark.parametrize("radius", RADII)
def test_rows_lie_between_the_two_float64_balls(world, radius):
    m, q, host, tree = world
    off, idx, d2 = ref.radius_ref(host, q, radius)
    inner = tree.query_ball_point(q.astype(np.float64), radius * (1 - 1e-5))
    outer = tree.query_ball_point(q.astype(np.float64), radius * (1 + 1e-5))
    differ = 0
    for i in range(len(q)):
        row = set(idx[off[i]:off[i + 1]].tolist())
        assert len(row) == off[i + 1] - off[i]
        assert set(inner[i]) <= row <= set(outer[i]), (radius, i)
        differ += len(inner[i]) != len(outer[i])
    counts = np.diff(off)
    print("radius %g: total %d, %d empty rows, %d rows above 64, %d of %d rows whose balls differ" % (radius, off[-1], (counts == 0).sum(), (counts > 64).sum(), differ, len(q)))
    assert differ <= len(q) // 100
    assert off[-1] == TOTALS[radius]
    assert radius != 0.3 or (counts == 0).sum() == 191
    assert radius != 2.0 or (counts > 64).sum() == 538
    # index order: ascending position, which for HostIndex is ascending id
    assert all((np.diff(idx[off[i]:off[i + 1]]) > 0).all() for i in range(len(q)))


@pytest.mark.parametrize("radius", RADII)
def test_distance_order_starts_with_the_knn_list(world, radius):
    m, q, host, _ = world
    off, idx, d2 = ref.radius_ref(host, q, radius, "distance")
    off_i, idx_i, d2_i = ref.radius_ref(host, q, radius, "index")
    assert np.array_equal(off, off_i)
    r2 = np.float32(radius * radius)
    ki, kd, kc = knn_ref(host, q, 64, r2)
    ci, cd, cc = ref.rows_cut(off, idx, d2, 64)
    assert np.array_equal(cc, kc) and np.array_equal(cd, kd) and np.array_equal(ci, ki)
    for i in range(len(q)):                                                    # the same entries in both orders, d2 ascending
        a, b = off[i], off[i + 1]
        assert np.array_equal(np.sort(idx[a:b]), idx_i[a:b]) and np.array_equal(d2[a:b], np.sort(d2_i[a:b]))
