"""The restatement of the neighbour-reuse certificate (tests/reuse_ref_np.py) pinned on seeded clouds, without a device.

The property the launch list's speed rests on: a cache entry (neighbour j, E = D + M_then) whose D really bounds the distance of
every other point at write time, read under a motion bound M_now that really bounds how far the query has moved, certifies only
while j is still what a full search returns.  Here D is the ideal bound D* -- the float64 distance to the nearest other accepted
point at write time, rounded down to float32 -- and M the largest float64 displacement of any query: every certified entry must
carry the brute-force nearest.  The same clouds with D* inflated by 5 % must show violations: the property can fail, and the
check that tests/test_gpu_reuse_bound.py runs on the production kernels' entries would see it."""
import numpy as np
import pytest

import reuse_ref_np as R

F = np.float32
THR = F(0.3 * 0.3)


rigid = R.rigid


def step_bound(Ta, Tb, x0):
    """an honest motion step: no query moves farther between the two poses (float64, rounded up)"""
    x = np.c_[x0.astype(np.float64), np.ones(len(x0))]
    d = np.linalg.norm((x @ Tb.T - x @ Ta.T)[:, :3], axis=1)
    return float(d.max()) * (1.0 + 1.0e-9)


def world(seed, offset=0.0):
    rng = np.random.default_rng(seed)
    clumps = rng.uniform(0, 6, (60, 3))[rng.integers(0, 60, 2500)] + rng.normal(0, 0.05, (2500, 3))
    pts = np.concatenate([clumps, rng.uniform(0, 6, (1500, 3))])
    pts = np.concatenate([pts, pts[rng.integers(0, len(pts), 200)]])               # exact twins: D* = 0, never certified
    P = (pts + offset).astype(np.float32)
    # queries: near points, between a point and a close other point a little off the bisector, and far from everything
    near = P[rng.integers(0, len(P), 500)] + rng.normal(0, 0.01, (500, 3)).astype(np.float32)
    a = P[rng.integers(0, 2500, 900)]
    b = a + rng.normal(0, 0.05, a.shape).astype(np.float32)
    P = np.concatenate([P, b]).astype(np.float32)
    mid = (a.astype(np.float64) + b) / 2 + (a.astype(np.float64) - b) * rng.uniform(0.0, 0.02, (len(a), 1))
    far = rng.uniform(0, 6, (100, 3)) + [0, 0, 7.0] + offset
    want = np.concatenate([near, mid, far])
    T0 = rigid([0.02, -0.01, 0.03], [0.01, 0.02, -0.015], offset + 3.0)
    x0 = (np.c_[want, np.ones(len(want))] @ np.linalg.inv(T0).T)[:, :3].astype(np.float32)
    x0[::97] = np.nan                                                              # non-finite scan points never certify
    return P, x0, T0


def entries_and_check(P, ok_pt, x0, poses, inflate):
    """Entries written at poses[1] (after one update from poses[0]) with the ideal bound times `inflate`, read at poses[2].
    -> (certified, violations, finite queries)"""
    M1 = step_bound(poses[0], poses[1], x0[np.isfinite(x0).all(1)])
    M2 = M1 + step_bound(poses[1], poses[2], x0[np.isfinite(x0).all(1)])
    q1 = R.query32(poses[1], x0)
    none = np.full(len(q1), -1)
    j, c1, E = R.ideal_entries(q1, P, ok_pt, THR, M1, inflate)
    q2 = R.query32(poses[2], x0)
    cert = R.certifies(E, j.astype(np.int32), q2, c1, THR, M2)
    # the search's answer now, whatever the acceptance radius (a cached neighbour that has drifted beyond it is still the nearest)
    pos2, d2_2, _ = R.brute(q2, P, ok_pt, np.inf, none)
    with_j = cert & (j >= 0)
    bad = with_j & ((pos2 != j) | (R.l2_simple(q2, c1).view(np.uint32) != d2_2.view(np.uint32)))
    bad |= cert & (j < 0) & (d2_2 < THR)                                            # "still nothing within the acceptance radius"
    return int(cert.sum()), int(bad.sum()), int(np.isfinite(q2).all(1).sum())


@pytest.mark.parametrize("offset", [0.0, 1000.0])
@pytest.mark.parametrize("window", ["none", "sphere", "obb"])
def test_the_ideal_bound_certifies_only_the_nearest_and_an_inflated_one_does_not(window, offset):
    certified = violations = 0
    for seed in (1, 2, 3):
        P, x0, T0 = world(seed, offset)
        if window == "sphere":
            ok_pt = R.sphere_accept(P, np.array([3.0, 3.0, 3.0]) + offset, 2.8)
        elif window == "obb":
            ok_pt = R.obb_accept(P, np.array([3.0, 3.0, 3.0]) + offset, [[0.9, -0.3, 0.05], [0.35, 0.95, 0.0], [0.0, 0.1, 1.1]], [4.0, 5.0, 4.4])
        else:
            ok_pt = np.ones(len(P), bool)
        assert 500 < ok_pt.sum()
        poses = [T0, rigid([0.004, 0.002, -0.003], [0.001, -0.0005, 0.0008], offset + 3.0) @ T0, None]
        poses[2] = rigid([-0.0008, 0.0005, 0.0005], [0.0001, 0.0001, -0.0001], offset + 3.0) @ poses[1]
        n_cert, n_bad, n_fin = entries_and_check(P, ok_pt, x0, poses, 1.0)
        assert n_bad == 0, (seed, n_bad)
        assert n_cert > 0.5 * n_fin, (seed, n_cert, n_fin)                          # the check is not run on nobody
        n_cert5, n_bad5, _ = entries_and_check(P, ok_pt, x0, poses, 1.05)
        assert n_cert5 >= n_cert
        certified += n_cert
        violations += n_bad5
    print("window %s offset %g: %d certified under the ideal bound, %d violations under the bound inflated by 5 %%" % (window, offset, certified, violations))
    assert violations > 0


def test_reach_and_entry_are_float32_and_an_empty_entry_never_certifies():
    q = np.array([[1.0, -2.0, 3.0], [np.nan, 0.0, 0.0], [1.0e3, 1.0e3, 1.0e3]], np.float32)
    e = np.array([0.5, 0.5, 0.5], np.float32)
    r = R.reach32(e, 0.125, q)
    assert r.dtype == np.float32
    # by hand, operation by operation
    want = F(F(F(F(0.5) - F(F(0.125) * F(1.000002))) - F(F(7.0) * F(1.3e-7))) - F(F(0.625) * F(5.0e-7))) - F(1.0e-6)
    assert r[0] == want
    assert r[2] < r[0]                                                             # the |q| term carries weight 1 km out
    c1 = np.zeros((3, 3), np.float32)
    j = np.array([4, 4, -1], np.int32)
    assert not R.certifies(np.zeros(3, np.float32), j, q, c1, THR, 0.0).any()      # E = 0: no search behind the entry
    assert not R.certifies(e, j, q, c1, THR, 0.0)[1]                               # a non-finite query
    assert R.entry32(np.array([0.0], np.float32), 0.0)[0] == F(1.0e-30)
    assert R.entry32(np.array([1.0], np.float32), 0.0)[0] == F(F(F(1.0) * F(0.9999)) + F(0.0)) - F(1.0e-6)
    assert np.array_equal(R.query32(np.eye(4), q)[[0, 2]], q[[0, 2]])
