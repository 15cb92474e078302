"""Stage 0 of the neighbour-table look-up (the nearest gap of sf::nn_research_table in sf_nn.hpp) as a rule, in numpy
(tests/nbr_gap_np.py) against the table rule (tests/nbr_rule_np.py) and brute force.  No reference counterpart: the reference
descends a kd-tree for every point in every iteration (localization/src/icp_point_to_point.cpp:64-69).

Every query the gap settles must be one the table rule serves, with the same index and d2 -- so the served flags of the device
stay nb.research's -- its winner must be brute force's, and its bound must not exceed the true distance of any other point
(of ANY point when the verdict is "nothing under thr")."""
import numpy as np

import nbr_gap_np as ng
import nbr_rule_np as nb

F = np.float32
CELL = 0.25


def table_for(pts):
    sp, org, inv_h, dims, eps = nb.simple_grid(pts, CELL)
    ids, r = nb.build_table(sp, nb.cells_of(sp, org, inv_h, dims), F(CELL), eps)
    g1 = ng.nearest_gap(sp, ids, nb.cap_of(F(CELL), eps))
    return sp, ids, r, g1


def queries_near(rng, sp, m, lo=0.005, hi=0.15):
    seed = rng.integers(0, len(sp), m)
    u = rng.normal(size=(m, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    return (sp[seed].astype(np.float64) + u * rng.uniform(lo, hi, (m, 1))).astype(F), seed


def check(sp, ids, r, g1, q, seed, thr):
    passed, win, d2, lb = ng.stage0(sp, g1, q, seed, thr)
    served, twin, td2, tlb = nb.research(sp, ids, r, q, seed, thr)
    s = np.nonzero(passed)[0]
    assert served[s].all()                                                   # nothing the table rule would not serve
    assert np.array_equal(win[s], twin[s]) and np.array_equal(d2[s].view(np.uint32), td2[s].view(np.uint32))
    bwin, bd2 = nb.brute_force(sp, q[s], thr)
    assert np.array_equal(win[s], bwin) and np.array_equal(d2[s], bd2)
    assert (lb[s].astype(np.float64) <= nb.min_other_distance(sp, q[s], bwin)).all()
    assert (g1 <= r).all()                                                   # the gap is never the wider radius
    return passed


def test_gap_is_the_nearest_other_point():
    rng = np.random.default_rng(21)
    sp, ids, r, g1 = table_for(rng.uniform(0.0, 2.0, (1500, 3)))
    true = nb.min_other_distance(sp, sp, np.arange(len(sp)))
    listed = ids[:, 0] != nb.NONE
    assert listed.any() and (g1[listed].astype(np.float64) <= true[listed]).all() and (g1[listed] >= F(0.999) * true[listed].astype(F)).all()
    assert (g1.astype(np.float64) <= true).all()                             # the cap too is a lower bound


def test_random_points():
    rng = np.random.default_rng(22)
    sp, ids, r, g1 = table_for(rng.uniform(0.0, 2.0, (3000, 3)))
    q, seed = queries_near(rng, sp, 20_000)
    passed = check(sp, ids, r, g1, q, seed, 0.25)
    print("the gap settles %.3f of the random queries" % passed.mean())
    assert passed.mean() > 0.1
    near, nseed = queries_near(rng, sp, 5_000, 0.001, 0.02)                  # a converged alignment's distances
    assert check(sp, ids, r, g1, near, nseed, 0.25).mean() > 0.7


def test_lattice_with_exact_ties():
    rng = np.random.default_rng(23)
    g = np.arange(0, 14, dtype=np.float64) * 0.1
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F)
    sp, ids, r, g1 = table_for(pts)
    q, seed = queries_near(rng, sp, 4_000, 0.0005, 0.08)
    s2 = rng.integers(0, len(sp), 3_000)
    step = np.array([[0.1, 0, 0], [0, 0.1, 0], [0.1, 0.1, 0], [0, 0.1, 0.1]])[rng.integers(0, 4, 3_000)]
    mid = ((sp[s2].astype(np.float64) + (sp[s2].astype(np.float64) + step).astype(F).astype(np.float64)) / 2).astype(F)
    passed = check(sp, ids, r, g1, np.concatenate([q, mid, sp[s2]]), np.concatenate([seed, s2, s2]), 0.25)
    assert passed[:len(q)].any() and passed[len(q) + len(mid):].all()          # the lattice points themselves: dp = 0
    assert not passed[len(q):len(q) + len(mid)].any()                          # midway between two points: 2 dp >= g1 never passes


def test_coincident_points_pass_nothing():
    rng = np.random.default_rng(24)
    pts = np.concatenate([np.repeat(np.array([[1.0, 1.0, 1.0]], F), 9, axis=0), rng.uniform(0.0, 2.0, (200, 3)).astype(F)])
    sp, ids, r, g1 = table_for(pts)
    twins = np.nonzero((sp == F(1.0)).all(1))[0]
    assert len(twins) == 9 and (g1[twins] == 0).all()
    seed = twins[rng.integers(0, 9, 500)]
    q = (sp[seed] + rng.normal(0, 0.01, (500, 3))).astype(F)
    q[:20] = sp[seed[:20]]
    assert not check(sp, ids, r, g1, q, seed, 0.25).any()


def test_thresholds_below_the_seed_distance():
    """the "nothing under thr" form: the bound then covers the cached point too"""
    rng = np.random.default_rng(25)
    sp, ids, r, g1 = table_for(rng.uniform(0.0, 2.0, (3000, 3)))
    q, seed = queries_near(rng, sp, 10_000, 0.005, 0.08)
    for thr in (0.03 ** 2, float(nb.brute_force(sp, q, np.inf)[1].min()) * 0.5):
        passed = check(sp, ids, r, g1, q, seed, thr)
        _, win, d2, lb = ng.stage0(sp, g1, q, seed, thr)
        none = passed & (win == -1)
        assert none.sum() > 500
        assert (lb[none].astype(np.float64) <= nb.min_other_distance(sp, q[none], np.full(none.sum(), -1))).all()
