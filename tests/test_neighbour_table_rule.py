"""The neighbour-table re-search (sf_map_build_neighbour_table, sf::nn_research_table in sf_nn.hpp) as a rule, in
numpy (tests/nbr_rule_np.py) against brute force.  No reference counterpart: the reference descends a kd-tree for every point
in every iteration (localization/src/icp_point_to_point.cpp:64-69).

A served query's winner -- and its "nothing under thr" verdict -- must be brute force's lexicographic (d2, position) answer,
its runner-up bound must not exceed the true distance of any other point, and the rule must serve at least half of the
random queries (a rule that serves nothing would pass everything else)."""
import numpy as np

import nbr_rule_np as nb

F = np.float32
CELL = 0.25


def table_for(pts):
    sp, org, inv_h, dims, eps = nb.simple_grid(pts, CELL)
    ids, r = nb.build_table(sp, nb.cells_of(sp, org, inv_h, dims), F(CELL), eps)
    return sp, ids, r


def queries_near(rng, sp, m, lo=0.005, hi=0.15):
    seed = rng.integers(0, len(sp), m)
    u = rng.normal(size=(m, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    q = (sp[seed].astype(np.float64) + u * rng.uniform(lo, hi, (m, 1))).astype(F)
    return q, seed


def check(sp, ids, r, q, seed, thr):
    served, win, d2b, lb = nb.research(sp, ids, r, q, seed, thr)
    bwin, bd2 = nb.brute_force(sp, q, thr)
    s = np.nonzero(served)[0]
    assert np.array_equal(win[s], bwin[s])
    assert np.array_equal(d2b[s], bd2[s])
    # the bound: every point but the winner is at least lb away -- EVERY point when the verdict is "nothing under thr" (such a
    # cache entry later certifies "still nothing" from the bound alone)
    others = nb.min_other_distance(sp, q[s], bwin[s])
    assert (lb[s].astype(np.float64) <= others).all()
    return served


def test_random_points():
    rng = np.random.default_rng(5)
    sp, ids, r = table_for(rng.uniform(0.0, 2.0, (3000, 3)))
    q, seed = queries_near(rng, sp, 20_000)
    served = check(sp, ids, r, q, seed, 0.25)
    print("served %.3f of the random queries" % served.mean())
    assert served.mean() >= 0.5


def test_lattice_with_exact_ties():
    rng = np.random.default_rng(6)
    g = np.arange(0, 14, dtype=np.float64) * 0.1                          # 14^3 sites: interior points list 6 + 1 of the 12 diagonals
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F)
    sp, ids, r = table_for(pts)
    q, seed = queries_near(rng, sp, 4_000, 0.0005, 0.08)
    # midpoints of lattice neighbours and of face diagonals: equal distances to two or four points
    s2 = rng.integers(0, len(sp), 3_000)
    step = np.array([[0.1, 0, 0], [0, 0.1, 0], [0.1, 0.1, 0], [0, 0.1, 0.1]])[rng.integers(0, 4, 3_000)]
    mid = ((sp[s2].astype(np.float64) + (sp[s2].astype(np.float64) + step).astype(F).astype(np.float64)) / 2).astype(F)
    served = check(sp, ids, r, np.concatenate([q, mid, sp[s2]]), np.concatenate([seed, s2, s2]), 0.25)
    ties = served[len(q):len(q) + len(mid)]
    print("served %.3f, of the midpoints %.3f" % (served.mean(), ties.mean()))
    assert served[:len(q)].mean() > 0.3 and ties.any()


def test_coincident_points_serve_nothing():
    rng = np.random.default_rng(7)
    pts = np.concatenate([np.repeat(np.array([[1.0, 1.0, 1.0]], F), 9, axis=0), rng.uniform(0.0, 2.0, (200, 3)).astype(F)])
    sp, ids, r = table_for(pts)
    twins = np.nonzero((sp == F(1.0)).all(1))[0]
    assert len(twins) == 9 and (r[twins] == 0).all()
    seed = twins[rng.integers(0, 9, 500)]
    q = (sp[seed] + rng.normal(0, 0.01, (500, 3))).astype(F)
    q[:20] = sp[seed[:20]]
    served = check(sp, ids, r, q, seed, 0.25)
    assert not served.any()


def test_threshold_below_the_best_distance():
    rng = np.random.default_rng(8)
    sp, ids, r = table_for(rng.uniform(0.0, 2.0, (3000, 3)))
    q, seed = queries_near(rng, sp, 5_000, 0.02, 0.08)
    low = float(nb.brute_force(sp, q, np.inf)[1].min()) * 0.5              # below every query's best distance
    served, win, d2b, lb = nb.research(sp, ids, r, q, seed, low)
    assert served.mean() > 0.3 and (win[served] == -1).all()
    check(sp, ids, r, q, seed, low)
    thr = float(np.median(d2b))                                             # ... and one that splits the queries
    served = check(sp, ids, r, q, seed, thr)
    win = nb.research(sp, ids, r, q, seed, thr)[1][served]
    assert (win == -1).any() and (win >= 0).any()


def test_acceptance_radius_far_below_the_point_spacing():
    """thr = (3 cm)^2 against points ~8 cm apart: most served queries have no neighbour under thr.  Their bound must hold for
    EVERY point, the nearest one included -- it is all a later "still nothing" certificate rests on."""
    rng = np.random.default_rng(9)
    sp, ids, r = table_for(rng.uniform(0.0, 2.0, (3000, 3)))
    q, seed = queries_near(rng, sp, 10_000)
    thr = 0.03 ** 2
    served = check(sp, ids, r, q, seed, thr)
    _, win, d2b, lb = nb.research(sp, ids, r, q, seed, thr)
    none = served & (win == -1)
    assert none.sum() > 2000 and (served & (win >= 0)).sum() > 200
    nearest = nb.min_other_distance(sp, q[none], np.full(none.sum(), -1))
    assert (lb[none].astype(np.float64) <= nearest).all()
