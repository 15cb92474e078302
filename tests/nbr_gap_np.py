"""Stage 0 of the neighbour-table look-up -- the nearest gap (k_neighbour_table's gap array, the head of sf::nn_research_table)
-- written out in numpy, float32 operation by float32 operation, on top of tests/nbr_rule_np.py.  For
tests/test_nearest_gap_rule.py (against the table rule and brute force) and tests/test_gpu_nearest_gap.py (against the device).
Not a test module."""
import numpy as np

import nbr_rule_np as nb

F = np.float32
BY_GAP, BY_TABLE = 1, 2


def nearest_gap(pts, ids, cap):
    """g1 [n] float32: sqrt(d2 of the first listed) * 0.9999, the cap where nothing is listed"""
    pts = np.asarray(pts, F)
    has = ids[:, 0] != nb.NONE
    first = np.where(has, ids[:, 0], 0).astype(np.int64)
    g = np.sqrt(nb.l2_simple(pts, pts[first]), dtype=F) * F(0.9999)
    return np.where(has, g, F(cap)).astype(F)


def square_below(lb):
    """lb2 as the look-up leaves it: one step below the rounded square, 0 for a zero bound"""
    l2 = (np.asarray(lb, F) * np.asarray(lb, F)).astype(F)
    return np.where(l2 > 0, (l2.view(np.uint32) - np.uint32(1)).view(F), F(0)).astype(F)


def stage0(pts, g1, q, seed, thr):
    """-> passed [m] bool, winner [m] int64 (the seed, -1 when it is not under thr), d2 [m] float32 of the seed, lb [m] float32"""
    pts, q = np.asarray(pts, F), np.asarray(q, F)
    seed = np.asarray(seed, np.int64)
    d2 = nb.l2_simple(q, pts[seed])
    dp = np.sqrt(d2, dtype=F)
    g = g1[seed]
    passed = ((dp + dp) * F(1.0001) + F(2.0e-6)) < g
    lb = np.maximum(g - dp * F(1.0001) - F(1.0e-6), F(0)).astype(F)
    lb = np.where(d2 < F(thr), lb, np.minimum(lb, dp * F(0.9999))).astype(F)
    return passed, np.where(d2 < F(thr), seed, -1), d2, lb


def research_stages(pts, ids, r, g1, q, seed, thr):
    """the whole look-up: stage [m] (0 not served, BY_GAP, BY_TABLE), winner, d2 of the best candidate, lb2"""
    passed, w0, d0, lb0 = stage0(pts, g1, q, seed, thr)
    served, w1, d1, lb1 = nb.research(pts, ids, r, q, seed, thr)
    stage = np.where(passed, BY_GAP, np.where(served, BY_TABLE, 0))
    return stage, np.where(passed, w0, w1), np.where(passed, d0, d1).astype(F), square_below(np.where(passed, lb0, lb1).astype(F))
