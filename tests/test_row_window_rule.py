"""The window rule of the wave search's first trip (sf_nn.hpp: first_window) as tools/probes/ring1_window_proxy.py restates it
in numpy: for random row bounds and gaps the window is contiguous, holds at most four positions (eight for the whole-row
variant), lies inside the own row, takes the own cell first, and together with the three residual ranges (tasks 0, 1 and 10)
tiles the row exactly."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def proxy():
    spec = importlib.util.spec_from_file_location("ring1_window_proxy", os.path.join(ROOT, "tools", "probes", "ring1_window_proxy.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def random_rows(seed, n=20_000):
    rng = np.random.default_rng(seed)
    s0 = rng.integers(0, 1000, n)
    left, own, right = (rng.choice([0, 1, 2, 3, 4, 5, 6, 9], n) for _ in range(3))
    s1, s2, s3 = s0 + left, s0 + left + own, s0 + left + own + right
    gxm = rng.uniform(0.0, 0.25, n).astype(np.float32)
    gxp = np.float32(0.25) - gxm
    gxm2, gxp2 = gxm * gxm, gxp * gxp
    gxm2[rng.random(n) < 0.1] = np.float32(3.0e38)                    # no left neighbour in the grid: what lies there is another row's
    gxp2[rng.random(n) < 0.1] = np.float32(3.0e38)
    eq = rng.random(n) < 0.05
    gxp2[eq] = gxm2[eq]                                               # equal gaps: the right side
    return s0, s1, s2, s3, gxm2, gxp2


@pytest.mark.parametrize("variant", ["own_cell", "nearer_first", "right_then_left", "whole_row"])
def test_window_and_residuals_tile_the_own_row(proxy, variant):
    s0, s1, s2, s3, gxm2, gxp2 = random_rows(3)
    cap = 8 if variant == "whole_row" else 4
    lo, hi = proxy.first_window(s0, s1, s2, s3, gxm2, gxp2, variant)
    own = s2 - s1
    assert np.all(lo <= hi) and np.all(hi - lo <= cap) and np.all(s0 <= lo) and np.all(hi <= s3)
    assert np.all(np.minimum(hi, s2) - np.maximum(lo, s1) == np.minimum(own, cap))     # the own cell first
    assert np.all((lo == s1) | (own < cap)) and np.all((hi <= s2) | (own < cap))        # neighbours only in slots the own cell leaves idle
    (la, lb), (ra, rb), (oa, ob) = proxy.residuals(s0, s1, s2, s3, lo, hi)
    # the pieces in CSR order: left rest, window, rest of the own cell, right rest -- each starts where the last one ended
    assert np.all(la == s0) and np.all(np.maximum(lb, la) == lo)
    assert np.all(np.where(oa < ob, oa, hi) == hi) and np.all(np.where(oa < ob, ob, ra) == ra)
    assert np.all(np.maximum(ra, hi) == ra) and np.all(rb == s3)
    covered = np.maximum(lb - la, 0) + (hi - lo) + np.maximum(ob - oa, 0) + np.maximum(rb - ra, 0)
    assert np.all(covered == s3 - s0)
    # a side without a neighbour gets no slot
    assert np.all(lo[gxm2 > 1e38] == s1[gxm2 > 1e38]) and np.all(hi[gxp2 > 1e38] <= s2[gxp2 > 1e38])
    if variant == "own_cell":
        assert np.all(lo == s1) and np.all(hi == s1 + np.minimum(own, 4))
        return
    # no slot stays idle while a neighbour that exists still has a position left
    nl = np.where(gxm2 < 1e38, s1 - s0, 0)
    nr = np.where(gxp2 < 1e38, s3 - s2, 0)
    assert np.all(hi - lo == np.minimum(cap, np.minimum(own, cap) + nl + nr))
    # the preferred side is served first: the other side holds a position only when the preferred one is taken whole
    right_first = np.ones(len(lo), bool) if variant == "right_then_left" else gxp2 <= gxm2
    took_l, took_r = s1 - lo, np.maximum(hi - s2, 0)
    assert np.all(~(right_first & (took_l > 0)) | (took_r == nr))
    assert np.all(~(~right_first & (took_r > 0)) | (took_l == nl))


def test_a_side_that_can_never_be_queued_gets_no_slot(proxy):
    s0, s1, s2, s3, gxm2, gxp2 = random_rows(4)
    start = np.float32(0.01)                                          # a seed 0.1 m away: gaps of 0.1 m and more are cut
    r0, r1, r2, r3 = proxy.slot_row(s0, s1, s2, s3, gxm2, gxp2, start)
    assert np.all(r1 == s1) and np.all(r2 == s2)
    cut_l, cut_r = ~(gxm2 * np.float32(0.998) < start), ~(gxp2 * np.float32(0.998) < start)
    assert cut_l.any() and cut_r.any() and (~cut_l).any() and (~cut_r).any()
    assert np.all(r0 == np.where(cut_l, s1, s0)) and np.all(r3 == np.where(cut_r, s2, s3))
    lo, hi = proxy.first_window(r0, r1, r2, r3, gxm2, gxp2)
    assert np.all(lo[cut_l] == s1[cut_l]) and np.all(hi[cut_r] <= s2[cut_r])
    # the residual of a side that was cut off is never a task: its gap cannot pass a bound that only falls; what is a task
    # (the gap passes) tiles the row with the window as before
    (la, lb), (ra, rb), _ = proxy.residuals(s0, s1, s2, s3, lo, hi)
    assert np.all((lb - la)[~cut_l] == (lo - s0)[~cut_l]) and np.all((rb - ra)[~cut_r] == (s3 - np.maximum(hi, s2))[~cut_r])


def test_scalars_and_the_benchmark_table(proxy):
    """One hand-checked row: 2 left, 1 own, 5 right, the query nearer its right face."""
    lo, hi = proxy.first_window(10, 12, 13, 18, np.float32(0.04), np.float32(0.01))
    assert (int(lo), int(hi)) == (12, 16)
    lo, hi = proxy.first_window(10, 12, 13, 18, np.float32(0.01), np.float32(0.04))
    assert (int(lo), int(hi)) == (10, 14)
    lo, hi = proxy.first_window(10, 12, 13, 18, np.float32(0.01), np.float32(3.0e38))
    assert (int(lo), int(hi)) == (10, 13)
    world = proxy.make_map(np.random.default_rng(1), lx=8.0, ly=8.0, lz=4.0)
    today = proxy.run(np.random.default_rng(2), world, (0.10, -0.05, 0.02), 6_000, "own_cell")
    new = proxy.run(np.random.default_rng(2), world, (0.10, -0.05, 0.02), 6_000, "nearer_first")
    assert today["first"] < 2.1 and new["first"] > 3.4                  # 1.9 live slots of four today
    assert new["tasks"] < 0.75 * today["tasks"] and new["bound"] < today["bound"]
