"""The NDT line search and the coarse-to-fine schedule as tests/ndt_ls_ref_np.py restates them, on the CPU: the
search switched off is ndt_ref_np.align, and the conditions of the fixtures that tests/test_gpu_ndt_ls.py relies on when it compares
integers (iterations, converged, modified, flags, the chosen k of every iteration) exactly."""
import numpy as np
import pytest

import ndt_ls_ref_np as ls
import ndt_ref_np as nr

MARGIN = 16.0      # every Armijo comparison made is this many (summed) score bounds away from equality


@pytest.mark.parametrize("case", ["room_near", "terrain_far", "room_outside"])
def test_without_trials_it_is_the_plain_alignment(case):
    tgt, start, _ = nr.CASES[case]
    a, b = ls.align(nr.model_of(tgt), nr.source_of(tgt), start, trials=0), nr.reference_alignment(case)
    assert set(a) == set(b)
    for k in ("T64", "score", "gradient", "hessian", "trace"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    for k in ("n_inside", "n_terms", "iterations", "converged", "modified", "flags"):
        assert a[k] == b[k], k


def test_pick_is_the_smallest_k_that_passes():
    phi0, slope, amax = -10.0, -4.0, 0.5
    lim = [phi0 + (1e-4 * float(np.ldexp(amax, -k))) * slope for k in range(4)]
    assert ls.pick(phi0, slope, amax, [lim[0], -99.0, -99.0, -99.0], [5, 5, 5, 5], 1e-4) == 0           # equality passes
    assert ls.pick(phi0, slope, amax, [np.nextafter(lim[0], 0.0), lim[1], -99.0, -99.0], [5, 5, 5, 5], 1e-4) == 1
    assert ls.pick(phi0, slope, amax, [-99.0, -99.0, lim[2], -99.0], [0, 0, 5, 5], 1e-4) == 2            # no terms: not accepted
    assert ls.pick(phi0, slope, amax, [-np.inf, np.nan, np.inf, -10.5], [5, 5, 5, 5], 1e-4) == 3         # not finite: not accepted
    assert ls.pick(phi0, slope, amax, [-9.0, -9.5, -9.9, phi0], [5, 5, 5, 5], 1e-4) == -1                # phi0 itself is above every limit (slope < 0)


def _conditions(r, res):
    """What lets the GPU test compare integers exactly: no transformed point within 1e-9 resolution of a cell face at any pose
    evaluated (the trials included); no Hessian eigenvalue within a factor 2 of the floor; the length of the accepted step at least MARGIN step
    bounds away from transformation_epsilon; every Armijo comparison made at least MARGIN bounds from equality."""
    assert r["face_gap"] >= 1e-9 * res
    for st in r["steps"]:
        assert np.abs(st["eig"]).min() >= 2.0 * st["floor"]
    for k, row in enumerate(r["rows"]):
        assert row["margin"] >= MARGIN, row["margin"]
        if row["chosen"] >= 0:                                 # (ndt_ref_np.step_bound is at least twice the error of the direction)
            length = float(np.ldexp(row["alpha_max"], -row["chosen"])) * row["raw_length"]
            assert abs(length - nr.DEFAULTS["transformation_epsilon"]) >= MARGIN * nr.step_bound(r["evaluations"][k], r["steps"][k], r["trace"][k])


@pytest.mark.parametrize("case,chosen", [("room_near", [0, 1, 1, 2, 1, 3, 0, 0, 0]), ("terrain_near", [2, 1, 2, 0, 0, 0, 0])])
def test_near_fixtures(case, chosen):
    """Measured: the least margin is 8.0e5 bounds on room_near and 1.2e5 on terrain_near (the bound here is the sum of the two scores'
    bounds, about twice a single one)."""
    r = ls.reference_ls(case)
    print("%s: %d iterations, chosen %s, least margin / bound %.3g" % (case, r["iterations"], r["chosen"], min(row["margin"] for row in r["rows"])))
    assert r["chosen"] == chosen and r["iterations"] == len(chosen) and r["converged"] and r["flags"] == 0
    assert any(k > 0 for k in r["chosen"])                     # at least one iteration backtracks
    _conditions(r, nr.ALIGN_RES[nr.CASES[case][0]])
    dt = np.linalg.norm(r["T64"][:3, 3])
    assert dt < 0.05


@pytest.mark.parametrize("case", ["room_far", "terrain_negative"])
def test_the_replay_only_fixtures_converge_too(case):
    """(their margins are 0.8 and 0.2 bounds: only the replay test of tests/test_gpu_ndt_ls.py uses them, which holds whatever the margins)"""
    r = ls.reference_ls(case)
    print("%s: %d iterations, chosen %s, least margin / bound %.3g" % (case, r["iterations"], r["chosen"], min(row["margin"] for row in r["rows"])))
    assert r["converged"] and r["flags"] == 0 and np.linalg.norm(r["T64"][:3, 3]) < 0.05


def test_room_coarse_stall():
    r = ls.reference_stall()
    tgt, res, start = ls.STALL["room_coarse_stall"]
    print("room_coarse_stall: %d iterations, chosen %s, least margin / bound %.3g" % (r["iterations"], r["chosen"], min(row["margin"] for row in r["rows"])))
    assert res == 2.0 and r["flags"] == ls.STALLED and not r["converged"] and r["chosen"][-1] == -1 and all(k >= 0 for k in r["chosen"][:-1])
    assert len(r["rows"]) == r["iterations"] + 1 and len(r["trace"]) == r["iterations"] + 1
    assert r["T64"].tobytes() == r["trace"][-1].tobytes()      # the pose stays where the last accepted step left it
    assert 1 <= r["iterations"] < nr.DEFAULTS["max_iterations"]
    last = r["rows"][-1]
    assert (last["n_terms"] > 0).all() and np.isfinite(last["phi"]).all()                  # it stalls on the scores, not for want of overlap
    _conditions(r, res)
    assert 1.4 < np.linalg.norm(start[:3, 3]) < 1.6              # (the truth is the identity)


@pytest.mark.parametrize("case", ["room_wide", "terrain_wide"])
def test_wide_fixtures(case):
    plain, last, per_level = ls.reference_wide(case)
    tgt = ls.WIDE[case][0]
    e_plain, e_pyr = np.linalg.norm(plain["T64"][:3, 3]), np.linalg.norm(last["T64"][:3, 3])
    print("%s: plain at 1 m ends %.3g m from the truth, levels %s with the search %.3g m; per level (iterations, flags) %s"
          % (case, e_plain, ls.LEVELS[tgt], e_pyr, [(p["iterations"], p["flags"]) for p in per_level]))
    assert ls.LEVELS[tgt][-1] == nr.ALIGN_RES[tgt] == 1.0 and len(per_level) == len(ls.LEVELS[tgt])
    assert e_plain > 0.5 and e_pyr < 0.05
    for a, b in zip(per_level[:-1], per_level[1:]):            # every level starts where the previous one ended, whatever its flags
        assert b["trace"][0].tobytes() == a["T64"].tobytes()
    assert per_level[0]["trace"][0].tobytes() == ls.WIDE[case][1].tobytes()
    assert any(p["flags"] & ls.STALLED for p in per_level[:-1])                            # (a stalled coarse level still hands its pose on)
