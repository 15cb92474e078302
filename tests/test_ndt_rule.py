"""The NDT rule as tests/ndt_ref_np.py restates it, on the CPU: the constants against their closed form, the
gradient and the Hessian against central differences of the restatement's own objective, and the conditions of the fixtures that
tests/test_gpu_ndt.py relies on when it compares integers (iterations, converged, modified, flags) exactly."""
import math

import numpy as np
import pytest

import ndt_ref_np as nr


@pytest.mark.parametrize("r", [1.0, 2.0])
def test_constants_against_their_closed_form(r):
    """d1 exp(-d2 x / 2) + d3 meets -ln(c1 exp(-x / 2) + c2) at x = 0 and x = 1 and tends to it at infinity: that defines d1, d2, d3."""
    p = 0.55
    c1, c2 = 10.0 * (1.0 - p), p / r ** 3
    d1, d2, d3 = nr.constants(r, p)
    mix = lambda x: -math.log(c1 * math.exp(-0.5 * x) + c2)
    assert d3 == pytest.approx(-math.log(c2), rel=1e-15)
    assert d1 == pytest.approx(math.log(c2 / (c1 + c2)), rel=1e-14) and d1 < 0.0 and d2 > 0.0
    assert d1 + d3 == pytest.approx(mix(0.0), rel=1e-14, abs=1e-15)
    assert d1 * math.exp(-0.5 * d2) + d3 == pytest.approx(mix(1.0), rel=1e-13)
    assert d2 == pytest.approx(-2.0 * math.log((mix(1.0) - d3) / d1), rel=1e-14)
    assert d3 == pytest.approx(mix(1e9), rel=1e-15)


def _clear_of_faces(mdl, src, T, margin):
    """the points whose image stays `margin` metres away from every cell face (a difference stencil must not carry one across)"""
    gc = (nr.transform(T, src) - mdl["org"]) * mdl["inv_h"]
    return src[(np.abs(gc - np.round(gc)) * mdl["h"]).min(1) >= margin]


def _differences(f, h):
    e = np.eye(6) * h
    g = np.array([(f(e[i]) - f(-e[i])) / (2.0 * h) for i in range(6)])
    H = np.zeros((6, 6))
    f0 = f(np.zeros(6))
    for i in range(6):
        H[i, i] = (f(e[i]) - 2.0 * f0 + f(-e[i])) / (h * h)
        for j in range(i + 1, 6):
            H[i, j] = H[j, i] = (f(e[i] + e[j]) - f(e[i] - e[j]) - f(-e[i] + e[j]) + f(-e[i] - e[j])) / (4.0 * h * h)
    return g, H


@pytest.mark.parametrize("neighbours", [1, 7])
@pytest.mark.parametrize("target", ["room", "terrain"])
def test_gradient_and_hessian_against_central_differences(target, neighbours):
    """delta -> f(M(delta) T) through vec6_to_mat4's own convention, at three poses per fixture.  The accuracy asked is the one the
    differences have: central differences at h and h / 2 differ by 3/4 of the error of the first, which is 3 times the error of the
    second, so the change between the two bounds the error of the second (largest entry against largest entry)."""
    mdl, h = nr.model_of(target), 2e-4
    for T in nr.EVAL_POSES:
        src = _clear_of_faces(mdl, nr.source_of(target), T, 0.05)   # a stencil moves a point by at most sqrt(2) h (1 + |y|) < 0.005 m
        assert len(src) > 300
        ev = nr.evaluate(mdl, src, T, neighbours)
        assert ev["n_terms"] > 300
        f = lambda d: nr.objective(mdl, src, nr.vec6_to_mat4(d) @ T, neighbours)
        g1, H1 = _differences(f, h)
        g2, H2 = _differences(f, 0.5 * h)
        eg, eh = np.abs(g1 - g2).max(), np.abs(H1 - H2).max()
        print("%s DIRECT%d: gradient off by %.3g (differences change by %.3g, |g| %.3g); Hessian off by %.3g (%.3g, |H| %.3g)"
              % (target, neighbours, np.abs(ev["gradient"] - g2).max(), eg, np.abs(g2).max(), np.abs(ev["hessian"] - H2).max(), eh, np.abs(H2).max()))
        assert np.abs(ev["gradient"] - g2).max() <= eg
        assert np.abs(ev["hessian"] - H2).max() <= eh
        assert eg < 1e-2 * np.abs(g2).max() and eh < 1e-2 * np.abs(H2).max()   # (the differences themselves are sharp: the comparison says something)
        assert np.array_equal(ev["hessian"], ev["hessian"].T)


@pytest.mark.parametrize("case", sorted(nr.CASES))
def test_fixture_conditions(case):
    """What lets the GPU tests compare integers exactly: at every iterate of the restatement no transformed point lies within
    1e-9 resolution of a cell face; no Hessian eigenvalue is within a factor 2 of the floor (hence of a sign change: below the floor
    the sign does not matter); the applied step is never within a factor 2 of transformation_epsilon; the raw step is never within
    a factor 2 of the clamp, except in the fixtures made for the clamp."""
    target, _, made_for_clamp = nr.CASES[case]
    res = nr.ALIGN_RES[target]
    r = nr.reference_alignment(case)
    assert r["face_gap"] >= 1e-9 * res
    eps, step = nr.DEFAULTS["transformation_epsilon"], nr.DEFAULTS["step_size"]
    for st in r["steps"]:
        assert np.abs(st["eig"]).min() >= 2.0 * st["floor"]
        assert st["length"] >= 2.0 * eps or st["length"] <= 0.5 * eps
        if not made_for_clamp:
            assert st["raw_length"] >= 2.0 * step or st["raw_length"] <= 0.5 * step
    if case == "terrain_negative":
        assert (r["steps"][0]["eig"] < 0.0).any() and r["modified"] >= 1
    if case == "room_outside":
        assert r["flags"] == nr.NO_OVERLAP and r["iterations"] == 0 and np.array_equal(r["T64"], nr.CASES[case][1])
    else:
        assert r["converged"] and r["flags"] == 0
    if made_for_clamp:
        assert sum(st["raw_length"] > step for st in r["steps"]) >= 5


def test_the_salted_room():
    """32 cells; the salted cells are voxels or not as the rule says, with one and with two floored eigenvalues"""
    Q, ids = nr.salted_room()
    assert len(Q) <= 20_000
    v = nr.voxels(Q, nr.ROOM_RES)
    assert tuple(v["grid"]["dims"]) == (4, 4, 2) and v["n_occupied"] == 32 and len(v["cell"]) == 30
    assert ids["below"] not in v["cell"] and ids["coincident"] not in v["cell"] and ids["exact"] in v["cell"]
    for name, floored in (("planar", 1), ("collinear", 2)):
        k = int(np.flatnonzero(v["cell"] == ids[name])[0])
        lam = np.linalg.eigvalsh(nr.sym3(v["cov"][k]))
        assert np.sum(np.isclose(lam, 0.01 * lam.max(), rtol=1e-9)) == floored
    assert np.array_equal(v["cell"], np.sort(v["cell"]))
