"""The numpy restatement of the radius normals (tests/normals_ref_np.py) held against two other statements of the same rule -- the
oracle's normals_radius_cov and a scipy cKDTree ball query -- and the precondition of every fixture the GPU test relies on."""
import numpy as np
import pytest

import normals_ref_np as nr

F = np.float32
NAMES = sorted(nr.cases())


def finite(case):
    P = case["points"]
    keep = np.isfinite(P).all(1)
    return P[keep], keep


@pytest.mark.parametrize("name", NAMES)
def test_no_pair_sits_on_a_rounding_of_the_predicate(name):
    assert nr.reference(name)["ambiguous"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_against_the_oracle(orc, name):
    case, ref = nr.cases()[name], nr.reference(name)
    P, keep = finite(case)
    if len(P) == 0:                                                              # (the oracle takes no empty cloud)
        assert len(ref["count"]) == 0
        return
    nrm, cnt, cov = orc.normals_radius_cov(P, case["radius"])
    assert np.array_equal(cnt, ref["count"][keep]), np.flatnonzero(cnt != ref["count"][keep])[:5]
    ok = cnt >= 3
    tol = ref["tol"]
    assert not cov[~ok].any() and (nrm[~ok] == nr.Z_UP).all()
    if ok.any():
        assert (np.abs(cov - ref["cov6"][keep]).max(1) <= tol["cov"][keep])[ok].all()
        sep = tol["separated"][keep] & ok
        sin = np.linalg.norm(np.cross(nrm.astype(np.float64), ref["normal64"][keep]), axis=1)
        assert (sin <= tol["sin"][keep] + 2.0 ** -24)[sep].all()                 # (the oracle's vector is a float32 too, not normalised again)


@pytest.mark.parametrize("name", NAMES)
def test_against_a_kdtree_ball_query(name):
    from scipy.spatial import cKDTree
    case, ref = nr.cases()[name], nr.reference(name)
    P, keep = finite(case)
    if len(P) == 0:
        assert len(ref["count"]) == 0
        return
    tree = cKDTree(P.astype(np.float64))
    cnt = tree.query_ball_point(P.astype(np.float64), r=case["radius"], return_length=True)
    assert np.array_equal(cnt, ref["count"][keep])
    assert not ref["count"][~keep].any()


def test_long_double_sums_agree_with_fsum():
    for name in ("scene_2.5", "far_3km", "size_257"):
        case, ref = nr.cases()[name], nr.reference(name)
        rows = np.flatnonzero(ref["count"] >= 3)[::97]
        got = nr.estimate_fsum(case["points"], case["radius"], rows)
        for i in rows:
            # fsum works on the float64 roundings of the centred differences and products: two of the bound's first-order terms
            assert np.abs(got[i] - ref["cov6"][i]).max() <= ref["tol"]["cov"][i]


# ------------------------------------------------------------------ preconditions
@pytest.mark.parametrize("cell,ratio", nr.STRADDLE)
def test_straddle_pairs_lie_one_cell_beyond_the_old_reach(cell, ratio):
    case = nr.cases()["straddle_%g_%d" % (cell, ratio)]
    ref = nr.reference("straddle_%g_%d" % (cell, ratio))
    P, radius, h = case["points"], F(case["radius"]), F(case["cell"])
    assert radius == F(F(ratio) * F(cell))
    R_old = max(1, int(np.ceil(float(radius) / float(h) - 1e-9)))
    assert R_old == ratio
    org = P.min(0)
    assert np.array_equal(P[case["anchor"]], org)
    others = np.delete(P, case["anchor"], 0).astype(np.float64)
    assert np.linalg.norm(others - org.astype(np.float64), axis=1).min() > float(radius)
    inv_h = F(1.0 / float(h))
    assert sorted(a for _, _, a in case["pairs"]) == [0, 1, 2]
    for iq, ip, axis in case["pairs"]:
        q, p = P[iq], P[ip]
        off = [a for a in range(3) if a != axis]
        assert np.array_equal(q[off], p[off])
        assert float(p[axis]) - float(q[axis]) <= float(radius)                   # within the radius by the float64 rule
        assert ip in nr.neighbours(P, radius)[0][iq]
        gq = F(F(q[axis] - org[axis]) * inv_h)
        gp = F(F(p[axis] - org[axis]) * inv_h)
        assert int(np.floor(gp)) - int(np.floor(gq)) == R_old + 1, (gq, gp)
        assert int(np.floor(gp)) < int(np.floor((float(P[:, axis].max()) - float(org[axis])) / float(h)))     # clear of the clamp
        assert ref["count"][iq] >= 3 and ref["count"][ip] >= 3
        # without the other end the covariance moves by far more than its bound
        for a, b in ((iq, ip), (ip, iq)):
            without = nr.estimate(np.delete(P, b, 0), radius)
            row = a - (b < a)
            assert np.abs(without["cov6"][row] - ref["cov6"][a]).max() > 1e6 * ref["tol"]["cov"][a]


def test_straddle_pairs_are_enough():
    assert sum(len(nr.cases()["straddle_%g_%d" % ck]["pairs"]) for ck in nr.STRADDLE) >= 12


@pytest.mark.parametrize("name", ["boundary_0.25", "boundary_0.3", "boundary_0.3_cell_0.25"])
def test_boundary_has_both_kinds(name):
    case, ref = nr.cases()[name], nr.reference(name)
    P = case["points"].astype(np.float64)
    r = case["radius"]
    assert ref["at_r"] >= 20
    outside = 0
    for axis in range(3):
        e = np.abs(P[:, None, :] - P[None, :, :])
        d = e[:, :, axis]
        same = (np.delete(e, axis, 2) == 0).all(2)
        up = np.nextafter((P[:, axis].astype(F)), F(np.inf)).astype(np.float64)
        dn = np.nextafter((P[:, axis].astype(F)), F(-np.inf)).astype(np.float64)
        # pairs (a, b) on this axis where b lies one float32 step beyond a point exactly r from a
        one_past = ((dn[None, :] - P[:, None, axis] == r) | (P[:, None, axis] - up[None, :] == r)) & same
        assert (d[one_past] > r).all()
        outside += int(one_past.sum())
    assert outside >= 20
    lists = nr.neighbours(case["points"], r)[0]
    assert all(len(v) == c for v, c in zip(lists, ref["count"]))


def test_counts_fixture():
    case, ref = nr.cases()["counts"], nr.reference("counts")
    want = np.concatenate([np.full(g, g) for g in case["groups"]])
    assert np.array_equal(ref["count"], want)


def test_degenerate_fixture():
    case, ref = nr.cases()["degenerate"], nr.reference("degenerate")
    assert ref["count"].min() >= 3
    a, b = case["groups"]["spot"]
    assert b - a == 300 and (ref["count"][a:b] == 300).all() and not ref["cov6"][a:b].any()
    for name, axis in case["answers"].items():
        a, b = case["groups"][name]
        assert ref["exact"][a:b].all(), name
        assert (ref["normal"][a:b] == np.eye(3, dtype=F)[axis]).all(), name
    a, b = case["groups"]["line_d"]
    assert not ref["tol"]["separated"][a:b].any() and not ref["exact"][a:b].any()
    for name in ("plane_x", "plane_y", "plane_z"):
        a, b = case["groups"][name]
        assert ref["tol"]["separated"][a:b].all()


def test_tilted_fixture():
    case, ref = nr.cases()["tilted"], nr.reference("tilted")
    assert (ref["count"] == 25).all() and ref["tol"]["separated"].all() and not ref["exact"].any()
    a, b = case["groups"]["xy"]
    assert not ref["cov6"][a:b, 2].any() and not ref["cov6"][a:b, 4].any() and (ref["cov6"][a:b, 1] > 0).all()
    s = np.sqrt(0.5)
    a, b = case["groups"]["xz"]
    assert np.abs(np.abs(ref["normal64"][a:b]) - [s, 0, s]).max() < 1e-12
    a, b = case["groups"]["xy"]
    assert np.abs(np.abs(ref["normal64"][a:b]) - [s, s, 0]).max() < 1e-12


@pytest.mark.parametrize("n", nr.SIZES)
def test_size_fixture(n):
    ref = nr.reference("size_%d" % n)
    assert len(ref["count"]) == n
    if n >= 63:
        assert (ref["count"] >= 3).mean() >= 0.9
    if n < 3:
        assert (ref["count"] < 3).all()


def test_grid_edge_fixtures():
    for name in ("sheet", "rod"):
        case, ref = nr.cases()[name], nr.reference(name)
        P = case["points"]
        for axis in case["dims_one"]:
            assert P[:, axis].min() == P[:, axis].max()
        ok = ref["count"] >= 3
        assert ok.sum() >= 100 and ref["exact"][ok].all()
        assert (ref["normal"][ok] == np.eye(3, dtype=F)[2 if name == "sheet" else 1]).all()
    case, ref = nr.cases()["whole_extent"], nr.reference("whole_extent")
    assert (ref["count"] == len(case["points"])).all()
    assert 1900 <= len(nr.scene_points()) <= 2100
    for a, b in nr.SAME_COUNTS:
        ca, cb = nr.cases()[a], nr.cases()[b]
        assert np.array_equal(ca["points"], cb["points"]) and ca["radius"] == cb["radius"]
        assert (ca["cell"], ca["lattice"]) != (cb["cell"], cb["lattice"])
    for cells in (0.1, 1.6, 2.5, 3.3):
        assert nr.cases()["scene_%g" % cells]["radius"] == float(F(cells) * F(0.25))
    assert (nr.reference("scene_0.1")["count"] < 3).mean() > 0.5 and (nr.reference("scene_3.3")["count"] >= 3).all()


def test_far_fixtures_scale_the_bound():
    near, f1, f3 = nr.reference("scene_1.6"), nr.reference("far_1km"), nr.reference("far_3km")
    assert 1000 < f1["coord_max"] < 1020 and 3000 < f3["coord_max"] < 3020
    m = 50.0
    assert nr.cov_tol(m, 3000.0, 0.4) > nr.cov_tol(m, 1000.0, 0.4) > nr.cov_tol(m, 10.0, 0.4)
    assert (f3["count"] >= 3).mean() > 0.9 and near["tol"]["separated"].mean() > 0.9


def test_nonfinite_fixture():
    case, ref = nr.cases()["nonfinite"], nr.reference("nonfinite")
    bad = ~np.isfinite(case["points"]).all(1)
    assert bad.sum() == 12 and np.array_equal(np.flatnonzero(bad), case["bad_rows"])
    P = case["points"]
    assert np.isnan(P).any() and (P == np.inf).any() and (P == -np.inf).any()
    assert not ref["indexed"][bad].any() and not ref["count"][bad].any() and not ref["normal"][bad].any() and not ref["cov6"][bad].any()
    assert (ref["count"][~bad] >= 1).all()
