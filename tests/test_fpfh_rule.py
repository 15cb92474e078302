"""The numpy restatement of the FPFH and matching rules (tests/fpfh_ref_np.py) held against facts it was not built from, and the
condition the exact GPU comparisons rest on: no binned value of a fixture within 1e-9 of an inner bin edge (the device's and numpy's
atan2 / sqrt differ by a few ulp of float64, about 1e-15, which then cannot move a bin).  CPU only."""
import numpy as np
import pytest

import fpfh_ref_np as ref

MARGIN = 1e-9


def spacing_ok(got, want):
    """every value within one float32 spacing of the reference value"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.maximum(np.abs(got), np.abs(want))).astype(np.float64)


@pytest.mark.parametrize("name", sorted(ref.fixtures()))
def test_fixture_margin_and_group_sums(name):
    r = ref.reference(name)
    assert r["margin"] >= MARGIN, (name, r["margin"])
    cnt, P = r["counts"].astype(np.int64), r["n_pairs"].astype(np.int64)
    for g in range(3):                                      # every pair lands in exactly one bin of every group
        assert np.array_equal(cnt[:, g * 11:(g + 1) * 11].sum(1), P)
    has = P > 0
    assert np.array_equal(r["valid"], has)
    spf = cnt[has] * (100.0 / P[has])[:, None]
    assert np.allclose(spf.reshape(-1, 3, 11).sum(2), 100.0, rtol=0, atol=1e-9)
    sums = r["rows64"][has].reshape(-1, 3, 11).sum(2)
    assert np.all((np.abs(sums - 200.0) < 1e-9) | (np.abs(sums - 100.0) < 1e-9))
    assert np.all(r["rows64"][~has] == 0) and np.all(r["rows"][~has] == 0)
    if has.any() and name.startswith("scene"):
        assert (np.abs(sums - 200.0) < 1e-9).mean() > 0.9   # a point with a featured neighbour has S_g > 0


def test_special_fixture_holds_every_edge_case():
    f, r = ref.fixtures()["special"], ref.reference("special")
    n = len(f["points"])
    assert np.all(r["n_pairs"][n - 5:] == 0) and not r["valid"][n - 5:].any()      # the |v| = 0 pair and the non-finite points
    assert np.all(r["n_pairs"][20:32] == 0)                                          # zero and non-finite normals
    assert r["stats"]["n_valid"] == n - 3 and 0 < r["stats"]["n_featured"] < n - 17
    dup = np.arange(n - 15, n - 5)
    assert np.array_equal(r["counts"][dup], r["counts"][dup - (n - 15)])            # a duplicate shares every pair but the L = 0 one


def test_planar_lattice_with_equal_normals():
    g = np.arange(12, dtype=np.float32) * np.float32(0.125)
    pts = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    pts = np.concatenate([pts, np.full((len(pts), 1), 0.5, np.float32)], 1).astype(np.float32)
    nrm = np.broadcast_to(np.float32([0, 0, 1]), pts.shape)
    r = ref.fpfh(pts, nrm, 0.3)
    assert r["valid"].all() and abs(r["margin"] - 0.5) < 1e-12    # every value sits at 5.5
    other = np.ones(33, bool)
    other[[5, 16, 27]] = False
    assert np.all(r["counts"][:, other] == 0) and np.all(r["counts"][:, [5, 16, 27]] == r["n_pairs"][:, None])
    assert np.all(r["rows"][:, [5, 16, 27]] == 200.0) and np.all(r["rows"][:, other] == 0.0)


@pytest.mark.parametrize("orient, toward", [(0, (0, 0, 1)), (1, (0.3, -0.2, 1.0)), (2, (2.0, 1.0, 3.0))])
def test_rigid_motion_leaves_the_descriptors(orient, toward):
    """A quarter turn about z and a dyadic translation move points on a 2^-10 lattice exactly, and leave the float32 d2 as it was
    bit for bit (dx and dy trade places under a commutative sum): the neighbours are the same, only float64 roundings differ."""
    pts, nrm = ref.scene_cloud(500, 21)
    pts = (np.round(pts.astype(np.float64) * 1024) / 1024).astype(np.float32)
    R = np.float64([[0, -1, 0], [1, 0, 0], [0, 0, 1]])
    t = np.float64([1.0, -2.0, 0.5])
    pts2 = (pts.astype(np.float64) @ R.T + t).astype(np.float32)
    assert np.array_equal(pts2.astype(np.float64), pts.astype(np.float64) @ R.T + t)
    nrm2 = (nrm.astype(np.float64) @ R.T).astype(np.float32)
    tw = np.float64(toward)
    tw2 = R @ tw + (t if orient == 2 else 0.0)
    a, b = ref.fpfh(pts, nrm, 0.3, orient, tw), ref.fpfh(pts2, nrm2, 0.3, orient, tw2)
    assert a["margin"] >= MARGIN and b["margin"] >= MARGIN
    assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["valid"], b["valid"]) and a["stats"] == b["stats"]
    assert spacing_ok(a["rows"], b["rows"]).all()
    assert a["stats"]["n_featured"] > 400


def test_orientation_rules():
    f = ref.fixtures()
    inside, none = ref.reference("orient_inside"), None
    p = f["orient_inside"]
    none = ref.fpfh(p["points"], -p["normals"], p["radius"], 0)      # the viewpoint inside the sphere flips every outward normal
    assert np.array_equal(inside["counts"], none["counts"]) and np.array_equal(inside["rows"], none["rows"])
    n, has = ref.oriented_normals(p["points"], p["normals"], 2, p["toward"])
    assert has.all() and np.array_equal(n, -p["normals"].astype(np.float64))
    q = f["orient_direction"]
    n, _ = ref.oriented_normals(q["points"], q["normals"], 1, q["toward"])
    assert np.all(n @ np.float64(q["toward"]) >= 0) and np.array_equal(np.abs(n), np.abs(q["normals"].astype(np.float64)))
    assert not np.array_equal(ref.reference("orient_none")["counts"], ref.reference("orient_direction")["counts"])


def test_matcher_reference_against_scipy():
    cdist = pytest.importorskip("scipy.spatial.distance").cdist
    A, B = ref.descriptor_rows(300, 1), ref.descriptor_rows(700, 2)
    va, vb = np.ones(300, bool), np.ones(700, bool)
    va[::17] = False
    vb[::5] = False
    m = ref.match(A, va, B, vb)
    D = cdist(A.astype(np.float64), B.astype(np.float64), "sqeuclidean")
    D[:, ~vb] = np.inf
    srt = np.sort(D, axis=1)
    assert ((srt[:, 1] - srt[:, 0]) > 1e-5 * srt[:, 0]).all()       # no near-ties (float32 D errs by < 33 * 2^-23): the same winner
    assert np.array_equal(m["idx"][va], np.argmin(D, axis=1)[va]) and np.all(m["idx"][~va] == -1)
    assert np.allclose(m["dist2"][va], srt[va, 0], rtol=1e-5) and np.allclose(m["second2"][va], srt[va, 1], rtol=1e-5)
    assert np.all(np.isinf(m["dist2"][~va])) and m["stats"]["n_matched"] == int(va.sum()) == len(m["pairs"])


def test_matcher_reference_rules():
    A = ref.descriptor_rows(200, 3)
    B = np.concatenate([A[50:150], A[50:150]])                       # every candidate twice: the smaller index wins, runner-up = best
    m = ref.match(A, None, B, None, ratio=0.9)
    hit = np.arange(50, 150)
    assert np.array_equal(m["idx"][hit], hit - 50) and np.all(m["dist2"][hit] == 0) and np.all(m["second2"][hit] == 0)
    assert not np.isin(m["pairs"][:, 0], hit).any()                  # 0 < r * 0 fails: a duplicated best is ambiguous
    mu = ref.match(A, None, B, None, mutual=True)
    assert np.isin(hit, mu["pairs"][:, 0]).all() and len(mu["pairs"]) <= len(B)
    back = ref.match(B, None, A, None)["idx"]
    assert all(back[j] == i for i, j in mu["pairs"])
    self_ = ref.match(A, None, A, None, mutual=True)
    assert np.all(self_["dist2"] == 0) and np.array_equal(self_["idx"], np.arange(200)) and self_["stats"]["n_matched"] == 200
    bad = A.copy()
    bad[7, 3] = np.nan
    r = ref.match(bad, np.ones(200), A, None, cap_pairs=5)
    assert r["idx"][7] == -1 and r["stats"]["n_src_valid"] == 199 and r["stats"]["n_matched"] == 199 and len(r["pairs"]) == 5
    none = ref.match(A, None, A, np.zeros(200))
    assert np.all(none["idx"] == -1) and np.all(np.isinf(none["dist2"])) and none["stats"]["n_matched"] == 0
