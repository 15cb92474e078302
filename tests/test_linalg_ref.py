"""tests/linalg_ref_np.py checked against itself where two routes exist (the long-double Kabsch against the float64 one of
tests/test_oracle_icp.py on centred data, the long-double elimination against numpy.linalg.solve, Rz Ry Rx against a
rotation-vector composition), and every generated case set against its own preconditions: the stated ranks, gaps and condition
numbers.  No GPU: the device side of these case sets is tests/test_gpu_linalg_direct.py."""
import math

import numpy as np
import pytest

import linalg_ref_np as ref
from linalg_ref_np import EPS, LD
from test_oracle_icp import np_kabsch


def test_long_double_is_wider_than_double():
    assert np.finfo(LD).eps < EPS / 1000


def test_kabsch_ld_against_float64_kabsch_on_centred_data():
    rng = np.random.default_rng(1)
    for src, tgt, R, t in ref.rigid_sets(rng):
        c = src.mean(0)
        T64 = np_kabsch(src - c, tgt - c)
        Tld, unique = ref.kabsch_ld(src - c, tgt - c)
        assert unique
        assert np.abs(T64 - Tld).max() <= 256 * EPS * (1 + np.abs(t).max())       # the float64 route is the loose one
        assert np.abs(Tld[:3, :3] - R).max() <= 8 * EPS                              # the polished one finds the motion itself


def test_polish_recovers_a_perturbed_rotation():
    rng = np.random.default_rng(2)
    for src, tgt, R, t in ref.rigid_sets(rng, sizes=(5, 50)):
        s, g = src.astype(LD), tgt.astype(LD)
        H = (s - s.mean(0)).T @ (g - g.mean(0))
        bad = ref.rodrigues(rng.normal(size=3) * 1e-9) @ R
        assert np.abs(bad - R).max() > 1e-10
        assert np.abs(ref.polish_rotation_ld(bad, H).astype(float) - R).max() <= 8 * EPS


def test_solve6_ld_against_numpy_solve():
    rng = np.random.default_rng(3)
    for cond in (1.0, 1e3, 1e6):
        for _ in range(20):
            A, b = ref.spd_with_cond(rng, cond), rng.normal(size=6)
            x = ref.solve6_ld(A, b).astype(float)
            xn = np.linalg.solve(A, b)
            assert np.linalg.norm(x - xn) <= 64 * cond * EPS * np.linalg.norm(xn)
            assert np.abs((A.astype(LD) @ ref.solve6_ld(A, b) - b).astype(float)).max() <= 64 * np.finfo(LD).eps * cond * np.abs(b).max()


def test_vec6_ref_is_the_rotation_vector_composition():
    rng = np.random.default_rng(4)
    for v in ref.vec6_cases(rng)[::37]:
        want = ref.rodrigues([0, 0, v[2]]) @ ref.rodrigues([0, v[1], 0]) @ ref.rodrigues([v[0], 0, 0])
        T = ref.vec6_ref(v).astype(float)
        assert np.abs(T[:3, :3] - want).max() <= 16 * EPS * max(1.0, np.abs(v[:3]).max())   # (float64 range reduction of 1e3 rad)
        assert (T[:3, 3] == v[3:]).all() and (T[3] == [0, 0, 0, 1]).all()
    assert np.abs(ref.vec6_ref([0, 0, math.pi / 2, 1, 2, 3]).astype(float)[:3, :3] - [[0, -1, 0], [1, 0, 0], [0, 0, 1]]).max() <= EPS


def test_robust_ref_known_values():
    K = ref.ROBUST_KINDS
    assert ref.robust_ref(K["none"], 1.0, 5.0) == 1
    assert ref.robust_ref(K["huber"], 2.0, 1.0) == 1 and ref.robust_ref(K["huber"], 2.0, -8.0) == 0.25
    assert ref.robust_ref(K["cauchy"], 2.0, 2.0) == 0.5
    assert ref.robust_ref(K["tukey"], 2.0, 1.0) == 0.5625 and ref.robust_ref(K["tukey"], 2.0, 2.5) == 0
    assert ref.robust_ref(K["gm"], 1.0, 1.0) == 0.25
    rows = ref.robust_cases(np.random.default_rng(5))
    assert set(rows[:, 0]) == set(K.values()) and (rows[:, 1] > 0).all()
    for k in set(rows[:, 1]):
        assert ((rows[:, 1] == k) & (rows[:, 2] == k)).any() and ((rows[:, 1] == k) & (rows[:, 2] == -k)).any() and ((rows[:, 1] == k) & (rows[:, 2] == 0)).any()
    assert (np.abs(rows[:, 2]) / rows[:, 1]).max() == 1e6


def test_rsqrt_cases_are_inside_the_domain():
    x = ref.rsqrt_cases(np.random.default_rng(6))
    assert (x >= ref.DBL_MIN).all() and (x <= 1e300).all() and np.isfinite(x).all()
    assert (x == ref.DBL_MIN).any() and x.min() == ref.DBL_MIN and x.max() == 1e300
    rs, rc = ref.rsqrt_ref(np.array([4.0, 0.25]))
    assert (rs == [0.5, 2.0]).all() and (rc == [0.25, 4.0]).all()
    assert (ref.ulps(np.array([1.0 + EPS]), np.array([1.0], dtype=LD)) == 1).all()


def test_svd3_case_sets_have_their_ranks():
    sets = ref.svd3_cases(np.random.default_rng(7))
    for name, (A, rank) in sets.items():
        assert len(A) == len(rank) and np.isfinite(A).all()
        s = np.linalg.svd(A, compute_uv=False)
        numerical = (s > 8 * EPS * np.maximum(s[:, :1], 1e-300)).sum(1)         # svd3's own rank threshold
        assert (numerical == rank).all(), name
        if name in ("rank1", "rank2"):
            assert (A == np.round(A)).all()                                      # exact: small integers
    assert (np.linalg.det(sets["det_negative"][0]) < 0).all()
    noise = sets["rank2_noise"][0] - sets["rank2"][0]
    assert 0 < np.abs(noise).max() < 1e-16
    s = np.linalg.svd(sets["repeated"][0], compute_uv=False)
    assert (np.abs(s[:100, 0] - s[:100, 1]) < 16 * EPS).all() and (np.abs(s[100:200] - 1) < 16 * EPS).all()
    assert len(sets["random"][0]) >= 1000 and len(sets["permutation"][0]) == 18


def test_rigid_sets_are_well_spread_and_where_they_claim():
    for offset in (0.0, 1e2, 1e3, 1e4):
        sets = ref.rigid_sets(np.random.default_rng(8), offset=offset)
        assert sorted({len(s) for s, _, _, _ in sets}) == [3, 4, 5, 7, 10, 33, 100, 500, 2000]
        for src, tgt, R, t in sets:
            assert ref.scatter_cond(src) <= ref.RIGID_COND
            assert abs(np.linalg.norm(src.mean(0)) - offset) <= 5 * 5.0 / math.sqrt(len(src)) + 1e-9
            assert np.abs(R.T @ R - np.eye(3)).max() <= 8 * EPS and np.abs(src @ R.T + t - tgt).max() == 0
            assert np.abs(tgt.mean(0) - src.mean(0)).max() <= 1 + 0.5 * 5.0 * 5              # an ICP-sized step
    assert ref.offset_law_bound(0.0) == 64 * EPS and ref.offset_law_bound(1e3) == 16 * EPS * 1e9 / 25 + 64 * EPS * 1001
    # the law stays below the float32 quantum 2^-24 |c| while |c| / sigma < 2^14
    c = 5.0 * 2 ** 14 * 0.99
    assert EPS * c ** 3 / 25 < 2.0 ** -24 * c


def test_ldlt6_case_sets_have_their_conditions():
    cases = ref.ldlt6_cond_cases(np.random.default_rng(9))
    for name, A, b in cases:
        assert np.array_equal(A, A.T)
        if name.startswith("cond"):
            want = float(name[4:])
            assert 0.5 * want <= np.linalg.cond(A) <= 2 * want * (1 + 1e-3 * (want >= 1e12)), name
        else:
            assert np.linalg.eigvalsh(A).min() > 0
    assert np.median([np.linalg.cond(A) for n, A, _ in cases if n == "walls1000"]) > 100 * np.median([np.linalg.cond(A) for n, A, _ in cases if n == "walls0"])
    refused = dict(ref.ldlt6_refused_cases())
    assert np.linalg.matrix_rank(refused["normals_all_z"]) == 3 and (refused["normals_all_z"][2] == 0).all()
    assert np.linalg.matrix_rank(refused["rank1"]) == 1 and not refused["zero"].any()
    assert sum(1 for n in refused if n.startswith(("nan", "inf", "-inf"))) == 3 * 21
    A, b, rank = ref.ldlt6_deficient_cases(np.random.default_rng(10), 300)
    ok = np.isfinite(A).all((1, 2))
    assert ok.mean() > 0.5 and set(rank) == {1, 2, 3, 4, 5}
    for Ai, ri in zip(A[ok][:100], rank[ok][:100]):
        assert np.linalg.matrix_rank(Ai / np.abs(Ai).max(), tol=1e-9) == ri
    lg = np.log10(np.abs(A[ok]).max((1, 2)))
    assert lg.min() < -200 and lg.max() > 200
    A, b = ref.near_planar_case()
    assert 1e18 < np.linalg.cond(A) and np.isfinite(A).all()


@pytest.mark.parametrize("n", [3, 6])
def test_jacobi_case_sets(n):
    sets = ref.jacobi_cases(np.random.default_rng(11), n)
    for name, A in sets.items():
        assert np.array_equal(A, np.swapaxes(A, 1, 2)) and np.isfinite(A).all(), name
    lam = np.linalg.eigvalsh(sets["psd_wide"])
    assert (lam[:, 0] > -1e-10).all() and (lam[:, -1] / np.maximum(lam[:, 0], 1e-300)).max() > 1e10
    assert (np.diagonal(sets["zero_diagonal"], axis1=1, axis2=2) == 0).all() and np.abs(sets["zero_diagonal"]).max() > 0
    lam = np.linalg.eigvalsh(sets["indefinite"])
    assert (lam[:, 0] < 0).all() and (lam[:, -1] > 0).all()
    lam = np.linalg.eigvalsh(sets["clustered"])
    assert ((lam[:, 1] - lam[:, 0]) < 1e-8).mean() > 0.6
    d = sets["diagonal"]
    assert (d == d * np.eye(n)).all()


def test_eigvec_case_sets():
    sets = ref.eigvec_cases(np.random.default_rng(12))
    for name, Cm in sets.items():
        assert np.array_equal(Cm, np.swapaxes(Cm, 1, 2)) and np.isfinite(Cm).all()
    lam = np.linalg.eigvalsh(sets["plane"])
    assert (lam[:, 0] < 1e-2 * lam[:, 1]).all() and len(lam) == 200
    assert np.log10(lam[:, 2]).min() < -6 and np.log10(lam[:, 2]).max() > 2
    ax = sets["axis_aligned"]
    assert (ax == ax * np.eye(3)).all() and {int(np.argmin(np.diag(c))) for c in ax} == {0, 1, 2}
    lam = np.linalg.eigvalsh(sets["line"])
    assert (lam[:, 1] < 1e-3 * lam[:, 2]).all()
    lam = np.linalg.eigvalsh(sets["blob"])
    assert (lam[:, 0] > 0.05 * lam[:, 2]).all()
    assert not sets["zero"].any()
    assert ref.sign_rule([0, 0, 1]) and ref.sign_rule([1, 0, 0]) and ref.sign_rule([-1, 1, 0]) and not ref.sign_rule([0, -1, 0]) and not ref.sign_rule([1, 1, -1e-9])
    pts = np.random.default_rng(13).normal(size=(20, 3))
    assert np.allclose(ref.neighbourhood_cov(pts), np.cov(pts.astype(np.float32).astype(float).T, bias=True) * 20, rtol=1e-12)


def test_reduce_inputs():
    rng = np.random.default_rng(14)
    v = ref.reduce_inputs(rng, (1000, 30), "integer")
    assert (v == np.round(v)).all() and np.abs(v).max() < 2 ** 30
    assert np.array_equal(ref.fsum_columns(v), v.sum(0))                           # 1000 * 2^30 < 2^53: exact in any order
    v = ref.reduce_inputs(rng, (256, 32), "random")
    assert (v < 0).any() and (v > 0).any() and np.log10(np.abs(v).max() / np.abs(v).min()) > 10
    assert ref.fsum_columns(np.array([[1e16], [1.0], [-1e16]]))[0] == 1.0
    k = ref.kabsch_record(np.array([[1.0, 2, 3], [4, 5, 6]]), np.array([[1.0, 0, 0], [0, 1, 0]]))
    assert k[0] == 2 and (k[1:4] == [5, 7, 9]).all() and (k[4:7] == [1, 1, 0]).all() and (k[7:16] == [1, 4, 0, 2, 5, 0, 3, 6, 0]).all() and not k[16:].any()
