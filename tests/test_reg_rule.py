"""tests/reg_ref_np.py, the numpy restatement of the pose-from-matches rule, pinned to facts it was not built
from: the known answers of the generator, numpy.linalg.svd Kabsch for Horn's closed form, a float64 distance count for the score, and
the known pose of the fixtures.  No device call."""
import os

import numpy as np
import pytest

import plane_ref_np as plane
import reg_ref_np as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "register_small.npz")
THR, SIM, H, SEED = 0.05, 0.9, 4096, 1


def test_mix_known_answers():
    """the section 18 answers hold here: the same generator, pairs in place of points"""
    assert ref.mix(0) == 0xE220A8397B1DCDAF
    s = ref.samples(1, 2, 20000)
    assert s.dtype == np.int32 and s.tolist() == [[8519, 10590, 235], [8761, 10048, 7045]]
    assert ref.samples((1 << 64) - 1, 3, 7).max() < 7            # the seed wraps around
    for seed in (0, 1, 12345, (1 << 64) - 5):
        assert np.array_equal(ref.samples(seed, 300, 2999), plane.samples(seed, 300, 2999))
    x = np.array([0, 1, (1 << 64) - 1, 0x9E3779B97F4A7C15], np.uint64)
    assert [int(v) for v in ref.mix_u64(x)] == [ref.mix(int(v)) for v in x]


def kabsch_svd(P, Q):
    """numpy.linalg.svd Kabsch: the proper rotation and translation that map P onto Q in the least-squares sense"""
    cp, cq = P.mean(axis=0), Q.mean(axis=0)
    U, _, Vt = np.linalg.svd((P - cp).T @ (Q - cq))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, cq - R @ cp


def random_rotation(rng):
    q = rng.normal(size=4)
    return ref.rotation_of(q / np.linalg.norm(q))


def test_horn_against_svd_kabsch():
    """Horn's closed form against Kabsch on random triangles (noisy: the fit is not exact), within 64 eps |N| / gap per entry of R"""
    rng = np.random.default_rng(5)
    worst = 0.0
    for case in range(400):
        P = rng.uniform(-10, 10, (3, 3)) + rng.uniform(-50, 50, 3)
        R0, t0 = random_rotation(rng), rng.uniform(-20, 20, 3)
        Q = P @ R0.T + t0 + rng.normal(0, 0.02, (3, 3))
        cs, ct = P.mean(axis=0), Q.mean(axis=0)
        T, gap, norm = ref.horn((P - cs).T @ (Q - ct), cs, ct)
        R, t = kabsch_svd(P, Q)
        tol_r, tol_t = ref.horn_tolerance(gap, norm, cs, ct)
        err = np.abs(T[:3, :3] - R).max()
        worst = max(worst, err / tol_r)
        assert err <= tol_r, (case, err, tol_r)
        assert np.abs(T[:3, 3] - t).max() <= tol_t, (case, np.abs(T[:3, 3] - t).max(), tol_t)
        assert np.array_equal(T[3], [0, 0, 0, 1])
    print("largest |dR| / (64 eps |N| / gap) over 400 triangles: %.4f" % worst)
    assert worst > 0                                              # two solvers, not one


def test_rotation_is_proper_even_for_a_mirrored_target():
    rng = np.random.default_rng(6)
    for case in range(100):
        P = rng.uniform(-5, 5, (3, 3))
        Q = P @ random_rotation(rng).T + rng.uniform(-5, 5, 3)
        if case % 2:
            Q = Q * np.array([1.0, 1.0, -1.0])                   # a reflection: no proper rotation fits exactly
        cs, ct = P.mean(axis=0), Q.mean(axis=0)
        R = ref.horn((P - cs).T @ (Q - ct), cs, ct)[0][:3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1.0) < 1e-14, case
    q = np.array([0.5, -0.5, 0.5, 0.5])
    assert np.allclose(ref.rotation_of(q) @ [1.0, 0.0, 0.0], [0.0, 0.0, -1.0])        # x -> -z under this quaternion: Hamilton's convention


def triangle_status(s3, t3, sim):
    s, t = np.asarray(s3, np.float32), np.asarray(t3, np.float32)
    return int(ref.hypotheses_from_samples(s, t, np.array([[0, 1, 2]], np.int32), sim)["status"][0])


def test_edge_check_and_degenerate_cases():
    s3 = np.array([[0, 0, 0], [4, 0, 0], [0, 2, 0]], np.float64)
    quarter = s3 @ ref.rot_z(90).T + [8, -4, 0.5]                   # exact in float32
    assert triangle_status(s3, quarter, 1.0) == 0                  # a congruent triangle passes at 1.0
    scaled = quarter.copy()
    scaled[1] = quarter[0] + 0.89 * (quarter[1] - quarter[0])      # edge (0, 1) at 0.89 of its length
    assert triangle_status(s3, scaled, 0.9) == 2 and triangle_status(s3, scaled, 0.0) == 0 and triangle_status(s3, scaled, 0.85) == 0
    assert triangle_status(scaled, s3, 0.9) == 2                   # the check is symmetric
    assert triangle_status([[0, 0, 0], [1, 1, 1], [2, 2, 2]], quarter, 0.0) == 1       # collinear
    assert triangle_status(s3, [[0, 0, 0], [1, 0, 0], [np.nan, 0, 0]], 0.0) == 1       # a non-finite point
    s, t = np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32)
    assert ref.hypotheses_from_samples(s, t, np.array([[0, 0, 1], [1, 2, 1], [3, 2, 2]], np.int32), 0.0)["status"].tolist() == [1, 1, 1]   # equal samples
    hyp = ref.hypotheses_from_samples(s3.astype(np.float32), scaled.astype(np.float32), np.array([[0, 1, 2], [0, 0, 1]], np.int32), 0.9)
    assert np.isnan(hyp["T"]).all()                                # statuses 1 and 2 carry sixteen NaNs


def test_score_against_a_float64_count():
    src, dst, pairs, truth, T = ref.workhorse()
    s, t = ref.pack(src, dst, pairs)
    Tf = ref.to_f32(np.stack([T, np.eye(4), ref.pose(10.0, (0, 0, 0))]))
    counts = ref.score(s, t, Tf, THR)
    d = np.linalg.norm(s.astype(np.float64) @ T[:3, :3].T + T[:3, 3] - t, axis=1)
    assert abs(int(counts[0]) - int((d < THR).sum())) <= int((np.abs(d - THR) < 1e-4).sum())   # only pairs at the threshold may differ
    assert counts[0] >= 0.95 * truth.sum() and counts[1] < 5 and counts[2] < 5
    bad = np.full((1, 12), np.nan, np.float32)
    assert ref.score(s, t, bad, THR)[0] == 0                       # NaN never compares


def test_tile_sum_is_a_sum():
    rng = np.random.default_rng(3)
    for n in (0, 1, 63, 64, 255, 256, 257, 3000):
        v = rng.uniform(0, 1, n)
        assert abs(ref.tile_sum(v) - float(np.sum(v))) <= 1e-12 * max(n, 1)


@pytest.fixture(scope="module")
def workhorse():
    src, dst, pairs, truth, T = ref.workhorse()
    return dict(src=src, dst=dst, pairs=pairs, truth=truth, T=T, reg=ref.register(src, dst, pairs, THR, SIM, H, 2, 3, 8, SEED))


def test_the_workhorse_finds_the_pose(workhorse):
    """m = 3000, a quarter true under 140 degrees of yaw and 12 m, sigma 0.01; threshold 0.05, similarity 0.9, H = 4096, seed 1"""
    w, reg = workhorse, workhorse["reg"]
    assert abs(np.linalg.norm(w["T"][:3, 3]) - 12.0) < 0.05 and w["truth"].sum() == 750
    all_true = w["truth"][reg["samples"]].all(axis=1)
    assert all_true.sum() >= 8, all_true.sum()                     # about 4096 / 64 are expected: the fixture cannot pass by luck
    assert reg["found"] == 1 and all_true[reg["stats"]["best"]] and reg["stats"]["rounds_done"] == 2
    moved = w["src"].astype(np.float64) @ reg["T"][:3, :3].T + reg["T"][:3, 3]
    want = w["src"].astype(np.float64) @ w["T"][:3, :3].T + w["T"][:3, 3]
    assert np.linalg.norm(moved - want, axis=1).max() < THR       # every point within the threshold of where the truth puts it
    noise = np.linalg.norm(want - w["dst"].astype(np.float64), axis=1)
    assert not (reg["inlier"] & ~w["truth"]).any()                 # the inlier set is the true pairs ...
    assert not (w["truth"] & ~reg["inlier"] & (noise <= 0.03)).any()   # ... up to those beyond 3 sigma
    st = reg["stats"]
    assert st["n_degenerate"] + st["n_rejected"] + st["n_scored"] == H and st["n_rejected"] > 0.9 * H
    assert [c["count"] for c in reg["top"]] == sorted((c["count"] for c in reg["top"]), reverse=True) and reg["top"][0]["h"] == st["best"]
    assert st["fitness"] == st["n_inliers"] / 3000 and 0 < st["rmse"] < 3 * 0.01 * np.sqrt(3)


def test_the_golden_fixture_is_the_workhorse(workhorse):
    """tests/golden/register_small.npz: the inputs and the restatement's exact results, what the device test compares with"""
    g = np.load(GOLDEN, allow_pickle=False)
    w, reg = workhorse, workhorse["reg"]
    for name in ("src", "dst", "pairs", "truth", "T"):
        assert g[name].dtype == w[name].dtype and np.array_equal(g[name], w[name]), name
    assert np.array_equal(g["samples"], reg["samples"]) and np.array_equal(g["status"], reg["hyp"]["status"])
    assert np.array_equal(g["counts"], reg["counts"])
    assert [int(g[k]) for k in ("best", "best_count")] == [reg["stats"]["best"], reg["stats"]["best_count"]]
    assert os.path.getsize(GOLDEN) < 256 * 1024


def test_the_dyadic_tie():
    """noise-free, a quarter turn and a dyadic translation: every all-true hypothesis maps every true pair exactly, so several tie at
    the full true count and the smallest h must win"""
    src, dst, pairs, truth, T = ref.dyadic()
    reg = ref.register(src, dst, pairs, THR, SIM, H, 0, 3, 8, SEED)
    counts, n_true = reg["counts"], int(truth.sum())
    tied = np.flatnonzero(counts == counts.max())
    assert counts.max() == n_true == 128 and len(tied) >= 8 and reg["stats"]["best"] == tied[0] == 42
    assert [c["h"] for c in reg["top"]] == tied[:8].tolist()
    assert np.array_equal(reg["inlier"], truth) and reg["stats"]["rmse"] < 1e-12
    assert np.abs(reg["T"] - T).max() < 1e-13 and reg["stats"]["rounds_done"] == 0
