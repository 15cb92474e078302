"""Pose estimation from matches on the device (sf_cloud_pair_hypotheses, sf_cloud_score_poses, sf_cloud_register_pairs,
sf_test_score_poses) against the numpy restatement of the rule (tests/reg_ref_np.py), which
tests/test_reg_rule.py pins to independent code.

Samples, statuses and their counts are compared exactly.  A status-0 transform comes from another eigen-solver than the
restatement's, so it is compared within reg_ref_np.horn_tolerance (64 eps |N| / gap per entry of R, carried through cs into t).
Everything downstream of a transform -- inlier counts, the choice, the top list, the mask, n_inliers, rmse -- is a function of the
float32 transform's bits, so it is compared exactly against the rule applied to the transforms the device itself returned (or was
given).  The workhorse is tests/golden/register_small.npz (reg_ref_np.workhorse(): m = 3000, a quarter true under 140 degrees of
yaw and 12 m, sigma 0.01), at threshold 0.05, similarity 0.9, H = 4096, seed 1."""
import ctypes
import os

import numpy as np
import pytest

import reg_ref_np as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR, SIM, H, SEED = 0.05, 0.9, 4096, 1
INVALID = "error -1:"


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "register_small.npz"), allow_pickle=False))
    for v in g.values():
        v.setflags(write=False)
    return g


@pytest.fixture(scope="module")
def dev(api, ctx, gold):
    s, d = api.Cloud(ctx, gold["src"]), api.Cloud(ctx, gold["dst"])
    yield s, d
    s.close()
    d.close()


@pytest.fixture(scope="module")
def packed(gold):
    return ref.pack(gold["src"], gold["dst"], gold["pairs"])


def check_transforms(T, hyp, where):
    """status-0 transforms within the Horn tolerance of the restatement's, the others sixteen NaNs"""
    ok = hyp["status"] == 0
    assert np.isnan(T[~ok]).all(), where
    if not ok.any():
        return 0.0
    tol_r, tol_t = ref.horn_tolerance(hyp["gap"][ok], hyp["norm"][ok], hyp["cs"][ok], hyp["ct"][ok])
    err_r = np.abs(T[ok][:, :3, :3] - hyp["T"][ok][:, :3, :3]).max(axis=(1, 2))
    err_t = np.abs(T[ok][:, :3, 3] - hyp["T"][ok][:, :3, 3]).max(axis=1)
    assert (err_r <= tol_r).all(), (where, float((err_r / tol_r).max()))
    assert (err_t <= tol_t).all(), (where, float((err_t / tol_t).max()))
    assert np.array_equal(T[ok][:, 3], np.broadcast_to([0.0, 0.0, 0.0, 1.0], (int(ok.sum()), 4))), where
    return float((err_r / tol_r).max())


# ------------------------------------------------------------------ 1. hypotheses
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_pair_hypotheses(dev, gold, packed, seed):
    src, dst = dev
    worst = 0.0
    for n_hyp in (1, 2, 63, 64, 65, 257, 4096, 65537):
        idx = ref.samples(seed, n_hyp, len(gold["pairs"]))
        for sim in (SIM, 0.0):
            samples, status, T = src.pair_hypotheses(dst, gold["pairs"], sim, n_hyp, seed)
            hyp = ref.hypotheses_from_samples(packed[0], packed[1], idx, sim)
            assert samples.dtype == np.int32 and np.array_equal(samples, idx), (n_hyp, sim)
            assert np.array_equal(status, hyp["status"]), (n_hyp, sim, np.flatnonzero(status != hyp["status"])[:5])
            worst = max(worst, check_transforms(T, hyp, (n_hyp, sim)))
    print("seed %d: largest |dR| / (64 eps |N| / gap) device against numpy: %.4f" % (seed, worst))
    if seed == SEED:
        samples, status, _ = src.pair_hypotheses(dst, gold["pairs"], SIM, H, SEED)
        assert np.array_equal(samples, gold["samples"]) and np.array_equal(status, gold["status"])


def test_hypotheses_of_planted_triangles(api, ctx):
    """degenerate and rejected by construction: collinear points, a non-finite point, an edge at 0.89 of its length"""
    s3 = np.array([[0, 0, 0], [4, 0, 0], [0, 2, 0]], np.float32)
    quarter = (s3.astype(np.float64) @ ref.rot_z(90).T + [8, -4, 0.5]).astype(np.float32)
    scaled = quarter.copy()
    scaled[1] = quarter[0] + np.float32(0.89) * (quarter[1] - quarter[0])
    pairs = np.stack([np.arange(3), np.arange(3)], axis=1).astype(np.int32)
    for tgt, sim, want in ((quarter, 1.0, 0), (scaled, 0.9, 2), (scaled, 0.85, 0), (scaled, 0.0, 0), (np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32), 0.0, 1),
                           (np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0]], np.float32), 0.0, 1)):
        a, b = api.Cloud(ctx, s3), api.Cloud(ctx, tgt)
        samples, status, T = a.pair_hypotheses(b, pairs, sim, 64, 5)
        hyp = ref.hypotheses_from_samples(s3, tgt, samples, sim)
        distinct = (samples[:, 0] != samples[:, 1]) & (samples[:, 0] != samples[:, 2]) & (samples[:, 1] != samples[:, 2])
        assert distinct.any() and np.array_equal(status, hyp["status"]) and (status[distinct] == want).all() and (status[~distinct] == 1).all(), (sim, want)
        check_transforms(T, hyp, (sim, want))
        if want == 0 and tgt is quarter:
            assert np.abs(T[distinct][:, :3, :3] - ref.rot_z(90)).max() < 1e-14 and np.abs(T[distinct][:, :3, 3] - [8, -4, 0.5]).max() < 1e-13
        a.close()
        b.close()


# ------------------------------------------------------------------ 2. scoring
@pytest.fixture(scope="module")
def bank(gold):
    """4096 float32 transforms round the true pose, with the truth, the identity, a NaN, a far one and duplicates planted; and the
    workhorse with non-finite points planted on both sides"""
    rng = np.random.default_rng(21)
    T = np.repeat(gold["T"][None], 4096, axis=0).copy()
    for k in range(6, 4096):
        T[k, :3, :3] = ref.rot_z(140.0 + rng.normal(0, 0.15))
        T[k, :3, 3] += rng.normal(0, 0.02, 3)
    T[1] = np.eye(4)
    T[2] = np.nan
    T[3, :3, 3] = 1.0e6
    T[5] = T[4] = T[100]
    T[4095] = T[0]
    Tf = ref.to_f32(T)
    Tf[7, 5] = np.inf
    src, dst = gold["src"].copy(), gold["dst"].copy()
    for k, (i, c, v) in enumerate(((0, 0, np.nan), (1, 2, np.inf), (64, 1, -np.inf), (1000, 0, np.nan), (2999, 2, np.nan))):
        (src if k % 2 == 0 else dst)[i, c] = v
    Tf.setflags(write=False)
    return Tf, src, dst


@pytest.fixture(scope="module")
def dev_bad(api, ctx, bank):
    s, d = api.Cloud(ctx, bank[1]), api.Cloud(ctx, bank[2])
    yield s, d
    s.close()
    d.close()


@pytest.mark.parametrize("m", [1, 2, 3, 63, 64, 65, 257, 1023, 1024, 1025, 3000])
def test_score_poses(api, dev_bad, bank, gold, m):
    Tf, src, dst = bank
    a, b = dev_bad
    pairs = gold["pairs"][:m] if m < 3000 else gold["pairs"]
    if m == 257:
        pairs = gold["pairs"][::-1][:m]                           # another subset: the last pairs, reversed
    s, t = ref.pack(src, dst, pairs)
    want = ref.score(s, t, Tf, THR)
    assert want[2] == 0 and want[3] == 0 and want[7] == 0 and want[4] == want[5] == want[100] and want[0] == want[4095]
    if m == 3000:
        assert want[0] > 700 and len(np.unique(want)) > 50       # the counts tell the transforms apart
    for n in (1, 2, 63, 64, 65, 257, 4096):
        got = a.score_poses(b, pairs, Tf[:n], THR)
        assert got.dtype == np.int64 and np.array_equal(got, want[:n]), (m, n, np.flatnonzero(got != want[:n])[:5])
        for max_blocks in (1, 3, 0):
            for chunk in (64, 1000, 0):
                got = api.hook_score_poses(a, b, pairs, Tf[:n], THR, max_blocks, chunk)
                assert np.array_equal(got, want[:n]), (m, n, max_blocks, chunk, np.flatnonzero(got != want[:n])[:5])


def test_score_poses_of_the_device_hypotheses(dev, gold, packed):
    """the transforms the device builds, rounded as the device rounds them, score as the rule says"""
    src, dst = dev
    _, status, T = src.pair_hypotheses(dst, gold["pairs"], SIM, H, SEED)
    Tf = ref.to_f32(T)
    want = ref.score(packed[0], packed[1], Tf, THR)
    assert np.array_equal(src.score_poses(dst, gold["pairs"], Tf, THR), want)
    assert (want[status != 0] == 0).all() and want.max() == gold["best_count"] and int(np.argmax(want)) == gold["best"]


# ------------------------------------------------------------------ 3. the whole call
def reference_from_device_hypotheses(src, dst, pairs, s, t, thr, sim, n_hyp, seed, top_k):
    """the choice and the top list by the rule, from the transforms sf_cloud_pair_hypotheses returned"""
    samples, status, T = src.pair_hypotheses(dst, pairs, sim, n_hyp, seed)
    counts = ref.score(s, t, ref.to_f32(T), thr)
    best, count, _ = ref.choose(counts)
    return dict(samples=samples, status=status, T=T, counts=counts, best=best, best_count=count, top=ref.top(counts, status, T, top_k))


def check_choice(r, want, where):
    st = r["stats"]
    assert (st["best"], st["best_count"]) == (want["best"], want["best_count"]), where
    assert (st["n_degenerate"], st["n_rejected"], st["n_scored"]) == tuple(int((want["status"] == k).sum()) for k in (1, 2, 0)), where
    assert [(c["h"], c["status"], c["count"]) for c in r["top"]] == [(c["h"], 0, c["count"]) for c in want["top"]] and st["n_top"] == len(want["top"]), where
    for c in r["top"]:
        assert c["T"].tobytes() == want["T"][c["h"]].tobytes(), (where, c["h"])


def check_final(r, s, t, thr, where):
    """the mask, n_inliers, fitness and rmse exactly, by the rule applied to the transform the device returned"""
    inl, n, fit, rmse = ref.final(s, t, r["T"], thr)
    assert np.array_equal(r["inlier"], inl) and r["stats"]["n_inliers"] == n, where
    assert r["stats"]["fitness"] == fit and r["stats"]["rmse"] == rmse, (where, r["stats"]["rmse"], rmse)


def test_register_workhorse(dev, gold, packed):
    src, dst = dev
    s, t = packed
    want = reference_from_device_hypotheses(src, dst, gold["pairs"], s, t, THR, SIM, H, SEED, 8)
    assert want["best"] == gold["best"] and want["best_count"] == gold["best_count"] and len(want["top"]) == 8
    r0 = src.register_pairs(dst, gold["pairs"], THR, SIM, H, 0, 3, 8, SEED)
    check_choice(r0, want, "rounds 0")
    assert r0["found"] == 1 and r0["stats"]["rounds_done"] == 0 and r0["stats"]["n_pairs"] == 3000
    assert r0["T"].tobytes() == want["T"][want["best"]].tobytes()   # refine_rounds = 0: bit-equal to the best hypothesis
    check_final(r0, s, t, THR, "rounds 0")
    s_ref, t_ref = (v[want["samples"][want["best"], 0]].astype(np.float64) for v in (s, t))
    prev = r0["T"]
    for rounds in (1, 2, 3):
        r = src.register_pairs(dst, gold["pairs"], THR, SIM, H, rounds, 3, 8, SEED)
        check_choice(r, want, rounds)
        assert r["stats"]["rounds_done"] == rounds and r["found"] == 1
        Tn, gap, norm, cs, ct = ref.refit_once(s, t, prev, THR, s_ref, t_ref)   # one round from the device's own previous transform: the same inliers
        tol_r, tol_t = ref.horn_tolerance(gap, norm, cs, ct)
        err_r, err_t = np.abs(r["T"][:3, :3] - Tn[:3, :3]).max(), np.abs(r["T"][:3, 3] - Tn[:3, 3]).max()
        print("refit round %d: |dR| %.3e (tolerance %.3e)  |dt| %.3e (tolerance %.3e)" % (rounds, err_r, tol_r, err_t, tol_t))
        assert err_r <= tol_r and err_t <= tol_t and np.array_equal(r["T"][3], [0, 0, 0, 1]), (rounds, err_r, tol_r, err_t, tol_t)
        check_final(r, s, t, THR, rounds)
        prev = r["T"]
    moved = gold["src"].astype(np.float64) @ r["T"][:3, :3].T + r["T"][:3, 3]
    truth = gold["src"].astype(np.float64) @ gold["T"][:3, :3].T + gold["T"][:3, 3]
    assert np.linalg.norm(moved - truth, axis=1).max() < THR and not (r["inlier"] & ~gold["truth"]).any()


def test_register_without_the_edge_check_and_with_many_hypotheses(dev, gold, packed):
    src, dst = dev
    s, t = packed
    for sim, n_hyp, seed, top_k in ((0.0, 4096, 2, 64), (SIM, 65537, 3, 5), (0.5, 257, 1, 1), (SIM, 1, 1, 3)):
        want = reference_from_device_hypotheses(src, dst, gold["pairs"], s, t, THR, sim, n_hyp, seed, top_k)
        r = src.register_pairs(dst, gold["pairs"], THR, sim, n_hyp, 2, 3, top_k, seed)
        check_choice(r, want, (sim, n_hyp))
        check_final(r, s, t, THR, (sim, n_hyp))
        assert r["found"] == int(want["best_count"] >= 3)
        if not r["found"]:
            assert np.array_equal(r["T"], np.eye(4)) and not r["inlier"].any() and r["stats"]["rounds_done"] == 0


def test_the_tie(api, ctx):
    """reg_ref_np.dyadic(): several hypotheses tie at the full true count, the smallest h wins (tests/test_reg_rule.py: h = 42)"""
    src, dst, pairs, truth, T = ref.dyadic()
    a, b = api.Cloud(ctx, src), api.Cloud(ctx, dst)
    s, t = ref.pack(src, dst, pairs)
    want = reference_from_device_hypotheses(a, b, pairs, s, t, THR, SIM, H, SEED, 8)
    tied = np.flatnonzero(want["counts"] == want["counts"].max())
    assert want["best"] == tied[0] == 42 and len(tied) >= 8 and want["best_count"] == truth.sum()
    r = a.register_pairs(b, pairs, THR, SIM, H, 2, 3, 8, SEED)
    check_choice(r, want, "tie")
    check_final(r, s, t, THR, "tie")
    assert [c["h"] for c in r["top"]] == tied[:8].tolist() and np.array_equal(r["inlier"], truth)
    assert np.abs(r["T"] - T).max() < 1e-12 and r["stats"]["rounds_done"] == 2
    a.close()
    b.close()


def test_three_calls_return_the_same_bits(dev, gold):
    src, dst = dev
    runs = [src.register_pairs(dst, gold["pairs"], THR, SIM, H, 2, 3, 8, SEED, profile=(k == 1)) for k in range(3)]
    timed = runs[1]["stats"]
    assert timed["hyp_ms"] > 0 and timed["score_ms"] > 0 and timed["refit_ms"] > 0
    assert runs[0]["stats"]["hyp_ms"] == runs[0]["stats"]["score_ms"] == runs[0]["stats"]["refit_ms"] == -1.0
    for r in runs[1:]:
        assert r["T"].tobytes() == runs[0]["T"].tobytes() and np.array_equal(r["inlier"], runs[0]["inlier"])
        assert [(c["h"], c["count"], c["T"].tobytes()) for c in r["top"]] == [(c["h"], c["count"], c["T"].tobytes()) for c in runs[0]["top"]]
        for key, v in runs[0]["stats"].items():
            if not key.endswith("_ms"):
                assert np.float64(r["stats"][key]).tobytes() == np.float64(v).tobytes(), key


def test_outcomes_that_are_not_errors(api, ctx, dev, gold):
    src, dst = dev
    r = src.register_pairs(dst, gold["pairs"], THR, SIM, H, 2, 2000, 4, SEED)       # min_inliers not reached
    assert r["found"] == 0 and np.array_equal(r["T"], np.eye(4)) and not r["inlier"].any() and len(r["inlier"]) == 3000
    st = r["stats"]
    assert (st["best"], st["best_count"], st["n_inliers"], st["rounds_done"], st["fitness"], st["rmse"]) == (gold["best"], gold["best_count"], 0, 0, 0.0, 0.0)
    assert len(r["top"]) == 4                                    # the candidates are listed all the same
    zero = dict(n_pairs=0, n_degenerate=0, n_rejected=0, n_scored=0, best=0, best_count=0, n_inliers=0, found=0, rounds_done=0, fitness=0.0, rmse=0.0, hyp_ms=-1.0,
                score_ms=-1.0, refit_ms=-1.0, n_top=0)
    for m in (0, 1, 2):
        r = src.register_pairs(dst, gold["pairs"][:m], THR, SIM, 64, 2, 3, 4, SEED)
        assert r["found"] == 0 and np.array_equal(r["T"], np.eye(4)) and r["inlier"].shape == (m,) and not r["inlier"].any() and r["top"] == [] and r["stats"] == zero
        samples, status, T = src.pair_hypotheses(dst, gold["pairs"][:m], SIM, 64, SEED)
        assert (samples == -1).all() and (status == 1).all() and np.isnan(T).all()
        Tf = ref.to_f32(np.stack([gold["T"], np.eye(4)]))
        assert np.array_equal(src.score_poses(dst, gold["pairs"][:m], Tf, THR), ref.score(*ref.pack(gold["src"], gold["dst"], gold["pairs"][:m]), Tf, THR))
    empty = api.Cloud(ctx, np.zeros((0, 3), np.float32))
    r = empty.register_pairs(dst, gold["pairs"], THR, SIM, 64, 2, 3, 0, SEED)      # an empty cloud: nothing is read, not even the indices
    assert r["found"] == 0 and r["stats"] == zero
    assert np.array_equal(src.score_poses(empty, gold["pairs"], np.zeros((2, 12), np.float32), THR), [0, 0])
    empty.close()
    line = (np.arange(300, dtype=np.float32)[:, None] * np.array([[1.0, 2.0, -0.5]], np.float32))
    a, b = api.Cloud(ctx, line), api.Cloud(ctx, line + np.float32(3.0))
    pairs = np.stack([np.arange(300), np.arange(300)], axis=1).astype(np.int32)
    r = a.register_pairs(b, pairs, THR, SIM, 257, 2, 3, 4, SEED)                   # collinear pairs: every hypothesis is degenerate
    assert r["found"] == 0 and r["stats"]["n_degenerate"] == 257 and r["stats"]["n_scored"] == 0 and r["stats"]["best"] == 0 and r["top"] == []
    assert np.array_equal(r["T"], np.eye(4)) and not r["inlier"].any()
    a.close()
    b.close()


def test_the_clouds_stay_as_they_are(api, ctx, gold):
    a, b = api.Cloud(ctx, gold["src"]), api.Cloud(ctx, gold["dst"])
    a.crop_aabb((-100, -100, -100), (100, 100, 0))               # leaves last indices behind
    b.crop_aabb((-100, -100, -100), (100, 100, 100))
    before = (a.download(), a.last_indices(), b.download(), b.last_indices())
    assert 0 < len(before[0]) < 3000 and len(before[3]) == 3000
    n = len(before[0])
    pairs = np.stack([np.arange(n), before[1]], axis=1).astype(np.int32)           # true pairs where the source survived
    r = a.register_pairs(b, pairs, THR, SIM, 1024, 2, 3, 4, SEED)
    a.pair_hypotheses(b, pairs, SIM, 64, SEED)
    a.score_poses(b, pairs, ref.to_f32(r["T"][None]), THR)
    after = (a.download(), a.last_indices(), b.download(), b.last_indices())
    for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes()
    assert r["stats"]["n_pairs"] == n
    a.close()
    b.close()


def test_refusals_touch_nothing(api, ctx, dev, gold):
    src, dst = dev
    pairs = gold["pairs"]
    good = dict(distance_threshold=THR, edge_similarity=SIM, num_hypotheses=64, refine_rounds=2, min_inliers=3, top_k=2, seed=SEED)
    for change in (dict(num_hypotheses=0), dict(num_hypotheses=(1 << 20) + 1), dict(refine_rounds=-1), dict(refine_rounds=9), dict(min_inliers=2), dict(top_k=-1),
                   dict(top_k=65), dict(distance_threshold=0.0), dict(distance_threshold=-1.0), dict(distance_threshold=np.nan), dict(distance_threshold=np.inf),
                   dict(edge_similarity=1.5), dict(edge_similarity=np.nan)):
        with pytest.raises(api.SlamFusionError, match=INVALID):
            src.register_pairs(dst, pairs, **{**good, **change})
    for bad in ((0, -1), (5, 3000), (3000, 0), (-1, 0)):          # an index outside its cloud, in the first or a later pair
        for at in (0, 2999):
            p = pairs.copy()
            p[at] = bad
            for call in (lambda: src.register_pairs(dst, p, **good), lambda: src.pair_hypotheses(dst, p, SIM, 64, SEED),
                         lambda: src.score_poses(dst, p, np.zeros((2, 12), np.float32), THR), lambda: src.register_pairs(dst, p[max(at - 1, 0):][:2], **good)):
                with pytest.raises(api.SlamFusionError, match="outside its cloud"):
                    call()
    for thr in (0.0, np.nan):
        with pytest.raises(api.SlamFusionError, match=INVALID):
            src.score_poses(dst, pairs, np.zeros((2, 12), np.float32), thr)
    for n in (0, (1 << 20) + 1):
        with pytest.raises(api.SlamFusionError, match=INVALID):
            src.score_poses(dst, pairs, np.zeros((n, 12), np.float32), THR)
    for max_blocks, chunk in ((-1, 0), (65537, 0), (0, -1)):
        with pytest.raises(api.SlamFusionError, match=INVALID):
            api.hook_score_poses(src, dst, pairs, np.zeros((2, 12), np.float32), THR, max_blocks, chunk)
    other = api.Context(0)
    far = api.Cloud(other, gold["dst"])
    with pytest.raises(api.SlamFusionError, match="different contexts"):
        src.register_pairs(far, pairs, **good)
    far.close()
    other.close()
    # through the ABI: the outputs of a refused call are as they went in
    lib = api.load_library()
    p = api._reg_params(THR, SIM, 64, 2, 3, 2, SEED, False)
    T, inl, st = np.full(16, 7.0), np.full(3000, 9, np.uint8), api.RegStats()
    top = (api.RegCandidate * 2)()
    st.n_pairs = top[0].h = -7
    p2 = pairs.copy()
    p2[1234] = (0, 3000)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.sf_cloud_register_pairs(src.h, dst.h, ptr(p2), ctypes.c_int64(3000), ctypes.byref(p), ptr(T), ptr(inl), top, ctypes.byref(st)) == -1
    assert lib.sf_cloud_register_pairs(src.h, dst.h, ptr(p2), ctypes.c_int64(1 << 31), ctypes.byref(p), ptr(T), ptr(inl), top, ctypes.byref(st)) == -1
    assert lib.sf_cloud_register_pairs(src.h, dst.h, ptr(p2), ctypes.c_int64(-1), ctypes.byref(p), ptr(T), ptr(inl), top, ctypes.byref(st)) == -1
    assert (T == 7.0).all() and (inl == 9).all() and st.n_pairs == -7 and top[0].h == -7
    assert np.array_equal(src.download(), gold["src"]) and np.array_equal(dst.download(), gold["dst"])
