"""The NDT line search, the score pass and the coarse-to-fine levels on the device (sf_ndt_set_line_search, sf_ndt_scores,
sf_ndt_line_search_read, sf_ndt_align_levels; csrc/sf_ndt.hip) against the numpy restatement tests/ndt_ls_ref_np.py, on the fixtures whose
conditions tests/test_ndt_ls_rule.py holds.  As in tests/test_gpu_ndt.py the per-row comparisons hand the restatement the device's
downloaded voxels; whole alignments are compared with the restatement run on its own voxels."""
import ctypes

import numpy as np
import pytest

import ndt_ls_ref_np as ls
import ndt_ref_np as nr

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 2000)                   # wave and workgroup edges
WORST = dict(score=0.0, phi0=0.0, delta=0.0, slope=0.0, phi=0.0, step=0.0, final=0.0)
ARMIJO, STEP_MAX, TRIALS = ls.LS_DEFAULTS["armijo"], ls.LS_DEFAULTS["step_max"], ls.LS_DEFAULTS["trials"]


@pytest.fixture(scope="module")
def ndts(api, ctx):
    """Ndt objects by (target name, resolution, neighbours, searched), built once; searched ones have the default line search on"""
    made, clouds = {}, {}

    def cloud(target):
        if target not in clouds:
            pts = dict(room=nr.room_target, terrain=nr.terrain_target)[target]()
            clouds[target] = (api.Cloud(ctx, pts), pts)
        return clouds[target]

    def get(target, resolution, neighbours=7, searched=False):
        key = (target, float(resolution), int(neighbours), bool(searched))
        if key not in made:
            made[key] = api.Ndt(ctx, cloud(target)[0], resolution, neighbours=neighbours)
            if searched:
                made[key].set_line_search()
        return made[key]

    get.points = lambda target: cloud(target)[1]
    get.cloud = lambda target: cloud(target)[0]
    yield get
    for n in made.values():
        n.close()


def _same_bits(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].tobytes() == b[k].tobytes(), k
        else:
            assert a[k] == b[k], k


def _case(name):
    """-> (target, resolution, start, the restatement's searched alignment)"""
    if name in ls.STALL:
        tgt, res, start = ls.STALL[name]
        return tgt, res, start, ls.reference_stall(name)
    tgt, start, _ = nr.CASES[name]
    return tgt, nr.ALIGN_RES[tgt], start, ls.reference_ls(name)


def _some_poses(k, seed):
    """k poses within 0.5 m / 5 degrees of the identity"""
    rng = np.random.default_rng(seed)
    return np.array([nr.pose(rng.uniform(-0.5, 0.5, 3), rng.uniform(-5.0, 5.0, 3)) for _ in range(k)])


def _compare_scores(ndt, mdl, src, poses, neighbours):
    score, terms = ndt.scores(src, poses)
    dev = ndt.derivatives(src, poses)
    assert score.shape == terms.shape == (len(poses),) and score.dtype == np.float64 and terms.dtype == np.int64
    for i, T in enumerate(poses):
        assert np.float64(dev[i]["score"]).tobytes() == score[i].tobytes() and dev[i]["n_terms"] == terms[i], i
    for i in range(min(len(poses), 3)):
        ev = nr.evaluate(mdl, src, poses[i], neighbours, derivs=False)
        assert ev["n_terms"] == terms[i]
        if ev["n_terms"]:
            ratio = abs(score[i] - ev["score"]) / nr.deriv_bound(ev)[0]
            WORST["score"] = max(WORST["score"], float(ratio))
            assert ratio <= 1.0, ratio
        else:
            assert score[i] == 0.0
    return score, terms


@pytest.mark.parametrize("neighbours", [1, 7])
@pytest.mark.parametrize("n", SIZES)
def test_scores_are_the_scores_of_the_derivatives(ndts, n, neighbours):
    ndt = ndts("room", nr.ALIGN_RES["room"], neighbours)
    mdl = nr.model(ndts.points("room"), nr.ALIGN_RES["room"], vox=ndt.voxels())
    src = nr.room_source()[:n]
    score, terms = _compare_scores(ndt, mdl, src, np.array(nr.EVAL_POSES), neighbours)
    assert n < 255 or terms[0] > n // 2                        # (the comparison is not one of zeros)


@pytest.mark.parametrize("k", [1, 8, 16, 17, 65, 1025])
def test_scores_of_k_poses(ndts, k):
    """(a launch of this library takes up to 1024 poses; sf_ndt_derivatives takes 64)"""
    ndt = ndts("room", nr.ALIGN_RES["room"])
    mdl = nr.model(ndts.points("room"), nr.ALIGN_RES["room"], vox=ndt.voxels())
    score, terms = _compare_scores(ndt, mdl, nr.room_source()[:257], _some_poses(k, 2510 + k), 7)
    assert (terms > 0).all() and len(set(score.tolist())) == k


def test_scores_of_no_pose_and_of_poses_outside_the_grid(ndts):
    ndt, src = ndts("room", nr.ALIGN_RES["room"]), nr.room_source()[:257]
    score, terms = ndt.scores(src, np.zeros((0, 4, 4)))
    assert len(score) == 0 and len(terms) == 0
    poses = [nr.pose(t, (0, 0, 0)) for t in ((9.5, 0, 0), (0, -9.5, 0), (0, 0, 9.5))] + [np.eye(4)]   # the room spans 8 x 8 x 4 m
    score, terms = ndt.scores(src, np.array(poses))
    assert not score[:3].any() and not terms[:3].any() and score[3] < 0.0 and terms[3] > 0


def test_the_search_switched_on_and_off_again(api, ctx, ndts):
    tgt, res, start, _ = _case("room_near")
    src, never = nr.source_of(tgt), ndts(tgt, res)
    ndt = api.Ndt(ctx, ndts.cloud(tgt), res)
    before = ndt.align(src, start, trace=True)
    on = ndt.set_line_search().align(src, start, trace=True)
    assert on["iterations"] != before["iterations"] and on["T64"].tobytes() != before["T64"].tobytes()
    after = ndt.set_line_search(trials=0).align(src, start, trace=True)
    _same_bits(before, after)
    _same_bits(never.align(src, start, trace=True), after)
    _same_bits(ndts(tgt, res, searched=True).align(src, start, trace=True), on)
    ndt.close()


@pytest.mark.parametrize("case", ["room_near", "room_far", "terrain_negative", "room_coarse_stall"])
def test_every_row_replayed_from_the_devices_own_numbers(api, ndts, case):
    """Whatever the margins: the choice is re-made from the device's phi0, slope, alpha_max, phi and n_terms (comparisons and IEEE
    products only: exact), and every number of a row is within its bound of the restatement evaluated at the device's pose."""
    tgt, res, start, _ = _case(case)
    ndt, src = ndts(tgt, res, searched=True), nr.source_of(tgt)
    mdl = nr.model(ndts.points(tgt), res, vox=ndt.voxels())
    dev = ndt.align(src, start, trace=True)
    rows, tr = ndt.line_search_rows(), dev["trace"]
    stalled = bool(dev["flags"] & api.SF_NDT_FLAG_LINE_SEARCH_STALLED)
    assert len(rows) == dev["iterations"] + int(stalled) and len(tr) == dev["iterations"] + 1 and len(rows) >= 5
    assert stalled == (case == "room_coarse_stall") and tr[-1].tobytes() == dev["T64"].tobytes()
    for i, row in enumerate(rows):
        T = tr[i]
        assert row["trials"] == TRIALS and len(row["phi"]) == TRIALS
        assert row["chosen"] == ls.pick(row["phi0"], row["slope"], row["alpha_max"], row["phi"], row["n_terms"], ARMIJO), i
        assert (row["chosen"] < 0) == (stalled and i == len(rows) - 1)
        ev = nr.evaluate(mdl, src, T, 7)
        st = ls.direction(ev)
        bd, br, bs = ls.direction_bound(ev, st, T)
        ratios = dict(phi0=abs(row["phi0"] - ev["score"]) / nr.deriv_bound(ev)[0], delta=np.abs(row["delta"] - st["delta"]).max() / bd,
                      slope=abs(row["slope"] - ls.slope_of(ev["gradient"], st["delta"])) / bs)
        assert abs(row["raw_length"] - st["raw_length"]) <= br
        amax = ls.step_range(st, STEP_MAX)
        assert abs(row["alpha_max"] - amax) <= amax * (br / st["raw_length"] + 4.0 * nr.U) and 0.0 < row["alpha_max"] <= 1.0
        for k in range(TRIALS):
            e = nr.evaluate(mdl, src, nr.vec6_to_mat4(float(np.ldexp(row["alpha_max"], -k)) * row["delta"]) @ T, 7, derivs=False)
            assert e["n_terms"] == row["n_terms"][k] and e["face_gap"] >= 1e-9 * res
            ratios["phi"] = max(ratios.get("phi", 0.0), abs(row["phi"][k] - e["score"]) / nr.deriv_bound(e)[0])
        if row["chosen"] >= 0:
            ref_next = nr.vec6_to_mat4(float(np.ldexp(amax, -row["chosen"])) * st["delta"]) @ T
            ratios["step"] = np.abs(ref_next - tr[i + 1]).max() / ls.trial_step_bound(ev, st, T, amax)
        for name, r in ratios.items():
            WORST[name] = max(WORST[name], float(r))
        print("%s row %d: chosen %d, error / bound %s" % (case, i, row["chosen"], {k: "%.3g" % v for k, v in ratios.items()}))
        assert all(r <= 1.0 for r in ratios.values()), (i, ratios)


@pytest.mark.parametrize("case", ["room_near", "terrain_near", "room_coarse_stall"])
def test_alignment_with_the_search(ndts, case):
    tgt, res, start, ref = _case(case)
    ndt, src = ndts(tgt, res, searched=True), nr.source_of(tgt)
    dev = ndt.align(src, start)
    chosen = [row["chosen"] for row in ndt.line_search_rows()]
    for k in ("iterations", "converged", "modified", "flags", "n_inside", "n_terms"):
        assert dev[k] == ref[k], (k, dev[k], ref[k])
    assert chosen == ref["chosen"]
    assert all(np.isfinite(dev[k]).all() for k in ("T64", "score", "gradient", "hessian"))
    amax = [ls.step_range(st, STEP_MAX) for st in ref["steps"]]
    bound = sum(ls.trial_step_bound(ev, st, T, a) for ev, st, T, a in zip(ref["evaluations"], ref["steps"], ref["trace"], amax))
    diff = float(np.abs(dev["T64"] - ref["T64"]).max())
    WORST["final"] = max(WORST["final"], diff / bound)
    print("%s: %d iterations, chosen %s, |T_device - T_restatement| %.3g, the sum of the step bounds %.3g" % (case, dev["iterations"], chosen, diff, bound))
    assert diff <= bound


def test_alignment_without_overlap(api, ndts):
    tgt, start, _ = nr.CASES["room_outside"]
    dev = ndts(tgt, nr.ALIGN_RES[tgt], searched=True).align(nr.source_of(tgt), start)
    assert dev["iterations"] == 0 and dev["flags"] == api.SF_NDT_FLAG_NO_OVERLAP and not dev["converged"] and dev["T64"].tobytes() == np.asarray(start).tobytes()
    assert dev["score"] == 0.0 and not dev["gradient"].any() and not dev["hessian"].any() and dev["n_terms"] == 0
    assert ndts(tgt, nr.ALIGN_RES[tgt], searched=True).line_search_rows() == []


@pytest.mark.parametrize("batch", [1, 3])
def test_align_batch_entry_b_is_the_single_alignment(ndts, batch):
    ndt, src = ndts("room", nr.ALIGN_RES["room"], searched=True), nr.source_of("room")
    scans = np.stack([src[600 * b:600 * (b + 1)] for b in range(batch)])
    starts = [nr.CASES["room_near"][1], nr.CASES["room_far"][1], nr.EVAL_POSES[1]][:batch]
    out = ndt.align_batch(scans, np.array(starts))
    assert len(out) == batch
    for b in range(batch):
        _same_bits(out[b], ndt.align(scans[b], starts[b]))
    assert batch == 1 or len({o["iterations"] for o in out}) > 1   # (the restatement takes 11, 16 and 12 iterations: entries end while others go on)


def test_align_batch_with_an_entry_that_stalls(api, ndts):
    """the room at 2 m, one scan three times: entry 0 stalls after 5 steps, entry 1 converges after 8, entry 2 goes on"""
    tgt, res, start, _ = _case("room_coarse_stall")
    ndt, src = ndts(tgt, res, searched=True), nr.source_of(tgt)
    starts = [start, nr.CASES["room_near"][1], nr.EVAL_POSES[1]]
    out = ndt.align_batch(np.stack([src, src, src]), np.array(starts))
    for b in range(3):
        _same_bits(out[b], ndt.align(src, starts[b]))
    assert out[0]["flags"] == api.SF_NDT_FLAG_LINE_SEARCH_STALLED and not out[0]["converged"] and out[0]["iterations"] == 5
    assert out[1]["flags"] == 0 and out[1]["converged"] and out[1]["iterations"] == 8 and out[2]["iterations"] > 8


@pytest.mark.parametrize("case", ["room_wide", "terrain_wide"])
def test_levels(api, ctx, ndts, synth, case):
    tgt, start = ls.WIDE[case]
    src = nr.source_of(tgt)
    pyr = api.NdtPyramid(ctx, ndts.cloud(tgt), ls.LEVELS[tgt])
    assert [lv.params.resolution for lv in pyr.levels] == list(ls.LEVELS[tgt])
    got = pyr.align(src, start)
    T, by_hand = start, []
    for lv in pyr.levels:                                      # the chain done by hand
        by_hand.append(lv.align(src, T))
        T = by_hand[-1]["T64"]
    assert len(got["per_level"]) == len(by_hand)
    for a, b in zip(got["per_level"], by_hand):
        _same_bits(a, b)
    _same_bits({k: v for k, v in got.items() if k != "per_level"}, by_hand[-1])
    two = pyr.align_batch(np.stack([src, src]), np.array([start, nr.CASES["room_near"][1]]))      # a batch: entry 0 is the same alignment
    _same_bits({k: v for k, v in two[0].items() if k != "per_level"}, by_hand[-1])
    assert two[1]["T64"].tobytes() != two[0]["T64"].tobytes() and len(two[1]["per_level"]) == len(by_hand)
    plain = ndts(tgt, 1.0).align(src, start)
    e_pyr, e_plain = synth.pose_error(got["T64"], np.eye(4))[0], synth.pose_error(plain["T64"], np.eye(4))[0]
    print("%s: plain at 1 m ends %.3g m from the truth, levels %s with the search %.3g m; per level (iterations, flags) %s"
          % (case, e_plain, ls.LEVELS[tgt], e_pyr, [(p["iterations"], p["flags"]) for p in got["per_level"]]))
    assert e_pyr < 0.05 and e_plain > 0.5
    pyr.close()


def test_refusals_that_need_a_handle(api, ctx, ndts):
    lib = api.load_library()
    cloud, src = ndts.cloud("room"), nr.room_source()
    ndt = api.Ndt(ctx, cloud, 2.0)
    n, res, pose = ctypes.c_int64(-7), (api.NdtResult * 2)(), np.eye(4).reshape(16)
    p_pose = pose.ctypes.data_as(ctypes.c_void_p)
    assert lib.sf_ndt_line_search_read(ndt.h, None, ctypes.c_int64(0), ctypes.byref(n)) == -4 and n.value == -7      # SF_ERR_STATE: no alignment yet
    score, terms = np.zeros(1), np.zeros(1, np.int64)
    assert lib.sf_ndt_scores(ndt.h, p_pose, ctypes.c_int64(1), score.ctypes.data_as(ctypes.c_void_p), terms.ctypes.data_as(ctypes.c_void_p)) == -1   # no source yet
    assert b"bad arguments" in lib.sf_last_error()
    ndt.align(src[:300])
    assert lib.sf_ndt_line_search_read(ndt.h, None, ctypes.c_int64(0), ctypes.byref(n)) == -4                         # an alignment without the search
    ndt.set_line_search().align(src[:300], nr.CASES["room_near"][1])
    assert lib.sf_ndt_line_search_read(ndt.h, None, ctypes.c_int64(0), ctypes.byref(n)) == 0 and n.value >= 1
    row = api.NdtLsRow()
    if n.value > 1:
        assert lib.sf_ndt_line_search_read(ndt.h, ctypes.byref(row), ctypes.c_int64(1), None) == -1 and b"bad arguments" in lib.sf_last_error()
    with pytest.raises(api.SlamFusionError):
        ndt.set_line_search(trials=17)
    # levels that do not go together
    other_size, other_batch, no_source, no_target = api.Ndt(ctx, cloud, 1.0), api.Ndt(ctx, cloud, 1.0), api.Ndt(ctx, cloud, 1.0), api.Ndt(ctx, None, 1.0)
    other_size._set_source(src[:299])
    other_batch._set_source(np.stack([src[:300], src[300:600]]))
    no_target._set_source(src[:300])
    ctx2 = api.Context(0)
    elsewhere = api.Ndt(ctx2, api.Cloud(ctx2, nr.room_target()[:2000]), 1.0)
    elsewhere._set_source(src[:300])
    for bad in (other_size, other_batch, no_source, no_target, elsewhere):
        for pair in ((ndt, bad), (bad, ndt)):
            levels = (ctypes.c_void_p * 2)(pair[0].h.value, pair[1].h.value)
            assert lib.sf_ndt_align_levels(levels, 2, p_pose, res, None) == -1 and b"bad arguments" in lib.sf_last_error()
    levels = (ctypes.c_void_p * 2)(ndt.h.value, ndt.h.value)
    assert lib.sf_ndt_align_levels(levels, 2, p_pose, res, None) == 0                                                  # the same level twice goes together
    for o in (other_size, other_batch, no_source, no_target, elsewhere, ndt):
        o.close()
    ctx2.close()


def test_zz_report_the_largest_error_over_bound_of_the_session():
    """(runs last in this file) the largest error / bound over everything above: DESIGN section 25 records these"""
    print("NDT line search largest error / bound: scores %.3g, phi0 %.3g, direction %.3g, slope %.3g, trial scores %.3g, accepted pose %.3g, "
          "final pose against the summed step bounds %.3g" % tuple(WORST[k] for k in ("score", "phi0", "delta", "slope", "phi", "step", "final")))
    assert max(WORST.values()) <= 1.0
