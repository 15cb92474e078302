"""The brute-force start-up alignment (sf_bf.hip: k_bf_score<false / true>, k_bf_finish, the host walk of sf_bf_align_clouds) at its
edges.  Every case runs against the oracle's bf_align bit for bit -- found, index, candidate count, every score the reference
computed, the returned pose, the pose a second call starts from after a miss -- and against the float64 restatement of
tests/bf_ref_np.py within the bound derived there (tests/test_bf_rule.py holds the oracle itself to it on the CPU).  The cases are
bf_ref_np's table: source sizes around the 64-lane groups of k_bf_finish and the 256-thread block of k_bf_score, index cells of
0.1 / 0.25 / 1.0 / automatic, targets of one and two points, coplanar and full of duplicates, a general pose 1 km out, a scan that
lies wholly outside the target's box and candidates 1.5 m apart (ring after ring in the cooperative search), windows, non-finite
source points, and everything sf_bf_align_clouds refuses."""
import ctypes as C

import numpy as np
import pytest

import bf_ref_np as ref

pytestmark = pytest.mark.gpu

SF_ERR_INVALID, SF_ERR_STATE = -1, -4


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def configure(bf, prm):
    bf.setMeanErrorThreshold(prm["threshold"])
    bf.setXYZStep(prm["x_step"], prm["y_step"], prm["z_step"])
    bf.setXYZRange(prm["x_range"], prm["y_range"], prm["z_range"])
    bf.setRotationStep(prm["yaw_step"])
    bf.setRotationRange(prm["yaw_range"])


def build_target(api, ctx, c):
    """The case's target as the device searches it: a Map of the case's cell with the case's window, or the bare array (automatic cell)."""
    if c["cell"] is None:
        return c["tgt"]
    mp = api.Map(ctx, api.Cloud(ctx, c["tgt"]), c["cell"])
    if c["window"] is not None:
        getattr(mp, "window_" + c["window"][0])(*c["window"][1:])
    return mp


def fresh(api, ctx, name, threshold, prev=None, target=None):
    c = ref.case(name)
    bf = api.BruteForceAlignment(ctx)
    configure(bf, ref.params(name, threshold))
    bf.setInitialGuess(c["prev"] if prev is None else prev)                        # the handle starts at the identity: accepted
    bf.setSourceCloud(c["src"])
    bf.setTargetCloud(build_target(api, ctx, c) if target is None else target)
    return bf


def align_and_compare(bf, o, r=None):
    """One alignClouds against the oracle's answer `o`, bit for bit, and against bf_ref's `r`."""
    locked = bf.firstAlignmentCompleted()
    found = bf.alignClouds()
    res = bf.last_result()
    assert (found, res["index"], res["n_candidates"]) == (o["found"], o["index"], o["n_candidates"])
    assert bf.firstAlignmentCompleted() == (locked or o["found"])                  # a hit sets the flag, a miss leaves it
    bf.resetFirstAlignment(found)                                                  # getBestTransformation: best once locked, else previous
    T = bf.getBestTransformation()
    bf.resetFirstAlignment(locked or found)
    done = np.isfinite(o["scores"])                                                # the only mask: what the reference left unscored at its exit
    assert done[:o["index"] + 1].all() and np.isfinite(res["scores"][done]).all() and np.isnan(res["scores"][~done]).all()
    assert np.array_equal(bits(res["scores"][done]), bits(o["scores"][done]))
    assert np.array_equal(bits(res["score"]), bits(o["best_score"]))
    assert np.array_equal(bits(T), bits(o["best_T"]))
    if r is not None:
        ref.check(r, found, res["index"], res["n_candidates"], res["scores"], T)
    return res, T


@pytest.fixture(scope="module")
def oracle_of(orc):
    """The oracle's answers, computed once per (case, threshold, starting pose)."""
    memo = {}

    def get(name, threshold, prev=None):
        c = ref.case(name)
        p = np.asarray(c["prev"] if prev is None else prev, np.float32)
        key = (name, threshold, p.tobytes())
        if key not in memo:
            memo[key] = orc.bf_align(c["src"], ref.target_of(name), p, **ref.params(name, threshold))
        return memo[key]
    return get


@pytest.mark.parametrize("name,threshold", ref.RUNS, ids=["%s-%g" % r for r in ref.RUNS])
def test_case_matches_oracle_and_rule(api, ctx, oracle_of, name, threshold):
    bf = fresh(api, ctx, name, threshold)
    assert not bf.firstAlignmentCompleted()
    o = oracle_of(name, threshold)
    align_and_compare(bf, o, ref.run(name, threshold))
    if not o["found"]:                                                             # previous <- best: the next call starts there
        assert np.array_equal(bits(bf.getBestTransformation()), bits(o["prev_T_after"]))
        align_and_compare(bf, oracle_of(name, threshold, o["prev_T_after"]))
    bf.close()


def test_ties_first_of_equal_scores_wins(api, ctx):
    """{-0, +0}^4: sixteen poses that differ in the sign of a zero.  Equal scores, candidate 0 on a miss and on a hit."""
    for threshold in (ref.MISS, 1.0e3):
        bf = fresh(api, ctx, "ties", threshold)
        found = bf.alignClouds()
        res = bf.last_result()
        assert res["n_candidates"] == 16 and res["index"] == 0 and found == (threshold != ref.MISS)
        if found:
            assert np.isfinite(res["scores"][0]) and np.isnan(res["scores"][1:]).all()   # the walk ends at the hit
        else:
            assert np.isfinite(res["scores"][0]) and (bits(res["scores"]) == bits(res["scores"])[0]).all()
        bf.close()


def test_shrinking_source_and_changing_grid_on_one_handle(api, ctx, oracle_of):
    """1 500 points, then 65 (src is not shrunk, X / Y / Z move to the new n), then more candidates (poses, partials, scores
    grow) and back: every call equals the oracle's and a fresh handle's."""
    mp = build_target(api, ctx, ref.case("n1500"))
    bf = fresh(api, ctx, "n1500", ref.HIT, target=mp)
    steps = [("n1500", ref.HIT), ("n65", ref.HIT), ("n65_g128", ref.MISS), ("n65", ref.HIT), ("n1500", ref.MISS), ("n65", ref.MISS)]
    prev = ref.case("n1500")["prev"]
    for name, threshold in steps:
        configure(bf, ref.params(name, threshold))
        bf.setSourceCloud(ref.case(name)["src"])
        o = oracle_of(name, threshold, prev)
        res, T = align_and_compare(bf, o, ref.run(name, threshold) if np.array_equal(prev, ref.case(name)["prev"]) else None)
        other = fresh(api, ctx, name, threshold, prev=prev, target=mp)
        assert other.alignClouds() == o["found"]
        assert np.array_equal(bits(other.last_result()["scores"]), bits(res["scores"]))
        assert np.array_equal(bits(other.getBestTransformation()), bits(T))
        other.close()
        prev = o["prev_T_after"]                                                   # unchanged by a hit
    bf.close()


def test_windows_on_one_handle_then_none(api, ctx, orc, oracle_of):
    """A sphere and an oriented box on one map, one handle: each equals the oracle on the points the window keeps (bf_ref_np's
    predicates, which test_bf_rule holds to the oracle's crops); window_none() then equals the run on the whole map."""
    c = ref.case("sphere")
    mp = api.Map(ctx, api.Cloud(ctx, c["tgt"]), c["cell"])
    bf = fresh(api, ctx, "sphere", ref.HIT, target=mp)
    for name in ("sphere", "obb", "single"):
        w = ref.case(name)["window"]
        getattr(mp, "window_" + w[0])(*w[1:])
        assert mp.window_count() == len(ref.target_of(name))
        threshold = 1.0e3 if name == "single" else ref.HIT                         # hits: the starting pose stays
        configure(bf, ref.params(name, threshold))
        bf.setSourceCloud(ref.case(name)["src"])
        align_and_compare(bf, oracle_of(name, threshold), ref.run(name, threshold))
    mp.window_none()
    for name in ("sphere", "single"):                                              # the same scans against everything
        cc = ref.case(name)
        configure(bf, ref.params(name, ref.HIT))
        bf.setSourceCloud(cc["src"])
        o = orc.bf_align(cc["src"], cc["tgt"], cc["prev"], **ref.params(name, ref.HIT))
        align_and_compare(bf, o, ref.bf_ref(cc["src"], cc["tgt"], cc["prev"], ref.params(name, ref.HIT)))
        assert o["found"]
    bf.close()


@pytest.mark.parametrize("threshold", (ref.HIT, ref.MISS))
def test_nonfinite_source_points_add_zero_and_still_divide(api, ctx, threshold):
    """NaN / Inf source points: zero contribution, divisor n (k_bf_score's header).  The reference is undefined there, so the
    yardstick is bf_ref_np's rule alone."""
    bf = fresh(api, ctx, "nonfinite", threshold)
    found = bf.alignClouds()
    res = bf.last_result()
    r = ref.run("nonfinite", threshold)
    assert r["found"] == (threshold == ref.HIT)
    ref.check(r, found, res["index"], res["n_candidates"], res["scores"], bf.getBestTransformation())
    bf.close()


def test_two_runs_give_equal_bits(api, ctx):
    for name, threshold in (("far", ref.MISS), ("outside", ref.MISS), ("sphere", ref.MISS)):
        out = []
        for _ in range(2):
            bf = fresh(api, ctx, name, threshold)
            bf.alignClouds()
            out.append((bits(bf.last_result()["scores"]).copy(), bits(bf.getBestTransformation()).copy(), bf.last_result()["index"]))
            bf.close()
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


# ------------------------------------------------------------------ refusals
def state(bf):
    """previous, best, first_alignment_completed, last_index, last_score, last_scores, as bytes."""
    done = bf.firstAlignmentCompleted()
    bf.resetFirstAlignment(False)
    previous = bf.getBestTransformation().tobytes()
    bf.resetFirstAlignment(True)
    best = bf.getBestTransformation().tobytes()
    bf.resetFirstAlignment(done)
    res = bf.last_result()
    return done, previous, best, res["index"], np.float32(res["score"]).tobytes(), res["n_candidates"], res["scores"].tobytes()


def refused(bf, code):
    before = state(bf)
    found = C.c_int(-7)
    rc = bf.lib.sf_bf_align_clouds(bf.h, C.byref(found))
    assert rc == code, (rc, code)
    assert state(bf) == before
    with pytest.raises(Exception):
        bf.alignClouds()


BAD_GRIDS = {
    "x step 0": dict(x_step=0.0), "y step 0": dict(y_step=0.0), "z step 0": dict(z_step=0.0), "yaw step 0": dict(yaw_step=0.0),
    "x step -0": dict(x_step=-0.0), "x step < 0": dict(x_step=-0.1), "yaw step < 0": dict(yaw_step=-0.1),
    "x step nan": dict(x_step=np.nan), "z step nan": dict(z_step=np.nan), "y step inf": dict(y_step=np.inf), "yaw step inf": dict(yaw_step=np.inf),
    "x step tiny": dict(x_step=1.0e-45, x_range=1.0),                           # range / (2 step) overflows to +inf
    "x range < 0": dict(x_range=-0.1), "yaw range < 0": dict(yaw_range=-1.0), "y range nan": dict(y_range=np.nan), "z range inf": dict(z_range=np.inf),
    "x range -inf": dict(x_range=-np.inf),
    "long sequence": dict(x_range=1000.0, x_step=0.1),                          # 10 002 entries
    "long yaw sequence": dict(yaw_range=2048.0, yaw_step=0.5),                  # 4 098: one i past the cap
    "total over the cap": dict(x_range=2047.0, x_step=0.5, yaw_range=32.0, yaw_step=0.5),   # 4 096 x 2 x 2 x 66
    "slice over 65 535": dict(y_range=4.1, z_range=4.1, yaw_range=4.1),         # 2 x 44 x 44 x 44
}


def test_bad_grid_table_is_what_it_claims():
    """The lengths the table's comments state, from the rule (no device): which check each entry meets."""
    def lens(d):
        p = dict(ref.G32, **d)
        return [ref.sequence_length(p[a + "_range"], p[a + "_step"]) for a in ("x", "y", "z", "yaw")]
    assert lens(BAD_GRIDS["long sequence"])[0] == 10002 and lens(BAD_GRIDS["long yaw sequence"])[3] == 4098
    l = lens(BAD_GRIDS["total over the cap"])
    assert l == [4096, 2, 2, 66] and np.prod(l) > 2 ** 20 and np.prod(l[1:]) <= 65535
    l = lens(BAD_GRIDS["slice over 65 535"])
    assert l == [4, 44, 44, 44] and np.prod(l) <= 2 ** 20 and np.prod(l[1:]) > 65535
    assert lens(dict(x_range=2047.0, x_step=0.5))[0] == 4096                      # the longest sequence that is accepted


@pytest.mark.parametrize("history", ("fresh", "after a miss", "after a hit"))
def test_refusals_leave_the_state_alone(api, ctx, oracle_of, history):
    c = ref.case("n65")
    mp = build_target(api, ctx, c)
    threshold = ref.HIT if history == "after a hit" else ref.MISS
    bf = fresh(api, ctx, "n65", threshold, target=mp)
    if history != "fresh":
        assert bf.alignClouds() == (history == "after a hit")
    good = ref.params("n65", threshold)
    for what, change in BAD_GRIDS.items():
        configure(bf, dict(good, **change))
        refused(bf, SF_ERR_INVALID)
    configure(bf, good)
    empty = api.Map(ctx, api.Cloud(ctx, np.zeros((0, 3), np.float32)))
    bf.setTargetCloud(empty)
    refused(bf, SF_ERR_STATE)                                                      # a target with no point
    bf.setTargetCloud(mp)
    mp.window_sphere([100.0, 100.0, 100.0], 0.5)
    assert mp.window_count() == 0
    refused(bf, SF_ERR_STATE)                                                      # a window that accepts nothing
    mp.window_obb([100.0, 0.0, 0.0], np.eye(3), [1.0, 1.0, 1.0])
    refused(bf, SF_ERR_STATE)
    mp.window_none()
    bf.setSourceCloud(np.zeros((0, 3), np.float32))
    refused(bf, SF_ERR_STATE)                                                      # an empty source
    bf.setSourceCloud(c["src"])
    # and the handle still answers: what a fresh one answers from the same starting pose
    before = state(bf)
    prev = np.frombuffer(before[1], np.float32).reshape(4, 4)
    align_and_compare(bf, oracle_of("n65", threshold, prev))
    bf.close()


def test_refusals_without_source_or_target(api, ctx):
    c = ref.case("n65")
    bf = api.BruteForceAlignment(ctx)
    configure(bf, ref.params("n65", ref.MISS))
    refused(bf, SF_ERR_STATE)                                                      # neither
    bf.setSourceCloud(c["src"])
    refused(bf, SF_ERR_STATE)                                                      # no target
    bf.close()
    bf = api.BruteForceAlignment(ctx)
    configure(bf, ref.params("n65", ref.MISS))
    bf.setTargetCloud(c["tgt"])
    refused(bf, SF_ERR_STATE)                                                      # no source
    bf.setTargetCloud(np.zeros((0, 3), np.float32))                                # the handle's own map, empty
    bf.setSourceCloud(c["src"])
    refused(bf, SF_ERR_STATE)
    bf.close()
