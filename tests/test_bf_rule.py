"""The oracle's bf_align -- the bit-exact yardstick of tests/test_gpu_bf_direct.py -- against the plain float64 restatement of the
rule in tests/bf_ref_np.py, at every shape the device is tested at: found, index, candidate count, every score within the bound
derived there, the returned pose and the pose a miss leaves behind.  CPU only."""
import numpy as np
import pytest

import bf_ref_np as ref


@pytest.mark.parametrize("name,threshold", ref.RUNS, ids=["%s-%g" % r for r in ref.RUNS])
def test_oracle_bf_follows_the_rule(orc, name, threshold):
    c, r = ref.case(name), ref.run(name, threshold)
    o = orc.bf_align(c["src"], ref.target_of(name), c["prev"], **ref.params(name, threshold))
    ref.check(r, o["found"], o["index"], o["n_candidates"], o["scores"], o["best_T"])
    done = ~np.isnan(r["scores"])
    assert np.array_equal(np.isfinite(o["scores"]), done)                          # the reference stops where the rule stops
    assert abs(np.float64(o["best_score"]) - r["scores"][o["index"]]) <= r["bounds"][o["index"]]
    after = np.asarray(o["prev_T_after"], np.float64)
    if r["found"]:
        assert np.array_equal(o["prev_T_after"], c["prev"])                         # previous untouched on a hit
    else:
        assert np.array_equal(o["prev_T_after"], o["best_T"])                       # previous <- best
        assert (np.abs(after - r["T"][o["index"]]) <= r["T_bound"][o["index"]]).all()


def test_cases_are_what_they_claim():
    """The table of cases, checked on its own terms: hits hit and misses miss, the thresholds between, every source size there."""
    for name, threshold in ref.RUNS:
        r = ref.run(name, threshold)
        assert r["found"] == (threshold != ref.MISS), (name, threshold)
    for n in ref.SIZES:
        assert len(ref.case("n%d" % n)["src"]) == n
        assert ref.run("n%d" % n, ref.HIT)["index"] >= 3 * 8                        # the true pose is xs[3]: three slices are scored first
    assert ref.run("ties", ref.MISS)["n_candidates"] == 16 and ref.run("ties", ref.MISS)["index"] == 0
    s = ref.run("ties", ref.MISS)["scores"]
    assert (s == s[0]).all()                                                        # {-0, +0}^4: sixteen equal scores, the first wins
    assert ref.run("n65_g128", ref.MISS)["n_candidates"] == 128 and ref.run("wide", ref.MISS)["n_candidates"] == 64
    assert len(ref.target_of("single")) == 1 and 100 < len(ref.target_of("sphere")) < 700 and 100 < len(ref.target_of("obb")) < 700
    c = ref.case("outside")                                                         # every query of every candidate beyond the box by > 2 m
    q = c["src"].astype(np.float64) @ c["prev"][:3, :3].astype(np.float64).T + c["prev"][:3, 3]
    assert (q[:, 0] - 3.0).min() > 2.0 + 0.1
    flat = ref.case("plane")["tgt"]
    assert np.ptp(flat[:, 2]) == 0.0
    assert len(np.unique(ref.case("dup")["tgt"], axis=0)) == 160
    assert (~np.isfinite(ref.case("nonfinite")["src"]).all(1)).sum() == 4


def mul4_f32(A, B, fused):
    """prev @ L in float32, k ascending: the products rounded before they are added, or fused into the additions (the float64
    product of two float32 values is exact, so rounding product + sum once is the fused result up to a double rounding)."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    C = np.empty((4, 4), np.float32)
    for r in range(4):
        for c in range(4):
            acc = A[r, 0] * B[0, c]
            for k in (1, 2, 3):
                acc = np.float32(np.float64(A[r, k]) * np.float64(B[k, c]) + np.float64(acc)) if fused else acc + A[r, k] * B[k, c]
            C[r, c] = acc
    return C


def test_general_pose_case_tells_a_contracted_product_apart(orc):
    """What the "far" case is for: the float32 T = prev L of its candidates changes when the multiply-adds are contracted, so
    "T is bit-identical to the reference" fails on the device if its host code ever is.  (With y, z and yaw at 0 every product
    but one is by 0 or 1 and the two forms agree: the size cases cannot tell.)  The unfused form is the oracle's, bit for bit."""
    def L_of(x, y, z, w):
        cs, sn = np.float32(np.cos(np.float64(w))), np.float32(np.sin(np.float64(w)))
        o = np.float32(0)
        return np.array([[o + cs, o - sn, 0, x], [o + sn, o + cs, 0, y], [0, 0, (np.float32(1) - cs) + cs, z], [0, 0, 0, 1]], np.float32)
    c = ref.case("far")
    xs, ys, zs, ws = ref.grid(c["grid"])
    differ = sum(not np.array_equal(mul4_f32(c["prev"], L_of(x, y, z, w), True), mul4_f32(c["prev"], L_of(x, y, z, w), False))
                 for x in xs for y in ys for z in zs for w in ws)
    assert differ >= 128                                                           # every candidate with a non-zero yaw, at the least
    s = ref.case("n257")
    xs, ys, zs, ws = ref.grid(s["grid"])
    assert all(np.array_equal(mul4_f32(s["prev"], L_of(x, y, z, w), True), mul4_f32(s["prev"], L_of(x, y, z, w), False))
               for x in xs for y in ys for z in zs for w in ws)
    o = orc.bf_align(c["src"], c["tgt"], c["prev"], **ref.params("far", ref.HIT))
    k = o["index"]
    x, y, z, w = xs_at(ref.grid(c["grid"]), k)
    assert o["found"] and w == 0                                                   # (a yaw of 0: no sinf / cosf rounding to argue about)
    assert np.array_equal(mul4_f32(c["prev"], L_of(x, y, z, w), False).view(np.uint32), o["best_T"].view(np.uint32))


def xs_at(g, k):
    xs, ys, zs, ws = g
    d, k = k % len(ws), k // len(ws)
    c, k = k % len(zs), k // len(zs)
    b, a = k % len(ys), k // len(ys)
    return xs[a], ys[b], zs[c], ws[d]


def test_windows_are_the_oracles_crops(orc):
    """The numpy predicates keep exactly the points the oracle's crops keep."""
    tgt = ref.case("sphere")["tgt"]
    _, idx = orc.crop_radius(tgt, np.asarray(ref.SPHERE["center"], np.float32), ref.SPHERE["radius"])
    assert np.array_equal(np.flatnonzero(ref.case("sphere")["accept"](tgt)), np.sort(idx))
    _, idx = orc.crop_obb(tgt, ref.OBB["center"], ref.OBB["R"], ref.OBB["extent"])
    assert np.array_equal(np.flatnonzero(ref.case("obb")["accept"](tgt)), np.sort(idx))
    _, idx = orc.crop_radius(tgt, tgt[17], 0.01)
    assert list(idx) == [17]


def test_nonfinite_rule_scales_the_finite_score():
    """Points that add 0 and still divide: the score of the finite points alone, times (n - k) / n."""
    c = ref.case("nonfinite")
    r = ref.run("nonfinite", ref.MISS)
    keep = np.isfinite(c["src"]).all(1)
    f = ref.bf_ref(c["src"][keep], c["tgt"], c["prev"], ref.params("nonfinite", ref.MISS))
    assert np.allclose(r["scores"], f["scores"] * keep.sum() / len(keep), rtol=1e-14, atol=0)
    with pytest.raises(AssertionError):
        ref.bf_ref(c["src"], c["tgt"], c["prev"], ref.params("nonfinite", ref.MISS))


def test_sequence_length_is_the_loops(orc):
    """The count the device refuses grids by, 2 * ceil(range / (2 step) + 1) in float32, against the loop it stands for: the
    oracle's, and the one restated here."""
    rng = np.random.default_rng(5)
    pairs = [(0.0, 0.1), (0.1, 0.1), (0.2, 0.1), (1.5, 0.1), (0.1, 0.05), (np.pi / 6, np.pi / 18), (3.0, 1.5), (2047.0, 0.5), (1.0, 3.0e38),
             (1.0e-40, 1.0e-40), (0.0, 1.0e-45), (4.1, 0.1)]
    pairs += [(float(r), float(s)) for r, s in zip(rng.uniform(0, 4, 300), rng.uniform(0.01, 1.0, 300))]
    pairs += [(float(np.float32(s) * np.float32(2 * k)), float(s)) for k, s in zip(rng.integers(0, 40, 100), rng.uniform(0.01, 1.0, 100))]  # b a whole number
    for r, s in pairs:
        want = ref.sequence_length(r, s)
        assert want == len(orc.bf_sequence(r, s)) == len(ref.sequence(r, s)), (r, s)
        assert np.array_equal(orc.bf_sequence(r, s), ref.sequence(r, s))
    assert len(orc.bf_sequence(1.5, 0.1)) == 18
    for r, s in ((1.0, 0.0), (1.0, -0.1), (1.0, np.nan), (1.0, np.inf), (-1.0, 0.1), (np.nan, 0.1), (np.inf, 0.1), (1.0, 1.0e-45)):
        assert ref.sequence_length(r, s) is None                                   # (the last: b overflows to +inf)
