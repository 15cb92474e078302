"""Plain float64 restatement of the brute-force start-up alignment (sf_bf_align_clouds; brute_force_alignment.cpp:65-136), what
tests/test_gpu_bf_direct.py holds the device to and tests/test_bf_rule.py holds the oracle's bf_align to, and the table of cases
both files run.  Not a test module.

The rule.  Four candidate sequences {-0, +0, -s, +s, -2s, ...}: entries -i*s and i*s in float32 for every int i with
float32(i) < b, b = range / (2 * step) + 1 evaluated in float32 -- ceil(b) values of i, 2 * ceil(b) entries.  Candidates in the
nesting order x, y, z, yaw (yaw fastest).  T = prev @ L with L = [Rz(yaw) | x y z].  The score of a candidate is the mean over the
source points p of the squared distance from T p to the nearest target point (every target point tried: an n x m matrix, no tree).
Walking the candidates in order: the best so far is replaced on a strictly smaller score; the first score under the threshold ends
the walk ("found", that candidate is the result, `previous` stays); if none is, the best is the result and previous <- best.
`accept` masks target points (a window of the map).  `nonfinite_zero`: a source point with a non-finite coordinate adds 0 to the sum
and still counts in the divisor -- the device's documented rule (k_bf_score); without the flag such a source is refused, because
the reference's behaviour is undefined there.

The error bound of a float32 score against this float64 one, u = 2^-24, gamma_k = k u / (1 - k u).  Nothing here is fitted to
what any implementation returns.

 1. The transform.  With A = |prev| @ |L| (entrywise absolute values), the float32 T differs from the float64 one by at most
    gamma_8 A entrywise: each entry is a sum of four products formed unfused, k ascending -- its first product meets 4 roundings
    (one multiply, three adds) -- and the entries of L are sinf / cosf of the float32 yaw (within 1 ulp = 2u) and fl(fl(1 - c) + c)
    for the 1 (within 2u); the translations -i*s, i*s are exact float32 products in both.  4 + 2 roundings, stated as gamma_8.  The
    query is q_r = fl(fl(fl(T_r0 x + T_r1 y) + T_r2 z) + T_r3), unfused: four roundings per coordinate on |T_row| . |p| + |t|.  With
    |T32| <= (1 + gamma_8) A that is, per coordinate r,
        e_r <= g (A_r0 |x| + A_r1 |y| + A_r2 |z| + A_r3),   g = gamma_4 (1 + gamma_8) + gamma_8,
    and eps = sqrt(e_0^2 + e_1^2 + e_2^2) bounds the distance between the float32 query and the exact one.
 2. l2_simple.  d2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)) with dx = fl(qx - px): one rounding in dx, so two in its square, one
    for the product, two adds: five roundings on a sum of non-negative terms, relative gamma_5 (plus 3 * 2^-149 for products
    that fall into the subnormals).  The device's search returns the exact minimum over the target of that float32 d2.  With D
    the exact distance of the exact query to its nearest target point, every target point is within eps of where the exact query
    sees it, so  (D - eps)_+^2 (1 - gamma_5) <= min d2 <= (D + eps)^2 (1 + gamma_5), hence per point
        b = (2 D eps + eps^2)(1 + gamma_5) + gamma_5 D^2 + 3 * 2^-149.
 3. The sum and the division.  A serial float32 sum of n non-negative terms and one division by float32(n) (exact for
    n < 2^24): relative gamma_n <= (n + 2) u while n (n + 2) u <= 2, which bf_ref asserts.  So
        |score32 - score64| <= mean(b) (1 + (n + 2) u) + (n + 2) u score64.
"""
import functools

import numpy as np

U = 2.0 ** -24
F32 = np.float32


def gamma(k):
    return k * U / (1.0 - k * U)


def sequence_length(rng, step):
    """Entries of sequence(rng, step) by arithmetic: 2 * ceil(b).  None where the rule gives no sequence (a step that is not a
    finite positive number, a range that is not a finite non-negative one)."""
    rng, step = F32(rng), F32(step)
    if not (np.isfinite(step) and step > 0 and np.isfinite(rng) and rng >= 0):
        return None
    with np.errstate(over="ignore"):
        b = rng / (F32(2) * step) + F32(1)
    return None if not np.isfinite(b) else 2 * int(np.ceil(np.float64(b)))


def sequence(rng, step):
    """The loop itself (brute_force_alignment.cpp:148-180), float32."""
    rng, step = F32(rng), F32(step)
    with np.errstate(over="ignore"):                                                # 2 * step may be +inf: b is 1 then
        b = rng / (F32(2) * step) + F32(1)
    assert b.dtype == np.float32 and np.isfinite(b) and b < 4096
    out, i = [], 0
    while F32(i) < b:
        out += [F32(-i) * step, F32(i) * step]
        i += 1
    return np.array(out, np.float32)


def grid(prm):
    return (sequence(prm["x_range"], prm["x_step"]), sequence(prm["y_range"], prm["y_step"]),
            sequence(prm["z_range"], prm["z_step"]), sequence(prm["yaw_range"], prm["yaw_step"]))


def nearest_d2(q, tgt, chunk=512):
    """Exact nearest squared distance of each q among tgt: the n x m matrix, in chunks of rows."""
    out = np.empty(len(q))
    for s in range(0, len(q), chunk):
        d = q[s:s + chunk, None, :] - tgt[None, :, :]
        out[s:s + chunk] = (d * d).sum(-1).min(1)
    return out


def bf_ref(src, tgt, prev, prm, accept=None, nonfinite_zero=False):
    """-> dict(found, index, n_candidates, scores [n_candidates] float64 (NaN: after the exit), bounds [n_candidates] (same),
    T [n_candidates, 4, 4] and T_bound (gamma_8 A; NaN after the exit), best_T, prev_after)."""
    src32 = np.asarray(src, np.float32).reshape(-1, 3)
    tgt32 = np.asarray(tgt, np.float32).reshape(-1, 3)
    if accept is not None:
        tgt32 = tgt32[np.asarray(accept(tgt32), bool)]
    src, tgt, prev = src32.astype(np.float64), tgt32.astype(np.float64), np.asarray(prev, np.float32).astype(np.float64).reshape(4, 4)
    n = len(src)
    assert n > 0 and len(tgt) > 0, "nothing to score: the rule has no answer"
    assert n * (n + 2) * U <= 2.0
    ok = np.isfinite(src).all(1)
    assert nonfinite_zero or ok.all(), "a non-finite source point is undefined in the reference: ask for nonfinite_zero"
    p, pa = src[ok], np.abs(src[ok])
    xs, ys, zs, ws = grid(prm)
    total = len(xs) * len(ys) * len(zs) * len(ws)
    thr = np.float64(F32(prm["threshold"]))
    scores, bounds = np.full(total, np.nan), np.full(total, np.nan)
    Ts, Tb = np.full((total, 4, 4), np.nan), np.full((total, 4, 4), np.nan)
    g = gamma(4) * (1.0 + gamma(8)) + gamma(8)
    rel = (n + 2) * U
    best, best_idx, found, k = np.inf, -1, False, 0
    for x in xs:
        for y in ys:
            for z in zs:
                for w in ws:
                    w64 = np.float64(w)
                    L = np.eye(4)
                    L[:2, :2] = [[np.cos(w64), -np.sin(w64)], [np.sin(w64), np.cos(w64)]]
                    L[:3, 3] = [x, y, z]
                    T = prev @ L
                    A = np.abs(prev) @ np.abs(L)
                    Ts[k], Tb[k] = T, gamma(8) * A
                    Tb[k, 3] = 0.0                                                  # 0 0 0 1 of prev: exact products
                    d2 = nearest_d2(p @ T[:3, :3].T + T[:3, 3], tgt)
                    eps = np.sqrt(((g * (pa @ A[:3, :3].T + A[:3, 3])) ** 2).sum(1))
                    D = np.sqrt(d2)
                    b = (2.0 * D * eps + eps * eps) * (1.0 + gamma(5)) + gamma(5) * d2 + 3.0 * 2.0 ** -149
                    scores[k] = d2.sum() / n                                        # the points left out add 0, the divisor stays n
                    bounds[k] = b.sum() / n * (1.0 + rel) + rel * scores[k]
                    if scores[k] < best:
                        best, best_idx = scores[k], k
                    if scores[k] < thr:
                        found = True
                        break
                    k += 1
                if found:
                    break
            if found:
                break
        if found:
            break
    index = k if found else best_idx
    return dict(found=found, index=index, n_candidates=total, scores=scores, bounds=bounds, T=Ts, T_bound=Tb, best_T=Ts[index],
                prev_after=prev if found else Ts[best_idx], threshold=F32(prm["threshold"]))


def check(r, found, index, n_candidates, scores, best_T=None):
    """An implementation's answer (float32 scores; entries the reference did not compute are ignored) against bf_ref's `r`:
    the count; every score within its bound; the decision, as the rule makes it from the implementation's OWN float32 scores
    (first under the threshold, else the first smallest), and as bf_ref made it wherever the bounds leave no doubt."""
    assert n_candidates == r["n_candidates"] == len(scores)
    done = ~np.isnan(r["scores"])
    s32 = np.asarray(scores, np.float32)
    assert np.isfinite(s32[done]).all()
    err = np.abs(s32[done].astype(np.float64) - r["scores"][done])
    worst = int(np.argmax(err - r["bounds"][done]))
    assert (err <= r["bounds"][done]).all(), (worst, err[worst], r["bounds"][done][worst])
    thr = r["threshold"]
    # the case itself must be decisive: no exact score within its bound of the threshold
    assert (np.abs(r["scores"][done] - np.float64(thr)) > r["bounds"][done]).all(), "ill-posed case: a score sits at the threshold"
    assert bool(found) == r["found"]
    own = s32[:int(done.sum())]
    under = np.flatnonzero(own < thr)
    if r["found"]:
        assert index == r["index"] == under[0]
    else:
        assert len(under) == 0 and index == int(np.argmin(own))                     # strict <: the first of equal scores
        assert r["scores"][index] - r["bounds"][index] <= r["scores"][r["index"]] + r["bounds"][r["index"]]
    if best_T is not None:
        assert (np.abs(np.asarray(best_T, np.float64) - r["T"][index]) <= r["T_bound"][index]).all()


# ------------------------------------------------------------------ windows, as the device decides them (sf_nn.hpp window_accepts)
def sphere_accept(center, radius):
    c, r2 = np.asarray(center, np.float32), F32(float(radius) * float(radius))

    def accept(P):
        P = np.asarray(P, np.float32)
        dx, dy, dz = c[0] - P[:, 0], c[1] - P[:, 1], c[2] - P[:, 2]
        d2 = ((dx * dx) + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        return d2 < r2
    return accept


def obb_accept(center, R, extent):
    c, R, half = np.asarray(center, np.float64), np.asarray(R, np.float64).reshape(3, 3), np.asarray(extent, np.float64) / 2

    def accept(P):
        d = np.asarray(P, np.float32).astype(np.float64) - c
        ok = np.ones(len(d), bool)
        for k in range(3):
            ok &= np.abs((d[:, 0] * R[0, k] + d[:, 1] * R[1, k]) + d[:, 2] * R[2, k]) <= half[k]
        return ok
    return accept


# ------------------------------------------------------------------ the cases
SIZES = (1, 2, 63, 64, 65, 128, 255, 256, 257, 1500)   # a lone point, a short wave, 64 exactly (no tail), one past, around the 256-thread block
HIT, MISS = 1.0e-3, 1.0e-9                              # the true pose scores 3 sigma^2 = 7.5e-5; a pose 0.1 m off about 1e-2
SIGMA = 0.005
G32 = dict(x_step=0.1, y_step=0.1, z_step=0.1, yaw_step=0.1, x_range=0.1, y_range=0.0, z_range=0.0, yaw_range=0.0)    # 4 x 2 x 2 x 2
G128 = dict(x_step=0.1, y_step=0.1, z_step=0.1, yaw_step=0.1, x_range=0.2, y_range=0.2, z_range=0.0, yaw_range=0.2)   # 4 x 4 x 2 x 4
G256 = dict(x_step=0.1, y_step=0.1, z_step=0.1, yaw_step=0.1, x_range=0.1, y_range=0.1, z_range=0.1, yaw_range=0.1)   # 4 x 4 x 4 x 4: every entry of L in play
G16 = dict(x_step=0.1, y_step=0.1, z_step=0.1, yaw_step=0.1, x_range=0.0, y_range=0.0, z_range=0.0, yaw_range=0.0)    # {-0, +0}^4: ties
G64W = dict(x_step=1.5, y_step=1.5, z_step=0.1, yaw_step=0.1, x_range=3.0, y_range=3.0, z_range=0.0, yaw_range=0.0)   # +-1.5 m: 6 cells of 0.25
L_TRUE = (0.1, 0.0, 0.0)                               # the grid point the scans are made for: xs[3] of G32 and G128


def make_T(xyz, rpy_deg):
    r, p, y = np.radians(rpy_deg)
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rz @ Ry @ Rx, xyz
    return T


PREV = make_T((1.5, -0.7, 0.3), (2.0, -3.0, 20.0)).astype(np.float32)
PREV_FAR = make_T((1000.5, -987.25, 1012.125), (30.0, -20.0, 65.0)).astype(np.float32)
FAR = np.array([1000.0, -990.0, 1010.0])
OBB = dict(center=[0.2, -0.1, 0.0], R=make_T((0, 0, 0), (0.0, 0.0, 30.0))[:3, :3], extent=[4.0, 3.0, 1.5])
SPHERE = dict(center=[0.5, 0.5, 0.0], radius=2.0)


@functools.lru_cache(maxsize=None)
def world(kind="box"):
    """The targets: 800 points uniform in [-3, 3]^2 x [-1, 1] (mean spacing 0.45 m: nearly two cells of 0.25) and what is cut from them."""
    rng = np.random.default_rng(20240607)
    box = np.c_[rng.uniform(-3, 3, 800), rng.uniform(-3, 3, 800), rng.uniform(-1, 1, 800)].astype(np.float32)
    if kind == "box":
        out = box
    elif kind == "far":
        out = (box.astype(np.float64) + FAR).astype(np.float32)
    elif kind == "plane":
        out = box.copy()
        out[:, 2] = 0.5
    elif kind == "dup":
        out = np.tile(box[:160], (5, 1))[rng.permutation(800)]
    elif kind == "one":
        out = box[17:18].copy()
    elif kind == "two":
        out = box[17:19].copy()
    out.setflags(write=False)
    return out


def scan(tgt, n, prev, seed):
    """n noisy samples of tgt (with repeats) as a sensor at prev @ [I | L_TRUE] sees them."""
    rng = np.random.default_rng(seed)
    T = np.asarray(prev, np.float64) @ make_T(L_TRUE, (0, 0, 0))
    p = tgt[rng.integers(0, len(tgt), n)].astype(np.float64) + rng.normal(0.0, SIGMA, (n, 3))
    return ((p - T[:3, 3]) @ T[:3, :3]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(src, tgt, prev, grid, cell (of the device's index: 0.25, or None for the automatic one), accept / window (or None),
    nonfinite).  The threshold is not part of a case: run(name, threshold) adds it."""
    c = dict(tgt=world("box"), prev=PREV, grid=G32, cell=0.25, accept=None, window=None, nonfinite=False)
    if name[0] == "n" and name[1:].isdigit():                  # "n257": the source sizes
        c["src"] = scan(c["tgt"], int(name[1:]), PREV, 100 + int(name[1:]))
    elif name == "n65_g128":                                   # the same scan over more candidates
        c["src"], c["grid"] = case("n65")["src"], G128
    elif name in ("cell0.1", "cell1.0", "cellauto"):
        c["src"] = scan(c["tgt"], 257, PREV, 357)
        c["cell"] = None if name == "cellauto" else float(name[4:])
    elif name in ("one", "two", "plane", "dup"):
        c["tgt"] = world(name)
        c["src"] = scan(world("plane" if name == "plane" else "dup" if name == "dup" else "box"), 130, PREV, 7)
    elif name == "far":                                        # rotation about all three axes, everything 1 km out; candidates that
        c["tgt"], c["prev"], c["grid"] = world("far"), PREV_FAR, G256      # move in y, z and yaw too: with those at 0 every product of
        c["src"] = scan(c["tgt"], 130, PREV_FAR, 8)                        # prev @ L but one is by 0 or 1, and fused or not is the same T
    elif name == "outside":                                    # the whole scan 3 m and more beyond the target's box
        c["prev"] = (make_T((9.0, 0.0, 0.0), (0, 0, 0)) @ PREV.astype(np.float64)).astype(np.float32)
        c["src"] = scan(c["tgt"], 200, PREV, 9)
    elif name == "wide":                                       # candidates 1.5 m apart
        c["grid"] = G64W
        c["src"] = scan(c["tgt"], 100, PREV, 10)
    elif name == "ties":
        c["grid"] = G16
        c["src"] = scan(c["tgt"], 65, PREV, 11)
    elif name in ("sphere", "obb", "single"):                  # the scan sees what the window keeps (a hit is possible), the map holds all
        if name == "sphere":
            c["window"] = ("sphere", SPHERE["center"], SPHERE["radius"])
            c["accept"] = sphere_accept(SPHERE["center"], SPHERE["radius"])
        elif name == "obb":
            c["window"] = ("obb", OBB["center"], OBB["R"], OBB["extent"])
            c["accept"] = obb_accept(OBB["center"], OBB["R"], OBB["extent"])
        else:                                                  # a sphere of 1 cm about one target point
            c["window"] = ("sphere", c["tgt"][17], 0.01)
            c["accept"] = sphere_accept(c["tgt"][17], 0.01)
        c["src"] = scan(c["tgt"][c["accept"](c["tgt"])] if name != "single" else c["tgt"], 200, PREV, 12)
    elif name == "nonfinite":
        s = scan(c["tgt"], 130, PREV, 13).copy()
        s[3, 0], s[64, 1], s[65, 2], s[129] = np.nan, np.inf, -np.inf, np.nan
        c["src"], c["nonfinite"] = s, True
    else:
        raise KeyError(name)
    c["src"].setflags(write=False)
    return c


def params(name, threshold):
    return dict(case(name)["grid"], threshold=threshold)


@functools.lru_cache(maxsize=None)
def run(name, threshold):
    """bf_ref of a case, computed once per process."""
    c = case(name)
    return bf_ref(c["src"], c["tgt"], c["prev"], params(name, threshold), accept=c["accept"], nonfinite_zero=c["nonfinite"])


def target_of(name):
    """The target as the oracle is given it: the points the case's window accepts."""
    c = case(name)
    return c["tgt"] if c["accept"] is None else c["tgt"][c["accept"](c["tgt"])]


# every (case, threshold) both test files run; the one-point, two-point and single-point-window targets, the scan outside the
# target's box and the grid of ties hit only under a threshold above the squared size of the world; the wide grid has no
# candidate nearer the truth than 0.1 m (score 1e-2 at most), its others are 1.5 m off
RUNS = [("n%d" % n, t) for n in SIZES for t in (HIT, MISS)] + [
    ("n65_g128", HIT), ("n65_g128", MISS),
    ("cell0.1", HIT), ("cell0.1", MISS), ("cell1.0", HIT), ("cell1.0", MISS), ("cellauto", HIT), ("cellauto", MISS),
    ("one", MISS), ("one", 1.0e3), ("two", MISS), ("two", 1.0e3), ("plane", HIT), ("plane", MISS), ("dup", HIT), ("dup", MISS),
    ("far", HIT), ("far", MISS), ("outside", MISS), ("outside", 1.0e3), ("wide", 0.03), ("wide", MISS), ("ties", MISS), ("ties", 1.0e3),
    ("sphere", HIT), ("sphere", MISS), ("obb", HIT), ("obb", MISS), ("single", MISS), ("single", 1.0e3),
]
