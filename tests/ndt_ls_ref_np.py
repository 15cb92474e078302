"""numpy restatement of the NDT line search and of the coarse-to-fine schedule (include/slamfusion.h behind the NDT block, DESIGN section
25), on top of tests/ndt_ref_np.py, and the named fixtures of their tests.

Per iteration, when trials >= 1:
 1. the derivatives at T as ndt_ref_np.evaluate gives them: phi0 (the score), g, H; not usable: NO_OVERLAP as in ndt_ref_np.align;
 2. d = -V L~^-1 V^T g, ndt_ref_np.newton_step's solve before the clamp; raw = |d|;
 3. alpha_max = step_max / raw when raw > step_max, else 1; slope = ((((g0 d0 + g1 d1) + g2 d2) + g3 d3) + g4 d4) + g5 d5;
 4. trial k = 0 .. trials - 1: alpha_k = ldexp(alpha_max, -k), T_k = M(alpha_k d) T;
 5. phi_k, terms_k: the score and the number of terms at T_k;
 6. the smallest k with terms_k > 0, phi_k finite and phi_k <= phi0 + (armijo * alpha_k) * slope is taken: T <- T_k, iterations + 1,
    modified + 1 when an eigenvalue was negative or floored, converged when alpha_k * raw < transformation_epsilon;
 7. no such k: LINE_SEARCH_STALLED, the pose stays, the alignment ends with converged = 0 (modified is not counted: no step was taken).
step_size is not used.  The final evaluation is ndt_ref_np.align's.

Margin of a comparison.  The device compares its own phi_k with its own limit_k = phi0 + (armijo * alpha_k) * slope.  phi_k and phi0 are
each within ndt_ref_np.deriv_bound of the restatement's at the same pose; the term (armijo * alpha_k) * slope is 1e-4 of a directional
derivative and moves by far less.  A comparison falls the same way on both sides when |phi_k - limit_k| exceeds the sum of the two score
bounds; the rule tests ask 16 times that sum (row["margin"] is |phi_k - limit_k| / (bound_k + bound_0), the least over the comparisons
made: k <= chosen, or every k of a stalled row)."""
import functools

import numpy as np

import ndt_ref_np as nr

STALLED = 2
LS_DEFAULTS = dict(trials=8, step_max=1.0, armijo=1e-4)
MAX_TRIALS = 16


def slope_of(g, d):
    return ((((g[0] * d[0] + g[1] * d[1]) + g[2] * d[2]) + g[3] * d[3]) + g[4] * d[4]) + g[5] * d[5]


def direction(ev, hessian_floor=1e-6):
    """-> None (not usable), else ndt_ref_np.newton_step without the clamp: delta = d, length = raw_length = |d|"""
    return nr.newton_step(ev, np.inf, hessian_floor)


def step_range(st, step_max):
    raw = st["raw_length"]
    return step_max / raw if raw > step_max else 1.0


def pick(phi0, slope, alpha_max, phi, n_terms, armijo):
    """Rule steps 6 and 7 on given numbers (comparisons and IEEE products only) -> chosen k or -1"""
    for k in range(len(phi)):
        alpha = float(np.ldexp(alpha_max, -k))
        if n_terms[k] > 0 and np.isfinite(phi[k]) and phi[k] <= phi0 + (armijo * alpha) * slope:
            return k
    return -1


def search(mdl, src, T, ev, st, trials, step_max, armijo, neighbours=7, outlier_ratio=0.55):
    """One iteration's row from the evaluation `ev` and the direction `st` at T -> dict(alpha_max, raw_length, phi0, slope, delta, phi
    [trials], n_terms [trials], chosen, trials, poses [trials, 4, 4], bounds [trials] (bound_k + bound_0), margin, face_gap (the least over the trials))"""
    d = st["delta"]
    alpha_max = step_range(st, step_max)
    slope = float(slope_of(ev["gradient"], d))
    b0 = nr.deriv_bound(ev)[0]
    phi, terms, poses, bounds, gap = [], [], [], [], np.inf
    for k in range(trials):
        Tk = nr.vec6_to_mat4(float(np.ldexp(alpha_max, -k)) * d) @ T
        e = nr.evaluate(mdl, src, Tk, neighbours, outlier_ratio, derivs=False)
        phi.append(e["score"]); terms.append(e["n_terms"]); poses.append(Tk); bounds.append(nr.deriv_bound(e)[0] + b0)
        gap = min(gap, e["face_gap"])
    chosen = pick(ev["score"], slope, alpha_max, phi, terms, armijo)
    last = chosen if chosen >= 0 else trials - 1
    margin = min(abs(phi[k] - (ev["score"] + (armijo * float(np.ldexp(alpha_max, -k))) * slope)) / bounds[k] for k in range(last + 1))
    return dict(alpha_max=alpha_max, raw_length=st["raw_length"], phi0=ev["score"], slope=slope, delta=d, phi=np.array(phi), n_terms=np.array(terms, np.int64),
                chosen=chosen, trials=trials, poses=np.array(poses), bounds=np.array(bounds), margin=float(margin), face_gap=gap)


def align(mdl, src, T0, trials=8, step_max=1.0, armijo=1e-4, neighbours=7, outlier_ratio=0.55, transformation_epsilon=1e-4, max_iterations=30, hessian_floor=1e-6,
          step_size=0.1, **_):
    """ndt_ref_np.align's dict; with trials >= 1 also rows (search() of every evaluated iteration), chosen (their k) and steps (the
    direction() of every iteration taken)"""
    if trials == 0:
        return nr.align(mdl, src, T0, neighbours=neighbours, outlier_ratio=outlier_ratio, step_size=step_size, transformation_epsilon=transformation_epsilon,
                        max_iterations=max_iterations, hessian_floor=hessian_floor)
    T = np.array(T0, np.float64).reshape(4, 4)
    trace, steps, rows, evs = [T.copy()], [], [], []
    it, converged, modified, flags, gap = 0, False, 0, 0, np.inf
    while it < max_iterations and not converged:
        ev = nr.evaluate(mdl, src, T, neighbours, outlier_ratio)
        gap = min(gap, ev["face_gap"])
        st = direction(ev, hessian_floor)
        if st is None or not np.isfinite(st["raw_length"]):
            flags |= nr.NO_OVERLAP
            break
        row = search(mdl, src, T, ev, st, trials, step_max, armijo, neighbours, outlier_ratio)
        rows.append(row); evs.append(ev)
        gap = min(gap, row["face_gap"])
        if row["chosen"] < 0:
            flags |= STALLED
            break
        steps.append(st)
        T = row["poses"][row["chosen"]].copy()
        trace.append(T.copy())
        it += 1
        modified += int(st["modified"])
        converged = bool(float(np.ldexp(row["alpha_max"], -row["chosen"])) * st["raw_length"] < transformation_epsilon)
    ev = nr.evaluate(mdl, src, T, neighbours, outlier_ratio)
    gap = min(gap, ev["face_gap"])
    ok = nr.usable(ev)
    if not ok:
        flags |= nr.NO_OVERLAP
    return dict(T64=T, score=ev["score"] if ok else 0.0, gradient=ev["gradient"] if ok else np.zeros(6), hessian=ev["hessian"] if ok else np.zeros((6, 6)),
                n_inside=ev["n_inside"], n_terms=ev["n_terms"], iterations=it, converged=converged, modified=modified, flags=flags,
                trace=np.array(trace), steps=steps, rows=rows, evaluations=evs, chosen=[r["chosen"] for r in rows], face_gap=gap)


def align_levels(models, src, T0, line_search=LS_DEFAULTS, **params):
    """Coarse to fine: every level starts where the previous one ended, whatever its flags -> (the last level's dict, every level's)"""
    T, per_level = np.array(T0, np.float64).reshape(4, 4), []
    for mdl in models:
        per_level.append(align(mdl, src, T, **dict(params, **(line_search or dict(trials=0)))))
        T = per_level[-1]["T64"]
    return per_level[-1], per_level


def trial_step_bound(ev, st, T, alpha_max):
    """ndt_ref_np.step_bound for an entry of M(ldexp(alpha_max, -k) d) T: doubled, as for the clamp, when alpha_max = step_max / raw
    rescales the direction (the powers of two are exact and only shrink the error); st: direction()"""
    return nr.step_bound(ev, dict(st, length=st["raw_length"] if alpha_max == 1.0 else 0.0), T)


def direction_bound(ev, st, T):
    """-> (of an entry of d, of raw = |d|, of the slope g . d): ndt_ref_np.step_bound is at least twice the 2-norm error of the direction,
    hence a bound of every entry and of the norm; the norm of six entries adds 8 roundings, the slope the error of g against |d|, that
    of d against |g| and 8 roundings of its sum"""
    dd = nr.step_bound(ev, st, T)
    eg = nr.deriv_bound(ev)[1]
    g, d = ev["gradient"], st["delta"]
    return dd, dd + 8.0 * nr.U * st["raw_length"], np.linalg.norm(eg) * st["raw_length"] + np.linalg.norm(g) * dd + 8.0 * nr.U * np.abs(g * d).sum()


# ------------------------------------------------------------------ fixtures (each computed once per session)
# The starts below were drawn at random (numpy default_rng, the seed and the draw are named) on the sphere of the given distance and
# angle and kept when the restatement met what tests/test_ndt_ls_rule.py asserts of them.
LEVELS = dict(room=(2.0, 1.0), terrain=(4.0, 2.0, 1.0))


@functools.lru_cache(maxsize=None)
def model_at(target, resolution):
    if resolution == nr.ALIGN_RES[target]:
        return nr.model_of(target)
    return nr.model(nr.room_target() if target == "room" else nr.terrain_target(), resolution)


# name -> (target, resolution, start): about 1.5 m / 12 degrees (draw 1 of default_rng(2501): a unit direction times 1.5 m, a unit axis
# times 12 degrees as roll, pitch, yaw, both rounded as written).  At 2 m a cell of the room holds floor and walls together; the
# alignment backtracks twice, then no trial down to alpha_max / 128 lowers the score enough, every comparison by >= 8e9 bounds.
STALL = dict(room_coarse_stall=("room", 2.0, nr.pose((0.94, 0.89, -0.75), (3.3, 3.7, 10.9))))
# name -> (target, start): room at 1.5 m / 12 degrees (draw 5 of default_rng(2502)), terrain at 2 m / 16 degrees (draw 0 of
# default_rng(2503)).  The plain alignment at 1 m ends 2.5 m / 3.2 m from the truth, the pyramid with the search within 6 mm / 4 mm.
WIDE = dict(room_wide=("room", nr.pose((0.82, -1.25, -0.14), (-8.5, -4.6, -7.1))),
            terrain_wide=("terrain", nr.pose((-0.12, 1.45, -1.37), (13.8, -7.5, 3.0))))


@functools.lru_cache(maxsize=None)
def reference_ls(case):
    """the searched alignment (defaults 8 / 1.0 / 1e-4) of a case of ndt_ref_np.CASES at the alignment resolution"""
    tgt, start, _ = nr.CASES[case]
    return align(nr.model_of(tgt), nr.source_of(tgt), start, **LS_DEFAULTS)


@functools.lru_cache(maxsize=None)
def reference_stall(case="room_coarse_stall"):
    tgt, res, start = STALL[case]
    return align(model_at(tgt, res), nr.source_of(tgt), start, **LS_DEFAULTS)


@functools.lru_cache(maxsize=None)
def reference_wide(case):
    """-> (the plain alignment at the finest level, the pyramid's last level, its levels)"""
    tgt, start = WIDE[case]
    src = nr.source_of(tgt)
    plain = nr.align(model_at(tgt, LEVELS[tgt][-1]), src, start)
    last, per_level = align_levels([model_at(tgt, r) for r in LEVELS[tgt]], src, start)
    return plain, last, per_level
