"""The pose-from-matches rule restated in numpy (include/slamfusion.h, sf_cloud_register_pairs): samples,
hypotheses (degenerate test, edge check, Horn's closed form), score, choice, refit and final flags, stage by stage, so that the
device can be compared with each of them.  Nothing here calls the library.  tests/test_reg_rule.py pins this file to facts it was
not built from (the known answers of mix, numpy.linalg.svd Kabsch, a float64 distance count); tests/test_gpu_register.py compares
the device with it."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
MAX_HYPOTHESES = 1 << 20
EPS = float(np.finfo(np.float64).eps)


def mix(x):
    """the splitmix64 step on uint64 with wrap-around (python ints)"""
    z = (x + GOLDEN) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mix_u64(x):
    """the same step on a uint64 array (numpy wraps)"""
    with np.errstate(over="ignore"):
        z = x + np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def samples(seed, num_hypotheses, m):
    """int32 [H, 3]: hypothesis h samples the pairs mix(seed + GOLDEN (3h + j + 1)) mod m"""
    k = np.arange(1, 3 * num_hypotheses + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = np.uint64(seed & M64) + np.uint64(GOLDEN) * k
    return (mix_u64(x) % np.uint64(m)).astype(np.int32).reshape(num_hypotheses, 3)


def pack(src, dst, pairs):
    """-> (s, t) float32 [m, 3]: the points of the pairs"""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    return np.asarray(src, np.float32)[pairs[:, 0]], np.asarray(dst, np.float32)[pairs[:, 1]]


def _len2(a, b):
    d = a - b
    l = d[..., 0] * d[..., 0]
    l = l + d[..., 1] * d[..., 1]
    l = l + d[..., 2] * d[..., 2]
    return l


def _spans(a, b, c):
    u, v = b - a, c - a
    cx = u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1]
    cy = u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2]
    cz = u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]
    cc = cx * cx
    cc = cc + cy * cy
    cc = cc + cz * cz
    return (cc > 0) & np.isfinite(cc)


def horn_matrix(S):
    """Horn's symmetric 4x4 matrix of S_ab = sum s_a t_b, [..., 3, 3] -> [..., 4, 4]"""
    S = np.asarray(S, np.float64)
    N = np.empty(S.shape[:-2] + (4, 4))
    xx, xy, xz, yx, yy, yz, zx, zy, zz = (S[..., a, b] for a in range(3) for b in range(3))
    N[..., 0, 0] = (xx + yy) + zz
    N[..., 1, 1] = (xx - yy) - zz
    N[..., 2, 2] = (yy - xx) - zz
    N[..., 3, 3] = (zz - xx) - yy
    N[..., 0, 1] = N[..., 1, 0] = yz - zy
    N[..., 0, 2] = N[..., 2, 0] = zx - xz
    N[..., 0, 3] = N[..., 3, 0] = xy - yx
    N[..., 1, 2] = N[..., 2, 1] = xy + yx
    N[..., 1, 3] = N[..., 3, 1] = zx + xz
    N[..., 2, 3] = N[..., 3, 2] = yz + zy
    return N


def rotation_of(q):
    """the rotation of the unit quaternion (w, x, y, z), [..., 4] -> [..., 3, 3]"""
    w, x, y, z = (q[..., k] for k in range(4))
    ww, xx, yy, zz = w * w, x * x, y * y, z * z
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = ((ww + xx) - yy) - zz
    R[..., 0, 1] = 2.0 * (x * y - w * z)
    R[..., 0, 2] = 2.0 * (x * z + w * y)
    R[..., 1, 0] = 2.0 * (x * y + w * z)
    R[..., 1, 1] = ((ww - xx) + yy) - zz
    R[..., 1, 2] = 2.0 * (y * z - w * x)
    R[..., 2, 0] = 2.0 * (x * z - w * y)
    R[..., 2, 1] = 2.0 * (y * z + w * x)
    R[..., 2, 2] = ((ww - xx) - yy) + zz
    return R


def horn(S, cs, ct):
    """S [..., 3, 3] about the centroids cs, ct [..., 3] -> (T [..., 4, 4], gap [...]: the two largest eigenvalues apart, norm [...]: the
    Frobenius norm of Horn's matrix).  Non-finite input gives NaN transforms."""
    N = horn_matrix(S)
    bad = ~np.isfinite(N).all(axis=(-1, -2))
    Ns = np.where(bad[..., None, None], np.eye(4), N)
    w, V = np.linalg.eigh(Ns)                      # ascending
    q = V[..., :, 3]
    q = q / np.sqrt(((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3])[..., None]
    q = np.where((q[..., 0] < 0)[..., None], -q, q)
    R = rotation_of(q)
    T = np.zeros(N.shape[:-2] + (4, 4))
    T[..., :3, :3] = R
    with np.errstate(all="ignore"):
        for r in range(3):
            T[..., r, 3] = ct[..., r] - ((R[..., r, 0] * cs[..., 0] + R[..., r, 1] * cs[..., 1]) + R[..., r, 2] * cs[..., 2])
    T[..., 3, 3] = 1.0
    T[bad] = np.nan
    return T, w[..., 3] - w[..., 2], np.sqrt((Ns * Ns).sum(axis=(-1, -2)))


def horn_tolerance(gap, norm, cs, ct):
    """What two correct solves of one Horn matrix may differ by, per entry: 64 eps |N| / gap for the rotation; for the translation
    t = ct - R cs that rotation error through cs (three terms) plus the roundings of the four-term expression itself."""
    with np.errstate(all="ignore"):
        tol_r = 64.0 * EPS * norm / gap
        a, b = np.abs(cs).max(axis=-1), np.abs(ct).max(axis=-1)
        return tol_r, 3.0 * tol_r * a + 8.0 * EPS * (b + 3.0 * a)


def hypotheses_from_samples(s, t, idx, edge_similarity=0.9):
    """s, t float32 [m, 3], idx int32 [H, 3] -> dict(status int32 [H], T float64 [H, 4, 4] (NaN unless status 0), gap, norm, cs, ct)"""
    S3, T3 = s[idx].astype(np.float64), t[idx].astype(np.float64)          # [H, 3 samples, 3]
    H = len(idx)
    with np.errstate(all="ignore"):
        deg = (idx[:, 0] == idx[:, 1]) | (idx[:, 0] == idx[:, 2]) | (idx[:, 1] == idx[:, 2])
        deg |= ~_spans(S3[:, 0], S3[:, 1], S3[:, 2]) | ~_spans(T3[:, 0], T3[:, 1], T3[:, 2])
        rej = np.zeros(H, bool)
        if edge_similarity > 0:
            e2 = np.float64(edge_similarity) * np.float64(edge_similarity)
            for a, b in ((0, 1), (0, 2), (1, 2)):
                ls2, lt2 = _len2(S3[:, a], S3[:, b]), _len2(T3[:, a], T3[:, b])
                rej |= ~((ls2 >= e2 * lt2) & (lt2 >= e2 * ls2))
        status = np.where(deg, 1, np.where(rej, 2, 0)).astype(np.int32)
        cs = ((S3[:, 0] + S3[:, 1]) + S3[:, 2]) / 3.0
        ct = ((T3[:, 0] + T3[:, 1]) + T3[:, 2]) / 3.0
        ds, dt = S3 - cs[:, None, :], T3 - ct[:, None, :]
        S = ds[:, 0, :, None] * dt[:, 0, None, :]
        S = S + ds[:, 1, :, None] * dt[:, 1, None, :]
        S = S + ds[:, 2, :, None] * dt[:, 2, None, :]
        T, gap, norm = horn(S, cs, ct)
    status[(status == 0) & ~np.isfinite(T).all(axis=(1, 2))] = 1
    T[status != 0] = np.nan
    return dict(status=status, T=T, gap=gap, norm=norm, cs=cs, ct=ct)


def hypotheses(src, dst, pairs, num_hypotheses, seed=0, edge_similarity=0.9):
    """-> (samples int32 [H, 3], the dict of hypotheses_from_samples)"""
    s, t = pack(src, dst, pairs)
    idx = samples(seed, num_hypotheses, len(s))
    return idx, hypotheses_from_samples(s, t, idx, edge_similarity)


def to_f32(T):
    """the twelve entries of [R | t] rounded to float32, [..., 4, 4] -> [..., 12]"""
    T = np.asarray(T, np.float64)
    with np.errstate(all="ignore"):
        return T[..., :3, :].reshape(T.shape[:-2] + (12,)).astype(np.float32)


def distances2(s, t, Tf):
    """float32 [H, m]: d2 of every pair under every float32 transform [H, 12], unfused, in the order of the rule"""
    s, t, Tf = np.asarray(s, np.float32), np.asarray(t, np.float32), np.asarray(Tf, np.float32).reshape(-1, 12)
    x, y, z = s[None, :, 0], s[None, :, 1], s[None, :, 2]
    with np.errstate(all="ignore"):
        d2 = None
        for r in range(3):
            q = Tf[:, 4 * r:4 * r + 1] * x
            q = q + Tf[:, 4 * r + 1:4 * r + 2] * y
            q = q + Tf[:, 4 * r + 2:4 * r + 3] * z
            q = q + Tf[:, 4 * r + 3:4 * r + 4]
            d = q - t[None, :, r]
            d2 = d * d if d2 is None else d2 + d * d
    assert d2.dtype == np.float32
    return d2


def threshold2(distance_threshold):
    return np.float32(np.float64(distance_threshold) * np.float64(distance_threshold))


def score(s, t, Tf, distance_threshold, chunk=256):
    """int64 [H]: the inliers of every float32 transform"""
    Tf = np.asarray(Tf, np.float32).reshape(-1, 12)
    t2 = threshold2(distance_threshold)
    counts = np.zeros(len(Tf), np.int64)
    for lo in range(0, len(Tf), chunk):
        counts[lo:lo + chunk] = (distances2(s, t, Tf[lo:lo + chunk]) < t2).sum(axis=1)
    return counts


def choose(counts, min_inliers=3):
    """-> (best: the largest count, on a tie the smallest h; its count; found)"""
    best = int(np.argmax(counts))
    return best, int(counts[best]), int(counts[best] >= min_inliers)


def top(counts, status, T, top_k):
    """the top_k best in (count descending, h ascending) order, only status 0 with count > 0 -> list of dict(h, status, count, T)"""
    order = np.lexsort((np.arange(len(counts)), -np.asarray(counts)))
    out = []
    for h in order:
        if len(out) >= top_k or counts[h] <= 0:
            break
        if status[h] == 0:
            out.append(dict(h=int(h), status=0, count=int(counts[h]), T=T[h].copy()))
    return out


def refit_once(s, t, T, distance_threshold, s_ref, t_ref):
    """one refit round from the transform T [4, 4] -> (T' or None when the previous transform stands, gap, norm, cs, ct)"""
    sel = distances2(s, t, to_f32(T))[0] < threshold2(distance_threshold)
    n = int(sel.sum())
    if n < 3:
        return None, None, None, None, None
    p, q = s[sel].astype(np.float64) - s_ref, t[sel].astype(np.float64) - t_ref
    sp, sq = p.sum(axis=0), q.sum(axis=0)
    S = (p[:, :, None] * q[:, None, :]).sum(axis=0) - np.outer(sp, sq) / n
    cs, ct = s_ref + sp / n, t_ref + sq / n
    Tn, gap, norm = horn(S, cs, ct)
    if not np.isfinite(Tn).all():
        return None, None, None, None, None
    return Tn, gap, norm, cs, ct


def tile_sum(values):
    """the float64 sum in the order of the rule: tiles of 256, within each 64 a balanced tree over adjacent pairs, the four 64s left to
    right, the tiles in ascending order"""
    v = np.asarray(values, np.float64)
    v = np.concatenate([v, np.zeros(-len(v) % 256)]).reshape(-1, 4, 64)
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    v = v[..., 0]
    total = 0.0
    for row in ((v[:, 0] + v[:, 1]) + v[:, 2]) + v[:, 3]:
        total = total + row
    return float(total)


def final(s, t, T, distance_threshold):
    """the outputs under the final transform -> (inlier bool [m], n_inliers, fitness, rmse)"""
    d2 = distances2(s, t, to_f32(T))[0]
    inl = d2 < threshold2(distance_threshold)
    n = int(inl.sum())
    rmse = float(np.sqrt(np.float64(tile_sum(np.where(inl, d2.astype(np.float64), 0.0))) / n)) if n else 0.0
    return inl, n, n / len(s), rmse


def register(src, dst, pairs, distance_threshold, edge_similarity=0.9, num_hypotheses=4096, refine_rounds=2, min_inliers=3, top_k=0, seed=0):
    """the whole call -> dict(T, found, inlier, top, stats, counts, hyp, samples)"""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    m = len(pairs)
    st = dict(n_pairs=0, n_degenerate=0, n_rejected=0, n_scored=0, best=0, best_count=0, n_inliers=0, found=0, rounds_done=0, fitness=0.0, rmse=0.0, n_top=0)
    out = dict(T=np.eye(4), found=0, inlier=np.zeros(m, bool), top=[], stats=st, counts=None, hyp=None, samples=None)
    if m < 3 or len(src) == 0 or len(dst) == 0:
        return out
    s, t = pack(src, dst, pairs)
    idx = samples(seed, num_hypotheses, m)
    hyp = hypotheses_from_samples(s, t, idx, edge_similarity)
    counts = score(s, t, to_f32(hyp["T"]), distance_threshold)
    best, count, found = choose(counts, min_inliers)
    st.update(n_pairs=m, n_degenerate=int((hyp["status"] == 1).sum()), n_rejected=int((hyp["status"] == 2).sum()), n_scored=int((hyp["status"] == 0).sum()),
              best=best, best_count=count, found=found)
    out.update(counts=counts, hyp=hyp, samples=idx, top=top(counts, hyp["status"], hyp["T"], top_k))
    st["n_top"] = len(out["top"])
    if not found:
        return out
    T = hyp["T"][best].copy()
    s_ref, t_ref = s[idx[best, 0]].astype(np.float64), t[idx[best, 0]].astype(np.float64)
    for _ in range(refine_rounds):
        Tn = refit_once(s, t, T, distance_threshold, s_ref, t_ref)[0]
        if Tn is None:
            break
        T = Tn
        st["rounds_done"] += 1
    inl, n, fit, rmse = final(s, t, T, distance_threshold)
    st.update(n_inliers=n, fitness=fit, rmse=rmse)
    out.update(T=T, found=1, inlier=inl)
    return out


# ------------------------------------------------------------------ the workhorse fixture of the tests
def rot_z(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def pose(yaw_deg=140.0, translation=(7.0, -9.0, 3.6)):
    """the known pose of the fixtures: 140 degrees of yaw and 12 m of translation (7^2 + 9^2 + 3.6^2 = 142.96)"""
    T = np.eye(4)
    T[:3, :3] = rot_z(yaw_deg)
    T[:3, 3] = translation
    return T


def workhorse(m=3000, true_share=0.25, sigma=0.01, seed=7, T=None):
    """m pairs (k, k) of two clouds of m points: the first true_share of them (shuffled into place) true pairs under the pose with
    sigma noise on the target, the rest random against random -> (src, dst float32 [m, 3], pairs int32 [m, 2], truth bool [m], T)"""
    T = pose() if T is None else T
    rng = np.random.default_rng(seed)
    src = rng.uniform(-10, 10, (m, 3))
    dst = rng.uniform(-10, 10, (m, 3)) + T[:3, 3]
    truth = np.zeros(m, bool)
    truth[rng.permutation(m)[:int(round(m * true_share))]] = True
    src32 = src.astype(np.float32)
    dst[truth] = src32[truth].astype(np.float64) @ T[:3, :3].T + T[:3, 3] + rng.normal(0, sigma, (int(truth.sum()), 3))
    pairs = np.stack([np.arange(m), np.arange(m)], axis=1).astype(np.int32)
    return src32, dst.astype(np.float32), pairs, truth, T


def dyadic(m=512, true_share=0.25, seed=11):
    """the noise-free variant: integer coordinates, a quarter turn about z and a dyadic translation, so that every true pair is
    mapped exactly by every all-true hypothesis -> as workhorse"""
    T = np.eye(4)
    T[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [8.0, -4.0, 0.5]
    rng = np.random.default_rng(seed)
    src = rng.integers(-64, 64, (m, 3)).astype(np.float64)
    dst = rng.integers(-64, 64, (m, 3)).astype(np.float64)
    truth = np.zeros(m, bool)
    truth[rng.permutation(m)[:int(round(m * true_share))]] = True
    dst[truth] = src[truth] @ T[:3, :3].T + T[:3, 3]
    pairs = np.stack([np.arange(m), np.arange(m)], axis=1).astype(np.int32)
    return src.astype(np.float32), dst.astype(np.float32), pairs, truth, T
