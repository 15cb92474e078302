"""The rule of the range images and the visibility classes (include/slamfusion.h) restated in numpy from the header
text: float64, np.arctan2, the same expressions in the same order.  Nothing here calls the library.

An image's parameters are a dict(width, height, el_min, el_max, min_range, max_range) (api.RangeImage.params); a pose is [4, 4] or
[16] row-major parent <- sensor, or None for the identity; the window and margins are a dict(half_cols, half_rows, min_hits,
range_margin, range_ratio)."""
import math

import numpy as np

PI = math.pi
OUTSIDE, UNKNOWN, WITHIN, OCCLUDED, SEEN_THROUGH = 0, 1, 2, 3, 4
DEFAULT_WINDOW = dict(half_cols=1, half_rows=1, min_hits=1, range_margin=0.2, range_ratio=0.01)


def default_params(**over):
    p = dict(width=2048, height=64, el_min=-25.0 * PI / 180.0, el_max=3.0 * PI / 180.0, min_range=0.5, max_range=120.0)
    p.update(over)
    return p


def window(**over):
    w = dict(DEFAULT_WINDOW)
    w.update(over)
    return w


def project(points, pose, prm):
    """-> dict(finite, inside bool [n]; r, u, v, y float64 [n]; row, col int64 [n] (meaningful where inside))"""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    T = np.eye(4).reshape(16) if pose is None else np.asarray(pose, np.float64).reshape(16)
    finite = np.isfinite(pts).all(axis=1)
    p = np.where(finite[:, None], pts, np.float32(1.0)).astype(np.float64)
    d0, d1, d2 = p[:, 0] - T[3], p[:, 1] - T[7], p[:, 2] - T[11]
    x = (T[0] * d0 + T[4] * d1) + T[8] * d2
    y = (T[1] * d0 + T[5] * d1) + T[9] * d2
    z = (T[2] * d0 + T[6] * d1) + T[10] * d2
    h2 = x * x + y * y
    r = np.sqrt(h2 + z * z)
    az = np.arctan2(y, x)
    el = np.arctan2(z, np.sqrt(h2))
    W, H = int(prm["width"]), int(prm["height"])
    u = (az + PI) / (2 * PI) * W
    col = np.floor(u).astype(np.int64)
    col = np.where(col >= W, col - W, col)
    v = (el - prm["el_min"]) / (prm["el_max"] - prm["el_min"]) * H
    row = np.floor(v).astype(np.int64)
    in_range = (r > 0) & (prm["min_range"] <= r) & (r <= prm["max_range"])
    inside = finite & ~((v < 0) | (row >= H) | ~in_range)
    return dict(finite=finite, inside=inside, r=r, u=u, v=v, y=y, row=row, col=col, in_range=finite & in_range)


def build(points, pose, prm):
    """-> (range float32 [H, W] (+inf: empty), index int32 [H, W] (-1: empty), stats dict)"""
    q = project(points, pose, prm)
    W, H = int(prm["width"]), int(prm["height"])
    sel = np.flatnonzero(q["inside"])
    bits = q["r"][sel].astype(np.float32).view(np.uint32).astype(np.uint64)
    key = (bits << np.uint64(32)) | sel.astype(np.uint64)
    keys = np.full(H * W, np.uint64(0xFFFFFFFFFFFFFFFF))
    np.minimum.at(keys, q["row"][sel] * W + q["col"][sel], key)
    filled = keys != np.uint64(0xFFFFFFFFFFFFFFFF)
    rng = np.where(filled, (keys >> np.uint64(32)).astype(np.uint32), np.uint32(0x7F800000)).astype(np.uint32).view(np.float32)
    idx = np.where(filled, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    n = len(q["finite"])
    stats = dict(n_points=n, n_projected=int(q["inside"].sum()), n_outside=int((q["finite"] & ~q["inside"]).sum()), n_nonfinite=int((~q["finite"]).sum()),
                 n_filled=int(filled.sum()))
    return rng.reshape(H, W), idx.reshape(H, W), stats


def classify(points, pose, prm, image, win=None):
    """The class of every point against one image = (range [H, W], index [H, W]) built with prm -> uint8 [n]."""
    win = window() if win is None else win
    rng, idx = image
    q = project(points, pose, prm)
    W, H = int(prm["width"]), int(prm["height"])
    n = len(q["finite"])
    row, col = np.where(q["inside"], q["row"], 0), np.where(q["inside"], q["col"], 0)
    n_hit = np.zeros(n, np.int64)
    r_near, r_far = np.full(n, np.inf, np.float32), np.full(n, -np.inf, np.float32)
    for dr in range(-min(win["half_rows"], H), min(win["half_rows"], H) + 1):
        rr = row + dr
        ok = (rr >= 0) & (rr < H)
        rr = np.clip(rr, 0, H - 1)
        for dc in range(-win["half_cols"], win["half_cols"] + 1):
            cc = (col + dc) % W
            hit = ok & (idx[rr, cc] >= 0)
            f = rng[rr, cc]
            n_hit += hit
            r_near = np.where(hit & (f < r_near), f, r_near)
            r_far = np.where(hit & (f > r_far), f, r_far)
    r = q["r"]
    margin = win["range_margin"] + win["range_ratio"] * r
    cls = np.full(n, WITHIN, np.uint8)
    with np.errstate(invalid="ignore"):
        occluded = r - margin > r_far.astype(np.float64)
        seen = r + margin < r_near.astype(np.float64)
    cls[occluded] = OCCLUDED
    cls[seen] = SEEN_THROUGH
    cls[n_hit < win["min_hits"]] = UNKNOWN
    cls[~q["inside"]] = OUTSIDE
    return cls


def class_stats(cls_list, n_valid):
    """The statistics of a call from the classes of its images (n_removed apart)."""
    c = np.concatenate([np.asarray(k).reshape(-1) for k in cls_list]) if len(cls_list) else np.zeros(0, np.uint8)
    n = len(cls_list[0]) if len(cls_list) else 0
    return dict(n_points=n, n_valid=int(n_valid), n_outside=int((c == OUTSIDE).sum()), n_unknown=int((c == UNKNOWN).sum()), n_within=int((c == WITHIN).sum()),
                n_occluded=int((c == OCCLUDED).sum()), n_seen_through=int((c == SEEN_THROUGH).sum()))


def votes(points, images, poses, win=None):
    """images: a list of (prm, (range, index)); poses [B] or None -> (seen_through uint16 [n], within uint16 [n], the classes [B][n])"""
    n = len(np.asarray(points).reshape(-1, 3))
    seen, within, all_cls = np.zeros(n, np.uint16), np.zeros(n, np.uint16), []
    for b, (prm, image) in enumerate(images):
        cls = classify(points, None if poses is None else poses[b], prm, image, win)
        seen += cls == SEEN_THROUGH
        within += cls == WITHIN
        all_cls.append(cls)
    return seen, within, all_cls


def remove_mask(seen, within, min_seen=1, max_within=0):
    """True where sf_cloud_remove_seen_through takes the point away."""
    return (seen >= min_seen) & (within <= max_within)


def edge_distance(points, pose, prm):
    """How far the u and v of the points that pass the range test lie from an integer: (min over u, min over v).  Points whose
    sensor-frame y is +-0 are left out of u (atan2 is exact there by definition)."""
    q = project(points, pose, prm)
    sel = q["in_range"]
    du = np.abs(q["u"] - np.rint(q["u"]))[sel & (q["y"] != 0)]
    dv = np.abs(q["v"] - np.rint(q["v"]))[sel]
    return (float(du.min()) if len(du) else np.inf), (float(dv.min()) if len(dv) else np.inf)
