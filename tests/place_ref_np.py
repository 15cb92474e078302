"""The rule of the Scan Context descriptor, its distance and the top-k (include/slamfusion.h) restated in numpy from
the header text: float64, np.arctan2, the same expressions in the same order, every sum a loop over its index.  Nothing here calls
the library.

Parameters are a dict(num_rings, num_sectors, min_range, max_range, sensor_height) (api.PlaceDB.params); a pose is [4, 4] or [16]
row-major parent <- sensor, or None for the identity; a descriptor is float32 [num_rings, num_sectors]."""
import math

import numpy as np

PI = math.pi
STAT_KEYS = ("n_points", "n_nonfinite", "n_outside", "n_below", "n_binned", "n_filled")


def default_params(**over):
    p = dict(num_rings=20, num_sectors=60, min_range=0.5, max_range=80.0, sensor_height=2.0)
    p.update(over)
    return p


def project(points, pose, prm):
    """-> dict(finite, outside, below, binned bool [n]; rho, u, v, y float64 [n]; ring, col int64 [n]; hgt float32 [n])"""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    T = np.eye(4).reshape(16) if pose is None else np.asarray(pose, np.float64).reshape(16)
    Nr, Ns = int(prm["num_rings"]), int(prm["num_sectors"])
    finite = np.isfinite(pts).all(axis=1)
    p = np.where(finite[:, None], pts, np.float32(1.0)).astype(np.float64)
    d0, d1, d2 = p[:, 0] - T[3], p[:, 1] - T[7], p[:, 2] - T[11]
    x = (T[0] * d0 + T[4] * d1) + T[8] * d2
    y = (T[1] * d0 + T[5] * d1) + T[9] * d2
    z = (T[2] * d0 + T[6] * d1) + T[10] * d2
    h2 = x * x + y * y
    rho = np.sqrt(h2)
    az = np.arctan2(y, x)
    u = (az + PI) / (2 * PI) * Ns
    col = np.floor(u).astype(np.int64)
    col = np.where(col >= Ns, col - Ns, col)
    v = rho / prm["max_range"] * Nr
    ring = np.floor(v).astype(np.int64)
    hgt = (z + prm["sensor_height"]).astype(np.float32)
    outside = finite & (~(prm["min_range"] <= rho) | (ring >= Nr))
    below = finite & ~outside & (hgt <= 0)
    binned = finite & ~outside & ~below
    return dict(finite=finite, outside=outside, below=below, binned=binned, rho=rho, u=u, v=v, y=y, ring=ring, col=col, hgt=hgt)


def descriptor(points, pose, prm):
    """-> (float32 [Nr, Ns], stats dict)"""
    q = project(points, pose, prm)
    Nr, Ns = int(prm["num_rings"]), int(prm["num_sectors"])
    sel = np.flatnonzero(q["binned"])
    bits = np.zeros(Nr * Ns, np.uint32)                      # a positive float orders like its bits; +0 is all zero bits
    np.maximum.at(bits, q["ring"][sel] * Ns + q["col"][sel], q["hgt"][sel].view(np.uint32))
    desc = bits.view(np.float32).reshape(Nr, Ns)
    stats = dict(n_points=len(q["finite"]), n_nonfinite=int((~q["finite"]).sum()), n_outside=int(q["outside"].sum()), n_below=int(q["below"].sum()),
                 n_binned=int(q["binned"].sum()), n_filled=int((bits != 0).sum()))
    return desc, stats


def edge_distance(points, pose, prm):
    """How far the u of the points that reach the sector rule (binned ones) lies from an integer; points whose sensor-frame y is +-0 are
    left out (atan2 is exact there by definition).  v comes from IEEE operations and a correctly rounded sqrt alone."""
    q = project(points, pose, prm)
    du = np.abs(q["u"] - np.rint(q["u"]))[q["binned"] & (q["y"] != 0)]
    return float(du.min()) if len(du) else np.inf


def unit_columns(desc):
    """-> (u float64 [Nr, Ns], valid bool [Ns])"""
    a = np.asarray(desc, np.float32).astype(np.float64)
    total = np.zeros(a.shape[1])
    for i in range(a.shape[0]):                              # i ascending, from 0
        total = total + a[i] * a[i]
    n = np.sqrt(total)
    valid = n > 0
    u = np.where(valid[None, :], a / np.where(valid, n, 1.0)[None, :], 0.0)
    return u, valid


def shift_distances(UQ, VQ, UC, VC):
    """d(s) of every pair: UQ [Q, Nr, Ns], VQ [Q, Ns], UC [N, Nr, Ns], VC [N, Ns] -> float64 [Q, N, Ns].  The pairs and the shifts
    stand side by side in the arrays; the two sums of the rule are the two loops."""
    Q, Nr, Ns = UQ.shape
    N = len(UC)
    s_idx = np.arange(Ns)
    S, V = np.zeros((Q, N, Ns)), np.zeros((Q, N, Ns), np.int64)
    for j in range(Ns):                                      # j ascending
        jc = (j + s_idx) % Ns
        both = VQ[:, j][:, None, None] & VC[:, jc][None, :, :]
        cos = np.zeros((Q, N, Ns))
        for i in range(Nr):                                  # i ascending, multiply then add
            cos = cos + UQ[:, i, j][:, None, None] * UC[:, i, jc][None, :, :]
        S = np.where(both, S + cos, S)
        V = V + both
    return np.where(V > 0, 1.0 - S / np.maximum(V, 1), 1.0)


def distances(queries, entries):
    """-> (D float64 [Q, N], shift int32 [Q, N]): the minimum over the shifts and the smallest shift that attains it"""
    queries, entries = np.asarray(queries, np.float32), np.asarray(entries, np.float32)
    Q, N = len(queries), len(entries)
    if Q == 0 or N == 0:
        return np.zeros((Q, N)), np.zeros((Q, N), np.int32)
    uq, uc = [unit_columns(q) for q in queries], [unit_columns(c) for c in entries]
    d = shift_distances(np.stack([u for u, _ in uq]), np.stack([v for _, v in uq]), np.stack([u for u, _ in uc]), np.stack([v for _, v in uc]))
    sh = np.argmin(d, axis=2)                                # the first minimum: the smallest s
    return np.take_along_axis(d, sh[:, :, None], axis=2)[:, :, 0], sh.astype(np.int32)


def candidate_pose(T_entry, shift, num_sectors):
    """T_entry . Rz(shift 2 pi / Ns)"""
    ang = shift * (2 * PI / num_sectors)
    c, s = math.cos(ang), math.sin(ang)
    Rz = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
    return np.asarray(T_entry, np.float64).reshape(4, 4) @ Rz


def top_k(D, shift, k, poses=None, num_sectors=None):
    """-> dict(idx int32 [Q, k], dist float64 [Q, k], shift int32 [Q, k], poses float64 [Q, k, 4, 4] when entry poses are given)"""
    Q, N = D.shape
    idx, dist, sh = np.full((Q, k), -1, np.int32), np.full((Q, k), np.inf), np.zeros((Q, k), np.int32)
    out_poses = np.zeros((Q, k, 4, 4))
    for q in range(Q):
        order = sorted(range(N), key=lambda c: (D[q, c], c))[:k]
        for r, c in enumerate(order):
            idx[q, r], dist[q, r], sh[q, r] = c, D[q, c], shift[q, c]
            if poses is not None:
                out_poses[q, r] = candidate_pose(poses[c], int(shift[q, c]), num_sectors)
    return dict(idx=idx, dist=dist, shift=sh, poses=out_poses)
