#!/usr/bin/env python3
"""CPU proxy for stage 0 of the neighbour-table look-up (the nearest gap; DESIGN section 3, profiles/LADDER.md round 8): what
share of the queries whose cached neighbour is tried would the one-float test settle, launch by launch?  numpy and scipy only.

A `synth.make_map` at the benchmark's density, voxel-filtered at 0.1 m (voxel centroids); one `synth.make_scan` from the identity
prior; point-to-plane Gauss-Newton with a 0.5 m acceptance radius against normals from the 0.25 m neighbourhood (estimated for
the map points that are ever a neighbour).  Per launch index: the pose error before it, the distance dp from each query to the
PREVIOUS launch's neighbour, the share whose nearest neighbour is unchanged, the share that passes
2 dp 1.0001 + 2e-6 < min(g1, 0.25) 0.9999 (g1: distance from the cached point to its nearest other map point), the share the
table's rule serves with r4 (the fourth nearest other point's distance) and with r (the seventh's), and the failing lanes per wave
of 64.  Every query is counted as tried (on the device only those whose box-bound certificate failed are).
   python tools/probes/nearest_gap_proxy.py [--map-points 1000000] [--scan-points 100000] [--launches 5]"""
import argparse
import os
import sys

import numpy as np
from scipy.spatial import cKDTree

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from slam_sensor_fusion_amd import synth  # noqa: E402


def voxel_centroids(p, leaf):
    key = np.floor(p.astype(np.float64) / leaf).astype(np.int64)
    key -= key.min(0)
    dims = key.max(0) + 1
    flat = (key[:, 2] * dims[1] + key[:, 1]) * dims[0] + key[:, 0]
    _, inv, cnt = np.unique(flat, return_inverse=True, return_counts=True)
    out = np.zeros((len(cnt), 3))
    np.add.at(out, inv, p.astype(np.float64))
    return (out / cnt[:, None]).astype(np.float32)


def normals_of(tree, pts, idx, radius):
    out = np.zeros((len(idx), 3))
    for k, nb in enumerate(tree.query_ball_point(pts[idx], radius)):
        if len(nb) >= 3:
            q = pts[nb].astype(np.float64)
            w, v = np.linalg.eigh(np.cov(q.T))
            out[k] = v[:, 0]
    return out


def gauss_newton_step(T, src, tgt, nrm):
    y = src @ T[:3, :3].T + T[:3, 3]
    r = ((y - tgt) * nrm).sum(1)
    J = np.concatenate([np.cross(y, nrm), nrm], axis=1)
    x = np.linalg.solve(J.T @ J, -J.T @ r)
    a, b, c = x[:3]
    dR = synth.rpy_to_R(a, b, c)
    D = np.eye(4)
    D[:3, :3] = dR
    D[:3, 3] = x[3:]
    return D @ T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=1_000_000)
    ap.add_argument("--scan-points", type=int, default=100_000)
    ap.add_argument("--launches", type=int, default=5)
    args = ap.parse_args()
    ds = voxel_centroids(synth.make_map(args.map_points), 0.1)
    tree = cKDTree(ds)
    d8, _ = tree.query(ds, 8)                      # self, then the seven nearest others
    g1, r4, r7 = d8[:, 1], d8[:, 4], d8[:, 7]
    print("map %d points; g1 median %.3f m, 5 %% quantile %.3f m" % (len(ds), np.median(g1), np.quantile(g1, 0.05)))
    scan = synth.make_scan(ds, args.scan_points)[0].astype(np.float64)
    truth = synth.t_true()
    T = np.eye(4)
    ncache = {}
    prev = None
    print("| launch index | pose error before it | dp median / p90 | NN unchanged | gap test passes | table rule (r4 / r) serves | failing lanes per wave of 64 | passed with a changed neighbour |")
    print("|---|---|---|---|---|---|---|---|")
    for launch in range(args.launches):
        y = scan @ T[:3, :3].T + T[:3, 3]
        d, j = tree.query(y)
        if prev is not None:
            dp = np.linalg.norm(y - ds[prev], axis=1)
            gap = 2 * dp * 1.0001 + 2e-6 < np.minimum(g1[prev], 0.25) * 0.9999
            # the table's rule with the true winner among the listed points (d: the distance to the nearest of all points)
            s4 = (dp + d) * 1.0001 + 2e-6 < np.minimum(r4[prev], 0.25) * 0.9999
            s7 = (dp + d) * 1.0001 + 2e-6 < np.minimum(r7[prev], 0.25) * 0.9999
            print("| %d | %.1f mm | %.1f / %.1f mm | %.3f | %.3f | %.3f / %.3f | %.1f | %d |" % (
                launch, 1e3 * synth.pose_error(T, truth)[0], 1e3 * np.median(dp), 1e3 * np.quantile(dp, 0.9), (j == prev).mean(), gap.mean(), s4.mean(), s7.mean(),
                64 * (1 - gap.mean()), int((gap & (j != prev)).sum())))
        ok = d < 0.5
        need = np.setdiff1d(np.unique(j[ok]), np.fromiter(ncache.keys(), np.int64, len(ncache)))
        for k, n in zip(need, normals_of(tree, ds, need, 0.25)):
            ncache[int(k)] = n
        nrm = np.array([ncache[int(k)] for k in j[ok]])
        T = gauss_newton_step(T, scan[ok], ds[j[ok]].astype(np.float64), nrm)
        prev = j


if __name__ == "__main__":
    main()
