#!/usr/bin/env python3
"""Exact k-NN (sf_map_knn) and k-NN map normals (sf_map_estimate_normals_knn) at the bench's map size, beside their yardsticks
in the same process: Map.nn for the same queries, and the radius normals at 0.25 m and 0.4 m.  The map is the bench's
(--map-points raw points, voxel 0.1 m, index cell 0.25 m), the queries are synth.make_scan of it.  Every shape is warmed up
once, then the legs alternate --reps times; the times are device events around the kernel launches (sf_map_profile_launches:
no upload, no download), medians reported.  One JSON line per leg, then one with the ratios.
The bytes figure is a MODEL, not a measurement: per query 12 B + (8 k + 4) B of result + 16 B per map point of the cells of the
block the exactness certificate needs -- (2 R + 1)^3 cells, R = max(1, ceil(r_k / cell)), r_k the query's k-th neighbour distance,
at the map's mean points per cell -- read once per wave (a wave serves one query at a time), over the kernel time, against 8 TB/s.
   python tools/knn_bench.py [--map-points 10000000] [--queries 1000000] [--reps 3]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slam_sensor_fusion_amd import api, synth  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--cell", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ks", type=int, nargs="*", default=[1, 8, 20, 32, 64])
    ap.add_argument("--normals-ks", type=int, nargs="*", default=[10, 20, 30])
    ap.add_argument("--normals-radii", type=float, nargs="*", default=[0.25, 0.4])
    args = ap.parse_args()
    ctx = api.Context(0)
    cloud = api.Cloud(ctx, synth.make_map(args.map_points))
    cloud.voxel_downsample(0.1, "pcl")
    ds = cloud.download()
    mp = api.Map(ctx, cloud, args.cell)
    cell, dims = mp.cell_size()
    n_map = len(mp)
    per_cell = n_map / float(np.prod([float(d) for d in dims]))
    q = synth.make_scan(ds, args.queries)[0]
    del ds
    mp.profile_launches(True)
    legs = [("nn", None)] + [("knn", k) for k in args.ks] + [("normals_radius", r) for r in args.normals_radii] + [("normals_knn", k) for k in args.normals_ks]
    times = {leg: [] for leg in legs}
    model = {}
    for rep in range(args.reps + 1):                                  # rep 0: the warm-up of every shape
        for leg in legs:
            kind, arg = leg
            if kind == "nn":
                mp.nn(q)
            elif kind == "knn":
                _, d2, cnt = mp.knn(q, arg)
                if rep == 0:
                    rk = np.sqrt(d2[np.arange(len(q)), np.maximum(cnt, 1) - 1].astype(np.float64))
                    R = np.maximum(1, np.ceil(rk / cell))
                    model[leg] = dict(mean_rings=float(R.mean()), bytes_per_query=float(12 + 8 * arg + 4 + 16 * per_cell * np.mean((2 * R + 1) ** 3)),
                                      kth_distance_m_median=float(np.median(rk)), kth_distance_m_max=float(rk.max()))
                del d2, cnt
            elif kind == "normals_radius":
                mp.estimate_normals(arg)
            else:
                mp.estimate_normals_knn(arg)
            if rep > 0:
                times[leg].append(mp.last_launch_ms())
    ms = {leg: float(np.median(t)) for leg, t in times.items()}
    common = dict(map_points=n_map, cell_m=cell, grid=list(dims), mean_points_per_cell=per_cell, reps=args.reps, device=ctx.device_name())
    for leg in legs:
        kind, arg = leg
        n = len(q) if kind in ("nn", "knn") else n_map
        out = dict(leg=kind, arg=arg, queries=n, kernel_ms=ms[leg], kernel_ms_all=[round(t, 3) for t in times[leg]], queries_per_s=n / (ms[leg] * 1e-3))
        if leg in model:
            b = model[leg]["bytes_per_query"] * n
            out.update(model[leg], model_compulsory_bytes=b, model_fraction_of_8TBps=b / (ms[leg] * 1e-3) / PEAK_BYTES_PER_S)
        print(json.dumps(dict(out, **common)), flush=True)
    ratios = {}
    if ("knn", 1) in ms:
        ratios["knn_k1_over_nn"] = ms[("knn", 1)] / ms[("nn", None)]
    if ("normals_knn", 20) in ms and ("normals_radius", 0.4) in ms:
        ratios["normals_knn20_over_normals_radius_0.4"] = ms[("normals_knn", 20)] / ms[("normals_radius", 0.4)]
    if ("normals_knn", 20) in ms and ("normals_radius", 0.25) in ms:
        ratios["normals_knn20_over_normals_radius_0.25"] = ms[("normals_knn", 20)] / ms[("normals_radius", 0.25)]
    # what the radius forms hold on this map (the yardstick's neighbourhood sizes)
    for r in args.normals_radii:
        mp.estimate_normals(r)
        cnt = mp.download_normals()[1]
        ratios["radius_%g_neighbours_median" % r] = float(np.median(cnt))
        ratios["radius_%g_share_below_3" % r] = float((cnt < 3).mean())
    print(json.dumps(dict(leg="ratios", **ratios, **common)), flush=True)


if __name__ == "__main__":
    main()
