#!/usr/bin/env python3
"""The outlier filters (sf_map_statistical_outliers, sf_map_radius_outliers) on a city surface map with scattered points, beside
their yardsticks in the same process: the k-NN normals at k = 21 (the same search plus point loads and a Jacobi solve) for the
statistical filter at k = 20, and the radius normals (the same walk twice, in float64, plus the solve) at the same radius for the
radius filter.  The map is synth.sample_city on synth.make_city (the extent scaled to keep city_bench's density), voxel-filtered at
0.1 m, plus 0.5 % points scattered uniformly over its bounding box; the index cell is 0.25 m.  Every leg is warmed up once, then the
legs alternate --reps times; the times are device events around the kernel launches (sf_map_profile_launches), medians reported.
One JSON line per leg, then one with the ratios and with what the filters did: the share of the scattered points removed and of the
surface points kept.  The lines go to stdout and to --out.
   python tools/outlier_bench.py [--map-points 2000000] [--reps 3] [--out profiles/outlier_bench.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_sensor_fusion_amd import api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=2_000_000)
    ap.add_argument("--cell", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--std-ratio", type=float, default=2.0)
    ap.add_argument("--radii", type=float, nargs="*", default=[0.25, 0.4])
    ap.add_argument("--min-neighbors", type=int, default=5)
    ap.add_argument("--scattered", type=float, default=0.005, help="scattered points as a share of the surface points")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outlier_bench.jsonl"))
    args = ap.parse_args()
    ctx = api.Context(0)
    extent = 240.0 * float(np.sqrt(args.map_points / 10_000_000))
    boxes = synth.make_city(extent, max(1, int(120 * (extent / 240.0) ** 2)))
    cloud = api.Cloud(ctx, synth.sample_city(boxes, extent, args.map_points))
    cloud.voxel_downsample(0.1, "pcl")
    surface = cloud.download()
    n_surface = len(surface)
    rng = np.random.default_rng(17)
    lo, hi = surface.min(0), surface.max(0)
    scattered = rng.uniform(lo, hi, (int(round(args.scattered * n_surface)), 3)).astype(np.float32)
    pts = np.concatenate([surface, scattered])
    del surface
    mp = api.Map(ctx, api.Cloud(ctx, pts), args.cell)
    cell, dims = mp.cell_size()
    mp.profile_launches(True)
    legs = [("statistical_pcl", args.k), ("statistical_o3d", args.k), ("normals_knn", args.k + 1)]
    legs += [("radius", r) for r in args.radii] + [("normals_radius", r) for r in args.radii]
    times = {leg: [] for leg in legs}
    did = {}
    for rep in range(args.reps + 1):                                  # rep 0: the warm-up of every leg
        for leg in legs:
            kind, arg = leg
            if kind.startswith("statistical"):
                keep, _, st = mp.statistical_outliers(arg, args.std_ratio, kind[-3:])
            elif kind == "radius":
                keep, _, st = mp.radius_outliers(arg, args.min_neighbors)
            elif kind == "normals_knn":
                mp.estimate_normals_knn(arg)
            else:
                mp.estimate_normals(arg)
            if rep > 0:
                times[leg].append(mp.last_launch_ms())
            elif kind.startswith("statistical") or kind == "radius":
                did[leg] = dict(stats=st, scattered_removed=float(1.0 - keep[n_surface:].mean()), surface_kept=float(keep[:n_surface].mean()))
    ms = {leg: float(np.median(t)) for leg, t in times.items()}
    common = dict(surface_points=n_surface, scattered_points=len(scattered), extent_m=extent, cell_m=cell, grid=list(dims), reps=args.reps, device=ctx.device_name())
    lines = []
    for leg in legs:
        kind, arg = leg
        out = dict(leg=kind, arg=arg, kernel_ms=ms[leg], kernel_ms_all=[round(t, 3) for t in times[leg]], points_per_s=len(pts) / (ms[leg] * 1e-3))
        if leg in did:
            out.update(did[leg])
            if kind == "radius":
                out["min_neighbors"] = args.min_neighbors
            else:
                out["std_ratio"] = args.std_ratio
        lines.append(dict(out, **common))
    ratios = {"statistical_pcl%d_over_normals_knn%d" % (args.k, args.k + 1): ms[("statistical_pcl", args.k)] / ms[("normals_knn", args.k + 1)],
              "statistical_o3d%d_over_normals_knn%d" % (args.k, args.k + 1): ms[("statistical_o3d", args.k)] / ms[("normals_knn", args.k + 1)]}
    for r in args.radii:
        ratios["radius_%g_over_normals_radius_%g" % (r, r)] = ms[("radius", r)] / ms[("normals_radius", r)]
    lines.append(dict(leg="ratios", **ratios, **common))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
