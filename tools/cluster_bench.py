#!/usr/bin/env python3
"""Clustering (sf_map_cluster_euclidean, sf_map_cluster_dbscan) on a city surface map with scattered points and parked cars, beside
its yardstick in the same process: the radius filter (sf_map_radius_outliers, one walk of k_radius_count) at the same radius.  The
Euclidean form does one such walk (the hooking), DBSCAN three (count, hook, border); the streaming passes come on top.  The map is
tools/outlier_bench.py's -- synth.sample_city on synth.make_city (the extent scaled to keep city_bench's density) plus the surfaces of
--cars car-sized boxes placed as city_bench --dynamic-boxes places them, voxel-filtered at 0.1 m, plus 0.5 % points scattered
uniformly over the bounding box; the index cell is 0.25 m.  Every leg is warmed up once, then the legs alternate --reps times; the
times are device events around the kernel launches (sf_map_profile_launches), medians reported.  One JSON line per leg, then one with
the ratios and with what sf_cloud_filter_clusters(0.25, min_size = 50) did: the share of the scattered and of the car points removed
and of the surface points kept on the whole map, where the cars stand on the ground and belong to its piece; and what the same call
with max_size = --car-max-size extracts from the map less its ground (z > 0.15 m), where the cars stand alone: the share of the car,
surface and scattered points among what it keeps.  The lines go to stdout and to --out.
   python tools/cluster_bench.py [--map-points 2000000] [--reps 3] [--out profiles/cluster_bench.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_sensor_fusion_amd import api, synth  # noqa: E402


def shares(kept_idx, n_surface, n_cars, n_total):
    kept = np.zeros(n_total, bool)
    kept[kept_idx] = True
    a, b = n_surface, n_surface + n_cars
    return dict(surface_kept=float(kept[:a].mean()), cars_removed=float(1.0 - kept[a:b].mean()) if n_cars else 0.0,
                scattered_removed=float(1.0 - kept[b:].mean()) if n_total > b else 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=2_000_000)
    ap.add_argument("--cell", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--euclidean", type=float, nargs="*", default=[0.25, 0.4])
    ap.add_argument("--dbscan", nargs="*", default=["0.25:5", "0.4:10"], help="eps:min_points")
    ap.add_argument("--cars", type=int, default=40)
    ap.add_argument("--scattered", type=float, default=0.005, help="scattered points as a share of the surface points")
    ap.add_argument("--filter-tolerance", type=float, default=0.25)
    ap.add_argument("--filter-min-size", type=int, default=50)
    ap.add_argument("--car-max-size", type=int, default=5000)
    ap.add_argument("--skip-filter", action="store_true", help="only the timed legs (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_bench.jsonl"))
    args = ap.parse_args()
    ctx = api.Context(0)
    extent = 240.0 * float(np.sqrt(args.map_points / 10_000_000))
    boxes = synth.make_city(extent, max(1, int(120 * (extent / 240.0) ** 2)))
    cars = synth.make_cars(boxes, [(0.0, 0.0)], args.cars, radius=(3.0, 20.0)) if args.cars > 0 else np.zeros((0, 6))

    def area(bx, ground):
        dx, dy, dz = bx[:, 3] - bx[:, 0], bx[:, 4] - bx[:, 1], bx[:, 5]
        return float(ground + (dx * dy + 2 * dy * dz + 2 * dx * dz).sum())

    def voxelised(raw):
        c = api.Cloud(ctx, raw)
        c.voxel_downsample(0.1, "pcl")
        out = c.download()
        c.close()
        return out

    surface = voxelised(synth.sample_city(boxes, extent, args.map_points))
    n_car_raw = int(round(args.map_points * area(cars, 0.0) / area(boxes, extent * extent))) if len(cars) else 0   # the same density
    car_pts = voxelised(synth.sample_city(cars, 0.0, n_car_raw, seed=synth.CITY_SEED + 5)) if n_car_raw else np.zeros((0, 3), np.float32)
    n_surface, n_cars = len(surface), len(car_pts)
    rng = np.random.default_rng(17)
    lo, hi = surface.min(0), surface.max(0)
    scattered = rng.uniform(lo, hi, (int(round(args.scattered * n_surface)), 3)).astype(np.float32)
    pts = np.concatenate([surface, car_pts, scattered])
    del surface
    mp = api.Map(ctx, api.Cloud(ctx, pts), args.cell)
    cell, dims = mp.cell_size()
    mp.profile_launches(True)
    dbscan = [(float(s.split(":")[0]), int(s.split(":")[1])) for s in args.dbscan]
    radii = sorted(set(args.euclidean) | {e for e, _ in dbscan})
    legs = [("euclidean", (t,)) for t in args.euclidean] + [("dbscan", p) for p in dbscan] + [("radius", (r,)) for r in radii]
    times = {leg: [] for leg in legs}
    did = {}
    for rep in range(args.reps + 1):                                  # rep 0: the warm-up of every leg
        for leg in legs:
            kind, arg = leg
            if kind == "euclidean":
                st = mp.cluster_euclidean(arg[0])[2]
            elif kind == "dbscan":
                st = mp.cluster_dbscan(*arg)[2]
            else:
                st = mp.radius_outliers(arg[0], 0)[2]
            if rep > 0:
                times[leg].append(mp.last_launch_ms())
            else:
                did[leg] = st
    ms = {leg: float(np.median(t)) for leg, t in times.items()}
    common = dict(surface_points=n_surface, car_points=n_cars, cars=len(cars), scattered_points=len(scattered), extent_m=extent, cell_m=cell, grid=list(dims),
                  reps=args.reps, device=ctx.device_name())
    lines = []
    for leg in legs:
        kind, arg = leg
        out = dict(leg=kind, arg=list(arg), kernel_ms=ms[leg], kernel_ms_all=[round(t, 3) for t in times[leg]], points_per_s=len(pts) / (ms[leg] * 1e-3))
        if kind != "radius":
            out["stats"] = did[leg]
        lines.append(dict(out, **common))
    ratios = {}
    for t in args.euclidean:
        ratios["euclidean_%g_over_radius_%g" % (t, t)] = ms[("euclidean", (t,))] / ms[("radius", (t,))]
    for e, k in dbscan:
        ratios["dbscan_%g_%d_over_radius_%g" % (e, k, e)] = ms[("dbscan", (e, k))] / ms[("radius", (e,))]
    filt = None
    if not args.skip_filter:                                          # what the filter does
        tol, min_size = args.filter_tolerance, args.filter_min_size
        cloud = api.Cloud(ctx, pts)
        st = cloud.filter_clusters(tol, min_size, 0, args.cell)
        whole = dict(shares(cloud.last_indices(), n_surface, n_cars, len(pts)), stats=st)
        cloud.close()
        up = np.flatnonzero(pts[:, 2] > 0.15)
        cloud = api.Cloud(ctx, pts[up])
        st = cloud.filter_clusters(tol, min_size, args.car_max_size, args.cell)
        above = np.zeros(len(pts), bool)
        above[up] = True
        kept = np.zeros(len(pts), bool)
        kept[up[cloud.last_indices()]] = True
        a, b = n_surface, n_surface + n_cars
        # what stays are the pieces of min_size .. max_size points: the cars, should they stand alone once the ground is gone
        objects = dict(points=int(len(up)), max_size=args.car_max_size, car_points_kept=float(kept[a:b][above[a:b]].mean()) if above[a:b].any() else 0.0,
                       surface_points_kept=float(kept[:a][above[:a]].mean()), scattered_points_kept=float(kept[b:][above[b:]].mean()) if above[b:].any() else 0.0, stats=st)
        cloud.close()
        filt = dict(tolerance=tol, min_size=min_size, whole_map=whole, objects_without_ground=objects)
    lines.append(dict(leg="ratios", **ratios, filter=filt, **common))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
