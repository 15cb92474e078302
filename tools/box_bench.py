#!/usr/bin/env python3
"""Per-label boxes (sf_cloud_label_boxes, sf_cloud_cluster_boxes) and multi-box removal (sf_cloud_remove_boxes) on the map of
tools/cluster_bench.py -- synth.sample_city on synth.make_city plus the surfaces of --cars car-sized boxes, voxel-filtered at 0.1 m,
plus 0.5 % scattered points -- with the ground removed as DESIGN section 15 does (z > 0.15 m), so that the cars stand alone.
Legs, each warmed up once, then --reps alternating repetitions, medians:
  label_boxes     device events from the first to the last kernel (profile = True: the label upload is not in it), the labels those of
                  sf_map_cluster_euclidean(0.25, 50, --car-max-size), per mode;
  crop_aabb       the yardstick, one streaming pass with its compaction: sf_cloud_crop_aabb of the same cloud (a box that holds every
                  point), host time of the call with the context drained before it.  The mark is `passes` times it: the passes
                  label_boxes makes over the cloud's points -- the keys, two per sort pass (histogram, scatter), the three segmented ones;
  cluster_boxes   beside sf_cloud_filter_clusters with the same arguments, host time of either call on its own copy of the cloud
                  (the difference should be near the label_boxes time);
  remove_boxes    with the recovered boxes, beside one sf_cloud_crop_obb call per box on copies of the cloud, host times.
Then what the boxes are: per car the recovered extents (descending) against the placed 4.5 x 1.8 x 1.5 m, and how many car, building
and scattered points remove_boxes(margin = 0.1) takes from the FULL map.  One JSON line per leg and one summary; stdout and --out.
   python tools/box_bench.py [--map-points 2000000] [--reps 5] [--out profiles/box_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_sensor_fusion_amd import api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=2_000_000)
    ap.add_argument("--cell", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cars", type=int, default=40)
    ap.add_argument("--scattered", type=float, default=0.005)
    ap.add_argument("--tolerance", type=float, default=0.25)
    ap.add_argument("--min-size", type=int, default=50)
    ap.add_argument("--car-max-size", type=int, default=5000)
    ap.add_argument("--modes", nargs="*", default=["pca", "upright", "aabb"])
    ap.add_argument("--skip-summary", action="store_true", help="only the timed legs (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_bench.jsonl"))
    args = ap.parse_args()
    ctx = api.Context(0)
    extent = 240.0 * float(np.sqrt(args.map_points / 10_000_000))
    city = synth.make_city(extent, max(1, int(120 * (extent / 240.0) ** 2)))
    cars = synth.make_cars(city, [(0.0, 0.0)], args.cars, radius=(3.0, 20.0))

    def area(bx, ground):
        dx, dy, dz = bx[:, 3] - bx[:, 0], bx[:, 4] - bx[:, 1], bx[:, 5]
        return float(ground + (dx * dy + 2 * dy * dz + 2 * dx * dz).sum())

    def voxelised(raw):
        c = api.Cloud(ctx, raw)
        c.voxel_downsample(0.1, "pcl")
        out = c.download()
        c.close()
        return out

    surface = voxelised(synth.sample_city(city, extent, args.map_points))
    n_car_raw = int(round(args.map_points * area(cars, 0.0) / area(city, extent * extent)))
    car_pts = voxelised(synth.sample_city(cars, 0.0, n_car_raw, seed=synth.CITY_SEED + 5))
    n_surface, n_cars = len(surface), len(car_pts)
    rng = np.random.default_rng(17)
    scattered = rng.uniform(surface.min(0), surface.max(0), (int(round(args.scattered * n_surface)), 3)).astype(np.float32)
    full = np.concatenate([surface, car_pts, scattered])
    del surface
    objs = full[full[:, 2] > 0.15]                                    # the ground removed as section 15 does
    src = api.Cloud(ctx, objs)
    mp = api.Map(ctx, src, args.cell)
    labels, sizes, cst = mp.cluster_euclidean(args.tolerance, args.min_size, args.car_max_size)
    mp.close()
    n_labels = len(sizes)
    sort_passes = -(-max(int(n_labels).bit_length(), 1) // 8)          # keys 0 .. n_labels
    passes = 1 + 2 * sort_passes + 3
    lo, hi = objs.min(0).astype(np.float64) - 1.0, objs.max(0).astype(np.float64) + 1.0
    work = api.Cloud(ctx, objs)

    def host_ms(call, fresh=True):
        if fresh:
            work.copy_from(src)
        ctx.synchronize()
        t0 = time.perf_counter()
        out = call()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    boxes = src.label_boxes(labels, n_labels, "pca")[0]

    def crops():
        for b in boxes:
            work.copy_from(src)
            work.crop_obb(b["center"], b["R"], b["extent"])

    legs = [("label_boxes", m) for m in args.modes] + [("crop_aabb", None), ("cluster_boxes", "pca"), ("filter_clusters", None), ("remove_boxes", None), ("crop_obb_each", None)]
    times = {leg: [] for leg in legs}
    for rep in range(args.reps + 1):                                  # rep 0: the warm-up of every leg
        for leg in legs:
            kind, mode = leg
            if kind == "label_boxes":
                ms = src.label_boxes(labels, n_labels, mode, profile=True)[1]["device_ms"]
            elif kind == "crop_aabb":
                ms = host_ms(lambda: work.crop_aabb(lo, hi))[0]
            elif kind == "cluster_boxes":
                ms = host_ms(lambda: work.cluster_boxes(args.tolerance, args.min_size, args.car_max_size, args.cell, mode))[0]
            elif kind == "filter_clusters":
                ms = host_ms(lambda: work.filter_clusters(args.tolerance, args.min_size, args.car_max_size, args.cell))[0]
            elif kind == "remove_boxes":
                ms = host_ms(lambda: work.remove_boxes(boxes))[0]
            else:
                ms = host_ms(crops, fresh=False)[0]                   # (its copies are inside: subtract n_labels copies' worth when comparing)
            if rep > 0:
                times[leg].append(ms)
    med = {leg: float(np.median(t)) for leg, t in times.items()}
    common = dict(points=len(objs), n_labels=n_labels, labelled_points=int((labels >= 0).sum()), passes=passes, reps=args.reps, device=ctx.device_name())
    lines = []
    for leg in legs:
        out = dict(leg=leg[0], mode=leg[1], ms=med[leg], ms_all=[round(t, 4) for t in times[leg]], timer="device events" if leg[0] == "label_boxes" else "host")
        if leg[0] == "label_boxes":
            out.update(mark_ms=passes * med[("crop_aabb", None)], over_mark=med[leg] / (passes * med[("crop_aabb", None)]))
        lines.append(dict(out, **common))
    summary = dict(leg="summary", cluster_stats=cst, cluster_boxes_minus_filter_clusters_ms=med[("cluster_boxes", "pca")] - med[("filter_clusters", None)],
                   remove_boxes_over_crops=med[("remove_boxes", None)] / med[("crop_obb_each", None)])
    if not args.skip_summary:
        placed = np.c_[(cars[:, :3] + cars[:, 3:]) / 2, cars[:, 3:] - cars[:, :3]]
        up = src.label_boxes(labels, n_labels, "upright")[0]
        per_car = []
        for k, car in enumerate(placed):
            l = int(np.argmin(np.linalg.norm(up["center"][:, :2] - car[:2], axis=1))) if n_labels else -1
            if l < 0 or np.linalg.norm(up["center"][l, :2] - car[:2]) > 1.0:
                per_car.append(dict(car=k, label=None))
                continue
            per_car.append(dict(car=k, label=l, count=int(up["count"][l]), placed=sorted((float(v) for v in car[3:]), reverse=True),
                                upright=[round(float(v), 3) for v in sorted(up["extent"][l], reverse=True)],
                                pca=[round(float(v), 3) for v in sorted(boxes["extent"][l], reverse=True)]))
        found = [c for c in per_car if c["label"] is not None]
        err = np.array([np.array(c["upright"]) - np.array(c["placed"]) for c in found]) if found else np.zeros((0, 3))
        whole = api.Cloud(ctx, full)
        n_inside = whole.remove_boxes(up, margin=0.1)
        kept = np.zeros(len(full), bool)
        kept[whole.last_indices()] = True
        whole.close()
        a, b = n_surface, n_surface + n_cars
        summary.update(cars_placed=len(cars), cars_matched=len(found), upright_extent_error_m=dict(mean=[round(float(v), 3) for v in err.mean(0)] if len(err) else None,
                                                                                                    worst=round(float(np.abs(err).max()), 3) if len(err) else None),
                       per_car=per_car,
                       remove_boxes_full_map=dict(margin=0.1, inside=int(n_inside), car_points_removed=int((~kept[a:b]).sum()), car_points=n_cars,
                                                  building_and_ground_points_removed=int((~kept[:a]).sum()), surface_points=n_surface,
                                                  scattered_points_removed=int((~kept[b:]).sum()), scattered_points=len(scattered)))
    lines.append(dict(summary, **common))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
