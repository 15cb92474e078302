#!/usr/bin/env python3
"""Plane segmentation (sf_cloud_segment_plane, sf_cloud_remove_plane) on the city map of tools/cluster_bench.py -- the surface, --cars
car-sized boxes, 0.5 % scattered points -- ROTATED by a few degrees of roll and pitch, so that no z cut finds the ground.
Legs: the scoring launches (sf_plane_stats.score_ms) at 256, 1024 and 4096 hypotheses and the whole call (total_ms), device events,
every leg warmed up once, then alternating --reps times, medians reported; beside them sf_cloud_remove_floor, the streaming
yardstick, by host time around a synchronised call (it has no events).  Per scoring leg: the point-plane tests per second and the
VALU floor of the same work, N H / 64 x VALU_PER_TEST wave instructions at one per 2 cycles on each of CUs x 4 SIMDs; the clock is
the shader clock the driver reported while the legs ran (sysfs, pp_dpm_sclk), the nominal one only where that cannot be read.  The
mark is twice the floor.  Then what DESIGN.md section 15 could only do with the hand cut z > 0.15: remove_plane (axis = the rotated up
direction, 15 degrees) followed by filter_clusters(0.25, 50, 5000) -- the clusters that remain and the shares of the car, building
and scattered points they hold -- next to the same figures for the level map with the hand cut.  One JSON line per leg to stdout and
to --out.
   python tools/plane_bench.py [--map-points 2000000] [--reps 5] [--out profiles/plane_bench.jsonl]"""
import argparse
import glob
import json
import os
import re
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_sensor_fusion_amd import api, synth  # noqa: E402

# vector instructions per wave and point-plane test in the inner loop of k_plane_score (profiles/plane_score_isa.txt: one trip is
# 8 planes x 4 points = 32 tests per lane and 152 vector instructions: per plane 6 packed multiplies, 6 packed adds, 4 compares and
# 3 for the lane's counter)
VALU_PER_TEST = 152.0 / 32.0
SIMDS_PER_CU = 4
CYCLES_PER_WAVE_INSTRUCTION = 2


class ClockSampler(threading.Thread):
    """the highest active shader clock among the cards, sampled while the legs run (the busy card is the one that clocks up)"""

    def __init__(self):
        super().__init__(daemon=True)
        self.files = glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")
        self.samples, self.stop = [], False

    def run(self):
        while not self.stop and self.files:
            best = 0
            for path in self.files:
                try:
                    with open(path) as f:
                        for m in re.finditer(r"(\d+)Mhz \*", f.read()):
                            best = max(best, int(m.group(1)))
                except OSError:
                    pass
            if best:
                self.samples.append(best)
            time.sleep(0.002)

    def median_mhz(self):
        return float(np.median(self.samples)) if self.samples else None


def rotation(roll_deg, pitch_deg):
    r, p = np.radians(roll_deg), np.radians(pitch_deg)
    rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    return ry @ rx


def objects(ctx, pts, keep_idx, n_surface, n_cars, args, stats_of_cut):
    """filter_clusters(tolerance, min_size, car_max_size) on pts[keep_idx]: what §15 reports for the map less its ground"""
    cloud = api.Cloud(ctx, pts[keep_idx])
    st = cloud.filter_clusters(args.filter_tolerance, args.filter_min_size, args.car_max_size, args.cell)
    above = np.zeros(len(pts), bool)
    above[keep_idx] = True
    kept = np.zeros(len(pts), bool)
    kept[keep_idx[cloud.last_indices()]] = True
    cloud.close()
    a, b = n_surface, n_surface + n_cars

    def share(lo, hi):
        return float(kept[lo:hi][above[lo:hi]].mean()) if above[lo:hi].any() else 0.0
    return dict(points=int(len(keep_idx)), clusters=st["n_clusters"], car_points_kept=share(a, b), surface_points_kept=share(0, a), scattered_points_kept=share(b, len(pts)),
                car_points_left_by_the_cut=float(above[a:b].mean()) if n_cars else 0.0, kept_points=st["n_kept"], largest_size=st["largest_size"], cut=stats_of_cut)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=2_000_000)
    ap.add_argument("--cell", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hypotheses", type=int, nargs="*", default=[256, 1024, 4096])
    ap.add_argument("--threshold", type=float, default=0.15, help="the distance threshold (§15's hand cut is z > 0.15)")
    ap.add_argument("--roll", type=float, default=3.0)
    ap.add_argument("--pitch", type=float, default=-2.0)
    ap.add_argument("--max-angle", type=float, default=15.0)
    ap.add_argument("--cars", type=int, default=40)
    ap.add_argument("--scattered", type=float, default=0.005)
    ap.add_argument("--filter-tolerance", type=float, default=0.25)
    ap.add_argument("--filter-min-size", type=int, default=50)
    ap.add_argument("--car-max-size", type=int, default=5000)
    ap.add_argument("--skip-filter", action="store_true", help="only the timed legs (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_bench.jsonl"))
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
    n_car_raw = int(round(args.map_points * area(cars, 0.0) / area(boxes, extent * extent))) if len(cars) else 0
    car_pts = voxelised(synth.sample_city(cars, 0.0, n_car_raw, seed=synth.CITY_SEED + 5)) if n_car_raw else np.zeros((0, 3), np.float32)
    n_surface, n_cars = len(surface), len(car_pts)
    rng = np.random.default_rng(17)
    lo, hi = surface.min(0), surface.max(0)
    scattered = rng.uniform(lo, hi, (int(round(args.scattered * n_surface)), 3)).astype(np.float32)
    level = np.concatenate([surface, car_pts, scattered])
    del surface
    R = rotation(args.roll, args.pitch)
    up = R @ np.array([0.0, 0.0, 1.0])
    pts = (level.astype(np.float64) @ R.T).astype(np.float32)
    n = len(pts)
    cloud = api.Cloud(ctx, pts)
    plane_kw = dict(distance_threshold=args.threshold, refine=True, seed=0, axis=up, max_angle_deg=args.max_angle)

    legs = [("score", h) for h in args.hypotheses] + [("remove_floor", 0)]
    times = {leg: [] for leg in legs}
    totals = {h: [] for h in args.hypotheses}
    did = {}
    scratch = api.Cloud(ctx)
    sampler = ClockSampler()
    sampler.start()
    for rep in range(args.reps + 1):                                  # rep 0: the warm-up of every leg
        for leg in legs:
            kind, h = leg
            if kind == "score":
                plane, _, st = cloud.segment_plane(num_hypotheses=h, profile=True, **plane_kw)
                ms, total = st["score_ms"], st["total_ms"]
                did[leg] = dict(plane=[float(v) for v in plane], stats=st)
            else:
                scratch.copy_from(cloud)
                ctx.synchronize()
                t0 = time.perf_counter()
                scratch.remove_floor()                                # (compaction synchronises: the kept count is a host value)
                ms, total = (time.perf_counter() - t0) * 1e3, None
            if rep > 0:
                times[leg].append(ms)
                if total is not None:
                    totals[h].append(total)
    sampler.stop = True
    sampler.join()
    scratch.close()
    sclk = sampler.median_mhz()
    props = None
    try:
        import torch
        props = torch.cuda.get_device_properties(0)
    except Exception:
        pass
    cus = int(getattr(props, "multi_processor_count", 256) or 256)
    nominal = float(getattr(props, "clock_rate", 0) or 0) / 1e3 or None
    clock_mhz, clock_source = (sclk, "pp_dpm_sclk while the legs ran") if sclk else (nominal or 2400.0, "nominal")
    rate = cus * SIMDS_PER_CU * clock_mhz * 1e6 / CYCLES_PER_WAVE_INSTRUCTION      # wave instructions per second
    common = dict(points=n, surface_points=n_surface, car_points=n_cars, cars=len(cars), scattered_points=len(scattered), extent_m=extent, roll_deg=args.roll,
                  pitch_deg=args.pitch, up=[float(v) for v in up], threshold=args.threshold, reps=args.reps, device=ctx.device_name(), compute_units=cus,
                  clock_mhz=clock_mhz, clock_source=clock_source, nominal_clock_mhz=nominal)
    lines = []
    floor_ms = float(np.median(times[("remove_floor", 0)]))
    for h in args.hypotheses:
        ms = float(np.median(times[("score", h)]))
        tests = float(n) * h
        floor = tests / 64.0 * VALU_PER_TEST / rate * 1e3
        lines.append(dict(leg="score", hypotheses=h, score_ms=ms, score_ms_all=[round(t, 4) for t in times[("score", h)]], tests_per_s=tests / (ms * 1e-3),
                          valu_per_test=VALU_PER_TEST, valu_floor_ms=floor, mark_ms=2 * floor, over_floor=ms / floor, within_mark=bool(ms <= 2 * floor),
                          total_ms=float(np.median(totals[h])), total_ms_all=[round(t, 4) for t in totals[h]], remove_floor_host_ms=floor_ms,
                          total_over_remove_floor=float(np.median(totals[h])) / floor_ms, **did[("score", h)], **common))
    lines.append(dict(leg="remove_floor", host_ms=floor_ms, host_ms_all=[round(t, 4) for t in times[("remove_floor", 0)]], points_per_s=n / (floor_ms * 1e-3), **common))
    if not args.skip_filter:
        work = api.Cloud(ctx, pts)
        plane, st = work.remove_plane(num_hypotheses=1024, **plane_kw)
        rotated = objects(ctx, pts, work.last_indices().astype(np.int64), n_surface, n_cars, args, dict(plane=[float(v) for v in plane], stats=st))
        work.close()
        hand = objects(ctx, level, np.flatnonzero(level[:, 2] > args.threshold), n_surface, n_cars, args, dict(rule="z > %g on the level map" % args.threshold))
        # the reference's floor on the rotated map, for the record: z > 0 takes half the ground away and leaves the other half
        floor_cloud = api.Cloud(ctx, pts)
        floor_cloud.remove_floor()
        kept = np.zeros(n, bool)
        kept[floor_cloud.last_indices()] = True
        floor_cloud.close()
        ground = level[:n_surface, 2] <= args.threshold                # what the hand cut takes from the level map's surface
        lines.append(dict(leg="objects", tolerance=args.filter_tolerance, min_size=args.filter_min_size, max_size=args.car_max_size, rotated_map_remove_plane=rotated,
                          level_map_hand_cut=hand, remove_floor_on_rotated_map=dict(ground_points=int(ground.sum()), ground_points_left=float(kept[:n_surface][ground].mean())),
                          **common))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
