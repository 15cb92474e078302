#!/usr/bin/env python3
"""Range images (sf_range_image_build) and visibility votes (sf_map_visibility_votes, sf_cloud_remove_seen_through) on the city of
tools/city_bench.py: synth.sample_city on synth.make_city, voxel-filtered at 0.1 m, with the surfaces of --cars car-sized boxes
(synth.make_cars) sampled into the MAP and absent from the world the --scans scans are ray-cast in, from poses along the street.
Legs, each warmed up once, then --reps alternating repetitions, medians:
  build           device events around the fill and the two kernels of one 128-ring scan (about 254 k points) into a 2048 x 64 image;
  votes_B         device events around the one kernel of sf_map_visibility_votes at B = 1, 4 and 16 images (profile = True);
  crop_aabb       the yardstick of tools/box_bench.py, one streaming pass with its compaction: sf_cloud_crop_aabb of the map's points
                  (a box that holds every point), host time of the call with the context drained before it;
  remove_seen     sf_cloud_remove_seen_through at 16 images on a copy of the map's cloud, host time like the yardstick.
Every figure comes with its ratio to the yardstick of the same run and with the bytes it must move (the floor: those bytes at
6.3 TB/s).  Then what the votes are worth: the share of car points flagged at min_seen 1, 2 and 4 (max_within 0, and any), the share
of static points flagged, split into ground (z < 0.15 m) and the rest (walls, roofs), for a few windows and margins -- grazing ground
is where the method misfires.  Nothing is gated.  One JSON line per leg and one summary; stdout and --out.
   python tools/visibility_bench.py [--map-points 4000000] [--reps 5] [--out profiles/visibility_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_sensor_fusion_amd import api, synth  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cars", type=int, default=40)
    ap.add_argument("--scans", type=int, default=16)
    ap.add_argument("--rings", type=int, default=64, help="rings of the voting scans (the build leg always times a 128-ring scan)")
    ap.add_argument("--skip-summary", action="store_true", help="only the timed legs (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visibility_bench.jsonl"))
    args = ap.parse_args()
    ctx = api.Context(0)
    extent = 240.0 * float(np.sqrt(args.map_points / 10_000_000))
    city = synth.make_city(extent, max(1, int(120 * (extent / 240.0) ** 2)))
    xs = np.linspace(-12.0, 12.0, args.scans)
    poses = np.stack([synth.make_T((x, 0.0, 1.8), (0.0, 0.0, 0.0)) for x in xs]).astype(np.float64)
    cars = synth.make_cars(city, [(x, 0.0) for x in xs], args.cars, radius=(4.0, 15.0))

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
    car_pts = car_pts[car_pts[:, 2] > 0.05]                           # (a car's footprint on the ground is ground)
    full = np.concatenate([surface, car_pts])
    n_surface, n = len(surface), len(full)
    is_car = np.arange(n) >= n_surface
    is_ground = ~is_car & (full[:, 2] < 0.15)
    is_wall = ~is_car & ~is_ground
    del surface

    scans = [synth.raycast_scan(city, T, rings=args.rings, seed=synth.CITY_SEED + 10 + k) for k, T in enumerate(poses)]
    big_scan = synth.raycast_scan(city, poses[len(poses) // 2], rings=128, seed=synth.CITY_SEED + 9)
    images = []
    for s in scans:
        img = api.RangeImage(ctx)
        img.build(api.Cloud(ctx, s))
        images.append(img)
    prm = images[0].params
    pixels = prm["width"] * prm["height"]
    big_cloud, big_img = api.Cloud(ctx, big_scan), api.RangeImage(ctx)

    src = api.Cloud(ctx, full)
    mp = api.Map(ctx, src, 0.25)
    work = api.Cloud(ctx, full)
    lo, hi = full.min(0).astype(np.float64) - 1.0, full.max(0).astype(np.float64) + 1.0

    def host_ms(call):
        work.copy_from(src)
        ctx.synchronize()
        t0 = time.perf_counter()
        out = call()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    counts = [b for b in (1, 4, 16) if b <= len(images)]
    legs = ["build"] + ["votes_%d" % b for b in counts] + ["crop_aabb", "remove_seen"]
    times = {leg: [] for leg in legs}
    for rep in range(args.reps + 1):                                  # rep 0: the warm-up of every leg
        for leg in legs:
            if leg == "build":
                ms = big_img.build(big_cloud)["device_ms"]
            elif leg.startswith("votes_"):
                b = int(leg[6:])
                ms = mp.visibility_votes(images[:b], poses[:b], profile=True)[2]["device_ms"]
            elif leg == "crop_aabb":
                ms = host_ms(lambda: work.crop_aabb(lo, hi))[0]
            else:
                ms = host_ms(lambda: work.remove_seen_through(images, poses))[0]
            if rep > 0:
                times[leg].append(ms)
    med = {leg: float(np.median(t)) for leg, t in times.items()}
    yard = med["crop_aabb"]
    # the bytes each leg must move: the build reads 12 B a point, fills and reads back 8 B a pixel, writes 4 B a pixel and sends one
    # 8-byte atomic a point; the votes read 16 B a point and each image's plane once, and write two uint16 a point
    floor = {"build": 12 * len(big_scan) + 8 * len(big_scan) + (8 + 8 + 4) * pixels, "crop_aabb": (12 + 1 + 12 + 4) * n, "remove_seen": 12 * n + n + 4 * pixels * len(images) + (12 + 1 + 12 + 4) * n}
    for b in counts:
        floor["votes_%d" % b] = 16 * n + 4 * n + 4 * pixels * b
    common = dict(map_points=n, car_points=int(is_car.sum()), ground_points=int(is_ground.sum()), wall_points=int(is_wall.sum()), scan_points=[len(s) for s in scans],
                  build_scan_points=len(big_scan), image=[prm["width"], prm["height"]], reps=args.reps, device=ctx.device_name())
    lines = []
    for leg in legs:
        lines.append(dict(leg=leg, ms=med[leg], ms_all=[round(t, 4) for t in times[leg]], timer="host" if leg in ("crop_aabb", "remove_seen") else "device events",
                          over_crop_aabb=med[leg] / yard, bytes_moved=int(floor[leg]), floor_ms=floor[leg] / HBM_BYTES_PER_S * 1e3, **common))
    if not args.skip_summary:
        quality = []
        for hc, hr, margin, ratio in ((1, 1, 0.2, 0.01), (0, 0, 0.2, 0.01), (2, 1, 0.2, 0.01), (1, 1, 0.5, 0.02), (1, 1, 0.1, 0.0)):
            seen, within, st = mp.visibility_votes(images, poses, half_cols=hc, half_rows=hr, range_margin=margin, range_ratio=ratio)
            row = dict(half_cols=hc, half_rows=hr, range_margin=margin, range_ratio=ratio, stats=st)
            for k in (1, 2, 4):
                for name, ok in (("max_within_0", within == 0), ("any_within", np.ones(n, bool))):
                    flag = (seen >= k) & ok
                    row["min_seen_%d_%s" % (k, name)] = dict(car=float(flag[is_car].mean()), ground=float(flag[is_ground].mean()), wall=float(flag[is_wall].mean()))
            quality.append(row)
        lines.append(dict(leg="summary", quality=quality, **common))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
