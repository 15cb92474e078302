#!/usr/bin/env python3
"""FPFH descriptors and descriptor matching (sf_map_compute_fpfh, sf_features_match) on tools/cluster_bench.py's city surface map
(synth.sample_city on synth.make_city, the extent scaled to keep city_bench's density, voxel-filtered at 0.1 m; index cell 0.25 m).
Legs, each warmed up once and then repeated --reps times, medians of device-event times:
  normals_knn      sf_map_estimate_normals_knn at k = 20, what the descriptors are computed from;
  radius / spfh / fpfh at 2, 3 and 5 voxels: sf_map_radius_outliers is the same walk with a counter for a visitor, the floor of the
                   first pass; spfh_ms and fpfh_ms are the two passes of sf_map_compute_fpfh;
  match            the descriptors of a ray-cast ring scan (voxel-filtered at 0.1 m, normals and descriptors by sf_cloud_compute_fpfh,
                   oriented to the sensor) against the map's (oriented to the sensor's true position), at two sizes: every fourth
                   scan point against the map within --near metres, and the whole scan against the whole map.  Pairs per second
                   beside the VALU floor: 99 float32 operations a pair over the guide's 157.3 TFLOP/s vector rate (which counts a
                   packed FMA as four; the rule forbids fusing, so the unfused packed rate, half of it, is given too);
  and the share of the mutual matches (and of those that also pass Lowe's ratio test at --ratio) that land within one feature
  radius of their true partner under the scan's known pose.
One JSON line per leg to stdout and to --out.
   python tools/feature_bench.py [--map-points 2000000] [--reps 2] [--out profiles/feature_bench.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_sensor_fusion_amd import api, synth  # noqa: E402

VOXEL = 0.1
FP32_VECTOR_RATE = 157.3e12                       # MI355X peak float32 vector rate, packed FMA
OPS_PER_PAIR = 99                                 # 33 x (subtract, multiply, add)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=2_000_000)
    ap.add_argument("--cell", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--radii-voxels", type=float, nargs="*", default=[2.0, 3.0, 5.0])
    ap.add_argument("--match-radius-voxels", type=float, default=5.0)
    ap.add_argument("--near", type=float, default=25.0)
    ap.add_argument("--ratio", type=float, default=0.8, help="Lowe's ratio of the second acceptance reported beside the plain mutual one")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_bench.jsonl"))
    args = ap.parse_args()
    ctx = api.Context(0)
    extent = 240.0 * float(np.sqrt(args.map_points / 10_000_000))
    boxes = synth.make_city(extent, max(1, int(120 * (extent / 240.0) ** 2)))
    cloud = api.Cloud(ctx, synth.sample_city(boxes, extent, args.map_points))
    cloud.voxel_downsample(VOXEL, "pcl")
    pts = cloud.download()
    mp = api.Map(ctx, cloud, args.cell)
    cell, dims = mp.cell_size()
    mp.profile_launches(True)
    common = dict(map_points=len(pts), extent_m=extent, cell_m=cell, grid=list(dims), reps=args.reps, device=ctx.device_name())
    lines = []

    def emit(**line):
        lines.append(dict(line, **common))
        print(json.dumps(lines[-1]), flush=True)

    t = []
    for rep in range(args.reps + 1):
        mp.estimate_normals_knn(args.k)
        if rep > 0:
            t.append(mp.last_launch_ms())
    emit(leg="normals_knn", arg=args.k, kernel_ms=float(np.median(t)), points_per_s=len(pts) / (np.median(t) * 1e-3))

    for rv in args.radii_voxels:
        r = rv * VOXEL
        tr, ts, tf, st = [], [], [], None
        for rep in range(args.reps + 1):
            mp.radius_outliers(r, 1)
            if rep > 0:
                tr.append(mp.last_launch_ms())
            _, st = mp.compute_fpfh(r, "direction", (0, 0, 1), profile=True)
            if rep > 0:
                ts.append(st["spfh_ms"])
                tf.append(st["fpfh_ms"])
        m_r, m_s, m_f = float(np.median(tr)), float(np.median(ts)), float(np.median(tf))
        emit(leg="fpfh", radius_m=r, radius_voxels=rv, radius_count_ms=m_r, spfh_ms=m_s, fpfh_ms=m_f, spfh_over_radius_count=m_s / m_r, fpfh_over_spfh=m_f / m_s,
             pairs=st["n_pairs"], max_pairs=st["max_pairs"], n_featured=st["n_featured"], mean_pairs=st["n_pairs"] / max(st["n_featured"], 1),
             spfh_pairs_per_s=st["n_pairs"] / (m_s * 1e-3), fpfh_pairs_per_s=st["n_pairs"] / (m_f * 1e-3))

    # the scan: seen from 1.8 m above the ground at a street position, turned by 30 degrees
    ground = [(x, y) for x in np.linspace(-0.3, 0.3, 13) * extent for y in np.linspace(-0.3, 0.3, 13) * extent
              if not np.any((boxes[:, 0] - 3 < x) & (x < boxes[:, 3] + 3) & (boxes[:, 1] - 3 < y) & (y < boxes[:, 4] + 3))]
    sx, sy = ground[len(ground) // 2]
    T = synth.make_T((sx, sy, 1.8), (0.0, 0.0, 30.0))
    scan = api.Cloud(ctx, synth.raycast_scan(boxes, T))
    scan.voxel_downsample(VOXEL, "pcl")
    scan_pts = scan.download()
    r = args.match_radius_voxels * VOXEL
    nr = 2.5 * VOXEL
    f_scan, st_scan = scan.compute_fpfh(nr, r, "viewpoint", (0, 0, 0), cell=args.cell)
    mp.estimate_normals(nr)
    f_map, st_map = mp.compute_fpfh(r, "viewpoint", T[:3, 3])
    truth = scan_pts.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    near = np.nonzero(np.linalg.norm(pts[:, :2].astype(np.float64) - T[:2, 3], axis=1) < args.near)[0]
    rows_m, valid_m = f_map.download()
    rows_s, valid_s = f_scan.download()
    sizes = [("quarter_scan_vs_near_map", np.arange(0, len(scan_pts), 4), near), ("scan_vs_map", np.arange(len(scan_pts)), np.arange(len(pts)))]
    for name, si, mi in sizes:
        fs, fm = api.Features(ctx, rows_s[si], valid_s[si]), api.Features(ctx, rows_m[mi], valid_m[mi])
        one, both, res = [], [], None
        for rep in range(args.reps + 1):
            a = fs.match(fm, profile=True)
            res = fs.match(fm, mutual=True, profile=True)
            if rep > 0:
                one.append(a["stats"]["match_ms"])
                both.append(res["stats"]["match_ms"])
        stt = res["stats"]
        pairs = stt["n_src_valid"] * stt["n_dst_valid"]
        ms = float(np.median(one))
        p = res["pairs"]
        err = np.linalg.norm(truth[si][p[:, 0]] - pts[mi][p[:, 1]].astype(np.float64), axis=1) if len(p) else np.zeros(0)
        strict = fs.match(fm, ratio=args.ratio, mutual=True)["pairs"]
        err_s = np.linalg.norm(truth[si][strict[:, 0]] - pts[mi][strict[:, 1]].astype(np.float64), axis=1) if len(strict) else np.zeros(0)
        emit(leg="match", size=name, n_src=stt["n_src"], n_dst=stt["n_dst"], n_src_valid=stt["n_src_valid"], n_dst_valid=stt["n_dst_valid"], match_ms=ms,
             mutual_match_ms=float(np.median(both)), pairs_per_s=pairs / (ms * 1e-3), flops_per_s=OPS_PER_PAIR * pairs / (ms * 1e-3),
             valu_floor_ms=OPS_PER_PAIR * pairs / FP32_VECTOR_RATE * 1e3, unfused_floor_ms=OPS_PER_PAIR * pairs / (FP32_VECTOR_RATE / 2) * 1e3,
             times_the_floor=ms / (OPS_PER_PAIR * pairs / FP32_VECTOR_RATE * 1e3), n_mutual=int(stt["n_matched"]), ratio=args.ratio, n_mutual_ratio=len(strict),
             mutual_ratio_within_radius=float((err_s < r).mean()) if len(strict) else 0.0, mutual_ratio_within_radius_count=int((err_s < r).sum()),
             feature_radius_m=r, normal_radius_m=nr, mutual_within_radius=float((err < r).mean()) if len(p) else 0.0,
             mutual_within_radius_count=int((err < r).sum()), scan_featured=st_scan["n_featured"], map_featured=st_map["n_featured"])

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
