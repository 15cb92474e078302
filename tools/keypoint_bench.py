#!/usr/bin/env python3
"""ISS keypoints (sf_map_iss_keypoints) and the keypoint-restricted global registration (api.global_register with src_keypoints /
dst_keypoints).  Legs, each warmed up once and then repeated --reps times, medians of device-event times:
  city     tools/feature_bench.py's city surface map (synth.sample_city on synth.make_city, voxel-filtered at 0.1 m, cell 0.25 m):
           saliency_ms and nms_ms at salient radii of 3, 5 and 8 voxels (the non-maximum radius two thirds of it, Open3D's ratio);
           beside them sf_map_radius_outliers at the salient radius -- the same walk with a counter for a visitor, the floor of the
           first pass -- and spfh_ms, the first pass of sf_map_compute_fpfh at that radius (k-NN normals at k = 20).  Each radius
           at every min_lambda3 of --floors (default: none, 2.5e-5 m^2 = the square of the 5 mm the city is sampled with, and four
           times that): the keypoints and the share of them that lie within one salient radius of an edge of a building (roof rim, wall corner,
           foot of a wall) -- whether the keypoints leave the planes;
  terrain  synth.make_terrain(60, 0.2, 1) and the local scan of tools/register_bench.py under its pose, FPFH at 1.0 m (normals at
           0.5 m): api.global_register on all rows and on the ISS keypoints (0.6 / 0.4 m, min_lambda3 3.6e-7 m^2) -- the keypoint
           counts, match_ms (mutual, device events), the share of the mutual matches that are right, the pose error.
One JSON line per leg to stdout and to --out.
   python tools/keypoint_bench.py [--map-points 2000000] [--reps 3] [--out profiles/keypoint_bench.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_sensor_fusion_amd import api, synth  # noqa: E402

VOXEL = 0.1


def box_edges(boxes):
    """the 12 edges of every box (x0, y0, z0, x1, y1, z1) -> (a, b) float64 [12 B, 3] each"""
    a, b = [], []
    for x0, y0, z0, x1, y1, z1 in boxes:
        c = np.array([[x, y, z] for x in (x0, x1) for y in (y0, y1) for z in (z0, z1)])
        for i in range(8):
            for j in range(i + 1, 8):
                if np.count_nonzero(c[i] != c[j]) == 1:
                    a.append(c[i])
                    b.append(c[j])
    return np.array(a), np.array(b)


def edge_distance(points, a, b, chunk=4096):
    """the distance of every point from the nearest segment [a_k, b_k]"""
    out = np.empty(len(points))
    ab = b - a
    ll = (ab * ab).sum(1)
    for s in range(0, len(points), chunk):
        p = points[s:s + chunk].astype(np.float64)[:, None, :]
        t = np.clip(((p - a[None]) * ab[None]).sum(2) / ll[None], 0.0, 1.0)
        d = p - (a[None] + t[:, :, None] * ab[None])
        out[s:s + chunk] = np.sqrt((d * d).sum(2)).min(1)
    return out


def true_pose():
    a = np.deg2rad(140.0)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = (7.0, -9.0, 3.6)
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=2_000_000)
    ap.add_argument("--cell", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--radii-voxels", type=float, nargs="*", default=[3.0, 5.0, 8.0])
    ap.add_argument("--floors", type=float, nargs="*", default=[0.0, 2.5e-5, 1.0e-4], help="min_lambda3 of the city legs (m^2)")
    ap.add_argument("--extent", type=float, default=60.0, help="side of the terrain (m)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keypoint_bench.jsonl"))
    args = ap.parse_args()
    ctx = api.Context(0)
    lines = []

    def emit(**line):
        lines.append(dict(line, reps=args.reps, device=ctx.device_name()))
        print(json.dumps(lines[-1]), flush=True)

    # ---- the city
    extent = 240.0 * float(np.sqrt(args.map_points / 10_000_000))
    boxes = synth.make_city(extent, max(1, int(120 * (extent / 240.0) ** 2)))
    cloud = api.Cloud(ctx, synth.sample_city(boxes, extent, args.map_points))
    cloud.voxel_downsample(VOXEL, "pcl")
    pts = cloud.download()
    mp = api.Map(ctx, cloud, args.cell)
    cell, dims = mp.cell_size()
    mp.profile_launches(True)
    mp.estimate_normals_knn(20)
    ea, eb = box_edges(boxes)
    common = dict(map_points=len(pts), extent_m=extent, cell_m=cell, grid=list(dims), boxes=len(boxes))
    for rv in args.radii_voxels:
        rs, rn = rv * VOXEL, rv * VOXEL * 2.0 / 3.0
        tr, tp = [], []
        for rep in range(args.reps + 1):
            mp.radius_outliers(rs, 1)
            if rep > 0:
                tr.append(mp.last_launch_ms())
            _, st = mp.compute_fpfh(rs, "direction", (0, 0, 1), profile=True)
            if rep > 0:
                tp.append(st["spfh_ms"])
        m_r, m_p = float(np.median(tr)), float(np.median(tp))
        for floor in args.floors:
            ts, tn, kp = [], [], None
            for rep in range(args.reps + 1):
                kp = mp.iss_keypoints(rs, rn, min_lambda3=floor, profile=True)
                if rep > 0:
                    ts.append(kp["stats"]["saliency_ms"])
                    tn.append(kp["stats"]["nms_ms"])
            m_s, m_n = float(np.median(ts)), float(np.median(tn))
            near = edge_distance(pts[kp["indices"]], ea, eb) < rs if len(kp["indices"]) else np.zeros(0, bool)
            st = kp["stats"]
            emit(leg="city", salient_radius_m=rs, non_max_radius_m=rn, radius_voxels=rv, min_lambda3=floor, saliency_ms=m_s, nms_ms=m_n, radius_count_ms=m_r, spfh_ms=m_p,
                 saliency_over_radius_count=m_s / m_r, saliency_over_spfh=m_s / m_p, nms_over_saliency=m_n / m_s, n_salient=st["n_salient"], n_keypoints=st["n_keypoints"],
                 max_neighbors=st["max_neighbors"], keypoints_near_an_edge=int(near.sum()), share_near_an_edge=float(near.mean()) if len(near) else 0.0, **common)
    mp.close()
    cloud.close()

    # ---- the terrain
    T = true_pose()
    terrain = synth.make_terrain(args.extent, 0.2, 1)
    scan, idx = synth.make_local_scan(terrain, (2.0, -1.0), 8.0, T, 0.005, 2)
    map_cloud, scan_cloud = api.Cloud(ctx, terrain), api.Cloud(ctx, scan)
    tm = api.Map(ctx, map_cloud, 0.5)
    tm.estimate_normals(0.5)
    f_map = tm.compute_fpfh(1.0, "direction", (0, 0, 1))[0]
    f_scan = scan_cloud.compute_fpfh(0.5, 1.0, "direction", (0, 0, 1))[0]
    rs, rn, floor = 0.6, 0.4, 1e-6 * 0.6 ** 2
    k_map = tm.iss_keypoints(rs, rn, min_lambda3=floor, profile=True)
    k_scan = scan_cloud.iss_keypoints(rs, rn, min_lambda3=floor, profile=True)
    base = dict(map_points=len(terrain), scan_points=len(scan), extent_m=args.extent, salient_radius_m=rs, non_max_radius_m=rn, min_lambda3=floor)
    full_ms = None
    for name, ks, km in (("all_rows", None, None), ("keypoints", k_scan["indices"], k_map["indices"])):
        t, g = [], None
        for rep in range(args.reps + 1):
            g = api.global_register(scan_cloud, f_scan, map_cloud, f_map, 0.05, num_hypotheses=4096, seed=1, profile=True, src_keypoints=ks, dst_keypoints=km)
            if rep > 0:
                t.append(g["match_stats"]["match_ms"])
        p = g["pairs"]
        right = idx[p[:, 0]] == p[:, 1]
        dt, dr = synth.pose_error(g["T"], T)
        ms = float(np.median(t))
        full_ms = ms if full_ms is None else full_ms
        emit(leg="terrain", rows=name, scan_rows=g["match_stats"]["n_src"], map_rows=g["match_stats"]["n_dst"], scan_keypoints=len(k_scan["indices"]),
             map_keypoints=len(k_map["indices"]), map_saliency_ms=k_map["stats"]["saliency_ms"], map_nms_ms=k_map["stats"]["nms_ms"], match_ms=ms,
             match_ms_over_all_rows=ms / full_ms, mutual_matches=len(p), right=int(right.sum()), right_share=float(right.mean()) if len(p) else 0.0, found=g["found"],
             inliers=g["ransac"]["stats"]["n_inliers"], pose_error_m=dt, pose_error_rad=dr, **base)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
