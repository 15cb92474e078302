#!/usr/bin/env python3
"""NDT scan-to-map registration (api.Ndt) on the city map, beside point-to-plane ICP from the same priors.  Legs:
  build    tools/feature_bench.py's city surface map (synth.sample_city on synth.make_city, voxel-filtered at 0.1 m): build_ms of the NDT
           voxels (the cell flags, both scans, k_ndt_voxels, the compaction -- not the grid index before them) at resolution 1 m and
           2 m, device events, the median of --reps builds after one warm-up; cells, occupied cells, voxels;
  derivs   one derivative pass (k_ndt_derivs and the reduction launch behind it) of a ray-cast scan at its true pose, DIRECT1 and
           DIRECT7, device events: of a single pose (the latency of one iteration) and per pose of 64 poses in one launch.  Beside
           it the floor the tool computes from what the pass must move and compute: 12 bytes per point, 4 bytes per cell looked
           up, 80 bytes per voxel record gathered; FLOPS_PER_TERM float64 operations per term and FLOPS_PER_POINT per point, against
           --hbm-tbs and --fp64-tflops (the MI355X's 8 TB/s and 78.6 TFLOP/s vector float64);
  scores   the score pass of a line search (k_ndt_scores and the reduction launch behind it, api.Ndt.scores) of the same scan at 8 and
           at 16 poses in one launch, DIRECT1 and DIRECT7, device events, per launch and per pose; the floor computed the same way
           from what a score pass must move and compute: per pose 12 bytes per point, 4 bytes per cell looked up, 80 bytes per
           voxel record gathered; FLOPS_PER_SCORE_TERM float64 operations per term and FLOPS_PER_POINT per point;
  align    --scans sensor poses along the streets, each from a prior off by 0.25, 0.5, 1 and 2 m (a horizontal direction drawn at
           random) and by 2, 4, 8 and 16 degrees of yaw: NDT (resolution --resolution, DIRECT7, 30 iterations) and point-to-plane
           ICP (--icp-corr m correspondence distance, 30 iterations, k-NN normals at k = 20) -- the median pose error, the share of
           scans brought within 5 cm of the truth, ms per alignment (the host's clock around the synchronised call; for NDT also
           the device events around its launches).  Beside them, from the same priors: NDT with the line search at the same
           resolution (ndt_ls_*) and the pyramid of --levels with the line search (ndt_pyr_*, api.NdtPyramid; device ms summed
           over the levels).
One JSON line per leg to stdout and to --out.  Reads nothing outside the repository.
   python tools/ndt_bench.py [--map-points 2000000] [--reps 5] [--scans 8] [--out profiles/ndt_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_sensor_fusion_amd import api, synth  # noqa: E402

VOXEL = 0.1
FLOPS_PER_TERM = 340   # B q 15, q^T B q 5, exp ~40, a 9, B J 27, the gradient 12, 21 Hessian entries of ~11
FLOPS_PER_POINT = 40   # T x 18, the grid coordinates 6, the comparisons
FLOPS_PER_SCORE_TERM = 62   # B q 15, q^T B q 5, exp ~40, the sum 2


def yaw_pose(x, y, z, yaw_deg):
    a = np.deg2rad(yaw_deg)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = (x, y, z)
    return T


def free_poses(boxes, extent, n, rng):
    """sensor poses 1.8 m above the ground, at least 2 m clear of every building"""
    out = []
    while len(out) < n:
        x, y = rng.uniform(-0.3 * extent, 0.3 * extent, 2)
        if np.all((x < boxes[:, 0] - 2.0) | (x > boxes[:, 3] + 2.0) | (y < boxes[:, 1] - 2.0) | (y > boxes[:, 4] + 2.0)):
            out.append(yaw_pose(x, y, 1.8, rng.uniform(-180.0, 180.0)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scans", type=int, default=8)
    ap.add_argument("--resolution", type=float, default=1.0)
    ap.add_argument("--icp-corr", type=float, default=1.0)
    ap.add_argument("--levels", type=float, nargs="+", default=[4.0, 2.0, 1.0], help="the pyramid's resolutions, descending")
    ap.add_argument("--scan-stride", type=int, default=4, help="every n-th hit of the 64 x 2032 ray-cast scan")
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--fp64-tflops", type=float, default=78.6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ndt_bench.jsonl"))
    args = ap.parse_args()
    ctx = api.Context(0)
    lines = []

    def emit(**line):
        lines.append(dict(line, reps=args.reps, device=ctx.device_name()))
        print(json.dumps(lines[-1]), flush=True)

    extent = 240.0 * float(np.sqrt(args.map_points / 10_000_000))
    boxes = synth.make_city(extent, max(1, int(120 * (extent / 240.0) ** 2)))
    cloud = api.Cloud(ctx, synth.sample_city(boxes, extent, args.map_points))
    cloud.voxel_downsample(VOXEL, "pcl")
    n_map = len(cloud)
    common = dict(map_points=n_map, extent_m=extent, boxes=len(boxes))

    # ---- build
    for res in (1.0, 2.0):
        ndt = api.Ndt(ctx, cloud, res, profile=True)
        t = []
        for _ in range(args.reps):
            ndt.set_target(cloud)
            t.append(ndt.stats()["build_ms"])
        st = ndt.stats()
        emit(leg="build", resolution_m=res, build_ms=float(np.median(t)), n_cells=st["n_cells"], n_occupied=st["n_occupied"], n_voxels=st["n_voxels"], grid=list(st["dims"]), **common)
        ndt.close()

    # ---- one derivative pass
    rng = np.random.default_rng(5)
    truths = free_poses(boxes, extent, args.scans, rng)
    scans = [synth.raycast_scan(boxes, T, seed=100 + k)[::args.scan_stride].astype(np.float32) for k, T in enumerate(truths)]
    for nb in (1, 7):
        ndt = api.Ndt(ctx, cloud, args.resolution, neighbours=nb, profile=True)
        for k_poses in (1, 64):
            poses = np.repeat(truths[0][None], k_poses, 0)
            t, r = [], None
            for rep in range(args.reps + 1):
                r = ndt.derivatives(scans[0], poses)[0]
                if rep > 0:
                    t.append(ndt.stats()["align_ms"] / k_poses)
            n, terms = len(scans[0]), r["n_terms"]
            nbytes = 12.0 * n + 4.0 * nb * n + 80.0 * terms
            flops = float(FLOPS_PER_TERM) * terms + float(FLOPS_PER_POINT) * n
            floor_ms = 1e3 * max(nbytes / (args.hbm_tbs * 1e12), flops / (args.fp64_tflops * 1e12))
            ms = float(np.median(t))
            emit(leg="derivs", neighbours=nb, resolution_m=args.resolution, poses_per_launch=k_poses, scan_points=n, n_terms=terms, n_inside=r["n_inside"], ms_per_pass=ms,
                 bytes=nbytes, flops=flops, floor_ms=floor_ms, over_floor=ms / floor_ms, **common)
        for k_poses in (8, 16):                                   # the trials of one line-search iteration in one launch
            poses = np.repeat(truths[0][None], k_poses, 0)
            t, terms = [], None
            for rep in range(args.reps + 1):
                _, terms = ndt.scores(scans[0], poses)
                if rep > 0:
                    t.append(ndt.stats()["align_ms"])
            n, terms = len(scans[0]), int(terms[0])
            nbytes = k_poses * (12.0 * n + 4.0 * nb * n + 80.0 * terms)
            flops = k_poses * (float(FLOPS_PER_SCORE_TERM) * terms + float(FLOPS_PER_POINT) * n)
            floor_ms = 1e3 * max(nbytes / (args.hbm_tbs * 1e12), flops / (args.fp64_tflops * 1e12))
            ms = float(np.median(t))
            emit(leg="scores", neighbours=nb, resolution_m=args.resolution, poses_per_launch=k_poses, scan_points=n, n_terms=terms, ms_per_launch=ms, ms_per_pose=ms / k_poses,
                 bytes=nbytes, flops=flops, floor_ms=floor_ms, over_floor=ms / floor_ms, **common)
        ndt.close()

    # ---- alignments beside point-to-plane ICP
    mp = api.Map(ctx, cloud, 0.25)
    mp.estimate_normals_knn(20)
    icp = api.Icp(ctx, args.icp_corr, 30, 0.0, 1e-6)
    icp.set_target(mp)
    ndt = api.Ndt(ctx, cloud, args.resolution, profile=True)
    ndt_ls = api.Ndt(ctx, cloud, args.resolution, profile=True).set_line_search()
    pyr = api.NdtPyramid(ctx, cloud, args.levels, profile=True)
    for off, yaw in ((0.25, 2.0), (0.5, 4.0), (1.0, 8.0), (2.0, 16.0)):
        res = dict(ndt=dict(err=[], rot=[], ms=[], dev_ms=[], it=[]), icp=dict(err=[], rot=[], ms=[], it=[]),
                   ndt_ls=dict(err=[], rot=[], ms=[], dev_ms=[], it=[], stalled=[]), ndt_pyr=dict(err=[], rot=[], ms=[], dev_ms=[], it=[], stalled=[]))
        for k, (T, scan) in enumerate(zip(truths, scans)):
            a = rng.uniform(0.0, 2.0 * np.pi)
            prior = T.copy()                                       # the yaw turns the sensor where it stands
            prior[:3, :3] = yaw_pose(0.0, 0.0, 0.0, yaw * (1.0 if k % 2 else -1.0))[:3, :3] @ T[:3, :3]
            prior[:3, 3] = T[:3, 3] + (off * np.cos(a), off * np.sin(a), 0.0)
            for rep in range(2):                                   # the first run of a scan warms up
                ctx.synchronize()
                t0 = time.perf_counter()
                r = ndt.align(scan, prior)
                t1 = time.perf_counter()
            dt, dr = synth.pose_error(r["T64"], T)
            res["ndt"]["err"].append(dt); res["ndt"]["rot"].append(dr); res["ndt"]["ms"].append(1e3 * (t1 - t0)); res["ndt"]["dev_ms"].append(ndt.stats()["align_ms"])
            res["ndt"]["it"].append(r["iterations"])
            for name, obj in (("ndt_ls", ndt_ls), ("ndt_pyr", pyr)):
                for rep in range(2):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    r = obj.align(scan, prior)
                    t1 = time.perf_counter()
                dt, dr = synth.pose_error(r["T64"], T)
                levels = r.get("per_level", [r])
                v = res[name]
                v["err"].append(dt); v["rot"].append(dr); v["ms"].append(1e3 * (t1 - t0)); v["it"].append(sum(p["iterations"] for p in levels))
                v["dev_ms"].append(sum(lv.stats()["align_ms"] for lv in pyr.levels) if obj is pyr else obj.stats()["align_ms"])
                v["stalled"].append(bool(r["flags"] & api.SF_NDT_FLAG_LINE_SEARCH_STALLED))
            icp.set_source(scan)
            for rep in range(2):
                icp.set_initial_transformation(prior)
                ctx.synchronize()
                t0 = time.perf_counter()
                r = icp.align("p2plane")
                t1 = time.perf_counter()
            dt, dr = synth.pose_error(r["T64"], T)
            res["icp"]["err"].append(dt); res["icp"]["rot"].append(dr); res["icp"]["ms"].append(1e3 * (t1 - t0)); res["icp"]["it"].append(r["iterations"])
        line = dict(leg="align", prior_off_m=off, prior_yaw_deg=yaw, scans=len(scans), scan_points=int(np.median([len(s) for s in scans])), ndt_resolution_m=args.resolution,
                    icp_max_corr_m=args.icp_corr, pyramid_levels_m=list(args.levels))
        for name, v in res.items():
            line.update({name + "_median_err_m": float(np.median(v["err"])), name + "_median_err_rad": float(np.median(v["rot"])),
                         name + "_within_5cm": float(np.mean(np.array(v["err"]) < 0.05)), name + "_ms": float(np.median(v["ms"])),
                         name + "_median_iterations": float(np.median(v["it"]))})
        for name in ("ndt", "ndt_ls", "ndt_pyr"):
            line[name + "_device_ms"] = float(np.median(res[name]["dev_ms"]))
        for name in ("ndt_ls", "ndt_pyr"):                         # (of a pyramid: the last level's flag)
            line[name + "_stalled"] = float(np.mean(res[name]["stalled"]))
        line["both_within_5cm"] = float(np.mean((np.array(res["ndt"]["err"]) < 0.05) & (np.array(res["icp"]["err"]) < 0.05)))
        emit(**line, **common)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
