#!/usr/bin/env python3
"""A growth step of the map at size (`*map_cloud += *cloud` + VoxelGrid + setTargetPointCloud: global_map_frames_manager.cpp:131,
142-146, icp_point_to_point.cpp:49-55): sf_cloud_voxel_merge followed by sf_map_build, against the same merge followed by
sf_map_patch.  The map is a voxel-filtered uniform volume of --map-points raw points; every step adds --scans registered
scans of --scan-points points, half of them re-observing the map and half beyond its +x face.  One JSON line.
--normals RADIUS adds two legs on the same workload for a map that keeps normals (point-to-plane registration): "patch + full
estimate" (sf_map_patch, then sf_map_estimate_normals over the whole map) and "patch with carry" (sf_map_set_normals_carry:
the normals ride along with the patch and are estimated again only where the merge changed a neighbourhood), and compares
the two results bit for bit after the last step.  Every leg also lists the times of its steps (step_ms_all: merge + index, ms), for a
caller that needs the spread behind the medians.
   python tools/growth_bench.py [--map-points 20000000] [--steps 12] [--normals 0.25]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slam_sensor_fusion_amd import api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=20_000_000)
    ap.add_argument("--scans", type=int, default=10)
    ap.add_argument("--scan-points", type=int, default=20_000)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--cell", type=float, default=0.25)
    ap.add_argument("--normals", type=float, default=0.0, metavar="RADIUS", help="also time the growth step of a map with normals of this radius: patch + full estimate against patch with carry")
    ap.add_argument("--merge-min", type=int, default=-1, help="sf_cloud_voxel_merge_min_points (map size from which the filter merges; -1: the library's default)")
    args = ap.parse_args()
    ctx = api.Context(0)
    if args.merge_min >= 0:
        api.voxel_merge_min_points(args.merge_min)
    raw = synth.make_map(args.map_points)
    L = float(raw[:, 0].max())
    out = {}
    full_normals = None
    for how in ("build", "patch") + (("patch_full_estimate", "patch_carry") if args.normals > 0 else ()):
        rng = np.random.default_rng(3)
        cloud = api.Cloud(ctx, raw)
        cloud.voxel_downsample(0.1, "pcl")
        n0 = len(cloud)
        mp = api.Map(ctx, cloud, args.cell)
        if how in ("patch_full_estimate", "patch_carry"):
            mp.estimate_normals(args.normals)
            mp.set_normals_carry(how == "patch_carry")
        ds = None
        t_merge, t_index, patched, n_merged = [], [], 0, 0
        t_normals, redone, carried = [], [], 0
        for k in range(args.steps + 2):
            m = args.scans * args.scan_points
            seen = (np.stack([rng.uniform(L - 6.0, L - 1.0, m // 2), rng.uniform(-L + 1, L - 1, m // 2), rng.uniform(-4.5, 4.5, m // 2)], 1)).astype(np.float32)
            new = (np.stack([rng.uniform(L - 1.0, L + 0.05 * (k + 1), m - m // 2), rng.uniform(-L + 1, L - 1, m - m // 2), rng.uniform(-4.5, 4.5, m - m // 2)], 1)).astype(np.float32)
            pending = api.Cloud(ctx, np.concatenate([seen, new]))
            ctx.synchronize()
            t0 = time.perf_counter()
            _, merged = cloud.voxel_merge(pending, 0.1)
            ctx.synchronize()
            t1 = time.perf_counter()
            if how == "build":
                mp.build(cloud, args.cell)
            else:
                patched += int(mp.patch(cloud))
            ctx.synchronize()
            t2 = time.perf_counter()
            if how == "patch_full_estimate":                          # the only way to normals without the carry: the whole map again
                mp.estimate_normals(args.normals)
                ctx.synchronize()
            t3 = time.perf_counter()
            n_merged += int(merged)
            if k >= 2:
                t_merge.append((t1 - t0) * 1e3)
                t_index.append((t3 - t1) * 1e3)
                t_normals.append((t3 - t2) * 1e3)
                if how == "patch_carry":
                    info = mp.normals_carry_info()
                    carried += int(info[0] == 1)
                    redone.append(info[2] / max(info[3], 1))
                elif how == "patch_full_estimate":
                    redone.append(1.0)
        out[how] = dict(merge_ms_median=float(np.median(t_merge)), index_ms_median=float(np.median(t_index)), step_ms_median=float(np.median(np.add(t_merge, t_index))),
                        step_ms_max=float(np.max(np.add(t_merge, t_index))), step_ms_all=[round(float(t), 4) for t in np.add(t_merge, t_index)], merged_steps=n_merged, patched_steps=patched, map_points_start_end=[int(n0), int(len(cloud))])
        if how in ("patch_full_estimate", "patch_carry"):
            # the normals' share of the step: the estimate itself / what the patch takes beyond the plain patch leg of this run
            nrm_ms = float(np.median(t_normals)) if how == "patch_full_estimate" else out[how]["index_ms_median"] - out["patch"]["index_ms_median"]
            out[how].update(normals_radius=args.normals, normals_ms_median=nrm_ms, normals_share_of_step=nrm_ms / out[how]["step_ms_median"],
                            points_reestimated_over_map_points_median=float(np.median(redone)), points_reestimated_over_map_points_max=float(np.max(redone)))
            nrm, cnt = mp.download_normals()
            if how == "patch_full_estimate":
                full_normals = (nrm, cnt)
            else:
                out[how]["carried_steps"] = carried
                out["carried_normals_equal_full"] = bool(nrm.shape == full_normals[0].shape and np.array_equal(nrm.view(np.uint32), full_normals[0].view(np.uint32))
                                                         and np.array_equal(cnt, full_normals[1]))
                out["carried_step_over_full_estimate_step"] = out["patch_carry"]["step_ms_median"] / out["patch_full_estimate"]["step_ms_median"]
            del nrm, cnt
        if how == "patch":                                            # the index after the last step equals a build of the same cloud
            a, b = mp.index(), api.Map(ctx, cloud, args.cell).index()
            out["patched_index_equals_build"] = bool(all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("pts4", "cell_start")))
        cell, dims = mp.cell_size()
        out["cell_m"], out["grid"] = cell, list(dims)
        del mp, cloud
    print(json.dumps(dict(workload="growth step: %d scans x %d points merged into a voxel-filtered map (leaf 0.1 m), index cell %.2f m; host clock around the calls, %d steps"
                                   % (args.scans, args.scan_points, args.cell, args.steps), **out)))


if __name__ == "__main__":
    main()
