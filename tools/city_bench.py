#!/usr/bin/env python3
"""The bench's registration step on a SENSOR-shaped workload (not BASELINE's metric config: an extra measurement): ring scans
(rings x 2032 azimuths, ray cast) of a synthetic city registered against its voxel-filtered surface map, `--batch` scans in
flight, 20 point-to-plane iterations, each scan from its own pose with its own prior error.  Surfaces make the occupied
map cells dense and the neighbour structure anisotropic, and a scan converges from a per-scan prior instead of the metric
config's common 0.1 m offset -- what the reference's callback sees (a cropped ring scan and a blended prior,
localization_node.cpp:292-305,329-337).

One JSON line per (rings, prior error) case: scans/s with the library's defaults, with the frozen pairs off, with the neighbour
reuse off; per-launch times, the share of queries that search per launch, and sf_icp_freeze_stats (froze / thawed / voided /
active share).  Frozen pairs need wide scans (include/slamfusion.h, sf_icp_set_wide_scan_points): above 131 072 points, or above
65 536 in a batch that no single launch could take -- a 64-ring scan (<= 130 048 returns) in a batch of 64 qualifies.
--dynamic-boxes N adds N seeded car-sized boxes (4.5 x 1.8 x 1.5 m, on the ground around the sensor positions) to the world the
scans are ray cast in but not to the map (parked cars, dynamic objects); --robust KIND:K adds a run under that robust kernel
(sf_icp_set_robust_kernel, e.g. tukey:0.1) to every case.  The pose errors against the ray-casting truth (median / p95 /
max, translation and rotation) are reported for the plain run and, under "robust", for the robust one; a robust kernel
keeps P2PLANE from freezing, so its fair throughput baseline is scans_per_s_no_freeze.
--covariance adds a run with the pose covariance on (sf_icp_set_covariance, degeneracy thresholds 0.03 / 1.0 m^2): per scan the
smallest normalised eigenvalue of the marginal translation / rotation information and the flags, and scans/s with the switch
off and on (same object, same settings).  --tunnel replaces the city by synth.make_tunnel (walls along x, ends out of range,
40 m rays): the degenerate scene, where the translation flag is expected on every scan.
--normals-knn K estimates the map normals from each point's K nearest map points (sf_map_estimate_normals_knn) instead of the
0.25 m radius: every figure is then for the k-NN normals, and "normals" holds the share of map points with fewer than 3
neighbours under both forms and the pose errors of the same scans registered against the radius normals.
   python tools/city_bench.py [--map-points 10000000] [--batch 64] [--rings 64 128] [--prior 0.06:0.3 0.3:1.5] [--dynamic-boxes 40] [--robust tukey:0.1] [--covariance [--tunnel]] [--normals-knn 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slam_sensor_fusion_amd import api, synth  # noqa: E402


def timed(icp, ctx, mode, steps, batch):
    icp.align_batch(mode)
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        icp.align_batch_async(mode)
    ctx.synchronize()
    return batch * steps / (time.perf_counter() - t0)


def pose_errors(res, truths):
    errs = np.array([synth.pose_error(r["T64"], T) for r, T in zip(res, truths)])
    return {"max_translation_err_m": float(errs[:, 0].max()), "max_rotation_err_rad": float(errs[:, 1].max()),
            "median_translation_err_m": float(np.median(errs[:, 0])), "p95_translation_err_m": float(np.percentile(errs[:, 0], 95)),
            "median_rotation_err_deg": float(np.degrees(np.median(errs[:, 1]))), "p95_rotation_err_deg": float(np.degrees(np.percentile(errs[:, 1], 95)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=10_000_000)
    ap.add_argument("--extent", type=float, default=240.0)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rings", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--prior", nargs="+", default=["0.06:0.3", "0.3:1.5"], help="1-sigma prior error per axis, metres:degrees")
    ap.add_argument("--wide-from", type=int, default=0, help="sf_icp_set_wide_scan_points (0: the library's own rule -- above 131 072 points, or above 65 536 in a batch no single launch could take)")
    ap.add_argument("--dynamic-boxes", type=int, default=0, help="car-sized boxes in the ray-cast world that the map does not hold")
    ap.add_argument("--robust", default=None, help="KIND:K -- also register under this robust kernel (huber, cauchy, tukey, gm; K in metres)")
    ap.add_argument("--covariance", action="store_true", help="also register with sf_icp_set_covariance on: eigenvalues, flags, scans/s off vs on")
    ap.add_argument("--normals-knn", type=int, default=0, metavar="K", help="map normals from the K nearest map points instead of the 0.25 m radius; reports both")
    ap.add_argument("--tunnel", action="store_true", help="the degenerate scene (synth.make_tunnel) instead of the city")
    args = ap.parse_args()
    mode = "p2plane"
    ctx = api.Context(0)
    if args.tunnel:
        boxes, raw = synth.make_tunnel(m_points=args.map_points)
    else:
        boxes = synth.make_city(args.extent, int(120 * (args.extent / 240.0) ** 2))
        raw = synth.sample_city(boxes, args.extent, args.map_points)
    cloud = api.Cloud(ctx, raw)
    del raw
    cloud.voxel_downsample(0.1, "pcl")
    n_map = len(cloud)
    mp = api.Map(ctx, cloud, 0.25)
    mp.estimate_normals(0.25)
    normals_info = None
    if args.normals_knn > 0:
        cnt_r = mp.download_normals()[1]
        mp.estimate_normals_knn(args.normals_knn)
        cnt_k = mp.download_normals()[1]
        normals_info = dict(k=args.normals_knn, radius_m=0.25, share_below_3_radius=float((cnt_r < 3).mean()), share_below_3_knn=float((cnt_k < 3).mean()),
                            share_below_6_radius=float((cnt_r < 6).mean()), neighbours_radius_median=float(np.median(cnt_r)), neighbours_radius_p99=float(np.percentile(cnt_r, 99)))
        del cnt_r, cnt_k
    cell, dims = mp.cell_size()
    cars = synth.make_cars(boxes, [(0.0, 0.0)], args.dynamic_boxes, radius=(3.0, 20.0)) if args.dynamic_boxes > 0 else np.zeros((0, 6))
    world = np.r_[boxes, cars]
    for rings in args.rings:
        rng = np.random.default_rng(77)
        truths, scans = [], []
        while len(scans) < args.batch:
            xy = rng.uniform(-12.0, 12.0, 2)
            if args.tunnel: # along the axis, between the walls, heading within 10 degrees of it either way
                T = synth.make_T((xy[0], xy[1] / 6.0, 1.8), (0.0, 0.0, rng.uniform(-10, 10) + 180.0 * rng.integers(2)))
                s = synth.raycast_scan(world, T, rings=rings, max_range=40.0, seed=synth.CITY_SEED + 10 + len(scans))
            else:
                T = synth.make_T((xy[0], xy[1], 1.8), (0.0, 0.0, rng.uniform(0, 360)))
                s = synth.raycast_scan(world, T, rings=rings, seed=synth.CITY_SEED + 10 + len(scans))
            if len(s) < 0.45 * rings * 2032:
                continue
            truths.append(T)
            scans.append(s)
        n = min(len(s) for s in scans)
        scans = np.stack([s[rng.choice(len(s), n, replace=False)] for s in scans])     # a common length, uniformly thinned
        for prior in args.prior:
            sig_t, sig_r = (float(v) for v in prior.split(":"))
            prng = np.random.default_rng(78)
            inits = np.stack([T @ synth.make_T(prng.normal(0, sig_t, 3), prng.normal(0, sig_r, 3)) for T in truths])
            icp = api.Icp(ctx, 0.5, args.iters, 0.05, 1e-5)
            icp.set_target(mp)
            icp.use_graph(True)
            if args.wide_from > 0:
                icp.set_wide_scan_points(args.wide_from)
            icp.set_source_batch(scans)
            icp.set_initial_batch(inits)
            out = {}
            res = icp.align_batch(mode)
            out.update(pose_errors(res, truths))
            out["scans_per_s"] = timed(icp, ctx, mode, args.steps, args.batch)
            fs = icp.freeze_stats()
            out["freeze_stats"] = dict(fs, active_share=fs["active_queries"] / float(n * args.batch), scans=args.batch, wide_from=args.wide_from or "library rule")
            icp.use_graph(False)
            icp.profile_enable(True)
            icp.align_batch_async(mode)
            ctx.synchronize()
            ms, sq, _ = icp.profile_launches()
            icp.profile_enable(False)
            icp.use_graph(True)
            out["per_launch_us"] = [round(float(v) * 1e3, 1) for v in ms]
            out["per_launch_queries_searching_frac"] = [round(float(v) / (n * args.batch), 4) for v in sq]
            icp.set_freeze(False)
            off = icp.align_batch(mode)
            out["scans_per_s_no_freeze"] = timed(icp, ctx, mode, args.steps, args.batch)
            out["freeze_vs_no_freeze_max_pose_diff_m"] = max(synth.pose_error(a["T64"], b["T64"])[0] for a, b in zip(res, off))
            icp.set_freeze("auto")
            icp.set_nn_reuse(False)
            out["scans_per_s_no_reuse"] = timed(icp, ctx, mode, max(2, args.steps // 2), args.batch)
            icp.set_nn_reuse(True)
            if args.robust:
                kind, k = args.robust.split(":")
                icp.set_robust_kernel(kind, float(k))
                rob = pose_errors(icp.align_batch(mode), truths)
                rob["scans_per_s"] = timed(icp, ctx, mode, args.steps, args.batch)
                out["robust"] = dict(kernel=args.robust, **rob)
                icp.set_robust_kernel("none")
            if args.covariance:
                out["scans_per_s_covariance_off"] = timed(icp, ctx, mode, args.steps, args.batch)
                icp.set_degeneracy_thresholds(0.03, 1.0)
                icp.set_covariance(True)
                icp.align_batch(mode)
                covs = icp.fetch_covariance()
                out["scans_per_s_covariance_on"] = timed(icp, ctx, mode, args.steps, args.batch)
                out["covariance"] = dict(min_trans_info=[round(float(c["trans_info"][0]), 5) for c in covs], min_rot_info_m2=[round(float(c["rot_info"][0]), 3) for c in covs],
                                         flags=[int(c["flags"]) for c in covs], sigma_hat_m=[round(float(np.sqrt(c["sigma2_hat"])), 4) for c in covs],
                                         weakest_trans_dir_of_scan_0=[round(float(v), 4) for v in covs[0]["trans_dir"][0]])
                icp.set_covariance(False)
            if normals_info is not None:                             # the same scans against the radius normals
                mp.estimate_normals(0.25)
                icp.set_target(mp)
                icp.set_source_batch(scans)
                icp.set_initial_batch(inits)
                rad = pose_errors(icp.align_batch(mode), truths)
                mp.estimate_normals_knn(args.normals_knn)
                out["normals"] = dict(normals_info, median_translation_err_m_knn=out["median_translation_err_m"], median_translation_err_m_radius=rad["median_translation_err_m"],
                                      median_rotation_err_deg_knn=out["median_rotation_err_deg"], median_rotation_err_deg_radius=rad["median_rotation_err_deg"],
                                      p95_translation_err_m_knn=out["p95_translation_err_m"], p95_translation_err_m_radius=rad["p95_translation_err_m"])
            icp.close()
            print(json.dumps(dict(workload="ring scans (%d x 2032 rays) vs a %.0f m synthetic %s, %d samples -> %d map points (voxel 0.1 m), %d scans in flight x %d points, "
                                           "%d %s iterations, prior error %.2f m / %.1f deg (1 sigma per axis)" % (rings, args.extent, "tunnel" if args.tunnel else "city", args.map_points, n_map, args.batch, n, args.iters,
                                                                                                                  mode, sig_t, sig_r),
                                  rings=rings, dynamic_boxes=len(cars), prior_sigma_m=sig_t, prior_sigma_deg=sig_r, points_per_scan=int(n), cell_m=cell, grid=list(dims), **out)), flush=True)


if __name__ == "__main__":
    main()
