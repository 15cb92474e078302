#!/usr/bin/env python3
"""Pose estimation from matches (sf_cloud_register_pairs, api.global_register) on a terrain map (synth.make_terrain) with a local scan
under a large unknown pose: 140 degrees of yaw and 12 m.  Legs: the match (the share of the mutual matches that are right -- the
column DESIGN.md section 21 found empty on the city); hyp_ms, score_ms and refit_ms (device events) at 4 096, 65 536 and 2^20
hypotheses, with the edge check at 0.9 (production: few hypotheses survive to be scored) and without it (every hypothesis is
scored: the scoring kernel at scale), every leg warmed up once, then alternating --reps times, medians reported.  Per scoring leg:
the transform-pair tests per second and the VALU floor of the same work -- ceil(survivors / 64) waves x m pairs x
CYCLES_PER_WAVE_PAIR on each of CUs x 4 SIMDs; the clock is the shader clock the driver reported while the legs ran (sysfs,
pp_dpm_sclk), the nominal one only where that cannot be read.  Then the pose error against the truth before and after ICP, for the
refit pose alone and for the best of the top 8 candidates run as one batch.  One JSON line per leg to stdout and to --out.
   python tools/register_bench.py [--extent 60] [--reps 5] [--out profiles/register_bench.jsonl]"""
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

# SIMD cycles per wave and pair in the inner loop of k_reg_score (profiles/register_score_isa.txt: one trip is 8 pairs per lane --
# 48 packed multiplies and 56 packed adds, two pairs each, at 4 cycles; 8 compares, 4 selects and 4 add-with-carry at 2)
CYCLES_PER_WAVE_PAIR = (104 * 4 + 16 * 2) / 8.0
SIMDS_PER_CU = 4


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


def true_pose():
    a = np.deg2rad(140.0)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = (7.0, -9.0, 3.6)
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--extent", type=float, default=60.0)
    ap.add_argument("--spacing", type=float, default=0.2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--scan-radius", type=float, default=8.0)
    ap.add_argument("--sigma", type=float, default=0.005)
    ap.add_argument("--feature-radius", type=float, default=1.0)
    ap.add_argument("--normal-radius", type=float, default=0.5)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--hypotheses", type=int, nargs="*", default=[4096, 65536, 1 << 20])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register_bench.jsonl"))
    args = ap.parse_args()
    ctx = api.Context(0)
    T = true_pose()
    terrain = synth.make_terrain(args.extent, args.spacing, args.seed)
    scan, idx = synth.make_local_scan(terrain, (2.0, -1.0), args.scan_radius, T, args.sigma, args.seed + 1)
    map_cloud, scan_cloud = api.Cloud(ctx, terrain), api.Cloud(ctx, scan)
    mp = api.Map(ctx, map_cloud, 0.5)
    mp.estimate_normals(args.normal_radius)
    f_map = mp.compute_fpfh(args.feature_radius, "direction", (0, 0, 1))[0]
    f_scan = scan_cloud.compute_fpfh(args.normal_radius, args.feature_radius, "direction", (0, 0, 1))[0]
    match = f_scan.match(f_map, mutual=True, profile=True)
    pairs = match["pairs"]
    m = len(pairs)
    right = idx[pairs[:, 0]] == pairs[:, 1]
    common = dict(map_points=len(terrain), scan_points=len(scan), extent_m=args.extent, spacing=args.spacing, sigma=args.sigma, feature_radius=args.feature_radius,
                  threshold=args.threshold, reps=args.reps, device=ctx.device_name())
    lines = [dict(leg="match", mutual_matches=m, right=int(right.sum()), right_share=float(right.mean()) if m else 0.0, match_ms=match["stats"]["match_ms"], **common)]

    legs = [(h, sim) for h in args.hypotheses for sim in (0.9, 0.0)]
    times = {leg: dict(hyp_ms=[], score_ms=[], refit_ms=[]) for leg in legs}
    did = {}
    sampler = ClockSampler()
    sampler.start()
    for rep in range(args.reps + 1):                                  # rep 0: the warm-up of every leg
        for leg in legs:
            h, sim = leg
            r = scan_cloud.register_pairs(map_cloud, pairs, args.threshold, sim, h, 2, 3, 8, args.seed, profile=True)
            did[leg] = r
            if rep > 0:
                for key in times[leg]:
                    times[leg][key].append(r["stats"][key])
    sampler.stop = True
    sampler.join()
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
    cycles_per_s = cus * SIMDS_PER_CU * clock_mhz * 1e6
    common.update(compute_units=cus, clock_mhz=clock_mhz, clock_source=clock_source, nominal_clock_mhz=nominal, pairs=m)
    for leg in legs:
        h, sim = leg
        st = did[leg]["stats"]
        med = {key: float(np.median(v)) for key, v in times[leg].items()}
        waves = -(-st["n_scored"] // 64)
        floor = waves * m * CYCLES_PER_WAVE_PAIR / cycles_per_s * 1e3
        dt, dr = synth.pose_error(did[leg]["T"], T)
        lines.append(dict(leg="register", hypotheses=h, edge_similarity=sim, **med, score_ms_all=[round(t, 4) for t in times[leg]["score_ms"]],
                          hyp_ms_all=[round(t, 4) for t in times[leg]["hyp_ms"]], survivors=st["n_scored"], tests=float(st["n_scored"]) * m,
                          tests_per_s=float(st["n_scored"]) * m / (med["score_ms"] * 1e-3) if med["score_ms"] > 0 else None, cycles_per_wave_pair=CYCLES_PER_WAVE_PAIR,
                          valu_floor_ms=floor, score_over_floor=med["score_ms"] / floor if floor > 0 else None, hypotheses_per_s=h / (med["hyp_ms"] * 1e-3),
                          pose_error_m=dt, pose_error_rad=dr, stats={k: v for k, v in st.items() if not k.endswith("_ms")}, **common))

    def factory(batch):
        icp = api.Icp(ctx, 0.5, 30)
        icp.set_target(mp)
        return icp
    for top_k in (0, 8):
        g = api.global_register(scan_cloud, f_scan, map_cloud, f_map, args.threshold, num_hypotheses=4096, top_k=top_k, seed=args.seed, icp=factory)
        before, after = synth.pose_error(g["ransac"]["T"], T), synth.pose_error(g["T"], T)
        lines.append(dict(leg="global_register", top_k=top_k, batch=len(g["icp"]), chosen=g["chosen"], ransac_fitness=g["ransac"]["stats"]["fitness"], icp_fitness=g["fitness"],
                          icp_rmse=g["rmse"], icp_iterations=[r["iterations"] for r in g["icp"]], pose_error_before_icp_m=before[0], pose_error_before_icp_rad=before[1],
                          pose_error_after_icp_m=after[0], pose_error_after_icp_rad=after[1], **common))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
