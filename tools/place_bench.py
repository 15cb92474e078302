#!/usr/bin/env python3
"""Scan Context place recognition (sf_cloud_scan_context, sf_place_db_distances, sf_place_db_query) on the city of
synth.make_city(300, 150).  Keyframes are ray-cast (32 rings x 360 azimuths, sensor 2 m up) from the points of a 20 m lattice that lie
outside the buildings; a database of N entries is those descriptors padded with seeded perturbations of them (every height scaled by
a factor in [0.9, 1.1], 5 % of the bins emptied, the columns rolled by a seeded shift).
Legs, each warmed up once, then --reps repetitions, medians, all by device events:
  build            the fill and the two kernels of the descriptor of one 128-ring scan (about 250 k points);
  distances_N_Q    the match of Q = 1 and 64 queries against N = 256, 4 096 and 16 384 entries (the queries' unit columns included);
  select_N_Q       the selection of the 8 smallest (D, index) per query behind the same match (sf_place_db_query).
Each match stands beside two floors computed here: its float64 operations (2 Q N Ns^2 Nr: the rule's multiply and add are separate
instructions) at the float64 vector instruction rate, and the database's unit columns (8 N Nr Ns bytes) at the HBM rate.  Then what
the descriptor is worth: top-1 recall and shift correctness of queries cast --offsets metres off a keyframe under --yaws degrees,
against the real keyframes.  Nothing is gated.  One JSON line per leg and one summary; stdout and --out.
   python tools/place_bench.py [--reps 5] [--out profiles/place_bench.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_sensor_fusion_amd import api, synth  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
# MI355X: 157.3 TFLOP/s of float32 vector work counts a fused multiply-add as two; float64 vector instructions issue at half the
# float32 rate, and an unfused multiply or add is one operation an instruction
FP64_VECTOR_INSTR_PER_S = 157.3e12 / 2.0 / 2.0


def _yaw(yaw_deg, xyz):
    """[4, 4] map <- sensor: a yaw about z and a position"""
    a = np.radians(yaw_deg)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = xyz
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--keyframes", type=int, default=64)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 4096, 16384])
    ap.add_argument("--offsets", type=float, nargs="+", default=[0.0, 0.5, 1.0, 2.0, 3.0])
    ap.add_argument("--yaws", type=float, nargs="+", default=[0.0, 32.0, 90.0, -138.0])
    ap.add_argument("--skip-summary", action="store_true", help="only the timed legs (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_bench.jsonl"))
    args = ap.parse_args()
    ctx = api.Context(0)
    boxes = synth.make_city(300, 150)
    clear = lambda x, y, m=1.0: not ((boxes[:, 0] - m < x) & (x < boxes[:, 3] + m) & (boxes[:, 1] - m < y) & (y < boxes[:, 4] + m)).any()
    lattice = [(x, y) for y in np.arange(-100.0, 101.0, 20.0) for x in np.arange(-100.0, 101.0, 20.0) if clear(x, y)][:args.keyframes]
    cast = lambda T, seed, rings=32, az=360: synth.raycast_scan(boxes, T, rings=rings, azimuths=az, max_range=80.0, seed=seed)

    db = api.PlaceDB(ctx)
    prm = db.params
    Nr, Ns = prm["num_rings"], prm["num_sectors"]
    for k, (x, y) in enumerate(lattice):
        db.add(api.Cloud(ctx, cast(_yaw(0.0, (x, y, 2.0)), 7000 + k)), _yaw(0.0, (x, y, 2.0)))
    real, real_poses = db.download()

    def padded(n):
        """the real keyframes, then seeded perturbations of them, n rows in all"""
        rng = np.random.default_rng(n)
        out = [real[:n]]
        while sum(len(o) for o in out) < n:
            a = real * rng.uniform(0.9, 1.1, real.shape).astype(np.float32)
            a[rng.uniform(size=a.shape) < 0.05] = 0.0
            out.append(np.stack([np.roll(r, int(rng.integers(Ns)), axis=1) for r in a]))
        return np.concatenate(out)[:n]

    big_scan = cast(_yaw(0.0, lattice[len(lattice) // 2] + (2.0,)), 7999, rings=128, az=2032)
    big = api.Cloud(ctx, big_scan)
    q_rng = np.random.default_rng(99)
    queries = np.stack([np.roll(real[k % len(real)], int(q_rng.integers(Ns)), axis=1) for k in range(64)]) * q_rng.uniform(0.95, 1.05, (64, Nr, Ns)).astype(np.float32)

    times = {"build": []}
    for rep in range(args.reps + 1):                                  # rep 0: the warm-up
        ms = big.scan_context()[1]["device_ms"]
        if rep > 0:
            times["build"].append(ms)
    lines = []
    common = dict(shape=[Nr, Ns], keyframes=len(lattice), reps=args.reps, device=ctx.device_name())
    # the build reads 12 B a point and sends one 4-byte atomic a point; the bins are filled and read once
    build_bytes = (12 + 4) * len(big_scan) + 3 * 4 * Nr * Ns
    lines.append(dict(leg="build", ms=float(np.median(times["build"])), ms_all=[round(t, 4) for t in times["build"]], scan_points=len(big_scan), bytes_moved=build_bytes,
                      floor_hbm_ms=build_bytes / HBM_BYTES_PER_S * 1e3, **common))
    for n in args.sizes:
        bench = api.PlaceDB(ctx)
        bench.add_descriptors(padded(n))
        for q in (1, 64):
            match, match2, select = [], [], []
            for rep in range(args.reps + 1):
                a = bench.distances(queries[:q])[2]
                b = bench.query(queries[:q], 8)["stats"]
                if rep > 0:
                    match.append(a["match_ms"])
                    match2.append(b["match_ms"])
                    select.append(b["select_ms"])
            ops = 2.0 * q * n * Ns * Ns * Nr
            db_bytes = 8.0 * n * Nr * Ns
            floor_ops, floor_hbm = ops / FP64_VECTOR_INSTR_PER_S * 1e3, db_bytes / HBM_BYTES_PER_S * 1e3
            ms = float(np.median(match))
            lines.append(dict(leg="distances_%d_%d" % (n, q), ms=ms, ms_all=[round(t, 4) for t in match], ms_inside_query=float(np.median(match2)), entries=n, queries=q,
                              float64_ops=ops, floor_ops_ms=floor_ops, over_floor_ops=ms / floor_ops, database_bytes=db_bytes, floor_hbm_ms=floor_hbm,
                              over_floor_hbm=ms / floor_hbm, **common))
            lines.append(dict(leg="select_%d_%d" % (n, q), ms=float(np.median(select)), ms_all=[round(t, 4) for t in select], entries=n, queries=q, k=8,
                              bytes_read=8.0 * 8 * q * n, **common))
        bench.close()
    if not args.skip_summary:
        sites = [len(lattice) // 5, 2 * len(lattice) // 5, 3 * len(lattice) // 5, 4 * len(lattice) // 5]
        sweep = []
        for off in args.offsets:
            for yaw in args.yaws:
                right = shift_ok = total = 0
                gaps = []
                for s, kf in enumerate(sites):
                    ang = np.radians(40.0 + 90.0 * s)                 # the direction of the offset differs from site to site
                    x, y = lattice[kf][0] + off * np.cos(ang), lattice[kf][1] + off * np.sin(ang)
                    if not clear(x, y, 0.3):
                        continue
                    got = db.query_cloud(api.Cloud(ctx, cast(_yaw(yaw, (x, y, 2.0)), 8000 + 100 * s + int(10 * off) + int(abs(yaw)))), 2)
                    total += 1
                    hit = int(got["idx"][0, 0]) == kf
                    right += hit
                    shift_ok += hit and int(got["shift"][0, 0]) == int(round(yaw / (360.0 / Ns))) % Ns
                    gaps.append(float(got["dist"][0, 1] - got["dist"][0, 0]))
                sweep.append(dict(offset_m=off, yaw_deg=yaw, queries=total, top1=right, shift_right=shift_ok, smallest_gap_to_second=min(gaps) if gaps else None))
        total = sum(r["queries"] for r in sweep)
        lines.append(dict(leg="summary", top1_recall=sum(r["top1"] for r in sweep) / max(total, 1), shift_right=sum(r["shift_right"] for r in sweep) / max(total, 1),
                          queries=total, sweep=sweep, **common))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
