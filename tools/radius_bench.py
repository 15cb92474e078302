#!/usr/bin/env python3
"""The radius search (sf_map_radius_graph, sf_map_radius_search) on a city surface map, beside its yardsticks in the
same process: sf_map_radius_outliers at the same radius (the count pass of the graph form is its walk in its order) and
sf_map_knn(64, r2) on the same queries (the hybrid route).  The map is synth.sample_city on synth.make_city (the extent scaled to
keep city_bench's density), voxel-filtered at 0.1 m; the index cell is 0.25 m; the search queries are one ray-cast ring scan from a
street position, in the map frame.  Per radius the legs -- radius_outliers, the graph and the search in both orders and both fill
forms, knn -- are warmed up once and then alternate --reps times.  The times are device events around the kernel launches
(sf_map_profile_launches; the radius calls split theirs into count + scan, fill, sort: sf_map_radius_launch_ms), medians with
min / max; the fill is also reported as the bytes it writes over its time.  The rows stay on the device (nothing is downloaded).
A total beyond 2^32 - 2 entries is reported as refused and the tool goes on.  One JSON line per leg to stdout and --out, and the
lane / wave table to --ab.
   python tools/radius_bench.py [--map-points 2000000] [--reps 5] [--out profiles/radius_search_bench.jsonl] [--ab profiles/radius_search_ab.txt]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_sensor_fusion_amd import api, synth  # noqa: E402

SF_ERR_OVERFLOW = -5


def radius_call(mp, queries, radius, order):
    """the C call without the download: -> (return code, stats dict)"""
    st = api.RadiusStats()
    o = api.RADIUS_ORDERS[order]
    if queries is None:
        rc = mp.lib.sf_map_radius_graph(mp.h, C.c_double(radius), C.c_int(o), None, C.byref(st))
    else:
        rc = mp.lib.sf_map_radius_search(mp.h, queries.ctypes.data_as(C.c_void_p), C.c_int64(len(queries)), C.c_double(radius), C.c_int(o), None, C.byref(st))
    return rc, st.as_dict()


def spread(t):
    return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=2_000_000)
    ap.add_argument("--cell", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--radii", type=float, nargs="*", default=[0.15, 0.25, 0.4])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radius_search_bench.jsonl"))
    ap.add_argument("--ab", default=os.path.join(ROOT, "profiles", "radius_search_ab.txt"))
    args = ap.parse_args()
    ctx = api.Context(0)
    extent = 240.0 * float(np.sqrt(args.map_points / 10_000_000))
    boxes = synth.make_city(extent, max(1, int(120 * (extent / 240.0) ** 2)))
    cloud = api.Cloud(ctx, synth.sample_city(boxes, extent, args.map_points))
    cloud.voxel_downsample(0.1, "pcl")
    n_map = len(cloud)
    mp = api.Map(ctx, cloud, args.cell)
    cell, dims = mp.cell_size()
    mp.profile_launches(True)
    # the scan: seen from 1.8 m above the ground at a street position, turned by 30 degrees, brought into the map frame
    ground = [(x, y) for x in np.linspace(-0.3, 0.3, 13) * extent for y in np.linspace(-0.3, 0.3, 13) * extent
              if not np.any((boxes[:, 0] - 3 < x) & (x < boxes[:, 3] + 3) & (boxes[:, 1] - 3 < y) & (y < boxes[:, 4] + 3))]
    sx, sy = ground[len(ground) // 2]
    T = synth.make_T((sx, sy, 1.8), (0.0, 0.0, 30.0))
    scan = np.ascontiguousarray((synth.raycast_scan(boxes, T).astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32))
    common = dict(map_points=n_map, scan_points=len(scan), extent_m=extent, cell_m=cell, grid=list(dims), reps=args.reps, device=ctx.device_name())
    lines, table = [], []

    def emit(**kw):
        lines.append(dict(kw, **common))
        print(json.dumps(lines[-1]), flush=True)

    for r in args.radii:
        legs = [("radius_outliers", None, None, None), ("knn64", "scan", None, None)]
        legs += [(kind, kind_q, order, fill) for kind, kind_q in (("radius_graph", "map"), ("radius_search", "scan")) for order in ("index", "distance") for fill in ("lane", "wave")]
        times = {leg: [] for leg in legs}
        stats, refused = {}, set()
        for rep in range(args.reps + 1):                              # rep 0: the warm-up of every leg
            for leg in legs:
                kind, kind_q, order, fill = leg
                if leg in refused:
                    continue
                if kind == "radius_outliers":
                    mp.radius_outliers(r, 5)
                    t = (mp.last_launch_ms(),)
                elif kind == "knn64":
                    mp.knn(scan, 64, np.float32(r * r))
                    t = (mp.last_launch_ms(),)
                else:
                    mp.set_radius_fill(fill)
                    rc, st = radius_call(mp, None if kind == "radius_graph" else scan, r, order)
                    if rc == SF_ERR_OVERFLOW:
                        refused.add(leg)
                        emit(leg=kind, radius_m=r, order=order, fill=fill, refused="SF_ERR_OVERFLOW: more than 2^32 - 2 entries", message=mp.lib.sf_last_error().decode())
                        continue
                    api._check(rc)
                    stats[leg] = st
                    t = mp.radius_launch_ms()
                if rep > 0:
                    times[leg].append(t)
        mp.set_radius_fill("auto")
        for leg in legs:
            kind, kind_q, order, fill = leg
            if leg in refused:
                continue
            t = np.array(times[leg], np.float64)
            if kind in ("radius_outliers", "knn64"):
                emit(leg=kind, radius_m=r, kernel_ms=spread(t[:, 0]), queries=n_map if kind == "radius_outliers" else len(scan))
                continue
            st = stats[leg]
            entry_bytes = 8 if order == "index" else 12                # id + d2, or id + the 64-bit key
            fill_ms = spread(t[:, 1])
            out = dict(leg=kind, radius_m=r, order=order, fill=fill, stats=st, mean_row=st["total"] / max(st["n_searched"], 1), count_scan_ms=spread(t[:, 0]), fill_ms=fill_ms,
                       sort_ms=spread(t[:, 2]), total_ms=spread(t.sum(1)), fill_bytes=st["total"] * entry_bytes, fill_GBps=st["total"] * entry_bytes / (fill_ms["median"] * 1e-3) / 1e9)
            if order == "distance":
                out["sort_over_fill"] = out["sort_ms"]["median"] / fill_ms["median"]
            emit(**out)
        # the lane / wave table, the count pass beside its yardstick, the hybrid route
        med = lambda leg, k: float(np.median(np.array(times[leg])[:, k])) if leg not in refused else float("nan")
        for kind, kind_q in (("radius_graph", "map"), ("radius_search", "scan")):
            for order in ("index", "distance"):
                a, b = (kind, kind_q, order, "lane"), (kind, kind_q, order, "wave")
                if a in refused or b in refused:
                    table.append("%-14s r %.2f %-8s refused (SF_ERR_OVERFLOW)" % (kind, r, order))
                    continue
                table.append("%-14s r %.2f %-8s mean row %7.1f  max %5d  fill lane %8.3f ms  wave %8.3f ms  wave/lane %5.2f  count+scan %8.3f ms  sort %8.3f ms" %
                             (kind, r, order, stats[a]["total"] / max(stats[a]["n_searched"], 1), stats[a]["max_count"], med(a, 1), med(b, 1), med(b, 1) / med(a, 1), med(a, 0), med(a, 2)))
        g = ("radius_graph", "map", "index", "lane")
        if g not in refused:
            ro = np.array(times[("radius_outliers", None, None, None)])[:, 0]
            table.append("count pass     r %.2f graph count+scan %8.3f ms [%.3f, %.3f]   radius_outliers %8.3f ms [%.3f, %.3f]   ratio %.3f" %
                         (r, med(g, 0), np.min(np.array(times[g])[:, 0]), np.max(np.array(times[g])[:, 0]), np.median(ro), ro.min(), ro.max(), med(g, 0) / np.median(ro)))
        s = ("radius_search", "scan", "distance", "lane")
        if s not in refused:
            kn = np.array(times[("knn64", "scan", None, None)])[:, 0]
            best = min(float(np.median(np.array(times[(s[0], s[1], s[2], f)]).sum(1))) for f in ("lane", "wave"))
            table.append("hybrid route   r %.2f scan: distance-ordered search %8.3f ms (the faster fill)   knn(64, r2) %8.3f ms [%.3f, %.3f]" % (r, best, np.median(kn), kn.min(), kn.max()))
    for path, text in ((args.out, "".join(json.dumps(line) + "\n" for line in lines)),
                       (args.ab, "# tools/radius_bench.py on %s: %d map points, %d scan points, cell %g m, medians of %d\n" % (ctx.device_name(), n_map, len(scan), cell, args.reps) + "\n".join(table) + "\n")):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
    print("\n".join(table))


if __name__ == "__main__":
    main()
