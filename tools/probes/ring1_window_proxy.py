#!/usr/bin/env python3
"""CPU proxy for the first trip of nn_search_wave and the ring-1 tasks that follow it (sf_nn.hpp: first_window, the mask of
the 11 tasks, round_task; DESIGN section 3, profiles/LADDER.md round 12): how many tasks does a query queue, how many rounds
does a wave of 64 walk, and how many lane accesses does it all take, when the first trip's four slots are filled from the
query's own ROW instead of its own cell alone?  numpy only.

A uniform map at the benchmark's density (95 points / m^3: 1.48 per 0.25 m cell); queries = map points + 1 cm noise + an
offset (the benchmark's start offset for launch 0, what is left of it one launch later, none for the steady search); the
window rule and the mask rule exactly as the kernel has them (gap * 0.998 < best), without a seed and without a cache.
One line per (offset, variant).
   python tools/probes/ring1_window_proxy.py [--queries 120000]"""
import argparse

import numpy as np

H = 0.25
VARIANTS = ("own_cell", "nearer_first", "right_then_left", "whole_row")   # SF_NN_ROW_WINDOW 0, 1, 2, 3


def first_window(s0, s1, s2, s3, gxm2, gxp2, variant="nearer_first"):
    """The first trip's window [lo, hi) over the own row's CSR range [s0, s3) (own cell [s1, s2)); arrays or scalars.
    gxm2 / gxp2: squared gaps to the left / right x neighbour, 3e38 where the grid has none."""
    s0, s1, s2, s3 = (np.asarray(v, np.int64) for v in (s0, s1, s2, s3))
    gxm2, gxp2 = np.asarray(gxm2, np.float32), np.asarray(gxp2, np.float32)
    cap = 8 if variant == "whole_row" else 4
    own = np.minimum(s2 - s1, cap)
    if variant == "own_cell":
        return s1, s1 + own
    idle = cap - own
    nl = np.where(gxm2 < np.float32(1.0e38), s1 - s0, 0)
    nr = np.where(gxp2 < np.float32(1.0e38), s3 - s2, 0)
    right_first = np.ones(np.shape(own), bool) if variant == "right_then_left" else gxp2 <= gxm2
    t1 = np.minimum(idle, np.where(right_first, nr, nl))
    t2 = np.minimum(idle - t1, np.where(right_first, nl, nr))
    return s1 - np.where(right_first, t2, t1), s1 + own + np.where(right_first, t1, t2)


def slot_row(s0, s1, s2, s3, gxm2, gxp2, start):
    """sf_nn.hpp slot_row: a neighbour whose gap does not pass the bound the search starts from is cut off the row the window
    is laid over (it could never be queued, so it gets no slot).  With the acceptance radius of 0.5 m as the start no gap of a
    0.25 m cell is cut; a seed's distance, from the second launch on, cuts most."""
    left = np.asarray(gxm2, np.float32) * np.float32(0.998) < np.float32(start)
    right = np.asarray(gxp2, np.float32) * np.float32(0.998) < np.float32(start)
    return np.where(left, s0, s1), s1, s2, np.where(right, s3, s2)


def residuals(s0, s1, s2, s3, lo, hi):
    """What the window leaves of the own row: tasks 0, 1 and 10 as half-open ranges (empty where a >= b)."""
    return (s0, np.minimum(lo, s1)), (np.maximum(hi, s2), s3), (np.maximum(hi, s1), s2)


def make_map(rng, lx=24.0, ly=24.0, lz=10.0, density=95.0):
    n = int(density * lx * ly * lz)
    p = np.c_[rng.uniform(0, lx, n), rng.uniform(0, ly, n), rng.uniform(0, lz, n)].astype(np.float32)
    dims = np.array([int(lx / H), int(ly / H), int(lz / H)])
    c = np.minimum((p / H).astype(np.int64), dims - 1)
    key = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    o = np.argsort(key, kind="stable")
    return p[o], np.searchsorted(key[o], np.arange(dims.prod() + 1)), dims, (lx, ly, lz)


def run(rng, world, off, nq, variant):
    p, start, dims, ext = world
    nx, ny = int(dims[0]), int(dims[1])
    q = p[rng.choice(len(p), nq, replace=False)].astype(np.float64) + rng.normal(0, 0.01, (nq, 3)) + np.asarray(off)
    q = q[((q > 1.0) & (q < np.asarray(ext) - 1.0)).all(1)]
    nq = len(q)
    qc = (q / H).astype(np.int64)
    cell = (qc[:, 2] * ny + qc[:, 1]) * nx + qc[:, 0]
    s0, s1, s2, s3 = start[cell - 1], start[cell], start[cell + 1], start[cell + 2]
    fr = q / H - qc
    gxm, gxp, gym, gyp, gzm, gzp = fr[:, 0] * H, (1 - fr[:, 0]) * H, fr[:, 1] * H, (1 - fr[:, 1]) * H, fr[:, 2] * H, (1 - fr[:, 2]) * H
    lo, hi = first_window(*slot_row(s0, s1, s2, s3, gxm * gxm, gxp * gxp, 0.25), gxm * gxm, gxp * gxp, variant)
    best = np.full(nq, 0.25)                                    # the acceptance radius 0.5 m, squared
    for k in range(8):
        j = lo + k
        m = j < hi
        d = ((p[np.where(m, j, 0)].astype(np.float64) - q) ** 2).sum(1)
        best = np.where(m & (d < best), d, best)
    rows, steps = [], []
    for dy in (-1, 0, 1):
        for dz in (-1, 0, 1):
            if dy or dz:
                gy = np.where(dy < 0, gym, np.where(dy > 0, gyp, 0.0))
                gz = np.where(dz < 0, gzm, np.where(dz > 0, gzp, 0.0))
                rows.append(gy * gy + gz * gz)
                steps.append(dy * nx + dz * nx * ny)
    rows = np.array(rows)
    row_task = rows * 0.998 < best
    (la, lb), (ra, rb), (oa, ob) = residuals(s0, s1, s2, s3, lo, hi)
    left = (la < lb) & (gxm * gxm * 0.998 < best)
    right = (ra < rb) & (gxp * gxp * 0.998 < best)
    rest = oa < ob
    tasks = left.astype(int) + right + rest + row_task.sum(0)
    cand = left * (lb - la) + right * (rb - ra) + rest * (ob - oa)
    for k, step in enumerate(steps):
        r0, r1, r2, r3 = (start[cell + step + d] for d in (-1, 0, 1, 2))
        a = np.where((rows[k] + gxm * gxm) * 0.998 < best, r0, r1)
        b = np.where((rows[k] + gxp * gxp) * 0.998 < best, r3, r2)
        cand = cand + np.where(row_task[k], b - a, 0)
    m = (nq // 64) * 64
    per_wave = tasks[:m].reshape(-1, 64).sum(1)
    return dict(tasks=tasks.mean(), rounds=np.ceil(per_wave / 64).mean(), bound=np.sqrt(best).mean(), own_empty=(s1 == s2).mean(),
                first=(hi - lo).mean(), row_bounds=row_task.sum(0).mean(), cand=cand.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=120_000)
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    world = make_map(rng)
    print("| query offset | first trip | tasks / query | rounds / wave | mean bound before the mask | own cell empty | lane accesses / query (first trip + row bounds + task candidates) |")
    print("|---|---|---|---|---|---|---|")
    for label, off in (("0.115 m (launch 0)", (0.10, -0.05, 0.02)), ("33 mm (launch 1, unseeded)", (0.03, -0.012, 0.005)), ("0 (steady)", (0.0, 0.0, 0.0))):
        for variant in VARIANTS:
            r = run(np.random.default_rng(2), world, off, args.queries, variant)
            print("| %s | %s | %.2f | %.2f | %.3f m | %.3f | %.2f + %.2f + %.2f = %.1f |" % (
                label, variant, r["tasks"], r["rounds"], r["bound"], r["own_empty"], r["first"], r["row_bounds"], r["cand"], r["first"] + r["row_bounds"] + r["cand"]))


if __name__ == "__main__":
    main()
