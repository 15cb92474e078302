"""The first trip of the wave search (sf_nn.hpp: first_window, nn_search_wave, round_task): its four slots go to a window of
consecutive CSR positions of the query's own ROW -- the own cell first, what it leaves idle from the x neighbour whose face is
nearer, then from the other -- and tasks 0, 1 and 10 cover only what the window left.  The clouds here are built cell by cell
on a 0.25 m index with its origin at 0, so that every way the window can lie is met: own cells of 0, 1, 3, 4 and 5 points next
to x neighbours of 0, 1, 3 and 6, own cells in the first and last x cell of a row (where the table's neighbour entry belongs to
another row), empty own rows between filled ones, duplicates and mirrored points whose ties cross the window's edges, queries on
the x faces and a few float32 steps either side.  The result must be the exact 1-NN, the lexicographic minimum of (d2, position)
of a float32 brute force, to the bit; the runner-up bound that now takes candidate distances where it took gaps is checked
through the one thing that reads it, the neighbour-reuse certificate."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H = np.float32(0.25)
NX = 9
OWN, SIDE = (0, 1, 3, 4, 5), (0, 1, 3, 6)
COMBOS = [(o, l, r) for o in OWN for l in SIDE for r in SIDE]          # 80 rows, the triple in x cells 3, 4, 5


def cell_points(rng, cx, cy, cz, n):
    """n points inside cell (cx, cy, cz), 1 cm off its faces; 5 points: the fifth repeats the first, 6: three points twice (index
    ties that cross the end of a four-slot window, wherever it starts)"""
    distinct = {5: 4, 6: 3}.get(n, n)
    p = (np.array([cx, cy, cz], np.float32) * H + rng.uniform(0.01, 0.24, (distinct, 3)).astype(np.float32)).astype(np.float32)
    return np.concatenate([p, p[:n - distinct]]) if n > distinct else p


def row_cloud(seed):
    rng = np.random.default_rng(seed)
    out = [np.zeros((1, 3), np.float32)]                                # the grid origin at 0: cell faces at k * H
    for i, (o, l, r) in enumerate(COMBOS):
        cy, cz = 2 * (i % 10), i // 10
        left, own, right = (cell_points(rng, cx, cy, cz, n) for cx, n in ((3, l), (4, o), (5, r)))
        if o and l and i % 2:     # the last point of the left cell mirrored across the face into the own cell: equal d2 from the face
            own[0] = left[-1]
            left[-1, 0], own[0, 0] = np.float32(1.0 - 0.03125), np.float32(1.0 + 0.03125)
            if o == 5:
                own[4] = own[0]
        out += [left, own, right]
        # the ends of the row: first and last x cell and their inner neighbours
        out += [cell_points(rng, cx, cy, cz, n) for cx, n in ((0, i % 4), (1, (i // 4) % 3), (8, (i + 1) % 4), (7, (i // 4 + 1) % 3))]
        # the row between this one and the next holds points in its end cells only: what lies before / behind a row's first / last
        # cell in memory, and rows whose own x triple is empty between rows that are filled
        out += [cell_points(rng, cx, cy + 1, cz, 2) for cx in (0, 8)]
    return np.concatenate(out).astype(np.float32)


def row_queries(pts, seed):
    rng = np.random.default_rng(seed)
    q = [pts, pts + rng.normal(0.0, 0.01, pts.shape).astype(np.float32)]
    steps = np.float32([0.0, 0.25, 0.75, 1.0, 1.25, 2.0, 2.25])          # x faces: the ends of the row, the triple's, the last cell's
    for i in range(len(COMBOS)):
        cy, cz = 2 * (i % 10), i // 10
        for row in (cy, cy + 1):
            inside = (np.array([0, row, cz], np.float32) * H + rng.uniform(0.0, 1.0, (36, 3)).astype(np.float32) * np.float32([NX, 1, 1]) * H)
            q.append(inside.astype(np.float32))
            yz = (np.array([row, cz], np.float32) * H + rng.uniform(0.0, 0.25, (len(steps), 2)).astype(np.float32)).astype(np.float32)
            for k in (-3, -1, 0, 1, 3):                                 # on the face and float32 steps either side
                x = steps.copy()
                for _ in range(abs(k)):
                    x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf)).astype(np.float32)
                q.append(np.column_stack([x, yz]).astype(np.float32))
    # on the face between a mirrored pair, level with it and a little off
    m = pts[(pts[:, 0] == np.float32(1.0 + 0.03125))]
    for dy in (0.0, 0.004):
        f = m.copy()
        f[:, 0] = 1.0
        f[:, 1] += np.float32(dy)
        q.append(f)
    return np.concatenate(q).astype(np.float32)                        # (a few lie just outside the grid: binned into its end cells)


def brute(q, P, ok_pt, max_d2):
    """-> (position of the lexicographic minimum of (d2 bits, position) in the index, its d2, hit); l2_simple in float32, unfused."""
    pos = np.full(len(q), -1, np.int64)
    d2 = np.full(len(q), np.inf, np.float32)
    idx = np.arange(len(P), dtype=np.uint64)
    for s in range(0, len(q), 256):
        c = q[s:s + 256]
        dx, dy, dz = (c[:, None, k] - P[None, :, k] for k in range(3))
        d = ((dx * dx) + dy * dy) + dz * dz
        assert d.dtype == np.float32
        ok = (d < np.float32(max_d2)) & ok_pt[None, :]
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx[None, :]
        key[~ok] = np.uint64(0xFFFFFFFFFFFFFFFF)
        best = key.argmin(1)
        took = ok[np.arange(len(c)), best]
        pos[s:s + 256] = np.where(took, best, -1)
        d2[s:s + 256] = np.where(took, d[np.arange(len(c)), best], np.inf)
    return pos, d2, pos >= 0


@pytest.fixture(scope="module")
def rows(api, ctx):
    pts = row_cloud(7)
    q = row_queries(pts, 8)
    mp = api.Map(ctx, api.Cloud(ctx, pts), float(H))
    index = mp.index()
    P = np.ascontiguousarray(index["pts4"][:, :3])
    ids = index["pts4"][:, 3].view(np.uint32).astype(np.int64)
    ref = {m: brute(q, P, np.ones(len(P), bool), m) for m in (np.inf, 0.04)}     # computed once, shared, left unchanged
    return dict(pts=pts, q=q, mp=mp, index=index, P=P, ids=ids, ref=ref)


def check_nn(rows, ref, max_d2, what):
    idx, d2 = rows["mp"].nn(rows["q"], max_d2)
    pos, rd2, hit = ref
    assert np.array_equal(idx >= 0, hit), (what, np.flatnonzero((idx >= 0) != hit)[:5])
    assert np.array_equal(d2[hit], rd2[hit]), (what, np.flatnonzero(d2 != rd2)[:5])
    assert np.all(np.isinf(d2[~hit])), what
    # the index names a point at exactly that distance ...
    d = rows["q"][hit] - rows["pts"][idx[hit]]
    own = ((d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert np.array_equal(own, rd2[hit]), what
    # ... and among equals the one that lies first in the index
    assert np.array_equal(idx[hit], rows["ids"][pos[hit]]), (what, np.flatnonzero(idx[hit] != rows["ids"][pos[hit]])[:5])


def test_the_cloud_holds_every_case_the_window_rule_has(api, rows):
    """The cases are a property of the index as the library built it, not of how the cloud was meant."""
    index, q = rows["index"], rows["q"]
    cell, dims = rows["mp"].cell_size()
    assert cell == 0.25 and dims[0] == NX and np.all(index["org"] == 0.0)
    cs = index["cell_start"].astype(np.int64)
    c = np.clip(np.floor(q * np.float32(4.0)).astype(np.int64), 0, np.array(dims) - 1)
    lin = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    own = cs[lin + 1] - cs[lin]
    inner = (c[:, 0] > 0) & (c[:, 0] < NX - 1)
    left = np.where(inner, cs[lin] - cs[np.maximum(lin - 1, 0)], -1)
    right = np.where(inner, cs[np.minimum(lin + 2, len(cs) - 1)] - cs[lin + 1], -1)
    seen = set(zip(own[inner].tolist(), left[inner].tolist(), right[inner].tolist()))
    assert all(combo in seen for combo in COMBOS), [combo for combo in COMBOS if combo not in seen]
    assert (0, 0, 0) in seen                                              # nothing in the own row: only y / z rows hold points
    # first and last x cell of a row with points before / behind them in memory (another row's), own cell empty and not
    first, last = c[:, 0] == 0, c[:, 0] == NX - 1
    before = cs[lin] - cs[np.maximum(lin - 1, 0)]
    behind = cs[np.minimum(lin + 2, len(cs) - 1)] - cs[lin + 1]
    for edge, other in ((first & (lin > 0), before), (last & (lin + 2 < len(cs)), behind)):
        assert (edge & (other > 0) & (own == 0)).any() and (edge & (other > 0) & (own > 0) & (own < 4)).any()
    # queries on an x face (binned right of it) and one float32 step below it (binned left)
    x4 = q[:, 0] * np.float32(4.0)
    assert (x4 == np.float32(4.0)).sum() >= 80 and (np.nextafter(q[:, 0], np.float32(np.inf)) == np.float32(1.0)).sum() >= 80
    # ties: duplicates inside cells of 5 and 6 points, and pairs mirrored across the face x = 1
    P = rows["P"]
    assert len(np.unique(P, axis=0)) < len(P) - 100 and (P[:, 0] == np.float32(1.0 - 0.03125)).sum() >= 10


@pytest.mark.parametrize("max_d2", [np.inf, 0.04])
def test_exact_neighbour_whatever_the_window_takes(rows, max_d2):
    check_nn(rows, rows["ref"][max_d2], max_d2, max_d2)


@pytest.mark.parametrize("window", ["sphere", "obb"])
def test_window_forms_match_a_brute_force_over_what_the_window_accepts(rows, window):
    mp, P = rows["mp"], rows["P"]
    centre = np.array([1.1, 2.4, 0.9], np.float32)
    try:
        if window == "sphere":
            mp.window_sphere(centre, 1.3)
            d = centre[None, :] - P
            ok = ((d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] < np.float32(1.3 * 1.3)
        else:
            R = np.array([[0.9, -0.3, 0.05], [0.35, 0.95, 0.0], [0.0, 0.1, 1.1]])           # not orthonormal
            ext = np.array([1.6, 3.0, 1.4])
            mp.window_obb(centre.astype(np.float64), R, ext)
            d = P.astype(np.float64) - centre.astype(np.float64)[None, :]
            ok = np.ones(len(P), bool)
            for k in range(3):
                ok &= np.abs((d[:, 0] * R[0, k] + d[:, 1] * R[1, k]) + d[:, 2] * R[2, k]) <= ext[k] / 2
        assert 100 < ok.sum() < len(P) - 100                               # the window cuts through the cloud
        for max_d2 in (np.inf, 0.04):
            check_nn(rows, brute(rows["q"], P, ok, max_d2), max_d2, (window, max_d2))
    finally:
        mp.window_none()


def cells_cloud(seed, counts, probs, dims=(32, 32, 8)):
    """counts[k] points with probability probs[k] in every cell of a dims grid of 0.25 m cells"""
    rng = np.random.default_rng(seed)
    n = rng.choice(counts, size=dims, p=probs)
    cell = np.argwhere(n > 0)
    cell = np.repeat(cell, n[n > 0], axis=0).astype(np.float32)
    pts = (cell * H + rng.uniform(0.005, 0.245, cell.shape).astype(np.float32)).astype(np.float32)
    pts = np.concatenate([pts, pts[rng.integers(0, len(pts), len(pts) // 20)]])          # exact duplicates
    pts[0] = 0.0
    return pts


@pytest.mark.parametrize("mode", ["p2plane", "o3d_p2p"])
@pytest.mark.parametrize("density", ["rows", "sparse"])
def test_reuse_certificate_holds_with_the_bound_the_window_leaves(api, ctx, synth, mode, density):
    """Alignments that reuse neighbours form bit for bit the pairs of alignments that search every query: a runner-up bound
    that came out too large anywhere would keep a stale neighbour.  `rows`: cells of 0, 1, 3, 4, 5 and 6 points, as above;
    `sparse`: about 1.5 points per cell, where most first trips reach into the neighbours."""
    if density == "rows":
        pts = cells_cloud(21, [0, 1, 3, 4, 5, 6], [0.2, 0.2, 0.2, 0.15, 0.15, 0.1])
    else:
        pts = cells_cloud(22, [0, 1, 2, 3, 4], [0.22, 0.33, 0.25, 0.13, 0.07])             # mean 1.5
    mp = api.Map(ctx, api.Cloud(ctx, pts), float(H))
    mp.estimate_normals(0.25)
    rng = np.random.default_rng(23)
    scans = np.stack([pts[rng.choice(len(pts), 9_000, replace=False)] + rng.normal(0.0, 0.01, size=(9_000, 3)).astype(np.float32)
                      for _ in range(3)]).astype(np.float32)
    inits = np.stack([synth.make_T((0.03 * k, -0.02, 0.01), (0.0, 0.01, 0.2 * k)) for k in range(3)])
    keys = ("iterations", "converged", "n_corr", "flags", "rmse", "fitness")
    out = []
    for reuse in (False, True):
        icp = api.Icp(ctx, 0.5, 15, 0.05, 1e-5)
        icp.use_graph(False)
        icp.set_nn_reuse(reuse)
        icp.set_target(mp)
        icp.set_source_batch(scans)
        icp.set_initial_batch(inits)
        out.append(icp.align_batch(mode))
        icp.close()
    for a, b in zip(*out):
        assert np.array_equal(a["T64"], b["T64"]) and all(a[k] == b[k] for k in keys), (mode, density)
        assert np.isfinite(a["T64"]).all() and a["n_corr"] > 8_000
    mp.close()


def test_a_wide_frozen_run_equals_the_run_without_freezing(api, ctx, synth, small_world):
    """Frozen pairs rest on the same bound: scans of 10 000 points put on the wide launch list (two queries per lane) freeze, and
    must give the pairs of the launch-by-launch run and, to float64 summation order, its poses (the rule and the 1e-10 of
    tests/test_gpu_freeze.py between frozen and unfrozen runs)."""
    ds = small_world["map"]
    mp = api.Map(ctx, api.Cloud(ctx, ds), 0.25)
    mp.estimate_normals(0.25)
    scans = [synth.make_scan(ds, 10_000, scan_id=60 + k)[0] for k in range(3)]
    n = min(len(s) for s in scans)
    scans = np.stack([s[:n] for s in scans])
    inits = np.stack([np.eye(4), synth.make_T((0.04, -0.03, 0.02), (0.2, -0.1, 0.3)), synth.make_T((-0.05, 0.05, 0.0), (0.0, 0.3, -0.4))])
    res = []
    for freeze in (False, True):
        icp = api.Icp(ctx, 0.5, 20, 0.05, 1e-5)
        icp.set_target(mp)
        icp.use_graph(False)
        icp.set_query_order("cell")
        icp.set_wide_scan_points(1024)
        icp.set_freeze(freeze)
        icp.set_source_batch(scans)
        icp.set_initial_batch(inits)
        res.append((icp.align_batch("p2plane"), icp.freeze_stats()))
        icp.close()
    (off, s_off), (on, s_on) = res
    assert s_off["froze"] == 0 and s_on["froze"] >= 3 and s_on["failed"] == 0, (s_off, s_on)
    for x, y in zip(on, off):
        assert x["iterations"] == y["iterations"] and x["n_corr"] == y["n_corr"] and x["flags"] == y["flags"] and x["converged"] == y["converged"]
        assert np.abs(x["T64"] - y["T64"]).max() < 1e-10, np.abs(x["T64"] - y["T64"]).max()
        assert abs(x["rmse"] - y["rmse"]) < 1e-11 and x["fitness"] == y["fitness"]
    mp.close()
