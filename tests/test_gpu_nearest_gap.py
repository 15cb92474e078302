"""Stage 0 of the neighbour-table look-up on the device: the nearest-gap array that k_neighbour_table (sf_map.hip) writes behind
the table, the head of sf::nn_research_table (sf_nn.hpp) through sf_map_nn_seeded_stages, and the alignments that run through it
(nn_pair / k_nn_red_df in sf_icp.hip).  No reference counterpart: the reference descends a kd-tree for every point in every
iteration (localization/src/icp_point_to_point.cpp:64-69).

(a) the gap array equals the numpy value (tests/nbr_gap_np.py) bit for bit; (b) stage, index, d2 and the runner-up bound lb2 of
the seeded look-up equal the numpy model bit for bit, degenerate inputs included; (c) alignments through stage 0 equal those
with the table off, with reuse off and as a replayed graph bitwise, those with frozen pairs within the 1e-10 between two
summation orders, and the gap counter is positive and not above the served count."""
import numpy as np
import pytest

import nbr_gap_np as ng
import nbr_rule_np as nb

pytestmark = pytest.mark.gpu

F = np.float32
N_SCAN = 140_000          # above 131 072: two queries per lane, the launch list
N_SMALL = 60_000          # one query per lane
TOL = 1e-10


def numpy_model(mp):
    ix = mp.index()
    pts = ix["pts4"][:, :3]
    h, dims = mp.cell_size()
    cells = nb.cells_of(pts, ix["org"], ix["inv_h"], dims)
    ids, r = nb.build_table(pts, cells, F(h), F(ix["gap_eps"]))
    cap = nb.cap_of(F(h), F(ix["gap_eps"]))
    return pts, ix["pts4"][:, 3].copy().view(np.int32), ids, r, ng.nearest_gap(pts, ids, cap), cap


def assert_gap(mp):
    pts, _, ids, r, g1, cap = numpy_model(mp)
    got = mp.download_nearest_gap()
    assert got.shape == g1.shape and np.array_equal(got.view(np.uint32), g1.view(np.uint32))
    assert mp.neighbour_table_info()["bytes"] == 32 * len(pts)               # the entries are what they were
    return ids, g1, cap


def test_gap_array_equals_numpy(api, ctx):
    rng = np.random.default_rng(11)
    cloud = (rng.uniform(0.0, 1.0, (5000, 3)) * [3.0, 3.0, 1.5]).astype(F)
    mp = api.Map(ctx, api.Cloud(ctx, cloud), 0.25).build_neighbour_table()
    ids, g1, cap = assert_gap(mp)
    assert (ids[:, 0] != nb.NONE).all() and (g1 < cap).all()                  # a dense cloud: every gap is a listed point's distance
    mp.build(api.Cloud(ctx, cloud[:3000]), 0.25)                             # a rebuild drops the array with the table
    with pytest.raises(Exception):
        mp.download_nearest_gap()
    mp.build_neighbour_table()
    assert_gap(mp)
    ids, g1, cap = assert_gap(api.Map(ctx, api.Cloud(ctx, cloud[:5]), 0.25).build_neighbour_table())
    assert (g1[ids[:, 0] == nb.NONE] == cap).all()
    _, one, cap = assert_gap(api.Map(ctx, api.Cloud(ctx, cloud[:1]), 0.25).build_neighbour_table())
    assert len(one) == 1 and one[0] == cap
    twins = np.concatenate([np.repeat(np.array([[1.0, 1.0, 1.0]], F), 9, axis=0), rng.uniform(0.0, 2.0, (200, 3)).astype(F)])
    mp = api.Map(ctx, api.Cloud(ctx, twins), 0.25).build_neighbour_table()
    _, g1, _ = assert_gap(mp)
    assert (g1[(mp.index()["pts4"][:, :3] == F(1.0)).all(1)] == 0).all()


def near(rng, pts, m, lo, hi):
    seed = rng.integers(0, len(pts), m)
    u = rng.normal(size=(m, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    return (pts[seed].astype(np.float64) + u * rng.uniform(lo, hi, (m, 1))).astype(F), seed.astype(np.int32)


def assert_stages(mp, model, q, seed, thr):
    pts, orig, ids, r, g1, _ = model
    idx, d2, stage, lb2 = mp.nn_seeded_stages(q, seed, thr)
    ms, mw, md, ml = ng.research_stages(pts, ids, r, g1, q, seed, thr)
    assert np.array_equal(stage, ms)
    has = (ms > 0) & (mw >= 0)
    assert np.array_equal(idx, np.where(has, orig[np.maximum(mw, 0)], -1))
    assert np.array_equal(d2[has].view(np.uint32), md[has].view(np.uint32)) and np.isinf(d2[~has]).all()
    assert np.array_equal(lb2.view(np.uint32), np.where(ms > 0, ml, F(0)).astype(F).view(np.uint32))
    # the older entry reports the same queries served, with the same answers
    i0, d0, s0 = mp.nn_seeded(q, seed, thr)
    assert np.array_equal(s0, stage > 0) and np.array_equal(i0, idx) and np.array_equal(d0.view(np.uint32), d2.view(np.uint32))
    return stage, mw


def test_seeded_stages_equal_numpy(api, ctx):
    rng = np.random.default_rng(13)
    cloud = rng.uniform(0.0, 2.0, (3000, 3)).astype(F)
    mp = api.Map(ctx, api.Cloud(ctx, cloud), 0.25).build_neighbour_table()
    model = numpy_model(mp)
    pts = model[0]
    q, seed = near(rng, pts, 20_000, 0.005, 0.15)
    stage, _ = assert_stages(mp, model, q, seed, 0.25)
    print("by the gap %.3f, by the table %.3f" % ((stage == ng.BY_GAP).mean(), (stage == ng.BY_TABLE).mean()))
    assert (stage == ng.BY_GAP).mean() > 0.1 and (stage == ng.BY_TABLE).mean() > 0.1 and (stage == 0).any()
    # a threshold below every seed distance (the "nothing" form, the bound covering p), and one that splits the queries
    dp2 = nb.l2_simple(q, pts[seed])
    stage, win = assert_stages(mp, model, q, seed, float(dp2.min()) * 0.5)
    assert (stage == ng.BY_GAP).any() and (win[stage == ng.BY_GAP] == -1).all()
    stage, win = assert_stages(mp, model, q, seed, float(np.median(dp2)))
    gap = stage == ng.BY_GAP
    assert (win[gap] == -1).any() and (win[gap] >= 0).any()
    # NaN and inf queries, queries far outside the grid, no seed, a seed beyond the index: never served
    bad = q[:4000].copy()
    bseed = seed[:4000].copy()
    bad[:1000, rng.integers(0, 3, 1000)] = np.nan
    bad[1000:1100, 0] = np.inf
    bad[1100:2000] += F(50.0)
    bseed[2000:3000] = -1
    bseed[3000:3500] = len(pts)
    bseed[3500:4000] = np.iinfo(np.int32).max
    idx, d2, stage, lb2 = mp.nn_seeded_stages(bad, bseed, 0.25)
    assert not stage.any() and (idx == -1).all() and np.isinf(d2).all() and not lb2.any()


def test_seeded_stages_lattice_midpoints_and_duplicates(api, ctx):
    rng = np.random.default_rng(14)
    g = np.arange(0, 21, dtype=np.float64) * 0.1
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F)
    mp = api.Map(ctx, api.Cloud(ctx, lattice), 0.25).build_neighbour_table()
    model = numpy_model(mp)
    p = model[0]
    q, seed = near(rng, p, 6_000, 0.0005, 0.08)
    s2 = rng.integers(0, len(p), 3_000).astype(np.int32)
    step = np.array([[0.1, 0, 0], [0, 0.1, 0], [0.1, 0.1, 0], [0, 0.1, 0.1]])[rng.integers(0, 4, 3_000)]
    mid = ((p[s2].astype(np.float64) + (p[s2].astype(np.float64) + step).astype(F).astype(np.float64)) / 2).astype(F)
    stage, _ = assert_stages(mp, model, np.concatenate([q, mid, p[s2]]), np.concatenate([seed, s2, s2]), 0.25)
    assert (stage[:len(q)] == ng.BY_GAP).any()
    assert not (stage[len(q):len(q) + len(mid)] == ng.BY_GAP).any()          # 2 dp == g1 (and beyond) does not pass
    assert (stage[len(q) + len(mid):] == ng.BY_GAP).all()                    # the lattice points themselves: dp = 0
    twins = np.concatenate([np.repeat(np.array([[1.0, 1.0, 1.0]], F), 9, axis=0), rng.uniform(0.0, 2.0, (200, 3)).astype(F)])
    mp = api.Map(ctx, api.Cloud(ctx, twins), 0.25).build_neighbour_table()
    model = numpy_model(mp)
    pos = np.nonzero((model[0] == F(1.0)).all(1))[0].astype(np.int32)
    assert len(pos) == 9
    seed = pos[rng.integers(0, 9, 500)]
    q = (model[0][seed] + rng.normal(0, 0.01, (500, 3))).astype(F)
    q[:20] = model[0][seed[:20]]
    stage, _ = assert_stages(mp, model, q, seed, 0.25)
    assert not stage.any()                                                   # gap 0, radius 0: nothing is served


# ------------------------------------------------------------------ alignments
@pytest.fixture(scope="module")
def world(api, ctx, orc, synth):
    raw = synth.make_map(400_000)
    ds = orc.voxel_pcl(raw, 0.1)[0]
    scans = np.stack([synth.make_scan(ds, N_SCAN, scan_id=40 + k)[0] for k in range(3)])
    inits = np.stack([np.eye(4), synth.make_T((0.04, -0.03, 0.02), (0.2, -0.1, 0.3)), synth.make_T((-0.05, 0.05, 0.0), (0.0, 0.3, -0.4))])

    def new_map(mode):
        mp = api.Map(ctx, api.Cloud(ctx, ds), 0.25)
        mp.estimate_normals(0.25)
        mp.set_neighbour_table(mode)
        return mp
    return dict(scans=scans, inits=inits, never=new_map("never"), always=new_map("always"))


def run(api, ctx, mp, world, mode, freeze=False, graph=False, reuse=True, profile=False, scans=None):
    icp = api.Icp(ctx, 0.5, 20, 0.05, 1e-5)
    icp.set_target(mp)
    icp.use_graph(graph)
    icp.set_query_order("cell")
    icp.set_freeze(freeze)
    icp.set_nn_reuse(reuse)
    if profile:
        icp.profile_enable(True)
    icp.set_source_batch(world["scans"] if scans is None else scans)
    icp.set_initial_batch(world["inits"])
    res = icp.align_batch(mode)
    stats = icp.neighbour_gap_stats() if profile else None
    icp.close()
    return res, stats


def bitwise(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x["T64"], y["T64"], equal_nan=True) and x["n_corr"] == y["n_corr"] and x["iterations"] == y["iterations"]
        assert x["rmse"] == y["rmse"] or (np.isnan(x["rmse"]) and np.isnan(y["rmse"]))


@pytest.mark.parametrize("mode", ["p2plane", "o3d_p2p"])
def test_alignment_through_the_gap_equals_without(api, ctx, world, mode):
    off, s0 = run(api, ctx, world["never"], world, mode, profile=True)
    on, s1 = run(api, ctx, world["always"], world, mode, profile=True)
    print("table", s1)
    bitwise(on, off)
    assert s0["served"] == 0 and s0["by_gap"] == 0
    assert 0 < s1["by_gap"] <= s1["served"]
    bitwise(on, run(api, ctx, world["always"], world, mode)[0])                   # unprofiled
    bitwise(on, run(api, ctx, world["always"], world, mode, graph=True)[0])       # as a replayed graph
    bitwise(on, run(api, ctx, world["always"], world, mode, reuse=False)[0])      # reuse off


@pytest.mark.parametrize("mode", ["p2plane", "o3d_p2p"])
def test_one_query_per_lane_through_the_gap(api, ctx, world, mode):
    scans = np.ascontiguousarray(world["scans"][:, :N_SMALL])
    off, _ = run(api, ctx, world["never"], world, mode, scans=scans)
    on, st = run(api, ctx, world["always"], world, mode, scans=scans, profile=True)
    print("table", st)
    bitwise(on, off)
    assert 0 < st["by_gap"] <= st["served"]


def test_frozen_pairs_through_the_gap(api, ctx, world):
    off, _ = run(api, ctx, world["never"], world, "p2plane", freeze=True)
    on, _ = run(api, ctx, world["always"], world, "p2plane", freeze=True)
    for x, y in zip(on, off):
        assert x["iterations"] == y["iterations"] and x["n_corr"] == y["n_corr"] and x["flags"] == y["flags"]
        d = np.abs(x["T64"] - y["T64"]).max()
        print("max |dT64| %.3e" % d)
        assert not d >= TOL, d
    bitwise(on, run(api, ctx, world["always"], world, "p2plane", freeze=True, graph=True)[0])
    _, st = run(api, ctx, world["always"], world, "p2plane", freeze=True, profile=True)
    print("table", st)
    assert 0 < st["by_gap"] <= st["served"]
