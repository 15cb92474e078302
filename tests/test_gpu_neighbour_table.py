"""The map's neighbour table (sf_map_build_neighbour_table, k_neighbour_table in sf_map.hip), the re-search from it
(sf::nn_research_table in sf_nn.hpp, alone through sf_map_nn_seeded) and the alignments that consult it (nn_pair / k_nn_red_df in
sf_icp.hip).  No reference counterpart: the reference descends a kd-tree for every point in every iteration
(localization/src/icp_point_to_point.cpp:64-69).

(a) the table equals the numpy table (tests/nbr_rule_np.py) entry for entry, ids in key order and r bit for bit; (b) a served
query of sf_map_nn_seeded equals sf_map_nn bit for bit and the degenerate inputs come back not served; (c) alignments with the
table forced on equal those with it off -- bitwise without frozen pairs (the same pairs in the same lanes), within the 1e-10
between two summation orders with them (E changes, and with it what is deferred and frozen); (d) the automatic rule."""
import numpy as np
import pytest

import nbr_rule_np as nb

pytestmark = pytest.mark.gpu

F = np.float32
N_SCAN = 140_000          # above 131 072: two queries per lane, the launch list (tests/test_gpu_deferred_search.py's world)
TOL = 1e-10


def numpy_table(mp):
    ix = mp.index()
    pts = ix["pts4"][:, :3]
    h, dims = mp.cell_size()
    cells = nb.cells_of(pts, ix["org"], ix["inv_h"], dims)
    ids, r = nb.build_table(pts, cells, F(h), F(ix["gap_eps"]))
    return pts, cells, np.array(dims), ids, r


def assert_table(mp):
    pts, cells, dims, ids, r = numpy_table(mp)
    info = mp.neighbour_table_info()
    assert info["present"] and info["entries"] == len(pts) and info["bytes"] == 32 * len(pts)
    dids, dr = mp.download_neighbour_table()
    assert np.array_equal(dids, ids)
    assert np.array_equal(dr.view(np.uint32), r.view(np.uint32))
    return pts, cells, dims, ids, r


def test_table_equals_numpy(api, ctx):
    rng = np.random.default_rng(11)
    cloud = (rng.uniform(0.0, 1.0, (5000, 3)) * [3.0, 3.0, 1.5]).astype(F)
    mp = api.Map(ctx, api.Cloud(ctx, cloud), 0.25)
    assert not mp.neighbour_table_info()["present"]
    mp.profile_launches(True)
    mp.build_neighbour_table()
    pts, cells, dims, ids, r = assert_table(mp)
    assert mp.neighbour_table_info()["build_ms"] >= 0
    border = ((cells == 0) | (cells == dims - 1)).any(1)
    assert border.any() and (ids[border] != nb.NONE).any()          # points in border cells of the grid, with neighbours
    assert (ids[:, 6] != nb.NONE).any() and (ids[:, 6] == nb.NONE).any()   # both forms of the radius
    mp.estimate_normals(0.25)                                         # a normals pass keeps the table
    assert mp.neighbour_table_info()["present"]
    mp.build(api.Cloud(ctx, cloud[:3000]), 0.25)                     # a rebuild drops it
    assert not mp.neighbour_table_info()["present"]
    mp.build_neighbour_table()
    assert_table(mp)
    few = api.Map(ctx, api.Cloud(ctx, cloud[:5]), 0.25).build_neighbour_table()
    assert_table(few)


def test_table_after_patch(api, ctx):
    rng = np.random.default_rng(12)
    prev = api.voxel_merge_min_points(0)
    try:
        dev = api.Cloud(ctx, (rng.uniform(0.0, 1.0, (6000, 3)) * [3.0, 3.0, 1.5]).astype(F))
        dev.voxel_downsample(0.1, "pcl")
        mp = api.Map(ctx).set_origin_lattice(64).build(dev, 0.25)
        mp.build_neighbour_table()
        assert_table(mp)
        add = (rng.uniform(0.2, 0.8, (1500, 3)) * [3.0, 3.0, 1.5]).astype(F)
        st, merged = dev.voxel_merge(api.Cloud(ctx, add), 0.1)
        assert st == 0 and merged
        assert mp.patch(dev)
        assert not mp.neighbour_table_info()["present"]              # the points moved: the table went with them
        mp.build_neighbour_table()
        assert_table(mp)
    finally:
        api.voxel_merge_min_points(prev)


def seeded_case(api, ctx, cloud, q_of, thr, min_served):
    mp = api.Map(ctx, api.Cloud(ctx, cloud), 0.25).build_neighbour_table()
    pts = mp.index()["pts4"][:, :3]
    q, seed = q_of(pts)
    idx, d2, served = mp.nn_seeded(q, seed, thr)
    ri, rd = mp.nn(q, thr)
    assert np.array_equal(idx[served], ri[served]) and np.array_equal(d2[served].view(np.uint32), rd[served].view(np.uint32))
    assert (idx[~served] == -1).all() and np.isinf(d2[~served]).all()
    print("served %.3f" % served.mean())
    assert served.mean() >= min_served
    return mp, pts, q, seed, served


def near(rng, pts, m, lo, hi):
    seed = rng.integers(0, len(pts), m)
    u = rng.normal(size=(m, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    return (pts[seed].astype(np.float64) + u * rng.uniform(lo, hi, (m, 1))).astype(F), seed.astype(np.int32)


def test_seeded_search_equals_full_search(api, ctx):
    rng = np.random.default_rng(13)
    cloud = rng.uniform(0.0, 2.0, (3000, 3)).astype(F)
    mp, pts, q, seed, served = seeded_case(api, ctx, cloud, lambda p: near(rng, p, 20_000, 0.005, 0.15), 0.25, 0.5)
    # the same rule on the host decides the same queries
    _, _, _, ids, r = numpy_table(mp)
    assert np.array_equal(served, nb.research(pts, ids, r, q, seed, 0.25)[0])
    # a threshold below the best distance, and one that splits the queries
    low = float(mp.nn(q)[1].min()) * 0.5
    idx, d2, s2 = mp.nn_seeded(q, seed, low)
    assert np.array_equal(s2, served) and (idx == -1).all()
    seeded_case(api, ctx, cloud, lambda p: (q, seed), float(np.median(mp.nn(q)[1])), 0.5)
    # NaN queries, queries far outside the grid, no seed, a seed beyond the index: never served
    bad = q[:4000].copy()
    bseed = seed[:4000].copy()
    bad[:1000, rng.integers(0, 3, 1000)] = np.nan
    bad[1000:1100, 0] = np.inf
    bad[1100:2000] += F(50.0)
    bseed[2000:3000] = -1
    bseed[3000:3500] = len(pts)
    bseed[3500:4000] = np.iinfo(np.int32).max
    idx, d2, sb = mp.nn_seeded(bad, bseed, 0.25)
    assert not sb.any() and (idx == -1).all() and np.isinf(d2).all()


def test_seeded_search_lattice_and_duplicates(api, ctx):
    rng = np.random.default_rng(14)
    g = np.arange(0, 21, dtype=np.float64) * 0.1
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F)

    def lattice_queries(p):
        q, seed = near(rng, p, 6_000, 0.0005, 0.08)
        s2 = rng.integers(0, len(p), 3_000).astype(np.int32)
        step = np.array([[0.1, 0, 0], [0, 0.1, 0], [0.1, 0.1, 0], [0, 0.1, 0.1]])[rng.integers(0, 4, 3_000)]
        mid = ((p[s2].astype(np.float64) + (p[s2].astype(np.float64) + step).astype(F).astype(np.float64)) / 2).astype(F)
        return np.concatenate([q, mid, p[s2]]), np.concatenate([seed, s2, s2])
    seeded_case(api, ctx, lattice, lattice_queries, 0.25, 0.3)
    twins = np.concatenate([np.repeat(np.array([[1.0, 1.0, 1.0]], F), 9, axis=0), rng.uniform(0.0, 2.0, (200, 3)).astype(F)])
    mp = api.Map(ctx, api.Cloud(ctx, twins), 0.25).build_neighbour_table()
    pts = mp.index()["pts4"][:, :3]
    pos = np.nonzero((pts == F(1.0)).all(1))[0].astype(np.int32)
    assert len(pos) == 9
    seed = pos[rng.integers(0, 9, 500)]
    q = (pts[seed] + rng.normal(0, 0.01, (500, 3))).astype(F)
    q[:20] = pts[seed[:20]]
    assert not mp.nn_seeded(q, seed, 0.25)[2].any()                   # radius 0: nothing is served


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
    return dict(map=ds, scans=scans, inits=inits, new_map=new_map, never=new_map("never"), always=new_map("always"))


def make_icp(api, ctx, mp, world, freeze=False, graph=False, reuse=True, profile=False, scans=None, inits=None, max_corr=0.5):
    icp = api.Icp(ctx, max_corr, 20, 0.05, 1e-5)
    icp.set_target(mp)
    icp.use_graph(graph)
    icp.set_query_order("cell")
    icp.set_freeze(freeze)
    icp.set_nn_reuse(reuse)
    if profile:
        icp.profile_enable(True)
    icp.set_source_batch(world["scans"] if scans is None else scans)
    icp.set_initial_batch(world["inits"] if inits is None else inits)
    return icp


def run(api, ctx, mp, world, mode, **kw):
    icp = make_icp(api, ctx, mp, world, **kw)
    res = icp.align_batch(mode)
    stats = icp.neighbour_stats() if kw.get("profile") else None
    icp.close()
    return res, stats


def bitwise(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x["T64"], y["T64"], equal_nan=True) and x["n_corr"] == y["n_corr"] and x["iterations"] == y["iterations"]
        assert x["rmse"] == y["rmse"] or (np.isnan(x["rmse"]) and np.isnan(y["rmse"]))


@pytest.mark.parametrize("mode", ["p2plane", "o3d_p2p"])
def test_alignment_with_the_table_equals_without(api, ctx, world, mode):
    off, s0 = run(api, ctx, world["never"], world, mode, profile=True)
    on, s1 = run(api, ctx, world["always"], world, mode, profile=True)
    print("table", s1)
    bitwise(on, off)
    assert s0["served"] == 0 and s0["not_served"] == 0 and s1["served"] > 0
    assert world["always"].neighbour_table_info()["present"] and not world["never"].neighbour_table_info()["present"]
    plain, _ = run(api, ctx, world["always"], world, mode)                        # unprofiled, and as a replayed graph
    bitwise(on, plain)
    bitwise(on, run(api, ctx, world["always"], world, mode, graph=True)[0])
    bitwise(on, run(api, ctx, world["always"], world, mode, reuse=False)[0])       # reuse off == reuse on, as always


@pytest.mark.parametrize("mode", ["p2plane", "o3d_p2p"])
@pytest.mark.parametrize("max_corr", [0.03, 0.05])
def test_acceptance_radius_below_half_the_point_spacing(api, ctx, world, synth, mode, max_corr):
    """max_corr far below the 0.1 m voxel spacing: a served query often has NO neighbour within max_corr, and its cache entry
    then says "nothing" with a bound that a later launch trusts for every map point (reuse_certificate) -- the bound must
    cover the nearest point too, or a pair that comes within reach as the pose moves is dropped.  Priors a few centimetres
    off, so that pairs appear and disappear from launch to launch; bitwise against the table off and against reuse off."""
    inits = np.stack([synth.make_T((0.02, -0.015, 0.01), (0.1, -0.05, 0.15)), synth.make_T((0.03, 0.02, -0.02), (0.0, 0.2, -0.2)),
                      synth.make_T((-0.025, 0.025, 0.0), (0.15, 0.1, 0.0))])
    off, _ = run(api, ctx, world["never"], world, mode, inits=inits, max_corr=max_corr)
    on, st = run(api, ctx, world["always"], world, mode, inits=inits, max_corr=max_corr, profile=True)
    print("table", st, "n_corr", [r["n_corr"] for r in on], "iterations", [r["iterations"] for r in on])
    bitwise(on, off)
    assert st["served"] > 0 and min(r["n_corr"] for r in on) > 1000
    bitwise(on, run(api, ctx, world["always"], world, mode, inits=inits, max_corr=max_corr, reuse=False)[0])


def test_frozen_pairs_with_the_table_equal_without(api, ctx, world):
    off, _ = run(api, ctx, world["never"], world, "p2plane", freeze=True)
    on, _ = run(api, ctx, world["always"], world, "p2plane", freeze=True)
    for x, y in zip(on, off):
        assert x["iterations"] == y["iterations"] and x["n_corr"] == y["n_corr"] and x["flags"] == y["flags"]
        d = np.abs(x["T64"] - y["T64"]).max()
        print("max |dT64| %.3e" % d)
        assert not d >= TOL, d
    bitwise(on, run(api, ctx, world["always"], world, "p2plane", freeze=True, graph=True)[0])


def test_graph_replay_across_the_tables_appearance(api, ctx, world):
    """one object with a captured graph: no table (auto, a small batch), the table built by hand, the map rebuilt -- each
    alignment equals a fresh object's"""
    mp = world["new_map"]("auto")
    icp = make_icp(api, ctx, mp, world, graph=True)
    for step in range(3):
        if step == 1:
            mp.build_neighbour_table()
        if step == 2:
            mp.build(api.Cloud(ctx, world["map"][: len(world["map"]) * 9 // 10]), 0.25)
            mp.estimate_normals(0.25)
            icp.set_target(mp)
        assert mp.neighbour_table_info()["present"] == (step == 1)
        got = icp.align_batch("p2plane")
        assert mp.neighbour_table_info()["present"] == (step == 1)               # (d): the small batch builds none under auto
        bitwise(got, run(api, ctx, mp, world, "p2plane")[0])
    caps, _ = icp.graph_counts()
    assert caps == 3
    icp.close()


def test_two_lanes_equal_one_lane(api, ctx, world):
    out = []
    for pipeline in (False, True):
        icp = make_icp(api, ctx, world["always"], world, graph=True)
        icp.set_pipeline(pipeline)
        icp.align_batch_async("p2plane")
        if pipeline:
            icp.align_batch_async("p2plane")
            out.append((icp.fetch_previous(), icp.fetch_results()))
        else:
            first = icp.fetch_results()
            icp.align_batch_async("p2plane")
            out.append((first, icp.fetch_results()))
        icp.close()
    bitwise(out[0][0], out[0][1])
    bitwise(out[0][0], out[1][0])
    bitwise(out[0][1], out[1][1])


def test_auto_rule(api, ctx, world, synth):
    """auto: a batch of the automatic frozen-pairs size (0.7 M queries) builds the table of a map that has only been built; a
    map patched after it served an alignment gets none"""
    scans = np.stack([synth.make_scan(world["map"], N_SCAN, scan_id=60 + k)[0] for k in range(5)])      # 700 000 queries
    inits = np.stack([np.eye(4)] * 5)
    fresh = world["new_map"]("auto")
    run(api, ctx, fresh, world, "p2plane")                                        # small batch: none
    assert not fresh.neighbour_table_info()["present"]
    run(api, ctx, fresh, world, "p2plane", scans=scans, inits=inits)
    assert fresh.neighbour_table_info()["present"]
    prev = api.voxel_merge_min_points(0)
    try:
        dev = api.Cloud(ctx, world["map"])
        dev.voxel_downsample(0.1, "pcl")
        mp = api.Map(ctx).set_origin_lattice(64).build(dev, 0.25)
        mp.estimate_normals(0.25)
        run(api, ctx, mp, world, "p2plane")                                       # serves an alignment
        rng = np.random.default_rng(15)
        add = (world["map"][rng.choice(len(world["map"]), 2000, replace=False)] + rng.normal(0, 0.004, (2000, 3))).astype(F)
        st, merged = dev.voxel_merge(api.Cloud(ctx, add), 0.1)
        assert st == 0 and merged and mp.patch(dev)
        mp.estimate_normals(0.25)
        run(api, ctx, mp, world, "p2plane", scans=scans, inits=inits)
        assert not mp.neighbour_table_info()["present"]
        mp.build_neighbour_table()                                                # its owner may still build one: it is consulted
        res, st = run(api, ctx, mp, world, "p2plane", scans=scans, inits=inits, profile=True)
        assert st["served"] > 0
    finally:
        api.voxel_merge_min_points(prev)
