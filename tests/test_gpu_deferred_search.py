"""Deferred search (sf_icp_set_defer_search, k_nn_red_df / k_nn_deferred in sf_icp.hip): in the frozen-pairs schedule the launch
before the first chance to freeze does not search its stragglers in place -- a wave with up to 8 failing queries lists
them, a dense pass behind the launch searches them 64 per wave, and their records are added after the rows' own.  No reference counterpart (the reference searches every point in every iteration,
localization/src/icp_point_to_point.cpp:64-69).

Checked here, on scans above 131 072 points with freezing forced: the switch on gives the pairs of the switch off and of the
launch-by-launch evaluation (n_corr, iterations, flags, fitness equal; float64 sums in another order: T64 within 1e-10, the
tolerance tests/test_gpu_freeze.py puts between two summation orders), and sf_icp_defer_stats proves which path ran; the
result is bitwise equal from run to run, under graph replay, on two lanes and through the stepping API."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_SCAN = 140_000          # above 131 072: two queries per lane, the launch list
TOL = 1e-10


@pytest.fixture(scope="module")
def world(api, ctx, orc, synth):
    raw = synth.make_map(400_000)
    ds = orc.voxel_pcl(raw, 0.1)[0]
    mp = api.Map(ctx, api.Cloud(ctx, ds), 0.25)
    mp.estimate_normals(0.25)
    scans = np.stack([synth.make_scan(ds, N_SCAN, scan_id=40 + k)[0] for k in range(3)])
    inits = np.stack([np.eye(4), synth.make_T((0.04, -0.03, 0.02), (0.2, -0.1, 0.3)), synth.make_T((-0.05, 0.05, 0.0), (0.0, 0.3, -0.4))])
    return dict(map=ds, mp=mp, scans=scans, inits=inits)


def make_icp(api, ctx, mp, scans, inits, freeze=True, defer=True, graph=False, params=None, thr=0.5, iters=20, order="cell"):
    icp = api.Icp(ctx, thr, iters, 0.05, 1e-5)
    icp.set_target(mp)
    icp.use_graph(graph)
    icp.set_query_order(order)
    icp.set_freeze(freeze)
    icp.set_defer_search(defer)
    if params:
        icp.set_freeze_params(**params)
    icp.set_source_batch(scans)
    icp.set_initial_batch(inits)
    return icp


def run(api, ctx, mp, scans, inits, **kw):
    icp = make_icp(api, ctx, mp, scans, inits, **kw)
    res = icp.align_batch("p2plane")
    fz, df = icp.freeze_stats(), icp.defer_stats()
    icp.close()
    return res, fz, df


def same_result(a, b, tol=TOL):
    for x, y in zip(a, b):
        assert x["iterations"] == y["iterations"] and x["n_corr"] == y["n_corr"] and x["flags"] == y["flags"] and x["converged"] == y["converged"]
        assert x["fitness"] == y["fitness"]
        d = np.abs(x["T64"] - y["T64"]).max()
        print("max |dT64| %.3e" % d)
        assert np.array_equal(np.isnan(x["T64"]), np.isnan(y["T64"])) and not d >= tol, d


def bitwise(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x["T64"], y["T64"], equal_nan=True) and x["n_corr"] == y["n_corr"] and x["iterations"] == y["iterations"]
        assert x["rmse"] == y["rmse"] or (np.isnan(x["rmse"]) and np.isnan(y["rmse"]))


def three_ways(api, ctx, mp, scans, inits, **kw):
    """switch on / switch off / frozen pairs off; returns the switch-on results and counters"""
    plain, fz0, df0 = run(api, ctx, mp, scans, inits, freeze=False, **{k: v for k, v in kw.items() if k != "params"})
    off, fz1, df1 = run(api, ctx, mp, scans, inits, defer=False, **kw)
    on, fz2, df2 = run(api, ctx, mp, scans, inits, defer=True, **kw)
    print("freeze", fz2, "defer", df2)
    assert df0 == {"deferred_queries": 0, "capped_waves": 0} and df1 == df0
    same_result(on, off)
    same_result(on, plain)
    return on, fz2, df2


def test_switch_on_equals_switch_off_and_the_launch_by_launch_evaluation(api, ctx, world):
    on, fz, df = three_ways(api, ctx, world["mp"], world["scans"], world["inits"])
    assert fz["froze"] >= 3 and fz["frozen_at_end"] == 3
    assert df["deferred_queries"] > 0
    again, _, df2 = run(api, ctx, world["mp"], world["scans"], world["inits"])
    bitwise(on, again)                                                        # run to run
    assert df2 == df
    replay, _, df3 = run(api, ctx, world["mp"], world["scans"], world["inits"], graph=True)
    bitwise(on, replay)                                                       # graph replay == plain launches
    assert df3 == df


def test_two_lanes_equal_one_lane(api, ctx, world):
    out = []
    for pipeline in (False, True):
        icp = make_icp(api, ctx, world["mp"], world["scans"], world["inits"], graph=True, params=dict(from_launch=5))   # (pinned: no schedule learnt from the first alignment)
        icp.set_pipeline(pipeline)
        icp.align_batch_async("p2plane")
        if pipeline:
            icp.align_batch_async("p2plane")                                  # the other lane, its own lists and rows, beside the first
            out.append((icp.fetch_previous(), icp.fetch_results()))
        else:
            first = icp.fetch_results()
            icp.align_batch_async("p2plane")
            out.append((first, icp.fetch_results()))
        assert icp.defer_stats()["deferred_queries"] > 0
        icp.close()
    bitwise(out[0][0], out[0][1])
    bitwise(out[0][0], out[1][0])
    bitwise(out[0][1], out[1][1])


def test_stepping_equals_one_shot(api, ctx, world):
    one, _, df = run(api, ctx, world["mp"], world["scans"], world["inits"], params=dict(from_launch=5))
    icp = make_icp(api, ctx, world["mp"], world["scans"], world["inits"], params=dict(from_launch=5))
    for k in range(20):
        icp.step_begin("p2plane", first=1 if k == 0 else 0)
        icp.step_end("p2plane", last=(k == 19))
    stepped = icp.fetch_results()
    assert icp.defer_stats() == df and df["deferred_queries"] > 0
    icp.close()
    bitwise(one, stepped)


def fuzz_map(rng, kind, n_map, ext, clusters=400):
    """uniform slab (0), clustered with every seventh point an exact twin of its neighbour in the array (1), lattice (2), two planes (3)"""
    if kind == 0:
        m = rng.uniform(-ext, ext, (n_map, 3)) * [1.0, 1.0, 0.2]
    elif kind == 1:
        c = rng.uniform(-ext, ext, (clusters, 3))
        m = c[rng.integers(0, clusters, n_map)] + rng.normal(0, 0.2, (n_map, 3))
        k7 = len(m[1::7])
        m[::7][:k7] = m[1::7]
    elif kind == 2:
        m = np.round(rng.uniform(-ext, ext, (n_map, 3)) * [1.0, 1.0, 0.2] * 8) / 8
    else:
        m = rng.uniform(-ext, ext, (n_map, 3))
        m[: n_map // 2, 2] = 0.0
        m[n_map // 2:, 0] = 2.0
    return m.astype(np.float32)


@pytest.mark.parametrize("scan_from", ["all", "unique"])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_clustered_duplicated_lattice_and_planar_maps(api, ctx, synth, kind, scan_from):
    """The maps of test_nn_reuse_fuzz_wide_scans (tests/test_gpu_parity.py), one of each kind, with from_launch 5 (the default): launch
    index 4 is the deferring one whether or not a freeze is ever asked for, and the counters must show that it ran.
    "all": scan points drawn from every map point, as that test does.  On the clustered map (every seventh point an exact
    duplicate of its neighbour in the array) and on the lattice map (several points per lattice site) a query whose neighbour
    has an exact twin can never certify -- the runner-up is as near as the neighbour --, so two in seven / most queries fail in
    every launch, every wave holds more than the cap and searches in place: capped waves > 0 is what proves the path there.
    "unique": scan points drawn from the map points that have no exact twin, and from_launch 9 (launch index 8 defers: the
    clustered map holds a thousand points per cluster 0.03 m apart, where at launch 4 the pose still moves by more than the
    margin between neighbour and runner-up); the same maps, but now only stragglers fail, and every kind must show deferred
    queries > 0."""
    rng = np.random.default_rng(780 + kind)
    n_map = int(rng.integers(100_000, 400_000))
    ext = float(rng.choice([6.0, 12.0, 20.0]))
    m = fuzz_map(rng, kind, n_map, ext)
    mp = api.Map(ctx, api.Cloud(ctx, m), float(rng.choice([0.0, 0.25, 0.5])))
    mp.estimate_normals(0.4)
    n_scan = int(rng.integers(131_073, 160_000))
    pool = np.arange(len(m))
    if scan_from == "unique":
        _, inv, cnt = np.unique(m, axis=0, return_inverse=True, return_counts=True)
        pool = np.nonzero(cnt[inv.ravel()] == 1)[0]
        assert len(pool) > 1000
    scans = []
    for s in range(3):
        T = synth.make_T(rng.normal(0, 0.08 if s else 0.01, 3), rng.normal(0, 0.6 if s else 0.05, 3))
        idx = pool[rng.integers(0, len(pool), n_scan)]
        p = m[idx].astype(np.float64) + rng.normal(0, 0.02, (n_scan, 3))
        Ti = np.linalg.inv(T)
        scans.append((p @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32))
    scans, inits = np.stack(scans), np.stack([np.eye(4)] * 3)
    late = scan_from == "unique"
    on, fz, df = three_ways(api, ctx, mp, scans, inits, thr=float(rng.choice([0.3, 0.5, 1.0])), iters=12, order="cell" if kind % 2 else "as_given",
                            params=dict(from_launch=9) if late else None)
    assert min(r["iterations"] for r in on) > (9 if late else 5)   # every scan reaches the deferring launch
    if scan_from == "all" and kind in (1, 2):
        assert df["capped_waves"] > 0
    else:
        assert df["deferred_queries"] > 0


def test_nan_points_and_points_beyond_the_map(api, ctx, world):
    scans = world["scans"].copy()
    n = scans.shape[1]
    scans[0, : n // 3] += np.array([0.0, 0.0, 30.0], dtype=np.float32)          # far above the map: no pair, ever
    scans[1, ::7] += np.array([500.0, 0.0, 0.0], dtype=np.float32)              # beyond the grid's box
    scans[2, ::5] = np.nan
    scans[2, 1::97, 1] = np.inf
    on, fz, df = three_ways(api, ctx, world["mp"], scans, world["inits"], thr=0.3)
    assert fz["froze"] >= 2 and df["deferred_queries"] > 0


def test_a_start_so_far_off_that_some_waves_exceed_the_cap(api, ctx, synth, world):
    """Priors 0.08 m / 0.5 degrees off converge a few launches later: at the last verifying launch many waves hold more failing
    queries than the cap and search in place, next to waves that defer -- both branches in one launch."""
    rng = np.random.default_rng(21)
    inits = np.stack([synth.make_T(rng.normal(0, 0.08, 3), rng.normal(0, 0.5, 3)) @ T for T in world["inits"]])
    on, fz, df = three_ways(api, ctx, world["mp"], world["scans"], inits, iters=25, params=dict(from_launch=5))
    assert df["deferred_queries"] > 0 and df["capped_waves"] > 0


@pytest.mark.parametrize("from_launch", [4, 6])
def test_other_first_launches(api, ctx, world, from_launch):
    """from_launch 6: launch index 5 defers, index 4 searches in place; from_launch 4: the launch before it still runs one query
    per lane and searches nearly everything -- nothing is deferred and the counters say so"""
    on, fz, df = three_ways(api, ctx, world["mp"], world["scans"], world["inits"], params=dict(from_launch=from_launch, guard_max=1e-3))
    assert fz["froze"] >= 3
    assert (df["deferred_queries"] > 0) == (from_launch == 6) and (df["deferred_queries"] + df["capped_waves"] > 0) == (from_launch == 6)
    replay, _, df2 = run(api, ctx, world["mp"], world["scans"], world["inits"], graph=True, params=dict(from_launch=from_launch, guard_max=1e-3))
    bitwise(on, replay)
    assert df2 == df


def test_a_thaw_followed_by_a_refreeze(api, ctx, world):
    """A guard far below the next update's motion: every scan thaws at once and freezes again, up to max_tries times (those later
    launches run FZ_FEW workgroups per scan and search in place; the launch before the first freeze defers)."""
    on, fz, df = three_ways(api, ctx, world["mp"], world["scans"], world["inits"], params=dict(guard_scale=0.0, guard_min=1e-12, guard_max=1e-12))
    assert fz["thawed"] >= 3 and fz["froze"] >= 6 and df["deferred_queries"] > 0
