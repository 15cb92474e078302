"""Look-up launches (sf_icp_lookup_launch_stats; Schedule::lookup_first / defer_first in csrc/sf_schedule.hpp): an alignment on the frozen-pairs
schedule that consults the map's neighbour table runs every launch from the first that consults it (sf_icp_set_neighbour_research,
default 2) up to the launch before from_launch (sf_icp_set_freeze_params, default 5) through k_nn_red_df -- two queries per lane,
certificate, nearest gap and table first, what they leave to the dense pass k_nn_deferred -- instead of the one-query-per-lane
searching kernel.  No reference counterpart (the reference searches every point in every iteration,
localization/src/icp_point_to_point.cpp:64-69).

Checked here on the world of tests/test_gpu_neighbour_table.py (three scans of 140 000 points: the wide launch list, the table
and the frozen schedule all run): the pairs are those of the table off and of the launch-by-launch evaluation (iterations, n_corr,
flags, converged, fitness equal; the float64 sums are taken in another order: T64 within the 1e-10 that tests/test_gpu_freeze.py
puts between two summation orders); the counters say which launches ran in which form; the result is bitwise equal from run to
run, under graph replay, on two lanes and through the stepping API."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_SCAN = 140_000          # above 131 072: two queries per lane, the launch list
TOL = 1e-10
NONE = {"launches": 0, "deferred_queries": 0, "capped_waves": 0, "first": -1}


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
    return dict(map=ds, scans=scans, inits=inits, never=new_map("never"), always=new_map("always"))


def make_icp(api, ctx, mp, scans, inits, freeze=True, graph=False, profile=False, params=None, thr=0.5, iters=20, order="cell", research=None):
    icp = api.Icp(ctx, thr, iters, 0.05, 1e-5)
    icp.set_target(mp)
    icp.use_graph(graph)
    icp.set_query_order(order)
    icp.set_freeze(freeze)
    if params:
        icp.set_freeze_params(**params)
    if research is not None:
        icp.set_neighbour_research(research)
    if profile:
        icp.profile_enable(True)
    icp.set_source_batch(scans)
    icp.set_initial_batch(inits)
    return icp


def run(api, ctx, mp, scans, inits, **kw):
    icp = make_icp(api, ctx, mp, scans, inits, **kw)
    res = icp.align_batch("p2plane")
    out = dict(res=res, fz=icp.freeze_stats(), df=icp.defer_stats(), lk=icp.lookup_launch_stats(), nb=icp.neighbour_stats() if kw.get("profile") else None)
    icp.close()
    return out


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


def three_ways(api, ctx, world, scans, inits, from_launch=5, nbr_from=2, **kw):
    """table always / table never / frozen pairs off (with the table); returns the table-always run"""
    plain = run(api, ctx, world["always"], scans, inits, freeze=False, **{k: v for k, v in kw.items() if k != "params"})
    off = run(api, ctx, world["never"], scans, inits, **kw)
    on = run(api, ctx, world["always"], scans, inits, **kw)
    print("lookup", on["lk"], "defer", on["df"], "freeze", on["fz"], "| table never: defer", off["df"])
    assert plain["lk"] == NONE and off["lk"] == NONE
    assert plain["df"] == {"deferred_queries": 0, "capped_waves": 0}
    want = max(from_launch - nbr_from, 0) if nbr_from >= 1 else 0
    assert on["lk"]["launches"] == want and on["lk"]["first"] == (nbr_from if want else -1)
    if want:   # with a table every deferring launch is a look-up launch
        assert on["df"] == {k: on["lk"][k] for k in ("deferred_queries", "capped_waves")}
    same_result(on["res"], off["res"])
    same_result(on["res"], plain["res"])
    return on, off


def test_table_always_equals_never_and_frozen_pairs_off(api, ctx, world):
    on, off = three_ways(api, ctx, world, world["scans"], world["inits"])
    assert on["lk"]["launches"] == 3 and on["lk"]["first"] == 2          # the defaults: launch indices 2, 3 and 4
    assert on["fz"]["froze"] >= 3 and on["fz"]["frozen_at_end"] == 3
    prof = run(api, ctx, world["always"], world["scans"], world["inits"], profile=True)
    print("table", prof["nb"])
    assert prof["nb"]["served"] > 0 and prof["lk"] == on["lk"]
    bitwise(on["res"], prof["res"])                                       # the profiling counters change nothing


def test_run_to_run_and_graph_replay(api, ctx, world):
    a = run(api, ctx, world["always"], world["scans"], world["inits"])
    b = run(api, ctx, world["always"], world["scans"], world["inits"])
    bitwise(a["res"], b["res"])
    assert a["lk"] == b["lk"] and a["lk"]["launches"] == 3
    g = run(api, ctx, world["always"], world["scans"], world["inits"], graph=True)
    bitwise(a["res"], g["res"])
    assert g["lk"] == a["lk"]
    # one object, one captured graph per launch list: moving the first look-up launch is another list, not a replay of the old one
    icp = make_icp(api, ctx, world["always"], world["scans"], world["inits"], graph=True, params=dict(from_launch=5))
    bitwise(a["res"], icp.align_batch("p2plane"))
    icp.set_neighbour_research(3)
    moved = icp.align_batch("p2plane")
    assert icp.lookup_launch_stats()["launches"] == 2 and icp.lookup_launch_stats()["first"] == 3
    assert icp.graph_counts()[0] == 2
    icp.close()
    bitwise(moved, run(api, ctx, world["always"], world["scans"], world["inits"], research=3, params=dict(from_launch=5))["res"])


def test_two_lanes_equal_one_lane(api, ctx, world):
    out = []
    for pipeline in (False, True):
        icp = make_icp(api, ctx, world["always"], world["scans"], world["inits"], graph=True, params=dict(from_launch=5))   # (pinned: no schedule learnt from the first alignment)
        icp.set_pipeline(pipeline)
        icp.align_batch_async("p2plane")
        if pipeline:
            icp.align_batch_async("p2plane")                                  # the other lane: its own lists and deferred rows
            out.append((icp.fetch_previous(), icp.fetch_results()))
        else:
            first = icp.fetch_results()
            icp.align_batch_async("p2plane")
            out.append((first, icp.fetch_results()))
        assert icp.lookup_launch_stats()["launches"] == 3
        icp.close()
    bitwise(out[0][0], out[0][1])
    bitwise(out[0][0], out[1][0])
    bitwise(out[0][1], out[1][1])


def test_stepping_equals_one_shot(api, ctx, world):
    one = run(api, ctx, world["always"], world["scans"], world["inits"], params=dict(from_launch=5))
    icp = make_icp(api, ctx, world["always"], world["scans"], world["inits"], params=dict(from_launch=5))
    for k in range(20):
        icp.step_begin("p2plane", first=1 if k == 0 else 0)
        icp.step_end("p2plane", last=(k == 19))
    stepped = icp.fetch_results()
    assert icp.lookup_launch_stats() == one["lk"] and icp.defer_stats() == one["df"] and one["lk"]["launches"] == 3
    icp.close()
    bitwise(one["res"], stepped)


@pytest.mark.parametrize("from_launch", [4, 6, 9])
def test_other_freeze_launches(api, ctx, world, from_launch):
    """the look-up launches are the indices nbr_from .. from_launch - 1, and the launch at from_launch freezes as it does without a table"""
    prm = dict(from_launch=from_launch, guard_max=1e-3)
    on, off = three_ways(api, ctx, world, world["scans"], world["inits"], from_launch=from_launch, params=prm)
    assert on["lk"]["first"] == 2 and on["lk"]["launches"] == from_launch - 2
    assert on["fz"]["froze"] >= 3 and on["fz"]["froze"] == off["fz"]["froze"] and on["fz"]["frozen_at_end"] == off["fz"]["frozen_at_end"] == 3
    replay = run(api, ctx, world["always"], world["scans"], world["inits"], graph=True, params=prm)
    bitwise(on["res"], replay["res"])
    assert replay["lk"] == on["lk"]


@pytest.mark.parametrize("research", [3, 5, -1])
def test_other_first_look_up_launches(api, ctx, world, research):
    """sf_icp_set_neighbour_research moves the first look-up launch; from the freeze launch on (5) or switched off there is none and
    the schedule is the one without a table: launch index 4 alone defers"""
    on, off = three_ways(api, ctx, world, world["scans"], world["inits"], nbr_from=research, research=research, params=dict(from_launch=5))
    if research == 3:
        assert on["lk"]["launches"] == 2 and on["lk"]["first"] == 3
    else:
        assert on["lk"] == NONE and on["df"]["deferred_queries"] > 0
    if research == -1:
        bitwise(on["res"], off["res"])                                    # no table consulted: the same launches


def test_a_start_so_far_off_that_some_waves_exceed_the_cap(api, ctx, synth, world):
    """Priors 0.08 m / 0.5 degrees further off: the early look-up launches still move the pose by more than the table's radii allow for
    many queries -- waves with more than the cap left search in place next to waves that defer."""
    rng = np.random.default_rng(21)
    inits = np.stack([synth.make_T(rng.normal(0, 0.08, 3), rng.normal(0, 0.5, 3)) @ T for T in world["inits"]])
    on, _ = three_ways(api, ctx, world, world["scans"], inits, iters=25, params=dict(from_launch=5))
    assert on["lk"]["deferred_queries"] > 0 and on["lk"]["capped_waves"] > 0
    # one look-up launch alone (the first moved up to index 4, the last before the freeze launch): both branches in ONE launch
    single, _ = three_ways(api, ctx, world, world["scans"], inits, iters=25, nbr_from=4, research=4, params=dict(from_launch=5))
    assert single["lk"]["launches"] == 1 and single["lk"]["deferred_queries"] > 0 and single["lk"]["capped_waves"] > 0


@pytest.mark.parametrize("max_corr", [0.03, 0.05])
def test_acceptance_radius_below_half_the_point_spacing(api, ctx, world, synth, max_corr):
    """max_corr far below the 0.1 m voxel spacing: served queries often have NO neighbour within max_corr and their entries say so"""
    inits = np.stack([synth.make_T((0.02, -0.015, 0.01), (0.1, -0.05, 0.15)), synth.make_T((0.03, 0.02, -0.02), (0.0, 0.2, -0.2)),
                      synth.make_T((-0.025, 0.025, 0.0), (0.15, 0.1, 0.0))])
    on, _ = three_ways(api, ctx, world, world["scans"], inits, thr=max_corr)
    assert on["lk"]["launches"] == 3 and min(r["n_corr"] for r in on["res"]) > 1000
    prof = run(api, ctx, world["always"], world["scans"], inits, thr=max_corr, profile=True)
    assert prof["nb"]["served"] > 0
    bitwise(on["res"], prof["res"])


def test_nan_points_and_points_beyond_the_map(api, ctx, world):
    scans = world["scans"].copy()
    n = scans.shape[1]
    scans[0, : n // 3] += np.array([0.0, 0.0, 30.0], dtype=np.float32)          # far above the map: no pair, ever
    scans[1, ::7] += np.array([500.0, 0.0, 0.0], dtype=np.float32)              # beyond the grid's box
    scans[2, ::5] = np.nan
    scans[2, 1::97, 1] = np.inf
    on, _ = three_ways(api, ctx, world, scans, world["inits"], thr=0.3)
    assert on["lk"]["launches"] == 3 and on["fz"]["froze"] >= 2


@pytest.mark.parametrize("kind", [1, 2])
def test_duplicated_and_lattice_maps(api, ctx, synth, kind):
    """Kinds 1 and 2 of test_clustered_duplicated_lattice_and_planar_maps (tests/test_gpu_deferred_search.py) at its sizes, scan
    points drawn from every map point: every seventh point an exact duplicate / several points per 1/8 m lattice site.  A point with
    an exact twin has nearest gap 0, so a tried lane with such a cached neighbour passes the gap by and reads the table entry, whose
    rule cannot hold either: those queries are left to the cap or the dense pass in every look-up launch."""
    rng = np.random.default_rng(780 + kind)
    n_map = int(rng.integers(100_000, 400_000))
    ext = float(rng.choice([6.0, 12.0, 20.0]))
    if kind == 1:
        c = rng.uniform(-ext, ext, (400, 3))
        m = c[rng.integers(0, 400, n_map)] + rng.normal(0, 0.2, (n_map, 3))
        k7 = len(m[1::7])
        m[::7][:k7] = m[1::7]
    else:
        m = np.round(rng.uniform(-ext, ext, (n_map, 3)) * [1.0, 1.0, 0.2] * 8) / 8
    m = m.astype(np.float32)
    cell = float(rng.choice([0.0, 0.25, 0.5]))
    maps = {}
    for mode in ("never", "always"):
        maps[mode] = api.Map(ctx, api.Cloud(ctx, m), cell)
        maps[mode].estimate_normals(0.4)
        maps[mode].set_neighbour_table(mode)
    n_scan = int(rng.integers(131_073, 160_000))
    scans = []
    for s in range(3):
        T = synth.make_T(rng.normal(0, 0.08 if s else 0.01, 3), rng.normal(0, 0.6 if s else 0.05, 3))
        idx = rng.integers(0, len(m), n_scan)
        p = m[idx].astype(np.float64) + rng.normal(0, 0.02, (n_scan, 3))
        Ti = np.linalg.inv(T)
        scans.append((p @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32))
    scans, inits = np.stack(scans), np.stack([np.eye(4)] * 3)
    on, _ = three_ways(api, ctx, maps, scans, inits, thr=float(rng.choice([0.3, 0.5, 1.0])), iters=12, order="cell" if kind % 2 else "as_given")
    assert on["lk"]["launches"] == 3 and min(r["iterations"] for r in on["res"]) > 5
    assert on["lk"]["capped_waves"] > 0


def test_the_next_alignment_starts_its_look_up_launches_behind_the_capped_ones(api, ctx, synth, world):
    """From the far-off priors of the cap test, from_launch left to the library: the first alignment's early look-up launches hold
    capped waves by the thousand (more than one wave in eight), so the second alignment of the same object starts its look-up
    launches later or has none -- same pairs either way; with from_launch pinned nothing is learnt."""
    rng = np.random.default_rng(21)
    inits = np.stack([synth.make_T(rng.normal(0, 0.08, 3), rng.normal(0, 0.5, 3)) @ T for T in world["inits"]])
    for pinned in (False, True):
        icp = make_icp(api, ctx, world["always"], world["scans"], inits, iters=25, graph=True, params=dict(from_launch=5) if pinned else None)
        first = icp.align_batch("p2plane")
        lk1 = icp.lookup_launch_stats()
        second = icp.align_batch("p2plane")
        lk2 = icp.lookup_launch_stats()
        icp.close()
        print("pinned", pinned, lk1, lk2)
        assert lk1["first"] == 2 and lk1["capped_waves"] * 8 > 3 * 274 * 4 * lk1["launches"]   # (3 scans x 274 rows x 4 waves per launch)
        if pinned:
            assert lk2 == lk1
            bitwise(first, second)
        else:
            assert lk2["first"] == -1 or lk2["first"] > 2
            same_result(first, second)


# ---------------------------------------------------------------- the schedule as a value (csrc/sf_schedule.hpp)
def old_key_sum(eps, guard_scale=8.0, guard_min=2.0e-5, guard_max=3.0e-4, max_tries=3):
    """the one float into which the captured graph's key used to fold the by-value parameters, in float32 as the library added them"""
    f = np.float32
    return f(f(f(f(f(eps) + f(f(guard_scale) * f(1.0e-3))) + f(guard_min)) + f(guard_max)) + f(max_tries))


def test_a_replay_never_outlives_the_transformation_epsilon(api, ctx, synth, world):
    """REF_CPP: k_ref_decide takes IcpParams by value inside the captured list.  1e-8 and 1e-7 are one float32 once 3.008 is added."""
    assert old_key_sum(1e-8) == old_key_sum(1e-7)
    scan = synth.make_scan(world["map"], 5_000, scan_id=77)[0]

    def new_icp(eps):
        icp = api.Icp(ctx, 0.5, 30, 1e-4, eps)
        icp.set_target(world["never"])
        icp.use_graph(True)
        icp.set_fused(False)
        icp.set_source(scan)
        return icp
    icp = new_icp(1e-8)
    before = icp.align("ref_cpp")
    assert icp.graph_counts()[0] == 1
    icp.set_transformation_epsilon(1e-7)
    after = icp.align("ref_cpp")
    captures = icp.graph_counts()[0]
    icp.close()
    fresh = new_icp(1e-7)
    want = fresh.align("ref_cpp")
    fresh.close()
    print("iterations at 1e-8: %d, at 1e-7: %d (fresh object %d); captures %d" % (before["iterations"], after["iterations"], want["iterations"], captures))
    assert captures == 2
    bitwise([after], [want])
    assert after["flags"] == want["flags"] and after["converged"] == want["converged"]


def test_a_replay_never_outlives_the_freeze_parameters(api, ctx, world):
    """P2PLANE, frozen pairs: k_reduce_solve_fz takes FreezeParams by value.  (2e-5, 3e-4) and (1.2e-4, 2e-4) have one float32 sum."""
    a, b = dict(guard_min=2e-5, guard_max=3e-4, from_launch=5), dict(guard_min=1.2e-4, guard_max=2e-4, from_launch=5)
    assert old_key_sum(1e-5, guard_min=a["guard_min"], guard_max=a["guard_max"]) == old_key_sum(1e-5, guard_min=b["guard_min"], guard_max=b["guard_max"])
    icp = make_icp(api, ctx, world["never"], world["scans"], world["inits"], graph=True, params=a)
    icp.align_batch("p2plane")
    assert icp.graph_counts()[0] == 1
    icp.set_freeze_params(**b)
    after = icp.align_batch("p2plane")
    captures, fz = icp.graph_counts()[0], icp.freeze_stats()
    icp.close()
    want = run(api, ctx, world["never"], world["scans"], world["inits"], graph=True, params=b)
    print("captures", captures, "freeze", fz, "fresh object", want["fz"])
    assert captures == 2
    bitwise(after, want["res"])
    assert fz == want["fz"] and [r["flags"] for r in after] == [r["flags"] for r in want["res"]]


@pytest.mark.parametrize("iters", [6, 20])
@pytest.mark.parametrize("table", ["never", "always"])
@pytest.mark.parametrize("defer", [True, False])
@pytest.mark.parametrize("research", [-1, 1, 2, 3])
@pytest.mark.parametrize("from_launch", [4, 5, 7])
def test_stepping_equals_one_shot_over_the_corners_of_the_schedule(api, ctx, world, from_launch, research, defer, table, iters):
    """the launch list and sf_icp_step_begin / _end read one schedule: the same launches, bit for bit, and the same account of them
    (tile search off: the stepping drivers have no tile form)"""
    out = []
    for stepped in (False, True):
        icp = make_icp(api, ctx, world[table], world["scans"], world["inits"], iters=iters, research=research, params=dict(from_launch=from_launch))
        icp.set_defer_search(defer)
        icp.set_tile_search(False)
        if stepped:
            for k in range(iters):
                icp.step_begin("p2plane", first=1 if k == 0 else 0)
                icp.step_end("p2plane", last=(k == iters - 1))
            res = icp.fetch_results()
        else:
            res = icp.align_batch("p2plane")
        out.append(dict(res=res, df=icp.defer_stats(), lk=icp.lookup_launch_stats(), fz=icp.freeze_stats()))
        icp.close()
    one, stepped = out
    print("lookup", one["lk"], "defer", one["df"], "freeze", one["fz"])
    bitwise(one["res"], stepped["res"])
    assert [r["flags"] for r in one["res"]] == [r["flags"] for r in stepped["res"]]
    assert one["df"] == stepped["df"] and one["lk"] == stepped["lk"] and one["fz"] == stepped["fz"]


def test_the_statistics_describe_the_alignment_that_was_enqueued(api, ctx, world):
    """two lanes: the next batch's source (another batch size: one scan) goes ahead into the other source set while the alignment is
    unfetched -- its statistics stay those of its own schedule, and the next alignment is what it is alone"""
    prm = dict(from_launch=5)   # (pinned: the next alignment does not start from a schedule learnt here)
    alone = run(api, ctx, world["always"], world["scans"], world["inits"], params=prm)
    next_alone = run(api, ctx, world["always"], world["scans"][:1], world["inits"][:1], params=prm)
    icp = make_icp(api, ctx, world["always"], world["scans"], world["inits"], params=prm)
    icp.set_pipeline(True)
    icp.align_batch_async("p2plane")
    icp.set_source_batch(world["scans"][:1])
    icp.set_initial_batch(world["inits"][:1])
    res = icp.fetch_results()
    got = dict(df=icp.defer_stats(), lk=icp.lookup_launch_stats(), fz=icp.freeze_stats())
    nxt = icp.align_batch("p2plane")
    got_next = dict(df=icp.defer_stats(), lk=icp.lookup_launch_stats(), fz=icp.freeze_stats())
    icp.close()
    print("enqueued", got, "| next", got_next)
    assert len(res) == 3 and alone["lk"]["launches"] == 3
    bitwise(res, alone["res"])
    assert got["df"] == alone["df"] and got["lk"] == alone["lk"] and got["fz"] == alone["fz"]
    bitwise(nxt, next_alone["res"])
    assert got_next == {k: next_alone[k] for k in ("df", "lk", "fz")}
