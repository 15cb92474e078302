"""Consecutive sf_icp_align_batch_async calls overlap on two internal lanes (sf_icp_set_pipeline, include/slamfusion.h): the
results must be those of the same alignment run alone -- same kernels, same data -- whatever is enqueued between the calls:
nothing (the alignments run side by side), new initial poses, a new source, a rebuilt target.  No reference counterpart (the
reference registers one scan per callback on one thread, localization_node.cpp:337, main.cpp:18)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(api, ctx, synth):
    raw = synth.make_map(300_000)
    cloud = api.Cloud(ctx, raw)
    cloud.voxel_downsample(0.1, "pcl")
    ds = cloud.download()
    mp = api.Map(ctx, cloud, 0.25)
    mp.estimate_normals(0.25)
    scans = np.stack([synth.make_scan(ds, 140_000, scan_id=70 + b)[0][:140_000] for b in range(4)])
    return dict(map=mp, ds=ds, scans=scans)


def make(api, ctx, world, pipeline, graph, iters=12):
    icp = api.Icp(ctx, 0.5, iters, 0.05, 1e-5)
    icp.set_target(world["map"])
    icp.use_graph(graph)
    icp.set_pipeline(pipeline)
    icp.set_freeze(True)
    icp.set_source_batch(world["scans"])
    icp.set_initial_batch(None)
    return icp


def bitwise(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x["T64"], y["T64"]) and x["iterations"] == y["iterations"] and x["n_corr"] == y["n_corr"] and x["rmse"] == y["rmse"]


@pytest.mark.parametrize("graph", [False, True])
def test_back_to_back_alignments_equal_one_alone(api, ctx, synth, world, graph):
    ref = make(api, ctx, world, False, graph).align_batch("p2plane")
    icp = make(api, ctx, world, True, graph)
    for _ in range(5):
        icp.align_batch_async("p2plane")
    bitwise(icp.fetch_results(), ref)
    bitwise(icp.align_batch("p2plane"), ref)            # and again, on the other lane
    for mode in ("o3d_p2p", "ref_cpp"):
        want = make(api, ctx, world, False, graph).align_batch(mode)
        for _ in range(3):
            icp.align_batch_async(mode)
        bitwise(icp.fetch_results(), want)


def test_inputs_changed_between_calls_are_seen(api, ctx, synth, world):
    icp = make(api, ctx, world, True, True)
    alone = make(api, ctx, world, False, True)
    inits = np.stack([synth.make_T((0.03 * k, -0.02, 0.01), (0.1 * k, 0.0, 0.2)) for k in range(4)])
    icp.align_batch_async("p2plane")
    icp.set_initial_batch(inits)                          # new priors while the first alignment is still in flight
    icp.align_batch_async("p2plane")
    alone.set_initial_batch(inits)
    bitwise(icp.fetch_results(), alone.align_batch("p2plane"))
    other = world["scans"][::-1].copy()
    icp.align_batch_async("p2plane")
    icp.set_source_batch(other)                           # a new source: uploaded behind the alignment in flight, seen by the next
    icp.set_initial_batch(inits)
    icp.align_batch_async("p2plane")
    alone.set_source_batch(other)
    alone.set_initial_batch(inits)
    bitwise(icp.fetch_results(), alone.align_batch("p2plane"))


def test_a_target_rebuilt_between_calls(api, ctx, synth, world):
    cloud = api.Cloud(ctx, world["ds"])
    mp = api.Map(ctx, cloud, 0.25)
    mp.estimate_normals(0.25)
    w = dict(world, map=mp)
    icp = make(api, ctx, w, True, True)
    icp.align_batch_async("p2plane")
    half = world["ds"][world["ds"][:, 0] > -2.0]          # the map shrinks while the alignment is in flight
    mp.build(api.Cloud(ctx, half), 0.25)
    mp.estimate_normals(0.25)
    icp.align_batch_async("p2plane")
    got = icp.fetch_results()
    alone = make(api, ctx, w, False, True)
    bitwise(got, alone.align_batch("p2plane"))


def test_random_call_sequences_equal_the_same_calls_on_one_lane(api, ctx, synth, small_world):
    """Seeded fuzz: the same random sequence of calls -- asynchronous alignments in all three modes, whole stepped alignments
    (sf_icp_step_begin / sf_icp_step_end, O3D_P2P and P2PLANE: they decline REF_CPP and the covariance switch, neither is drawn),
    new priors, new sources of several batch sizes and scan sizes, another iteration count, fetches -- on an object with the lanes
    and on one without; every fetched result must be bit-identical.  One source is larger in scans and in points than every other
    and is held back until a source is drawn behind an unfetched alignment, so its first upload goes ahead into buffers no
    alignment has sized yet.  Small scans through the launch list (sf_icp_set_fused(0)) keep it quick.  A second pair of objects
    with the single launch left on draws the same sequence without the stepped alignments, now and then with an injected barrier
    timeout in front of an alignment (the fetch redoes it through the launch list).  SF_FUZZ_TRIALS / SF_FUZZ_SEED override the
    defaults."""
    import os
    m = small_world["map"]
    mp = api.Map(ctx, api.Cloud(ctx, m), 0.25)
    mp.estimate_normals(0.25)
    rng = np.random.default_rng(int(os.environ.get("SF_FUZZ_SEED", "5")))
    shapes = [(6000, 3), (6000, 3), (6000, 3), (4000, 2), (5000, 4), (9000, 5)]          # (points per scan, scans); the last one beyond all others
    pool = [np.stack([synth.make_scan(m, n, scan_id=300 + 5 * k + b)[0][:n] for b in range(nb)]) for k, (n, nb) in enumerate(shapes)]
    assert all(pool[-1].shape[0] > q.shape[0] and pool[-1].shape[1] > q.shape[1] for q in pool[:-1])

    def pair(fused):
        out = []
        for pipe in (True, False):
            icp = api.Icp(ctx, 0.5, 8, 0.05, 1e-5)
            icp.set_target(mp)
            if not fused:
                icp.set_fused(False)
            icp.use_graph(True)
            icp.set_pipeline(pipe)
            icp.set_source_batch(pool[0])
            icp.set_initial_batch(None)
            out.append(icp)
        return out
    objs, single = pair(False), pair(True)
    pending = pending_single = False
    cur, iters, largest_used = 0, 8, False
    for t in range(int(os.environ.get("SF_FUZZ_TRIALS", "60"))):
        op = rng.choice(["align", "align", "align", "step", "inits", "source", "iters", "fetch"])
        if op == "align":
            mode = str(rng.choice(["p2plane", "o3d_p2p", "ref_cpp"]))
            inject = rng.integers(0, 8) == 0
            for icp in objs:
                icp.align_batch_async(mode)
            for icp in single:
                if inject:
                    icp.test_inject_barrier_timeout()
                icp.align_batch_async(mode)
            pending = pending_single = True
        elif op == "step":
            mode = str(rng.choice(["p2plane", "o3d_p2p"]))
            steps = iters + 1 if mode == "o3d_p2p" else iters         # (as the library's own stepping loops count them)
            for icp in objs:
                for k in range(steps):
                    icp.step_begin(mode, first=1 if k == 0 else 0)
                    icp.step_end(mode, last=(k == steps - 1))
            pending = True
        elif op == "inits":
            inits = np.stack([synth.make_T(rng.normal(0, 0.02, 3), rng.normal(0, 0.2, 3)) for _ in range(len(pool[cur]))])
            for icp in objs + single:
                icp.set_initial_batch(inits)
        elif op == "source":
            cur = int(rng.integers(0, len(pool) if largest_used else len(pool) - 1))
            if pending and not largest_used:                          # behind an unfetched alignment: now the largest one
                cur = len(pool) - 1
            largest_used = largest_used or cur == len(pool) - 1
            for icp in objs + single:
                icp.set_source_batch(pool[cur])
                icp.set_initial_batch(None)
            pending = pending_single = False
        elif op == "iters":
            iters = int(rng.integers(1, 12))
            for icp in objs + single:
                icp.set_num_iterations(iters)
        else:
            if pending:
                bitwise(objs[0].fetch_results(), objs[1].fetch_results())
            if pending_single:
                got, want = single[0].fetch_results(), single[1].fetch_results()
                assert len(got) == len(want)
                bitwise(got, want)
    if pending:
        bitwise(objs[0].fetch_results(), objs[1].fetch_results())
    if pending_single:
        got, want = single[0].fetch_results(), single[1].fetch_results()
        assert len(got) == len(want)
        bitwise(got, want)
    assert single[0].fused_count() > 0 and single[1].fused_count() > 0      # (the second pair did take the single launch)


def stepped(icp, mode, iters):
    steps = iters + 1 if mode == "o3d_p2p" else iters
    for k in range(steps):
        icp.step_begin(mode, first=1 if k == 0 else 0)
        icp.step_end(mode, last=(k == steps - 1))


def test_a_stepped_alignment_behind_a_source_set_ahead(api, ctx, synth, world):
    """sf_icp_align_batch_async on three scans, then -- no fetch -- a host source of FIVE scans with more points each and new
    priors, then a whole alignment through sf_icp_step_begin(first = 1) / sf_icp_step_end.  With the lanes on the source goes ahead
    (other source set, a lane's stream, output buffers left alone: SrcScope, icp_alloc(outputs = false)); the stepped alignment
    runs on the context's stream in the buffers at hand.  Its five results must be bitwise those of an object without the lanes
    given the same calls, and those of a fresh object that only ran the stepped alignment.

    What makes it pass: step_adopt_source, called by sf_icp_step_begin when first != 0 (csrc/sf_icp_pipeline.hpp) -- the context's stream
    waits for src_ready, and lane_reserve + the xchg_own reserve size the states, partial rows and exchange records for five
    scans.  Without it the step reads a source still uploading and writes five scans' states and records into buffers sized for
    three.  That fetch_results returns the stepped alignment's five scans (and not three, described by the asynchronous one) is the
    description sf_icp_step_begin(first = 1) now leaves in cur().meta."""
    iters = 12
    first = world["scans"][:3, :100_000].copy()
    second = np.concatenate([world["scans"], world["scans"][:1, ::-1]])        # five scans of 140 000 points
    assert len(second) == 5 and second.shape[1] > first.shape[1]
    inits = np.stack([synth.make_T((0.03 * k, -0.02, 0.01), (0.1 * k, 0.0, 0.2)) for k in range(5)])
    for mode in ("p2plane", "o3d_p2p"):
        got = []
        for pipeline, opening in ((True, True), (False, True), (False, False)):
            icp = make(api, ctx, world, pipeline, False, iters)
            if opening:
                icp.set_source_batch(first)
                icp.set_initial_batch(None)
                icp.align_batch_async("p2plane")
            icp.set_source_batch(second)
            icp.set_initial_batch(inits)
            stepped(icp, mode, iters)
            got.append(icp.fetch_results())
            icp.close()
        assert [len(g) for g in got] == [5, 5, 5]
        bitwise(got[0], got[1])
        bitwise(got[0], got[2])
        assert all(r["iterations"] > 0 and r["n_corr"] > 100_000 for r in got[0])


def test_a_shard_set_behind_a_source_set_ahead(api, ctx, synth, world):
    """The same opening -- an asynchronous alignment on three scans, then a larger host source of five scans set ahead of it --
    on every member of a group of three slabs, then sf_icp_set_shard and sf_icp_align_group (the construction of
    tests/test_robust_icp.py test_gpu_sharded_group_equals_unsharded).  Bitwise the results of a group built without the opening, and
    the unsharded alignment of the same scans to 1e-9 (that test's bar: only the order of the sums differs).

    What makes it pass: step_adopt_source at the head of an alignment in sf_icp_step_begin (first != 0), through which
    sf_icp_align_group starts every member (and, for sf_icp_align_sharded / _async, the same call at the head of
    sf_icp_align_sharded_async): SrcScope declines to go ahead only once the object IS sharded, so a shard set after the upload
    reaches the sharded path with src_ahead set and the states, partial rows and exchange records sized for three scans."""
    from slam_sensor_fusion_amd import sharded
    iters, max_dist = 12, 0.5
    ds = world["ds"]
    normals = world["map"].download_normals()[0]
    first = world["scans"][:3, :60_000].copy()
    second = np.concatenate([world["scans"], world["scans"][:1, ::-1]])[:, :100_000].copy()
    inits = np.stack([synth.make_T((0.03 * k, -0.02, 0.01), (0.1 * k, 0.0, 0.2)) for k in range(5)])

    def make_map(keep=None):
        mp = api.Map(ctx, api.Cloud(ctx, ds if keep is None else ds[keep]), 0.25)
        mp.set_normals(normals if keep is None else normals[keep])    # the same normals everywhere: not a source of difference
        return mp

    def make_icp(mp):
        icp = api.Icp(ctx, max_dist, iters, 0.05, 1e-5)
        icp.set_target(mp)
        icp.set_pipeline(True)
        icp.set_freeze(False)
        return icp
    ref_icp = make_icp(make_map())
    ref_icp.set_source_batch(second)
    ref_icp.set_initial_batch(inits)
    ref = ref_icp.align_batch("p2plane")
    edges = sharded.slab_edges(ds[:, 0], 3)
    out = []
    for opening in (True, False):
        members = []
        for r in range(3):
            icp = make_icp(make_map(sharded.slab_select(ds, edges, r, halo=max_dist + 0.3 + 0.25)))
            if opening:
                icp.set_source_batch(first)
                icp.set_initial_batch(None)
                icp.align_batch_async("p2plane")
            icp.set_source_batch(second)
            icp.set_initial_batch(inits)
            icp.set_shard(float(max(edges[r], -1e30)), float(min(edges[r + 1], 1e30)))
            members.append(icp)
        res, _ = api.align_group(members, "p2plane")
        out.append(res)
        for icp in members:
            icp.close()
    assert len(out[0]) == len(out[1]) == 5
    bitwise(out[0], out[1])
    for b in range(5):
        assert out[0][b]["iterations"] == ref[b]["iterations"] == iters and out[0][b]["n_corr"] == ref[b]["n_corr"]
        dt, dr = synth.pose_error(out[0][b]["T64"], ref[b]["T64"])
        assert dt < 1e-9 and dr < 1e-9, (b, dt, dr)


def test_fetch_previous_delivers_every_result_of_a_stream(api, ctx, synth, world):
    """The streaming loop of include/slamfusion.h (sf_icp_fetch_previous): enqueue the next alignment, fetch the one before it.
    Every result is that of the same alignment run alone, bit for bit; new priors between the calls are seen by the next
    alignment only."""
    inits = [None] + [np.stack([synth.make_T((0.02 * k * s, -0.01 * s, 0.01), (0.1 * k, 0.05 * s, 0.2)) for k in range(4)]) for s in (1, 2, 3)]
    alone = make(api, ctx, world, False, True)
    want = []
    for T in inits:
        alone.set_initial_batch(T)
        want.append(alone.align_batch("p2plane"))
    icp = make(api, ctx, world, True, True)
    got = []
    for i, T in enumerate(inits):
        icp.set_initial_batch(T)
        icp.align_batch_async("p2plane")
        if i > 0:
            got.append(icp.fetch_previous())
    got.append(icp.fetch_results())
    assert len(got) == len(want)
    for g, w in zip(got, want):
        bitwise(g, w)
    # nothing left: the previous one was fetched, and after a fetch the next alignment takes the buffers at hand
    with pytest.raises(api.SlamFusionError):
        icp.fetch_previous()
    icp.align_batch_async("p2plane")
    with pytest.raises(api.SlamFusionError):
        icp.fetch_previous()
    bitwise(icp.fetch_results(), want[-1])


def test_fetch_previous_across_modes_and_batch_sizes(api, ctx, synth, world):
    """The earlier alignment is described by what it was enqueued with: another mode, another number of scans."""
    icp = make(api, ctx, world, True, False)
    alone = make(api, ctx, world, False, False)
    icp.align_batch_async("o3d_p2p")                      # four scans, point-to-point
    two = world["scans"][:2].copy()
    icp.set_source_batch(two)
    icp.set_initial_batch(None)
    icp.align_batch_async("p2plane")                      # two scans, point-to-plane, beside it
    first = icp.fetch_previous()
    bitwise(first, alone.align_batch("o3d_p2p"))
    alone.set_source_batch(two)
    alone.set_initial_batch(None)
    bitwise(icp.fetch_results(), alone.align_batch("p2plane"))
    # pipeline off: alignments share one set of buffers, there is never a previous one to fetch
    off = make(api, ctx, world, False, False)
    off.align_batch_async("p2plane")
    off.align_batch_async("p2plane")
    with pytest.raises(api.SlamFusionError):
        off.fetch_previous()
    off.fetch_results()


def test_a_stream_of_new_batches_equals_each_alone(api, ctx, synth, world):
    """The whole streaming loop: a NEW source batch and new priors every step, set while the previous step's alignment is in
    flight (the upload takes the other source set on the next lane's stream, sf_icp_pipeline.hpp SrcScope), the previous step's results
    fetched while this step runs.  Every step's results are those of the same batch registered alone, bit for bit -- also when a
    step sets its source twice, changes the number of scans, or fetches in between."""
    rng = np.random.default_rng(11)
    pool = [world["scans"], world["scans"][::-1].copy(), world["scans"][[1, 3, 0, 2]].copy(), world["scans"][:2].copy(), world["scans"][1:4].copy()]
    plan = [0, 1, 2, 3, 1, 4, 0, 2, 2, 1]
    steps = []
    for i, k in enumerate(plan):
        B = len(pool[k])
        inits = np.stack([synth.make_T(rng.normal(0, 0.02, 3), rng.normal(0, 0.2, 3)) for _ in range(B)])
        steps.append((k, inits))
    alone = make(api, ctx, world, False, True)
    want = []
    for k, inits in steps:
        alone.set_source_batch(pool[k])
        alone.set_initial_batch(inits)
        want.append(alone.align_batch("p2plane"))
    for graph in (True, False):
        icp = make(api, ctx, world, True, graph)
        got, prev_batch = [], None
        for i, (k, inits) in enumerate(steps):
            if i == 4:
                icp.set_source_batch(pool[0])             # a source that is replaced before any alignment reads it
            icp.set_source_batch(pool[k])
            icp.set_initial_batch(inits)
            if i == 6:                                    # a fetch between the source and its alignment: the latest alignment, as it was enqueued
                got.append(icp.fetch_results())
                prev_batch = None
            icp.align_batch_async("p2plane")
            if prev_batch is not None:
                got.append(icp.fetch_previous())
            prev_batch = len(pool[k])
        got.append(icp.fetch_results())
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert len(g) == len(w)
            bitwise(g, w)


def test_priors_set_before_the_next_source_are_kept(api, ctx, synth, world):
    """The setters are order independent: priors set BEFORE a source of the same number of scans stay, also when that source goes
    into the other source set because an alignment is in flight (whose batch size the set at hand may not share)."""
    inits = np.stack([synth.make_T((0.03 * k, -0.02, 0.01), (0.1 * k, 0.0, 0.2)) for k in range(4)])
    other = world["scans"][::-1].copy()
    alone = make(api, ctx, world, False, True)
    alone.set_source_batch(other)
    alone.set_initial_batch(inits)
    want = alone.align_batch("p2plane")
    icp = make(api, ctx, world, True, True)
    icp.align_batch_async("p2plane")
    icp.set_initial_batch(inits)
    icp.set_source_batch(other)                           # ahead of the alignment in flight: the first use of the second source set
    icp.align_batch_async("p2plane")
    icp.fetch_previous()
    bitwise(icp.fetch_results(), want)


def test_random_streams_deliver_every_result(api, ctx, synth, small_world):
    """Seeded fuzz of the streaming loop: random sources (three batches of different sizes, set once or twice, before or after the
    priors), priors, modes and iteration counts; one object streams -- enqueue, then sf_icp_fetch_previous, now and then a plain
    fetch in between -- the other registers every step alone.  EVERY step's results must agree bit for bit.  Launch list only
    (sf_icp_set_fused(0)); SF_FUZZ_TRIALS / SF_FUZZ_SEED override the defaults."""
    import os
    m = small_world["map"]
    mp = api.Map(ctx, api.Cloud(ctx, m), 0.25)
    mp.estimate_normals(0.25)
    rng = np.random.default_rng(int(os.environ.get("SF_FUZZ_SEED", "9")))
    pool = [np.stack([synth.make_scan(m, n, scan_id=400 + 5 * k + b)[0][:n] for b in range(nb)]) for k, (n, nb) in enumerate(((6000, 3), (4000, 2), (7000, 4)))]
    objs = []
    for pipe in (True, False):
        icp = api.Icp(ctx, 0.5, 8, 0.05, 1e-5)
        icp.set_target(mp)
        icp.set_fused(False)
        icp.use_graph(True)
        icp.set_pipeline(pipe)
        icp.set_source_batch(pool[0])
        icp.set_initial_batch(None)
        objs.append(icp)
    stream, alone = objs
    cur = 0
    want, got = [], []
    in_flight = 0        # alignments of `stream` enqueued and not fetched (0, 1 or 2)
    for t in range(int(os.environ.get("SF_FUZZ_TRIALS", "80"))):
        op = rng.choice(["align", "align", "align", "source", "inits", "iters", "fetch"])
        if op == "source":
            for _ in range(int(rng.integers(1, 3))):      # now and then a source that is replaced before it is read
                cur = int(rng.integers(0, 3))
                for icp in objs:
                    icp.set_source_batch(pool[cur])
                    icp.set_initial_batch(None)
        elif op == "inits":
            inits = np.stack([synth.make_T(rng.normal(0, 0.02, 3), rng.normal(0, 0.2, 3)) for _ in range(len(pool[cur]))])
            for icp in objs:
                icp.set_initial_batch(inits)
        elif op == "iters":
            it = int(rng.integers(1, 12))
            for icp in objs:
                icp.set_num_iterations(it)
        elif op == "fetch":
            if in_flight == 1:
                got.append(stream.fetch_results())
                in_flight = 0
        else:
            mode = str(rng.choice(["p2plane", "o3d_p2p", "ref_cpp"]))
            want.append(alone.align_batch(mode))
            if in_flight == 2:                            # (two in flight at most: the older one first)
                raise AssertionError("test bookkeeping")
            stream.align_batch_async(mode)
            in_flight += 1
            if in_flight == 2:
                got.append(stream.fetch_previous())
                in_flight = 1
    if in_flight == 1:
        got.append(stream.fetch_results())
    assert len(got) == len(want) and len(want) > 10
    for g, w in zip(got, want):
        assert len(g) == len(w)
        bitwise(g, w)
