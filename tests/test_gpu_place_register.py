"""Place recognition end to end on the city (sf_place_db_add_cloud, sf_place_db_query_cloud, api.place_register):
the database is built on the device from the ray-cast keyframes, a query scan finds its keyframe and its yaw as the restatement says
(tests/place_ref_np.py; tests/test_place_rule.py shows the gaps of these fixtures), and ICP from the candidates ends where the oracle's
ICP from the restatement's candidate ends."""
import numpy as np
import pytest

import place_fixtures as fx
import place_ref_np as ref

pytestmark = pytest.mark.gpu

POSE_TOL_M, POSE_TOL_RAD = 1e-9, 1e-9          # GPU against the float64 oracle, O3D_P2P from one init (tests/test_gpu_parity.py)
MAX_CORR, ITERS = 0.5, 30


@pytest.fixture(scope="module")
def city_db(api, ctx):
    c = fx.city()
    db = api.PlaceDB(ctx, **c["prm"])
    for k, (scan, T) in enumerate(zip(c["scans"], c["poses"])):
        index, st = db.add(api.Cloud(ctx, scan), T)
        assert index == k and st["n_points"] == len(scan)
    yield db
    db.close()


@pytest.fixture(scope="module")
def city_map(api, ctx, synth):
    """the surfaces within 90 m of keyframe 7, where the near query stands: (points float32 [m, 3], Map)"""
    c = fx.city()
    b = c["boxes"]
    near = b[(np.abs(0.5 * (b[:, 0] + b[:, 3])) < 100.0) & (np.abs(0.5 * (b[:, 1] + b[:, 4])) < 100.0)]
    pts = synth.sample_city(near, 180.0, 200_000, seed=970)
    mp = api.Map(ctx, api.Cloud(ctx, pts), 0.5)
    yield pts, mp
    mp.close()


def test_the_database_holds_the_restatements_rows(city_db):
    desc, poses = city_db.download()
    want = fx.city_descriptors()[0]
    assert np.array_equal(desc.view(np.uint32), want.view(np.uint32)) and np.array_equal(poses, np.stack(fx.city()["poses"]))


def test_query_cloud_finds_the_keyframe_and_the_yaw(api, ctx, city_db):
    c = fx.city()
    keyframes, queries, near = fx.city_descriptors()
    scans = list(c["query_scans"]) + [c["near_scan"]]
    truth = list(zip(c["query_keyframes"], c["query_shifts"])) + [(c["near_keyframe"], c["near_shift"])]
    want_d, want_s = ref.distances(np.concatenate([queries, near[None]]), keyframes)
    for q, (scan, (kf, shift)) in enumerate(zip(scans, truth)):
        got = city_db.query_cloud(api.Cloud(ctx, scan), 4)
        want = ref.top_k(want_d[q:q + 1], want_s[q:q + 1], 4, c["poses"], 60)
        assert np.array_equal(got["idx"], want["idx"]) and np.array_equal(got["shift"], want["shift"]), q
        assert np.array_equal(got["dist"].view(np.uint64), want["dist"].view(np.uint64)), (q, np.abs(got["dist"] - want["dist"]).max())
        assert np.abs(got["poses"] - want["poses"]).max() <= 1e-12, q
        assert got["idx"][0, 0] == kf and got["shift"][0, 0] == shift, q
        assert got["stats"]["n_entries"] == 15 and got["build_stats"]["n_points"] == len(scan)
    plain = api.place_register(city_db, api.Cloud(ctx, scans[3]), k=4)
    assert plain["found"] and plain["icp"] is None and plain["chosen"] == 0 and plain["index"] == 7 and plain["shift"] == 15
    assert plain["T"].tobytes() == plain["candidates"]["poses"][0, 0].tobytes()
    empty = api.PlaceDB(ctx)
    none = api.place_register(empty, api.Cloud(ctx, scans[3]), k=4)
    assert not none["found"] and none["index"] == -1 and (none["candidates"]["idx"] == -1).all() and np.isposinf(none["candidates"]["dist"]).all()


def test_place_register_refines_to_where_the_oracle_ends(api, ctx, synth, orc, city_db, city_map):
    c = fx.city()
    pts, mp = city_map
    scan, truth = c["near_scan"], c["near_pose"]

    def make(batch):
        icp = api.Icp(ctx, MAX_CORR, ITERS)
        icp.set_target(mp)
        return icp

    r = api.place_register(city_db, api.Cloud(ctx, scan), k=4, icp=make)
    cand = r["candidates"]
    assert r["found"] and len(r["icp"]) == 4 and r["index"] == c["near_keyframe"] and r["shift"] == c["near_shift"] and r["chosen"] == 0
    # the batch member that Icp itself gives for those inits
    solver = make(4)
    solver.set_source_batch(np.broadcast_to(scan, (4,) + scan.shape))
    solver.set_initial_batch(cand["poses"][0])
    res = solver.align_batch("o3d_p2p")
    best = max(range(4), key=lambda j: (res[j]["fitness"], -res[j]["rmse"], -j))
    assert best == r["chosen"] and res[best]["T64"].tobytes() == r["T"].tobytes()
    solver.close()
    # the candidate is within 0.5 m and 3 degrees of the truth; ICP takes it nearer, to where the oracle's ICP from the restatement's candidate ends
    want_pose = ref.candidate_pose(c["poses"][c["near_keyframe"]], c["near_shift"], 60)
    before, after = synth.pose_error(cand["poses"][0, 0], truth), synth.pose_error(r["T"], truth)
    assert before[0] < 0.5 and before[1] < np.radians(3.0)
    o = orc.icp_o3d_p2p(scan, pts, want_pose, MAX_CORR, ITERS)
    dt, dr = synth.pose_error(r["T"], o["T"])
    print("candidate %.3e m %.3e rad from the truth, refined %.3e m %.3e rad; GPU against the oracle %.3e m %.3e rad (iterations %d / %d, fitness %.4f)"
          % (before + after + (dt, dr, r["icp"][0]["iterations"], o["iterations"], r["icp"][0]["fitness"])))
    assert dt < POSE_TOL_M and dr < POSE_TOL_RAD, (dt, dr)
    assert after[0] < before[0] and after[1] < before[1], (before, after)
