"""The device chain end to end: FPFH on a terrain map and on a local scan of it under a large unknown pose,
the mutual matches, sf_cloud_register_pairs on them, ICP from the estimate, and api.global_register.

The scene: synth.make_terrain(30, 0.2, 1) (22 801 points); the scan is the 5 020 points within 8 m of (2, -1) under
reg_ref_np.pose() -- 140 degrees of yaw and 12 m -- with sigma = 5 mm; FPFH at 1.0 m (normals at 0.5 m), both sides oriented toward
+z.  On the CPU, before this ran on a device, the numpy chain (PCA normals, fpfh_ref_np.fpfh, fpfh_ref_np.match, reg_ref_np.register
at threshold 0.05, similarity 0.9, H = 4096, seed 1) gave 3 929 mutual matches of which 3 234 are right, and a pose that moves
every scan point to within 0.31 mm of where the truth puts it (best = 6 with 3 234 inliers; the device chain returns the same figures).

ICP_TOL: the oracle's float64 Open3D-style ICP (oracle.icp_o3d_p2p, 0.5 m, 30 iterations) was run on this fixture from the numpy
chain's estimate and from the truth: both stop after 2 iterations, at one fixed point of one basin, 2.0e-15 m and 1.1e-16 rad apart.  Ten times that; the
device's two runs measured 4.0e-15 m and 3.9e-17 rad apart."""
import numpy as np
import pytest

import reg_ref_np as ref

pytestmark = pytest.mark.gpu

THR, SIM, H, SEED = 0.05, 0.9, 4096, 1
ICP_TOL = (10 * 1.9860273225978185e-15, 10 * 1.133029972839493e-16)      # metres, radians: ten times the oracle's own difference


@pytest.fixture(scope="module")
def scene(api, ctx, synth):
    T = ref.pose()
    terrain = synth.make_terrain(30, 0.2, 1)
    scan, idx = synth.make_local_scan(terrain, (2.0, -1.0), 8.0, T, 0.005, 2)
    assert len(terrain) == 22801 and len(scan) == 5020
    map_cloud, scan_cloud = api.Cloud(ctx, terrain), api.Cloud(ctx, scan)
    mp = api.Map(ctx, map_cloud, 0.5)
    mp.estimate_normals(0.5)
    f_map = mp.compute_fpfh(1.0, "direction", (0, 0, 1))[0]
    f_scan = scan_cloud.compute_fpfh(0.5, 1.0, "direction", (0, 0, 1))[0]
    yield dict(T=T, terrain=terrain, scan=scan, idx=idx, map_cloud=map_cloud, scan_cloud=scan_cloud, map=mp, f_map=f_map, f_scan=f_scan)
    for obj in (f_scan, f_map, mp, scan_cloud, map_cloud):
        obj.close()


def icp_factory(api, ctx, mp):
    def make(batch):
        icp = api.Icp(ctx, 0.5, 30)
        icp.set_target(mp)
        return icp
    return make


def test_the_chain_finds_the_pose(api, ctx, synth, scene):
    m = scene["f_scan"].match(scene["f_map"], mutual=True)
    pairs = m["pairs"]
    right = scene["idx"][pairs[:, 0]] == pairs[:, 1]
    print("mutual matches %d, right %d (%.1f %%)" % (len(pairs), right.sum(), 100.0 * right.mean()))
    assert len(pairs) > 1000 and right.mean() > 0.5               # the column section 21 found empty on the city
    r = scene["scan_cloud"].register_pairs(scene["map_cloud"], pairs, THR, SIM, H, 2, 3, 0, SEED)
    assert r["found"] == 1
    scan64 = scene["scan"].astype(np.float64)
    moved, want = scan64 @ r["T"][:3, :3].T + r["T"][:3, 3], scan64 @ scene["T"][:3, :3].T + scene["T"][:3, 3]
    err = np.linalg.norm(moved - want, axis=1).max()
    print("register_pairs: %s; largest displacement from the truth %.2e m" % (r["stats"], err))
    assert err < THR
    assert r["stats"]["n_inliers"] >= right.sum() * 0.95 and r["stats"]["fitness"] > 0.5
    # the inliers under the rule applied to the returned transform, exactly
    inl, n, fit, rmse = ref.final(*ref.pack(scene["scan"], scene["terrain"], pairs), r["T"], THR)
    assert np.array_equal(r["inlier"], inl) and (r["stats"]["n_inliers"], r["stats"]["fitness"], r["stats"]["rmse"]) == (n, fit, rmse)
    # ICP from the estimate ends where ICP from the truth ends
    ends = []
    for init in (r["T"], scene["T"]):
        icp = api.Icp(ctx, 0.5, 30)
        icp.set_target(scene["map"])
        icp.set_source(scene["scan"])
        icp.set_initial_transformation(np.asarray(init, np.float64))
        ends.append(icp.align("o3d_p2p"))
        icp.close()
    dt, dr = synth.pose_error(ends[0]["T64"], ends[1]["T64"])
    before, after = synth.pose_error(r["T"], scene["T"]), synth.pose_error(ends[0]["T64"], scene["T"])
    print("ICP from the estimate / from the truth: iterations %d / %d, apart %.3e m %.3e rad (tolerance %.1e m %.1e rad)" % (ends[0]["iterations"], ends[1]["iterations"],
                                                                                                                          dt, dr, ICP_TOL[0], ICP_TOL[1]))
    print("pose error against the truth before ICP %.3e m %.3e rad, after %.3e m %.3e rad" % (before + after))
    assert dt <= ICP_TOL[0] and dr <= ICP_TOL[1], (dt, dr)


def test_global_register_with_candidates_is_no_worse(api, ctx, synth, scene):
    make = icp_factory(api, ctx, scene["map"])
    args = (scene["scan_cloud"], scene["f_scan"], scene["map_cloud"], scene["f_map"], THR)
    plain = api.global_register(*args, num_hypotheses=H, seed=SEED)
    assert plain["found"] == 1 and plain["icp"] is None and plain["chosen"] is None and plain["T"].tobytes() == plain["ransac"]["T"].tobytes()
    single = api.global_register(*args, num_hypotheses=H, seed=SEED, top_k=0, icp=make)
    many = api.global_register(*args, num_hypotheses=H, seed=SEED, top_k=8, icp=make)
    assert len(single["icp"]) == 1 and len(many["icp"]) == 9 and len(many["ransac"]["top"]) == 8
    print("fitness: RANSAC %.4f, ICP from the refit pose %.6f, best of 9 %.6f (member %d)" % (plain["fitness"], single["fitness"], many["fitness"], many["chosen"]))
    assert many["fitness"] >= single["fitness"]
    assert many["icp"][8]["fitness"] == single["icp"][0]["fitness"]      # the refit pose is the last member of the batch
    dt, dr = synth.pose_error(many["T"], scene["T"])
    assert dt < 0.01 and dr < 1e-3, (dt, dr)                      # sigma = 5 mm over 5 020 points: the refined pose is well inside 1 cm
