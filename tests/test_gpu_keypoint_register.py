"""ISS keypoints in front of the device chain of test_gpu_global_register.py: the same terrain map
(synth.make_terrain(30, 0.2, 1), 22 801 points) and the same 5 020-point scan under reg_ref_np.pose(), FPFH at 1.0 m (normals at
0.5 m) oriented toward +z -- but only the keypoints' descriptors are matched, through api.global_register(src_keypoints=,
dst_keypoints=).  ISS at a salient radius of 0.6 m and a non-maximum radius of 0.4 m, gammas 0.975, min_neighbors 5, and
min_lambda3 = iss_ref_np.TERRAIN_FLOOR = 3.6e-7 m^2: the terrain's cylinders have exactly flat tops, where lambda3 is 0 in exact
arithmetic and whether a point is salient is rounding noise without the floor (with a floor of 0 the restatement has the same
971 map keypoints; the floor only makes the comparison flag for flag a safe one -- tests/test_iss_rule.py asserts its margins).

On the CPU, before this ran on a device, the restatement chain (iss_ref_np.keypoints under the float32 neighbour rule, the oracle's
radius normals, fpfh_ref_np.fpfh on both clouds, fpfh_ref_np.match of the keypoint rows, reg_ref_np.register at threshold 0.05,
similarity 0.9, H = 4096, seed 1) gave 971 map keypoints and 234 scan keypoints (174 of the scan keypoints' true partners lie within
0.3 m of a map keypoint), 174 mutual matches of the keypoint rows of which 102 are right (58.6 %), best = 6 with 102 inliers
(fitness 0.586, rmse 8.27 mm), and a pose that moves every scan point to within 2.0 mm of where the truth puts it: all four
conditions below hold for the restatement at these radii, so the radii stay.  The match is 234 x 971 rows instead of 5 020 x 22 801."""
import numpy as np
import pytest

import iss_ref_np as iss
import reg_ref_np as ref

pytestmark = pytest.mark.gpu

THR, SIM, H, SEED = 0.05, 0.9, 4096, 1
RS, RN = iss.TERRAIN_RADII


@pytest.fixture(scope="module")
def scene(api, ctx, synth):
    T = ref.pose()
    terrain, scan = iss.fixture("terrain_map")["points"], iss.fixture("terrain_scan")["points"]
    _, idx = synth.make_local_scan(terrain, (2.0, -1.0), 8.0, T, 0.005, 2)
    assert len(terrain) == 22801 and len(scan) == 5020 == len(idx)
    map_cloud, scan_cloud = api.Cloud(ctx, terrain), api.Cloud(ctx, scan)
    mp = api.Map(ctx, map_cloud, 0.5)
    mp.estimate_normals(0.5)
    f_map = mp.compute_fpfh(1.0, "direction", (0, 0, 1))[0]
    f_scan = scan_cloud.compute_fpfh(0.5, 1.0, "direction", (0, 0, 1))[0]
    k_map = mp.iss_keypoints(RS, RN, min_lambda3=iss.TERRAIN_FLOOR)
    k_scan = scan_cloud.iss_keypoints(RS, RN, min_lambda3=iss.TERRAIN_FLOOR)
    yield dict(T=T, terrain=terrain, scan=scan, idx=idx, map_cloud=map_cloud, scan_cloud=scan_cloud, map=mp, f_map=f_map, f_scan=f_scan, k_map=k_map, k_scan=k_scan)
    for obj in (f_scan, f_map, mp, scan_cloud, map_cloud):
        obj.close()


def test_the_keypoints_are_the_restatements(scene):
    for side, name in (("k_map", "terrain_map"), ("k_scan", "terrain_scan")):
        want = iss.reference(name)
        got = scene[side]
        print("%s: %d keypoints of %d salient points" % (name, got["stats"]["n_keypoints"], got["stats"]["n_salient"]))
        assert np.array_equal(got["indices"], want["indices"]) and got["stats"]["n_salient"] == want["stats"]["n_salient"]
    assert len(scene["k_map"]["indices"]) == 971 and len(scene["k_scan"]["indices"]) == 234
    assert np.array_equal(scene["k_map"]["flags"], iss.reference("terrain_map")["flags"])


def test_global_register_on_the_keypoints_finds_the_pose(api, scene):
    ks, km = scene["k_scan"]["indices"], scene["k_map"]["indices"]
    g = api.global_register(scene["scan_cloud"], scene["f_scan"], scene["map_cloud"], scene["f_map"], THR, num_hypotheses=H, seed=SEED, src_keypoints=ks, dst_keypoints=km)
    pairs = g["pairs"]
    right = scene["idx"][pairs[:, 0]] == pairs[:, 1]
    scan64 = scene["scan"].astype(np.float64)
    moved, want = scan64 @ g["T"][:3, :3].T + g["T"][:3, 3], scan64 @ scene["T"][:3, :3].T + scene["T"][:3, 3]
    err = np.linalg.norm(moved - want, axis=1).max()
    print("keypoints %d x %d: mutual matches %d, right %d (%.1f %%); %s; largest displacement from the truth %.2e m" % (
        len(ks), len(km), len(pairs), right.sum(), 100.0 * right.mean(), g["ransac"]["stats"], err))
    assert g["found"] == 1
    assert len(pairs) >= 50
    assert right.mean() > 0.4
    assert err < THR
    # the pairs index the clouds: keypoints on both sides, and the match saw only the gathered rows
    assert np.isin(pairs[:, 0], ks).all() and np.isin(pairs[:, 1], km).all()
    assert g["match_stats"]["n_src"] == len(ks) and g["match_stats"]["n_dst"] == len(km) and g["match_stats"]["n_matched"] == len(pairs)
    # fed to register_pairs directly they give the bits of the ransac entry
    r = scene["scan_cloud"].register_pairs(scene["map_cloud"], pairs, THR, SIM, H, 2, 3, 0, SEED)
    assert r["T"].tobytes() == g["ransac"]["T"].tobytes() == g["T"].tobytes() and np.array_equal(r["inlier"], g["ransac"]["inlier"])
    assert {k: v for k, v in r["stats"].items() if not k.endswith("_ms")} == {k: v for k, v in g["ransac"]["stats"].items() if not k.endswith("_ms")}
    # the same chain by hand: gather, match, map back
    m = scene["f_scan"].gather(ks).match(scene["f_map"].gather(km), mutual=True)
    assert np.array_equal(np.stack([ks[m["pairs"][:, 0]], km[m["pairs"][:, 1]]], 1), pairs)


def test_either_side_alone(api, scene):
    ks, km = scene["k_scan"]["indices"], scene["k_map"]["indices"]
    args = (scene["scan_cloud"], scene["f_scan"], scene["map_cloud"], scene["f_map"], THR)
    a = api.global_register(*args, num_hypotheses=H, seed=SEED, src_keypoints=ks)
    assert np.isin(a["pairs"][:, 0], ks).all() and a["match_stats"]["n_src"] == len(ks) and a["match_stats"]["n_dst"] == 22801
    b = api.global_register(*args, num_hypotheses=H, seed=SEED, dst_keypoints=km.astype(np.int64))
    assert np.isin(b["pairs"][:, 1], km).all() and b["match_stats"]["n_src"] == 5020 and b["match_stats"]["n_dst"] == len(km)
    assert a["pairs"].dtype == np.int32 and b["pairs"].dtype == np.int32


def test_without_keypoints_nothing_changes(api, scene):
    args = (scene["scan_cloud"], scene["f_scan"], scene["map_cloud"], scene["f_map"], THR)
    old = api.global_register(*args, num_hypotheses=H, seed=SEED)
    new = api.global_register(*args, num_hypotheses=H, seed=SEED, src_keypoints=None, dst_keypoints=None)
    assert old["T"].tobytes() == new["T"].tobytes() and np.array_equal(old["pairs"], new["pairs"]) and old["match_stats"]["n_matched"] == new["match_stats"]["n_matched"]
    assert np.array_equal(old["ransac"]["inlier"], new["ransac"]["inlier"]) and old["found"] == new["found"] == 1
    assert {k: v for k, v in old["ransac"]["stats"].items() if not k.endswith("_ms")} == {k: v for k, v in new["ransac"]["stats"].items() if not k.endswith("_ms")}
    assert len(old["pairs"]) > 1000                                      # the full-set match of test_gpu_global_register.py
