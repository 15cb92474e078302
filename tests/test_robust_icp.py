"""Robust M-estimator kernels of point-to-plane ICP (sf_icp_set_robust_kernel, include/slamfusion.h).

The oracle has no robust mode, so this file carries its own numpy restatement of orc_icp_p2plane (oracle/icp.c) with a
per-pair weight: the same correspondences (orc.KdTreeD, d2 < max_dist^2), the same Jacobian and residual, the normal
equations sum w J J^T x = -sum w J r solved by numpy, Open3D's vec6 -> 4x4, exactly num_iters iterations.  With kind
"none" it equals the oracle (test 1), which licenses it as the reference for the GPU tests.

The dynamic-object scene is small_scene of tests/test_city_scan.py plus six seeded parked cars that the ray-cast scan
sees but the map does not hold: plain point-to-plane is pulled 35 mm / 0.024 deg off the true pose, Tukey (k = 0.1 m)
lands within 0.4 mm / 0.005 deg (CPU restatement; the bounds below leave room)."""
import ctypes as C

import numpy as np
import pytest

MAX_DIST, ITERS, N_CARS = 0.5, 25, 6
SF_ERR_INVALID = -1
KINDS = [("huber", 0.05), ("cauchy", 0.1), ("tukey", 0.1), ("gm", 0.1)]


# ------------------------------------------------------------------ the restatement
def vec6_to_mat4(v):
    """Open3D TransformVector6dToMatrix4d (oracle/icp.c vec6_to_mat4): R = Rz(v2) Ry(v1) Rx(v0), t = v[3:6]."""
    ca, sa, cb, sb, cg, sg = np.cos(v[0]), np.sin(v[0]), np.cos(v[1]), np.sin(v[1]), np.cos(v[2]), np.sin(v[2])
    T = np.eye(4)
    T[:3, :3] = [[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
                 [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                 [-sb, cb * sa, cb * ca]]
    T[:3, 3] = v[3:]
    return T


def robust_weight(kind, r, k):
    """The SF_ROBUST_* table of include/slamfusion.h."""
    a = np.abs(r)
    if kind == "none":
        return np.ones_like(r)
    if kind == "huber":
        return np.where(a <= k, 1.0, k / np.maximum(a, 1e-300))
    if kind == "cauchy":
        return 1.0 / (1.0 + (r / k) ** 2)
    if kind == "tukey":
        return np.where(a <= k, (1.0 - (r / k) ** 2) ** 2, 0.0)
    if kind == "gm":
        return (k * k / (k * k + r * r)) ** 2
    raise ValueError(kind)


def p2plane_robust(orc, src, tgt, normals, init, max_dist, num_iters, kind="none", k=0.0):
    t, s0, nrm = (np.asarray(a, np.float32).astype(np.float64) for a in (tgt, src, normals))
    tree = orc.KdTreeD(t)
    T = np.array(init, dtype=np.float64)
    it, nc, fit, rmse = 0, 0, 0.0, 0.0
    for _ in range(num_iters):
        pcd = s0 @ T[:3, :3].T + T[:3, 3]
        idx, d2 = tree.nn(pcd)
        ok = (idx >= 0) & (d2 < max_dist * max_dist)
        nc = int(ok.sum())
        fit = nc / len(s0)
        rmse = float(np.sqrt(d2[ok].sum() / nc)) if nc else 0.0
        s, q, n = pcd[ok], t[idx[ok]], nrm[idx[ok]]
        r = ((s - q) * n).sum(1)
        J = np.c_[np.cross(s, n), n]
        Jw = J * robust_weight(kind, r, k)[:, None]
        if nc < 6:
            break
        x = np.linalg.solve(Jw.T @ J, -(Jw.T @ r))
        T = vec6_to_mat4(x) @ T
        it += 1
    return dict(T=T, iterations=it, n_corr=nc, fitness=fit, rmse=rmse)


# ------------------------------------------------------------------ scenes
@pytest.fixture(scope="module")
def city(orc, synth):
    """small_scene of tests/test_city_scan.py, with the oracle's normals, plus the same pose seen with parked cars."""
    boxes = synth.make_city(80.0, 30)
    ds = orc.voxel_pcl(synth.sample_city(boxes, 80.0, 600_000), 0.1)[0]
    T_true = synth.make_T((1.0, -2.0, 1.8), (0.4, -0.3, 20.0))
    prior = synth.make_T((0.15, -0.1, 0.05), (0.0, 0.0, 0.8)) @ T_true
    normals, _ = orc.normals_radius(ds, 0.3)
    scan = synth.raycast_scan(boxes, T_true, rings=16, azimuths=360, max_range=40.0)
    cars = synth.make_cars(boxes, [T_true[:2, 3]], N_CARS)
    scan_cars = synth.raycast_scan(np.r_[boxes, cars], T_true, rings=16, azimuths=360, max_range=40.0)
    return dict(ds=ds, normals=normals, T_true=T_true, prior=prior, scan=scan, scan_cars=scan_cars)


def check_dynamic_bounds(synth, T_plain, T_tukey, T_true):
    dt_p, dr_p = synth.pose_error(T_plain, T_true)
    dt_t, dr_t = synth.pose_error(T_tukey, T_true)
    assert dt_p > 0.02 and dt_p >= 3.0 * dt_t and dr_p >= 3.0 * dr_t, (dt_p, dr_p, dt_t, dr_t)
    assert dt_t < 3e-3 and dr_t < np.radians(0.02), (dt_t, dr_t)    # a few mm, a few hundredths of a degree


# ------------------------------------------------------------------ CPU
def test_restatement_without_kernel_equals_oracle(orc, city):
    ref = orc.icp_p2plane(city["scan"], city["ds"], city["normals"], city["prior"], MAX_DIST, ITERS)
    me = p2plane_robust(orc, city["scan"], city["ds"], city["normals"], city["prior"], MAX_DIST, ITERS)
    from slam_sensor_fusion_amd import synth
    dt, dr = synth.pose_error(me["T"], ref["T"])
    assert dt < 1e-10 and dr < 1e-10, (dt, dr)                      # only the summation order differs
    assert me["iterations"] == ref["iterations"] == ITERS and me["n_corr"] == ref["n_corr"]
    assert abs(me["fitness"] - ref["fitness"]) < 1e-15 and abs(me["rmse"] - ref["error"]) < 1e-12


def test_restatement_shows_the_dynamic_object_effect(orc, synth, city):
    assert len(city["scan_cars"]) == len(city["scan"])               # every ray hits something; cars take some of them
    assert np.abs(city["scan_cars"] - city["scan"]).max() > 1.0
    plain = p2plane_robust(orc, city["scan_cars"], city["ds"], city["normals"], city["prior"], MAX_DIST, ITERS)
    tukey = p2plane_robust(orc, city["scan_cars"], city["ds"], city["normals"], city["prior"], MAX_DIST, ITERS, "tukey", 0.1)
    check_dynamic_bounds(synth, plain["T"], tukey["T"], city["T_true"])


def test_library_and_api_expose_the_setter(api):
    lib = api.load_library()
    assert hasattr(lib, "sf_icp_set_robust_kernel")
    assert callable(getattr(api.Icp, "set_robust_kernel", None))
    assert api.ROBUST_KINDS == {"none": 0, "huber": 1, "cauchy": 2, "tukey": 3, "gm": 4}


# ------------------------------------------------------------------ GPU
def make_map(api, ctx, city, keep=None):
    ds = city["ds"] if keep is None else city["ds"][keep]
    mp = api.Map(ctx, api.Cloud(ctx, ds), 0.25)
    mp.set_normals(city["normals"] if keep is None else city["normals"][keep])   # the oracle's normals: not a source of difference
    return mp


@pytest.fixture(scope="module")
def gmap(api, ctx, city):
    return make_map(api, ctx, city)


def make_icp(api, ctx, mp, kind="none", k=None, fused=True):
    icp = api.Icp(ctx, MAX_DIST, ITERS, 0.05, 1e-5)
    icp.set_target(mp)
    icp.set_fused(fused)
    if kind != "none":
        icp.set_robust_kernel(kind, k)
    return icp


def align_one(icp, scan, prior, mode="p2plane"):
    icp.set_source(scan)
    icp.set_initial_transformation(prior)
    return icp.align(mode)


def bitwise(a, b):
    assert np.array_equal(np.asarray(a["T64"]), np.asarray(b["T64"])), (a["T64"], b["T64"])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,k", KINDS)
def test_gpu_each_kind_matches_restatement(api, ctx, orc, synth, city, gmap, kind, k):
    ref = p2plane_robust(orc, city["scan_cars"], city["ds"], city["normals"], city["prior"], MAX_DIST, ITERS, kind, k)
    icp = make_icp(api, ctx, gmap, kind, k)
    for order in ("as_given", "cell"):
        icp.set_query_order(order)
        r = align_one(icp, city["scan_cars"], city["prior"])
        assert r["iterations"] == ref["iterations"] == ITERS and r["n_corr"] == ref["n_corr"] and r["flags"] == 0
        assert abs(r["fitness"] - ref["fitness"]) < 1e-12 and abs(r["rmse"] - ref["rmse"]) < 1e-7   # unweighted
        dt, dr = synth.pose_error(r["T64"], ref["T"])
        assert dt < 1e-8 and dr < 1e-9, (kind, order, dt, dr)


@pytest.mark.gpu
def test_gpu_single_launch_equals_launch_list(api, ctx, city, gmap):
    fused = make_icp(api, ctx, gmap, "tukey", 0.1, fused=True)
    listed = make_icp(api, ctx, gmap, "tukey", 0.1, fused=False)
    n0 = fused.fused_count()
    a = align_one(fused, city["scan_cars"], city["prior"])
    assert fused.fused_count() == n0 + 1                               # the single-launch robust kernel ran
    b = align_one(listed, city["scan_cars"], city["prior"])
    assert listed.fused_count() == 0
    bitwise(a, b)
    assert a["n_corr"] == b["n_corr"] and a["iterations"] == b["iterations"]


@pytest.mark.gpu
def test_gpu_batched_wide_scans_no_freeze(api, ctx, synth, city, gmap):
    priors = np.stack([synth.make_T((0.02 * s, -0.015 * s, 0.01), (0.05 * s, -0.03 * s, 0.1 * s)) @ city["prior"] for s in range(8)])
    icp = make_icp(api, ctx, gmap, "tukey", 0.1)
    icp.set_wide_scan_points(1024)                                     # two queries per lane: the launch list that may freeze
    icp.set_freeze("always")
    icp.set_source_batch(np.stack([city["scan_cars"]] * 8))
    icp.set_initial_batch(priors)
    got = icp.align_batch("p2plane")
    assert icp.freeze_stats() == {"froze": 0, "thawed": 0, "failed": 0, "active_queries": 0, "frozen_at_end": 0}
    one = make_icp(api, ctx, gmap, "tukey", 0.1)
    for s in range(8):
        r = align_one(one, city["scan_cars"], priors[s])
        assert got[s]["n_corr"] == r["n_corr"] and got[s]["iterations"] == r["iterations"]
        dt, dr = synth.pose_error(got[s]["T64"], r["T64"])
        assert dt < 1e-9 and dr < 1e-9, (s, dt, dr)


@pytest.mark.gpu
def test_gpu_none_restores_default_and_other_modes_ignore_it(api, ctx, city, gmap):
    fresh = make_icp(api, ctx, gmap)
    used = make_icp(api, ctx, gmap, "gm", 0.1)
    scan, prior = city["scan_cars"], city["prior"]
    robust = align_one(used, scan, prior)
    plain = align_one(fresh, scan, prior)
    assert not np.array_equal(robust["T64"], plain["T64"])
    for mode in ("o3d_p2p", "ref_cpp"):                               # ignored by the point-to-point modes, bit for bit
        bitwise(align_one(used, scan, prior, mode), align_one(fresh, scan, prior, mode))
    used.set_robust_kernel("none")
    bitwise(align_one(used, scan, prior), plain)
    used.set_fused(False)
    fresh.set_fused(False)
    bitwise(align_one(used, scan, prior), align_one(fresh, scan, prior))


@pytest.mark.gpu
def test_gpu_sharded_group_equals_unsharded(api, ctx, synth, city):
    from slam_sensor_fusion_amd import sharded
    ds = city["ds"]
    scans = np.stack([city["scan_cars"]] * 2)
    inits = np.stack([city["prior"], synth.make_T((0.03, 0.02, 0.0), (0.0, 0.0, 0.2)) @ city["prior"]])
    ref_icp = make_icp(api, ctx, make_map(api, ctx, city), "tukey", 0.1)
    ref_icp.set_source_batch(scans)
    ref_icp.set_initial_batch(inits)
    ref = ref_icp.align_batch("p2plane")
    edges = sharded.slab_edges(ds[:, 0], 3)
    members = []
    for r in range(3):
        keep = sharded.slab_select(ds, edges, r, halo=MAX_DIST + 0.3 + 0.25)
        icp = make_icp(api, ctx, make_map(api, ctx, city, keep), "tukey", 0.1)
        icp.set_source_batch(scans)
        icp.set_initial_batch(inits)
        icp.set_shard(float(max(edges[r], -1e30)), float(min(edges[r + 1], 1e30)))
        members.append(icp)
    res, _ = api.align_group(members, "p2plane")
    for b in range(2):
        assert res[b]["iterations"] == ref[b]["iterations"] == ITERS and res[b]["n_corr"] == ref[b]["n_corr"]
        dt, dr = synth.pose_error(res[b]["T64"], ref[b]["T64"])
        assert dt < 1e-9 and dr < 1e-9, (b, dt, dr)


@pytest.mark.gpu
def test_gpu_graph_recaptured_when_scale_changes(api, ctx, city, gmap):
    icp = make_icp(api, ctx, gmap, "tukey", 0.1, fused=False)
    icp.use_graph(True)
    align_one(icp, city["scan_cars"], city["prior"])
    c1, _ = icp.graph_counts()
    icp.set_robust_kernel("tukey", 0.05)
    r = icp.align("p2plane")
    c2, _ = icp.graph_counts()
    assert c1 == 1 and c2 == 2                                         # the key holds the kind and the scale
    fresh = make_icp(api, ctx, gmap, "tukey", 0.05, fused=False)
    bitwise(r, align_one(fresh, city["scan_cars"], city["prior"]))
    r2 = icp.align("p2plane")                                          # unchanged setting: replayed
    assert icp.graph_counts() == (2, 3)
    bitwise(r2, r)


@pytest.mark.gpu
def test_gpu_pipelined_alignments_keep_their_own_setting(api, ctx, synth, city, gmap):
    scans = np.stack([city["scan_cars"]] * 2)
    inits = np.stack([city["prior"], synth.make_T((0.03, 0.02, 0.0), (0.0, 0.0, 0.2)) @ city["prior"]])

    def alone(kind, k):
        icp = make_icp(api, ctx, gmap, kind, k, fused=False)
        icp.set_source_batch(scans)
        icp.set_initial_batch(inits)
        return icp.align_batch("p2plane")

    icp = make_icp(api, ctx, gmap, "tukey", 0.1, fused=False)
    icp.set_source_batch(scans)
    icp.set_initial_batch(inits)
    icp.align_batch_async("p2plane")
    icp.set_robust_kernel("cauchy", 0.2)
    icp.align_batch_async("p2plane")                                   # beside the first one, on the other lane
    first, second = icp.fetch_previous(), icp.fetch_results()
    for got, want in ((first, alone("tukey", 0.1)), (second, alone("cauchy", 0.2))):
        for g, w in zip(got, want):
            bitwise(g, w)
    assert not np.array_equal(first[0]["T64"], second[0]["T64"])


@pytest.mark.gpu
def test_gpu_tile_search_declines_under_a_robust_kernel(api, ctx, city, gmap):
    def run(kind, k, tile):
        icp = make_icp(api, ctx, gmap, kind, k)
        icp.set_wide_scan_points(1024)                                 # tile search takes wide scans only
        icp.set_query_order("cell")
        icp.set_tile_search("always" if tile else "off")
        icp.set_source_batch(np.stack([city["scan_cars"]] * 2))
        icp.set_initial_batch(np.stack([city["prior"]] * 2))
        return icp.align_batch("p2plane"), icp.tile_info()["on"]

    assert run("none", None, True)[1]                                  # the configuration takes the tile path without a kernel
    with_tile, on = run("tukey", 0.1, True)
    assert not on
    without, _ = run("tukey", 0.1, False)
    for g, w in zip(with_tile, without):
        bitwise(g, w)


@pytest.mark.gpu
def test_gpu_bad_arguments_keep_the_setting(api, ctx, city, gmap):
    icp = make_icp(api, ctx, gmap, "huber", 0.05)
    want = align_one(icp, city["scan_cars"], city["prior"])
    lib = api.load_library()
    for kind, k in ((5, 0.1), (-1, 0.1), (3, 0.0), (3, -1.0), (3, float("nan")), (3, float("inf"))):
        assert lib.sf_icp_set_robust_kernel(icp.h, C.c_int(kind), C.c_double(k)) == SF_ERR_INVALID, (kind, k)
    with pytest.raises(api.SlamFusionError):
        icp.set_robust_kernel("tukey")                                 # no scale
    with pytest.raises(KeyError):
        icp.set_robust_kernel("welsch", 0.1)
    bitwise(align_one(icp, city["scan_cars"], city["prior"]), want)
    assert lib.sf_icp_set_robust_kernel(icp.h, C.c_int(0), C.c_double(float("nan"))) == 0   # NONE takes no scale


@pytest.mark.gpu
def test_gpu_dynamic_object_scene(api, ctx, synth, city, gmap):
    plain = align_one(make_icp(api, ctx, gmap), city["scan_cars"], city["prior"])
    tukey = align_one(make_icp(api, ctx, gmap, "tukey", 0.1), city["scan_cars"], city["prior"])
    check_dynamic_bounds(synth, plain["T64"], tukey["T64"], city["T_true"])
