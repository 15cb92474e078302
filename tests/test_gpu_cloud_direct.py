"""The kernels of csrc/sf_cloud.hip (PointCloud2 unpack, subsample, the radius / box / floor crops and the stream compaction behind
them, transform, append, the bounds reduction) and the two voxel filters of csrc/sf_voxel.hip, compared EXACTLY with the numpy
restatement of tests/cloud_ref_np.py at their edges.  tests/test_cloud_rule.py holds that restatement
against the CPU oracle on the same tables and asserts every case's precondition; here the preconditions are asserted again, so a
case cannot pass by missing its edge.  No tolerance anywhere: np.array_equal on indices, bit patterns for points that are only
moved; the one exception is the bounds, compared with == (fminf(-0.0, +0.0) may return either zero).  The compaction and the
bounds run through the hooks sf_test_compact / sf_test_cloud_minmax, which call the production functions.

The sizes sit on the boundaries of the kernels: 64 lanes, 256 flags per workgroup, 1024 block counts per round of k_scan_blocks
(262 144 points: from 262 145 on the scan carries a total into a second round and k_minmax_partial starts its grid-stride loop),
the sort's tile of 1024 keys."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import cloud_ref_np as ref

pytestmark = pytest.mark.gpu
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def moved(got, want):
    """points a kernel only copies: the same bit patterns, NaN payloads and signs of zero included"""
    return got.dtype == F32 and got.shape == want.shape and np.array_equal(bits(got), bits(want))


def same(a, b):
    """computed values: equal, NaN where the reference has NaN, and the same sign of zero"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def n_last_idx(cloud):
    """the count sf_cloud_last_indices reports; -1 when it has none to report (it refuses before it writes the count)"""
    n = C.c_int64(-1)
    cloud.lib.sf_cloud_last_indices(cloud.h, None, C.c_int64(0), C.byref(n))
    return n.value


def check_crop(cloud, want_pts, want_idx, what):
    assert len(cloud) == len(want_idx) == n_last_idx(cloud), (what, len(cloud), len(want_idx))
    assert np.array_equal(cloud.last_indices(), want_idx), (what, "indices")
    assert moved(cloud.download(), want_pts), (what, "points")


# ---------------------------------------------------------------- compaction
@pytest.mark.parametrize("n", ref.BOUNDARY_SIZES)
def test_compaction_every_pattern(api, ctx, n):
    p = ref.payload(n)
    cloud = api.Cloud(ctx)
    for name, flags in ref.compact_cases(n):
        cloud.upload(p)
        pts, idx = api.hook_compact(cloud, flags)
        want_pts, want_idx = ref.compact(p, flags)
        assert len(cloud) == len(want_idx) == n_last_idx(cloud) == np.count_nonzero(flags), (name, len(cloud), len(want_idx))
        assert idx.dtype == np.int32 and np.array_equal(idx, want_idx), (name, "indices")
        assert moved(pts, want_pts), (name, "points")
    cloud.close()


def test_compaction_twice_on_one_cloud_ignores_stale_block_counts(api, ctx):
    """the block counts and offsets of the first run stay in the context's scratch; the second run, with other flags, a smaller
    cloud or another cloud of the context, must not see them"""
    n = ref.BIG
    p = ref.payload(n)
    cloud, other = api.Cloud(ctx), api.Cloud(ctx)
    for name, m in (("all", n), ("bernoulli_0.01", n), ("all", n), ("bernoulli_0.5", ref.STRIDE + 1), ("none", n), ("last", n), ("bernoulli_0.99", 1025), ("alternating", n)):
        flags = ref.flag_pattern(name, m, seed=5)
        for c in (cloud, other) if m == n else (cloud,):
            c.upload(p[:m])
            pts, idx = api.hook_compact(c, flags)
            want_pts, want_idx = ref.compact(p[:m], flags)
            assert len(c) == len(want_idx) == n_last_idx(c), (name, m)
            assert np.array_equal(idx, want_idx) and moved(pts, want_pts), (name, m)
    kept = ref.flag_pattern("bernoulli_0.5", len(cloud), seed=6)        # and a compaction of the compacted cloud: indices into IT
    before = cloud.download()
    pts, idx = api.hook_compact(cloud, kept)
    assert np.array_equal(idx, np.nonzero(kept)[0]) and moved(pts, before[kept != 0])
    with pytest.raises(api.SlamFusionError):
        api.hook_compact(cloud, kept)                                    # the flags no longer fit the cloud: refused by the wrapper
    cloud.close()
    other.close()


# ---------------------------------------------------------------- bounds
def check_bounds(api, cloud, mn, mx, count, what):
    for enqueue in (False, True):
        g_mn, g_mx, g_cnt = api.hook_cloud_minmax(cloud, enqueue)
        assert g_cnt == count, (what, enqueue, g_cnt, count)
        assert g_mn.dtype == F32 and (g_mn == mn).all() and (g_mx == mx).all(), (what, enqueue, g_mn, g_mx, mn, mx)      # ==, not bits: either zero


@pytest.mark.parametrize("n", ref.BOUNDARY_SIZES)
def test_bounds_with_the_extremes_placed(api, ctx, n):
    cloud = api.Cloud(ctx)
    if n == 0:
        check_bounds(api, cloud, np.zeros(3), np.zeros(3), 0, "never uploaded")
    for rot in range(max(1, len(ref.minmax_positions(n)) if n else 1)):
        p, mn, mx = ref.minmax_placed(n, rot)
        cloud.upload(p)
        check_bounds(api, cloud, mn, mx, n, (n, rot))
    cloud.close()


@pytest.mark.parametrize("case", ref.minmax_special_cases(), ids=lambda c: c["name"])
def test_bounds_of_special_values(api, ctx, case):
    mn, mx, count = ref.minmax(case["p"])
    assert case["pre"]((mn, mx, count))
    cloud = api.Cloud(ctx, case["p"])
    check_bounds(api, cloud, mn, mx, count, case["name"])
    cloud.close()


def test_bounds_after_a_larger_cloud_ignore_stale_partials(api, ctx):
    """1024 partials of a large cloud stay in the context's scratch; a small cloud folds only its own"""
    cloud = api.Cloud(ctx)
    for n, rot in ((ref.BIG, 0), (257, 1), (0, 0), (ref.STRIDE + 1, 2), (1, 0)):
        p, mn, mx = ref.minmax_placed(n, rot, seed=9)
        cloud.upload(p)
        check_bounds(api, cloud, mn, mx, n, n)
    cloud.close()


# ---------------------------------------------------------------- radius crop
@pytest.mark.parametrize("order", ["sorted", "unsorted"])
@pytest.mark.parametrize("case", ref.radius_cases(), ids=lambda c: c["name"])
def test_radius_crop(api, ctx, case, order):
    p, c, r = case["p"], case["c"], case["radius"]
    assert case["pre"](p, c, r)
    want_pts, want_idx = ref.crop_radius(p, c, r, order == "sorted")
    cloud = api.Cloud(ctx, p).crop_radius(c, r, sorted=order == "sorted")
    check_crop(cloud, want_pts, want_idx, (case["name"], order))
    cloud.close()


# ---------------------------------------------------------------- boxes, floor, subsample
@pytest.mark.parametrize("case", ref.aabb_cases(), ids=lambda c: c["name"])
def test_aabb_crop(api, ctx, case):
    assert case["pre"](case)
    want_pts, want_idx = ref.crop_aabb(case["p"], case["lo"], case["hi"])
    cloud = api.Cloud(ctx, case["p"]).crop_aabb(case["lo"], case["hi"])
    check_crop(cloud, want_pts, want_idx, case["name"])
    cloud.close()


@pytest.mark.parametrize("case", ref.obb_cases(), ids=lambda c: c["name"])
def test_obb_crop(api, ctx, case):
    assert case["pre"](case)
    want_pts, want_idx = ref.crop_obb(case["p"], case["center"], case["R"], case["extent"])
    cloud = api.Cloud(ctx, case["p"]).crop_obb(case["center"], case["R"], case["extent"])
    check_crop(cloud, want_pts, want_idx, case["name"])
    cloud.close()


def test_floor_removal(api, ctx):
    p = ref.floor_case()
    want_pts, want_idx = ref.remove_floor(p)
    assert list(want_idx) == [2, 5, 7]                               # 1e-45 (a denormal), +inf, 1e-6; not -0.0, +0.0, -1e-45, NaN, -inf
    cloud = api.Cloud(ctx, p).remove_floor()
    check_crop(cloud, want_pts, want_idx, "floor")
    big = np.tile(p, (ref.STRIDE // len(p) + 3, 1))                  # the same eight values through every lane and a second scan round
    want_pts, want_idx = ref.remove_floor(big)
    check_crop(cloud.upload(big).remove_floor(), want_pts, want_idx, "floor, tiled")
    cloud.close()


@pytest.mark.parametrize("n,step", ref.SUBSAMPLE_CASES)
def test_subsample(api, ctx, n, step):
    p = ref.payload(n)
    want_pts, want_idx = ref.subsample(p, step)
    cloud = api.Cloud(ctx, p).subsample(step)
    assert len(cloud) == len(want_pts) and moved(cloud.download(), want_pts)
    if want_idx is None:                                              # fewer points than the step: untouched, and no indices to report
        assert n < step and n_last_idx(cloud) == -1
        with pytest.raises(api.SlamFusionError):
            cloud.last_indices()
    else:
        assert n_last_idx(cloud) == len(want_idx) and np.array_equal(cloud.last_indices(), want_idx)
    cloud.close()


# ---------------------------------------------------------------- transform
@pytest.mark.parametrize("case", ref.transform_cases(), ids=lambda c: c["name"])
def test_transform(api, ctx, case):
    want = ref.transform(case["p"], case["T"])
    cloud = api.Cloud(ctx, case["p"]).transform(case["T"])
    got = cloud.download()
    assert np.isnan(want).any() or case["name"] in ("n_1", "signed_zero_sums")
    assert same(got, want), (case["name"], got[~(bits(got) == bits(want)).all(1)], want[~(bits(got) == bits(want)).all(1)])
    cloud.close()


# ---------------------------------------------------------------- PointCloud2
@pytest.mark.parametrize("case", ref.pc2_cases(), ids=lambda c: c["name"])
def test_pointcloud2_unaligned_fields(api, ctx, case):
    dt = 8 if case["f64"] else 7
    fields = [SimpleNamespace(name=nm, offset=off, datatype=dt) for nm, off in zip("xyz", case["offsets"])]
    msg = SimpleNamespace(width=case["width"], height=case["height"], point_step=case["point_step"], row_step=case["row_step"], is_bigendian=False, data=case["data"],
                          fields=fields)
    want = ref.unpack_pc2(case["data"], case["width"], case["height"], case["point_step"], case["row_step"], case["offsets"], case["f64"])
    assert np.array_equal(bits(want), case["want_bits"])
    cloud = api.Cloud(ctx).from_pointcloud2(msg)
    got = cloud.download()
    assert len(cloud) == case["width"] * case["height"]
    bad = ~(bits(got) == case["want_bits"]).all(1)
    assert not bad.any(), (case["name"], np.nonzero(bad)[0][:5], bits(got)[bad][:5], case["want_bits"][bad][:5])
    cloud.close()


# ---------------------------------------------------------------- append
def test_append(api, ctx):
    rng = np.random.default_rng(53)
    parts = [rng.uniform(-9, 9, (n, 3)).astype(F32) for n in (1000, 5000, 257, 20000)]
    parts[1][7] = [np.nan, -0.0, np.inf]
    dst = api.Cloud(ctx)                                              # onto a cloud that never held anything
    dst.append(api.Cloud(ctx, parts[0]))
    assert len(dst) == 1000 and moved(dst.download(), parts[0])
    dst.append(api.Cloud(ctx, np.zeros((0, 3), F32)))                 # of an empty cloud
    dst.append(api.Cloud(ctx))
    assert len(dst) == 1000 and moved(dst.download(), parts[0])
    empty = api.Cloud(ctx, np.zeros((0, 3), F32))                     # onto an uploaded, empty cloud
    empty.append(dst)
    assert moved(empty.download(), parts[0])
    for k in (1, 2, 3):                                               # three appends in a row, each past the capacity: the content before the seam stays
        dst.append(api.Cloud(ctx, parts[k]))
        assert len(dst) == sum(len(q) for q in parts[:k + 1])
        assert moved(dst.download(), np.concatenate(parts[:k + 1])), k
    with pytest.raises(api.SlamFusionError):
        dst.append(dst)                                               # self-append
    assert moved(dst.download(), np.concatenate(parts))
    dst.crop_aabb([-5] * 3, [5] * 3)
    kept = dst.last_indices()
    assert n_last_idx(dst) == len(kept) == len(dst) > 0
    dst.append(api.Cloud(ctx, parts[2]))
    assert n_last_idx(dst) == -1 and len(dst) == len(kept) + 257      # the indices of the crop no longer describe the cloud
    with pytest.raises(api.SlamFusionError):
        dst.last_indices()
    assert moved(dst.download(), np.concatenate([np.concatenate(parts)[kept], parts[2]]))


# ---------------------------------------------------------------- voxel filters
@pytest.mark.parametrize("flavour", ["pcl", "pcl64"])
@pytest.mark.parametrize("case", ref.voxel_pcl_cases(), ids=lambda c: c["name"])
def test_voxel_pcl(api, ctx, case, flavour):
    assert case["pre"](case)
    wide = flavour == "pcl64"
    p, leaf = case["p"], case["leaf"]
    cen, ids, out_ids, status = ref.voxel_pcl(p, leaf, wide)
    assert status == (0 if wide else case["status"])
    cloud = api.Cloud(ctx, p)
    flags = cloud.voxel_downsample(leaf, flavour)
    got_ids = cloud.voxel_point_ids64() if wide else cloud.voxel_point_ids()
    got_out = cloud.voxel_out_ids64() if wide else cloud.voxel_out_ids()
    if status == -1:                                                  # "Leaf size is too small": output = input, no grid was built
        assert flags == api.SF_FLAG_VOXEL_OVERFLOW and moved(cloud.download(), p) and len(got_ids) == 0 and len(got_out) == 0
    elif len(out_ids) == 0:                                           # no finite point: empty output, no grid was built
        assert flags == 0 and len(cloud) == 0 and len(got_ids) == 0 and len(got_out) == 0
    else:
        assert flags == 0 and len(cloud) == len(out_ids)
        assert got_ids.dtype == ids.dtype and np.array_equal(got_ids, ids), (case["name"], "per-point ids")
        assert np.array_equal(got_out, out_ids), (case["name"], "per-voxel ids")
        assert same(cloud.download(), cen), (case["name"], "centroids")
    cloud.close()


@pytest.mark.parametrize("case", ref.voxel_o3d_cases(), ids=lambda c: c["name"])
def test_voxel_o3d(api, ctx, case):
    assert case["pre"](case)
    means, ijk, out_ijk = ref.voxel_o3d(case["p"], case["leaf"])
    cloud = api.Cloud(ctx, case["p"])
    assert cloud.voxel_downsample(case["leaf"], "o3d") == 0 and len(cloud) == len(means)
    assert np.array_equal(cloud.voxel_point_ids().reshape(-1, 3), ijk), (case["name"], "per-point ijk")
    assert np.array_equal(cloud.voxel_out_ids().reshape(-1, 3), out_ijk), (case["name"], "per-voxel ijk")
    assert np.array_equal(cloud.voxel_out_means_f64(), means), (case["name"], "float64 means")
    assert same(cloud.download(), means.astype(F32)), (case["name"], "float32 means")
    cloud.close()
