"""The map-growth path against numpy, bit for bit, at the edges of its own kernels: sf_cloud_voxel_merge (csrc/sf_voxel.hip: the
64-wide coarse table of k_merge_copy, the wave-boundary re-read of k_merge_old_keys, the serial sums of k_merge_groups, the carried
bounds) against the plain voxel filter of the concatenation, and sf_map_patch / sf_map_build (csrc/sf_map.hip: the 256-entry blocks
and 32-bit bitmap words of the patch, the candidate ranges of k_patch_ranges, the clamp to the upper face) against the index
sf_map_build documents, computed from the merged cloud alone.  The rules and the case tables are tests/growth_ref_np.py, held
against the CPU oracle and against their own preconditions by tests/test_growth_rule.py; nothing here compares the library with
itself but gap_eps.  Which way the device went -- merged or not, patched or built and why -- is asserted against the prediction in
every case, so that a silent fall-back cannot stand in for the path a case is there for.  The largest cloud is 4097 + 257 points."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import growth_ref_np as ref

pytestmark = pytest.mark.gpu
F32 = np.float32


@contextlib.contextmanager
def _merge_every_size(api):
    """maps below sf_cloud_voxel_merge_min_points take the full path by default: merge them here, and put the threshold back"""
    prev = api.voxel_merge_min_points(0)
    try:
        yield
    finally:
        api.voxel_merge_min_points(prev)


@contextlib.contextmanager
def _closing():
    made = []

    def keep(obj):
        made.append(obj)
        return obj
    try:
        yield keep
    finally:
        for obj in reversed(made):
            obj.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _merge_step(api, keep, ctx, dev, host, pend, leaf, name):
    """one sf_cloud_voxel_merge on the device and by the rule: the way it went, the status, the cloud.  -> the merged cloud (host)"""
    st, merged = dev.voxel_merge(keep(api.Cloud(ctx, pend)), leaf)
    want, (cen, _, _, ref_st) = ref.expect_merged(host, pend, leaf), ref.merge(host, pend, leaf)
    assert merged == want, (name, "merged" if merged else "fell back")
    assert st == (api.SF_FLAG_VOXEL_OVERFLOW if ref_st == -1 else 0), (name, st)
    got = dev.download()
    assert got.shape == cen.shape and np.array_equal(got, cen), (name, got.shape, cen.shape, int(np.sum((got != cen).any(1))) if got.shape == cen.shape else -1)
    return cen


def _assert_index(api, keep, ctx, mp, host, cell, lattice, name):
    """the index on the device against growth_ref_np.index of the same cloud: pts4, cell_start and org bit for bit, dims and inv_h as
    values, gap_eps against a fresh build"""
    org, dims = ref.geometry(host, cell, lattice)
    want, got = ref.index(host, org, cell, dims), mp.index()
    h, got_dims = mp.cell_size()
    assert h == F32(cell) and tuple(got_dims) == want["dims"], (name, got_dims, want["dims"])
    assert np.array_equal(_bits(got["org"]), _bits(want["org"])) and F32(got["inv_h"]) == want["inv_h"], (name, got["org"], want["org"])
    assert got["pts4"].shape == want["pts4"].shape and got["cell_start"].shape == want["cell_start"].shape, name
    wrong = np.nonzero((_bits(got["pts4"]) != _bits(want["pts4"])).any(1))[0]
    assert len(wrong) == 0, (name, "pts4", len(wrong), wrong[:8])
    wrong = np.nonzero(got["cell_start"] != want["cell_start"])[0]
    assert len(wrong) == 0, (name, "cell_start", len(wrong), wrong[:8])
    fresh = keep(api.Map(ctx)).set_origin_lattice(lattice).build(keep(api.Cloud(ctx, host)), cell)
    assert got["gap_eps"] == fresh.index()["gap_eps"] and len(mp) == len(host), name


# ------------------------------------------------------------------ the merge
@pytest.mark.parametrize("case", ref.merge_cases(), ids=lambda c: c["name"])
def test_merge_equals_the_filter_of_the_concatenation(api, ctx, case):
    """sizes around the 64-wide coarse table, the wave and the block; placements (no fresh voxel, all in front, all behind, ranks 63 /
    64 / 65 / 127 / 128 / n, 200 of one rank, 257 points in one voxel, copies, faces, non-finite points); the bounds moved on each of
    the six sides; a centroid that rounding has pushed across a voxel face (merged while the ids still ascend, the full path when two
    are equal); the other fall-backs; three steps on one cloud with the bounds carried from step to step"""
    with _merge_every_size(api), _closing() as keep:
        dev, host = keep(api.Cloud(ctx, case["old"])), case["old"]
        for k, pend in enumerate(case["steps"]):
            host = _merge_step(api, keep, ctx, dev, host, pend, case["leaf"], (case["name"], k))


# ------------------------------------------------------------------ the patch
def _patch_params():
    out = []
    for lattice in ref.LATTICES:
        out += [(c, lattice) for c in ref.patch_subset() + ref.replaced_position_cases(lattice) + ref.clamped_cases(lattice)]
    out += [(c, c["lattice"]) for c in ref.origin_cases()]
    return out


@pytest.mark.parametrize("case,lattice", _patch_params(), ids=lambda v: v["name"] if isinstance(v, dict) else "L%d" % v)
def test_patch_equals_the_index_of_the_merged_cloud(api, ctx, case, lattice):
    """merge, then patch, step by step: sf_map_patch reports the predicted SF_PATCH_* code and leaves the index of the merged cloud.
    Beyond the merge cases: the replaced entries at sorted positions 0, 31, 32, 255, 256 and the last, a whole block of 256, none; a
    point the old grid clamped to its upper face, with growth that frees it (SF_PATCH_CLAMPED_POINT), growth that does not (1), and
    itself replaced (1, or SF_PATCH_CLAMPED_POINT where k_patch_groups gives up: the index is the reference's either way), the
    last with 0 to 7 more entries in front so that every alignment of the binary searches over the old entries is walked; a centroid
    below the origin without and with an origin lattice.

    The replaced clamped point is the case that found a defect: by its new cell the entry sorts behind the three entries that follow
    it in its old cell, k_patch_new's search stopped at it and put the centroid in front of them (two rows of pts4 out of order, code 1).
    k_patch_groups now hands such a merge to the build."""
    with _merge_every_size(api), _closing() as keep:
        dev, host = keep(api.Cloud(ctx, case["old"])), case["old"]
        mp = keep(api.Map(ctx)).set_origin_lattice(lattice).build(dev, case["cell"])
        _assert_index(api, keep, ctx, mp, host, case["cell"], lattice, (case["name"], "build"))
        for k, pend in enumerate(case["steps"]):
            code = ref.expect_patch(host, pend, case["leaf"], case["cell"], lattice)
            accepted = np.atleast_1d(case["want"][k]) if "want" in case else [code]
            assert code in accepted
            host = _merge_step(api, keep, ctx, dev, host, pend, case["leaf"], (case["name"], k))
            patched = mp.patch(dev)
            assert mp.last_patch in accepted and patched == (mp.last_patch == 1), (case["name"], k, lattice, mp.last_patch, list(accepted))
            _assert_index(api, keep, ctx, mp, host, case["cell"], lattice, (case["name"], k))


def test_patch_past_2_32_cells_takes_the_build(api, ctx):
    """An explicit cell of 0.05 m on a sparse map of 64 points over 50 m x 50 m x 10 m (2e8 cells) that grows to 235 m x 235 m: 4.4e9
    cells, past the 32-bit cell ids of the patch.  SF_PATCH_LIMITS, and the index is the build's: the points in (64-bit cell, id)
    order, origin, dims and inv_h against numpy; the table of 4.4e9 entries (17.7 GB) stays on the device."""
    case = ref.limits_case()
    with _merge_every_size(api), _closing() as keep:
        dev, host = keep(api.Cloud(ctx, case["old"])), case["old"]
        mp = keep(api.Map(ctx)).build(dev, case["cell"])
        for k, pend in enumerate([None] + case["steps"]):
            if pend is not None:
                host = _merge_step(api, keep, ctx, dev, host, pend, case["leaf"], case["name"])
                assert not mp.patch(dev) and mp.last_patch == ref.SF_PATCH_LIMITS == case["want"][0]
            org, dims = ref.geometry(host, case["cell"], 0)
            want = ref.index(host, org, case["cell"], dims, table=False)
            n, nc, g_org, inv_h = C.c_int64(), C.c_int64(), (C.c_float * 3)(), C.c_float()
            assert mp.lib.sf_map_index_info(mp.h, C.byref(n), C.byref(nc), g_org, C.byref(inv_h), None) == 0
            pts4 = np.empty((n.value, 4), F32)
            assert mp.lib.sf_map_download_index(mp.h, pts4.ctypes.data_as(C.c_void_p), C.c_int64(len(pts4)), None, C.c_int64(0)) == 0
            assert tuple(mp.cell_size()[1]) == want["dims"] and nc.value == dims[0] * dims[1] * dims[2] and (nc.value >= 2 ** 32) == (k == 1)
            assert np.array_equal(_bits(np.array(list(g_org), F32)), _bits(want["org"])) and F32(inv_h.value) == want["inv_h"]
            assert pts4.shape == want["pts4"].shape and np.array_equal(_bits(pts4), _bits(want["pts4"]))


# ------------------------------------------------------------------ the build
@pytest.mark.parametrize("lattice", ref.LATTICES, ids=lambda v: "L%d" % v)
@pytest.mark.parametrize("case", ref.build_cases(), ids=lambda c: c["name"])
def test_build_of_tiny_maps(api, ctx, case, lattice):
    """sf_map_build at 0, 1, 2, 63, 64, 65 and 257 points, all points identical, all in one cell, trailing non-finite rows (not indexed)"""
    with _closing() as keep:
        mp = keep(api.Map(ctx)).set_origin_lattice(lattice).build(keep(api.Cloud(ctx, case["p"])), ref.CELL)
        org, dims = ref.geometry(case["p"], ref.CELL, lattice)
        want, got = ref.index(case["p"], org, ref.CELL, dims), mp.index()
        assert tuple(mp.cell_size()[1]) == want["dims"] and F32(got["inv_h"]) == want["inv_h"] and np.array_equal(_bits(got["org"]), _bits(want["org"]))
        assert got["pts4"].shape == want["pts4"].shape and np.array_equal(_bits(got["pts4"]), _bits(want["pts4"]))
        assert np.array_equal(got["cell_start"], want["cell_start"])
        assert len(mp) == len(case["p"])
