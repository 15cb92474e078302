"""tests/growth_ref_np.py -- the numpy restatement tests/test_gpu_growth_direct.py compares sf_cloud_voxel_merge, sf_map_patch and
sf_map_build with -- pinned without a device: the merge rule against the CPU oracle on every generated case, the index rule
against the invariants of the cell table, the geometry and the predicted SF_PATCH_* codes against hand-made examples, and every
constructed edge case against the property it is named after (the generators assert their own preconditions while they build
the tables: a generator that cannot construct its case raises).  Every comparison is exact."""
import os
import re

import numpy as np
import pytest

import cloud_ref_np as cloud
import growth_ref_np as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _steps(case):
    """(map before the step, pending) for every step of a case, the map carried along with the rule itself"""
    host = case["old"]
    for pend in case["steps"]:
        yield host, pend
        host = ref.merge(host, pend, case["leaf"])[0]


@pytest.mark.parametrize("case", ref.merge_cases() + ref.patch_only_cases(), ids=lambda c: c["name"])
def test_merge_rule_is_the_oracles_filter_of_the_concatenation(orc, case):
    for host, pend in _steps(case):
        cen, _, _, st = ref.merge(host, pend, case["leaf"])
        o_cen, _, _, o_st = orc.voxel_pcl(np.concatenate([host, pend]), case["leaf"])
        assert st == (0 if o_st == 0 else -1)
        if st == 0:                                  # (on overflow the oracle's output buffer is not the rule's business: the filter returns its input)
            assert cen.shape == o_cen.shape and np.array_equal(cen.view(np.uint32), o_cen.view(np.uint32))
        else:
            assert np.array_equal(cen.view(np.uint32), np.concatenate([host, pend]).view(np.uint32))


def test_the_case_tables_hold_what_the_issue_lists():
    names = [c["name"] for c in ref.merge_cases()]
    assert len(names) == len(set(names)) and len(set(c["name"] for c in ref.patch_only_cases())) == len(ref.patch_only_cases()) == 2 * (3 + 10) + 3
    assert [(c["n_old"], c["m"]) for c in ref.size_cases()] == [(n, m) for n in (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4097) for m in (1, 63, 64, 65, 257)]
    for c in ref.size_cases():
        assert len(c["old"]) == c["n_old"] and len(c["steps"][0]) == c["m"]
    assert max(len(c["old"]) + sum(len(s) for s in c["steps"]) for c in ref.merge_cases()) <= 4097 + 257
    assert sum(n.endswith("_n200") for n in names) == sum(n.endswith("_n4097") for n in names) == 12
    assert [n for n in names if n.startswith("beyond_")] == ["beyond_" + s + d for d in "xyz" for s in "-+"]
    assert sum("falls_back" in n for n in names) == 7 and all(len(c["steps"]) == 3 for c in ref.chain_cases())
    subset = [c["name"] for c in ref.patch_subset()]
    assert sorted(set(c["n_old"] for c in ref.patch_subset() if "n_old" in c)) == [1, 64, 65, 255, 256, 257, 4097]
    assert "centroid_across_a_face_neighbour_empty" in subset and "centroid_across_a_face_neighbour_occupied_falls_back" not in subset


def test_the_predicted_way_of_every_case():
    """every case takes the merge path except the ones named after their fall-back, step by step"""
    for case in ref.merge_cases():
        for host, pend in _steps(case):
            assert ref.expect_merged(host, pend, case["leaf"]) == ("falls_back" not in case["name"]), case["name"]


def test_expect_merged_conditions_one_by_one():
    old, rows = ref.old_map(64, ref.FACES, 9)
    pend = ref.points_in([(5, 5, 5)], np.random.default_rng(0))
    assert ref.expect_merged(old, pend, 0.1)
    assert not ref.expect_merged(old[:0], pend, 0.1) and not ref.expect_merged(old, pend[:0], 0.1)
    bad = old.copy()
    bad[3, 1] = np.inf
    assert not ref.expect_merged(bad, pend, 0.1)
    assert not ref.expect_merged(old, np.array([[np.nan, 0, 0]], F32), 0.1) and ref.expect_merged(old, np.array([[np.nan, 0, 0], [0, 0, 0]], F32), 0.1)
    assert not ref.expect_merged(old, np.array([[500.0, 500.0, 500.0]], F32), 0.1)           # 5 000^3 voxels
    assert not ref.expect_merged(old[::-1], pend, 0.1) and not ref.expect_merged(np.concatenate([old[:5], old[4:]]), pend, 0.1)   # descending; one id twice


def test_the_face_crossing_centroid_is_the_issues():
    """leaf 0.1, x = -0.8000001 three times: the float32 centroid is -0.8, on the face, hence keyed into the next voxel"""
    x = np.nextafter(F32(-8) * F32(0.1), F32(-np.inf))
    p = np.array([[x, 0.05, 0.05]] * 3 + [[-1.95, -1.95, -1.95], [1.95, 1.95, 1.95]], F32)
    cen, pt_ids, out_ids, st = cloud.voxel_pcl(p, 0.1)
    assert F32(-0.8000001) == x and cen[1, 0] == F32(-0.8) and out_ids[1] == pt_ids[0]
    assert cloud.voxel_pcl_keys(cen, 0.1)[0][1] == pt_ids[0] + 1
    a, b = ref.crossing_cases()
    for c, occupied in ((a, False), (b, True)):
        ids = cloud.voxel_pcl_keys(c["old"], 0.1)[0]
        assert (np.sum(np.diff(ids) == 0) == 1) == occupied and np.all(np.diff(ids) >= 0)
        assert ref.expect_merged(c["old"], c["steps"][0], 0.1) == (not occupied)


def test_index_rule_has_the_invariants_of_the_cell_table():
    """as tests/test_gpu_map_growth.py::test_cell_table_is_the_lower_bound_of_the_sorted_keys asks of the device: every finite point once,
    (cell, id) order, cell_start the lower bound of the sorted keys -- and cell_start against a plain count, point by point"""
    rng = np.random.default_rng(3)
    pts = rng.uniform(-3, 5, (3000, 3)).astype(F32)
    pts[[5, 2999]] = [[np.nan, 0, 0], [0, 0, np.inf]]
    for lattice in ref.LATTICES:
        org, dims = ref.geometry(pts, 0.25, lattice)
        ix = ref.index(pts, org, 0.25, dims)
        cells = dims[0] * dims[1] * dims[2]
        p4 = ix["pts4"]
        ids = p4[:, 3].copy().view(np.uint32)
        fin = np.nonzero(np.isfinite(pts).all(1))[0]
        assert len(p4) == 2998 and np.array_equal(np.sort(ids), fin) and np.array_equal(p4[:, :3], pts[ids])
        c = [np.clip(np.floor((p4[:, d] - org[d]) * F32(4)), 0, dims[d] - 1).astype(np.int64) for d in range(3)]
        keys = (c[2] * dims[1] + c[1]) * dims[0] + c[0]
        assert np.array_equal(keys, ix["keys"]) and ix["inv_h"] == F32(4)
        assert np.all(np.diff(keys) >= 0) and np.all((np.diff(keys) > 0) | (np.diff(ids.astype(np.int64)) > 0))
        count = np.bincount(keys, minlength=cells)
        assert len(ix["cell_start"]) == cells + 1 and ix["cell_start"].dtype == np.uint32
        assert np.array_equal(ix["cell_start"].astype(np.int64), np.r_[0, np.cumsum(count)])
        assert ref.index(pts, org, 0.25, dims, table=False)["cell_start"] is None
        mn, mx, _ = cloud.minmax(pts)
        if lattice:
            assert np.array_equal(org, (np.floor(mn.astype(np.float64) / 16.0) * 16.0).astype(F32)) and np.all(org <= mn) and np.all(org == [-16, -16, -16])
        else:
            assert np.array_equal(org, mn)
        assert all(org[d] + 0.25 * (dims[d] - 1) <= mx[d] < org[d] + 0.25 * dims[d] for d in range(3))
    org, dims = ref.geometry(np.zeros((0, 3), F32), 0.25, 64)
    assert not org.any() and dims == (1, 1, 1) and np.array_equal(ref.index(np.zeros((0, 3), F32), org, 0.25, dims)["cell_start"], [0, 0])


def test_the_patch_codes_are_the_headers():
    text = open(os.path.join(ROOT, "include", "slamfusion.h")).read()
    got = {name: int(val) for name, val in re.findall(r"#define (SF_PATCH_\w+)\s+\(?(-?\d+)\)?", text)}
    for name in ("SF_PATCH_NO_MERGE", "SF_PATCH_ORIGIN_MOVED", "SF_PATCH_LIMITS", "SF_PATCH_CLAMPED_POINT"):
        assert got[name] == getattr(ref, name), name
    assert ref.PATCHED == 1 and all(v <= 0 for v in got.values())


@pytest.mark.parametrize("lattice", ref.LATTICES)
def test_the_clamped_point_has_fc_equal_dim(lattice):
    """the point with the largest x lies below the face of the last cell in float64 -- dim is counted there -- and on it in the float32
    of k_cell_keys; growth beyond +x frees it, growth beyond +y does not; re-observed by a copy of itself it is replaced"""
    cases = ref.clamped_cases(lattice)
    assert len(cases) == 10
    for c in cases:
        old, pend = c["old"], c["steps"][0]
        org, dims = ref.geometry(old, c["cell"], lattice)
        at = int(np.argmax(old[:, 0]))
        fc = ref.raw_cells(old, org, c["cell"])
        assert fc[at, 0] == dims[0] and (float(old[at, 0]) - float(org[0])) / 0.25 < dims[0]
        assert np.sum(fc >= np.array(dims)) == 1                         # the only one
        dims1 = ref.geometry(ref.merge(old, pend, 0.1)[0], c["cell"], lattice)[1]
        code = ref.expect_patch(old, pend, 0.1, c["cell"], lattice)
        if "+y" in c["name"]:
            assert dims1[0] == dims[0] and dims1[1] > dims[1] and code == 1 and c["want"] == [1]
        elif "+x" in c["name"]:
            assert dims1[0] > dims[0] and code == ref.SF_PATCH_CLAMPED_POINT and c["want"] == [code]
        else:
            assert dims1[0] > dims[0] and code == 1 and c["want"] == [(1, ref.SF_PATCH_CLAMPED_POINT)]
            assert (pend == old[at]).all(1).sum() == 1
            # the replaced entry lies in front of three entries of its OLD cell and, by its new cell, behind them: the order k_patch_new searches
            k0 = ref.index(old, org, c["cell"], dims)
            pos = int(np.nonzero(k0["pts4"][:, 3].view(np.uint32) == at)[0][0])
            assert np.all(k0["keys"][pos:pos + 4] == k0["keys"][pos]) and (pos + 4 == len(old) or k0["keys"][pos + 4] > k0["keys"][pos])


def test_the_other_patch_cases_have_their_property():
    for lattice in ref.LATTICES:
        for c in ref.replaced_position_cases(lattice):
            assert ref.expect_patch(c["old"], c["steps"][0], 0.1, 0.25, lattice) == 1
    lo, hi = ref.origin_cases()
    assert np.array_equal(lo["old"], hi["old"]) and lo["lattice"] == 0 and hi["lattice"] == 64
    merged = ref.merge(lo["old"], lo["steps"][0], 0.1)[0]
    assert merged[:, 0].min() < lo["old"][:, 0].min()
    assert ref.geometry(merged, 0.25, 0)[0][0] < ref.geometry(lo["old"], 0.25, 0)[0][0] and ref.geometry(merged, 0.25, 64)[0][0] == ref.geometry(lo["old"], 0.25, 64)[0][0] == -16
    lim = ref.limits_case()
    assert ref.expect_patch(lim["old"], lim["steps"][0], 0.1, lim["cell"], 0) == ref.SF_PATCH_LIMITS and ref.expect_merged(lim["old"], lim["steps"][0], 0.1)
    # the codes of the subset: a patch wherever the origin stays; the low sides move it without a lattice, the one-point and two-point
    # maps whenever their own points are re-observed; the overflow has no merge
    for lattice in ref.LATTICES:
        for c in ref.patch_subset():
            host = c["old"]
            for pend in c["steps"]:
                code = ref.expect_patch(host, pend, c["leaf"], c["cell"], lattice)
                if "falls_back" in c["name"]:
                    assert code == ref.SF_PATCH_NO_MERGE
                elif lattice == 64 or not (c["name"].startswith(("beyond_-", "n1_", "n2_")) or "chain" in c["name"]):
                    assert code == 1, (c["name"], lattice, code)
                else:
                    assert code in (1, ref.SF_PATCH_ORIGIN_MOVED), (c["name"], code)
                host = ref.merge(host, pend, c["leaf"])[0]


def test_the_build_cases():
    cases = {c["name"]: c["p"] for c in ref.build_cases()}
    assert [len(cases["n%d" % n]) for n in (0, 1, 2, 63, 64, 65, 257)] == [0, 1, 2, 63, 64, 65, 257]
    assert len(np.unique(cases["all_points_identical"], axis=0)) == 1
    for lattice in ref.LATTICES:
        p = cases["all_points_in_one_cell"]
        org, dims = ref.geometry(p, 0.25, lattice)
        ix = ref.index(p, org, 0.25, dims)
        assert len(np.unique(ix["keys"])) == 1 and np.array_equal(ix["pts4"][:, 3].view(np.uint32), np.arange(len(p)))
    p = cases["last_rows_non_finite"]
    assert np.isfinite(p[:126]).all() and not np.isfinite(p[126:]).all(1).any()
