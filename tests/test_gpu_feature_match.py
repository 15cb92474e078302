"""sf_features and sf_features_match on the device against the numpy restatement (tests/fpfh_ref_np.py): idx, dist2,
second2, pairs and the stats bit for bit -- the reference loops over k on float32 arrays, which is the device's arithmetic.
The kernel stages 64 candidate rows at a time and splits the candidates into slices of at least 256 rows (at most 64 slices), so the
candidate counts straddle 64, 256 and several slices; the query counts straddle the wave and the 256-lane block."""
import ctypes as C

import numpy as np
import pytest

import fpfh_ref_np as ref

pytestmark = pytest.mark.gpu

N_SRC = (1, 63, 64, 65, 255, 257, 1000)
N_DST = (1, 63, 65, 255, 256, 257, 5000)


def world():
    """dst: 5000 rows, the last 600 repeating rows below 4000 (so the copies of a row lie in different slices) and rows 40 .. 59
    repeating rows 0 .. 19 (inside the first tile); src: 1000 rows, a third exact copies of dst rows, a third noisy copies, a third
    unrelated; then flags and non-finite values take a tenth of either side out.  clean: dst before anything was taken out."""
    if not hasattr(world, "cache"):
        rng = np.random.default_rng(11)
        dst = ref.descriptor_rows(5000, 5)
        dst[40:60] = dst[:20]
        dst[4400:] = dst[rng.integers(0, 4000, 600)]
        clean = dst.copy()
        pick = rng.integers(0, 5000, 1000)
        src = dst[pick].copy()
        src[333:666] += rng.normal(0, 0.5, (333, 33)).astype(np.float32)
        src[666:] = ref.descriptor_rows(334, 6)
        src[:40] = dst[rng.integers(0, 60, 40)]                      # matches among the first rows, whatever the candidate count
        vs, vd = rng.random(1000) > 0.08, rng.random(5000) > 0.08
        src[rng.integers(0, 1000, 20), rng.integers(0, 33, 20)] = np.nan
        dst[rng.integers(0, 5000, 60), rng.integers(0, 33, 60)] = np.inf
        world.cache = (src, vs, dst, vd, clean)
    return world.cache


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check(api, ctx, src, vs, dst, vd, ratio, mutual, max_pairs=None):
    fs, fd = api.Features(ctx, src, vs), api.Features(ctx, dst, vd)
    got = fs.match(fd, ratio=ratio, mutual=mutual, max_pairs=max_pairs)
    want = ref.match(src, vs, dst, vd, ratio, mutual, max_pairs)
    tag = (len(src), len(dst), ratio, mutual)
    assert np.array_equal(got["idx"], want["idx"]), tag
    assert same_bits(got["dist2"], want["dist2"]) and same_bits(got["second2"], want["second2"]), tag
    assert np.array_equal(got["pairs"], want["pairs"]) and got["pairs"].dtype == np.int32, tag
    st = dict(got["stats"])
    assert st.pop("match_ms") == -1.0 and st == want["stats"], (tag, st, want["stats"])
    return got


@pytest.mark.parametrize("n_dst", N_DST)
def test_sizes_around_the_wave_the_tile_and_the_slices(api, ctx, n_dst):
    src, vs, dst, vd, clean = world()
    for n_src in N_SRC:
        a = check(api, ctx, src[:n_src], vs[:n_src], dst[:n_dst], vd[:n_dst], 0.0, False)
        b = check(api, ctx, src[:n_src], vs[:n_src], dst[:n_dst], vd[:n_dst], 0.9, True)
        assert len(b["pairs"]) <= len(a["pairs"]) == a["stats"]["n_matched"]
    if n_dst == 5000:
        assert len(a["pairs"]) > 800 and 100 < len(b["pairs"]) < len(a["pairs"])
        check(api, ctx, src, vs, dst, vd, 0.9, False)
        check(api, ctx, src, vs, dst, vd, 1.5, True)                 # ratio >= 1: no ratio test


def test_the_smallest_index_wins_among_duplicates_in_different_slices(api, ctx):
    src, vs, dst, vd, clean = world()
    got = check(api, ctx, clean[4400:], None, clean, None, 0.0, False)   # the repeated rows as queries, every row a candidate
    assert np.all(got["dist2"] == 0) and np.all(got["idx"] < 4000) and np.all(got["second2"] == 0)   # the runner-up is a copy
    assert np.any(got["idx"] < 20)                                   # a row with three copies: 0 .. 19, 40 .. 59 and the tail
    assert np.all(np.arange(4400, 5000) // 256 != got["idx"] // 256)     # winner and query lie in different slices


def test_a_set_against_itself(api, ctx):
    src, vs, dst, vd, clean = world()
    got = check(api, ctx, dst[:1500], vd[:1500], dst[:1500], vd[:1500], 0.0, True)
    v = got["idx"] >= 0
    assert v.sum() == got["stats"]["n_src_valid"] > 1200
    assert np.all(got["dist2"][v] == 0) and np.all(got["idx"][v] <= np.nonzero(v)[0])
    assert np.array_equal(got["pairs"][:, 0], got["pairs"][:, 1])   # mutual: only the first of equal rows pairs, with itself


def test_invalid_rows_and_an_all_invalid_side(api, ctx):
    src, vs, dst, vd, clean = world()
    got = check(api, ctx, src[:300], vs[:300], dst[:700], np.zeros(700, bool), 0.8, True)
    assert np.all(got["idx"] == -1) and np.all(np.isinf(got["dist2"])) and len(got["pairs"]) == 0 and got["stats"]["n_dst_valid"] == 0
    got = check(api, ctx, src[:300], np.zeros(300, bool), dst[:700], vd[:700], 0.0, False)
    assert np.all(got["idx"] == -1) and got["stats"]["n_src_valid"] == 0
    one = np.zeros(700, bool)
    last = int(np.nonzero(np.isfinite(dst[:700]).all(1))[0][-1])
    one[last] = True                                                 # a single candidate: no runner-up
    got = check(api, ctx, src[:300], None, dst[:700], one, 0.0, False)
    ok = np.isfinite(src[:300]).all(1)
    assert np.all(got["idx"][ok] == last) and np.all(np.isinf(got["second2"])) and np.all(np.isfinite(got["dist2"][ok]))
    empty = np.zeros((0, 33), np.float32)
    got = check(api, ctx, src[:10], None, empty, None, 0.0, True)
    assert np.all(got["idx"] == -1)
    got = check(api, ctx, empty, None, dst[:10], None, 0.5, True)
    assert got["idx"].shape == (0,) and got["pairs"].shape == (0, 2)


def test_cap_pairs_truncates_the_list_not_the_count(api, ctx):
    src, vs, dst, vd, clean = world()
    full = check(api, ctx, src, vs, dst[:2000], vd[:2000], 0.0, False)
    cut = check(api, ctx, src, vs, dst[:2000], vd[:2000], 0.0, False, max_pairs=17)
    assert cut["stats"]["n_matched"] == full["stats"]["n_matched"] > 17 and np.array_equal(cut["pairs"], full["pairs"][:17])
    none = check(api, ctx, src, vs, dst[:2000], vd[:2000], 0.0, False, max_pairs=0)
    assert len(none["pairs"]) == 0 and none["stats"]["n_matched"] == full["stats"]["n_matched"]


def test_upload_download_and_validity(api, ctx):
    src, vs, dst, vd, clean = world()
    flags = np.where(vs, 3, 0).astype(np.uint8)                      # any non-zero flag offers the row; the byte comes out as 0 / 1
    f = api.Features(ctx)
    assert len(f) == 0 and f.download()[0].shape == (0, 33)
    lib = api.load_library()
    assert lib.sf_features_upload(f.h, src.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p), C.c_int64(len(src))) == 0
    rows, valid = np.zeros((1000, 33), np.float32), np.full(1000, 9, np.uint8)
    n = C.c_int64()
    assert lib.sf_features_download(f.h, rows.ctypes.data_as(C.c_void_p), valid.ctypes.data_as(C.c_void_p), C.c_int64(999), C.byref(n)) == -1 and n.value == 1000
    assert np.all(valid == 9)
    assert lib.sf_features_download(f.h, rows.ctypes.data_as(C.c_void_p), valid.ctypes.data_as(C.c_void_p), C.c_int64(1000), C.byref(n)) == 0
    assert same_bits(rows, src) and np.array_equal(valid, (vs & np.isfinite(src).all(1)).astype(np.uint8)) and set(np.unique(valid)) == {0, 1}
    f.upload(src[:7])                                                # no flags: every finite row is valid; a smaller set replaces the larger
    rows, valid = f.download()
    assert len(f) == 7 and same_bits(rows, src[:7]) and np.array_equal(valid, np.isfinite(src[:7]).all(1))
    f.upload(np.zeros((0, 33), np.float32))
    assert len(f) == 0


def test_timing_and_refusals(api, ctx):
    src, vs, dst, vd, clean = world()
    fs, fd = api.Features(ctx, src[:100]), api.Features(ctx, dst[:300])
    a, b = fs.match(fd, profile=True), fs.match(fd)
    assert a["stats"]["match_ms"] > 0 and b["stats"]["match_ms"] == -1.0
    assert np.array_equal(a["idx"], b["idx"]) and same_bits(a["dist2"], b["dist2"])
    other = api.Context(0)
    foreign = api.Features(other, dst[:10])
    with pytest.raises(api.SlamFusionError, match="error -1"):
        fs.match(foreign)
    foreign.close()
    other.close()
    with pytest.raises(api.SlamFusionError):
        fs.match(dst[:10])                                           # not a Features object
    fm, st = api.Map(ctx, api.Cloud(ctx, ref.sphere_cloud(300, 2)[0]), 0.2), None
    fm.set_normals(ref.sphere_cloud(300, 2)[1])
    feat, st = fm.compute_fpfh(0.4)                                  # the product of compute_fpfh is a candidate set like any other
    got = feat.match(feat, mutual=True)
    rows, valid = feat.download()
    want = ref.match(rows, valid, rows, valid, 0.0, True)
    assert np.array_equal(got["idx"], want["idx"]) and same_bits(got["dist2"], want["dist2"]) and got["stats"]["n_src_valid"] == st["n_featured"]
