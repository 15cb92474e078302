"""The query ordering in front of an alignment (csrc/sf_order.hpp: k_order_hist -> k_order_scan -> k_order_move, or the ids +
gather form k_order_scatter + k_order_gather), run directly through the hook sf_test_query_order and compared EXACTLY with numpy:
every scan must come back as points[numpy.argsort(keys, kind="stable")], bit for bit, in both forms.  No tolerance anywhere.

Sizes: the edges of a lane (1), of a wave's 64-element chunk (63, 64, 65), of a wave's span of 1 024 elements, of a tile of 4 096
and several tiles with a ragged last one; batches of 1, 3, 8 and 9 scans (the grid pads the scans to a multiple of 8, one per
XCD).  Contents: see CONTENTS.  Every content asserts its own precondition on the returned keys (plain cell key), so a case
cannot pass by missing its edge; the comparison itself runs under the plain key and under the density table of the index.

Then the library's own path: an alignment of 3 x 140 000 points (above the automatic ordering threshold) with the query order
"cell" and "as_given" equals, byte for byte, the results the commit before k_order_move returned (tests/golden/
query_order_align_3x140k.npy, written by record_alignments below on that commit's build), and "cell" equals an "as_given"
alignment of the scans ordered beforehand by the hook's ids + gather form."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32 = np.float32
KEY_NONE = 1023
TILE = 4096
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 3 * 4096 + 17)
BATCHES = (1, 3, 8, 9)
CONTENTS = ("random",      # uniform over the map's box and a little beyond it
            "one_cell",    # every point in one map cell: one bucket, runs as long as the tile
            "spread",      # element e in bucket 7 e mod K (K >= MIN_BUCKETS): no bucket gets two queries of a tile of up to K elements
            "stretches",   # equal keys in stretches of 300 elements: stability across the chunks of a wave and across waves
            "nonfinite")   # NaN and +-inf coordinates scattered through the scan: last in their scan, in element order
BOX_LO, BOX_HI = np.array([-8.0, -8.0, -4.0]), np.array([8.0, 8.0, 4.0])
CELL = 0.5
MIN_BUCKETS = 500          # buckets of the plain key that hold a cell of the test's map, at least


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def scan_pose(synth, b):
    """map <- scan b: different from scan to scan"""
    return synth.make_T((0.3 * b, -0.2 * b, 0.1 * b), (0.5 * b, -0.25 * b, 7.0 * b))


def to_scan_frame(p_map, T):
    """float32 scan points whose posed position is p_map (up to rounding)"""
    Ti = np.linalg.inv(T)
    with np.errstate(all="ignore"):                            # (the non-finite points stay non-finite)
        return (np.asarray(p_map, np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(F32)


@pytest.fixture(scope="module")
def world(api, ctx):
    """a map of 6 000 points, and one representative cell centre per bucket of the plain key"""
    rng = np.random.Generator(np.random.PCG64(20240))
    pts = rng.uniform(BOX_LO, BOX_HI, (6000, 3)).astype(F32)
    pts[:2] = BOX_LO, BOX_HI                                   # the grid spans the whole box
    mp = api.Map(ctx, pts, CELL)
    ax = [np.arange(lo + CELL / 2, hi, CELL) for lo, hi in zip(BOX_LO, BOX_HI)]
    centres = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(1, -1, 3).astype(F32)
    keys, _ = api.hook_query_order(mp, centres, form=0, table=False)
    uniq, first = np.unique(keys[0], return_index=True)
    assert len(uniq) >= MIN_BUCKETS and uniq.max() < KEY_NONE, (len(uniq), uniq.max())   # the plain key spreads this grid over the buckets
    return dict(map=mp, bucket_centres=centres[0][first].astype(np.float64))


def make_content(kind, n, b, world, rng):
    """scan b of n points in the MAP frame (float64), and what the plain keys of the scan must look like"""
    cen = world["bucket_centres"]
    jitter = rng.uniform(-0.1, 0.1, (n, 3))
    if kind == "random":
        return rng.uniform(BOX_LO - 1.0, BOX_HI + 1.0, (n, 3)), None
    if kind == "one_cell":
        return cen[(37 * b + 5) % len(cen)] + jitter, "one"
    if kind == "spread":
        return cen[(np.arange(n) * 7 + b) % len(cen)] + jitter, "spread"      # (7 and len(cen) need not be coprime: checked on the keys)
    if kind == "stretches":
        return cen[((np.arange(n) // 300) % 5) * 11 + b] + jitter, "stretches"
    p = rng.uniform(BOX_LO, BOX_HI, (n, 3))
    bad = rng.uniform(size=n) < 0.07
    if n >= 3:
        bad[[0, n // 2, n - 1]] = True                                          # the first and the last element among them
    return p, bad


def scan_points(made, T, rng):
    """the scan as it is handed over; the non-finite coordinates go into the scan's own frame, one per marked point, so that
    the other two still tell the marked points apart"""
    p_map, what = made
    s = to_scan_frame(p_map, T)
    if isinstance(what, np.ndarray):
        s[what, rng.integers(0, 3, what.sum())] = rng.choice(np.array([np.nan, np.inf, -np.inf], F32), what.sum())
    return s


def check_pattern(what, keys, n, case):
    if what is None:
        return
    if isinstance(what, np.ndarray):
        assert np.all(keys[what] == KEY_NONE) and np.all(keys[~what] < KEY_NONE), case
    elif what == "one":
        assert len(np.unique(keys)) == 1 and keys[0] < KEY_NONE, case
    elif what == "spread":
        nb = len(np.unique(keys))
        for t in range(0, n, TILE):
            counts = np.bincount(keys[t:t + TILE], minlength=1024)
            assert counts.max() <= -(-min(TILE, n - t) // nb) + 1, (case, counts.max())
            if min(TILE, n - t) <= MIN_BUCKETS:
                assert counts.max() == 1, case                                  # runs of one
    elif what == "stretches":
        change = np.flatnonzero(np.diff(keys.astype(np.int64)) != 0) + 1
        assert np.all(np.diff(np.r_[0, change]) == 300) and len(np.unique(keys)) == min(5, -(-n // 300)), case


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", CONTENTS)
def test_order_equals_numpy_stable_sort(api, synth, world, kind, n):
    rng = np.random.Generator(np.random.PCG64(1000 * CONTENTS.index(kind) + n))
    for batch in BATCHES:
        poses = np.stack([scan_pose(synth, b) for b in range(batch)])
        made = [make_content(kind, n, b, world, rng) for b in range(batch)]
        points = np.stack([scan_points(made[b], poses[b], rng) for b in range(batch)])
        for table in (False, True):
            got = {}
            for form in (0, 1):
                keys, ordered = api.hook_query_order(world["map"], points, poses, form=form, table=table)
                case = (kind, n, batch, "table" if table else "plain", "form %d" % form)
                assert keys.shape == (batch, n) and keys.dtype == np.uint16 and ordered.shape == points.shape and ordered.dtype == F32, case
                for b in range(batch):
                    if not table:
                        check_pattern(made[b][1], keys[b], n, case + (b,))
                    want = points[b][np.argsort(keys[b], kind="stable")]
                    assert np.array_equal(bits(ordered[b]), bits(want)), case + (b,)
                got[form] = (keys, ordered)
            assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(bits(got[0][1]), bits(got[1][1])), (kind, n, batch, table)


def test_a_scan_is_ordered_alone(api, synth, world):
    """the order of a scan does not depend on what else is in the batch, nor on where in the batch it stands"""
    rng = np.random.Generator(np.random.PCG64(77))
    n = 2 * TILE + 100
    points = rng.uniform(BOX_LO, BOX_HI, (9, n, 3)).astype(F32)
    poses = np.stack([scan_pose(synth, b) for b in range(9)])
    keys, ordered = api.hook_query_order(world["map"], points, poses, form=1, table=True)
    for b in (0, 4, 8):
        k1, o1 = api.hook_query_order(world["map"], points[b:b + 1], poses[b:b + 1], form=1, table=True)
        assert np.array_equal(k1[0], keys[b]) and np.array_equal(bits(o1[0]), bits(ordered[b])), b


def test_hook_refuses_bad_arguments(api, world):
    lib, mp = api.load_library(), world["map"]
    p, T = np.zeros((1, 4, 3), F32), np.eye(4)[None]
    k, o = np.zeros((1, 4), np.uint16), np.zeros((1, 4, 3), F32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.sf_test_query_order(mp.h, ptr(p), 1, 4, ptr(T), 2, 0, ptr(k), ptr(o)) != 0      # unknown form
    assert lib.sf_test_query_order(mp.h, ptr(p), 0, 4, ptr(T), 1, 0, ptr(k), ptr(o)) != 0      # no scan
    assert lib.sf_test_query_order(mp.h, ptr(p), 65, 4, ptr(T), 1, 0, ptr(k), ptr(o)) != 0
    assert lib.sf_test_query_order(mp.h, ptr(p), 1, 0, ptr(T), 1, 0, ptr(k), ptr(o)) != 0      # no point
    assert lib.sf_test_query_order(mp.h, None, 1, 4, ptr(T), 1, 0, ptr(k), ptr(o)) != 0
    assert lib.sf_test_query_order(None, ptr(p), 1, 4, ptr(T), 1, 0, ptr(k), ptr(o)) != 0
    assert "sf_test_query_order" in lib.sf_last_error().decode()
    empty = api.Map(mp.ctx)
    assert lib.sf_test_query_order(empty.h, ptr(p), 1, 4, ptr(T), 1, 0, ptr(k), ptr(o)) != 0   # a map without an index


# ---------------------------------------------------------------- through the library
ALIGN_N, ALIGN_BATCH, ALIGN_ITERS = 140_000, 3, 8
GOLDEN = "query_order_align_3x140k.npy"


def align_world(api, ctx, synth):
    raw = synth.make_map(300_000)
    mp = api.Map(ctx, raw, 0.25)
    mp.estimate_normals(0.25)
    scans = np.stack([synth.make_scan(raw, ALIGN_N, scan_id=b)[0] for b in range(ALIGN_BATCH)])
    return mp, scans


def align_bytes(api, ctx, mp, scans, order):
    """the sf_icp_result array of one p2plane alignment on an object of its own (what an object has learnt from earlier
    alignments does not enter), as bytes"""
    icp = api.Icp(ctx, 0.5, ALIGN_ITERS, 0.05, 1e-5)
    icp.set_target(mp)
    icp.set_query_order(order)
    icp.set_source_batch(scans)
    icp.set_initial_batch(None)
    icp.align_batch_async("p2plane")
    raw = icp.fetch_results(raw=True)
    out = np.frombuffer(bytes(raw), np.uint8).copy()
    icp.close()
    return out


def record_alignments(api, ctx, synth):
    """what the golden file holds: rows "cell", "as_given\""""
    mp, scans = align_world(api, ctx, synth)
    return np.stack([align_bytes(api, ctx, mp, scans, order) for order in ("cell", "as_given")])


def test_alignment_is_what_it_was(api, ctx, synth):
    from conftest import load_golden
    mp, scans = align_world(api, ctx, synth)
    golden = load_golden(GOLDEN)
    cell = align_bytes(api, ctx, mp, scans, "cell")
    given = align_bytes(api, ctx, mp, scans, "as_given")
    res = (api.IcpResult * ALIGN_BATCH).from_buffer_copy(cell.tobytes())
    assert all(r.iterations == ALIGN_ITERS and r.n_corr > ALIGN_N // 2 for r in res), [(r.iterations, r.n_corr) for r in res]   # the alignment did its work
    assert not np.array_equal(cell, given)               # the order is felt in the last bits: "cell" did order
    assert np.array_equal(given, golden[1]), "as_given differs from the recorded results"
    assert np.array_equal(cell, golden[0]), "cell differs from the results recorded before k_order_move"
    # and without the record: the scans ordered beforehand by the ids + gather form, aligned as given
    keys, ordered = api.hook_query_order(mp, scans, None, form=0, table=True)
    assert np.array_equal(align_bytes(api, ctx, mp, ordered, "as_given"), cell)
