"""The bucket keys of the query ordering themselves (csrc/sf_order.hpp k_order_hist with CellKeyFn of sf_icp.hip), pinned bit for bit.

tests/test_gpu_query_order.py proves that every scan comes back as the stable sort of WHATEVER keys the histogram pass wrote; a
change of the key arithmetic (another fmaf nesting, a cell taken on the other side of a face, another clamp, a table entry read
at another place) would pass it and still move Xq and with it every float64 sum of an alignment.  Here the keys returned by the
hook sf_test_query_order must equal the keys recorded on the build of the commit before the histogram pass went stage by stage
(tests/golden/query_order_keys_small.npz, written by record_keys below on that commit's build).  No tolerance anywhere.

Content of a scan, mixed point by point: uniform points a little beyond the map's box; points ON the faces of the map's cells and
up to three float32 steps to either side of them on every axis (scan 0 has the identity pose, so there the posed position IS the
face; under the other poses it lies within rounding of it) -- where a changed rounding flips the bucket; 7 % NaN / +-inf coordinates,
the first and the last element among them.  Both the plain key and the density table, both forms of the hook (they share the
histogram pass and must return the same keys), sizes at the edges of a lane, a wave's chunk, a wave's span and a tile.

Then the two instantiations the hook does not reach, through alignments compared bitwise (T64, iterations, n_corr) with results
recorded on the same build: the id-carrying histogram and scatter (the owned queries of two x-slabs: segment offsets and
src_idx), and the tile sort (k_order_hist_tile, two digits, the second one through the first one's ids).  The sharded and tile
tests of the suite compare with an unsharded / untiled alignment to 1e-9 and 1e-12, which a moved key passes."""
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32 = np.float32
KEY_NONE = 1023
BOX_LO, BOX_HI = np.array([-8.0, -8.0, -4.0]), np.array([8.0, 8.0, 4.0])
CELL = 0.5
CASES = ((1, 3), (64, 3), (65, 3), (1025, 3), (4097, 9), (2 * 4096 + 17, 1))       # (points per scan, scans)
GOLDEN = "query_order_keys_small.npz"
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)


def case_name(n, batch, table):
    return "n%d_b%d_%s" % (n, batch, "table" if table else "plain")


@pytest.fixture(scope="module")
def key_map(api, ctx):
    """the 6 000-point map with 0.5 m cells of tests/test_gpu_query_order.py"""
    return make_key_map(api, ctx)


def make_key_map(api, ctx):
    rng = np.random.Generator(np.random.PCG64(20240))
    pts = rng.uniform(BOX_LO, BOX_HI, (6000, 3)).astype(F32)
    pts[:2] = BOX_LO, BOX_HI
    mp = api.Map(ctx, pts, CELL)
    org = mp.index()["org"]
    assert np.array_equal(org, BOX_LO.astype(F32)), org            # the faces below are the faces of this grid
    return mp


def step_f32(v, steps):
    """v moved by `steps` float32 steps (negative: down)"""
    v = np.asarray(v, F32).copy()
    for k in range(1, int(np.abs(steps).max()) + 1):
        v = np.where(steps >= k, np.nextafter(v, F32(np.inf)), np.where(steps <= -k, np.nextafter(v, F32(-np.inf)), v)).astype(F32)
    return v


def make_scans(synth, n, batch):
    """-> points float32 [batch][n][3] as handed over, poses [batch][4][4], and per point its kind (0 uniform, 1 face, 2 non-finite)"""
    rng = np.random.Generator(np.random.PCG64(77_000 + 16 * n + batch))
    points, poses, kinds = [], [], []
    dims = ((BOX_HI - BOX_LO) / CELL).astype(int)
    for b in range(batch):
        T = np.eye(4) if b == 0 else synth.make_T((0.3 * b, -0.2 * b, 0.1 * b), (0.5 * b, -0.25 * b, 7.0 * b))
        kind = rng.choice(3, n, p=(0.50, 0.43, 0.07))
        if n >= 3:
            kind[[0, n - 1]] = 2
        uni = rng.uniform(BOX_LO - 1.0, BOX_HI + 1.0, (n, 3))
        face = BOX_LO + CELL * np.stack([rng.integers(0, d + 1, n) for d in dims], 1)          # exact in float32
        face = step_f32(face, rng.integers(-3, 4, (n, 3)))
        p_map = np.where((kind == 1)[:, None], face.astype(np.float64), uni)
        Ti = np.linalg.inv(T)
        s = p_map.astype(F32) if b == 0 else (p_map @ Ti[:3, :3].T + Ti[:3, 3]).astype(F32)
        bad = np.flatnonzero(kind == 2)
        s[bad, rng.integers(0, 3, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], F32), len(bad))
        points.append(s); poses.append(T); kinds.append(kind)
    return np.stack(points), np.stack(poses), np.stack(kinds)


def crc(a):
    return np.uint32(zlib.crc32(np.ascontiguousarray(a).tobytes()))


def record_keys(api, ctx, synth, path=GOLDEN_PATH):
    """writes the fixture: the keys of every case (form 0), the crc of the points they were computed from, and the two alignments"""
    mp = make_key_map(api, ctx)
    out = {}
    for n, batch in CASES:
        points, poses, _ = make_scans(synth, n, batch)
        out["crc_n%d_b%d" % (n, batch)] = crc(points)
        for table in (False, True):
            out[case_name(n, batch, table)] = api.hook_query_order(mp, points, poses, form=0, table=table)[0]
    world = make_align_world(api, ctx, synth)
    for name, fn in (("shard", align_owned), ("tile", align_tiled)):
        res = fn(api, ctx, world)[0]
        for k, v in res.items():
            out["%s_%s" % (name, k)] = v
    np.savez_compressed(path, **out)
    return out


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN_PATH, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("n,batch", CASES)
def test_keys_are_what_they_were(api, synth, key_map, golden, n, batch):
    points, poses, kinds = make_scans(synth, n, batch)
    assert crc(points) == golden["crc_n%d_b%d" % (n, batch)], "the test's own points differ from the recorded ones"
    if n >= 3:
        assert np.all(kinds[:, 0] == 2) and np.all(kinds[:, -1] == 2)
    if n >= 1000:
        assert all((kinds == k).sum() > 0.03 * kinds.size for k in range(3))                   # every kind of point is there
    got = {}
    for table in (False, True):
        for form in (0, 1):
            keys, _ = api.hook_query_order(key_map, points, poses, form=form, table=table)
            case = (n, batch, "table" if table else "plain", "form %d" % form)
            assert keys.shape == (batch, n) and keys.dtype == np.uint16, case
            assert np.all(keys[kinds == 2] == KEY_NONE) and np.all(keys[kinds != 2] < KEY_NONE), case
            want = golden[case_name(n, batch, table)]
            assert np.array_equal(keys, want), (case, int((keys != want).sum()), "keys differ from the recorded ones")
            got[table, form] = keys
    if n >= 1000:
        assert not np.array_equal(got[False, 0], got[True, 0])                                  # the table was in effect
        face0 = got[False, 0][0][kinds[0] == 1]
        assert len(np.unique(face0)) > 100, len(np.unique(face0))                               # the face points spread over the grid


# ---------------------------------------------------------------- the id-carrying and the tile instantiations, through alignments
ALIGN_N, ALIGN_BATCH, ALIGN_ITERS = 6000, 3, 8


@pytest.fixture(scope="module")
def align_world(api, ctx, synth):
    return make_align_world(api, ctx, synth)


def make_align_world(api, ctx, synth):
    raw = synth.make_map(600_000)                         # 24.5 m x 24.5 m x 10 m: more than 1 024 map tiles, so the tile sort takes two digits
    mp = api.Map(ctx, raw, 0.25)
    mp.estimate_normals(0.25)
    scans = np.stack([synth.make_scan(raw, ALIGN_N, scan_id=b)[0] for b in range(ALIGN_BATCH)])
    return dict(map=mp, scans=scans)


def pack(res):
    return dict(T64=np.stack([np.asarray(r["T64"], np.float64).reshape(4, 4) for r in res]), iterations=np.array([r["iterations"] for r in res], np.int64),
                n_corr=np.array([r["n_corr"] for r in res], np.int64))


def align_owned(api, ctx, world):
    """two x-slabs of one map stepping together: each orders the queries it owns (segment offsets + src_idx)"""
    edges = (-1e30, 0.0, 1e30)
    members = []
    for r in range(2):
        icp = api.Icp(ctx, 0.5, ALIGN_ITERS, 0.05, 1e-5)
        icp.set_target(world["map"])
        icp.set_query_order("cell")
        icp.set_source_batch(world["scans"])
        icp.set_initial_batch(None)
        icp.set_shard(edges[r], edges[r + 1])
        members.append(icp)
    res, _ = api.align_group(members, "p2plane")
    owned = np.stack([m.owned_counts() for m in members])
    for m in members:
        m.close()
    return pack(res), owned


def align_tiled(api, ctx, world):
    icp = api.Icp(ctx, 0.5, ALIGN_ITERS, 0.05, 1e-5)
    icp.set_target(world["map"])
    icp.set_query_order("cell")
    icp.set_wide_scan_points(1024)                        # scans of 6 000 points on the launch list of wide scans: the one the tile search serves
    icp.set_tile_search("always")
    icp.set_source_batch(world["scans"])
    icp.set_initial_batch(None)
    res = icp.align_batch("p2plane")
    info = icp.tile_info()
    icp.close()
    return pack(res), info


def same_bits(got, golden, name):
    for k, v in got.items():
        want = golden["%s_%s" % (name, k)]
        assert v.dtype == want.dtype and v.shape == want.shape and v.tobytes() == want.tobytes(), (name, k, v, want)


def test_owned_query_alignment_is_what_it_was(api, ctx, align_world, golden):
    got, owned = align_owned(api, ctx, align_world)
    assert np.all(owned > 0.3 * ALIGN_N) and np.all(owned < 0.8 * ALIGN_N), owned               # each slab owns about half of every scan (+ margin)
    assert np.all(got["iterations"] == ALIGN_ITERS) and np.all(got["n_corr"] > ALIGN_N // 2), got
    same_bits(got, golden, "shard")


def test_tile_sorted_alignment_is_what_it_was(api, ctx, align_world, golden):
    got, info = align_tiled(api, ctx, align_world)
    assert info["on"] and int(np.prod(info["tiles"])) > 1024, info                              # two digits: the second pass reads the first one's ids
    assert np.all(got["iterations"] == ALIGN_ITERS) and np.all(got["n_corr"] > ALIGN_N // 2), got
    same_bits(got, golden, "tile")
