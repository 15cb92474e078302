"""The map-growth path -- sf_cloud_voxel_merge (csrc/sf_voxel.hip, the k_merge_* kernels) and sf_map_patch / sf_map_build
(csrc/sf_map.hip, the k_patch_* kernels, k_cell_keys and the cell table) -- restated in plain numpy, and the case tables that
tests/test_growth_rule.py (numpy against the CPU oracle, every case against its own precondition) and
tests/test_gpu_growth_direct.py (the HIP kernels against numpy, bit for bit) walk.  Nothing here comes from the library.

The reference of the merge is the plain voxel filter of the concatenation (cloud_ref_np.voxel_pcl), not the device's full path
and not the C oracle; the reference of the patch is the index sf_map_build documents, computed from the merged cloud alone.

A case is a dict(name, old, steps, leaf, cell): `old` is a voxel-filtered map made on the host (voxel_pcl(raw, leaf)[0]) unless
the case is about a map that is not one, `steps` the pending clouds merged into it one after the other.  The generators place
their points in a grid of G voxels per axis around the origin; most anchor the bounds with points that nothing else reaches, so
that placing a voxel does not move min_b.  Every generator asserts the property its case is named after and raises when it
cannot construct it; the tables are built once and nothing may write into their arrays."""
import functools

import numpy as np

import cloud_ref_np as cloud

F32 = np.float32
LEAF, CELL = 0.1, 0.25
G, HALF = 40, 20                       # voxels per axis; voxel v spans [(v - HALF) * leaf, (v - HALF + 1) * leaf)
PATCHED, SF_PATCH_NO_MERGE, SF_PATCH_ORIGIN_MOVED, SF_PATCH_LIMITS, SF_PATCH_CLAMPED_POINT = 1, 0, -2, -3, -4   # include/slamfusion.h


# ------------------------------------------------------------------ the rules
def merge(old, pending, leaf):
    """`*map_cloud += *cloud` + VoxelGrid: the plain filter of the concatenation.  -> cloud_ref_np.voxel_pcl's tuple"""
    return cloud.voxel_pcl(np.concatenate([cloud.f32(old), cloud.f32(pending)]), leaf)


def expect_merged(old, pending, leaf):
    """Which way sf_cloud_voxel_merge must go (with sf_cloud_voxel_merge_min_points at 0): the merge path iff the map is a
    non-empty, finite cloud whose voxel ids under the union's geometry strictly ascend, a finite pending point exists and
    PCL's int32 index does not overflow"""
    old, pending = cloud.f32(old), cloud.f32(pending)
    if len(old) == 0 or not np.isfinite(old).all() or not np.isfinite(pending).all(1).any():
        return False
    ids, _, overflow, _ = cloud.voxel_pcl_keys(np.concatenate([old, pending]), leaf)
    return not overflow and bool(np.all(np.diff(ids[:len(old)]) > 0))


def geometry(points, cell, lattice, org=None):
    """The grid sf_map_build chooses for an explicit cell -- origin at the smallest finite coordinates, or those snapped down
    to a multiple of `lattice` cells in float64 and rounded to float32 -- and sf_map_patch keeps (org given): per axis
    floor((max - org) / cell) + 1 cells in float64.  No finite point: origin 0, one cell.  -> (org float32 [3], dims [3])"""
    mn, mx, cnt = cloud.minmax(points)
    h = float(F32(cell))
    if cnt == 0:
        return np.zeros(3, F32), (1, 1, 1)
    if org is None:
        org = mn if lattice <= 0 else (np.floor(mn.astype(np.float64) / (lattice * h)) * (lattice * h)).astype(F32)
    org = np.asarray(org, F32)
    dims = np.floor((mx.astype(np.float64) - org.astype(np.float64)) / h).astype(np.int64) + 1
    return org, tuple(int(d) for d in dims)


def raw_cells(points, org, cell):
    """k_cell_keys before its clamp: floor((x - org) * inv_h), float32 operation by operation, inv_h = float32(1 / cell)"""
    inv_h = F32(1.0 / float(F32(cell)))
    with np.errstate(all="ignore"):
        return np.floor((cloud.f32(points) - np.asarray(org, F32)[None, :]) * inv_h)


def index(points, org, cell, dims, table=True):
    """The index of sf_map_build: the finite points in stable (cell, id) order with the id bit-cast into column 3, the cell
    of a point from raw_cells clamped to [0, dim - 1] per axis, cell id (cz * dim_y + cy) * dim_x + cx, and
    cell_start[c] = first sorted position whose cell id is >= c for c in [0, cells] (table=False leaves it out: a table
    of billions of cells).  -> dict(pts4, cell_start, org, dims, inv_h, keys: the sorted cell ids)"""
    p = cloud.f32(points)
    ids = np.nonzero(np.isfinite(p).all(1))[0]
    fc = raw_cells(p[ids], org, cell)
    c = [np.clip(fc[:, d], 0, dims[d] - 1).astype(np.int64) for d in range(3)]
    keys = (c[2] * dims[1] + c[1]) * dims[0] + c[0]
    order = np.argsort(keys, kind="stable")
    pts4 = np.zeros((len(ids), 4), F32)
    pts4[:, :3] = p[ids[order]]
    pts4[:, 3] = ids[order].astype(np.uint32).view(F32)
    cells = int(dims[0]) * int(dims[1]) * int(dims[2])
    start = np.searchsorted(keys[order], np.arange(cells + 1), side="left").astype(np.uint32) if table else None
    return dict(pts4=pts4, cell_start=start, org=np.asarray(org, F32), dims=tuple(dims), inv_h=F32(1.0 / float(F32(cell))), keys=keys[order])


def expect_patch(old, pending, leaf, cell, lattice):
    """The code sf_map_patch must report for an index built on `old` after sf_cloud_voxel_merge(old, pending): SF_PATCH_NO_MERGE
    when the merge took its full path; SF_PATCH_ORIGIN_MOVED when a build of the merged cloud chooses another origin;
    SF_PATCH_LIMITS when the grown grid has 2^32 - 1 cells or more; SF_PATCH_CLAMPED_POINT when an old point that stays (no
    pending point in its voxel) falls into another cell under the new dims than under the old ones; else 1"""
    old, pending = cloud.f32(old), cloud.f32(pending)
    if not expect_merged(old, pending, leaf):
        return SF_PATCH_NO_MERGE
    merged = merge(old, pending, leaf)[0]
    org0, dims0 = geometry(old, cell, lattice)
    org1, dims1 = geometry(merged, cell, lattice)
    if not np.array_equal(org0, org1):
        return SF_PATCH_ORIGIN_MOVED
    if dims1[0] * dims1[1] * dims1[2] >= 2 ** 32 - 1:
        return SF_PATCH_LIMITS
    ids = cloud.voxel_pcl_keys(np.concatenate([old, pending]), leaf)[0]
    stays = ~np.isin(ids[:len(old)], ids[len(old):])
    fc = raw_cells(old[stays], org0, cell)
    for d in range(3):
        if np.any(np.clip(fc[:, d], 0, dims0[d] - 1) != np.clip(fc[:, d], 0, dims1[d] - 1)):
            return SF_PATCH_CLAMPED_POINT
    return PATCHED


# ------------------------------------------------------------------ building blocks of the cases
CORNERS = ((0, 0, 0), (G - 1, G - 1, G - 1))
FACES = ((0, HALF, HALF), (HALF, 0, HALF), (HALF, HALF, 0), (G - 1, HALF, HALF), (HALF, G - 1, HALF), (HALF, HALF, G - 1))   # one bound each
BAND = tuple((i, j, 10) for j in range(8) for i in range(G))        # 320 voxels with consecutive ids that no old map of the placement cases uses


def vkey(v):
    """the voxel id of voxel coordinates under anchored bounds"""
    v = np.asarray(v, np.int64).reshape(-1, 3)
    return v[:, 0] + v[:, 1] * G + v[:, 2] * G * G


def vox_of(key):
    key = np.asarray(key, np.int64)
    return np.stack([key % G, (key // G) % G, key // (G * G)], 1)


def points_in(vox, rng, leaf=LEAF, u=None):
    """one point per row of voxel coordinates, between a quarter and three quarters of the way through the voxel"""
    vox = np.asarray(vox, np.float64).reshape(-1, 3)
    u = rng.uniform(0.25, 0.75, vox.shape) if u is None else np.broadcast_to(np.asarray(u, np.float64), vox.shape)
    return ((vox - HALF + u) * leaf).astype(F32)


def anchor_points(anchors, leaf=LEAF):
    """the points that hold the bounds: a tenth into the voxel on an axis where the voxel is the first, nine tenths where it is the last"""
    a = np.asarray(anchors, np.float64).reshape(-1, 3)
    return points_in(a, None, leaf, np.where(a == 0, 0.1, np.where(a == G - 1, 0.9, 0.5)))


def old_map(n_old, anchors, seed, leaf=LEAF, exclude=()):
    """A filtered map of exactly n_old voxels: the anchors and voxels drawn from the inner (G - 2)^3, one to three raw points
    each.  -> (old, voxel coordinates of its rows)"""
    rng = np.random.default_rng([7, n_old, seed])
    taken = [int(k) for k in vkey(anchors)] + ([int(k) for k in vkey(exclude)] if len(exclude) else [])
    inner = vkey(np.stack(np.meshgrid(*[np.arange(1, G - 1)] * 3, indexing="ij"), -1).reshape(-1, 3))
    inner = inner[~np.isin(inner, taken)]
    vox = vox_of(rng.choice(inner, n_old - len(anchors), replace=False))
    raw = np.concatenate([anchor_points(anchors, leaf)] + [points_in(vox, rng, leaf)[rng.random(len(vox)) < p] for p in (1.0, 0.5, 0.25)])
    raw = raw[rng.permutation(len(raw))]
    old, _, out_ids, st = cloud.voxel_pcl(raw, leaf)
    assert st == 0 and len(old) == n_old
    rows = vox_of(out_ids) if len(anchors) > 1 else np.asarray(anchors).reshape(1, 3)
    if len(anchors) > 1:
        assert np.array_equal(np.sort(vkey(rows)), np.sort(np.r_[vkey(anchors), vkey(vox)]))     # the ids are vkey's: the anchors hold the bounds
    return old, rows


def free_voxels(rows, count, rng, exclude=()):
    """`count` voxels of the inner grid that the map (and `exclude`) does not have"""
    inner = vkey(np.stack(np.meshgrid(*[np.arange(1, G - 1)] * 3, indexing="ij"), -1).reshape(-1, 3))
    inner = inner[~np.isin(inner, np.r_[vkey(rows), vkey(exclude) if len(exclude) else np.zeros(0, np.int64)])]
    return vox_of(rng.choice(inner, count, replace=False))


def mixed(rows, n_anchor, m, rng, leaf=LEAF):
    """m pending points: m // 2 re-observe voxels of the map (not its anchors, where it has other voxels), the rest open new
    ones, one each; in random order"""
    keys = vkey(rows)
    pool = rows[~np.isin(keys, vkey(FACES + CORNERS))] if len(rows) > n_anchor else rows
    seen = pool[rng.integers(0, len(pool), m // 2)]
    new = free_voxels(rows, m - m // 2, rng)
    return points_in(np.concatenate([seen, new]), rng, leaf)[rng.permutation(m)]


def _case(name, old, steps, leaf=LEAF, cell=CELL, falls_back=False, **kw):
    old = cloud.f32(old).copy()
    steps = [cloud.f32(s).copy() for s in steps]
    for a in [old] + steps:
        a.setflags(write=False)
    c = dict(name=name, old=old, steps=steps, leaf=leaf, cell=cell, **kw)
    host = old                                       # what the case is named after holds: which way every step goes
    want = falls_back if isinstance(falls_back, (list, tuple)) else [falls_back] * len(steps)
    for s, fb in zip(steps, want):
        assert expect_merged(host, s, leaf) == (not fb), (name, "merge path expected" if not fb else "fall-back expected")
        host = merge(host, s, leaf)[0]
    return c


def fresh_ranks(old, pending, leaf=LEAF):
    """the ranks of the fresh voxels of a merge: for every voxel of the pending points that the map does not have, the number
    of map voxels with a smaller id (k_merge_groups' g_rank), ascending"""
    ids = cloud.voxel_pcl_keys(np.concatenate([old, pending]), leaf)[0]
    old_ids, new_ids = ids[:len(old)], np.unique(ids[len(old):][ids[len(old):] >= 0])
    assert np.all(np.diff(old_ids) > 0)
    return np.searchsorted(old_ids, new_ids[~np.isin(new_ids, old_ids)], side="left")


# ------------------------------------------------------------------ merge: sizes
SIZES_OLD = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4097)
SIZES_PENDING = (1, 63, 64, 65, 257)
PATCH_SIZES_OLD = (1, 64, 65, 255, 256, 257, 4097)


@functools.lru_cache(None)
def size_cases():
    """n_old x m, half of the pending points on voxels the map has and half on new ones"""
    out = []
    for n_old in SIZES_OLD:
        anchors = CORNERS if n_old >= 2 else CORNERS[:1]        # (one point: the low corner, so that what is added lies above the origin)
        old, rows = old_map(n_old, anchors, 0)
        for m in SIZES_PENDING:
            rng = np.random.default_rng([11, n_old, m])
            pend = mixed(rows, len(anchors), m, rng)
            c = _case("n%d_m%d" % (n_old, m), old, [pend], n_old=n_old, m=m)
            r = fresh_ranks(old, pend)
            assert len(r) == m - m // 2                                   # every new voxel is one, and none is the map's
            out.append(c)
    return out


# ------------------------------------------------------------------ merge: placements
PLACEMENT_SIZES = (200, 4097)


def _placement_base(n_old):
    for seed in range(50):                            # a map with room for one voxel in front of the points 63, 64, 65, 127 and 128
        old, rows = old_map(n_old, FACES, seed, exclude=BAND)
        keys = vkey(rows)
        if all(keys[r] - keys[r - 1] >= 2 for r in (63, 64, 65, 127, 128)):
            return old, rows
    raise AssertionError("no map with a free voxel id in front of points 63, 64, 65, 127, 128")


@functools.lru_cache(None)
def placement_cases():
    out = []
    nan, inf = np.nan, np.inf
    for n_old in PLACEMENT_SIZES:
        old, rows = _placement_base(n_old)
        keys = vkey(rows)
        rng = np.random.default_rng([13, n_old])
        inner_rows = rows[~np.isin(keys, vkey(FACES))]
        tag = lambda s: "%s_n%d" % (s, n_old)

        pend = points_in(inner_rows[rng.integers(0, len(inner_rows), 150)], rng)
        assert len(fresh_ranks(old, pend)) == 0 and len(merge(old, pend, LEAF)[0]) == n_old
        out.append(_case(tag("every_point_re_observes"), old, [pend]))

        front = np.array([(i, j, 0) for j in range(3, 9) for i in range(5, 10)])
        pend = points_in(front, rng)
        assert np.all(fresh_ranks(old, pend) == 0) and len(fresh_ranks(old, pend)) == 30
        out.append(_case(tag("every_point_in_front_of_the_first"), old, [pend]))

        back = np.array([(i, j, G - 1) for j in range(30, 36) for i in range(5, 10)])
        pend = points_in(back, rng)
        assert np.all(fresh_ranks(old, pend) == n_old) and len(fresh_ranks(old, pend)) == 30
        out.append(_case(tag("every_point_behind_the_last"), old, [pend]))

        ranks = [63, 64, 65, 127, 128, n_old]
        vox = vox_of([keys[r] - 1 if r < n_old else keys[-1] + 1 for r in ranks])
        pend = points_in(vox, rng)[rng.permutation(len(vox))]
        assert list(fresh_ranks(old, pend)) == ranks                                        # 64 and 128: exactly 64 b, the edge of coarse[]
        out.append(_case(tag("one_fresh_voxel_at_ranks_63_64_65_127_128_n"), old, [pend]))

        vox = np.asarray(BAND)[rng.choice(len(BAND), 200, replace=False)]
        pend = points_in(vox, rng)
        r = fresh_ranks(old, pend)
        assert len(r) == 200 and len(np.unique(r)) == 1 and 0 < r[0] < n_old                  # between two adjacent points of the map
        out.append(_case(tag("200_fresh_voxels_of_one_rank"), old, [pend]))

        pend = points_in(np.tile(inner_rows[len(inner_rows) // 3], (257, 1)), rng)
        ids = cloud.voxel_pcl_keys(np.concatenate([old, pend]), LEAF)[0]
        assert len(np.unique(ids[n_old:])) == 1 and ids[n_old] in ids[:n_old]
        out.append(_case(tag("one_voxel_takes_257_points"), old, [pend]))

        j = int(np.nonzero(~np.isin(keys, vkey(FACES)))[0][len(inner_rows) // 2])
        out.append(_case(tag("40_copies_of_one_map_point"), old, [np.tile(old[j], (40, 1))]))

        idx = np.unique(np.r_[0, n_old - 1, 63, 64, rng.integers(0, n_old, 46)])
        pend = old[idx][rng.permutation(len(idx))]
        assert len(fresh_ranks(old, pend)) == 0
        out.append(_case(tag("points_equal_to_map_points"), old, [pend]))

        face = [F32(k) * F32(0.1) for k in range(-5, 6)]
        pend = np.array([[v, -v, 0.0] for v in face] + [[-v, F32(-0.0), v] for v in face] + [[F32(-0.0), v, F32(-0.0)] for v in face], F32)
        assert np.signbit(pend).any() and np.sum(pend == 0) > 30
        ids = cloud.voxel_pcl_keys(np.concatenate([old, pend]), LEAF)[0][n_old:]
        assert len(np.unique(ids)) >= 20
        out.append(_case(tag("coordinates_on_voxel_faces"), old, [pend]))

        bad = np.array([[nan, 0, 0], [0, inf, 0], [0, 0, -inf], [nan, nan, nan], [-inf, inf, 0]], F32)
        for name, at in (("front", [0, 1, 2]), ("back", [127, 128, 129]), ("lanes_63_64", [63, 64])):
            pend = mixed(rows, len(FACES), 130, rng).copy()
            pend[at] = bad[:len(at)]
            assert np.sum(~np.isfinite(pend).all(1)) == len(at)
            out.append(_case(tag("non_finite_pending_points_at_the_" + name), old, [pend]))
    return out


# ------------------------------------------------------------------ merge: geometry
@functools.lru_cache(None)
def geometry_cases():
    out = []
    old, rows = old_map(200, FACES, 1)
    for d in range(3):
        for side in (0, 1):
            rng = np.random.default_rng([17, d, side])
            far = np.array([HALF, HALF, HALF])
            far[d] = -7 if side == 0 else G + 6
            pend = np.concatenate([mixed(rows, len(FACES), 20, rng), points_in(far[None], rng)])
            a, b = cloud.voxel_pcl_keys(old, LEAF), cloud.voxel_pcl_keys(np.concatenate([old, pend]), LEAF)
            assert (b[3][d] < a[3][d]) == (side == 0) and b[1] > a[1]                          # min_b moves on the low sides only; more voxels
            assert (not np.array_equal(a[0], b[0][:200])) == (side == 0 or d < 2)              # the ids of the map change with min_b or a stride
            if side == 0:
                assert np.all(a[0] != b[0][:200])
            out.append(_case("beyond_%s%s" % ("-+"[side], "xyz"[d]), old, [pend]))
    leaf = 0.01                                        # 8 000 x 8 000 x 40 voxels: PCL's int32 index overflows, the filter returns its input
    old, rows = old_map(200, FACES, 2, leaf)
    rng = np.random.default_rng(19)
    pend = np.concatenate([mixed(rows, len(FACES), 20, rng, leaf), np.array([[80.0, 80.0, 0.0]], F32)])
    assert cloud.voxel_pcl_keys(np.concatenate([old, pend]), leaf)[2] and merge(old, pend, leaf)[3] == -1
    out.append(_case("int32_overflow_falls_back", old, [pend], leaf=leaf, falls_back=True))
    return out


# ------------------------------------------------------------------ merge: a centroid across a voxel face
def _crossing_triple():
    """Three equal points one ulp below a voxel face whose float32 centroid lies ON the face, hence in the next voxel.
    -> (x of the points, voxel coordinate of the points, of the centroid)"""
    inv = F32(1) / F32(LEAF)
    for k in range(-15, 16):
        x = np.nextafter(F32(k) * F32(LEAF), F32(-np.inf))
        cen = ((x + x) + x) / F32(3)
        a, b = int(np.floor(x * inv)), int(np.floor(cen * inv))
        if b == a + 1 and 1 < a + HALF < G - 3:
            return x, a + HALF, b + HALF
    raise AssertionError("no face of the grid is crossed by the centroid of three equal points")


@functools.lru_cache(None)
def crossing_cases():
    x, va, vb = _crossing_triple()
    rng = np.random.default_rng(23)
    row = [(i, 5, 5) for i in range(G)]
    inner = free_voxels(np.asarray(FACES), 30, rng, exclude=row)
    other = points_in(np.concatenate([np.asarray(FACES), inner]), rng)
    other[:len(FACES)] = anchor_points(FACES)
    yz = points_in([(0, 5, 5)], rng)[0, 1:]
    triple = np.array([[x, yz[0], yz[1]]] * 3, F32)
    out = []
    for occupied in (False, True):
        raw = np.concatenate([other, triple] + ([points_in([(vb, 5, 5)], rng)] if occupied else []))
        old, pt_ids, out_ids, st = cloud.voxel_pcl(raw, LEAF)
        at = int(np.nonzero(out_ids == pt_ids[len(other)])[0][0])                 # the row of the triple's centroid
        ids = cloud.voxel_pcl_keys(old, LEAF)[0]
        assert ids[at] == out_ids[at] + 1 and old[at, 0] == F32(va - HALF + 1) * F32(LEAF)    # the centroid is keyed into the next voxel: it lies on the face
        assert (np.sum(ids == ids[at]) == 2) == occupied
        pend = np.concatenate([points_in([(vb, 5, 5), (va, 5, 5)], rng), mixed(vox_of(out_ids), len(FACES), 10, rng)])
        got = cloud.voxel_pcl_keys(np.concatenate([old, pend]), LEAF)[0]
        assert got[len(old)] == ids[at] and got[len(old) + 1] == ids[at] - 1      # one pending point in the centroid's voxel, one where its points were
        out.append(_case("centroid_across_a_face_neighbour_%s" % ("occupied_falls_back" if occupied else "empty"), old, [pend], falls_back=occupied))
    return out


# ------------------------------------------------------------------ merge: the other fall-backs
@functools.lru_cache(None)
def fallback_cases():
    old, rows = old_map(200, FACES, 3)
    rng = np.random.default_rng(29)
    pend = mixed(rows, len(FACES), 64, rng)
    out = []
    a = old.copy()
    a[77] = [np.nan, a[77, 1], a[77, 2]]
    out.append(_case("map_with_one_nan_falls_back", a, [pend], falls_back=True))
    a = old.copy()
    a[[100, 101]] = a[[101, 100]]
    out.append(_case("map_with_two_rows_swapped_falls_back", a, [pend], falls_back=True))
    out.append(_case("every_pending_point_non_finite_falls_back", old, [np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]] * 22, F32)], falls_back=True))
    out.append(_case("empty_pending_cloud_falls_back", old, [np.zeros((0, 3), F32)], falls_back=True))
    out.append(_case("empty_map_falls_back", np.zeros((0, 3), F32), [pend], falls_back=True))
    return out


# ------------------------------------------------------------------ merge: chains
@functools.lru_cache(None)
def chain_cases():
    """three steps on one cloud; the second replaces a point that holds a bound (the bounds a merge carries over are not
    carried then: the third step looks again)"""
    out = []
    old, rows = old_map(200, FACES, 4)
    for name, anchor, d in (("smallest_x", FACES[0], 0), ("largest_z", FACES[5], 2)):
        rng = np.random.default_rng([31, d])
        host, steps = old, []
        for k in range(3):
            have = vox_of(cloud.voxel_pcl_keys(host, LEAF)[0])
            pend = mixed(have, len(FACES), 60, rng)
            if k == 1:
                pend = np.concatenate([pend[:30], points_in([anchor], rng), pend[30:]])
                holder = (np.argmin if d == 0 else np.argmax)(host[:, d])
                after = merge(host, pend, LEAF)[0]
                assert (after[:, d].min() > host[holder, d]) if d == 0 else (after[:, d].max() < host[holder, d])   # the bound moved inwards
            steps.append(pend)
            host = merge(host, pend, LEAF)[0]
        out.append(_case("chain_replaces_the_" + name, old, steps))
    return out


def merge_cases():
    return size_cases() + placement_cases() + geometry_cases() + crossing_cases() + fallback_cases() + chain_cases()


# ------------------------------------------------------------------ patch: the subset and its own cases
LATTICES = (0, 64)


def patch_subset():
    sizes = [c for c in size_cases() if c["n_old"] in PATCH_SIZES_OLD]
    return sizes + placement_cases() + geometry_cases() + crossing_cases()[:1] + chain_cases()


def sorted_ids(old, cell, lattice):
    """the point ids of a map in the order of its index"""
    org, dims = geometry(old, cell, lattice)
    return index(old, org, cell, dims)["pts4"][:, 3].copy().view(np.uint32).astype(np.int64)


@functools.lru_cache(None)
def replaced_position_cases(lattice):
    """the entries a merge replaces, placed in the index of the old map: sorted positions 0, 31, 32, 255, 256 and n_old - 1 (the
    bitmap's word and block edges), all 256 entries of the second block, none.  A point that holds a bound is re-observed by
    a copy of itself (its centroid is the point: the bounds stay), any other by a point elsewhere in its voxel."""
    n_old = 600
    old, rows = old_map(n_old, FACES, 5)
    order = sorted_ids(old, CELL, lattice)
    holds = np.isin(vkey(rows), vkey(FACES))
    out = []
    for name, pos in (("positions_0_31_32_255_256_last", [0, 31, 32, 255, 256, n_old - 1]), ("a_whole_block_of_256", list(range(256, 512))), ("no_entry", [])):
        rng = np.random.default_rng([37, len(pos), lattice])
        ids = order[pos]
        again = np.array([old[i] if holds[i] else points_in(rows[i][None], rng)[0] for i in ids], F32).reshape(-1, 3)
        pend = np.concatenate([again, points_in(free_voxels(rows, 40, rng), rng)])
        pend = pend[rng.permutation(len(pend))]
        got = cloud.voxel_pcl_keys(np.concatenate([old, pend]), LEAF)[0]
        replaced = np.nonzero(np.isin(got[:n_old], got[n_old:]))[0]
        assert np.array_equal(np.sort(replaced), np.sort(ids))                         # exactly these entries, at exactly these positions
        assert np.array_equal(np.nonzero(np.isin(order, replaced))[0], np.sort(pos))
        c = _case("replaced_%s_L%d" % (name, lattice), old, [pend])
        assert expect_patch(old, pend, LEAF, CELL, lattice) == PATCHED
        out.append(c)
    return out


def _clamped_map(lattice, pad):
    """A map whose largest x lies one to three ulp below a cell face so that float32 puts it INTO the next cell -- fc == dim --
    and the grid clamps it back; three more points share its cell with larger ids (higher voxels), `pad` more points elsewhere
    shift its place in the index.  -> (old, row of the clamped point)"""
    rng = np.random.default_rng([41, lattice, pad])
    base = np.concatenate([anchor_points(FACES), points_in(free_voxels(np.asarray(FACES), 20 + pad, rng), rng)])
    y = z = F32(0.05)
    for _ in range(2000):
        if lattice == 0:
            base[0, 0] = F32(-1.99 + rng.uniform(0, 0.005))             # another origin with every try
        org = geometry(base, CELL, lattice)[0]
        face = float(org[0]) + (int(np.ceil((2.25 - float(org[0])) / CELL)) + int(rng.integers(0, 24))) * CELL   # a cell face beyond the x anchor
        x = F32(face)
        for _ in range(int(rng.integers(1, 4))):
            x = np.nextafter(x, F32(-np.inf))
        if not (float(x) < face and x > base[:, 0].max()):
            continue
        mates = np.array([[x - F32(0.12), y, 0.15], [x - F32(0.12), y, 0.22], [x - F32(0.12), 0.15, 0.22]], F32)   # y, z in [0.01, 0.25): one cell with either origin
        raw = np.concatenate([base, [[x, y, z]], mates]).astype(F32)
        old, _, _, st = cloud.voxel_pcl(raw, LEAF)
        assert st == 0 and len(old) == len(raw)
        org, dims = geometry(old, CELL, lattice)
        at = int(np.argmax(old[:, 0]))
        fc = raw_cells(old, org, CELL)
        if old[at, 0] == x and fc[at, 0] == dims[0]:
            cells = np.clip(fc, 0, np.array(dims) - 1)
            same = np.nonzero((cells == cells[at]).all(1))[0]
            assert len(same) == 4 and same.min() == at                   # it is the first of its cell by id, with three behind it
            assert all(np.all(fc[np.arange(len(old)) != at, d] < dims[d]) for d in range(3))   # and the only point the grid clamps
            return old, at
    raise AssertionError("no point found that the grid clamps to its upper face")


@functools.lru_cache(None)
def clamped_cases(lattice):
    """A point clamped to the +x face: growth beyond +x frees it (SF_PATCH_CLAMPED_POINT), growth beyond +y does not (1); re-observed
    by a copy of itself it is replaced, and no clamped point stays (1; the device may also leave it to the build).  `want` holds the
    accepted codes per step."""
    out = []
    old, at = _clamped_map(lattice, 0)
    rows = vox_of(cloud.voxel_pcl_keys(old, LEAF)[0])
    rng = np.random.default_rng([43, lattice])
    some = points_in(free_voxels(rows, 10, rng), rng)
    beyond_x = np.concatenate([some, [[old[at, 0] + F32(1.0), old[at, 1], old[at, 2]]]]).astype(F32)
    beyond_y = np.concatenate([some, [[old[at, 0] - F32(1.0), old[:, 1].max() + F32(1.0), old[at, 2]]]]).astype(F32)
    out.append(_case("clamped_point_growth_beyond_+x_L%d" % lattice, old, [beyond_x], want=[SF_PATCH_CLAMPED_POINT]))
    out.append(_case("clamped_point_growth_beyond_+y_L%d" % lattice, old, [beyond_y], want=[PATCHED]))
    for pad in range(8):                              # 0 .. 7 more entries: every alignment of the binary searches that walk over the entry
        old, at = _clamped_map(lattice, pad)
        pend = np.concatenate([some, [[old[at, 0] + F32(1.0), old[at, 1], old[at, 2]]], old[at][None]]).astype(F32)
        got = cloud.voxel_pcl_keys(np.concatenate([old, pend]), LEAF)[0]
        assert got[-1] == got[at] and (merge(old, pend, LEAF)[0] == old[at]).all(1).any()       # replaced by a centroid that is the point itself
        out.append(_case("clamped_point_re_observed_pad%d_L%d" % (pad, lattice), old, [pend], want=[(PATCHED, SF_PATCH_CLAMPED_POINT)]))
    for c in out:
        pred = expect_patch(c["old"], c["steps"][0], LEAF, CELL, lattice)
        assert pred in np.atleast_1d(c["want"][0]), (c["name"], pred)
    return out


@functools.lru_cache(None)
def origin_cases():
    """a centroid below the smallest x: without a lattice the origin moves, with one of 64 cells (16 m) it stays"""
    old, rows = old_map(200, FACES, 6)
    rng = np.random.default_rng(47)
    pend = np.concatenate([mixed(rows, len(FACES), 20, rng), [[old[:, 0].min() - F32(1.0), 0.0, 0.0]]]).astype(F32)
    assert expect_patch(old, pend, LEAF, CELL, 0) == SF_PATCH_ORIGIN_MOVED and expect_patch(old, pend, LEAF, CELL, 64) == PATCHED
    return [_case("centroid_below_the_origin_L0", old, [pend], lattice=0, want=[SF_PATCH_ORIGIN_MOVED]),
            _case("centroid_below_the_origin_L64", old, [pend], lattice=64, want=[PATCHED])]


@functools.lru_cache(None)
def limits_case():
    """A sparse map of 64 points over 50 m x 50 m x 10 m at a cell of 0.05 m (2e8 cells) that grows to 235 m x 235 m: 4.4e9 cells, past
    2^32.  The voxel grid at leaf 0.1 stays inside int32."""
    rng = np.random.default_rng(53)
    raw = np.concatenate([[[0, 0, 0], [49.99, 49.99, 9.99]], rng.uniform(1, 49, (62, 3)) * [1, 1, 0.2]]).astype(F32)
    old = cloud.voxel_pcl(raw, LEAF)[0]
    pend = np.concatenate([rng.uniform(1, 49, (20, 3)) * [1, 1, 0.2], [[234.99, 234.99, 5.0]]]).astype(F32)
    cell = 0.05
    d0, d1 = geometry(old, cell, 0)[1], geometry(merge(old, pend, LEAF)[0], cell, 0)[1]
    assert len(old) == 64 and np.prod(d0, dtype=np.float64) < 2 ** 28 and np.prod(d1, dtype=np.float64) >= 2 ** 32
    assert expect_patch(old, pend, LEAF, cell, 0) == SF_PATCH_LIMITS
    return _case("grid_grows_past_2^32_cells", old, [pend], cell=cell, lattice=0, want=[SF_PATCH_LIMITS])


def patch_only_cases():
    """the cases beyond the subset, every lattice"""
    out = []
    for lattice in LATTICES:
        out += replaced_position_cases(lattice) + clamped_cases(lattice)
    return out + origin_cases() + [limits_case()]


# ------------------------------------------------------------------ build: tiny maps
@functools.lru_cache(None)
def build_cases():
    rng = np.random.default_rng(59)
    out = []
    for n in (0, 1, 2, 63, 64, 65, 257):
        out.append(dict(name="n%d" % n, p=rng.uniform(-2, 2, (n, 3)).astype(F32)))
    out.append(dict(name="all_points_identical", p=np.tile(np.array([[0.3, -1.7, 0.9]], F32), (70, 1))))
    p = (np.array([0.26, -0.74, 0.51]) + rng.uniform(0, 0.2, (70, 3))).astype(F32)
    out.append(dict(name="all_points_in_one_cell", p=p))
    p = rng.uniform(-2, 2, (130, 3)).astype(F32)
    p[126:] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3]
    out.append(dict(name="last_rows_non_finite", p=p))
    for c in out:
        c["p"].setflags(write=False)
    return out
