"""The rules of csrc/sf_cloud.hip and of the two voxel filters of csrc/sf_voxel.hip in plain numpy, and the case tables both
tests/test_cloud_rule.py (numpy against the CPU oracle) and tests/test_gpu_cloud_direct.py (the HIP kernels against numpy) walk.
Every function names the reference line it restates, as oracle/crops.c and oracle/voxel.c do.  numpy rounds every float32
operation on its own (one ufunc per operation: nothing is fused), which is what the reference's x86-64 build does.

A case is a dict; its "pre" entry is a function that asserts, on the numpy side, that the inputs really sit on the edge the case
is named after, so that a case cannot pass by missing it.  The tables are built once and nothing may write into their arrays."""
import functools

import numpy as np

F32 = np.float32
INT32_MAX = 2 ** 31 - 1
FLT_MAX = np.finfo(np.float32).max
CB = 256                      # flags per workgroup of the compaction
SCAN = 1024                   # block counts per round of k_scan_blocks; also the grid cap of k_minmax_partial
STRIDE = CB * SCAN            # 262 144: from here on the scan takes a second round and the bounds reduction a second stride


def _quiet(fn):
    @functools.wraps(fn)
    def wrapped(*a, **k):
        with np.errstate(all="ignore"):
            return fn(*a, **k)
    return wrapped


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)


# ------------------------------------------------------------------ the rules
def compact(p, flags):
    """sf::compact_cloud: the points whose flag is not 0, in order, and their indices"""
    flags = np.asarray(flags)
    return f32(p)[flags != 0], np.nonzero(flags)[0].astype(np.int32)


@_quiet
def minmax(p):
    """pcl::getMinMax3D (common/impl/common.hpp) as voxel_grid.hpp calls it: over the points whose three coordinates are
    finite; zeros and 0 when there is none (sf::cloud_minmax)"""
    p = f32(p)
    fin = np.isfinite(p).all(1)
    if not fin.any():
        return np.zeros(3, F32), np.zeros(3, F32), 0
    return p[fin].min(0), p[fin].max(0), int(fin.sum())


@_quiet
def radius_d2(p, c, radius):
    """FLANN L2_Simple with the query first: diff = centre - point, result += diff * diff over x, y, z, all float32; the
    squared radius is the float64 product rounded once (point_cloud_processing.hpp:37-45)"""
    p, c = f32(p), np.asarray(c, F32)
    r2 = F32(np.float64(radius) * np.float64(radius))
    d = c[None, :] - p
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return d2, r2


@_quiet
def crop_radius(p, c, radius, sorted):
    """point_cloud_processing.hpp:31-53: finite points with d2 < r2 (strict); sorted: by (d2, index) as the kd-tree search
    returns them, else in index order.  -> (points, indices)"""
    p = f32(p)
    d2, r2 = radius_d2(p, c, radius)
    idx = np.nonzero(np.isfinite(p).all(1) & (d2 < r2))[0]
    if sorted:
        idx = idx[np.lexsort((idx, d2[idx]))]
    return p[idx], idx.astype(np.int32)


@_quiet
def crop_aabb(p, lo, hi):
    """localization_node.py:105-115: rows with a NaN dropped (skip_nans), the rest widened to float64, bounds inclusive"""
    p = f32(p)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    x = p.astype(np.float64)
    keep = ~np.isnan(p).any(1) & (x >= lo).all(1) & (x <= hi).all(1)
    return p[keep], np.nonzero(keep)[0].astype(np.int32)


@_quiet
def crop_obb(p, center, R, extent):
    """localization_node.py:222-225, Open3D GetPointIndicesWithinBoundingBox: d = p - center in float64,
    |d . R[:, k]| <= extent[k] / 2 for every k; written as <= so that a NaN projection fails"""
    p = f32(p)
    c, R, e = np.asarray(center, np.float64), np.asarray(R, np.float64).reshape(3, 3), np.asarray(extent, np.float64)
    d = p.astype(np.float64) - c
    keep = np.ones(len(p), bool)
    for k in range(3):
        proj = (d[:, 0] * R[0, k] + d[:, 1] * R[1, k]) + d[:, 2] * R[2, k]
        keep &= np.abs(proj) <= e[k] / 2
    return p[keep], np.nonzero(keep)[0].astype(np.int32)


@_quiet
def remove_floor(p):
    """point_cloud_processing.hpp:76-92: z > 0 stays"""
    p = f32(p)
    keep = p[:, 2] > 0
    return p[keep], np.nonzero(keep)[0].astype(np.int32)


def subsample(p, step):
    """point_cloud_processing.hpp:55-74: untouched (indices None) when there are fewer points than the step, else every step-th"""
    p = f32(p)
    if len(p) < step:
        return p, None
    return p[::step], np.arange(0, len(p), step, dtype=np.int32)


@_quiet
def transform(p, T):
    """icp_point_to_point.cpp:99-110: separate float32 multiplies and adds, left to right"""
    p, T = f32(p), np.asarray(T, F32).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)


@_quiet
def unpack_pc2(buf, width, height, point_step, row_step, offsets, is_f64):
    """pcl::fromROSMsg (localization_node.cpp:290-291): point i at row (i / width) * row_step + (i % width) * point_step, its
    fields gathered byte by byte; float64 fields rounded to float32 (nearest even, overflow to inf)"""
    buf = np.frombuffer(bytes(buf), np.uint8)
    i = np.arange(width * height, dtype=np.int64)
    base = (i // width) * (row_step or width * point_step) + (i % width) * point_step
    size = 8 if is_f64 else 4
    cols = []
    for off in offsets:
        raw = np.ascontiguousarray(buf[base[:, None] + off + np.arange(size)[None, :]])
        cols.append(raw.view("<f8").astype(F32).reshape(-1) if is_f64 else raw.view("<f4").reshape(-1))
    return np.stack(cols, 1) if len(i) else np.zeros((0, 3), F32)


@_quiet
def voxel_pcl_keys(p, leaf, wide=False):
    """pcl::VoxelGrid<PointXYZ>::applyFilter (filters/impl/voxel_grid.hpp) up to the linear index:
    -> (ids [n] with -1 for a non-finite point, voxel count div0 * div1 * div2, overflow verdict, min_b)"""
    p = f32(p)
    inv = F32(1) / F32(leaf)
    ids = np.full(len(p), -1, np.int64)
    mn, mx, cnt = minmax(p)
    if cnt == 0:
        return ids, 0, False, np.zeros(3, np.int64)
    span = ((mx - mn) * inv).astype(np.int64) + 1                     # float32 arithmetic, then int64
    overflow = int(span[0]) * int(span[1]) * int(span[2]) > INT32_MAX
    if overflow and not wide:
        return ids, 0, True, np.zeros(3, np.int64)
    min_b = np.floor(mn * inv).astype(np.int64)
    max_b = np.floor(mx * inv).astype(np.int64)
    div = max_b - min_b + 1
    fin = np.isfinite(p).all(1)
    ijk = (np.floor(p[fin] * inv) - min_b.astype(F32)).astype(np.int64)  # static_cast<int>(floor(p * inv) - float(min_b))
    ids[fin] = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    return ids, int(div[0]) * int(div[1]) * int(div[2]), False, min_b


@_quiet
def voxel_pcl(p, leaf, wide=False):
    """the whole filter: per voxel the float32 sums taken sequentially in ascending point id, divided by the float32 count;
    output in ascending id.  -> (centroids, per-point ids, per-voxel ids, status: 0 | -1 = overflow, output = input)"""
    p = f32(p)
    ids, _, overflow, _ = voxel_pcl_keys(p, leaf, wide)
    dt = np.int64 if wide else np.int32
    if overflow:
        return p.copy(), ids.astype(dt), np.zeros(0, dt), -1
    pts = np.nonzero(ids >= 0)[0]
    pts = pts[np.argsort(ids[pts], kind="stable")]
    out_ids, first = np.unique(ids[pts], return_index=True)
    cen = np.zeros((len(out_ids), 3), F32)
    for v, (a, b) in enumerate(zip(first, list(first[1:]) + [len(pts)])):
        cen[v] = np.cumsum(np.r_[np.zeros((1, 3), F32), p[pts[a:b]]], axis=0, dtype=F32)[-1] / F32(b - a)   # from +0, one addition after the other
    return cen, ids.astype(dt), out_ids.astype(dt), 0


@_quiet
def voxel_o3d(p, voxel):
    """open3d PointCloud::VoxelDownSample (PointCloud.cpp): index floor((p - (min_bound - v/2)) / v) in float64, per voxel the
    float64 mean with the sum taken in point order; voxels in ascending (i, j, k).  -> (means f64, per-point ijk, per-voxel ijk)"""
    x = f32(p).astype(np.float64)
    vmin = x.min(0) - voxel * 0.5
    ijk = np.floor((x - vmin) / voxel).astype(np.int32)
    order = np.lexsort((np.arange(len(x)), ijk[:, 2], ijk[:, 1], ijk[:, 0]))
    s = ijk[order]
    first = np.nonzero(np.r_[True, (s[1:] != s[:-1]).any(1)])[0]
    means = np.zeros((len(first), 3))
    for v, (a, b) in enumerate(zip(first, list(first[1:]) + [len(order)])):
        means[v] = np.cumsum(np.r_[np.zeros((1, 3)), x[order[a:b]]], axis=0)[-1] / float(b - a)
    return means, ijk, s[first]


# ------------------------------------------------------------------ case tables
def payload(n):
    """p[i] = (i, i + 0.5, -i): exact in float32 below 2^24, so a misplaced point shows"""
    i = np.arange(n, dtype=np.float64)
    return np.stack([i, i + 0.5, -i], 1).astype(F32)


BOUNDARY_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025,
                  STRIDE - 1, STRIDE, STRIDE + 1,         # 1024 blocks; 1024 blocks; 1025: the second round / the second stride
                  2 * STRIDE + 1,                         # 2049 blocks: a third round
                  2 * STRIDE + 77]                        # ragged
BIG = 2 * STRIDE + 77
FLAG_PATTERNS = ["all", "none", "first", "last", "last_ragged", "alternating", "lanes_63_64", "one_wave", "blocks_empty_then_full",
                 "bernoulli_0.01", "bernoulli_0.5", "bernoulli_0.99", "values_0_1_2_255"]


def flag_pattern(name, n, seed=0):
    """uint8 flags of one pattern, or None where the pattern does not exist at this size (last_ragged without a ragged block)"""
    i = np.arange(n)
    rng = np.random.default_rng([seed, n, FLAG_PATTERNS.index(name)])
    if name == "all":
        return np.ones(n, np.uint8)
    if name == "none":
        return np.zeros(n, np.uint8)
    if name in ("first", "last", "last_ragged"):
        if name == "last_ragged" and n % CB == 0:
            return None
        f = np.zeros(n, np.uint8)
        if n:
            f[0 if name == "first" else n - 1] = 1
        return f
    if name == "alternating":
        return (i & 1).astype(np.uint8)
    if name == "lanes_63_64":                      # the last lane of wave 0 and the first of wave 1, in every block
        return np.isin(i % CB, (63, 64)).astype(np.uint8)
    if name == "one_wave":                         # wave 2 of every block, whole
        return ((i % CB) // 64 == 2).astype(np.uint8)
    if name == "blocks_empty_then_full":
        return (i // CB >= (n + CB - 1) // CB // 2).astype(np.uint8)
    if name.startswith("bernoulli_"):
        return (rng.random(n) < float(name.split("_")[1])).astype(np.uint8)
    if name == "values_0_1_2_255":                 # any non-zero value keeps
        return np.array([0, 1, 2, 255], np.uint8)[rng.integers(0, 4, n)]
    raise AssertionError(name)


def compact_cases(n):
    """[(pattern, flags)] of one size, every pattern that exists there"""
    out = [(name, flag_pattern(name, n)) for name in FLAG_PATTERNS]
    out = [(name, f) for name, f in out if f is not None]
    assert ("last_ragged" in [name for name, _ in out]) == (n % CB != 0)
    return out


# -- bounds
def minmax_positions(n):
    """where the extremes go: index 0, n - 1, the middle of the ragged last block, and 5 into the second stride"""
    pos = [0, n - 1]
    if n % CB and n > CB:
        pos.append(n - (n % CB + 1) // 2)
    if n > STRIDE + 5:
        pos.append(STRIDE + 5)
    return sorted(set(pos))


def minmax_placed(n, rot, seed=3):
    """n points strictly inside (-100, 100)^3 but for six coordinates that hold one bound each: bound e (x, y, z minimum, then
    x, y, z maximum) sits at position e + rot of minmax_positions, the two bounds of an axis never on one point.
    -> (points, mn, mx); n = 1: the point is its own bounds"""
    rng = np.random.default_rng([seed, n])
    p = rng.uniform(-100, 100, (n, 3)).astype(F32)
    if n <= 1:
        return p, (p[0] if n else np.zeros(3, F32)), (p[0] if n else np.zeros(3, F32))
    pos = minmax_positions(n)
    mn, mx = np.array([-150.5, -160.25, -170.125], F32), np.array([151.5, 161.25, 171.125], F32)
    for e in range(6):
        at = pos[(e + rot + (1 if e >= 3 and len(pos) == 3 else 0)) % len(pos)]
        p[at, e % 3] = (mn if e < 3 else mx)[e % 3]
        assert np.sum(np.abs(p[:, e % 3]) >= 100) == (1 if e < 3 else 2)      # the precondition: each bound is held once, where it was put
        assert (np.argmin if e < 3 else np.argmax)(p[:, e % 3]) == at
    return p, mn, mx


@functools.lru_cache(None)
def minmax_special_cases():
    """[dict(name, p, pre)]: non-finite points and the edges of float32"""
    rng = np.random.default_rng(17)
    out = []
    n = STRIDE + 77
    base = rng.uniform(-5, 5, (n, 3)).astype(F32)

    p = base.copy()
    for at in (0, 300, STRIDE + 5, n - 1):
        p[at] = [-1e6, np.nan, 0]                   # x would be the minimum; the point is ignored as a whole
    p[7] = [0, 1e6, np.nan]
    p[STRIDE + 9] = [np.nan, 0, -1e6]
    out.append(dict(name="nan_beside_a_would_be_bound", p=p, pre=lambda r: _assert(r[2] == n - 6 and (r[0] > -5).all() and (r[1] < 5).all())))

    p = base.copy()
    p[0], p[63], p[STRIDE + 5], p[n - 1] = [np.inf, 0, 0], [0, -np.inf, 0], [0, 0, np.inf], [-np.inf, -np.inf, -np.inf]
    p[100] = [-7, 8, -9]                            # a finite bound holder right among them
    out.append(dict(name="inf_points", p=p, pre=lambda r: _assert(r[2] == n - 4 and r[0][0] == -7 and r[1][1] == 8 and r[0][2] == -9 and np.isfinite(r[0]).all() and np.isfinite(r[1]).all())))

    p = np.full((300, 3), np.nan, F32)
    p[::3, 0], p[1::3] = 1.0, np.inf                # one NaN coordinate is enough; whole inf rows
    out.append(dict(name="every_point_non_finite", p=p, pre=lambda r: _assert(r[2] == 0 and not r[0].any() and not r[1].any())))
    out.append(dict(name="every_point_non_finite_two_strides", p=np.full((STRIDE + 3, 3), np.nan, F32), pre=lambda r: _assert(r[2] == 0)))

    p = base[:1500].copy()
    p[3], p[1499] = [FLT_MAX, -FLT_MAX, FLT_MAX], [-FLT_MAX, FLT_MAX, -FLT_MAX]
    out.append(dict(name="flt_max", p=p, pre=lambda r: _assert((r[0] == -FLT_MAX).all() and (r[1] == FLT_MAX).all() and r[2] == 1500)))

    tiny = np.float32(1e-45)
    p = (rng.integers(-1000, 1000, (777, 3)).astype(F32) * tiny).astype(F32)   # every coordinate a denormal (or zero)
    p[5], p[776] = [-2000 * tiny] * 3, [2000 * tiny] * 3
    out.append(dict(name="denormals", p=p, pre=lambda r: _assert((r[0] == F32(-2000) * tiny).all() and (r[1] == F32(2000) * tiny).all() and r[0][0] != 0 and abs(r[0][0]) < np.finfo(F32).tiny)))

    p = np.zeros((513, 3), F32)
    p[::2] = -0.0
    out.append(dict(name="signed_zeros", p=p, pre=lambda r, p=p: _assert(np.signbit(p).any() and not np.signbit(p).all() and (r[0] == 0).all() and (r[1] == 0).all() and r[2] == 513)))

    p = -np.abs(base[:700])                         # every coordinate negative: the maxima are below the zero a reduction might start from
    p[p == 0] = -1
    out.append(dict(name="all_negative", p=p, pre=lambda r: _assert((r[1] < 0).all())))
    for c in out:
        c["p"].setflags(write=False)
    return out


def _assert(cond):
    assert cond
    return True


# -- radius crop
def _radius_case(name, p, c, radius, pre):
    p = f32(p).copy()
    p.setflags(write=False)
    return dict(name=name, p=p, c=np.asarray(c, F32), radius=float(radius), pre=pre)


def _tie_groups(p, c, radius):
    pts, idx = crop_radius(p, c, radius, True)
    d2, r2 = radius_d2(p, c, radius)
    return len(idx), len(np.unique(d2[idx])), int(np.sum(np.isfinite(p).all(1) & (d2 == r2)))


@functools.lru_cache(None)
def radius_cases():
    rng = np.random.default_rng(23)
    out = []

    g = np.arange(17, dtype=np.float64) * 0.25 - 2.0
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F32)
    lat = lat[rng.permutation(len(lat))]
    lat = np.concatenate([lat[:1000], [[np.nan, 0, 0]], lat[1000:3000], [[0.25, np.inf, 0]], lat[3000:]]).astype(F32)
    out.append(_radius_case("lattice", lat, (0.25, -0.5, 0), 1.25,
                            lambda p, c, r: _assert(len(p) == 4915 and _tie_groups(p, c, r) == (485, 22, 30))))

    for k in (0, 1, 2, 1023, 1024, 1025):           # kept counts around the sort's tile of 1024 keys
        m = k + 301
        u = rng.normal(size=(m, 3))
        u /= np.linalg.norm(u, axis=1)[:, None]
        rad = np.where(np.arange(m) < k, rng.uniform(0.0, 0.9, m), rng.uniform(1.1, 3.0, m))
        p = (u * rad[:, None])[rng.permutation(m)]
        out.append(_radius_case("kept_%d" % k, p, (0, 0, 0), 1.0, lambda p, c, r, k=k: _assert(len(crop_radius(p, c, r, False)[1]) == k)))

    r = 1.3                                          # float32(r * r) in float64 is not float32(r) squared in float32
    x = F32(1.3)
    xs = [x]
    for _ in range(40):
        xs = [np.nextafter(xs[0], F32(0))] + xs + [np.nextafter(xs[-1], F32(2))]
    p = np.zeros((len(xs), 3), F32)
    p[:, 0] = xs

    def pre_rr(p, c, r):
        d2, r2 = radius_d2(p, c, r)
        other = F32(r) * F32(r)
        assert other != r2
        assert np.any((d2 >= min(r2, other)) & (d2 < max(r2, other)))     # a point the other squared radius would decide differently
        assert np.any(d2 < min(r2, other)) and np.any(d2 >= max(r2, other))
        return True
    out.append(_radius_case("r_times_r_in_float64", p[rng.permutation(len(p))], (0, 0, 0), r, pre_rr))

    r2 = F32(1.5625)                                 # radius 1.25: a pair on the rim one ulp apart, one in and one out
    below = np.nextafter(r2, F32(0))
    pair = None
    xx = np.nextafter(F32(1.25), F32(0))
    for k in range(1, 4096):
        yy = F32(np.sqrt(k * 2.0 ** -26))
        if F32(xx * xx) + F32(yy * yy) == below:
            pair = yy
            break
    assert pair is not None
    p = np.array([[1.25, 0, 0], [xx, pair, 0], [0, -1.25, 0], [1.0, 0.75, 0], [0, xx, pair], [0, 0, 1.25], [0.75, 0, -1.0]], F32)

    def pre_rim(p, c, r):
        d2, r2 = radius_d2(p, c, r)
        assert np.sum(d2 == r2) >= 1 and np.sum(d2 == np.nextafter(r2, F32(0))) >= 1
        return True
    out.append(_radius_case("rim_pair_one_ulp_apart", p, (0, 0, 0), 1.25, pre_rim))

    k = np.arange(13, dtype=np.float64)              # denormal d2: k * 1e-20 from a zero centre, radius 1e-19
    p = np.zeros((13 * 3, 3))
    for d in range(3):
        p[13 * d:13 * d + 13, d] = k * 1e-20 * (-1) ** d
    p = p[rng.permutation(len(p))]

    def pre_den(p, c, r):
        d2, r2 = radius_d2(p, c, r)
        tiny = np.finfo(F32).tiny
        assert 0 < r2 < tiny and np.sum((d2 > 0) & (d2 < tiny)) >= 30     # the squared radius and the distances are denormals
        assert np.sum(d2 < r2) == 3 * 10 and np.sum(d2 >= r2) == 3 * 3 and len(np.unique(d2[d2 < r2])) == 10
        return True
    out.append(_radius_case("denormal_d2", p, (0, 0, 0), 1e-19, pre_den))

    p = np.array([[1, 2, 3], [1, 2, 3], [1 + 1e-6, 2, 3], [0, 0, 0]], F32)
    out.append(_radius_case("radius_zero", p, (1, 2, 3), 0.0, lambda p, c, r: _assert(np.sum(radius_d2(p, c, r)[0] == 0) == 2 and len(crop_radius(p, c, r, False)[1]) == 0)))

    p = np.concatenate([rng.uniform(-1e6, 1e6, (300, 3)), [[3e19, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [-FLT_MAX / 4, 0, 0], [1.2e19, 1.2e19, 1.2e19], [1e18, -1e18, 1e18]]])
    p = p[rng.permutation(len(p))]

    def pre_huge(p, c, r):
        d2, r2 = radius_d2(p, c, r)
        fin = np.isfinite(p).all(1)
        assert np.isinf(r2) and np.sum(fin & np.isinf(d2)) == 3            # d2 < r2 is false for them: inf < inf
        assert len(crop_radius(p, c, r, False)[1]) == np.sum(fin & np.isfinite(d2)) == 301
        return True
    out.append(_radius_case("huge_radius_r2_inf", p, (0.5, 0, 0), 1e30, pre_huge))
    return out


# -- boxes
def _box_case(name, p, pre=None, **kw):
    p = f32(p).copy()
    p.setflags(write=False)
    return dict(name=name, p=p, pre=pre or (lambda *a: True), **kw)


def _neighbours(v):
    v = F32(v)
    return [np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))]


@functools.lru_cache(None)
def aabb_cases():
    rng = np.random.default_rng(29)
    out = []
    lo, hi = np.array([-1.0, -2.0, -3.0]), np.array([1.0, 2.0, 3.0])
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-2, 2) for z in (-3, 3)], F32)
    outside = []
    for cnr in corners:
        for d in range(3):
            q = cnr.copy()
            q[d] = np.nextafter(q[d], F32(np.sign(q[d]) * np.inf))
            outside.append(q)
    p = np.concatenate([corners, outside])[rng.permutation(32)]
    out.append(_box_case("inclusive_corners", p, lo=lo, hi=hi, pre=lambda c: _assert(len(crop_aabb(c["p"], c["lo"], c["hi"])[1]) == 8)))

    p = np.array([[a, b, c] for a in _neighbours(0.5) for b in _neighbours(0.5) for c in _neighbours(0.5)], F32)
    out.append(_box_case("lo_equals_hi", p, lo=[0.5] * 3, hi=[0.5] * 3, pre=lambda c: _assert(len(crop_aabb(c["p"], c["lo"], c["hi"])[1]) == 1)))

    p = np.array([[v, 0, 0] for v in _neighbours(0.1)] + [[0, v, 0] for v in _neighbours(0.1)] + [[0, 0, v] for v in _neighbours(0.1)], F32)
    up = lambda c: _assert(float(F32(0.1)) > 0.1 and float(np.nextafter(F32(0.1), F32(0))) < 0.1)
    out.append(_box_case("hi_0.1_point_at_float32_0.1_is_out", p, lo=[-1] * 3, hi=[0.1] * 3,
                         pre=lambda c: up(c) and _assert(len(crop_aabb(c["p"], c["lo"], c["hi"])[1]) == 3)))      # only the value below
    out.append(_box_case("lo_0.1_point_at_float32_0.1_is_in", p + F32(0.1) * (p == 0), lo=[0.1] * 3, hi=[1] * 3,
                         pre=lambda c: up(c) and _assert(float(F32(0.1)) >= 0.1 and len(crop_aabb(c["p"], c["lo"], c["hi"])[1]) == 6)))
    cloud = rng.uniform(-2, 2, (257, 3)).astype(F32)
    out.append(_box_case("lo_above_hi", cloud, lo=[1, -1, -1], hi=[-1, 1, 1], pre=lambda c: _assert(len(crop_aabb(c["p"], c["lo"], c["hi"])[1]) == 0)))
    out.append(_box_case("nan_bound", cloud, lo=[-1, np.nan, -1], hi=[1, 1, 1], pre=lambda c: _assert(len(crop_aabb(c["p"], c["lo"], c["hi"])[1]) == 0)))
    p = np.array([[np.inf, 0, 0], [0, -np.inf, 0], [np.inf, -np.inf, np.inf], [0, 0, 0], [np.nan, np.inf, 0], [0, 0, -np.inf]], F32)
    out.append(_box_case("inf_bounds_inf_points", p, lo=[-np.inf] * 3, hi=[np.inf] * 3, pre=lambda c: _assert(len(crop_aabb(c["p"], c["lo"], c["hi"])[1]) == 5)))
    out.append(_box_case("inf_hi_only", p, lo=[0, 0, 0], hi=[np.inf] * 3, pre=lambda c: _assert(list(crop_aabb(c["p"], c["lo"], c["hi"])[1]) == [0, 3])))
    p = np.zeros((6, 3), F32)
    p[0, 0] = p[1, 1] = p[2, 2] = np.nan
    p[3] = [np.nan, np.nan, 0]
    p[4] = np.nan
    out.append(_box_case("nan_in_each_coordinate", p, lo=[-1] * 3, hi=[1] * 3, pre=lambda c: _assert(list(crop_aabb(c["p"], c["lo"], c["hi"])[1]) == [5])))
    for n in (1, 257, STRIDE + 1):
        p = rng.uniform(-2, 2, (n, 3)).astype(F32)
        p[::97] = [np.nan, 0, 0]
        p[n - 1] = [0.5, 0.5, 0.5]
        out.append(_box_case("size_%d" % n, p, lo=[-1, -0.1, 0.1], hi=[1.5, 0.7, 1.9],
                             pre=lambda c: _assert(crop_aabb(c["p"], c["lo"], c["hi"])[1][-1] == len(c["p"]) - 1)))
    return out


@functools.lru_cache(None)
def obb_cases():
    rng = np.random.default_rng(31)
    out = []
    eye = np.eye(3)
    one_up = np.nextafter(F32(1), F32(2))
    p = []
    for d in range(3):
        for s in (-1, 1):
            for v in (F32(1), one_up):
                q = np.zeros(3, F32)
                q[d] = s * v
                p.append(q)
    p += [[1, 1, 1], [-1, -1, -1], [one_up, 1, 1], [1, 1, -one_up]]
    cnt = lambda c: len(crop_obb(c["p"], c["center"], c["R"], c["extent"])[1])
    out.append(_box_case("identity_points_at_one", p, center=[0, 0, 0], R=eye, extent=[2, 2, 2], pre=lambda c: _assert(cnt(c) == 8)))

    p = np.array([[0.3, 0.5, -0.2], [0.3, np.nextafter(F32(0.5), F32(1)), 0], [-0.9, 0.5, 0.9], [0, np.nextafter(F32(0.5), F32(0)), 0], [2, 0.5, 0]], F32)
    out.append(_box_case("zero_extent_points_on_the_plane", p, center=[0, 0.5, 0], R=eye, extent=[2, 0, 2], pre=lambda c: _assert(cnt(c) == 2)))
    cloud = rng.uniform(-2, 2, (1025, 3)).astype(F32)
    cloud[0] = 0
    out.append(_box_case("negative_extent", cloud, center=[0, 0, 0], R=eye, extent=[2, -1e-300, 2], pre=lambda c: _assert(cnt(c) == 0)))
    th = 0.4                                         # tests/test_gpu_parity.py::test_crops_match_oracle: not orthonormal
    R = 0.8 * np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]) + 0.2 * eye
    out.append(_box_case("non_orthonormal_R", cloud, center=[0.5, 0.2, 0.0], R=R, extent=[3.0, 1.5, 1.5], pre=lambda c: _assert(50 < cnt(c) < 1000)))
    p = cloud[:300].copy()
    p[5], p[6], p[7], p[8], p[299] = [np.nan, 0, 0], [0, np.inf, 0], [-np.inf, 0, 0], [0, 0, np.nan], [np.inf, np.inf, np.inf]
    out.append(_box_case("nan_inf_points", p, center=[0, 0, 0], R=R, extent=[1e300, 1e300, 1e300], pre=lambda c: _assert(cnt(c) == 295)))

    q = np.nextafter(F32(0.6), F32(1))               # a centre float32 cannot hold: rounding it to float32 would let q in
    half = float(q) - 0.1 - 7e-10

    def pre_centre(c):
        ctr = np.array(c["center"])
        assert float(F32(0.1)) != 0.1
        mine = crop_obb(c["p"], ctr, c["R"], c["extent"])[1]
        rounded = crop_obb(c["p"], ctr.astype(F32).astype(np.float64), c["R"], c["extent"])[1]
        assert list(mine) == [1] and list(rounded) == [0, 1]
        return True
    out.append(_box_case("centre_not_a_float32", [[q, 0.1, 0.1], [0.5, 0.1, 0.1]], center=[0.1, 0.1, 0.1], R=eye, extent=[2 * half] * 3, pre=pre_centre))
    return out


@functools.lru_cache(None)
def floor_case():
    z = np.array([-0.0, 0.0, 1e-45, -1e-45, np.nan, np.inf, -np.inf, 1e-6], F32)
    p = payload(len(z)).copy()
    p[:, 2] = z
    p.setflags(write=False)
    kept = remove_floor(p)[1]
    assert list(kept) == [2, 5, 7] and p[2, 2] > 0 and p[2, 2] < np.finfo(F32).tiny and np.signbit(p[0, 2]) and not np.signbit(p[1, 2])
    return p


SUBSAMPLE_CASES = [(3, 7), (6, 7), (7, 7), (8, 7), (300, 1), (256 * 3, 3), (256 * 3 + 1, 3), (10, 6), (1000, 999), (STRIDE + 1, 2)]   # (n, step)


@functools.lru_cache(None)
def transform_cases():
    rng = np.random.default_rng(37)
    T = np.array([[0.8, -0.6, 0.1, 12.5], [0.6, 0.8, -0.05, -3.25], [0.02, 0.03, 0.99, 0.75], [0, 0, 0, 1]], F32)
    out = []
    for n in (1, 255, 256, 257):
        p = rng.uniform(-50, 50, (n, 3)).astype(F32)
        for at, row in ((0, [np.nan, 1, 2]), (n // 2, [1, np.inf, 2]), (n - 1, [-0.0, -0.0, -0.0]), (n // 3, [3, 4, -np.inf])):
            if n >= 255 or at == 0:
                p[at] = row
        if n == 1:
            p[0] = [-0.0, -0.0, -0.0]
        p.setflags(write=False)
        out.append(dict(name="n_%d" % n, p=p, T=T))
    z = np.array([[0.0, -0.0, 0.0]] * 3 + [[-0.0, -0.0, -0.0]], F32)
    out.append(dict(name="signed_zero_sums", p=z, T=np.array([[1, 1, 1, -0.0], [-1, 1, 1, -0.0], [1, -1, -1, 0], [0, 0, 0, 1]], F32)))
    return out


# -- PointCloud2
def _pc2_pack(vals, width, height, point_step, offsets, pad, seed):
    """vals[n][3] (float32 or float64) -> the bytes of a message with `pad` spare bytes behind every row; the bytes between
    the fields are noise"""
    rng = np.random.default_rng(seed)
    row_step = width * point_step + pad
    buf = rng.integers(0, 256, height * row_step, dtype=np.uint8)
    size = vals.dtype.itemsize
    raw = vals.view(np.uint8).reshape(len(vals), 3, size)
    for i in range(len(vals)):
        base = (i // width) * row_step + (i % width) * point_step
        for f in range(3):
            buf[base + offsets[f]:base + offsets[f] + size] = raw[i, f]
    return buf.tobytes(), row_step


@functools.lru_cache(None)
def pc2_cases():
    """[dict(name, data, width, height, point_step, row_step, offsets, f64, want_bits uint32 [n][3])]"""
    rng = np.random.default_rng(41)
    out = []
    f32_specials = np.array([0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc12345, 0x7f800001, 0x7f7fffff, 0x00800000, 0x3f800000], np.uint32)
    a = F32(1.0)
    odd, even = np.nextafter(a, F32(2)), np.nextafter(np.nextafter(a, F32(2)), F32(2))
    tiny = 2.0 ** -149
    f64_specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, float(FLT_MAX), float(FLT_MAX) * (1 + 2.0 ** -25), float(FLT_MAX) * (1 + 2.0 ** -24), 1e39, -1e300,
                             (float(a) + float(odd)) / 2, (float(odd) + float(even)) / 2, -(float(a) + float(odd)) / 2,      # halfway: to even
                             float(odd) + 2.0 ** -40, 1e-40, -3e-42, tiny, tiny / 2, tiny * 0.75, tiny * 1.5, tiny * 2.5, 2.0 ** -126, 2.0 ** -126 * (1 - 2.0 ** -25), 1e-300,
                             0.1, 1 / 3.0], np.float64)
    shapes = {1: (1, 1), 255: (85, 3), 256: (64, 4), 257: (1, 257)}
    for n, (width, height) in shapes.items():
        for is_f64 in (False, True):
            if is_f64:
                vals = rng.normal(0, 100, (n, 3))
                flat = vals.reshape(-1)
                k = min(len(flat), len(f64_specials))
                flat[rng.permutation(len(flat))[:k]] = f64_specials[rng.permutation(len(f64_specials))[:k]]
                if n == 1:
                    flat[:] = [float(FLT_MAX) * (1 + 2.0 ** -24), (float(a) + float(odd)) / 2, 1e-40]
                with np.errstate(all="ignore"):
                    want = vals.astype(F32)
                step, offs = 25, (1, 9, 17)
            else:
                bits = rng.integers(0, 1 << 32, (n, 3), dtype=np.uint64).astype(np.uint32)
                flat = bits.reshape(-1)
                k = min(len(flat), len(f32_specials))
                flat[rng.permutation(len(flat))[:k]] = f32_specials[rng.permutation(len(f32_specials))[:k]]
                vals = bits.view(F32)
                want = vals
                step, offs = 13, (1, 5, 9)
            data, row_step = _pc2_pack(np.ascontiguousarray(vals), width, height, step, offs, 5, n)
            out.append(dict(name="%s_n%d" % ("f64" if is_f64 else "f32", n), data=data, width=width, height=height, point_step=step, row_step=row_step,
                            offsets=offs, f64=is_f64, want_bits=np.ascontiguousarray(want).view(np.uint32).copy()))
    # the specials really are what they are named
    with np.errstate(all="ignore"):
        s = f64_specials.astype(F32)
    assert s[5] == FLT_MAX and s[6] == FLT_MAX and np.isinf(s[7]) and np.isinf(s[8]) and s[10] == a and s[11] == even and s[12] == -a and s[13] == odd
    assert 0 < s[14] < np.finfo(F32).tiny and s[16] == F32(tiny) and s[17] == 0 and s[18] == F32(tiny) and s[19] == F32(2 * tiny) and s[20] == F32(2 * tiny)
    assert s[22] == F32(2.0 ** -126) and s[23] == 0
    return out


# -- voxel filters
def _vox_case(name, p, leaf, status, pre=None):
    p = f32(p).copy()
    p.setflags(write=False)
    return dict(name=name, p=p, leaf=leaf, status=status, pre=pre or (lambda c: True))


@functools.lru_cache(None)
def voxel_pcl_cases():
    rng = np.random.default_rng(43)
    out = []
    rows = []
    for k in range(-20, 21):                         # the voxel faces k * float32(0.1) with their two float32 neighbours, along (x, -x, 0)
        for v in _neighbours(F32(k) * F32(0.1)):
            rows.append([v, -v, 0])

    def pre_faces(c):
        ids, nvox, ovf, min_b = voxel_pcl_keys(c["p"], c["leaf"])
        assert len(c["p"]) == 123 and len(np.unique(ids)) == 83 and (min_b[:2] < 0).all() and not ovf and (ids >= 0).all()
        assert all(len(np.unique(ids[t:t + 3])) >= 2 for t in range(0, 123, 3))      # a face runs through every triple
        return True
    out.append(_vox_case("faces", rows, 0.1, 0, pre_faces))

    def pre_near(c):
        ids, nvox, ovf, _ = voxel_pcl_keys(c["p"], c["leaf"])
        assert not ovf and nvox == 1290 ** 3 == 2146689000 and list(ids) == [0, 2146688999, -1, 1065850240]
        return True
    out.append(_vox_case("near_int32_limit", [[0, 0, 0], [128.95] * 3, [np.nan, 0, 0], [64] * 3], 0.1, 0, pre_near))
    out.append(_vox_case("past_int32_limit", [[0, 0, 0], [129.15] * 3, [np.nan, 0, 0], [64] * 3], 0.1, -1,
                         lambda c: _assert(voxel_pcl_keys(c["p"], c["leaf"])[2])))
    same = np.tile(np.array([[1.23, -4.56, 7.89]], F32), (100, 1))
    out.append(_vox_case("identical_points", same, 0.1, 0, lambda c: _assert(voxel_pcl_keys(c["p"], c["leaf"])[1] == 1)))
    p = same.copy()
    p[[0, 17, 50, 99]] = [[np.nan, 0, 0], [0, np.inf, 0], [np.nan] * 3, [1.23, -4.56, -np.inf]]
    out.append(_vox_case("identical_points_and_nan_rows", p, 0.1, 0,
                         lambda c: _assert(voxel_pcl_keys(c["p"], c["leaf"])[1] == 1 and np.sum(voxel_pcl_keys(c["p"], c["leaf"])[0] < 0) == 4)))
    out.append(_vox_case("every_point_non_finite", [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3, [np.inf] * 3], 0.1, 0,
                         lambda c: _assert(len(voxel_pcl(c["p"], c["leaf"])[0]) == 0)))
    out.append(_vox_case("one_point", [[-3.3, 0.05, 9.99]], 0.1, 0))
    p = rng.uniform(-10, 10, (4097, 3)).astype(F32)
    p[[0, 1, 63, 1024, 2049, 4000, 4096]] = [[np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan], [np.inf, 0, 0], [0, -np.inf, 0], [np.nan] * 3, [0, 0, np.inf]]
    out.append(_vox_case("seven_non_finite_in_4097", p, 0.1, 0, lambda c: _assert(np.sum(voxel_pcl_keys(c["p"], c["leaf"])[0] < 0) == 7)))
    return out


@functools.lru_cache(None)
def voxel_o3d_cases():
    rng = np.random.default_rng(47)
    out = []
    p = rng.uniform(0, 3, (600, 3)).astype(F32)
    p[::5, 0], p[1::7, 1], p[2::11, 2], p[599] = 0, 0, 0, [0, 0, 0]       # points exactly on the minimum bound, on each face and the corner
    out.append(_vox_case("on_the_minimum_bound", p, 0.1, 0, lambda c: _assert((c["p"].min(0) == 0).all() and (voxel_o3d(c["p"], c["leaf"])[1].min(0) == 0).all())))
    out.append(_vox_case("one_point", [[-3.3, 0.05, 9.99]], 0.1, 0))
    out.append(_vox_case("identical_points", np.tile(np.array([[1.23, -4.56, 7.89]], F32), (100, 1)), 0.1, 0,
                         lambda c: _assert(len(voxel_o3d(c["p"], c["leaf"])[0]) == 1)))
    k = rng.integers(0, 12, (500, 3))
    p = np.where(k == 0, 0.0, k * 0.5 - 0.25)                              # (p - (0 - 0.25)) / 0.5 = k exactly
    p[0] = 0

    def pre_int(c):
        x = c["p"].astype(np.float64)
        ref = (x - (x.min(0) - c["leaf"] * 0.5)) / c["leaf"]
        assert (x.min(0) == 0).all() and np.sum(ref == np.floor(ref)) > 1000
        return True
    out.append(_vox_case("exact_integer_coordinates", p, 0.5, 0, pre_int))
    return out
