"""The stable LSD radix sort and the device scans of csrc/sf_sort.hpp, run directly through the test hooks
sf_test_radix_sort / sf_test_scan_u32 and compared EXACTLY with numpy (np.argsort(kind="stable"), uint32 cumsum,
np.maximum.accumulate): no tolerances anywhere.  vals = arange(n) turns any loss of stability into a mismatch of the
sorted values against the reference permutation; the hooks surround every device array with guards and report the
guard words a kernel overwrote.  Sizes sit on and next to the tile boundaries of both instantiations (1024 keys per
tile below 2^20 pairs, 4096 from there on) and next to the switch itself; widths cover single passes, passes narrower
than 8 bits and the calls the library makes (63: the PCL64 voxel grid, 64 keys only: the sorted crop).  No reference
counterpart: the reference sorts inside pcl::VoxelGrid (global_map_frames_manager.cpp:142-146)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL_N = 1 << 20                    # SORT_SMALL_N: below it tiles of 1024 keys, from it on tiles of 4096
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097,
         8 * 1024 - 1, 8 * 1024, 8 * 1024 + 1,      # ntiles % 8 = 0, 0, 1
         13 * 1024 + 5]                             # ntiles = 14: ntiles % 8 = 6
BIG_SIZES = [SMALL_N - 1,                           # 1024 small tiles
             SMALL_N,                               # 256 large tiles
             SMALL_N + 1,                           # 257 large tiles, the last holding one key
             SMALL_N + 7 * 4096 + 3]                # 264 large tiles, the last ragged
WIDTHS32 = [1, 2, 7, 8, 9, 16, 17, 24, 25, 31, 32]
WIDTHS64 = [8, 33, 40, 57, 63, 64]
WIDTHS = [(np.uint32, e) for e in WIDTHS32] + [(np.uint64, e) for e in WIDTHS64]
# around the switch: a single pass, narrow passes (3 x 6), full 32-bit keys, full 64-bit keys
BIG_WIDTHS = [(np.uint32, 8), (np.uint32, 17), (np.uint32, 32), (np.uint64, 64)]
LEADS = [(0, 0), (0, 1), (3, 0), (1, 2)]
DISTS = ["uniform", "zero", "max", "two", "ascending", "descending", "top_digit", "low_digit", "eight_copies", "tile_runs", "seven_largest"]


def passes_bits(end_bit):
    """the pass layout radix_sort_pairs derives from end_bit"""
    passes = (end_bit + 7) // 8
    return passes, (end_bit + passes - 1) // passes


def below(rng, end_bit, size, dtype):
    """uniform keys in [0, 2^end_bit)"""
    if end_bit == 64:
        return rng.integers(0, 1 << 64, size, dtype=np.uint64, endpoint=False).astype(dtype)
    return rng.integers(0, 1 << end_bit, size, dtype=np.uint64).astype(dtype)


def make_keys(rng, dist, n, dtype, end_bit):
    """keys of one distribution, all below 2^end_bit"""
    passes, bits = passes_bits(end_bit)
    top = (1 << end_bit) - 1
    tile = 1024 if n < SMALL_N else 4096
    if dist == "uniform":
        return below(rng, end_bit, n, dtype)
    if dist == "zero":                                   # one digit owns every tile in every pass
        return np.zeros(n, dtype)
    if dist == "max":
        return np.full(n, top, dtype)
    if dist == "two":
        return below(rng, end_bit, 2, dtype)[rng.integers(0, 2, n)]
    if dist == "ascending":
        return np.sort(below(rng, end_bit, n, dtype))
    if dist == "descending":
        return np.sort(below(rng, end_bit, n, dtype))[::-1].copy()
    if dist == "top_digit":                              # only the last pass moves anything
        shift = (passes - 1) * bits
        low = int(below(rng, shift, 1, np.uint64)[0]) if shift else 0
        return ((below(rng, end_bit - shift, n, np.uint64) << np.uint64(shift)) | np.uint64(low)).astype(dtype)
    if dist == "low_digit":                              # only the first pass moves anything
        w = min(bits, end_bit)
        high = (int(below(rng, end_bit, 1, np.uint64)[0]) >> w) << w
        return (below(rng, w, n, np.uint64) | np.uint64(high)).astype(dtype)
    if dist == "eight_copies":                           # the voxel shape: about 8 points per voxel, in random order
        return below(rng, end_bit, max(1, n // 8), dtype)[rng.integers(0, max(1, n // 8), n)]
    if dist == "tile_runs":                              # tile t all one key, tile t + 1 another
        return below(rng, end_bit, n // tile + 1, dtype)[np.arange(n) // tile]
    if dist == "seven_largest":                          # the key of the non-finite points: a few copies of the largest key
        k = below(rng, end_bit, n, dtype)
        k[rng.choice(n, min(7, n), replace=False)] = top
        return k
    raise AssertionError(dist)


def check_sort(api, ctx, keys, end_bit, vals="arange", leads=(0, 0), rng=None, order_by=None, perm=None, what=""):
    """one run of the hook against np.argsort(kind='stable'); order_by: the key bits the order is defined on; perm: that
    reference permutation when the caller already has it"""
    n = len(keys)
    if perm is None:
        perm = np.argsort(keys if order_by is None else order_by, kind="stable")
    if vals == "arange":
        v = np.arange(n, dtype=np.uint32)
    elif vals == "random":
        v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    else:
        v = None
    got_k, got_v, damage = api.hook_radix_sort(ctx, keys, v, end_bit, leads[0], leads[1])
    assert damage == 0, (what, "guard words overwritten", damage)
    assert got_k.dtype == keys.dtype and np.array_equal(got_k, keys[perm]), (what, "keys")
    if v is not None:
        assert np.array_equal(got_v, v[perm]), (what, "values: stability or pairing")


@pytest.mark.parametrize("dtype,end_bit", WIDTHS, ids=lambda p: getattr(p, "__name__", str(p)))
def test_sort_every_size_and_distribution(api, ctx, dtype, end_bit):
    """the full product of the sizes up to 13 k x every distribution, for one key width"""
    rng = np.random.default_rng(1000 + end_bit + (64 if dtype is np.uint64 else 0))
    for n in SIZES:
        for dist in DISTS:
            check_sort(api, ctx, make_keys(rng, dist, n, dtype, end_bit), end_bit, what=(n, dist))
        keys = make_keys(rng, "eight_copies", n, dtype, end_bit)
        check_sort(api, ctx, keys, end_bit, vals="random", rng=rng, what=(n, "random values"))   # a mispairing cannot hide behind the identity
        check_sort(api, ctx, keys, end_bit, vals=None, what=(n, "keys only"))


@pytest.mark.parametrize("n", BIG_SIZES)
@pytest.mark.parametrize("dtype,end_bit", BIG_WIDTHS, ids=lambda p: getattr(p, "__name__", str(p)))
def test_sort_across_the_small_to_large_switch(api, ctx, dtype, end_bit, n):
    """both instantiations right at SORT_SMALL_N; the 64-bit width runs keys only as well (the crop's call)"""
    rng = np.random.default_rng(n + end_bit)
    for dist in DISTS:
        check_sort(api, ctx, make_keys(rng, dist, n, dtype, end_bit), end_bit, what=(n, dist))
    keys = make_keys(rng, "eight_copies", n, dtype, end_bit)
    check_sort(api, ctx, keys, end_bit, vals="random", rng=rng, what=(n, "random values"))
    check_sort(api, ctx, keys, end_bit, vals=None, what=(n, "keys only"))


@pytest.mark.parametrize("n", [4096, 4097, SMALL_N, SMALL_N + 1])
@pytest.mark.parametrize("dtype,end_bit", [(np.uint32, 17), (np.uint64, 33)], ids=["uint32", "uint64"])
def test_sort_alignment_of_either_buffer(api, ctx, dtype, end_bit, n):
    """k_sort_hist loads 16 bytes per lane from an aligned full tile and element by element otherwise: with (0, 1) the
    passes alternate between the two branches, with (3, 0) the other way round, with (1, 2) uint32 keys never take the
    vector branch and uint64 keys take it in every other pass"""
    rng = np.random.default_rng(n + end_bit)
    for dist in ("uniform", "eight_copies", "zero"):
        keys = make_keys(rng, dist, n, dtype, end_bit)
        perm = np.argsort(keys, kind="stable")                                            # one reference for the four placements
        for leads in LEADS:
            check_sort(api, ctx, keys, end_bit, leads=leads, perm=perm, what=(leads, dist))
            if dist == "uniform":
                check_sort(api, ctx, keys, end_bit, vals=None, leads=leads, perm=perm, what=(leads, "keys only"))


HIGH_BIT_WIDTHS = [(d, e) for d, e in WIDTHS if passes_bits(e)[0] * passes_bits(e)[1] < 8 * np.dtype(d).itemsize]


@pytest.mark.parametrize("dtype,end_bit", HIGH_BIT_WIDTHS, ids=lambda p: getattr(p, "__name__", str(p)))
def test_sort_orders_by_passes_times_bits_and_carries_keys_whole(api, ctx, dtype, end_bit):
    """The contract as the code keeps it: the order is the stable order of key & (2^(passes x bits) - 1) -- up to 7 bits
    more than end_bit --, bits above that are carried along and ignored."""
    passes, bits = passes_bits(end_bit)
    pb = passes * bits
    rng = np.random.default_rng(2000 + end_bit)
    for n in (257, 4097, 13 * 1024 + 5) + ((SMALL_N + 1,) if end_bit in (9, 33) else ()):
        low = below(rng, pb, n, np.uint64) if n < SMALL_N else below(rng, pb, n // 8, np.uint64)[rng.integers(0, n // 8, n)]
        garbage = (below(rng, 64, n, np.uint64) >> np.uint64(pb)) << np.uint64(pb)
        keys = (low | garbage).astype(dtype)
        assert (keys >> dtype(pb)).any()
        check_sort(api, ctx, keys, end_bit, order_by=keys & dtype((1 << pb) - 1), what=(n, "garbage above passes x bits"))


def test_sort_fuzz(api, ctx):
    """Seeded fuzz over (n <= 20 000, key width, end_bit, distribution, leads, values); SF_FUZZ_TRIALS / SF_FUZZ_SEED override
    the defaults."""
    rng = np.random.default_rng(int(os.environ.get("SF_FUZZ_SEED", "31")))
    for trial in range(int(os.environ.get("SF_FUZZ_TRIALS", "150"))):
        dtype = (np.uint32, np.uint64)[int(rng.integers(0, 2))]
        end_bit = int(rng.integers(1, 8 * np.dtype(dtype).itemsize + 1))
        n = int(rng.integers(0, 20_001))
        dist = DISTS[int(rng.integers(0, len(DISTS)))]
        leads = (int(rng.integers(0, 4)), int(rng.integers(0, 4)))
        vals = ("arange", "random", None)[int(rng.integers(0, 3))]
        check_sort(api, ctx, make_keys(rng, dist, n, dtype, end_bit), end_bit, vals=vals, leads=leads, rng=rng,
                   what=(trial, dtype.__name__, end_bit, n, dist, leads, vals))


# ------------------------------------------------------------------ scans
SCAN_TILE = 4096
SCAN_SIZES = [1, 63, 64, 65, 4095, 4096, 4097,
              256 * SCAN_TILE - 1, 256 * SCAN_TILE, 256 * SCAN_TILE + 1,    # k_scan_tiles walks the tile sums 256 at a time: one chunk, one chunk, two
              2 * 256 * SCAN_TILE + 4097]                                   # three chunks, the last tile ragged
CARRIES = [0, 5, (1 << 32) - 1]


def scan_inputs(rng, op, n):
    flags = rng.integers(0, 2, n, dtype=np.uint64).astype(np.uint32)                       # head flags
    words = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)                 # full range: the sums wrap
    if op == 0:
        return [("flags", flags), ("random words", words)]
    tails = np.zeros(n, np.uint32)                                                         # cell ends: mostly zeros, the rest ascending
    at = np.flatnonzero(rng.random(n) < 0.1)
    tails[at] = np.sort(rng.integers(1, 1 << 31, len(at), dtype=np.uint64)).astype(np.uint32)
    return [("flags", flags), ("cell tails", tails), ("random words", words)]


def scan_reference(op, a, carry0):
    if op == 0:
        excl = np.zeros(len(a), np.uint32)
        np.cumsum(a[:-1], dtype=np.uint32, out=excl[1:])
        return excl + np.full(1, carry0, np.uint32)                                        # uint32 arrays: wraps like the device
    return np.maximum(np.uint32(carry0), np.maximum.accumulate(a))


@pytest.mark.parametrize("n", SCAN_SIZES)
@pytest.mark.parametrize("op", [0, 1], ids=["sum", "max"])
def test_scan_matches_numpy(api, ctx, op, n):
    rng = np.random.default_rng(3000 + n + op)
    for name, a in scan_inputs(rng, op, n):
        for carry0 in CARRIES:
            want = scan_reference(op, a, carry0)
            for in_place in (False, True):
                got, damage = api.hook_scan_u32(ctx, op, a, carry0, in_place)
                assert damage == 0, (name, carry0, in_place, "guard words overwritten", damage)
                assert got.dtype == np.uint32 and np.array_equal(got, want), (name, carry0, in_place)


def test_scan_of_nothing(api, ctx):
    for op in (0, 1):
        got, damage = api.hook_scan_u32(ctx, op, np.zeros(0, np.uint32), 7, False)
        assert len(got) == 0 and damage == 0


# ------------------------------------------------------------------ arguments
SENTINEL = 0x5EED5EED


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_bad_arguments_are_refused_and_touch_nothing(api, ctx):
    lib = api.load_library()
    n = 100
    k32 = np.arange(n, dtype=np.uint32)[::-1].copy()
    k64 = k32.astype(np.uint64)
    vals = np.arange(n, dtype=np.uint32)
    cap = 1 << 26

    def sort_call(key_bytes=4, keys=k32, v=vals, count=n, end_bit=8, lead=0, lead_alt=0, keys_out=True, vals_out=True, damage=True, handle=ctx.h):
        ko = np.full(n, SENTINEL, np.uint64)
        vo = np.full(n, SENTINEL, np.uint32)
        dmg = C.c_int64(SENTINEL)
        rc = lib.sf_test_radix_sort(handle, key_bytes, _ptr(keys), _ptr(v), count, end_bit, lead, lead_alt, _ptr(ko) if keys_out else None, _ptr(vo) if vals_out else None,
                                    C.addressof(dmg) if damage else None)
        return rc, ko, vo, dmg.value

    def scan_call(op=0, a=vals, count=n, out=True, damage=True, handle=ctx.h):
        o = np.full(n, SENTINEL, np.uint32)
        dmg = C.c_int64(SENTINEL)
        rc = lib.sf_test_scan_u32(handle, op, _ptr(a), count, 0, 0, _ptr(o) if out else None, C.addressof(dmg) if damage else None)
        return rc, o, dmg.value

    bad_sorts = [dict(key_bytes=3), dict(key_bytes=0), dict(key_bytes=16), dict(end_bit=0), dict(end_bit=33), dict(key_bytes=8, keys=k64, end_bit=65),
                 dict(lead=-1), dict(lead=4), dict(lead_alt=-1), dict(lead_alt=4), dict(count=-1), dict(count=cap + 1), dict(keys=None), dict(keys_out=False),
                 dict(vals_out=False), dict(v=None), dict(damage=False), dict(handle=None)]
    for kw in bad_sorts:
        rc, ko, vo, dmg = sort_call(**kw)
        assert rc == -1, (kw, rc)                                                          # SF_ERR_INVALID
        assert lib.sf_last_error(), kw
        assert (ko == SENTINEL).all() and (vo == SENTINEL).all() and dmg == SENTINEL, kw
    for kw in [dict(op=2), dict(op=-1), dict(count=-1), dict(count=cap + 1), dict(a=None), dict(out=False), dict(damage=False), dict(handle=None)]:
        rc, o, dmg = scan_call(**kw)
        assert rc == -1, (kw, rc)
        assert lib.sf_last_error(), kw
        assert (o == SENTINEL).all() and dmg == SENTINEL, kw
    # a good call after the refusals
    rc, ko, vo, dmg = sort_call()
    assert rc == 0 and dmg == 0 and np.array_equal(ko.view(np.uint32)[:n], k32[::-1]) and np.array_equal(vo, vals[::-1])
    rc, ko, vo, dmg = sort_call(key_bytes=8, keys=k64, end_bit=64)
    assert rc == 0 and dmg == 0 and np.array_equal(ko, k64[::-1]) and np.array_equal(vo, vals[::-1])
    rc, o, dmg = scan_call()
    assert rc == 0 and dmg == 0 and np.array_equal(o, scan_reference(0, vals, 0))
    # n = 0 and n = 1: the output is the input, whatever end_bit says
    for count in (0, 1):
        rc, ko, vo, dmg = sort_call(count=count, end_bit=0)
        assert rc == 0 and dmg == 0 and np.array_equal(ko.view(np.uint32)[:count], k32[:count]) and np.array_equal(vo[:count], vals[:count])
        assert (vo[count:] == SENTINEL).all()
