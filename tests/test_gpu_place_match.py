"""The Scan Context match and selection on the device (sf_place_db_distances, sf_place_db_query) against the numpy
restatement of the rule (tests/place_ref_np.py): D and shift of every pair, then the top-k.  Integers and the order compare exactly,
distances bit for bit: the rule uses IEEE add, multiply and divide and a correctly rounded square root only."""
import numpy as np
import pytest

import place_fixtures as fx
import place_ref_np as ref

pytestmark = pytest.mark.gpu

INVALID = "error -1:"
DEFAULT = (20, 60)


def database(api, ctx, shape, entries, poses=None):
    db = api.PlaceDB(ctx, num_rings=shape[0], num_sectors=shape[1])
    if len(entries):
        db.add_descriptors(entries, poses)
    assert len(db) == len(entries)
    return db


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def check(db, queries, entries, poses, ks, what):
    """distances and the top-k of `queries` against the restatement -> (D, shift) of the restatement"""
    shape = db.shape
    want_d, want_s = ref.distances(queries, entries)
    dist, shift, st = db.distances(queries)
    assert dist.dtype == np.float64 and shift.dtype == np.int32, what
    assert np.array_equal(shift, want_s), what
    assert same_bits(dist, want_d), (what, np.abs(dist - want_d).max() if dist.size else 0.0)
    assert st["n_queries"] == len(queries) and st["n_entries"] == len(entries) and st["match_ms"] >= 0.0, what
    for k in ks:
        got, want = db.query(queries, k), ref.top_k(want_d, want_s, k, poses, shape[1])
        assert np.array_equal(got["idx"], want["idx"]) and np.array_equal(got["shift"], want["shift"]) and same_bits(got["dist"], want["dist"]), (what, k)
        if poses is not None:
            assert np.abs(got["poses"] - want["poses"]).max() <= 1e-12, (what, k)
        if k > len(entries):
            assert (got["idx"][:, len(entries):] == -1).all() and np.isposinf(got["dist"][:, len(entries):]).all() and not got["poses"][:, len(entries):].any(), (what, k)
    return want_d, want_s


@pytest.mark.parametrize("n", fx.DB_SIZES)
def test_every_database_size(api, ctx, n):
    """the tails of a four-pairs-a-block mapping and of the growth by doubling; k = 5 runs past the smaller ones"""
    entries, poses, queries = fx.rows(n, DEFAULT), fx.entry_poses(n), fx.rows(3, DEFAULT, seed=1)
    db = database(api, ctx, DEFAULT, entries, poses if n else None)
    check(db, queries, entries, poses, (1, 5), n)
    check(db, queries[:1], entries, poses, (5,), (n, "one query"))
    desc, got_poses = db.download()
    assert np.array_equal(desc, entries) and np.array_equal(got_poses, poses)


@pytest.mark.parametrize("shape", fx.SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_shape(api, ctx, shape):
    entries, poses = fx.rows(65, shape), fx.entry_poses(65)
    db = database(api, ctx, shape, entries, poses)
    check(db, fx.rows(3, shape, seed=1), entries, poses, (1, 5, 32), shape)
    check(db, fx.rows(1, shape, seed=2), entries, poses, (32,), (shape, "one query"))
    small = database(api, ctx, shape, entries[:5], poses[:5])
    check(small, fx.rows(64, shape, seed=3), entries[:5], poses[:5], (5, 32), (shape, "64 queries"))


def test_sixty_four_queries(api, ctx):
    entries, poses = fx.rows(65, DEFAULT), fx.entry_poses(65)
    db = database(api, ctx, DEFAULT, entries, poses)
    check(db, fx.rows(64, DEFAULT, seed=4), entries, poses, (1, 32), "64 x 65")
    check(db, fx.rows(63, DEFAULT, seed=5), entries, poses, (5,), "63 x 65")   # an odd count: the last block of queries is half full


def test_engineered_rows(api, ctx):
    Nr, Ns = DEFAULT
    base = fx.rows(4, DEFAULT, seed=6)
    q = base[1]
    flat = np.repeat(base[2][:, :1], Ns, axis=1)                               # every column the same: every shift gives the same bits
    rolled = np.stack([np.roll(q, s, axis=1) for s in range(Ns)])              # entry column (j + s) mod Ns = query column j
    entries = np.concatenate([np.stack([base[0], q, base[0], np.zeros(DEFAULT, np.float32), flat, q]), rolled])
    db = database(api, ctx, DEFAULT, entries)
    # an all-zero query: every D = 1, shift 0, and the top-k is the first entries
    d, s = check(db, np.zeros((1,) + DEFAULT, np.float32), entries, None, (5,), "zero query")
    assert (d == 1.0).all() and (s == 0).all()
    d, s = check(db, np.stack([q, flat]), entries, None, (8,), "engineered")
    assert d[0, 3] == 1.0 and s[0, 3] == 0                                     # an all-zero entry
    assert s[1, 4] == 0 and abs(d[1, 4]) < 1e-15                               # all columns equal: the smallest shift of the tie
    assert np.array_equal(s[0, 6:], np.arange(Ns)) and (np.abs(d[0, 6:]) < 1e-15).all()     # the rolled copies at every s
    got = db.query(q[None], 8)
    same = [1, 5] + list(range(6, 6 + Ns))                                     # the query itself twice and its rolled copies: bitwise ties ...
    assert len(set(got["dist"][0, :8].tolist())) == 1 and got["idx"][0].tolist() == same[:8]   # ... the smaller index first
    got = db.query(base[0][None], 2)
    assert got["idx"][0].tolist() == [0, 2] and got["dist"][0, 0] == got["dist"][0, 1]          # duplicated entries


def test_one_at_a_time_and_in_bulk_and_two_databases(api, ctx):
    entries, poses, queries = fx.rows(65, DEFAULT), fx.entry_poses(65), fx.rows(3, DEFAULT, seed=1)
    bulk = database(api, ctx, DEFAULT, entries, poses)
    single = api.PlaceDB(ctx, num_rings=DEFAULT[0], num_sectors=DEFAULT[1])
    for k in range(65):                                                        # 16 -> 32 -> 64 -> 128: what the database held is carried over
        single.add_descriptors(entries[k], poses[k:k + 1])
    other_entries = fx.rows(5, (3, 7))
    other = database(api, ctx, (3, 7), other_entries)                          # a second database on the same context, another shape
    other_q = fx.rows(3, (3, 7), seed=1)
    want_other = ref.distances(other_q, other_entries)
    for _ in range(2):                                                         # queried in alternation
        a, b = bulk.distances(queries), single.distances(queries)
        c = other.distances(other_q)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        assert same_bits(c[0], want_other[0]) and np.array_equal(c[1], want_other[1])
    qa, qb = bulk.query(queries, 5), single.query(queries, 5)
    assert all(qa[key].tobytes() == qb[key].tobytes() for key in ("idx", "dist", "shift", "poses"))
    assert np.array_equal(single.download()[0], entries) and np.array_equal(single.download()[1], poses)
    single.clear()
    assert len(single) == 0 and single.distances(queries)[0].shape == (3, 0)
    single.add_descriptors(entries[:2])
    assert same_bits(single.distances(queries)[0], a[0][:, :2])


def test_the_error_cases(api, ctx):
    entries, queries = fx.rows(5, DEFAULT), fx.rows(3, DEFAULT, seed=1)
    db = database(api, ctx, DEFAULT, entries)
    before = db.distances(queries)
    for value in (-1.0, np.nan, np.inf):
        bad = entries[:2].copy()
        bad[1, 3, 4] = value
        with pytest.raises(api.SlamFusionError, match=INVALID):
            db.add_descriptors(bad)
        with pytest.raises(api.SlamFusionError, match=INVALID):
            db.distances(bad)
        with pytest.raises(api.SlamFusionError, match=INVALID):
            db.query(bad, 1)
    for k in (0, -1, 33):
        with pytest.raises(api.SlamFusionError, match=INVALID):
            db.query(queries, k)
    with pytest.raises(api.SlamFusionError, match=INVALID):
        db.distances(fx.rows(65, DEFAULT))                                     # more than 64 queries
    with pytest.raises(api.SlamFusionError, match=INVALID):
        db.distances(np.zeros((0,) + DEFAULT, np.float32))
    bad_pose = np.stack([np.eye(4), np.eye(4)])
    bad_pose[1, 0, 3] = np.nan
    with pytest.raises(api.SlamFusionError, match=INVALID):
        db.add_descriptors(entries[:2], bad_pose)
    after = db.distances(queries)
    assert len(db) == 5 and before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()    # nothing touched
    assert db.query(queries, 32)["idx"].shape == (3, 32)
