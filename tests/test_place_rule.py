"""The numpy restatement of the Scan Context rule (tests/place_ref_np.py; include/slamfusion.h) pinned to facts it
was not built from, the edge condition of every cloud the GPU tests compare exactly (tests/place_fixtures.py), and the gaps of the
city fixtures.  No device call."""
import numpy as np
import pytest

import place_fixtures as fx
import place_ref_np as ref


def test_a_single_point_lands_in_the_bin_computed_by_hand():
    """(3, 4, 1.5): rho = 5 of 80 m in 20 rings -> ring 1 (1.25); az = atan2(4, 3) = 53.13 degrees, (53.13 + 180) / 6 = 38.86 -> sector
    38; height 1.5 + 2"""
    desc, st = ref.descriptor(np.array([[3.0, 4.0, 1.5]], np.float32), None, ref.default_params())
    assert desc.shape == (20, 60) and desc.dtype == np.float32
    assert np.argwhere(desc != 0).tolist() == [[1, 38]] and desc[1, 38] == 3.5
    assert st == dict(n_points=1, n_nonfinite=0, n_outside=0, n_below=0, n_binned=1, n_filled=1)
    # seen from a sensor standing at (10, 0, 1) and facing +y, the same point is 7 m behind and 4 m to the right ... (x, y) = (4, 7)
    T = fx.yaw_pose(90.0, (10.0, 0.0, 1.0))
    desc, _ = ref.descriptor(np.array([[3.0, 4.0, 1.5]], np.float32), T, ref.default_params())
    ring, col = np.argwhere(desc != 0)[0]
    assert ring == int(np.hypot(4.0, 7.0) / 4.0) == 2 and col == int((np.degrees(np.arctan2(7.0, 4.0)) + 180.0) / 6.0) == 40 and desc[ring, col] == 2.5
    # the classes: beyond max_range, nearer than min_range, on the ground, not finite
    pts = np.array([[80.0, 0, 1], [0.3, 0, 1], [5, 5, -2.0], [5, 5, -3.0], [np.nan, 0, 0], [79.9, 0, 1]], np.float32)
    desc, st = ref.descriptor(pts, None, ref.default_params())
    assert st == dict(n_points=6, n_nonfinite=1, n_outside=2, n_below=2, n_binned=1, n_filled=1) and desc[19, 30] == 3.0


def test_a_quarter_turn_of_the_sensor_is_a_quarter_of_the_sectors():
    """the sensor turned by +90 degrees about z where it stood: shift Ns / 4, not 3 Ns / 4; the candidate pose is the query's pose"""
    prm = ref.default_params(max_range=40.0)
    world = fx.disc(4000, 31, rho_hi=39.0, z_lo=-1.0, z_hi=12.0)
    entry, _ = ref.descriptor(world, None, prm)
    turned = fx.yaw_pose(90.0, (0.0, 0.0, 0.0))
    query, _ = ref.descriptor(world, turned, prm)                       # the same world seen by the turned sensor
    D, shift = ref.distances(query[None], entry[None])
    assert shift[0, 0] == 15 and D[0, 0] < 1e-15
    assert np.array_equal(query, np.roll(entry, -15, axis=1))            # what stood at sector j + 15 stands at j now
    assert np.abs(ref.candidate_pose(np.eye(4), 15, 60) - turned).max() < 1e-15
    back, _ = ref.descriptor(world, fx.yaw_pose(-90.0, (0.0, 0.0, 0.0)), prm)
    assert ref.distances(back[None], entry[None])[1][0, 0] == 45


@pytest.mark.parametrize("shape", fx.SHAPES, ids=lambda s: "%dx%d" % s)
def test_a_rolled_descriptor_is_found_at_its_shift(shape):
    a = fx.rows(2, shape, seed=9)[1] + np.float32(1.0)                 # (no empty bin: the 1 x 1 row is not all zero)
    for s in range(shape[1]):
        D, shift = ref.distances(a[None], np.roll(a, s, axis=1)[None])
        assert D[0, 0] < 1e-15 and (shift[0, 0] == s or shape[1] == 1), (shape, s)


def test_the_distance_against_a_dense_formulation():
    """d(s) = 1 - mean over the valid column pairs of the cosine between the columns, written with einsum and np.roll"""
    rows = fx.rows(10, (20, 60), seed=2)                                 # rows 0 and 5 have all-zero columns
    D, shift = ref.distances(rows, rows)
    a = rows.astype(np.float64)
    norm = np.sqrt((a * a).sum(axis=1))                                  # [n, Ns]
    unit = np.divide(a, norm[:, None, :], out=np.zeros_like(a), where=norm[:, None, :] > 0)
    valid = norm > 0
    for q in range(10):
        dense = np.empty((10, 60))
        for s in range(60):
            uc, vc = np.roll(unit, -s, axis=2), np.roll(valid, -s, axis=1)            # column j of the rolled entry = column j + s
            cos = np.einsum("ij,cij->cj", unit[q], uc)
            both = valid[q][None, :] & vc
            dense[:, s] = 1.0 - (cos * both).sum(axis=1) / both.sum(axis=1)
        assert np.abs(dense.min(axis=1) - D[q]).max() < 1e-13
        assert np.array_equal(np.argmin(np.round(dense, 12), axis=1), shift[q])
    assert (np.abs(np.diag(D)) < 1e-15).all() and (np.diag(shift) == 0).all()


def test_all_zero_columns_are_skipped_and_counted_out():
    a = np.zeros((3, 4), np.float32)
    a[:, 0], a[:, 2] = (1, 2, 2), (3, 0, 4)
    u, valid = ref.unit_columns(a)
    assert valid.tolist() == [True, False, True, False] and np.array_equal(u[:, 0], np.array([1, 2, 2]) / 3.0) and np.array_equal(u[:, 2], np.array([3, 0, 4]) / 5.0)
    assert not u[:, 1].any() and not u[:, 3].any()
    b = np.zeros((3, 4), np.float32)
    b[:, 0] = (1, 2, 2)                                                  # one valid column, the same as a's column 0
    d = ref.shift_distances(*[x[None] for x in ref.unit_columns(b) + ref.unit_columns(a)])[0, 0]
    # s = 0: b0 . a0 = 1 over V = 1; s = 2: b0 . a2 = (3 + 8) / 15 over V = 1; s = 1, 3: b0 meets an all-zero column, V = 0: exactly 1
    assert d[0] == 0.0 and d[1] == 1.0 and d[3] == 1.0 and abs(d[2] - (1.0 - 11.0 / 15.0)) < 1e-15
    assert ref.distances(np.zeros((1, 3, 4), np.float32), a[None])[0][0, 0] == 1.0 and ref.distances(a[None], np.zeros((1, 3, 4), np.float32))[1][0, 0] == 0
    # V counts pairs, not columns of the query: a against itself has two pairs at s = 0 and s = 2, none at s = 1, 3
    d = ref.shift_distances(*[x[None] for x in ref.unit_columns(a) + ref.unit_columns(a)])[0, 0]
    assert abs(d[0]) < 1e-15 and d[1] == 1.0 and d[3] == 1.0 and abs(d[2] - (1.0 - 11.0 / 15.0)) < 1e-15


def test_the_top_k_orders_by_distance_then_index():
    D = np.array([[0.5, 0.25, 0.5, 0.25, 0.75]])
    shift = np.array([[1, 2, 3, 4, 5]], np.int32)
    got = ref.top_k(D, shift, 7)
    assert got["idx"].tolist() == [[1, 3, 0, 2, 4, -1, -1]] and got["shift"].tolist() == [[2, 4, 1, 3, 5, 0, 0]]
    assert got["dist"][0, :5].tolist() == [0.25, 0.25, 0.5, 0.5, 0.75] and np.isposinf(got["dist"][0, 5:]).all()


def test_no_fixture_has_a_point_on_a_sector_edge():
    cases = fx.build_cases()
    assert len(cases) > 40
    for name, pts, T, prm in cases:
        assert ref.edge_distance(pts, T, prm) > 1e-9, name


def test_the_city_finds_its_keyframes_with_room_to_spare():
    c = fx.city()
    keyframes, queries, near = fx.city_descriptors()
    assert len(keyframes) == 15 and c["query_shifts"] == (15, 37, 1)
    all_q = np.concatenate([queries, near[None]])
    truth = list(zip(c["query_keyframes"], c["query_shifts"])) + [(c["near_keyframe"], c["near_shift"])]
    D, shift = ref.distances(all_q, keyframes)
    uk = [ref.unit_columns(k) for k in keyframes]
    for q, (kf, s) in enumerate(truth):
        order = np.argsort(D[q], kind="stable")
        assert order[0] == kf and shift[q, kf] == s, q
        assert D[q, order[1]] - D[q, order[0]] > 1e-3, q                  # the runner-up keyframe
        d = np.sort(ref.shift_distances(*[x[None] for x in ref.unit_columns(all_q[q]) + uk[kf]])[0, 0])
        assert d[1] - d[0] > 1e-3, q                                      # the runner-up shift
        gaps = np.diff(np.sort(D[q]))[:4]
        assert gaps.min() > 1e-9, q                                       # the top 5 of the query are apart: their order is no matter of rounding
    off = [np.linalg.norm(T[:2, 3] - c["poses"][kf][:2, 3]) for T, kf in zip(c["query_poses"], c["query_keyframes"])]
    assert 0.9 - 1e-12 <= min(off) and max(off) <= 1.61                   # (30.9 - 30 is one rounding short of 0.9)
