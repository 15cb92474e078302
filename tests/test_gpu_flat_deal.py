"""Flat rounds of the wave search (sf_nn.hpp, nn_search_wave): the ring-1 candidates of a round are laid end to end and
dealt out over the 64 lanes instead of one range per lane.  The clouds here are made to stress the dealing -- clumps far
denser than a cell of a coarse 0.45 m index (a round's ranges run to hundreds of candidates: many trips per round, ranges
that cross trips), exact duplicates (index ties) and queries on cell faces -- and the result must still be the exact
1-NN: the same squared distance as a brute-force float32 search, to the bit.  The runner-up bound that the flat rounds
fold per candidate is checked through the neighbour-reuse certificate, the one thing that reads it: alignments that
reuse neighbours must form bit-for-bit the pairs of alignments that search every query."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CELL = 0.45


def dense_cloud(seed):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0.0, 12.0, size=(150, 3)).astype(np.float32)
    centres[:, 2] *= 0.25
    clumps = centres[rng.integers(0, len(centres), 24_000)] + rng.normal(0.0, 0.04, size=(24_000, 3)).astype(np.float32)
    sparse = rng.uniform(0.0, 12.0, size=(6_000, 3)).astype(np.float32) * np.float32([1.0, 1.0, 0.25])
    pts = np.concatenate([clumps, sparse]).astype(np.float32)
    pts = np.concatenate([pts, pts[rng.integers(0, len(pts), 3_000)]])   # exact duplicates: ties on d2, settled by index
    pts = np.abs(pts)
    pts[0] = 0.0                                                        # the grid origin at 0: cell faces at k * CELL
    return pts.astype(np.float32)


def l2_simple_min(q, p, chunk=64):
    """min over p of ((dx*dx) + dy*dy) + dz*dz in float32, unfused (numpy rounds every operation)."""
    out = np.empty(len(q), np.float32)
    for s in range(0, len(q), chunk):
        d = q[s:s + chunk, None, :] - p[None, :, :]
        r = d[..., 0] * d[..., 0]
        r = r + d[..., 1] * d[..., 1]
        r = r + d[..., 2] * d[..., 2]
        out[s:s + chunk] = r.min(axis=1)
    return out


def queries(pts, seed):
    rng = np.random.default_rng(seed)
    near = pts[rng.integers(0, len(pts), 3_000)] + rng.normal(0.0, 0.05, size=(3_000, 3)).astype(np.float32)
    on_points = pts[rng.integers(0, len(pts), 500)]                      # distance 0, duplicates among them
    faces = rng.uniform(0.0, 12.0, size=(1_500, 3)).astype(np.float32) * np.float32([1.0, 1.0, 0.25])
    ax = rng.integers(0, 3, len(faces))
    faces[np.arange(len(faces)), ax] = np.round(faces[np.arange(len(faces)), ax] / CELL).astype(np.float32) * np.float32(CELL)
    return np.concatenate([near, on_points, faces]).astype(np.float32)


@pytest.mark.parametrize("seed", [3, 17])
def test_dense_cells_duplicates_and_faces_give_the_exact_neighbour(api, ctx, seed):
    pts = dense_cloud(seed)
    q = queries(pts, seed + 1)
    mp = api.Map(ctx, api.Cloud(ctx, pts), CELL)
    for max_d2 in (np.inf, 0.04):
        idx, d2 = mp.nn(q, max_d2)
        ref = l2_simple_min(q, pts)
        hit = ref < np.float32(max_d2) if np.isfinite(max_d2) else np.ones(len(q), bool)
        assert np.array_equal(idx >= 0, hit)
        assert np.array_equal(d2[hit], ref[hit])
        assert np.all(np.isinf(d2[~hit]))
        # the index names a point at exactly that distance (which duplicate it is, is the index rule's business)
        d = q[hit] - pts[idx[hit]]
        own = d[:, 0] * d[:, 0]
        own = own + d[:, 1] * d[:, 1]
        own = own + d[:, 2] * d[:, 2]
        assert np.array_equal(own, ref[hit])


@pytest.mark.parametrize("mode", ["p2plane", "o3d_p2p"])
def test_reuse_certificate_holds_on_dense_cells(api, ctx, synth, mode):
    pts = dense_cloud(5)
    mp = api.Map(ctx, api.Cloud(ctx, pts), CELL)
    mp.estimate_normals(0.25)
    rng = np.random.default_rng(6)
    scans = np.stack([pts[rng.choice(len(pts), 9_000, replace=False)] + rng.normal(0.0, 0.01, size=(9_000, 3)).astype(np.float32)
                      for _ in range(3)]).astype(np.float32)
    inits = np.stack([synth.make_T((0.03 * k, -0.02, 0.01), (0.0, 0.01, 0.2 * k)) for k in range(3)])
    keys = ("iterations", "converged", "n_corr", "flags", "rmse", "fitness")
    out = []
    for reuse in (False, True):
        icp = api.Icp(ctx, 0.5, 15, 0.05, 1e-5)
        icp.use_graph(False)
        icp.set_nn_reuse(reuse)
        icp.set_target(mp)
        icp.set_source_batch(scans)
        icp.set_initial_batch(inits)
        out.append(icp.align_batch(mode))
    for a, b in zip(*out):
        assert np.array_equal(a["T64"], b["T64"]) and all(a[k] == b[k] for k in keys), mode
