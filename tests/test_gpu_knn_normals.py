"""sf_map_estimate_normals_knn against a float64 restatement of its rule: the neighbourhood of map point i is the
k-NN list of its own float32 coordinates (the rule of tests/test_gpu_knn.py, max_d2 = float32(max_radius^2) or inf, no window),
the sums run over the list positions 0..63 in a pairwise tree with absent positions as +0.0."""
import numpy as np
import pytest

from test_gpu_knn import knn_ref, mixed_map

pytestmark = pytest.mark.gpu


def tree(v):
    """[n, 64] -> [n]: ((v0 + v1) + (v2 + v3)) + ..."""
    while v.shape[1] > 1:
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def normals_ref(mp, k, max_radius=np.inf):
    """-> cnt [n], C [n, 6] (centred sums xx xy xz yy yz zz), cov6 [n, 6], all in ORIGINAL point order"""
    pts4 = mp.index()["pts4"]
    P = np.ascontiguousarray(pts4[:, :3])
    ids = pts4[:, 3].view(np.uint32).astype(np.int64)
    r = np.float32(max_radius)
    max_d2 = np.float32(r * r) if np.isfinite(r) and r > 0 else np.inf
    pos, _, cnt = knn_ref(mp, P, k, max_d2, positions=True)
    n = len(P)
    have = np.arange(64)[None, :] < cnt[:, None]
    nb = np.zeros((n, 64, 3), np.float64)
    nb[:, :k] = P[np.maximum(pos, 0)].astype(np.float64)
    nb[~have] = 0.0
    safe = np.maximum(cnt, 1).astype(np.float64)
    mean = np.stack([tree(nb[:, :, d]) for d in range(3)], 1) / safe[:, None]
    a = np.where(have[:, :, None], nb - mean[:, None, :], 0.0)
    C = np.stack([tree(a[:, :, i] * a[:, :, j]) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], 1)
    C[cnt < 3] = 0.0
    cov = C / safe[:, None]
    out_cnt, out_C, out_cov = np.empty_like(cnt), np.empty_like(C), np.empty_like(cov)
    out_cnt[ids], out_C[ids], out_cov[ids] = cnt, C, cov
    return out_cnt, out_C, out_cov


@pytest.fixture(scope="module")
def noisy_map():
    rng = np.random.default_rng(31)
    m = mixed_map(rng, 3000, sigma=0.005)
    lone = np.stack([-5.9 + 0.6 * np.arange(20), np.full(20, 7.5), np.full(20, 7.5)], 1).astype(np.float32)   # 0.6 m from each other, 1.5 m from the rest
    return m, np.concatenate([m, lone])


@pytest.mark.parametrize("k,max_radius", [(10, np.inf), (20, np.inf), (20, 0.3), (64, np.inf)])
def test_against_the_float64_restatement(api, ctx, noisy_map, k, max_radius):
    m = noisy_map[1] if np.isfinite(max_radius) else noisy_map[0]
    mp = api.Map(ctx, api.Cloud(ctx, m), 0.25)
    mp.estimate_normals_knn(k, max_radius, covariance=True)
    nrm, cnt = mp.download_normals()
    cov = mp.download_covariances()
    rcnt, rC, rcov = normals_ref(mp, k, max_radius)
    assert np.array_equal(cnt, rcnt), np.flatnonzero(cnt != rcnt)[:5]
    assert cnt.max() <= k and (np.isfinite(max_radius) or cnt.min() == k)
    err = np.abs(cov - rcov).max()
    print("k %d max_radius %g: max |cov6 - ref| %.3e, %d points below 3 neighbours" % (k, max_radius, err, int((cnt < 3).sum())))
    assert err <= 1e-12
    few = cnt < 3
    if np.isfinite(max_radius):
        assert few[-20:].all() and few.sum() > 20
    assert np.array_equal(nrm[few], np.tile(np.array([[0, 0, 1]], np.float32), (int(few.sum()), 1))) and not cov[few].any()
    n64 = nrm.astype(np.float64)
    assert np.abs(np.linalg.norm(n64, axis=1) - 1).max() <= 1e-6
    x, y, z = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    assert ((z > 0) | ((z == 0) & ((y > 0) | ((y == 0) & (x >= 0))))).all()                 # the sign rule of smallest_eigvec
    ok = ~few
    M = np.zeros((len(m), 3, 3))
    for d, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        M[:, i, j] = M[:, j, i] = rC[:, d]
    lam = np.linalg.eigh(M[ok])[0]
    excess = np.einsum("ni,nij,nj->n", n64[ok], M[ok], n64[ok]) - lam[:, 0]
    print("   Rayleigh excess / lambda_max: max %.3e" % (excess / lam[:, 2]).max())
    assert (excess <= 2e-5 * lam[:, 2]).all()
    mp.close()


def test_normals_attach_to_point_to_plane(api, ctx, orc, synth, small_world):
    m, scan = small_world["map"], small_world["scan"]
    mp = api.Map(ctx, api.Cloud(ctx, m), 0.25)
    mp.estimate_normals_knn(20)
    normals, cnt = mp.download_normals()
    assert (cnt == 20).all()
    icp = api.Icp(ctx, 0.5, 20, 0.05, 1e-5)
    icp.set_target(mp)
    icp.set_source(scan)
    r = icp.align("p2plane")
    o = orc.icp_p2plane(scan, m, normals, None, 0.5, 20)
    assert r["iterations"] == o["iterations"] == 20
    dt, dr = synth.pose_error(r["T64"], o["T"])
    assert dt < 1e-9 and dr < 1e-9, (dt, dr)
    dt, dr = synth.pose_error(r["T64"], synth.t_true())
    assert dt < 2e-3 and dr < 2e-4, (dt, dr)                                                 # and it is the right answer
    mp.close()


def test_bitwise_repeatability(api, ctx, noisy_map):
    got = []
    for _ in range(2):
        mp = api.Map(ctx, api.Cloud(ctx, noisy_map[1]), 0.25)
        mp.estimate_normals_knn(20, 0.5, covariance=True)
        got.append(mp.download_normals() + (mp.download_covariances(),))
        mp.close()
    for a, b in zip(*got):
        assert np.array_equal(a.view(np.uint64 if a.dtype == np.float64 else np.uint32), b.view(np.uint64 if b.dtype == np.float64 else np.uint32))


LEAF = 0.1


def _same(mp, ref, cov):
    na, ca = mp.download_normals()
    nb, cb = ref.download_normals()
    assert np.array_equal(na.view(np.uint32), nb.view(np.uint32)) and np.array_equal(ca, cb)
    if cov:
        assert np.array_equal(mp.download_covariances().view(np.uint64), ref.download_covariances().view(np.uint64))


def test_patch_runs_the_knn_estimate_again(api, ctx, synth):
    rng = np.random.default_rng(41)
    prev = api.voxel_merge_min_points(0)
    try:
        base = synth.make_map(150_000)
        inner = base[(np.abs(base[:, 0]) < 5.0) & (np.abs(base[:, 1]) < 5.0)]
        dev = api.Cloud(ctx, inner)
        dev.voxel_downsample(LEAF, "pcl")
        core = inner[(np.abs(inner[:, 0]) < 4.5) & (np.abs(inner[:, 1]) < 4.5) & (np.abs(inner[:, 2]) < 4.5)]
        near = lambda n: (core[rng.choice(len(core), n, replace=False)] + rng.normal(0, 0.004, (n, 3))).astype(np.float32)

        def grow(mp, n=2_000):
            st, merged = dev.voxel_merge(api.Cloud(ctx, near(n)), LEAF)
            assert st == 0 and merged
            return mp.patch(dev)

        def fresh(k, r, cov):
            ref = api.Map(ctx).set_origin_lattice(64).build(dev, 0.25)
            ref.estimate_normals_knn(k, r, cov)
            return ref
        for k, r, cov in ((20, np.inf, True), (10, 0.3, False)):
            mp = api.Map(ctx).set_origin_lattice(64).build(dev, 0.25)
            mp.estimate_normals_knn(k, r, cov)
            mp.set_normals_carry(True)
            assert grow(mp), mp.last_patch                                                   # the index is merged ...
            n = len(dev)
            assert len(mp) == n and mp.normals_carry_info() == (0, 0, n, n)                  # ... the normals estimated again in full
            _same(mp, fresh(k, r, cov), cov)
            if not cov:
                with pytest.raises(api.SlamFusionError):
                    mp.download_covariances()
            # where the patch takes the build: the same
            st, merged = dev.voxel_merge(api.Cloud(ctx, near(500)), LEAF)
            assert merged
            dev.transform(np.eye(4, dtype=np.float32))
            assert not mp.patch(dev)
            n = len(dev)
            assert mp.normals_carry_info() == (0, 0, n, n)
            _same(mp, fresh(k, r, cov), cov)
            mp.close()
        # the switch off: dropped, as for the radius form
        mp = api.Map(ctx).set_origin_lattice(64).build(dev, 0.25)
        mp.estimate_normals_knn(20)
        assert grow(mp) and mp.normals_carry_info()[0] == -1
        with pytest.raises(api.SlamFusionError):
            mp.download_normals()
        # a radius estimate after a k-NN estimate: carried entry by entry again
        mp.estimate_normals_knn(20)
        mp.estimate_normals(0.25)
        mp.set_normals_carry(True)
        assert grow(mp) and mp.normals_carry_info()[0] == 1
        ref = api.Map(ctx).set_origin_lattice(64).build(dev, 0.25)
        ref.estimate_normals(0.25)
        _same(mp, ref, False)
        # ... and set_normals forgets the k-NN estimate
        mp.estimate_normals_knn(20)
        mp.set_normals(np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (len(dev), 1)))
        assert grow(mp) and mp.normals_carry_info()[0] == -1
        mp.close()
    finally:
        api.voxel_merge_min_points(prev)
