"""sf_map_estimate_normals_cov (k_normals -> normals_point, csrc/sf_map.hip) against the numpy restatement of its rule
(tests/normals_ref_np.py: brute force over all pairs, long double sums, numpy.linalg.eigh) on every fixture of that module: the counts
exactly, cov6 and the normals within the bounds derived there, the fallback rows, the rows that are not indexed, the sign rule and the
exact rows bit for bit.  The straddle cases hold pairs within the radius whose cells lie one beyond ceil(radius / cell): each case
checks on the downloaded index that its pairs do straddle, so that none passes by missing its edge."""
import numpy as np
import pytest

import normals_ref_np as nr

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = list(nr.cases())
WORST = dict(cov=0.0, sin=0.0, unit=0.0, rayleigh=0.0)


def build(api, ctx, case):
    mp = api.Map(ctx)
    if case["lattice"]:
        mp.set_origin_lattice(case["lattice"])
    return mp.build(api.Cloud(ctx, case["points"]), case["cell"])


def run(api, ctx, case, covariance=True):
    mp = build(api, ctx, case)
    mp.estimate_normals(case["radius"], covariance=covariance)
    nrm, cnt = mp.download_normals()
    cov = mp.download_covariances() if covariance else None
    return mp, nrm, cnt, cov


@pytest.fixture(scope="module")
def device(api, ctx):
    """name -> (normals, counts, cov6) of the case, estimated once with covariance=True"""
    made = {}

    def get(name):
        if name not in made:
            mp, nrm, cnt, cov = run(api, ctx, nr.cases()[name])
            mp.close()
            made[name] = (nrm, cnt, cov)
        return made[name]
    return get


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def pairs_straddle(api, ctx, case):
    """every pair of a straddle case: within the radius, and in the index as it lies on the device reach_old + 1 cells apart on its axis"""
    mp = build(api, ctx, case)
    ix = mp.index()
    h, dims = mp.cell_size()
    mp.close()
    assert F(h) == F(case["cell"])
    P, radius = case["points"], F(case["radius"])
    R_old = max(1, int(np.ceil(float(radius) / float(F(h)) - 1e-9)))
    ids = ix["pts4"][:, 3].view(np.uint32).astype(np.int64)
    where = np.empty(len(P), np.int64)
    where[ids] = np.arange(len(ids))
    cell_of = np.searchsorted(ix["cell_start"].astype(np.int64), where, side="right") - 1
    cells = np.stack([cell_of % dims[0], (cell_of // dims[0]) % dims[1], cell_of // (dims[0] * dims[1])], 1)
    org, inv_h = ix["org"], F(ix["inv_h"])
    assert np.array_equal(org, P.min(0))                                            # the anchor is the origin the maker searched with
    for iq, ip, axis in case["pairs"]:
        assert float(P[ip, axis]) - float(P[iq, axis]) <= float(radius)
        sim = [int(np.floor(F(F(P[i, axis] - org[axis]) * inv_h))) for i in (iq, ip)]
        assert sim == [cells[iq, axis], cells[ip, axis]], (sim, cells[iq], cells[ip])
        assert cells[ip, axis] - cells[iq, axis] == R_old + 1, (axis, cells[iq], cells[ip], R_old)
        other = [a for a in range(3) if a != axis]
        assert np.array_equal(cells[ip, other], cells[iq, other])


@pytest.mark.parametrize("name", NAMES)
def test_against_the_restatement(api, ctx, device, name):
    case = nr.cases()[name]
    if name.startswith("straddle"):
        pairs_straddle(api, ctx, case)
    nrm, cnt, cov = device(name)
    worst = nr.compare(name, nrm, cnt, cov)
    ref = nr.reference(name)
    print("%-24s n %4d  count <= %4d  separated %4d  exact %4d  error / bound: cov %.3f  sin %.3f  unit %.3f  rayleigh %.3f"
          % (name, len(cnt), int(cnt.max()) if len(cnt) else 0, int(ref["tol"]["separated"].sum()), int(ref["exact"].sum()), worst["cov"], worst["sin"], worst["unit"],
             worst["rayleigh"]))
    for k, v in worst.items():
        WORST[k] = max(WORST[k], v)
        assert v <= 1.0, (name, k, v)


def test_the_sign_rule_flips_on_each_branch(device):
    """the tilted dyadic planes: z > 0 where the raw vector had z < 0; z == 0 exactly and y > 0 where it had z == 0 and y < 0"""
    case = nr.cases()["tilted"]
    nrm = device("tilted")[0]
    s = np.sqrt(0.5)
    a, b = case["groups"]["xz"]
    assert (nrm[a:b, 2] > 0).all() and np.abs(nrm[a:b].astype(np.float64) - [-s, 0, s]).max() <= 2.0 ** -24
    a, b = case["groups"]["xy"]
    assert (nrm[a:b, 2] == 0).all() and (nrm[a:b, 1] > 0).all() and np.abs(nrm[a:b].astype(np.float64) - [-s, s, 0]).max() <= 2.0 ** -24


@pytest.mark.parametrize("a,b", nr.SAME_COUNTS)
def test_the_index_does_not_matter(device, a, b):
    """one cloud and one radius under two cell sizes, and with the origin on a lattice: equal counts, cov6 within the sum of the two
    bounds (the order of the sums changes with the cells), the normals within the sum of theirs"""
    (na, ca, va), (nb, cb, vb) = device(a), device(b)
    tol = nr.reference(a)["tol"]
    assert np.array_equal(ca, cb)
    assert (np.abs(va - vb).max(1) <= 2.0 * tol["cov"]).all()
    sep = tol["separated"]
    sin = np.linalg.norm(np.cross(na.astype(np.float64), nb.astype(np.float64)), axis=1)
    assert (sin <= 2.0 * tol["sin"])[sep].all()


@pytest.mark.parametrize("name", ["scene_1.6", "straddle_0.25_1", "size_257", "degenerate"])
def test_two_runs_give_the_same_bits(api, ctx, device, name):
    mp, nrm, cnt, cov = run(api, ctx, nr.cases()[name])
    mp.close()
    first = device(name)
    assert np.array_equal(bits(nrm), bits(first[0])) and np.array_equal(cnt, first[1]) and np.array_equal(bits(cov), bits(first[2]))


@pytest.mark.parametrize("name", ["scene_1.6", "straddle_0.3_2", "nonfinite"])
def test_without_covariance_the_normals_are_the_same_bits(api, ctx, device, name):
    mp, nrm, cnt, _ = run(api, ctx, nr.cases()[name], covariance=False)
    first = device(name)
    assert np.array_equal(bits(nrm), bits(first[0])) and np.array_equal(cnt, first[1])
    with pytest.raises(api.SlamFusionError):
        mp.download_covariances()
    mp.close()


def test_a_radius_estimate_replaces_a_knn_estimate(api, ctx, device):
    case = nr.cases()["scene_1.6"]
    mp = build(api, ctx, case)
    mp.estimate_normals_knn(10, covariance=True)
    assert (mp.download_normals()[1] == 10).all()
    mp.estimate_normals(case["radius"], covariance=True)
    nrm, cnt = mp.download_normals()
    cov = mp.download_covariances()
    mp.close()
    first = device("scene_1.6")
    assert np.array_equal(bits(nrm), bits(first[0])) and np.array_equal(cnt, first[1]) and np.array_equal(bits(cov), bits(first[2]))


def test_worst_error_over_bound(device):
    """runs last: the worst error / bound of every quantity over all fixtures"""
    for name in NAMES:
        for k, v in nr.compare(name, *device(name)).items():
            WORST[k] = max(WORST[k], v)
    print("radius normals, worst error / bound: cov6 %.3f  sin(angle) %.3f  |n| - 1 %.3f  Rayleigh excess %.3f" % (WORST["cov"], WORST["sin"], WORST["unit"], WORST["rayleigh"]))
    assert max(WORST.values()) <= 1.0
