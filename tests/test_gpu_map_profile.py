"""sf_map_profile_launches / sf_map_last_launch_ms: device events around the kernel launches of the map's queries and
estimates.  Off by default, nothing to read until a call was timed, and the results of the timed calls do not change."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_map_launch_times(api, ctx):
    rng = np.random.default_rng(17)
    m = rng.uniform(-3, 3, (2000, 3)).astype(np.float32)
    q = rng.uniform(-3, 3, (300, 3)).astype(np.float32)
    mp = api.Map(ctx, api.Cloud(ctx, m), 0.25)
    with pytest.raises(api.SlamFusionError):
        mp.last_launch_ms()                                     # off by default
    plain = mp.nn(q), mp.knn(q, 7)
    mp.profile_launches(True)
    with pytest.raises(api.SlamFusionError):
        mp.last_launch_ms()                                     # switched on, nothing timed yet
    timed = mp.nn(q)
    assert 0.0 < mp.last_launch_ms() < 1000.0
    for a, b in zip(plain[0], timed):
        assert np.array_equal(a, b)
    timed = mp.knn(q, 7)
    assert 0.0 < mp.last_launch_ms() < 1000.0
    for a, b in zip(plain[1], timed):
        assert np.array_equal(a, b)
    mp.estimate_normals(0.25)
    assert 0.0 < mp.last_launch_ms() < 1000.0
    mp.estimate_normals_knn(10)
    assert 0.0 < mp.last_launch_ms() < 1000.0
    mp.profile_launches(False)
    with pytest.raises(api.SlamFusionError):
        mp.last_launch_ms()
    mp.profile_launches(True)                                   # on again: the events are reused
    mp.knn(q, 7)
    assert 0.0 < mp.last_launch_ms() < 1000.0
    mp.close()
