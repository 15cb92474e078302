"""The launch schedule (csrc/sf_schedule.hpp) against what the three drivers of csrc/sf_icp.hip each decided for themselves before it
(tests/schedule_ref.py), over the whole product of its inputs and every launch index; the hook's place in the header and the
library; the two statistics calls that now read the stored schedule keep their signatures.  Host code alone: no device call."""
import os
import re

import numpy as np
import pytest

import schedule_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VALUES = dict(mode=(1, 2), K=(0, 1, 2, 5, 6, 7, 8, 20), qpl=(1, 2), sharded=(0, 1), whole=(0, 1), reuse=(0, 1), window=(0, 1), robust=(0, 1), wanted=(0, 1),
              fz_from=(4, 5, 6, 12, 20), defer=(0, 1), table=(0, 1), nbr_from=(-1, 1, 2, 3), lk_min=(0, 3, 5), tile_on=(0, 1))
# combinations no driver accepts: the launch list refuses a sharded object, and order_queries never sorts a sharded object's queries by tile
NO_DRIVER = (("sharded", "whole"), ("tile_on", "sharded"))


def _configs(api, K):
    """every accepted combination with K iterations -> (int32 [rows][inputs], dict of columns)"""
    assert tuple(VALUES) == api.SCHEDULE_INPUTS
    axes = [np.asarray(v if name != "K" else (K,), np.int32) for name, v in VALUES.items()]
    rows = np.stack([g.ravel() for g in np.meshgrid(*axes, indexing="ij")], axis=1)
    col = {name: i for i, name in enumerate(VALUES)}
    keep = np.ones(len(rows), bool)
    for a, b in NO_DRIVER:
        keep &= ~((rows[:, col[a]] != 0) & (rows[:, col[b]] != 0))
    rows = np.ascontiguousarray(rows[keep])
    return rows, {name: rows[:, i].astype(np.int64) for name, i in col.items()}


def _eq(got, want, what, rows, k, where=None):
    bad = np.asarray(got) != np.asarray(want)
    if where is not None:
        bad &= where
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError("%s: launch %d of %s gives %d, the driver %d (%d rows differ)" % (
            what, k, dict(zip(VALUES, rows[i].tolist())), np.asarray(got)[i], np.broadcast_to(want, bad.shape)[i], int(bad.sum())))


@pytest.mark.parametrize("K", VALUES["K"])
def test_every_launch_is_what_its_driver_made_of_it(api, K):
    rows, c = _configs(api, K)
    assert len(rows) == 2 * 2 * 5 * 2 ** 6 * 5 * 4 * 3               # mode, qpl, the (sharded, whole, tile_on) a driver accepts, six switches, fz_from, nbr_from, lk_min
    whole, sharded = c["whole"] != 0, c["sharded"] != 0
    for k in range(K + 1):
        out = api.hook_launch_schedule(rows, k)
        h = {name: out[:, i].astype(np.int64) for i, name in enumerate(api.SCHEDULE_OUTPUTS)}
        live = k < h["launches"]                                      # (O3D_P2P runs K + 1 launches)
        frozen = (h["nn"] == api.NN_FREEZE) | (h["nn"] == api.NN_FROZEN_FEW)
        deferring = h["nn"] == api.NN_DEFERRING
        L, S, P = ref.launch_list(c, k), ref.stepping(c, k), ref.shard_p2p(c, k)

        # --- the launch list
        m = live & whole
        _eq(h["launches"], L["launches"], "launch list, launches", rows, k, whole)
        _eq(h["nn"], L["nn"], "launch list, NN form", rows, k, m)
        _eq(h["one_per_lane"], L["q1"], "launch list, one query per lane", rows, k, m)
        _eq((h["solve_takes_freeze_state"] != 0) | (h["deferred_rows"] != 0), L["solve_fz"], "launch list, k_reduce_solve_fz", rows, k, m)
        _eq(h["deferred_rows"], L["df_rows"], "launch list, deferred rows", rows, k, m)
        _eq(h["ask_freeze"], L["request"], "launch list, request", rows, k, m)
        _eq(h["attempt_from"], L["attempt_from"], "launch list, attempt_from", rows, k, m & deferring)

        # --- sf_icp_step_begin / sf_icp_step_end, sharded or not
        m = live & ~whole
        _eq(h["launches"], S["launches"], "stepping, launches", rows, k, ~whole)
        _eq(h["nn"], S["nn"], "stepping, NN form", rows, k, m)
        _eq(h["one_per_lane"], S["q1"], "stepping, one query per lane", rows, k, m)
        _eq(frozen, S["reduce_fz"], "stepping, FreezeState of the reduction", rows, k, m)
        _eq(h["deferred_rows"], S["df_rows"], "stepping, deferred rows", rows, k, m)
        _eq(h["solve_takes_freeze_state"], S["solve_fz"], "stepping, FreezeState of the solve", rows, k, m)
        _eq(h["ask_freeze"], S["request"], "stepping, request", rows, k, m & (S["solve_fz"] != 0))
        _eq(h["ask_freeze"], 0, "stepping, request without a FreezeState", rows, k, m & (S["solve_fz"] == 0))
        _eq(h["attempt_from"], S["attempt_from"], "stepping, attempt_from", rows, k, m & deferring)

        # --- shard_step_p2p
        m = live & ~whole & sharded
        _eq(h["launches"], P["launches"], "P2P sharded loop, launches", rows, k, ~whole & sharded)
        _eq(h["nn"], P["nn"], "P2P sharded loop, NN form", rows, k, m)
        _eq(h["one_per_lane"], P["q1"], "P2P sharded loop, one query per lane", rows, k, m)
        _eq(frozen, P["reduce_fz"], "P2P sharded loop, FreezeState of the reduction", rows, k, m)
        _eq(h["deferred_rows"], 0, "P2P sharded loop, deferred rows", rows, k, m)
        _eq(h["solve_takes_freeze_state"], P["solve_fz"], "P2P sharded loop, FreezeState of the solve", rows, k, m)
        _eq(h["ask_freeze"], P["request"], "P2P sharded loop, request", rows, k, m & (P["solve_fz"] != 0))


@pytest.mark.parametrize("K", VALUES["K"])
def test_the_drivers_agreed_with_each_other(api, K):
    """Wherever more than one driver can run a configuration the restatements say the same: the two sharded loops in everything; the launch
    list and the stepping path in the NN launch of every k, and in the solve up to the one documented difference -- the list adds the
    deferred rows in k_reduce_solve_fz (so that solve runs behind every deferring launch), stepping adds them in k_reduce_only."""
    rows, c = _configs(api, K)
    sharded = c["sharded"] != 0
    both = (c["whole"] == 0) & ~sharded & (c["tile_on"] == 0)          # the same configuration enqueued whole: only `whole` differs
    as_list = dict(c, whole=np.ones_like(c["whole"]))
    for k in range(K + 1):
        S, P, L = ref.stepping(c, k), ref.shard_p2p(c, k), ref.launch_list(as_list, k)
        live = k < S["launches"]
        for name in ("launches", "nn", "q1", "reduce_fz", "df_rows", "solve_fz", "request"):
            _eq(S[name], P[name], "stepping against the P2P sharded loop, " + name, rows, k, live & sharded)
        m = live & both
        for name in ("launches", "nn", "q1"):
            _eq(L[name], S[name], "launch list against stepping, " + name, rows, k, m)
        _eq(L["attempt_from"], S["attempt_from"], "launch list against stepping, attempt_from", rows, k, m & (S["nn"] == ref.DEFER))
        _eq(L["solve_fz"], (S["solve_fz"] != 0) | (S["df_rows"] != 0), "launch list against stepping, the solve kernel", rows, k, m)
        _eq(L["df_rows"], S["df_rows"], "launch list against stepping, deferred rows", rows, k, m)
        _eq(L["request"], (S["solve_fz"] != 0) & (S["request"] != 0), "launch list against stepping, request", rows, k, m)


def test_the_hook_checks_its_arguments(api):
    lib = api.load_library()
    assert lib.sf_test_launch_schedule(None, 0, 0, None) == 0
    assert lib.sf_test_launch_schedule(None, 1, 0, None) != 0
    assert api.hook_launch_schedule(np.zeros((0, len(api.SCHEDULE_INPUTS)), np.int32), 3).shape == (0, len(api.SCHEDULE_OUTPUTS))


# ---------------------------------------------------------------- header and exports
DECLARATIONS = (
    r"int sf_test_launch_schedule(const int32_t *in, int64_t rows, int k, int32_t *out);",
    r"int sf_icp_defer_stats(sf_icp *icp, int64_t out[2]);",
    r"int sf_icp_lookup_launch_stats(sf_icp *icp, int64_t out[4]);",
    r"#define SF_TEST_SCHEDULE_IN 15",
    r"#define SF_TEST_SCHEDULE_OUT 10",
)


def _header():
    with open(os.path.join(ROOT, "include", "slamfusion.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_header_declares_the_hook_and_keeps_the_statistics_calls():
    text = _header()
    for decl in DECLARATIONS:
        assert re.sub(r"\s+", " ", decl) in text, decl
    assert text.index("int sf_test_label_boxes(") < text.index("int sf_test_launch_schedule(")   # at the end of the hook block
    assert text.index("int sf_icp_freeze_stats(") < text.index("int sf_icp_defer_stats(") < text.index("int sf_icp_lookup_launch_stats(") < text.index("int sf_icp_set_neighbour_research(")


def test_library_exports_them(api):
    lib = api.load_library()
    for name in ("sf_test_launch_schedule", "sf_icp_defer_stats", "sf_icp_lookup_launch_stats"):
        assert getattr(lib, name) is not None, name
    assert len(api.SCHEDULE_INPUTS) == 15 and len(api.SCHEDULE_OUTPUTS) == 10
    assert (api.NN_SEARCH, api.NN_TILE_SEARCH, api.NN_DEFERRING, api.NN_FREEZE, api.NN_FROZEN_FEW) == (ref.SEARCH, ref.TILE, ref.DEFER, ref.FREEZE, ref.FEW)


def test_the_header_of_the_schedule_is_plain_host_code():
    with open(os.path.join(ROOT, "slam_sensor_fusion_amd", "csrc", "sf_schedule.hpp")) as f:
        text = f.read()
    code = re.sub(r"//[^\n]*", " ", text)
    for word in ("hip", "__global__", "__device__", "sf_icp", "std::vector", "new ", "malloc"):
        assert word not in code, word
    assert re.findall(r'#include\s+[<"]([^>"]+)', code) == ["slamfusion.h"]


def _compiled_from(unit):
    """the files of csrc/ that the dependency file of a translation unit (csrc/Makefile, -MMD) names: what the compiler opened"""
    csrc = os.path.join(ROOT, "slam_sensor_fusion_amd", "csrc")
    dep = os.path.join(ROOT, "slam_sensor_fusion_amd", "lib", "obj", unit + ".d")
    if not os.path.isfile(dep):
        pytest.skip("no dependency file: the library was not built by csrc/Makefile here")
    with open(dep) as f:
        words = f.read().replace("\\\n", " ").split()
    return {os.path.basename(w) for w in words if not w.endswith(":") and os.path.realpath(os.path.join(csrc, os.path.dirname(w))) == os.path.realpath(csrc)}


def test_the_source_hash_reads_what_the_compiler_read(api):
    """kernel_source_hash follows the #include "..." lines from sf_icp.hip; the dependency file the compiler wrote for that
    translation unit names what it opened.  The two sets of csrc files must be the same."""
    named = _compiled_from("sf_icp.hip")
    assert named == set(api.kernel_sources()), sorted(named ^ set(api.kernel_sources()))
    assert "sf_icp.hip" in named and len(api.kernel_source_hash()) == 16


def test_the_source_hash_takes_the_numerical_core_and_no_ndt(api):
    """The dominant kernel is compiled from the core headers; NDT is a translation unit of its own and no longer moves the hash."""
    names = api.kernel_sources()
    assert {"sf_linalg.hpp", "sf_reduce.hpp", "sf_jacobi.hpp"} <= set(names), names
    assert not [n for n in names if n.startswith("sf_ndt")], names


def test_ndt_is_compiled_from_the_core_and_nothing_of_icp():
    named = _compiled_from("sf_ndt.hip")
    assert {"sf_ndt.hip", "sf_linalg.hpp", "sf_reduce.hpp", "sf_jacobi.hpp", "sf_sort.hpp", "sf_common.hpp"} <= named, sorted(named)
    assert not named & {"sf_icp.hip", "sf_nn.hpp", "sf_cov.hpp", "sf_schedule.hpp", "sf_icp_object.hpp"}, sorted(named)


def test_the_wrappers_keep_their_shape(api):
    import inspect
    assert list(inspect.signature(api.Icp.defer_stats).parameters) == ["self"]
    assert list(inspect.signature(api.Icp.lookup_launch_stats).parameters) == ["self"]
    assert list(inspect.signature(api.hook_launch_schedule).parameters) == ["configs", "k"]


def test_the_version_stays(api):
    assert api.load_library().sf_version() == 210
