"""What each of the three drivers of csrc/sf_icp.hip did with launch k of an alignment BEFORE the schedule became a value of its own
(csrc/sf_schedule.hpp): a restatement in numpy of the launch list (enqueue_align), of sf_icp_step_begin / sf_icp_step_end and of
shard_step_p2p as they stood in the commit that introduced the look-up launches, one function per driver, with the helpers the three
of them shared then (freeze_on, lookup_first, defer_first, defer_now, one_per_lane_now, tile_launch).  Written from those drivers, not
from the header: tests/test_schedule_rule.py holds the header against it.

A configuration is a dict of equally shaped integer arrays, one per input of the schedule (api.SCHEDULE_INPUTS); k is one launch
index for all of them.  Every function returns a dict of arrays:
  launches     launches of the alignment
  nn           the NN launch: SEARCH (k_nn_red), TILE (k_tile_search + k_red_cached), DEFER (k_nn_red_df + k_nn_deferred),
               FREEZE (k_nn_red_fz), FEW (k_nn_red_fz_few)
  q1           the launch ran one query per lane, so the slab had nblocks (sharded: own_nblocks * qpl) rows and the reduction read
               them with one query per lane
  reduce_fz    (stepping drivers) the reduction behind the launch got the FreezeState
  df_rows      the reduction got the rows of the dense pass
  solve_fz     the launch list: the solve was k_reduce_solve_fz (it always got the FreezeState); stepping: the solve got the FreezeState
  request      the `request` argument of that solve (read by the kernel only next to a FreezeState)
  attempt_from the last argument of k_nn_red_df (read where nn == DEFER)
"""
import numpy as np

O3D_P2P, P2PLANE = 1, 2
VERIFY_FROM_SEARCH = 4
WIDE_QPL = 2
SEARCH, TILE, DEFER, FREEZE, FEW = range(5)


def _b(a):
    return np.asarray(a) != 0


# ---------------------------------------------------------------- the helpers the drivers shared
def freeze_on(c):
    return ((c["mode"] == P2PLANE) & _b(c["wanted"]) & ~_b(c["robust"]) & _b(c["reuse"]) & (c["qpl"] == WIDE_QPL) & (c["window"] == 0)
            & (c["K"] > c["fz_from"] + 1) & (c["fz_from"] >= VERIFY_FROM_SEARCH))


def lookup_first(c):
    none = ~freeze_on(c) | ~_b(c["defer"]) | _b(c["sharded"]) | ~_b(c["table"]) | (c["nbr_from"] < 1)
    return np.where(none, c["fz_from"], np.minimum(c["fz_from"], np.maximum(c["nbr_from"], c["lk_min"])))


def lookup_form(c):
    return lookup_first(c) < c["fz_from"]


def defer_first(c):
    none = ~freeze_on(c) | ~_b(c["defer"]) | _b(c["sharded"])
    last = np.where(c["fz_from"] - 1 >= VERIFY_FROM_SEARCH, c["fz_from"] - 1, c["fz_from"])
    return np.where(none, c["fz_from"], np.minimum(lookup_first(c), last))


def defer_now(c, k):
    return (k >= defer_first(c)) & (k < c["fz_from"])


def one_per_lane_now(c, k):
    return (c["mode"] == P2PLANE) & (c["qpl"] > 1) & (k < VERIFY_FROM_SEARCH) & ~defer_now(c, k)


def tile_launch(c, k):
    return _b(c["tile_on"]) & (~_b(c["reuse"]) | (k < VERIFY_FROM_SEARCH))


def _attempt_from(c):       # launch_nn_red_df
    return np.where(lookup_form(c), lookup_first(c), VERIFY_FROM_SEARCH)


def _steps(c):              # the launch list's loops and sharded_steps
    return np.where(c["mode"] == O3D_P2P, c["K"] + 1, c["K"])


def _out(c, **kw):
    shape = np.broadcast(*c.values()).shape
    return {name: np.broadcast_to(np.asarray(v).astype(np.int64), shape) for name, v in kw.items()}


# ---------------------------------------------------------------- enqueue_align
def launch_list(c, k):
    o3d = c["mode"] == O3D_P2P
    fz = freeze_on(c)
    wide = (c["qpl"] > 1) & ~_b(c["sharded"])
    df = defer_now(c, k)
    q1 = wide & (k < VERIFY_FROM_SEARCH) & ~df
    frozen = fz & (k >= c["fz_from"])
    nn = np.where(frozen, np.where(k > c["fz_from"], FEW, FREEZE), np.where(df, DEFER, np.where(tile_launch(c, k), TILE, SEARCH)))
    solve_fz = fz & (df | (k + 1 >= c["fz_from"]))
    request = solve_fz & (k + 1 >= c["fz_from"]) & (k + 2 < c["K"])
    # O3D_P2P: launch_tile_search<1>(icp, false) | launch_nn_red<1>(icp), k_reduce_solve<1> over nblocks_nn rows
    return _out(c, launches=_steps(c), nn=np.where(o3d, np.where(tile_launch(c, k), TILE, SEARCH), nn), q1=~o3d & q1, solve_fz=~o3d & solve_fz,
                df_rows=~o3d & solve_fz & df, request=~o3d & request, attempt_from=_attempt_from(c))


# ---------------------------------------------------------------- sf_icp_step_begin / sf_icp_step_end (k = fz_step)
def stepping(c, k):
    o3d = c["mode"] == O3D_P2P
    fz = freeze_on(c)
    q1 = one_per_lane_now(c, k)
    df = (c["mode"] == P2PLANE) & defer_now(c, k)
    freeze_nn_now = fz & (k >= c["fz_from"])
    freeze_solve_now = fz & (k + 1 >= c["fz_from"])
    nn = np.where(freeze_nn_now, np.where(k > c["fz_from"], FEW, FREEZE), np.where(df, DEFER, SEARCH))
    # O3D_P2P: launch_nn_red<1>(icp, shard), k_reduce_only<1> with qpl and no FreezeState, k_solve_only<1> with nullptr and 0
    return _out(c, launches=_steps(c), nn=np.where(o3d, SEARCH, nn), q1=q1, reduce_fz=~o3d & freeze_nn_now, df_rows=~o3d & df, solve_fz=~o3d & freeze_solve_now,
                request=~o3d & (k + 2 < c["K"]), attempt_from=_attempt_from(c))


# ---------------------------------------------------------------- shard_step_p2p (k = fz_step; always sharded)
def shard_p2p(c, k):
    o3d = c["mode"] == O3D_P2P
    fz = freeze_on(c)
    q1 = (c["mode"] == P2PLANE) & (c["qpl"] > 1) & (k < VERIFY_FROM_SEARCH)
    fz_nn = fz & (k >= c["fz_from"])
    fz_solve = fz & (k + 1 >= c["fz_from"])
    nn = np.where(fz_nn, np.where(k > c["fz_from"], FEW, FREEZE), SEARCH)
    return _out(c, launches=_steps(c), nn=np.where(o3d, SEARCH, nn), q1=q1, reduce_fz=~o3d & fz_nn, df_rows=np.zeros_like(o3d), solve_fz=~o3d & fz_solve,
                request=~o3d & (k + 2 < c["K"]), attempt_from=_attempt_from(c))
