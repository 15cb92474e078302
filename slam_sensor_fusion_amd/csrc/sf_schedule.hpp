// sf_schedule.hpp — which form launch k of an O3D_P2P / P2PLANE alignment takes ("The schedule").  Plain host
// C++: a value built once per alignment from the configuration as it stands when the alignment is enqueued, read by every driver of
// csrc/sf_icp.hip (the launch list and its captured graph, sf_icp_step_begin / _end, the P2P sharded loop), by the graph key and
// by the statistics of the alignment it describes.  REF_CPP keeps its own launch list and is not described here.
#pragma once
#include "slamfusion.h"

#ifndef SF_WIDE_QPL
#define SF_WIDE_QPL 2 // queries per lane of a wide scan's launches (csrc/sf_icp.hip: k_nn_red)
#endif

namespace sf {

// wide scans WITHOUT a neighbour table: from the fifth launch of an alignment on a wave first tries to verify all its queries at once
// (with a table the look-up launches start earlier, at the first launch that consults it: Schedule::lookup_first)
constexpr int VERIFY_FROM_SEARCH = 4;

struct Schedule {
    // what the form of a launch depends on, in the order sf_test_launch_schedule takes them
    int mode = 0, K = 0, qpl = 1;        // SF_ICP_O3D_P2P | SF_ICP_P2PLANE; IcpParams::num_iters; queries per lane of the source set (1 | SF_WIDE_QPL)
    int sharded = 0, whole = 0;          // the rank searches its owned queries only; enqueued whole (launch list, graph) | stepped (sf_icp_step_begin / _end, the sharded loops)
    int reuse = 0, window = 0;           // neighbour reuse on; SfWindow::kind of the map (0: whole map)
    int robust = 0, wanted = 0;          // the pairs are weighted; frozen pairs asked for: sf_icp_set_freeze(2), or (1) with FREEZE_AUTO_MIN_QUERIES queries
    int fz_from = 0, defer = 0;          // first launch that may be a freeze launch; sf_icp_set_defer_search
    int table = 0, nbr_from = 0;         // the alignment consults the map's neighbour table, from this launch on (sf_icp_set_neighbour_research)
    int lk_min = 0, tile_on = 0;         // no look-up launch before this one (learnt with fz_from); the queries are sorted by map tile
    // derived (make_schedule): frozen pairs run; the first look-up launch and the first deferring launch (fz_from: none)
    int fz = 0, lookup_first = 0, defer_first = 0;
    bool operator==(const Schedule &o) const
    {
        return mode == o.mode && K == o.K && qpl == o.qpl && sharded == o.sharded && whole == o.whole && reuse == o.reuse && window == o.window && robust == o.robust &&
               wanted == o.wanted && fz_from == o.fz_from && defer == o.defer && table == o.table && nbr_from == o.nbr_from && lk_min == o.lk_min && tile_on == o.tile_on &&
               fz == o.fz && lookup_first == o.lookup_first && defer_first == o.defer_first;
    }
    bool deferring() const { return defer_first < fz_from; }       // some launch hands its stragglers to the dense pass
    int lookup_launches() const { return fz_from - lookup_first; } // launches in look-up form
};

enum NnForm { NN_SEARCH = 0, NN_TILE_SEARCH = 1, NN_DEFERRING = 2, NN_FREEZE = 3, NN_FROZEN_FEW = 4 };
struct LaunchStep {
    int nn = NN_SEARCH;               // NnForm
    int one_per_lane = 0;             // a wide scan's launch with ONE query per lane: rows of 256 queries, twice as many
    int solve_takes_freeze_state = 0; // the solve behind the launch reads and writes the FreezeState
    int ask_freeze = 0;               // ... and may ask for a freeze launch
    int deferred_rows = 0;            // the rows of the dense pass are added to the launch's record
    int attempt_from = 0;             // k_nn_red_df: launches from this index on first try to verify a whole wave
    bool frozen() const { return nn == NN_FREEZE || nn == NN_FROZEN_FEW; } // the launch itself works on the FreezeState
};

// `in`: the fields above `derived` filled in
inline Schedule make_schedule(Schedule s)
{
    // frozen pairs: P2PLANE of wide scans with the neighbour reuse on, whole map, plain pairs -- and a launch left to freeze in
    s.fz = s.mode == SF_ICP_P2PLANE && s.wanted && !s.robust && s.reuse && s.qpl == SF_WIDE_QPL && s.window == 0 && s.K > s.fz_from + 1 && s.fz_from >= VERIFY_FROM_SEARCH;
    const bool df = s.fz && s.defer && !s.sharded;
    // look-up launches: with a table every launch from the first that consults it (never before lk_min) up to the freeze launch
    const int lk = s.nbr_from > s.lk_min ? s.nbr_from : s.lk_min;
    s.lookup_first = df && s.table && s.nbr_from >= 1 && lk < s.fz_from ? lk : s.fz_from;
    // without a table the one launch before the first chance to freeze defers, when it is a verifying launch
    const int last = s.fz_from - 1 >= VERIFY_FROM_SEARCH ? s.fz_from - 1 : s.fz_from;
    s.defer_first = !df ? s.fz_from : s.lookup_first < last ? s.lookup_first : last;
    return s;
}

// O3D_P2P runs one launch more: its last solve only scores the final pose
inline int launches(int mode, int K) { return mode == SF_ICP_O3D_P2P ? K + 1 : K; } // (for a loop that starts before its first step builds the schedule)
inline int launches(const Schedule &s) { return launches(s.mode, s.K); }

inline LaunchStep step_of(const Schedule &s, int k)
{
    LaunchStep st;
    const bool df = k >= s.defer_first && k < s.fz_from; // (only on the frozen-pairs schedule: defer_first == fz_from otherwise)
    // one query per lane while nearly every query searches (fewer registers: measured 929, 804, 508, 414 against 954, 836, 539, 439 us),
    // unless the launch is a look-up launch; part of the summation order, so the same with the reuse off.  O3D_P2P never.
    st.one_per_lane = s.mode == SF_ICP_P2PLANE && s.qpl > 1 && k < VERIFY_FROM_SEARCH && !df;
    if (s.fz && k == s.fz_from) st.nn = NN_FREEZE;
    else if (s.fz && k > s.fz_from) st.nn = NN_FROZEN_FEW;
    else if (df) st.nn = NN_DEFERRING;
    // tile by tile while nearly every query searches: every launch with the neighbour reuse off, the first VERIFY_FROM_SEARCH with it
    // on (afterwards whole waves certify and k_nn_red streams the cache).  Only an alignment enqueued whole: the stepping drivers
    // have no tile form and search with k_nn_red even when order_queries has sorted the queries by tile.
    else if (s.whole && s.tile_on && (!s.reuse || k < VERIFY_FROM_SEARCH)) st.nn = NN_TILE_SEARCH;
    // the solve before the first chance to freeze is the first that may ask; the last launch a freeze could serve is K - 1
    st.solve_takes_freeze_state = s.fz && k + 1 >= s.fz_from;
    st.ask_freeze = st.solve_takes_freeze_state && k + 2 < s.K;
    st.deferred_rows = df;
    st.attempt_from = s.lookup_first < s.fz_from ? s.lookup_first : VERIFY_FROM_SEARCH;
    return st;
}

} // namespace sf
