// sf_icp_object.hpp -- the object behind the public handle: struct sf_icp with its lanes (cur() / prev()) and source sets
// (src()), then, in the anonymous namespace, what the host code asks of it everywhere: soa(), queries(), robust_on(),
// robust_arg(), the span of the walk order (order_span, order_key_shift) and reuse_reset().
// A fragment, not a stand-alone header: sf_icp.hip includes it at file scope, first thing behind the device code.  It uses
// IcpState, IcpParams, RobustArg, FreezeParams, CovArg (sf_cov.hpp) and the constants of that file's device code;
// fused_capacity() is declared here and defined with the single-launch kernels' host side in sf_icp.hip.

struct sf_icp {
    sf_ctx *ctx = nullptr;
    IcpParams prm{};
    int debug = 0;
    int64_t cache_n = 0;     // entries per array of the lane's qcache
    bool reuse = true;       // sf_icp_set_nn_reuse
    int order = SF_ORDER_AUTO;
    bool ordered = false;    // this alignment reads Xq
    std::vector<double> inits; // batch * 16
    double *h_inits = nullptr;          // pinned staging of the batch's initial transforms
    size_t h_inits_cap = 0;
    hipEvent_t inits_ev = nullptr;      // recorded after the staging buffer's last copy
    bool inits_ev_pending = false;
    // target
    sf_map *map = nullptr;
    sf_map *own_map = nullptr;
    sf_cloud *own_cloud = nullptr;
    // device state
    sf::DevBuf xchg_own;
    void *xchg = nullptr;
    int64_t xchg_bytes = 0;
    int64_t wide_from = WIDE_SCAN_POINTS; // sf_icp_set_wide_scan_points: scans above this many points take two queries per lane (and may freeze)
    bool wide_auto = true;   // no explicit limit: scans above WIDE_AUTO_POINTS are wide too when the batch is beyond every single-launch kernel (set_source_common)
    std::vector<IcpState> h_state;
    // sharding
    bool shard = false;
    float xlo = 0, xhi = 0;
    sf::DevBuf own_idx, own_blk, own_count, own_off, own_keep; // sharded path: owned-query compaction (own_keep: the screening ballots, 1 bit per point)
    std::vector<uint32_t> h_own;                      // host copy of counts / offsets
    int64_t own_total = 0;                            // owned-query candidates of this rank (all scans)
    float own_margin = 1.0f;                          // sf_icp_set_shard_margin
    int own_nblocks = 1;                              // workgroups per scan on the sharded path (largest scan)
    sf::DevBuf d_box;                        // sf::MinMaxDev: bounding box of the source batch (finite points), left on the device
    int last_mode = 0;
    // REF_CPP in one launch (k_ref_fused)
    bool fused = true;       // sf_icp_set_fused
    bool last_fused = false; // the last alignment ran as the single launch
    sf::DevBuf bar;          // per scan: {arrival counter, departure counter} of the grid barrier
    int fused_limit[4] = {-1, -1, -1, -1}; // per mode, [3] P2PLANE under a robust kernel: workgroups that are certainly resident together (-1: not asked yet)
    double fused_share = 0.0; // share of the device the single-launch grid in flight holds in the ledger (0: none)
    int64_t fused_redone = 0; // alignments redone through the launch list after a barrier gave up
    bool inject_timeout = false; // test hook (sf_icp_test_inject_barrier_timeout): treat the next single-launch alignment as timed out
    int64_t fused_launches = 0;
    IcpState *h_pin = nullptr; // pinned, device-visible: the single-launch forms write the final states here themselves (no copy back)
    size_t h_pin_cap = 0;
    // graph
    bool use_graph = false;
    int64_t graph_captures = 0, graph_replays = 0; // sf_icp_graph_counts
    // everything a captured launch list bakes in: kernel arguments passed by value (thresholds, IcpParams, the
    // SfGrid geometry and pointers) and the addresses of this object's buffers.  A replay is only valid while all of
    // it is unchanged; sf_map stamps every build / normals pass with a process-unique generation, DevBuf counts its
    // reallocations (epoch).
    struct GraphKey {
        int batch = -1, ordered = -1, robust_kind = -1, cov_on = -1;
        sf::Schedule sched; // which launches the list holds (mode, iterations, window kind and reuse are fields of it)
        int64_t n = -1;
        const void *map = nullptr;
        uint64_t map_generation = 0, epochs = 0;
        uint64_t nbr_stamp = 0; // the neighbour table this alignment consults (0: none) and its address (the first launch that does: sched.nbr_from)
        const void *nbr = nullptr;
        float max_corr = 0, accept = 0, eps = 0, guard_scale = 0, guard_min = 0, guard_max = 0; // IcpParams and FreezeParams as the kernels take them: by value, each field itself
        int max_tries = 0;
        double robust_k = 0;
        double cov_prm[5] = {0, 0, 0, 0, 0};
        bool operator==(const GraphKey &o) const
        {
            return batch == o.batch && ordered == o.ordered && sched == o.sched && n == o.n && map == o.map && map_generation == o.map_generation && epochs == o.epochs &&
                   nbr_stamp == o.nbr_stamp && nbr == o.nbr && max_corr == o.max_corr && accept == o.accept && eps == o.eps &&
                   guard_scale == o.guard_scale && guard_min == o.guard_min && guard_max == o.guard_max && max_tries == o.max_tries &&
                   robust_kind == o.robust_kind && robust_k == o.robust_k && cov_on == o.cov_on && std::memcmp(cov_prm, o.cov_prm, sizeof(cov_prm)) == 0;
        }
    };
    // what a lane's last alignment was (sf_icp_fetch_previous reads prev()'s states with prev()'s description)
    struct LaneMeta {
        bool valid = false;
        bool cov = false; // it ran with the covariance switch on: cov_out of its lane holds its sf_icp_covariance entries
        int batch = 0, mode = 0;
        std::vector<double> inits;
        int src_set = 0;          // the source set it read, and that set's version then: a redo after a barrier timeout aligns THAT source
        uint64_t src_version = 0;
        sf::Schedule sched;       // its launches, as enqueued (zeros: the single launch): what the drivers dispatch on and the statistics describe
        int64_t lk_waves = 0;     // the waves of one of its two-queries-per-lane launches (freeze_learn_schedule)
    };
    // Consecutive asynchronous alignments of the launch list overlap: an alignment's last launches (frozen pairs: fourteen 16 us
    // kernels on an otherwise idle device) run under the next one's searching launches.  Two LANES take turns; each has its own
    // stream and its own copy of everything an alignment writes.  cur() = lanes[lane] is the lane of the latest alignment, prev()
    // the other; taking turns is `lane ^= 1`, so a lane's allocations -- and the graph captured over them -- never move.
    // Ordering (LaneScope): a lane starts after the context's stream as it stood when the inputs -- source, initial poses,
    // target -- last changed, and the context's stream waits for every alignment right after it is enqueued, so whatever the caller
    // enqueues next (a fetch, an upload, a map rebuild) is ordered behind it as before; only back-to-back alignments of unchanged
    // inputs run side by side.  Same kernels, same data, same results (tests/test_gpu_pipeline.py).
    struct Lane {
        sf::DevBuf X;            // SoA: x[B*n], y[B*n], z[B*n] (REF_CPP: the moving points)
        sf::DevBuf qcache;       // neighbour reuse, two float4 arrays of cache_n entries: (neighbour, its index), (neighbour's normal, E) -- O3D_P2P: the second array holds E alone, as floats
        sf::DevBuf Xq, qkeys, qkeys2, qidx, qidx2; // cell-ordered copy of X0 and the sort's buffers
        sf::DevBuf corr;         // float4 [B*n] (REF_CPP): a point's target (x, y, z, sorted position or -1 = dead)
        sf::DevBuf state, d_inits, partials;
        sf::DevBuf fz_state, fz_part, fz_cnt, fz_ids, fz_all; // frozen pairs (k_nn_red_fz)
        sf::DevBuf df_cnt, df_ids, df_part, df_stat;          // deferred search (k_nn_red_df)
        sf::DevBuf qtkey, tseg, tile_stats; // tile search: tile key of every ordered query; per (tile, scan) segment starts; counters
        sf::DevBuf cov_part, cov_out;       // pose covariance (sf_cov.hpp): the rows and the result
        hipGraphExec_t graph_exec = nullptr;
        GraphKey graph_key;
        std::vector<double> inits_uploaded; // what d_inits holds (the copy is skipped while nothing changed)
        uint32_t d_inits_epoch = 0xffffffffu;
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr; // the end of the lane's last alignment, whatever stream it ran on
        bool used = false;         // `done` has been recorded
        // started: recorded on the lane's stream when its latest alignment begins (behind everything it waits for).  A source written
        // ahead starts its upload behind the START of the alignment on the other lane: two uploads issued back to back -- the host
        // fetched two results that became ready together -- would otherwise share the link, end together and let both alignments
        // start together, a lockstep in which nothing overlaps (measured: upload + upload, then alignment + alignment, for good).
        hipEvent_t started = nullptr;
        bool started_rec = false;
        LaneMeta meta;
    } lanes[2];
    int lane = 0;                 // index of cur()
    Lane &cur() { return lanes[lane]; }
    const Lane &cur() const { return lanes[lane]; }
    Lane &prev() { return lanes[lane ^ 1]; }
    // Two SOURCE SETS: srcs[src_set] = src() is the set at hand, the one the next alignment reads and sf_icp_set_source* writes.  A
    // source set while an alignment of this object is still unfetched goes into the OTHER set (`src_set ^= 1` first), the one that
    // alignment does not read, on the stream of the lane the next alignment will take, so the next batch's upload / conversion runs
    // beside the alignment in flight instead of behind it (SrcScope).  Per set an event marks the end of the last alignment that
    // read it; `src_ready` the end of the last upload that ran on a lane's stream.
    struct SrcSet {
        sf::DevBuf X0;           // SoA: x[B*n], y[B*n], z[B*n]
        sf::DevBuf X0r;          // the same points as float4 records (gather source of the query ordering)
        sf::DevBuf stage;        // persistent upload staging of sf_icp_set_source* (AoS)
        sf::DevBuf d_boxes, d_box_parts; // ScanBox per scan (motion bound of the reuse certificate, owned-array margin), and the partial boxes of their reduction
        sf::DevBuf n_dev;        // the point count in device memory (single-scan REF_CPP kernels read it)
        int64_t n = 0;           // points per scan
        int64_t n_cap = 0;       // single scan: n rounded up (launch geometry of the REF_CPP kernels)
        int64_t plane = 0;       // component stride of the SoA arrays X0 / X / Xq
        int batch = 0;
        int nblocks = 0;         // workgroups of 256 points covering a scan (REF_CPP kernels, owned-query compaction)
        int nblocks_nn = 0;      // k_nn_red workgroups per scan = slab rows (256 * qpl queries each)
        int qpl = 1;             // queries per lane of k_nn_red: 1 up to wide_from points per scan, SF_WIDE_QPL beyond (part of the summation order)
        bool have_source = false;
        bool n_on_device = false; // sf_icp_set_source_scan: n is an upper bound, the count itself is in n_dev (single scan, REF_CPP)
        hipEvent_t used = nullptr; // the end of the last alignment that read this set
        bool used_rec = false;
    } srcs[2];
    int src_set = 0;              // index of src()
    SrcSet &src() { return srcs[src_set]; }
    const SrcSet &src() const { return srcs[src_set]; }
    hipEvent_t src_ready = nullptr;
    bool src_ahead = false;       // src() was written on a lane's stream (src_ready) and no alignment has been ordered behind it yet
    hipEvent_t unmarked_ev = nullptr;
    bool src_unmarked_use = false; // an alignment read a source set before the lanes' events existed (the per-scan path never creates them): the first source written ahead waits for the context's stream instead
    bool prev_ok = false;         // the alignment before the latest one ran on prev() and has not been overwritten or fetched
    std::vector<IcpState> h_prev;
    sf::DevBuf order_lut;         // k_order_lut_*: histogram (uint32) and key table (uint16) over the walk order of the attached index
    uint64_t order_lut_gen = 0;   // sf_map::generation the table was built for
    int order_lut_shift = 0, order_lut_on = 1; // order_lut_on: SF_ORDER_LUT=0 in the environment switches the table off (A/B runs)
    int pipeline = 1;             // sf_icp_set_pipeline: 0 = every alignment on the context's stream
    hipEvent_t main_mark = nullptr;
    bool unfetched = false;       // an alignment has been enqueued since the last fetch (the next one may run beside it)
    bool mark_valid = false;      // main_mark stands for the inputs as described by the fields below
    uint64_t src_version = 0, mark_src_version = 0, mark_map_generation = 0;
    const void *mark_map = nullptr;
    SfWindow mark_window{};
    // profiling
    bool profiling = false;
    std::vector<hipEvent_t> ev;
    size_t ev_used = 0;
    int64_t prof_launches = 0;
    double prof_ms = 0;
    std::vector<float> prof_each;   // duration of every profiled launch, in launch order
    std::vector<int> ev_kind;       // SF_PROF_* of every event pair
    std::vector<float> prof_phase[SF_PROF_KINDS]; // sharded path: durations of the other phases, in order
    sf::DevBuf nn_stats;            // per profiled k_nn_red launch: {queries that searched, waves that searched}
    // frozen pairs (k_nn_red_fz)
    int freeze = 1;                 // sf_icp_set_freeze: 0 off, 1 when the batch is large enough to gain (FREEZE_AUTO_MIN_QUERIES), 2 always
    FreezeParams fz_prm{8.0f, 2.0e-5f, 3.0e-4f, 3};
    int fz_from = 5;                // launch index of the first launch that may be a freeze launch
    bool fz_from_auto = true;       // learnt from the last fetched alignment (sf_icp_fetch_results); sf_icp_set_freeze_params fixes it
    int fz_fetches = 0;             // fetched alignments since fz_from was last reset to its default (every FZ_PROBE_EVERY-th starts over)
    int fz_step = 0;                // stepping paths: launches since the pass began
    int nbr_from = SF_NBR_FROM;     // sf_icp_set_neighbour_research: first launch index that consults the map's neighbour table (negative: off)
    bool nbr_active = false;        // the alignment being enqueued consults it (nbr_prepare)
    int64_t nbr_stats_first = 0;    // nn_stats slot of the last alignment's first launch (sf_icp_neighbour_stats)
    uint64_t mark_nbr_stamp = 0;
    int defer = 1;                  // sf_icp_set_defer_search: the verifying launches of the frozen-pairs schedule list their stragglers for a dense pass (k_nn_red_df)
    int lk_min = 0;                 // no look-up launch before this index: learnt with fz_from (freeze_learn_schedule), 0 while from_launch is pinned
    int64_t nn_stats_used = 0;
    static constexpr int64_t NN_STATS_CAP = 1024;
    // robust kernel of P2PLANE (sf_icp_set_robust_kernel): read at enqueue, passed to the kernels by value
    int robust_kind = SF_ROBUST_NONE;
    double robust_k = 0.0;
    // pose covariance (sf_cov.hpp): read at enqueue, passed to the kernels by value; the rows and the result live per lane
    int cov_on = 0;
    CovArg cov_arg{0.0, 0.0, 0.0, 0.0, 0.0};
    bool prev_cov_ok = false; // sf_icp_fetch_covariance_previous has something to read (set with prev_ok, cleared by its own fetch)
    // tile search (sf_tile.hpp): the searching launches of large batches
    int tile_mode = 0;              // sf_icp_set_tile_search: 0 off, 1 when the batch is large enough to gain (TILE_AUTO_MIN_QUERIES), 2 whenever possible
    bool tile_on = false;           // this alignment's queries are sorted by tile and its searching launches run k_tile_search
    sf::SfTiles tiles{};
};

namespace {

using Lane = sf_icp::Lane;
using SrcSet = sf_icp::SrcSet;
float *soa(sf::DevBuf &b, int64_t total, int axis) { return b.as<float>() + (size_t)axis * (size_t)total; }
// the query arrays this alignment walks: the cell-ordered copy or the scans as given
const float *queries(sf_icp *icp, int axis)
{
    Lane &ln = icp->cur(); SrcSet &ss = icp->src();
    if (icp->shard) return soa(ln.Xq, icp->own_total, axis); // compact, cell-ordered owned queries (shard_build)
    return soa(icp->ordered ? ln.Xq : ss.X0, ss.plane, axis);
}

int fused_capacity(sf_icp *icp, int mode, bool robust = false); // (workgroups the single-launch kernels keep resident; defined with them)

// this alignment's pairs are weighted (P2PLANE only; the other modes ignore the setting)
bool robust_on(const sf_icp *icp, int mode) { return mode == SF_ICP_P2PLANE && icp->robust_kind != SF_ROBUST_NONE; }
RobustArg robust_arg(const sf_icp *icp) { return RobustArg{icp->robust_kind, icp->robust_k}; }

// AUTO orders when there is enough work for the order to pay for the sort.  Measured, 200 k-point
// scans, 20 iterations: 1 scan in flight +1.5 % (break-even), 2: +8 %, 4: +32 %, 32: +65 %
constexpr int64_t ORDER_AUTO_MIN_QUERIES = 300000;

// the cells the walk order (order_cell) spans, and the bits that number them
struct OrderSpan { uint64_t cells; int bits; };
OrderSpan order_span(const SfGrid &g)
{
    const uint64_t ny_pad = ((uint64_t)g.dim[1] + ORDER_YBLK - 1) / ORDER_YBLK * ORDER_YBLK; // order_cell pads y to whole blocks
    OrderSpan sp{(uint64_t)g.dim[0] * ny_pad * (uint64_t)g.dim[2], 0};
    while (sp.bits < 63 && (1ull << sp.bits) < sp.cells) ++sp.bits;
    return sp;
}

// key = position of the query's cell in the walk order, shifted down to the bits the sort takes (sf::ORD_KEY_BITS)
int order_key_shift(const SfGrid &g) { return std::max(0, order_span(g).bits - sf::ORD_KEY_BITS); }

// neighbour reuse starts empty at every alignment (a zero bound certifies nothing)
int reuse_reset(sf_icp *icp, int64_t count)
{
    if (!icp->reuse && !icp->tile_on) return SF_OK; // (tile launches hand their pairs to k_red_cached through the cache arrays)
    const size_t c = (size_t)std::max<int64_t>(count, 1);
    // nothing is cleared: a scan's entries count only once IcpState::cache_live says they have been written (every lane
    // writes its entry in the first launch after a start or a rebuild of the owned arrays)
    SF_TRY(icp->cur().qcache.reserve(sizeof(float4) * 2 * c));
    icp->cache_n = (int64_t)c;
    return SF_OK;
}

} // namespace
