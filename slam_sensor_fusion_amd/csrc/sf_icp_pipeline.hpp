// sf_icp_pipeline.hpp -- the two lanes and the two source sets at work: ensure_lanes, wait_src_ahead, SrcScope (a call that
// writes the source), lane_reserve, icp_alloc, icp_set_source_device_aos, LaneScope (the enqueue of one alignment), lane_describe
// and step_adopt_source (the stepping and sharded entry points, which take no LaneScope).
// A fragment, not a stand-alone header: sf_icp.hip includes it at file scope, after sf_icp_order_host.hpp.  It uses Lane, SrcSet,
// soa() and the declaration of fused_capacity() (sf_icp_object.hpp), and of sf_icp.hip's device code BLK, REC_STRIDE, BOX_PARTS,
// ScanBox, IcpState, nblk, WIDE_AUTO_POINTS and the kernels k_soa_from_aos, k_set_int and k_scan_boxes_*; SF_WIDE_QPL is
// sf_schedule.hpp's.  The input mark (main_mark, mark_*) and the lanes' and source sets' events are read and written here only,
// but for their creation's twin in sf_icp_destroy.

namespace {
// the lanes' streams and every event of the pipeline, once
int ensure_lanes(sf_icp *icp)
{
    for (int l = 0; l < 2; ++l) {
        Lane &ln = icp->lanes[l];
        if (!ln.stream) SF_HIP(hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking));
        if (!ln.done) SF_HIP(hipEventCreateWithFlags(&ln.done, hipEventDisableTiming));
        if (!icp->srcs[l].used) SF_HIP(hipEventCreateWithFlags(&icp->srcs[l].used, hipEventDisableTiming));
        if (!ln.started) SF_HIP(hipEventCreateWithFlags(&ln.started, hipEventDisableTiming));
    }
    if (!icp->main_mark) SF_HIP(hipEventCreateWithFlags(&icp->main_mark, hipEventDisableTiming));
    if (!icp->src_ready) SF_HIP(hipEventCreateWithFlags(&icp->src_ready, hipEventDisableTiming));
    if (!icp->unmarked_ev) SF_HIP(hipEventCreateWithFlags(&icp->unmarked_ev, hipEventDisableTiming));
    return SF_OK;
}

// src() was written on a lane's stream and nothing has been ordered behind that upload yet: stream `s` waits for it
int wait_src_ahead(sf_icp *icp, hipStream_t s)
{
    if (!icp->src_ahead) return SF_OK;
    SF_HIP(hipStreamWaitEvent(s, icp->src_ready, 0));
    icp->src_ahead = false;
    return SF_OK;
}

// RAII around a call that writes the source.  While an alignment of this object is unfetched (and the lanes are on) the new
// source goes into the OTHER source set -- the constructor flips src_set, so src() is the set being written from then on -- on
// the stream of prev(), the lane the next alignment will take: it waits for the last alignment that read that set, not for the
// alignment in flight.  Otherwise: the set at hand on the context's stream, as before.
struct SrcScope {
    sf_icp *icp;
    hipStream_t main = nullptr;
    bool ahead = false;
    uint64_t version0 = 0;
    int rc = SF_OK;
    SrcScope(sf_icp *i, bool allowed) : icp(i), main(i->ctx->stream), version0(i->src_version)
    {
        static const bool ahead_on = []() { const char *e = std::getenv("SF_SRC_AHEAD"); return !e || std::atoi(e) != 0; }(); // (A/B switch)
        const bool go = ahead_on && allowed && icp->pipeline != 0 && icp->unfetched && !icp->shard && !icp->profiling;
        if (!go) { // the set at hand on the context's stream: behind an upload that went to a lane's stream, if there was one
            rc = wait_src_ahead(icp, main);
            return;
        }
        rc = ensure_lanes(icp);
        if (rc != SF_OK) return;
        if (!icp->src_ahead) icp->src_set ^= 1; // (a second source before any alignment: the same set, the same stream, again)
        const SrcSet &ss = icp->src();
        hipStream_t ls = icp->prev().stream;
        if (icp->src_unmarked_use) { // readers that left no event: everything the context's stream holds
            if (hipEventRecord(icp->unmarked_ev, main) != hipSuccess || hipStreamWaitEvent(ls, icp->unmarked_ev, 0) != hipSuccess) { rc = SF_ERR_HIP; return; }
            icp->src_unmarked_use = false;
        }
        if (ss.used_rec && hipStreamWaitEvent(ls, ss.used, 0) != hipSuccess) { rc = SF_ERR_HIP; return; }
        static const bool stagger_on = []() { const char *e = std::getenv("SF_UPLOAD_STAGGER"); return !e || std::atoi(e) != 0; }(); // (A/B switch)
        if (stagger_on && icp->cur().started_rec && hipStreamWaitEvent(ls, icp->cur().started, 0) != hipSuccess) { rc = SF_ERR_HIP; return; } // see Lane::started
        icp->ctx->stream = ls;
        ahead = true;
    }
    ~SrcScope()
    {
        hipStream_t ran = icp->ctx->stream;
        icp->ctx->stream = main;
        if (!ahead) return;
        if (hipEventRecord(icp->src_ready, ran) == hipSuccess) icp->src_ahead = true;
        // (this source did not pass the context's stream: the mark of the inputs that did stands as it stood)
        if (icp->mark_valid && icp->mark_src_version == version0) icp->mark_src_version = icp->src_version;
    }
};

// what an alignment of the source at hand writes per scan, in the lane at hand
int lane_reserve(sf_icp *icp)
{
    Lane &ln = icp->cur(); const SrcSet &ss = icp->src();
    const int batch = std::max(ss.batch, 1);
    SF_TRY(ln.state.reserve(sizeof(IcpState) * (size_t)batch));
    SF_TRY(ln.d_inits.reserve(sizeof(double) * 16 * (size_t)batch));
    SF_TRY(ln.partials.reserve(sizeof(double) * (size_t)REC_STRIDE * (size_t)std::max(ss.nblocks, 1) * (size_t)batch));
    return SF_OK;
}

// outputs = false (a source written ahead of an alignment in flight): the lane's output buffers are left to lane_reserve at the next enqueue
int icp_alloc(sf_icp *icp, int64_t n, int batch, bool outputs = true)
{
    Lane &ln = icp->cur(); SrcSet &ss = icp->src();
    const int64_t total = n * batch;
    // plane = distance between the x, y and z components of the SoA arrays: rounded up and never shrinking, so that the
    // component pointers a captured launch list holds survive scans of slightly different sizes
    ss.plane = std::max<int64_t>(ss.plane, sf::div_up(std::max<int64_t>(total, 1), 4096) * 4096);
    SF_TRY(ss.X0.reserve(sizeof(float) * 3 * (size_t)ss.plane));
    SF_TRY(ss.X0r.reserve(sizeof(float4) * (size_t)ss.plane));
    // single scan: workgroups for the point count rounded up to 4096 (the kernels bound themselves by the count in
    // device memory), so the launch geometry -- and with it a captured graph -- is shared by scans of similar size
    ss.n_cap = batch == 1 ? sf::div_up(std::max<int64_t>(n, 1), 4096) * 4096 : n;
    ss.nblocks = (int)std::max<int64_t>(1, sf::div_up(ss.n_cap, BLK));
    // Two queries per lane are part of the summation order, so the choice must not depend on which path runs an alignment: above
    // wide_from always; between WIDE_AUTO_POINTS and wide_from when no single-launch kernel could take the batch anyway (more
    // rows than any of them keeps resident) -- a 64-ring sensor's 130 k points in a batch then run wide and may freeze.
    bool wide = n > icp->wide_from;
    if (!wide && icp->wide_auto && n > WIDE_AUTO_POINTS) {
        const int64_t cap = std::max(fused_capacity(icp, SF_ICP_O3D_P2P), fused_capacity(icp, SF_ICP_P2PLANE));
        wide = sf::div_up(n, BLK) * (int64_t)batch > cap;
    }
    ss.qpl = wide ? SF_WIDE_QPL : 1;
    ss.nblocks_nn = (int)std::max<int64_t>(1, sf::div_up(n, BLK * ss.qpl));
    // (set before the outputs: lane_reserve sizes them from the set, so after a failed reservation the set says n and batch as it says n_cap / nblocks / qpl; batch >= 1 from every caller, so its max(.., 1) is idle)
    ss.n = n;
    ss.batch = batch;
    if (outputs) {
        const auto e0 = ln.state.epoch;
        SF_TRY(lane_reserve(icp));
        if (ln.state.epoch != e0) ln.meta.valid = false; // (the states of this lane's last alignment went with the old allocation: sf_icp_fetch_previous has nothing to read)
        SF_TRY(icp->xchg_own.reserve(sizeof(double) * REC_STRIDE * (size_t)batch));
    }
    if (icp->inits.size() != (size_t)batch * 16) { // (by the priors' own size, not by the batch of whichever source set was at hand)
        icp->inits.assign((size_t)batch * 16, 0.0);
        for (int b = 0; b < batch; ++b)
            for (int d = 0; d < 4; ++d) icp->inits[(size_t)b * 16 + 5 * d] = 1.0;
    }
    icp->h_state.resize((size_t)batch);
    return SF_OK;
}

int icp_set_source_device_aos(sf_icp *icp, const float *d_aos, int64_t n, int batch, bool ahead = false)
{
    SrcSet &ss = icp->src();
    SF_TRY(icp_alloc(icp, n, batch, !ahead));
    ss.n_on_device = false;
    const int64_t total = n * batch;
    if (total > 0)
        hipLaunchKernelGGL(k_soa_from_aos, dim3(nblk(total)), dim3(256), 0, icp->ctx->stream, d_aos, total, soa(ss.X0, ss.plane, 0), soa(ss.X0, ss.plane, 1),
                           soa(ss.X0, ss.plane, 2), ss.X0r.as<float4>());
    SF_TRY(ss.n_dev.reserve(sizeof(int)));
    hipLaunchKernelGGL(k_set_int, dim3(1), dim3(1), 0, icp->ctx->stream, ss.n_dev.as<int>(), (int)n);
    SF_HIP(hipGetLastError());
    // bounding box of every scan on its own, reduced on the device and left there (no host synchronisation per scan): what moves
    // a scan's points is bounded by ITS box (a batch of 10 m scans spread over a 100 m map has a 100 m box and every rotation a
    // 50 m lever arm).  (The box of the whole batch, which rounds 1-3 also formed here, had no reader left.)
    SF_TRY(ss.d_boxes.reserve(sizeof(ScanBox) * (size_t)std::max(batch, 1)));
    SF_TRY(ss.d_box_parts.reserve(sizeof(ScanBox) * BOX_PARTS * (size_t)std::max(batch, 1)));
    hipLaunchKernelGGL(k_scan_boxes_partial, dim3(BOX_PARTS, (unsigned)std::max(batch, 1)), dim3(256), 0, icp->ctx->stream, soa(ss.X0, ss.plane, 0), soa(ss.X0, ss.plane, 1),
                       soa(ss.X0, ss.plane, 2), (int)n, ss.d_box_parts.as<ScanBox>());
    hipLaunchKernelGGL(k_scan_boxes_final, dim3(nblk(std::max(batch, 1), 64)), dim3(64), 0, icp->ctx->stream, ss.d_box_parts.as<ScanBox>(), std::max(batch, 1), ss.d_boxes.as<ScanBox>());
    ss.have_source = true;
    icp->src_version += 1;
    return SF_OK;
}

// RAII around the enqueue of one alignment.  An alignment enqueued while an earlier one of this object has not been fetched yet
// (back-to-back sf_icp_align_batch_async: the throughput pattern) takes the OTHER lane -- the constructor flips `lane`, so cur()
// is the lane of this alignment from then on -- and that lane's stream; the first one after a fetch -- and every alignment of a
// caller that fetches each result before asking for the next -- runs on the context's stream in the lane it finds, as before.
// Per lane an event marks its last alignment, whatever stream it ran on.
struct LaneScope {
    sf_icp *icp;
    hipStream_t main = nullptr;
    bool piped = false;
    int rc = SF_OK;
    LaneScope(sf_icp *i, bool allowed) : icp(i), main(i->ctx->stream)
    {
        if (!allowed && !icp->lanes[0].done) { // the per-scan path (single launch) of an object that has never piped: no streams, no events, nothing to record
            icp->src_unmarked_use = true;
            return;
        }
        rc = ensure_lanes(icp); // (every alignment marks the end of its reading of the source set: the events must exist)
        if (rc != SF_OK) return;
        if (!allowed) { // the context's stream, the lane at hand -- behind a source that was written on a lane's stream, if one was
            rc = wait_src_ahead(icp, main);
            return;
        }
        // the mark: where the context's stream stood when the inputs last changed (taken before anything of this alignment is enqueued)
        const sf_map *m = icp->map;
        // (the initial poses are not part of it: they travel in the kernel arguments or through the lane's own copy, on the lane's stream)
        const bool same = icp->mark_valid && icp->mark_src_version == icp->src_version && icp->mark_map == (const void *)m && icp->mark_map_generation == m->generation && icp->mark_nbr_stamp == m->nbr_stamp &&
                          std::memcmp(&icp->mark_window, &m->window, sizeof(SfWindow)) == 0;
        if (!same) {
            if (hipEventRecord(icp->main_mark, main) != hipSuccess) { rc = SF_ERR_HIP; return; }
            icp->mark_valid = true;
            icp->mark_src_version = icp->src_version;
            icp->mark_map = (const void *)m;
            icp->mark_map_generation = m->generation;
            icp->mark_nbr_stamp = m->nbr_stamp;
            icp->mark_window = m->window;
        }
        if (!icp->unfetched && !icp->src_ahead) { // nothing of this object in flight: the context's stream, the lane at hand
            if (hipEventRecord(icp->cur().started, main) == hipSuccess) icp->cur().started_rec = true;
            return;
        }
        icp->lane ^= 1; // take turns (a source written ahead went to this lane's stream)
        Lane &ln = icp->cur();
        rc = lane_reserve(icp);
        if (rc != SF_OK) return;
        // after the inputs, and after this lane's previous alignment (which may have run on the context's stream)
        if (hipStreamWaitEvent(ln.stream, icp->main_mark, 0) != hipSuccess) { rc = SF_ERR_HIP; return; }
        if (ln.used && hipStreamWaitEvent(ln.stream, ln.done, 0) != hipSuccess) { rc = SF_ERR_HIP; return; }
        rc = wait_src_ahead(icp, ln.stream);
        if (rc != SF_OK) return;
        icp->ctx->stream = ln.stream;
        piped = true;
        if (hipEventRecord(ln.started, ln.stream) == hipSuccess) ln.started_rec = true;
    }
    ~LaneScope()
    {
        hipStream_t ran = icp->ctx->stream;
        icp->ctx->stream = main;
        Lane &ln = icp->cur(); SrcSet &ss = icp->src();
        if (!ln.done) return; // (the lanes have never been set up: nothing to mark)
        if (ss.used && hipEventRecord(ss.used, ran) == hipSuccess) ss.used_rec = true; // the last reader of this source set
        if (hipEventRecord(ln.done, ran) != hipSuccess) return;
        ln.used = true;
        // whatever the caller enqueues next on the context's stream is ordered behind this alignment
        if (piped) { hipError_t e = hipStreamWaitEvent(main, ln.done, 0); (void)e; }
    }
};

// cur().meta <- the alignment being enqueued: sf_icp_fetch_results and a redo describe the latest alignment as it was enqueued
void lane_describe(sf_icp *icp, int mode, bool cov)
{
    sf_icp::LaneMeta &M = icp->cur().meta;
    M.valid = true; M.cov = cov; M.batch = icp->src().batch; M.mode = mode;
    M.inits = icp->inits; M.src_set = icp->src_set; M.src_version = icp->src_version;
    M.sched = sf::Schedule{}; M.lk_waves = 0; // (schedule_describe, once the queries are ordered; the single launch has none)
}

// The stepping and the sharded entry points run on the context's stream in the lane at hand, without a LaneScope.  A source that
// SrcScope wrote ahead of an unfetched alignment (on a lane's stream, icp_alloc(outputs = false)) is theirs to adopt at the start of
// an alignment: the context's stream waits for the upload, and everything an alignment writes per scan -- states, initial poses,
// partial rows, the exchange records -- is sized for the source now at hand.  They leave no event on the source set they read: the
// next source written ahead waits for the context's stream instead (src_unmarked_use).
int step_adopt_source(sf_icp *icp)
{
    SF_TRY(wait_src_ahead(icp, icp->ctx->stream));
    Lane &ln = icp->cur();
    const auto e0 = ln.state.epoch;
    SF_TRY(lane_reserve(icp));
    if (ln.state.epoch != e0) ln.meta.valid = false; // (as icp_alloc: the states of the last alignment went with the old allocation)
    SF_TRY(icp->xchg_own.reserve(sizeof(double) * REC_STRIDE * (size_t)std::max(icp->src().batch, 1)));
    icp->src_unmarked_use = true;
    return SF_OK;
}
} // namespace
