// sf_ndt_host.hpp -- the host side of the NDT calls (include/slamfusion.h, sf_ndt_*): the object, the voxel build on an index of
// its own and the launch list of an alignment.  Included by sf_icp.hip at file scope, after everything else; the kernels are
// sf_ndt.hpp's.  An alignment enqueues max_iterations pairs (k_ndt_derivs, k_ndt_step), one more derivative pass at the final
// pose and the copy of the states, and waits once.  With the line search on (sf_ndt_set_line_search) an iteration is four launches
// (k_ndt_derivs, k_ndt_step_ls, k_ndt_scores over every entry's trials, k_ndt_pick), still without a wait in between;
// sf_ndt_align_levels runs one such alignment per level.

struct sf_ndt {
    sf_ctx *ctx = nullptr;
    sf_ndt_params prm{};
    sf_map *index = nullptr;    // the grid index at cell = resolution (its own, also for a map target)
    sf_cloud *points = nullptr; // sf_ndt_set_target_map: the map's points in original order
    sf::DevBuf flag, pos, occ, is_voxel, vpos, tmp, vox, cov, vcell, vcount, cell_voxel;
    sf::DevBuf src, state, partials, trace;
    sf_ndt_line_search ls{0, 0, 1.0, 1e-4};            // trials 0: off
    sf::DevBuf ls_entry, ls_partials, ls_rows, poses, scores;
    std::vector<sf_ndt_ls_row> rows;                   // entry 0 of the last sf_ndt_align with the search on
    bool has_rows = false;
    int64_t n_points = 0, n_cells = 0, n_occupied = 0, n_voxels = 0, n_src = 0;
    int batch = 0;
    bool has_target = false, has_source = false;
    float build_ms = -1.0f, align_ms = -1.0f;
    hipEvent_t ev[2] = {nullptr, nullptr};
};

namespace {

constexpr int NDT_MAX_BATCH = 64;

int ndt_check_params(const sf_ndt_params *p)
{
    SF_CHECK(p, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(std::isfinite(p->resolution) && p->resolution > 0.0, SF_ERR_INVALID, "bad arguments: ndt resolution must be positive and finite (got %g)", p->resolution);
    SF_CHECK(p->outlier_ratio > 0.0 && p->outlier_ratio < 1.0, SF_ERR_INVALID, "bad arguments: ndt outlier_ratio must lie in (0, 1) (got %g)", p->outlier_ratio);
    SF_CHECK(p->min_points >= 3, SF_ERR_INVALID, "bad arguments: ndt min_points must be >= 3 (got %d)", (int)p->min_points);
    SF_CHECK(p->neighbours == SF_NDT_DIRECT1 || p->neighbours == SF_NDT_DIRECT7, SF_ERR_INVALID, "bad arguments: ndt neighbours must be 1 or 7 (got %d)", (int)p->neighbours);
    SF_CHECK(p->max_iterations >= 0 && p->max_iterations <= 1024, SF_ERR_INVALID, "bad arguments: ndt max_iterations must be 0 .. 1024 (got %d)", (int)p->max_iterations);
    SF_CHECK(p->step_size > 0.0, SF_ERR_INVALID, "bad arguments: ndt step_size must be positive (got %g)", p->step_size);
    return SF_OK;
}

NdtConst ndt_constants(const sf_ndt_params &p)
{
    const double r = p.resolution, c1 = 10.0 * (1.0 - p.outlier_ratio), c2 = p.outlier_ratio / (r * r * r);
    const double d3 = -std::log(c2), d1 = -std::log(c1 + c2) - d3;
    const double d2 = -2.0 * std::log((-std::log(c1 * std::exp(-0.5) + c2) - d3) / d1);
    return NdtConst{d1, 0.5 * d2, d2, -(d1 * d2)};
}

inline unsigned ndt_blocks(int64_t n, int per) { return (unsigned)std::max<int64_t>(sf::div_up(n, per), 1); }

int ndt_event_ms(sf_ndt *ndt, float *ms)
{
    *ms = -1.0f;
    if (ndt->prm.profile) SF_HIP(hipEventElapsedTime(ms, ndt->ev[0], ndt->ev[1]));
    return SF_OK;
}

int ndt_mark(sf_ndt *ndt, int k)
{
    if (!ndt->prm.profile) return SF_OK;
    if (!ndt->ev[k]) SF_HIP(hipEventCreate(&ndt->ev[k]));
    SF_HIP(hipEventRecord(ndt->ev[k], ndt->ctx->stream));
    return SF_OK;
}

// the index of `cloud` at cell = resolution, then the voxels
int ndt_build(sf_ndt *ndt, sf_cloud *cloud)
{
    sf_ctx *ctx = ndt->ctx;
    ndt->has_target = false;
    ndt->build_ms = -1.0f;
    if (!ndt->index) SF_TRY(sf_map_create(ctx, &ndt->index));
    SF_TRY(sf_map_build(ndt->index, cloud, (float)ndt->prm.resolution)); // (refuses a table that does not fit: SF_ERR_OVERFLOW)
    const SfGrid &G = ndt->index->grid;
    const uint64_t ncell = (uint64_t)G.dim[0] * (uint64_t)G.dim[1] * (uint64_t)G.dim[2];
    SF_CHECK(ncell < (1ull << 31), SF_ERR_OVERFLOW, "ndt: %.3g cells at resolution %g: the cell -> voxel table holds fewer than 2^31", (double)ncell, ndt->prm.resolution);
    hipStream_t s = ctx->stream;
    const int64_t nc = (int64_t)ncell;
    SF_TRY(ndt->flag.reserve(sizeof(uint32_t) * (size_t)nc));
    SF_TRY(ndt->pos.reserve(sizeof(uint32_t) * (size_t)nc));
    SF_TRY(ndt->cell_voxel.reserve(sizeof(int32_t) * (size_t)nc));
    SF_TRY(ndt_mark(ndt, 0));
    SF_HIP(hipMemsetAsync(ndt->cell_voxel.p, 0xff, sizeof(int32_t) * (size_t)nc, s));
    hipLaunchKernelGGL(k_ndt_cell_flags, dim3(ndt_blocks(nc, 256)), dim3(256), 0, s, G.cell_start, nc, ndt->flag.as<uint32_t>());
    SF_TRY(sf::scan_u32<0>(ctx, ndt->flag.as<uint32_t>(), ndt->pos.as<uint32_t>(), nc));
    uint32_t last[2] = {0, 0};
    SF_HIP(hipMemcpyAsync(&last[0], ndt->pos.as<uint32_t>() + (nc - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    SF_HIP(hipMemcpyAsync(&last[1], ndt->flag.as<uint32_t>() + (nc - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    SF_HIP(hipStreamSynchronize(s));
    const int64_t n_occ = (int64_t)last[0] + (int64_t)last[1];
    int64_t n_vox = 0;
    if (n_occ > 0) {
        SF_TRY(ndt->occ.reserve(sizeof(uint32_t) * (size_t)n_occ));
        SF_TRY(ndt->is_voxel.reserve(sizeof(uint32_t) * (size_t)n_occ));
        SF_TRY(ndt->vpos.reserve(sizeof(uint32_t) * (size_t)n_occ));
        SF_TRY(ndt->tmp.reserve(sizeof(double) * NDT_TMP_STRIDE * (size_t)n_occ));
        SF_TRY(ndt->vox.reserve(sizeof(double) * NDT_VOX_STRIDE * (size_t)n_occ));
        SF_TRY(ndt->cov.reserve(sizeof(double) * 6 * (size_t)n_occ));
        SF_TRY(ndt->vcell.reserve(sizeof(int64_t) * (size_t)n_occ));
        SF_TRY(ndt->vcount.reserve(sizeof(int32_t) * (size_t)n_occ));
        hipLaunchKernelGGL(k_ndt_occupied, dim3(ndt_blocks(nc, 256)), dim3(256), 0, s, ndt->flag.as<uint32_t>(), ndt->pos.as<uint32_t>(), nc, ndt->occ.as<uint32_t>());
        hipLaunchKernelGGL(k_ndt_voxels, dim3(ndt_blocks(n_occ, BLK / 64)), dim3(BLK), 0, s, G.pts, G.cell_start, ndt->occ.as<uint32_t>(), n_occ, (int)ndt->prm.min_points,
                           ndt->prm.min_eig_ratio, ndt->tmp.as<double>(), ndt->is_voxel.as<uint32_t>());
        SF_TRY(sf::scan_u32<0>(ctx, ndt->is_voxel.as<uint32_t>(), ndt->vpos.as<uint32_t>(), n_occ));
        hipLaunchKernelGGL(k_ndt_compact, dim3(ndt_blocks(n_occ, 256)), dim3(256), 0, s, ndt->occ.as<uint32_t>(), ndt->is_voxel.as<uint32_t>(), ndt->vpos.as<uint32_t>(), n_occ,
                           ndt->tmp.as<double>(), ndt->vox.as<double>(), ndt->cov.as<double>(), ndt->vcell.as<int64_t>(), ndt->vcount.as<int32_t>(),
                           ndt->cell_voxel.as<int32_t>());
        SF_HIP(hipGetLastError());
        SF_TRY(ndt_mark(ndt, 1));
        SF_HIP(hipMemcpyAsync(&last[0], ndt->vpos.as<uint32_t>() + (n_occ - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        SF_HIP(hipMemcpyAsync(&last[1], ndt->is_voxel.as<uint32_t>() + (n_occ - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        SF_HIP(hipStreamSynchronize(s));
        n_vox = (int64_t)last[0] + (int64_t)last[1];
    } else {
        SF_HIP(hipGetLastError());
        SF_TRY(ndt_mark(ndt, 1));
        SF_HIP(hipStreamSynchronize(s));
    }
    SF_TRY(ndt_event_ms(ndt, &ndt->build_ms));
    ndt->n_points = cloud->n;
    ndt->n_cells = nc;
    ndt->n_occupied = n_occ;
    ndt->n_voxels = n_vox;
    ndt->has_target = true;
    return SF_OK;
}

NdtGrid ndt_grid(const sf_ndt *ndt)
{
    const SfGrid &G = ndt->index->grid;
    NdtGrid g;
    for (int d = 0; d < 3; ++d) { g.org[d] = (double)G.org[d]; g.dim[d] = G.dim[d]; }
    g.inv_h = (double)G.inv_h;
    g.cell_voxel = ndt->cell_voxel.as<int32_t>();
    g.vox = ndt->vox.as<double>();
    return g;
}

void ndt_launch_derivs(sf_ndt *ndt, const NdtGrid &g, const NdtConst &cn, int entries, size_t src_stride, int force, int nblocks)
{
    hipStream_t s = ndt->ctx->stream;
    const dim3 grid((unsigned)nblocks, (unsigned)entries);
    if (ndt->prm.neighbours == SF_NDT_DIRECT7)
        hipLaunchKernelGGL(k_ndt_derivs<7>, grid, dim3(BLK), 0, s, g, cn, ndt->src.as<float>(), (int)ndt->n_src, src_stride, ndt->state.as<NdtState>(), force,
                           ndt->partials.as<double>(), nblocks);
    else
        hipLaunchKernelGGL(k_ndt_derivs<1>, grid, dim3(BLK), 0, s, g, cn, ndt->src.as<float>(), (int)ndt->n_src, src_stride, ndt->state.as<NdtState>(), force,
                           ndt->partials.as<double>(), nblocks);
}

void ndt_result(const NdtState &S, sf_ndt_result *o)
{
    for (int i = 0; i < 16; ++i) o->T[i] = S.T[i];
    o->score = S.score;
    for (int i = 0; i < 6; ++i) o->gradient[i] = S.g[i];
    for (int i = 0; i < 36; ++i) o->hessian[i] = S.H[i];
    o->n_inside = (int64_t)S.n_inside;
    o->n_terms = (int64_t)S.n_terms;
    o->iterations = S.iterations;
    o->converged = S.converged;
    o->modified = S.modified;
    o->flags = S.flags;
}

int ndt_reserve_run(sf_ndt *ndt, int entries, int nblocks)
{
    SF_TRY(ndt->state.reserve(sizeof(NdtState) * (size_t)entries));
    SF_TRY(ndt->partials.reserve(sizeof(double) * REC_STRIDE * (size_t)nblocks * (size_t)entries));
    return SF_OK;
}

// the scores of gridDim.y * gridDim.z poses in one launch: pose (y, z) at poses + y * pose_stride + 16 z, its rows at slab y * nz + z
void ndt_launch_scores(sf_ndt *ndt, const NdtGrid &g, const NdtConst &cn, int ny, int nz, size_t src_stride, const NdtState *done, const double *poses, size_t pose_stride,
                       double *partials, int nblocks)
{
    hipStream_t s = ndt->ctx->stream;
    const dim3 grid((unsigned)nblocks, (unsigned)ny, (unsigned)nz);
    if (ndt->prm.neighbours == SF_NDT_DIRECT7)
        hipLaunchKernelGGL(k_ndt_scores<7>, grid, dim3(BLK), 0, s, g, cn, ndt->src.as<float>(), (int)ndt->n_src, src_stride, done, poses, pose_stride, partials, nblocks);
    else
        hipLaunchKernelGGL(k_ndt_scores<1>, grid, dim3(BLK), 0, s, g, cn, ndt->src.as<float>(), (int)ndt->n_src, src_stride, done, poses, pose_stride, partials, nblocks);
}

// entries states start at `poses` [entries][16]; iterations > 0: the Newton loop first; then the derivatives at the final poses
// with the line search on, an iteration is (k_ndt_derivs, k_ndt_step_ls, k_ndt_scores, k_ndt_pick); want_rows: the rows of entry 0
int ndt_run(sf_ndt *ndt, const double *poses, int entries, size_t src_stride, int iterations, bool timed, sf_ndt_result *out, double *trace, bool want_rows = false)
{
    sf_ctx *ctx = ndt->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int nblocks = (int)ndt_blocks(ndt->n_src, BLK);
    SF_TRY(ndt_reserve_run(ndt, entries, nblocks));
    std::vector<NdtState> h((size_t)entries);
    for (int b = 0; b < entries; ++b) {
        std::memset(&h[(size_t)b], 0, sizeof(NdtState));
        for (int i = 0; i < 16; ++i) h[(size_t)b].T[i] = poses[16 * (size_t)b + i];
    }
    double *d_trace = nullptr;
    if (trace) {
        SF_TRY(ndt->trace.reserve(sizeof(double) * 16 * (size_t)(iterations + 1)));
        d_trace = ndt->trace.as<double>();
    }
    const int trials = iterations > 0 ? (int)ndt->ls.trials : 0;
    sf_ndt_ls_row *d_rows = nullptr;
    if (want_rows) ndt->has_rows = false;
    if (trials > 0) {
        SF_TRY(ndt->ls_entry.reserve(sizeof(NdtLsEntry) * (size_t)entries));
        SF_TRY(ndt->ls_partials.reserve(sizeof(double) * REC_STRIDE * (size_t)nblocks * (size_t)trials * (size_t)entries));
        if (want_rows) {
            SF_TRY(ndt->ls_rows.reserve(sizeof(sf_ndt_ls_row) * (size_t)iterations));
            d_rows = ndt->ls_rows.as<sf_ndt_ls_row>();
        }
    }
    SF_TRY(sf::upload_staged(ctx, ndt->state.p, h.data(), sizeof(NdtState) * (size_t)entries));
    const NdtGrid g = ndt_grid(ndt);
    const NdtConst cn = ndt_constants(ndt->prm);
    const NdtStepArg sa{ndt->prm.step_size, ndt->prm.transformation_epsilon, ndt->prm.hessian_floor};
    SF_TRY(ndt_mark(ndt, 0));
    const NdtLsArg la{ndt->ls.step_max, ndt->ls.armijo, ndt->prm.transformation_epsilon, ndt->prm.hessian_floor, trials};
    for (int it = 0; it < iterations; ++it) {
        ndt_launch_derivs(ndt, g, cn, entries, src_stride, 0, nblocks);
        if (trials == 0) {
            hipLaunchKernelGGL(k_ndt_step, dim3((unsigned)entries), dim3(NDT_SBLK), 0, s, ndt->state.as<NdtState>(), ndt->partials.as<double>(), nblocks, sa, it, 0, d_trace);
            continue;
        }
        hipLaunchKernelGGL(k_ndt_step_ls, dim3((unsigned)entries), dim3(NDT_SBLK), 0, s, ndt->state.as<NdtState>(), ndt->partials.as<double>(), nblocks, la, it,
                           ndt->ls_entry.as<NdtLsEntry>(), d_rows);
        ndt_launch_scores(ndt, g, cn, entries, trials, src_stride, ndt->state.as<NdtState>(), reinterpret_cast<const double *>(ndt->ls_entry.p), sizeof(NdtLsEntry) / sizeof(double),
                          ndt->ls_partials.as<double>(), nblocks);
        hipLaunchKernelGGL(k_ndt_pick, dim3((unsigned)entries), dim3(NDT_SBLK), 0, s, ndt->state.as<NdtState>(), ndt->ls_partials.as<double>(), nblocks, la, it,
                           ndt->ls_entry.as<NdtLsEntry>(), d_trace, d_rows);
    }
    ndt_launch_derivs(ndt, g, cn, entries, src_stride, 1, nblocks);
    hipLaunchKernelGGL(k_ndt_step, dim3((unsigned)entries), dim3(NDT_SBLK), 0, s, ndt->state.as<NdtState>(), ndt->partials.as<double>(), nblocks, sa, iterations, 1, d_trace);
    SF_HIP(hipGetLastError());
    SF_TRY(ndt_mark(ndt, 1));
    SF_HIP(hipMemcpyAsync(h.data(), ndt->state.p, sizeof(NdtState) * (size_t)entries, hipMemcpyDeviceToHost, s));
    SF_HIP(hipStreamSynchronize(s));
    if (timed) SF_TRY(ndt_event_ms(ndt, &ndt->align_ms));
    for (int b = 0; b < entries; ++b) ndt_result(h[(size_t)b], out + b);
    if (trace) {
        for (int i = 0; i < 16; ++i) trace[i] = poses[i];
        const int rows = out[0].iterations;
        if (rows > 0) SF_HIP(hipMemcpy(trace + 16, d_trace + 16, sizeof(double) * 16 * (size_t)rows, hipMemcpyDeviceToHost));
    }
    if (d_rows) { // one row per iteration whose trials were evaluated: the steps taken and the stalled one
        const int rows = out[0].iterations + ((out[0].flags & SF_NDT_FLAG_LINE_SEARCH_STALLED) ? 1 : 0);
        ndt->rows.resize((size_t)rows);
        if (rows > 0) SF_HIP(hipMemcpy(ndt->rows.data(), d_rows, sizeof(sf_ndt_ls_row) * (size_t)rows, hipMemcpyDeviceToHost));
        ndt->has_rows = true;
    }
    return SF_OK;
}

int ndt_check_line_search(const sf_ndt_line_search *p)
{
    SF_CHECK(p->trials >= 0 && p->trials <= SF_NDT_MAX_TRIALS, SF_ERR_INVALID, "bad arguments: ndt line search trials must be 0 .. 16 (got %d)", (int)p->trials);
    SF_CHECK(std::isfinite(p->step_max) && p->step_max > 0.0, SF_ERR_INVALID, "bad arguments: ndt line search step_max must be positive and finite (got %g)", p->step_max);
    SF_CHECK(p->armijo > 0.0 && p->armijo < 1.0, SF_ERR_INVALID, "bad arguments: ndt line search armijo must lie in (0, 1) (got %g)", p->armijo);
    return SF_OK;
}

} // namespace

extern "C" void sf_ndt_default_params(sf_ndt_params *p)
{
    if (!p) return;
    *p = sf_ndt_params{1.0, 0.55, 0.1, 1e-4, 0.01, 1e-6, 6, SF_NDT_DIRECT7, 30, 0};
}

extern "C" int sf_ndt_create(sf_ctx *ctx, const sf_ndt_params *p, sf_ndt **out)
{
    SF_CHECK(ctx && p && out, SF_ERR_INVALID, "bad arguments");
    SF_TRY(ndt_check_params(p));
    sf_ndt *ndt = new (std::nothrow) sf_ndt();
    SF_CHECK(ndt, SF_ERR_NOMEM, "out of host memory");
    ndt->ctx = ctx;
    ndt->prm = *p;
    sf::ctx_retain(ctx);
    *out = ndt;
    return SF_OK;
}

extern "C" void sf_ndt_destroy(sf_ndt *ndt)
{
    if (!ndt) return;
    hipError_t e = hipStreamSynchronize(ndt->ctx->stream);
    (void)e;
    if (ndt->index) sf_map_destroy(ndt->index);
    if (ndt->points) sf_cloud_destroy(ndt->points);
    for (hipEvent_t ev : ndt->ev)
        if (ev) { hipError_t e2 = hipEventDestroy(ev); (void)e2; }
    sf_ctx *ctx = ndt->ctx;
    delete ndt;
    sf::ctx_release(ctx);
}

extern "C" int sf_ndt_set_target_cloud(sf_ndt *ndt, sf_cloud *cloud)
{
    SF_CHECK(ndt && cloud, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(cloud->ctx == ndt->ctx, SF_ERR_INVALID, "bad arguments: the cloud belongs to another context");
    SF_HIP(hipSetDevice(ndt->ctx->device));
    return ndt_build(ndt, cloud);
}

extern "C" int sf_ndt_set_target_map(sf_ndt *ndt, sf_map *map)
{
    SF_CHECK(ndt && map, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(map->ctx == ndt->ctx, SF_ERR_INVALID, "bad arguments: the map belongs to another context");
    SF_CHECK(map->built, SF_ERR_STATE, "map not built");
    sf_ctx *ctx = ndt->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    if (ndt->points) { sf_cloud_destroy(ndt->points); ndt->points = nullptr; }
    SF_TRY(sf_cloud_create(ctx, &ndt->points));
    sf_cloud *c = ndt->points;
    const int64_t n = map->n;
    SF_TRY(c->xyz.reserve(sizeof(float) * 3 * (size_t)std::max<int64_t>(n, 1)));
    if (n > 0) {
        hipLaunchKernelGGL(k_ndt_unsort, dim3(ndt_blocks(n, 256)), dim3(256), 0, ctx->stream, map->grid.pts, n, c->xyz.as<float>());
        SF_HIP(hipGetLastError());
    }
    c->n = n;
    sf::cloud_touch(c);
    return ndt_build(ndt, c);
}

extern "C" int sf_ndt_download_voxels(sf_ndt *ndt, int64_t *cell, int32_t *count, double *mean, double *cov, double *icov, int64_t cap, int64_t *n)
{
    SF_CHECK(ndt, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(ndt->has_target, SF_ERR_INVALID, "bad arguments: ndt has no target");
    const int64_t nv = ndt->n_voxels;
    if (n) *n = nv;
    SF_CHECK(cap >= nv || !(cell || count || mean || cov || icov), SF_ERR_INVALID, "bad arguments: cap %lld is below the %lld voxels", (long long)cap, (long long)nv);
    if (nv == 0) return SF_OK;
    sf_ctx *ctx = ndt->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    if (cell) SF_HIP(hipMemcpy(cell, ndt->vcell.p, sizeof(int64_t) * (size_t)nv, hipMemcpyDeviceToHost));
    if (count) SF_HIP(hipMemcpy(count, ndt->vcount.p, sizeof(int32_t) * (size_t)nv, hipMemcpyDeviceToHost));
    if (cov) SF_HIP(hipMemcpy(cov, ndt->cov.p, sizeof(double) * 6 * (size_t)nv, hipMemcpyDeviceToHost));
    if (mean || icov) {
        std::vector<double> rec((size_t)nv * NDT_VOX_STRIDE);
        SF_HIP(hipMemcpy(rec.data(), ndt->vox.p, sizeof(double) * rec.size(), hipMemcpyDeviceToHost));
        for (int64_t v = 0; v < nv; ++v) {
            const double *r = rec.data() + (size_t)v * NDT_VOX_STRIDE;
            if (mean) for (int d = 0; d < 3; ++d) mean[3 * v + d] = r[d];
            if (icov) for (int e = 0; e < 6; ++e) icov[6 * v + e] = r[3 + e];
        }
    }
    return SF_OK;
}

extern "C" int sf_ndt_set_source_batch(sf_ndt *ndt, const float *xyz, int64_t n_per_scan, int batch)
{
    SF_CHECK(ndt && n_per_scan >= 0 && (xyz || n_per_scan == 0), SF_ERR_INVALID, "bad arguments");
    SF_CHECK(batch >= 1 && batch <= NDT_MAX_BATCH, SF_ERR_INVALID, "bad arguments: ndt batch must be 1 .. 64 (got %d)", batch);
    SF_CHECK(n_per_scan < (int64_t)1 << 30, SF_ERR_INVALID, "bad arguments: ndt source of %lld points", (long long)n_per_scan);
    sf_ctx *ctx = ndt->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    const size_t bytes = sizeof(float) * 3 * (size_t)n_per_scan * (size_t)batch;
    SF_TRY(ndt->src.reserve(std::max<size_t>(bytes, 16)));
    SF_TRY(sf::upload_staged(ctx, ndt->src.p, xyz, bytes));
    ndt->n_src = n_per_scan;
    ndt->batch = batch;
    ndt->has_source = true;
    return SF_OK;
}

extern "C" int sf_ndt_set_source_cloud(sf_ndt *ndt, sf_cloud *cloud)
{
    SF_CHECK(ndt && cloud, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(cloud->ctx == ndt->ctx, SF_ERR_INVALID, "bad arguments: the cloud belongs to another context");
    SF_CHECK(cloud->n < (int64_t)1 << 30, SF_ERR_INVALID, "bad arguments: ndt source of %lld points", (long long)cloud->n);
    sf_ctx *ctx = ndt->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    const size_t bytes = sizeof(float) * 3 * (size_t)cloud->n;
    SF_TRY(ndt->src.reserve(std::max<size_t>(bytes, 16)));
    if (bytes) SF_HIP(hipMemcpyAsync(ndt->src.p, cloud->xyz.p, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    ndt->n_src = cloud->n;
    ndt->batch = 1;
    ndt->has_source = true;
    return SF_OK;
}

extern "C" int sf_ndt_derivatives(sf_ndt *ndt, const double *poses, int64_t k, sf_ndt_result *out)
{
    SF_CHECK(ndt && k >= 0 && ((poses && out) || k == 0), SF_ERR_INVALID, "bad arguments");
    SF_CHECK(ndt->has_target && ndt->has_source, SF_ERR_INVALID, "bad arguments: ndt needs a target and a source first");
    for (int64_t at = 0; at < k; at += NDT_MAX_BATCH) {
        const int chunk = (int)std::min<int64_t>(NDT_MAX_BATCH, k - at);
        SF_TRY(ndt_run(ndt, poses + 16 * at, chunk, 0, 0, true, out + at, nullptr)); // every pose reads entry 0 of the source
    }
    return SF_OK;
}

extern "C" int sf_ndt_align_batch(sf_ndt *ndt, const double *inits, sf_ndt_result *out)
{
    SF_CHECK(ndt && inits && out, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(ndt->has_target && ndt->has_source, SF_ERR_INVALID, "bad arguments: ndt needs a target and a source first");
    return ndt_run(ndt, inits, ndt->batch, 3 * (size_t)ndt->n_src, (int)ndt->prm.max_iterations, true, out, nullptr);
}

extern "C" int sf_ndt_align(sf_ndt *ndt, const double init[16], sf_ndt_result *out, double *trace)
{
    SF_CHECK(ndt && init && out, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(ndt->has_target && ndt->has_source, SF_ERR_INVALID, "bad arguments: ndt needs a target and a source first");
    return ndt_run(ndt, init, 1, 3 * (size_t)ndt->n_src, (int)ndt->prm.max_iterations, true, out, trace, true);
}

extern "C" int sf_ndt_stats_read(sf_ndt *ndt, sf_ndt_stats *out)
{
    SF_CHECK(ndt && out, SF_ERR_INVALID, "bad arguments");
    *out = sf_ndt_stats{ndt->n_points, ndt->n_cells, ndt->n_occupied, ndt->n_voxels, {0, 0, 0}, ndt->build_ms, ndt->align_ms};
    if (ndt->has_target)
        for (int d = 0; d < 3; ++d) out->dims[d] = ndt->index->grid.dim[d];
    return SF_OK;
}

extern "C" void sf_ndt_default_line_search(sf_ndt_line_search *p)
{
    if (!p) return;
    *p = sf_ndt_line_search{8, 0, 1.0, 1e-4};
}

extern "C" int sf_ndt_set_line_search(sf_ndt *ndt, const sf_ndt_line_search *p)
{
    SF_CHECK(ndt, SF_ERR_INVALID, "bad arguments");
    if (p) SF_TRY(ndt_check_line_search(p));
    if (p && p->trials > 0) ndt->ls = sf_ndt_line_search{p->trials, 0, p->step_max, p->armijo};
    else ndt->ls.trials = 0;
    return SF_OK;
}

extern "C" int sf_ndt_scores(sf_ndt *ndt, const double *poses, int64_t k, double *score, int64_t *n_terms)
{
    SF_CHECK(ndt && k >= 0 && ((poses && score && n_terms) || k == 0), SF_ERR_INVALID, "bad arguments");
    SF_CHECK(ndt->has_target && ndt->has_source, SF_ERR_INVALID, "bad arguments: ndt needs a target and a source first");
    if (k == 0) return SF_OK;
    sf_ctx *ctx = ndt->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int nblocks = (int)ndt_blocks(ndt->n_src, BLK);
    const int64_t cap = std::min<int64_t>(k, NDT_MAX_BATCH * SF_NDT_MAX_TRIALS); // poses per launch
    SF_TRY(ndt->poses.reserve(sizeof(double) * 16 * (size_t)cap));
    SF_TRY(ndt->scores.reserve(sizeof(double) * 2 * (size_t)cap));
    SF_TRY(ndt->ls_partials.reserve(sizeof(double) * REC_STRIDE * (size_t)nblocks * (size_t)cap));
    const NdtGrid g = ndt_grid(ndt);
    const NdtConst cn = ndt_constants(ndt->prm);
    std::vector<double> h(2 * (size_t)cap);
    for (int64_t at = 0; at < k; at += cap) {
        const int chunk = (int)std::min<int64_t>(cap, k - at);
        SF_TRY(sf::upload_staged(ctx, ndt->poses.p, poses + 16 * at, sizeof(double) * 16 * (size_t)chunk));
        SF_TRY(ndt_mark(ndt, 0));
        ndt_launch_scores(ndt, g, cn, chunk, 1, 0, nullptr, ndt->poses.as<double>(), 16, ndt->ls_partials.as<double>(), nblocks); // every pose reads entry 0 of the source
        hipLaunchKernelGGL(k_ndt_scores_out, dim3((unsigned)chunk), dim3(NDT_SBLK), 0, s, ndt->ls_partials.as<double>(), nblocks, ndt->scores.as<double>());
        SF_HIP(hipGetLastError());
        SF_TRY(ndt_mark(ndt, 1));
        SF_HIP(hipMemcpyAsync(h.data(), ndt->scores.p, sizeof(double) * 2 * (size_t)chunk, hipMemcpyDeviceToHost, s));
        SF_HIP(hipStreamSynchronize(s));
        SF_TRY(ndt_event_ms(ndt, &ndt->align_ms));
        for (int i = 0; i < chunk; ++i) {
            score[at + i] = h[2 * (size_t)i];
            n_terms[at + i] = (int64_t)h[2 * (size_t)i + 1];
        }
    }
    return SF_OK;
}

extern "C" int sf_ndt_line_search_read(sf_ndt *ndt, sf_ndt_ls_row *rows, int64_t cap, int64_t *n)
{
    SF_CHECK(ndt, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(ndt->has_rows, SF_ERR_STATE, "ndt: no sf_ndt_align with the line search on has run");
    const int64_t have = (int64_t)ndt->rows.size();
    if (n) *n = have;
    SF_CHECK(!rows || cap >= have, SF_ERR_INVALID, "bad arguments: cap %lld is below the %lld rows", (long long)cap, (long long)have);
    if (rows) std::copy(ndt->rows.begin(), ndt->rows.end(), rows);
    return SF_OK;
}

extern "C" int sf_ndt_align_levels(sf_ndt *const *levels, int n_levels, const double *inits, sf_ndt_result *out, sf_ndt_result *per_level)
{
    SF_CHECK(levels && inits && out, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(n_levels >= 1, SF_ERR_INVALID, "bad arguments: ndt needs at least one level (got %d)", n_levels);
    for (int l = 0; l < n_levels; ++l) {
        const sf_ndt *a = levels[l], *f = levels[0];
        SF_CHECK(a, SF_ERR_INVALID, "bad arguments");
        SF_CHECK(a->has_target && a->has_source, SF_ERR_INVALID, "bad arguments: ndt level %d needs a target and a source first", l);
        SF_CHECK(a->ctx == f->ctx, SF_ERR_INVALID, "bad arguments: ndt level %d belongs to another context", l);
        SF_CHECK(a->batch == f->batch && a->n_src == f->n_src, SF_ERR_INVALID, "bad arguments: ndt level %d holds %d scans of %lld points, level 0 %d of %lld", l, a->batch,
                 (long long)a->n_src, f->batch, (long long)f->n_src);
    }
    const int batch = levels[0]->batch;
    std::vector<double> poses(inits, inits + 16 * (size_t)batch);
    std::vector<sf_ndt_result> res((size_t)batch);
    for (int l = 0; l < n_levels; ++l) {
        sf_ndt *ndt = levels[l];
        SF_TRY(ndt_run(ndt, poses.data(), batch, 3 * (size_t)ndt->n_src, (int)ndt->prm.max_iterations, true, res.data(), nullptr));
        for (int b = 0; b < batch; ++b) {
            for (int i = 0; i < 16; ++i) poses[16 * (size_t)b + i] = res[(size_t)b].T[i];
            if (per_level) per_level[(size_t)l * batch + b] = res[(size_t)b];
        }
    }
    for (int b = 0; b < batch; ++b) out[b] = res[(size_t)b];
    return SF_OK;
}
