// sf_icp_order_host.hpp -- the host side of the query order: which alignments go tile by tile and with which tiles (tile_plan,
// tile_wanted), the key table of the attached index (order_lut_build, order_lut_prepare), the launches of the plain path
// (launch_order_plain), the segmented sort (run_order_sort) and order_queries.
// A fragment, not a stand-alone header: sf_icp.hip includes it at file scope, after sf_icp_object.hpp.  It launches the k_order_*,
// k_order_lut_* and k_tile_* kernels of sf_icp.hip's device code with that code's CellKeyFn, TileKeyFn, IcpState, nblk, GATHER_TILE,
// ORDER_LUT_LOG2, TILE_KEY_NONE and TILE_STATS, and uses Lane, SrcSet, soa(), robust_on(), order_span() and order_key_shift()
// (sf_icp_object.hpp).

namespace {

// ---- tile search: which alignments, which tiles
// The searching launches of a batch go tile by tile when there is enough work to amortise staging every tile that holds a
// query and the second sorting pass (measured break-even: TILE_AUTO_MIN_QUERIES), on the whole map (no window), unsharded,
// with the queries ordered.  Tile shape: cells per axis such that the staged region (core + 2 cells all round) holds about
// 3/4 of TILE_PCAP points at the map's mean density -- 8 x 8 x 4 cells at the metric configuration (0.25 m cells, 1.5 points
// per cell: 12 x 12 x 8 = 1 152 staged cells, ~1 700 points) -- within the limits of the LDS tables.
constexpr int64_t TILE_AUTO_MIN_QUERIES = 2000000;
bool tile_plan(const SfGrid &g, sf::SfTiles *out)
{
    const double ncell = (double)g.dim[0] * (double)g.dim[1] * (double)g.dim[2];
    if (g.n <= 0 || ncell <= 0) return false;
    const double density = (double)g.n / ncell; // points per cell (empty space included: an upper-bound-free mean; denser tiles fall back one by one)
    int tc[3] = {8, 8, 4};
    auto region_cells = [&](const int *c) { return (double)(c[0] + 2 * sf::TILE_HALO) * (c[1] + 2 * sf::TILE_HALO) * (c[2] + 2 * sf::TILE_HALO); };
    auto fits_tables = [&](const int *c) { return c[0] + 2 * sf::TILE_HALO <= sf::TILE_RX_MAX && (c[1] + 2 * sf::TILE_HALO) * (c[2] + 2 * sf::TILE_HALO) <= sf::TILE_ROWS_MAX; };
    const double budget = 0.75 * sf::TILE_PCAP;
    while (region_cells(tc) * density > budget) { // shrink the longest axis
        int a = tc[0] >= tc[1] && tc[0] >= tc[2] ? 0 : (tc[1] >= tc[2] ? 1 : 2);
        if (tc[a] <= 2) return false; // too dense for any tile: the global index
        tc[a] /= 2;
    }
    for (;;) { // grow the shortest axis while there is room (sparse maps)
        int a = tc[2] <= tc[1] && tc[2] <= tc[0] ? 2 : (tc[1] <= tc[0] ? 1 : 0);
        int t2[3] = {tc[0], tc[1], tc[2]};
        t2[a] *= 2;
        if (!fits_tables(t2) || region_cells(t2) * density > budget) break;
        tc[0] = t2[0]; tc[1] = t2[1]; tc[2] = t2[2];
    }
    if (!fits_tables(tc)) return false;
    sf::SfTiles tl;
    int64_t nt = 1;
    for (int a = 0; a < 3; ++a) {
        tl.tc[a] = tc[a];
        tl.nt[a] = (g.dim[a] + tc[a] - 1) / tc[a];
        nt *= tl.nt[a];
    }
    if (nt >= (int64_t)TILE_KEY_NONE) return false;
    tl.ntiles = (int)nt;
    *out = tl;
    return true;
}

bool tile_wanted(const sf_icp *icp, int mode)
{
    const SrcSet &ss = icp->src();
    // (k_red_cached sums unit weights: under a robust kernel the searching launches stay with k_nn_red_rob)
    if (icp->tile_mode == 0 || robust_on(icp, mode) || icp->shard || icp->map->window.kind != 0 || (mode != SF_ICP_P2PLANE && mode != SF_ICP_O3D_P2P)) return false;
    if (ss.qpl == 1) return false; // scans the single-launch kernels can take keep their summation order (and their launch list)
    return icp->tile_mode == 2 || ss.n * ss.batch >= TILE_AUTO_MIN_QUERIES;
}

// The key table of the attached index (k_order_lut_*), (re)built when the index has changed.  Enqueued on the context's stream
// BEFORE an alignment takes a lane: the lanes order themselves behind the context's stream whenever the target changes
// (LaneScope), so both see the finished table.
constexpr int ORDER_LUT_BINS = (1 << ORDER_LUT_LOG2) + 1;
// the table of index g into buf (histogram, then the keys), enqueued on st; *shift: what CellKeyFn::lut_shift takes
int order_lut_build(hipStream_t st, const SfGrid &g, sf::DevBuf &buf, int *shift)
{
    const OrderSpan sp = order_span(g);
    *shift = std::max(0, sp.bits - ORDER_LUT_LOG2);
    const int nbins = (int)(sp.cells >> *shift) + 1;
    SF_TRY(buf.reserve(sizeof(uint32_t) * (size_t)ORDER_LUT_BINS + sizeof(uint16_t) * (size_t)ORDER_LUT_BINS));
    uint32_t *hist = buf.as<uint32_t>();
    uint16_t *lut = reinterpret_cast<uint16_t *>(hist + ORDER_LUT_BINS);
    SF_HIP(hipMemsetAsync(hist, 0, sizeof(uint32_t) * (size_t)ORDER_LUT_BINS, st));
    hipLaunchKernelGGL(k_order_lut_hist, dim3(nblk(g.n)), dim3(256), 0, st, g, *shift, hist);
    hipLaunchKernelGGL(k_order_lut_make, dim3(1), dim3(1024), 0, st, hist, nbins, (uint32_t)g.n, lut);
    SF_HIP(hipGetLastError());
    return SF_OK;
}
int order_lut_prepare(sf_icp *icp)
{
    if (!icp->order_lut_on || !icp->map || !icp->map->built) return SF_OK;
    const SfGrid &g = icp->map->grid;
    if (g.n <= 0 || (icp->order_lut.p && icp->order_lut_gen == icp->map->generation)) return SF_OK;
    SF_TRY(order_lut_build(icp->ctx->stream, g, icp->order_lut, &icp->order_lut_shift));
    icp->order_lut_gen = icp->map->generation;
    return SF_OK;
}

// The plain path of the sort: uniform segments (src.nseg scans of src.n queries in element order), one 10-bit digit.
// k_order_hist -> k_order_scan -> form 1: k_order_move (x0 -> xq in one pass, no ids); form 0: k_order_scatter + k_order_gather
// through `ids` and the float4 records `rec` (what the sharded start and the tile sort still run, and what sf_test_query_order
// compares the move kernel with).  x0 / xq: the three planes of the scans as given / in cell order.
void launch_order_plain(hipStream_t s, const sf::OrderSrc &src, const CellKeyFn &kf, uint16_t *keys, uint32_t *counts, int form, uint32_t *ids, const float4 *rec,
                        float *const xq[3])
{
    const dim3 grid(sf::order_grid(src.tiles, src.nseg)), blk(sf::ORD_BLK);
    hipLaunchKernelGGL(k_order_hist, grid, blk, 0, s, src, kf, keys, counts);
    hipLaunchKernelGGL(sf::k_order_scan, dim3((unsigned)src.nseg), dim3(sf::ORD_BINS), 0, s, counts, src.tiles);
    if (form == 1) {
        hipLaunchKernelGGL(k_order_move, grid, blk, 0, s, src, keys, counts, kf.x, kf.y, kf.z, xq[0], xq[1], xq[2]);
        return;
    }
    hipLaunchKernelGGL(k_order_scatter, grid, blk, 0, s, src, keys, counts, ids);
    const int gt = (int)std::max<int64_t>(1, sf::div_up(src.n, GATHER_TILE));
    hipLaunchKernelGGL(k_order_gather, dim3(sf::order_grid(gt, src.nseg)), dim3(256), 0, s, rec, ids, (int64_t)src.n * src.nseg, src.n, gt, src.nseg, xq[0], xq[1], xq[2]);
}

// the segmented stable bucket sort of sf_order.hpp: nseg segments (uniform: nseg scans of n queries; sharded: the
// owned-query candidates of each scan, seg_off / src_idx on the device), `longest` = the longest segment
int run_order_sort(sf_icp *icp, int nseg, int64_t longest, int64_t total, const uint32_t *seg_off, const uint32_t *src_idx)
{
    Lane &ln = icp->cur(); SrcSet &ss = icp->src();
    const SfGrid &g = icp->map->grid;
    if (seg_off) icp->tile_on = false; // (the sharded path's owned-query arrays keep the cell order)
    sf::OrderSrc src;
    src.src_idx = src_idx;
    src.seg_off = seg_off;
    src.n = (int)ss.n;
    src.tiles = (int)std::max<int64_t>(1, sf::div_up(longest, sf::ORD_TILE));
    CellKeyFn kf;
    kf.g = g;
    kf.x = soa(ss.X0, ss.plane, 0); kf.y = soa(ss.X0, ss.plane, 1); kf.z = soa(ss.X0, ss.plane, 2);
    kf.st = ln.state.as<IcpState>();
    kf.shift = order_key_shift(g);
    kf.lut = nullptr;
    kf.lut_shift = 0;
    if (icp->order_lut_on && icp->order_lut.p && icp->order_lut_gen == icp->map->generation) { // (prepared by order_lut_prepare; otherwise the plain key)
        kf.lut = reinterpret_cast<const uint16_t *>(icp->order_lut.as<uint32_t>() + ORDER_LUT_BINS);
        kf.lut_shift = icp->order_lut_shift;
    }
    const size_t cap = (size_t)std::max<int64_t>(total, 1);
    SF_TRY(ln.Xq.reserve(sizeof(float) * 3 * std::max(cap, (size_t)(seg_off ? 0 : ss.plane))));
    SF_TRY(ln.qkeys.reserve(sizeof(uint16_t) * cap));                                                      // bucket key of every element
    SF_TRY(ln.qkeys2.reserve(sizeof(uint32_t) * (size_t)nseg * (size_t)(src.tiles + 1) * sf::ORD_BINS));  // per-tile bucket counts / starts
    uint16_t *keys = ln.qkeys.as<uint16_t>();
    uint32_t *counts = ln.qkeys2.as<uint32_t>();
    hipStream_t s = icp->ctx->stream;
    src.nseg = nseg;
    if (!icp->tile_on && !seg_off && !src_idx) { // the plain path: ranked and moved in one pass, no ids (and no qidx: 4 bytes per query and lane)
        float *const xq[3] = {soa(ln.Xq, ss.plane, 0), soa(ln.Xq, ss.plane, 1), soa(ln.Xq, ss.plane, 2)};
        launch_order_plain(s, src, kf, keys, counts, 1, nullptr, nullptr, xq);
        SF_HIP(hipGetLastError());
        return SF_OK;
    }
    // the sharded start (seg_off / src_idx) and the two-digit tile sort need the ids between their passes
    SF_TRY(ln.qidx.reserve(sizeof(uint32_t) * cap));                                                       // ordered query ids
    uint32_t *ordered = ln.qidx.as<uint32_t>();
    const dim3 grid(sf::order_grid(src.tiles, nseg)), blk(sf::ORD_BLK);
    if (icp->tile_on) { // by map tile: a 20-bit key, least significant 10-bit digit first (stable passes)
        TileKeyFn tk;
        tk.g = g; tk.tl = icp->tiles;
        tk.x = kf.x; tk.y = kf.y; tk.z = kf.z;
        tk.st = kf.st; tk.n = (int)ss.n;
        const bool two = icp->tiles.ntiles > sf::ORD_BINS;
        uint32_t *first = ordered;
        if (two) {
            SF_TRY(ln.qidx2.reserve(sizeof(uint32_t) * cap));
            first = ln.qidx2.as<uint32_t>();
        }
        tk.digit = 0;
        hipLaunchKernelGGL(k_order_hist_tile, grid, blk, 0, s, src, tk, keys, counts);
        hipLaunchKernelGGL(sf::k_order_scan, dim3((unsigned)nseg), dim3(sf::ORD_BINS), 0, s, counts, src.tiles);
        hipLaunchKernelGGL(k_order_scatter, grid, blk, 0, s, src, keys, counts, first);
        if (two) {
            sf::OrderSrc src2 = src;
            src2.src_idx = first;
            tk.digit = 1;
            hipLaunchKernelGGL(k_order_hist_tile, grid, blk, 0, s, src2, tk, keys, counts);
            hipLaunchKernelGGL(sf::k_order_scan, dim3((unsigned)nseg), dim3(sf::ORD_BINS), 0, s, counts, src2.tiles);
            hipLaunchKernelGGL(k_order_scatter, grid, blk, 0, s, src2, keys, counts, ordered);
        }
    } else {
        hipLaunchKernelGGL(k_order_hist, grid, blk, 0, s, src, kf, keys, counts);
        hipLaunchKernelGGL(sf::k_order_scan, dim3((unsigned)nseg), dim3(sf::ORD_BINS), 0, s, counts, src.tiles);
        hipLaunchKernelGGL(k_order_scatter, grid, blk, 0, s, src, keys, counts, ordered);
    }
    const int64_t qplane = seg_off ? total : ss.plane; // sharded: the compact arrays have their own length
    if (seg_off) {
        hipLaunchKernelGGL(k_order_gather, dim3(nblk(total, GATHER_TILE)), dim3(256), 0, s, ss.X0r.as<float4>(), ordered, total, 0, 0, 0, soa(ln.Xq, qplane, 0),
                           soa(ln.Xq, qplane, 1), soa(ln.Xq, qplane, 2));
    } else {
        const int gt = (int)std::max<int64_t>(1, sf::div_up(ss.n, GATHER_TILE));
        hipLaunchKernelGGL(k_order_gather, dim3(sf::order_grid(gt, nseg)), dim3(256), 0, s, ss.X0r.as<float4>(), ordered, total, (int)ss.n, gt, nseg,
                           soa(ln.Xq, qplane, 0), soa(ln.Xq, qplane, 1), soa(ln.Xq, qplane, 2));
    }
    if (icp->tile_on) { // where each tile's queries start in every scan's ordered array
        TileKeyFn tk;
        tk.g = g; tk.tl = icp->tiles;
        tk.x = soa(ln.Xq, qplane, 0); tk.y = soa(ln.Xq, qplane, 1); tk.z = soa(ln.Xq, qplane, 2);
        tk.st = kf.st; tk.n = (int)ss.n; tk.digit = 0;
        const int64_t rows = (int64_t)icp->tiles.ntiles + 1;
        SF_TRY(ln.qtkey.reserve(sizeof(uint32_t) * cap));
        SF_TRY(ln.tseg.reserve(sizeof(uint32_t) * (size_t)rows * (size_t)nseg));
        SF_TRY(ln.tile_stats.reserve(sizeof(unsigned long long) * TILE_STATS));
        SF_HIP(hipMemsetAsync(ln.tile_stats.p, 0, sizeof(unsigned long long) * TILE_STATS, s));
        hipLaunchKernelGGL(k_tile_keys, dim3(nblk(total)), dim3(256), 0, s, tk, total, ln.qtkey.as<uint32_t>());
        hipLaunchKernelGGL(k_tile_starts, dim3(nblk(rows * nseg)), dim3(256), 0, s, ln.qtkey.as<uint32_t>(), (int)ss.n, nseg, icp->tiles.ntiles, ln.tseg.as<uint32_t>());
    }
    SF_HIP(hipGetLastError());
    return SF_OK;
}

int order_queries(sf_icp *icp, int mode)
{
    SrcSet &ss = icp->src();
    const int64_t total = ss.n * ss.batch;
    const bool want = icp->order == SF_ORDER_CELL || (icp->order == SF_ORDER_AUTO && total >= ORDER_AUTO_MIN_QUERIES);
    icp->ordered = false;
    icp->tile_on = false;
    if (!want || total == 0 || icp->map->grid.n == 0 || ss.n_on_device) return SF_OK; // (a count left on the device: the tail of the arrays is not data)
    icp->tile_on = tile_wanted(icp, mode) && tile_plan(icp->map->grid, &icp->tiles);
    SF_TRY(run_order_sort(icp, ss.batch, ss.n, total, nullptr, nullptr));
    icp->ordered = true;
    return SF_OK;
}

} // namespace
