// sf_map.hip — device-resident uniform-grid index over the WHOLE map (gfx950).
//
// Replaces ICPPointToPoint::setTargetPointCloud (localization/src/icp_point_to_point.cpp:
// 49-55: deep copy + FLANN kd-tree over a 10 m crop, rebuilt every 3 m of travel,
// localization/src/localization_node.cpp:299-305).  The map is indexed once; the crop
// becomes a window predicate (sf_map_window_*).  Layout in HBM:
//   pts4[n]       float4  x, y, z, bitcast(original index), sorted by cell id (x fastest)
//   cell_start[ncell+1] u32  first sorted position of each cell
//   nrm4[n]       float4  normal xyz + neighbour count (sorted order), optional
#include "sf_common.hpp"
#include "sf_nn.hpp"
#include "sf_knn.hpp"
#include "sf_walk.hpp"

#include "sf_sort.hpp"
#include <cmath>
#include <cstring>

namespace {

inline unsigned nblk(int64_t n, int b = 256) { return (unsigned)sf::div_up(n > 0 ? n : 1, b); }

struct GridGeom { float org[3]; float inv_h; int dim[3]; uint64_t ncell; };

// sf_map_profile_launches: events around the launches of a query / estimate call, read (prof_read) after the call's own
// synchronise.  The span closes at end() or, on a return before it, when the scope is left: the next call never starts inside one.
struct ProfSpan {
    sf_map *m;
    bool open = true;
    explicit ProfSpan(sf_map *map) : m(map)
    {
        if (!m->profile) return;
        for (int i = 0; i < 2; ++i) // (each on its own: one that could not be created is tried again, never recorded on)
            if (!m->prof_ev[i] && hipEventCreate(&m->prof_ev[i]) != hipSuccess) { m->prof_ev[i] = nullptr; m->profile = false; return; }
        hipError_t e = hipEventRecord(m->prof_ev[0], m->ctx->stream);
        (void)e;
    }
    ProfSpan(const ProfSpan &) = delete;
    ProfSpan &operator=(const ProfSpan &) = delete;
    void end()
    {
        if (!open) return;
        open = false;
        if (!m->profile) return;
        hipError_t e = hipEventRecord(m->prof_ev[1], m->ctx->stream);
        (void)e;
    }
    ~ProfSpan() { end(); }
};
inline void prof_read(sf_map *m)
{
    float ms = -1.0f;
    if (m->profile && hipEventElapsedTime(&ms, m->prof_ev[0], m->prof_ev[1]) == hipSuccess) m->last_launch_ms = ms;
}

// n (+ n2) 8-byte words from the device into ctx->h_pinned->readback, one run after the other; synchronises the stream
int read_words(sf_ctx *ctx, const void *d, int n, const void *d2 = nullptr, int n2 = 0)
{
    unsigned long long *h = ctx->h_pinned->readback;
    SF_HIP(hipGetLastError());
    SF_HIP(hipMemcpyAsync(h, d, sizeof(unsigned long long) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (n2 > 0) SF_HIP(hipMemcpyAsync(h + n, d2, sizeof(unsigned long long) * (size_t)n2, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    return SF_OK;
}

// K = uint32_t while the grid has fewer than 2^32 cells, uint64_t beyond (large sparse extents: a dense table over
// 1 km x 1 km x 100 m at 0.25 m is 6.4e9 cells = 25.6 GB of the 288 GB)
template <class K>
__global__ void k_cell_keys(const float *__restrict__ xyz, int64_t n, GridGeom g, K *__restrict__ keys, uint32_t *__restrict__ vals)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    K key = (K)g.ncell; // non-finite points sort last and are not indexed (PCL drops them too)
    if (isfinite(x) && isfinite(y) && isfinite(z)) {
        const int cx = sf::grid_cell((x - g.org[0]) * g.inv_h, g.dim[0]), cy = sf::grid_cell((y - g.org[1]) * g.inv_h, g.dim[1]), cz = sf::grid_cell((z - g.org[2]) * g.inv_h, g.dim[2]);
        key = ((K)cz * (K)g.dim[1] + (K)cy) * (K)g.dim[0] + (K)cx;
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
}

// Large tables: a point must not fill the empty cells in front of it one by one (a gap can be billions of cells).  The
// END of every non-empty cell is written to the entry of the cell after it (t[key + 1] = position after the run), the
// rest stays 0, and an inclusive MAX scan turns that into cell_start: the largest end among the cells before c is the
// first sorted position whose key is >= c.
template <class K>
__global__ void k_cell_tails(const K *__restrict__ keys, int64_t n_valid, uint32_t *__restrict__ cell_start)
{
    int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_valid) return;
    const K k = keys[j];
    if (j == n_valid - 1 || keys[j + 1] != k) cell_start[(size_t)k + 1] = (uint32_t)(j + 1);
}

__global__ void k_carry_max(uint32_t *__restrict__ p) { p[0] = max(p[0], p[-1]); }

__global__ void k_gather_sorted(const float *__restrict__ xyz, const uint32_t *__restrict__ vals, int64_t n, float4 *__restrict__ pts4)
{
    int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    uint32_t i = vals[j];
    pts4[j] = make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], __uint_as_float(i));
}

// cell_start[c] = first sorted position whose key >= c, for c in [0, ncell] (tables below 2^28 cells: the gaps are short)
__global__ void k_cell_bounds(const uint32_t *__restrict__ keys, int64_t n_valid, uint32_t ncell, uint32_t *__restrict__ cell_start)
{
    int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_valid) return;
    uint32_t k = keys[j];
    uint32_t prev_next = j == 0 ? 0u : keys[j - 1] + 1u;
    for (uint32_t c = prev_next; c <= k; ++c) cell_start[c] = (uint32_t)j;
    if (j == n_valid - 1)
        for (uint32_t c = k + 1; c <= ncell; ++c) cell_start[c] = (uint32_t)n_valid;
}

__global__ void k_fill_u32(uint32_t *p, int64_t n, uint32_t v)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

} // namespace

// SfGrid / SfWindow are passed to kernels by value
namespace {
template <bool WINDOW>
__global__ __launch_bounds__(256) void k_map_nn_t(SfGrid g, SfWindow w, const float *__restrict__ q, int64_t n, float thr, int32_t *__restrict__ idx,
                                                 float *__restrict__ d2)
{
    // the wave-cooperative search of the ICP kernel (every lane of the wave takes part, with or without a query)
    __shared__ sf::WaveNN ws[256 / 64];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n;
    const float qx = valid ? q[3 * i] : 0.0f, qy = valid ? q[3 * i + 1] : 0.0f, qz = valid ? q[3 * i + 2] : 0.0f;
    const sf::NNHit hit = sf::nn_search_wave<WINDOW, true>(g, w, valid, qx, qy, qz, thr, &ws[threadIdx.x >> 6]);
    if (!valid) return;
    idx[i] = hit.j >= 0 ? (int32_t)__float_as_uint(g.pts[hit.j].w) : -1;
    d2[i] = hit.j >= 0 ? hit.d2 : INFINITY;
}
} // namespace

namespace {
// The grid's origin: the smallest coordinate, or -- sf_map_set_origin_lattice -- that coordinate snapped DOWN to a multiple of
// `lattice` cells, so that a map which grows by a few metres in ANY direction keeps its origin, every point its cell
// coordinates and the index its order (sf_map_patch).  The result is a float <= mn.
inline float grid_origin(float mn, double h, int lattice)
{
    if (lattice <= 0) return mn;
    const double step = (double)lattice * h;
    return (float)(std::floor((double)mn / step) * step);
}

inline bool table_by_scan(uint64_t ncell, int64_t n_points, int lattice) { return ncell > (1ull << 28) || lattice > 0 || ncell > 16ull * (uint64_t)std::max<int64_t>(n_points, 1); }

// cell_start[0 .. ncell] (+ pads) from the sorted keys of the n_valid indexed points; the buffer is reserved by the caller
int build_cell_table(sf_map *m, const GridGeom &g, const void *sorted_keys, int64_t n_valid, bool wide, bool by_scan)
{
    sf_ctx *ctx = m->ctx;
    hipStream_t st = ctx->stream;
    uint32_t *cs = m->cell_start.as<uint32_t>() + 1;
    if (by_scan && n_valid > 0) {
        // [pad = 0 | t[0..ncell] | pads]: ends of the non-empty cells, then an inclusive max scan in pieces of 2^30 entries
        // (the carry is the entry before the piece); the trailing pads come out as n_valid like the rest of the tail
        const size_t entries = (size_t)g.ncell + 8;
        SF_HIP(hipMemsetAsync(m->cell_start.p, 0, sizeof(uint32_t) * entries, st));
        if (wide) hipLaunchKernelGGL(k_cell_tails<uint64_t>, dim3(nblk(n_valid)), dim3(256), 0, st, static_cast<const uint64_t *>(sorted_keys), n_valid, cs);
        else hipLaunchKernelGGL(k_cell_tails<uint32_t>, dim3(nblk(n_valid)), dim3(256), 0, st, static_cast<const uint32_t *>(sorted_keys), n_valid, cs);
        const size_t piece = (size_t)1 << 30;
        uint32_t *t = m->cell_start.as<uint32_t>();
        for (size_t off = 0; off < entries; off += piece) {
            const size_t len = std::min(piece, entries - off);
            if (off > 0) hipLaunchKernelGGL(k_carry_max, dim3(1), dim3(1), 0, st, t + off);
            SF_TRY(sf::scan_u32<1>(ctx, t + off, t + off, (int64_t)len)); // (the carry of a later piece sits in its first entry: k_carry_max)
        }
    } else {
        hipLaunchKernelGGL(k_fill_u32, dim3(nblk((int64_t)g.ncell + 8)), dim3(256), 0, st, m->cell_start.as<uint32_t>(), (int64_t)g.ncell + 8, (uint32_t)n_valid);
        SF_HIP(hipMemsetAsync(m->cell_start.p, 0, sizeof(uint32_t), st));
        if (n_valid > 0)
            hipLaunchKernelGGL(k_cell_bounds, dim3(nblk(n_valid)), dim3(256), 0, st, static_cast<const uint32_t *>(sorted_keys), n_valid, (uint32_t)g.ncell, cs);
        else
            hipLaunchKernelGGL(k_fill_u32, dim3(nblk((int64_t)g.ncell + 2)), dim3(256), 0, st, cs, (int64_t)g.ncell + 2, 0u);
    }
    return SF_OK;
}
} // namespace

extern "C" int sf_map_create(sf_ctx *ctx, sf_map **out)
{
    SF_CHECK(ctx && out, SF_ERR_INVALID, "bad arguments");
    sf_map *m = new (std::nothrow) sf_map();
    SF_CHECK(m, SF_ERR_NOMEM, "out of host memory");
    m->ctx = ctx;
    sf::ctx_retain(ctx);
    *out = m;
    return SF_OK;
}

extern "C" void sf_map_destroy(sf_map *m)
{
    if (!m) return;
    hipError_t e = hipStreamSynchronize(m->ctx->stream);
    (void)e;
    m->pts4.release(); m->nrm4.release(); m->cov6.release(); m->d_window.release(); m->cell_start.release(); m->keys.release(); m->vals.release();
    m->keys2.release(); m->vals2.release(); m->pts4_alt.release(); m->patch_tmp.release();
    m->nrm4_alt.release(); m->cov6_alt.release(); m->carry_tmp.release(); m->carry_list.release();
    for (hipEvent_t ev : m->prof_ev)
        if (ev) { hipError_t e2 = hipEventDestroy(ev); (void)e2; }
    for (hipEvent_t ev : m->nbr_ev)
        if (ev) { hipError_t e2 = hipEventDestroy(ev); (void)e2; }
    m->nbr.release();
    m->out_flags.release(); m->out_val.release(); m->out_red.release();
    m->cl.release();
    m->rad_cnt.release(); m->rad_off.release(); m->rad_red.release(); m->rad_ids.release(); m->rad_ids_alt.release(); m->rad_d2.release();
    m->rad_keys.release(); m->rad_keys_alt.release(); m->rad_q.release();
    for (hipEvent_t ev : m->rad_ev)
        if (ev) { hipError_t e2 = hipEventDestroy(ev); (void)e2; }
    sf_ctx *ctx = m->ctx;
    delete m;
    sf::ctx_release(ctx);
}

extern "C" int sf_map_build(sf_map *m, sf_cloud *cloud, float cell)
{
    SF_CHECK(m && cloud, SF_ERR_INVALID, "bad arguments");
    // the search addresses candidates through a buffer descriptor (byte offsets and size in 32 bits, sf_nn.hpp)
    SF_CHECK(cloud->n < (int64_t)(1 << 28), SF_ERR_OVERFLOW, "map too large for one GPU index (2^28 points): shard it");
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t n = cloud->n;
    m->built = false;
    m->has_normals = false;
    m->nrm_estimated = false; // (sf_map_patch remembers the estimate it carries before it comes here)
    m->nrm_knn_k = 0;
    m->n = 0;
    m->window.kind = 0;
    const float *xyz = cloud->xyz.as<float>();

    // 1. bounds of the finite points
    sf::MinMaxHost mm;
    if (n > 0 && cloud->stamp != 0 && cloud->bounds_stamp == cloud->stamp) { // left behind by a voxel merge: all points finite, nothing has changed since
        for (int d = 0; d < 3; ++d) { mm.mn[d] = cloud->bounds_mn[d]; mm.mx[d] = cloud->bounds_mx[d]; }
        mm.n_finite = n;
    } else {
        SF_TRY(sf::cloud_minmax(ctx, xyz, n, &mm));
    }
    const int64_t n_valid = mm.n_finite;

    // 2. geometry: automatic cell ~ 1.5 points per cell, clamped; grow until it fits u32
    double ext[3];
    for (int d = 0; d < 3; ++d) ext[d] = n_valid > 0 ? (double)mm.mx[d] - (double)mm.mn[d] : 0.0;
    double h = cell;
    if (!(h > 0)) {
        double vol = std::max(ext[0], 1e-3) * std::max(ext[1], 1e-3) * std::max(ext[2], 1e-3);
        h = std::cbrt(1.5 * vol / (double)std::max<int64_t>(n_valid, 1));
        h = std::min(std::max(h, 0.05), 1.0e6);
    }
    // the dense cell table may take a quarter of what the device has free (288 GB HBM: a 1 km x 1 km x 100 m extent at
    // 0.25 m is 6.4e9 cells = 25.6 GB), never more than 2^35 cells; automatic sizing grows the cell until it fits, an
    // explicit cell that does not fit is refused
    size_t free_b = 0, total_b = 0;
    SF_HIP(hipMemGetInfo(&free_b, &total_b));
    const double max_cells = std::min(34359738368.0, std::max(1.0e9, (double)free_b / 4.0 / sizeof(uint32_t)));
    int dim[3];
    float org[3] = {0, 0, 0};
    for (;;) {
        h = (double)(float)h; // the cell is a float32 everywhere else (sf_map_cell_size, SfGrid::h): a rebuild with the reported cell is the same index
        double cells = 1;
        bool ok = true;
        for (int d = 0; d < 3; ++d) {
            org[d] = n_valid > 0 ? grid_origin(mm.mn[d], h, m->origin_lattice) : 0.0f;
            double c = std::floor((n_valid > 0 ? (double)mm.mx[d] - (double)org[d] : 0.0) / h) + 1;
            if (c > 16777216.0) ok = false; // grid_cell clamps with (float)(dim - 1): beyond 2^24 cells that float can be dim itself, a cell past the grid
            dim[d] = ok ? (int)c : 1;
            cells *= c;
        }
        if (ok && cells <= max_cells) break;
        SF_CHECK(cell <= 0, SF_ERR_OVERFLOW, "cell %.4g gives too many cells for this extent (%.3g; this device holds a table of %.3g, an axis 2^24 cells)", (double)cell, cells, max_cells);
        h *= 1.5;
    }
    GridGeom g;
    for (int d = 0; d < 3; ++d) { g.org[d] = org[d]; g.dim[d] = dim[d]; }
    g.inv_h = (float)(1.0 / h);
    g.ncell = (uint64_t)dim[0] * (uint64_t)dim[1] * (uint64_t)dim[2];
    const bool wide = g.ncell >= 0xffffffffull;     // keys (cell ids, ncell itself for non-finite points) no longer fit 32 bits
    // long empty stretches -- a large or sparsely filled table, the margin in front of a snapped origin (whole empty layers) --:
    // bounds by scan (k_cell_bounds has ONE lane walk the gap in front of its point: 0.2 s for 16 M empty cells)
    const bool by_scan = table_by_scan(g.ncell, n_valid, m->origin_lattice);

    // 3. keys -> stable radix sort -> gather
    const size_t np = (size_t)std::max<int64_t>(n, 1), ksz = wide ? sizeof(uint64_t) : sizeof(uint32_t);
    SF_TRY(m->keys.reserve(ksz * np));
    SF_TRY(m->vals.reserve(sizeof(uint32_t) * np));
    SF_TRY(m->keys2.reserve(ksz * np));
    SF_TRY(m->vals2.reserve(sizeof(uint32_t) * np));
    SF_TRY(m->pts4.reserve(sizeof(float4) * np));
    SF_TRY(m->cell_start.reserve(sizeof(uint32_t) * ((size_t)g.ncell + 8))); // [pad | start[0..ncell] | pad..]: sf_nn.hpp reads start[c-1..c+2] in one load
    const void *sorted_keys = m->keys2.p; // where the sort leaves its result (either ping-pong buffer)
    uint32_t *sorted_vals = m->vals2.as<uint32_t>();
    if (n > 0) {
        unsigned bits = 1;
        while (bits < 64 && (1ull << bits) <= (unsigned long long)g.ncell) ++bits;
        // stable: points of a cell stay in ascending point id (deterministic in-cell order => deterministic tie-breaks)
        if (wide) {
            hipLaunchKernelGGL(k_cell_keys<uint64_t>, dim3(nblk(n)), dim3(256), 0, st, xyz, n, g, m->keys.as<uint64_t>(), m->vals.as<uint32_t>());
            uint64_t *sk = nullptr;
            SF_TRY(sf::radix_sort_pairs<uint64_t>(ctx, m->keys.as<uint64_t>(), m->keys2.as<uint64_t>(), m->vals.as<uint32_t>(), m->vals2.as<uint32_t>(), n, bits, &sk, &sorted_vals));
            sorted_keys = sk;
        } else {
            hipLaunchKernelGGL(k_cell_keys<uint32_t>, dim3(nblk(n)), dim3(256), 0, st, xyz, n, g, m->keys.as<uint32_t>(), m->vals.as<uint32_t>());
            uint32_t *sk = nullptr;
            SF_TRY(sf::radix_sort_pairs<uint32_t>(ctx, m->keys.as<uint32_t>(), m->keys2.as<uint32_t>(), m->vals.as<uint32_t>(), m->vals2.as<uint32_t>(), n, bits, &sk, &sorted_vals));
            sorted_keys = sk;
        }
        hipLaunchKernelGGL(k_gather_sorted, dim3(nblk(n)), dim3(256), 0, st, xyz, sorted_vals, n, m->pts4.as<float4>());
    }
    SF_TRY(build_cell_table(m, g, sorted_keys, n_valid, wide, by_scan));
    SF_HIP(hipGetLastError());
    SF_HIP(hipStreamSynchronize(st));

    m->n = n;
    SfGrid &G = m->grid;
    for (int d = 0; d < 3; ++d) { G.org[d] = g.org[d]; G.dim[d] = dim[d]; }
    G.inv_h = g.inv_h;
    G.h = (float)h;
    // |computed grid coordinate - true one| <= 2^-23 * coordinate for the point and for the query, so a
    // face distance derived from them can be too long by 2^-22 * (largest coordinate) cells; 1.5 x for the
    // roundings of the gap arithmetic itself.  Every pruning decision of the search subtracts it (sf_nn.hpp).
    G.gap_eps = 1.5f * 2.384186e-7f * (float)std::max(dim[0], std::max(dim[1], dim[2])) * (float)h;
    G.cell_start = m->cell_start.as<uint32_t>() + 1;
    G.pts = m->pts4.as<float4>();
    G.nrm = nullptr;
    G.n = n_valid;
    m->built = true;
    m->has_cov = false;
    m->generation = sf::next_generation();
    sf::map_points_moved(m);
    m->h_exact = h;
    for (int d = 0; d < 3; ++d) { m->src_mn[d] = n_valid > 0 ? mm.mn[d] : 0.0f; m->src_mx[d] = n_valid > 0 ? mm.mx[d] : 0.0f; }
    m->src_stamp = cloud->stamp;
    return SF_OK;
}

// ------------------------------------------------------------------ the index carried over a map growth step
// `*map_cloud += *cloud` + voxel filter + setTargetPointCloud (global_map_frames_manager.cpp:131,142-146,
// icp_point_to_point.cpp:49-55) when the filter ran as a merge (sf_cloud_voxel_merge): the merge knows which old points
// stay (their ids move up by the fresh voxels in front of them), which are replaced by a new centroid and which voxels are
// new.  With the grid origin unchanged, a point's cell coordinates are what they were, the cell-sorted order of the points that
// stay is what it was (ascending id inside a cell, and ids keep their order), and the new index is a MERGE of two sorted
// sequences: the old entries minus the replaced ones, and the centroids sorted by (cell, id).  One streaming pass over the
// old entries instead of four sort passes and a random gather; the result is bit-identical to sf_map_build of the merged
// cloud with the same cell (tests/test_gpu_map_growth.py against a rebuild, tests/test_gpu_growth_direct.py against numpy).  Anything
// this cannot express -- the smallest coordinate of the map changed, a point that sat clamped at the old upper face (one that stays
// or one the merge replaced), 64-bit cell ids -- takes the build.
namespace {

struct PatchGeom { float org[3]; float inv_h; int dim[3]; int old_dim[3]; };

__device__ __forceinline__ uint32_t patch_key(const PatchGeom &g, float x, float y, float z, bool *moved)
{
    // the coordinates before the clamp to the upper face, then under the new and under the old grid
    const int rx = (int)fminf(fmaxf(floorf((x - g.org[0]) * g.inv_h), 0.0f), 2.0e9f), ry = (int)fminf(fmaxf(floorf((y - g.org[1]) * g.inv_h), 0.0f), 2.0e9f),
              rz = (int)fminf(fmaxf(floorf((z - g.org[2]) * g.inv_h), 0.0f), 2.0e9f);
    const int cx = min(rx, g.dim[0] - 1), cy = min(ry, g.dim[1] - 1), cz = min(rz, g.dim[2] - 1);
    if (moved) *moved = cx != min(rx, g.old_dim[0] - 1) || cy != min(ry, g.old_dim[1] - 1) || cz != min(rz, g.old_dim[2] - 1); // one of the grids clamps it into another cell
    return ((uint32_t)cz * (uint32_t)g.dim[1] + (uint32_t)cy) * (uint32_t)g.dim[0] + (uint32_t)cx;
}

using sf::PatchFlags;

// thread t in two roles.  As voxel g = t: key of its centroid, and the old entry it replaces marked in the bitmap over the old
// sorted positions (+ the count of its block of 256 positions)
__global__ void k_patch_groups(PatchGeom geo, const uint32_t *__restrict__ g_rank, const uint32_t *__restrict__ g_fresh, const float *__restrict__ g_centroid,
                               const float *__restrict__ g_old, int64_t n_groups, const float4 *__restrict__ pts, int64_t n_old, uint32_t *__restrict__ ins_key,
                               uint32_t *__restrict__ ins_val, uint32_t *__restrict__ bitmap, uint32_t *__restrict__ blk_cnt, PatchFlags *__restrict__ ext)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    ins_key[g] = patch_key(geo, g_centroid[3 * g], g_centroid[3 * g + 1], g_centroid[3 * g + 2], nullptr);
    ins_val[g] = (uint32_t)g;
    if (!g_fresh[g]) { // the old point of this voxel: where it lies in the index (entries ascend in (cell, id))
        bool moved;
        const uint32_t r = g_rank[g], key = patch_key(geo, g_old[3 * g], g_old[3 * g + 1], g_old[3 * g + 2], &moved);
        // a replaced point that the old grid had clamped to its upper face: the index has it in its old cell, in front of the later
        // entries of that cell, while its key under the new grid is larger than theirs -- the old entries do not ascend across it, and
        // the searches over them (here, k_patch_ranges, k_patch_new) go astray whenever they probe it.  The build decides, as for a
        // clamped point that stays (k_patch_old); the entry is still looked for, so that the bitmap is whole when it is found
        if (moved) ext->moved = 1u;
        int64_t lo = 0, hi = n_old;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            const float4 a = pts[mid];
            const uint32_t k = patch_key(geo, a.x, a.y, a.z, nullptr);
            if (k < key || (k == key && __float_as_uint(a.w) < r)) lo = mid + 1;
            else hi = mid;
        }
        if (lo >= n_old || __float_as_uint(pts[lo].w) != r) { ext->moved = 1u; return; } // (an order the search cannot follow: the build decides)
        const uint32_t p = (uint32_t)lo;
        atomicOr(&bitmap[p >> 5], 1u << (p & 31u));
        atomicAdd(&blk_cnt[p >> 8], 1u);
    }
}

// sorted centroid e -> (cell, rank among the old ids) in one word: old entry (cell', id) comes after it iff packed(e) <= (cell' << 32 | id)
__global__ void k_patch_pack(const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sval, const uint32_t *__restrict__ g_rank, int64_t n_groups, uint64_t *__restrict__ packed)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n_groups) packed[e] = ((uint64_t)skey[e] << 32) | (uint64_t)g_rank[sval[e]];
}

// per block of 256 old entries: its candidates among the sorted centroids, [first with cell >= the block's first cell, first with
// cell > its last cell) -- searched by one thread per bound, all blocks at once (inside k_patch_old the same two searches
// were a serial chain of ~18 dependent loads in front of every workgroup)
__global__ void k_patch_ranges(PatchGeom geo, const float4 *__restrict__ pts, int64_t n_old, const uint64_t *__restrict__ packed, int64_t n_groups, int64_t n_blocks,
                               uint32_t *__restrict__ range)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * n_blocks) return;
    const int64_t blk = t >> 1, p0 = blk * 256;
    const bool upper = (t & 1) != 0;
    const float4 a = pts[upper ? min(p0 + 255, n_old - 1) : p0];
    const uint64_t k = (uint64_t)patch_key(geo, a.x, a.y, a.z, nullptr) << 32;
    const uint64_t v = upper ? (k | 0xffffffffull) : k;
    int64_t lo = 0, hi = n_groups;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (upper ? packed[mid] <= v : packed[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    range[t] = (uint32_t)lo;
}

__device__ __forceinline__ uint32_t patch_del_before(const uint32_t *__restrict__ bitmap, const uint32_t *__restrict__ blk_pre, uint32_t p)
{
    const uint32_t blk = p >> 8, w = (p & 255u) >> 5;
    uint32_t c = blk_pre[blk];
    for (uint32_t k = 0; k < w; ++k) c += (uint32_t)__popc(bitmap[blk * 8u + k]);
    return c + (uint32_t)__popc(bitmap[blk * 8u + w] & ((1u << (p & 31u)) - 1u));
}

// one lane per OLD entry, in sorted order: where it goes, with its new id.  CARRY (sf_map_set_normals_carry): 1 = its normal
// goes with it, 2 = its normal and the 6 doubles of its covariance (16 B / 64 B more per point, streaming like the point
// itself); 0 compiles to the pass without them
template <int CARRY>
__global__ __launch_bounds__(256) void k_patch_old(PatchGeom geo, const float4 *__restrict__ pts, int64_t n_old, const uint32_t *__restrict__ bitmap, const uint32_t *__restrict__ blk_pre,
                                                    const uint64_t *__restrict__ packed, const uint32_t *__restrict__ range, const uint32_t *__restrict__ coarse,
                                                    const uint32_t *__restrict__ fresh_rank,
                                                    float4 *__restrict__ pts_out, uint32_t *__restrict__ keys_out, PatchFlags *__restrict__ ext,
                                                    const float4 *__restrict__ nrm, float4 *__restrict__ nrm_out, const double2 *__restrict__ cov, double2 *__restrict__ cov_out,
                                                    int64_t n_out)
{
    __shared__ uint32_t words[8], wpre[8];
    const int64_t p0 = (int64_t)blockIdx.x * 256, p = p0 + threadIdx.x;
    if (threadIdx.x >= 64 && threadIdx.x < 72) words[threadIdx.x - 64] = bitmap[(size_t)blockIdx.x * 8 + (threadIdx.x - 64)];
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = blk_pre[blockIdx.x];
        for (int k = 0; k < 8; ++k) { wpre[k] = c; c += (uint32_t)__popc(words[k]); }
    }
    __syncthreads();
    if (p >= n_old) return;
    const uint32_t w = threadIdx.x >> 5, bit = threadIdx.x & 31u;
    if ((words[w] >> bit) & 1u) return; // replaced by a centroid
    const float4 a = pts[p];
    bool moved;
    const uint32_t key = patch_key(geo, a.x, a.y, a.z, &moved);
    if (moved) ext->moved = 1u;
    const uint32_t j = __float_as_uint(a.w);
    const uint64_t mine = ((uint64_t)key << 32) | (uint64_t)j;
    int64_t lo = range[2 * (size_t)blockIdx.x], hi = range[2 * (size_t)blockIdx.x + 1]; // centroids that sort before this entry: packed <= mine
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (packed[mid] <= mine) lo = mid + 1;
        else hi = mid;
    }
    uint32_t f = coarse[j >> 6];
    const uint32_t f_end = coarse[(j >> 6) + 1];
    while (f < f_end && fresh_rank[f] <= j) ++f;
    const uint32_t del = wpre[w] + (uint32_t)__popc(words[w] & ((1u << bit) - 1u));
    const size_t o = (size_t)p - (size_t)del + (size_t)lo;
    const uint32_t id = j + f;
    // o is this entry's rank in the merged sequence, hence below n_out, unless k_patch_groups gave up on a voxel (ext->moved)
    // and left the bitmap short: that pass's output is abandoned.  The carrying passes write nothing then; the plain pass is
    // kept instruction for instruction as it was (all its outputs are reserved alike, with the allocator's slack)
    if (CARRY >= 1 && o >= (size_t)n_out) return;
    pts_out[o] = make_float4(a.x, a.y, a.z, __uint_as_float(id));
    keys_out[o] = key;
    if (CARRY >= 1) {
        nrm_out[o] = nrm[p];
        if (CARRY == 2) {
#pragma unroll
            for (int d = 0; d < 3; ++d) cov_out[3 * o + d] = cov[3 * (size_t)p + d];
        }
    }
}

// one lane per centroid, in (cell, id) order: the old entries in front of it, less the replaced ones, plus its own rank
__global__ __launch_bounds__(256) void k_patch_new(PatchGeom geo, const float4 *__restrict__ pts, int64_t n_old, const uint32_t *__restrict__ bitmap, const uint32_t *__restrict__ blk_pre,
                                                    const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sval, int64_t n_groups, const uint32_t *__restrict__ g_rank,
                                                    const uint32_t *__restrict__ fresh_pos, const float *__restrict__ g_centroid, float4 *__restrict__ pts_out,
                                                    uint32_t *__restrict__ keys_out)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_groups) return;
    const uint32_t key = skey[e], g = sval[e], r = g_rank[g];
    int64_t lo = 0, hi = n_old; // old entries with (cell, id) < (key, r)
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const float4 a = pts[mid];
        const uint32_t k = patch_key(geo, a.x, a.y, a.z, nullptr);
        if (k < key || (k == key && __float_as_uint(a.w) < r)) lo = mid + 1;
        else hi = mid;
    }
    const size_t o = (size_t)e + (size_t)lo - (size_t)patch_del_before(bitmap, blk_pre, (uint32_t)lo);
    const uint32_t id = r + fresh_pos[g];
    pts_out[o] = make_float4(g_centroid[3 * (size_t)g], g_centroid[3 * (size_t)g + 1], g_centroid[3 * (size_t)g + 2], __uint_as_float(id));
    keys_out[o] = key;
}

// the normals after a patch (defined with the normals kernels below): which points the merge left with another neighbourhood,
// and those re-estimated on the patched index
int carry_reestimate(sf_map *m, const sf_cloud::MergeRecord &rec, const int old_dim[3], float radius, bool with_cov, int64_t *n_dirty);

} // namespace

extern "C" int sf_map_patch(sf_map *m, sf_cloud *cloud, int *patched)
{
    SF_CHECK(m && cloud, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(m->built, SF_ERR_STATE, "sf_map_patch: the map has no index yet (sf_map_build)");
    SF_CHECK(m->ctx == cloud->ctx, SF_ERR_INVALID, "map and cloud must live on the same context");
    if (patched) *patched = 0;
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const float cell = (float)m->h_exact;
    const sf_cloud::MergeRecord &rec = cloud->merge;
    const SfGrid old = m->grid;
    const uint64_t old_cells = (uint64_t)old.dim[0] * (uint64_t)old.dim[1] * (uint64_t)old.dim[2];
    const int64_t n_old = rec.n_old, ng = rec.n_groups, n_out = cloud->n;
    // the estimate to carry (sf_map_set_normals_carry): normals that sf_map_estimate_normals_cov wrote, with its arguments
    // a k-NN estimate (sf_map_estimate_normals_knn) is not carried entry by entry -- a point added or removed can change a
    // neighbourhood arbitrarily far away -- but run again in full behind the patch, on every path
    const int knn_k = (m->normals_carry && m->has_normals && m->nrm_estimated) ? m->nrm_knn_k : 0;
    const bool knn_cov = knn_k > 0 && m->has_cov && m->nrm_with_cov;
    const bool carry = m->normals_carry && m->has_normals && m->nrm_estimated && knn_k == 0;
    const float carry_radius = m->nrm_radius;
    const bool carry_cov = carry && m->has_cov && m->nrm_with_cov;
    auto knn_again = [&]() -> int {
        SF_TRY(sf_map_estimate_normals_knn(m, knn_k, carry_radius, knn_cov ? 1 : 0));
        m->carry_info[0] = 0;
        m->carry_info[1] = 0;
        m->carry_info[2] = m->grid.n;
        return SF_OK;
    };
    m->carry_info[0] = -1; m->carry_info[1] = m->carry_info[2] = 0; m->carry_info[3] = m->n;
    auto rebuild = [&](int why) -> int { // *patched: 0 / negative = the build ran, and why
        if (patched) *patched = why;
        SF_TRY(sf_map_build(m, cloud, cell));
        m->carry_info[3] = m->n;
        if (knn_k > 0) return knn_again();
        if (!carry) return SF_OK;
        SF_TRY(sf_map_estimate_normals_cov(m, carry_radius, carry_cov ? 1 : 0)); // nothing of the old estimate survives a build: in full, as remembered
        m->carry_info[0] = 0;
        m->carry_info[2] = m->grid.n;
        return SF_OK;
    };
    if (!rec.valid || rec.epoch != ctx->merge_epoch || rec.stamp_after != cloud->stamp || rec.stamp_before != m->src_stamp || n_old != m->n || old.n != m->n || ng <= 0 ||
        n_out != n_old + rec.n_fresh)
        return rebuild(SF_PATCH_NO_MERGE);
    if (n_out >= (int64_t)(1 << 28) || old_cells >= 0xffffffffull) return rebuild(SF_PATCH_LIMITS);

    // 1. do the bounds of the map survive?  (the merge looked: sf_voxel.hip, k_merge_extremes)
    float new_mn[3], new_mx[3];
    for (int d = 0; d < 3; ++d)
        if (rec.old_mn[d] != m->src_mn[d] || rec.old_mx[d] != m->src_mx[d]) return rebuild(SF_PATCH_NO_MERGE); // (not the bounds this index was built on)
    if (rec.touched_extreme) {
        // a point that held a bound was replaced: one reduction over the merged cloud says what the bounds are now (a tenth
        // of a build)
        sf::MinMaxHost mm;
        SF_TRY(sf::cloud_minmax(ctx, cloud->xyz.as<float>(), n_out, &mm));
        if (mm.n_finite != n_out) return rebuild(SF_PATCH_BOUND_REPLACED);
        for (int d = 0; d < 3; ++d) { cloud->bounds_mn[d] = new_mn[d] = mm.mn[d]; cloud->bounds_mx[d] = new_mx[d] = mm.mx[d]; }
        cloud->bounds_stamp = cloud->stamp; // (the next merge need not look again)
    } else {
        for (int d = 0; d < 3; ++d) { new_mn[d] = std::min(m->src_mn[d], rec.cen_mn[d]); new_mx[d] = std::max(m->src_mx[d], rec.cen_mx[d]); }
    }
    for (int d = 0; d < 3; ++d) // the origin a build would choose must be the one the index has: every cell changes otherwise
        if (grid_origin(new_mn[d], m->h_exact, m->origin_lattice) != old.org[d]) return rebuild(SF_PATCH_ORIGIN_MOVED);

    // 2. the geometry a build of the merged cloud would choose (sf_map_build, step 2, explicit cell)
    const double h = m->h_exact;
    size_t free_b = 0, total_b = 0;
    SF_HIP(hipMemGetInfo(&free_b, &total_b));
    free_b += m->cell_start.cap; // (the table being replaced counts as free: the build would reuse it)
    const double max_cells = std::min(34359738368.0, std::max(1.0e9, (double)free_b / 4.0 / sizeof(uint32_t)));
    GridGeom g;
    PatchGeom pg;
    double cells = 1;
    for (int d = 0; d < 3; ++d) {
        const double c = std::floor(((double)new_mx[d] - (double)old.org[d]) / h) + 1;
        if (c > 16777216.0) return rebuild(SF_PATCH_LIMITS); // (more than 2^24 cells on an axis: the build refuses)
        g.org[d] = pg.org[d] = old.org[d];
        g.dim[d] = pg.dim[d] = (int)c;
        pg.old_dim[d] = old.dim[d];
        cells *= c;
    }
    if (cells > max_cells || cells >= 4294967295.0) return rebuild(SF_PATCH_LIMITS);
    g.inv_h = pg.inv_h = old.inv_h;
    g.ncell = (uint64_t)g.dim[0] * (uint64_t)g.dim[1] * (uint64_t)g.dim[2];
    const bool by_scan = table_by_scan(g.ncell, n_out, m->origin_lattice); // (as sf_map_build)

    // 3. the centroids in (cell, id) order; the replaced entries as a bitmap over the old sorted positions
    const int64_t nb256 = sf::div_up(n_old, 256) + 1;
    const size_t off_key = 0, off_key2 = off_key + 4 * (size_t)ng, off_val = off_key2 + 4 * (size_t)ng, off_val2 = off_val + 4 * (size_t)ng, off_packed = (off_val2 + 4 * (size_t)ng + 7) & ~(size_t)7,
                 off_bitmap = off_packed + 8 * (size_t)ng, off_cnt = off_bitmap + 4 * 8 * (size_t)nb256, off_pre = off_cnt + 4 * (size_t)nb256, off_range = off_pre + 4 * (size_t)nb256,
                 off_ext = (off_range + 8 * (size_t)nb256 + 15) & ~(size_t)15, total = off_ext + sizeof(PatchFlags);
    SF_TRY(m->patch_tmp.reserve(total));
    unsigned char *base = m->patch_tmp.as<unsigned char>();
    uint32_t *ins_key = reinterpret_cast<uint32_t *>(base + off_key), *ins_key2 = reinterpret_cast<uint32_t *>(base + off_key2), *ins_val = reinterpret_cast<uint32_t *>(base + off_val),
             *ins_val2 = reinterpret_cast<uint32_t *>(base + off_val2), *bitmap = reinterpret_cast<uint32_t *>(base + off_bitmap), *blk_cnt = reinterpret_cast<uint32_t *>(base + off_cnt),
             *blk_pre = reinterpret_cast<uint32_t *>(base + off_pre), *range = reinterpret_cast<uint32_t *>(base + off_range);
    uint64_t *packed = reinterpret_cast<uint64_t *>(base + off_packed);
    PatchFlags *d_ext = reinterpret_cast<PatchFlags *>(base + off_ext);
    PatchFlags *h_ext = &ctx->h_pinned->patch;
    SF_TRY(m->pts4_alt.reserve(sizeof(float4) * (size_t)n_out));
    SF_TRY(m->keys.reserve(sizeof(uint32_t) * (size_t)n_out));
    if (carry) SF_TRY(m->nrm4_alt.reserve(sizeof(float4) * (size_t)n_out));
    if (carry_cov) SF_TRY(m->cov6_alt.reserve(sizeof(double) * 6 * (size_t)n_out));
    SF_HIP(hipMemsetAsync(bitmap, 0, off_range - off_bitmap, st)); // bitmap, block counts, their prefix
    SF_HIP(hipMemsetAsync(d_ext, 0, sizeof(PatchFlags), st));
    hipLaunchKernelGGL(k_patch_groups, dim3(nblk(ng)), dim3(256), 0, st, pg, rec.g_rank, rec.g_fresh, rec.g_centroid, rec.g_old, ng, old.pts, n_old, ins_key, ins_val, bitmap, blk_cnt,
                       d_ext);
    unsigned bits = 1;
    while (bits < 32 && (1ull << bits) <= (unsigned long long)g.ncell) ++bits;
    uint32_t *skey = nullptr, *sval = nullptr;
    SF_TRY(sf::radix_sort_pairs<uint32_t>(ctx, ins_key, ins_key2, ins_val, ins_val2, ng, bits, &skey, &sval)); // stable: equal cells stay in ascending id
    hipLaunchKernelGGL(k_patch_pack, dim3(nblk(ng)), dim3(256), 0, st, skey, sval, rec.g_rank, ng, packed);
    SF_TRY(sf::scan_u32<0>(ctx, blk_cnt, blk_pre, nb256));
    hipLaunchKernelGGL(k_patch_ranges, dim3(nblk(2 * (nb256 - 1))), dim3(256), 0, st, pg, old.pts, n_old, packed, ng, nb256 - 1, range);

    // 4. the merge
    float4 *pts_out = m->pts4_alt.as<float4>();
    uint32_t *keys_out = m->keys.as<uint32_t>();
    if (carry_cov)
        hipLaunchKernelGGL(k_patch_old<2>, dim3(nblk(n_old)), dim3(256), 0, st, pg, old.pts, n_old, bitmap, blk_pre, packed, range, rec.coarse, rec.fresh_rank, pts_out, keys_out, d_ext,
                           old.nrm, m->nrm4_alt.as<float4>(), m->cov6.as<double2>(), m->cov6_alt.as<double2>(), n_out);
    else if (carry)
        hipLaunchKernelGGL(k_patch_old<1>, dim3(nblk(n_old)), dim3(256), 0, st, pg, old.pts, n_old, bitmap, blk_pre, packed, range, rec.coarse, rec.fresh_rank, pts_out, keys_out, d_ext,
                           old.nrm, m->nrm4_alt.as<float4>(), nullptr, nullptr, n_out);
    else
        hipLaunchKernelGGL(k_patch_old<0>, dim3(nblk(n_old)), dim3(256), 0, st, pg, old.pts, n_old, bitmap, blk_pre, packed, range, rec.coarse, rec.fresh_rank, pts_out, keys_out, d_ext,
                           nullptr, nullptr, nullptr, nullptr, n_out);
    hipLaunchKernelGGL(k_patch_new, dim3(nblk(ng)), dim3(256), 0, st, pg, old.pts, n_old, bitmap, blk_pre, skey, sval, ng, rec.g_rank, rec.fresh_pos, rec.g_centroid, pts_out, keys_out);
    SF_HIP(hipMemcpyAsync(h_ext, d_ext, sizeof(PatchFlags), hipMemcpyDeviceToHost, st));

    // 5. the cell table from the merged keys (from here on the old index is gone: an error leaves the map without one)
    m->built = false;
    SF_TRY(m->cell_start.reserve(sizeof(uint32_t) * ((size_t)g.ncell + 8)));
    SF_TRY(build_cell_table(m, g, keys_out, n_out, false, by_scan));
    SF_HIP(hipGetLastError());
    SF_HIP(hipStreamSynchronize(st));
    m->pts4.swap(m->pts4_alt);
    if (h_ext->moved) return rebuild(SF_PATCH_CLAMPED_POINT); // a point that the old grid had clamped to its upper face: its cell, and the order, changed

    m->n = n_out;
    m->built = true;
    m->has_normals = false;
    m->nrm_estimated = false;
    m->nrm_knn_k = 0;
    m->window.kind = 0;
    SfGrid &G = m->grid;
    for (int d = 0; d < 3; ++d) G.dim[d] = g.dim[d];
    G.gap_eps = 1.5f * 2.384186e-7f * (float)std::max(g.dim[0], std::max(g.dim[1], g.dim[2])) * (float)h;
    G.cell_start = m->cell_start.as<uint32_t>() + 1;
    G.pts = m->pts4.as<float4>();
    G.nrm = nullptr;
    G.n = n_out;
    m->has_cov = false;
    m->generation = sf::next_generation();
    sf::map_points_moved(m);
    for (int d = 0; d < 3; ++d) { m->src_mn[d] = new_mn[d]; m->src_mx[d] = new_mx[d]; }
    m->src_stamp = cloud->stamp;
    m->carry_info[3] = m->n;
    if (carry) {
        // the entries that stayed brought their normals along (k_patch_old); the slots of the centroids and of every point
        // within the radius of a position that was added or removed are estimated on the patched index
        m->nrm4.swap(m->nrm4_alt);
        if (carry_cov) m->cov6.swap(m->cov6_alt);
        G.nrm = m->nrm4.as<float4>();
        int64_t n_dirty = 0;
        SF_TRY(carry_reestimate(m, rec, pg.old_dim, carry_radius, carry_cov, &n_dirty));
        m->has_normals = true;
        m->has_cov = carry_cov;
        m->nrm_estimated = true;
        m->nrm_radius = carry_radius;
        m->nrm_with_cov = carry_cov;
        m->carry_info[0] = 1;
        m->carry_info[1] = 2 * ng - rec.n_fresh; // every centroid, and the old point of every voxel that had one
        m->carry_info[2] = n_dirty;
    }
    if (knn_k > 0) SF_TRY(knn_again());
    if (patched) *patched = 1;
    return SF_OK;
}

// the index as it lies in HBM, for the parity tests: pts4 (x, y, z, bitcast id) in cell order, cell_start[0 .. n_cells]
extern "C" int sf_map_index_info(sf_map *m, int64_t *n_indexed, int64_t *n_cells, float org[3], float *inv_h, float *gap_eps)
{
    SF_CHECK(m && m->built, SF_ERR_STATE, "map not built");
    if (n_indexed) *n_indexed = m->grid.n;
    if (n_cells) *n_cells = (int64_t)m->grid.dim[0] * (int64_t)m->grid.dim[1] * (int64_t)m->grid.dim[2];
    if (org) for (int d = 0; d < 3; ++d) org[d] = m->grid.org[d];
    if (inv_h) *inv_h = m->grid.inv_h;
    if (gap_eps) *gap_eps = m->grid.gap_eps;
    return SF_OK;
}

extern "C" int sf_map_download_index(sf_map *m, float *pts4, int64_t cap_points, uint32_t *cell_start, int64_t cap_cells)
{
    SF_CHECK(m && m->built, SF_ERR_STATE, "map not built");
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    const int64_t n = m->grid.n, nc = (int64_t)m->grid.dim[0] * (int64_t)m->grid.dim[1] * (int64_t)m->grid.dim[2] + 1;
    SF_CHECK((!pts4 || cap_points >= n) && (!cell_start || cap_cells >= nc), SF_ERR_INVALID, "buffer too small");
    if (pts4 && n > 0) SF_HIP(hipMemcpyAsync(pts4, m->pts4.p, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (cell_start) SF_HIP(hipMemcpyAsync(cell_start, m->grid.cell_start, sizeof(uint32_t) * (size_t)nc, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    return SF_OK;
}

extern "C" int sf_map_set_origin_lattice(sf_map *m, int cells)
{
    SF_CHECK(m && cells >= 0 && cells <= 4096, SF_ERR_INVALID, "the lattice is 0 (off) to 4 096 cells");
    m->origin_lattice = cells; // takes effect with the next sf_map_build
    return SF_OK;
}

extern "C" int sf_map_size(sf_map *m, int64_t *n)
{
    SF_CHECK(m && n, SF_ERR_INVALID, "bad arguments");
    *n = m->n;
    return SF_OK;
}

extern "C" int sf_map_cell_size(sf_map *m, float *cell, int32_t dims[3])
{
    SF_CHECK(m && m->built, SF_ERR_STATE, "map not built");
    if (cell) *cell = m->grid.h;
    if (dims) for (int d = 0; d < 3; ++d) dims[d] = m->grid.dim[d];
    return SF_OK;
}

extern "C" int sf_map_window_none(sf_map *m)
{
    SF_CHECK(m, SF_ERR_INVALID, "bad arguments");
    m->window.kind = 0;
    return SF_OK;
}

extern "C" int sf_map_window_sphere(sf_map *m, const float center[3], double radius)
{
    SF_CHECK(m && center, SF_ERR_INVALID, "bad arguments");
    m->window.kind = 1;
    for (int d = 0; d < 3; ++d) m->window.c[d] = center[d];
    m->window.r2 = (float)(radius * radius);
    return SF_OK;
}

extern "C" int sf_map_window_obb(sf_map *m, const double center[3], const double R[9], const double extent[3])
{
    SF_CHECK(m && center && R && extent, SF_ERR_INVALID, "bad arguments");
    m->window.kind = 2;
    for (int d = 0; d < 3; ++d) { m->window.oc[d] = center[d]; m->window.ohalf[d] = extent[d] / 2; }
    for (int k = 0; k < 9; ++k) m->window.oR[k] = R[k];
    return SF_OK;
}

namespace {
__global__ __launch_bounds__(256) void k_window_count(SfGrid g, SfWindow w, unsigned long long *__restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool in = false;
    if (j < g.n) {
        const float4 p = g.pts[j];
        in = sf::window_accepts(w, p.x, p.y, p.z);
    }
    const unsigned long long b = __ballot(in);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(out, (unsigned long long)__popcll(b)); // integer: order independent
}
} // namespace

extern "C" int sf_map_window_count(sf_map *m, int64_t *n)
{
    SF_CHECK(m && m->built && n, SF_ERR_STATE, "map not built");
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    if (m->window.kind == 0 || m->grid.n == 0) { *n = m->grid.n; return SF_OK; }
    SF_TRY(ctx->scratch2.reserve(sizeof(unsigned long long)));
    unsigned long long *d = ctx->scratch2.as<unsigned long long>();
    SF_HIP(hipMemsetAsync(d, 0, sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(k_window_count, dim3(nblk(m->grid.n)), dim3(256), 0, ctx->stream, m->grid, m->window, d);
    SF_TRY(read_words(ctx, d, 1));
    *n = (int64_t)ctx->h_pinned->readback[0];
    return SF_OK;
}

extern "C" int sf_map_nn(sf_map *m, const float *queries, int64_t n, float max_d2, int32_t *idx, float *d2)
{
    SF_CHECK(m && m->built, SF_ERR_STATE, "map not built");
    SF_CHECK(n >= 0 && (n == 0 || (queries && idx && d2)), SF_ERR_INVALID, "bad arguments");
    if (n == 0) return SF_OK;
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    sf::DevBuf dq, di, dd;
    SF_TRY(dq.reserve(sizeof(float) * 3 * (size_t)n));
    SF_TRY(di.reserve(sizeof(int32_t) * (size_t)n));
    SF_TRY(dd.reserve(sizeof(float) * (size_t)n));
    SF_HIP(hipMemcpyAsync(dq.p, queries, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    ProfSpan span(m);
    if (m->window.kind)
        hipLaunchKernelGGL(k_map_nn_t<true>, dim3(nblk(n)), dim3(256), 0, ctx->stream, m->grid, m->window, dq.as<float>(), n, max_d2, di.as<int32_t>(), dd.as<float>());
    else
        hipLaunchKernelGGL(k_map_nn_t<false>, dim3(nblk(n)), dim3(256), 0, ctx->stream, m->grid, m->window, dq.as<float>(), n, max_d2, di.as<int32_t>(), dd.as<float>());
    span.end();
    SF_HIP(hipGetLastError());
    SF_HIP(hipMemcpyAsync(idx, di.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipMemcpyAsync(d2, dd.p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    prof_read(m);
    return SF_OK;
}

// ------------------------------------------------------------------ the neighbour table
// Per indexed point p one 32-byte entry: the sorted positions of the up to 7 OTHER points with the smallest key
// hit_key(l2_simple(p, x), position) among the points of the 27 cells around p's cell with d2 < cap^2, 0xffffffff where
// there is none, and a radius r that bounds from below the distance from p to every point that is neither p nor listed.
// cap = safe_gap(h, gap_eps) * 0.999, the search's own convention: everything outside the 27-cell block is at least a cell
// (less the rounding of the grid coordinates) away.  Seven listed: r = sqrt(d2 of the 7th) * 0.9999; fewer: r = cap.
// One lane per point; the seven keys stay sorted in registers by an unrolled insertion.  The entry depends on the index
// alone: the key order is total, whatever order the cells are walked in.
// Behind the n entries, in the same allocation, one float per point (sf::nbr_gap): the nearest gap g1 = sqrt(d2 of the first
// listed) * 0.9999, the cap when nothing is listed, 0 for a point with a coincident twin -- stage 0 of the look-up.
namespace {
__global__ __launch_bounds__(256) void k_neighbour_table(SfGrid g, uint4 *__restrict__ tab, float *__restrict__ gap)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= g.n) return;
    const float4 p = g.pts[j];
    const int cx = sf::grid_cell((p.x - g.org[0]) * g.inv_h, g.dim[0]), cy = sf::grid_cell((p.y - g.org[1]) * g.inv_h, g.dim[1]), cz = sf::grid_cell((p.z - g.org[2]) * g.inv_h, g.dim[2]);
    const float cap = sf::safe_gap(g.h, g.gap_eps) * 0.999f;
    const float cap2 = cap * cap;
    unsigned long long key[sf::NBR_K];
#pragma unroll
    for (int i = 0; i < sf::NBR_K; ++i) key[i] = ~0ull;
    sf::block_rows(g, cx, cy, cz, 1, [&](uint32_t a, uint32_t b) {
        for (uint32_t k = a; k < b; ++k) {
            const float4 q = g.pts[k];
            const float d2 = sf::l2_simple(p.x, p.y, p.z, q.x, q.y, q.z);
            if (k == (uint32_t)j || !(d2 < cap2)) continue;
            unsigned long long v = sf::hit_key(d2, (int)k);
            if (v >= key[sf::NBR_K - 1]) continue;
#pragma unroll
            for (int i = 0; i < sf::NBR_K; ++i) { // v sinks to its place, the larger keys move down one, the largest falls out
                const unsigned long long lo = v < key[i] ? v : key[i], hi = v < key[i] ? key[i] : v;
                key[i] = lo;
                v = hi;
            }
        }
    });
    const bool full = key[sf::NBR_K - 1] != ~0ull;
    const float r = full ? sqrtf(__uint_as_float((uint32_t)(key[sf::NBR_K - 1] >> 32))) * 0.9999f : cap;
    // (an absent slot's key is all ones: its low half is the "none" id)
    tab[2 * (size_t)j] = make_uint4((uint32_t)key[0], (uint32_t)key[1], (uint32_t)key[2], (uint32_t)key[3]);
    tab[2 * (size_t)j + 1] = make_uint4((uint32_t)key[4], (uint32_t)key[5], (uint32_t)key[6], __float_as_uint(r));
    gap[j] = key[0] != ~0ull ? sqrtf(__uint_as_float((uint32_t)(key[0] >> 32))) * 0.9999f : cap;
}

// the re-search of sf_nn.hpp on its own, one query per lane: sf_map_nn_seeded
__global__ __launch_bounds__(256) void k_map_nn_seeded(SfGrid g, const float *__restrict__ q, int64_t n, const int32_t *__restrict__ seed_pos, float thr, int32_t *__restrict__ idx,
                                                       float *__restrict__ d2, uint8_t *__restrict__ stage, float *__restrict__ lb2)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float qx = q[3 * i], qy = q[3 * i + 1], qz = q[3 * i + 2];
    const int32_t s = seed_pos[i];
    int ok = 0; // the stage that served it (sf::NBR_BY_GAP / sf::NBR_BY_TABLE)
    sf::NNHit hit{0.0f, -1, 0.0f, 0.0f, 0.0f, 0.0f};
    if (s >= 0 && (int64_t)s < g.n && isfinite(qx) && isfinite(qy) && isfinite(qz)) {
        const float4 p = g.pts[s];
        const sf::NNHit seed{sf::l2_simple(qx, qy, qz, p.x, p.y, p.z), s, p.x, p.y, p.z, 0.0f};
        ok = sf::nn_research_table(g, qx, qy, qz, thr, seed, hit);
    }
    const bool has = ok && hit.j >= 0;
    idx[i] = has ? (int32_t)__float_as_uint(g.pts[hit.j].w) : -1;
    d2[i] = has ? hit.d2 : INFINITY;
    stage[i] = (uint8_t)ok;
    if (lb2) lb2[i] = ok ? hit.lb2 : 0.0f; // (sf_map_nn_seeded_stages)
}
} // namespace

namespace sf {
void map_points_moved(sf_map *m)
{
    m->pts_stamp = next_generation();
    m->nbr_stamp = 0; // the table (its allocation is kept) describes other points
    m->rad_valid = false; // ... and so do the radius lists
    if (m->served) m->moved_after_serving = true;
}

int map_neighbour_table_ensure(sf_map *m)
{
    if (map_neighbour_table_present(m)) return SF_OK;
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    SF_TRY(m->nbr.reserve((sizeof(uint4) * 2 + sizeof(float)) * (size_t)std::max<int64_t>(m->grid.n, 1))); // the entries, then the nearest gaps
    m->nbr_timed = false;
    if (m->profile) {
        bool ok = true;
        for (int i = 0; i < 2; ++i)
            if (!m->nbr_ev[i] && hipEventCreate(&m->nbr_ev[i]) != hipSuccess) { m->nbr_ev[i] = nullptr; ok = false; }
        m->nbr_timed = ok && hipEventRecord(m->nbr_ev[0], ctx->stream) == hipSuccess;
    }
    SfGrid g = m->grid;
    g.nbr = nullptr;
    if (g.n > 0) hipLaunchKernelGGL(k_neighbour_table, dim3(nblk(g.n)), dim3(256), 0, ctx->stream, g, m->nbr.as<uint4>(), reinterpret_cast<float *>(m->nbr.as<uint4>() + 2 * (size_t)g.n));
    SF_HIP(hipGetLastError());
    if (m->nbr_timed) m->nbr_timed = hipEventRecord(m->nbr_ev[1], ctx->stream) == hipSuccess;
    m->nbr_build_ms = -1.0f;
    m->nbr_stamp = m->pts_stamp;
    return SF_OK;
}
} // namespace sf

extern "C" int sf_map_build_neighbour_table(sf_map *m)
{
    SF_CHECK(m && m->built, SF_ERR_STATE, "map not built");
    SF_TRY(sf::map_neighbour_table_ensure(m));
    SF_HIP(hipStreamSynchronize(m->ctx->stream));
    return SF_OK;
}

extern "C" int sf_map_set_neighbour_table(sf_map *m, int mode)
{
    SF_CHECK(m, SF_ERR_INVALID, "map is NULL");
    SF_CHECK(mode >= 0 && mode <= 2, SF_ERR_INVALID, "mode must be 0 (never), 1 (auto) or 2 (always)");
    m->nbr_mode = mode;
    return SF_OK;
}

// out: present (0 / 1), entries, bytes, the last build's device time in whole ms (rounded up; -1: not timed -- builds are timed
// while sf_map_profile_launches is on)
extern "C" int sf_map_neighbour_table_info(sf_map *m, int64_t out[4])
{
    SF_CHECK(m && out, SF_ERR_INVALID, "bad arguments");
    const bool present = m->built && sf::map_neighbour_table_present(m);
    if (m->nbr_timed) { // (timed builds only: sf_map_profile_launches)
        SF_HIP(hipStreamSynchronize(m->ctx->stream));
        float ms = -1.0f;
        if (hipEventElapsedTime(&ms, m->nbr_ev[0], m->nbr_ev[1]) == hipSuccess) m->nbr_build_ms = ms;
        m->nbr_timed = false;
    }
    out[0] = present ? 1 : 0;
    out[1] = present ? m->grid.n : 0;
    out[2] = present ? (int64_t)(sizeof(uint4) * 2) * m->grid.n : 0;
    out[3] = m->nbr_build_ms >= 0.0f ? (int64_t)std::ceil((double)m->nbr_build_ms) : -1; // whole milliseconds, rounded up; -1: not timed
    return SF_OK;
}

// the table as it lies in HBM, for the parity tests: [n][8] uint32 (seven sorted positions, the radius's float bits)
extern "C" int sf_map_download_neighbour_table(sf_map *m, uint32_t *table, int64_t cap_entries, int64_t *n)
{
    SF_CHECK(m && m->built && n, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(sf::map_neighbour_table_present(m), SF_ERR_STATE, "no neighbour table (sf_map_build_neighbour_table)");
    *n = m->grid.n;
    if (!table || m->grid.n == 0) return SF_OK;
    SF_CHECK(cap_entries >= m->grid.n, SF_ERR_INVALID, "buffer too small");
    SF_HIP(hipSetDevice(m->ctx->device));
    SF_HIP(hipMemcpyAsync(table, m->nbr.p, sizeof(uint32_t) * 8 * (size_t)m->grid.n, hipMemcpyDeviceToHost, m->ctx->stream));
    SF_HIP(hipStreamSynchronize(m->ctx->stream));
    return SF_OK;
}

// the nearest gaps behind the table (stage 0 of the look-up), for the parity tests: [n] float32 in sorted order
extern "C" int sf_map_download_nearest_gap(sf_map *m, float *gap, int64_t cap_entries, int64_t *n)
{
    SF_CHECK(m && m->built && n, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(sf::map_neighbour_table_present(m), SF_ERR_STATE, "no neighbour table (sf_map_build_neighbour_table)");
    *n = m->grid.n;
    if (!gap || m->grid.n == 0) return SF_OK;
    SF_CHECK(cap_entries >= m->grid.n, SF_ERR_INVALID, "buffer too small");
    SF_HIP(hipSetDevice(m->ctx->device));
    SF_HIP(hipMemcpyAsync(gap, m->nbr.as<uint4>() + 2 * (size_t)m->grid.n, sizeof(float) * (size_t)m->grid.n, hipMemcpyDeviceToHost, m->ctx->stream));
    SF_HIP(hipStreamSynchronize(m->ctx->stream));
    return SF_OK;
}

// Test entry of the table re-search: query i starts from the indexed point at SORTED position seed_pos[i] (-1, or anything
// outside the index: no seed).  served[i] = 1: idx / d2 are sf_map_nn's answer for the query, bit for bit (original ids,
// -1 / +inf when nothing lies within max_d2); served[i] = 0: the table could not decide it (idx = -1, d2 = +inf).
namespace {
// -> stage[i]: 0 not served, sf::NBR_BY_GAP / sf::NBR_BY_TABLE; lb2 (optional): the squared runner-up bound
int map_nn_seeded(sf_map *m, const float *queries, int64_t n, const int32_t *seed_pos, float max_d2, int32_t *idx, float *d2, uint8_t *stage, float *lb2)
{
    SF_CHECK(m && m->built, SF_ERR_STATE, "map not built");
    SF_CHECK(n >= 0 && (n == 0 || (queries && seed_pos && idx && d2 && stage)), SF_ERR_INVALID, "bad arguments");
    SF_CHECK(sf::map_neighbour_table_present(m), SF_ERR_STATE, "no neighbour table (sf_map_build_neighbour_table)");
    SF_CHECK(m->window.kind == 0, SF_ERR_STATE, "the neighbour table knows no window");
    if (n == 0) return SF_OK;
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    sf::DevBuf dq, ds, di, dd, dv, dl;
    SF_TRY(dq.reserve(sizeof(float) * 3 * (size_t)n));
    SF_TRY(ds.reserve(sizeof(int32_t) * (size_t)n));
    SF_TRY(di.reserve(sizeof(int32_t) * (size_t)n));
    SF_TRY(dd.reserve(sizeof(float) * (size_t)n));
    SF_TRY(dv.reserve((size_t)n));
    if (lb2) SF_TRY(dl.reserve(sizeof(float) * (size_t)n));
    SF_HIP(hipMemcpyAsync(dq.p, queries, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    SF_HIP(hipMemcpyAsync(ds.p, seed_pos, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    SfGrid g = m->grid;
    g.nbr = m->nbr.as<uint4>();
    hipLaunchKernelGGL(k_map_nn_seeded, dim3(nblk(n)), dim3(256), 0, ctx->stream, g, dq.as<float>(), n, ds.as<int32_t>(), max_d2, di.as<int32_t>(), dd.as<float>(), dv.as<uint8_t>(),
                       lb2 ? dl.as<float>() : nullptr);
    SF_HIP(hipGetLastError());
    SF_HIP(hipMemcpyAsync(idx, di.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipMemcpyAsync(d2, dd.p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipMemcpyAsync(stage, dv.p, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (lb2) SF_HIP(hipMemcpyAsync(lb2, dl.p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    return SF_OK;
}
} // namespace

extern "C" int sf_map_nn_seeded(sf_map *m, const float *queries, int64_t n, const int32_t *seed_pos, float max_d2, int32_t *idx, float *d2, uint8_t *served)
{
    SF_TRY(map_nn_seeded(m, queries, n, seed_pos, max_d2, idx, d2, served, nullptr));
    for (int64_t i = 0; i < n; ++i) served[i] = served[i] != 0; // the stage, collapsed to the flag
    return SF_OK;
}

// sf_map_nn_seeded with the stage that served each query (0: not served, 1: the nearest gap alone, 2: the table) and the
// runner-up bound lb2 it left (squared; 0 where not served)
extern "C" int sf_map_nn_seeded_stages(sf_map *m, const float *queries, int64_t n, const int32_t *seed_pos, float max_d2, int32_t *idx, float *d2, uint8_t *stage, float *lb2)
{
    SF_CHECK(n == 0 || lb2, SF_ERR_INVALID, "bad arguments");
    return map_nn_seeded(m, queries, n, seed_pos, max_d2, idx, d2, stage, lb2);
}

// ------------------------------------------------------------------ exact k-NN (sf_knn.hpp)
namespace {
// a wave walks its 64 consecutive queries one after another, all lanes on the same query; result rows are written by lanes 0 .. k-1
template <bool WINDOW>
__global__ __launch_bounds__(256) void k_map_knn_t(SfGrid g, SfWindow w, const float *__restrict__ q, int64_t n, int k, float thr, int32_t *__restrict__ idx, float *__restrict__ d2,
                                                  int32_t *__restrict__ count)
{
    __shared__ sf::WaveKNN ws[256 / 64];
    // the window from LDS: as a kernel argument its 35 dwords stay in SGPRs across the whole walk, which is wave-uniform and
    // lives in SGPRs itself, and the register file spills
    __shared__ SfWindow sw;
    if (WINDOW) {
        if (threadIdx.x == 0) sw = w;
        __syncthreads();
    }
    const int lane = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
    const int64_t base = ((int64_t)blockIdx.x * 4 + wv) * 64;
    if (base >= n) return; // (the whole wave: no workgroup barrier below)
    const int64_t i = base + lane;
    const bool valid = i < n;
    const float mx = valid ? q[3 * i] : 0.0f, my = valid ? q[3 * i + 1] : 0.0f, mz = valid ? q[3 * i + 2] : 0.0f;
    const int nq = (int)min((int64_t)64, n - base);
    for (int t = 0; t < nq; ++t) {
        const float qx = __shfl(mx, t), qy = __shfl(my, t), qz = __shfl(mz, t);
        unsigned long long key;
        const int cnt = sf::knn_search<WINDOW>(g, WINDOW ? sw : w, qx, qy, qz, k, thr, &ws[wv], key);
        if (lane < k) {
            const bool has = lane < cnt;
            int32_t id = -1;
            if (has) id = (int32_t)__float_as_uint(g.pts[(uint32_t)key].w);
            idx[(size_t)(base + t) * (size_t)k + lane] = id;
            d2[(size_t)(base + t) * (size_t)k + lane] = has ? __uint_as_float((uint32_t)(key >> 32)) : INFINITY;
        }
        if (lane == 0) count[base + t] = cnt;
    }
}
} // namespace

extern "C" int sf_map_knn(sf_map *m, const float *queries, int64_t n, int k, float max_d2, int32_t *idx, float *d2, int32_t *count)
{
    SF_CHECK(m && m->built, SF_ERR_STATE, "map not built");
    SF_CHECK(k >= 1 && k <= SF_KNN_MAX, SF_ERR_INVALID, "k must be 1 .. %d (got %d)", SF_KNN_MAX, k);
    SF_CHECK(n >= 0 && (n == 0 || (queries && idx && d2)), SF_ERR_INVALID, "bad arguments");
    if (n == 0) return SF_OK;
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    sf::DevBuf dq, di, dd, dc;
    SF_TRY(dq.reserve(sizeof(float) * 3 * (size_t)n));
    SF_TRY(di.reserve(sizeof(int32_t) * (size_t)n * (size_t)k));
    SF_TRY(dd.reserve(sizeof(float) * (size_t)n * (size_t)k));
    SF_TRY(dc.reserve(sizeof(int32_t) * (size_t)n));
    SF_HIP(hipMemcpyAsync(dq.p, queries, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    ProfSpan span(m);
    if (m->window.kind)
        hipLaunchKernelGGL(k_map_knn_t<true>, dim3(nblk(n)), dim3(256), 0, ctx->stream, m->grid, m->window, dq.as<float>(), n, k, max_d2, di.as<int32_t>(), dd.as<float>(), dc.as<int32_t>());
    else
        hipLaunchKernelGGL(k_map_knn_t<false>, dim3(nblk(n)), dim3(256), 0, ctx->stream, m->grid, m->window, dq.as<float>(), n, k, max_d2, di.as<int32_t>(), dd.as<float>(), dc.as<int32_t>());
    span.end();
    SF_HIP(hipGetLastError());
    SF_HIP(hipMemcpyAsync(idx, di.p, sizeof(int32_t) * (size_t)n * (size_t)k, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipMemcpyAsync(d2, dd.p, sizeof(float) * (size_t)n * (size_t)k, hipMemcpyDeviceToHost, ctx->stream));
    if (count) SF_HIP(hipMemcpyAsync(count, dc.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    prof_read(m);
    return SF_OK;
}

// ------------------------------------------------------------------ normals (extension x2, no reference code)
// PCA of all neighbours within `radius` (self included), float64, two passes (mean, then
// centred covariance); smallest-eigenvalue vector by cyclic Jacobi.  The batch is
// 3 x k . k x 3 with k ~ 10-30: VALU work, not a dense contraction worth MFMA.
namespace {

// Unit eigenvector of the smallest eigenvalue of the symmetric C, oriented z > 0, then y > 0, then x > 0.  An axis-aligned C
// (off-diagonals exactly 0) takes no rotation: the answer is the axis of the smallest diagonal entry, the FIRST one among
// equals -- so the zero matrix (every neighbour on one spot) gives +x, while store_normal_cov gives +z below 3 neighbours
// without coming here.  Pinned by tests/test_gpu_linalg_direct.py::test_smallest_eigvec_matches_eigh[zero].
__device__ void smallest_eigvec(const double C[9], double nrm[3])
{
    double a[9], v[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int i = 0; i < 9; ++i) a[i] = C[i];
    for (int sweep = 0; sweep < 50; ++sweep) {
        const double off = fabs(a[1]) + fabs(a[2]) + fabs(a[5]);
        const double dia = fabs(a[0]) + fabs(a[4]) + fabs(a[8]);
        if (off <= 1e-300 || off <= 2.220446049250313e-16 * dia * 1e-3) break;
        for (int k = 0; k < 3; ++k) {
            const int p = k == 2 ? 1 : 0, q = k == 0 ? 1 : 2;
            const double apq = a[3 * p + q];
            if (fabs(apq) < 1e-300) continue;
            const double theta = (a[3 * q + q] - a[3 * p + p]) / (2 * apq);
            const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1));
            const double c = 1 / sqrt(t * t + 1), s = t * c;
            for (int i = 0; i < 3; ++i) {
                const double aip = a[3 * i + p], aiq = a[3 * i + q];
                a[3 * i + p] = c * aip - s * aiq;
                a[3 * i + q] = s * aip + c * aiq;
            }
            for (int i = 0; i < 3; ++i) {
                const double api = a[3 * p + i], aqi = a[3 * q + i];
                a[3 * p + i] = c * api - s * aqi;
                a[3 * q + i] = s * api + c * aqi;
            }
            for (int i = 0; i < 3; ++i) {
                const double vip = v[3 * i + p], viq = v[3 * i + q];
                v[3 * i + p] = c * vip - s * viq;
                v[3 * i + q] = s * vip + c * viq;
            }
        }
    }
    int best = 0;
    if (a[4] < a[3 * best + best]) best = 1;
    if (a[8] < a[3 * best + best]) best = 2;
    double x = v[best], y = v[3 + best], z = v[6 + best];
    const double nn = sqrt(x * x + y * y + z * z);
    if (!(nn > 0)) { nrm[0] = 0; nrm[1] = 0; nrm[2] = 1; return; }
    x /= nn; y /= nn; z /= nn;
    if (z < 0 || (z == 0 && (y < 0 || (y == 0 && x < 0)))) { x = -x; y = -y; z = -z; }
    nrm[0] = x; nrm[1] = y; nrm[2] = z;
}

// position j's normal (the smallest eigenvector of the centred sums C of its cnt neighbours; +z below 3), the count in .w, and
// where asked xx xy xz yy yz zz of the centred neighbourhood divided by the count (zeros below 3 neighbours)
__device__ __forceinline__ void store_normal_cov(int cnt, const double C[6], int64_t j, float4 *__restrict__ nrm4, double *__restrict__ cov6)
{
    double nv[3] = {0, 0, 1};
    if (cnt >= 3) {
        const double M[9] = {C[0], C[1], C[2], C[1], C[3], C[4], C[2], C[4], C[5]};
        smallest_eigvec(M, nv);
    }
    nrm4[j] = make_float4((float)nv[0], (float)nv[1], (float)nv[2], __int_as_float(cnt));
    if (cov6) {
#pragma unroll
        for (int d = 0; d < 6; ++d) cov6[6 * (size_t)j + d] = cnt >= 3 ? C[d] / (double)cnt : 0.0;
    }
}

// the estimate of sorted position j: cells z-major, then y, then one contiguous x-run per row (box_rows over the ball_box: the
// layers of cells that can hold a neighbour), ascending id inside a cell.  The order of these float64 sums is what makes a carried estimate
// (sf_map_patch) the bits of a full one: k_normals and k_normals_list both come here.  R, trim: normals_walk of the host
__device__ __forceinline__ void normals_point(const SfGrid &g, double r2, float trim, int R, int64_t j, float4 *__restrict__ nrm4, double *__restrict__ cov6)
{
    const float4 p = g.pts[j];
    const float gx = (p.x - g.org[0]) * g.inv_h, gy = (p.y - g.org[1]) * g.inv_h, gz = (p.z - g.org[2]) * g.inv_h;
    const int cx = sf::grid_cell(gx, g.dim[0]), cy = sf::grid_cell(gy, g.dim[1]), cz = sf::grid_cell(gz, g.dim[2]);
    const sf::BallBox box = sf::ball_box(g, gx, gy, gz, cx, cy, cz, R, trim);
    double sum[3] = {0, 0, 0}, mean[3] = {0, 0, 0}, C[6] = {0, 0, 0, 0, 0, 0};
    int cnt = 0;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) {
            if (cnt < 3) break;
            for (int d = 0; d < 3; ++d) mean[d] = sum[d] / cnt;
        }
        sf::box_rows(g, box, [&](uint32_t a, uint32_t b) {
            for (uint32_t k = a; k < b; ++k) {
                const float4 q = g.pts[k];
                const double ex = (double)q.x - (double)p.x, ey = (double)q.y - (double)p.y, ez = (double)q.z - (double)p.z;
                if (!(ex * ex + ey * ey + ez * ez <= r2)) continue;
                if (pass == 0) { sum[0] += q.x; sum[1] += q.y; sum[2] += q.z; ++cnt; }
                else {
                    const double ax = q.x - mean[0], ay = q.y - mean[1], az = q.z - mean[2];
                    C[0] += ax * ax; C[1] += ax * ay; C[2] += ax * az; C[3] += ay * ay; C[4] += ay * az; C[5] += az * az;
                }
            }
        });
    }
    store_normal_cov(cnt, C, j, nrm4, cov6);
}

__global__ __launch_bounds__(256) void k_normals(SfGrid g, double r2, float trim, int R, float4 *__restrict__ nrm4, double *__restrict__ cov6)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= g.n) return;
    normals_point(g, r2, trim, R, j, nrm4, cov6);
}

// ---- k-NN / hybrid normals: the neighbourhood is the k-NN list of the point's own coordinates (sf_knn.hpp), the
// float64 sums run over the list positions in the pairwise tree of wave_tree_sum (absent positions +0.0), so they depend on the
// list alone.  A wave walks its 64 consecutive points one after another; each lane keeps the count and the six sums of "its"
// point in registers and the Jacobi solve then runs once, lane per point (not once per wave with 63 lanes redundant).
__global__ __launch_bounds__(256) void k_normals_knn(SfGrid g, SfWindow w, int k, float thr, float4 *__restrict__ nrm4, double *__restrict__ cov6)
{
    __shared__ sf::WaveKNN ws[256 / 64];
    const int lane = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
    const int64_t base = ((int64_t)blockIdx.x * 4 + wv) * 64;
    if (base >= g.n) return; // (the whole wave: no workgroup barrier below)
    const int64_t i = base + lane;
    const float4 mine = i < g.n ? g.pts[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int nq = (int)min((int64_t)64, g.n - base);
    double myC[6] = {0, 0, 0, 0, 0, 0};
    int mycnt = 0;
    for (int t = 0; t < nq; ++t) {
        const float qx = __shfl(mine.x, t), qy = __shfl(mine.y, t), qz = __shfl(mine.z, t);
        unsigned long long key;
        const int cnt = sf::knn_search<false>(g, w, qx, qy, qz, k, thr, &ws[wv], key);
        const bool has = lane < cnt;
        const float4 p = sf::load_point(g, (uint32_t)key, has);
        double C[6] = {0, 0, 0, 0, 0, 0};
        if (cnt >= 3) {
            const double sx = sf::wave_tree_sum(has ? (double)p.x : 0.0), sy = sf::wave_tree_sum(has ? (double)p.y : 0.0), sz = sf::wave_tree_sum(has ? (double)p.z : 0.0);
            const double mx = sx / cnt, my = sy / cnt, mz = sz / cnt;
            const double ax = has ? (double)p.x - mx : 0.0, ay = has ? (double)p.y - my : 0.0, az = has ? (double)p.z - mz : 0.0;
            C[0] = sf::wave_tree_sum(has ? __dmul_rn(ax, ax) : 0.0);
            C[1] = sf::wave_tree_sum(has ? __dmul_rn(ax, ay) : 0.0);
            C[2] = sf::wave_tree_sum(has ? __dmul_rn(ax, az) : 0.0);
            C[3] = sf::wave_tree_sum(has ? __dmul_rn(ay, ay) : 0.0);
            C[4] = sf::wave_tree_sum(has ? __dmul_rn(ay, az) : 0.0);
            C[5] = sf::wave_tree_sum(has ? __dmul_rn(az, az) : 0.0);
        }
        if (lane == t) {
            mycnt = cnt;
#pragma unroll
            for (int d = 0; d < 6; ++d) myC[d] = C[d];
        }
    }
    if (i >= g.n) return;
    store_normal_cov(mycnt, myC, i, nrm4, cov6);
}

// ---- the estimate carried over sf_map_patch: only where a neighbourhood changed
// One lane per changed position -- t < n_groups: the centroid of voxel t (added), beyond: the old point of voxel t - n_groups
// where it had one (removed).  Every point of the patched index that has it within the radius gets its bit: the cells within
// R of the position's cell, k_normals' own predicate (symmetric in the two points, so "it is my neighbour" and "I am within
// its radius" agree exactly), walked through the same ball_box with the same reach.  A removed point is looked up in the cell the OLD
// grid had it in (its clamp to the old upper face is the one its neighbours' walks saw).  Exact rather than whole cells: the
// re-estimate costs two walks per marked point, the mark one; a sphere holds a sixth of the points of the cube of cells around it.
__global__ __launch_bounds__(256) void k_normals_mark(SfGrid g, int odx, int ody, int odz, double r2, float trim, int R, const uint32_t *__restrict__ g_fresh, const float *__restrict__ g_centroid,
                                                       const float *__restrict__ g_old, int64_t n_groups, uint32_t *__restrict__ bitmap)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * n_groups) return;
    const bool removed = t >= n_groups;
    const int64_t v = removed ? t - n_groups : t;
    if (removed && g_fresh[v]) return;
    const float *src = removed ? g_old : g_centroid;
    const float px = src[3 * v], py = src[3 * v + 1], pz = src[3 * v + 2];
    const int nx = g.dim[0], ny = g.dim[1], nz = g.dim[2];
    const float gx = (px - g.org[0]) * g.inv_h, gy = (py - g.org[1]) * g.inv_h, gz = (pz - g.org[2]) * g.inv_h;
    const int cx = sf::grid_cell(gx, removed ? odx : nx), cy = sf::grid_cell(gy, removed ? ody : ny), cz = sf::grid_cell(gz, removed ? odz : nz);
    // (a removed point beyond a grid that shrank: box_rows visits nothing when the x-range is empty, before it reads a bound; empty y / z ranges never enter their loops)
    sf::box_rows(g, sf::ball_box(g, gx, gy, gz, cx, cy, cz, R, trim), [&](uint32_t a, uint32_t b) {
        for (uint32_t k = a; k < b; ++k) {
            const float4 q = g.pts[k];
            const double ex = (double)px - (double)q.x, ey = (double)py - (double)q.y, ez = (double)pz - (double)q.z;
            if (!(ex * ex + ey * ey + ez * ez <= r2)) continue;
            const uint32_t bit = 1u << (k & 31u);
            if (!(bitmap[k >> 5] & bit)) atomicOr(&bitmap[k >> 5], bit); // (neighbouring positions mark the same points: most find the bit set)
        }
    });
}

// dirty positions per block of 256 (8 words of the bitmap)
__global__ void k_normals_count(const uint32_t *__restrict__ bitmap, int64_t n_blocks, uint32_t *__restrict__ blk_cnt)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blocks) return;
    const uint4 lo = reinterpret_cast<const uint4 *>(bitmap)[2 * b], hi = reinterpret_cast<const uint4 *>(bitmap)[2 * b + 1];
    blk_cnt[b] = (uint32_t)(__popc(lo.x) + __popc(lo.y) + __popc(lo.z) + __popc(lo.w) + __popc(hi.x) + __popc(hi.y) + __popc(hi.z) + __popc(hi.w));
}

// bitmap -> the dirty positions in ascending order: one lane per position, its slot = the dirty ones in front of it
__global__ __launch_bounds__(256) void k_normals_compact(const uint32_t *__restrict__ bitmap, const uint32_t *__restrict__ blk_pre, int64_t n, int64_t cap, uint32_t *__restrict__ list)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint32_t w = threadIdx.x >> 5, bit = threadIdx.x & 31u;
    const uint32_t *words = bitmap + (size_t)blockIdx.x * 8;
    const uint32_t mine = words[w];
    if (!((mine >> bit) & 1u)) return;
    uint32_t o = blk_pre[blockIdx.x] + (uint32_t)__popc(mine & ((1u << bit) - 1u));
    for (uint32_t k = 0; k < w; ++k) o += (uint32_t)__popc(words[k]);
    if ((int64_t)o < cap) list[o] = (uint32_t)p;
}

__global__ __launch_bounds__(256) void k_normals_list(SfGrid g, double r2, float trim, int R, const uint32_t *__restrict__ list, int64_t n_list, float4 *__restrict__ nrm4, double *__restrict__ cov6)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_list) return;
    normals_point(g, r2, trim, R, (int64_t)list[t], nrm4, cov6);
}

// What k_normals, k_normals_mark and k_normals_list walk by, one function so that a carried estimate and a full one see the same
// cells: the rule's r2 in float64, the reach of sf_walk.hpp (c) in float64, capped by the grid before the conversion, and
// ball_box's trim for that reach, rounded up (a larger trim only keeps more cells).
struct NormalsWalk { double r2; float trim; int R; };
inline NormalsWalk normals_walk(const SfGrid &g, float radius)
{
    NormalsWalk w;
    w.r2 = (double)radius * (double)radius;
    const double reach = std::ceil(((double)radius * (1.0 + 1.0e-6) + (double)g.gap_eps) * (double)g.inv_h);
    w.R = (int)std::min(std::max(reach, 1.0), (double)std::max(g.dim[0], std::max(g.dim[1], g.dim[2])));
    const double trim = ((double)radius * (1.0 + 1.0e-6) + (double)g.gap_eps) * (double)g.inv_h - (double)(w.R - 1);
    w.trim = (float)trim;
    if ((double)w.trim < trim) w.trim = std::nextafter(w.trim, INFINITY);
    return w;
}

int carry_reestimate(sf_map *m, const sf_cloud::MergeRecord &rec, const int old_dim[3], float radius, bool with_cov, int64_t *n_dirty)
{
    sf_ctx *ctx = m->ctx;
    hipStream_t st = ctx->stream;
    const SfGrid &g = m->grid;
    const int64_t n = g.n, ng = rec.n_groups;
    *n_dirty = 0;
    if (n <= 0) return SF_OK;
    const NormalsWalk w = normals_walk(g, radius);
    // [bitmap: 8 words per block of 256 positions | counts | their exclusive prefix (one entry more: the total)]
    const int64_t nb = sf::div_up(n, 256);
    const size_t off_cnt = 4 * 8 * (size_t)nb, off_pre = off_cnt + 4 * (size_t)(nb + 1), total = off_pre + 4 * (size_t)(nb + 1);
    SF_TRY(m->carry_tmp.reserve(total));
    unsigned char *base = m->carry_tmp.as<unsigned char>();
    uint32_t *bitmap = reinterpret_cast<uint32_t *>(base), *blk_cnt = reinterpret_cast<uint32_t *>(base + off_cnt), *blk_pre = reinterpret_cast<uint32_t *>(base + off_pre);
    SF_HIP(hipMemsetAsync(base, 0, off_pre, st)); // bitmap and counts (the count behind the last block stays 0)
    hipLaunchKernelGGL(k_normals_mark, dim3(nblk(2 * ng)), dim3(256), 0, st, g, old_dim[0], old_dim[1], old_dim[2], w.r2, w.trim, w.R, rec.g_fresh, rec.g_centroid, rec.g_old, ng, bitmap);
    hipLaunchKernelGGL(k_normals_count, dim3(nblk(nb)), dim3(256), 0, st, bitmap, nb, blk_cnt);
    SF_TRY(sf::scan_u32<0>(ctx, blk_cnt, blk_pre, nb + 1));
    uint32_t *h_cnt = &ctx->h_pinned->carry_count;
    SF_HIP(hipMemcpyAsync(h_cnt, blk_pre + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SF_HIP(hipGetLastError());
    SF_HIP(hipStreamSynchronize(st)); // the one read-back: the size of the list launch (and sf_map_normals_carry_info)
    const int64_t nd = (int64_t)*h_cnt;
    *n_dirty = nd;
    if (nd <= 0) return SF_OK;
    // (the list grows in steps: a growth step's share of the map moves little from one step to the next)
    SF_TRY(m->carry_list.reserve(sizeof(uint32_t) * (size_t)std::max<int64_t>(nd + nd / 2, 1 << 16)));
    uint32_t *list = m->carry_list.as<uint32_t>();
    hipLaunchKernelGGL(k_normals_compact, dim3((unsigned)nb), dim3(256), 0, st, bitmap, blk_pre, n, nd, list);
    hipLaunchKernelGGL(k_normals_list, dim3(nblk(nd)), dim3(256), 0, st, g, w.r2, w.trim, w.R, list, nd, m->nrm4.as<float4>(), with_cov ? m->cov6.as<double>() : nullptr);
    SF_HIP(hipGetLastError());
    return SF_OK; // enqueued behind the patch: every reader of the normals is on this stream
}

__global__ void k_normals_from_host_order(SfGrid g, const float *__restrict__ nrm_orig, float4 *__restrict__ nrm4)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= g.n) return;
    const uint32_t i = __float_as_uint(g.pts[j].w);
    nrm4[j] = make_float4(nrm_orig[3 * (size_t)i], nrm_orig[3 * (size_t)i + 1], nrm_orig[3 * (size_t)i + 2], __int_as_float(0));
}

__global__ void k_cov_to_host_order(SfGrid g, const double *__restrict__ cov6, double *__restrict__ cov_orig)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= g.n) return;
    const uint32_t i = __float_as_uint(g.pts[j].w);
#pragma unroll
    for (int d = 0; d < 6; ++d) cov_orig[6 * (size_t)i + d] = cov6[6 * (size_t)j + d];
}

__global__ void k_normals_to_host_order(SfGrid g, const float4 *__restrict__ nrm4, float *__restrict__ nrm_orig, int32_t *__restrict__ cnt_orig)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= g.n) return;
    const uint32_t i = __float_as_uint(g.pts[j].w);
    const float4 v = nrm4[j];
    nrm_orig[3 * (size_t)i] = v.x; nrm_orig[3 * (size_t)i + 1] = v.y; nrm_orig[3 * (size_t)i + 2] = v.z;
    cnt_orig[i] = __float_as_int(v.w);
}

// test hook (sf_test_linalg, op eigvec): smallest_eigvec itself, one case per thread, workgroups of 64
__global__ __launch_bounds__(64) void k_test_eigvec(const double *__restrict__ in, int in_stride, int64_t cases, double *__restrict__ out, int out_stride)
{
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= cases) return;
    double C[9], nv[3];
    for (int k = 0; k < 9; ++k) C[k] = in[(size_t)i * in_stride + k];
    smallest_eigvec(C, nv);
    for (int k = 0; k < 3; ++k) out[(size_t)i * out_stride + k] = nv[k];
}

} // namespace

int sf::test_map_eigvec(sf_ctx *ctx, const double *in, int in_stride, int64_t cases, double *out, int out_stride)
{
    if (cases == 0) return SF_OK;
    SF_HIP(hipSetDevice(ctx->device));
    const size_t n_in = (size_t)cases * in_stride, n_out = (size_t)cases * out_stride;
    sf::DevBuf din, dout; // freed on every path
    SF_TRY(din.reserve(sizeof(double) * n_in));
    SF_TRY(dout.reserve(sizeof(double) * n_out));
    SF_TRY(sf::upload_staged(ctx, din.p, in, sizeof(double) * n_in));
    SF_TRY(sf::upload_staged(ctx, dout.p, out, sizeof(double) * n_out));
    hipLaunchKernelGGL(k_test_eigvec, dim3((unsigned)sf::div_up(cases, 64)), dim3(64), 0, ctx->stream, din.as<double>(), in_stride, cases, dout.as<double>(), out_stride);
    SF_HIP(hipGetLastError());
    SF_HIP(hipMemcpyAsync(out, dout.p, sizeof(double) * n_out, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    return SF_OK;
}

namespace {
// what the two estimates share: the buffers, the profiled span around launch(nrm4, cov6 or nullptr), the synchronise and the
// record of how the normals were made (what sf_map_patch carries or re-runs: sf_map_set_normals_carry)
template <class L>
int estimate_normals(sf_map *m, int knn_k, float radius, int with_covariance, L launch)
{
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    SF_TRY(m->nrm4.reserve(sizeof(float4) * (size_t)std::max<int64_t>(m->n, 1)));
    m->has_cov = false;
    if (with_covariance) SF_TRY(m->cov6.reserve(sizeof(double) * 6 * (size_t)std::max<int64_t>(m->n, 1)));
    ProfSpan span(m);
    if (m->grid.n > 0) launch(m->nrm4.as<float4>(), with_covariance ? m->cov6.as<double>() : nullptr);
    span.end();
    SF_HIP(hipGetLastError());
    SF_HIP(hipStreamSynchronize(ctx->stream));
    prof_read(m);
    m->grid.nrm = m->nrm4.as<float4>();
    m->has_normals = true;
    m->has_cov = with_covariance != 0;
    m->nrm_estimated = true;
    m->nrm_knn_k = knn_k; // 0: the radius form, carried; > 0: re-run in full behind a patch
    m->nrm_radius = radius;
    m->nrm_with_cov = with_covariance != 0;
    m->generation = sf::next_generation();
    return SF_OK;
}
} // namespace

extern "C" int sf_map_estimate_normals_cov(sf_map *m, float radius, int with_covariance)
{
    SF_CHECK(m && m->built, SF_ERR_STATE, "map not built");
    SF_CHECK(radius > 0, SF_ERR_INVALID, "radius must be positive");
    const NormalsWalk w = normals_walk(m->grid, radius);
    return estimate_normals(m, 0, radius, with_covariance, [&](float4 *nrm4, double *cov6) {
        hipLaunchKernelGGL(k_normals, dim3(nblk(m->grid.n)), dim3(256), 0, m->ctx->stream, m->grid, w.r2, w.trim, w.R, nrm4, cov6);
    });
}

extern "C" int sf_map_estimate_normals_knn(sf_map *m, int k, float max_radius, int with_covariance)
{
    SF_CHECK(m && m->built, SF_ERR_STATE, "map not built");
    SF_CHECK(k >= 1 && k <= SF_KNN_MAX, SF_ERR_INVALID, "k must be 1 .. %d (got %d)", SF_KNN_MAX, k);
    SF_CHECK(!std::isnan(max_radius), SF_ERR_INVALID, "max_radius must be a number (<= 0 or inf: no limit)");
    const float thr = (max_radius > 0 && std::isfinite(max_radius)) ? (float)(max_radius * max_radius) : INFINITY;
    return estimate_normals(m, k, max_radius, with_covariance, [&](float4 *nrm4, double *cov6) {
        hipLaunchKernelGGL(k_normals_knn, dim3(nblk(m->grid.n)), dim3(256), 0, m->ctx->stream, m->grid, SfWindow{}, k, thr, nrm4, cov6);
    });
}

// ------------------------------------------------------------------ outlier removal (extension, no reference code)
namespace {

// the mean neighbour distance of every indexed point, the shape of k_normals_knn: a wave walks its 64 consecutive points, all lanes
// on one query; list position p is lane p and contributes sqrt((double)d2) of its key's upper word (absent: +0.0), no point is
// loaded; lane t keeps the result of point t and the wave writes its 64 results at the end, in original point order
__global__ __launch_bounds__(256) void k_knn_mean_dist(SfGrid g, int K, int pcl, double *__restrict__ mean_dist)
{
    __shared__ sf::WaveKNN ws[256 / 64];
    const int lane = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
    const int64_t base = ((int64_t)blockIdx.x * 4 + wv) * 64;
    if (base >= g.n) return; // (the whole wave: no workgroup barrier below)
    const int64_t i = base + lane;
    const float4 mine = i < g.n ? g.pts[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int nq = (int)min((int64_t)64, g.n - base);
    const SfWindow none{}; // (never read: knn_search<false>)
    double myd = 0.0;
    for (int t = 0; t < nq; ++t) {
        const float qx = __shfl(mine.x, t), qy = __shfl(mine.y, t), qz = __shfl(mine.z, t);
        unsigned long long key;
        const int cnt = sf::knn_search<false>(g, none, qx, qy, qz, K, INFINITY, &ws[wv], key);
        const double sum = sf::wave_tree_sum(lane < cnt ? sqrt((double)__uint_as_float((uint32_t)(key >> 32))) : 0.0);
        const int div = pcl ? cnt - 1 : cnt; // PCL: position 0 is the point itself (or a coincident one), a zero that is not a neighbour
        const double d = div > 0 ? sum / (double)div : 0.0;
        if (lane == t) myd = d;
    }
    if (i < g.n) mean_dist[__float_as_uint(mine.w)] = myd;
}

__global__ void k_fill_f64(double *__restrict__ p, int64_t n, double v)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// One level of the float64 pairwise tree: workgroup b sums leaves [256 b, 256 b + 256) -- wave_tree_sum over the 64 leaves of each
// wave, the four wave sums pairwise -- which is the subtree over those leaves of the full tree v[0::2] + v[1::2] ... over the
// array padded with +0.0 to a power of two; applied again to its own output until one value is left.  A NaN leaf (a point that is
// not indexed) and a leaf past the end are +0.0.  sq: the leaf is (v - mean)^2, the product formed by its own multiply.
__global__ __launch_bounds__(256) void k_tree_sum(const double *__restrict__ v, int64_t n, int sq, double mean, double *__restrict__ out)
{
    __shared__ double wsum[256 / 64];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double x = 0.0;
    if (i < n) {
        const double d = v[i];
        if (d == d) x = sq ? __dmul_rn(__dsub_rn(d, mean), __dsub_rn(d, mean)) : d;
    }
    x = sf::wave_tree_sum(x);
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = __dadd_rn(__dadd_rn(wsum[0], wsum[1]), __dadd_rn(wsum[2], wsum[3]));
}

// The kept count: every wave adds its ballot's popcount to one of KEPT_SLOTS integer counters, 128 bytes apart, and k_sum_kept adds
// those up into the word behind them.  Atomics on one address are served one after another where that cache line lives, so one
// counter for all waves would put n / 64 of them in a single queue; consecutive waves go to different lines instead and each
// line's queue is KEPT_SLOTS times shorter.  Integer sums: order independent.
constexpr int KEPT_SLOTS = 256, KEPT_STRIDE = 16, KEPT_WORDS = (KEPT_SLOTS + 1) * KEPT_STRIDE; // in 8-byte words
__device__ __forceinline__ void add_kept(bool keep, unsigned long long *__restrict__ kept)
{
    const unsigned long long b = __ballot(keep);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(kept + (size_t)((blockIdx.x * 4u + (threadIdx.x >> 6)) & (KEPT_SLOTS - 1)) * KEPT_STRIDE, (unsigned long long)__popcll(b));
}
__global__ __launch_bounds__(KEPT_SLOTS) void k_sum_kept(unsigned long long *__restrict__ kept)
{
    __shared__ unsigned long long wsum[KEPT_SLOTS / 64];
    unsigned long long v = kept[(size_t)threadIdx.x * KEPT_STRIDE];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) kept[(size_t)KEPT_SLOTS * KEPT_STRIDE] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// keep iff d <= thr (PCL) / d < thr (strict: O3D) in float64; NaN (not indexed) is not kept.
__global__ __launch_bounds__(256) void k_flag_mean_dist(const double *__restrict__ mean_dist, int64_t n, double thr, int strict, uint8_t *__restrict__ flags,
                                                         unsigned long long *__restrict__ kept)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    if (i < n) {
        const double d = mean_dist[i];
        keep = strict ? d < thr : d <= thr;
        flags[i] = keep ? 1 : 0;
    }
    add_kept(keep, kept);
}

// count_j = the number of indexed points q with l2_simple(p_j, q) < r2 (p_j itself included), one lane per indexed point: the
// radius_walk of sf_walk.hpp, which proves that nothing the rule accepts is lost.  No early exit at count > min_neighbors: the
// counts are an output.
__global__ __launch_bounds__(256) void k_radius_count(SfGrid g, float r2, int R, int min_neighbors, int32_t *__restrict__ n_neighbors, uint8_t *__restrict__ flags,
                                                       unsigned long long *__restrict__ kept)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    if (j < g.n) {
        const float4 p = g.pts[j];
        int cnt = 0;
        sf::radius_walk<false, false>(g, p, r2, R, 0u, nullptr, [&](uint32_t, int32_t, bool hit) { cnt += hit ? 1 : 0; });
        const uint32_t id = __float_as_uint(p.w);
        keep = cnt > min_neighbors;
        n_neighbors[id] = cnt;
        flags[id] = keep ? 1 : 0;
    }
    add_kept(keep, kept);
}

// K of the statistical filter's neighbour list, 0 for arguments it refuses
inline int sor_list_length(int k, int flavour)
{
    if (flavour == SF_SOR_PCL) return (k >= 1 && k <= SF_KNN_MAX - 1) ? k + 1 : 0;
    if (flavour == SF_SOR_O3D) return (k >= 1 && k <= SF_KNN_MAX) ? k : 0;
    return 0;
}
#define SF_CHECK_SOR(k, flavour) SF_CHECK(sor_list_length(k, flavour) > 0, SF_ERR_INVALID, "statistical outliers: flavour SF_SOR_PCL with k 1 .. %d or SF_SOR_O3D with k 1 .. %d (got flavour %d, k %d)", SF_KNN_MAX - 1, SF_KNN_MAX, flavour, k)
#define SF_CHECK_ROR(radius, min_neighbors) SF_CHECK((radius) > 0 && std::isfinite(radius) && (min_neighbors) >= 0, SF_ERR_INVALID, "radius outliers: radius must be positive and finite, min_neighbors >= 0 (got %g, %d)", (double)(radius), min_neighbors)

// out_red: [the kept counters and their sum, KEPT_WORDS words | the levels of the tree, one after another]
int outlier_buffers(sf_map *m, size_t val_bytes)
{
    const size_t n = (size_t)m->n, nb = (size_t)sf::div_up(m->n, 256);
    SF_TRY(m->out_flags.reserve(n));
    SF_TRY(m->out_val.reserve(val_bytes * n));
    // the levels hold nb, ceil(nb / 256), ... 1 sums: each at most a 256th of the one before plus one, so together below
    // nb + nb / 255 + (number of levels <= 4, m->n < 2^28) <= nb + nb / 128 + 8
    SF_TRY(m->out_red.reserve(sizeof(double) * (KEPT_WORDS + nb + nb / 128 + 8)));
    SF_HIP(hipMemsetAsync(m->out_red.p, 0, sizeof(unsigned long long) * KEPT_WORDS, m->ctx->stream));
    return SF_OK;
}

// the tree sum of v[0 .. n) (or of its squared deviations from mean) -> *h_sum; synchronises the stream
int tree_sum(sf_map *m, const double *v, int64_t n, bool sq, double mean, double *h_sum)
{
    sf_ctx *ctx = m->ctx;
    double *level = m->out_red.as<double>() + KEPT_WORDS;
    const double *in = v;
    int64_t cnt = n;
    bool first = true;
    do {
        const int64_t nb = sf::div_up(cnt, 256);
        hipLaunchKernelGGL(k_tree_sum, dim3((unsigned)nb), dim3(256), 0, ctx->stream, in, cnt, (first && sq) ? 1 : 0, mean, level);
        in = level;
        level += nb;
        cnt = nb;
        first = false;
    } while (cnt > 1);
    SF_TRY(read_words(ctx, in, 1));
    std::memcpy(h_sum, ctx->h_pinned->readback, sizeof(double));
    return SF_OK;
}

int read_kept(sf_map *m, sf_outlier_stats *st)
{
    SF_TRY(read_words(m->ctx, m->out_red.as<unsigned long long>() + (size_t)KEPT_SLOTS * KEPT_STRIDE, 1));
    prof_read(m);
    st->n_kept = (int64_t)m->ctx->h_pinned->readback[0];
    return SF_OK;
}

// The filters proper, shared by the map calls and the cloud calls: the flags stay in m->out_flags, the distances / counts in
// m->out_val (original point order), only the statistics come to the host.  Arguments are checked by the callers.
int statistical_outliers_device(sf_map *m, int K, bool pcl, double std_ratio, sf_outlier_stats *st)
{
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t n = m->n, nv = m->grid.n;
    *st = sf_outlier_stats{n, nv, 0, 0.0, 0.0, 0.0};
    if (n == 0) return SF_OK;
    SF_TRY(outlier_buffers(m, sizeof(double)));
    double *dist = m->out_val.as<double>();
    ProfSpan span(m);
    hipLaunchKernelGGL(k_fill_f64, dim3(nblk(n)), dim3(256), 0, s, dist, n, (double)NAN);
    if (nv > 0) {
        hipLaunchKernelGGL(k_knn_mean_dist, dim3(nblk(nv)), dim3(256), 0, s, m->grid, K, pcl ? 1 : 0, dist);
        double sum = 0.0, sum2 = 0.0;
        int rc = tree_sum(m, dist, n, false, 0.0, &sum);
        st->mean = sum / (double)nv;
        if (rc == SF_OK && nv >= 2) {
            rc = tree_sum(m, dist, n, true, st->mean, &sum2);
            st->stddev = std::sqrt(sum2 / (double)(nv - 1));
        }
        SF_TRY(rc);
        st->threshold = st->mean + std_ratio * st->stddev;
    }
    hipLaunchKernelGGL(k_flag_mean_dist, dim3(nblk(n)), dim3(256), 0, s, dist, n, st->threshold, pcl ? 0 : 1, m->out_flags.as<uint8_t>(), m->out_red.as<unsigned long long>());
    hipLaunchKernelGGL(k_sum_kept, dim3(1), dim3(KEPT_SLOTS), 0, s, m->out_red.as<unsigned long long>());
    span.end();
    return read_kept(m, st);
}

// the reach (radius_walk, (c)), in float64, capped by the grid before the conversion
inline int radius_reach(const SfGrid &g, float r2)
{
    const double reach = std::ceil((std::sqrt((double)r2) * (1.0 + 1.0e-6) + (double)g.gap_eps) * (double)g.inv_h);
    return (int)std::min(std::max(reach, 1.0), (double)std::max(g.dim[0], std::max(g.dim[1], g.dim[2])));
}

int radius_outliers_device(sf_map *m, double radius, int min_neighbors, sf_outlier_stats *st)
{
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t n = m->n, nv = m->grid.n;
    *st = sf_outlier_stats{n, nv, 0, 0.0, 0.0, 0.0};
    if (n == 0) return SF_OK;
    SF_TRY(outlier_buffers(m, sizeof(int32_t)));
    const float r2 = (float)(radius * radius);
    const SfGrid &g = m->grid;
    const int R = radius_reach(g, r2);
    SF_HIP(hipMemsetAsync(m->out_flags.p, 0, (size_t)n, s)); // points that are not indexed: not kept, no neighbours
    SF_HIP(hipMemsetAsync(m->out_val.p, 0, sizeof(int32_t) * (size_t)n, s));
    ProfSpan span(m);
    if (nv > 0)
        hipLaunchKernelGGL(k_radius_count, dim3(nblk(nv)), dim3(256), 0, s, g, r2, R, min_neighbors, m->out_val.as<int32_t>(), m->out_flags.as<uint8_t>(),
                           m->out_red.as<unsigned long long>());
    hipLaunchKernelGGL(k_sum_kept, dim3(1), dim3(KEPT_SLOTS), 0, s, m->out_red.as<unsigned long long>());
    span.end();
    return read_kept(m, st);
}

int download_outliers(sf_map *m, uint8_t *keep, void *val, size_t val_bytes)
{
    sf_ctx *ctx = m->ctx;
    if (m->n == 0 || (!keep && !val)) return SF_OK;
    if (keep) SF_HIP(hipMemcpyAsync(keep, m->out_flags.p, (size_t)m->n, hipMemcpyDeviceToHost, ctx->stream));
    if (val) SF_HIP(hipMemcpyAsync(val, m->out_val.p, val_bytes * (size_t)m->n, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    return SF_OK;
}

// index the cloud with a temporary map, let flag(map, &st) leave the keep flags in its out_flags, compact (the order is kept:
// compact_cloud, as after a crop).  The outlier filters and the cluster filters (sf_cluster.hpp) of a cloud all come here.
template <class S, class F>
int filter_cloud(sf_cloud *c, float cell, S *stats, F flag)
{
    S st{};
    if (stats) *stats = st;
    sf::cloud_touch(c);
    if (c->n == 0) { c->n_last_idx = 0; return SF_OK; }
    sf_map *tmp = nullptr;
    SF_TRY(sf_map_create(c->ctx, &tmp));
    int rc = sf_map_build(tmp, c, cell);
    if (rc == SF_OK) rc = flag(tmp, &st);
    if (rc == SF_OK) rc = sf::compact_cloud(c, tmp->out_flags.as<uint8_t>());
    sf_map_destroy(tmp);
    if (rc == SF_OK && stats) *stats = st;
    return rc;
}

} // namespace

extern "C" int sf_map_statistical_outliers(sf_map *m, int k, double std_ratio, int flavour, uint8_t *keep, double *mean_dist, sf_outlier_stats *stats)
{
    SF_CHECK(m && m->built, SF_ERR_STATE, "map not built");
    SF_CHECK_SOR(k, flavour);
    sf_outlier_stats st;
    SF_TRY(statistical_outliers_device(m, sor_list_length(k, flavour), flavour == SF_SOR_PCL, std_ratio, &st));
    if (stats) *stats = st;
    return download_outliers(m, keep, mean_dist, sizeof(double));
}

extern "C" int sf_map_radius_outliers(sf_map *m, double radius, int min_neighbors, uint8_t *keep, int32_t *n_neighbors, sf_outlier_stats *stats)
{
    SF_CHECK(m && m->built, SF_ERR_STATE, "map not built");
    SF_CHECK_ROR(radius, min_neighbors);
    sf_outlier_stats st;
    SF_TRY(radius_outliers_device(m, radius, min_neighbors, &st));
    if (stats) *stats = st;
    return download_outliers(m, keep, n_neighbors, sizeof(int32_t));
}

extern "C" int sf_cloud_remove_statistical_outliers(sf_cloud *c, int k, double std_ratio, int flavour, float cell, sf_outlier_stats *stats)
{
    SF_CHECK(c, SF_ERR_INVALID, "bad arguments");
    SF_CHECK_SOR(k, flavour);
    const int K = sor_list_length(k, flavour);
    return filter_cloud(c, cell, stats, [=](sf_map *m, sf_outlier_stats *st) { return statistical_outliers_device(m, K, flavour == SF_SOR_PCL, std_ratio, st); });
}

extern "C" int sf_cloud_remove_radius_outliers(sf_cloud *c, double radius, int min_neighbors, float cell, sf_outlier_stats *stats)
{
    SF_CHECK(c, SF_ERR_INVALID, "bad arguments");
    SF_CHECK_ROR(radius, min_neighbors);
    return filter_cloud(c, cell, stats, [=](sf_map *m, sf_outlier_stats *st) { return radius_outliers_device(m, radius, min_neighbors, st); });
}

// ------------------------------------------------------------------ radius search with variable-length rows (extension, no reference code)
#include "sf_radius.hpp"

// ------------------------------------------------------------------ clustering (extension, no reference code)
#include "sf_cluster.hpp"

// ------------------------------------------------------------------ plane segmentation (extension, no reference code)
#include "sf_plane.hpp"

// ------------------------------------------------------------------ per-label boxes, multi-box removal (extension, no reference code)
#include "sf_box.hpp"

extern "C" int sf_map_profile_launches(sf_map *m, int on)
{
    SF_CHECK(m, SF_ERR_INVALID, "bad arguments");
    m->profile = on != 0;
    m->last_launch_ms = -1.0f;
    return SF_OK;
}

extern "C" int sf_map_last_launch_ms(sf_map *m, float *ms)
{
    SF_CHECK(m && ms, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(m->profile && m->last_launch_ms >= 0.0f, SF_ERR_STATE, "nothing timed (sf_map_profile_launches, then a query or an estimate)");
    *ms = m->last_launch_ms;
    return SF_OK;
}

extern "C" int sf_map_set_normals_carry(sf_map *m, int on)
{
    SF_CHECK(m, SF_ERR_INVALID, "bad arguments");
    m->normals_carry = on != 0;
    return SF_OK;
}

extern "C" int sf_map_normals_carry_info(sf_map *m, int64_t out[4])
{
    SF_CHECK(m && out, SF_ERR_INVALID, "bad arguments");
    for (int k = 0; k < 4; ++k) out[k] = m->carry_info[k];
    return SF_OK;
}

extern "C" int sf_map_estimate_normals(sf_map *m, float radius) { return sf_map_estimate_normals_cov(m, radius, 0); }

extern "C" int sf_map_download_covariances(sf_map *m, double *cov6, int64_t cap, int64_t *n)
{
    SF_CHECK(m && m->built && m->has_cov, SF_ERR_STATE, "no covariances (sf_map_estimate_normals_cov with with_covariance = 1)");
    if (n) *n = m->n;
    SF_CHECK(cap >= m->n && cov6, SF_ERR_INVALID, "buffer too small");
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    sf::DevBuf dc;
    const size_t bytes = sizeof(double) * 6 * (size_t)std::max<int64_t>(m->n, 1);
    SF_TRY(dc.reserve(bytes));
    SF_HIP(hipMemsetAsync(dc.p, 0, bytes, ctx->stream)); // points that are not indexed (non-finite) keep zeros
    if (m->grid.n > 0)
        hipLaunchKernelGGL(k_cov_to_host_order, dim3(nblk(m->grid.n)), dim3(256), 0, ctx->stream, m->grid, m->cov6.as<double>(), dc.as<double>());
    SF_HIP(hipMemcpyAsync(cov6, dc.p, sizeof(double) * 6 * (size_t)m->n, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    return SF_OK;
}

extern "C" int sf_map_set_normals(sf_map *m, const float *normals, int64_t n)
{
    SF_CHECK(m && m->built, SF_ERR_STATE, "map not built");
    SF_CHECK(normals && n == m->n, SF_ERR_INVALID, "normals must match the map size (%lld)", (long long)m->n);
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    SF_TRY(m->nrm4.reserve(sizeof(float4) * (size_t)std::max<int64_t>(m->n, 1)));
    sf::DevBuf tmp;
    SF_TRY(tmp.reserve(sizeof(float) * 3 * (size_t)std::max<int64_t>(n, 1)));
    SF_HIP(hipMemcpyAsync(tmp.p, normals, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    if (m->grid.n > 0)
        hipLaunchKernelGGL(k_normals_from_host_order, dim3(nblk(m->grid.n)), dim3(256), 0, ctx->stream, m->grid, tmp.as<float>(), m->nrm4.as<float4>());
    SF_HIP(hipStreamSynchronize(ctx->stream));
    m->grid.nrm = m->nrm4.as<float4>();
    m->has_normals = true;
    m->has_cov = false;
    m->nrm_estimated = false; // normals of the caller's: nothing to re-estimate them with, sf_map_patch drops them
    m->nrm_knn_k = 0;
    m->generation = sf::next_generation();
    return SF_OK;
}

extern "C" int sf_map_download_normals(sf_map *m, float *normals, int32_t *n_neighbors, int64_t cap, int64_t *n)
{
    SF_CHECK(m && m->built && m->has_normals, SF_ERR_STATE, "no normals");
    if (n) *n = m->n;
    SF_CHECK(cap >= m->n && normals, SF_ERR_INVALID, "buffer too small");
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    sf::DevBuf dn, dc;
    SF_TRY(dn.reserve(sizeof(float) * 3 * (size_t)std::max<int64_t>(m->n, 1)));
    SF_TRY(dc.reserve(sizeof(int32_t) * (size_t)std::max<int64_t>(m->n, 1)));
    SF_HIP(hipMemsetAsync(dn.p, 0, sizeof(float) * 3 * (size_t)std::max<int64_t>(m->n, 1), ctx->stream));
    SF_HIP(hipMemsetAsync(dc.p, 0, sizeof(int32_t) * (size_t)std::max<int64_t>(m->n, 1), ctx->stream));
    if (m->grid.n > 0)
        hipLaunchKernelGGL(k_normals_to_host_order, dim3(nblk(m->grid.n)), dim3(256), 0, ctx->stream, m->grid, m->nrm4.as<float4>(), dn.as<float>(), dc.as<int32_t>());
    SF_HIP(hipMemcpyAsync(normals, dn.p, sizeof(float) * 3 * (size_t)m->n, hipMemcpyDeviceToHost, ctx->stream));
    if (n_neighbors) SF_HIP(hipMemcpyAsync(n_neighbors, dc.p, sizeof(int32_t) * (size_t)m->n, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    return SF_OK;
}
