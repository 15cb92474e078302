// sf_cluster.hpp -- Euclidean and DBSCAN clustering of an indexed map (extension, no reference code).  Included by
// sf_map.hip after the outlier block: it uses that block's k_radius_count, radius_reach, outlier_buffers, the kept counters and
// filter_cloud, and ProfSpan / read_words of sf_map.hip.  Neighbours are found by sf::radius_walk (sf_walk.hpp), the walk of
// k_radius_count itself, so the core flags and the edges of the graph come from one rule and one proof.
//
// The graph: indexed points i != j are adjacent iff l2_simple(x_i, x_j) < r2 (float32, unfused, strict -- symmetric bit for bit).
// Clusters are the connected components of the graph restricted to core points (count_i >= min_points; Euclidean: every indexed
// point), found by a lock-free union-find over the SORTED positions j of the index, then numbered by the smallest ORIGINAL index of
// their core points.  Only integer atomics are used and every step computes a function of the components, so the labels depend on
// the cloud and the parameters alone.
#pragma once

namespace {

constexpr uint32_t CL_NONE = 0xFFFFFFFFu;

// ---- the union-find of k_cluster_hook.  parent[x] <= x always and parent[x] < x once x is not a root; a position that has
// stopped being a root never becomes one again.  Inside the kernel EVERY access to parent[] is an agent-scope relaxed atomic
// (the L2s of the XCDs are not coherent and a CU's L1 is never refreshed by another CU's stores, so a plain load may be stale
// without bound and may be kept in a register).  Even so a load may return an older value: that is an earlier parent of x, which
// is an ancestor of x still.  So every find descends strictly and ends at some ancestor, root or not; whether it IS a root is
// decided by the compare-and-swap alone, which acts on the one copy of the word.
__device__ __forceinline__ uint32_t par_load(uint32_t *parent, uint32_t x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// path halving: x's parent becomes its grandparent, then x moves there.  The store is made only to an x seen with a parent other
// than itself -- never a root again, so no compare-and-swap is waiting on that word -- and writes an ancestor of x below x; two
// lanes that race here both write ancestors.
__device__ __forceinline__ uint32_t cl_find(uint32_t *parent, uint32_t x)
{
    for (;;) {
        const uint32_t p = par_load(parent, x);
        if (p == x) return x;
        const uint32_t gp = par_load(parent, p);
        if (gp == p) return p;
        __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = gp;
    }
}

// unites the sets of a and b, returns a position of the united set (the smaller end of the hook).  The larger of the two ends found
// is hooked under the smaller iff it is a root at that instant.  A failure means another lane hooked it meanwhile: the value seen is
// where, and the finds start again from there.  Nothing here waits for another wave's store: every find descends, every failed
// compare-and-swap is paid for by a hook that succeeded elsewhere, and there are fewer hooks than points.
__device__ __forceinline__ uint32_t cl_unite(uint32_t *parent, uint32_t a, uint32_t b)
{
    uint32_t ra = cl_find(parent, a), rb = cl_find(parent, b);
    while (ra != rb) {
        const uint32_t hi = max(ra, rb), lo = min(ra, rb);
        uint32_t seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return lo;
        ra = cl_find(parent, seen);
        rb = cl_find(parent, lo);
    }
    return ra;
}

// sorted order: parent[j] = j, the per-root minimum id and size cleared, core[j] = the flag k_radius_count left for the point
__global__ __launch_bounds__(256) void k_cluster_init(SfGrid g, const uint8_t *__restrict__ flags, uint32_t *__restrict__ parent, uint32_t *__restrict__ rmin,
                                                       uint32_t *__restrict__ rsize, uint8_t *__restrict__ core)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= g.n) return;
    parent[j] = (uint32_t)j;
    rmin[j] = CL_NONE;
    rsize[j] = 0u;
    if (flags) core[j] = flags[__float_as_uint(g.pts[j].w)];
}

// One lane per core position j: every accepted core candidate k < j is united with j, so each edge of the core graph is met once,
// from its larger end.  `mine` follows j's set down (any position of the set will do for the next union).
template <bool ALL_CORE>
__global__ __launch_bounds__(256) void k_cluster_hook(SfGrid g, float r2, int R, const uint8_t *__restrict__ core, uint32_t *parent)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= g.n) return;
    if (!ALL_CORE && !core[j]) return;
    uint32_t mine = (uint32_t)j;
    sf::radius_walk<false, true>(g, g.pts[j], r2, R, (uint32_t)j, nullptr, [&](uint32_t k, int32_t, bool hit) {
        if (hit && (ALL_CORE || core[k])) mine = cl_unite(parent, mine, k);
    });
}

// After the kernel boundary: parent[j] = the root of j, which is the smallest sorted position of its component.  Plain loads: what
// another lane of this launch writes meanwhile is that lane's root, an ancestor as well.  The root learns the smallest original id
// and the number of its core points, one atomic of each kind per wave and distinct root: a surface map is one component, and
// atomics on one word are served one after another.
template <bool ALL_CORE>
__global__ __launch_bounds__(256) void k_cluster_flatten(SfGrid g, const uint8_t *__restrict__ core, uint32_t *parent, uint32_t *__restrict__ rmin,
                                                          uint32_t *__restrict__ rsize)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = j < g.n && (ALL_CORE || core[j]);
    uint32_t root = CL_NONE, id = CL_NONE;
    if (live) {
        uint32_t x = (uint32_t)j;
        for (uint32_t p = parent[x]; p != x; p = parent[x]) x = p;
        parent[j] = x;
        root = x;
        id = __float_as_uint(g.pts[j].w);
    }
    // one round per distinct root among the wave's lanes: the first lane left speaks for all lanes with its root
    for (unsigned long long todo = __ballot(live); todo != 0ull;) {
        const int lead = __ffsll((long long)todo) - 1;
        const uint32_t root0 = __shfl(root, lead);
        const bool mine = live && root == root0;
        const unsigned long long group = __ballot(mine);
        uint32_t mn = mine ? id : CL_NONE;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) mn = min(mn, (uint32_t)__shfl_xor(mn, o));
        if ((int)(threadIdx.x & 63u) == lead) {
            atomicMin(rmin + root0, mn);
            atomicAdd(rsize + root0, (uint32_t)__popcll(group));
        }
        todo &= ~group;
    }
}

// head[i] = 1 for the smallest original id of every component (head is n + 1 long and zero; its exclusive scan is the rank)
template <bool ALL_CORE>
__global__ __launch_bounds__(256) void k_cluster_heads(int64_t nv, const uint8_t *__restrict__ core, const uint32_t *__restrict__ parent,
                                                        const uint32_t *__restrict__ rmin, uint32_t *__restrict__ head)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nv && (ALL_CORE || core[j]) && parent[j] == (uint32_t)j) head[rmin[j]] = 1u;
}

// the label of a core point = the rank of its component's smallest id; slab (sorted order) holds it for the border pass, -1 for
// the others; the root writes the size of its label
template <bool ALL_CORE>
__global__ __launch_bounds__(256) void k_cluster_labels(SfGrid g, const uint8_t *__restrict__ core, const uint32_t *__restrict__ parent, const uint32_t *__restrict__ rmin,
                                                         const uint32_t *__restrict__ rsize, const uint32_t *__restrict__ rank, int32_t *__restrict__ slab,
                                                         int32_t *__restrict__ labels, int32_t *__restrict__ sizes)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= g.n) return;
    int32_t l = -1;
    if (ALL_CORE || core[j]) {
        const uint32_t root = parent[j];
        l = (int32_t)rank[rmin[root]];
        labels[__float_as_uint(g.pts[j].w)] = l;
        if (root == (uint32_t)j) sizes[l] = (int32_t)rsize[j];
    }
    slab[j] = l;
}

// One lane per indexed point that is not core and has a neighbour (count > 1): the same walk over all positions; the smallest label
// among the accepted core candidates (as unsigned, -1 is the largest), if there is one.  slab is only read here.
__global__ __launch_bounds__(256) void k_cluster_border(SfGrid g, float r2, int R, const int32_t *__restrict__ counts, const int32_t *__restrict__ slab,
                                                         int32_t *__restrict__ labels, int32_t *__restrict__ sizes)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= g.n || slab[j] >= 0) return;
    const float4 p = g.pts[j];
    const uint32_t id = __float_as_uint(p.w);
    if (counts[id] <= 1) return;
    uint32_t best = CL_NONE;
    sf::radius_walk<true, false>(g, p, r2, R, 0u, slab, [&](uint32_t, int32_t l, bool hit) { if (hit) best = min(best, (uint32_t)l); });
    if (best != CL_NONE) {
        labels[id] = (int32_t)best;
        atomicAdd(sizes + best, 1);
    }
}

// the size filter: keepc[c] = 1 for a label that stays (keepc is nv + 1 long; *n_clusters lives on the device)
__global__ __launch_bounds__(256) void k_cluster_size_keep(const int32_t *__restrict__ sizes, const uint32_t *__restrict__ n_clusters, int64_t nv, int64_t min_size,
                                                            int64_t max_size, uint32_t *__restrict__ keepc)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c > nv) return;
    uint32_t keep = 0u;
    if (c < (int64_t)*n_clusters) {
        const int64_t s = sizes[c];
        keep = (s >= min_size && (max_size <= 0 || s <= max_size)) ? 1u : 0u;
    }
    keepc[c] = keep;
}

// newrank = the exclusive scan of keepc: a label stays iff newrank steps behind it
__global__ __launch_bounds__(256) void k_cluster_remap_sizes(const int32_t *__restrict__ sizes, const uint32_t *__restrict__ n_clusters, const uint32_t *__restrict__ newrank,
                                                              int32_t *__restrict__ sizes_out)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < (int64_t)*n_clusters && newrank[c + 1] != newrank[c]) sizes_out[newrank[c]] = sizes[c];
}

__global__ __launch_bounds__(256) void k_cluster_remap_labels(int32_t *__restrict__ labels, int64_t n, const uint32_t *__restrict__ newrank)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t l = labels[i];
    if (l >= 0) labels[i] = newrank[l + 1] != newrank[l] ? (int32_t)newrank[l] : -1;
}

// stat[0] += the sizes, stat[1] = max of (size << 32 | ~label): the largest cluster and, among equals, the smallest label;
// stat[2] = the number of clusters.  Integer atomics, one pair per wave.
__global__ __launch_bounds__(256) void k_cluster_stats(const int32_t *__restrict__ sizes, const uint32_t *__restrict__ n_clusters, unsigned long long *__restrict__ stat)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nc = (int64_t)*n_clusters;
    if (c == 0) stat[2] = (unsigned long long)nc;
    unsigned long long sum = 0ull, key = 0ull;
    if (c < nc) {
        sum = (unsigned long long)(uint32_t)sizes[c];
        key = (sum << 32) | (unsigned long long)(CL_NONE - (uint32_t)c);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        sum += __shfl_xor(sum, o);
        const unsigned long long other = __shfl_xor(key, o);
        key = other > key ? other : key;
    }
    if ((threadIdx.x & 63u) == 0 && key) {
        atomicAdd(stat, sum);
        atomicMax(stat + 1, key);
    }
}

// the cloud calls: flags from labels on the device.  largest: keep the one label stat[1] names, otherwise every label >= 0
__global__ __launch_bounds__(256) void k_cluster_keep_flags(const int32_t *__restrict__ labels, int64_t n, int largest, const unsigned long long *__restrict__ stat,
                                                             uint8_t *__restrict__ flags)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t l = labels[i];
    const int32_t want = (int32_t)(CL_NONE - (uint32_t)stat[1]); // (no cluster at all: stat[1] = 0, want = -1, and no label >= 0 exists)
    flags[i] = (l >= 0 && (!largest || l == want)) ? 1 : 0;
}

#define SF_CHECK_CLUSTER_DBSCAN(eps, min_points) SF_CHECK((eps) > 0 && std::isfinite(eps) && (min_points) >= 1, SF_ERR_INVALID, "cluster_dbscan: eps must be positive and finite, min_points >= 1 (got %g, %d)", (double)(eps), min_points)
#define SF_CHECK_CLUSTER_EUCLIDEAN(tol, min_size) SF_CHECK((tol) > 0 && std::isfinite(tol) && (min_size) >= 1, SF_ERR_INVALID, "cluster_euclidean: tolerance must be positive and finite, min_size >= 1 (got %g, %lld)", (double)(tol), (long long)(min_size))

// m->cl, in 4-byte words after the three 8-byte statistics: what cluster_device leaves for its callers
struct ClusterBufs {
    unsigned long long *stat; // [3]
    uint32_t *parent;         // [nv]     sorted order
    uint32_t *rmin;           // [nv + 1] per root: smallest original id; afterwards the size filter's keep flags and their scan
    uint32_t *rsize;          // [nv + 1] per root: core points; afterwards the sizes that passed the size filter
    int32_t *slab;            // [nv]     sorted order: label of a core point, -1
    uint32_t *head;           // [n + 1]  original order: 1 at a component's smallest id; scanned: the rank, [n] = the number of clusters
    int32_t *labels;          // [n]      original order
    int32_t *sizes;           // [nv + 1] per label
    uint8_t *core;            // [nv]     sorted order
    // where the results are once cluster_device has returned
    const int32_t *sizes_final;
};

int cluster_buffers(sf_map *m, ClusterBufs *b)
{
    const size_t n = (size_t)m->n, nv = (size_t)m->grid.n;
    const size_t words = 6 + nv + (nv + 1) + (nv + 1) + nv + (n + 1) + n + (nv + 1);
    SF_TRY(m->cl.reserve(sizeof(uint32_t) * words + nv));
    uint32_t *w = m->cl.as<uint32_t>();
    b->stat = reinterpret_cast<unsigned long long *>(w); w += 6;
    b->parent = w; w += nv;
    b->rmin = w; w += nv + 1;
    b->rsize = w; w += nv + 1;
    b->slab = reinterpret_cast<int32_t *>(w); w += nv;
    b->head = w; w += n + 1;
    b->labels = reinterpret_cast<int32_t *>(w); w += n;
    b->sizes = reinterpret_cast<int32_t *>(w); w += nv + 1;
    b->core = reinterpret_cast<uint8_t *>(w);
    b->sizes_final = b->sizes;
    return SF_OK;
}

// components of the core graph -> labels (and the border pass where there are points that are not core)
template <bool ALL_CORE>
int cluster_label(sf_map *m, const ClusterBufs &b, float r2, int R, const int32_t *counts)
{
    hipStream_t s = m->ctx->stream;
    const SfGrid &g = m->grid;
    const dim3 grid(nblk(g.n)), blk(256);
    hipLaunchKernelGGL(k_cluster_hook<ALL_CORE>, grid, blk, 0, s, g, r2, R, b.core, b.parent);
    hipLaunchKernelGGL(k_cluster_flatten<ALL_CORE>, grid, blk, 0, s, g, b.core, b.parent, b.rmin, b.rsize);
    hipLaunchKernelGGL(k_cluster_heads<ALL_CORE>, grid, blk, 0, s, g.n, b.core, b.parent, b.rmin, b.head);
    SF_TRY(sf::scan_u32<0>(m->ctx, b.head, b.head, m->n + 1));
    hipLaunchKernelGGL(k_cluster_labels<ALL_CORE>, grid, blk, 0, s, g, b.core, b.parent, b.rmin, b.rsize, b.head, b.slab, b.labels, b.sizes);
    if (!ALL_CORE) hipLaunchKernelGGL(k_cluster_border, grid, blk, 0, s, g, r2, R, counts, b.slab, b.labels, b.sizes);
    return SF_OK;
}

// The clustering proper, shared by the four entry points.  min_points == 1: every indexed point is core, no counts are taken and
// there is no border pass (the Euclidean form; min_size / max_size apply to it alone and are (1, 0) for DBSCAN).  Labels [n] and
// sizes stay on the device (ClusterBufs), the statistics come to the host.  Arguments are checked by the callers.
int cluster_device(sf_map *m, double eps, int min_points, int64_t min_size, int64_t max_size, ClusterBufs *b, sf_cluster_stats *st)
{
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t n = m->n, nv = m->grid.n;
    *st = sf_cluster_stats{n, nv, 0, 0, 0, 0, 0, 0};
    if (n == 0) return SF_OK;
    const bool all_core = min_points <= 1, filter = min_size > 1 || max_size > 0;
    SF_TRY(cluster_buffers(m, b));
    SF_TRY(outlier_buffers(m, sizeof(int32_t))); // (clears the kept counters)
    const float r2 = (float)(eps * eps);
    const SfGrid &g = m->grid;
    const int R = radius_reach(g, r2);
    SF_HIP(hipMemsetAsync(b->stat, 0, sizeof(unsigned long long) * 3, s));
    SF_HIP(hipMemsetAsync(b->head, 0, sizeof(uint32_t) * (size_t)(n + 1), s));
    SF_HIP(hipMemsetAsync(b->labels, 0xFF, sizeof(int32_t) * (size_t)n, s)); // -1: what is not indexed, not core and not border keeps it
    const uint32_t *n_clusters = b->head + n;
    ProfSpan span(m);
    if (nv > 0) {
        const dim3 grid(nblk(nv)), blk(256);
        int32_t *counts = m->out_val.as<int32_t>();
        uint8_t *flags = m->out_flags.as<uint8_t>();
        if (!all_core) { // count_i and the core flag: the radius filter's kernel as it is, keep iff count > min_points - 1
            SF_HIP(hipMemsetAsync(flags, 0, (size_t)n, s));
            SF_HIP(hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)n, s));
            hipLaunchKernelGGL(k_radius_count, grid, blk, 0, s, g, r2, R, min_points - 1, counts, flags, m->out_red.as<unsigned long long>());
            hipLaunchKernelGGL(k_sum_kept, dim3(1), dim3(KEPT_SLOTS), 0, s, m->out_red.as<unsigned long long>());
        }
        hipLaunchKernelGGL(k_cluster_init, grid, blk, 0, s, g, all_core ? (const uint8_t *)nullptr : flags, b->parent, b->rmin, b->rsize, b->core);
        SF_TRY(all_core ? cluster_label<true>(m, *b, r2, R, counts) : cluster_label<false>(m, *b, r2, R, counts));
        if (filter) { // rmin and rsize are free by now
            uint32_t *keepc = b->rmin;
            int32_t *sizes_out = reinterpret_cast<int32_t *>(b->rsize);
            hipLaunchKernelGGL(k_cluster_size_keep, dim3(nblk(nv + 1)), blk, 0, s, b->sizes, n_clusters, nv, min_size, max_size, keepc);
            SF_TRY(sf::scan_u32<0>(ctx, keepc, keepc, nv + 1));
            hipLaunchKernelGGL(k_cluster_remap_sizes, grid, blk, 0, s, b->sizes, n_clusters, keepc, sizes_out);
            hipLaunchKernelGGL(k_cluster_remap_labels, dim3(nblk(n)), blk, 0, s, b->labels, n, keepc);
            n_clusters = keepc + nv;
            b->sizes_final = sizes_out;
        }
        hipLaunchKernelGGL(k_cluster_stats, grid, blk, 0, s, b->sizes_final, n_clusters, b->stat);
    }
    span.end();
    SF_TRY(read_words(ctx, b->stat, 3, m->out_red.as<unsigned long long>() + (size_t)KEPT_SLOTS * KEPT_STRIDE, 1));
    prof_read(m);
    const unsigned long long *h = ctx->h_pinned->readback;
    st->n_kept = (int64_t)h[0];
    st->largest_size = (int64_t)(h[1] >> 32);
    st->n_clusters = (int64_t)h[2];
    st->n_core = all_core ? nv : (nv > 0 ? (int64_t)h[3] : 0);
    st->n_border = all_core ? 0 : st->n_kept - st->n_core;
    st->n_noise = nv - st->n_kept;
    return SF_OK;
}

int download_clusters(sf_map *m, const ClusterBufs &b, const sf_cluster_stats &st, int32_t *labels, int32_t *sizes, int64_t cap_sizes)
{
    sf_ctx *ctx = m->ctx;
    const int64_t ns = sizes ? std::min(st.n_clusters, cap_sizes) : 0;
    if (m->n == 0 || (!labels && ns <= 0)) return SF_OK;
    if (labels) SF_HIP(hipMemcpyAsync(labels, b.labels, sizeof(int32_t) * (size_t)m->n, hipMemcpyDeviceToHost, ctx->stream));
    if (ns > 0) SF_HIP(hipMemcpyAsync(sizes, b.sizes_final, sizeof(int32_t) * (size_t)ns, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    return SF_OK;
}

// filter_cloud with Euclidean clustering: the labels become keep flags on the device
int filter_cloud_clusters(sf_cloud *c, double tolerance, int64_t min_size, int64_t max_size, bool largest, float cell, sf_cluster_stats *stats)
{
    return filter_cloud(c, cell, stats, [=](sf_map *m, sf_cluster_stats *st) {
        ClusterBufs b{};
        SF_TRY(cluster_device(m, tolerance, 1, min_size, max_size, &b, st));
        hipLaunchKernelGGL(k_cluster_keep_flags, dim3(nblk(m->n)), dim3(256), 0, m->ctx->stream, b.labels, m->n, largest ? 1 : 0, b.stat, m->out_flags.as<uint8_t>());
        if (largest) { // what stays is the largest cluster alone
            st->n_kept = st->largest_size;
            st->n_noise = st->n_valid - st->n_kept;
        }
        return (int)SF_OK;
    });
}

} // namespace

extern "C" int sf_map_cluster_dbscan(sf_map *m, double eps, int min_points, int32_t *labels, int32_t *sizes, int64_t cap_sizes, sf_cluster_stats *stats)
{
    SF_CHECK(m && m->built, SF_ERR_STATE, "map not built");
    SF_CHECK_CLUSTER_DBSCAN(eps, min_points);
    SF_CHECK(!sizes || cap_sizes >= 0, SF_ERR_INVALID, "cluster_dbscan: cap_sizes must not be negative");
    sf_cluster_stats st;
    ClusterBufs b{};
    SF_TRY(cluster_device(m, eps, min_points, 1, 0, &b, &st));
    if (stats) *stats = st;
    return download_clusters(m, b, st, labels, sizes, cap_sizes);
}

extern "C" int sf_map_cluster_euclidean(sf_map *m, double tolerance, int64_t min_size, int64_t max_size, int32_t *labels, int32_t *sizes, int64_t cap_sizes,
                                        sf_cluster_stats *stats)
{
    SF_CHECK(m && m->built, SF_ERR_STATE, "map not built");
    SF_CHECK_CLUSTER_EUCLIDEAN(tolerance, min_size);
    SF_CHECK(!sizes || cap_sizes >= 0, SF_ERR_INVALID, "cluster_euclidean: cap_sizes must not be negative");
    sf_cluster_stats st;
    ClusterBufs b{};
    SF_TRY(cluster_device(m, tolerance, 1, min_size, max_size, &b, &st));
    if (stats) *stats = st;
    return download_clusters(m, b, st, labels, sizes, cap_sizes);
}

extern "C" int sf_cloud_filter_clusters(sf_cloud *c, double tolerance, int64_t min_size, int64_t max_size, float cell, sf_cluster_stats *stats)
{
    SF_CHECK(c, SF_ERR_INVALID, "bad arguments");
    SF_CHECK_CLUSTER_EUCLIDEAN(tolerance, min_size);
    return filter_cloud_clusters(c, tolerance, min_size, max_size, false, cell, stats);
}

extern "C" int sf_cloud_keep_largest_cluster(sf_cloud *c, double tolerance, float cell, sf_cluster_stats *stats)
{
    SF_CHECK(c, SF_ERR_INVALID, "bad arguments");
    SF_CHECK_CLUSTER_EUCLIDEAN(tolerance, 1);
    return filter_cloud_clusters(c, tolerance, 1, 0, true, cell, stats);
}
