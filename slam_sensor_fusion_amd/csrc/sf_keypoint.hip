// sf_keypoint.hip — Intrinsic Shape Signatures keypoints on the uniform-grid index and the gather that restricts a descriptor set
// to chosen rows (extension, no reference code; the rule is in include/slamfusion.h and DESIGN §23, restated in
// tests/iss_ref_np.py).  gfx950 only, wave64.
//
// One call: k_iss_saliency (the radius_walk of sf_walk.hpp at the salient radius, ten float64 accumulators per lane, the 3 x 3
// Jacobi solve, the salient test) -> k_iss_nms (the same walk at the non-maximum radius over what the first pass left in sorted
// order) -> an exclusive scan of the keypoint flags (sf_sort.hpp) -> k_iss_compact.  The host waits once, at the end.  Integer
// atomics serve the three counts only.
#include "sf_keypoint.hpp"
#include "sf_sort.hpp"
#include "sf_walk.hpp"

namespace {

#include "sf_jacobi.hpp"

using sf::GATHER_BLOCK;
using sf::ISS_BLOCK;
using sf::ISS_NOT_SALIENT;

constexpr int DIM = SF_FPFH_DIM;

inline unsigned nblk(int64_t n, int block) { return (unsigned)sf::div_up(n, block); }

// stats words: [0] salient points, [1] the largest count, [2] keypoints
constexpr int ISS_STAT_WORDS = 3;

// Pass 1, one lane per sorted position j.  The visitor takes the walk's `accepted` flag as data: a candidate that is not a
// neighbour (or an empty slot of a trip of four) adds zeros, so no float64 work sits under a divergent branch.  The point is
// re-read by the visitor under the flag (load_point drops the access of a lane without a candidate): the walk hands out positions.
// -> key[j] in SORTED order (lambda3 if salient, ISS_NOT_SALIENT otherwise) for pass 2; lambda [id][3], n_neighbors [id],
// salient [id] in ORIGINAL order (zeroed beforehand: points that are not indexed are not touched).
__global__ __launch_bounds__(ISS_BLOCK) void k_iss_saliency(SfGrid g, float r2, int R, int min_neighbors, double gamma_21, double gamma_32, double min_lambda3,
                                                             double *__restrict__ key, double *__restrict__ lambda, int32_t *__restrict__ n_neighbors,
                                                             uint8_t *__restrict__ salient, unsigned long long *__restrict__ stats)
{
    __shared__ int s_max;
    if (threadIdx.x == 0) s_max = 0;
    const int64_t j = (int64_t)blockIdx.x * ISS_BLOCK + threadIdx.x;
    bool is_salient = false;
    int cnt = 0;
    if (j < g.n) {
        const float4 p = g.pts[j];
        const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
        double sx = 0.0, sy = 0.0, sz = 0.0, qxx = 0.0, qxy = 0.0, qxz = 0.0, qyy = 0.0, qyz = 0.0, qzz = 0.0;
        sf::radius_walk<false, false>(g, p, r2, R, 0u, nullptr, [&](uint32_t k, int32_t, bool hit) {
            const float4 q = sf::load_point(g, k, hit);
            const double dx = hit ? (double)q.x - px : 0.0, dy = hit ? (double)q.y - py : 0.0, dz = hit ? (double)q.z - pz : 0.0;
            cnt += hit ? 1 : 0;
            sx = sx + dx; sy = sy + dy; sz = sz + dz;
            qxx = qxx + dx * dx; qxy = qxy + dx * dy; qxz = qxz + dx * dz;
            qyy = qyy + dy * dy; qyz = qyz + dy * dz; qzz = qzz + dz * dz;
        });
        double l1 = 0.0, l2 = 0.0, l3 = 0.0;
        if (cnt > 0) {
            const double n = (double)cnt;
            const double mx = sx / n, my = sy / n, mz = sz / n;
            double A[9], V[9];
            A[0] = qxx / n - mx * mx;
            A[1] = A[3] = qxy / n - mx * my;
            A[2] = A[6] = qxz / n - mx * mz;
            A[4] = qyy / n - my * my;
            A[5] = A[7] = qyz / n - my * mz;
            A[8] = qzz / n - mz * mz;
            jacobi_sym<3>(A, V);
            l1 = A[0]; l2 = A[4]; l3 = A[8];
            double t;
            if (l1 < l2) { t = l1; l1 = l2; l2 = t; }
            if (l2 < l3) { t = l2; l2 = l3; l3 = t; }
            if (l1 < l2) { t = l1; l1 = l2; l2 = t; }
            l1 = fmax(l1, 0.0); l2 = fmax(l2, 0.0); l3 = fmax(l3, 0.0);
        }
        is_salient = cnt >= min_neighbors && l2 < gamma_21 * l1 && l3 < gamma_32 * l2 && l3 > min_lambda3;
        const uint32_t id = __float_as_uint(p.w);
        key[j] = is_salient ? l3 : ISS_NOT_SALIENT;
        lambda[3 * (size_t)id] = l1; lambda[3 * (size_t)id + 1] = l2; lambda[3 * (size_t)id + 2] = l3;
        n_neighbors[id] = cnt;
        salient[id] = is_salient ? 1 : 0;
    }
    int wmax = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) wmax = max(wmax, __shfl_xor(wmax, o));
    __syncthreads();
    if ((threadIdx.x & 63u) == 0u && wmax > 0) atomicMax(&s_max, wmax);
    const int c = __syncthreads_count(is_salient ? 1 : 0);
    if (threadIdx.x == 0) {
        if (c > 0) atomicAdd(stats, (unsigned long long)c);
        if (s_max > 0) atomicMax(stats + 1, (unsigned long long)s_max);
    }
}

// Pass 2, one lane per sorted position j; only a salient point walks.  Per candidate: key (lambda3 and the salient bit in one
// word, sorted order: the candidates of a cell row are contiguous) and the original index for the tie, both read at the lane's
// own position when the candidate is no neighbour -- the point does not beat itself, so that adds nothing.  Branch-free as well.
// -> flags [id] (uint8) and live [id] (uint32, what the scan reads) in ORIGINAL order, zeroed beforehand.
__global__ __launch_bounds__(ISS_BLOCK) void k_iss_nms(SfGrid g, float r2, int R, int min_neighbors, const double *__restrict__ key, uint8_t *__restrict__ flags,
                                                        uint32_t *__restrict__ live, unsigned long long *__restrict__ stats)
{
    const int64_t j = (int64_t)blockIdx.x * ISS_BLOCK + threadIdx.x;
    bool keep = false;
    if (j < g.n) {
        const double mine = key[j];
        if (mine >= 0.0) {
            const float4 p = g.pts[j];
            const uint32_t id = __float_as_uint(p.w);
            const uint32_t *ids = reinterpret_cast<const uint32_t *>(g.pts);
            int cnt = 0, beaten = 0;
            sf::radius_walk<false, false>(g, p, r2, R, 0u, nullptr, [&](uint32_t k, int32_t, bool hit) {
                const size_t kk = hit ? (size_t)k : (size_t)j;
                const double other = key[kk];
                const uint32_t oid = ids[4 * kk + 3];
                cnt += hit ? 1 : 0;
                beaten |= (other > mine || (other == mine && oid < id)) ? 1 : 0;
            });
            keep = cnt >= min_neighbors && beaten == 0;
            flags[id] = keep ? 1 : 0;
            live[id] = keep ? 1u : 0u;
        }
    }
    const int c = __syncthreads_count(keep ? 1 : 0);
    if (threadIdx.x == 0 && c > 0) atomicAdd(stats + 2, (unsigned long long)c);
}

// the keypoints in ascending original index: slot pos[i] (the exclusive scan of live) gets i, up to cap slots
__global__ __launch_bounds__(256) void k_iss_compact(const uint32_t *__restrict__ live, const uint32_t *__restrict__ pos, int64_t n, int64_t cap,
                                                      int32_t *__restrict__ indices)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !live[i]) return;
    const uint32_t s = pos[i];
    if ((int64_t)s < cap) indices[s] = (int32_t)i;
}

// out row t / 33, word t % 33 <- the same word of src row rows[t / 33]: a row is taken by 33 consecutive lanes, reads and writes
// are runs of consecutive words.  The lane of word 0 carries the validity byte.  An index outside src: zeros, and the flag is
// raised (read by the host at the one wait of the call).  *count = the valid rows (one integer atomic per wave).
__global__ __launch_bounds__(GATHER_BLOCK) void k_features_gather(const float *__restrict__ src_rows, const uint8_t *__restrict__ src_valid, int64_t ns,
                                                                   const int32_t *__restrict__ rows, int64_t k, float *__restrict__ out_rows,
                                                                   uint8_t *__restrict__ out_valid, uint32_t *__restrict__ bad, unsigned long long *__restrict__ count)
{
    const int64_t t = (int64_t)blockIdx.x * GATHER_BLOCK + threadIdx.x;
    bool counted = false;
    if (t < k * DIM) {
        const int64_t r = t / DIM;
        const int w = (int)(t - r * DIM);
        const int64_t i = rows[r];
        const bool ok = i >= 0 && i < ns;
        out_rows[t] = ok ? src_rows[(size_t)i * DIM + w] : 0.0f;
        if (w == 0) {
            const uint8_t v = ok ? src_valid[i] : (uint8_t)0;
            out_valid[r] = v;
            counted = v != 0;
            if (!ok) atomicOr(bad, 1u);
        }
    }
    const unsigned long long b = __ballot(counted);
    if ((threadIdx.x & 63u) == 0u && b) atomicAdd(count, (unsigned long long)__popcll(b));
}

// device events around the two passes, created only when a call is profiled
struct Events {
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    bool on = false;
    Events() = default;
    Events(const Events &) = delete;
    Events &operator=(const Events &) = delete;
    ~Events()
    {
        for (hipEvent_t e : ev)
            if (e) { hipError_t rc = hipEventDestroy(e); (void)rc; }
    }
    int start(bool profile)
    {
        on = profile;
        if (on)
            for (hipEvent_t &e : ev) SF_HIP(hipEventCreate(&e));
        return SF_OK;
    }
    int mark(int k, hipStream_t s)
    {
        if (on) SF_HIP(hipEventRecord(ev[k], s));
        return SF_OK;
    }
    int ms(int a, int b, float *out) // after the stream was synchronised
    {
        *out = -1.0f;
        if (on) SF_HIP(hipEventElapsedTime(out, ev[a], ev[b]));
        return SF_OK;
    }
};

int check_iss_params(const sf_iss_params *p)
{
    SF_CHECK(p, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(std::isfinite(p->salient_radius) && p->salient_radius > 0.0, SF_ERR_INVALID, "iss: the salient radius must be positive and finite (got %g)", p->salient_radius);
    SF_CHECK(std::isfinite(p->non_max_radius) && p->non_max_radius > 0.0, SF_ERR_INVALID, "iss: the non-maximum radius must be positive and finite (got %g)", p->non_max_radius);
    SF_CHECK(p->gamma_21 > 0.0 && p->gamma_21 <= 1.0 && p->gamma_32 > 0.0 && p->gamma_32 <= 1.0, SF_ERR_INVALID, "iss: gamma_21 and gamma_32 must be in (0, 1] (got %g, %g)",
             p->gamma_21, p->gamma_32);
    SF_CHECK(p->min_lambda3 >= 0.0, SF_ERR_INVALID, "iss: min_lambda3 must not be negative (got %g)", p->min_lambda3);
    SF_CHECK(p->min_neighbors >= 1, SF_ERR_INVALID, "iss: min_neighbors must be >= 1 (got %d)", (int)p->min_neighbors);
    return SF_OK;
}

int check_iss_outputs(const int32_t *indices, int64_t cap)
{
    SF_CHECK(cap >= 0, SF_ERR_INVALID, "iss: cap must not be negative (got %lld)", (long long)cap);
    SF_CHECK(indices || cap == 0, SF_ERR_INVALID, "iss: indices is NULL with cap > 0");
    return SF_OK;
}

// the call's own scratch: pass 1's outputs in original order, its key in sorted order, pass 2's flags and their scan
struct IssBufs {
    sf::DevBuf key, lambda, count, salient, flags, live, pos, indices, stats;
};

// pass 1 on the map's index (n > 0); the outputs of points that are not indexed stay zero
int saliency_enqueue(sf_map *m, const sf_iss_params *p, IssBufs &B)
{
    sf_ctx *ctx = m->ctx;
    hipStream_t s = ctx->stream;
    const int64_t n = m->n, nv = m->grid.n;
    SF_TRY(B.key.reserve(sizeof(double) * (size_t)std::max<int64_t>(nv, 1)));
    SF_TRY(B.lambda.reserve(sizeof(double) * 3 * (size_t)n));
    SF_TRY(B.count.reserve(sizeof(int32_t) * (size_t)n));
    SF_TRY(B.salient.reserve((size_t)n));
    SF_TRY(B.stats.reserve(sizeof(unsigned long long) * ISS_STAT_WORDS));
    SF_HIP(hipMemsetAsync(B.lambda.p, 0, sizeof(double) * 3 * (size_t)n, s));
    SF_HIP(hipMemsetAsync(B.count.p, 0, sizeof(int32_t) * (size_t)n, s));
    SF_HIP(hipMemsetAsync(B.salient.p, 0, (size_t)n, s));
    SF_HIP(hipMemsetAsync(B.stats.p, 0, sizeof(unsigned long long) * ISS_STAT_WORDS, s));
    if (nv == 0) return SF_OK;
    const float r2 = (float)(p->salient_radius * p->salient_radius);
    hipLaunchKernelGGL(k_iss_saliency, dim3(nblk(nv, ISS_BLOCK)), dim3(ISS_BLOCK), 0, s, m->grid, r2, sf::feature_reach(m->grid, r2), (int)p->min_neighbors, p->gamma_21,
                       p->gamma_32, p->min_lambda3, B.key.as<double>(), B.lambda.as<double>(), B.count.as<int32_t>(), B.salient.as<uint8_t>(),
                       B.stats.as<unsigned long long>());
    SF_HIP(hipGetLastError());
    return SF_OK;
}

// The device code of sf_map_iss_keypoints, shared with the cloud form; arguments are checked by the callers.  The outputs are
// written only after the one wait.
int keypoints_device(sf_map *m, const sf_iss_params *p, int32_t *indices, int64_t cap, int64_t *n_keypoints, uint8_t *flags, sf_iss_stats *stats)
{
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t n = m->n, nv = m->grid.n;
    sf_iss_stats st{n, nv, 0, 0, 0, -1.0f, -1.0f};
    if (n == 0 || nv == 0) {
        if (flags && n > 0) std::memset(flags, 0, (size_t)n);
        if (n_keypoints) *n_keypoints = 0;
        if (stats) *stats = st;
        return SF_OK;
    }
    const int64_t slots = std::min(cap, n);
    IssBufs B;
    Events ev;
    SF_TRY(B.flags.reserve((size_t)n));
    SF_TRY(B.live.reserve(sizeof(uint32_t) * (size_t)n));
    SF_TRY(B.pos.reserve(sizeof(uint32_t) * (size_t)n));
    SF_TRY(B.indices.reserve(sizeof(int32_t) * (size_t)std::max<int64_t>(slots, 1)));
    SF_TRY(ev.start(p->profile != 0));
    SF_TRY(ev.mark(0, s));
    SF_TRY(saliency_enqueue(m, p, B));
    SF_TRY(ev.mark(1, s));
    SF_HIP(hipMemsetAsync(B.flags.p, 0, (size_t)n, s));
    SF_HIP(hipMemsetAsync(B.live.p, 0, sizeof(uint32_t) * (size_t)n, s));
    const float r2 = (float)(p->non_max_radius * p->non_max_radius);
    hipLaunchKernelGGL(k_iss_nms, dim3(nblk(nv, ISS_BLOCK)), dim3(ISS_BLOCK), 0, s, m->grid, r2, sf::feature_reach(m->grid, r2), (int)p->min_neighbors,
                       B.key.as<double>(), B.flags.as<uint8_t>(), B.live.as<uint32_t>(), B.stats.as<unsigned long long>());
    SF_HIP(hipGetLastError());
    SF_TRY(ev.mark(2, s));
    std::vector<int32_t> h_idx((size_t)slots);
    std::vector<uint8_t> h_flags(flags ? (size_t)n : 0);
    if (slots > 0) {
        SF_TRY(sf::scan_u32<0>(ctx, B.live.as<uint32_t>(), B.pos.as<uint32_t>(), n));
        hipLaunchKernelGGL(k_iss_compact, dim3(nblk(n, 256)), dim3(256), 0, s, B.live.as<uint32_t>(), B.pos.as<uint32_t>(), n, slots, B.indices.as<int32_t>());
        SF_HIP(hipGetLastError());
        SF_HIP(hipMemcpyAsync(h_idx.data(), B.indices.p, sizeof(int32_t) * (size_t)slots, hipMemcpyDeviceToHost, s));
    }
    if (flags) SF_HIP(hipMemcpyAsync(h_flags.data(), B.flags.p, (size_t)n, hipMemcpyDeviceToHost, s));
    unsigned long long h[ISS_STAT_WORDS] = {0, 0, 0};
    SF_HIP(hipMemcpyAsync(h, B.stats.p, sizeof(h), hipMemcpyDeviceToHost, s));
    SF_HIP(hipStreamSynchronize(s));
    st.n_salient = (int64_t)h[0];
    st.max_neighbors = (int64_t)h[1];
    st.n_keypoints = (int64_t)h[2];
    SF_TRY(ev.ms(0, 1, &st.saliency_ms));
    SF_TRY(ev.ms(1, 2, &st.nms_ms));
    const int64_t take = std::min(slots, st.n_keypoints); // only the slots that hold a keypoint were written
    if (take > 0) std::memcpy(indices, h_idx.data(), sizeof(int32_t) * (size_t)take);
    if (flags) std::memcpy(flags, h_flags.data(), (size_t)n);
    if (n_keypoints) *n_keypoints = st.n_keypoints;
    if (stats) *stats = st;
    return SF_OK;
}

} // namespace

extern "C" void sf_iss_default_params(sf_iss_params *p)
{
    if (!p) return;
    *p = sf_iss_params{0.0, 0.0, 0.975, 0.975, 0.0, 5, 0};
}

extern "C" int sf_map_iss_saliency(sf_map *m, const sf_iss_params *p, double *lambda, int32_t *n_neighbors, uint8_t *salient)
{
    SF_CHECK(m, SF_ERR_INVALID, "bad arguments");
    SF_TRY(check_iss_params(p));
    SF_CHECK(m->built, SF_ERR_STATE, "map not built");
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t n = m->n;
    if (n == 0) return SF_OK;
    IssBufs B;
    SF_TRY(saliency_enqueue(m, p, B));
    if (lambda) SF_HIP(hipMemcpyAsync(lambda, B.lambda.p, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost, s));
    if (n_neighbors) SF_HIP(hipMemcpyAsync(n_neighbors, B.count.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    if (salient) SF_HIP(hipMemcpyAsync(salient, B.salient.p, (size_t)n, hipMemcpyDeviceToHost, s));
    SF_HIP(hipStreamSynchronize(s));
    return SF_OK;
}

extern "C" int sf_map_iss_keypoints(sf_map *m, const sf_iss_params *p, int32_t *indices, int64_t cap, int64_t *n_keypoints, uint8_t *flags, sf_iss_stats *stats)
{
    SF_CHECK(m, SF_ERR_INVALID, "bad arguments");
    SF_TRY(check_iss_params(p));
    SF_TRY(check_iss_outputs(indices, cap));
    SF_CHECK(m->built, SF_ERR_STATE, "map not built");
    return keypoints_device(m, p, indices, cap, n_keypoints, flags, stats);
}

extern "C" int sf_cloud_iss_keypoints(sf_cloud *c, const sf_iss_params *p, float cell, int32_t *indices, int64_t cap, int64_t *n_keypoints, sf_iss_stats *stats)
{
    SF_CHECK(c, SF_ERR_INVALID, "bad arguments");
    SF_TRY(check_iss_params(p));
    SF_TRY(check_iss_outputs(indices, cap));
    if (c->n == 0) {
        if (n_keypoints) *n_keypoints = 0;
        if (stats) *stats = sf_iss_stats{0, 0, 0, 0, 0, -1.0f, -1.0f};
        return SF_OK;
    }
    sf_map *tmp = nullptr;
    SF_TRY(sf_map_create(c->ctx, &tmp));
    int rc = sf_map_build(tmp, c, cell);
    if (rc == SF_OK) rc = keypoints_device(tmp, p, indices, cap, n_keypoints, nullptr, stats);
    sf_map_destroy(tmp);
    return rc;
}

extern "C" int sf_features_gather(sf_features *src, const int32_t *rows, int64_t k, sf_features *out)
{
    SF_CHECK(src && out, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(src != out, SF_ERR_INVALID, "gather: out must not be the source set");
    SF_CHECK(src->ctx == out->ctx, SF_ERR_INVALID, "the two feature sets belong to different contexts");
    SF_CHECK(k >= 0 && k < (int64_t)1 << 31, SF_ERR_INVALID, "gather: k must be 0 .. 2^31 - 1 (got %lld)", (long long)k);
    SF_CHECK(rows || k == 0, SF_ERR_INVALID, "bad arguments");
    if (k == 0) {
        out->n = 0;
        out->n_valid = 0;
        return SF_OK;
    }
    sf_ctx *ctx = src->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // gathered beside `out` and exchanged with it after the wait: a refused call leaves out as it was
    sf::DevBuf g_rows, g_valid, d_rows, word;
    SF_TRY(g_rows.reserve(sizeof(float) * DIM * (size_t)k));
    SF_TRY(g_valid.reserve((size_t)k));
    SF_TRY(d_rows.reserve(sizeof(int32_t) * (size_t)k));
    SF_TRY(word.reserve(sizeof(unsigned long long) * 2)); // [0] the valid rows, [1] (low word) an index out of range
    unsigned long long *d_count = word.as<unsigned long long>();
    SF_HIP(hipMemsetAsync(word.p, 0, sizeof(unsigned long long) * 2, s));
    SF_TRY(sf::upload_staged(ctx, d_rows.p, rows, sizeof(int32_t) * (size_t)k));
    hipLaunchKernelGGL(k_features_gather, dim3(nblk(k * DIM, GATHER_BLOCK)), dim3(GATHER_BLOCK), 0, s, src->rows.as<float>(), src->valid.as<uint8_t>(), src->n,
                       d_rows.as<int32_t>(), k, g_rows.as<float>(), g_valid.as<uint8_t>(), reinterpret_cast<uint32_t *>(d_count + 1), d_count);
    SF_HIP(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    SF_HIP(hipMemcpyAsync(h, word.p, sizeof(h), hipMemcpyDeviceToHost, s));
    SF_HIP(hipStreamSynchronize(s));
    SF_CHECK(h[1] == 0, SF_ERR_INVALID, "gather: a row index lies outside the source set");
    out->rows.swap(g_rows);
    out->valid.swap(g_valid);
    out->n = k;
    out->n_valid = (int64_t)h[0];
    return SF_OK;
}
