// sf_feature.hip — FPFH descriptors on the uniform-grid index and brute-force descriptor matching (extension, no reference code;
// the rule is in include/slamfusion.h and DESIGN §21, restated in tests/fpfh_ref_np.py).  gfx950 only, wave64.
#include "sf_feature.hpp"
#include "sf_walk.hpp"

namespace {

using sf::FPFH_BINS;
using sf::FPFH_BLOCK;
using sf::MATCH_BLOCK;
using sf::MATCH_TILE;

constexpr int DIM = SF_FPFH_DIM;
static_assert(DIM == 3 * FPFH_BINS, "a row is three groups of bins");

inline unsigned nblk(int64_t n, int block) { return (unsigned)sf::div_up(n, block); }

struct Normal { double x, y, z; bool ok; };

// the stored normal of sorted position k in float64, oriented as it is loaded; ok = false: the point has no normal
__device__ __forceinline__ Normal load_normal(const SfGrid &g, uint32_t k, const float4 &p, int orient, double tx, double ty, double tz)
{
    const float4 f = g.nrm[k];
    Normal n{(double)f.x, (double)f.y, (double)f.z, false};
    n.ok = isfinite(f.x) && isfinite(f.y) && isfinite(f.z) && !(f.x == 0.0f && f.y == 0.0f && f.z == 0.0f);
    if (orient != SF_ORIENT_NONE) {
        double ax = tx, ay = ty, az = tz;
        if (orient == SF_ORIENT_VIEWPOINT) { ax = tx - (double)p.x; ay = ty - (double)p.y; az = tz - (double)p.z; }
        const double s = n.x * ax + n.y * ay + n.z * az;
        if (s < 0.0) { n.x = -n.x; n.y = -n.y; n.z = -n.z; }
    }
    return n;
}

__device__ __forceinline__ int fpfh_bin(double x) { return (int)fmin(fmax(floor(x), 0.0), (double)(FPFH_BINS - 1)); }

// the pair feature of (i, j) seen from i -> its three bins; false: the pair is skipped (L == 0 or |v| == 0)
__device__ __forceinline__ bool pair_bins(const float4 &pi, const Normal &ni, const float4 &pj, const Normal &nj, int &b_theta, int &b_alpha, int &b_phi)
{
    double dx = (double)pj.x - (double)pi.x, dy = (double)pj.y - (double)pi.y, dz = (double)pj.z - (double)pi.z;
    const double L = sqrt(dx * dx + dy * dy + dz * dz);
    if (L == 0.0) return false;
    const double ai = (ni.x * dx + ni.y * dy + ni.z * dz) / L, aj = (nj.x * dx + nj.y * dy + nj.z * dz) / L;
    const bool swap = fabs(ai) < fabs(aj);
    const double sx = swap ? nj.x : ni.x, sy = swap ? nj.y : ni.y, sz = swap ? nj.z : ni.z;
    const double ux = swap ? ni.x : nj.x, uy = swap ? ni.y : nj.y, uz = swap ? ni.z : nj.z;
    const double phi = swap ? -aj : ai;
    if (swap) { dx = -dx; dy = -dy; dz = -dz; }
    double vx = dy * sz - dz * sy, vy = dz * sx - dx * sz, vz = dx * sy - dy * sx;
    const double vn = sqrt(vx * vx + vy * vy + vz * vz);
    if (vn == 0.0) return false;
    vx = vx / vn; vy = vy / vn; vz = vz / vn;
    const double wx = sy * vz - sz * vy, wy = sz * vx - sx * vz, wz = sx * vy - sy * vx;
    const double alpha = vx * ux + vy * uy + vz * uz;
    const double theta = atan2(wx * ux + wy * uy + wz * uz, sx * ux + sy * uy + sz * uz);
    const double pi_ = 3.14159265358979323846;
    b_theta = fpfh_bin(11.0 * (theta + pi_) / (2.0 * pi_));
    b_alpha = fpfh_bin(11.0 * (alpha + 1.0) / 2.0);
    b_phi = fpfh_bin(11.0 * (phi + 1.0) / 2.0);
    return true;
}

// Pass 1, one lane per sorted position j: cnt[j][33] and P_j over the radius_walk of sf_walk.hpp (scale_j = 100 / P_j, 0: no
// SPFH).  The 33 counters of a lane live in LDS at a stride of 33 words: the stride is odd, so the bins that the lanes of a wave
// pick at run time fall into different banks unless they are the same word's, and no register array is indexed dynamically.
// The block's counters are the block's rows of cnt in memory order: they leave in one coalesced copy.
// stats: [0] points with an SPFH, [1] sum of P, [2] max P (integer atomics, one per block and word).
__global__ __launch_bounds__(FPFH_BLOCK) void k_spfh(SfGrid g, float r2, int R, int orient, double tx, double ty, double tz, uint32_t *__restrict__ cnt,
                                                      int32_t *__restrict__ n_pairs, double *__restrict__ scale, unsigned long long *__restrict__ stats)
{
    __shared__ uint32_t s_cnt[FPFH_BLOCK * DIM];
    __shared__ unsigned long long s_stat[3];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * FPFH_BLOCK, j = base + tid;
    uint32_t *mine = s_cnt + tid * DIM;
    for (int b = 0; b < DIM; ++b) mine[b] = 0u;
    if (tid < 3) s_stat[tid] = 0ull;
    __syncthreads();
    int P = 0;
    if (j < g.n) {
        const float4 p = g.pts[j];
        const Normal ni = load_normal(g, (uint32_t)j, p, orient, tx, ty, tz);
        if (ni.ok)
            sf::radius_walk<false, false>(g, p, r2, R, 0u, nullptr, [&](uint32_t k, int32_t, bool hit) {
                if (hit && k != (uint32_t)j) {
                    const float4 q = g.pts[k];
                    const Normal nj = load_normal(g, k, q, orient, tx, ty, tz);
                    int bt, ba, bp;
                    if (nj.ok && pair_bins(p, ni, q, nj, bt, ba, bp)) {
                        mine[bt] += 1u;
                        mine[FPFH_BINS + ba] += 1u;
                        mine[2 * FPFH_BINS + bp] += 1u;
                        P += 1;
                    }
                }
            });
        n_pairs[j] = P;
        scale[j] = P > 0 ? 100.0 / (double)P : 0.0;
    }
    if (P > 0) {
        atomicAdd(&s_stat[0], 1ull);
        atomicAdd(&s_stat[1], (unsigned long long)P);
        atomicMax(&s_stat[2], (unsigned long long)P);
    }
    __syncthreads();
    const int64_t rows = min((int64_t)FPFH_BLOCK, g.n - base);
    for (int t = tid; t < (int)rows * DIM; t += FPFH_BLOCK) cnt[(size_t)base * DIM + t] = s_cnt[t];
    if (tid < 2 && s_stat[tid] != 0ull) atomicAdd(&stats[tid], s_stat[tid]);
    if (tid == 2 && s_stat[2] != 0ull) atomicMax(&stats[2], s_stat[2]);
}

// Pass 2, one lane per sorted position j with an SPFH: the weighted sum of its neighbours' SPFH rows (a gather of 132-byte rows
// that pass 1 left in sorted order, so the rows of one cell are neighbours in memory), normalised per group, plus its own ->
// rows[id][33] and valid[id] in ORIGINAL order (both zeroed beforehand: points without a descriptor are not touched).
__global__ __launch_bounds__(FPFH_BLOCK) void k_fpfh(SfGrid g, float r2, int R, const uint32_t *__restrict__ cnt, const double *__restrict__ scale,
                                                      float *__restrict__ rows, uint8_t *__restrict__ valid)
{
    const int64_t j = (int64_t)blockIdx.x * FPFH_BLOCK + threadIdx.x;
    if (j >= g.n) return;
    const double sc = scale[j];
    if (!(sc > 0.0)) return;
    const float4 p = g.pts[j];
    double W[DIM];
#pragma unroll
    for (int b = 0; b < DIM; ++b) W[b] = 0.0;
    sf::radius_walk<false, false>(g, p, r2, R, 0u, nullptr, [&](uint32_t k, int32_t, bool hit) {
        if (hit && k != (uint32_t)j) {
            const double sk = scale[k];
            const float4 q = g.pts[k];
            const float d2 = sf::l2_simple(p.x, p.y, p.z, q.x, q.y, q.z); // the walk's own expression: the same bits
            if (sk > 0.0 && d2 > 0.0f) {
                const double dd = (double)d2;
                const uint32_t *row = cnt + (size_t)k * DIM;
#pragma unroll
                for (int b = 0; b < DIM; ++b) W[b] = W[b] + ((double)row[b] * sk) / dd;
            }
        }
    });
    const uint32_t id = __float_as_uint(p.w);
    const uint32_t *own = cnt + (size_t)j * DIM;
    float *out = rows + (size_t)id * DIM;
#pragma unroll
    for (int g0 = 0; g0 < DIM; g0 += FPFH_BINS) {
        double S = 0.0;
#pragma unroll
        for (int b = 0; b < FPFH_BINS; ++b) S = S + W[g0 + b];
        const double f = S > 0.0 ? 100.0 / S : 0.0;
#pragma unroll
        for (int b = 0; b < FPFH_BINS; ++b) out[g0 + b] = (float)((S > 0.0 ? W[g0 + b] * f : 0.0) + (double)own[g0 + b] * sc);
    }
    valid[id] = 1;
}

// sf_map_compute_spfh: cnt and P from sorted to ORIGINAL order (the outputs are zeroed beforehand)
__global__ __launch_bounds__(256) void k_spfh_to_host_order(SfGrid g, const uint32_t *__restrict__ cnt, const int32_t *__restrict__ n_pairs,
                                                             uint32_t *__restrict__ out_cnt, int32_t *__restrict__ out_pairs)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= g.n) return;
    const uint32_t id = __float_as_uint(g.pts[j].w);
    for (int b = 0; b < DIM; ++b) out_cnt[(size_t)id * DIM + b] = cnt[(size_t)j * DIM + b];
    out_pairs[id] = n_pairs[j];
}

// valid[i] = (the flag offered, 1 without flags) and every value of the row finite; *count = the valid rows
__global__ __launch_bounds__(256) void k_validate_rows(const float *__restrict__ rows, int64_t n, int have_flags, uint8_t *__restrict__ valid,
                                                        unsigned long long *__restrict__ count)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = false;
    if (i < n) {
        ok = have_flags ? valid[i] != 0 : true;
        for (int k = 0; k < DIM; ++k) ok = ok && isfinite(rows[(size_t)i * DIM + k]);
        valid[i] = ok ? 1 : 0;
    }
    const int c = __syncthreads_count(ok ? 1 : 0);
    if (threadIdx.x == 0 && c > 0) atomicAdd(count, (unsigned long long)c);
}

// Brute-force matching, one query row per lane in registers, the candidates of slice blockIdx.y staged through LDS a tile at a
// time: every lane reads the same candidate row, a broadcast without bank conflicts.  D is float32, unfused, ascending k (the
// flags of the build keep a - b, t * t and acc + t apart).  Candidates come in ascending index, so a strict < keeps the smallest
// index among equal distances.  -> the slice's (best, index, runner-up) record per query, [slice][nq].
// The plainest form on purpose.  Four others were measured on 51 775 x 1 661 108 rows (this one: 161 to 166 ms): two candidate
// rows interleaved in LDS against one query and two queries per lane against one candidate word, both compiling to 99
// v_pk_add_f32 / v_pk_mul_f32 for two pairs (166 and 159 ms); this kernel built without the SLP vectoriser, i.e. without the dozen
// packed instructions the compiler forms by itself (161 ms); and two queries per lane in plain instructions (150 ms).  None is
// worth its text; what holds all of them at 1.4 to 1.5 times the unfused VALU floor was not found.
__global__ __launch_bounds__(MATCH_BLOCK) void k_match(const float *__restrict__ q_rows, const uint8_t *__restrict__ q_valid, int64_t nq,
                                                        const float *__restrict__ c_rows, const uint8_t *__restrict__ c_valid, int64_t nc, int64_t slice_rows,
                                                        float *__restrict__ p_best, int32_t *__restrict__ p_idx, float *__restrict__ p_second)
{
    __shared__ float s_rows[MATCH_TILE * DIM];
    __shared__ uint8_t s_ok[MATCH_TILE];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * MATCH_BLOCK + tid;
    const int64_t c0 = (int64_t)blockIdx.y * slice_rows, c1 = min(nc, c0 + slice_rows);
    const bool live = i < nq && q_valid[i] != 0;
    float a[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) a[k] = live ? q_rows[(size_t)i * DIM + k] : 0.0f;
    float best = INFINITY, second = INFINITY;
    int32_t idx = -1;
    for (int64_t t0 = c0; t0 < c1; t0 += MATCH_TILE) {
        const int rows = (int)min((int64_t)MATCH_TILE, c1 - t0);
        __syncthreads();
        for (int t = tid; t < rows * DIM; t += MATCH_BLOCK) s_rows[t] = c_rows[(size_t)t0 * DIM + t];
        if (tid < rows) s_ok[tid] = c_valid[t0 + tid];
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            if (s_ok[r] == 0) continue; // the same for every lane
            const float *b = s_rows + r * DIM;
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < DIM; ++k) {
                float t = a[k] - b[k];
                t = t * t;
                acc = acc + t;
            }
            if (idx < 0 || acc < best) {
                second = best;
                best = acc;
                idx = (int32_t)(t0 + r);
            } else if (acc < second)
                second = acc;
        }
    }
    if (i < nq) {
        const size_t o = (size_t)blockIdx.y * (size_t)nq + (size_t)i;
        p_best[o] = live ? best : INFINITY;
        p_idx[o] = live ? idx : -1;
        p_second[o] = live ? second : INFINITY;
    }
}

// the slices' records of one query, merged in ascending slice (hence ascending index) order
__global__ __launch_bounds__(256) void k_match_merge(const float *__restrict__ p_best, const int32_t *__restrict__ p_idx, const float *__restrict__ p_second,
                                                      int64_t nq, int n_slices, int32_t *__restrict__ idx, float *__restrict__ dist2, float *__restrict__ second2)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    float best = INFINITY, second = INFINITY;
    int32_t bi = -1;
    for (int s = 0; s < n_slices; ++s) {
        const size_t o = (size_t)s * (size_t)nq + (size_t)i;
        const float b2 = p_best[o], s2 = p_second[o];
        const int32_t i2 = p_idx[o];
        if (i2 < 0) continue;
        if (bi < 0 || b2 < best) {
            second = fminf(best, s2);
            best = b2;
            bi = i2;
        } else
            second = fminf(second, b2);
    }
    idx[i] = bi;
    dist2[i] = best;
    if (second2) second2[i] = second;
}

// accepted[i] per the acceptance rule; *count = their number
__global__ __launch_bounds__(256) void k_match_accept(const int32_t *__restrict__ idx, const float *__restrict__ dist2, const float *__restrict__ second2, int64_t nq,
                                                       int use_ratio, float rr, const int32_t *__restrict__ back, uint8_t *__restrict__ accepted,
                                                       unsigned long long *__restrict__ count)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = false;
    if (i < nq) {
        const int32_t t = idx[i];
        ok = t >= 0;
        if (ok && use_ratio) ok = dist2[i] < rr * second2[i];
        if (ok && back) ok = (int64_t)back[t] == i;
        accepted[i] = ok ? 1 : 0;
    }
    const int c = __syncthreads_count(ok ? 1 : 0);
    if (threadIdx.x == 0 && c > 0) atomicAdd(count, (unsigned long long)c);
}

// device events around a pass, created only when a call is profiled
struct Events {
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    bool on = false;
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

int check_fpfh_params(const sf_fpfh_params *p)
{
    SF_CHECK(p, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(std::isfinite(p->radius) && p->radius > 0.0, SF_ERR_INVALID, "fpfh: the radius must be positive and finite (got %g)", p->radius);
    SF_CHECK(p->orient == SF_ORIENT_NONE || p->orient == SF_ORIENT_DIRECTION || p->orient == SF_ORIENT_VIEWPOINT, SF_ERR_INVALID,
             "fpfh: orient must be SF_ORIENT_NONE, _DIRECTION or _VIEWPOINT (got %d)", p->orient);
    SF_CHECK(std::isfinite(p->toward[0]) && std::isfinite(p->toward[1]) && std::isfinite(p->toward[2]), SF_ERR_INVALID, "fpfh: toward must be finite");
    return SF_OK;
}

// scratch of the two passes, in sorted order
struct SpfhBufs {
    sf::DevBuf cnt, pairs, scale, stats; // uint32[nv][33], int32[nv], double[nv], unsigned long long[3]
};

// pass 1 on the map's index (nv > 0); stats zeroed first
int spfh_enqueue(sf_map *m, const sf_fpfh_params *p, SpfhBufs &B, float r2, int R)
{
    sf_ctx *ctx = m->ctx;
    const int64_t nv = m->grid.n;
    SF_TRY(B.cnt.reserve(sizeof(uint32_t) * DIM * (size_t)nv));
    SF_TRY(B.pairs.reserve(sizeof(int32_t) * (size_t)nv));
    SF_TRY(B.scale.reserve(sizeof(double) * (size_t)nv));
    SF_TRY(B.stats.reserve(sizeof(unsigned long long) * 3));
    SF_HIP(hipMemsetAsync(B.stats.p, 0, sizeof(unsigned long long) * 3, ctx->stream));
    hipLaunchKernelGGL(k_spfh, dim3(nblk(nv, FPFH_BLOCK)), dim3(FPFH_BLOCK), 0, ctx->stream, m->grid, r2, R, p->orient, p->toward[0], p->toward[1], p->toward[2],
                       B.cnt.as<uint32_t>(), B.pairs.as<int32_t>(), B.scale.as<double>(), B.stats.as<unsigned long long>());
    SF_HIP(hipGetLastError());
    return SF_OK;
}

// the device code of sf_map_compute_fpfh, shared with the cloud form; arguments are checked by the callers
int fpfh_device(sf_map *m, const sf_fpfh_params *p, sf_features *out, sf_fpfh_stats *st)
{
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t n = m->n, nv = m->grid.n;
    *st = sf_fpfh_stats{n, nv, 0, 0, 0, -1.0f, -1.0f};
    out->n = n;
    out->n_valid = 0;
    if (n == 0) return SF_OK;
    SF_TRY(out->rows.reserve(sizeof(float) * DIM * (size_t)n));
    SF_TRY(out->valid.reserve((size_t)n));
    SF_HIP(hipMemsetAsync(out->rows.p, 0, sizeof(float) * DIM * (size_t)n, s));
    SF_HIP(hipMemsetAsync(out->valid.p, 0, (size_t)n, s));
    if (nv == 0) {
        SF_HIP(hipStreamSynchronize(s));
        return SF_OK;
    }
    const float r2 = (float)(p->radius * p->radius);
    const int R = sf::feature_reach(m->grid, r2);
    SpfhBufs B;
    Events ev;
    SF_TRY(ev.start(p->profile != 0));
    SF_TRY(ev.mark(0, s));
    SF_TRY(spfh_enqueue(m, p, B, r2, R));
    SF_TRY(ev.mark(1, s));
    hipLaunchKernelGGL(k_fpfh, dim3(nblk(nv, FPFH_BLOCK)), dim3(FPFH_BLOCK), 0, s, m->grid, r2, R, B.cnt.as<uint32_t>(), B.scale.as<double>(), out->rows.as<float>(),
                       out->valid.as<uint8_t>());
    SF_HIP(hipGetLastError());
    SF_TRY(ev.mark(2, s));
    unsigned long long h[3] = {0, 0, 0};
    SF_HIP(hipMemcpyAsync(h, B.stats.p, sizeof(h), hipMemcpyDeviceToHost, s));
    SF_HIP(hipStreamSynchronize(s));
    st->n_featured = (int64_t)h[0];
    st->n_pairs = (int64_t)h[1];
    st->max_pairs = (int64_t)h[2];
    SF_TRY(ev.ms(0, 1, &st->spfh_ms));
    SF_TRY(ev.ms(1, 2, &st->fpfh_ms));
    out->n_valid = st->n_featured;
    return SF_OK;
}

inline int match_slices(int64_t nc) { return (int)std::max<int64_t>(sf::div_up(nc, sf::match_slice_rows(nc)), 1); }
// bytes of the slices' records of nq queries against nc candidates
inline size_t match_part_bytes(int64_t nq, int64_t nc) { return (size_t)match_slices(nc) * (size_t)nq * (sizeof(float) * 2 + sizeof(int32_t)); }

// queries q against candidates c -> d_idx, d_dist2, d_second2 (may be nullptr) on the device; part (match_part_bytes, reserved by
// the caller before the first launch: growing it between two launches would free what the first still reads) holds the records
int match_enqueue(sf_ctx *ctx, const sf_features *q, const sf_features *c, sf::DevBuf &part, int32_t *d_idx, float *d_dist2, float *d_second2)
{
    const int64_t nq = q->n, nc = c->n;
    if (nq == 0) return SF_OK;
    const int64_t slice_rows = sf::match_slice_rows(nc);
    const int n_slices = match_slices(nc);
    const size_t per = (size_t)n_slices * (size_t)nq;
    float *p_best = part.as<float>(), *p_second = p_best + per;
    int32_t *p_idx = reinterpret_cast<int32_t *>(p_second + per);
    hipLaunchKernelGGL(k_match, dim3(nblk(nq, MATCH_BLOCK), (unsigned)n_slices), dim3(MATCH_BLOCK), 0, ctx->stream, q->rows.as<float>(), q->valid.as<uint8_t>(), nq,
                       c->rows.as<float>(), c->valid.as<uint8_t>(), nc, slice_rows, p_best, p_idx, p_second);
    SF_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_match_merge, dim3(nblk(nq, 256)), dim3(256), 0, ctx->stream, p_best, p_idx, p_second, nq, n_slices, d_idx, d_dist2, d_second2);
    SF_HIP(hipGetLastError());
    return SF_OK;
}

} // namespace

extern "C" int sf_features_create(sf_ctx *ctx, sf_features **out)
{
    SF_CHECK(ctx && out, SF_ERR_INVALID, "bad arguments");
    sf_features *f = new (std::nothrow) sf_features();
    SF_CHECK(f, SF_ERR_NOMEM, "out of host memory");
    f->ctx = ctx;
    sf::ctx_retain(ctx);
    *out = f;
    return SF_OK;
}

extern "C" void sf_features_destroy(sf_features *f)
{
    if (!f) return;
    hipError_t e = hipStreamSynchronize(f->ctx->stream);
    (void)e;
    f->rows.release();
    f->valid.release();
    sf_ctx *ctx = f->ctx;
    delete f;
    sf::ctx_release(ctx);
}

extern "C" int sf_features_size(const sf_features *f, int64_t *n)
{
    SF_CHECK(f && n, SF_ERR_INVALID, "bad arguments");
    *n = f->n;
    return SF_OK;
}

extern "C" int sf_features_upload(sf_features *f, const float *rows, const uint8_t *valid, int64_t n)
{
    SF_CHECK(f && n >= 0 && (rows || n == 0), SF_ERR_INVALID, "bad arguments");
    sf_ctx *ctx = f->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    f->n = 0;
    f->n_valid = 0;
    if (n == 0) return SF_OK;
    sf::DevBuf count;
    SF_TRY(count.reserve(sizeof(unsigned long long)));
    SF_TRY(f->rows.reserve(sizeof(float) * DIM * (size_t)n));
    SF_TRY(f->valid.reserve((size_t)n));
    SF_HIP(hipMemsetAsync(count.p, 0, sizeof(unsigned long long), ctx->stream));
    SF_TRY(sf::upload_staged(ctx, f->rows.p, rows, sizeof(float) * DIM * (size_t)n));
    if (valid) SF_TRY(sf::upload_staged(ctx, f->valid.p, valid, (size_t)n));
    hipLaunchKernelGGL(k_validate_rows, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream, f->rows.as<float>(), n, valid ? 1 : 0, f->valid.as<uint8_t>(),
                       count.as<unsigned long long>());
    SF_HIP(hipGetLastError());
    unsigned long long h = 0;
    SF_HIP(hipMemcpyAsync(&h, count.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    f->n = n;
    f->n_valid = (int64_t)h;
    return SF_OK;
}

extern "C" int sf_features_download(sf_features *f, float *rows, uint8_t *valid, int64_t cap, int64_t *n)
{
    SF_CHECK(f, SF_ERR_INVALID, "bad arguments");
    if (n) *n = f->n;
    SF_CHECK(cap >= f->n && (rows || f->n == 0), SF_ERR_INVALID, "buffer too small");
    if (f->n == 0) return SF_OK;
    sf_ctx *ctx = f->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    SF_HIP(hipMemcpyAsync(rows, f->rows.p, sizeof(float) * DIM * (size_t)f->n, hipMemcpyDeviceToHost, ctx->stream));
    if (valid) SF_HIP(hipMemcpyAsync(valid, f->valid.p, (size_t)f->n, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    return SF_OK;
}

extern "C" void sf_fpfh_default_params(sf_fpfh_params *p)
{
    if (!p) return;
    *p = sf_fpfh_params{0.0, SF_ORIENT_NONE, 0, {0.0, 0.0, 1.0}};
}

extern "C" void sf_match_default_params(sf_match_params *p)
{
    if (!p) return;
    *p = sf_match_params{0.0, 0, 0};
}

extern "C" int sf_map_compute_fpfh(sf_map *m, const sf_fpfh_params *p, sf_features *out, sf_fpfh_stats *stats)
{
    SF_CHECK(m && out, SF_ERR_INVALID, "bad arguments");
    SF_TRY(check_fpfh_params(p));
    SF_CHECK(m->ctx == out->ctx, SF_ERR_INVALID, "the map and the feature set belong to different contexts");
    SF_CHECK(m->built, SF_ERR_STATE, "map not built");
    SF_CHECK(m->n == 0 || m->has_normals, SF_ERR_STATE, "no normals (sf_map_estimate_normals[_knn] or sf_map_set_normals first)");
    sf_fpfh_stats st;
    SF_TRY(fpfh_device(m, p, out, &st));
    if (stats) *stats = st;
    return SF_OK;
}

extern "C" int sf_map_compute_spfh(sf_map *m, const sf_fpfh_params *p, uint32_t *counts, int32_t *n_pairs)
{
    SF_CHECK(m, SF_ERR_INVALID, "bad arguments");
    SF_TRY(check_fpfh_params(p));
    SF_CHECK(m->built, SF_ERR_STATE, "map not built");
    SF_CHECK(m->n == 0 || m->has_normals, SF_ERR_STATE, "no normals (sf_map_estimate_normals[_knn] or sf_map_set_normals first)");
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    const int64_t n = m->n, nv = m->grid.n;
    if (n == 0) return SF_OK;
    sf::DevBuf oc, op;
    SF_TRY(oc.reserve(sizeof(uint32_t) * DIM * (size_t)n));
    SF_TRY(op.reserve(sizeof(int32_t) * (size_t)n));
    SF_HIP(hipMemsetAsync(oc.p, 0, sizeof(uint32_t) * DIM * (size_t)n, ctx->stream));
    SF_HIP(hipMemsetAsync(op.p, 0, sizeof(int32_t) * (size_t)n, ctx->stream));
    SpfhBufs B;
    if (nv > 0) {
        const float r2 = (float)(p->radius * p->radius);
        SF_TRY(spfh_enqueue(m, p, B, r2, sf::feature_reach(m->grid, r2)));
        hipLaunchKernelGGL(k_spfh_to_host_order, dim3(nblk(nv, 256)), dim3(256), 0, ctx->stream, m->grid, B.cnt.as<uint32_t>(), B.pairs.as<int32_t>(), oc.as<uint32_t>(),
                           op.as<int32_t>());
        SF_HIP(hipGetLastError());
    }
    if (counts) SF_HIP(hipMemcpyAsync(counts, oc.p, sizeof(uint32_t) * DIM * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (n_pairs) SF_HIP(hipMemcpyAsync(n_pairs, op.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    return SF_OK;
}

extern "C" int sf_cloud_compute_fpfh(sf_cloud *c, double normal_radius, const sf_fpfh_params *p, float cell, sf_features *out, sf_fpfh_stats *stats)
{
    SF_CHECK(c && out, SF_ERR_INVALID, "bad arguments");
    SF_TRY(check_fpfh_params(p));
    SF_CHECK(std::isfinite(normal_radius) && normal_radius > 0.0, SF_ERR_INVALID, "fpfh: the normal radius must be positive and finite (got %g)", normal_radius);
    SF_CHECK(c->ctx == out->ctx, SF_ERR_INVALID, "the cloud and the feature set belong to different contexts");
    sf_fpfh_stats st{0, 0, 0, 0, 0, -1.0f, -1.0f};
    if (c->n == 0) {
        out->n = 0;
        out->n_valid = 0;
        if (stats) *stats = st;
        return SF_OK;
    }
    sf_map *tmp = nullptr;
    SF_TRY(sf_map_create(c->ctx, &tmp));
    int rc = sf_map_build(tmp, c, cell);
    if (rc == SF_OK) rc = sf_map_estimate_normals(tmp, (float)normal_radius);
    if (rc == SF_OK) rc = fpfh_device(tmp, p, out, &st);
    sf_map_destroy(tmp);
    if (rc == SF_OK && stats) *stats = st;
    return rc;
}

extern "C" int sf_features_match(sf_features *src, sf_features *dst, const sf_match_params *p, int32_t *idx, float *dist2, float *second2, int32_t *pairs,
                                 int64_t cap_pairs, sf_match_stats *stats)
{
    SF_CHECK(src && dst && p, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(src->ctx == dst->ctx, SF_ERR_INVALID, "the two feature sets belong to different contexts");
    SF_CHECK(src->n < (int64_t)1 << 31 && dst->n < (int64_t)1 << 31, SF_ERR_INVALID, "a feature set of 2^31 rows or more cannot be matched");
    SF_CHECK(cap_pairs >= 0 || !pairs, SF_ERR_INVALID, "cap_pairs must not be negative");
    SF_CHECK(!std::isnan(p->ratio), SF_ERR_INVALID, "match: the ratio is not a number");
    sf_ctx *ctx = src->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t ns = src->n, nd = dst->n;
    sf_match_stats st{ns, nd, src->n_valid, dst->n_valid, 0, -1.0f, 0};
    if (ns == 0) {
        if (stats) *stats = st;
        return SF_OK;
    }
    const bool use_ratio = p->ratio > 0.0 && p->ratio < 1.0, mutual = p->mutual != 0 && nd > 0;
    const float rr = (float)(p->ratio * p->ratio);
    sf::DevBuf part, res, back, flags, count;
    SF_TRY(res.reserve((size_t)ns * (sizeof(int32_t) + 2 * sizeof(float))));
    int32_t *d_idx = res.as<int32_t>();
    float *d_dist2 = reinterpret_cast<float *>(d_idx + ns), *d_second2 = d_dist2 + ns;
    SF_TRY(flags.reserve((size_t)ns));
    SF_TRY(count.reserve(sizeof(unsigned long long)));
    if (mutual) SF_TRY(back.reserve((size_t)nd * (sizeof(int32_t) + sizeof(float))));
    SF_TRY(part.reserve(std::max(match_part_bytes(ns, nd), mutual ? match_part_bytes(nd, ns) : (size_t)0)));
    SF_HIP(hipMemsetAsync(count.p, 0, sizeof(unsigned long long), s));
    Events ev;
    SF_TRY(ev.start(p->profile != 0));
    SF_TRY(ev.mark(0, s));
    SF_TRY(match_enqueue(ctx, src, dst, part, d_idx, d_dist2, d_second2));
    if (mutual) { // the same kernels with the roles swapped (part is reused: the stream orders the two)
        int32_t *b_idx = back.as<int32_t>();
        SF_TRY(match_enqueue(ctx, dst, src, part, b_idx, reinterpret_cast<float *>(b_idx + nd), nullptr));
    }
    hipLaunchKernelGGL(k_match_accept, dim3(nblk(ns, 256)), dim3(256), 0, s, d_idx, d_dist2, d_second2, ns, use_ratio ? 1 : 0, rr,
                       mutual ? back.as<int32_t>() : (const int32_t *)nullptr, flags.as<uint8_t>(), count.as<unsigned long long>());
    SF_HIP(hipGetLastError());
    SF_TRY(ev.mark(1, s));
    std::vector<int32_t> h_idx;
    std::vector<uint8_t> h_flags;
    if (pairs && cap_pairs > 0) {
        h_idx.resize((size_t)ns);
        h_flags.resize((size_t)ns);
        SF_HIP(hipMemcpyAsync(h_idx.data(), d_idx, sizeof(int32_t) * (size_t)ns, hipMemcpyDeviceToHost, s));
        SF_HIP(hipMemcpyAsync(h_flags.data(), flags.p, (size_t)ns, hipMemcpyDeviceToHost, s));
    }
    if (idx) SF_HIP(hipMemcpyAsync(idx, d_idx, sizeof(int32_t) * (size_t)ns, hipMemcpyDeviceToHost, s));
    if (dist2) SF_HIP(hipMemcpyAsync(dist2, d_dist2, sizeof(float) * (size_t)ns, hipMemcpyDeviceToHost, s));
    if (second2) SF_HIP(hipMemcpyAsync(second2, d_second2, sizeof(float) * (size_t)ns, hipMemcpyDeviceToHost, s));
    unsigned long long h_count = 0;
    SF_HIP(hipMemcpyAsync(&h_count, count.p, sizeof(h_count), hipMemcpyDeviceToHost, s));
    SF_HIP(hipStreamSynchronize(s));
    st.n_matched = (int64_t)h_count;
    SF_TRY(ev.ms(0, 1, &st.match_ms));
    if (pairs && cap_pairs > 0) { // the accepted pairs in ascending i
        int64_t w = 0;
        for (int64_t i = 0; i < ns && w < cap_pairs; ++i)
            if (h_flags[(size_t)i]) {
                pairs[2 * w] = (int32_t)i;
                pairs[2 * w + 1] = h_idx[(size_t)i];
                ++w;
            }
    }
    if (stats) *stats = st;
    return SF_OK;
}
