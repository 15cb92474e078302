// sf_place.hip -- Scan Context place recognition over a keyframe database (sf_cloud_scan_context, sf_place_db_*; include/slamfusion.h;
// extension, no reference code: the rule is in DESIGN section 29 and restated in tests/place_ref_np.py).  gfx950 only, wave64.  A
// translation unit of its own over sf_common.hpp; nothing of sf_map.hip or sf_icp.hip.
//
// Descriptor (per scan):
//   a fill         every bin +0: empty
//   k_sc_build     one lane per point: the sensor frame, ring and sector in float64, then a 32-bit integer atomicMax of the bits of the
//                  float32 height, one for the lanes of a wave that share a bin -- a positive float orders like its bits, so the bin
//                  holds the same bits whatever the arrival order
//   k_sc_filled    one lane per bin: the count of bins that are not empty
//   k_sc_unit      one lane per column of a row of the database (or of a query): n[j] and the unit column u[.][j] in float64, once
// Match (per call):
//   k_sc_match     one lane per shift s of one (query, entry) pair, several pairs a block: the unit columns of QB queries and of the
//                  block's entries are staged in LDS; the lane walks j ascending, reads uq[i][j] as a broadcast and uc[i][(j+s) mod Ns]
//                  at consecutive addresses, and sums in the rule's order -- no Gram matrix, no cross-lane sum, no scratch.  A column
//                  that is not valid is all +0 and adds +0 to S, which leaves S as it is: only V looks at the flags.  The minimum over
//                  s is taken by the pair's first lane over the Ns values in LDS, ascending, so the smaller s wins a tie.
//   k_sc_select    one block per query: k rounds of "the smallest (D, index) above the last one taken"
#include "sf_common.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr double SC_PI = 3.141592653589793;
constexpr int SC_MAX_RINGS = 40, SC_MAX_SECTORS = 120, SC_MAX_QUERIES = 64, SC_MAX_K = 32;
constexpr int SC_SLOTS = 16, SC_WORDS = 8;
constexpr size_t SC_STAT_BYTES = sizeof(unsigned long long) * SC_SLOTS * SC_WORDS;
constexpr size_t SC_LDS_BUDGET = 64 * 1024; // what a block may ask for without an attribute

inline unsigned nblk(int64_t n, int b = 256) { return (unsigned)sf::div_up(n > 0 ? n : 1, b); }

// a[] = T[0] T[4] T[8] | T[1] T[5] T[9] | T[2] T[6] T[10] (the rows of R^T), t = T[3] T[7] T[11]
struct ScFrame {
    double a[9], t[3];
    double min_range, max_range, sensor_height;
    int Nr, Ns;
};

// The counters of a build: SC_SLOTS copies of SC_WORDS words, block b adding into copy b % SC_SLOTS and the host summing the copies
// (one address taking an atomic from every wave costs more than the launch's own work).
template <int NW>
__device__ __forceinline__ void block_add(const uint32_t (&wave_tot)[NW], unsigned long long *__restrict__ stat)
{
    __shared__ uint32_t part[4][NW];
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int k = 0; k < NW; ++k) part[threadIdx.x >> 6][k] = wave_tot[k];
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)NW) {
        const uint32_t t = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (t) atomicAdd(stat + (blockIdx.x % SC_SLOTS) * SC_WORDS + threadIdx.x, (unsigned long long)t);
    }
}

__global__ __launch_bounds__(256) void k_sc_build(const float *__restrict__ xyz, int64_t n, ScFrame g, uint32_t *__restrict__ desc, unsigned long long *__restrict__ stat)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool have = i < n;
    const float xf = have ? xyz[3 * i] : 0.0f, yf = have ? xyz[3 * i + 1] : 0.0f, zf = have ? xyz[3 * i + 2] : 0.0f;
    const bool fin = have && isfinite(xf) && isfinite(yf) && isfinite(zf);
    bool outside = false, below = false, binned = false;
    int bin = 0;
    uint32_t bits = 0u;
    if (fin) {
        const double d0 = (double)xf - g.t[0], d1 = (double)yf - g.t[1], d2 = (double)zf - g.t[2];
        const double x = (g.a[0] * d0 + g.a[1] * d1) + g.a[2] * d2;
        const double y = (g.a[3] * d0 + g.a[4] * d1) + g.a[5] * d2;
        const double z = (g.a[6] * d0 + g.a[7] * d1) + g.a[8] * d2;
        const double h2 = x * x + y * y;
        const double rho = sqrt(h2);
        const double v = rho / g.max_range * (double)g.Nr;
        outside = !(g.min_range <= rho) || !(v < (double)g.Nr); // floor(v) >= Nr iff v >= Nr
        if (!outside) {
            const float hgt = (float)(z + g.sensor_height);
            below = !(hgt > 0.0f);
            if (!below) {
                const double az = atan2(y, x);
                const double u = (az + SC_PI) / (2.0 * SC_PI) * (double)g.Ns;
                int col = (int)floor(u);
                if (col >= g.Ns) col -= g.Ns;
                col = min(max(col, 0), g.Ns - 1); // (a guard only: az lies in [-PI, PI], so u in [0, Ns])
                const int ring = min((int)floor(v), g.Nr - 1);
                bin = ring * g.Ns + col;
                bits = __float_as_uint(hgt);
                binned = true;
            }
        }
    }
    // The lanes of a wave that share a bin send ONE atomic, the largest of their heights: a ring scan puts dozens of consecutive lanes
    // into one bin, and 200 atomics on one address cost more than the rest of the launch.  The maximum is the same whoever sends it.
    // A bin only ever grows, so whatever a plain load returns is no more than the bin holds now: a height that does not exceed it
    // cannot change the bin and is not sent at all.
    unsigned long long todo = __ballot(binned);
    while (todo) {
        const int leader = __ffsll(todo) - 1;
        const int lead_bin = __shfl(bin, leader);
        const bool mine = binned && bin == lead_bin;
        uint32_t top = mine ? bits : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) top = max(top, (uint32_t)__shfl_xor((int)top, o));
        if ((int)(threadIdx.x & 63u) == leader && *reinterpret_cast<volatile uint32_t *>(desc + lead_bin) < top) atomicMax(desc + lead_bin, top);
        todo &= ~__ballot(mine);
    }
    const uint32_t tot[4] = {(uint32_t)__popcll(__ballot(have && !fin)), (uint32_t)__popcll(__ballot(outside)), (uint32_t)__popcll(__ballot(below)),
                             (uint32_t)__popcll(__ballot(binned))};
    block_add<4>(tot, stat); // not finite, outside, below, binned
}

__global__ __launch_bounds__(256) void k_sc_filled(const uint32_t *__restrict__ desc, int D, unsigned long long *__restrict__ stat)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool filled = i < D && desc[i] != 0u;
    const uint32_t tot[1] = {(uint32_t)__popcll(__ballot(filled))};
    block_add<1>(tot, stat + 4);
}

// rows [0, rows) of desc (float [rows][Nr][Ns]) -> unit (double, the same shape) and valid (uint8 [rows][Ns]); one lane per column
__global__ __launch_bounds__(256) void k_sc_unit(const float *__restrict__ desc, int64_t rows, int Nr, int Ns, double *__restrict__ unit, uint8_t *__restrict__ valid)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * Ns) return;
    const int64_t row = t / Ns;
    const int j = (int)(t - row * Ns);
    const float *__restrict__ a = desc + row * (int64_t)Nr * Ns + j;
    double *__restrict__ u = unit + row * (int64_t)Nr * Ns + j;
    double sum = 0.0;
    for (int i = 0; i < Nr; ++i) {
        const double v = (double)a[i * Ns];
        sum = sum + v * v;
    }
    const double nj = sqrt(sum);
    const bool ok = nj > 0.0;
    for (int i = 0; i < Nr; ++i) u[i * Ns] = ok ? (double)a[i * Ns] / nj : 0.0;
    valid[row * Ns + j] = ok ? 1 : 0;
}

// grid (blocks of `pairs` entries, groups of QB queries); dynamic LDS: [QB][D] doubles when QLDS | [pairs][D] doubles | [QB][blockDim]
// doubles | [QB][Ns] + [pairs][Ns] flags.  Thread t: pair slot t / Ns, shift t % Ns.
template <int QB, bool QLDS>
__global__ __launch_bounds__(256) void k_sc_match(const double *__restrict__ uq, const uint8_t *__restrict__ vq, int Q, const double *__restrict__ uc,
                                                  const uint8_t *__restrict__ vc, int N, int Nr, int Ns, int pairs, double *__restrict__ dist, int32_t *__restrict__ shift)
{
    extern __shared__ double lds[];
    const int D = Nr * Ns;
    const int q0 = blockIdx.y * QB, c0 = blockIdx.x * pairs;
    const int nq = min(QB, Q - q0), nc = min(pairs, N - c0);
    double *lq = lds;
    double *le = lds + (QLDS ? QB * D : 0);
    double *red = le + pairs * D;
    uint8_t *fq = reinterpret_cast<uint8_t *>(red + QB * blockDim.x);
    uint8_t *fe = fq + QB * Ns;
    const int tid = threadIdx.x, nt = blockDim.x;
    if (QLDS)
        for (int k = tid; k < QB * D; k += nt) lq[k] = k < nq * D ? uq[(size_t)q0 * D + k] : 0.0;
    for (int k = tid; k < nc * D; k += nt) le[k] = uc[(size_t)c0 * D + k];
    for (int k = tid; k < QB * Ns; k += nt) fq[k] = k < nq * Ns ? vq[(size_t)q0 * Ns + k] : 0;
    for (int k = tid; k < nc * Ns; k += nt) fe[k] = vc[(size_t)c0 * Ns + k];
    __syncthreads();
    const int p = tid / Ns, s = tid - p * Ns;
    const bool live = p < nc;
    if (live) {
        const double *__restrict__ e = le + p * D;
        const uint8_t *__restrict__ ve = fe + p * Ns;
        const double *__restrict__ qb[QB];
#pragma unroll
        for (int b = 0; b < QB; ++b) qb[b] = QLDS ? lq + b * D : uq + (size_t)(q0 + min(b, nq - 1)) * D;
        double S[QB];
        int V[QB];
#pragma unroll
        for (int b = 0; b < QB; ++b) { S[b] = 0.0; V[b] = 0; }
        int jc = s;
        for (int j = 0; j < Ns; ++j) {
            double cs[QB];
#pragma unroll
            for (int b = 0; b < QB; ++b) cs[b] = 0.0;
#pragma unroll 4
            for (int i = 0; i < Nr; ++i) {
                const double c = e[i * Ns + jc];
#pragma unroll
                for (int b = 0; b < QB; ++b) cs[b] = cs[b] + qb[b][i * Ns + j] * c;
            }
            const int okc = ve[jc];
#pragma unroll
            for (int b = 0; b < QB; ++b) {
                S[b] = S[b] + cs[b];
                V[b] += okc & (int)fq[b * Ns + j];
            }
            jc = jc + 1 == Ns ? 0 : jc + 1;
        }
#pragma unroll
        for (int b = 0; b < QB; ++b) red[b * nt + tid] = V[b] > 0 ? 1.0 - S[b] / (double)V[b] : 1.0;
    }
    __syncthreads();
    if (live && s == 0) {
#pragma unroll
        for (int b = 0; b < QB; ++b) {
            if (b < nq) {
                const double *r = red + b * nt + tid;
                double best = r[0];
                int at = 0;
                for (int k = 1; k < Ns; ++k)
                    if (r[k] < best) { best = r[k]; at = k; }
                dist[(size_t)(q0 + b) * N + (c0 + p)] = best;
                shift[(size_t)(q0 + b) * N + (c0 + p)] = at;
            }
        }
    }
}

// one block per query: slot r gets the smallest (D, index) above slot r - 1's; slots past N get -1, +inf, 0
__global__ __launch_bounds__(256) void k_sc_select(const double *__restrict__ dist, const int32_t *__restrict__ shift, int N, int k, int32_t *__restrict__ o_idx,
                                                   double *__restrict__ o_dist, int32_t *__restrict__ o_shift)
{
    __shared__ double s_d[256];
    __shared__ int s_i[256];
    const int q = blockIdx.x, tid = threadIdx.x;
    const double *__restrict__ d = dist + (size_t)q * N;
    double last_d = -INFINITY;
    int last_i = -1;
    for (int r = 0; r < k; ++r) {
        double bd = INFINITY;
        int bi = -1;
        for (int c = tid; c < N; c += 256) {
            const double v = d[c];
            const bool above = v > last_d || (v == last_d && c > last_i);
            if (above && (bi < 0 || v < bd)) { bd = v; bi = c; } // (c ascends: the first one met keeps a tie)
        }
        s_d[tid] = bd;
        s_i[tid] = bi;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) {
                const double od = s_d[tid + w];
                const int oi = s_i[tid + w];
                const bool take = oi >= 0 && (s_i[tid] < 0 || od < s_d[tid] || (od == s_d[tid] && oi < s_i[tid]));
                if (take) { s_d[tid] = od; s_i[tid] = oi; }
            }
            __syncthreads();
        }
        last_d = s_d[0];
        last_i = s_i[0];
        if (tid == 0) {
            o_idx[q * k + r] = last_i;
            o_dist[q * k + r] = last_i >= 0 ? last_d : INFINITY;
            o_shift[q * k + r] = last_i >= 0 ? shift[(size_t)q * N + last_i] : 0;
        }
        __syncthreads();
        if (last_i < 0) { // nothing left: the remaining slots are empty too
            for (int rr = r + 1 + tid; rr < k; rr += 256) {
                o_idx[q * k + rr] = -1;
                o_dist[q * k + rr] = INFINITY;
                o_shift[q * k + rr] = 0;
            }
            break;
        }
    }
}

struct Events { // hipEvents around the kernels; the times are read after the stream was synchronised
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    Events() = default;
    Events(const Events &) = delete;
    Events &operator=(const Events &) = delete;
    ~Events()
    {
        for (hipEvent_t e : ev)
            if (e) { hipError_t rc = hipEventDestroy(e); (void)rc; }
    }
    int start()
    {
        for (hipEvent_t &e : ev) SF_HIP(hipEventCreate(&e));
        return SF_OK;
    }
    int mark(int i, hipStream_t s)
    {
        SF_HIP(hipEventRecord(ev[i], s));
        return SF_OK;
    }
    int ms(int a, int b, float *out)
    {
        SF_HIP(hipEventElapsedTime(out, ev[a], ev[b]));
        return SF_OK;
    }
};

bool pose_finite(const double *T)
{
    if (!T) return true;
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(T[k])) return false;
    return true;
}

int check_params(const sf_place_params *p)
{
    SF_CHECK(p, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(p->num_rings >= 1 && p->num_rings <= SC_MAX_RINGS && p->num_sectors >= 1 && p->num_sectors <= SC_MAX_SECTORS, SF_ERR_INVALID,
             "scan context: num_rings must be 1 .. %d and num_sectors 1 .. %d (got %d, %d)", SC_MAX_RINGS, SC_MAX_SECTORS, (int)p->num_rings, (int)p->num_sectors);
    SF_CHECK(std::isfinite(p->min_range) && std::isfinite(p->max_range) && std::isfinite(p->sensor_height), SF_ERR_INVALID, "scan context: the ranges and the height must be finite");
    SF_CHECK(p->min_range >= 0.0 && p->max_range > p->min_range, SF_ERR_INVALID, "scan context: 0 <= min_range < max_range (got %g, %g)", p->min_range, p->max_range);
    return SF_OK;
}

ScFrame frame_arg(const sf_place_params &prm, const double *T)
{
    static const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (!T) T = I;
    ScFrame g{};
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) g.a[3 * r + k] = T[4 * k + r];
        g.t[r] = T[4 * r + 3];
    }
    g.min_range = prm.min_range;
    g.max_range = prm.max_range;
    g.sensor_height = prm.sensor_height;
    g.Nr = prm.num_rings;
    g.Ns = prm.num_sectors;
    return g;
}

// the fill and the two kernels of a descriptor build into d_desc (float [Nr][Ns]), enqueued; d_stat is zeroed first
int build_enqueue(sf_ctx *ctx, const sf_place_params &prm, sf_cloud *c, const double *pose, float *d_desc, unsigned long long *d_stat)
{
    hipStream_t s = ctx->stream;
    const int D = prm.num_rings * prm.num_sectors;
    SF_HIP(hipMemsetAsync(d_stat, 0, SC_STAT_BYTES, s));
    SF_HIP(hipMemsetAsync(d_desc, 0, sizeof(float) * (size_t)D, s));
    if (c->n > 0)
        hipLaunchKernelGGL(k_sc_build, dim3(nblk(c->n)), dim3(256), 0, s, c->xyz.as<float>(), c->n, frame_arg(prm, pose), reinterpret_cast<uint32_t *>(d_desc), d_stat);
    hipLaunchKernelGGL(k_sc_filled, dim3(nblk(D)), dim3(256), 0, s, reinterpret_cast<const uint32_t *>(d_desc), D, d_stat);
    SF_HIP(hipGetLastError());
    return SF_OK;
}

// the counters of a build, summed over the copies; synchronises the stream
int read_build_stats(sf_ctx *ctx, const unsigned long long *d_stat, int64_t n_points, Events &ev, sf_place_stats *stats)
{
    unsigned long long h[SC_SLOTS * SC_WORDS], sum[5] = {0, 0, 0, 0, 0};
    SF_HIP(hipMemcpyAsync(h, d_stat, SC_STAT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 5; ++k)
        for (int slot = 0; slot < SC_SLOTS; ++slot) sum[k] += h[slot * SC_WORDS + k];
    if (stats) {
        sf_place_stats st{};
        st.n_points = n_points;
        st.n_nonfinite = (int64_t)sum[0];
        st.n_outside = (int64_t)sum[1];
        st.n_below = (int64_t)sum[2];
        st.n_binned = (int64_t)sum[3];
        st.n_filled = (int64_t)sum[4];
        SF_TRY(ev.ms(0, 1, &st.device_ms));
        *stats = st;
    }
    return SF_OK;
}

int check_cloud(const sf_ctx *ctx, const sf_cloud *c, const double *pose)
{
    SF_CHECK(c, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(c->ctx == ctx, SF_ERR_INVALID, "scan context: the cloud belongs to another context");
    SF_CHECK(pose_finite(pose), SF_ERR_INVALID, "scan context: the pose is not finite");
    SF_CHECK(c->n < (int64_t(1) << 31), SF_ERR_INVALID, "scan context: the cloud must hold fewer than 2^31 points");
    return SF_OK;
}

// a descriptor given by the host: every value finite and not negative
bool rows_valid(const float *desc, size_t count)
{
    for (size_t k = 0; k < count; ++k)
        if (!(desc[k] >= 0.0f) || !std::isfinite(desc[k])) return false;
    return true;
}

} // namespace

struct sf_place_db {
    sf_ctx *ctx = nullptr;
    sf_place_params prm{};
    int64_t n = 0, cap = 0;
    sf::DevBuf desc;  // float  [cap][Nr][Ns]
    sf::DevBuf unit;  // double [cap][Nr][Ns]: the unit columns, computed once at insertion
    sf::DevBuf valid; // uint8  [cap][Ns]
    std::vector<double> poses; // [n][16], host
    // the queries of a call: descriptors, unit columns, flags (SC_MAX_QUERIES rows), and its results
    sf::DevBuf q_desc, q_unit, q_valid, d_dist, d_shift, top, stat;
    int D() const { return prm.num_rings * prm.num_sectors; }
};

namespace {

// room for `extra` more rows: the capacity doubles (from 16) and what the database held is carried over
int db_grow(sf_place_db *db, int64_t extra)
{
    const int64_t need = db->n + extra;
    if (need <= db->cap) return SF_OK;
    SF_CHECK(need < (int64_t(1) << 24), SF_ERR_OVERFLOW, "place db: more than 2^24 entries");
    int64_t cap = db->cap > 0 ? db->cap : 16;
    while (cap < need) cap *= 2;
    hipStream_t s = db->ctx->stream;
    const size_t D = (size_t)db->D(), Ns = (size_t)db->prm.num_sectors;
    sf::DevBuf nd, nu, nv;
    SF_TRY(nd.reserve(sizeof(float) * D * (size_t)cap));
    SF_TRY(nu.reserve(sizeof(double) * D * (size_t)cap));
    SF_TRY(nv.reserve(Ns * (size_t)cap));
    if (db->n > 0) {
        SF_HIP(hipMemcpyAsync(nd.p, db->desc.p, sizeof(float) * D * (size_t)db->n, hipMemcpyDeviceToDevice, s));
        SF_HIP(hipMemcpyAsync(nu.p, db->unit.p, sizeof(double) * D * (size_t)db->n, hipMemcpyDeviceToDevice, s));
        SF_HIP(hipMemcpyAsync(nv.p, db->valid.p, Ns * (size_t)db->n, hipMemcpyDeviceToDevice, s));
    }
    SF_HIP(hipStreamSynchronize(s)); // the old allocations are freed when nd, nu, nv leave
    db->desc.swap(nd);
    db->unit.swap(nu);
    db->valid.swap(nv);
    db->cap = cap;
    return SF_OK;
}

int unit_enqueue(sf_place_db *db, const float *d_desc, int64_t rows, double *d_unit, uint8_t *d_valid)
{
    const int Nr = db->prm.num_rings, Ns = db->prm.num_sectors;
    hipLaunchKernelGGL(k_sc_unit, dim3(nblk(rows * Ns)), dim3(256), 0, db->ctx->stream, d_desc, rows, Nr, Ns, d_unit, d_valid);
    SF_HIP(hipGetLastError());
    return SF_OK;
}

template <int QB, bool QLDS>
int match_launch(sf_place_db *db, int Q)
{
    const int Nr = db->prm.num_rings, Ns = db->prm.num_sectors, N = (int)db->n;
    const size_t D = (size_t)Nr * Ns;
    // per block: the queries, a reduction row per query, the queries' flags; per pair: the entry and its flags
    int pairs = 256 / Ns;
    for (;; --pairs) {
        const int nt = (pairs * Ns + 63) / 64 * 64;
        const size_t bytes = sizeof(double) * ((QLDS ? QB * D : 0) + (size_t)pairs * D + (size_t)QB * nt) + (size_t)QB * Ns + (size_t)pairs * Ns;
        if (bytes <= SC_LDS_BUDGET || pairs == 1) {
            SF_CHECK(bytes <= SC_LDS_BUDGET, SF_ERR_INVALID, "place db: the shape does not fit a block");
            hipLaunchKernelGGL((k_sc_match<QB, QLDS>), dim3((unsigned)sf::div_up(N, pairs), (unsigned)sf::div_up(Q, QB)), dim3(nt), bytes, db->ctx->stream,
                               db->q_unit.as<double>(), db->q_valid.as<uint8_t>(), Q, db->unit.as<double>(), db->valid.as<uint8_t>(), N, Nr, Ns, pairs, db->d_dist.as<double>(),
                               db->d_shift.as<int32_t>());
            SF_HIP(hipGetLastError());
            return SF_OK;
        }
    }
}

// q_desc holds Q descriptors: their unit columns, then D and shift of every pair into d_dist / d_shift ([Q][N]); N > 0
int match_enqueue(sf_place_db *db, int Q)
{
    SF_TRY(unit_enqueue(db, db->q_desc.as<float>(), Q, db->q_unit.as<double>(), db->q_valid.as<uint8_t>()));
    SF_TRY(db->d_dist.reserve(sizeof(double) * (size_t)Q * (size_t)db->n));
    SF_TRY(db->d_shift.reserve(sizeof(int32_t) * (size_t)Q * (size_t)db->n));
    const size_t desc_bytes = sizeof(double) * (size_t)db->D();
    // two queries a lane halve the LDS reads per multiply-add; a shape too large to sit in LDS beside one entry reads its query from memory
    if (Q >= 2 && 2 * desc_bytes <= SC_LDS_BUDGET / 3) return match_launch<2, true>(db, Q);
    if (2 * desc_bytes + 4096 <= SC_LDS_BUDGET) return match_launch<1, true>(db, Q);
    return match_launch<1, false>(db, Q);
}

int check_queries(const sf_place_db *db, const float *queries, int64_t Q)
{
    SF_CHECK(db && queries, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(Q >= 1 && Q <= SC_MAX_QUERIES, SF_ERR_INVALID, "place db: the number of queries must be 1 .. %d (got %lld)", SC_MAX_QUERIES, (long long)Q);
    SF_CHECK(rows_valid(queries, (size_t)Q * (size_t)db->D()), SF_ERR_INVALID, "place db: a query holds a negative or non-finite value");
    return SF_OK;
}

int reserve_queries(sf_place_db *db)
{
    const size_t D = (size_t)db->D();
    SF_TRY(db->q_desc.reserve(sizeof(float) * D * SC_MAX_QUERIES));
    SF_TRY(db->q_unit.reserve(sizeof(double) * D * SC_MAX_QUERIES));
    SF_TRY(db->q_valid.reserve((size_t)db->prm.num_sectors * SC_MAX_QUERIES));
    return SF_OK;
}

// T_entry . Rz(shift 2 PI / Ns), float64
void candidate_pose(const double *T, int shift, int Ns, double *out)
{
    const double ang = (double)shift * (2.0 * SC_PI / (double)Ns);
    const double c = std::cos(ang), s = std::sin(ang);
    for (int r = 0; r < 4; ++r) {
        out[4 * r + 0] = T[4 * r + 0] * c + T[4 * r + 1] * s;
        out[4 * r + 1] = T[4 * r + 1] * c - T[4 * r + 0] * s;
        out[4 * r + 2] = T[4 * r + 2];
        out[4 * r + 3] = T[4 * r + 3];
    }
}

// the match and the selection for the Q descriptors in q_desc; ev[0] has been recorded.  Synchronises the stream.
int query_device(sf_place_db *db, int Q, int k, int32_t *idx, double *dist, int32_t *shift, double *poses, Events &ev, sf_place_match_stats *stats)
{
    sf_ctx *ctx = db->ctx;
    hipStream_t s = ctx->stream;
    const size_t slots = (size_t)Q * (size_t)k;
    std::vector<int32_t> h_idx(slots, -1), h_shift(slots, 0);
    std::vector<double> h_dist(slots, INFINITY);
    float match_ms = 0.0f, select_ms = 0.0f;
    if (db->n > 0) {
        const size_t off_d = (sizeof(int32_t) * slots + 255) & ~size_t(255), off_s = off_d + ((sizeof(double) * slots + 255) & ~size_t(255));
        SF_TRY(db->top.reserve(off_s + sizeof(int32_t) * slots));
        int32_t *t_idx = db->top.as<int32_t>();
        double *t_dist = reinterpret_cast<double *>(db->top.as<char>() + off_d);
        int32_t *t_shift = reinterpret_cast<int32_t *>(db->top.as<char>() + off_s);
        SF_TRY(match_enqueue(db, Q));
        SF_TRY(ev.mark(1, s));
        hipLaunchKernelGGL(k_sc_select, dim3((unsigned)Q), dim3(256), 0, s, db->d_dist.as<double>(), db->d_shift.as<int32_t>(), (int)db->n, k, t_idx, t_dist, t_shift);
        SF_HIP(hipGetLastError());
        SF_TRY(ev.mark(2, s));
        SF_HIP(hipMemcpyAsync(h_idx.data(), t_idx, sizeof(int32_t) * slots, hipMemcpyDeviceToHost, s));
        SF_HIP(hipMemcpyAsync(h_dist.data(), t_dist, sizeof(double) * slots, hipMemcpyDeviceToHost, s));
        SF_HIP(hipMemcpyAsync(h_shift.data(), t_shift, sizeof(int32_t) * slots, hipMemcpyDeviceToHost, s));
        SF_HIP(hipStreamSynchronize(s));
        SF_TRY(ev.ms(0, 1, &match_ms));
        SF_TRY(ev.ms(1, 2, &select_ms));
    }
    for (size_t t = 0; t < slots; ++t) {
        if (idx) idx[t] = h_idx[t];
        if (dist) dist[t] = h_dist[t];
        if (shift) shift[t] = h_shift[t];
        if (poses) {
            if (h_idx[t] >= 0) candidate_pose(db->poses.data() + 16 * (size_t)h_idx[t], h_shift[t], db->prm.num_sectors, poses + 16 * t);
            else std::fill(poses + 16 * t, poses + 16 * t + 16, 0.0);
        }
    }
    if (stats) *stats = sf_place_match_stats{Q, db->n, match_ms, select_ms};
    return SF_OK;
}

} // namespace

extern "C" void sf_place_default_params(sf_place_params *p)
{
    if (!p) return;
    *p = sf_place_params{20, 60, 0.5, 80.0, 2.0};
}

extern "C" int sf_cloud_scan_context(sf_cloud *c, const double *pose, const sf_place_params *p, float *desc, sf_place_stats *stats)
{
    SF_CHECK(c, SF_ERR_INVALID, "bad arguments");
    SF_TRY(check_params(p));
    SF_TRY(check_cloud(c->ctx, c, pose));
    sf_ctx *ctx = c->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t D = (size_t)p->num_rings * (size_t)p->num_sectors;
    sf::DevBuf buf; // the counters and, behind them, the descriptor
    SF_TRY(buf.reserve(SC_STAT_BYTES + sizeof(float) * D));
    unsigned long long *d_stat = buf.as<unsigned long long>();
    float *d_desc = reinterpret_cast<float *>(buf.as<char>() + SC_STAT_BYTES);
    Events ev;
    SF_TRY(ev.start());
    SF_TRY(ev.mark(0, s));
    SF_TRY(build_enqueue(ctx, *p, c, pose, d_desc, d_stat));
    SF_TRY(ev.mark(1, s));
    if (desc) SF_HIP(hipMemcpyAsync(desc, d_desc, sizeof(float) * D, hipMemcpyDeviceToHost, s));
    return read_build_stats(ctx, d_stat, c->n, ev, stats);
}

extern "C" int sf_place_db_create(sf_ctx *ctx, const sf_place_params *p, sf_place_db **out)
{
    SF_CHECK(ctx && out, SF_ERR_INVALID, "bad arguments");
    SF_TRY(check_params(p));
    SF_HIP(hipSetDevice(ctx->device));
    sf_place_db *db = new (std::nothrow) sf_place_db();
    SF_CHECK(db, SF_ERR_NOMEM, "out of host memory");
    db->ctx = ctx;
    db->prm = *p;
    int rc = db->stat.reserve(SC_STAT_BYTES);
    if (rc == SF_OK) rc = reserve_queries(db);
    if (rc != SF_OK) {
        delete db;
        return rc;
    }
    sf::ctx_retain(ctx);
    *out = db;
    return SF_OK;
}

extern "C" void sf_place_db_destroy(sf_place_db *db)
{
    if (!db) return;
    hipError_t e = hipStreamSynchronize(db->ctx->stream);
    (void)e;
    sf_ctx *ctx = db->ctx;
    delete db;
    sf::ctx_release(ctx);
}

extern "C" int sf_place_db_info(const sf_place_db *db, sf_place_params *p, int64_t *n_entries)
{
    SF_CHECK(db, SF_ERR_INVALID, "bad arguments");
    if (p) *p = db->prm;
    if (n_entries) *n_entries = db->n;
    return SF_OK;
}

extern "C" int sf_place_db_clear(sf_place_db *db)
{
    SF_CHECK(db, SF_ERR_INVALID, "bad arguments");
    db->n = 0;
    db->poses.clear();
    return SF_OK;
}

extern "C" int sf_place_db_add_cloud(sf_place_db *db, sf_cloud *c, const double *pose, const double *entry_pose, int64_t *index, sf_place_stats *stats)
{
    SF_CHECK(db, SF_ERR_INVALID, "bad arguments");
    SF_TRY(check_cloud(db->ctx, c, pose));
    SF_CHECK(pose_finite(entry_pose), SF_ERR_INVALID, "place db: the entry's pose is not finite");
    sf_ctx *ctx = db->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    SF_TRY(db_grow(db, 1));
    const size_t D = (size_t)db->D(), at = (size_t)db->n;
    float *d_desc = db->desc.as<float>() + at * D;
    Events ev;
    SF_TRY(ev.start());
    SF_TRY(ev.mark(0, s));
    SF_TRY(build_enqueue(ctx, db->prm, c, pose, d_desc, db->stat.as<unsigned long long>()));
    SF_TRY(ev.mark(1, s));
    SF_TRY(unit_enqueue(db, d_desc, 1, db->unit.as<double>() + at * D, db->valid.as<uint8_t>() + at * (size_t)db->prm.num_sectors));
    SF_TRY(read_build_stats(ctx, db->stat.as<unsigned long long>(), c->n, ev, stats));
    static const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const double *T = entry_pose ? entry_pose : I;
    db->poses.insert(db->poses.end(), T, T + 16);
    if (index) *index = db->n;
    db->n += 1;
    return SF_OK;
}

extern "C" int sf_place_db_add_descriptors(sf_place_db *db, const float *desc, const double *poses, int64_t n)
{
    SF_CHECK(db && n >= 0 && (desc || n == 0), SF_ERR_INVALID, "bad arguments");
    if (n == 0) return SF_OK;
    const size_t D = (size_t)db->D();
    SF_CHECK(rows_valid(desc, (size_t)n * D), SF_ERR_INVALID, "place db: a descriptor holds a negative or non-finite value");
    if (poses)
        for (int64_t k = 0; k < n; ++k) SF_CHECK(pose_finite(poses + 16 * k), SF_ERR_INVALID, "place db: pose %lld is not finite", (long long)k);
    sf_ctx *ctx = db->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    SF_TRY(db_grow(db, n));
    const size_t at = (size_t)db->n;
    float *d_desc = db->desc.as<float>() + at * D;
    SF_TRY(sf::upload_staged(ctx, d_desc, desc, sizeof(float) * D * (size_t)n));
    SF_TRY(unit_enqueue(db, d_desc, n, db->unit.as<double>() + at * D, db->valid.as<uint8_t>() + at * (size_t)db->prm.num_sectors));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    static const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    for (int64_t k = 0; k < n; ++k) {
        const double *T = poses ? poses + 16 * k : I;
        db->poses.insert(db->poses.end(), T, T + 16);
    }
    db->n += n;
    return SF_OK;
}

extern "C" int sf_place_db_download(sf_place_db *db, float *desc, double *poses, int64_t cap, int64_t *n)
{
    SF_CHECK(db, SF_ERR_INVALID, "bad arguments");
    if (n) *n = db->n;
    if (!desc && !poses) return SF_OK;
    SF_CHECK(cap >= db->n, SF_ERR_INVALID, "place db: room for %lld entries, the database holds %lld", (long long)cap, (long long)db->n);
    if (db->n == 0) return SF_OK;
    if (poses) std::copy(db->poses.begin(), db->poses.end(), poses);
    if (desc) {
        SF_HIP(hipSetDevice(db->ctx->device));
        SF_HIP(hipMemcpyAsync(desc, db->desc.p, sizeof(float) * (size_t)db->D() * (size_t)db->n, hipMemcpyDeviceToHost, db->ctx->stream));
        SF_HIP(hipStreamSynchronize(db->ctx->stream));
    }
    return SF_OK;
}

extern "C" int sf_place_db_distances(sf_place_db *db, const float *queries, int64_t Q, double *dist, int32_t *shift, sf_place_match_stats *stats)
{
    SF_TRY(check_queries(db, queries, Q));
    sf_ctx *ctx = db->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    float match_ms = 0.0f;
    if (db->n > 0) {
        SF_TRY(sf::upload_staged(ctx, db->q_desc.p, queries, sizeof(float) * (size_t)db->D() * (size_t)Q));
        Events ev;
        SF_TRY(ev.start());
        SF_TRY(ev.mark(0, s));
        SF_TRY(match_enqueue(db, (int)Q));
        SF_TRY(ev.mark(1, s));
        const size_t pairs = (size_t)Q * (size_t)db->n;
        if (dist) SF_HIP(hipMemcpyAsync(dist, db->d_dist.p, sizeof(double) * pairs, hipMemcpyDeviceToHost, s));
        if (shift) SF_HIP(hipMemcpyAsync(shift, db->d_shift.p, sizeof(int32_t) * pairs, hipMemcpyDeviceToHost, s));
        SF_HIP(hipStreamSynchronize(s));
        SF_TRY(ev.ms(0, 1, &match_ms));
    }
    if (stats) *stats = sf_place_match_stats{Q, db->n, match_ms, 0.0f};
    return SF_OK;
}

extern "C" int sf_place_db_query(sf_place_db *db, const float *queries, int64_t Q, int k, int32_t *idx, double *dist, int32_t *shift, double *poses,
                                 sf_place_match_stats *stats)
{
    SF_TRY(check_queries(db, queries, Q));
    SF_CHECK(k >= 1 && k <= SC_MAX_K, SF_ERR_INVALID, "place db: k must be 1 .. %d (got %d)", SC_MAX_K, k);
    sf_ctx *ctx = db->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    Events ev;
    if (db->n > 0) {
        SF_TRY(sf::upload_staged(ctx, db->q_desc.p, queries, sizeof(float) * (size_t)db->D() * (size_t)Q));
        SF_TRY(ev.start());
        SF_TRY(ev.mark(0, ctx->stream));
    }
    return query_device(db, (int)Q, k, idx, dist, shift, poses, ev, stats);
}

extern "C" int sf_place_db_query_cloud(sf_place_db *db, sf_cloud *c, const double *pose, int k, int32_t *idx, double *dist, int32_t *shift, double *poses,
                                       sf_place_match_stats *stats, sf_place_stats *build_stats)
{
    SF_CHECK(db, SF_ERR_INVALID, "bad arguments");
    SF_TRY(check_cloud(db->ctx, c, pose));
    SF_CHECK(k >= 1 && k <= SC_MAX_K, SF_ERR_INVALID, "place db: k must be 1 .. %d (got %d)", SC_MAX_K, k);
    sf_ctx *ctx = db->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    Events bev, ev;
    SF_TRY(bev.start());
    SF_TRY(bev.mark(0, s));
    SF_TRY(build_enqueue(ctx, db->prm, c, pose, db->q_desc.as<float>(), db->stat.as<unsigned long long>()));
    SF_TRY(bev.mark(1, s));
    SF_TRY(ev.start());
    SF_TRY(ev.mark(0, s));
    SF_TRY(query_device(db, 1, k, idx, dist, shift, poses, ev, stats));
    return read_build_stats(ctx, db->stat.as<unsigned long long>(), c->n, bev, build_stats);
}
