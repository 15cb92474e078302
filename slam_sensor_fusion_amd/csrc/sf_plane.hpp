// sf_plane.hpp -- RANSAC plane segmentation and ground removal of a cloud (extension, no reference code).  Included by
// sf_map.hip after the clustering block: it uses smallest_eigvec of the map normals, read_words and nblk of sf_map.hip.
//
// The rule.  mix(x) is the splitmix64 step (plane_mix below).  Hypothesis h of H samples the original indices
//   i_j = mix(seed + 0x9E3779B97F4A7C15 (3h + j + 1)) mod n,  j = 0, 1, 2.
// Hypotheses are built ON THE HOST in float64, unfused, left to right (x86-64 sqrt and / are correctly rounded, so numpy agrees bit
// for bit): u = p1 - p0, v = p2 - p0, N = u x v, nn = Nx^2 + Ny^2 + Nz^2.  Degenerate (four NaNs): two equal indices; nn not finite
// or not > 0; an axis is given and |N^ . axis| < axis_min_cos.  Otherwise N^ = N / sqrt(nn), oriented N^ . axis >= 0 with an axis
// and "the first non-zero of (z, y, x) is positive" without, d = -(N^ . p0), the four values rounded to float32 once.  The axis is
// normalised in float64 beforehand; all zeros mean none.
// Score: t = (float)distance_threshold; x is an inlier of (a, b, c, d) iff fabsf(s) < t with s = a x; s = s + b y; s = s + c z;
// s = s + d in float32, unfused (plane_hit below) -- a non-finite point or a NaN plane never matches.  count_h = the inliers.
// Choice: the largest count, on a tie the smallest h.  Below min_inliers no plane is found: found = 0, four zeros, no inlier, SF_OK.
// Refit (refine != 0): over the inliers of the best plane the float64 moments of x - c0 (count, 3 first, 6 second), c0 = -d (a, b, c)
// the plane's foot point; mean m and covariance from them; the normal is smallest_eigvec of the covariance signed so that it does
// not oppose (a, b, c); d' = -n' . (c0 + m); rounded to float32.  Fewer than 3 inliers or anything non-finite: the hypothesis plane
// stands, refined = 0.  The final inliers are those of the final plane under the score rule.  The sums are taken in an order fixed
// by n alone and only integer atomics are used: the same call returns the same bits every time.
#pragma once

namespace {

constexpr int PL_MAX_H = 4096;       // hypotheses per call: the LDS counters of k_plane_score (16 KiB)
constexpr int PL_TILE = 1024;        // points per workgroup and pass: 256 lanes x 4
constexpr int PL_MOM = 10;           // count, 3 first moments, 6 second moments
constexpr int PL_MOM_BLOCKS = 256;   // rows of partial moments at most: one per lane of k_plane_refit

struct PlaneBest { long long index, count; float plane[4]; int found, pad; };
struct PlaneFinal { float plane[4]; int found, refined; unsigned long long n_inliers; };
static_assert(sizeof(PlaneBest) == 40 && sizeof(PlaneFinal) == 32, "read back as 8-byte words");

// the score rule: four statements, unfused (-ffp-contract=off), in this order
__device__ __forceinline__ bool plane_hit(float a, float b, float c, float d, float x, float y, float z, float t)
{
    float s = a * x;
    s = s + b * y;
    s = s + c * z;
    s = s + d;
    return fabsf(s) < t;
}

// the same four statements on two points at once (packed float32 operations round like the single ones)
typedef float pl_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ pl_f2 plane_score2(const float4 pl, const pl_f2 x, const pl_f2 y, const pl_f2 z)
{
    pl_f2 s = pl.x * x;
    s = s + pl.y * y;
    s = s + pl.z * z;
    s = s + pl.w;
    return s;
}

__global__ __launch_bounds__(256) void k_plane_gather(const float *__restrict__ xyz, const int32_t *__restrict__ idx, int count, float *__restrict__ out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const size_t i = (size_t)idx[k];
    out[3 * k] = xyz[3 * i]; out[3 * k + 1] = xyz[3 * i + 1]; out[3 * k + 2] = xyz[3 * i + 2];
}

// N x H point-plane tests, the cloud read once.  A lane holds 4 consecutive points per pass (48 contiguous bytes of the AoS array,
// 16-byte aligned: the array is the cloud's own allocation) and runs every plane over them; the plane is a uniform index into a
// const __restrict__ argument, so its coefficients arrive in SGPRs.  Per wave, plane and pass the four ballots are counted into
// lane (h mod 64) of one register, and every 64 planes each lane adds its plane's count to the workgroup's LDS counter of that
// plane: one LDS add per wave, plane and pass, 64 of them in one instruction.  A workgroup strides over the tiles and leaves its
// counters as row blockIdx.x of the slab uint32[blocks][H].  The tail is masked (NaN points match nothing) and never read past the end.
__global__ __launch_bounds__(256) void k_plane_score(const float *__restrict__ xyz, int64_t n, const float4 *__restrict__ planes, int H, float t,
                                                      uint32_t *__restrict__ slab)
{
    __shared__ uint32_t cnt[PL_MAX_H];
    for (int h = threadIdx.x; h < H; h += 256) cnt[h] = 0u;
    __syncthreads();
    const int64_t ntiles = (n + PL_TILE - 1) / PL_TILE;
    const int lane = (int)(threadIdx.x & 63u);
    const float nan = __uint_as_float(0x7fc00000u);
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t g = tile * 256 + threadIdx.x, p0 = 4 * g;
        float p[12];
        if (p0 + 4 <= n) {
            const float4 *v = reinterpret_cast<const float4 *>(xyz) + 3 * g;
            const float4 q0 = v[0], q1 = v[1], q2 = v[2];
            p[0] = q0.x; p[1] = q0.y; p[2] = q0.z; p[3] = q0.w; p[4] = q1.x; p[5] = q1.y; p[6] = q1.z; p[7] = q1.w;
            p[8] = q2.x; p[9] = q2.y; p[10] = q2.z; p[11] = q2.w;
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) p[k] = p0 + k / 3 < n ? xyz[3 * p0 + k] : nan;
        }
        // two points per packed operation: (x, x'), (y, y'), (z, z') of points 0 | 1 and 2 | 3
        const pl_f2 xa = {p[0], p[3]}, ya = {p[1], p[4]}, za = {p[2], p[5]}, xb = {p[6], p[9]}, yb = {p[7], p[10]}, zb = {p[8], p[11]};
        for (int hb = 0; hb < H; hb += 64) { // lane k of acc: the wave's count of plane hb + k in this pass
            uint32_t acc = 0u;
#pragma unroll 8
            for (int k = 0; k < 64; ++k) { // (the planes are padded to a multiple of 64 with NaN planes, which count nothing)
                const float4 pl = planes[hb + k];
                const pl_f2 sa = plane_score2(pl, xa, ya, za), sb = plane_score2(pl, xb, yb, zb);
                uint32_t c = (uint32_t)__popcll(__ballot(fabsf(sa.x) < t));
                c += (uint32_t)__popcll(__ballot(fabsf(sa.y) < t));
                c += (uint32_t)__popcll(__ballot(fabsf(sb.x) < t));
                c += (uint32_t)__popcll(__ballot(fabsf(sb.y) < t));
                acc = lane == k ? c : acc;
            }
            if (hb + lane < H) atomicAdd(&cnt[hb + lane], acc);
        }
    }
    __syncthreads();
    for (int h = threadIdx.x; h < H; h += 256) slab[(size_t)blockIdx.x * H + h] = cnt[h];
}

// counts[h] += the column sums of the slab: 64 columns x 16 row lanes per workgroup, the rows dealt over blockIdx.y; the
// workgroups of a column meet in one integer atomic each (counts are zeroed beforehand)
__global__ __launch_bounds__(1024) void k_plane_colsum(const uint32_t *__restrict__ slab, int blocks, int H, unsigned long long *__restrict__ counts)
{
    __shared__ unsigned long long part[16][64];
    const int col = threadIdx.x & 63, r = threadIdx.x >> 6, h = blockIdx.x * 64 + col;
    unsigned long long s = 0ull;
    if (h < H)
        for (int b = blockIdx.y * 16 + r; b < blocks; b += 16 * gridDim.y) s += slab[(size_t)b * H + h];
    part[r][col] = s;
    __syncthreads();
    if (r == 0 && h < H) {
        for (int k = 1; k < 16; ++k) s += part[k][col];
        if (s) atomicAdd(counts + h, s);
    }
}

// arg-max by (count, -h): one workgroup; count < 2^31 and h < 2^12 share one 64-bit key
__global__ __launch_bounds__(1024) void k_plane_best(const unsigned long long *__restrict__ counts, int H, const float4 *__restrict__ planes, long long min_inliers,
                                                      PlaneBest *__restrict__ best)
{
    __shared__ unsigned long long wk[16];
    unsigned long long key = 0ull;
    for (int h = threadIdx.x; h < H; h += 1024) {
        const unsigned long long k = (counts[h] << 12) | (unsigned long long)(PL_MAX_H - 1 - h);
        key = k > key ? k : key;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long other = __shfl_xor(key, o);
        key = other > key ? other : key;
    }
    if ((threadIdx.x & 63u) == 0u) wk[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < 16; ++k) key = wk[k] > key ? wk[k] : key;
    const int h = PL_MAX_H - 1 - (int)(key & (unsigned long long)(PL_MAX_H - 1));
    const float4 pl = planes[h];
    best->index = h;
    best->count = (long long)(key >> 12);
    best->plane[0] = pl.x; best->plane[1] = pl.y; best->plane[2] = pl.z; best->plane[3] = pl.w;
    best->found = best->count >= min_inliers ? 1 : 0;
    best->pad = 0;
}

// the float64 moments of x - c0 over the inliers of the best plane: lane sums in ascending point order, the wave's by a butterfly,
// the workgroup's four in order -> row blockIdx.x of rows[blocks][PL_MOM].  Grid and strides depend on n alone.
__global__ __launch_bounds__(256) void k_plane_moments(const float *__restrict__ xyz, int64_t n, const PlaneBest *__restrict__ best, float t, double *__restrict__ rows)
{
    __shared__ double red[4][PL_MOM];
    const float a = best->plane[0], b = best->plane[1], c = best->plane[2], d = best->plane[3];
    const double cx = -(double)d * (double)a, cy = -(double)d * (double)b, cz = -(double)d * (double)c;
    double s[PL_MOM];
#pragma unroll
    for (int k = 0; k < PL_MOM; ++k) s[k] = 0.0;
    if (best->found) {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
            const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
            if (!plane_hit(a, b, c, d, x, y, z, t)) continue;
            const double dx = (double)x - cx, dy = (double)y - cy, dz = (double)z - cz;
            s[0] += 1.0; s[1] += dx; s[2] += dy; s[3] += dz;
            s[4] += dx * dx; s[5] += dx * dy; s[6] += dx * dz; s[7] += dy * dy; s[8] += dy * dz; s[9] += dz * dz;
        }
    }
#pragma unroll
    for (int k = 0; k < PL_MOM; ++k) {
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) s[k] += __shfl_xor(s[k], o);
    }
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int k = 0; k < PL_MOM; ++k) red[threadIdx.x >> 6][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < PL_MOM) rows[(size_t)blockIdx.x * PL_MOM + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// one workgroup: lane r holds row r (zeros beyond nrows), a fixed tree over the lanes sums them, lane 0 refits and writes the final
// plane.  refine == 0 or nothing found: no rows are read.
__global__ __launch_bounds__(PL_MOM_BLOCKS) void k_plane_refit(const PlaneBest *__restrict__ best, const double *__restrict__ rows, int nrows, int refine,
                                                                PlaneFinal *__restrict__ fin)
{
    __shared__ double T[PL_MOM][PL_MOM_BLOCKS];
    const int found = best->found, r = threadIdx.x;
    const bool read = found && refine && r < nrows;
#pragma unroll
    for (int k = 0; k < PL_MOM; ++k) T[k][r] = read ? rows[(size_t)r * PL_MOM + k] : 0.0;
    __syncthreads();
    for (int o = PL_MOM_BLOCKS / 2; o > 0; o >>= 1) {
        if (r < o) {
#pragma unroll
            for (int k = 0; k < PL_MOM; ++k) T[k][r] += T[k][r + o];
        }
        __syncthreads();
    }
    double S[PL_MOM];
#pragma unroll
    for (int k = 0; k < PL_MOM; ++k) S[k] = T[k][0];
    if (threadIdx.x != 0) return;
    float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int refined = 0;
    if (found) {
        const float a = best->plane[0], b = best->plane[1], c = best->plane[2], d = best->plane[3];
        out[0] = a; out[1] = b; out[2] = c; out[3] = d;
        if (refine && S[0] >= 3.0) {
            const double cnt = S[0], mx = S[1] / cnt, my = S[2] / cnt, mz = S[3] / cnt;
            const double C[9] = {S[4] / cnt - mx * mx, S[5] / cnt - mx * my, S[6] / cnt - mx * mz, S[5] / cnt - mx * my, S[7] / cnt - my * my,
                                 S[8] / cnt - my * mz, S[6] / cnt - mx * mz, S[8] / cnt - my * mz, S[9] / cnt - mz * mz};
            bool ok = true;
            for (int k = 0; k < 9; ++k) ok = ok && isfinite(C[k]);
            if (ok) {
                double nv[3];
                smallest_eigvec(C, nv);
                if (nv[0] * (double)a + nv[1] * (double)b + nv[2] * (double)c < 0.0) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; }
                const double px = -(double)d * (double)a + mx, py = -(double)d * (double)b + my, pz = -(double)d * (double)c + mz;
                const double dd = -(nv[0] * px + nv[1] * py + nv[2] * pz);
                const float r[4] = {(float)nv[0], (float)nv[1], (float)nv[2], (float)dd};
                if (isfinite(r[0]) && isfinite(r[1]) && isfinite(r[2]) && isfinite(r[3])) {
                    out[0] = r[0]; out[1] = r[1]; out[2] = r[2]; out[3] = r[3];
                    refined = 1;
                }
            }
        }
    }
    fin->plane[0] = out[0]; fin->plane[1] = out[1]; fin->plane[2] = out[2]; fin->plane[3] = out[3];
    fin->found = found;
    fin->refined = refined;
    fin->n_inliers = 0ull;
}

// the inliers of the final plane and their number (one integer atomic per workgroup; the grid is capped and strides).  mode 0:
// flags = inlier; 1 / 2: the keep flags of remove_plane, the non-inliers / the inliers, and every point when no plane was found.
__global__ __launch_bounds__(256) void k_plane_flags(const float *__restrict__ xyz, int64_t n, const PlaneFinal *fin, float t, int mode, uint8_t *__restrict__ flags,
                                                      unsigned long long *n_inliers)
{
    __shared__ uint32_t wcnt[4];
    const int found = fin->found;
    const float a = fin->plane[0], b = fin->plane[1], c = fin->plane[2], d = fin->plane[3];
    uint32_t mine = 0u;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) { // (uniform per workgroup)
        const int64_t i = base + threadIdx.x;
        bool in = false;
        if (i < n && found) in = plane_hit(a, b, c, d, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], t);
        mine += in ? 1u : 0u;
        if (i < n) flags[i] = mode == 0 ? (in ? 1 : 0) : (!found || in == (mode == 2)) ? 1 : 0;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63u) == 0u) wcnt[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t total = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        if (total) atomicAdd(n_inliers, (unsigned long long)total);
    }
}

// ---- host side
inline uint64_t plane_mix(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the axis normalised (false: none) -- the caller has checked that it is finite
inline bool plane_axis(const sf_plane_params *p, double ax[3])
{
    const double x = p->axis[0], y = p->axis[1], z = p->axis[2];
    if (x == 0 && y == 0 && z == 0) return false;
    const double nrm = std::sqrt(x * x + y * y + z * z);
    ax[0] = x / nrm; ax[1] = y / nrm; ax[2] = z / nrm;
    return true;
}

// the hypotheses from the gathered samples pts[3H][3]: float64, unfused, left to right; -> the number of degenerate ones
int64_t plane_build(const int32_t *idx, const float *pts, int H, bool has_axis, const double ax[3], double min_cos, float *planes)
{
    int64_t n_deg = 0;
    const float qnan = std::nanf("");
    for (int h = 0; h < H; ++h) {
        const float *q = pts + 9 * (size_t)h;
        float *out = planes + 4 * (size_t)h;
        const int32_t i0 = idx[3 * h], i1 = idx[3 * h + 1], i2 = idx[3 * h + 2];
        const double p0x = q[0], p0y = q[1], p0z = q[2];
        const double ux = (double)q[3] - p0x, uy = (double)q[4] - p0y, uz = (double)q[5] - p0z;
        const double vx = (double)q[6] - p0x, vy = (double)q[7] - p0y, vz = (double)q[8] - p0z;
        const double Nx = uy * vz - uz * vy, Ny = uz * vx - ux * vz, Nz = ux * vy - uy * vx;
        double nn = Nx * Nx;
        nn = nn + Ny * Ny;
        nn = nn + Nz * Nz;
        bool ok = i0 != i1 && i0 != i2 && i1 != i2 && std::isfinite(nn) && nn > 0;
        double nx = 0, ny = 0, nz = 0;
        if (ok) {
            const double len = std::sqrt(nn);
            nx = Nx / len; ny = Ny / len; nz = Nz / len;
            bool flip;
            if (has_axis) {
                double dot = nx * ax[0];
                dot = dot + ny * ax[1];
                dot = dot + nz * ax[2];
                if (std::fabs(dot) < min_cos) ok = false;
                flip = !(dot >= 0);
            } else {
                flip = nz < 0 || (nz == 0 && (ny < 0 || (ny == 0 && nx < 0)));
            }
            if (flip) { nx = -nx; ny = -ny; nz = -nz; }
        }
        if (!ok) {
            out[0] = out[1] = out[2] = out[3] = qnan;
            ++n_deg;
            continue;
        }
        double dd = nx * p0x;
        dd = dd + ny * p0y;
        dd = dd + nz * p0z;
        out[0] = (float)nx; out[1] = (float)ny; out[2] = (float)nz; out[3] = (float)-dd;
    }
    return n_deg;
}

#define SF_CHECK_PLANE(c, p)                                                                                                                                    \
    do {                                                                                                                                                        \
        SF_CHECK((c) && (p), SF_ERR_INVALID, "bad arguments");                                                                                                  \
        SF_CHECK((p)->num_hypotheses >= 1 && (p)->num_hypotheses <= PL_MAX_H, SF_ERR_INVALID, "plane: num_hypotheses must be 1 .. %d (got %d)", PL_MAX_H,       \
                 (int)(p)->num_hypotheses);                                                                                                                     \
        SF_CHECK(std::isfinite((p)->distance_threshold) && (p)->distance_threshold > 0, SF_ERR_INVALID, "plane: distance_threshold must be positive and finite (got %g)", \
                 (p)->distance_threshold);                                                                                                                      \
        SF_CHECK((p)->min_inliers >= 3, SF_ERR_INVALID, "plane: min_inliers must be >= 3 (got %lld)", (long long)(p)->min_inliers);                             \
        SF_CHECK((p)->axis_min_cos >= 0 && (p)->axis_min_cos <= 1, SF_ERR_INVALID, "plane: axis_min_cos must be in [0, 1] (got %g)", (p)->axis_min_cos);        \
        SF_CHECK(std::isfinite((p)->axis[0]) && std::isfinite((p)->axis[1]) && std::isfinite((p)->axis[2]), SF_ERR_INVALID, "plane: the axis must be finite");  \
        SF_CHECK((c)->n < (int64_t(1) << 31), SF_ERR_INVALID, "plane: the cloud must hold fewer than 2^31 points");                                             \
    } while (0)

// everything a call needs on the device, carved from the context's small scratch (16-byte steps)
struct PlaneBufs {
    float4 *planes;     // [H rounded up to 64]: the tail holds NaN planes (k_plane_score runs 64 at a time)
    unsigned long long *counts;  // [H]
    PlaneBest *best;
    PlaneFinal *fin;
    double *rows;       // [PL_MOM_BLOCKS][PL_MOM]
    int32_t *sidx;      // [3H]
    float *spts;        // [3H][3]
    uint32_t *slab;     // [blocks][H]
};

inline int plane_pad(int H) { return (H + 63) & ~63; }

int plane_buffers(sf_ctx *ctx, int H, int blocks, PlaneBufs *b)
{
    const auto up = [](size_t v) { return (v + 15) & ~size_t(15); };
    const size_t sz[8] = {sizeof(float4) * (size_t)plane_pad(H), up(sizeof(long long) * (size_t)H), up(sizeof(PlaneBest)), up(sizeof(PlaneFinal)),
                          up(sizeof(double) * PL_MOM * PL_MOM_BLOCKS), up(sizeof(int32_t) * 3 * (size_t)H), up(sizeof(float) * 9 * (size_t)H),
                          up(sizeof(uint32_t) * (size_t)blocks * (size_t)H)};
    size_t total = 0;
    for (size_t s : sz) total += s;
    SF_TRY(ctx->scratch2.reserve(total));
    char *w = ctx->scratch2.as<char>();
    b->planes = reinterpret_cast<float4 *>(w); w += sz[0];
    b->counts = reinterpret_cast<unsigned long long *>(w); w += sz[1];
    b->best = reinterpret_cast<PlaneBest *>(w); w += sz[2];
    b->fin = reinterpret_cast<PlaneFinal *>(w); w += sz[3];
    b->rows = reinterpret_cast<double *>(w); w += sz[4];
    b->sidx = reinterpret_cast<int32_t *>(w); w += sz[5];
    b->spts = reinterpret_cast<float *>(w); w += sz[6];
    b->slab = reinterpret_cast<uint32_t *>(w);
    return SF_OK;
}

// workgroups of k_plane_score: one per tile up to 8 per compute unit (max_blocks > 0: the test hook's cap)
inline int plane_score_blocks(const sf_ctx *ctx, int64_t n, int max_blocks)
{
    const int64_t ntiles = sf::div_up(n, PL_TILE);
    const int64_t cap = max_blocks > 0 ? max_blocks : 8 * (int64_t)std::max(ctx->prop.multiProcessorCount, 1);
    return (int)std::max<int64_t>(1, std::min(ntiles, cap));
}

// planes (device) -> counts (device): the scoring launches
void plane_score_launch(sf_cloud *c, const PlaneBufs &b, int H, int blocks, float t)
{
    hipStream_t s = c->ctx->stream;
    hipLaunchKernelGGL(k_plane_score, dim3(blocks), dim3(256), 0, s, c->xyz.as<float>(), c->n, b.planes, H, t, b.slab);
    hipError_t e = hipMemsetAsync(b.counts, 0, sizeof(unsigned long long) * (size_t)H, s); // (a failure surfaces at the caller's hipGetLastError / wait)
    (void)e;
    const unsigned split = (unsigned)std::min<int64_t>(16, sf::div_up(blocks, 128));
    hipLaunchKernelGGL(k_plane_colsum, dim3((unsigned)sf::div_up(H, 64), split), dim3(1024), 0, s, b.slab, blocks, H, b.counts);
}

// the samples of every hypothesis, gathered on the device and brought to the host (one wait), and the planes built from them
int plane_hypotheses_host(sf_cloud *c, const sf_plane_params *p, const PlaneBufs &b, std::vector<int32_t> &idx, std::vector<float> &planes, int64_t *n_deg)
{
    sf_ctx *ctx = c->ctx;
    const int H = p->num_hypotheses;
    idx.resize(3 * (size_t)H);
    planes.assign(4 * (size_t)plane_pad(H), std::nanf("")); // with the padding k_plane_score reads
    for (int k = 0; k < 3 * H; ++k) idx[k] = (int32_t)(plane_mix(p->seed + 0x9E3779B97F4A7C15ull * (uint64_t)(k + 1)) % (uint64_t)c->n);
    std::vector<float> pts(9 * (size_t)H);
    SF_TRY(sf::upload_staged(ctx, b.sidx, idx.data(), sizeof(int32_t) * idx.size()));
    hipLaunchKernelGGL(k_plane_gather, dim3(nblk(3 * H)), dim3(256), 0, ctx->stream, c->xyz.as<float>(), b.sidx, 3 * H, b.spts);
    SF_HIP(hipGetLastError());
    SF_HIP(hipMemcpyAsync(pts.data(), b.spts, sizeof(float) * pts.size(), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    double ax[3] = {0, 0, 0};
    const bool has_axis = plane_axis(p, ax);
    *n_deg = plane_build(idx.data(), pts.data(), H, has_axis, ax, p->axis_min_cos, planes.data());
    return SF_OK;
}

struct PlaneEvents { // profile != 0: [0, 3] around everything, [1, 2] around the scoring launches
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool on = false;
    PlaneEvents() = default;
    PlaneEvents(const PlaneEvents &) = delete;
    PlaneEvents &operator=(const PlaneEvents &) = delete;
    void start(bool want)
    {
        if (!want) return;
        on = true;
        for (int i = 0; i < 4; ++i)
            if (hipEventCreate(&ev[i]) != hipSuccess) { ev[i] = nullptr; on = false; }
    }
    void mark(int i, hipStream_t s)
    {
        if (!on) return;
        hipError_t e = hipEventRecord(ev[i], s);
        (void)e;
    }
    float ms(int i, int j) const
    {
        float v = -1.0f;
        if (!on || hipEventElapsedTime(&v, ev[i], ev[j]) != hipSuccess) return -1.0f;
        return v;
    }
    ~PlaneEvents()
    {
        for (int i = 0; i < 4; ++i)
            if (ev[i]) { hipError_t e = hipEventDestroy(ev[i]); (void)e; }
    }
};

// The segmentation proper.  mode as in k_plane_flags; the flags stay in c->flags.  After the hypothesis upload the host waits once,
// at the end (read_words).  inlier (host, [n]) or NULL.  The cloud's points, stamp and last indices are left alone.
int plane_segment_device(sf_cloud *c, const sf_plane_params *p, int mode, float plane[4], uint8_t *inlier, sf_plane_stats *stats)
{
    sf_ctx *ctx = c->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t n = c->n;
    const int H = p->num_hypotheses;
    sf_plane_stats st{};
    st.n_points = n;
    st.score_ms = st.total_ms = -1.0f;
    for (int k = 0; k < 4; ++k) plane[k] = 0.0f;
    if (stats) *stats = st;
    if (n == 0) return SF_OK;
    const float t = (float)p->distance_threshold;
    const int blocks = plane_score_blocks(ctx, n, 0), mom_blocks = (int)std::min<int64_t>(sf::div_up(n, 256), PL_MOM_BLOCKS);
    PlaneBufs b{};
    SF_TRY(plane_buffers(ctx, H, blocks, &b));
    SF_TRY(c->flags.reserve((size_t)n));
    PlaneEvents ev;
    ev.start(p->profile != 0);
    ev.mark(0, s);
    std::vector<int32_t> idx;
    std::vector<float> planes;
    SF_TRY(plane_hypotheses_host(c, p, b, idx, planes, &st.n_degenerate));
    SF_TRY(sf::upload_staged(ctx, b.planes, planes.data(), sizeof(float) * planes.size()));
    ev.mark(1, s);
    plane_score_launch(c, b, H, blocks, t);
    hipLaunchKernelGGL(k_plane_best, dim3(1), dim3(1024), 0, s, b.counts, H, b.planes, (long long)p->min_inliers, b.best);
    ev.mark(2, s);
    if (p->refine) hipLaunchKernelGGL(k_plane_moments, dim3(mom_blocks), dim3(256), 0, s, c->xyz.as<float>(), n, b.best, t, b.rows);
    hipLaunchKernelGGL(k_plane_refit, dim3(1), dim3(PL_MOM_BLOCKS), 0, s, b.best, b.rows, mom_blocks, p->refine ? 1 : 0, b.fin);
    hipLaunchKernelGGL(k_plane_flags, dim3(std::min(nblk(n), 2048u)), dim3(256), 0, s, c->xyz.as<float>(), n, b.fin, t, mode, c->flags.as<uint8_t>(), &b.fin->n_inliers);
    ev.mark(3, s);
    if (inlier) SF_HIP(hipMemcpyAsync(inlier, c->flags.p, (size_t)n, hipMemcpyDeviceToHost, s));
    SF_TRY(read_words(ctx, b.fin, 4, b.best, 2));
    PlaneFinal fin;
    const unsigned long long *h = ctx->h_pinned->readback;
    std::memcpy(&fin, h, sizeof(fin));
    for (int k = 0; k < 4; ++k) plane[k] = fin.plane[k];
    st.n_hypotheses = H;
    st.best_index = (int64_t)h[4];
    st.best_count = (int64_t)h[5];
    st.n_inliers = (int64_t)fin.n_inliers;
    st.found = fin.found;
    st.refined = fin.refined;
    st.score_ms = ev.ms(1, 2);
    st.total_ms = ev.ms(0, 3);
    if (stats) *stats = st;
    return SF_OK;
}

// sf_cloud_score_planes and its test hook
int plane_score_host(sf_cloud *c, const float *planes, int64_t n_planes, double thr, int max_blocks, int64_t *counts)
{
    SF_CHECK(c && planes && counts, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(n_planes >= 1 && n_planes <= PL_MAX_H, SF_ERR_INVALID, "score_planes: n_planes must be 1 .. %d (got %lld)", PL_MAX_H, (long long)n_planes);
    SF_CHECK(std::isfinite(thr) && thr > 0, SF_ERR_INVALID, "score_planes: distance_threshold must be positive and finite (got %g)", thr);
    SF_CHECK(max_blocks >= 0 && max_blocks <= 65536, SF_ERR_INVALID, "score_planes: max_blocks must be 0 .. 65536");
    SF_CHECK(c->n < (int64_t(1) << 31), SF_ERR_INVALID, "plane: the cloud must hold fewer than 2^31 points");
    sf_ctx *ctx = c->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    const int H = (int)n_planes;
    if (c->n == 0) {
        for (int h = 0; h < H; ++h) counts[h] = 0;
        return SF_OK;
    }
    const int blocks = plane_score_blocks(ctx, c->n, max_blocks);
    PlaneBufs b{};
    SF_TRY(plane_buffers(ctx, H, blocks, &b));
    std::vector<float> padded(4 * (size_t)plane_pad(H), std::nanf(""));
    std::memcpy(padded.data(), planes, sizeof(float) * 4 * (size_t)H);
    SF_TRY(sf::upload_staged(ctx, b.planes, padded.data(), sizeof(float) * padded.size()));
    plane_score_launch(c, b, H, blocks, (float)thr);
    SF_HIP(hipGetLastError());
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counts are copied as they are");
    SF_HIP(hipMemcpyAsync(counts, b.counts, sizeof(int64_t) * (size_t)H, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    return SF_OK;
}

} // namespace

extern "C" void sf_plane_default_params(sf_plane_params *p)
{
    if (!p) return;
    *p = sf_plane_params{};
    p->distance_threshold = 0.1;
    p->num_hypotheses = 1024;
    p->refine = 1;
    p->min_inliers = 3;
}

extern "C" int sf_cloud_plane_hypotheses(sf_cloud *c, const sf_plane_params *p, float *planes, int32_t *samples, int64_t *n_degenerate)
{
    SF_CHECK_PLANE(c, p);
    SF_CHECK(planes, SF_ERR_INVALID, "bad arguments");
    const int H = p->num_hypotheses;
    if (c->n == 0) { // nothing to sample: every hypothesis is degenerate
        for (int k = 0; k < 4 * H; ++k) planes[k] = std::nanf("");
        if (samples)
            for (int k = 0; k < 3 * H; ++k) samples[k] = -1;
        if (n_degenerate) *n_degenerate = H;
        return SF_OK;
    }
    sf_ctx *ctx = c->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    PlaneBufs b{};
    SF_TRY(plane_buffers(ctx, H, 1, &b));
    std::vector<int32_t> idx;
    std::vector<float> pl;
    int64_t n_deg = 0;
    SF_TRY(plane_hypotheses_host(c, p, b, idx, pl, &n_deg));
    std::memcpy(planes, pl.data(), sizeof(float) * 4 * (size_t)H);
    if (samples) std::memcpy(samples, idx.data(), sizeof(int32_t) * idx.size());
    if (n_degenerate) *n_degenerate = n_deg;
    return SF_OK;
}

extern "C" int sf_cloud_score_planes(sf_cloud *c, const float *planes, int64_t n_planes, double distance_threshold, int64_t *counts)
{
    return plane_score_host(c, planes, n_planes, distance_threshold, 0, counts);
}

extern "C" int sf_test_plane_score(sf_cloud *c, const float *planes, int64_t n_planes, double t, int max_blocks, int64_t *counts)
{
    return plane_score_host(c, planes, n_planes, t, max_blocks, counts);
}

extern "C" int sf_cloud_segment_plane(sf_cloud *c, const sf_plane_params *p, float plane[4], uint8_t *inlier, sf_plane_stats *stats)
{
    SF_CHECK_PLANE(c, p);
    SF_CHECK(plane, SF_ERR_INVALID, "bad arguments");
    return plane_segment_device(c, p, 0, plane, inlier, stats);
}

extern "C" int sf_cloud_remove_plane(sf_cloud *c, const sf_plane_params *p, int keep_inliers, float plane[4], sf_plane_stats *stats)
{
    SF_CHECK_PLANE(c, p);
    SF_CHECK(plane, SF_ERR_INVALID, "bad arguments");
    sf::cloud_touch(c);
    SF_TRY(plane_segment_device(c, p, keep_inliers ? 2 : 1, plane, nullptr, stats));
    if (c->n == 0) { c->n_last_idx = 0; return SF_OK; }
    return sf::compact_cloud(c, c->flags.as<uint8_t>());
}
