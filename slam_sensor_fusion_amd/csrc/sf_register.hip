// sf_register.hip — RANSAC pose estimation from descriptor matches (extension, no reference code; the rule is in
// include/slamfusion.h and DESIGN §22, restated in tests/reg_ref_np.py).  gfx950 only, wave64.
//
// One call: k_reg_gather packs the m pairs (six coordinates each) -> k_reg_hypotheses builds one hypothesis per lane in float64 ->
// the status-0 ones are compacted behind an exclusive scan (sf_sort.hpp) -> k_reg_score counts survivors x pairs in float32 ->
// k_reg_round (once per candidate) and k_reg_best take the arg-max and the top-K -> refine_rounds x (k_reg_moments, k_reg_refit) -> k_reg_flags, k_reg_finish.  The host
// waits once, at the end.  Integer atomics only; every summation order is fixed by m and the parameters.
#include <cfloat>

#include "sf_register.hpp"
#include "sf_sort.hpp"

namespace {

#include "sf_jacobi.hpp"

using sf::REG_BLOCK;
using sf::REG_MAX_H;
using sf::REG_MAX_TOP;
using sf::REG_MOM_BLOCKS;
using sf::REG_REC;

inline unsigned nblk(int64_t n) { return (unsigned)std::max<int64_t>(sf::div_up(n, REG_BLOCK), 1); }

constexpr unsigned long long REG_GOLDEN = 0x9E3779B97F4A7C15ull;

// the splitmix64 step of the plane segmentation (sf_plane.hpp, plane_mix)
__host__ __device__ __forceinline__ unsigned long long reg_mix(unsigned long long x)
{
    unsigned long long z = x + REG_GOLDEN;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// what the choice leaves for the refit and the final flags, and what the host reads back
struct RegState {
    double T[16];                    // the current transform, row-major
    float Tf[12];                    // its twelve entries rounded to float32: what scores
    double sref[3], tref[3];         // sample 0 of the chosen hypothesis
    double sum_d2;
    long long best, best_count;
    unsigned long long n_inliers, n_deg, n_rej, n_live;
    int32_t found, rounds_done, stopped, n_top;
};
static_assert(sizeof(RegState) % 8 == 0, "copied as it is");

struct RegFlags { uint32_t bad_index, n_live, pad[2]; };
constexpr size_t REG_STAT_BYTES = sizeof(unsigned long long) * (2 + REG_MAX_TOP + 1);

// a pair as k_reg_gather leaves it: a = (sx, sy, sz, tx), b = (ty, tz, 0, 0)
__global__ __launch_bounds__(REG_BLOCK) void k_reg_gather(const float *__restrict__ src, int64_t ns, const float *__restrict__ dst, int64_t nd,
                                                           const int32_t *__restrict__ pairs, int m, float4 *__restrict__ pk, RegFlags *__restrict__ flags)
{
    const int k = blockIdx.x * REG_BLOCK + threadIdx.x;
    if (k >= m) return;
    const int64_t i = pairs[2 * (size_t)k], j = pairs[2 * (size_t)k + 1];
    const float nan = __uint_as_float(0x7fc00000u);
    float4 a = {nan, nan, nan, nan}, b = {nan, nan, 0.0f, 0.0f};
    if (i >= 0 && i < ns && j >= 0 && j < nd) {
        a.x = src[3 * i]; a.y = src[3 * i + 1]; a.z = src[3 * i + 2];
        a.w = dst[3 * j]; b.x = dst[3 * j + 1]; b.y = dst[3 * j + 2];
    } else {
        atomicOr(&flags->bad_index, 1u);
    }
    pk[2 * (size_t)k] = a;
    pk[2 * (size_t)k + 1] = b;
}

// Horn's closed form: S_ab = sum s_a t_b about the centroids cs, ct -> T = [R | ct - R cs].  False: something is not finite.
__device__ __forceinline__ bool reg_horn(const double (&S)[9], const double (&cs)[3], const double (&ct)[3], double (&T)[16])
{
    double N[16], V[16];
    N[0] = (S[0] + S[4]) + S[8];
    N[5] = (S[0] - S[4]) - S[8];
    N[10] = (S[4] - S[0]) - S[8];
    N[15] = (S[8] - S[0]) - S[4];
    N[1] = N[4] = S[5] - S[7];
    N[2] = N[8] = S[6] - S[2];
    N[3] = N[12] = S[1] - S[3];
    N[6] = N[9] = S[1] + S[3];
    N[7] = N[13] = S[6] + S[2];
    N[11] = N[14] = S[5] + S[7];
    jacobi_sym<4>(N, V);
    double lam = N[0], w = V[0], x = V[4], y = V[8], z = V[12];
    if (N[5] > lam) { lam = N[5]; w = V[1]; x = V[5]; y = V[9]; z = V[13]; }
    if (N[10] > lam) { lam = N[10]; w = V[2]; x = V[6]; y = V[10]; z = V[14]; }
    if (N[15] > lam) { lam = N[15]; w = V[3]; x = V[7]; y = V[11]; z = V[15]; }
    const double nrm = sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / nrm; x = x / nrm; y = y / nrm; z = z / nrm;
    if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z;
    const double R[9] = {((ww + xx) - yy) - zz, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                         2.0 * (x * y + w * z), ((ww - xx) + yy) - zz, 2.0 * (y * z - w * x),
                         2.0 * (x * z - w * y), 2.0 * (y * z + w * x), ((ww - xx) - yy) + zz};
    bool ok = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double tr = ct[r] - ((R[3 * r] * cs[0] + R[3 * r + 1] * cs[1]) + R[3 * r + 2] * cs[2]);
        T[4 * r] = R[3 * r]; T[4 * r + 1] = R[3 * r + 1]; T[4 * r + 2] = R[3 * r + 2]; T[4 * r + 3] = tr;
        ok = ok && isfinite(R[3 * r]) && isfinite(R[3 * r + 1]) && isfinite(R[3 * r + 2]) && isfinite(tr);
    }
    T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
    return ok;
}

__device__ __forceinline__ double reg_len2(const double (&a)[3], const double (&b)[3])
{
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    double l = dx * dx;
    l = l + dy * dy;
    l = l + dz * dz;
    return l;
}

// |(b - a) x (c - a)|^2 > 0 and finite
__device__ __forceinline__ bool reg_spans(const double (&a)[3], const double (&b)[3], const double (&c)[3])
{
    const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2], vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    double cc = cx * cx;
    cc = cc + cy * cy;
    cc = cc + cz * cz;
    return cc > 0.0 && isfinite(cc);
}

__device__ __forceinline__ bool reg_edge_ok(double ls2, double lt2, double e2) { return ls2 >= e2 * lt2 && lt2 >= e2 * ls2; }

// One hypothesis per lane, float64.  samples (may be nullptr) [H][3], status [H], live [H] (1: status 0), T [H][16]; stat[0] / [1]
// count the degenerate / the rejected ones (one integer atomic per wave).  jacobi_sym<4> sets the register count.
__global__ __launch_bounds__(REG_BLOCK) void k_reg_hypotheses(const float4 *__restrict__ pk, int m, int H, unsigned long long seed, double e2, int32_t *__restrict__ samples,
                                                               int32_t *__restrict__ status, uint32_t *__restrict__ live, double *__restrict__ T,
                                                               unsigned long long *__restrict__ stat)
{
    const int h = blockIdx.x * REG_BLOCK + threadIdx.x;
    int st = -1;
    if (h < H) {
        int k[3];
        double s[3][3], t[3][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            k[j] = (int)(reg_mix(seed + REG_GOLDEN * (unsigned long long)(3ll * h + j + 1)) % (unsigned long long)m);
            const float4 a = pk[2 * (size_t)k[j]], b = pk[2 * (size_t)k[j] + 1];
            s[j][0] = (double)a.x; s[j][1] = (double)a.y; s[j][2] = (double)a.z;
            t[j][0] = (double)a.w; t[j][1] = (double)b.x; t[j][2] = (double)b.y;
        }
        if (samples) { samples[3 * (size_t)h] = k[0]; samples[3 * (size_t)h + 1] = k[1]; samples[3 * (size_t)h + 2] = k[2]; }
        double out[16];
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
        for (int i = 0; i < 16; ++i) out[i] = nan;
        st = 0;
        if (k[0] == k[1] || k[0] == k[2] || k[1] == k[2] || !reg_spans(s[0], s[1], s[2]) || !reg_spans(t[0], t[1], t[2])) st = 1;
        if (st == 0 && e2 > 0.0) {
            const bool ok = reg_edge_ok(reg_len2(s[0], s[1]), reg_len2(t[0], t[1]), e2) && reg_edge_ok(reg_len2(s[0], s[2]), reg_len2(t[0], t[2]), e2) &&
                            reg_edge_ok(reg_len2(s[1], s[2]), reg_len2(t[1], t[2]), e2);
            if (!ok) st = 2;
        }
        if (st == 0) {
            double cs[3], ct[3], S[9];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                cs[a] = ((s[0][a] + s[1][a]) + s[2][a]) / 3.0;
                ct[a] = ((t[0][a] + t[1][a]) + t[2][a]) / 3.0;
            }
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    double v = (s[0][a] - cs[a]) * (t[0][b] - ct[b]);
                    v = v + (s[1][a] - cs[a]) * (t[1][b] - ct[b]);
                    v = v + (s[2][a] - cs[a]) * (t[2][b] - ct[b]);
                    S[3 * a + b] = v;
                }
            double Th[16];
            if (reg_horn(S, cs, ct, Th)) {
#pragma unroll
                for (int i = 0; i < 16; ++i) out[i] = Th[i];
            } else {
                st = 1;
            }
        }
        status[h] = st;
        live[h] = st == 0 ? 1u : 0u;
#pragma unroll
        for (int i = 0; i < 16; ++i) T[16 * (size_t)h + i] = out[i];
    }
    const unsigned long long deg = __ballot(st == 1), rej = __ballot(st == 2);
    if ((threadIdx.x & 63u) == 0u) {
        if (deg) atomicAdd(stat, (unsigned long long)__popcll(deg));
        if (rej) atomicAdd(stat + 1, (unsigned long long)__popcll(rej));
    }
}

// the status-0 hypotheses in ascending h: slot pos[h] gets the float32 transform and h; the lane of the last h leaves their number
__global__ __launch_bounds__(REG_BLOCK) void k_reg_compact(const uint32_t *__restrict__ live, const uint32_t *__restrict__ pos, const double *__restrict__ T, int H,
                                                            float *__restrict__ Tf, int32_t *__restrict__ hid, RegFlags *__restrict__ flags)
{
    const int h = blockIdx.x * REG_BLOCK + threadIdx.x;
    if (h >= H) return;
    const uint32_t on = live[h], s = pos[h];
    if (h == H - 1) flags->n_live = s + on;
    if (!on) return;
#pragma unroll
    for (int i = 0; i < 12; ++i) Tf[12 * (size_t)s + i] = (float)T[16 * (size_t)h + i];
    hid[s] = h;
}

// the score rule on one pair: four statements per coordinate and three for the distance, unfused (-ffp-contract=off)
__device__ __forceinline__ bool reg_hit(const float (&c)[12], float x, float y, float z, float tx, float ty, float tz, float t2, float *d2_out = nullptr)
{
    float qx = c[0] * x;
    qx = qx + c[1] * y;
    qx = qx + c[2] * z;
    qx = qx + c[3];
    float qy = c[4] * x;
    qy = qy + c[5] * y;
    qy = qy + c[6] * z;
    qy = qy + c[7];
    float qz = c[8] * x;
    qz = qz + c[9] * y;
    qz = qz + c[10] * z;
    qz = qz + c[11];
    const float dx = qx - tx, dy = qy - ty, dz = qz - tz;
    float d2 = dx * dx;
    d2 = d2 + dy * dy;
    d2 = d2 + dz * dz;
    if (d2_out) *d2_out = d2;
    return d2 < t2;
}

// Transforms x pairs, the hot path: a transform per lane, its twelve coefficients in VGPRs, the count in a register; the packed
// pairs are read at wave-uniform addresses (scalar loads), so every VALU instruction takes one SGPR operand at most.  The grid is
// one-dimensional and cut on the device, because only the device knows how many transforms there are (n_live; nullptr: H):
// workgroup b takes the 256 transforms of column b mod gx and the pairs of slice b / gx.  fix_gx > 0 (the test hook): gx and the
// slice length chunk are given.  Otherwise, with nb = the columns the transforms fill: more columns than workgroups -- one slice,
// the workgroups stride over the columns; fewer -- the pairs are split into as many slices as there are workgroups per column
// (of at least REG_MIN_CHUNK pairs, a multiple of 8), so that few survivors still fill the chip.  The slices of a transform meet
// in one integer atomic each (counts are zeroed beforehand): the result does not depend on the cut.
__global__ __launch_bounds__(REG_BLOCK) void k_reg_score(const float4 *__restrict__ pk, int m, const float *__restrict__ Tf, const uint32_t *__restrict__ n_live, int H, float t2,
                                                          int fix_gx, int64_t chunk, unsigned long long *__restrict__ counts)
{
    const int64_t n = n_live ? (int64_t)*n_live : (int64_t)H;
    int64_t gx = fix_gx, slices = ((int64_t)gridDim.x + gx - 1) / (gx > 0 ? gx : 1);
    if (fix_gx <= 0) {
        const int64_t nb = (n + REG_BLOCK - 1) / REG_BLOCK, G = gridDim.x;
        if (nb >= G) {
            gx = G; slices = 1;
        } else {
            gx = nb > 0 ? nb : 1;
            const int64_t most = m / sf::REG_MIN_CHUNK > 0 ? m / sf::REG_MIN_CHUNK : 1;
            slices = G / gx < most ? G / gx : most;
        }
        chunk = ((m + slices - 1) / slices + 7) & ~int64_t(7);
    }
    const int64_t col = (int64_t)blockIdx.x % gx, y = (int64_t)blockIdx.x / gx;
    const int64_t k0 = y * chunk;
    if (y >= slices || k0 >= (int64_t)m) return;
    const int k1 = (int)(k0 + chunk < (int64_t)m ? k0 + chunk : (int64_t)m);
    for (int64_t base = col * REG_BLOCK; base < n; base += gx * REG_BLOCK) { // (uniform per workgroup)
        const int64_t h = base + threadIdx.x;
        const bool on = h < n;
        const float4 *tp = reinterpret_cast<const float4 *>(Tf + 12 * (size_t)(on ? h : base));
        const float4 r0 = tp[0], r1 = tp[1], r2 = tp[2];
        const float c[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
        uint32_t cnt = 0u;
#pragma unroll 4
        for (int k = (int)k0; k < k1; ++k) {
            const float4 a = pk[2 * (size_t)k], b = pk[2 * (size_t)k + 1];
            cnt += reg_hit(c, a.x, a.y, a.z, a.w, b.x, b.y, t2) ? 1u : 0u;
        }
        if (on && cnt) atomicAdd(counts + h, (unsigned long long)cnt);
    }
}

// Round r of the choice: the largest key below the key of round r - 1 (round 0: the largest), over the whole grid; the workgroups
// meet in one 64-bit integer atomic each.  count < 2^31 and h < 2^20 share the key (count, -h), keys are distinct, a count of 0 is no
// candidate.  slot[r] is zeroed beforehand; once a round finds nothing the later ones leave at once.
__global__ __launch_bounds__(REG_BLOCK) void k_reg_round(const unsigned long long *__restrict__ counts, const int32_t *__restrict__ hid, const RegFlags *__restrict__ flags,
                                                          unsigned long long *slot, int r)
{
    __shared__ unsigned long long wk[4];
    const int n = (int)flags->n_live;
    const unsigned long long below = r > 0 ? slot[r - 1] : ~0ull;
    if (below == 0ull) return; // (uniform)
    unsigned long long key = 0ull;
    for (int64_t s = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x; s < n; s += (int64_t)gridDim.x * REG_BLOCK) {
        const unsigned long long c = counts[s];
        const unsigned long long kk = c ? (c << 20) | (unsigned long long)(REG_MAX_H - 1 - hid[s]) : 0ull;
        key = kk < below && kk > key ? kk : key;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long other = __shfl_xor(key, o);
        key = other > key ? other : key;
    }
    if ((threadIdx.x & 63u) == 0u) wk[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < 4; ++k) key = wk[k] > key ? wk[k] : key;
    if (key) atomicMax(slot + r, key);
}

// the choice from the rounds' keys: the winner (all counts 0: h = 0), the top list, and the state the refit starts from; one wave
__global__ __launch_bounds__(64) void k_reg_best(const unsigned long long *__restrict__ slot, const double *__restrict__ T, const float4 *__restrict__ pk, int m,
                                                  unsigned long long seed, long long min_inliers, int top_k, const unsigned long long *__restrict__ stat,
                                                  const RegFlags *__restrict__ flags, RegState *__restrict__ state, sf_reg_candidate *__restrict__ top)
{
    int n_top = 0;
    for (int r = 0; r < top_k; ++r) { // (uniform)
        const unsigned long long key = slot[r];
        if (key == 0ull) break;
        const int h = REG_MAX_H - 1 - (int)(key & (unsigned long long)(REG_MAX_H - 1));
        if (threadIdx.x < 16) top[r].T[threadIdx.x] = T[16 * (size_t)h + threadIdx.x];
        if (threadIdx.x == 0) { top[r].h = h; top[r].status = 0; top[r].count = (long long)(key >> 20); }
        n_top = r + 1;
    }
    if (threadIdx.x != 0) return;
    const unsigned long long first = slot[0];
    const long long count = (long long)(first >> 20);
    const int h = count > 0 ? REG_MAX_H - 1 - (int)(first & (unsigned long long)(REG_MAX_H - 1)) : 0;
    const int found = count >= min_inliers ? 1 : 0;
    for (int i = 0; i < 16; ++i) state->T[i] = found ? T[16 * (size_t)h + i] : (i % 5 == 0 ? 1.0 : 0.0);
    for (int i = 0; i < 12; ++i) state->Tf[i] = (float)state->T[i];
    const int k = (int)(reg_mix(seed + REG_GOLDEN * (unsigned long long)(3ll * h + 1)) % (unsigned long long)m);
    const float4 a = pk[2 * (size_t)k], b = pk[2 * (size_t)k + 1];
    state->sref[0] = (double)a.x; state->sref[1] = (double)a.y; state->sref[2] = (double)a.z;
    state->tref[0] = (double)a.w; state->tref[1] = (double)b.x; state->tref[2] = (double)b.y;
    state->sum_d2 = 0.0;
    state->best = h;
    state->best_count = count;
    state->n_inliers = 0ull;
    state->n_deg = stat[0];
    state->n_rej = stat[1];
    state->n_live = (unsigned long long)flags->n_live;
    state->found = found;
    state->rounds_done = 0;
    state->stopped = found ? 0 : 1;
    state->n_top = n_top;
}

// the float64 record of the inliers of the current transform: lane sums in ascending pair order, the wave's by a butterfly, the
// workgroup's four in order -> row blockIdx.x of rows[blocks][REG_REC].  Grid and strides depend on m alone.
__global__ __launch_bounds__(REG_BLOCK) void k_reg_moments(const float4 *__restrict__ pk, int m, const RegState *__restrict__ state, float t2, double *__restrict__ rows)
{
    __shared__ double red[4][REG_REC];
    double s[REG_REC];
#pragma unroll
    for (int k = 0; k < REG_REC; ++k) s[k] = 0.0;
    if (!state->stopped) {
        float c[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) c[i] = state->Tf[i];
        const double rs[3] = {state->sref[0], state->sref[1], state->sref[2]}, rt[3] = {state->tref[0], state->tref[1], state->tref[2]};
        for (int64_t k = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x; k < m; k += (int64_t)gridDim.x * REG_BLOCK) {
            const float4 a = pk[2 * (size_t)k], b = pk[2 * (size_t)k + 1];
            if (!reg_hit(c, a.x, a.y, a.z, a.w, b.x, b.y, t2)) continue;
            const double p[3] = {(double)a.x - rs[0], (double)a.y - rs[1], (double)a.z - rs[2]};
            const double q[3] = {(double)a.w - rt[0], (double)b.x - rt[1], (double)b.y - rt[2]};
            s[0] += 1.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                s[1 + i] += p[i];
                s[4 + i] += q[i];
#pragma unroll
                for (int j = 0; j < 3; ++j) s[7 + 3 * i + j] += p[i] * q[j];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < REG_REC; ++k) {
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) s[k] += __shfl_xor(s[k], o);
    }
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int k = 0; k < REG_REC; ++k) red[threadIdx.x >> 6][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < REG_REC) rows[(size_t)blockIdx.x * REG_REC + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// one workgroup: lane r holds row r (zeros beyond nrows), a fixed tree over the lanes sums them, lane 0 solves and, when the
// result stands, replaces the transform; otherwise the rounds end
__global__ __launch_bounds__(REG_MOM_BLOCKS) void k_reg_refit(RegState *__restrict__ state, const double *__restrict__ rows, int nrows)
{
    __shared__ double A[REG_REC][REG_MOM_BLOCKS];
    const int r = threadIdx.x;
    const bool read = !state->stopped && r < nrows;
#pragma unroll
    for (int k = 0; k < REG_REC; ++k) A[k][r] = read ? rows[(size_t)r * REG_REC + k] : 0.0;
    __syncthreads();
    for (int o = REG_MOM_BLOCKS / 2; o > 0; o >>= 1) {
        if (r < o) {
#pragma unroll
            for (int k = 0; k < REG_REC; ++k) A[k][r] += A[k][r + o];
        }
        __syncthreads();
    }
    if (r != 0 || state->stopped) return;
    double M[REG_REC];
#pragma unroll
    for (int k = 0; k < REG_REC; ++k) M[k] = A[k][0];
    const double n = M[0];
    bool ok = n >= 3.0;
    double Tn[16];
    if (ok) {
        double cs[3], ct[3], S[9];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            cs[a] = state->sref[a] + M[1 + a] / n;
            ct[a] = state->tref[a] + M[4 + a] / n;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) S[3 * a + b] = M[7 + 3 * a + b] - M[1 + a] * M[4 + b] / n;
        ok = reg_horn(S, cs, ct, Tn);
    }
    if (!ok) { state->stopped = 1; return; }
    for (int i = 0; i < 16; ++i) state->T[i] = Tn[i];
    for (int i = 0; i < 12; ++i) state->Tf[i] = (float)Tn[i];
    state->rounds_done = state->rounds_done + 1;
}

// the inliers of the final transform, their number (one integer atomic per workgroup) and the tile's sum of (double)d2: one tile of
// 256 consecutive pairs per workgroup, a balanced tree within each 64 (the butterfly), the four 64s left to right
__global__ __launch_bounds__(REG_BLOCK) void k_reg_flags(const float4 *__restrict__ pk, int m, RegState *state, float t2, uint8_t *__restrict__ inlier,
                                                          double *__restrict__ tile_sum)
{
    __shared__ double wsum[4];
    __shared__ uint32_t wcnt[4];
    const int64_t k = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x;
    bool in = false;
    double d = 0.0;
    if (k < m && state->found) {
        float c[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) c[i] = state->Tf[i];
        const float4 a = pk[2 * (size_t)k], b = pk[2 * (size_t)k + 1];
        float d2 = 0.0f;
        in = reg_hit(c, a.x, a.y, a.z, a.w, b.x, b.y, t2, &d2);
        d = in ? (double)d2 : 0.0;
    }
    if (k < m) inlier[k] = in ? 1 : 0;
    uint32_t mine = in ? 1u : 0u;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        mine += __shfl_xor(mine, o);
        d += __shfl_xor(d, o);
    }
    if ((threadIdx.x & 63u) == 0u) { wcnt[threadIdx.x >> 6] = mine; wsum[threadIdx.x >> 6] = d; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t total = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        if (total) atomicAdd(&state->n_inliers, (unsigned long long)total);
        tile_sum[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    }
}

// the tiles' sums in ascending order, by one lane
__global__ void k_reg_finish(RegState *__restrict__ state, const double *__restrict__ tile_sum, int tiles)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int b = 0; b < tiles; ++b) s += tile_sum[b];
    state->sum_d2 = s;
}

// ---- host side
struct Events { // profile != 0: hipEvents at the marks; the times are read after the stream was synchronised
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool on = false;
    Events() = default;
    Events(const Events &) = delete;
    Events &operator=(const Events &) = delete;
    ~Events()
    {
        for (hipEvent_t e : ev)
            if (e) { hipError_t rc = hipEventDestroy(e); (void)rc; }
    }
    int start(bool want)
    {
        if (!want) return SF_OK;
        for (hipEvent_t &e : ev) SF_HIP(hipEventCreate(&e));
        on = true;
        return SF_OK;
    }
    int mark(int i, hipStream_t s)
    {
        if (on) SF_HIP(hipEventRecord(ev[i], s));
        return SF_OK;
    }
    int ms(int a, int b, float *out)
    {
        *out = -1.0f;
        if (on) SF_HIP(hipEventElapsedTime(out, ev[a], ev[b]));
        return SF_OK;
    }
};

// everything a call needs on the device, carved from one allocation of the call's own (256-byte steps)
struct RegBufs {
    sf::DevBuf mem;
    int32_t *pairs = nullptr;             // [m][2]
    float4 *pk = nullptr;                 // [m][2]
    RegFlags *flags = nullptr;
    unsigned long long *stat = nullptr, *slot = nullptr; // [2]: degenerate, rejected; [REG_MAX_TOP + 1]: the keys of the choice's rounds
    int32_t *samples = nullptr, *status = nullptr, *hid = nullptr; // [H][3], [H], [H]
    uint32_t *live = nullptr, *pos = nullptr;                       // [H], [H]
    double *T = nullptr;                  // [H][16]
    float *Tf = nullptr;                  // [H][12]
    unsigned long long *counts = nullptr; // [H]
    RegState *state = nullptr;
    sf_reg_candidate *top = nullptr;      // [REG_MAX_TOP]
    double *rows = nullptr, *tile_sum = nullptr; // [REG_MOM_BLOCKS][REG_REC], [tiles]
    uint8_t *inlier = nullptr;            // [m]

    // hyp: the hypothesis stages are wanted (H hypotheses); score: Tf and counts for H transforms; fit: the choice and the refit
    int reserve(int64_t m, int64_t H, bool hyp, bool score, bool fit)
    {
        const auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
        const size_t um = (size_t)m, uH = (size_t)H, tiles = (size_t)sf::div_up(std::max<int64_t>(m, 1), REG_BLOCK);
        const size_t sz[16] = {up(8 * um), up(32 * um), up(sizeof(RegFlags)), up(REG_STAT_BYTES),
                               hyp ? up(12 * uH) : 0, hyp ? up(4 * uH) : 0, hyp ? up(4 * uH) : 0, hyp ? up(4 * uH) : 0, hyp ? up(4 * uH) : 0, hyp ? up(128 * uH) : 0,
                               score ? up(48 * uH) : 0, score ? up(8 * uH) : 0,
                               fit ? up(sizeof(RegState)) : 0, fit ? up(sizeof(sf_reg_candidate) * REG_MAX_TOP) : 0,
                               fit ? up(sizeof(double) * REG_REC * REG_MOM_BLOCKS) + up(8 * tiles) : 0, fit ? up(um) : 0};
        size_t total = 0;
        for (size_t s : sz) total += s;
        SF_TRY(mem.reserve(total));
        char *w = mem.as<char>();
        const auto take = [&w](size_t bytes) { char *p = w; w += bytes; return p; };
        pairs = reinterpret_cast<int32_t *>(take(sz[0]));
        pk = reinterpret_cast<float4 *>(take(sz[1]));
        flags = reinterpret_cast<RegFlags *>(take(sz[2]));
        stat = reinterpret_cast<unsigned long long *>(take(sz[3]));
        slot = stat + 2;
        samples = reinterpret_cast<int32_t *>(take(sz[4]));
        status = reinterpret_cast<int32_t *>(take(sz[5]));
        hid = reinterpret_cast<int32_t *>(take(sz[6]));
        live = reinterpret_cast<uint32_t *>(take(sz[7]));
        pos = reinterpret_cast<uint32_t *>(take(sz[8]));
        T = reinterpret_cast<double *>(take(sz[9]));
        Tf = reinterpret_cast<float *>(take(sz[10]));
        counts = reinterpret_cast<unsigned long long *>(take(sz[11]));
        state = reinterpret_cast<RegState *>(take(sz[12]));
        top = reinterpret_cast<sf_reg_candidate *>(take(sz[13]));
        rows = reinterpret_cast<double *>(take(sz[14]));
        tile_sum = rows + REG_REC * REG_MOM_BLOCKS;
        inlier = reinterpret_cast<uint8_t *>(take(sz[15]));
        return SF_OK;
    }
};

int check_pairs(const sf_cloud *src, const sf_cloud *dst, const int32_t *pairs, int64_t m, double thr)
{
    SF_CHECK(src && dst, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(src->ctx == dst->ctx, SF_ERR_INVALID, "register: the two clouds belong to different contexts");
    SF_CHECK(m >= 0 && m < (int64_t(1) << 31), SF_ERR_INVALID, "register: m must be 0 .. 2^31 - 1 (got %lld)", (long long)m);
    SF_CHECK(pairs || m == 0, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(std::isfinite(thr) && thr > 0, SF_ERR_INVALID, "register: distance_threshold must be positive and finite (got %g)", thr);
    return SF_OK;
}

int check_params(const sf_reg_params *p)
{
    SF_CHECK(p, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(p->num_hypotheses >= 1 && p->num_hypotheses <= REG_MAX_H, SF_ERR_INVALID, "register: num_hypotheses must be 1 .. %d (got %d)", REG_MAX_H, (int)p->num_hypotheses);
    SF_CHECK(p->refine_rounds >= 0 && p->refine_rounds <= sf::REG_MAX_ROUNDS, SF_ERR_INVALID, "register: refine_rounds must be 0 .. %d (got %d)", sf::REG_MAX_ROUNDS,
             (int)p->refine_rounds);
    SF_CHECK(p->min_inliers >= 3, SF_ERR_INVALID, "register: min_inliers must be >= 3 (got %lld)", (long long)p->min_inliers);
    SF_CHECK(p->top_k >= 0 && p->top_k <= REG_MAX_TOP, SF_ERR_INVALID, "register: top_k must be 0 .. %d (got %d)", REG_MAX_TOP, (int)p->top_k);
    SF_CHECK(!std::isnan(p->edge_similarity) && p->edge_similarity <= 1.0, SF_ERR_INVALID, "register: edge_similarity must be <= 0 (no check) or in (0, 1] (got %g)",
             p->edge_similarity);
    return SF_OK;
}

// pairs (host) -> pk (device), the flag of an index out of range raised; enqueue only
int gather_enqueue(sf_cloud *src, sf_cloud *dst, const int32_t *pairs, int64_t m, RegBufs &B)
{
    sf_ctx *ctx = src->ctx;
    SF_HIP(hipMemsetAsync(B.flags, 0, sizeof(RegFlags), ctx->stream));
    SF_HIP(hipMemsetAsync(B.stat, 0, REG_STAT_BYTES, ctx->stream));
    SF_TRY(sf::upload_staged(ctx, B.pairs, pairs, sizeof(int32_t) * 2 * (size_t)m));
    hipLaunchKernelGGL(k_reg_gather, dim3(nblk(m)), dim3(REG_BLOCK), 0, ctx->stream, src->xyz.as<float>(), src->n, dst->xyz.as<float>(), dst->n, B.pairs, (int)m, B.pk, B.flags);
    SF_HIP(hipGetLastError());
    return SF_OK;
}

int hypotheses_enqueue(sf_ctx *ctx, const sf_reg_params *p, int64_t m, RegBufs &B, bool want_samples)
{
    const int H = p->num_hypotheses;
    const double e2 = p->edge_similarity > 0.0 ? p->edge_similarity * p->edge_similarity : 0.0;
    hipLaunchKernelGGL(k_reg_hypotheses, dim3(nblk(H)), dim3(REG_BLOCK), 0, ctx->stream, B.pk, (int)m, H, (unsigned long long)p->seed, e2, want_samples ? B.samples : (int32_t *)nullptr,
                       B.status, B.live, B.T, B.stat);
    SF_HIP(hipGetLastError());
    return SF_OK;
}

// Tf [n] (n on the device when n_live is given, never more than H) x the m pairs -> counts; enqueue only.  max_blocks / pair_chunk:
// the test hook's cut (either > 0: columns capped at max_blocks, slices of pair_chunk, the other as reg_pair_chunk / H give it);
// both 0: 16 workgroups a compute unit at most, cut on the device.
int score_enqueue(sf_ctx *ctx, int64_t m, int64_t H, const uint32_t *n_live, int max_blocks, int64_t pair_chunk, float t2, RegBufs &B)
{
    SF_HIP(hipMemsetAsync(B.counts, 0, sizeof(unsigned long long) * (size_t)H, ctx->stream));
    int64_t grid = 0, chunk = 0;
    int fix_gx = 0;
    if (max_blocks > 0 || pair_chunk > 0) {
        chunk = sf::reg_pair_chunk(m, pair_chunk);
        fix_gx = (int)nblk(H);
        if (max_blocks > 0) fix_gx = std::min(fix_gx, max_blocks);
        grid = (int64_t)fix_gx * std::max<int64_t>(sf::div_up(m, chunk), 1);
    } else {
        const int64_t cap = 16 * (int64_t)std::max(ctx->prop.multiProcessorCount, 1);
        grid = std::min<int64_t>(cap, (int64_t)nblk(H) * std::max<int64_t>(m / sf::REG_MIN_CHUNK, 1));
    }
    hipLaunchKernelGGL(k_reg_score, dim3((unsigned)grid), dim3(REG_BLOCK), 0, ctx->stream, B.pk, (int)m, B.Tf, n_live, (int)H, t2, fix_gx, chunk, B.counts);
    SF_HIP(hipGetLastError());
    return SF_OK;
}

int score_poses_host(sf_cloud *src, sf_cloud *dst, const int32_t *pairs, int64_t m, const float *T12, int64_t n_poses, double thr, int max_blocks, int64_t pair_chunk,
                     int64_t *counts)
{
    SF_TRY(check_pairs(src, dst, pairs, m, thr));
    SF_CHECK(T12 && counts, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(n_poses >= 1 && n_poses <= REG_MAX_H, SF_ERR_INVALID, "score_poses: n_poses must be 1 .. %d (got %lld)", REG_MAX_H, (long long)n_poses);
    SF_CHECK(max_blocks >= 0 && max_blocks <= 65536 && pair_chunk >= 0, SF_ERR_INVALID, "score_poses: max_blocks must be 0 .. 65536 and pair_chunk >= 0");
    if (m == 0 || src->n == 0 || dst->n == 0) {
        for (int64_t h = 0; h < n_poses; ++h) counts[h] = 0;
        return SF_OK;
    }
    sf_ctx *ctx = src->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    RegBufs B;
    SF_TRY(B.reserve(m, n_poses, false, true, false));
    SF_TRY(gather_enqueue(src, dst, pairs, m, B));
    SF_TRY(sf::upload_staged(ctx, B.Tf, T12, sizeof(float) * 12 * (size_t)n_poses));
    SF_TRY(score_enqueue(ctx, m, n_poses, nullptr, max_blocks, pair_chunk, (float)(thr * thr), B));
    std::vector<int64_t> got((size_t)n_poses);
    RegFlags fl{};
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counts are copied as they are");
    SF_HIP(hipMemcpyAsync(got.data(), B.counts, sizeof(int64_t) * (size_t)n_poses, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipMemcpyAsync(&fl, B.flags, sizeof(fl), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    SF_CHECK(!fl.bad_index, SF_ERR_INVALID, "register: a pair holds an index outside its cloud");
    std::memcpy(counts, got.data(), sizeof(int64_t) * (size_t)n_poses);
    return SF_OK;
}

} // namespace

extern "C" void sf_reg_default_params(sf_reg_params *p)
{
    if (!p) return;
    *p = sf_reg_params{};
    p->edge_similarity = 0.9;
    p->num_hypotheses = 4096;
    p->refine_rounds = 2;
    p->min_inliers = 3;
}

extern "C" int sf_cloud_pair_hypotheses(sf_cloud *src, sf_cloud *dst, const int32_t *pairs, int64_t m, const sf_reg_params *p, int32_t *samples, int32_t *status, double *T)
{
    SF_TRY(check_params(p));
    SF_TRY(check_pairs(src, dst, pairs, m, p->distance_threshold));
    SF_CHECK(status, SF_ERR_INVALID, "bad arguments");
    const int64_t H = p->num_hypotheses;
    const bool none = src->n == 0 || dst->n == 0;
    sf_ctx *ctx = src->ctx;
    RegBufs B;
    RegFlags fl{};
    if (m > 0 && !none) {
        SF_HIP(hipSetDevice(ctx->device));
        SF_TRY(B.reserve(m, H, m >= 3, false, false));
        SF_TRY(gather_enqueue(src, dst, pairs, m, B));
        if (m < 3) {
            SF_HIP(hipMemcpyAsync(&fl, B.flags, sizeof(fl), hipMemcpyDeviceToHost, ctx->stream));
            SF_HIP(hipStreamSynchronize(ctx->stream));
            SF_CHECK(!fl.bad_index, SF_ERR_INVALID, "register: a pair holds an index outside its cloud");
        }
    }
    if (m < 3 || none) { // nothing to sample: every hypothesis is degenerate
        for (int64_t h = 0; h < H; ++h) status[h] = 1;
        if (samples)
            for (int64_t k = 0; k < 3 * H; ++k) samples[k] = -1;
        if (T)
            for (int64_t k = 0; k < 16 * H; ++k) T[k] = std::nan("");
        return SF_OK;
    }
    SF_TRY(hypotheses_enqueue(ctx, p, m, B, true));
    std::vector<int32_t> h_status((size_t)H), h_samples(samples ? 3 * (size_t)H : 0);
    std::vector<double> h_T(T ? 16 * (size_t)H : 0);
    hipStream_t s = ctx->stream;
    SF_HIP(hipMemcpyAsync(h_status.data(), B.status, sizeof(int32_t) * (size_t)H, hipMemcpyDeviceToHost, s));
    if (samples) SF_HIP(hipMemcpyAsync(h_samples.data(), B.samples, sizeof(int32_t) * 3 * (size_t)H, hipMemcpyDeviceToHost, s));
    if (T) SF_HIP(hipMemcpyAsync(h_T.data(), B.T, sizeof(double) * 16 * (size_t)H, hipMemcpyDeviceToHost, s));
    SF_HIP(hipMemcpyAsync(&fl, B.flags, sizeof(fl), hipMemcpyDeviceToHost, s));
    SF_HIP(hipStreamSynchronize(s));
    SF_CHECK(!fl.bad_index, SF_ERR_INVALID, "register: a pair holds an index outside its cloud");
    std::memcpy(status, h_status.data(), sizeof(int32_t) * (size_t)H);
    if (samples) std::memcpy(samples, h_samples.data(), sizeof(int32_t) * 3 * (size_t)H);
    if (T) std::memcpy(T, h_T.data(), sizeof(double) * 16 * (size_t)H);
    return SF_OK;
}

extern "C" int sf_cloud_score_poses(sf_cloud *src, sf_cloud *dst, const int32_t *pairs, int64_t m, const float *T12, int64_t n_poses, double distance_threshold,
                                    int64_t *counts)
{
    return score_poses_host(src, dst, pairs, m, T12, n_poses, distance_threshold, 0, 0, counts);
}

extern "C" int sf_test_score_poses(sf_cloud *src, sf_cloud *dst, const int32_t *pairs, int64_t m, const float *T12, int64_t n_poses, double distance_threshold, int max_blocks,
                                   int64_t pair_chunk, int64_t *counts)
{
    return score_poses_host(src, dst, pairs, m, T12, n_poses, distance_threshold, max_blocks, pair_chunk, counts);
}

extern "C" int sf_cloud_register_pairs(sf_cloud *src, sf_cloud *dst, const int32_t *pairs, int64_t m, const sf_reg_params *p, double *T, uint8_t *inlier,
                                       sf_reg_candidate *top, sf_reg_stats *stats)
{
    SF_TRY(check_params(p));
    SF_TRY(check_pairs(src, dst, pairs, m, p->distance_threshold));
    SF_CHECK(T && (top || p->top_k == 0), SF_ERR_INVALID, "bad arguments");
    sf_ctx *ctx = src->ctx;
    hipStream_t s = ctx->stream;
    const int64_t H = p->num_hypotheses;
    const bool none = src->n == 0 || dst->n == 0;
    sf_reg_stats st{};
    st.hyp_ms = st.score_ms = st.refit_ms = -1.0f;
    double Tout[16];
    for (int i = 0; i < 16; ++i) Tout[i] = i % 5 == 0 ? 1.0 : 0.0;
    RegBufs B;
    RegFlags fl{};
    if (m == 0 || none || m < 3) {
        if (m > 0 && !none) { // the indices are still checked
            SF_HIP(hipSetDevice(ctx->device));
            SF_TRY(B.reserve(m, H, false, false, false));
            SF_TRY(gather_enqueue(src, dst, pairs, m, B));
            SF_HIP(hipMemcpyAsync(&fl, B.flags, sizeof(fl), hipMemcpyDeviceToHost, s));
            SF_HIP(hipStreamSynchronize(s));
            SF_CHECK(!fl.bad_index, SF_ERR_INVALID, "register: a pair holds an index outside its cloud");
        }
        std::memcpy(T, Tout, sizeof(Tout));
        if (inlier) std::memset(inlier, 0, (size_t)m);
        if (stats) *stats = st;
        return SF_OK;
    }
    SF_HIP(hipSetDevice(ctx->device));
    SF_TRY(B.reserve(m, H, true, true, true));
    const float t2 = (float)(p->distance_threshold * p->distance_threshold);
    const int tiles = (int)sf::div_up(m, REG_BLOCK), mom_blocks = std::min(tiles, REG_MOM_BLOCKS);
    Events ev;
    SF_TRY(ev.start(p->profile != 0));
    SF_TRY(ev.mark(0, s));
    SF_TRY(gather_enqueue(src, dst, pairs, m, B));
    SF_TRY(hypotheses_enqueue(ctx, p, m, B, false));
    SF_TRY(ev.mark(1, s));
    SF_TRY(sf::scan_u32<0>(ctx, B.live, B.pos, H));
    hipLaunchKernelGGL(k_reg_compact, dim3(nblk(H)), dim3(REG_BLOCK), 0, s, B.live, B.pos, B.T, (int)H, B.Tf, B.hid, B.flags);
    SF_HIP(hipGetLastError());
    SF_TRY(score_enqueue(ctx, m, H, &B.flags->n_live, 0, 0, t2, B));
    const unsigned round_blocks = std::min(nblk(H), 1024u);
    for (int r = 0; r < std::max(p->top_k, 1); ++r)
        hipLaunchKernelGGL(k_reg_round, dim3(round_blocks), dim3(REG_BLOCK), 0, s, B.counts, B.hid, B.flags, B.slot, r);
    hipLaunchKernelGGL(k_reg_best, dim3(1), dim3(64), 0, s, B.slot, B.T, B.pk, (int)m, (unsigned long long)p->seed, (long long)p->min_inliers, (int)p->top_k, B.stat, B.flags,
                       B.state, B.top);
    SF_HIP(hipGetLastError());
    SF_TRY(ev.mark(2, s));
    for (int r = 0; r < p->refine_rounds; ++r) {
        hipLaunchKernelGGL(k_reg_moments, dim3((unsigned)mom_blocks), dim3(REG_BLOCK), 0, s, B.pk, (int)m, B.state, t2, B.rows);
        hipLaunchKernelGGL(k_reg_refit, dim3(1), dim3(REG_MOM_BLOCKS), 0, s, B.state, B.rows, mom_blocks);
    }
    hipLaunchKernelGGL(k_reg_flags, dim3((unsigned)tiles), dim3(REG_BLOCK), 0, s, B.pk, (int)m, B.state, t2, B.inlier, B.tile_sum);
    hipLaunchKernelGGL(k_reg_finish, dim3(1), dim3(64), 0, s, B.state, B.tile_sum, tiles);
    SF_HIP(hipGetLastError());
    SF_TRY(ev.mark(3, s));
    RegState hs;
    std::vector<uint8_t> h_in(inlier ? (size_t)m : 0);
    std::vector<sf_reg_candidate> h_top((size_t)p->top_k);
    SF_HIP(hipMemcpyAsync(&hs, B.state, sizeof(hs), hipMemcpyDeviceToHost, s));
    SF_HIP(hipMemcpyAsync(&fl, B.flags, sizeof(fl), hipMemcpyDeviceToHost, s));
    if (inlier) SF_HIP(hipMemcpyAsync(h_in.data(), B.inlier, (size_t)m, hipMemcpyDeviceToHost, s));
    if (p->top_k > 0) SF_HIP(hipMemcpyAsync(h_top.data(), B.top, sizeof(sf_reg_candidate) * (size_t)p->top_k, hipMemcpyDeviceToHost, s));
    SF_HIP(hipStreamSynchronize(s));
    SF_CHECK(!fl.bad_index, SF_ERR_INVALID, "register: a pair holds an index outside its cloud");
    st.n_pairs = m;
    st.n_degenerate = (int64_t)hs.n_deg;
    st.n_rejected = (int64_t)hs.n_rej;
    st.n_scored = (int64_t)hs.n_live;
    st.best = hs.best;
    st.best_count = hs.best_count;
    st.n_inliers = (int64_t)hs.n_inliers;
    st.found = hs.found;
    st.rounds_done = hs.rounds_done;
    st.fitness = (double)st.n_inliers / (double)m;
    st.rmse = st.n_inliers > 0 ? std::sqrt(hs.sum_d2 / (double)st.n_inliers) : 0.0;
    st.n_top = hs.n_top;
    SF_TRY(ev.ms(0, 1, &st.hyp_ms));
    SF_TRY(ev.ms(1, 2, &st.score_ms));
    SF_TRY(ev.ms(2, 3, &st.refit_ms));
    std::memcpy(T, hs.T, sizeof(hs.T));
    if (inlier) std::memcpy(inlier, h_in.data(), (size_t)m);
    for (int k = 0; k < hs.n_top; ++k) top[k] = h_top[(size_t)k];
    if (stats) *stats = st;
    return SF_OK;
}
