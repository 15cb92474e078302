// sf_box.hpp -- per-label boxes of a cloud and the removal of a set of boxes from a cloud (extension, no reference code; DESIGN §19;
// the rule is stated in include/slamfusion.h).  Included by sf_map.hip after the plane block: it uses cluster_device / ClusterBufs of
// sf_cluster.hpp, PlaneEvents of sf_plane.hpp, read_words and nblk of sf_map.hip, the radix sort of sf_sort.hpp and jacobi_sym<3>.
//
// A segmented reduction over labels.  key_i = label_i for a member, n_labels for every other point; (key, i) is sorted by the
// stable radix sort, so the members of a label are one run of the sorted ids, in ascending original index.  Three passes walk the
// sorted ids (k_box_pass<Op>): count / lo / hi, then the float64 moments about the pivot, then the projections on the axes; between
// them one lane per label turns the sums into mean, covariance and axes (k_box_axes) and at the end into center and extent
// (k_box_finish).  A pass deals the sorted positions to the workgroups in contiguous chunks of whole tiles of 256; the grid and the
// chunk depend on n alone.  Inside a tile the lanes run a segmented inclusive scan (a fixed tree over the wave, the four waves in
// order, then the chunk's earlier tiles through a carry), and the last lane of a run holds the run's total inside the chunk.  A run
// that lies inside a chunk is written to its label; the first run of a chunk and the run at its last position may go on in a
// neighbouring chunk and are left as the chunk's two partial rows, which k_box_fixup combines per label in workgroup order.  No
// atomics on the values at all, whatever share of the points one label holds.
#pragma once
#include "sf_jacobi.hpp"

namespace {

constexpr int BOX_MAX_BLOCKS = 1024;          // workgroups of a pass at most: 2048 partial rows for k_box_fixup
constexpr int64_t BOX_MAX_LABELS = int64_t(1) << 24;
constexpr int BOX_MAX_REMOVE = 1024;          // boxes of sf_cloud_remove_boxes
constexpr uint32_t BOX_KEY_OUT = 0xffffffffu; // a lane beyond the chunk
constexpr uint32_t BOX_KEY_END = 0xfffffffeu; // "the key after the chunk's last position": equal to no key
constexpr uint32_t BOX_KEY_NONE = 0xfffffffdu; // the carry before the first tile

static_assert(sizeof(sf_label_box) == 256 && offsetof(sf_label_box, mean) == 32 && offsetof(sf_label_box, center) == 104 && offsetof(sf_label_box, valid) == 248,
              "sf_label_box is 256 bytes");

__device__ __forceinline__ double box_shfl_up(double v, int o)
{
    const int lo = __shfl_up(__double2loint(v), o, 64), hi = __shfl_up(__double2hiint(v), o, 64);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ void box_pivot(const sf_label_box *b, double c0[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) c0[k] = ((double)b->lo[k] + (double)b->hi[k]) / 2;
}

// ---- the three reductions.  V: what a lane carries; load: the value of one member; join(a, b): a the earlier part of the run;
// up: V of the lane o below; store: the total of a label into its box (raw sums: k_box_axes / k_box_finish finish them)
struct BoxOpBounds {
    struct V { float lo[3], hi[3]; uint32_t cnt; };
    static __device__ __forceinline__ V none()
    {
        const float inf = __uint_as_float(0x7f800000u);
        return V{{inf, inf, inf}, {-inf, -inf, -inf}, 0u};
    }
    static __device__ __forceinline__ V load(const float *__restrict__ xyz, uint32_t id, const sf_label_box *)
    {
        const float x = xyz[3 * (size_t)id], y = xyz[3 * (size_t)id + 1], z = xyz[3 * (size_t)id + 2];
        return V{{x, y, z}, {x, y, z}, 1u};
    }
    static __device__ __forceinline__ V join(const V &a, const V &b)
    {
        V r;
#pragma unroll
        for (int k = 0; k < 3; ++k) { r.lo[k] = fminf(a.lo[k], b.lo[k]); r.hi[k] = fmaxf(a.hi[k], b.hi[k]); }
        r.cnt = a.cnt + b.cnt;
        return r;
    }
    static __device__ __forceinline__ V up(const V &v, int o)
    {
        V r;
#pragma unroll
        for (int k = 0; k < 3; ++k) { r.lo[k] = __shfl_up(v.lo[k], o, 64); r.hi[k] = __shfl_up(v.hi[k], o, 64); }
        r.cnt = __shfl_up(v.cnt, o, 64);
        return r;
    }
    static __device__ __forceinline__ void store(sf_label_box *b, const V &v)
    {
        b->count = (int64_t)v.cnt;
#pragma unroll
        for (int k = 0; k < 3; ++k) { b->lo[k] = v.lo[k]; b->hi[k] = v.hi[k]; }
    }
};

struct BoxOpMoments { // S1 (3) and S2 (6) about the pivot -> mean[3], cov[6] as raw sums
    struct V { double s[9]; };
    static __device__ __forceinline__ V none() { return V{{0, 0, 0, 0, 0, 0, 0, 0, 0}}; }
    static __device__ __forceinline__ V load(const float *__restrict__ xyz, uint32_t id, const sf_label_box *b)
    {
        double c0[3];
        box_pivot(b, c0);
        const double dx = (double)xyz[3 * (size_t)id] - c0[0], dy = (double)xyz[3 * (size_t)id + 1] - c0[1], dz = (double)xyz[3 * (size_t)id + 2] - c0[2];
        return V{{dx, dy, dz, dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz}};
    }
    static __device__ __forceinline__ V join(const V &a, const V &b)
    {
        V r;
#pragma unroll
        for (int k = 0; k < 9; ++k) r.s[k] = a.s[k] + b.s[k];
        return r;
    }
    static __device__ __forceinline__ V up(const V &v, int o)
    {
        V r;
#pragma unroll
        for (int k = 0; k < 9; ++k) r.s[k] = box_shfl_up(v.s[k], o);
        return r;
    }
    static __device__ __forceinline__ void store(sf_label_box *b, const V &v)
    {
#pragma unroll
        for (int k = 0; k < 3; ++k) b->mean[k] = v.s[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) b->cov[k] = v.s[3 + k];
    }
};

struct BoxOpExtent { // min and max of d . a_k -> center[3] (pmin), extent[3] (pmax) until k_box_finish
    struct V { double mn[3], mx[3]; };
    static __device__ __forceinline__ V none()
    {
        const double inf = __longlong_as_double(0x7ff0000000000000ll);
        return V{{inf, inf, inf}, {-inf, -inf, -inf}};
    }
    static __device__ __forceinline__ V load(const float *__restrict__ xyz, uint32_t id, const sf_label_box *b)
    {
        double c0[3];
        box_pivot(b, c0);
        const double dx = (double)xyz[3 * (size_t)id] - c0[0], dy = (double)xyz[3 * (size_t)id + 1] - c0[1], dz = (double)xyz[3 * (size_t)id + 2] - c0[2];
        V r;
#pragma unroll
        for (int k = 0; k < 3; ++k) { // unfused (-ffp-contract=off), left to right
            double p = dx * b->R[k] + dy * b->R[3 + k];
            p = p + dz * b->R[6 + k];
            r.mn[k] = p; r.mx[k] = p;
        }
        return r;
    }
    static __device__ __forceinline__ V join(const V &a, const V &b)
    {
        V r;
#pragma unroll
        for (int k = 0; k < 3; ++k) { r.mn[k] = fmin(a.mn[k], b.mn[k]); r.mx[k] = fmax(a.mx[k], b.mx[k]); }
        return r;
    }
    static __device__ __forceinline__ V up(const V &v, int o)
    {
        V r;
#pragma unroll
        for (int k = 0; k < 3; ++k) { r.mn[k] = box_shfl_up(v.mn[k], o); r.mx[k] = box_shfl_up(v.mx[k], o); }
        return r;
    }
    static __device__ __forceinline__ void store(sf_label_box *b, const V &v)
    {
#pragma unroll
        for (int k = 0; k < 3; ++k) { b->center[k] = v.mn[k]; b->extent[k] = v.mx[k]; }
    }
};

constexpr size_t BOX_ROW_BYTES = 72; // the largest V
static_assert(sizeof(BoxOpBounds::V) <= BOX_ROW_BYTES && sizeof(BoxOpMoments::V) == BOX_ROW_BYTES && sizeof(BoxOpExtent::V) <= BOX_ROW_BYTES, "rows hold any V");

// key and value of every point and the two counts that are not members: one pair of integer atomics per workgroup at most, the grid
// capped and striding (a workgroup per tile would put 4 777 atomics on one word for the city map: 60 us for a 30 MB pass)
__global__ __launch_bounds__(256) void k_box_keys(const float *__restrict__ xyz, const int32_t *__restrict__ labels, int64_t n, uint32_t L, uint32_t *__restrict__ keys,
                                                   uint32_t *__restrict__ ids, unsigned long long *__restrict__ stat)
{
    __shared__ uint32_t wc[4][2];
    uint32_t a = 0u, b = 0u;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) { // (uniform per workgroup)
        const int64_t i = base + threadIdx.x;
        bool ignored = false, nonfinite = false;
        if (i < n) {
            const int32_t l = labels[i];
            ignored = l < 0 || (uint32_t)l >= L;
            if (!ignored) nonfinite = !(isfinite(xyz[3 * i]) && isfinite(xyz[3 * i + 1]) && isfinite(xyz[3 * i + 2]));
            keys[i] = (ignored || nonfinite) ? L : (uint32_t)l;
            ids[i] = (uint32_t)i;
        }
        a += (uint32_t)__popcll(__ballot(ignored));
        b += (uint32_t)__popcll(__ballot(nonfinite));
    }
    if ((threadIdx.x & 63u) == 0u) { wc[threadIdx.x >> 6][0] = a; wc[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const uint32_t t = wc[0][threadIdx.x] + wc[1][threadIdx.x] + wc[2][threadIdx.x] + wc[3][threadIdx.x];
        if (t) atomicAdd(stat + threadIdx.x, (unsigned long long)t);
    }
}

// One segmented pass.  Workgroup b walks the sorted positions [b chunk, min(n, (b + 1) chunk)), a tile of 256 at a time.  Keys are
// ascending, so a run of equal keys is contiguous and "the key o lanes below is mine" means that every lane in between is too.
template <class Op>
__global__ __launch_bounds__(256) void k_box_pass(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ ids, const float *__restrict__ xyz, int64_t n,
                                                   int64_t chunk, uint32_t L, sf_label_box *boxes, int32_t *__restrict__ row_label, char *__restrict__ row_bytes)
{
    typedef typename Op::V V;
    __shared__ V tail[4], cval;        // the total of each wave's last run; the inclusive value at the previous tile's last lane
    __shared__ uint32_t kfirst[4], klast[4], ckey;
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t b0 = (int64_t)blockIdx.x * chunk, b1 = b0 + chunk < n ? b0 + chunk : n;
    if (b0 >= n) return;
    V *rows = reinterpret_cast<V *>(row_bytes);
    const uint32_t first_key = keys[b0];
    if (tid == 0) ckey = BOX_KEY_NONE;
    for (int64_t t0 = b0; t0 < b1; t0 += 256) {
        const int64_t pos = t0 + tid;
        const bool in = pos < b1;
        const uint32_t key = in ? keys[pos] : BOX_KEY_OUT;
        const uint32_t knext = pos + 1 < b1 ? keys[pos + 1] : BOX_KEY_END;
        const bool member = in && key < L;
        V v = Op::none();
        if (member) v = Op::load(xyz, ids[pos], boxes + key);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { // the wave: a fixed tree
            const V t = Op::up(v, o);
            const uint32_t kk = __shfl_up(key, o, 64);
            if (lane >= o && kk == key) v = Op::join(t, v);
        }
        if (lane == 0) kfirst[w] = key;
        if (lane == 63) { klast[w] = key; tail[w] = v; }
        __syncthreads();
        // what the chunk holds of this lane's run before its wave: the earlier tiles, then the earlier waves, in order.  A lane
        // that is not in its wave's first run finds nothing (its key is larger than every key before the wave).
        V acc = Op::none();
        if (ckey == key) acc = cval;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (k < w) {
                if (klast[k] != key) acc = Op::none();
                else if (kfirst[k] == key) acc = Op::join(acc, tail[k]);
                else acc = tail[k];
            }
        }
        if (member) v = Op::join(acc, v);
        __syncthreads();
        if (tid == 255) { ckey = key; cval = v; }
        if (member && key != knext) { // the last of its run inside the chunk
            if (key == first_key) { rows[2 * blockIdx.x] = v; row_label[2 * blockIdx.x] = (int32_t)key; }
            else if (pos == b1 - 1) { rows[2 * blockIdx.x + 1] = v; row_label[2 * blockIdx.x + 1] = (int32_t)key; }
            else Op::store(boxes + key, v);
        }
    }
}

// The partial rows (first run, last run of workgroup 0, of workgroup 1, ...; label -1: none) of one label are neighbours, with at
// most one empty "last" row between two of them (a chunk that is one run); an empty "first" row means that the chunk begins with
// non-members, and so does everything after it.  One wave per row: the wave of a label's first row gathers the label's rows, lane j
// rows j, j + 64, ... in ascending order, joins the lanes by the scan's fixed tree and writes the label.  One label holding every
// point is 32 trips of one wave, not one lane walking 2048 rows.
template <class Op>
__global__ __launch_bounds__(64) void k_box_fixup(const int32_t *__restrict__ row_label, const char *__restrict__ row_bytes, int nrows, sf_label_box *boxes)
{
    typedef typename Op::V V;
    const V *rows = reinterpret_cast<const V *>(row_bytes);
    const int r = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int32_t l = row_label[r];
    if (l < 0) return;
    int p = r - 1;
    if (p >= 0 && row_label[p] < 0) --p;
    if (p >= 0 && row_label[p] == l) return; // not the label's first row
    V acc = Op::none();
    for (int q0 = r;; q0 += 64) { // (uniform)
        const int q = q0 + lane;
        const int32_t lq = q < nrows ? row_label[q] : -2;
        const bool stop = lq == -2 || (lq >= 0 && lq != l) || (lq == -1 && (q & 1) == 0); // the end, another label, non-members from here on
        const unsigned long long sm = __ballot(stop);
        const int first = sm ? __ffsll((long long)sm) - 1 : 64;
        if (lq == l && lane < first) acc = Op::join(acc, rows[q]);
        if (sm) break;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const V t = Op::up(acc, o);
        if (lane >= o) acc = Op::join(t, acc);
    }
    if (lane == 63) Op::store(boxes + l, acc);
}

struct BoxAxesArg { int mode; double u[3], e1[3], e2[3]; };

__device__ __forceinline__ void box_sign(double a[3]) // the component of largest magnitude (the first on a tie) positive
{
    double am = a[0];
    if (fabs(a[1]) > fabs(am)) am = a[1];
    if (fabs(a[2]) > fabs(am)) am = a[2];
    if (am < 0) { a[0] = -a[0]; a[1] = -a[1]; a[2] = -a[2]; }
}

template <int A, int B>
__device__ __forceinline__ void box_order(double (&val)[3], double (&vec)[9]) // descending, equal values stay (vec: axes as rows)
{
    if (val[A] < val[B]) {
        double t = val[A]; val[A] = val[B]; val[B] = t;
#pragma unroll
        for (int i = 0; i < 3; ++i) { t = vec[3 * A + i]; vec[3 * A + i] = vec[3 * B + i]; vec[3 * B + i] = t; }
    }
}

__device__ __forceinline__ double box_quad(const double C[6], const double a[3], const double b[3]) // a^T C b
{
    const double cx = C[0] * b[0] + C[1] * b[1] + C[2] * b[2], cy = C[1] * b[0] + C[3] * b[1] + C[4] * b[2], cz = C[2] * b[0] + C[4] * b[1] + C[5] * b[2];
    return a[0] * cx + a[1] * cy + a[2] * cz;
}

// one lane per label, after the moments: mean, cov, axes, eigenvalues, valid
__global__ __launch_bounds__(64) void k_box_axes(sf_label_box *boxes, uint32_t L, BoxAxesArg arg)
{
    const uint32_t l = blockIdx.x * 64 + threadIdx.x;
    if (l >= L) return;
    sf_label_box *b = boxes + l;
    if (b->count == 0) return; // (zeros throughout)
    const double cnt = (double)b->count;
    double c0[3], m[3], C[6];
    box_pivot(b, c0);
#pragma unroll
    for (int k = 0; k < 3; ++k) m[k] = b->mean[k] / cnt;
    C[0] = b->cov[0] / cnt - m[0] * m[0]; C[1] = b->cov[1] / cnt - m[0] * m[1]; C[2] = b->cov[2] / cnt - m[0] * m[2];
    C[3] = b->cov[3] / cnt - m[1] * m[1]; C[4] = b->cov[4] / cnt - m[1] * m[2]; C[5] = b->cov[5] / cnt - m[2] * m[2];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) ok = ok && isfinite(C[k]);
    double ax[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, ev[3] = {0, 0, 0}; // axes as rows
    if (ok && arg.mode == SF_BOX_AABB) {
        ev[0] = C[0]; ev[1] = C[3]; ev[2] = C[5];
    } else if (ok && arg.mode == SF_BOX_PCA) {
        double A[9] = {C[0], C[1], C[2], C[1], C[3], C[4], C[2], C[4], C[5]}, V[9];
        jacobi_sym<3>(A, V);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ev[k] = A[4 * k];
#pragma unroll
            for (int i = 0; i < 3; ++i) ax[3 * k + i] = V[3 * i + k];
        }
        box_order<0, 1>(ev, ax);
        box_order<1, 2>(ev, ax);
        box_order<0, 1>(ev, ax);
        double a0[3] = {ax[0], ax[1], ax[2]}, a1[3] = {ax[3], ax[4], ax[5]};
        box_sign(a0);
        box_sign(a1);
        ax[0] = a0[0]; ax[1] = a0[1]; ax[2] = a0[2]; ax[3] = a1[0]; ax[4] = a1[1]; ax[5] = a1[2];
        ax[6] = a0[1] * a1[2] - a0[2] * a1[1]; ax[7] = a0[2] * a1[0] - a0[0] * a1[2]; ax[8] = a0[0] * a1[1] - a0[1] * a1[0];
    } else if (ok) { // SF_BOX_UPRIGHT
        const double c11 = box_quad(C, arg.e1, arg.e1), c12 = box_quad(C, arg.e1, arg.e2), c22 = box_quad(C, arg.e2, arg.e2);
        const double th = atan2(2.0 * c12, c11 - c22) / 2, ct = cos(th), st = sin(th);
        double a0[3] = {ct * arg.e1[0] + st * arg.e2[0], ct * arg.e1[1] + st * arg.e2[1], ct * arg.e1[2] + st * arg.e2[2]};
        box_sign(a0);
        const double *u = arg.u;
        const double a1[3] = {u[1] * a0[2] - u[2] * a0[1], u[2] * a0[0] - u[0] * a0[2], u[0] * a0[1] - u[1] * a0[0]};
        ax[0] = a0[0]; ax[1] = a0[1]; ax[2] = a0[2]; ax[3] = a1[0]; ax[4] = a1[1]; ax[5] = a1[2]; ax[6] = u[0]; ax[7] = u[1]; ax[8] = u[2];
        ev[0] = box_quad(C, a0, a0); ev[1] = box_quad(C, a1, a1); ev[2] = box_quad(C, u, u);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        b->mean[k] = c0[k] + m[k];
        b->eigenvalues[k] = ev[k];
#pragma unroll
        for (int i = 0; i < 3; ++i) b->R[3 * i + k] = ax[3 * k + i];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) b->cov[k] = C[k];
    b->valid = ok ? 1 : 2;
}

// center is the rule's exact value rounded once, as nearly as double-double arithmetic gives it (error-free sums and products, the
// low parts added in float64): the crop subtracts the ROUNDED center, so each of the three roundings of the plain evaluation moved
// the faces by up to half an ulp of |center| against the members that define them
struct BoxDD { double hi, lo; };
__device__ __forceinline__ BoxDD box_two_sum(double a, double b)
{
    const double s = a + b, bb = s - a;
    return BoxDD{s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ void box_dd_add_product(BoxDD &acc, double a, const BoxDD &h) // acc += a (h.hi + h.lo)
{
    const double p = a * h.hi, pe = fma(a, h.hi, -p) + a * h.lo;
    const BoxDD s = box_two_sum(acc.hi, p);
    acc.hi = s.hi;
    acc.lo = acc.lo + (s.lo + pe);
}

// one lane per label, after the projections: center and extent; stat[2] += the labels with members (one integer atomic per wave)
__global__ __launch_bounds__(64) void k_box_finish(sf_label_box *boxes, uint32_t L, unsigned long long *__restrict__ stat)
{
    const uint32_t l = blockIdx.x * 64 + threadIdx.x;
    const bool have = l < L && boxes[l].count != 0;
    if (have) {
        sf_label_box *b = boxes + l;
        double c0[3], e[3];
        BoxDD h[3];
        box_pivot(b, c0);
#pragma unroll
        for (int k = 0; k < 3; ++k) { // (pmin in center, pmax in extent)
            const BoxDD t = box_two_sum(b->center[k], b->extent[k]);
            h[k] = BoxDD{t.hi / 2, t.lo / 2};
            e[k] = b->extent[k] - b->center[k];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            BoxDD s{c0[i], 0.0};
            box_dd_add_product(s, b->R[3 * i], h[0]);
            box_dd_add_product(s, b->R[3 * i + 1], h[1]);
            box_dd_add_product(s, b->R[3 * i + 2], h[2]);
            b->center[i] = s.hi + s.lo;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) b->extent[k] = e[k];
    }
    const uint32_t cnt = (uint32_t)__popcll(__ballot(have));
    if (threadIdx.x == 0 && cnt) atomicAdd(stat + 2, (unsigned long long)cnt);
}

// ---- sf_cloud_remove_boxes.  k_flag_obb's predicate (sf_cloud.hip), box after box: the box is a uniform index into a const
// __restrict__ argument, so its 15 values arrive in SGPRs; a lane stops at its first hit and the wave when every lane has one.
struct BoxObb { double c[3], R[9], half[3]; };

__global__ __launch_bounds__(256) void k_flag_boxes(const float *__restrict__ xyz, int64_t n, const BoxObb *__restrict__ obb, int B, int keep_inside, uint8_t *__restrict__ flags,
                                                     unsigned long long *__restrict__ n_inside)
{
    __shared__ uint32_t wcnt[4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool have = i < n;
    const float xf = have ? xyz[3 * i] : 0.0f, yf = have ? xyz[3 * i + 1] : 0.0f, zf = have ? xyz[3 * i + 2] : 0.0f;
    bool open = have && isfinite(xf) && isfinite(yf) && isfinite(zf), inside = false; // open: still looking
    for (int b = 0; b < B; ++b) {
        if (__ballot(open) == 0ull) break;
        const BoxObb o = obb[b];
        if (open) {
            const double d0 = (double)xf - o.c[0], d1 = (double)yf - o.c[1], d2 = (double)zf - o.c[2];
            bool ok = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                double proj = d0 * o.R[k] + d1 * o.R[3 + k];
                proj = proj + d2 * o.R[6 + k];
                ok = ok && (fabs(proj) <= o.half[k]);
            }
            if (ok) { inside = true; open = false; }
        }
    }
    if (have) flags[i] = inside == (keep_inside != 0) ? 1 : 0;
    const uint32_t c = (uint32_t)__popcll(__ballot(inside));
    if ((threadIdx.x & 63u) == 0u) wcnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t total = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        if (total) atomicAdd(n_inside, (unsigned long long)total);
    }
}

// ---- host side
#define SF_CHECK_BOX(c, p, n_labels)                                                                                                                     \
    do {                                                                                                                                                 \
        SF_CHECK((c) && (p), SF_ERR_INVALID, "bad arguments");                                                                                           \
        SF_CHECK((n_labels) >= 0 && (n_labels) <= BOX_MAX_LABELS, SF_ERR_INVALID, "boxes: n_labels must be 0 .. 2^24 (got %lld)", (long long)(n_labels)); \
        SF_CHECK((c)->n < (int64_t(1) << 31), SF_ERR_INVALID, "boxes: the cloud must hold fewer than 2^31 points");                                      \
        SF_CHECK((p)->mode == SF_BOX_AABB || (p)->mode == SF_BOX_PCA || (p)->mode == SF_BOX_UPRIGHT, SF_ERR_INVALID, "boxes: unknown mode %d", (int)(p)->mode); \
        SF_CHECK(std::isfinite((p)->up[0]) && std::isfinite((p)->up[1]) && std::isfinite((p)->up[2]), SF_ERR_INVALID, "boxes: up must be finite");       \
    } while (0)

// u = up normalised (all zeros: +z), e1 = normalize(u x e_k) with k the coordinate of smallest |u_k|, e2 = u x e1: float64 on the host
BoxAxesArg box_axes_arg(const sf_box_params *p)
{
    BoxAxesArg a{};
    a.mode = p->mode;
    double x = p->up[0], y = p->up[1], z = p->up[2];
    if (x == 0 && y == 0 && z == 0) z = 1.0;
    double nn = x * x;
    nn = nn + y * y;
    nn = nn + z * z;
    const double nrm = std::sqrt(nn);
    double *u = a.u;
    u[0] = x / nrm; u[1] = y / nrm; u[2] = z / nrm;
    int k = 0;
    if (std::fabs(u[1]) < std::fabs(u[k])) k = 1;
    if (std::fabs(u[2]) < std::fabs(u[k])) k = 2;
    const double ek[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    double v[3] = {u[1] * ek[2] - u[2] * ek[1], u[2] * ek[0] - u[0] * ek[2], u[0] * ek[1] - u[1] * ek[0]};
    double vv = v[0] * v[0];
    vv = vv + v[1] * v[1];
    vv = vv + v[2] * v[2];
    const double vn = std::sqrt(vv);
    for (int i = 0; i < 3; ++i) a.e1[i] = v[i] / vn;
    a.e2[0] = u[1] * a.e1[2] - u[2] * a.e1[1]; a.e2[1] = u[2] * a.e1[0] - u[0] * a.e1[2]; a.e2[2] = u[0] * a.e1[1] - u[1] * a.e1[0];
    return a;
}

// workgroups and chunk of the three passes: whole tiles of 256, from n alone (max_blocks > 0: the test hook's cap)
inline void box_grid(int64_t n, int max_blocks, int *blocks, int64_t *chunk)
{
    const int64_t tiles = sf::div_up(n, 256), cap = max_blocks > 0 ? max_blocks : BOX_MAX_BLOCKS;
    const int64_t per = sf::div_up(tiles, std::min(tiles, cap));
    *chunk = per * 256;
    *blocks = (int)sf::div_up(n, *chunk);
}

template <class Op>
void box_pass_launch(sf_cloud *c, const uint32_t *keys, const uint32_t *ids, int blocks, int64_t chunk, uint32_t L, sf_label_box *boxes, int32_t *row_label, char *rows)
{
    hipStream_t s = c->ctx->stream;
    hipError_t e = hipMemsetAsync(row_label, 0xFF, sizeof(int32_t) * 2 * (size_t)blocks, s); // (a failure surfaces at the caller's hipGetLastError / wait)
    (void)e;
    hipLaunchKernelGGL(k_box_pass<Op>, dim3((unsigned)blocks), dim3(256), 0, s, keys, ids, c->xyz.as<float>(), c->n, chunk, L, boxes, row_label, rows);
    hipLaunchKernelGGL(k_box_fixup<Op>, dim3(2 * (unsigned)blocks), dim3(64), 0, s, row_label, rows, 2 * blocks, boxes);
}

// The boxes proper: d_labels [n] on the device -> out[min(L, cap)] on the host.  The host waits once, at the end.  c is left alone.
// n > 0 (the callers answer an empty cloud themselves).
int box_device(sf_cloud *c, const int32_t *d_labels, int64_t n_labels, const sf_box_params *p, int max_blocks, sf_label_box *out, int64_t cap, sf_box_stats *stats)
{
    sf_ctx *ctx = c->ctx;
    hipStream_t s = ctx->stream;
    const int64_t n = c->n;
    const uint32_t L = (uint32_t)n_labels;
    int blocks;
    int64_t chunk;
    box_grid(n, max_blocks, &blocks, &chunk);
    // the context's sort buffers of the voxel grids (temporaries of a call there as here: no allocation per call once they have grown)
    const auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
    const size_t rows_b = up(BOX_ROW_BYTES * 2 * (size_t)blocks), lab_b = up(sizeof(int32_t) * 2 * (size_t)blocks);
    const size_t box_b = sizeof(sf_label_box) * (size_t)std::max<int64_t>(n_labels, 1);
    sf::DevBuf own; // (boxes beyond 64 MiB -- 262 144 labels -- are not left with the context)
    sf::DevBuf &small = ctx->vox_tmp[4], &dbox = box_b > (size_t(64) << 20) ? own : ctx->vox_tmp[5];
    for (int k = 0; k < 4; ++k) SF_TRY(ctx->vox_tmp[k].reserve(sizeof(uint32_t) * (size_t)n));
    SF_TRY(small.reserve(rows_b + lab_b + 256));
    SF_TRY(dbox.reserve(box_b));
    uint32_t *keys = ctx->vox_tmp[0].as<uint32_t>(), *keys2 = ctx->vox_tmp[1].as<uint32_t>(), *ids = ctx->vox_tmp[2].as<uint32_t>(), *ids2 = ctx->vox_tmp[3].as<uint32_t>();
    char *rows = small.as<char>();
    int32_t *row_label = reinterpret_cast<int32_t *>(rows + rows_b);
    unsigned long long *stat = reinterpret_cast<unsigned long long *>(rows + rows_b + lab_b); // ignored, non-finite, valid
    sf_label_box *boxes = dbox.as<sf_label_box>();
    PlaneEvents ev;
    ev.start(p->profile != 0);
    ev.mark(0, s);
    SF_HIP(hipMemsetAsync(stat, 0, sizeof(unsigned long long) * 4, s));
    if (L > 0) SF_HIP(hipMemsetAsync(boxes, 0, sizeof(sf_label_box) * (size_t)L, s));
    hipLaunchKernelGGL(k_box_keys, dim3(std::min(nblk(n), (unsigned)BOX_MAX_BLOCKS)), dim3(256), 0, s, c->xyz.as<float>(), d_labels, n, L, keys, ids, stat);
    if (L > 0) {
        unsigned end_bit = 0;
        while ((uint64_t(1) << end_bit) <= (uint64_t)L) ++end_bit; // the keys are 0 .. L
        uint32_t *sk = nullptr, *sv = nullptr;
        SF_TRY(sf::radix_sort_pairs<uint32_t>(ctx, keys, keys2, ids, ids2, n, end_bit, &sk, &sv));
        const BoxAxesArg arg = box_axes_arg(p);
        box_pass_launch<BoxOpBounds>(c, sk, sv, blocks, chunk, L, boxes, row_label, rows);
        box_pass_launch<BoxOpMoments>(c, sk, sv, blocks, chunk, L, boxes, row_label, rows);
        hipLaunchKernelGGL(k_box_axes, dim3(nblk(L, 64)), dim3(64), 0, s, boxes, L, arg);
        box_pass_launch<BoxOpExtent>(c, sk, sv, blocks, chunk, L, boxes, row_label, rows);
        hipLaunchKernelGGL(k_box_finish, dim3(nblk(L, 64)), dim3(64), 0, s, boxes, L, stat);
    }
    ev.mark(3, s);
    const int64_t n_out = std::min<int64_t>(n_labels, cap);
    if (n_out > 0) SF_HIP(hipMemcpyAsync(out, boxes, sizeof(sf_label_box) * (size_t)n_out, hipMemcpyDeviceToHost, s));
    SF_TRY(read_words(ctx, stat, 3));
    const unsigned long long *h = ctx->h_pinned->readback;
    if (stats) {
        stats->n_points = n;
        stats->n_ignored = (int64_t)h[0];
        stats->n_nonfinite = (int64_t)h[1];
        stats->n_labelled = n - stats->n_ignored - stats->n_nonfinite;
        stats->n_labels = n_labels;
        stats->n_valid = (int64_t)h[2];
        stats->device_ms = ev.ms(0, 3);
        stats->pad = 0;
    }
    return SF_OK;
}

inline sf_box_stats box_empty_stats(int64_t n_labels)
{
    sf_box_stats st{};
    st.n_labels = n_labels;
    st.device_ms = -1.0f;
    return st;
}

int box_labels_host(sf_cloud *c, const int32_t *labels, int64_t n_labels, const sf_box_params *p, int max_blocks, sf_label_box *boxes, sf_box_stats *stats)
{
    SF_CHECK_BOX(c, p, n_labels);
    SF_CHECK(max_blocks >= 0 && max_blocks <= BOX_MAX_BLOCKS, SF_ERR_INVALID, "boxes: max_blocks must be 0 .. %d", BOX_MAX_BLOCKS);
    SF_CHECK((labels || c->n == 0) && (boxes || n_labels == 0), SF_ERR_INVALID, "bad arguments");
    if (stats) *stats = box_empty_stats(n_labels);
    if (c->n == 0) {
        if (n_labels > 0) std::memset(boxes, 0, sizeof(sf_label_box) * (size_t)n_labels);
        return SF_OK;
    }
    sf_ctx *ctx = c->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    sf::DevBuf dl;
    SF_TRY(dl.reserve(sizeof(int32_t) * (size_t)c->n));
    SF_TRY(sf::upload_staged(ctx, dl.p, labels, sizeof(int32_t) * (size_t)c->n));
    return box_device(c, dl.as<int32_t>(), n_labels, p, max_blocks, boxes, n_labels, stats);
}

} // namespace

extern "C" int sf_cloud_label_boxes(sf_cloud *c, const int32_t *labels, int64_t n_labels, const sf_box_params *p, sf_label_box *boxes, sf_box_stats *stats)
{
    return box_labels_host(c, labels, n_labels, p, 0, boxes, stats);
}

extern "C" int sf_test_label_boxes(sf_cloud *c, const int32_t *labels, int64_t n_labels, const sf_box_params *p, int max_blocks, sf_label_box *boxes, sf_box_stats *stats)
{
    return box_labels_host(c, labels, n_labels, p, max_blocks, boxes, stats);
}

extern "C" int sf_cloud_cluster_boxes(sf_cloud *c, double tolerance, int64_t min_size, int64_t max_size, float cell, const sf_box_params *p, sf_label_box *boxes,
                                      int64_t cap_boxes, sf_cluster_stats *cstats, sf_box_stats *bstats)
{
    SF_CHECK_BOX(c, p, 0);
    SF_CHECK_CLUSTER_EUCLIDEAN(tolerance, min_size);
    SF_CHECK(cap_boxes >= 0 && (boxes || cap_boxes == 0), SF_ERR_INVALID, "cluster_boxes: cap_boxes must not be negative, boxes not NULL");
    sf_cluster_stats cst{};
    if (cstats) *cstats = cst;
    if (bstats) *bstats = box_empty_stats(0);
    if (c->n == 0) return SF_OK;
    sf_map *tmp = nullptr;
    SF_TRY(sf_map_create(c->ctx, &tmp));
    int rc = sf_map_build(tmp, c, cell);
    ClusterBufs b{};
    if (rc == SF_OK) rc = cluster_device(tmp, tolerance, 1, min_size, max_size, &b, &cst);
    if (rc == SF_OK && cst.n_clusters > BOX_MAX_LABELS) { sf::set_error("cluster_boxes: more than 2^24 clusters (%lld)", (long long)cst.n_clusters); rc = SF_ERR_INVALID; }
    if (rc == SF_OK) rc = box_device(c, b.labels, cst.n_clusters, p, 0, boxes, cap_boxes, bstats);
    sf_map_destroy(tmp);
    if (rc == SF_OK && cstats) *cstats = cst;
    return rc;
}

extern "C" int sf_cloud_remove_boxes(sf_cloud *c, const double *center, const double *R, const double *extent, int64_t n_boxes, double margin, int keep_inside,
                                     int64_t *n_inside)
{
    SF_CHECK(c, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(n_boxes >= 0 && n_boxes <= BOX_MAX_REMOVE, SF_ERR_INVALID, "remove_boxes: n_boxes must be 0 .. %d (got %lld)", BOX_MAX_REMOVE, (long long)n_boxes);
    SF_CHECK(n_boxes == 0 || (center && R && extent), SF_ERR_INVALID, "bad arguments");
    SF_CHECK(std::isfinite(margin), SF_ERR_INVALID, "remove_boxes: the margin must be finite");
    SF_CHECK(c->n < (int64_t(1) << 31), SF_ERR_INVALID, "boxes: the cloud must hold fewer than 2^31 points");
    sf::cloud_touch(c);
    if (n_inside) *n_inside = 0;
    if (c->n == 0) { c->n_last_idx = 0; return SF_OK; }
    sf_ctx *ctx = c->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    std::vector<BoxObb> obb((size_t)std::max<int64_t>(n_boxes, 1));
    for (int64_t b = 0; b < n_boxes; ++b) {
        for (int d = 0; d < 3; ++d) { obb[b].c[d] = center[3 * b + d]; obb[b].half[d] = (extent[3 * b + d] + 2 * margin) / 2; }
        for (int k = 0; k < 9; ++k) obb[b].R[k] = R[9 * b + k];
    }
    sf::DevBuf dobb; // (its own allocation: compact_cloud carves the context's small scratch)
    SF_TRY(dobb.reserve(sizeof(BoxObb) * obb.size() + 16));
    unsigned long long *d_inside = reinterpret_cast<unsigned long long *>(dobb.as<char>() + sizeof(BoxObb) * obb.size());
    SF_TRY(sf::upload_staged(ctx, dobb.p, obb.data(), sizeof(BoxObb) * obb.size()));
    SF_HIP(hipMemsetAsync(d_inside, 0, sizeof(unsigned long long), ctx->stream));
    SF_TRY(c->flags.reserve((size_t)c->n));
    hipLaunchKernelGGL(k_flag_boxes, dim3(nblk(c->n)), dim3(256), 0, ctx->stream, c->xyz.as<float>(), c->n, dobb.as<BoxObb>(), (int)n_boxes, keep_inside, c->flags.as<uint8_t>(),
                       d_inside);
    SF_TRY(read_words(ctx, d_inside, 1));
    if (n_inside) *n_inside = (int64_t)ctx->h_pinned->readback[0];
    return sf::compact_cloud(c, c->flags.as<uint8_t>());
}
