// sf_visibility.hip -- range images and visibility-based removal of stale map points (sf_range_image_*, sf_map_visibility*,
// sf_cloud_remove_seen_through; include/slamfusion.h; extension, no reference code: the rule is in DESIGN section 28 and restated in
// tests/visibility_ref_np.py).  gfx950 only, wave64.  A translation unit of its own over sf_common.hpp; nothing of sf_map.hip.
//
// Build (per scan):
//   a fill         every key 0xff..ff: an empty pixel
//   k_ri_build     one lane per point: the sensor frame and the pixel in float64, then ONE 64-bit integer atomicMin of
//                  (bits((float)r) << 32) | i -- the smallest range, on a tie the smallest index, whatever the arrival order
//   k_ri_finish    one lane per pixel: the range plane (the high word of the key; 0xffffffff: empty) that the classify pass reads at
//                  4 bytes a pixel, and the count of filled pixels
// Classify (per call, however many images vote):
//   k_vis_votes    one lane per point of pts4 (or of the cloud's float3s, the same body): the point stays in registers while the lane
//                  walks the images -- pose, geometry and plane pointer of image b are a wave-uniform load from a const __restrict__
//                  array -- and counts its classes; the two votes, the class of the last image and the keep flag are written once, at
//                  the original index; the per-class counts are wave-reduced, summed over the block in LDS and added with integer atomics
// The range test comes before the two atan2: it is the float64 rule itself, so nothing needs a conservative float32 prefilter.
#include "sf_common.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

struct sf_range_image {
    sf_ctx *ctx = nullptr;
    sf_range_image_params prm{};
    sf::DevBuf keys; // uint64 [H][W]: (bits((float)r) << 32) | i, all ones = empty
    sf::DevBuf rng;  // uint32 [H][W]: the high words
    sf::DevBuf stat; // the counters of a build (VIS_SLOTS copies)
};

namespace {

constexpr double VIS_PI = 3.141592653589793;
constexpr uint32_t VIS_EMPTY = 0xffffffffu;
constexpr int VIS_MAX_IMAGES = 64;

inline unsigned nblk(int64_t n, int b = 256) { return (unsigned)sf::div_up(n > 0 ? n : 1, b); }

// one image as the kernels see it: a[] = T[0] T[4] T[8] | T[1] T[5] T[9] | T[2] T[6] T[10] (the rows of R^T), t = T[3] T[7] T[11]
struct VisImage {
    double a[9], t[3];
    double el_min, el_span, min_range, max_range;
    const uint32_t *rng;
    int W, H;
};

struct VisWin { int half_cols, half_rows, min_hits, pad; double range_margin, range_ratio; };

// the sensor frame and the pixel of part 1 of the rule (float64, unfused, left to right); false: outside
__device__ __forceinline__ bool vis_project(const VisImage &g, float xf, float yf, float zf, double &r, int &row, int &col)
{
    const double d0 = (double)xf - g.t[0], d1 = (double)yf - g.t[1], d2 = (double)zf - g.t[2];
    const double x = (g.a[0] * d0 + g.a[1] * d1) + g.a[2] * d2;
    const double y = (g.a[3] * d0 + g.a[4] * d1) + g.a[5] * d2;
    const double z = (g.a[6] * d0 + g.a[7] * d1) + g.a[8] * d2;
    const double h2 = x * x + y * y;
    r = sqrt(h2 + z * z);
    if (!(r > 0.0 && g.min_range <= r && r <= g.max_range)) return false;
    const double az = atan2(y, x), el = atan2(z, sqrt(h2));
    const double u = (az + VIS_PI) / (2.0 * VIS_PI) * (double)g.W;
    const double v = (el - g.el_min) / g.el_span * (double)g.H;
    if (!(v >= 0.0 && v < (double)g.H)) return false; // v < 0 or floor(v) >= H
    row = (int)floor(v);
    int c = (int)floor(u);
    if (c >= g.W) c -= g.W;
    col = min(max(c, 0), g.W - 1); // (a guard only: az lies in [-PI, PI], so u in [0, W])
    return true;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// The counters of a call: VIS_SLOTS copies of VIS_WORDS words, block b adding into copy b % VIS_SLOTS and the host summing the
// copies -- one address taking an atomic from every wave of a large launch costs more than the launch's own work.  Every thread of
// the block calls this with its wave's totals.
constexpr int VIS_SLOTS = 16, VIS_WORDS = 8;
constexpr size_t VIS_STAT_BYTES = sizeof(unsigned long long) * VIS_SLOTS * VIS_WORDS;

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
        if (t) atomicAdd(stat + (blockIdx.x % VIS_SLOTS) * VIS_WORDS + threadIdx.x, (unsigned long long)t);
    }
}

__global__ __launch_bounds__(256) void k_ri_build(const float *__restrict__ xyz, int64_t n, VisImage g, unsigned long long *__restrict__ keys,
                                                  unsigned long long *__restrict__ stat)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool have = i < n;
    const float xf = have ? xyz[3 * i] : 0.0f, yf = have ? xyz[3 * i + 1] : 0.0f, zf = have ? xyz[3 * i + 2] : 0.0f;
    const bool fin = have && isfinite(xf) && isfinite(yf) && isfinite(zf);
    bool in = false;
    if (fin) {
        double r;
        int row, col;
        in = vis_project(g, xf, yf, zf, r, row, col);
        if (in) {
            const unsigned long long key = ((unsigned long long)__float_as_uint((float)r) << 32) | (unsigned long long)(uint32_t)i;
            atomicMin(keys + ((size_t)row * (size_t)g.W + (size_t)col), key);
        }
    }
    const uint32_t tot[3] = {(uint32_t)__popcll(__ballot(in)), (uint32_t)__popcll(__ballot(fin && !in)), (uint32_t)__popcll(__ballot(have && !fin))};
    block_add<3>(tot, stat); // projected, outside, not finite
}

__global__ __launch_bounds__(256) void k_ri_finish(const unsigned long long *__restrict__ keys, int64_t npix, uint32_t *__restrict__ rng,
                                                   unsigned long long *__restrict__ stat)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool filled = false;
    if (i < npix) {
        const unsigned long long k = keys[i];
        filled = k != ~0ull;
        rng[i] = filled ? (uint32_t)(k >> 32) : VIS_EMPTY;
    }
    const uint32_t tot[1] = {(uint32_t)__popcll(__ballot(filled))};
    block_add<1>(tot, stat + 3);
}

// the class of a finite point against one image (part 2 of the rule)
__device__ __forceinline__ int vis_classify(const VisImage &g, const VisWin &w, float xf, float yf, float zf)
{
    double r;
    int row, col;
    if (!vis_project(g, xf, yf, zf, r, row, col)) return SF_VIS_OUTSIDE;
    const int hr = min(w.half_rows, g.H); // (rows outside [0, H) are skipped anyway)
    const int r0 = max(row - hr, 0), r1 = min(row + hr, g.H - 1);
    int n_hit = 0;
    float r_near = INFINITY, r_far = -INFINITY;
    for (int rr = r0; rr <= r1; ++rr) {
        const uint32_t *__restrict__ line = g.rng + (size_t)rr * (size_t)g.W;
        for (int dc = -w.half_cols; dc <= w.half_cols; ++dc) {
            int c = col + dc; // 2 half_cols + 1 <= W: one wrap is enough and no pixel is met twice
            c = c < 0 ? c + g.W : (c >= g.W ? c - g.W : c);
            const uint32_t bits = line[c];
            if (bits != VIS_EMPTY) {
                const float f = __uint_as_float(bits);
                ++n_hit;
                r_near = f < r_near ? f : r_near;
                r_far = f > r_far ? f : r_far;
            }
        }
    }
    if (n_hit < w.min_hits) return SF_VIS_UNKNOWN;
    const double margin = w.range_margin + w.range_ratio * r;
    if (r + margin < (double)r_near) return SF_VIS_SEEN_THROUGH;
    if (r - margin > (double)r_far) return SF_VIS_OCCLUDED;
    return SF_VIS_WITHIN;
}

// MAP: pts = float4 [n] of the index (w = the original index); otherwise float [n][3], the index is the position.
// cls / seen / within / keep may each be nullptr.  stat: outside, unknown, within, occluded, seen through, removed, finite points.
template <bool MAP>
__global__ __launch_bounds__(256) void k_vis_votes(const void *__restrict__ pts, int64_t n, const VisImage *__restrict__ imgs, int B, VisWin w, uint8_t *__restrict__ cls,
                                                   uint16_t *__restrict__ seen, uint16_t *__restrict__ within, uint8_t *__restrict__ keep, int min_seen, int max_within,
                                                   unsigned long long *__restrict__ stat)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool have = i < n;
    float xf = 0.0f, yf = 0.0f, zf = 0.0f;
    uint32_t idx = (uint32_t)i;
    if (have) {
        if (MAP) {
            const float4 p = reinterpret_cast<const float4 *>(pts)[i];
            xf = p.x; yf = p.y; zf = p.z;
            idx = __float_as_uint(p.w);
        } else {
            const float *q = reinterpret_cast<const float *>(pts) + 3 * i;
            xf = q[0]; yf = q[1]; zf = q[2];
        }
    }
    const bool fin = have && isfinite(xf) && isfinite(yf) && isfinite(zf);
    uint32_t cnt[5] = {0u, 0u, 0u, 0u, 0u};
    int last = SF_VIS_OUTSIDE;
    for (int b = 0; b < B; ++b) {
        int code = SF_VIS_OUTSIDE;
        if (fin) code = vis_classify(imgs[b], w, xf, yf, zf);
        last = code;
        if (have) {
#pragma unroll
            for (int k = 0; k < 5; ++k) cnt[k] += code == k ? 1u : 0u;
        }
    }
    bool removed = false;
    if (have) {
        removed = (int)cnt[SF_VIS_SEEN_THROUGH] >= min_seen && (int)cnt[SF_VIS_WITHIN] <= max_within;
        if (cls) cls[idx] = (uint8_t)last;
        if (seen) seen[idx] = (uint16_t)cnt[SF_VIS_SEEN_THROUGH];
        if (within) within[idx] = (uint16_t)cnt[SF_VIS_WITHIN];
        if (keep) keep[idx] = removed ? 0 : 1;
    }
    uint32_t tot[7];
#pragma unroll
    for (int k = 0; k < 5; ++k) tot[k] = wave_sum_u32(cnt[k]);
    tot[5] = (uint32_t)__popcll(__ballot(removed));
    tot[6] = (uint32_t)__popcll(__ballot(fin));
    block_add<7>(tot, stat);
}

struct Events { // profile: hipEvents around the kernels; the time is read after the stream was synchronised
    hipEvent_t ev[2] = {nullptr, nullptr};
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
    int ms(float *out)
    {
        *out = -1.0f;
        if (on) SF_HIP(hipEventElapsedTime(out, ev[0], ev[1]));
        return SF_OK;
    }
};

// the first `words` counters of a call, summed over the copies; synchronises the stream
int read_stat(sf_ctx *ctx, const unsigned long long *d_stat, int words, unsigned long long *out)
{
    unsigned long long h[VIS_SLOTS * VIS_WORDS];
    SF_HIP(hipMemcpyAsync(h, d_stat, VIS_STAT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < words; ++k) {
        out[k] = 0;
        for (int slot = 0; slot < VIS_SLOTS; ++slot) out[k] += h[slot * VIS_WORDS + k];
    }
    return SF_OK;
}

bool pose_finite(const double *T)
{
    if (!T) return true;
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(T[k])) return false;
    return true;
}

int check_image_params(const sf_range_image_params *p)
{
    SF_CHECK(p, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(p->width >= 1 && p->width <= 16384 && p->height >= 1 && p->height <= 4096, SF_ERR_INVALID, "range image: width must be 1 .. 16384 and height 1 .. 4096 (got %d x %d)",
             (int)p->width, (int)p->height);
    SF_CHECK(std::isfinite(p->el_min) && std::isfinite(p->el_max) && std::isfinite(p->min_range) && std::isfinite(p->max_range) && std::isfinite(p->el_max - p->el_min),
             SF_ERR_INVALID, "range image: the bounds must be finite");
    SF_CHECK(p->el_min < p->el_max, SF_ERR_INVALID, "range image: el_min must be below el_max (got %g, %g)", p->el_min, p->el_max);
    SF_CHECK(p->min_range >= 0.0 && p->max_range > p->min_range, SF_ERR_INVALID, "range image: 0 <= min_range < max_range (got %g, %g)", p->min_range, p->max_range);
    return SF_OK;
}

VisImage image_arg(const sf_range_image *img, const double *T)
{
    static const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (!T) T = I;
    VisImage g{};
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) g.a[3 * r + k] = T[4 * k + r];
        g.t[r] = T[4 * r + 3];
    }
    g.el_min = img->prm.el_min;
    g.el_span = img->prm.el_max - img->prm.el_min;
    g.min_range = img->prm.min_range;
    g.max_range = img->prm.max_range;
    g.rng = img->rng.as<uint32_t>();
    g.W = img->prm.width;
    g.H = img->prm.height;
    return g;
}

inline int64_t image_pixels(const sf_range_image *img) { return (int64_t)img->prm.width * (int64_t)img->prm.height; }

int image_clear(sf_range_image *img)
{
    const size_t npix = (size_t)image_pixels(img);
    SF_HIP(hipMemsetAsync(img->keys.p, 0xFF, sizeof(unsigned long long) * npix, img->ctx->stream));
    SF_HIP(hipMemsetAsync(img->rng.p, 0xFF, sizeof(uint32_t) * npix, img->ctx->stream));
    return SF_OK;
}

// everything a classify call is refused for, before anything is touched
int check_visibility(sf_ctx *ctx, sf_range_image *const *imgs, const double *poses, int64_t n_images, const sf_visibility_params *p)
{
    SF_CHECK(ctx && imgs && p, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(n_images >= 1 && n_images <= VIS_MAX_IMAGES, SF_ERR_INVALID, "visibility: n_images must be 1 .. %d (got %lld)", VIS_MAX_IMAGES, (long long)n_images);
    SF_CHECK(p->half_cols >= 0 && p->half_rows >= 0, SF_ERR_INVALID, "visibility: the window must not be negative (got %d, %d)", (int)p->half_cols, (int)p->half_rows);
    const int64_t window = (2 * (int64_t)p->half_cols + 1) * (2 * (int64_t)p->half_rows + 1);
    SF_CHECK(p->min_hits >= 1 && (int64_t)p->min_hits <= window, SF_ERR_INVALID, "visibility: min_hits must be 1 .. the pixels of the window (got %d)", (int)p->min_hits);
    SF_CHECK(std::isfinite(p->range_margin) && std::isfinite(p->range_ratio) && p->range_margin >= 0.0 && p->range_ratio >= 0.0, SF_ERR_INVALID,
             "visibility: the margin and the ratio must be finite and not negative (got %g, %g)", p->range_margin, p->range_ratio);
    for (int64_t b = 0; b < n_images; ++b) {
        SF_CHECK(imgs[b], SF_ERR_INVALID, "visibility: image %lld is NULL", (long long)b);
        SF_CHECK(imgs[b]->ctx == ctx, SF_ERR_INVALID, "visibility: image %lld belongs to another context", (long long)b);
        SF_CHECK(2 * (int64_t)p->half_cols + 1 <= (int64_t)imgs[b]->prm.width, SF_ERR_INVALID, "visibility: the window is wider than image %lld", (long long)b);
        SF_CHECK(pose_finite(poses ? poses + 16 * b : nullptr), SF_ERR_INVALID, "visibility: pose %lld is not finite", (long long)b);
    }
    return SF_OK;
}

struct VisOut { // device outputs of one classify call, each optional
    uint8_t *cls = nullptr;
    uint16_t *seen = nullptr, *within = nullptr;
    uint8_t *keep = nullptr;
};

// The one classify launch, for the map's pts4 (MAP) or a cloud's float3s, n > 0 points; *h gets the seven counters.  The caller has
// checked the arguments (check_visibility) and set the device.  Synchronises the stream.
template <bool MAP>
int votes_device(sf_ctx *ctx, const void *pts, int64_t n, sf_range_image *const *imgs, const double *poses, int64_t n_images, const sf_visibility_params *p, const VisOut &o,
                 int min_seen, int max_within, bool profile, unsigned long long h[7], float *device_ms)
{
    hipStream_t s = ctx->stream;
    std::vector<VisImage> arg((size_t)n_images);
    for (int64_t b = 0; b < n_images; ++b) arg[(size_t)b] = image_arg(imgs[b], poses ? poses + 16 * b : nullptr);
    sf::DevBuf d_arg; // the images and, behind them, the counters
    const size_t arg_b = (sizeof(VisImage) * arg.size() + 255) & ~size_t(255);
    SF_TRY(d_arg.reserve(arg_b + VIS_STAT_BYTES));
    unsigned long long *d_stat = reinterpret_cast<unsigned long long *>(d_arg.as<char>() + arg_b);
    SF_TRY(sf::upload_staged(ctx, d_arg.p, arg.data(), sizeof(VisImage) * arg.size()));
    SF_HIP(hipMemsetAsync(d_stat, 0, VIS_STAT_BYTES, s));
    const VisWin w{p->half_cols, p->half_rows, p->min_hits, 0, p->range_margin, p->range_ratio};
    Events ev;
    SF_TRY(ev.start(profile));
    SF_TRY(ev.mark(0, s));
    hipLaunchKernelGGL(k_vis_votes<MAP>, dim3(nblk(n)), dim3(256), 0, s, pts, n, d_arg.as<VisImage>(), (int)n_images, w, o.cls, o.seen, o.within, o.keep, min_seen, max_within,
                       d_stat);
    SF_HIP(hipGetLastError());
    SF_TRY(ev.mark(1, s));
    SF_TRY(read_stat(ctx, d_stat, 7, h));
    SF_TRY(ev.ms(device_ms));
    return SF_OK;
}

sf_visibility_stats stats_from(int64_t n_points, int64_t n_valid, const unsigned long long h[7], float device_ms)
{
    sf_visibility_stats st{};
    st.n_points = n_points;
    st.n_valid = n_valid;
    st.n_outside = (int64_t)h[SF_VIS_OUTSIDE];
    st.n_unknown = (int64_t)h[SF_VIS_UNKNOWN];
    st.n_within = (int64_t)h[SF_VIS_WITHIN];
    st.n_occluded = (int64_t)h[SF_VIS_OCCLUDED];
    st.n_seen_through = (int64_t)h[SF_VIS_SEEN_THROUGH];
    st.n_removed = (int64_t)h[5];
    st.device_ms = device_ms;
    return st;
}

// the two map forms: cls (one image) or the two vote arrays, original order, [m->n] on the host
int map_votes(sf_map *m, sf_range_image *const *imgs, const double *poses, int64_t n_images, const sf_visibility_params *p, uint8_t *cls, uint16_t *seen, uint16_t *within,
              sf_visibility_stats *stats)
{
    SF_CHECK(m, SF_ERR_INVALID, "bad arguments");
    SF_TRY(check_visibility(m->ctx, imgs, poses, n_images, p));
    SF_CHECK(m->built, SF_ERR_STATE, "map not built");
    sf_ctx *ctx = m->ctx;
    const int64_t n = m->n, nv = m->grid.n;
    unsigned long long h[7] = {0, 0, 0, 0, 0, 0, 0};
    float ms = -1.0f;
    if (n > 0) {
        SF_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        // the points the index does not hold (not finite) keep what the fill gives them: OUTSIDE, no vote
        sf::DevBuf d_cls, d_seen, d_within;
        VisOut o;
        if (cls) {
            SF_TRY(d_cls.reserve((size_t)n));
            SF_HIP(hipMemsetAsync(d_cls.p, SF_VIS_OUTSIDE, (size_t)n, s));
            o.cls = d_cls.as<uint8_t>();
        }
        if (seen) {
            SF_TRY(d_seen.reserve(sizeof(uint16_t) * (size_t)n));
            SF_HIP(hipMemsetAsync(d_seen.p, 0, sizeof(uint16_t) * (size_t)n, s));
            o.seen = d_seen.as<uint16_t>();
        }
        if (within) {
            SF_TRY(d_within.reserve(sizeof(uint16_t) * (size_t)n));
            SF_HIP(hipMemsetAsync(d_within.p, 0, sizeof(uint16_t) * (size_t)n, s));
            o.within = d_within.as<uint16_t>();
        }
        if (nv > 0) SF_TRY(votes_device<true>(ctx, m->pts4.p, nv, imgs, poses, n_images, p, o, 1, 0, p->profile != 0 || m->profile, h, &ms));
        h[SF_VIS_OUTSIDE] += (unsigned long long)(n - nv) * (unsigned long long)n_images;
        if (cls) SF_HIP(hipMemcpyAsync(cls, d_cls.p, (size_t)n, hipMemcpyDeviceToHost, s));
        if (seen) SF_HIP(hipMemcpyAsync(seen, d_seen.p, sizeof(uint16_t) * (size_t)n, hipMemcpyDeviceToHost, s));
        if (within) SF_HIP(hipMemcpyAsync(within, d_within.p, sizeof(uint16_t) * (size_t)n, hipMemcpyDeviceToHost, s));
        SF_HIP(hipStreamSynchronize(s));
    }
    h[5] = 0; // n_removed: nothing leaves a map
    if (stats) *stats = stats_from(n, nv, h, ms);
    return SF_OK;
}

} // namespace

extern "C" void sf_range_image_default_params(sf_range_image_params *p)
{
    if (!p) return;
    *p = sf_range_image_params{2048, 64, -25.0 * VIS_PI / 180.0, 3.0 * VIS_PI / 180.0, 0.5, 120.0};
}

extern "C" void sf_visibility_default_params(sf_visibility_params *p)
{
    if (!p) return;
    *p = sf_visibility_params{1, 1, 1, 0, 0.2, 0.01};
}

extern "C" int sf_range_image_create(sf_ctx *ctx, const sf_range_image_params *p, sf_range_image **out)
{
    SF_CHECK(ctx && out, SF_ERR_INVALID, "bad arguments");
    SF_TRY(check_image_params(p));
    SF_HIP(hipSetDevice(ctx->device));
    sf_range_image *img = new (std::nothrow) sf_range_image();
    SF_CHECK(img, SF_ERR_NOMEM, "out of host memory");
    img->ctx = ctx;
    img->prm = *p;
    const size_t npix = (size_t)image_pixels(img);
    int rc = img->keys.reserve(sizeof(unsigned long long) * npix);
    if (rc == SF_OK) rc = img->rng.reserve(sizeof(uint32_t) * npix);
    if (rc == SF_OK) rc = img->stat.reserve(VIS_STAT_BYTES);
    if (rc == SF_OK) rc = image_clear(img);
    if (rc != SF_OK) {
        delete img;
        return rc;
    }
    sf::ctx_retain(ctx);
    *out = img;
    return SF_OK;
}

extern "C" void sf_range_image_destroy(sf_range_image *img)
{
    if (!img) return;
    hipError_t e = hipStreamSynchronize(img->ctx->stream);
    (void)e;
    sf_ctx *ctx = img->ctx;
    delete img;
    sf::ctx_release(ctx);
}

extern "C" int sf_range_image_info(const sf_range_image *img, sf_range_image_params *p)
{
    SF_CHECK(img && p, SF_ERR_INVALID, "bad arguments");
    *p = img->prm;
    return SF_OK;
}

extern "C" int sf_range_image_build(sf_range_image *img, sf_cloud *c, const double *pose, sf_range_image_stats *stats)
{
    SF_CHECK(img && c, SF_ERR_INVALID, "bad arguments");
    SF_CHECK(img->ctx == c->ctx, SF_ERR_INVALID, "range image: the cloud belongs to another context");
    SF_CHECK(pose_finite(pose), SF_ERR_INVALID, "range image: the pose is not finite");
    SF_CHECK(c->n < (int64_t(1) << 31), SF_ERR_INVALID, "range image: the cloud must hold fewer than 2^31 points");
    sf_ctx *ctx = img->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t n = c->n, npix = image_pixels(img);
    unsigned long long *d_stat = img->stat.as<unsigned long long>();
    Events ev;
    SF_TRY(ev.start(true));
    SF_TRY(ev.mark(0, s));
    SF_HIP(hipMemsetAsync(d_stat, 0, VIS_STAT_BYTES, s));
    SF_HIP(hipMemsetAsync(img->keys.p, 0xFF, sizeof(unsigned long long) * (size_t)npix, s));
    if (n > 0)
        hipLaunchKernelGGL(k_ri_build, dim3(nblk(n)), dim3(256), 0, s, c->xyz.as<float>(), n, image_arg(img, pose), img->keys.as<unsigned long long>(), d_stat);
    hipLaunchKernelGGL(k_ri_finish, dim3(nblk(npix)), dim3(256), 0, s, img->keys.as<unsigned long long>(), npix, img->rng.as<uint32_t>(), d_stat);
    SF_HIP(hipGetLastError());
    SF_TRY(ev.mark(1, s));
    unsigned long long h[4];
    SF_TRY(read_stat(ctx, d_stat, 4, h));
    if (stats) {
        sf_range_image_stats st{};
        st.n_points = n;
        st.n_projected = (int64_t)h[0];
        st.n_outside = (int64_t)h[1];
        st.n_nonfinite = (int64_t)h[2];
        st.n_filled = (int64_t)h[3];
        SF_TRY(ev.ms(&st.device_ms));
        *stats = st;
    }
    return SF_OK;
}

extern "C" int sf_range_image_download(sf_range_image *img, float *range, int32_t *index)
{
    SF_CHECK(img, SF_ERR_INVALID, "bad arguments");
    if (!range && !index) return SF_OK;
    sf_ctx *ctx = img->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    const size_t npix = (size_t)image_pixels(img);
    std::vector<unsigned long long> keys(npix);
    SF_HIP(hipMemcpyAsync(keys.data(), img->keys.p, sizeof(unsigned long long) * npix, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t k = 0; k < npix; ++k) { // the keys split on the host: an empty pixel is +inf and -1
        const bool filled = keys[k] != ~0ull;
        if (range) {
            const uint32_t bits = filled ? (uint32_t)(keys[k] >> 32) : 0x7f800000u;
            std::memcpy(range + k, &bits, sizeof(bits));
        }
        if (index) index[k] = filled ? (int32_t)(uint32_t)(keys[k] & 0xffffffffull) : -1;
    }
    return SF_OK;
}

extern "C" int sf_map_visibility(sf_map *m, sf_range_image *img, const double *pose, const sf_visibility_params *p, uint8_t *cls, sf_visibility_stats *stats)
{
    sf_range_image *const imgs[1] = {img};
    SF_CHECK(img, SF_ERR_INVALID, "bad arguments");
    return map_votes(m, imgs, pose, 1, p, cls, nullptr, nullptr, stats);
}

extern "C" int sf_map_visibility_votes(sf_map *m, sf_range_image *const *imgs, const double *poses, int64_t n_images, const sf_visibility_params *p, uint16_t *seen_through,
                                       uint16_t *within, sf_visibility_stats *stats)
{
    return map_votes(m, imgs, poses, n_images, p, nullptr, seen_through, within, stats);
}

extern "C" int sf_cloud_remove_seen_through(sf_cloud *c, sf_range_image *const *imgs, const double *poses, int64_t n_images, const sf_visibility_params *p, int min_seen,
                                            int max_within, sf_visibility_stats *stats)
{
    SF_CHECK(c, SF_ERR_INVALID, "bad arguments");
    SF_TRY(check_visibility(c->ctx, imgs, poses, n_images, p));
    SF_CHECK(min_seen >= 1 && max_within >= 0, SF_ERR_INVALID, "remove_seen_through: min_seen must be >= 1 and max_within >= 0 (got %d, %d)", min_seen, max_within);
    SF_CHECK(c->n < (int64_t(1) << 31), SF_ERR_INVALID, "remove_seen_through: the cloud must hold fewer than 2^31 points");
    unsigned long long h[7] = {0, 0, 0, 0, 0, 0, 0};
    float ms = -1.0f;
    const int64_t n = c->n;
    sf::cloud_touch(c);
    if (n == 0) {
        c->n_last_idx = 0;
        if (stats) *stats = stats_from(0, 0, h, ms);
        return SF_OK;
    }
    sf_ctx *ctx = c->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    SF_TRY(c->flags.reserve((size_t)n));
    VisOut o;
    o.keep = c->flags.as<uint8_t>();
    SF_TRY(votes_device<false>(ctx, c->xyz.p, n, imgs, poses, n_images, p, o, min_seen, max_within, p->profile != 0, h, &ms));
    SF_TRY(sf::compact_cloud(c, c->flags.as<uint8_t>()));
    if (stats) *stats = stats_from(n, (int64_t)h[6], h, ms);
    return SF_OK;
}
