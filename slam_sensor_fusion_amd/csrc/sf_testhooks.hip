// sf_testhooks.hip — test hooks of the C ABI (gfx950): the radix sort and the device scans of sf_sort.hpp, run directly
// on host arrays.  Not part of the drop-in boundary and no reference counterpart: the reference sorts inside
// pcl::VoxelGrid (global_map_frames_manager.cpp:142-146).  The hooks launch exactly sf::radix_sort_pairs<K> /
// sf::scan_u32<OP> on the context's stream -- no copy of the kernels, no second implementation -- so that a test can
// compare them with numpy at the sizes, key distributions and pointer alignments the entry points never produce.
// And the launch schedule of an alignment (sf_schedule.hpp), evaluated on the host alone: sf_test_launch_schedule.
// And the stream compaction and the bounds reduction of sf_cloud.hip, run on a cloud with flags / points of the test's own
// choosing: sf_test_compact (sf::compact_cloud), sf_test_cloud_minmax (sf::cloud_minmax, sf::cloud_minmax_enqueue).
//
// Every device array of a run is carved from ONE allocation as [guard | lead | n elements | guard]: a guard is
// GUARD elements, the front one ends on a 16-byte boundary, `lead` elements displace the first element from it (the
// vector branch of k_sort_hist needs lead * sizeof(element) to be a multiple of 16).  Guards and leads are filled with
// a byte pattern before the run; afterwards the 32-bit words of them that no longer hold it are counted: an overrun of
// up to a tile (4096 elements) in either direction is seen and stays inside the hook's own allocation.
#include "sf_common.hpp"

#include "sf_sort.hpp"
#include "sf_schedule.hpp"

namespace {

constexpr int64_t GUARD = 4096;             // elements on either side of every array: one tile of the large instantiation
constexpr int64_t TEST_MAX_N = (int64_t)1 << 26;
constexpr int GUARD_BYTE = 0xA5;
constexpr uint32_t GUARD_WORD = 0xA5A5A5A5u;

// one array inside the allocation
struct Carve {
    size_t off = 0, elem = 0; // byte offset of the front guard (a multiple of 16); element size
    int64_t lead = 0, n = 0;
    size_t front_bytes() const { return (size_t)(GUARD + lead) * elem; }
    size_t data_off() const { return off + front_bytes(); }
    size_t data_bytes() const { return (size_t)n * elem; }
    size_t back_off() const { return data_off() + data_bytes(); }
    size_t back_bytes() const { return (size_t)GUARD * elem; }
    size_t end() const { return (back_off() + back_bytes() + 15u) & ~(size_t)15u; }
};

Carve carve_after(size_t off, size_t elem, int64_t lead, int64_t n)
{
    Carve c;
    c.off = off; c.elem = elem; c.lead = lead; c.n = n;
    return c;
}

// words of the guards of `c` that no longer hold the pattern, added to *damage (synchronises the stream)
int count_guard_damage(sf_ctx *ctx, const char *base, const Carve &c, std::vector<uint32_t> &host, int64_t *damage)
{
    const size_t off[2] = {c.off, c.back_off()}, bytes[2] = {c.front_bytes(), c.back_bytes()};
    for (int side = 0; side < 2; ++side) {
        host.assign(bytes[side] / sizeof(uint32_t), 0u);
        SF_HIP(hipMemcpyAsync(host.data(), base + off[side], bytes[side], hipMemcpyDeviceToHost, ctx->stream));
        SF_HIP(hipStreamSynchronize(ctx->stream));
        for (uint32_t w : host) *damage += (w != GUARD_WORD);
    }
    return SF_OK;
}

template <class K>
int run_sort(sf_ctx *ctx, const void *keys, const uint32_t *vals, int64_t n, unsigned end_bit, int lead, int lead_alt, void *keys_out, uint32_t *vals_out, int64_t *guard_damage)
{
    Carve a[4]; // keys, alt keys, vals, alt vals
    a[0] = carve_after(0, sizeof(K), lead, n);
    a[1] = carve_after(a[0].end(), sizeof(K), lead_alt, n);
    a[2] = carve_after(a[1].end(), sizeof(uint32_t), lead, n);
    a[3] = carve_after(a[2].end(), sizeof(uint32_t), lead_alt, n);
    const int narr = vals ? 4 : 2;
    const size_t total = a[narr - 1].end();
    sf::DevBuf buf; // freed on every path
    SF_TRY(buf.reserve(total));
    char *base = buf.as<char>();
    hipStream_t st = ctx->stream;
    SF_HIP(hipMemsetAsync(base, GUARD_BYTE, total, st));
    SF_TRY(sf::upload_staged(ctx, base + a[0].data_off(), keys, a[0].data_bytes()));
    if (vals) SF_TRY(sf::upload_staged(ctx, base + a[2].data_off(), vals, a[2].data_bytes()));
    K *sk = nullptr;
    uint32_t *sv = nullptr;
    SF_TRY(sf::radix_sort_pairs<K>(ctx, reinterpret_cast<K *>(base + a[0].data_off()), reinterpret_cast<K *>(base + a[1].data_off()),
                                   vals ? reinterpret_cast<uint32_t *>(base + a[2].data_off()) : nullptr, vals ? reinterpret_cast<uint32_t *>(base + a[3].data_off()) : nullptr, n,
                                   end_bit, &sk, &sv));
    if (n > 0) {
        SF_HIP(hipMemcpyAsync(keys_out, sk, a[0].data_bytes(), hipMemcpyDeviceToHost, st));
        if (vals) SF_HIP(hipMemcpyAsync(vals_out, sv, a[2].data_bytes(), hipMemcpyDeviceToHost, st));
    }
    SF_HIP(hipStreamSynchronize(st));
    int64_t damage = 0;
    std::vector<uint32_t> host;
    for (int k = 0; k < narr; ++k) SF_TRY(count_guard_damage(ctx, base, a[k], host, &damage));
    SF_HIP(hipGetLastError());
    *guard_damage = damage;
    return SF_OK;
}

} // namespace

extern "C" int sf_test_radix_sort(sf_ctx *ctx, int key_bytes, const void *keys, const uint32_t *vals, int64_t n, unsigned end_bit, int lead, int lead_alt, void *keys_out,
                                  uint32_t *vals_out, int64_t *guard_damage)
{
    SF_CHECK(ctx && guard_damage, SF_ERR_INVALID, "sf_test_radix_sort: ctx or guard_damage is NULL");
    SF_CHECK(key_bytes == 4 || key_bytes == 8, SF_ERR_INVALID, "sf_test_radix_sort: key_bytes %d (4 or 8)", key_bytes);
    SF_CHECK(n >= 0 && n <= TEST_MAX_N, SF_ERR_INVALID, "sf_test_radix_sort: n %lld outside [0, 2^26]", (long long)n);
    SF_CHECK(end_bit <= 8u * (unsigned)key_bytes && (end_bit > 0 || n <= 1), SF_ERR_INVALID, "sf_test_radix_sort: end_bit %u outside [1, %d]", end_bit, 8 * key_bytes);
    SF_CHECK(lead >= 0 && lead <= 3 && lead_alt >= 0 && lead_alt <= 3, SF_ERR_INVALID, "sf_test_radix_sort: lead %d / lead_alt %d outside [0, 3]", lead, lead_alt);
    SF_CHECK((keys && keys_out) || n == 0, SF_ERR_INVALID, "sf_test_radix_sort: keys or keys_out is NULL");
    SF_CHECK((vals == nullptr) == (vals_out == nullptr), SF_ERR_INVALID, "sf_test_radix_sort: vals and vals_out go together (both NULL: keys only)");
    SF_HIP(hipSetDevice(ctx->device));
    if (key_bytes == 4) return run_sort<uint32_t>(ctx, keys, vals, n, end_bit, lead, lead_alt, keys_out, vals_out, guard_damage);
    return run_sort<uint64_t>(ctx, keys, vals, n, end_bit, lead, lead_alt, keys_out, vals_out, guard_damage);
}

// the launch schedule (sf_schedule.hpp) row by row: host code alone, no context and no device
extern "C" int sf_test_launch_schedule(const int32_t *in, int64_t rows, int k, int32_t *out)
{
    SF_CHECK((in && out) || rows == 0, SF_ERR_INVALID, "sf_test_launch_schedule: in or out is NULL");
    SF_CHECK(rows >= 0, SF_ERR_INVALID, "sf_test_launch_schedule: rows %lld < 0", (long long)rows);
    for (int64_t r = 0; r < rows; ++r) {
        const int32_t *v = in + r * SF_TEST_SCHEDULE_IN;
        sf::Schedule s;
        s.mode = v[0]; s.K = v[1]; s.qpl = v[2]; s.sharded = v[3]; s.whole = v[4]; s.reuse = v[5]; s.window = v[6]; s.robust = v[7]; s.wanted = v[8]; s.fz_from = v[9];
        s.defer = v[10]; s.table = v[11]; s.nbr_from = v[12]; s.lk_min = v[13]; s.tile_on = v[14];
        s = sf::make_schedule(s);
        const sf::LaunchStep st = sf::step_of(s, k);
        const int32_t o[SF_TEST_SCHEDULE_OUT] = {sf::launches(s), st.nn, st.one_per_lane, st.solve_takes_freeze_state, st.ask_freeze, st.deferred_rows, st.attempt_from,
                                                 s.fz, s.lookup_first, s.defer_first};
        std::memcpy(out + r * SF_TEST_SCHEDULE_OUT, o, sizeof(o));
    }
    return SF_OK;
}

extern "C" int sf_test_scan_u32(sf_ctx *ctx, int op, const uint32_t *in, int64_t n, uint32_t carry0, int in_place, uint32_t *out, int64_t *guard_damage)
{
    SF_CHECK(ctx && guard_damage, SF_ERR_INVALID, "sf_test_scan_u32: ctx or guard_damage is NULL");
    SF_CHECK(op == 0 || op == 1, SF_ERR_INVALID, "sf_test_scan_u32: op %d (0: exclusive sum, 1: inclusive max)", op);
    SF_CHECK(n >= 0 && n <= TEST_MAX_N, SF_ERR_INVALID, "sf_test_scan_u32: n %lld outside [0, 2^26]", (long long)n);
    SF_CHECK((in && out) || n == 0, SF_ERR_INVALID, "sf_test_scan_u32: in or out is NULL");
    SF_HIP(hipSetDevice(ctx->device));
    Carve a[2]; // in, out (in place: one array)
    a[0] = carve_after(0, sizeof(uint32_t), 0, n);
    a[1] = carve_after(a[0].end(), sizeof(uint32_t), 0, n);
    const int narr = in_place ? 1 : 2;
    const size_t total = a[narr - 1].end();
    sf::DevBuf buf; // freed on every path
    SF_TRY(buf.reserve(total));
    char *base = buf.as<char>();
    hipStream_t st = ctx->stream;
    SF_HIP(hipMemsetAsync(base, GUARD_BYTE, total, st));
    SF_TRY(sf::upload_staged(ctx, base + a[0].data_off(), in, a[0].data_bytes()));
    const uint32_t *d_in = reinterpret_cast<const uint32_t *>(base + a[0].data_off());
    uint32_t *d_out = reinterpret_cast<uint32_t *>(base + a[narr - 1].data_off());
    if (op == 0) SF_TRY(sf::scan_u32<0>(ctx, d_in, d_out, n, carry0));
    else SF_TRY(sf::scan_u32<1>(ctx, d_in, d_out, n, carry0));
    if (n > 0) SF_HIP(hipMemcpyAsync(out, d_out, a[0].data_bytes(), hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    int64_t damage = 0;
    std::vector<uint32_t> host;
    for (int k = 0; k < narr; ++k) SF_TRY(count_guard_damage(ctx, base, a[k], host, &damage));
    SF_HIP(hipGetLastError());
    *guard_damage = damage;
    return SF_OK;
}

// the compaction behind every crop and filter, with the caller's flags: what the crops do after their predicate kernel
extern "C" int sf_test_compact(sf_cloud *c, const uint8_t *flags)
{
    SF_CHECK(c, SF_ERR_INVALID, "sf_test_compact: c is NULL");
    SF_CHECK(flags || c->n == 0, SF_ERR_INVALID, "sf_test_compact: flags is NULL");
    SF_HIP(hipSetDevice(c->ctx->device));
    if (c->n > 0) {
        SF_TRY(c->flags.reserve((size_t)c->n));
        SF_TRY(sf::upload_staged(c->ctx, c->flags.p, flags, (size_t)c->n));
    }
    sf::cloud_touch(c);
    return sf::compact_cloud(c, c->flags.as<uint8_t>());
}

// the bounds of the finite points in either form; the enqueue form writes into a buffer that starts as the guard pattern
extern "C" int sf_test_cloud_minmax(sf_cloud *c, int enqueue_form, float mn[3], float mx[3], int64_t *n_finite)
{
    SF_CHECK(c && mn && mx && n_finite, SF_ERR_INVALID, "sf_test_cloud_minmax: a NULL argument");
    sf_ctx *ctx = c->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    if (!enqueue_form) {
        sf::MinMaxHost h;
        SF_TRY(sf::cloud_minmax(ctx, c->xyz.as<float>(), c->n, &h));
        for (int d = 0; d < 3; ++d) { mn[d] = h.mn[d]; mx[d] = h.mx[d]; }
        *n_finite = h.n_finite;
        return SF_OK;
    }
    sf::DevBuf buf; // freed on every path
    SF_TRY(buf.reserve(sizeof(sf::MinMaxDev)));
    SF_HIP(hipMemsetAsync(buf.p, GUARD_BYTE, sizeof(sf::MinMaxDev), ctx->stream));
    SF_TRY(sf::cloud_minmax_enqueue(ctx, c->xyz.as<float>(), c->n, buf.as<sf::MinMaxDev>()));
    sf::MinMaxDev h;
    SF_HIP(hipMemcpyAsync(&h, buf.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    for (int d = 0; d < 3; ++d) { mn[d] = h.mn[d]; mx[d] = h.mx[d]; }
    *n_finite = (int64_t)h.cnt;
    return SF_OK;
}
