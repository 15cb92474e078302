// sf_radius.hpp — "everything within r" with variable-length rows: sf_map_radius_search (arbitrary queries, the window honoured) and
// sf_map_radius_graph (the map's own points, the window ignored), gfx950.  A fragment of sf_map.hip, included behind the outlier
// block: it uses radius_reach, ProfSpan / prof_read and read_words from there.  DESIGN §27.
//
// Row i holds every indexed point p the window accepts with l2_simple(q_i, p) < r2, r2 = (float)(radius * radius): the float32,
// unfused, strict rule of sf_map_nn / sf_map_knn / sf_map_radius_outliers.  Four steps on the context's stream:
//   count   one lane per row on radius_walk (sf_walk.hpp); count[row], and per workgroup one add each to the 64-bit total, the
//           maximum, the rows searched and the empty rows (in one of RAD_SLOTS groups; k_rad_combine folds the groups)
//   scan    scan_u32<0> over count[0 .. rows] (the last entry is 0: offsets[rows] = the total); the four counters are read back --
//           the call's one host synchronisation before the fill -- and a total the 32-bit offsets cannot hold is refused there
//   fill    the same walk again, writing (id, d2) from offsets[row] on.  Two forms with the same bytes: one lane per row
//           (k_rad_fill_lane: radius_walk, a lane's stores are a whole row apart from its neighbour's), and one wave per row
//           (k_rad_fill_wave: radius_runs, the lanes take consecutive candidates of each x-run, a ballot and the count of the hits
//           below a lane give its slot, the stores of a trip are contiguous).  Rows of cells are walked in memory order and hits are
//           compacted in lane order, so both leave a row in ascending position in the index.
//   sort    SF_RADIUS_ORDER_DISTANCE only: the fill writes the key (row << 32) | bits(d2) beside the id, one stable
//           radix_sort_pairs<uint64_t> over all entries (end_bit = 32 + the bits of rows - 1) orders them by (row, d2, position) --
//           d2 >= 0, so its bits order as its value does, and the position is the order the fill left -- and k_rad_unpack copies
//           the keys' low words out as the d2 array.  This is the order of sf_map_knn: the first 64 entries of a row are its list.
//
// Queries outside the grid.  radius_walk's argument (sf_walk.hpp (a) - (d)) is stated for indexed points, whose grid coordinate
// G(x) = fl(fl(x - org) * inv_h) has |G| < dim (1 + u).  A query may lie anywhere (sf_map_knn accepts such queries too).  Write
// out_a >= 0 for the number of cells the query lies beyond the grid on axis a.
//   Within reach.  |G(q)| < dim + out_a + 1, so the rounding of G(q) is 2u (dim + out_a) instead of 2u dim: (b) becomes
//   |G(q) - G(p)| <= |q - p| inv_h + 2^-22 dim (1 + 3u) + 2u out_a.  The first two terms are what gap_eps = 1.5 * 2^-22 maxdim h
//   already carries.  The new one is relative: every indexed point lies inside the grid, so every face the walk measures a gap to is
//   at least out_a cells away and any accepted point has out_a <= r inv_h (1 + 2u) <= R + 1 -- 2u out_a is at most 2u of the gap
//   (d) compares, which the 0.998 factor covers a thousand times over (it spends 13u), and at most 2u of r inv_h in the reach (c),
//   which the 1e-6 there covers beside the 2u of (a).  The cell of the query is the clamp of floor(G(q)), and (c) already says
//   that a clamp only brings cells closer.
//   Beyond reach.  The clamped cell has gap 0 to itself, so the walk would still read the face cells and have the rule reject
//   every candidate.  beyond_reach decides it first: e_a = safe_gap(max(-G_a, G_a - dim_a, 0) h, gap_eps) is a lower bound of the
//   axis distance to every indexed point (they have 0 <= (x - org) inv_h <= dim (1 + 3u); the rounding of G(q) is again 2u dim,
//   inside gap_eps, plus 2u of e_a itself), and when (e_x^2 + e_y^2 + e_z^2) * 0.998 >= r2 the rule rejects everything as in (d):
//   the row is empty without a walk.
//   Overflow.  For a finite query x - org is finite or +-inf, never NaN, and inv_h > 0 is finite, so G is finite or +-inf.
//   max(-G, G - dim, 0) is then +inf (never inf - inf: dim is finite), e_a = +inf, the sum +inf, and +inf * 0.998 >= r2: beyond
//   reach, before grid_cell or cell_gap see the value.  A non-finite query never gets this far (an empty row).  No NaN reaches a
//   comparison.
#pragma once

namespace {

// sf_map::rad_red: RAD_SLOTS groups of the four counters, 128 bytes apart as the kept counters of the outlier block are (a workgroup
// adds to the group of its index: one line's queue of atomics is RAD_SLOTS times shorter), and behind them their combination
enum { RAD_TOTAL = 0, RAD_MAX = 1, RAD_SEARCHED = 2, RAD_EMPTY = 3, RAD_WORDS = 4, RAD_SLOTS = 256, RAD_STRIDE = 16, RAD_RED_WORDS = (RAD_SLOTS + 1) * RAD_STRIDE };

__device__ __forceinline__ bool beyond_reach(const SfGrid &g, const float4 p, float r2)
{
    const float c[3] = {p.x, p.y, p.z};
    float s = 0.0f;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float gc = (c[d] - g.org[d]) * g.inv_h;
        const float e = sf::safe_gap(fmaxf(fmaxf(-gc, gc - (float)g.dim[d]), 0.0f) * g.h, g.gap_eps);
        s += e * e;
    }
    return !(s * 0.998f < r2);
}

// Row t of a launch.  GRAPH: the point at sorted position t, its row the ORIGINAL id.  Otherwise query t, its row t.
// exists: t is a row at all; finite: it is searched; walk: ... and not beyond reach, so it is walked.
struct RadRow { float4 p; uint32_t row; bool exists, finite, walk; };
template <bool GRAPH>
__device__ __forceinline__ RadRow rad_row(const SfGrid &g, const float *__restrict__ q, int64_t n, int64_t t, float r2)
{
    RadRow r{make_float4(0.0f, 0.0f, 0.0f, 0.0f), 0u, false, false, false};
    if (GRAPH) {
        if (t >= g.n) return r;
        r.p = g.pts[t];
        r.row = __float_as_uint(r.p.w);
        r.exists = r.finite = r.walk = true;
        return r;
    }
    if (t >= n) return r;
    r.p = make_float4(q[3 * t], q[3 * t + 1], q[3 * t + 2], 0.0f);
    r.row = (uint32_t)t;
    r.exists = true;
    r.finite = isfinite(r.p.x) && isfinite(r.p.y) && isfinite(r.p.z);
    r.walk = r.finite && !beyond_reach(g, r.p, r2);
    return r;
}

// the window from LDS, as k_map_knn_t has it (as a kernel argument its 35 dwords stay in SGPRs across the whole walk)
#define SF_RAD_WINDOW_TO_LDS(sw, w)      \
    __shared__ SfWindow sw;              \
    if (WINDOW) {                        \
        if (threadIdx.x == 0) sw = w;    \
        __syncthreads();                 \
    }

template <bool GRAPH, bool WINDOW>
__global__ __launch_bounds__(256) void k_rad_count(SfGrid g, SfWindow w, const float *__restrict__ q, int64_t n, float r2, int R, uint32_t *__restrict__ count,
                                                    unsigned long long *__restrict__ red)
{
    SF_RAD_WINDOW_TO_LDS(sw, w)
    __shared__ unsigned long long part[4][RAD_WORDS];
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const RadRow r = rad_row<GRAPH>(g, q, n, t, r2);
    int cnt = 0;
    if (r.walk) {
        if (WINDOW)
            sf::radius_walk<false, false, true>(g, r.p, r2, R, 0u, nullptr,
                                                [&](uint32_t, int32_t, bool hit, float, const float4 c) { cnt += (hit && sf::window_accepts(sw, c.x, c.y, c.z)) ? 1 : 0; });
        else
            sf::radius_walk<false, false>(g, r.p, r2, R, 0u, nullptr, [&](uint32_t, int32_t, bool hit) { cnt += hit ? 1 : 0; });
    }
    if (r.exists) count[r.row] = (uint32_t)cnt;
    unsigned long long sum = (unsigned long long)cnt, mx = (unsigned long long)cnt, srch = r.finite ? 1ull : 0ull, emp = (r.exists && cnt == 0) ? 1ull : 0ull;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        sum += __shfl_xor(sum, o);
        const unsigned long long other = __shfl_xor(mx, o);
        mx = other > mx ? other : mx;
        srch += __shfl_xor(srch, o);
        emp += __shfl_xor(emp, o);
    }
    const int wv = (int)(threadIdx.x >> 6);
    if ((threadIdx.x & 63u) == 0) { part[wv][RAD_TOTAL] = sum; part[wv][RAD_MAX] = mx; part[wv][RAD_SEARCHED] = srch; part[wv][RAD_EMPTY] = emp; }
    __syncthreads();
    if (threadIdx.x < RAD_WORDS) {
        const int k = (int)threadIdx.x;
        const unsigned long long a = part[0][k], b = part[1][k], c = part[2][k], d = part[3][k];
        unsigned long long *slot = red + (size_t)(blockIdx.x & (RAD_SLOTS - 1)) * RAD_STRIDE + k;
        if (k == RAD_MAX) {
            const unsigned long long v = max(max(a, b), max(c, d));
            if (v) atomicMax(slot, v);
        } else {
            const unsigned long long v = a + b + c + d;
            if (v) atomicAdd(slot, v);
        }
    }
}

// the RAD_SLOTS groups of counters -> the four words behind them
__global__ __launch_bounds__(RAD_SLOTS) void k_rad_combine(unsigned long long *__restrict__ red)
{
    __shared__ unsigned long long part[RAD_SLOTS / 64][RAD_WORDS];
    unsigned long long v[RAD_WORDS];
#pragma unroll
    for (int k = 0; k < RAD_WORDS; ++k) v[k] = red[(size_t)threadIdx.x * RAD_STRIDE + k];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
#pragma unroll
        for (int k = 0; k < RAD_WORDS; ++k) {
            const unsigned long long other = __shfl_xor(v[k], o);
            v[k] = k == RAD_MAX ? (other > v[k] ? other : v[k]) : v[k] + other;
        }
    if ((threadIdx.x & 63u) == 0)
        for (int k = 0; k < RAD_WORDS; ++k) part[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x < RAD_WORDS) {
        const int k = (int)threadIdx.x;
        const unsigned long long a = part[0][k], b = part[1][k], c = part[2][k], d = part[3][k];
        red[(size_t)RAD_SLOTS * RAD_STRIDE + k] = k == RAD_MAX ? max(max(a, b), max(c, d)) : a + b + c + d;
    }
}

// one entry of a row: the id always, beside it the float32 d2 (index order) or the sort key (distance order)
template <bool KEYS>
__device__ __forceinline__ void rad_store(uint32_t slot, uint32_t row, uint32_t id, float d2, uint32_t *__restrict__ ids, float *__restrict__ d2_out,
                                          unsigned long long *__restrict__ keys)
{
    ids[slot] = id;
    if (KEYS) keys[slot] = ((unsigned long long)row << 32) | (unsigned long long)__float_as_uint(d2);
    else d2_out[slot] = d2;
}

template <bool GRAPH, bool WINDOW, bool KEYS>
__global__ __launch_bounds__(256) void k_rad_fill_lane(SfGrid g, SfWindow w, const float *__restrict__ q, int64_t n, float r2, int R, const uint32_t *__restrict__ offs,
                                                        uint32_t *__restrict__ ids, float *__restrict__ d2_out, unsigned long long *__restrict__ keys)
{
    SF_RAD_WINDOW_TO_LDS(sw, w)
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const RadRow r = rad_row<GRAPH>(g, q, n, t, r2);
    if (!r.walk) return;
    uint32_t o = offs[r.row];
    sf::radius_walk<false, false, true>(g, r.p, r2, R, 0u, nullptr, [&](uint32_t, int32_t, bool hit, float d, const float4 c) {
        if (hit && (!WINDOW || sf::window_accepts(sw, c.x, c.y, c.z))) rad_store<KEYS>(o++, r.row, __float_as_uint(c.w), d, ids, d2_out, keys);
    });
}

// a wave per row: every lane holds the same query and walks the same runs (radius_runs), lane l takes candidate a + 64 j + l
template <bool GRAPH, bool WINDOW, bool KEYS>
__global__ __launch_bounds__(256) void k_rad_fill_wave(SfGrid g, SfWindow w, const float *__restrict__ q, int64_t n, float r2, int R, const uint32_t *__restrict__ offs,
                                                        uint32_t *__restrict__ ids, float *__restrict__ d2_out, unsigned long long *__restrict__ keys)
{
    SF_RAD_WINDOW_TO_LDS(sw, w)
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t t = (int64_t)blockIdx.x * 4 + (int64_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const RadRow r = rad_row<GRAPH>(g, q, n, t, r2); // (the whole wave alike: no workgroup barrier below)
    if (!r.walk) return;
    uint32_t o = offs[r.row];
    const unsigned long long below = (1ull << lane) - 1ull;
    sf::radius_runs(g, r.p, r2, R, [&](uint32_t a, uint32_t b) {
        for (uint32_t k0 = a; k0 < b; k0 += 64u) {
            const uint32_t k = k0 + lane;
            const bool there = k < b;
            const float4 c = sf::load_point(g, k, there);
            const float d = sf::l2_simple(r.p.x, r.p.y, r.p.z, c.x, c.y, c.z);
            const bool hit = there && d < r2 && (!WINDOW || sf::window_accepts(sw, c.x, c.y, c.z));
            const unsigned long long hits = __ballot(hit);
            if (hit) rad_store<KEYS>(o + (uint32_t)__popcll(hits & below), r.row, __float_as_uint(c.w), d, ids, d2_out, keys);
            o += (uint32_t)__popcll(hits);
        }
    });
}

__global__ __launch_bounds__(256) void k_rad_unpack(const unsigned long long *__restrict__ keys, int64_t n, float *__restrict__ d2_out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d2_out[i] = __uint_as_float((uint32_t)keys[i]);
}

void rad_mark(sf_map *m, int k)
{
    if (!m->profile) return;
    if (!m->rad_ev[k] && hipEventCreate(&m->rad_ev[k]) != hipSuccess) { m->rad_ev[k] = nullptr; return; }
    hipError_t e = hipEventRecord(m->rad_ev[k], m->ctx->stream);
    (void)e;
}

template <bool GRAPH, bool WINDOW>
void rad_launch_fill(sf_map *m, bool wave, bool keys, const float *dq, int64_t rows, float r2, int R)
{
    const SfGrid &g = m->grid;
    const int64_t lanes = GRAPH ? g.n : rows; // a row per sorted position, or per query
    const dim3 grid(wave ? nblk(lanes, 4) : nblk(lanes)), block(256);
    hipStream_t s = m->ctx->stream;
    const uint32_t *offs = m->rad_off.as<uint32_t>();
    uint32_t *ids = m->rad_ids.as<uint32_t>();
    float *d2 = m->rad_d2.as<float>();
    unsigned long long *k = m->rad_keys.as<unsigned long long>();
    if (wave) {
        if (keys) hipLaunchKernelGGL((k_rad_fill_wave<GRAPH, WINDOW, true>), grid, block, 0, s, g, m->window, dq, rows, r2, R, offs, ids, d2, k);
        else hipLaunchKernelGGL((k_rad_fill_wave<GRAPH, WINDOW, false>), grid, block, 0, s, g, m->window, dq, rows, r2, R, offs, ids, d2, k);
    } else {
        if (keys) hipLaunchKernelGGL((k_rad_fill_lane<GRAPH, WINDOW, true>), grid, block, 0, s, g, m->window, dq, rows, r2, R, offs, ids, d2, k);
        else hipLaunchKernelGGL((k_rad_fill_lane<GRAPH, WINDOW, false>), grid, block, 0, s, g, m->window, dq, rows, r2, R, offs, ids, d2, k);
    }
}

// The four steps.  dq: the queries on the device (NULL: the graph form, rows = m->n).  Arguments are checked by the callers.
int radius_lists(sf_map *m, const float *dq, int64_t rows, float r2, int order, int64_t *offsets, sf_radius_stats *stats)
{
    sf_ctx *ctx = m->ctx;
    hipStream_t s = ctx->stream;
    const bool graph = dq == nullptr, windowed = !graph && m->window.kind != 0, keys = order == SF_RADIUS_ORDER_DISTANCE;
    const SfGrid &g = m->grid;
    m->rad_valid = false;
    m->rad_total = 0;
    m->rad_ms[0] = m->rad_ms[1] = m->rad_ms[2] = 0.0f;
    sf_radius_stats st{rows, 0, rows, 0, 0};
    std::vector<uint32_t> h_off;
    if (offsets) {
        try { h_off.resize((size_t)rows + 1); } catch (const std::bad_alloc &) { SF_CHECK(false, SF_ERR_NOMEM, "radius search: no host memory for %lld offsets", (long long)rows + 1); }
    }
    SF_TRY(m->rad_cnt.reserve(sizeof(uint32_t) * ((size_t)rows + 1)));
    SF_TRY(m->rad_off.reserve(sizeof(uint32_t) * ((size_t)rows + 1)));
    SF_TRY(m->rad_red.reserve(sizeof(unsigned long long) * RAD_RED_WORDS));
    uint32_t *cnt = m->rad_cnt.as<uint32_t>(), *off = m->rad_off.as<uint32_t>();
    unsigned long long *red = m->rad_red.as<unsigned long long>();
    SF_HIP(hipMemsetAsync(cnt, 0, sizeof(uint32_t) * ((size_t)rows + 1), s)); // rows no lane writes (points that are not indexed), and the entry behind the last
    SF_HIP(hipMemsetAsync(red, 0, sizeof(unsigned long long) * RAD_RED_WORDS, s));
    const int R = g.n > 0 ? radius_reach(g, r2) : 1;
    rad_mark(m, 0);
    if (g.n > 0) {
        if (graph) hipLaunchKernelGGL((k_rad_count<true, false>), dim3(nblk(g.n)), dim3(256), 0, s, g, m->window, dq, rows, r2, R, cnt, red);
        else if (windowed) hipLaunchKernelGGL((k_rad_count<false, true>), dim3(nblk(rows)), dim3(256), 0, s, g, m->window, dq, rows, r2, R, cnt, red);
        else hipLaunchKernelGGL((k_rad_count<false, false>), dim3(nblk(rows)), dim3(256), 0, s, g, m->window, dq, rows, r2, R, cnt, red);
    }
    hipLaunchKernelGGL(k_rad_combine, dim3(1), dim3(RAD_SLOTS), 0, s, red);
    SF_TRY(sf::scan_u32<0>(ctx, cnt, off, rows + 1));
    rad_mark(m, 1);
    SF_TRY(read_words(ctx, red + (size_t)RAD_SLOTS * RAD_STRIDE, RAD_WORDS));
    const unsigned long long *h = ctx->h_pinned->readback;
    const unsigned long long total = h[RAD_TOTAL];
    st.total = (int64_t)total;
    st.max_count = (int64_t)h[RAD_MAX];
    st.n_searched = (int64_t)h[RAD_SEARCHED];
    st.n_empty = g.n > 0 ? (int64_t)h[RAD_EMPTY] + (graph ? rows - g.n : 0) : rows;
    // the offsets are 32-bit and wrap; the radix sort takes fewer than 2^32 - 1 pairs
    SF_CHECK(total <= 0xfffffffeull, SF_ERR_OVERFLOW, "radius search: %llu neighbours in all, the lists hold 2^32 - 2 at most (a smaller radius, or fewer queries per call)", total);
    SF_TRY(m->rad_ids.reserve(sizeof(uint32_t) * (size_t)total));
    SF_TRY(m->rad_d2.reserve(sizeof(float) * (size_t)total));
    if (keys) {
        SF_TRY(m->rad_ids_alt.reserve(sizeof(uint32_t) * (size_t)total));
        SF_TRY(m->rad_keys.reserve(sizeof(unsigned long long) * (size_t)total));
        SF_TRY(m->rad_keys_alt.reserve(sizeof(unsigned long long) * (size_t)total));
    }
    const uint32_t *idx = m->rad_ids.as<uint32_t>();
    rad_mark(m, 2);
    if (total > 0) {
        // "automatic" is the lane fill: it was the faster one at every mean row length measured (2.8 - 21 entries, by 2.5 - 8.7 x:
        // profiles/radius_search_ab.txt), so the wave fill stays behind the setter alone
        const bool wave = m->rad_fill == 2;
        if (graph) rad_launch_fill<true, false>(m, wave, keys, dq, rows, r2, R);
        else if (windowed) rad_launch_fill<false, true>(m, wave, keys, dq, rows, r2, R);
        else rad_launch_fill<false, false>(m, wave, keys, dq, rows, r2, R);
        SF_HIP(hipGetLastError());
    }
    rad_mark(m, 3);
    if (keys && total > 0) {
        unsigned row_bits = 0;
        while (row_bits < 32 && ((uint64_t)(rows - 1) >> row_bits) != 0) ++row_bits;
        unsigned long long *ks = nullptr;
        uint32_t *vs = nullptr;
        SF_TRY(sf::radix_sort_pairs<unsigned long long>(ctx, m->rad_keys.as<unsigned long long>(), m->rad_keys_alt.as<unsigned long long>(), m->rad_ids.as<uint32_t>(),
                                                        m->rad_ids_alt.as<uint32_t>(), (int64_t)total, 32u + row_bits, &ks, &vs));
        hipLaunchKernelGGL(k_rad_unpack, dim3(nblk((int64_t)total)), dim3(256), 0, s, ks, (int64_t)total, m->rad_d2.as<float>());
        SF_HIP(hipGetLastError());
        idx = vs;
    }
    rad_mark(m, 4);
    if (offsets) SF_HIP(hipMemcpyAsync(h_off.data(), off, sizeof(uint32_t) * ((size_t)rows + 1), hipMemcpyDeviceToHost, s));
    SF_HIP(hipStreamSynchronize(s));
    if (m->profile) {
        float ms[3] = {0.0f, 0.0f, 0.0f};
        const bool have = m->rad_ev[0] && m->rad_ev[1] && m->rad_ev[2] && m->rad_ev[3] && m->rad_ev[4];
        if (have && hipEventElapsedTime(&ms[0], m->rad_ev[0], m->rad_ev[1]) == hipSuccess && hipEventElapsedTime(&ms[1], m->rad_ev[2], m->rad_ev[3]) == hipSuccess &&
            hipEventElapsedTime(&ms[2], m->rad_ev[3], m->rad_ev[4]) == hipSuccess) {
            for (int k = 0; k < 3; ++k) m->rad_ms[k] = ms[k];
            m->last_launch_ms = ms[0] + ms[1] + ms[2];
        }
    }
    if (offsets)
        for (int64_t i = 0; i <= rows; ++i) offsets[i] = (int64_t)h_off[(size_t)i];
    m->rad_idx = reinterpret_cast<const int32_t *>(idx);
    m->rad_total = (int64_t)total;
    m->rad_valid = true;
    if (stats) *stats = st;
    return SF_OK;
}

// what both calls refuse; an empty set of rows is answered here (*done)
int radius_arguments(sf_map *m, int64_t rows, double radius, int order, int64_t *offsets, sf_radius_stats *stats, float *r2, bool *done)
{
    SF_CHECK(m && m->built, SF_ERR_STATE, "map not built");
    *r2 = (float)(radius * radius);
    SF_CHECK(radius > 0 && std::isfinite(radius) && std::isfinite(*r2) && *r2 > 0.0f, SF_ERR_INVALID, "radius search: radius must be positive and finite, and so must its float32 square (got %g)", radius);
    SF_CHECK(order == SF_RADIUS_ORDER_INDEX || order == SF_RADIUS_ORDER_DISTANCE, SF_ERR_INVALID, "radius search: order must be SF_RADIUS_ORDER_INDEX or SF_RADIUS_ORDER_DISTANCE (got %d)", order);
    SF_CHECK(rows >= 0 && rows < ((int64_t)1 << 31), SF_ERR_INVALID, "radius search: 0 .. 2^31 - 1 rows (got %lld)", (long long)rows);
    *done = rows == 0;
    if (*done) {
        if (offsets) offsets[0] = 0;
        if (stats) *stats = sf_radius_stats{0, 0, 0, 0, 0};
        m->rad_total = 0;
        m->rad_valid = true; // lists of no rows
        m->rad_ms[0] = m->rad_ms[1] = m->rad_ms[2] = 0.0f;
    }
    return SF_OK;
}

} // namespace

extern "C" int sf_map_radius_search(sf_map *m, const float *queries, int64_t n, double radius, int order, int64_t *offsets, sf_radius_stats *stats)
{
    float r2 = 0.0f;
    bool done = false;
    SF_CHECK(n <= 0 || queries, SF_ERR_INVALID, "bad arguments");
    SF_TRY(radius_arguments(m, n, radius, order, offsets, stats, &r2, &done));
    if (done) return SF_OK;
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    m->rad_valid = false;
    SF_TRY(m->rad_q.reserve(sizeof(float) * 3 * (size_t)n)); // the map's own staging: no allocation per call once it has grown
    SF_HIP(hipMemcpyAsync(m->rad_q.p, queries, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    return radius_lists(m, m->rad_q.as<float>(), n, r2, order, offsets, stats);
}

extern "C" int sf_map_radius_graph(sf_map *m, double radius, int order, int64_t *offsets, sf_radius_stats *stats)
{
    float r2 = 0.0f;
    bool done = false;
    SF_TRY(radius_arguments(m, m ? m->n : 0, radius, order, offsets, stats, &r2, &done));
    if (done) return SF_OK;
    SF_HIP(hipSetDevice(m->ctx->device));
    return radius_lists(m, nullptr, m->n, r2, order, offsets, stats);
}

extern "C" int sf_map_radius_results(sf_map *m, int32_t *idx, float *d2, int64_t cap, int64_t *total)
{
    SF_CHECK(m && total, SF_ERR_INVALID, "bad arguments");
    *total = 0;
    SF_CHECK(m->built && m->rad_valid, SF_ERR_STATE, "no radius lists (sf_map_radius_search / sf_map_radius_graph first; sf_map_build and sf_map_patch drop them)");
    *total = m->rad_total;
    SF_CHECK((!idx && !d2) || cap >= m->rad_total, SF_ERR_INVALID, "radius results: room for %lld entries, the lists hold %lld", (long long)cap, (long long)m->rad_total);
    if (m->rad_total == 0 || (!idx && !d2)) return SF_OK;
    sf_ctx *ctx = m->ctx;
    SF_HIP(hipSetDevice(ctx->device));
    if (idx) SF_HIP(hipMemcpyAsync(idx, m->rad_idx, sizeof(int32_t) * (size_t)m->rad_total, hipMemcpyDeviceToHost, ctx->stream));
    if (d2) SF_HIP(hipMemcpyAsync(d2, m->rad_d2.p, sizeof(float) * (size_t)m->rad_total, hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    return SF_OK;
}

extern "C" int sf_map_set_radius_fill(sf_map *m, int mode)
{
    SF_CHECK(m && mode >= 0 && mode <= 2, SF_ERR_INVALID, "radius fill: 0 automatic, 1 one lane per row, 2 one wave per row (got %d)", mode);
    m->rad_fill = mode;
    return SF_OK;
}

extern "C" int sf_map_radius_launch_ms(sf_map *m, float ms[3])
{
    SF_CHECK(m && ms, SF_ERR_INVALID, "bad arguments");
    for (int k = 0; k < 3; ++k) ms[k] = m->profile ? m->rad_ms[k] : 0.0f;
    return SF_OK;
}
