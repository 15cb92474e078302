// sf_knn.hpp — exact k nearest neighbours over the uniform-grid map index (device side, gfx950).
//
// One WAVE per query (a lane-per-query top-k would need a dynamically indexed k-entry array per lane: scratch).  The result
// is the first k entries of the candidates (d2 < threshold, window accepted) in ascending hit_key(d2, j) order, j = position
// in the sorted index -- the rule of sf_nn.hpp, so k = 1 is sf_map_nn bit for bit.
//
// Walk: the block of radius R around the query's cell grows ring by ring, R = 0 (the own cell), 1, 2, ...  A candidate enters the selection
// once: at ring R the rows outside the previous block are taken whole (their x-run trimmed from both ends while the end
// cell's gap prunes it), the rows inside it only in their two new end cells.  The 2 (2R+1)^2 (row, side) entries of a ring are
// looked up by the lanes in parallel, 64 at a time, pruned (gap^2 * 0.998 >= tau skips), laid end to end by a prefix sum and
// dealt out over the wave like the flat rounds of nn_search_wave, two candidates per lane per trip, loaded through
// load_point.  tau is search_start(threshold) until k candidates are held, then the k-th smallest d2 held; it only ever
// falls, so what a ring pruned stays pruned.
// Exactness: the certificate of nn_rings with tau in place of hit.d2 -- after ring R stop iff tau <= (safe_gap(m) * 0.999)^2
// or no grid cell lies outside the block.
//
// Selection: keys below the tau-key are appended to a per-wave LDS buffer of 128 keys by ballot compaction.  When the next
// append could overflow it (and at the end of every ring, for a tight tau) a bitonic sort of the 128 slots -- two keys per
// lane in registers, partners by ds_bpermute, 27 exchange steps -- keeps the k smallest and lowers tau.  The last sort
// leaves the result in lanes 0 .. cnt-1.  Keys are distinct (j is), so the outcome does not depend on the order candidates
// arrive in.
#pragma once
#include "sf_nn.hpp"

namespace sf {

constexpr int KNN_BUF = 128;
// the first block examined: the query's own cell alone, so that tau can fall before the 26 cells around it are looked at
// (starting from the 27 cells at once, one step less where the own cell cannot hold k points anyway, has not been timed against it)
constexpr int KNN_FIRST_RING = 0;

struct WaveKNN {
    unsigned long long buf[KNN_BUF]; // accepted keys, unsorted beyond what the last sort left
    alignas(4) uint8_t mark[128];    // dealing: lane + 1 of the entry whose range starts at this slot of the trip
};

// ascending bitonic sort of 128 keys: element i in `a` of lane i, element 64 + i in `b` of lane i
__device__ __forceinline__ void knn_sort128(unsigned long long &a, unsigned long long &b, int lane)
{
    // (rolled on purpose: unrolled, the 54 lane masks of the steps are hoisted out of the query loop and spill the SGPR file)
#pragma unroll 1
    for (int size = 2; size <= 128; size <<= 1) {
        if (size == 128) { // stride 64: the lane's own two keys
            const unsigned long long lo = a < b ? a : b, hi = a < b ? b : a;
            a = lo; b = hi;
        }
#pragma unroll 1
        for (int stride = size == 128 ? 32 : size >> 1; stride >= 1; stride >>= 1) {
            const bool lower = (lane & stride) == 0;
            const bool asc_a = (lane & size) == 0, asc_b = ((lane + 64) & size) == 0;
            const unsigned long long pa = __shfl_xor(a, stride), pb = __shfl_xor(b, stride);
            a = ((lower == asc_a) == (pa < a)) ? pa : a;
            b = ((lower == asc_b) == (pb < b)) ? pb : b;
        }
    }
}

// the running selection of one query (every member is wave-uniform)
struct KnnSel {
    unsigned long long tkey; // candidates are taken iff their key is below this
    int cnt;                 // keys held in the buffer
    bool dirty;              // appended to since the last sort
};

// keep the k smallest keys held; -> lane i's key of the sorted buffer (~0 beyond cnt)
__device__ __forceinline__ unsigned long long knn_compact(WaveKNN *ws, KnnSel &s, int k, int lane)
{
    wave_sync();
    unsigned long long a = lane < s.cnt ? ws->buf[lane] : ~0ull, b = lane + 64 < s.cnt ? ws->buf[lane + 64] : ~0ull;
    knn_sort128(a, b, lane);
    s.cnt = min(s.cnt, k);
    if (lane < s.cnt) ws->buf[lane] = a;
    if (s.cnt == k) s.tkey = __shfl(a, k - 1);
    s.dirty = false;
    wave_sync();
    return a;
}

// Every lane of the wave calls this with the SAME query.  -> cnt = min(k, candidates); lane i < cnt holds the i-th key in
// `out` (d2 bits << 32 | sorted position), the other lanes ~0.
template <bool WINDOW>
__device__ __forceinline__ int knn_search(const SfGrid &g, const SfWindow &w, float qx, float qy, float qz, int k, float thr, WaveKNN *ws, unsigned long long &out)
{
    const int lane = (int)__lane_id();
    const int nx = g.dim[0], ny = g.dim[1], nz = g.dim[2];
    out = ~0ull;
    if (!(isfinite(qx) && isfinite(qy) && isfinite(qz)) || g.n == 0 || !(thr > 0.0f)) return 0;
    if (WINDOW) {
        const float gap = window_gap(w, qx, qy, qz);
        if (gap * gap > thr) return 0; // nothing the window accepts is within the acceptance radius
    }
    {
        // farther from the grid's box (every point is inside it) than the acceptance radius: nothing, without a walk (nn_search_wave)
        const float ox = fmaxf(fmaxf(g.org[0] - qx, qx - (g.org[0] + (float)nx * g.h)), 0.0f);
        const float oy = fmaxf(fmaxf(g.org[1] - qy, qy - (g.org[1] + (float)ny * g.h)), 0.0f);
        const float oz = fmaxf(fmaxf(g.org[2] - qz, qz - (g.org[2] + (float)nz * g.h)), 0.0f);
        const float gap = fmaxf(sqrtf(ox * ox + oy * oy + oz * oz) * 0.9995f - 1.0e-3f, 0.0f);
        if (gap * gap > thr) return 0;
    }
    const float gx = (qx - g.org[0]) * g.inv_h, gy = (qy - g.org[1]) * g.inv_h, gz = (qz - g.org[2]) * g.inv_h;
    const int cx = grid_cell(gx, nx), cy = grid_cell(gy, ny), cz = grid_cell(gz, nz);
    const float h = g.h, ge = g.gap_eps;
    const int rcap = max(nx, max(ny, nz));
    KnnSel sel;
    sel.tkey = hit_key(search_start(thr), -1);
    sel.cnt = 0;
    sel.dirty = false;

    for (int R = KNN_FIRST_RING; R <= rcap; ++R) {
        const int y0 = max(cy - R, 0), y1 = min(cy + R, ny - 1);
        const int z0 = max(cz - R, 0), z1 = min(cz + R, nz - 1);
        const int x0 = max(cx - R, 0), x1 = min(cx + R, nx - 1);
        const int nyr = y1 - y0 + 1, entries = 2 * nyr * (z1 - z0 + 1);
        for (int e0 = 0; e0 < entries; e0 += 64) {
            // ---- one (row, side) entry per lane: its candidate range after pruning
            const float tau = __uint_as_float((uint32_t)(sel.tkey >> 32));
            const int e = e0 + lane;
            uint32_t a = 0, len = 0;
            if (e < entries) {
                const int row = e >> 1, side = e & 1;
                const int zi = row / nyr, y = y0 + (row - zi * nyr), z = z0 + zi;
                const float ry = safe_gap(cell_gap(gy, y, cy) * h, ge), rz = safe_gap(cell_gap(gz, z, cz) * h, ge);
                const float g2 = ry * ry + rz * rz;
                if (g2 * 0.998f < tau) {
                    const size_t rowbase = ((size_t)z * ny + y) * nx;
                    const bool inner = R > KNN_FIRST_RING && abs(y - cy) < R && abs(z - cz) < R; // examined up to x +- (R - 1) by the rings before
                    if (!inner) {
                        if (side == 0) { // the whole x-run, less the end cells whose gap prunes them (the query's own column never is)
                            // (trim_left / trim_right of sf_nn.hpp, written out: see there)
                            int xa = x0, xb = x1;
                            while (xa < cx) {
                                const float gl = safe_gap(cell_gap(gx, xa, cx) * h, ge);
                                if ((g2 + gl * gl) * 0.998f < tau) break;
                                ++xa;
                            }
                            while (xb > cx) {
                                const float gr = safe_gap(cell_gap(gx, xb, cx) * h, ge);
                                if ((g2 + gr * gr) * 0.998f < tau) break;
                                --xb;
                            }
                            a = g.cell_start[rowbase + xa];
                            len = g.cell_start[rowbase + xb + 1] - a;
                        }
                    } else {
                        const int x = side == 0 ? cx - R : cx + R;
                        if (x >= 0 && x <= nx - 1) {
                            const float gxx = safe_gap(cell_gap(gx, x, cx) * h, ge);
                            if ((g2 + gxx * gxx) * 0.998f < tau) {
                                a = g.cell_start[rowbase + x];
                                len = g.cell_start[rowbase + x + 1] - a;
                            }
                        }
                    }
                }
            }
            // ---- the ranges laid end to end, two candidates per lane per trip
            const uint32_t incl = wave_incl_scan<false>(len);
            const uint32_t off = incl - len;
            const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            const uint32_t base = a - off; // the candidate of slot s of this lane's entry is base + s (mod 2^32)
            uint32_t carry = 0;            // lane + 1 of the entry that holds the last slot of the previous trip
            for (uint32_t c0 = 0; c0 < tot; c0 += 128u) {
                for (int i = lane; i < 32; i += 64) reinterpret_cast<uint32_t *>(ws->mark)[i] = 0u;
                __builtin_amdgcn_wave_barrier();
                if (len != 0u && off >= c0 && off - c0 < 128u) ws->mark[off - c0] = (uint8_t)(lane + 1);
                wave_sync();
                uint32_t src[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) src[t] = wave_incl_scan<true>((uint32_t)ws->mark[64 * t + lane]);
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    src[t] = max(src[t], carry);
                    carry = (uint32_t)__builtin_amdgcn_readlane((int)src[t], 63);
                }
                wave_sync(); // the marks are read before the next trip clears them
                uint32_t j[2];
                float4 p[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const uint32_t s = c0 + 64u * (uint32_t)t + (uint32_t)lane;
                    const int from = (int)((src[t] - 1u) & 63u) << 2; // slots past the end read some entry: nothing is done with it
                    j[t] = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)base) + s;
                    p[t] = load_point(g, j[t], s < tot);
                }
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const bool live = c0 + 64u * (uint32_t)t + (uint32_t)lane < tot;
                    if (__ballot(live) == 0ull) continue;
                    if (sel.cnt + 64 > KNN_BUF) knn_compact(ws, sel, k, lane);
                    const float d2 = l2_simple(qx, qy, qz, p[t].x, p[t].y, p[t].z);
                    const unsigned long long key = hit_key(d2, (int)j[t]);
                    const bool take = live && key < sel.tkey && (!WINDOW || window_accepts(w, p[t].x, p[t].y, p[t].z));
                    const unsigned long long bal = __ballot(take);
                    if (bal != 0ull) {
                        const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                        if (take) ws->buf[sel.cnt + rank] = key;
                        sel.cnt += __popcll(bal);
                        sel.dirty = true;
                    }
                }
            }
        }
        if (sel.dirty && sel.cnt >= k) knn_compact(ws, sel, k, lane); // tau as tight as what has been seen allows
        const float m = block_face_gap(g, gx, gy, gz, cx, cy, cz, R);
        if (m >= 3.0e38f) break; // whole grid examined
        const float mm = safe_gap(m, ge) * 0.999f;
        if (__uint_as_float((uint32_t)(sel.tkey >> 32)) <= mm * mm) break;
    }
    if (sel.cnt == 0) return 0;
    out = knn_compact(ws, sel, k, lane);
    if (lane >= sel.cnt) out = ~0ull;
    return sel.cnt;
}

// sum of one double per lane in a fixed order: the pairwise tree over lanes 0..63 ((0+1)+(2+3))+..., the same bits in every lane
__device__ __forceinline__ double wave_tree_sum(double v)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = __dadd_rn(v, __shfl_xor(v, o));
    return v;
}

} // namespace sf
