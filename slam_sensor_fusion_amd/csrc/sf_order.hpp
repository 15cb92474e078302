// sf_order.hpp — query ordering: each scan's points bucketed by the map cell they fall in under the initial pose
// (gfx950, hand-written; replaces the rocPRIM radix_sort_pairs + key kernels of round 1 in the timed path).
//
// What is ordered: per scan (segment) a 10-bit key = position of the query's cell in the walk order of
// order_cell() shifted down to 10 bits, i.e. 1024 buckets per scan; inside a bucket the queries keep their
// original order (stable).  Measured on MI355X (200 k-point scans vs the 10 M-point map, 32 in flight, k_nn_red per
// launch): no order 194 us, 4 key bits 180, 6 bits 159, 8 bits 156, 10 bits 146, 12 bits 148, 16 bits 143, 20 bits
// 143 -- what the search needs is that chunk c of every scan in flight covers the same stretch of the map, not a
// total order, so ONE stable counting pass on 10 bits replaces round 1's four rocPRIM radix passes over a 24-bit
// key (and a two-pass 20-bit version of this file, which cost 133 us more per step than the 2 % it bought).
// Scans are independent segments: the order of a scan does not depend on what else is in the batch.
//
//   k_order_hist     per-tile bucket counts (LDS histogram, keys computed from the coordinates, the key of every
//                    query kept as a u16 so the scatter does not recompute it).  Stage by stage over a lane's 16 queries,
//                    every load of a stage in flight before the first is waited for: ids, 48 coordinate loads, positions
//                    (KEYFN::position, arithmetic), the 16 gathers from the density table (KEYFN::table), key stores, LDS
//                    adds.  93 -> 65 us per 64 x 200 k-point step, every key bit for bit the same
//                    (tests/test_gpu_order_keys.py).  What was tried beside it, and why the table is still gathered from
//                    L2: profiles/LADDER.md, round 11
//   k_order_scan     per segment: exclusive prefix over tiles and over buckets, in place
//   k_order_move     the plain path (uniform segments in element order, one digit): rank inside the tile + prefix, the tile
//                    put into bucket order in LDS and the three coordinate planes written to their ordered positions, slot
//                    i by thread i % 256 -- a bucket's queries of one tile are consecutive in the segment, so consecutive
//                    lanes store consecutive addresses while the bucket lasts (about 15 lines per wave and plane on
//                    randomly drawn scans, fewer on a sensor's sweep order).  No ids and no float4 records: 103 us per
//                    64 x 200 k-point step against 82 + 121 for the two kernels below, the same Xq bit for bit.  (Round 3's
//                    attempt stored x, y, z straight from the scatter in ELEMENT order: three scattered 4-byte streams,
//                    420 us.  The store pattern was the failure, not the fusion.)
//   k_order_scatter  rank inside the tile + prefix -> the query's id at its ordered position: the forms that need ids
//                    between their passes (segment offsets / src_idx of the sharded start, the two-digit tile sort)
//   k_order_gather   (sf_icp.hip) ids read coalesced, float4 records gathered, cell-ordered SoA written coalesced
// sf_test_query_order (include/slamfusion.h; tests/test_gpu_query_order.py) runs hist -> scan -> either form on host points.
//
// Stability inside a tile without a per-element sequential loop: a tile is split into contiguous quarters, one per
// wave; each wave keeps its own running counter per bucket in LDS (started at the tile's start for that bucket +
// what the waves before it hold) and walks its quarter 64 elements at a time: the lanes whose bucket equals mine are
// found with one ballot per key bit (10 ballots), my rank among them is the popcount below my lane, and the last of
// them advances the counter.  All counts are integers: the result is the unique stable order, bitwise reproducible.
#pragma once
#include "sf_common.hpp"

namespace sf {

constexpr int ORD_KEY_BITS = 10;
constexpr int ORD_BINS = 1 << ORD_KEY_BITS;
constexpr uint32_t ORD_KEY_NONE = ORD_BINS - 1u;  // non-finite queries: last bucket of their scan
constexpr int ORD_BLK = 256;
constexpr int ORD_WAVES = ORD_BLK / 64;
constexpr int ORD_PER_LANE = 16;                  // elements per lane
constexpr int ORD_TILE = ORD_BLK * ORD_PER_LANE;  // 4096 elements per workgroup
constexpr int ORD_WAVE_SPAN = 64 * ORD_PER_LANE;  // contiguous elements per wave

struct OrderSrc {
    const uint32_t *src_idx;     // element e of the segment space -> global query id, or nullptr (identity)
    const uint32_t *seg_off;     // segment offsets [nseg + 1], or nullptr (uniform: segment b = [b * n, (b + 1) * n))
    int n;                       // uniform segment length
    int tiles;                   // tiles per segment
    int nseg;                    // segments (grid: order_grid(tiles, nseg), see order_block)
};

// XCD-aware placement: workgroups are dealt round-robin to the 8 XCDs in launch order (linear id L runs on XCD L % 8).
// A one-dimensional grid of tiles x (segments rounded up to 8): all tiles of segment b run on XCD b % 8, eight segments
// at a time, so what a segment's workgroups write at random inside the segment (the ordered ids: 4-byte stores into
// 0.8 MB per 200 k-point scan) is merged into whole lines in ONE L2 and what they read at random (k_order_gather: 16-byte
// records, 3.2 MB per scan) is fetched into one L2 once -- a (tiles, segments) grid spreads every segment over the
// eight L2s, which do not share lines.  -> false: no such segment (padding)
__device__ __forceinline__ bool order_block(int tiles, int nseg, int *b, int *tile)
{
    const int lin = blockIdx.x, xcd = lin & 7, k = lin >> 3;
    *tile = k % tiles;
    *b = (k / tiles) * 8 + xcd;
    return *b < nseg;
}
inline unsigned order_grid(int tiles, int nseg) { return (unsigned)tiles * (unsigned)((nseg + 7) & ~7); }

__device__ __forceinline__ void order_segment(const OrderSrc &s, int b, uint32_t *start, uint32_t *len)
{
    if (s.seg_off) { *start = s.seg_off[b]; *len = s.seg_off[b + 1] - s.seg_off[b]; }
    else { *start = (uint32_t)b * (uint32_t)s.n; *len = (uint32_t)s.n; }
}

// the lanes of the wave whose key equals mine (only lanes with valid = true take part)
__device__ __forceinline__ unsigned long long order_peers(uint32_t key, bool valid)
{
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int k = 0; k < ORD_KEY_BITS; ++k) {
        const unsigned long long bk = __ballot((key >> k) & 1u);
        m &= ((key >> k) & 1u) ? bk : ~bk;
    }
    return m;
}

// element index (inside the segment) of chunk c of this lane: a wave owns ORD_WAVE_SPAN consecutive elements and
// walks them 64 at a time
__device__ __forceinline__ uint32_t order_element(int tile, int c)
{
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    return (uint32_t)tile * ORD_TILE + (uint32_t)wv * ORD_WAVE_SPAN + 64u * (uint32_t)c + (uint32_t)lane;
}

// counts[(seg * (tiles + 1) + tile) * ORD_BINS + key]; keys[segment space] <- KEYFN(global query id)
// Stage by stage over the lane's ORD_PER_LANE elements, nothing conditional between the loads of a stage: the ids (the test for
// src_idx around the whole loop -- a per-element "id or load" select makes the compiler branch around every id load and wait for
// everything in flight in front of the next element's coordinates), the 3 coordinate loads of every element behind one counted
// wait, KEYFN::position (arithmetic only), KEYFN::table (the table gathers of all elements in flight together), then the key stores
// and the LDS adds with no wait between them.  Elements past the segment's end read its last element and store nothing.
template <class KEYFN>
__device__ __forceinline__ void order_hist_body(const OrderSrc &s, KEYFN keyfn, uint16_t *__restrict__ keys, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t h[ORD_BINS];
    int b, tile;
    if (!order_block(s.tiles, s.nseg, &b, &tile)) return;
    uint32_t seg_start, seg_len;
    order_segment(s, b, &seg_start, &seg_len);
    uint32_t *dst = counts + ((size_t)b * (s.tiles + 1) + tile) * ORD_BINS; // row `tiles` of a segment's table: the bucket starts (k_order_scan)
    if ((uint32_t)tile * ORD_TILE >= seg_len) { // nothing of this segment here (shorter segments of a ragged batch)
        for (int d = threadIdx.x; d < ORD_BINS; d += ORD_BLK) dst[d] = 0;
        return;
    }
    for (int d = threadIdx.x; d < ORD_BINS; d += ORD_BLK) h[d] = 0;
    __syncthreads();
    const typename KEYFN::Pose pose = keyfn.prepare(b); // segment b is scan b
    const uint32_t last = seg_len - 1u;                 // (seg_len > 0: the tile holds an element)
    uint32_t o[ORD_PER_LANE];
    if (s.src_idx) {
#pragma unroll
        for (int c = 0; c < ORD_PER_LANE; ++c) o[c] = s.src_idx[seg_start + min(order_element(tile, c), last)];
    } else {
#pragma unroll
        for (int c = 0; c < ORD_PER_LANE; ++c) o[c] = seg_start + min(order_element(tile, c), last);
    }
    typename KEYFN::Point pt[ORD_PER_LANE];
#pragma unroll
    for (int c = 0; c < ORD_PER_LANE; ++c) pt[c] = keyfn.load(o[c]);
    uint32_t w[ORD_PER_LANE], key[ORD_PER_LANE];
#pragma unroll
    for (int c = 0; c < ORD_PER_LANE; ++c) w[c] = keyfn.position(pose, pt[c]);
    keyfn.table(w, key);
#pragma unroll
    for (int c = 0; c < ORD_PER_LANE; ++c) {
        const uint32_t e = order_element(tile, c);
        if (e < seg_len) keys[seg_start + e] = (uint16_t)key[c];
    }
#pragma unroll
    for (int c = 0; c < ORD_PER_LANE; ++c)
        if (order_element(tile, c) < seg_len) atomicAdd(&h[key[c]], 1u); // integer: order independent
    __syncthreads();
    for (int d = threadIdx.x; d < ORD_BINS; d += ORD_BLK) dst[d] = h[d];
}

// one workgroup of ORD_BINS threads per segment: counts -> exclusive start of (bucket, tile) within the segment
__global__ __launch_bounds__(ORD_BINS) void k_order_scan(uint32_t *__restrict__ counts, int tiles)
{
    __shared__ uint32_t sc[ORD_BINS];
    const int d = threadIdx.x;
    uint32_t *c = counts + (size_t)blockIdx.x * (tiles + 1) * ORD_BINS;
    uint32_t run = 0;
    for (int t0 = 0; t0 < tiles; t0 += 8) { // exclusive prefix over the tiles for this bucket (coalesced across buckets), 8 loads in flight
        uint32_t v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = t0 + k < tiles ? c[(size_t)(t0 + k) * ORD_BINS + d] : 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (t0 + k < tiles) c[(size_t)(t0 + k) * ORD_BINS + d] = run;
            run += v[k];
        }
    }
    sc[d] = run; // total of bucket d
    __syncthreads();
    for (int off = 1; off < ORD_BINS; off <<= 1) { // inclusive scan over the buckets
        const uint32_t t = d >= off ? sc[d - off] : 0u;
        __syncthreads();
        sc[d] += t;
        __syncthreads();
    }
    sc[d] -= run; // exclusive: where bucket d starts in the segment
    __syncthreads();
    // kept apart from the per-tile prefixes (the scatter adds the two): row `tiles` of the table
    c[(size_t)tiles * ORD_BINS + d] = sc[d];
}

// out[seg_start + rank] <- global query id
__device__ __forceinline__ void order_scatter_body(const OrderSrc &s, const uint16_t *__restrict__ keys, const uint32_t *__restrict__ starts, uint32_t *__restrict__ out)
{
    __shared__ uint32_t ctr[ORD_WAVES][ORD_BINS];
    int b, tile;
    if (!order_block(s.tiles, s.nseg, &b, &tile)) return;
    uint32_t seg_start, seg_len;
    order_segment(s, b, &seg_start, &seg_len);
    if ((uint32_t)tile * ORD_TILE >= seg_len) return;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int d = threadIdx.x; d < ORD_BINS * ORD_WAVES; d += ORD_BLK) (&ctr[0][0])[d] = 0;
    __syncthreads();
    uint32_t key[ORD_PER_LANE];
    bool valid[ORD_PER_LANE];
#pragma unroll
    for (int c = 0; c < ORD_PER_LANE; ++c) {
        const uint32_t e = order_element(tile, c);
        valid[c] = e < seg_len;
        key[c] = valid[c] ? (uint32_t)keys[seg_start + e] : 0u;
    }
#pragma unroll
    for (int c = 0; c < ORD_PER_LANE; ++c)
        if (valid[c]) atomicAdd(&ctr[wv][key[c]], 1u);
    __syncthreads();
    // per-wave counts -> per-wave running start: bucket start + tile prefix + what the waves before hold
    const uint32_t *seg_tab = starts + (size_t)b * (s.tiles + 1) * ORD_BINS;
    for (int d = threadIdx.x; d < ORD_BINS; d += ORD_BLK) {
        uint32_t run = seg_tab[(size_t)tile * ORD_BINS + d] + seg_tab[(size_t)s.tiles * ORD_BINS + d];
#pragma unroll
        for (int w = 0; w < ORD_WAVES; ++w) {
            const uint32_t v = ctr[w][d];
            ctr[w][d] = run;
            run += v;
        }
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t rank[ORD_PER_LANE];
#pragma unroll
    for (int c = 0; c < ORD_PER_LANE; ++c) { // the wave's chunks in order: stability.  LDS only in this loop: the global stores follow
        const unsigned long long peers = order_peers(key[c], valid[c]);
        rank[c] = valid[c] ? ctr[wv][key[c]] + (uint32_t)__popcll(peers & below) : 0u;
        __builtin_amdgcn_wave_barrier(); // every lane has read the counter before the group's last lane advances it
        if (valid[c] && (peers >> lane) <= 1ull) ctr[wv][key[c]] += (uint32_t)__popcll(peers);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    uint32_t id[ORD_PER_LANE]; // (the test for src_idx around the whole loop, as in order_hist_body; elements past the end read the last id and store nothing)
    if (s.src_idx) {
#pragma unroll
        for (int c = 0; c < ORD_PER_LANE; ++c) id[c] = s.src_idx[seg_start + min(order_element(tile, c), seg_len - 1u)];
    } else {
#pragma unroll
        for (int c = 0; c < ORD_PER_LANE; ++c) id[c] = seg_start + order_element(tile, c);
    }
#pragma unroll
    for (int c = 0; c < ORD_PER_LANE; ++c)
        if (valid[c]) out[seg_start + rank[c]] = id[c];
}

// ---- k_order_move: rank and move in one pass (uniform segments, identity ids)
// LDS of a workgroup: 16 KB that hold the per-wave counters while the tile is ranked and one coordinate plane of the tile
// afterwards, the key of every slot (8 KB) and per bucket what turns a slot into a position of the segment (4 KB): 28 KB.
struct OrderMoveLds {
    union {
        uint32_t ctr[ORD_WAVES][ORD_BINS]; // ranking: where the wave's next query of a bucket goes INSIDE the tile
        float plane[ORD_TILE];             // write-out: one coordinate of the tile in bucket order
    };
    uint32_t delta[ORD_BINS];              // (bucket start + tile prefix) - the bucket's offset inside the tile
    uint16_t skey[ORD_TILE];               // key of the query in slot i
    uint32_t wsum[ORD_WAVES];
};
static_assert(sizeof(uint32_t) * ORD_WAVES * ORD_BINS == sizeof(float) * ORD_TILE, "the plane takes the counters' place");

// one coordinate plane of the tile: v[c] (element order, in registers) -> LDS in bucket order -> dst, slot i by thread i % ORD_BLK
__device__ __forceinline__ void order_move_plane(OrderMoveLds &L, const float (&v)[ORD_PER_LANE], const bool (&valid)[ORD_PER_LANE], const uint32_t (&slot)[ORD_PER_LANE],
                                                 const uint32_t (&pos)[ORD_PER_LANE], uint32_t tile_cnt, float *__restrict__ dst)
{
#pragma unroll
    for (int c = 0; c < ORD_PER_LANE; ++c)
        if (valid[c]) L.plane[slot[c]] = v[c];
    __syncthreads();
    float o[ORD_PER_LANE];
#pragma unroll
    for (int j = 0; j < ORD_PER_LANE; ++j) {
        const uint32_t i = threadIdx.x + (uint32_t)ORD_BLK * j;
        o[j] = i < tile_cnt ? L.plane[i] : 0.0f;
    }
    __syncthreads(); // the plane is in registers: the next one may be written while the stores below drain
#pragma unroll
    for (int j = 0; j < ORD_PER_LANE; ++j)
        if (threadIdx.x + (uint32_t)ORD_BLK * j < tile_cnt) dst[pos[j]] = o[j];
}

// dx / dy / dz[seg_start + rank] <- sx / sy / sz[seg_start + e]: the ranks of order_scatter_body (bucket start + tile prefix + the
// waves before + the ballot rank, chunks of a wave in order), so every query lands where k_order_scatter + k_order_gather put it.
// A rank is formed as (slot inside the tile) + delta[key]: the tile's queries go to their slots in LDS first -- bucket order --
// and slot i is written out by thread i % ORD_BLK, so that consecutive lanes store consecutive addresses as long as the bucket
// lasts (a bucket's queries of one tile are consecutive in the segment) instead of one line per lane.  The three planes go
// through the same 16 KB one after the other with the positions computed once.  No atomic returns a value and every LDS word
// written between two barriers has exactly one writer: the result does not depend on the order lanes are served in.
__device__ __forceinline__ void order_move_body(const OrderSrc &s, const uint16_t *__restrict__ keys, const uint32_t *__restrict__ starts, const float *__restrict__ sx,
                                                const float *__restrict__ sy, const float *__restrict__ sz, float *__restrict__ dx, float *__restrict__ dy, float *__restrict__ dz)
{
    __shared__ OrderMoveLds L;
    int b, tile;
    if (!order_block(s.tiles, s.nseg, &b, &tile)) return;
    const uint32_t seg_len = (uint32_t)s.n, tile_first = (uint32_t)tile * ORD_TILE;
    if (tile_first >= seg_len) return;
    const size_t seg_start = (size_t)b * (size_t)s.n;
    const uint32_t tile_cnt = seg_len - tile_first < (uint32_t)ORD_TILE ? seg_len - tile_first : (uint32_t)ORD_TILE;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int d = threadIdx.x; d < ORD_BINS * ORD_WAVES; d += ORD_BLK) (&L.ctr[0][0])[d] = 0;
    __syncthreads();
    uint32_t key[ORD_PER_LANE];
    bool valid[ORD_PER_LANE];
    float vx[ORD_PER_LANE], vy[ORD_PER_LANE], vz[ORD_PER_LANE];
#pragma unroll
    for (int c = 0; c < ORD_PER_LANE; ++c) {
        const uint32_t e = order_element(tile, c);
        valid[c] = e < seg_len;
        key[c] = valid[c] ? (uint32_t)keys[seg_start + e] : 0u;
    }
#pragma unroll
    for (int c = 0; c < ORD_PER_LANE; ++c)
        if (valid[c]) atomicAdd(&L.ctr[wv][key[c]], 1u);
    __syncthreads();
    // per-wave counts -> per-wave running slot: the bucket's offset inside the tile (exclusive scan of the tile's ORD_BINS bucket
    // totals: four consecutive buckets per thread, then the workgroup's threads) + what the waves before hold
    {
        static_assert(ORD_BINS == 4 * ORD_BLK, "four buckets per thread");
        const int d0 = 4 * threadIdx.x;
        const uint32_t *seg_tab = starts + (size_t)b * (s.tiles + 1) * ORD_BINS;
        const uint4 tp = *reinterpret_cast<const uint4 *>(seg_tab + (size_t)tile * ORD_BINS + d0);
        const uint4 bs = *reinterpret_cast<const uint4 *>(seg_tab + (size_t)s.tiles * ORD_BINS + d0);
        const uint32_t first[4] = {tp.x + bs.x, tp.y + bs.y, tp.z + bs.z, tp.w + bs.w}; // where the tile's queries of the bucket start in the segment
        uint32_t cnt[ORD_WAVES][4], mine = 0;
#pragma unroll
        for (int w = 0; w < ORD_WAVES; ++w)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cnt[w][j] = L.ctr[w][d0 + j];
                mine += cnt[w][j];
            }
        uint32_t incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        if (lane == 63) L.wsum[wv] = incl;
        __syncthreads();
        uint32_t run = incl - mine;
#pragma unroll
        for (int w = 0; w < ORD_WAVES; ++w)
            if (w < wv) run += L.wsum[w];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            L.delta[d0 + j] = first[j] - run; // (uint32 arithmetic: slot + delta is the position in the segment)
#pragma unroll
            for (int w = 0; w < ORD_WAVES; ++w) {
                L.ctr[w][d0 + j] = run;
                run += cnt[w][j];
            }
        }
    }
    __syncthreads();
    // the x plane: in flight while the tile is ranked.  Requested here, behind the counting, so that the wait in front of the counting
    // covers the key loads alone (requested beside them it held the counting back for 16 more loads).  The y and z planes follow behind
    // the ranking; the compiler drains all three, vmcnt(0), in front of the first plane's LDS writes (profiles/LADDER.md, round 11)
#pragma unroll
    for (int c = 0; c < ORD_PER_LANE; ++c) vx[c] = valid[c] ? sx[seg_start + order_element(tile, c)] : 0.0f;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t slot[ORD_PER_LANE];
#pragma unroll
    for (int c = 0; c < ORD_PER_LANE; ++c) { // the wave's chunks in order: stability (the loop of order_scatter_body)
        const unsigned long long peers = order_peers(key[c], valid[c]);
        slot[c] = valid[c] ? L.ctr[wv][key[c]] + (uint32_t)__popcll(peers & below) : 0u;
        __builtin_amdgcn_wave_barrier(); // every lane has read the counter before the group's last lane advances it
        if (valid[c] && (peers >> lane) <= 1ull) L.ctr[wv][key[c]] += (uint32_t)__popcll(peers);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int c = 0; c < ORD_PER_LANE; ++c) {
        if (valid[c]) L.skey[slot[c]] = (uint16_t)key[c];
        vy[c] = valid[c] ? sy[seg_start + order_element(tile, c)] : 0.0f;
        vz[c] = valid[c] ? sz[seg_start + order_element(tile, c)] : 0.0f;
    }
    __syncthreads(); // the counters are done with (the plane takes their place) and every slot has its key
    uint32_t pos[ORD_PER_LANE];
#pragma unroll
    for (int j = 0; j < ORD_PER_LANE; ++j) {
        const uint32_t i = threadIdx.x + (uint32_t)ORD_BLK * j;
        pos[j] = i < tile_cnt ? L.delta[L.skey[i]] + i : 0u;
    }
    order_move_plane(L, vx, valid, slot, pos, tile_cnt, dx + seg_start);
    order_move_plane(L, vy, valid, slot, pos, tile_cnt, dy + seg_start);
    order_move_plane(L, vz, valid, slot, pos, tile_cnt, dz + seg_start);
}

} // namespace sf
