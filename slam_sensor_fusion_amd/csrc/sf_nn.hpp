// sf_nn.hpp — exact 1-NN over the uniform-grid map index (device side, gfx950).
//
// Replaces the N serial FLANN kd-tree descents of
// localization/src/icp_point_to_point.cpp:64-69 (sourceTargetCorrespondences) and the
// Open3D hybrid search behind localization_python/.../localization_node.py:233-237.
// One lane per query.  Two forms: nn_search (each lane on its own; map queries, REF_CPP mode)
// and nn_search_wave (the 64 lanes of a wave share the work; the ICP hot kernel k_nn_red, and
// the brute-force scorer k_bf_score as nn_search_wave<WINDOW, true>, rings included).
//
// Layout: the map is sorted by cell (x fastest), so a row of cells is one contiguous candidate
// range, and ONE 16-byte look-up returns the bounds of the three cells of a row.  The query's own
// cell is scanned first (nn_search_wave: with the slots it leaves idle filled from its x neighbours,
// first_window); its x neighbours and the 8 neighbouring rows only while their gap to the
// query is smaller than the best distance so far.
// What was measured on MI355X and shaped this file (profiles/): a branch per
// candidate load serialises the loads into one round trip each; clamped duplicate loads keep them
// in flight together but every duplicate is an L1 access, and the L1 / texture path is what the
// kernel runs out of -- buffer addressing with an out-of-range offset gives predication without
// either cost; the winner's coordinates stay in registers (re-reading them costs a round trip);
// a per-cell 128-byte bucket layout and 32-byte point+normal records were both slower; after
// the own-cell step only ~6 of 64 lanes have neighbour ranges left to scan, which is why
// nn_search_wave deals that work out across the wave.
//
// Exactness: after scanning the block of radius R around the query's cell, every
// unscanned point is at least m = distance(query, block boundary) away; the search stops
// when best <= m^2 (best starts at the acceptance threshold, so "nothing acceptable
// outside" ends it too), otherwise the block grows by one ring.  Cells, rows and rings are only
// skipped when their distance from the query -- computed in float32 grid coordinates, minus
// SfGrid::gap_eps for the rounding of those coordinates (a point and a query are binned by the
// same monotone float expression, so the true face distance can be shorter than the computed
// one by at most 2^-22 x the largest cell coordinate), times 0.998 -- is not below the best.
// Distance = FLANN L2_Simple in float32: ((dx*dx) + dy*dy) + dz*dz, unfused; strict "<".
#pragma once
#include "sf_common.hpp"

namespace sf {

// SF_PHASE_TRACE (diagnostic build only, tools/phase_trace.py): s_memtime stamps at the phase boundaries of a searching
// wave, summed per phase over the launch.  No stamp executes in the product build.
#ifdef SF_PHASE_TRACE
constexpr int PH_SLOTS = 16, PH_SHARDS = 64;
struct PhaseClock {
    unsigned long long t;
    unsigned acc[PH_SLOTS];
    __device__ __forceinline__ void start() { for (int i = 0; i < PH_SLOTS; ++i) acc[i] = 0; t = __builtin_amdgcn_s_memtime(); }
    __device__ __forceinline__ void mark(int i) { const unsigned long long n = __builtin_amdgcn_s_memtime(); acc[i] += (unsigned)(n - t); t = n; }
    __device__ __forceinline__ void count(int i, unsigned v) { acc[i] += v; }
};
#define SF_PH(pc, i) do { if (pc) (pc)->mark(i); } while (0)
#define SF_PHC(pc, i, v) do { if (pc) (pc)->count(i, v); } while (0)
#else
struct PhaseClock {};
#define SF_PH(pc, i) do { } while (0)
#define SF_PHC(pc, i, v) do { } while (0)
#endif

struct NNHit {
    float d2;         // squared distance of the best candidate (the largest float below the threshold if none)
    int j;            // sorted position of the best candidate, -1 if none
    float px, py, pz; // its coordinates (kept in registers: re-reading the winner costs a round trip)
    float lb2;        // nn_search_wave only: every OTHER map point is at least sqrt(lb2) away from the query
};

__device__ __forceinline__ float l2_simple(float qx, float qy, float qz, float px, float py, float pz)
{
    float dx = qx - px, dy = qy - py, dz = qz - pz;
    float r = __fmul_rn(dx, dx);
    r = __fadd_rn(r, __fmul_rn(dy, dy));
    r = __fadd_rn(r, __fmul_rn(dz, dz));
    return r;
}

__device__ __forceinline__ bool window_accepts(const SfWindow &w, float px, float py, float pz)
{
    if (w.kind == 1) return l2_simple(w.c[0], w.c[1], w.c[2], px, py, pz) < w.r2;
    if (w.kind == 2) {
        double d0 = (double)px - w.oc[0], d1 = (double)py - w.oc[1], d2 = (double)pz - w.oc[2];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double proj = __dadd_rn(__dadd_rn(__dmul_rn(d0, w.oR[k]), __dmul_rn(d1, w.oR[3 + k])), __dmul_rn(d2, w.oR[6 + k]));
            ok = ok && (fabs(proj) <= w.ohalf[k]);
        }
        return ok;
    }
    return true;
}

// A lower bound of the distance from the query to every point the window accepts (0 when the query is inside the
// window or the bound would be in doubt).  A point p passes a sphere window iff |p - c|^2 < r2, so every accepted point
// is at least |q - c| - r away (triangle inequality); for a box window the largest single-axis excess does the same.
// When that bound exceeds sqrt(thr) no candidate can be accepted AND close enough: the search of such a query is
// skipped -- no result changes, only the ring walk that would end empty is spared (on the per-scan path the scan points
// beyond the 10 m map crop of localization_node.cpp:302 are a large share of every scan) -- and the bound itself is the
// query's runner-up bound for the neighbour-reuse certificate.
__device__ __forceinline__ float window_gap(const SfWindow &w, float qx, float qy, float qz)
{
    if (w.kind == 1) {
        const float dx = qx - w.c[0], dy = qy - w.c[1], dz = qz - w.c[2];
        return fmaxf(sqrtf(dx * dx + dy * dy + dz * dz) * 0.9995f - sqrtf(w.r2) * 1.0005f - 1.0e-4f, 0.0f);
    }
    if (w.kind == 2) {
        const double d0 = (double)qx - w.oc[0], d1 = (double)qy - w.oc[1], d2 = (double)qz - w.oc[2];
        double out = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { // the axes need not be orthonormal (the prior is a blend): an excess along axis k is a distance only after division by its norm
            const double proj = d0 * w.oR[k] + d1 * w.oR[3 + k] + d2 * w.oR[6 + k];
            const double n2 = w.oR[k] * w.oR[k] + w.oR[3 + k] * w.oR[3 + k] + w.oR[6 + k] * w.oR[6 + k];
            const double over = fmax(fabs(proj) - w.ohalf[k], 0.0);
            out = fmax(out, over / sqrt(fmax(n2, 1.0e-30)));
        }
        return fmaxf((float)out * 0.9995f - 1.0e-4f, 0.0f);
    }
    return 0.0f;
}

// The best candidate is the LEXICOGRAPHIC minimum of (d2, j) over everything visited -- the same rule in every
// search form, whatever the order ranges are walked in.  One 64-bit unsigned compare of (float bits of d2, index): d2
// is a non-negative finite float, so its bit pattern orders like its value.  "No candidate yet" is the pair
// (largest float below the acceptance threshold, index -1 = 0xffffffff): a candidate is then taken iff d2 < threshold,
// strictly (search_start below).
// TRACK: hit.lb2 follows the smallest squared distance among the examined candidates that did not end up as the
// best (a displaced best included); the best itself, met again, is not "another point".
__device__ __forceinline__ unsigned long long hit_key(float d2, int j) { return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)(uint32_t)j; }

__device__ __forceinline__ float search_start(float thr) { return thr > 0.0f ? __uint_as_float(__float_as_uint(thr) - 1u) : -1.0f; }

template <bool WINDOW, bool TRACK = false>
__device__ __forceinline__ void consider(const SfWindow &w, float px, float py, float pz, int j, bool valid, float qx, float qy, float qz, NNHit &hit)
{
    const float d2 = l2_simple(qx, qy, qz, px, py, pz);
    const bool take = valid && hit_key(d2, j) < hit_key(hit.d2, hit.j) && (!WINDOW || window_accepts(w, px, py, pz));
    // runner-up bound: hit.d2 <= hit.lb2 holds while ranges are scanned, so the median of (this candidate, the best, the
    // bound) IS min(bound, the loser of this comparison) -- one v_med3_f32; the best itself met again and slots without a
    // candidate enter as +big and leave the bound alone
    if (TRACK) hit.lb2 = __builtin_amdgcn_fmed3f((valid && j != hit.j) ? d2 : 3.0e38f, hit.d2, hit.lb2);
    if (take) {
        hit.d2 = d2;
        hit.j = j;
        hit.px = px; hit.py = py; hit.pz = pz;
    }
}

// candidates [j, min(j + 4, b)) of a non-empty CSR range: four independent 16-byte loads, issued
// together.  Measured (TA / TCP counters): the kernel is bound by the number of per-lane accesses
// the L1 (TCP) has to look up, ~1 per clock per CU -- so a lane must not touch memory for a
// candidate that does not exist.  A branch per candidate serialises the loads (a round trip
// each, measured), clamping the index into the range keeps them in flight together but every
// duplicate is still an access; buffer addressing does both: an out-of-range offset makes the TA
// drop the lane's access and return zeros, without control flow.
#ifndef SF_NN_CLAMPED_LOADS
__device__ __forceinline__ float4 load_point(const SfGrid &g, uint32_t j, bool valid)
{
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)g.pts, 0, (int)((uint32_t)g.n * 16u), 0x00020000);
    const u4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, valid ? (int)(j * 16u) : -1, 0, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
#else
__device__ __forceinline__ float4 load_point(const SfGrid &g, uint32_t j, bool valid) { return g.pts[valid ? j : 0u]; }
#endif

template <bool WINDOW, bool TRACK = false>
__device__ __forceinline__ void scan4(const SfGrid &g, const SfWindow &w, uint32_t j, uint32_t b, float qx, float qy, float qz, NNHit &hit)
{
#ifndef SF_NN_CLAMPED_LOADS
    const float4 p0 = load_point(g, j, true), p1 = load_point(g, j + 1, j + 1 < b), p2 = load_point(g, j + 2, j + 2 < b), p3 = load_point(g, j + 3, j + 3 < b);
    consider<WINDOW, TRACK>(w, p0.x, p0.y, p0.z, (int)j, true, qx, qy, qz, hit);
    consider<WINDOW, TRACK>(w, p1.x, p1.y, p1.z, (int)(j + 1), j + 1 < b, qx, qy, qz, hit);
    consider<WINDOW, TRACK>(w, p2.x, p2.y, p2.z, (int)(j + 2), j + 2 < b, qx, qy, qz, hit);
    consider<WINDOW, TRACK>(w, p3.x, p3.y, p3.z, (int)(j + 3), j + 3 < b, qx, qy, qz, hit);
#else
    const uint32_t last = b - 1;
    const uint32_t j1 = min(j + 1, last), j2 = min(j + 2, last), j3 = min(j + 3, last);
    const float4 p0 = g.pts[j], p1 = g.pts[j1], p2 = g.pts[j2], p3 = g.pts[j3];
    consider<WINDOW, TRACK>(w, p0.x, p0.y, p0.z, (int)j, true, qx, qy, qz, hit);
    consider<WINDOW, TRACK>(w, p1.x, p1.y, p1.z, (int)j1, j + 1 < b, qx, qy, qz, hit);
    consider<WINDOW, TRACK>(w, p2.x, p2.y, p2.z, (int)j2, j + 2 < b, qx, qy, qz, hit);
    consider<WINDOW, TRACK>(w, p3.x, p3.y, p3.z, (int)j3, j + 3 < b, qx, qy, qz, hit);
#endif
}

// CSR candidates [a, b).  (Eight loads in flight per trip instead of four: measured slower at 32 scans in flight --
// 545 -> 609 us for a searching launch, 89 -> 94 us for a verifying one -- and slower on the per-scan path too, even
// when only the REF_CPP search was built that way: 404 -> 434 us per search at 32 in flight, callback 0.72 -> 0.76 ms.)
template <bool WINDOW, bool TRACK = false>
__device__ __forceinline__ void scan_range(const SfGrid &g, const SfWindow &w, uint32_t a, uint32_t b, float qx, float qy, float qz, NNHit &hit)
{
    for (uint32_t j = a; j < b; j += 4) scan4<WINDOW, TRACK>(g, w, j, b, qx, qy, qz, hit);
}

__device__ __forceinline__ float min3f(float a, float b, float c) { return fminf(fminf(a, b), c); } // one v_min3_f32

// cell_start[c-1 .. c+2] in ONE 16-byte load (the table carries one pad entry in front, so
// c - 1 >= -1 is addressable; dword alignment is enough for global_load_dwordx4)
struct __attribute__((packed, aligned(4))) RowBounds { uint32_t s0, s1, s2, s3; };
__device__ __forceinline__ RowBounds load_row_bounds(const SfGrid &g, size_t cell)
{
    return *reinterpret_cast<const RowBounds *>(g.cell_start + cell - 1);
}

// one (y,z) row around column cx: the query's own x cell first, then the left / right cell
// only while their gap (row gap + x gap) is still smaller than the best distance
template <bool WINDOW>
__device__ __forceinline__ void scan_row(const SfGrid &g, const SfWindow &w, const RowBounds &rb, float gap2yz, float gxm2, float gxp2, bool xm, bool xp, float qx,
                                         float qy, float qz, NNHit &hit)
{
    scan_range<WINDOW>(g, w, rb.s1, rb.s2, qx, qy, qz, hit);
    if (xm && (gap2yz + gxm2) * 0.998f < hit.d2) scan_range<WINDOW>(g, w, rb.s0, rb.s1, qx, qy, qz, hit);
    if (xp && (gap2yz + gxp2) * 0.998f < hit.d2) scan_range<WINDOW>(g, w, rb.s2, rb.s3, qx, qy, qz, hit);
}

// a face distance with the rounding slack of the grid coordinates taken off (never negative): the
// true distance is at least this
__device__ __forceinline__ float safe_gap(float gap, float eps) { return fmaxf(gap - eps, 0.0f); }

// distance (in cells, >= 0) from grid coordinate gc to the cell interval [c, c+1]
__device__ __forceinline__ float cell_gap(float gc, int c, int cq)
{
    if (c == cq) return 0.0f;
    float d = c < cq ? gc - (float)(c + 1) : (float)c - gc;
    return d > 0.0f ? d : 0.0f;
}

// the cell of grid coordinate gc on an axis of n cells.  Clamp in float first: a far-away query must not overflow the int
// conversion
__device__ __forceinline__ int grid_cell(float gc, int n) { return (int)fminf(fmaxf(floorf(gc), 0.0f), (float)(n - 1)); }

// The exactness certificate: the distance from grid coordinates (gx, gy, gz), binned in cell (cx, cy, cz), to the nearest face of
// the block of radius R around that cell that still has grid cells behind it; 3e38 when the block covers the grid.  Every point
// outside the block is at least safe_gap(this, gap_eps) away.
__device__ __forceinline__ float block_face_gap(const SfGrid &g, float gx, float gy, float gz, int cx, int cy, int cz, int R)
{
    const float h = g.h;
    float m = 3.0e38f;
    if (cx - R > 0) m = fminf(m, (gx - (float)(cx - R)) * h);
    if (cx + R < g.dim[0] - 1) m = fminf(m, ((float)(cx + R + 1) - gx) * h);
    if (cy - R > 0) m = fminf(m, (gy - (float)(cy - R)) * h);
    if (cy + R < g.dim[1] - 1) m = fminf(m, ((float)(cy + R + 1) - gy) * h);
    if (cz - R > 0) m = fminf(m, (gz - (float)(cz - R)) * h);
    if (cz + R < g.dim[2] - 1) m = fminf(m, ((float)(cz + R + 1) - gz) * h);
    return m;
}

// Row trim: the x-run [x0, x1] of a row whose (y, z) gap squared is g2, less the end cells whose own gap prunes them against
// `bound` (the query's own column cx never is).  Two functions that return a value: one with two reference results more than
// doubled every kernel that inlines it.  radius_walk (sf_walk.hpp) calls them; knn_search keeps the two loops written out,
// because called there they made k_normals_knn 0.3 - 4 % slower (profiles/grid_walk_first_form_ab.jsonl).
__device__ __forceinline__ int trim_left(const SfGrid &g, float gx, int cx, int x0, float g2, float bound)
{
    int xa = x0;
    while (xa < cx) {
        const float gl = safe_gap(cell_gap(gx, xa, cx) * g.h, g.gap_eps);
        if ((g2 + gl * gl) * 0.998f < bound) break;
        ++xa;
    }
    return xa;
}
__device__ __forceinline__ int trim_right(const SfGrid &g, float gx, int cx, int x1, float g2, float bound)
{
    int xb = x1;
    while (xb > cx) {
        const float gr = safe_gap(cell_gap(gx, xb, cx) * g.h, g.gap_eps);
        if ((g2 + gr * gr) * 0.998f < bound) break;
        --xb;
    }
    return xb;
}

// thr: candidates are accepted iff d2 < thr (reference: max_correspondence_dist_ itself,
// icp_point_to_point.cpp:70; Open3D: radius^2)
// rings R_first, R_first + 1, ... around the query's cell until the exactness test holds
template <bool WINDOW>
__device__ __forceinline__ void nn_rings(const SfGrid &g, const SfWindow &w, float qx, float qy, float qz, int R_first, NNHit &hit)
{
    const float gx = (qx - g.org[0]) * g.inv_h, gy = (qy - g.org[1]) * g.inv_h, gz = (qz - g.org[2]) * g.inv_h;
    const int nx = g.dim[0], ny = g.dim[1], nz = g.dim[2];
    const int cx = grid_cell(gx, nx), cy = grid_cell(gy, ny), cz = grid_cell(gz, nz);
    const float h = g.h;
    const int rcap = max(nx, max(ny, nz));

    for (int R = R_first; R <= rcap; ++R) {
        {
            // ---- CSR path: rows of 2R+1 cells
            const int x0 = max(cx - R, 0), x1 = min(cx + R, nx - 1);
            const int y0 = max(cy - R, 0), y1 = min(cy + R, ny - 1);
            const int z0 = max(cz - R, 0), z1 = min(cz + R, nz - 1);
            if (R == 1) {
                // Ring 1 on the CSR rows.  Per query: one 16-byte look-up gives the bounds of the
                // three cells of a row; the own cell is scanned first, the x neighbours and the
                // 8 neighbouring rows only while their gap is smaller than the best distance.
                // Which rows a query needs depends on where it sits in its cell, so the row list is
                // per-LANE data (bit mask walked with ffs) and the next row's bounds are requested
                // before the current row is scanned.
                //   k      0   1   2   3   4   5   6   7
                //   dy    -1  +1   0   0  -1  +1  -1  +1
                //   dz     0   0  -1  +1  -1  -1  +1  +1
                constexpr uint32_t OYP = 0u | (2u << 2) | (1u << 4) | (1u << 6) | (0u << 8) | (2u << 10) | (0u << 12) | (2u << 14);
                constexpr uint32_t OZP = 1u | (1u << 2) | (0u << 4) | (2u << 6) | (0u << 8) | (0u << 10) | (2u << 12) | (2u << 14);
                const float fx = gx - (float)cx, fy = gy - (float)cy, fz = gz - (float)cz;
                const float ge = g.gap_eps;
                const float gxm = safe_gap(fx * h, ge), gxp = safe_gap((1.0f - fx) * h, ge);
                const float gym = safe_gap(fy * h, ge), gyp = safe_gap((1.0f - fy) * h, ge);
                const float gzm = safe_gap(fz * h, ge), gzp = safe_gap((1.0f - fz) * h, ge);
                const float gxm2 = gxm * gxm, gxp2 = gxp * gxp;
                const bool xm = cx > 0, xp = cx < nx - 1;
                auto row_gap2 = [&](int k) -> float {
                    const int dy = (int)((OYP >> (2 * k)) & 3u) - 1, dz = (int)((OZP >> (2 * k)) & 3u) - 1;
                    const float ry = dy < 0 ? gym : (dy > 0 ? gyp : 0.0f);
                    const float rz = dz < 0 ? gzm : (dz > 0 ? gzp : 0.0f);
                    return ry * ry + rz * rz;
                };
                auto row_cell = [&](int k) -> size_t {
                    const int dy = (int)((OYP >> (2 * k)) & 3u) - 1, dz = (int)((OZP >> (2 * k)) & 3u) - 1;
                    return ((size_t)(cz + dz) * ny + (cy + dy)) * nx + cx;
                };
                {
                    const RowBounds rb = load_row_bounds(g, ((size_t)cz * ny + cy) * nx + cx);
                    scan_row<WINDOW>(g, w, rb, 0.0f, gxm2, gxp2, xm, xp, qx, qy, qz, hit);
                }
                uint32_t mask = 0;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int dy = (int)((OYP >> (2 * k)) & 3u) - 1, dz = (int)((OZP >> (2 * k)) & 3u) - 1;
                    const bool inside = (unsigned)(cy + dy) < (unsigned)ny && (unsigned)(cz + dz) < (unsigned)nz;
                    if (inside && row_gap2(k) * 0.998f < hit.d2) mask |= 1u << k;
                }
                int k = -1;
                RowBounds cur = {0, 0, 0, 0};
                if (mask) {
                    k = __ffs((int)mask) - 1;
                    mask &= mask - 1;
                    cur = load_row_bounds(g, row_cell(k));
                }
                while (k >= 0) {
                    int k1 = -1;
                    RowBounds nxt = cur;
                    while (mask) {
                        const int kk = __ffs((int)mask) - 1;
                        mask &= mask - 1;
                        if (row_gap2(kk) * 0.998f < hit.d2) {
                            k1 = kk;
                            nxt = load_row_bounds(g, row_cell(kk));
                            break;
                        }
                    }
                    const float g2 = row_gap2(k);
                    if (g2 * 0.998f < hit.d2) scan_row<WINDOW>(g, w, cur, g2, gxm2, gxp2, xm, xp, qx, qy, qz, hit);
                    k = k1;
                    cur = nxt;
                }
            } else {
                for (int z = z0; z <= z1; ++z) {
                    const float rz = safe_gap(cell_gap(gz, z, cz) * h, g.gap_eps);
                    for (int y = y0; y <= y1; ++y) {
                        const float ry = safe_gap(cell_gap(gy, y, cy) * h, g.gap_eps);
                        if ((ry * ry + rz * rz) * 0.998f >= hit.d2) continue;
                        const size_t row = ((size_t)z * ny + y) * nx;
                        scan_range<WINDOW>(g, w, g.cell_start[row + x0], g.cell_start[row + x1 + 1], qx, qy, qz, hit);
                    }
                }
            }
        }
        const float m = block_face_gap(g, gx, gy, gz, cx, cy, cz, R);
        if (m >= 3.0e38f) break; // whole grid scanned
        const float mm = safe_gap(m, g.gap_eps) * 0.999f;
        if (hit.d2 <= mm * mm) break;
    }
}

template <bool WINDOW>
__device__ __forceinline__ NNHit nn_search(const SfGrid &g, const SfWindow &w, float qx, float qy, float qz, float thr)
{
    NNHit hit;
    hit.d2 = search_start(thr);
    hit.j = -1;
    hit.px = hit.py = hit.pz = 0.0f;
    hit.lb2 = 0.0f;
    if (!(isfinite(qx) && isfinite(qy) && isfinite(qz)) || g.n == 0) return hit;
    if (WINDOW) {
        const float gap = window_gap(w, qx, qy, qz);
        if (gap * gap > thr) return hit;
    }
    nn_rings<WINDOW>(g, w, qx, qy, qz, 1, hit);
    return hit;
}

// ------------------------------------------------------------------ wave-cooperative search
// Measured (pass counters, 200 k-point scans vs the 10 M-point map): after every lane has scanned
// its query's own cell (one step with all 64 lanes busy), the per-lane walk above spends ~10 more
// wave-level steps on the x neighbours / neighbouring rows that still survive pruning, with ~6 of
// 64 lanes active in each -- in total fewer than 64 lane-steps of real work.  Here the surviving
// (query, range) TASKS of the whole wave go into an LDS queue and are dealt out one per lane, so
// that work takes one or two full steps.  A task scans one contiguous candidate range:
//   t = 0, 1   the left / right x neighbour of the own cell, less what the first trip's window took of it (first_window)
//   t = 2 + k  neighbouring row k (own-x cell plus the x neighbours whose gap is still below the best)
//   t = 10     what is left of an own cell that holds more than four points
// and lowers its owner's packed (d2, j) in LDS with ds_min_u64.  The result is the lexicographic
// minimum of (d2, j) over everything visited; pruning only ever skips ranges that cannot hold a
// candidate as good as the current best (0.2 % margin), and a task reports ties with the best it
// started from, so the result does not depend on the order in which lanes finish.
// Flat rounds (WINDOW = false): a lane does not scan its task's range itself.  The 64 ranges of a round, pruned as above,
// are laid end to end and their candidates dealt out over the wave, NN_DEAL_K per lane per trip, so a round costs
// ceil(sum of lengths / (64 NN_DEAL_K)) trips -- about one -- instead of the longest range's ceil(length / 4).  Same
// visited set, same result, same runner-up bound (the second smallest (d2, j) over what was visited, with the gaps of
// what was pruned -- which does not depend on the order of the comparisons).  A windowed search keeps one range per
// lane: there a candidate the window rejects enters the runner-up bound through the lane's running best.
#ifndef SF_NN_DEAL_K
#define SF_NN_DEAL_K 2
#endif
constexpr int NN_DEAL_K = SF_NN_DEAL_K; // candidate slots per lane in one trip of a flat round
struct WaveNN {
    unsigned long long best[64]; // (float bits of d2) << 32 | j; j = 0xffffffff: none
    uint32_t lb2[64];            // float bits: lower bound of the squared distance to every point but the best
    float4 q[64];                // the query and, in .w, its gxm2
    RowBounds rb0[64];           // bounds of the own cell and its x neighbours (tasks 0, 1, 10)
    float gap[5][64];            // the owner's other gaps (gxp2, gym, gyp, gzm, gzp) and ...
    unsigned long long cell0[64]; // ... the linear index of its cell: a task gets its geometry from here instead of recomputing it (~45 instructions per task)
    uint16_t task[64 * 11];      // owner lane << 4 | t, grouped by t
    alignas(4) uint8_t mark[64 * NN_DEAL_K]; // flat rounds: lane + 1 of the task whose range starts at this slot of the trip, 0 elsewhere
};

__device__ __forceinline__ unsigned long long pack_hit(float d2, int j) { return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)(uint32_t)j; }

struct QueryGeo {
    int cx, cy, cz;
    float gxm2, gxp2;          // (gap to the left / right x neighbour)^2, 3e38 at the grid border
    float gym, gyp, gzm, gzp;  // gaps to the neighbouring rows
};

__device__ __forceinline__ QueryGeo query_geo(const SfGrid &g, float qx, float qy, float qz)
{
    QueryGeo G;
    const float gx = (qx - g.org[0]) * g.inv_h, gy = (qy - g.org[1]) * g.inv_h, gz = (qz - g.org[2]) * g.inv_h;
    G.cx = grid_cell(gx, g.dim[0]);
    G.cy = grid_cell(gy, g.dim[1]);
    G.cz = grid_cell(gz, g.dim[2]);
    const float h = g.h;
    const float fx = gx - (float)G.cx, fy = gy - (float)G.cy, fz = gz - (float)G.cz;
    const float ge = g.gap_eps;
    const float gxm = safe_gap(fx * h, ge), gxp = safe_gap((1.0f - fx) * h, ge);
    G.gxm2 = G.cx > 0 ? gxm * gxm : 3.0e38f;
    G.gxp2 = G.cx < g.dim[0] - 1 ? gxp * gxp : 3.0e38f;
    G.gym = safe_gap(fy * h, ge);
    G.gyp = safe_gap((1.0f - fy) * h, ge);
    G.gzm = safe_gap(fz * h, ge);
    G.gzp = safe_gap((1.0f - fz) * h, ge);
    return G;
}

// The first trip of nn_search_wave: a window [lo, hi) of at most NN_ROW_CAP consecutive CSR positions of the query's own
// row, inside [rb.s0, rb.s3).  The own cell comes first; at 1.5 points per cell it seldom fills the trip's slots, and the x
// neighbours lie contiguous with it in the CSR, described by the row bounds the lane already holds -- so the slots the own
// cell leaves idle go to the neighbour whose face is nearer (the first positions of the right cell, the last of the left
// one), and what that side cannot supply to the other.  A side without a neighbour in the grid (gap 3e38) gets none: what
// lies there in memory is another row's.  round_task re-derives the same window from the same three values.
// SF_NN_ROW_WINDOW: 0 the own cell only, 1 nearer side first (shipped), 2 right then left, 3 the whole own row, up to 8
// positions in two trips (profiles/row_window_ab.txt)
#ifndef SF_NN_ROW_WINDOW
#define SF_NN_ROW_WINDOW 1
#endif
#ifndef SF_NN_ROW_GATE
#define SF_NN_ROW_GATE 0 // slot_row below: measured, off (every neighbour the grid has may fill idle slots; LADDER round 12)
#endif
constexpr uint32_t NN_ROW_CAP = SF_NN_ROW_WINDOW == 3 ? 8u : 4u;
struct RowWindow { uint32_t lo, hi; };
__device__ __forceinline__ RowWindow first_window(const RowBounds &rb, float gxm2, float gxp2)
{
    const uint32_t own = min(rb.s2 - rb.s1, NN_ROW_CAP);
    RowWindow W;
#if SF_NN_ROW_WINDOW == 0
    W.lo = rb.s1; W.hi = rb.s1 + own;
#else
    const uint32_t idle = NN_ROW_CAP - own;
    const uint32_t nl = gxm2 < 1.0e38f ? rb.s1 - rb.s0 : 0u, nr = gxp2 < 1.0e38f ? rb.s3 - rb.s2 : 0u;
    const bool right_first = SF_NN_ROW_WINDOW == 2 || gxp2 <= gxm2;
    const uint32_t t1 = min(idle, right_first ? nr : nl);
    const uint32_t t2 = min(idle - t1, right_first ? nl : nr);
    W.lo = rb.s1 - (right_first ? t2 : t1);
    W.hi = rb.s1 + own + (right_first ? t1 : t2); // (own < NN_ROW_CAP, or nothing is added: past rb.s2 only with the whole own cell inside)
#endif
    return W;
}

// The row the window is laid over (SF_NN_ROW_GATE; off, the row is the one loaded: the switch bought the second launch
// nothing and the third came out 13 us longer, profiles/row_window_ab.txt).  On: a neighbour whose gap does not pass the
// bound the search STARTS from (the acceptance threshold, or the seed's distance: small from the second launch of an
// alignment on) can never be queued -- the best only
// falls -- so it gets no slot either: a slot there is a lane access for nothing.  Its cell is cut off the row (s0 = s1,
// s3 = s2); the copy goes to WaveNN::rb0, so that round_task lays the same window (task 0 / 1 of a side that was cut off does
// not exist), while the mask of nn_search_wave still sees the cell in the bounds as loaded and gives its gap to the
// runner-up bound.
__device__ __forceinline__ RowBounds slot_row(RowBounds rb, float gxm2, float gxp2, float start)
{
#if SF_NN_ROW_GATE
    if (!(gxm2 * 0.998f < start)) rb.s0 = rb.s1;
    if (!(gxp2 * 0.998f < start)) rb.s3 = rb.s2;
#endif
    return rb;
}

// the candidates of a non-empty window: four loads issued together, slots past W.hi dropped (scan4)
template <bool WINDOW>
__device__ __forceinline__ void scan_first(const SfGrid &g, const SfWindow &w, const RowWindow &W, float qx, float qy, float qz, NNHit &hit)
{
    if constexpr (NN_ROW_CAP == 4u) scan4<WINDOW, true>(g, w, W.lo, W.hi, qx, qy, qz, hit);
    else scan_range<WINDOW, true>(g, w, W.lo, W.hi, qx, qy, qz, hit);
}

//   k      0   1   2   3   4   5   6   7
//   dy    -1  +1   0   0  -1  +1  -1  +1
//   dz     0   0  -1  +1  -1  -1  +1  +1
__device__ __forceinline__ int row_dy(int k) { return (int)((0x8858u >> (2 * k)) & 3u) - 1; } // dy + 1, two bits per k
__device__ __forceinline__ int row_dz(int k) { return (int)((0xa085u >> (2 * k)) & 3u) - 1; }

__device__ __forceinline__ float row_gap2(const QueryGeo &G, int k)
{
    const int dy = row_dy(k), dz = row_dz(k);
    const float ry = dy < 0 ? G.gym : (dy > 0 ? G.gyp : 0.0f);
    const float rz = dz < 0 ? G.gzm : (dz > 0 ? G.gzp : 0.0f);
    return ry * ry + rz * rz;
}

// inclusive scan (sum or max) of a 32-bit value over the 64 lanes: shifts of 1, 2, 4, 8 inside each row of 16, then
// row 0's last lane into row 1 and row 2's into row 3, then lane 31 into rows 2 and 3 -- DPP only, no LDS round trip
template <bool MAX>
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    auto op = [](uint32_t a, uint32_t b) { return MAX ? max(a, b) : a + b; };
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false)); // row_shr:1
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false)); // row_shr:2
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false)); // row_shr:4
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false)); // row_shr:8
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false)); // row_bcast:15 into rows 1, 3
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false)); // row_bcast:31 into rows 2, 3
    return v;
}

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// one ring-1 task of a round up to its candidate range: the owner's query, the owner's best at the start of the round,
// the range [a, b) after the x neighbours are pruned (live = false: the whole task is pruned) and the bound that what it
// prunes contributes to the owner's runner-up bound
struct RoundTask {
    int owner;
    bool live;
    uint32_t a, b;
    float bound;
    float4 Q;
    unsigned long long start;
};

__device__ __forceinline__ RoundTask round_task(const SfGrid &g, WaveNN *ws, uint32_t e)
{
    const int nx = g.dim[0], ny = g.dim[1];
    RoundTask T;
    T.owner = (int)(e >> 4);
    const int owner = T.owner, t = (int)(e & 15u);
    T.Q = ws->q[owner];
    QueryGeo G; // from the owner's entry (cx, cy, cz are not needed: the row is addressed relative to the owner's cell)
    G.cx = G.cy = G.cz = 0;
    G.gxm2 = T.Q.w; G.gxp2 = ws->gap[0][owner];
    G.gym = ws->gap[1][owner]; G.gyp = ws->gap[2][owner]; G.gzm = ws->gap[3][owner]; G.gzp = ws->gap[4][owner];
    T.start = __atomic_load_n(&ws->best[owner], __ATOMIC_RELAXED);
    const float cur = __uint_as_float((uint32_t)(T.start >> 32));
    const bool own_row = t < 2 || t == 10;
    const float g2 = own_row ? (t == 0 ? G.gxm2 : (t == 1 ? G.gxp2 : 0.0f)) : row_gap2(G, t - 2);
    T.bound = g2;
    T.a = T.b = 0;
    T.live = g2 * 0.998f < cur;
    if (T.live) {
        T.bound = 3.0e38f;
        if (own_row) {
            const RowBounds rb = ws->rb0[owner]; // what the first trip's window left of the own row
            const RowWindow W = first_window(rb, G.gxm2, G.gxp2);
            T.a = t == 0 ? rb.s0 : (t == 1 ? max(W.hi, rb.s2) : W.hi);
            T.b = t == 0 ? W.lo : (t == 1 ? rb.s3 : rb.s2);
        } else {
            const long long step = ((long long)row_dz(t - 2) * ny + row_dy(t - 2)) * nx; // the row's cell relative to the owner's (inside the grid: checked when queued)
            const RowBounds rb = load_row_bounds(g, (size_t)((long long)ws->cell0[owner] + step));
            const bool xm = (g2 + G.gxm2) * 0.998f < cur, xp = (g2 + G.gxp2) * 0.998f < cur;
            T.a = xm ? rb.s0 : rb.s1;
            T.b = xp ? rb.s3 : rb.s2;
            if (!xm && rb.s0 < rb.s1) T.bound = g2 + G.gxm2;
            if (!xp && rb.s2 < rb.s3) T.bound = fminf(T.bound, g2 + G.gxp2);
        }
    }
    return T;
}

// every lane of the wave must call this (lanes without a query pass valid = false: they still work).
// Besides the nearest neighbour the result carries lb2: a lower bound of the squared distance from
// the query to every OTHER map point (the runner-up among the examined candidates, the gaps of
// everything that was pruned, the boundary of the 27-cell block) -- what k_nn_red needs to prove,
// one iteration later, that the neighbour cannot have changed.
// seed (optional, seed.j >= 0): a map point already known for this query -- its neighbour of an earlier search -- with its
// CURRENT squared distance seed.d2 (l2_simple of the query and the point).  The search then starts from that bound
// instead of the acceptance threshold: the same exact result (the seed is a candidate like any other, met again when
// its range is scanned), most neighbour ranges pruned before they are visited.
// COOP: how the rare queries that need more than ring 1 go on (see the end of the function)
template <bool WINDOW, bool COOP = false>
__device__ __forceinline__ NNHit nn_search_wave(const SfGrid &g, const SfWindow &w, bool valid, float qx, float qy, float qz, float thr, WaveNN *ws, NNHit seed = NNHit{0.0f, -1, 0.0f, 0.0f, 0.0f, 0.0f},
                                               PhaseClock *pc = nullptr)
{
    const int lane = (int)__lane_id();
    const int nx = g.dim[0], ny = g.dim[1], nz = g.dim[2];
    NNHit hit;
    hit.d2 = search_start(thr);
    hit.j = -1;
    hit.px = hit.py = hit.pz = 0.0f;
    hit.lb2 = 3.0e38f;
    valid = valid && isfinite(qx) && isfinite(qy) && isfinite(qz) && g.n > 0;
    if (WINDOW && valid) {
        const float gap = window_gap(w, qx, qy, qz);
        if (gap * gap > thr) { // nothing the window accepts is within the acceptance radius
            hit.lb2 = gap * gap;
            valid = false;
        }
    }
    if (valid) {
        // a query farther from the map's bounding box (the grid's: every point is inside it) than the acceptance radius has
        // no neighbour -- known without a walk through empty rings, and the distance to the box is its runner-up bound: scan
        // points beyond the rim of the map certify as "still nothing" from then on instead of searching in every launch
        const float ox = fmaxf(fmaxf(g.org[0] - qx, qx - (g.org[0] + (float)nx * g.h)), 0.0f);
        const float oy = fmaxf(fmaxf(g.org[1] - qy, qy - (g.org[1] + (float)ny * g.h)), 0.0f);
        const float oz = fmaxf(fmaxf(g.org[2] - qz, qz - (g.org[2] + (float)nz * g.h)), 0.0f);
        const float gap = fmaxf(sqrtf(ox * ox + oy * oy + oz * oz) * 0.9995f - 1.0e-3f, 0.0f); // (1 mm: the float32 corner of the box)
        if (gap * gap > thr) {
            hit.lb2 = gap * gap;
            valid = false;
        }
    }
    if (valid && seed.j >= 0 && seed.d2 < thr) { hit.d2 = seed.d2; hit.j = seed.j; hit.px = seed.px; hit.py = seed.py; hit.pz = seed.pz; }
    uint32_t mask = 0;
    float q_gxm2 = 0.0f;
#ifdef SF_PHASE_TRACE
    QueryGeo G{};
    RowBounds rb0{0, 0, 0, 0};
    RowWindow W{0, 0};
    if (valid) {
        G = query_geo(g, qx, qy, qz);
        rb0 = load_row_bounds(g, ((size_t)G.cz * ny + G.cy) * nx + G.cx);
        const RowBounds rbw = slot_row(rb0, G.gxm2, G.gxp2, hit.d2);
        ws->rb0[lane] = rbw;
        W = first_window(rbw, G.gxm2, G.gxp2);
    }
    SF_PH(pc, 1);
    if (valid && W.lo < W.hi) scan_first<WINDOW>(g, w, W, qx, qy, qz, hit);
    { unsigned c = W.hi - W.lo; for (int o = 32; o > 0; o >>= 1) c += (unsigned)__shfl_xor((int)c, o); SF_PHC(pc, 15, c); } // live slots of the first trip
    SF_PH(pc, 2);
    if (valid) {
#else
    if (valid) {
        const QueryGeo G = query_geo(g, qx, qy, qz);
        const RowBounds rb0 = load_row_bounds(g, ((size_t)G.cz * ny + G.cy) * nx + G.cx);
        const RowBounds rbw = slot_row(rb0, G.gxm2, G.gxp2, hit.d2);
        ws->rb0[lane] = rbw;
        const RowWindow W = first_window(rbw, G.gxm2, G.gxp2);
        if (W.lo < W.hi) scan_first<WINDOW>(g, w, W, qx, qy, qz, hit);
#endif
        if (W.hi < rb0.s2) { // an own cell of more than NN_ROW_CAP points
            if (hit.d2 > 0.0f) mask |= 1u << 10;
            else hit.lb2 = 0.0f; // the rest of the cell is not examined
        }
        // the x neighbours, less what the window took of them: a range that is not queued because its gap is too large
        // bounds the runner-up by that gap
        if (rb0.s0 < W.lo) {
            if (G.gxm2 * 0.998f < hit.d2) mask |= 1u;
            else hit.lb2 = fminf(hit.lb2, G.gxm2);
        }
        if (max(W.hi, rb0.s2) < rb0.s3) {
            if (G.gxp2 * 0.998f < hit.d2) mask |= 2u;
            else hit.lb2 = fminf(hit.lb2, G.gxp2);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool inside = (unsigned)(G.cy + row_dy(k)) < (unsigned)ny && (unsigned)(G.cz + row_dz(k)) < (unsigned)nz;
            const float gap2 = row_gap2(G, k);
            if (inside) {
                if (gap2 * 0.998f < hit.d2) mask |= 4u << k;
                else hit.lb2 = fminf(hit.lb2, gap2);
            }
        }
        if (mask) { // what the tasks of this query need of its geometry (gxm2 goes with the query)
            q_gxm2 = G.gxm2;
            ws->gap[0][lane] = G.gxp2;
            ws->gap[1][lane] = G.gym; ws->gap[2][lane] = G.gyp; ws->gap[3][lane] = G.gzm; ws->gap[4][lane] = G.gzp;
            ws->cell0[lane] = ((unsigned long long)G.cz * (unsigned long long)ny + (unsigned long long)G.cy) * (unsigned long long)nx + (unsigned long long)G.cx;
        }
    }
    ws->best[lane] = pack_hit(hit.d2, hit.j);
    ws->lb2[lane] = __float_as_uint(hit.lb2);
    ws->q[lane] = make_float4(qx, qy, qz, q_gxm2);
    int total = 0;
#pragma unroll
    for (int t = 0; t < 11; ++t) {
        const bool has = (mask >> t) & 1u;
        const unsigned long long bal = __ballot(has);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if (has) ws->task[total + rank] = (uint16_t)((lane << 4) | t);
        total += __popcll(bal);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    SF_PH(pc, 3);
    SF_PHC(pc, 11, (unsigned)total);
#ifdef SF_PHASE_TRACE
    unsigned lane_trips = 0, lane_cands = 0;
#endif
    for (int i0 = 0; i0 < total; i0 += 64) {
        SF_PHC(pc, 9, 1u);
        const int idx = i0 + lane;
        if constexpr (WINDOW) { // one task per lane, its range scanned by the lane itself
#ifdef SF_PHASE_TRACE
            unsigned my_trips = 0;
#endif
            if (idx < total) {
                const RoundTask T = round_task(g, ws, ws->task[idx]);
                float bound = T.bound; // what this task contributes to the owner's runner-up bound
                if (T.live) {
                    // the task starts from the owner's best as it stands: ties are settled by the index rule of consider(),
                    // the best itself -- met again in its own range -- is neither taken nor counted as a runner-up
                    NNHit h;
                    h.d2 = __uint_as_float((uint32_t)(T.start >> 32));
                    h.j = (int)(uint32_t)T.start;
                    h.px = h.py = h.pz = 0.0f;
                    h.lb2 = 3.0e38f;
                    scan_range<WINDOW, true>(g, w, T.a, T.b, T.Q.x, T.Q.y, T.Q.z, h);
#ifdef SF_PHASE_TRACE
                    my_trips = (T.b - T.a + 3u) / 4u; lane_cands += T.b - T.a; lane_trips += my_trips;
#endif
                    bound = fminf(bound, h.lb2);
                    const unsigned long long mine = pack_hit(h.d2, h.j);
                    if (mine != T.start) { // something lexicographically smaller: whichever of (the best by now, this candidate) loses is a runner-up
                        const unsigned long long old = atomicMin(&ws->best[T.owner], mine);
                        bound = fminf(bound, __uint_as_float((uint32_t)((old > mine ? old : mine) >> 32)));
                    }
                }
                atomicMin(&ws->lb2[T.owner], __float_as_uint(bound));
            }
#ifdef SF_PHASE_TRACE
            { unsigned m = my_trips; for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o)); SF_PHC(pc, 10, m); }
#endif
        } else {
            // Flat round.  Each lane prunes its task exactly as above (against the owner's best at the start of the
            // round) and ends with a range [a, a + len); the ranges are laid end to end by an exclusive scan of len, and
            // slot s of trip c (s = c * 64 K + k * 64 + lane, k < K) takes the candidate at offset s of that list.
            uint32_t a = 0, len = 0;
            int owner = 0;
            if (idx < total) {
                const RoundTask T = round_task(g, ws, ws->task[idx]);
                owner = T.owner;
                if (T.live) { a = T.a; len = T.b - T.a; }
                atomicMin(&ws->lb2[owner], __float_as_uint(T.bound));
            }
            const uint32_t incl = wave_incl_scan<false>(len);
            const uint32_t off = incl - len;
            const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            const uint32_t base = a - off; // the candidate of slot s of this lane's task is base + s (mod 2^32)
            SF_PHC(pc, 13, tot);
            uint32_t carry = 0; // lane + 1 of the task that holds the last slot of the previous trip
            for (uint32_t c0 = 0; c0 < tot; c0 += 64u * NN_DEAL_K) {
                SF_PHC(pc, 10, 1u);
                // which task holds each slot: its lane + 1 marked at the slot where its range starts (ranges that are not
                // empty start at distinct slots), then a running max over the slots
                for (int i = lane; i < 16 * NN_DEAL_K; i += 64) reinterpret_cast<uint32_t *>(ws->mark)[i] = 0u;
                __builtin_amdgcn_wave_barrier();
                if (len != 0u && off - c0 < 64u * NN_DEAL_K && off >= c0) ws->mark[off - c0] = (uint8_t)(lane + 1);
                wave_sync();
                uint32_t src[NN_DEAL_K];
#pragma unroll
                for (int k = 0; k < NN_DEAL_K; ++k) src[k] = wave_incl_scan<true>((uint32_t)ws->mark[64 * k + lane]);
#pragma unroll
                for (int k = 0; k < NN_DEAL_K; ++k) {
                    src[k] = max(src[k], carry);
                    carry = (uint32_t)__builtin_amdgcn_readlane((int)src[k], 63);
                }
                wave_sync(); // the marks are read before the next trip clears them
                SF_PHC(pc, 12, (unsigned)__popcll(__ballot(c0 + (uint32_t)lane < tot)));
                // every slot's load goes out before any is folded in (the folds are LDS atomics: the compiler does not move
                // a load across them)
                uint32_t j[NN_DEAL_K];
                int ow[NN_DEAL_K];
                float4 p[NN_DEAL_K], Q[NN_DEAL_K];
                unsigned long long cur[NN_DEAL_K];
#pragma unroll
                for (int k = 0; k < NN_DEAL_K; ++k) {
                    const uint32_t s = c0 + 64u * (uint32_t)k + (uint32_t)lane;
                    const int from = (int)((src[k] - 1u) & 63u) << 2; // slots past the end read some task: nothing is done with it
                    j[k] = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)base) + s;
                    ow[k] = __builtin_amdgcn_ds_bpermute(from, owner);
                    p[k] = load_point(g, j[k], s < tot);
                }
#pragma unroll
                for (int k = 0; k < NN_DEAL_K; ++k) {
                    Q[k] = ws->q[ow[k]];
                    cur[k] = __atomic_load_n(&ws->best[ow[k]], __ATOMIC_RELAXED);
                }
                // fold each candidate into its owner: whichever of (the owner's best, the candidate) loses is a runner-up,
                // the best itself met again is neither taken nor counted -- the rule of consider(), so the runner-up bound
                // comes out the same whatever order the candidates are met in
#pragma unroll
                for (int k = 0; k < NN_DEAL_K; ++k) {
                    const bool live = c0 + 64u * (uint32_t)k + (uint32_t)lane < tot;
                    const float d2 = l2_simple(Q[k].x, Q[k].y, Q[k].z, p[k].x, p[k].y, p[k].z);
                    const unsigned long long mine = pack_hit(d2, (int)j[k]);
                    if (live && mine != cur[k]) {
                        uint32_t lose = __float_as_uint(d2);
                        if (mine < cur[k]) {
                            const unsigned long long old = atomicMin(&ws->best[ow[k]], mine);
                            lose = (uint32_t)((old > mine ? old : mine) >> 32);
                        }
                        atomicMin(&ws->lb2[ow[k]], lose);
                    }
                }
            }
            wave_sync();
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    SF_PH(pc, 4);
#ifdef SF_PHASE_TRACE
    { unsigned m = lane_trips, c = lane_cands; for (int o = 32; o > 0; o >>= 1) { m += (unsigned)__shfl_xor((int)m, o); c += (unsigned)__shfl_xor((int)c, o); } SF_PHC(pc, 12, m); SF_PHC(pc, 13, c); }
#endif
    bool more = false; // ring 1 did not settle this query
    if (valid) {
        const unsigned long long m = ws->best[lane];
        const int j = (int)(uint32_t)m;
        hit.lb2 = __uint_as_float(ws->lb2[lane]);
        if (j != hit.j) { // a task found something better: fetch the winner's coordinates
            const float4 p = g.pts[j];
            hit.d2 = __uint_as_float((uint32_t)(m >> 32));
            hit.j = j;
            hit.px = p.x; hit.py = p.y; hit.pz = p.z;
        }
        // exactness of ring 1 (same test as nn_rings); otherwise on to ring 2
        const float gx = (qx - g.org[0]) * g.inv_h, gy = (qy - g.org[1]) * g.inv_h, gz = (qz - g.org[2]) * g.inv_h;
        const int cx = grid_cell(gx, nx), cy = grid_cell(gy, ny), cz = grid_cell(gz, nz);
        const float mface = block_face_gap(g, gx, gy, gz, cx, cy, cz, 1);
        const float mm = safe_gap(mface, g.gap_eps) * 0.999f;
        if (mface < 3.0e38f) {
            hit.lb2 = fminf(hit.lb2, mm * mm); // nothing outside the 27 cells is closer than their boundary
            more = !(hit.d2 <= mm * mm);
        }
        if (!COOP && more) { // lane by lane (the dense batch kernels: rare there, and the cooperative form below costs k_nn_red 8 VGPRs = one wave per SIMD)
            nn_rings<WINDOW>(g, w, qx, qy, qz, 2, hit);
            hit.lb2 = 0.0f; // no bound kept for the per-lane rings
        }
    }
    SF_PH(pc, 5);
    if (!COOP) return hit;
    // COOP: queries whose best is still farther than the boundary of their 27 cells (scan points with no map point nearby:
    // new ground, moving objects, the rim of the map crop) go on ring by ring TOGETHER.  Lane by lane that is a serial walk
    // of (2R+1)^2 rows by a handful of lanes while the rest of the wave idles -- measured on the per-scan path: it made
    // every index cell below the acceptance radius slower than a 0.72 m cell (alignment 409 us at 0.72 m; 557 / 498 us at
    // 0.5 / 0.36 m lane by lane, 349 / 355 us with this).  Here the (query, row) pairs of ring R are dealt out over all 64
    // lanes like the ring-1 tasks: rows outside the previous block are scanned whole, rows inside it only in their two new
    // end cells, each pruned by its gap against the owner's best as it stands.  Same result as nn_rings: the lexicographic
    // minimum of (d2, j) over everything visited, and only ranges that cannot hold a better candidate are skipped.
    unsigned long long unres = __ballot(more);
    const int rcap = max(nx, max(ny, nz));
    for (int R = 2; unres != 0ull && R <= rcap; ++R) {
        {
            const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(unres >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)unres, 0u));
            if (more) {
                ws->task[rank] = (uint16_t)lane;
                ws->best[lane] = pack_hit(hit.d2, hit.j);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int side = 2 * R + 1, nrows = side * side, total = __popcll(unres) * nrows;
        const float h = g.h, ge = g.gap_eps;
        for (int idx = lane; idx < total; idx += 64) {
            const int u = idx / nrows, r = idx - u * nrows;
            const int owner = (int)ws->task[u];
            const int dyi = r / side - R, dzi = r - (r / side) * side - R;
            const float4 Q = ws->q[owner];
            const float gx = (Q.x - g.org[0]) * g.inv_h, gy = (Q.y - g.org[1]) * g.inv_h, gz = (Q.z - g.org[2]) * g.inv_h;
            const int cx = grid_cell(gx, nx), cy = grid_cell(gy, ny), cz = grid_cell(gz, nz);
            const int y = cy + dyi, z = cz + dzi;
            if ((unsigned)y >= (unsigned)ny || (unsigned)z >= (unsigned)nz) continue;
            const float ry = safe_gap(cell_gap(gy, y, cy) * h, ge), rz = safe_gap(cell_gap(gz, z, cz) * h, ge);
            const float g2 = ry * ry + rz * rz;
            const unsigned long long start = __atomic_load_n(&ws->best[owner], __ATOMIC_RELAXED);
            const float cur = __uint_as_float((uint32_t)(start >> 32));
            if (g2 * 0.998f >= cur) continue;
            NNHit t;
            t.d2 = cur;
            t.j = (int)(uint32_t)start;
            t.px = t.py = t.pz = 0.0f;
            t.lb2 = 0.0f;
            const size_t row = ((size_t)z * ny + y) * nx;
            const bool inner = abs(dyi) < R && abs(dzi) < R; // scanned up to x +- (R - 1) by the rings before
            if (!inner) {
                const int x0 = max(cx - R, 0), x1 = min(cx + R, nx - 1);
                scan_range<WINDOW>(g, w, g.cell_start[row + x0], g.cell_start[row + x1 + 1], Q.x, Q.y, Q.z, t);
            } else {
                if (cx - R >= 0) {
                    const float gl = safe_gap((gx - (float)(cx - R + 1)) * h, ge);
                    if ((g2 + gl * gl) * 0.998f < t.d2) scan_range<WINDOW>(g, w, g.cell_start[row + cx - R], g.cell_start[row + cx - R + 1], Q.x, Q.y, Q.z, t);
                }
                if (cx + R <= nx - 1) {
                    const float gr = safe_gap(((float)(cx + R) - gx) * h, ge);
                    if ((g2 + gr * gr) * 0.998f < t.d2) scan_range<WINDOW>(g, w, g.cell_start[row + cx + R], g.cell_start[row + cx + R + 1], Q.x, Q.y, Q.z, t);
                }
            }
            const unsigned long long mine = pack_hit(t.d2, t.j);
            if (mine != start) atomicMin(&ws->best[owner], mine);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (more) {
            const unsigned long long m = ws->best[lane];
            const int j = (int)(uint32_t)m;
            if (j != hit.j) {
                const float4 p = g.pts[j];
                hit.d2 = __uint_as_float((uint32_t)(m >> 32));
                hit.j = j;
                hit.px = p.x; hit.py = p.y; hit.pz = p.z;
            }
            hit.lb2 = 0.0f; // no runner-up bound is kept beyond ring 1
            const float gx = (qx - g.org[0]) * g.inv_h, gy = (qy - g.org[1]) * g.inv_h, gz = (qz - g.org[2]) * g.inv_h;
            const int cx = grid_cell(gx, nx), cy = grid_cell(gy, ny), cz = grid_cell(gz, nz);
            const float mface = block_face_gap(g, gx, gy, gz, cx, cy, cz, R);
            const float mm = safe_gap(mface, ge) * 0.999f;
            more = mface < 3.0e38f && !(hit.d2 <= mm * mm);
        }
        unres = __ballot(more);
    }
    return hit;
}

// ------------------------------------------------------------------ re-search from the map's own neighbour table
// The map does not move: a query whose cached neighbour p no longer certifies almost always ends at p again or at one
// of p's own nearest map points.  Entry jc of the table (sf_map_build_neighbour_table) lists the up to 7 map points
// nearest to p and a radius r with |x - p| >= r for every map point x that is neither p nor listed.  The candidates are p
// and the listed points; the winner is the lexicographic minimum of (d2, j) among them, as in every search form.
// Served iff (|q - p| + |q - best|) * 1.0001 + 2e-6 < r.  Then for every x outside the candidate set
// |x - q| >= |x - p| - |q - p| >= r - |q - p| > |q - best| (triangle inequality), so the full search cannot prefer x, ties
// included: the result is nn_search_wave's, bit for bit.  Margins: q, p, x are float32 values and l2_simple of two of them
// is within 4 ulp of the real squared distance, its square root within 2.5e-7 relative; 1e-4 relative + 2e-6 absolute on
// the left covers both distances of the sum and the one comparison of float32 d2 values the search itself would make.
// The runner-up bound of a served query: the second smallest candidate distance and r - |q - p|, both rounded down -- and
// the best candidate's own distance too when it is not under the threshold (no neighbour: the bound then covers every point).
// Early end: with five or more listed, the rule is first tried on p and the first four with r4 = |x4 - p| * 0.9999 in place of r
// (everything else is at least that far from p, by the key order of the list); it serves the same queries -- r4 <= r and the
// winner is proven among the five -- with a bound from r4.
// Pure: no LDS, no wave cooperation; the lane either takes the result or searches as before with its seed unchanged.
//
// Stage 0, the nearest gap: behind the n entries lies one float per point, g1 = |x1 - p| * 0.9999 for the first listed point
// x1 (the nearest other point of p; the cap when nothing is listed, 0 for a coincident twin).  A lane with
// (|q - p| + |q - p|) * 1.0001 + 2e-6 < g1 is settled from that one 4-byte gather: it is the served rule above with best = p
// and g1 in place of r.  Every other map point x has |x - p| >= g1 (the list is in key order), so
// |x - q| >= |x - p| - |q - p| >= g1 - |q - p| > |q - p|: p is the exact nearest, ties excluded, and g1 - |q - p| bounds the
// runner-up.  It serves nothing the table would not: the listed points are farther from q than p by the same inequality (the
// margins cover the roundings as above), so the table's winner is p too, and g1 <= r4 <= r under the same roundings -- sqrtf is
// monotone over the key order of the list, and a listed distance is under the cap -- so the table's rule holds with either
// radius.  The result is the table's for the winner p (index, d2, the "nothing within the acceptance radius" form); only the
// bound is the looser g1 - |q - p|.  A lane that fails it takes the look-up below unchanged.
constexpr uint32_t NBR_NONE = 0xffffffffu;
constexpr int NBR_K = 7;
constexpr int NBR_BY_GAP = 1, NBR_BY_TABLE = 2; // what nn_research_table returns for a served query (0: not served)

// the nearest-gap array of a table of g.n entries: behind the entries, in the same allocation (SfGrid does not grow)
__device__ __forceinline__ const float *nbr_gap(const SfGrid &g) { return reinterpret_cast<const float *>(g.nbr + 2 * (size_t)g.n); }

__device__ __forceinline__ void nbr_fold(const float4 &p, uint32_t id, float qx, float qy, float qz, unsigned long long &best, float4 &bp, float &second)
{
    const float d2 = l2_simple(qx, qy, qz, p.x, p.y, p.z);
    const unsigned long long key = hit_key(d2, (int)id);
    const bool valid = id != NBR_NONE;
    const bool take = valid && key < best;
    // whichever of (the best so far, this candidate) loses is a runner-up
    const float lose = take ? __uint_as_float((uint32_t)(best >> 32)) : (valid ? d2 : 3.0e38f);
    second = fminf(second, lose);
    if (take) { best = key; bp = p; }
}

// what a served look-up returns: best = (d2b, j, bp) is the winner, lb bounds every other point from below
__device__ __forceinline__ void nbr_result(float d2b, int j, const float4 &bp, float lb, float thr, NNHit &out)
{
    // nothing under the threshold: the entry will say "no neighbour", and for such an entry the bound speaks of EVERY map
    // point (reuse_certificate: "still nothing within the acceptance radius") -- the best candidate itself comes under it, as
    // the would-be best of a search that found nothing enters its runner-up bound
    if (!(d2b < thr)) lb = fminf(lb, sqrtf(d2b) * 0.9999f);
    const float l2 = lb * lb;
    out.lb2 = l2 > 0.0f ? __uint_as_float(__float_as_uint(l2) - 1u) : 0.0f; // one step below the rounded square
    if (d2b < thr) {
        out.d2 = d2b; out.j = j; out.px = bp.x; out.py = bp.y; out.pz = bp.z;
    } else { // nothing within the acceptance radius: what a search that found nothing returns
        out.d2 = search_start(thr); out.j = -1; out.px = out.py = out.pz = 0.0f;
    }
}

// seed: the cached neighbour (seed.j >= 0) with its current squared distance, as reuse_certificate leaves it
// -> 0: not served; NBR_BY_GAP / NBR_BY_TABLE: served, by which stage
__device__ __forceinline__ int nn_research_table(const SfGrid &g, float qx, float qy, float qz, float thr, const NNHit &seed, NNHit &out)
{
    const float dp = sqrtf(seed.d2);
    { // stage 0 (g1 is dead before the entry is loaded)
        const float g1 = nbr_gap(g)[seed.j];
        if ((dp + dp) * 1.0001f + 2.0e-6f < g1) {
            nbr_result(seed.d2, seed.j, make_float4(seed.px, seed.py, seed.pz, 0.0f), fmaxf(g1 - dp * 1.0001f - 1.0e-6f, 0.0f), thr, out);
            return NBR_BY_GAP;
        }
    }
    const uint4 e0 = g.nbr[2 * (size_t)seed.j], e1 = g.nbr[2 * (size_t)seed.j + 1];
    const float r = __uint_as_float(e1.w);
    unsigned long long best = hit_key(seed.d2, seed.j);
    float4 bp = make_float4(seed.px, seed.py, seed.pz, 0.0f);
    float second = 3.0e38f;
    float rr = r;
    bool rest = e1.x != NBR_NONE; // (key order: no fifth, no sixth or seventh)
    { // two batches (4 + 3): at most four candidates' coordinates live at a time
        const float4 p0 = load_point(g, e0.x, e0.x != NBR_NONE), p1 = load_point(g, e0.y, e0.y != NBR_NONE), p2 = load_point(g, e0.z, e0.z != NBR_NONE),
                     p3 = load_point(g, e0.w, e0.w != NBR_NONE);
        nbr_fold(p0, e0.x, qx, qy, qz, best, bp, second);
        nbr_fold(p1, e0.y, qx, qy, qz, best, bp, second);
        nbr_fold(p2, e0.z, qx, qy, qz, best, bp, second);
        nbr_fold(p3, e0.w, qx, qy, qz, best, bp, second);
        if (rest) {
            // the list is in key order, so the fourth point's distance from p bounds the fifth to seventh and everything
            // unlisted exactly as r bounds the unlisted: when the rule holds with it, the second batch cannot change the
            // winner and is not loaded (most lanes: 6 gathers instead of 9; the look-up is bound by gathers per lane)
            const float r4 = sqrtf(l2_simple(seed.px, seed.py, seed.pz, p3.x, p3.y, p3.z)) * 0.9999f;
            if ((dp + sqrtf(__uint_as_float((uint32_t)(best >> 32)))) * 1.0001f + 2.0e-6f < r4) { rr = r4; rest = false; }
        }
    }
    if (rest) {
        const float4 p4 = load_point(g, e1.x, true), p5 = load_point(g, e1.y, e1.y != NBR_NONE), p6 = load_point(g, e1.z, e1.z != NBR_NONE);
        nbr_fold(p4, e1.x, qx, qy, qz, best, bp, second);
        nbr_fold(p5, e1.y, qx, qy, qz, best, bp, second);
        nbr_fold(p6, e1.z, qx, qy, qz, best, bp, second);
    }
    const float d2b = __uint_as_float((uint32_t)(best >> 32));
    if (!((dp + sqrtf(d2b)) * 1.0001f + 2.0e-6f < rr)) return 0;
    nbr_result(d2b, (int)(uint32_t)best, bp, fmaxf(fminf(sqrtf(second) * 0.9999f, rr - dp * 1.0001f - 1.0e-6f), 0.0f), thr, out);
    return NBR_BY_TABLE;
}

} // namespace sf
