// sf_walk.hpp — the two lane-per-point walks over the block of cells around a point of the uniform-grid map index (device side,
// gfx950): radius_walk, trimmed by the gaps against a float32 radius rule (the radius filter, clustering), box_rows over a
// ball_box, trimmed per axis against the float64 rule of the normals and their carry marks, and block_rows, untrimmed (the
// neighbour table).  The geometry they rest on is sf_nn.hpp's.
#pragma once
#include "sf_nn.hpp"

namespace sf {

// visit(a, b) for the cell_start run [a, b) of every (z, y) row of the block of radius R around cell (cx, cy, cz): z-major, then
// y, one contiguous x-run per row.  The cell is one of the grid: the bounds of the x-run are read before any test.
template <class F>
__device__ __forceinline__ void block_rows(const SfGrid &g, int cx, int cy, int cz, int R, F visit)
{
    const int nx = g.dim[0], ny = g.dim[1], nz = g.dim[2];
    const int x0 = max(cx - R, 0), x1 = min(cx + R, nx - 1);
    const int y0 = max(cy - R, 0), y1 = min(cy + R, ny - 1);
    const int z0 = max(cz - R, 0), z1 = min(cz + R, nz - 1);
    for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y) {
            const size_t row = ((size_t)z * ny + y) * nx;
            visit(g.cell_start[row + x0], g.cell_start[row + x1 + 1]);
        }
}

// block_rows for the float64 rule of the normals and their carry marks, ex^2 + ey^2 + ez^2 <= r2d on the exact differences of the
// float32 coordinates: the box of cells within R of the position's cell, less on every axis and side the outermost layer of cells
// where it holds nothing the rule accepts.  ball_box decides that once per position (six comparisons, no loop), box_rows walks the
// box as block_rows walks its block (the same rows in the same order, nothing computed per row), so every float64 sum over the
// accepted points keeps its order and its bits whatever R is, as long as R reaches them all.  (gx, gy, gz) are the grid
// coordinates G of the position, (cx, cy, cz) its cell, which may lie beyond the grid on the upper side (k_normals_mark): an axis
// whose range comes out empty makes box_rows visit nothing, before any bound is read.
// The argument, in the terms of (a) - (c) of radius_walk below.  (a) holds exactly here: per axis |p - q| <= r, the differences
// being exact in float64.  (c) gives R = ceil((r (1 + 1e-6) + gap_eps) inv_h), normals_walk of the host.  The trim: f = G(p) - c
// is exact in float32 (c = floor(G(p)), or the clamp of it).  A point q of a cell <= c - R has G(q) < c - R + 1, so
// G(p) - G(q) > f + R - 1; one of a cell >= c + R has G(q) >= c + R (the clamped last cell too), so G(q) - G(p) >= R - f.  By (b)
// |p - q| inv_h >= |G(p) - G(q)| - S, so with trim = (r (1 + 1e-6) + gap_eps) inv_h - (R - 1), rounded up by the host -- the
// expression under the ceil of R less R - 1, hence in (0, 1] --, the lower layer holds no neighbour when f >= trim and the upper
// one when fl(1 - f) >= trim: gap_eps inv_h exceeds S by 2^-23 maxdim, more than the one rounding of 1 - f.  No layer nearer than
// R can ever be left out (its gap is below R - 1 <= r inv_h cells), so one comparison per side is all a loop could do.  At a
// radius of exactly one cell R = 2 and trim = 1e-6 + gap_eps inv_h: the walk stays the 27 cells it was with the reach
// ceil(radius / h), except within that margin of a face.  The margin is kept that small because a lane that keeps a layer makes
// its whole wave wait for it: with 1e-3 in place of 1e-6 the launch was 6 % slower.  (Per-row skips and x-trims as in radius_walk,
// and the same per-axis trim through trim_left / trim_right loops, were measured as well: profiles/normals_reach_ab.txt.)
struct BallBox { int xa, xb, ya, yb, za, zb; };
__device__ __forceinline__ BallBox ball_box(const SfGrid &g, float gx, float gy, float gz, int cx, int cy, int cz, int R, float trim)
{
    const float fx = gx - (float)cx, fy = gy - (float)cy, fz = gz - (float)cz;
    BallBox b;
    b.xa = max(cx - R + (fx >= trim ? 1 : 0), 0);
    b.xb = min(cx + R - (1.0f - fx >= trim ? 1 : 0), g.dim[0] - 1);
    b.ya = max(cy - R + (fy >= trim ? 1 : 0), 0);
    b.yb = min(cy + R - (1.0f - fy >= trim ? 1 : 0), g.dim[1] - 1);
    b.za = max(cz - R + (fz >= trim ? 1 : 0), 0);
    b.zb = min(cz + R - (1.0f - fz >= trim ? 1 : 0), g.dim[2] - 1);
    return b;
}
template <class F>
__device__ __forceinline__ void box_rows(const SfGrid &g, const BallBox &b, F visit)
{
    if (b.xa > b.xb) return;
    const int nx = g.dim[0], ny = g.dim[1];
    for (int z = b.za; z <= b.zb; ++z)
        for (int y = b.ya; y <= b.yb; ++y) {
            const size_t row = ((size_t)z * ny + y) * nx;
            visit(g.cell_start[row + b.xa], g.cell_start[row + b.xb + 1]);
        }
}

// visit(k, aux[k], accepted) for the candidates at sorted positions k, accepted = l2_simple(p, pts[k]) < r2 (float32, unfused,
// strict; p itself included when it is indexed) -- and, with accepted = false, for the empty slots of a trip of four.  The flag is
// an argument and not a branch around the call, so that a visitor which only counts stays free of branches (a branch per
// candidate cost k_radius_count 12 %).  The walk: the block of cells within R of p's own cell row by row, each row one contiguous
// cell_start run, four loads in flight (scan4 of sf_nn.hpp).  R is radius_reach(g, r2) of the host.
// END: only positions k < end.  Rows lie in memory in the order they are walked, so the first row that starts at or beyond `end`
// ends the walk.  AUX: aux[k] is loaded beside the point, four in flight as well, instead of behind the comparison.
//
// Nothing the rule accepts is lost.  Write G(x) = fl(fl(x - org) * inv_h) for the grid coordinate every point is binned by
// (k_cell_keys; the cell is grid_cell(G)), u = 2^-24, and let q be accepted for p.
// (a) Per axis |p - q| < r (1 + 2u), r = sqrt(r2): rounding is monotone, so the float sum of non-negative terms is at least each
//     term, fl(d2) >= fl(fl(dx)^2) >= dx^2 (1 - u)^3, and fl(d2) < r2.  (A square that underflows belongs to |dx| < 2^-62 m.)
// (b) G(x) = (x - org) inv_h (1 + e1)(1 + e2), |e| <= u, and (x - org) inv_h < dim (1 + u) for every indexed point, so
//     |G(p) - G(q)| <= |p - q| inv_h + S with S = 2^-22 maxdim (1 + 3u) cells: S h is below gap_eps = 1.5 * 2^-22 maxdim h, the
//     slack SfGrid carries for exactly this.
// (c) Reach: floor(a) - floor(b) <= ceil(D) whenever a - b <= D, and the clamp only brings cells closer, so q's cell is within
//     R = ceil((r (1 + 1e-6) + gap_eps) inv_h) of p's on every axis (the host computes it in float64; 1e-6 covers (a) and its own
//     roundings).  normals_walk (sf_map.hip) takes the same expression for the float64 rule of ball_box: ceil(radius / h) alone is
//     one short when r is a whole number of cells and G(p), G(q) round to either side of two faces r apart.
// (d) Row skip and x-trim (trim_left / trim_right), the rule of knn_search with tau = r2: a point binned in cell c != cq has G on
//     the far side of the face between, so by (b) its true axis distance from p is at least safe_gap(cell_gap * h, gap_eps), up to
//     the relative roundings of forming it (a few u).  A row or an end cell is left out only when the sum g2 of those squared gaps
//     has g2 * 0.998 >= r2; then dy^2 + dz^2 (+ dx^2) >= g2 (1 - 8u) and fl(d2) >= that (1 - 5u) >= r2 / 0.998 * (1 - 13u) > r2:
//     rejected by the rule itself.
// DETAIL: visit(k, aux[k], accepted, d2, q) instead, with the float32 d2 that was compared and the candidate q (its id in q.w), for
// the callers that hand the neighbours out (sf_radius.hpp); for an empty slot of a trip only accepted = false means anything (q is
// zeros and d2 the distance to them).  The default is the walk as it was,
// token for token: the choice is made while compiling.
template <bool AUX, bool END, bool DETAIL = false, class F>
__device__ __forceinline__ void radius_walk(const SfGrid &g, const float4 p, float r2, int R, uint32_t end, const int32_t *__restrict__ aux, F visit)
{
    const int nx = g.dim[0], ny = g.dim[1], nz = g.dim[2];
    const float gx = (p.x - g.org[0]) * g.inv_h, gy = (p.y - g.org[1]) * g.inv_h, gz = (p.z - g.org[2]) * g.inv_h;
    const int cx = grid_cell(gx, nx), cy = grid_cell(gy, ny), cz = grid_cell(gz, nz);
    const int x0 = max(cx - R, 0), x1 = min(cx + R, nx - 1);
    const int y0 = max(cy - R, 0), y1 = min(cy + R, ny - 1);
    const int z0 = max(cz - R, 0), z1 = min(cz + R, nz - 1);
    const float h = g.h, ge = g.gap_eps;
    for (int z = z0; z <= z1; ++z) {
        const float rz = safe_gap(cell_gap(gz, z, cz) * h, ge);
        if (!(rz * rz * 0.998f < r2)) continue;
        for (int y = y0; y <= y1; ++y) {
            const float ry = safe_gap(cell_gap(gy, y, cy) * h, ge);
            const float g2 = ry * ry + rz * rz;
            if (!(g2 * 0.998f < r2)) continue;
            const int xa = trim_left(g, gx, cx, x0, g2, r2), xb = trim_right(g, gx, cx, x1, g2, r2);
            const size_t row = ((size_t)z * ny + y) * nx;
            const uint32_t a = g.cell_start[row + xa];
            if (END && a >= end) return;
            const uint32_t b = END ? min(g.cell_start[row + xb + 1], end) : g.cell_start[row + xb + 1];
            for (uint32_t k = a; k < b; k += 4) {
                const float4 q0 = load_point(g, k, true), q1 = load_point(g, k + 1, k + 1 < b), q2 = load_point(g, k + 2, k + 2 < b), q3 = load_point(g, k + 3, k + 3 < b);
                const int32_t a0 = AUX ? aux[k] : 0, a1 = AUX ? aux[k + 1 < b ? k + 1 : k] : 0, a2 = AUX ? aux[k + 2 < b ? k + 2 : k] : 0,
                              a3 = AUX ? aux[k + 3 < b ? k + 3 : k] : 0;
                if constexpr (DETAIL) {
                    const float d0 = l2_simple(p.x, p.y, p.z, q0.x, q0.y, q0.z), d1 = l2_simple(p.x, p.y, p.z, q1.x, q1.y, q1.z),
                                d2 = l2_simple(p.x, p.y, p.z, q2.x, q2.y, q2.z), d3 = l2_simple(p.x, p.y, p.z, q3.x, q3.y, q3.z);
                    visit(k, a0, d0 < r2, d0, q0);
                    visit(k + 1, a1, k + 1 < b && d1 < r2, d1, q1);
                    visit(k + 2, a2, k + 2 < b && d2 < r2, d2, q2);
                    visit(k + 3, a3, k + 3 < b && d3 < r2, d3, q3);
                } else {
                    visit(k, a0, l2_simple(p.x, p.y, p.z, q0.x, q0.y, q0.z) < r2);
                    visit(k + 1, a1, k + 1 < b && l2_simple(p.x, p.y, p.z, q1.x, q1.y, q1.z) < r2);
                    visit(k + 2, a2, k + 2 < b && l2_simple(p.x, p.y, p.z, q2.x, q2.y, q2.z) < r2);
                    visit(k + 3, a3, k + 3 < b && l2_simple(p.x, p.y, p.z, q3.x, q3.y, q3.z) < r2);
                }
            }
        }
    }
}

// The rows of radius_walk alone: visit(a, b) for the x-run [a, b) of sorted positions of every row the walk above would enter, in
// its order, with its skips and trims -- for a caller that deals the candidates of a run over the lanes of a wave (the wave fill
// of sf_radius.hpp).  The same expressions on the same inputs, so the same runs: what one form visits the other does.
template <class F>
__device__ __forceinline__ void radius_runs(const SfGrid &g, const float4 p, float r2, int R, F visit)
{
    const int nx = g.dim[0], ny = g.dim[1], nz = g.dim[2];
    const float gx = (p.x - g.org[0]) * g.inv_h, gy = (p.y - g.org[1]) * g.inv_h, gz = (p.z - g.org[2]) * g.inv_h;
    const int cx = grid_cell(gx, nx), cy = grid_cell(gy, ny), cz = grid_cell(gz, nz);
    const int x0 = max(cx - R, 0), x1 = min(cx + R, nx - 1);
    const int y0 = max(cy - R, 0), y1 = min(cy + R, ny - 1);
    const int z0 = max(cz - R, 0), z1 = min(cz + R, nz - 1);
    const float h = g.h, ge = g.gap_eps;
    for (int z = z0; z <= z1; ++z) {
        const float rz = safe_gap(cell_gap(gz, z, cz) * h, ge);
        if (!(rz * rz * 0.998f < r2)) continue;
        for (int y = y0; y <= y1; ++y) {
            const float ry = safe_gap(cell_gap(gy, y, cy) * h, ge);
            const float g2 = ry * ry + rz * rz;
            if (!(g2 * 0.998f < r2)) continue;
            const int xa = trim_left(g, gx, cx, x0, g2, r2), xb = trim_right(g, gx, cx, x1, g2, r2);
            const size_t row = ((size_t)z * ny + y) * nx;
            visit(g.cell_start[row + xa], g.cell_start[row + xb + 1]);
        }
    }
}

} // namespace sf
