// sf_walk.hpp — the two lane-per-point walks over the block of cells around a point of the uniform-grid map index (device side,
// gfx950): radius_walk, trimmed by the gaps against a float32 radius rule (the radius filter, clustering), and block_rows,
// untrimmed (the normals, their carry marks, the neighbour table).  The geometry they rest on is sf_nn.hpp's.
#pragma once
#include "sf_nn.hpp"

namespace sf {

// visit(a, b) for the cell_start run [a, b) of every (z, y) row of the block of radius R around cell (cx, cy, cz): z-major, then
// y, one contiguous x-run per row.  (cx, cy, cz) may lie outside the grid on the upper side (k_normals_mark); the caller then
// makes sure the x-run is not empty, because its bounds are read before any test.
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
//     roundings).  normals_reach's ceil(radius / h - 1e-9) is one short when r is a whole number of cells and p, q straddle it.
// (d) Row skip and x-trim (trim_left / trim_right), the rule of knn_search with tau = r2: a point binned in cell c != cq has G on
//     the far side of the face between, so by (b) its true axis distance from p is at least safe_gap(cell_gap * h, gap_eps), up to
//     the relative roundings of forming it (a few u).  A row or an end cell is left out only when the sum g2 of those squared gaps
//     has g2 * 0.998 >= r2; then dy^2 + dz^2 (+ dx^2) >= g2 (1 - 8u) and fl(d2) >= that (1 - 5u) >= r2 / 0.998 * (1 - 13u) > r2:
//     rejected by the rule itself.
template <bool AUX, bool END, class F>
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
                visit(k, a0, l2_simple(p.x, p.y, p.z, q0.x, q0.y, q0.z) < r2);
                visit(k + 1, a1, k + 1 < b && l2_simple(p.x, p.y, p.z, q1.x, q1.y, q1.z) < r2);
                visit(k + 2, a2, k + 2 < b && l2_simple(p.x, p.y, p.z, q2.x, q2.y, q2.z) < r2);
                visit(k + 3, a3, k + 3 < b && l2_simple(p.x, p.y, p.z, q3.x, q3.y, q3.z) < r2);
            }
        }
    }
}

} // namespace sf
