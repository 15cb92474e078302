// sf_feature.hpp — the descriptor set and the shapes of the FPFH and matching kernels of sf_feature.hip (gfx950).
#pragma once
#include <algorithm>
#include <cmath>

#include "sf_common.hpp"

// n rows of SF_FPFH_DIM float32 and a validity byte per row, original point order of whatever produced them
struct sf_features {
    sf_ctx *ctx = nullptr;
    sf::DevBuf rows, valid; // float[n][33], uint8[n] (0 / 1)
    int64_t n = 0, n_valid = 0;
};

namespace sf {

constexpr int FPFH_BINS = 11;                  // per angle; a row is theta | alpha | phi
constexpr int FPFH_BLOCK = 128;                // pass 1: 33 LDS counters per lane, 16.5 KiB a block
constexpr int MATCH_BLOCK = 256;               // one query row per lane, held in registers
constexpr int MATCH_TILE = 64;                 // candidate rows staged in LDS at a time (8.25 KiB + their flags)
constexpr int MATCH_MAX_SLICES = 64;           // the candidates are split over at most this many grid slices ...
constexpr int MATCH_MIN_SLICE = 4 * MATCH_TILE; // ... of at least this many rows, a whole number of tiles each

// rows of one slice when n_dst candidates are split (a multiple of MATCH_TILE)
inline int64_t match_slice_rows(int64_t n_dst)
{
    const int64_t per = div_up(std::max<int64_t>(n_dst, 1), MATCH_MAX_SLICES);
    return std::max<int64_t>(MATCH_MIN_SLICE, div_up(per, MATCH_TILE) * MATCH_TILE);
}

// The reach of radius_walk (sf_walk.hpp, (c)), in float64, capped by the grid before the conversion: the expression of
// sf_map.hip's radius_reach, which that translation unit keeps to itself.
inline int feature_reach(const SfGrid &g, float r2)
{
    const double reach = std::ceil((std::sqrt((double)r2) * (1.0 + 1.0e-6) + (double)g.gap_eps) * (double)g.inv_h);
    return (int)std::min(std::max(reach, 1.0), (double)std::max(g.dim[0], std::max(g.dim[1], g.dim[2])));
}

} // namespace sf
