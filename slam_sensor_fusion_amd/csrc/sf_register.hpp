// sf_register.hpp — the shapes of the pose-from-matches kernels of sf_register.hip (gfx950).
#pragma once
#include <algorithm>
#include <cmath>

#include "sf_common.hpp"

namespace sf {

constexpr int REG_MAX_H = 1 << 20;       // hypotheses per call: h shares a 64-bit key with its count (k_reg_round)
constexpr int REG_MAX_TOP = 64;          // candidates returned at most
constexpr int REG_MAX_ROUNDS = 8;        // refit rounds at most
constexpr int REG_BLOCK = 256;           // one hypothesis (k_reg_hypotheses, k_reg_score) or one pair (the rest) per lane
constexpr int REG_REC = 16;              // the refit record: n, sum s' (3), sum t' (3), sum s' t'^T (9)
constexpr int REG_MOM_BLOCKS = 256;      // rows of partial records at most: one per lane of k_reg_refit
constexpr int REG_MIN_CHUNK = 64;        // k_reg_score: a slice of the pairs holds at least this many

// pairs per slice of k_reg_score under the test hook (asked > 0: its choice, otherwise one slice); at most 65535 slices, so that the
// hook's columns x slices stay a valid grid
inline int64_t reg_pair_chunk(int64_t m, int64_t asked)
{
    const int64_t want = asked > 0 ? asked : std::max<int64_t>(m, 1);
    return std::max<int64_t>(want, div_up(std::max<int64_t>(m, 1), 65535));
}

} // namespace sf
