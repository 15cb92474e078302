// sf_keypoint.hpp — the shapes of the ISS keypoint kernels and of the descriptor gather of sf_keypoint.hip (gfx950).
#pragma once
#include "sf_feature.hpp"

namespace sf {

constexpr int ISS_BLOCK = 256;    // both walks: one lane per sorted position, everything in registers
constexpr int GATHER_BLOCK = 256; // k_features_gather: one word of a row per lane, consecutive lanes consecutive words

// what k_iss_saliency leaves per SORTED position for k_iss_nms: lambda3 of a salient point, ISS_NOT_SALIENT otherwise.  A salient
// point has lambda3 > min_lambda3 >= 0, so the one value carries lambda3 and the salient bit: a point that is not salient loses
// every comparison and never ties.
constexpr double ISS_NOT_SALIENT = -1.0;

} // namespace sf
