// host_math.h -- the two rounding helpers of the host sources (no HIP, no context): OpenCV's cvRound and a round-up to a multiple.
// plan.cpp and host_logic.cpp keep bare-lrint copies of cv_round of their own: it has not been shown that the overflow guard
// below cannot fire for their arguments (scale factors and box coordinates that come from the caller), so their results stay as they are.
#pragma once
#include <climits>
#include <cmath>
#include <cstddef>

namespace nvca {

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline int cv_round(double v)
{
    if (!(v > -2147483648.5 && v < 2147483647.5)) return INT_MIN;   // _mm_cvtsd_si32 on overflow / inf
    return (int)lrint(v);
}

} // namespace nvca
