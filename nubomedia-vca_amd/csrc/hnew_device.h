// hnew_device.h -- the one piece of arithmetic that both evaluators of new-format HAAR cascades form per window (kernels_cascade_hnew.hip,
// kernels_roi_hnew.hip): HaarEvaluator::setWindow's varianceNormFactor.  Device code only.
#pragma once
#include "launch.h"

namespace nvca {

// 1 / nf of a window from the sums over its normrect: nf = area * valsq - valsum^2 (f64, no contraction: exact integer operands, one
// multiply-subtract pair), its correctly rounded root when positive, else 1
__device__ __forceinline__ double hnew_norm(double area, double valsq, int valsum)
{
    double nf = area * valsq - (double)valsum * (double)valsum;
    nf = nf > 0. ? sqrt(nf) : 1.;
    return 1. / nf;
}

} // namespace nvca
