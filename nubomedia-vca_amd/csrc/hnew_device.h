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

// ---- shared by the two large-image evaluators (kernels_cascade_hnew.hip: stumps; kernels_cascade_hgen.hip: trees and tilted features)
// 1 / nf of the window whose origin lo / hi point at (the level's Q planes): nf = area * valsq - valsum^2, its root when positive, else 1
__device__ __forceinline__ double hnew_vnf(int valsum, const unsigned *__restrict__ lo, const uint8_t *__restrict__ hi, const int *nr, double area)
{
    const unsigned long long q0 = ((unsigned long long)hi[nr[0]] << 32) | lo[nr[0]], q1 = ((unsigned long long)hi[nr[1]] << 32) | lo[nr[1]];
    const unsigned long long q2 = ((unsigned long long)hi[nr[2]] << 32) | lo[nr[2]], q3 = ((unsigned long long)hi[nr[3]] << 32) | lo[nr[3]];
    const double valsq = (double)(long long)(q0 - q1 - q2 + q3);          // an integer below 2^40: exact
    return hnew_norm(area, valsq, valsum);
}

__device__ __forceinline__ int hnew_rect(const int *__restrict__ p, const int *off) { return p[off[0]] - p[off[1]] - p[off[2]] + p[off[3]]; }

} // namespace nvca
