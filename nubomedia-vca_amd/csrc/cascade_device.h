// cascade_device.h -- device-only helpers shared by more than one of the cascade kernel files (kernels_cascade_gather.hip,
// kernels_cascade_tile.hip, kernels_cascade_deep.hip): the upright stump's vote from the sum plane and the closed form of
// OpenCV's adaptive x step.  A helper with callers in one file only lives in that file.
#pragma once
#include "launch.h"

#if defined(__HIPCC__)
namespace nvca {

// Wave-uniform table records are read through the constant address space: the compiler then issues scalar loads
// (s_load) for them even though the kernels also store to global memory.  The tables are never written by a kernel.
typedef const __attribute__((address_space(4))) TStumpRec CTStumpRec;

__device__ __forceinline__ int ldsum(const int *__restrict__ sum, unsigned idx) { return sum[idx]; }

// feature value of one stump on one window (v) against its threshold: returns the vote.  Records hold corner columns /
// rows relative to the window (geometry-independent tables); the plane offset is row * pitch + column.
template <bool PAIR, class Rec, bool UNI = false>
__device__ __forceinline__ double stump_vote(const int *__restrict__ sum, unsigned off, int pitch, double vnf, Rec &f)
{
    auto rs = [&](int q) {
        const unsigned r0 = off + (unsigned)(f.y0[q] * pitch), r1 = off + (unsigned)(f.y1[q] * pitch);
        return ldsum(sum, r0 + (unsigned)f.x0[q]) - ldsum(sum, r0 + (unsigned)f.x1[q]) - ldsum(sum, r1 + (unsigned)f.x0[q]) +
               ldsum(sum, r1 + (unsigned)f.x1[q]);
    };
    const int s0 = rs(0);
    const int s1 = rs(1);
    const double t = f.thr * vnf;                       // node->threshold * variance_norm_factor
    double v;
    if (PAIR) {
        const float fs = (float)s0 * f.w[0] + (float)s1 * f.w[1];     // SSE2 path: f32 add
        v = (double)fs;
    } else {
        v = (double)((float)s0 * f.w[0]);
        v += (double)((float)s1 * f.w[1]);
        if ((f.nrect & 255) == 3) {
            const int s2 = rs(2);
            v += (double)((float)s2 * f.w[2]);
        }
    }
    double a0 = f.a0, a1 = f.a1;
    if (UNI) asm("" : "+s"(a0), "+s"(a1));      // wave-uniform record: both votes stay in scalar registers
    return v >= t ? a1 : a0;
}

// visited by OpenCV's adaptive scan?  row_bits: the row's stage-0 reject words
__device__ __forceinline__ bool visited(const unsigned long long *__restrict__ row_bits, int ix)
{
    int d = 0, pos = ix;
    while (pos > 0) {
        const int p = pos - 1, b = p & 63;
        const unsigned long long m = row_bits[p >> 6] << (63 - b);       // bit p at the MSB
        const int ones = (~m == 0ull) ? 64 : __clzll((long long)~m);
        const int lim = b + 1;
        d += ones < lim ? ones : lim;
        if (ones < lim) break;
        pos -= lim;
    }
    return !(d & 1);
}

} // namespace nvca
#endif
