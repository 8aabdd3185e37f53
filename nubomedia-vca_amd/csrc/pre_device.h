// pre_device.h -- device-only helpers shared by more than one of the pre-processing kernel files (kernels_gray.hip,
// kernels_equalize.hip): the row count of their blocks and the histogram flush.  A helper with callers in one file only lives in
// that file.
#pragma once
#include "launch.h"

#if defined(__HIPCC__)
namespace nvca {

static constexpr int kGrayRows = 8;        // rows per block in the gray kernels

__device__ __forceinline__ void hist_flush(unsigned (*lh)[256], unsigned *hist, int tid)
{
    __syncthreads();
    unsigned v = lh[0][tid] + lh[1][tid] + lh[2][tid] + lh[3][tid];
    if (v) atomicAdd(&hist[tid], v);
}

} // namespace nvca
#endif
