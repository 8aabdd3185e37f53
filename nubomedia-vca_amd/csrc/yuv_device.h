// yuv_device.h -- device-only arithmetic of the 4:2:0 sources, shared by every kernel that reads NV12 / I420 planes
// (kernels_gray.hip: face streams, the part detectors' working images, nvca_yuv420_to_bgr; kernels_trk_pixel.hip: the tracker's pixel pass):
// cv::cvtColor(CV_YUV2BGR_NV12 / _I420) as OpenCV 2.4 color.cpp computes it, BT.601 limited range, shift 20 -- pixel
// (x, y) takes the chroma sample (x >> 1, y >> 1); all int32, the shift arithmetic -- and the BGR2GRAY / BGRA2GRAY that follows it.
#pragma once
#include "launch.h"

#if defined(__HIPCC__)
namespace nvca {

__device__ __forceinline__ int gray_of(int b, int g, int r)
{   // RGB2Gray<uchar>: B2Y 1868, G2Y 9617, R2Y 4899, shift 14, rounding 1<<13
    return (b * 1868 + g * 9617 + r * 4899 + 8192) >> 14;
}

// (ChromaTerm, chroma_term, sat8, yuv_bgr: pixel_rules.h -- the host loops of the 4:2:0 overlay share them)
__device__ __forceinline__ int yuv_gray(int Y, const ChromaTerm &c)
{
    int B, G, R;
    yuv_bgr(Y, c, B, G, R);
    return gray_of(B, G, R);
}
template <int FMT>
__device__ __forceinline__ ChromaTerm chroma_at(const uint8_t *__restrict__ src, const YuvPlanes &p, int cx, int cy)
{
    if (FMT == 1) { const uint8_t *c = src + p.off_u + (size_t)cy * p.cstride + 2 * cx; return chroma_term(c[0], c[1]); }
    return chroma_term(src[p.off_u + (size_t)cy * p.cstride + cx], src[p.off_v + (size_t)cy * p.vstride + cx]);
}

} // namespace nvca
#endif
