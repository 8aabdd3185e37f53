// yuv_device.h -- device-only arithmetic of the 4:2:0 sources (and, at the end, the fetches of the packed 4:2:2 ones), shared by every kernel that reads NV12 / I420 planes
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

// ---- packed 4:2:2 sources (FMT: NVCA_PIX_YUY2 / _UYVY / _YVYU).  The arithmetic is the one above; what is new is where Y, U
// and V are fetched from (yuv422_pos, pixel_rules.h).  YuvPlanes::off_y is the plane's offset; nothing else of it is read.
// one pixel pair as a little-endian word of its four bytes: the pair's chroma term and the luma of pixel j (0 / 1)
template <int FMT>
__device__ __forceinline__ ChromaTerm chroma_of_pair(unsigned w)
{
    constexpr Yuv422Pos q = yuv422_pos(FMT);
    return chroma_term((w >> (8 * q.u)) & 255, (w >> (8 * q.v)) & 255);
}
template <int FMT>
__device__ __forceinline__ int luma_of_pair(unsigned w, int j)
{
    constexpr Yuv422Pos q = yuv422_pos(FMT);
    return (w >> (8 * (q.y0 + 2 * j))) & 255;
}
// pixel (r, c) of a frame, byte reads (any alignment): its luma and the chroma term of its pair
template <int FMT>
__device__ __forceinline__ int yuv422_at(const uint8_t *__restrict__ src, const YuvPlanes &p, int sstride, int r, int c, ChromaTerm &ct)
{
    constexpr Yuv422Pos q = yuv422_pos(FMT);
    const uint8_t *pair = src + p.off_y + (size_t)r * sstride + 4 * (size_t)(c >> 1);
    ct = chroma_term(pair[q.u], pair[q.v]);
    return pair[q.y0 + 2 * (c & 1)];
}

} // namespace nvca
#endif
