// yuv_layout.h -- the geometry of a 4:2:0 frame in a caller's layout (nvca_pixel_layout): plane p of a w x h frame has
// yuv_plane_rows() rows of yuv_plane_row_bytes() bytes.  Pure host arithmetic (no HIP header, no context): host_copy.cpp's layout rules
// and copies and the staging sizes of trk_host.cpp share it.
#pragma once
#include <algorithm>
#include <cstddef>
#include "../../include/nubovca.h"

namespace nvca {

inline int yuv_planes_of(const nvca_pixel_layout &l) { return l.format == NVCA_PIX_NV12 ? 2 : 3; }
inline size_t yuv_plane_rows(int p, int h) { return p == 0 ? (size_t)h : (size_t)h / 2; }
inline size_t yuv_plane_row_bytes(const nvca_pixel_layout &l, int p, int w) { return (p == 0 || l.format == NVCA_PIX_NV12) ? (size_t)w : (size_t)w / 2; }
inline size_t yuv_plane_bytes(const nvca_pixel_layout &l, int p, int w, int h)
{
    return (size_t)l.stride[p] * (yuv_plane_rows(p, h) - 1) + yuv_plane_row_bytes(l, p, w);
}
// bytes from the frame's base to the end of its last plane
inline size_t yuv_extent(const nvca_pixel_layout &l, int w, int h)
{
    size_t e = 0;
    for (int p = 0; p < yuv_planes_of(l); p++) e = std::max(e, l.offset[p] + yuv_plane_bytes(l, p, w, h));
    return e;
}

} // namespace nvca
