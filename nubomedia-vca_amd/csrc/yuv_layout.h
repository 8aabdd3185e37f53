// yuv_layout.h -- the geometry of a 4:2:0 or packed 4:2:2 frame in a caller's layout (nvca_pixel_layout): plane p of a w x h frame has
// yuv_plane_rows() rows of yuv_plane_row_bytes() bytes; the one set of layout rules (yuv_layout_fault), layouts by value, the alignment
// the wide gray kernels want, and the pieces a sparse copy of a plane's rows is made of.  Pure host arithmetic (no HIP header, no
// context): host_copy.cpp's checks and copies and the staging sizes of trk_host.cpp share it.
#pragma once
#include <algorithm>
#include <cstddef>
#include "../../include/nubovca.h"

namespace nvca {

// packed 4:2:2 (NVCA_PIX_YUY2 / _UYVY / _YVYU): one plane of 2 bytes a pixel, every row with its own chroma (the byte order: pixel_rules.h, yuv422_pos)
inline bool yuv_is_422(int format) { return format == NVCA_PIX_YUY2 || format == NVCA_PIX_UYVY || format == NVCA_PIX_YVYU; }
inline bool yuv_is_420(int format) { return format == NVCA_PIX_NV12 || format == NVCA_PIX_I420; }
inline int yuv_planes_of(const nvca_pixel_layout &l) { return yuv_is_422(l.format) ? 1 : l.format == NVCA_PIX_NV12 ? 2 : 3; }
inline size_t yuv_plane_rows(int p, int h) { return p == 0 ? (size_t)h : (size_t)h / 2; }
inline size_t yuv_plane_row_bytes(const nvca_pixel_layout &l, int p, int w)
{
    if (yuv_is_422(l.format)) return 2 * (size_t)w;
    return (p == 0 || l.format == NVCA_PIX_NV12) ? (size_t)w : (size_t)w / 2;
}
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

// what is wrong with a w x h frame in this layout (null: nothing) -- the one set of layout rules, for the streams and for the
// calls that take a host frame without a context.  4:2:0: both sizes even (OpenCV asserts it); 4:2:2: the width even (a pixel pair
// shares one U, V), any height.
inline const char *yuv_layout_fault(const nvca_pixel_layout &l, int w, int h)
{
    const bool p422 = yuv_is_422(l.format);
    if (!p422 && !yuv_is_420(l.format)) return "pixel layout: format must be NVCA_PIX_BGR, NVCA_PIX_NV12, NVCA_PIX_I420, NVCA_PIX_YUY2, NVCA_PIX_UYVY or NVCA_PIX_YVYU";
    if (w <= 0 || h <= 0) return p422 ? "4:2:2 frame: width and height must be positive" : "4:2:0 frame: width and height must be positive";
    if (p422 && (w & 1)) return "4:2:2 frame: the width must be even (a pixel pair shares one U, V)";
    if (!p422 && ((w | h) & 1)) return "4:2:0 frame: width and height must be even (OpenCV's 4:2:0 conversions assert it)";
    const int np = yuv_planes_of(l);
    for (int p = 0; p < np; p++) {
        if (l.stride[p] <= 0 || (size_t)l.stride[p] < yuv_plane_row_bytes(l, p, w)) return p422 ? "4:2:2 frame: the stride is shorter than a row of 2 * width bytes" : "4:2:0 frame: a plane's stride is shorter than its row";
        if (l.offset[p] > ((size_t)1 << 40)) return p422 ? "4:2:2 frame: offset out of range" : "4:2:0 frame: plane offset out of range";
    }
    for (int p = 0; p < np; p++)
        for (int q = p + 1; q < np; q++) {
            const size_t a0 = l.offset[p], a1 = a0 + yuv_plane_bytes(l, p, w, h), b0 = l.offset[q], b1 = b0 + yuv_plane_bytes(l, q, w, h);
            if (a0 < b1 && b0 < a1) return "4:2:0 frame: planes overlap";
        }
    return nullptr;
}
inline bool same_layout(const nvca_pixel_layout &a, const nvca_pixel_layout &b)
{
    if (a.format != b.format) return false;
    for (int p = 0; p < 3; p++) if (a.offset[p] != b.offset[p] || a.stride[p] != b.stride[p]) return false;
    return true;
}
// frames of one layout: every plane and stride takes the wide gray kernel's loads -- k_gray_yuv16's (4:2:0) or k_gray_yuv422_16's (4:2:2:
// 16-byte loads of the one plane) -- given a base on 16 bytes (staged host frames start on 256 bytes)
inline bool yuv_layout_aligned16(const nvca_pixel_layout &l)
{
    if (yuv_is_422(l.format)) return !(l.offset[0] & 15) && !(l.stride[0] & 15);
    const bool nv12 = l.format == NVCA_PIX_NV12;
    const size_t cmask = nv12 ? 15 : 7;
    if ((l.offset[0] & 15) || (l.stride[0] & 15) || (l.offset[1] & cmask) || ((size_t)l.stride[1] & cmask)) return false;
    if (!nv12 && ((l.offset[2] & 7) || (l.stride[2] & 7))) return false;
    return true;
}

// Rows [first + k * period, + run), k < count, of an image plane (`rows` rows of `row_bytes` bytes, `stride` apart) as at most two 2-D
// copies between a buffer and its copy of the same geometry: `n` rows of `width` bytes from byte `off` on, `pitch` apart.  A run that
// ends on the plane's last row goes without the row padding (the buffer need not extend past the last pixel).
struct RowPiece { size_t off, pitch, width, n; };
inline int row_run_pieces(size_t stride, size_t row_bytes, size_t rows, size_t first, size_t period, size_t run, size_t count, RowPiece out[2])
{
    int np = 0;
    const size_t pitch = period * stride, start = first * stride;
    const bool tail = first + (count - 1) * period + run == rows;
    const size_t full = tail ? count - 1 : count;
    if (full > 0) out[np++] = RowPiece{start, pitch, run * stride, full};
    if (tail) out[np++] = RowPiece{start + full * pitch, pitch, (run - 1) * stride + row_bytes, 1};
    return np;
}

} // namespace nvca
