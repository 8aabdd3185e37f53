// yuv_out_host.cpp -- the way out in 4:2:0, on host memory: the loops of nvca_draw_shapes_yuv420 and nvca_overlay_blend_yuv420 on a
// mapped NV12 / I420 buffer, and the host statement of nvca_bgr_to_yuv420.  Pure host code: no HIP header, a plain C++ compiler
// takes it (tests/san/yuv_out_driver.cpp drives it under the sanitizers).  The arithmetic is pixel_rules.h's, shared with the
// kernels (kernels_yuv_out.hip).
#include "pixel_rules.h"
#include <algorithm>

namespace nvca {

// cv::cvtColor(CV_BGR2YUV_I420) into the planes of a layout; NV12: the same samples, U and V interleaved
void bgr_to_yuv420_host(const uint8_t *src, int w, int h, int stride, int channels, uint8_t *base, int ystride, const YuvPlanes &p)
{
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const uint8_t *s = src + (size_t)y * stride + (size_t)x * channels;
            int Y, U, V;
            bgr_yuv(s[0], s[1], s[2], Y, U, V);
            *yuv_luma_at(base, p, ystride, x, y) = (uint8_t)Y;
            if (!((x | y) & 1)) { *yuv_u_at(base, p, x >> 1, y >> 1) = (uint8_t)U; *yuv_v_at(base, p, x >> 1, y >> 1) = (uint8_t)V; }
        }
}

// view-* outlines on a host 4:2:0 frame: as draw_shapes_host, the shapes one after the other over their bounding boxes -- the last
// shape that covers a pixel leaves its Y there, and its chroma where the pixel is the top-left one of its block
void draw_shapes_yuv420_host(uint8_t *base, int w, int h, int ystride, const YuvPlanes &p, const nvca_shape *shapes, int n)
{
    for (int i = 0; i < n; i++) {
        const nvca_shape &sh = shapes[i];
        const ShapeBox b = shape_bounds(sh);
        const int x0 = std::max(b.x0, 0), y0 = std::max(b.y0, 0), x1 = std::min(b.x1, w - 1), y1 = std::min(b.y1, h - 1);
        int Y, U, V;
        bgr_yuv(sh.bgra[0], sh.bgra[1], sh.bgra[2], Y, U, V);
        for (int y = y0; y <= y1; y++)
            for (int x = x0; x <= x1; x++)
                if (shape_covers(sh, x, y)) {
                    *yuv_luma_at(base, p, ystride, x, y) = (uint8_t)Y;
                    if (!((x | y) & 1)) { *yuv_u_at(base, p, x >> 1, y >> 1) = (uint8_t)U; *yuv_v_at(base, p, x >> 1, y >> 1) = (uint8_t)V; }
                }
    }
}

// image-to-overlay on a host 4:2:0 frame: every box in order, each over the 2 x 2 blocks its placed image meets (overlay_block_yuv,
// the kernel's rule)
void overlay_blend_yuv420_host(uint8_t *base, int W, int H, int ystride, const YuvPlanes &yp, const nvca_rect *boxes, int n, const nvca_overlay &ov)
{
    if (ov.height_percent == 0 || ov.width_percent == 0) return;           // FACE/kmsfacedetect.cpp:436-439
    for (int b = 0; b < n; b++) {
        const OverlayPlace p = overlay_place(boxes[b], ov);
        if (p.w <= 0 || p.h <= 0) continue;
        const long long x0 = std::max<long long>(p.x, 0), y0 = std::max<long long>(p.y, 0);
        const long long x1 = std::min<long long>((long long)p.x + p.w, W) - 1, y1 = std::min<long long>((long long)p.y + p.h, H) - 1;
        if (x0 > x1 || y0 > y1) continue;
        ResizeTab tab;
        build_resize_tab(ov.width, ov.height, p.w, p.h, tab);
        const OverlayImage o{(const uint8_t *)ov.data, ov.height, ov.stride, ov.channels, tab.view()};
        for (int cy = (int)(y0 >> 1); cy <= (int)(y1 >> 1); cy++)
            for (int cx = (int)(x0 >> 1); cx <= (int)(x1 >> 1); cx++) overlay_block_yuv(base, W, H, ystride, yp, p, o, cx, cy);
    }
}

} // namespace nvca
