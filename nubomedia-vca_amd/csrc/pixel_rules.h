// pixel_rules.h -- the per-pixel arithmetic that a host loop and a kernel share (one rule, two callers), and the cv::resize
// tables both read.
#pragma once
#include <vector>
#include "../../include/nubovca.h"
#include "device_records.h"     // NVCA_HD

namespace nvca {

// resize tables (cv::resize INTER_LINEAR 8U fixed point)
struct ResizeTab {
    int sw = 0, sh = 0, dw = 0, dh = 0;
    int mode = 0;           // 0 identity, 1 bilinear, 2 area-fast 2x2
    int xmax = 0;
    std::vector<int> xofs, yofs;
    std::vector<short> ialpha, ibeta;
};
void build_resize_tab(int sw, int sh, int dw, int dh, ResizeTab &t);

// ---- view-* outlines (nvca_draw_shapes): one coverage rule for the host rasteriser and the kernel
NVCA_HD inline bool shape_covers(const nvca_shape &sh, int px, int py)
{
    if (sh.kind == NVCA_SHAPE_RING4) {
        if (sh.w < 0) return false;
        const long long ro = sh.w + 2, ri = sh.w - 2 > 0 ? sh.w - 2 : 0, dx = px - sh.x, dy = py - sh.y, d2 = dx * dx + dy * dy;
        return d2 <= ro * ro && d2 >= ri * ri;
    }
    int x0 = sh.x, y0 = sh.y, x1 = sh.x + sh.w, y1 = sh.y + sh.h;
    if (x0 > x1) { const int t = x0; x0 = x1; x1 = t; }
    if (y0 > y1) { const int t = y0; y0 = y1; y1 = t; }
    const int ax0 = px > x0 ? px - x0 : x0 - px, ax1 = px > x1 ? px - x1 : x1 - px;
    const int ay0 = py > y0 ? py - y0 : y0 - py, ay1 = py > y1 ? py - y1 : y1 - py;
    if (px >= x0 && px <= x1 && (ay0 <= 1 || ay1 <= 1)) return true;          // the two horizontal edges, 3 rows each
    if (py >= y0 && py <= y1 && (ax0 <= 1 || ax1 <= 1)) return true;          // the two vertical edges, 3 columns each
    const int mx = ax0 < ax1 ? ax0 : ax1, my = ay0 < ay1 ? ay0 : ay1;         // round joins: the 4-neighbourhood of a vertex
    return mx + my == 1;
}
void draw_shapes_host(uint8_t *data, int w, int h, int stride, int channels, const nvca_shape *shapes, int n);

// ---- image-to-overlay (nvca_overlay_blend): kms_face_detect_display_detections_overlay_img, FACE/kmsfacedetect.cpp:427-502.
// One arithmetic for the host loop and the kernel (as for the outlines above).
// Channel k of output pixel (x, y) of cvResize(costume, costumeAux, CV_INTER_LINEAR) on an 8-bit image with cn interleaved
// channels: cv::resize's fixed-point bilinear path (11-bit coefficients, tables from build_resize_tab), its 2 x 2 area
// shortcut, or the identity.
NVCA_HD inline int resize_sample_cn(const uint8_t *src, int sh, int sstride, int cn, int mode, const int *xofs, const short *ialpha,
                                    const int *yofs, const short *ibeta, int xmax, int x, int y, int k)
{
    if (mode == 0) return src[(size_t)y * sstride + (size_t)x * cn + k];
    if (mode == 2) {
        const uint8_t *s0 = src + (size_t)(2 * y) * sstride + (size_t)(2 * x) * cn + k, *s1 = s0 + sstride;
        return (s0[0] + s0[cn] + s1[0] + s1[cn] + 2) >> 2;
    }
    int sy0 = yofs[y], sy1 = sy0 + 1;
    sy0 = sy0 >= 0 ? (sy0 < sh ? sy0 : sh - 1) : 0;
    sy1 = sy1 >= 0 ? (sy1 < sh ? sy1 : sh - 1) : 0;
    const uint8_t *s0 = src + (size_t)sy0 * sstride + (size_t)xofs[x] * cn + k, *s1 = src + (size_t)sy1 * sstride + (size_t)xofs[x] * cn + k;
    const bool inner = x < xmax;
    const int a0 = inner ? ialpha[2 * x] : 2048, a1 = inner ? ialpha[2 * x + 1] : 0;
    const int h0 = s0[0] * a0 + (inner ? s0[cn] * a1 : 0), h1 = s1[0] * a0 + (inner ? s1[cn] * a1 : 0);
    return (((ibeta[2 * y] * (h0 >> 4)) >> 16) + ((ibeta[2 * y + 1] * (h1 >> 4)) >> 16) + 2) >> 2;
}
// the write of one overlay pixel v[0 .. cn) onto a BGR pixel of the frame (:467-490; SRC_OVERLAY is 1)
NVCA_HD inline void overlay_pixel(uint8_t *px, const int *v, int cn)
{
    if (cn == 1) { px[0] = px[1] = px[2] = (uint8_t)v[0]; return; }
    if (cn == 3) { px[0] = (uint8_t)v[0]; px[1] = (uint8_t)v[1]; px[2] = (uint8_t)v[2]; return; }
    const double proportion = (double)v[3] / (double)255;
    const double overlay = 1.0 * proportion, original = 1 - overlay;
    for (int k = 0; k < 3; k++) px[k] = (uint8_t)((v[k] * overlay) + (px[k] * original));
}
// where the reference puts the scaled image for a box, and how large (:441-444: the sums are truncated, not the products)
struct OverlayPlace { int x, y, w, h; };
inline OverlayPlace overlay_place(const nvca_rect &b, const nvca_overlay &ov)
{
    OverlayPlace p;
    p.x = (int)(b.x + (b.w * ov.offset_x_percent));
    p.y = (int)(b.y + (b.h * ov.offset_y_percent));
    p.h = (int)(b.h * ov.height_percent);
    p.w = (int)(b.w * ov.width_percent);
    return p;
}
void overlay_blend_host(uint8_t *frame, int W, int H, int stride, const nvca_rect *boxes, int n, const nvca_overlay &ov);

} // namespace nvca
