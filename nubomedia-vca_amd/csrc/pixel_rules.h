// pixel_rules.h -- the per-pixel arithmetic that a host loop and a kernel share (one rule, two callers): resize_sample, the one
// statement of cv::resize(INTER_LINEAR) on 8-bit images, over the tables both read (ResizeTab, seen through a ResizeView); shape
// coverage; the overlay blend; the 4:2:0 conversions.
#pragma once
#include <vector>
#include "../../include/nubovca.h"
#include "device_records.h"     // NVCA_HD, YuvPlanes

#if defined(__HIPCC__)
#define NVCA_HD_INLINE __host__ __device__ inline __attribute__((always_inline))
#else
#define NVCA_HD_INLINE inline
#endif

namespace nvca {

// resize tables (cv::resize INTER_LINEAR 8U fixed point)
struct ResizeTab {
    int sw = 0, sh = 0, dw = 0, dh = 0;
    int mode = 0;           // 0 identity, 1 bilinear, 2 area-fast 2x2
    int xmax = 0;
    std::vector<int> xofs, yofs;
    std::vector<short> ialpha, ibeta;
    ResizeView view() const { return ResizeView{mode, xmax, xofs.data(), ialpha.data(), yofs.data(), ibeta.data()}; }
};
void build_resize_tab(int sw, int sh, int dw, int dh, ResizeTab &t);

// Destination sample (x, y) of cv::resize(INTER_LINEAR) on an 8-bit image of N channels and `sh` rows (OpenCV 2.4 imgproc/imgwarp.cpp):
// the identity, the exact-2x area shortcut, or the fixed-point bilinear path -- 11-bit coefficients, rows clamped to the image, the
// horizontal pass of a row scaled down by 16 before the vertical one.  `tap(r, c, v)` leaves the N channel values of source pixel
// (r, c) in v: a packed pixel, a gray byte, a gray byte through a LUT, a pixel converted where it is read.  The right-hand column
// xofs[x] + 1 is tapped ONLY where x < xmax: from xmax on it does not exist, and on the last row of a tightly allocated image its
// bytes lie outside the buffer.  Returns the integers: the caller keeps its own truncation (& 255, a uint8_t cast, none).
template <int N, class Tap>
NVCA_HD_INLINE void resize_sample(Tap tap, int sh, const ResizeView &t, int x, int y, int *out)
{
    if (t.mode == 0) { tap(y, x, out); return; }
    if (t.mode == 2) {
        int p[4][N];
        tap(2 * y, 2 * x, p[0]); tap(2 * y, 2 * x + 1, p[1]); tap(2 * y + 1, 2 * x, p[2]); tap(2 * y + 1, 2 * x + 1, p[3]);
        for (int k = 0; k < N; k++) out[k] = (p[0][k] + p[1][k] + p[2][k] + p[3][k] + 2) >> 2;
        return;
    }
    int sy0 = t.yofs[y], sy1 = sy0 + 1;
    sy0 = sy0 >= 0 ? (sy0 < sh ? sy0 : sh - 1) : 0;
    sy1 = sy1 >= 0 ? (sy1 < sh ? sy1 : sh - 1) : 0;
    const int sx = t.xofs[x], b0 = t.ibeta[2 * y], b1 = t.ibeta[2 * y + 1];
    // the horizontal pass of the two rows.  Every tap stays inside its branch: a right-hand tap in front of the branch would read past
    // the image where x >= xmax, and the left-hand taps in front of it make two dependent trips to memory a sample where one serves
    // (measured on k_work_resize at ROI sizes: 8-11 % of its time)
    int h0[N], h1[N];
    if (x < t.xmax) {
        const int a0 = t.ialpha[2 * x], a1 = t.ialpha[2 * x + 1];
        int l0[N], r0[N], l1[N], r1[N];
        tap(sy0, sx, l0); tap(sy0, sx + 1, r0); tap(sy1, sx, l1); tap(sy1, sx + 1, r1);
        for (int k = 0; k < N; k++) { h0[k] = l0[k] * a0 + r0[k] * a1; h1[k] = l1[k] * a0 + r1[k] * a1; }
    } else {
        tap(sy0, sx, h0); tap(sy1, sx, h1);
        for (int k = 0; k < N; k++) { h0[k] *= 2048; h1[k] *= 2048; }
    }
    for (int k = 0; k < N; k++) out[k] = (((b0 * (h0[k] >> 4)) >> 16) + ((b1 * (h1[k] >> 4)) >> 16) + 2) >> 2;
}
// channel k of that sample for a packed image of cn interleaved channels, cn known only at run time (the overlay image)
NVCA_HD_INLINE int resize_sample_cn(const uint8_t *src, int sh, int sstride, int cn, const ResizeView &t, int x, int y, int k)
{
    int v;
    resize_sample<1>([&](int r, int c, int *p) { p[0] = src[(size_t)r * sstride + (size_t)c * cn + k]; }, sh, t, x, y, &v);
    return v;
}

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
// the box outside which shape_covers is false, unclipped: what a host loop walks and a launch covers
struct ShapeBox { int x0, y0, x1, y1; };
inline ShapeBox shape_bounds(const nvca_shape &sh)
{
    if (sh.kind == NVCA_SHAPE_RING4) { const int r = (sh.w > 0 ? sh.w : 0) + 2; return ShapeBox{sh.x - r, sh.y - r, sh.x + r, sh.y + r}; }
    const int xe = sh.x + sh.w, ye = sh.y + sh.h;
    return ShapeBox{(sh.x < xe ? sh.x : xe) - 1, (sh.y < ye ? sh.y : ye) - 1, (sh.x > xe ? sh.x : xe) + 1, (sh.y > ye ? sh.y : ye) + 1};
}
void draw_shapes_host(uint8_t *data, int w, int h, int stride, int channels, const nvca_shape *shapes, int n);

// ---- 4:2:0 frames, both directions.  A.13: cv::cvtColor(CV_YUV2BGR_NV12 / _I420) as OpenCV 2.4 color.cpp computes it, BT.601 limited
// range, shift 20 -- pixel (x, y) takes the chroma sample (x >> 1, y >> 1); all int32, the shift arithmetic.  (The kernels that read
// 4:2:0 frames: yuv_device.h.)
struct ChromaTerm { int r, g, b; };                      // what a chroma sample adds to every pixel of its 2 x 2 block, rounding included
NVCA_HD_INLINE ChromaTerm chroma_term(int U, int V)
{
    const int u = U - 128, v = V - 128;
    ChromaTerm c;
    c.r = (1 << 19) + 1673527 * v;
    c.g = (1 << 19) - 852492 * v - 409993 * u;
    c.b = (1 << 19) + 2116026 * u;
    return c;
}
NVCA_HD_INLINE int sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
NVCA_HD_INLINE void yuv_bgr(int Y, const ChromaTerm &c, int &B, int &G, int &R)
{
    const int y = (Y > 16 ? Y - 16 : 0) * 1220542;
    B = sat8((y + c.b) >> 20); G = sat8((y + c.g) >> 20); R = sat8((y + c.r) >> 20);
}
// A.18: cv::cvtColor(CV_YUV2BGR_YUY2 / _UYVY / _YVYU) on packed 4:2:2 -- in row y, pixels 2k and 2k + 1 take U and V from the four bytes
// 4k .. 4k + 3 of that row; nothing is shared between rows; the arithmetic is A.13's (chroma_term, yuv_bgr).  THE statement of the three
// byte orders: where Y0, U and V lie within a pair's four bytes (Y1 two bytes behind Y0).  Kernels (through the format as a template
// value), host code and the tests' driver read the positions here and nowhere else.
struct Yuv422Pos { int y0, u, v; };
NVCA_HD_INLINE constexpr Yuv422Pos yuv422_pos(int format)
{
    return format == NVCA_PIX_UYVY ? Yuv422Pos{1, 0, 2} : format == NVCA_PIX_YVYU ? Yuv422Pos{0, 3, 1} : Yuv422Pos{0, 1, 3};      // else: NVCA_PIX_YUY2
}
// A.14: cv::cvtColor(CV_BGR2YUV_I420), OpenCV 2.4 color.cpp (RGB888toYUV420pInvoker), BT.601 limited range, shift 20, all int32.  Y of
// every pixel; the chroma sample of a 2 x 2 block is (U, V) of the block's top-left pixel alone, nothing is averaged.  Over all 2^24
// colours Y stays in 16 .. 235 and U, V in 16 .. 240: nothing saturates.
NVCA_HD_INLINE void bgr_yuv(int B, int G, int R, int &Y, int &U, int &V)
{
    Y = (269484 * R + 528482 * G + 102760 * B + (1 << 19) + (16 << 20)) >> 20;
    U = (-155188 * R - 305135 * G + 460324 * B + (1 << 19) + (128 << 20)) >> 20;
    V = (460324 * R - 385875 * G - 74448 * B + (1 << 19) + (128 << 20)) >> 20;
}
// where the samples of a 4:2:0 buffer lie (`p`: the layout as the kernels read it, `ystride`: its luma stride): NV12 keeps V behind U
NVCA_HD_INLINE uint8_t *yuv_luma_at(uint8_t *base, const YuvPlanes &p, int ystride, int x, int y) { return base + p.off_y + (size_t)y * ystride + x; }
NVCA_HD_INLINE uint8_t *yuv_u_at(uint8_t *base, const YuvPlanes &p, int cx, int cy) { return base + p.off_u + (size_t)cy * p.cstride + (p.fmt == 1 ? 2 * cx : cx); }
NVCA_HD_INLINE uint8_t *yuv_v_at(uint8_t *base, const YuvPlanes &p, int cx, int cy) { return p.fmt == 1 ? yuv_u_at(base, p, cx, cy) + 1 : base + p.off_v + (size_t)cy * p.vstride + cx; }
// nvca_bgr_to_yuv420 on host memory is the device path through the staging ring; these two are what its kernels compute (the host
// statement a CPU driver checks the rule with): every pixel's Y, the chroma of every block from its top-left pixel
void bgr_to_yuv420_host(const uint8_t *src, int w, int h, int stride, int channels, uint8_t *base, int ystride, const YuvPlanes &p);

// ---- view-* outlines on a 4:2:0 frame (nvca_draw_shapes_yuv420): a covered pixel's Y byte becomes Y(colour); the chroma sample of a
// block becomes (U, V)(colour of the last shape covering the block's top-left pixel) if that pixel is covered; every other byte stays.
// = A.14 of the drawn BGR image, restricted to the samples whose defining pixel was drawn.
void draw_shapes_yuv420_host(uint8_t *base, int w, int h, int ystride, const YuvPlanes &p, const nvca_shape *shapes, int n);

// ---- image-to-overlay (nvca_overlay_blend): kms_face_detect_display_detections_overlay_img, FACE/kmsfacedetect.cpp:427-502.
// One arithmetic for the host loop and the kernel (as for the outlines above): the scaled image is resize_sample's
// (cvResize(costume, costumeAux, CV_INTER_LINEAR), tables from build_resize_tab), channel by channel.
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

// ---- image-to-overlay on a 4:2:0 frame (nvca_overlay_blend_yuv420), one box: the 2 x 2 block (cx, cy) of the frame.  A pixel inside the
// placed image and the frame is touched unless the image has 4 channels and its scaled alpha there is 0 (the reference leaves such a
// pixel's BGR value as it is: its bytes stay).  A touched pixel's BGR value before the box is A.13 of its Y and the block's chroma;
// overlay_pixel blends onto it; Y becomes A.14's Y of the result, and the block's chroma A.14's (U, V) of the blended top-left pixel if
// that one is touched.  Everything is read before anything is written, and nothing outside the block is read: blocks are independent.
struct OverlayImage { const uint8_t *img; int ih, istride, cn; ResizeView tab; };       // the image and its resize to one box's placed size
NVCA_HD_INLINE void overlay_block_yuv(uint8_t *base, int W, int H, int ystride, const YuvPlanes &yp, const OverlayPlace &p, const OverlayImage &o, int cx, int cy)
{
    uint8_t *pu = yuv_u_at(base, yp, cx, cy), *pv = yuv_v_at(base, yp, cx, cy);
    const ChromaTerm c = chroma_term(*pu, *pv);
    int ny[4], nu = -1, nv = -1;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int x = 2 * cx + (j & 1), y = 2 * cy + (j >> 1), w = x - p.x, h = y - p.y;
        ny[j] = -1;
        if (x >= W || y >= H || w < 0 || h < 0 || w >= p.w || h >= p.h) continue;
        int v[4] = {0, 0, 0, 0};
        for (int k = 0; k < o.cn; k++) v[k] = resize_sample_cn(o.img, o.ih, o.istride, o.cn, o.tab, w, h, k);
        if (o.cn == 4 && v[3] == 0) continue;
        int B, G, R, Y, U, V;
        yuv_bgr(*yuv_luma_at(base, yp, ystride, x, y), c, B, G, R);
        uint8_t px[3] = {(uint8_t)B, (uint8_t)G, (uint8_t)R};
        overlay_pixel(px, v, o.cn);
        bgr_yuv(px[0], px[1], px[2], Y, U, V);
        ny[j] = Y;
        if (j == 0) { nu = U; nv = V; }
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (ny[j] >= 0) *yuv_luma_at(base, yp, ystride, 2 * cx + (j & 1), 2 * cy + (j >> 1)) = (uint8_t)ny[j];
    if (nu >= 0) { *pu = (uint8_t)nu; *pv = (uint8_t)nv; }
}
void overlay_blend_yuv420_host(uint8_t *base, int W, int H, int ystride, const YuvPlanes &p, const nvca_rect *boxes, int n, const nvca_overlay &ov);

} // namespace nvca
