// imgproc.cpp -- the image primitives of the C ABI: cvtColor, resize, equalizeHist, the view-* outlines, the overlay, flip and
// the integral images.
#include "host_state.h"
#include "host_logic.h"
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>

using namespace nvca;

// =========================================================================
// imgproc primitives
// =========================================================================

extern "C" {

int nvca_bgr2gray(nvca_ctx *ctx, const void *src, int w, int h, int stride, int channels, int mem, void *dst, int dst_stride)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (channels != 3 && channels != 4) return NVCA_ERR_ARG;
    int rc = check_img(ctx, src, w, h, stride, channels, mem);
    if (rc || !dst || dst_stride < w) return NVCA_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    PreGeom g; make_geom(g, w, h, stride, channels, w, h);
    if ((rc = ensure_ws(ctx, g, 1))) return rc;
    nvca_frame f{src, w, h, stride, mem, 0};
    // The frame pointer reaches the kernel through a pointer table that is uploaded asynchronously from page-locked host
    // memory.  Callers that chain primitives without draining the stream (the part detectors queue many frames back to back)
    // must not reuse a table entry whose upload may still be pending: every call takes the next entry of a ring.
    static constexpr int kPtrRing = 1024;
    Workspace &ws = *ctx->ws;
    ResultBufs &rb = ws.res[ws.cur_res];
    if (rb.srcptrs.ensure(kPtrRing * sizeof(void *)) || rb.h_srcptrs.ensure(kPtrRing * sizeof(void *))) { ctx->set_error("allocation failed"); return NVCA_ERR_NOMEM; }
    if (ctx->defer_device_sync > 0 && ++ctx->ptr_ring_used >= kPtrRing) {       // a full turn without a drain: drain once
        NVCA_HIP_CHECK(ctx, hipDeviceSynchronize());
        ctx->ptr_ring_used = 0;
    }
    const int slot = ctx->defer_device_sync > 0 ? ctx->ptr_ring_used : 0;
    if ((rc = stage_frames(ctx, &f, nullptr, 1, channels, slot))) return rc;
    { TimedLaunch t(ctx, NVCA_K_GRAY);
      launch_gray(ctx->cs(), rb.srcptrs.as<const uint8_t *>() + slot, g, ResizeView{},
                  ctx->ws->ln().gray.as<uint8_t>(), nullptr, 1, frames_aligned4(&f, nullptr, 1)); }
    return unstage_2d(ctx, dst, dst_stride, ctx->ws->ln().gray.p, g.gpitch, w, h, mem);
}
NVCA_API_CATCH(ctx)

int nvca_yuv420_to_bgr(nvca_ctx *ctx, const void *base, int w, int h, const nvca_pixel_layout *layout, int mem, void *dst, int dst_stride)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (!base || !layout || !dst || (mem != NVCA_MEM_HOST && mem != NVCA_MEM_DEVICE)) return NVCA_ERR_ARG;
    if (yuv_is_422(layout->format)) { ctx->set_error("nvca_yuv420_to_bgr: the layout is packed 4:2:2 (nvca_yuv422_to_bgr converts those)"); return NVCA_ERR_ARG; }
    int rc = check_yuv_layout(ctx, *layout, w, h);
    if (rc) return rc;
    if (dst_stride < w * 3) return NVCA_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    const YuvPlanes planes = yuv_planes(layout);
    if (mem == NVCA_MEM_DEVICE) {          // read and written where they are (ordered on the context's stream)
        { TimedLaunch t(ctx, NVCA_K_GRAY);
          launch_yuv420_to_bgr(ctx->cs(), (const uint8_t *)base, w, h, layout->stride[0], planes, (uint8_t *)dst, dst_stride); }
        return finish_device_op(ctx);
    }
    Workspace &ws = *ctx->ws;
    const size_t dp = round_up((size_t)w * 3, 64);
    if (ws.ln().aux.ensure(dp * h + 64)) { ctx->set_error("allocation failed"); return NVCA_ERR_NOMEM; }
    nvca_frame f{base, w, h, layout->stride[0], mem, 0};
    if ((rc = stage_frames(ctx, &f, nullptr, 1, 1, 0, nullptr, nullptr, nullptr, layout))) return rc;
    { TimedLaunch t(ctx, NVCA_K_GRAY);
      launch_yuv420_to_bgr(ctx->cs(), ws.res[ws.cur_res].staging.as<uint8_t>(), w, h, layout->stride[0], planes, ws.ln().aux.as<uint8_t>(), (int)dp); }
    return unstage_2d(ctx, dst, dst_stride, ws.ln().aux.p, dp, (size_t)w * 3, h, mem);
}
NVCA_API_CATCH(ctx)

// cv::cvtColor(CV_YUV2BGR_YUY2 / _UYVY / _YVYU): nvca_yuv420_to_bgr's path with the one packed plane
int nvca_yuv422_to_bgr(nvca_ctx *ctx, const void *base, int w, int h, const nvca_pixel_layout *layout, int mem, void *dst, int dst_stride)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (!base || !layout || !dst || (mem != NVCA_MEM_HOST && mem != NVCA_MEM_DEVICE)) return NVCA_ERR_ARG;
    if (!yuv_is_422(layout->format)) { ctx->set_error("nvca_yuv422_to_bgr: format must be NVCA_PIX_YUY2, NVCA_PIX_UYVY or NVCA_PIX_YVYU"); return NVCA_ERR_ARG; }
    int rc = check_yuv_layout(ctx, *layout, w, h);
    if (rc) return rc;
    if (dst_stride < w * 3) { ctx->set_error("nvca_yuv422_to_bgr: dst_stride is shorter than a row of 3 * width bytes"); return NVCA_ERR_ARG; }
    (void)hipSetDevice(ctx->device);
    nvca_pixel_layout one{};                 // plane 0 only: what the format does not use is ignored
    one.format = layout->format; one.offset[0] = layout->offset[0]; one.stride[0] = layout->stride[0];
    const YuvPlanes planes = yuv_planes(&one);
    if (mem == NVCA_MEM_DEVICE) {          // read and written where they are (ordered on the context's stream)
        { TimedLaunch t(ctx, NVCA_K_GRAY);
          launch_yuv422_to_bgr(ctx->cs(), (const uint8_t *)base, w, h, one.stride[0], planes, (uint8_t *)dst, dst_stride); }
        return finish_device_op(ctx);
    }
    Workspace &ws = *ctx->ws;
    const size_t dp = round_up((size_t)w * 3, 64);
    if (ws.ln().aux.ensure(dp * h + 64)) { ctx->set_error("allocation failed"); return NVCA_ERR_NOMEM; }
    nvca_frame f{base, w, h, one.stride[0], mem, 0};
    if ((rc = stage_frames(ctx, &f, nullptr, 1, 1, 0, nullptr, nullptr, nullptr, &one))) return rc;
    { TimedLaunch t(ctx, NVCA_K_GRAY);
      launch_yuv422_to_bgr(ctx->cs(), ws.res[ws.cur_res].staging.as<uint8_t>(), w, h, one.stride[0], planes, ws.ln().aux.as<uint8_t>(), (int)dp); }
    return unstage_2d(ctx, dst, dst_stride, ws.ln().aux.p, dp, (size_t)w * 3, h, mem);
}
NVCA_API_CATCH(ctx)

int nvca_bgr_to_yuv420(nvca_ctx *ctx, const void *src, int w, int h, int stride, int channels, int mem, void *base, const nvca_pixel_layout *layout)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (channels != 3 && channels != 4) return NVCA_ERR_ARG;
    int rc = check_img(ctx, src, w, h, stride, channels, mem);
    if (rc || !base || !layout) return NVCA_ERR_ARG;
    if (yuv_is_422(layout->format)) { ctx->set_error("nvca_bgr_to_yuv420: the layout must be NVCA_PIX_NV12 or NVCA_PIX_I420 (the way out is 4:2:0 only)"); return NVCA_ERR_ARG; }
    if ((rc = check_yuv_layout(ctx, *layout, w, h))) return rc;
    (void)hipSetDevice(ctx->device);
    const YuvPlanes planes = yuv_planes(layout);
    const char *const names[2] = {"k_bgr_yuv_generic", "k_bgr_yuv16"};
    if (mem == NVCA_MEM_DEVICE) {          // read and written where they are (ordered on the context's stream)
        const bool aligned = yuv_layout_aligned16(*layout) && !(((uintptr_t)src | (uintptr_t)base | (uintptr_t)stride) & 15);
        bool wide;
        { TimedLaunch t(ctx, NVCA_K_GRAY);
          wide = launch_bgr_to_yuv420(ctx->cs(), (const uint8_t *)src, w, h, stride, channels, (uint8_t *)base, layout->stride[0], planes, aligned); }
        if (ctx->sw.plan_debug) fprintf(stderr, "[nvca plan] BGR to 4:2:0 of a device frame %d x %d: %s\n", w, h, names[wide]);
        return finish_device_op(ctx);
    }
    // host memory: the packed frame in through the staging ring, the planes computed at the caller's offsets of a device buffer of the
    // layout's extent, and back plane by plane, row by row: what lies between the written rows of the caller's buffer is never touched
    Workspace &ws = *ctx->ws;
    const size_t sp = round_up((size_t)w * channels, 64), extent = yuv_extent(*layout, w, h);
    if (ws.ln().staging.ensure(sp * h) || ws.ln().aux.ensure(extent)) { ctx->set_error("allocation failed"); return NVCA_ERR_NOMEM; }
    if ((rc = stage_2d(ctx, ws.ln().staging.p, sp, src, stride, (size_t)w * channels, h, mem))) return rc;
    bool wide;
    { TimedLaunch t(ctx, NVCA_K_GRAY);
      wide = launch_bgr_to_yuv420(ctx->cs(), ws.ln().staging.as<uint8_t>(), w, h, (int)sp, channels, ws.ln().aux.as<uint8_t>(), layout->stride[0], planes,
                                  yuv_layout_aligned16(*layout) && !(((uintptr_t)ws.ln().staging.p | (uintptr_t)ws.ln().aux.p) & 15)); }
    if (ctx->sw.plan_debug) fprintf(stderr, "[nvca plan] BGR to 4:2:0 of a host frame %d x %d: %s\n", w, h, names[wide]);
    const int np = layout->format == NVCA_PIX_NV12 ? 2 : 3;
    for (int p = 0; p < np; p++) {
        const size_t row = (p == 0 || np == 2) ? (size_t)w : (size_t)w / 2, rows = p == 0 ? (size_t)h : (size_t)h / 2;
        if ((rc = unstage_2d(ctx, (uint8_t *)base + layout->offset[p], (size_t)layout->stride[p], ws.ln().aux.as<uint8_t>() + layout->offset[p], (size_t)layout->stride[p], row, rows, mem))) return rc;
    }
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)

int nvca_resize_linear(nvca_ctx *ctx, const void *src, int sw, int sh, int sstride, int channels, int mem, void *dst,
                       int dw, int dh, int dstride)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (channels == 3) {
        int rc3 = check_img(ctx, src, sw, sh, sstride, 3, mem);
        if (rc3 || !dst || dw <= 0 || dh <= 0 || dstride < dw * 3) return NVCA_ERR_ARG;
        (void)hipSetDevice(ctx->device);
        Workspace &w3 = *ctx->ws;
        const size_t sp = round_up((size_t)sw * 3, 64), dp3 = round_up((size_t)dw * 3, 64);
        if (w3.ln().staging.ensure(sp * sh + 64) || w3.ln().aux.ensure(dp3 * dh + 64)) { ctx->set_error("allocation failed"); return NVCA_ERR_NOMEM; }
        if ((rc3 = stage_2d(ctx, w3.ln().staging.p, sp, src, sstride, (size_t)sw * 3, sh, mem))) return rc3;
        GeomPlan *gp3 = nullptr;
        if ((rc3 = get_resize_plan(ctx, sw, sh, dw, dh, &gp3))) return rc3;
        { TimedLaunch t(ctx, NVCA_K_RESIZE1);
          launch_resize3(ctx->cs(), w3.ln().staging.as<uint8_t>(), sw, sh, (int)sp, gp3->view(), w3.ln().aux.as<uint8_t>(), dw, dh, (int)dp3); }
        return unstage_2d(ctx, dst, dstride, w3.ln().aux.p, dp3, (size_t)dw * 3, dh, mem);
    }
    if (channels != 1) return NVCA_ERR_ARG;
    int rc = check_img(ctx, src, sw, sh, sstride, 1, mem);
    if (rc || !dst || dw <= 0 || dh <= 0 || dstride < dw) return NVCA_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    Workspace &ws = *ctx->ws;
    PreGeom gs; make_geom(gs, sw, sh, sstride, 1, sw, sh);
    PreGeom gd; make_geom(gd, sw, sh, sstride, 1, dw, dh);
    GeomPlan *gp = nullptr;
    if ((rc = get_resize_plan(ctx, sw, sh, dw, dh, &gp))) return rc;
    if (mem == NVCA_MEM_DEVICE) {          // device images are read and written in place (ordered on the context's stream)
        { TimedLaunch t(ctx, NVCA_K_RESIZE1);
          launch_resize1(ctx->cs(), (const uint8_t *)src, sw, sh, sstride, gp->view(), (uint8_t *)dst, dw, dh, dstride, nullptr); }
        return finish_device_op(ctx);
    }
    if ((rc = ensure_ws(ctx, gs, 1)) || (rc = ensure_ws(ctx, gd, 1))) return rc;
    if (ws.ln().aux.ensure(gd.gray_slot + 64)) { ctx->set_error("allocation failed"); return NVCA_ERR_NOMEM; }
    if ((rc = stage_2d(ctx, ws.ln().gray.p, gs.gpitch, src, sstride, sw, sh, mem))) return rc;
    { TimedLaunch t(ctx, NVCA_K_RESIZE1);
      launch_resize1(ctx->cs(), ws.ln().gray.as<uint8_t>(), sw, sh, gs.gpitch, gp->view(),
                     ws.ln().aux.as<uint8_t>(), dw, dh, gd.gpitch, nullptr); }
    return unstage_2d(ctx, dst, dstride, ws.ln().aux.p, gd.gpitch, dw, dh, mem);
}
NVCA_API_CATCH(ctx)

int nvca_equalize_hist(nvca_ctx *ctx, const void *src, int w, int h, int stride, int mem, void *dst, int dst_stride)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    int rc = check_img(ctx, src, w, h, stride, 1, mem);
    if (rc || !dst || dst_stride < w) return NVCA_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    Workspace &ws = *ctx->ws;
    PreGeom g; make_geom(g, w, h, stride, 1, w, h);
    if ((rc = ensure_ws(ctx, g, 1))) return rc;
    if (mem == NVCA_MEM_DEVICE) {          // histogram of the caller's image, LUT applied straight into the destination (in place allowed)
        NVCA_HIP_CHECK(ctx, hipMemsetAsync(ws.ln().hist.p, 0, 256 * sizeof(unsigned), ctx->cs()));
        { TimedLaunch t(ctx, NVCA_K_GRAY); launch_hist(ctx->cs(), (const uint8_t *)src, w, h, stride, ws.ln().hist.as<unsigned>()); }
        { TimedLaunch t(ctx, NVCA_K_LUT); launch_lut(ctx->cs(), ws.ln().hist.as<unsigned>(), w * h, ws.ln().lut.as<uint8_t>(), 1, 1); }
        launch_apply_lut(ctx->cs(), (const uint8_t *)src, w, h, stride, ws.ln().lut.as<uint8_t>(), (uint8_t *)dst, dst_stride);
        return finish_device_op(ctx);
    }
    if (ws.ln().aux.ensure(g.gray_slot + 64)) { ctx->set_error("allocation failed"); return NVCA_ERR_NOMEM; }
    if ((rc = stage_2d(ctx, ws.ln().gray.p, g.gpitch, src, stride, w, h, mem))) return rc;
    NVCA_HIP_CHECK(ctx, hipMemsetAsync(ws.ln().hist.p, 0, 256 * sizeof(unsigned), ctx->cs()));
    { TimedLaunch t(ctx, NVCA_K_GRAY); launch_hist(ctx->cs(), ws.ln().gray.as<uint8_t>(), w, h, g.gpitch, ws.ln().hist.as<unsigned>()); }
    { TimedLaunch t(ctx, NVCA_K_LUT); launch_lut(ctx->cs(), ws.ln().hist.as<unsigned>(), w * h, ws.ln().lut.as<uint8_t>(), 1, 1); }   // slot 0 left zeroed again
    launch_apply_lut(ctx->cs(), ws.ln().gray.as<uint8_t>(), w, h, g.gpitch, ws.ln().lut.as<uint8_t>(), ws.ln().aux.as<uint8_t>(), g.gpitch);
    return unstage_2d(ctx, dst, dst_stride, ws.ln().aux.p, g.gpitch, w, h, mem);
}
NVCA_API_CATCH(ctx)

// the common bounding box of a shape list, clipped to a w x h frame; false: nothing of it lies inside
static bool shapes_box(const nvca_shape *shapes, int n, int w, int h, int &bx0, int &by0, int &bx1, int &by1)
{
    bx0 = by0 = INT_MAX; bx1 = by1 = INT_MIN;
    for (int i = 0; i < n; i++) {
        const ShapeBox b = shape_bounds(shapes[i]);
        bx0 = std::min(bx0, b.x0); by0 = std::min(by0, b.y0); bx1 = std::max(bx1, b.x1); by1 = std::max(by1, b.y1);
    }
    bx0 = std::max(bx0, 0); by0 = std::max(by0, 0); bx1 = std::min(bx1, w - 1); by1 = std::min(by1, h - 1);
    return bx0 <= bx1 && by0 <= by1;
}

int nvca_draw_shapes(nvca_ctx *ctx, const nvca_frame *frame, int channels, const nvca_shape *shapes, int n)
try {
    // host frames need no device (and no context): plain loops over the mapped buffer
    const bool host = frame && frame->mem == NVCA_MEM_HOST;
    if (!frame || (!ctx && !host) || (channels != 3 && channels != 4)) return NVCA_ERR_ARG;
    if (!frame->data || frame->width <= 0 || frame->height <= 0 || frame->stride < frame->width * channels || (frame->mem != NVCA_MEM_HOST && frame->mem != NVCA_MEM_DEVICE)) return NVCA_ERR_ARG;
    if (check_shape_list(shapes, n)) return NVCA_ERR_ARG;
    if (!n) return NVCA_OK;
    if (host) { draw_shapes_host((uint8_t *)frame->data, frame->width, frame->height, frame->stride, channels, shapes, n); return NVCA_OK; }
    NVCA_LOCK_OR_FAIL(ctx);
    int rc;
    (void)hipSetDevice(ctx->device);
    int bx0, by0, bx1, by1;
    if (!shapes_box(shapes, n, frame->width, frame->height, bx0, by0, bx1, by1)) return NVCA_OK;
    void *d_shapes = nullptr;
    if ((rc = part_table(ctx, shapes, (size_t)n * sizeof(nvca_shape), &d_shapes))) return rc;
    launch_draw_shapes(ctx->cs(), (uint8_t *)frame->data, frame->width, frame->height, frame->stride, channels, (const nvca_shape *)d_shapes, n, bx0, by0, bx1, by1);
    return finish_device_op(ctx);
}
NVCA_API_CATCH(ctx)

int nvca_overlay_blend(nvca_ctx *ctx, const nvca_frame *frame, const nvca_rect *boxes, int n, const nvca_overlay *ov)
try {
    const bool host = frame && frame->mem == NVCA_MEM_HOST;
    if (!frame || (!ctx && !host)) return NVCA_ERR_ARG;
    if (!frame->data || frame->width <= 0 || frame->height <= 0 || frame->stride < frame->width * 3 || (frame->mem != NVCA_MEM_HOST && frame->mem != NVCA_MEM_DEVICE)) return NVCA_ERR_ARG;
    if (check_overlay_args(boxes, n, ov)) return NVCA_ERR_ARG;
    if (!n || ov->height_percent == 0 || ov->width_percent == 0) return NVCA_OK;           // FACE/kmsfacedetect.cpp:436-439
    if (host) { overlay_blend_host((uint8_t *)frame->data, frame->width, frame->height, frame->stride, boxes, n, *ov); return NVCA_OK; }
    NVCA_LOCK_OR_FAIL(ctx);
    (void)hipSetDevice(ctx->device);
    int rc;
    const size_t bytes = (size_t)ov->stride * (ov->height - 1) + (size_t)ov->width * ov->channels;
    if (ctx->overlay_img.ensure(bytes + 64)) { ctx->set_error("allocation failed (overlay image)"); return NVCA_ERR_NOMEM; }
    if ((rc = caller_h2d(ctx, ctx->overlay_img.p, ov->data, bytes, ctx->cs()))) return rc;
    for (int b = 0; b < n; b++) {            // in order: a later box overwrites an earlier one where they overlap
        const OverlayPlace p = overlay_place(boxes[b], *ov);
        if (p.w <= 0 || p.h <= 0) continue;
        GeomPlan *gp = nullptr;
        if ((rc = get_resize_plan(ctx, ov->width, ov->height, p.w, p.h, &gp))) return rc;
        launch_overlay(ctx->cs(), (uint8_t *)frame->data, frame->width, frame->height, frame->stride, p,
                       OverlayImage{ctx->overlay_img.as<uint8_t>(), ov->height, ov->stride, ov->channels, gp->view()});
    }
    // the image is the caller's: the upload must have left it before the call returns
    NVCA_LAUNCH_CHECK(ctx);
    NVCA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->cs()));
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)

// the argument checks nvca_draw_shapes_yuv420 and nvca_overlay_blend_yuv420 share: a 4:2:0 frame against its layout (the rules of the
// 4:2:0 streams, check_yuv_frame); a host frame needs no context
static int check_yuv_target(nvca_ctx *ctx, const nvca_frame *frame, const nvca_pixel_layout *layout)
{
    if (!frame || !layout) return NVCA_ERR_ARG;
    if (yuv_is_422(layout->format)) { if (ctx) ctx->set_error("drawing on a frame: the layout must be NVCA_PIX_NV12 or NVCA_PIX_I420 (the way out is 4:2:0 only)"); return NVCA_ERR_ARG; }
    if (!ctx && frame->mem != NVCA_MEM_HOST) return NVCA_ERR_ARG;
    return check_yuv_frame(ctx, *layout, *frame);
}

int nvca_draw_shapes_yuv420(nvca_ctx *ctx, const nvca_frame *frame, const nvca_pixel_layout *layout, const nvca_shape *shapes, int n)
try {
    if (check_yuv_target(ctx, frame, layout) || check_shape_list(shapes, n)) return NVCA_ERR_ARG;
    if (!n) return NVCA_OK;
    const YuvPlanes planes = yuv_planes(layout);
    if (frame->mem == NVCA_MEM_HOST) { draw_shapes_yuv420_host((uint8_t *)frame->data, frame->width, frame->height, frame->stride, planes, shapes, n); return NVCA_OK; }
    NVCA_LOCK_OR_FAIL(ctx);
    int rc;
    (void)hipSetDevice(ctx->device);
    int bx0, by0, bx1, by1;
    if (!shapes_box(shapes, n, frame->width, frame->height, bx0, by0, bx1, by1)) return NVCA_OK;
    void *d_shapes = nullptr;
    if ((rc = part_table(ctx, shapes, (size_t)n * sizeof(nvca_shape), &d_shapes))) return rc;
    // grown to even coordinates: the chroma blocks [bx0 >> 1, bx1 >> 1] x [by0 >> 1, by1 >> 1] (the frame's size is even)
    const bool uv2 = layout->format == NVCA_PIX_NV12 && !((((uintptr_t)frame->data + layout->offset[1]) | (uintptr_t)layout->stride[1]) & 1);
    launch_draw_shapes_yuv(ctx->cs(), (uint8_t *)frame->data, frame->stride, planes, (const nvca_shape *)d_shapes, n, bx0 >> 1, by0 >> 1, bx1 >> 1, by1 >> 1, uv2);
    return finish_device_op(ctx);
}
NVCA_API_CATCH(ctx)

int nvca_overlay_blend_yuv420(nvca_ctx *ctx, const nvca_frame *frame, const nvca_pixel_layout *layout, const nvca_rect *boxes, int n, const nvca_overlay *ov)
try {
    if (check_yuv_target(ctx, frame, layout) || check_overlay_args(boxes, n, ov)) return NVCA_ERR_ARG;
    if (!n || ov->height_percent == 0 || ov->width_percent == 0) return NVCA_OK;           // FACE/kmsfacedetect.cpp:436-439
    const YuvPlanes planes = yuv_planes(layout);
    const int W = frame->width, H = frame->height;
    if (frame->mem == NVCA_MEM_HOST) { overlay_blend_yuv420_host((uint8_t *)frame->data, W, H, frame->stride, planes, boxes, n, *ov); return NVCA_OK; }
    NVCA_LOCK_OR_FAIL(ctx);
    (void)hipSetDevice(ctx->device);
    int rc;
    const size_t bytes = (size_t)ov->stride * (ov->height - 1) + (size_t)ov->width * ov->channels;
    if (ctx->overlay_img.ensure(bytes + 64)) { ctx->set_error("allocation failed (overlay image)"); return NVCA_ERR_NOMEM; }
    if ((rc = caller_h2d(ctx, ctx->overlay_img.p, ov->data, bytes, ctx->cs()))) return rc;
    for (int b = 0; b < n; b++) {            // in order, one launch a box: each box works on the frame the previous one left
        const OverlayPlace p = overlay_place(boxes[b], *ov);
        if (p.w <= 0 || p.h <= 0) continue;
        const long long x0 = std::max<long long>(p.x, 0), y0 = std::max<long long>(p.y, 0);
        const long long x1 = std::min<long long>((long long)p.x + p.w, W) - 1, y1 = std::min<long long>((long long)p.y + p.h, H) - 1;
        if (x0 > x1 || y0 > y1) continue;
        GeomPlan *gp = nullptr;
        if ((rc = get_resize_plan(ctx, ov->width, ov->height, p.w, p.h, &gp))) return rc;
        const OverlayImage o{ctx->overlay_img.as<uint8_t>(), ov->height, ov->stride, ov->channels, gp->view()};
        launch_overlay_yuv(ctx->cs(), (uint8_t *)frame->data, W, H, frame->stride, planes, p, o, (int)(x0 >> 1), (int)(y0 >> 1), (int)(x1 >> 1), (int)(y1 >> 1));
    }
    // the image is the caller's: the upload must have left it before the call returns
    NVCA_LAUNCH_CHECK(ctx);
    NVCA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->cs()));
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)

int nvca_flip_horizontal(nvca_ctx *ctx, const void *src, int w, int h, int stride, int mem, void *dst, int dst_stride)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    int rc = check_img(ctx, src, w, h, stride, 1, mem);
    if (rc || !dst || dst_stride < w) return NVCA_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    Workspace &ws = *ctx->ws;
    PreGeom g; make_geom(g, w, h, stride, 1, w, h);
    if (mem == NVCA_MEM_DEVICE && src != dst) {
        launch_flip_h(ctx->cs(), (const uint8_t *)src, w, h, stride, (uint8_t *)dst, dst_stride);
        return finish_device_op(ctx);
    }
    if ((rc = ensure_ws(ctx, g, 1))) return rc;
    if (ws.ln().aux.ensure(g.gray_slot + 64)) { ctx->set_error("allocation failed"); return NVCA_ERR_NOMEM; }
    if ((rc = stage_2d(ctx, ws.ln().gray.p, g.gpitch, src, stride, w, h, mem))) return rc;
    launch_flip_h(ctx->cs(), ws.ln().gray.as<uint8_t>(), w, h, g.gpitch, ws.ln().aux.as<uint8_t>(), g.gpitch);
    return unstage_2d(ctx, dst, dst_stride, ws.ln().aux.p, g.gpitch, w, h, mem);
}
NVCA_API_CATCH(ctx)

int nvca_integral(nvca_ctx *ctx, const void *src, int w, int h, int stride, int mem, int32_t *sum, double *sqsum)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    int rc = check_img(ctx, src, w, h, stride, 1, mem);
    if (rc || !sum) return NVCA_ERR_ARG;
    if (mem != NVCA_MEM_HOST) { ctx->set_error("nvca_integral: host output only"); return NVCA_ERR_ARG; }
    (void)hipSetDevice(ctx->device);
    Workspace &ws = *ctx->ws;
    PreGeom g; make_geom(g, w, h, stride, 1, w, h);
    if ((rc = ensure_ws(ctx, g, 1))) return rc;
    if ((rc = stage_2d(ctx, ws.ln().gray.p, g.gpitch, src, stride, w, h, mem))) return rc;
    run_integral(ctx, g, nullptr, 1);
    rc = unstage_2d(ctx, sum, (size_t)(w + 1) * 4, ws.ln().sum.p, (size_t)g.spitch * 4, (size_t)(w + 1) * 4, h + 1, NVCA_MEM_HOST);
    if (rc) return rc;
    if (sqsum) {                                       // device layout: u32 low-word plane, then u8 high-byte plane
        const size_t n = (size_t)(w + 1) * (h + 1);
        std::vector<unsigned> lo(n); std::vector<uint8_t> hi(n);
        rc = unstage_2d(ctx, lo.data(), (size_t)(w + 1) * 4, ws.ln().sqsum.p, (size_t)g.spitch * 4, (size_t)(w + 1) * 4, h + 1, NVCA_MEM_HOST);
        if (rc) return rc;
        rc = unstage_2d(ctx, hi.data(), (size_t)(w + 1), ws.ln().sqsum.as<unsigned>() + g.sum_slot, (size_t)g.spitch, (size_t)(w + 1), h + 1, NVCA_MEM_HOST);
        if (rc) return rc;
        for (size_t i = 0; i < n; i++) sqsum[i] = (double)(((unsigned long long)hi[i] << 32) | lo[i]);
    }
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)

int nvca_integral_tilted(nvca_ctx *ctx, const void *src, int w, int h, int stride, int mem, int32_t *tilted)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    int rc = check_img(ctx, src, w, h, stride, 1, mem);
    if (rc || !tilted) return NVCA_ERR_ARG;
    if (mem != NVCA_MEM_HOST) { ctx->set_error("nvca_integral_tilted: host output only"); return NVCA_ERR_ARG; }
    (void)hipSetDevice(ctx->device);
    Workspace &ws = *ctx->ws;
    PreGeom g; make_geom(g, w, h, stride, 1, w, h);
    if ((rc = ensure_ws(ctx, g, 1))) return rc;
    if ((rc = stage_2d(ctx, ws.ln().gray.p, g.gpitch, src, stride, w, h, mem))) return rc;
    if ((rc = run_tilted(ctx, g, nullptr, 1))) return rc;
    return unstage_2d(ctx, tilted, (size_t)(w + 1) * 4, ws.ln().tilted.p, (size_t)g.spitch * 4, (size_t)(w + 1) * 4, h + 1, NVCA_MEM_HOST);
}
NVCA_API_CATCH(ctx)

} // extern "C"
