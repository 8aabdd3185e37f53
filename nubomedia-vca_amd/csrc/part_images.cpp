// part_images.cpp -- the working images of a batched part-detector call: the upload ring of the launches' small tables, the arena
// the images are carved from, the eye detectors' full-size gray images and LUTs, and the gray/equalize, resize and flip launch sets.
#include "part_call.h"
#include <algorithm>
#include <cstring>

namespace nvca {
// a small table for the next launch: page-locked staging ring -> device ring, copied on the current lane
int part_table(nvca_ctx *ctx, const void *host, size_t bytes, void **dev)
{
    PartWorkspace &pw = ctx->pw();
    static constexpr size_t kRing = 256 * 1024;
    if (pw.tables.ensure(kRing) || pw.h_tables.ensure(kRing)) { ctx->set_error("allocation failed (part detectors' tables)"); return NVCA_ERR_NOMEM; }
    const size_t room = round_up(bytes, 64);
    if (room > kRing) { ctx->set_error("part detectors: table too large"); return NVCA_ERR_ARG; }
    if (pw.tab_used + room > kRing) { NVCA_HIP_CHECK(ctx, hipDeviceSynchronize()); pw.tab_used = 0; }      // a full turn: earlier uploads must have been consumed
    uint8_t *h = pw.h_tables.as<uint8_t>() + pw.tab_used, *d = pw.tables.as<uint8_t>() + pw.tab_used;
    memcpy(h, host, bytes);
    NVCA_HIP_CHECK(ctx, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ctx->cs()));
    pw.tab_used += room;
    *dev = d;
    return NVCA_OK;
}

namespace {
// N images of one launch set: image k = [equalizeHist](resize(source k)) at dst + k * slot, pitch dw.  BGR sources: gray of the frame
// computed on the fly (cvtColor then resize); gray sources go through LUT lut_idx[k] of `luts` first when lut_idx is given
struct PartImageBatch {
    bool bgr = true, post_eq = true;
    YuvPlanes yuv{};                             // fmt 1 / 2: the sources are 4:2:0 frames of these planes (cvtColor(YUV2BGR), cvtColor, resize); 4 .. 6: packed 4:2:2
    int sw = 0, sh = 0, sstride = 0, dw = 0, dh = 0;
    std::vector<const void *> src; std::vector<int> lut_idx;
    uint8_t *dst = nullptr; size_t slot = 0;
};
int part_arena(nvca_ctx *ctx, size_t bytes, uint8_t **base)
{
    if (ctx->pw().arena.ensure(bytes + 256)) { ctx->set_error("allocation failed (part detectors' images)"); return NVCA_ERR_NOMEM; }
    *base = ctx->pw().arena.as<uint8_t>();
    return NVCA_OK;
}
int part_luts(nvca_ctx *ctx, int n_keep, int n_scratch, uint8_t **keep)
{
    PartWorkspace &pw = ctx->pw();
    const size_t need_l = (size_t)(n_keep + n_scratch + 1) * 256, need_h = (size_t)(std::max(n_keep, n_scratch) + 1) * 256 * sizeof(unsigned);
    if (pw.luts.ensure(need_l)) { ctx->set_error("allocation failed (part detectors' LUTs)"); return NVCA_ERR_NOMEM; }
    const void *old = pw.hist.p;
    if (pw.hist.ensure(need_h)) { ctx->set_error("allocation failed (part detectors' histograms)"); return NVCA_ERR_NOMEM; }
    if (pw.hist.p != old) NVCA_HIP_CHECK(ctx, hipMemset(pw.hist.p, 0, pw.hist.bytes));       // k_lut leaves what it read zeroed again
    *keep = pw.luts.as<uint8_t>();
    return NVCA_OK;
}
int part_gray_eq(nvca_ctx *ctx, const void *const *bgr, int n, int w, int h, int stride, const nvca_pixel_layout *yuv, uint8_t *gray, size_t slot, uint8_t *luts)
{
    int rc;
    void *d_ptrs = nullptr;
    if ((rc = part_table(ctx, bgr, (size_t)n * sizeof(void *), &d_ptrs))) return rc;
    PreGeom g; make_geom(g, w, h, stride, yuv ? 1 : 3, w, h);
    g.gpitch = w; g.gray_slot = slot;
    unsigned *hist = ctx->pw().hist.as<unsigned>();
    if (yuv) {
        // k_gray_yuv16 / k_gray_yuv422_16 store 16 bytes at gray + row * gpitch + x: the image's pitch is its width here, so the width, the slot and the
        // base must take the stores as the planes take the loads
        bool wide = yuv_layout_aligned16(*yuv) && w % 16 == 0 && slot % 16 == 0 && ((uintptr_t)gray & 15) == 0;
        for (int k = 0; k < n; k++) wide = wide && ((uintptr_t)bgr[k] & 15) == 0;
        TimedLaunch t(ctx, NVCA_K_GRAY);
        wide = launch_gray_yuv(ctx->cs(), (const uint8_t *const *)d_ptrs, g, yuv_planes(yuv), ResizeView{}, gray, hist, n, wide);
        if (ctx->sw.plan_debug) fprintf(stderr, "[nvca plan] %s eye gray of %d frame(s) %d x %d: %s\n", yuv_is_422(yuv->format) ? "4:2:2" : "4:2:0", n, w, h, gray_yuv_kernel_name(yuv->format, wide));
    } else {
      bool aligned = stride % 4 == 0 && w % 4 == 0 && slot % 4 == 0 && ((uintptr_t)gray & 3) == 0;
      for (int k = 0; k < n; k++) aligned = aligned && ((uintptr_t)bgr[k] & 3) == 0;
      TimedLaunch t(ctx, NVCA_K_GRAY);
      launch_gray(ctx->cs(), (const uint8_t *const *)d_ptrs, g, ResizeView{}, gray, hist, n, aligned); }
    { TimedLaunch t(ctx, NVCA_K_LUT); launch_lut(ctx->cs(), hist, w * h, luts, n, 1); }
    NVCA_LAUNCH_CHECK(ctx);
    return NVCA_OK;
}
int part_image_batch(nvca_ctx *ctx, const PartImageBatch &b, const uint8_t *luts)
{
    int rc;
    const int n = (int)b.src.size();
    if (!n) return NVCA_OK;
    GeomPlan *gp = nullptr;
    if ((rc = get_resize_plan(ctx, b.sw, b.sh, b.dw, b.dh, &gp))) return rc;
    // one table: n source pointers, then (gray sources with a LUT) n LUT indices
    std::vector<unsigned char> tab((size_t)n * sizeof(void *) + (size_t)n * sizeof(int));
    memcpy(tab.data(), b.src.data(), (size_t)n * sizeof(void *));
    const bool with_lut = !b.bgr && (int)b.lut_idx.size() == n;
    if (with_lut) memcpy(tab.data() + (size_t)n * sizeof(void *), b.lut_idx.data(), (size_t)n * sizeof(int));
    void *d_tab = nullptr;
    if ((rc = part_table(ctx, tab.data(), tab.size(), &d_tab))) return rc;
    unsigned *hist = b.post_eq ? ctx->pw().hist.as<unsigned>() : nullptr;
    uint8_t *scratch = ctx->pw().luts.as<uint8_t>() + ctx->pw().luts.bytes - (size_t)(n + 1) * 256;       // the scratch LUTs sit at the end
    if (b.post_eq && (size_t)(n + 1) * 256 > ctx->pw().luts.bytes) { ctx->set_error("internal: LUT storage"); return NVCA_ERR_ARG; }
    { TimedLaunch t(ctx, NVCA_K_RESIZE1);
      launch_work_resize(ctx->cs(), b.bgr, (const uint8_t *const *)d_tab, with_lut ? (const int *)((uint8_t *)d_tab + (size_t)n * sizeof(void *)) : nullptr, luts,
                         b.sh, b.sstride, gp->view(), b.dst, b.dw, b.dh, b.dw, b.slot, hist, n, b.yuv.fmt ? &b.yuv : nullptr); }
    if (b.post_eq) {
        { TimedLaunch t(ctx, NVCA_K_LUT); launch_lut(ctx->cs(), hist, b.dw * b.dh, scratch, n, 1); }
        launch_apply_lut(ctx->cs(), b.dst, b.dw, b.dh, b.dw, scratch, b.dst, b.dw, n, b.slot, b.slot);
    }
    NVCA_LAUNCH_CHECK(ctx);
    return NVCA_OK;
}
int part_flip_batch(nvca_ctx *ctx, const uint8_t *src, uint8_t *dst, int w, int h, int n, size_t slot)
{
    launch_flip_h(ctx->cs(), src, w, h, w, dst, w, n, slot, slot);
    NVCA_LAUNCH_CHECK(ctx);
    return NVCA_OK;
}
} // namespace

// Phase 1b of a call: the arena is carved (uploads of host frames | full-size gray images of the eye detectors' frames | the working
// images, batch by batch), host frames are uploaded, the eye detectors' gray images and LUTs are made, and every ImageBatch is one
// launch set (plus one flip launch for a batch with mirror images).  All on the current lane; nothing is waited for.
int part_images(nvca_ctx *ctx, std::vector<FrameGroup> &groups, std::vector<ImageBatch> &batches, int n_eye)
{
    int rc;
    size_t need = 0;
    auto carve = [&](size_t bytes) { const size_t at = need; need += (bytes + 255) & ~(size_t)255; return at; };
    for (FrameGroup &fg : groups) if (fg.mem == NVCA_MEM_HOST) fg.upload_at = carve(fg.yuv() ? yuv_extent(fg.layout, fg.w, fg.h) : (size_t)fg.stride * fg.h);
    for (int e = 0; e < n_eye; e++)              // in LUT order: frames of one geometry then sit at equal distances
        for (FrameGroup &fg : groups) if (fg.eye_index == e) fg.gray_at = carve((size_t)fg.w * fg.h);
    for (ImageBatch &b : batches) { b.slot = ((size_t)b.dw * b.dh + 255) & ~(size_t)255; b.at = carve(b.slot * b.members.size() * (b.flips ? 2 : 1)); }
    uint8_t *arena = nullptr, *eye_luts = nullptr;
    if ((rc = part_arena(ctx, need, &arena))) return rc;
    size_t max_members = 1;
    for (const ImageBatch &b : batches) max_members = std::max(max_members, b.members.size());
    if ((rc = part_luts(ctx, n_eye, (int)max_members, &eye_luts))) return rc;
    for (FrameGroup &fg : groups) {
        fg.bgr = fg.data;
        if (fg.mem == NVCA_MEM_HOST) {
            if (fg.yuv()) rc = caller_h2d_planes(ctx, arena + fg.upload_at, fg.data, fg.layout, fg.w, fg.h, ctx->cs());      // plane by plane, at the caller's offsets
            else rc = caller_h2d(ctx, arena + fg.upload_at, fg.data, (size_t)fg.stride * (fg.h - 1) + (size_t)fg.w * 3, ctx->cs());
            if (rc) return rc;
            fg.bgr = arena + fg.upload_at;
        }
    }
    // EYE :948-950: cvtColor + equalizeHist of the whole frame -- gray images + LUTs here, the LUT is applied where the resizes read
    {
        std::vector<char> done(groups.size(), 0);
        for (size_t gi = 0; gi < groups.size(); gi++) {
            if (groups[gi].eye_index < 0 || done[gi]) continue;
            // frames of one geometry whose gray slots and LUT indices run on: one launch set
            std::vector<const void *> srcs; const FrameGroup &g0 = groups[gi];
            const size_t slot = ((size_t)g0.w * g0.h + 255) & ~(size_t)255;
            for (size_t gj = gi; gj < groups.size(); gj++) {
                const FrameGroup &fg = groups[gj];
                if (fg.eye_index < 0 || done[gj] || fg.w != g0.w || fg.h != g0.h || fg.stride != g0.stride || !same_layout(fg.layout, g0.layout)) continue;
                if (fg.eye_index != g0.eye_index + (int)srcs.size() || fg.gray_at != g0.gray_at + slot * srcs.size()) continue;
                srcs.push_back(fg.bgr); done[gj] = 1;
            }
            if ((rc = part_gray_eq(ctx, srcs.data(), (int)srcs.size(), g0.w, g0.h, g0.stride, g0.yuv(), arena + g0.gray_at, slot, eye_luts + (size_t)g0.eye_index * 256))) return rc;
        }
    }
    for (ImageBatch &b : batches) {
        PartImageBatch ib;
        ib.bgr = !b.eye; if (!b.eye) ib.yuv = yuv_planes(&b.layout);
        ib.post_eq = b.post_eq; ib.sw = b.W; ib.sh = b.H; ib.sstride = b.eye ? b.W : b.stride; ib.dw = b.dw; ib.dh = b.dh;
        ib.dst = b.base = arena + b.at; ib.slot = b.slot;
        for (int gi : b.members) {
            const FrameGroup &fg = groups[gi];
            ib.src.push_back(b.eye ? (const void *)(arena + fg.gray_at) : fg.bgr);
            if (b.eye) ib.lut_idx.push_back(fg.eye_index);
        }
        if ((rc = part_image_batch(ctx, ib, eye_luts))) return rc;
        if (b.flips && (rc = part_flip_batch(ctx, b.base, b.base + b.slot * b.members.size(), b.dw, b.dh, (int)b.members.size(), b.slot))) return rc;     // EAR :800
    }
    return NVCA_OK;
}

int part_images_done(nvca_ctx *ctx, const int *lanes, int n)
{
    PartWorkspace &pw = ctx->pw();
    if (!pw.images_done) NVCA_HIP_CHECK(ctx, hipEventCreateWithFlags(&pw.images_done, hipEventDisableTiming));
    NVCA_HIP_CHECK(ctx, hipEventRecord(pw.images_done, ctx->cs()));
    for (int i = 0; i < n; i++)
        if (lanes[i] != ctx->cur_lane) NVCA_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->lane_streams[lanes[i]], pw.images_done, 0));
    return NVCA_OK;
}

} // namespace nvca
