// tracker.cpp -- NuboTracker stream objects: replaces gst_nubo_tracker_img_conf +
// gst_nubo_tracker_process (TRK/gstnubotracker.cpp:202-237, 339-421).  Per stream the
// device keeps the previous gray frame and the motion-history image; every frame runs
// k_trk_pixel + the connected-component kernels, then __join_objects on the host.  The pure parts of a call -- launch sets, the
// wide-kernel predicate, staged sizes, the component lists -- are trk_host.cpp's; the work buffers' layout is trk_layout.h's.
#include "host_state.h"
#include "host_logic.h"
#include "trk_host.h"
#include <chrono>
#include <algorithm>
#include <cstring>

using namespace nvca;

struct nvca_tracker {
    nvca_ctx *ctx;
    nvca_tracker_params p;
    int w = 0, h = 0, num_frames = 0;
    DevBuf prev, mhi;
    nvca_pixel_layout input{};        // format NVCA_PIX_BGR: packed BGRA frames; else the planes of its 4:2:0 frames (nvca_tracker_set_input)
    const nvca_pixel_layout *yuv() const { return input.format != NVCA_PIX_BGR ? &input : nullptr; }
};

extern "C" {

void nvca_tracker_params_default(nvca_tracker_params *p)
try {
    if (!p) return;
    p->threshold = 20; p->min_area = 50; p->max_area = 30000; p->distance = 35; p->mhi_duration = 0.2; p->seg_thresh = 32;
}
NVCA_API_CATCH_VOID

int nvca_tracker_create(nvca_ctx *ctx, const nvca_tracker_params *params, nvca_tracker **out)
try {
    if (!ctx || !out) return NVCA_ERR_ARG;
    nvca_tracker *t = new (std::nothrow) nvca_tracker();
    if (!t) return NVCA_ERR_NOMEM;
    t->ctx = ctx;
    if (params) t->p = *params; else nvca_tracker_params_default(&t->p);
    *out = t;
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)

void nvca_tracker_destroy(nvca_tracker *t)
try {
    if (!t) return;
    (void)hipSetDevice(t->ctx->device);
    (void)hipStreamSynchronize(t->ctx->lane_streams[kTrackerLane]);
    t->prev.release(); t->mhi.release();
    delete t;
}
NVCA_API_CATCH_VOID

int nvca_tracker_set_params(nvca_tracker *t, const nvca_tracker_params *params)
try {
    if (!t || !params) return NVCA_ERR_ARG;
    t->p = *params;
    return NVCA_OK;
}
NVCA_API_CATCH((t ? t->ctx : nullptr))

int nvca_tracker_set_input(nvca_tracker *t, const nvca_pixel_layout *layout)
try {
    if (!t) return NVCA_ERR_ARG;
    nvca_pixel_layout in{};
    if (int rc = parse_pixel_layout(t->ctx, layout, in)) return rc;
    t->input = in;                    // previous gray and motion history stay: gray values whatever the source
    return NVCA_OK;
}
NVCA_API_CATCH((t ? t->ctx : nullptr))

} // extern "C"

namespace {

// the three diagnostic variables of the tracker, read once: rows a block of the per-pixel component kernels walks (NVCA_CCL_ROWS: k_ccl_reduce /
// _collect; NVCA_CCL_ROWS_UF: k_ccl_flatten, the union-find walk) and the share of the pixels the root list holds (NVCA_TRK_ROOTS_DIV=n: 1 / n)
struct TrkTuning { int rows, rows_uf, roots_div; };
const TrkTuning &trk_tuning()
{
    static const TrkTuning t = [] {
        auto rows = [](const char *name, int dflt) { const char *e = getenv(name); const int v = e ? atoi(e) : 0; return v > 0 && v <= kCclRowsMax ? v : dflt; };
        const char *e = getenv("NVCA_TRK_ROOTS_DIV");
        const int div = e ? atoi(e) : 8;
        return TrkTuning{rows("NVCA_CCL_ROWS", kCclRowsDefault), rows("NVCA_CCL_ROWS_UF", kCclRowsUf), div >= 1 ? div : 8};
    }();
    return t;
}

// per-stream state of a launch set's members (gst_nubo_tracker_img_conf: MHI re-created zeroed on a size change)
int ensure_state(nvca_ctx *ctx, nvca_tracker *const *trackers, const int *idx, int batch, int W, int H)
{
    const size_t N = (size_t)W * H;
    for (int b = 0; b < batch; b++) {
        nvca_tracker *t = trackers[idx[b]];
        if (t->w == W && t->h == H) continue;
        if (t->prev.ensure(N + 64) || t->mhi.ensure(N * sizeof(float) + 64)) { ctx->set_error("tracker state allocation failed"); return NVCA_ERR_NOMEM; }
        NVCA_HIP_CHECK(ctx, hipMemsetAsync(t->mhi.p, 0, N * sizeof(float), ctx->cs()));
        NVCA_HIP_CHECK(ctx, hipMemsetAsync(t->prev.p, 0, N, ctx->cs()));
        t->w = W; t->h = H;
    }
    return NVCA_OK;
}

// the work buffers of a launch set (trk_layout.h) and its tick: the live-tile list's marks are zeroed when they are of another layout
int ensure_workspace(nvca_ctx *ctx, TrkWorkspace &ws, int W, int H, int batch, int roots_cap, size_t stage_bytes, int *tick)
{
    const size_t N = (size_t)W * H, tile_bytes = sizeof(int) * trk_tiles_words(W, H, batch), out_bytes = sizeof(int) * trk_comp_words(kCompCap);
    const void *tiles_before = ws.tiles.p;
    if (ws.slots.ensure(sizeof(TrkSlot) * batch) || ws.h_slots.ensure(sizeof(TrkSlot) * batch) ||
        ws.labels.ensure(sizeof(int) * N * batch) || ws.acc.ensure(sizeof(CompAcc) * N * batch) || ws.flags.ensure(trk_flag_bytes(W, H, batch) + 64) ||
        ws.out.ensure(out_bytes) || ws.h_out.ensure(out_bytes) ||
        ws.roots.ensure(sizeof(int) * trk_roots_words(roots_cap)) || ws.tiles.ensure(tile_bytes) ||
        (stage_bytes && ws.staging.ensure(stage_bytes))) { ctx->set_error("tracker workspace allocation failed"); return NVCA_ERR_NOMEM; }
    if (ws.tiles.p != tiles_before || ws.tiles_w != W || ws.tiles_h != H || ws.tiles_batch != batch || ws.tick >= 0x7ffffffe) {
        NVCA_HIP_CHECK(ctx, hipMemsetAsync(ws.tiles.p, 0, tile_bytes, ctx->cs()));       // marks of another layout (or of two billion ticks ago) mean nothing
        ws.tiles_w = W; ws.tiles_h = H; ws.tiles_batch = batch; ws.tick = 0;
    }
    *tick = ++ws.tick;
    return NVCA_OK;
}

// the slot table of a launch set; host frames go to the staging buffer one behind the other (trk_staged_bytes)
int fill_slots(nvca_ctx *ctx, TrkWorkspace &ws, nvca_tracker *const *trackers, const nvca_frame *frames, const double *ts, const int *idx, int batch, int W, int H)
{
    TrkSlot *hs = ws.h_slots.as<TrkSlot>();
    size_t off = 0;
    for (int b = 0; b < batch; b++) {
        nvca_tracker *t = trackers[idx[b]];
        const nvca_frame &f = frames[idx[b]];
        TrkSlot &s = hs[b];
        memset(&s, 0, sizeof(s));
        if (f.mem == NVCA_MEM_HOST) {
            uint8_t *d = ws.staging.as<uint8_t>() + off;
            if (const nvca_pixel_layout *yuv = t->yuv()) { if (int rc = caller_h2d_planes(ctx, d, f.data, *yuv, W, H, ctx->cs())) return rc; }
            else if (int rc = caller_h2d(ctx, d, f.data, (size_t)f.stride * (H - 1) + (size_t)W * 4, ctx->cs())) return rc;
            off += trk_staged_bytes(t->yuv(), f.stride, W, H);
            s.src = d;
        } else s.src = (const uint8_t *)f.data;
        s.yuv = yuv_planes(t->yuv());
        s.prev = t->prev.as<uint8_t>(); s.mhi = t->mhi.as<float>();
        const double timestamp = ts[idx[b]];
        s.ts = (float)timestamp; s.delbound = (float)(timestamp - t->p.mhi_duration);    // cvUpdateMotionHistory
        s.seg = (float)t->p.seg_thresh; s.threshold = t->p.threshold;
        s.has_prev = t->num_frames > 0; s.sstride = f.stride;
        s.min_area = t->p.min_area; s.max_area = (long long)t->p.max_area;
    }
    NVCA_HIP_CHECK(ctx, hipMemcpyAsync(ws.slots.p, hs, sizeof(TrkSlot) * batch, hipMemcpyHostToDevice, ctx->cs()));
    return NVCA_OK;
}

// the live-segment counts only steer the per-pixel kernels' visiting order: zeroed in front of a launch of those
int clear_segment_counts(nvca_ctx *ctx, TrkWorkspace &ws, int W, int H, int batch)
{
    NVCA_HIP_CHECK(ctx, hipMemsetAsync(ws.flags.as<uint8_t>() + trk_count_offset(W, H, batch), 0, sizeof(int) * (size_t)batch, ctx->cs()));
    return NVCA_OK;
}

int launch_route(nvca_ctx *ctx, const TrkLaunch &L, TrkRoute route)
{
    { TimedLaunch tl(ctx, NVCA_K_TRACKER);
      launch_tracker(ctx->cs(), L, route); }
    NVCA_LAUNCH_CHECK(ctx);
    return NVCA_OK;
}

// The component list of the launch that was just queued, in ws.h_out: the header with the first kCompFirstRead components, a wait, the
// rest if there are more.  A label error refuses; with `roots_overflowed` given, a root-list overflow is reported there and nothing
// else is read (the caller launches again); the count is checked before it sizes the second copy.
int read_components(nvca_ctx *ctx, TrkWorkspace &ws, int *total, bool *roots_overflowed)
{
    int *ho = ws.h_out.as<int>();
    NVCA_HIP_CHECK(ctx, hipMemcpyAsync(ho, ws.out.p, sizeof(int) * trk_comp_words(kCompFirstRead), hipMemcpyDeviceToHost, ctx->cs()));
    NVCA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->cs()));
    if (ho[kCompFlags] & kCompLabelError) {
        int dbg[kRootsErrorWords] = {0, 0, 0};
        (void)hipMemcpy(dbg, ws.roots.as<int>() + kRootsError, sizeof(dbg), hipMemcpyDeviceToHost);
        ctx->set_error("internal: tracker label walk met an unwritten word (" + std::to_string(dbg[0]) + " times; first at " + std::to_string(dbg[1]) + ", kernel " + std::to_string(dbg[2]) + ")");
        return NVCA_ERR_INTERNAL;
    }
    if (roots_overflowed && (ho[kCompFlags] & kCompRootsOverflowed)) { *roots_overflowed = true; return NVCA_OK; }
    *total = ho[kCompCount];
    std::string err;
    if (int rc = trk_component_count(*total, err)) { ctx->set_error(err); return rc; }
    if (*total > kCompFirstRead) {
        const size_t done = trk_comp_words(kCompFirstRead);
        NVCA_HIP_CHECK(ctx, hipMemcpyAsync(ho + done, ws.out.as<int>() + done, sizeof(int) * (trk_comp_words(*total) - done), hipMemcpyDeviceToHost, ctx->cs()));
        NVCA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->cs()));
    }
    return NVCA_OK;
}

} // namespace

extern "C" {

int nvca_tracker_batch_process(nvca_ctx *ctx, int n, nvca_tracker *const *trackers, const nvca_frame *frames,
                               const double *ts, nvca_rect *out, int cap, int *n_out)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (!ctx || n < 0 || (n > 0 && (!trackers || !frames || !ts || !n_out)) || cap < 0 || (cap > 0 && !out)) return NVCA_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    // the trackers' lane: a stream of its own, so the call neither queues behind a face batch in flight nor waits for it
    struct UseLane { nvca_ctx *c; int old; UseLane(nvca_ctx *x, int l) : c(x), old(x->cur_lane) { c->cur_lane = l; } ~UseLane() { c->cur_lane = old; } } use_lane(ctx, kTrackerLane);
    ctx->timer.tick(1);
    std::vector<TrkFrameKey> keys(n);
    for (int i = 0; i < n; i++) {
        n_out[i] = 0;
        const nvca_frame &f = frames[i];
        if (!trackers[i] || trackers[i]->ctx != ctx) return NVCA_ERR_ARG;
        // every frame is validated before any tracker's state advances: a refused call leaves all of them as they were
        if (const nvca_pixel_layout *yuv = trackers[i]->yuv()) { if (check_yuv_frame(ctx, *yuv, f)) return NVCA_ERR_ARG; }
        else if (!f.data || f.width <= 0 || f.height <= 0 || f.stride < f.width * 4 || (f.mem != NVCA_MEM_HOST && f.mem != NVCA_MEM_DEVICE)) return NVCA_ERR_ARG;
        for (int j = 0; j < i; j++) if (trackers[j] == trackers[i]) { ctx->set_error("a tracker may appear once per batch"); return NVCA_ERR_ARG; }
        keys[i] = TrkFrameKey{f.width, f.height, trackers[i]->input.format};
    }
    TrkWorkspace &ws = ctx->trk;
    const TrkTuning &tune = trk_tuning();
    const bool hostprof = ctx->sw.host_profile, fold = ctx->sw.trk_fold;
    auto tp0 = std::chrono::steady_clock::now(), tp1 = tp0, tp2 = tp0;
    int total_comps = 0;
    TrkLaunchSets sets;
    trk_launch_sets(keys.data(), n, sets);
    std::vector<std::vector<nvca_rect>> comps;
    for (int si = 0; si < sets.count(); si++) {
        const int *idx = sets.member.data() + sets.begin[si];
        const int batch = sets.begin[si + 1] - sets.begin[si];
        const int W = keys[idx[0]].w, H = keys[idx[0]].h, fmt = keys[idx[0]].fmt;
        // state
        if (int rc = ensure_state(ctx, trackers, idx, batch, W, H)) return rc;
        size_t stage_bytes = 0;
        bool any_ccl = false, wide = true;
        for (int b = 0; b < batch; b++) {
            const nvca_tracker *t = trackers[idx[b]];
            const nvca_frame &f = frames[idx[b]];
            if (f.mem == NVCA_MEM_HOST) stage_bytes += trk_staged_bytes(t->yuv(), f.stride, W, H);
            if (!trk_wide_ok(fmt, t->yuv(), f.mem, (uintptr_t)f.data, f.stride, W)) wide = false;
            if (t->num_frames > 0) any_ccl = true;
        }
        // workspace, slots
        TrkLaunch L{};
        L.roots_cap = trk_roots_cap(W, H, batch, tune.roots_div);
        if (int rc = ensure_workspace(ctx, ws, W, H, batch, L.roots_cap, stage_bytes, &L.tick)) return rc;
        if (int rc = fill_slots(ctx, ws, trackers, frames, ts, idx, batch, W, H)) return rc;
        L.slots = ws.slots.as<TrkSlot>(); L.batch = batch; L.w = W; L.h = H; L.fmt = fmt; L.wide = wide;
        L.labels = ws.labels.as<int>(); L.acc = ws.acc.as<CompAcc>(); L.out = ws.out.as<int>(); L.cap = kCompCap;
        L.flags = ws.flags.as<uint8_t>(); L.roots = ws.roots.as<int>(); L.tiles = ws.tiles.as<int>();
        L.order = ctx->sw.trk_order; L.rows = tune.rows; L.rows_uf = tune.rows_uf;
        // launch (the result header and the root list's header are cleared by the pixel kernel)
        if (!fold) if (int rc = clear_segment_counts(ctx, ws, W, H, batch)) return rc;
        if (yuv_is_422(fmt) && ctx->sw.plan_debug) fprintf(stderr, "[nvca plan] 4:2:2 tracker pass of %d frame(s) %d x %d: %s\n", batch, W, H, wide ? "k_trk_pixel_yuv422x4" : "k_trk_pixel_yuv422");
        else if (fmt != NVCA_PIX_BGR && ctx->sw.plan_debug) fprintf(stderr, "[nvca plan] 4:2:0 tracker pass of %d frame(s) %d x %d: %s\n", batch, W, H, wide ? "k_trk_pixel_yuv8" : "k_trk_pixel_yuv");
        if (int rc = launch_route(ctx, L, !any_ccl ? kTrkPixelOnly : fold ? kTrkFolded : kTrkPerPixel)) return rc;
        tp1 = std::chrono::steady_clock::now();
        // read back; fallback
        int total = 0;
        if (any_ccl) {
            bool roots_overflowed = false;
            if (int rc = read_components(ctx, ws, &total, fold ? &roots_overflowed : nullptr)) return rc;
            if (roots_overflowed) {
                // more tile roots than the list holds (a frame of single-pixel components): the same motion history through the per-pixel kernels
                NVCA_HIP_CHECK(ctx, hipMemsetAsync(ws.out.p, 0, kCompHdr * sizeof(int), ctx->cs()));
                if (int rc = clear_segment_counts(ctx, ws, W, H, batch)) return rc;
                if (int rc = launch_route(ctx, L, kTrkPerPixelAlone)) return rc;
                if (int rc = read_components(ctx, ws, &total, nullptr)) return rc;
            }
        } else
            NVCA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->cs()));
        tp2 = std::chrono::steady_clock::now(); total_comps += total;
        // host logic
        std::string err;
        if (int rc = trk_component_lists(ws.h_out.as<int>(), total, batch, comps, err)) { ctx->set_error(err); return rc; }
        for (int b = 0; b < batch; b++) {
            nvca_tracker *t = trackers[idx[b]];
            if (t->num_frames > 0) {
                std::vector<nvca_rect> &sb = comps[b];
                join_objects(sb, t->p.min_area, t->p.max_area, t->p.distance);      // __join_objects :380
                n_out[idx[b]] = (int)sb.size();
                for (int k = 0; k < std::min<int>(cap, (int)sb.size()); k++) out[(size_t)idx[b] * cap + k] = sb[k];
            }
            t->num_frames++;
        }
    }
    if (hostprof) {
        auto tp3 = std::chrono::steady_clock::now();
        auto us = [](auto a, auto b) { return (long)std::chrono::duration_cast<std::chrono::microseconds>(b - a).count(); };
        fprintf(stderr, "[nvca host] tracker: enqueue %ld us, wait %ld us, host logic %ld us, %d components\n", us(tp0, tp1), us(tp1, tp2), us(tp2, tp3), total_comps);
    }
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)

int nvca_tracker_process(nvca_tracker *t, const nvca_frame *f, double ts, nvca_rect *out, int cap, int *n_out)
try {
    if (!t || !f) return NVCA_ERR_ARG;
    nvca_tracker *arr[1] = {t};
    return nvca_tracker_batch_process(t->ctx, 1, arr, f, &ts, out, cap, n_out);
}
NVCA_API_CATCH((t ? t->ctx : nullptr))

} // extern "C"
