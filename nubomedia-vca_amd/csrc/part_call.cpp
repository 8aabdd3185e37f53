// part_call.cpp -- a batched call of the part detectors in two halves: orchestration only.  What a stream's frame needs and what
// becomes of its results is decided by part_logic.cpp; the working images are made by part_images.cpp.  Here the frames of a call
// are grouped, images requested, jobs built from what the logic returned, lanes assigned and the rounds run.
// front: the gates of every stream, the working images and the face passes QUEUED (nothing is waited for); back: the face passes'
// results, the part searches in every face's region, the merging heuristics.  nvca_part_batch_process runs them back to back;
// nvca_part_batch_submit / _collect let the caller queue the next frames' front half before it collects this frames' back half, so
// that the image chains and face passes of tick k + 1 fill the GPU while tick k's searches are advanced on the host (two calls may be
// in flight: each uses the working-image set, candidate buffers and lanes of its ticket's parity).
#include "part_call.h"
#include <algorithm>

namespace nvca {

PartCall::~PartCall()
{
    if (armed && ctx) {
        (void)hipDeviceSynchronize();
        for (size_t i = 0; i < snaps.size(); i++) part_restore(streams[i]->st, snaps[i]);
    }
    job_round_free(round);
}

namespace {
struct CallSets {            // the context's per-call selections, put back when the half is over
    nvca_ctx *c; int part_set, roi_set;
    CallSets(nvca_ctx *x, int parity) : c(x), part_set(x->part_set), roi_set(x->roi_set) { c->part_set = parity; c->roi_set = 1 + parity; }
    ~CallSets() { c->part_set = part_set; c->roi_set = roi_set; c->cur_lane = 0; }
};
static constexpr int kCallLanes = 3;                      // lanes of one call: images on the first, face passes and part searches side by side on all three
// lanes 1 .. 3 / 4 .. 6; calls with several streams stay off lane 0, where a face detector's batch may be in flight
int lane_base(const PartCall &c) { return c.parity ? 1 + kCallLanes : 1; }

// the frame group of frame f, handed to a stream of this layout
int frame_group(PartCall &c, const nvca_frame &f, const nvca_pixel_layout &layout)
{
    for (size_t gi = 0; gi < c.groups.size(); gi++) {
        const FrameGroup &fg = c.groups[gi];
        if (fg.data == f.data && fg.w == f.width && fg.h == f.height && fg.stride == f.stride && fg.mem == f.mem && same_layout(fg.layout, layout)) return (int)gi;
    }
    c.groups.emplace_back();
    FrameGroup &fg = c.groups.back();
    fg.data = f.data; fg.w = f.width; fg.h = f.height; fg.stride = f.stride; fg.mem = f.mem; fg.layout = layout;
    return (int)c.groups.size() - 1;
}
// image k of the batch of (frame geometry, size, chain): asked for by frame group gi
ImageRef request_image(PartCall &c, int gi, int dw, int dh, bool eye, bool post_eq)
{
    std::vector<ImageBatch> &batches = c.batches;
    const FrameGroup &fg = c.groups[gi];
    ImageRef r;
    for (size_t bi = 0; bi < batches.size() && r.batch < 0; bi++) {
        const ImageBatch &b = batches[bi];
        // the eye chain's images are read from the full-size gray images (pitch W), not from the frames: packed, NV12 and I420 frames
        // of one size share a batch whatever their strides and layouts
        const bool same_source = eye || (b.stride == fg.stride && same_layout(b.layout, fg.layout));
        if (b.W == fg.w && b.H == fg.h && same_source && b.dw == dw && b.dh == dh && b.eye == eye && b.post_eq == post_eq) r.batch = (int)bi;
    }
    if (r.batch < 0) {
        batches.emplace_back();
        ImageBatch &b = batches.back();
        b.W = fg.w; b.H = fg.h; b.stride = fg.stride; b.layout = fg.layout; b.dw = dw; b.dh = dh; b.eye = eye; b.post_eq = post_eq;
        r.batch = (int)batches.size() - 1;
    }
    ImageBatch &b = batches[r.batch];
    const auto it = std::find(b.members.begin(), b.members.end(), gi);
    r.k = (int)(it - b.members.begin());
    if (it == b.members.end()) b.members.push_back(gi);
    return r;
}
// the face pass of one kind, cascade and scale factor over a batch's images: one for however many streams ask for it
int request_pass(PartCall &c, int type, const nvca_cascade *casc, const ImageRef &img, double sf)
{
    std::deque<FacePass> &passes = c.passes;
    int pass = -1;
    for (size_t pi = 0; pi < passes.size(); pi++)
        if (passes[pi].type == type && passes[pi].c == casc && passes[pi].batch == img.batch && passes[pi].sf == sf) pass = (int)pi;
    if (pass < 0) { passes.emplace_back(); pass = (int)passes.size() - 1; FacePass &fp = passes.back(); fp.type = type; fp.c = casc; fp.batch = img.batch; fp.sf = sf; }
    FacePass &fp = passes[pass];
    if (std::find(fp.members.begin(), fp.members.end(), img.k) == fp.members.end()) fp.members.push_back(img.k);
    return pass;
}
// a stream's faces: result k of its pass's job (mirrored: of the mirror image)
const RectV &pass_result(const PartCall &c, const PartWork &w, bool mirrored)
{
    const FacePass &fp = c.passes[w.pass];
    const size_t pos = std::find(fp.members.begin(), fp.members.end(), w.small.k) - fp.members.begin();
    const size_t per_job = fp.per_job(), ji = pos / per_job, in_job = std::min(fp.members.size() - ji * per_job, per_job);
    return detect_job_out(fp.jobs[ji], (int)(pos % per_job + (mirrored ? in_job : 0)));
}
} // namespace

int part_front(nvca_ctx *ctx, PartCall &c, int n, nvca_part_stream *const *streams, const nvca_frame *frames)
{
    if (n < 0 || (n > 0 && (!streams || !frames))) return NVCA_ERR_ARG;
    for (int i = 0; i < n; i++) {
        const nvca_part_stream *s = streams[i]; const nvca_frame *f = &frames[i];
        if (!s || s->ctx != ctx || s->p.width_to_process <= 0) return NVCA_ERR_ARG;
        if (const nvca_pixel_layout *yuv = s->yuv()) { if (check_yuv_frame(ctx, *yuv, *f)) return NVCA_ERR_ARG; }
        else if (!f->data || f->width <= 0 || f->height <= 0 || f->stride < f->width * 3 || (f->mem != NVCA_MEM_HOST && f->mem != NVCA_MEM_DEVICE)) return NVCA_ERR_ARG;
        for (int j = 0; j < i; j++) if (streams[j] == s) { ctx->set_error("a part stream may appear once per batch"); return NVCA_ERR_ARG; }
        // every frame is validated before any stream's gate advances: a refused call leaves all streams as they were
        PartScales sc;
        if (!part_scales(s->p, f->width, f->height, sc)) { ctx->set_error("part stream: frame too small"); return NVCA_ERR_ARG; }
    }
    (void)hipSetDevice(ctx->device);
    c.ctx = ctx; c.n = n;
    c.streams.assign(streams, streams + n); c.frames.assign(frames, frames + n);
    c.work.resize(n);
    const int base = lane_base(c);
    CallSets sets(ctx, c.parity);
    c.snaps.reserve(n);
    for (int i = 0; i < n; i++) c.snaps.push_back(part_snapshot(streams[i]->st));
    int rc = NVCA_OK;
    const bool stats = ctx->sw.part_stats > 0;
    c.t0 = stats ? mono_s() : 0;
    // ---- phase 1a: gating of every stream, in stream order; what the streams that run need is only noted down here
    for (int i = 0; i < n; i++) {
        PartWork &w = c.work[i];
        nvca_part_stream *s = w.s = streams[i]; const nvca_frame *f = w.f = &c.frames[i];
        if (!part_scales(s->p, f->width, f->height, w.sc)) { ctx->set_error("part stream: frame too small"); return NVCA_ERR_ARG; }
        const PartFrame &g = w.gate = part_gate(s->st, s->p);
        if (g.popped) c.snaps[i].note_popped(s->st);
        if (!g.run) continue;
        w.group = frame_group(c, *f, s->input);
        w.lane = n > 1 ? base + w.group % kCallLanes : 0;          // the part searches of one frame's streams share a lane
        // the images this stream works on: requested here, computed below for all streams at once
        if (g.eye_chain && c.groups[w.group].eye_index < 0) c.groups[w.group].eye_index = c.n_eye++;
        if (g.face_image) w.small = request_image(c, w.group, w.sc.fw, w.sc.fh, g.eye_chain, g.face_post_eq);
        w.part_ref = request_image(c, w.group, w.sc.pw, w.sc.ph, g.eye_chain, true);
        if (g.mirror) c.batches[w.small.batch].flips = true;
        if (g.pass != kPassNone) w.pass = request_pass(c, g.pass, s->face, w.small, g.pass_sf);
    }
    // ---- phase 1b: every image the call needs, in a handful of launches
    ctx->cur_lane = n > 1 ? base : 0;
    if ((rc = part_images(ctx, c.groups, c.batches, c.n_eye))) return rc;
    // the face passes: members in image order, so that a pass over all images of a batch reads them in place
    int next_lane = base + 1;
    std::vector<int> used_lanes;
    for (FacePass &fp : c.passes) {
        std::sort(fp.members.begin(), fp.members.end());
        const ImageBatch &b = c.batches[fp.batch];
        const FacePassRule &rule = face_pass_rule(fp.type);
        const size_t per_job = fp.per_job();
        for (size_t m0 = 0; m0 < fp.members.size(); m0 += per_job) {
            const size_t m1 = std::min(fp.members.size(), m0 + per_job);
            DetectJob *job = detect_job_new();
            if (!job) return NVCA_ERR_NOMEM;
            fp.jobs.push_back(job);
            if ((rc = make_detect_job(ctx, *job, fp.c, b.image(fp.members[m0]), b.dw, b.dh, b.dw, NVCA_MEM_DEVICE, fp.sf, rule.min_neighbors, rule.flags,
                                      rule.minw, rule.minh, rule.max_is_image ? b.dw : 0, rule.max_is_image ? b.dh : 0, false))) return rc;
            for (size_t m = m0 + 1; m < m1; m++) if (detect_job_add_image(job, b.image(fp.members[m])) < 0) return NVCA_ERR_ARG;
            if (rule.mirrored)         // ... and the mirrored images: results k + count
                for (size_t m = m0; m < m1; m++) if (detect_job_add_image(job, b.image(fp.members[m], true)) < 0) return NVCA_ERR_ARG;
            const int lane = n > 1 ? next_lane : 0;
            next_lane = next_lane + 1 < base + kCallLanes ? next_lane + 1 : base + 1;
            c.jobs.push_back(job); c.job_lane.push_back(lane); used_lanes.push_back(lane);
        }
    }
    for (const PartWork &w : c.work) if (w.gate.run) used_lanes.push_back(w.lane);     // the part searches of phase 2 read these images on the streams' lanes
    std::sort(used_lanes.begin(), used_lanes.end());
    used_lanes.erase(std::unique(used_lanes.begin(), used_lanes.end()), used_lanes.end());
    if ((rc = part_images_done(ctx, used_lanes.data(), (int)used_lanes.size()))) return rc;
    c.t1 = stats ? mono_s() : 0;
    // the face passes' launch sets are queued here and collected by the back half (small-image jobs: one k_roi launch for all of them)
    if (!c.jobs.empty()) {
        c.round = job_round_new();
        if (!c.round) return NVCA_ERR_NOMEM;
        if ((rc = detect_jobs_begin(ctx, c.jobs.data(), (int)c.jobs.size(), c.job_lane.data(), c.round, &c.queued))) return rc;
    }
    return NVCA_OK;
}

int part_back(nvca_ctx *ctx, PartCall &c, nvca_rect *out_a, int cap_a, int *n_a, nvca_rect *out_b, int cap_b, int *n_b)
{
    const int n = c.n;
    if ((n > 0 && (!n_a || !n_b)) || cap_a < 0 || cap_b < 0 || (cap_a > 0 && !out_a) || (cap_b > 0 && !out_b)) return NVCA_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    std::vector<DetectJob *> &jobs = c.jobs;
    std::vector<int> &job_lane = c.job_lane;
    CallSets sets(ctx, c.parity);
    int rc = NVCA_OK;
    const bool stats = ctx->sw.part_stats > 0;    // diagnostic: the host's time per phase of calls with n (default 8) or more streams, every 8 such calls
    PartStats &ps = ctx->stats;
    const int stats_min = stats ? ctx->sw.part_stats : 8;
    const bool whole_on = stats && n >= ctx->sw.part_stats;
    const double ts0 = c.t0, ts1 = c.t1, tb0 = stats ? mono_s() : 0;
    PartStats::Timer whole(whole_on, ps.whole);
    whole.t0 -= ts1 - ts0;                            // (with the front half's time)
    // Every face pass waits for the images (part_images_done), so draining the passes' lanes drains the image lane's work
    // too.  A call without any face pass (detect-event streams: the faces were pushed) has nobody waiting for it: the H2D
    // copies of the caller's frames and the image kernels are drained here, before the call can return -- the caller may
    // recycle its buffers, and the next call carves the same arena on another lane.
    if (jobs.empty() && !c.groups.empty()) {
        const hipError_t he = hipStreamSynchronize(ctx->lane_streams[n > 1 ? lane_base(c) : 0]);
        if (he != hipSuccess) { ctx->set_error(std::string("hipStreamSynchronize: ") + hipGetErrorString(he)); return NVCA_ERR_HIP; }
    }
    if (!jobs.empty() && (rc = detect_jobs_finish(ctx, jobs.data(), (int)jobs.size(), job_lane.data(), c.round, c.queued))) return rc;          // wait 1: every face pass
    c.queued = false;
    const double ts2 = stats ? mono_s() : 0;
    // ---- phase 2: the part searches of every face of every stream
    jobs.clear(); job_lane.clear();
    for (int i = 0; i < n; i++) {
        PartWork &w = c.work[i];
        if (!w.gate.run) continue;
        nvca_part_stream *s = w.s;
        const uint8_t *part = c.batches[w.part_ref.batch].image(w.part_ref.k);
        const int cols = w.sc.pw;
        const bool mirrored = w.pass >= 0 && face_pass_rule(c.passes[w.pass].type).mirrored;
        part_rois(s->st, s->p, w.sc, w.gate, w.pass >= 0 ? &pass_result(c, w, false) : nullptr, mirrored ? &pass_result(c, w, true) : nullptr, w.searches);
        // detectMultiScale on a sub-matrix of a device image (pitch == cols), as a queued job
        for (const PartSearch &q : w.searches) {
            w.jobs.push_back(nullptr);
            if (!q.valid) continue;
            DetectJob *job = w.jobs.back() = detect_job_new();
            if (!job) return NVCA_ERR_NOMEM;
            if ((rc = make_detect_job(ctx, *job, q.cascade ? s->b : s->a, part + (size_t)q.roi.y * cols + q.roi.x, q.roi.w, q.roi.h, cols, NVCA_MEM_DEVICE, q.sf,
                                      q.min_neighbors, q.flags, q.minw, q.minh, 0, 0, false))) return rc;
            jobs.push_back(job); job_lane.push_back(w.lane);
        }
    }
    const double ts3 = stats ? mono_s() : 0;
    if ((rc = run_detect_jobs(ctx, jobs.data(), (int)jobs.size(), job_lane.data()))) return rc;          // wait 2 (+ one more for searches that narrowed)
    if (stats) {
        const double ts4 = mono_s();
        if (n >= stats_min) { ps.chains += ts1 - ts0; ps.face_passes += ts2 - tb0; ps.roi_setup += ts3 - ts2; ps.roi_searches += ts4 - ts3; ps.report(); }
        else ps.clear_rounds();
    }
    c.armed = false;                // nothing below can fail short of an exception -- which the containers' strong guarantee
                                           // and the ABI barrier turn into an error code; the device work is complete
    // ---- phase 3: merging heuristics, hysteresis, emission -- in stream order
    PartStats::Timer p3(whole_on, ps.merging);
    std::vector<const RectV *> results;
    for (int i = 0; i < n; i++) {
        PartWork &w = c.work[i];
        PartState &st = w.s->st;
        results.clear();
        for (const DetectJob *j : w.jobs) results.push_back(j ? &detect_job_out(j, 0) : nullptr);
        part_finish(st, w.s->p, w.sc, w.gate, w.searches, results);
        n_a[i] = (int)st.la.size(); n_b[i] = (int)st.lb.size();
        for (int k = 0; k < std::min(n_a[i], cap_a); k++) out_a[(size_t)i * cap_a + k] = st.la[k];
        for (int k = 0; k < std::min(n_b[i], cap_b); k++) out_b[(size_t)i * cap_b + k] = st.lb[k];
    }
    return NVCA_OK;
}

} // namespace nvca
