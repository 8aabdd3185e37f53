// face_stream.cpp -- NuboFaceDetector stream objects: the frame gating, the batched face path in two halves (submit: gating and
// every launch queued; collect: candidates -> tracked faces -> boxes) and its entry points.
#include "host_state.h"
#include "host_logic.h"
#include <algorithm>
#include <cstdio>
#include <new>

using namespace nvca;

// =========================================================================
// NuboFaceDetector stream
// =========================================================================
struct nvca_face_stream {
    nvca_ctx *ctx;
    const nvca_cascade *cascade;
    nvca_face_params p;
    Faces faces;
    int num_frame = 0, num_iter = 0, frames_with_no_detection = 0, num_frames_to_process = 0;
    int pending_events = 0;
    nvca_pixel_layout input{};        // format NVCA_PIX_BGR: packed frames; else the planes of its 4:2:0 frames (nvca_face_stream_set_input)
    const nvca_pixel_layout *yuv() const { return input.format != NVCA_PIX_BGR ? &input : nullptr; }
};

namespace {
constexpr int kGOP = 4;                               // FACE/kmsfacedetect.cpp:28
constexpr int kMaxNoDetection = 1;                    // :30
constexpr int kNumFramesToProcess = 10;               // :23

struct FrameWork {
    bool analysed = false;
    int cols = 0, rows = 0, norm_scale = 0;
    std::vector<nvca_rect> det;
};

// the frame gating of kms_face_detect_process_frame (:794-803, :829-830); independent of detection results
bool face_gate(nvca_face_stream *s)
{
    bool received = true;
    if (s->p.detect_event) {                          // __receive_event :722-755
        received = false;
        if (s->pending_events > 0) { s->pending_events--; received = true; s->num_frames_to_process = kNumFramesToProcess; }
    }
    if (!received && s->num_frames_to_process <= 0) return false;     // early return: counters untouched
    s->num_frame++; s->num_iter++;
    bool run = false;
    const int px = s->p.process_x_every_4;
    if ((2 == px && (1 == s->num_frame % 2)) || ((2 != px) && (s->num_frame <= px))) {
        s->num_frames_to_process--;
        run = true;
    }
    if (kGOP == s->num_frame) s->num_frame = 0;
    return run;
}
} // namespace

extern "C" {

void nvca_face_params_default(nvca_face_params *p)
try {
    if (!p) return;
    p->width_to_process = 160; p->process_x_every_4 = 4; p->scale_factor_pct = 25; p->track_threshold = 40;
    p->euclidean_threshold = 8; p->area_threshold = 500; p->min_neighbors = 3; p->detect_event = 0;
}
NVCA_API_CATCH_VOID

static int face_stream_new(nvca_ctx *ctx, const nvca_cascade *cascade, const nvca_face_params *params, nvca_face_stream **out)
{
    nvca_face_stream *s = new (std::nothrow) nvca_face_stream();
    if (!s) return NVCA_ERR_NOMEM;
    s->ctx = ctx; s->cascade = cascade;
    if (params) s->p = *params; else nvca_face_params_default(&s->p);
    *out = s;
    return NVCA_OK;
}
int nvca_face_stream_create(nvca_ctx *ctx, const nvca_cascade *cascade, const nvca_face_params *params, nvca_face_stream **out)
try {
    if (!ctx || !cascade || !out) return NVCA_ERR_ARG;
    if (cascade->format != NVCA_CASCADE_HAAR) { ctx->set_error("face streams do not take an LBP cascade (nvca_detect_multiscale does)"); return NVCA_ERR_UNSUPPORTED; }
    return face_stream_new(ctx, cascade, params, out);
}
NVCA_API_CATCH(ctx)
// FACE/kmsfacedetect.cpp:809-811 on whatever cascade file cv::CascadeClassifier::load took: a new-format LBP cascade's frames are
// scanned by the LBP evaluator on the equalised working image's pyramid (face_submit); a Haar cascade's stream is nvca_face_stream_create's
int nvca_face_stream_create_any(nvca_ctx *ctx, const nvca_cascade *cascade, const nvca_face_params *params, nvca_face_stream **out)
try {
    if (!ctx || !cascade || !out) return NVCA_ERR_ARG;
    if (cascade->ctx != ctx) { ctx->set_error("the cascade belongs to another context"); return NVCA_ERR_ARG; }      // (its plans and tables are its context's)
    if (cascade->format != NVCA_CASCADE_HAAR && cascade->format != NVCA_CASCADE_LBP && cascade->format != NVCA_CASCADE_HAAR_NEW) { ctx->set_error("face streams take an old-format Haar or a new-format LBP / HAAR cascade"); return NVCA_ERR_UNSUPPORTED; }
    return face_stream_new(ctx, cascade, params, out);
}
NVCA_API_CATCH(ctx)
void nvca_face_stream_destroy(nvca_face_stream *s) { delete s; }
int nvca_face_stream_set_params(nvca_face_stream *s, const nvca_face_params *params)
try {
    if (!s || !params) return NVCA_ERR_ARG;
    s->p = *params;
    return NVCA_OK;
}
NVCA_API_CATCH((s ? s->ctx : nullptr))
int nvca_face_stream_set_input(nvca_face_stream *s, const nvca_pixel_layout *layout)
try {
    if (!s) return NVCA_ERR_ARG;
    nvca_pixel_layout in{};
    if (int rc = parse_pixel_layout(s->ctx, layout, in)) return rc;
    s->input = in;                               // frames of a batch in flight keep the layout they were submitted with (its plan holds it)
    return NVCA_OK;
}
NVCA_API_CATCH((s ? s->ctx : nullptr))
int nvca_face_stream_motion_event(nvca_face_stream *s)
try {
    if (!s) return NVCA_ERR_ARG;
    s->pending_events++;
    return NVCA_OK;
}
NVCA_API_CATCH((s ? s->ctx : nullptr))

} // extern "C"

// A batch between its two halves: everything the second half (results -> temporal logic -> boxes) needs.
namespace nvca {
struct FaceTicket {
    bool pending = false;
    uint64_t serial = 0;
    int n = 0;
    std::vector<nvca_face_stream *> streams;
    std::vector<FrameWork> work;
    // gp: the group's pre-processing (and, Haar, scan) plan; scan: the plan whose candidates its jobs leave (gp, or an LBP group's "LBP|" plan)
    struct Group { GeomPlan *gp = nullptr, *scan = nullptr; std::vector<int> idx, gthr; std::vector<CascadeJob> jobs; };
    std::vector<Group> groups;
    hipEvent_t done = nullptr;
    // Two batches in flight run on two lanes (stream + planes each).  The second one's pre-processing (gray, LUT, integral:
    // bandwidth-bound) waits for the first one's band kernel and then runs beside its late-stage and grouping kernels (a few
    // hundred small workgroups that leave most of the GPU idle) -- not beside the band kernel itself, which wants every wave slot.
    int lane = 0;
    hipEvent_t band_done = nullptr;
};
}

// a job whose scan has no level (the working image is no larger than the window): an empty candidate list in its result slots
static int empty_job(nvca_ctx *ctx, CascadeJob &job)
{
    ResultBufs &rb = ctx->ws->res[ctx->ws->cur_res];
    const size_t hits_stride = (size_t)ctx->hit_cap + 1;
    const int total = std::max(job.total, job.r0 + job.n);
    if (rb.hits.ensure(hits_stride * total * sizeof(unsigned long long)) || rb.h_hits.ensure(hits_stride * total * sizeof(unsigned long long))) {
        ctx->set_error("device allocation failed for the cascade workspace"); return NVCA_ERR_NOMEM;
    }
    job.cap = (unsigned)ctx->hit_cap * (unsigned)job.n; job.dev_group = false;
    job.d_hits = rb.hits.as<unsigned long long>() + hits_stride * job.r0; job.h_hits = rb.h_hits.as<unsigned long long>() + hits_stride * job.r0;
    NVCA_HIP_CHECK(ctx, hipMemsetAsync(job.d_hits, 0, sizeof(unsigned long long), ctx->cs()));
    return cascade_fetch(ctx, job);
}

// first half: gating, then every launch of the batch queued on the context's stream (result set `res`); no waiting
static int face_submit(nvca_ctx *ctx, int n, nvca_face_stream *const *streams, const nvca_frame *frames, int res, FaceTicket &tk)
{
    if (n < 0 || (n > 0 && (!streams || !frames))) return NVCA_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    ctx->timer.tick(0);
    // a batch that overflowed its candidate lists was reported as such (its frames' gates had advanced: there is no re-run on
    // this path); the streams go on with lists sized for what that batch produced, so the following frames are answered
    if (ctx->hit_cap_wanted > ctx->hit_cap && !(ctx->face_tickets[1] && ctx->face_tickets[1]->pending) && !(ctx->face_tickets[2] && ctx->face_tickets[2]->pending)) {
        ctx->hit_cap = ctx->hit_cap_wanted; ctx->hit_cap_wanted = 0;
    }
    Workspace &ws = *ctx->ws;
    struct UseRes { Workspace &w; UseRes(Workspace &x, int r) : w(x) { w.cur_res = r; } ~UseRes() { w.cur_res = 0; } } use_res(ws, res);   // every other entry point works on set 0
    // the lane of this batch: the synchronous call and the first submitted batch on lane 0, the second submitted batch on its own
    tk.lane = res == 2 ? kFaceLane2 : 0;
    struct UseLane { nvca_ctx *c; int old; UseLane(nvca_ctx *x, int l) : c(x), old(x->cur_lane) { c->cur_lane = l; } ~UseLane() { c->cur_lane = old; } } use_lane(ctx, tk.lane);
    if (!tk.band_done) NVCA_HIP_CHECK(ctx, hipEventCreateWithFlags(&tk.band_done, hipEventDisableTiming));
    for (int o = 1; o < 3; o++) {
        // a batch in flight on the other lane: this one's kernels start behind its band kernel (see FaceTicket)
        FaceTicket *ot = ctx->face_tickets[o];
        if (o != res && ot && ot->pending && ot->lane != tk.lane && ot->band_done) NVCA_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->cs(), ot->band_done, 0));
    }
    bool band_recorded = false;
    tk.n = n; tk.streams.assign(streams, streams + n); tk.work.assign(n, FrameWork()); tk.groups.clear();
    std::vector<FrameWork> &work = tk.work;
    // ---- pass 1: geometry + gating, in frame order
    for (int i = 0; i < n; i++) {
        nvca_face_stream *s = streams[i];
        const nvca_frame &f = frames[i];
        if (!s || s->ctx != ctx) return NVCA_ERR_ARG;
        if (const nvca_pixel_layout *yuv = s->yuv()) {
            if (check_yuv_frame(ctx, *yuv, f)) return NVCA_ERR_ARG;
        } else if (check_img(ctx, f.data, f.width, f.height, f.stride, 3, f.mem)) return NVCA_ERR_ARG;
        if (s->p.width_to_process <= 0) { ctx->set_error("width-to-process must be > 0"); return NVCA_ERR_ARG; }
    }
    // The gates advance per-stream counters; plans and buffers are resolved after them and may still fail (too many scales,
    // allocation).  A failed submit must leave every stream as it found it -- callers (the GStreamer shim) re-submit the
    // frames one by one -- so the counters are restored on any error return.
    struct GateSnap { nvca_face_stream *s; int num_frame, num_iter, to_process, pending; };
    struct GateRollback {
        std::vector<GateSnap> v; bool armed = true;
        ~GateRollback() { if (armed) for (const GateSnap &g : v) { g.s->num_frame = g.num_frame; g.s->num_iter = g.num_iter; g.s->num_frames_to_process = g.to_process; g.s->pending_events = g.pending; } }
    } gates;
    for (int i = 0; i < n; i++) {
        nvca_face_stream *s = streams[i];
        bool seen = false;
        for (const GateSnap &g : gates.v) if (g.s == s) { seen = true; break; }
        if (!seen) gates.v.push_back(GateSnap{s, s->num_frame, s->num_iter, s->num_frames_to_process, s->pending_events});
    }
    for (int i = 0; i < n; i++) {
        nvca_face_stream *s = streams[i];
        const nvca_frame &f = frames[i];
        FrameWork &w = work[i];
        // kms_face_detect_conf_images :304 -- INTEGER ratio kept in a float; kms_face_send_event :190
        const float fscale = (float)(f.width / s->p.width_to_process);
        w.norm_scale = f.width / s->p.width_to_process;
        double scale = fscale;
        w.rows = f.height; w.cols = f.width;                           // process_frame :770-783
        if (cv_round(f.height / scale) > 0) w.rows = cv_round(f.height / scale); else scale = 1;
        if (cv_round(f.width / scale) > 0) w.cols = cv_round(f.width / scale); else scale = 1;
        w.analysed = face_gate(s);
    }
    // ---- pass 2: one launch set per distinct geometry; result slots are numbered over the whole batch
    std::vector<char> done(n, 0);
    int gbase = 0;
    size_t stage_off = 0;                      // host frames of all groups share this batch's staging buffer
    {
        ResultBufs &rb = ws.res[ws.cur_res];
        size_t need = 0; int na = 0;
        for (int i = 0; i < n; i++) if (work[i].analysed) { na++; need += staging_need(frames + i, nullptr, 1, streams[i]->yuv()); }
        if (rb.srcptrs.ensure((size_t)std::max(na, 1) * sizeof(void *)) || rb.h_srcptrs.ensure((size_t)std::max(na, 1) * sizeof(void *)) ||
            (need && rb.staging.ensure(need))) { ctx->set_error("allocation failed (frame staging)"); return NVCA_ERR_NOMEM; }
    }
    for (int i = 0; i < n; i++) {
        if (!work[i].analysed || done[i]) continue;
        const nvca_face_stream *s0 = streams[i];
        const nvca_frame &f0 = frames[i];
        tk.groups.emplace_back();
        FaceTicket::Group &grp = tk.groups.back();
        std::vector<int> &idx = grp.idx;
        for (int j = i; j < n; j++) {
            const nvca_face_stream *sj = streams[j];
            const nvca_frame &fj = frames[j];
            if (work[j].analysed && !done[j] && sj->cascade == s0->cascade && fj.width == f0.width && fj.height == f0.height &&
                fj.stride == f0.stride && work[j].cols == work[i].cols && work[j].rows == work[i].rows &&
                sj->p.scale_factor_pct == s0->p.scale_factor_pct && same_layout(sj->input, s0->input)) { idx.push_back(j); done[j] = 1; }
        }
        const int batch = (int)idx.size();
        const int cols = work[i].cols, rows = work[i].rows;
        GeomPlan *gp = nullptr, *scan = nullptr;
        const double sf = 1 + s0->p.scale_factor_pct * 1.0 / 100;      // MULTI_SCALE_FACTOR :142
        const bool lbp = s0->cascade->new_format();          // (a new-format scan, LBP or HAAR: lbp_job.cpp)
        int rc;
        if (lbp) {
            // the pre-processing half of the face plan and the LBP scan's own cached plan (no Haar scan tables from the cascade's empty `c`);
            // detectMultiScale :809-811 with minSize (cols / 20, rows / 20) and no maximum size (the image's: make_detect_job's default)
            if (!(sf > 1.0)) { ctx->set_error("scaleFactor must be greater than 1 (multi-scale-factor 0)"); return NVCA_ERR_ARG; }
            if ((rc = get_face_pre_plan(ctx, f0.width, f0.height, f0.stride, s0->yuv() ? 1 : 3, cols, rows, &gp, s0->yuv()))) return rc;
            grp.gp = gp; gp->inflight++;                               // (held while the second plan is stored: the cache may evict)
            if ((rc = lbp_plan(ctx, s0->cascade, cols, rows, sf, cols / 20, rows / 20, cols, rows, &scan))) return rc;
            grp.scan = scan; scan->inflight++;
        } else {
            if ((rc = get_face_plan(ctx, s0->cascade, f0.width, f0.height, f0.stride, s0->yuv() ? 1 : 3, cols, rows, sf, cols / 20, rows / 20, 0, 0, &gp, s0->yuv()))) return rc;
            grp.gp = grp.scan = scan = gp; gp->inflight++;
        }
        // Host frames: the batch goes through in chunks -- chunk c+1's H2D copies run on the copy stream while the
        // kernels of chunk c execute (with pageable memory the host blocks in the copy, the queued kernels do not).
        // Every chunk reuses planes [0, chunk); only its candidate list / box table are its own (CascadeJob).
        bool any_host = false;
        for (int b = 0; b < batch; b++) any_host = any_host || frames[idx[b]].mem == NVCA_MEM_HOST;
        const int chunk_env = ctx->sw.ingest_chunk;
        const int chunk = (any_host && chunk_env > 0 && batch >= 2 * chunk_env) ? chunk_env : batch;
        const bool piped = chunk < batch;
        if ((rc = ensure_ws(ctx, gp->g, chunk))) return rc;

        const nvca_pixel_layout *yuv = s0->yuv();
        std::vector<int> &gthr = grp.gthr;
        gthr.resize(batch);
        for (int b = 0; b < batch; b++) { const int mn = streams[idx[b]]->p.min_neighbors; gthr[b] = mn != 0 ? std::max(mn, 1) : 0; }
        std::vector<CascadeJob> &jobs = grp.jobs;
        for (int s0 = 0; s0 < batch; s0 += chunk) {
            const int nc = std::min(chunk, batch - s0);
            if ((rc = stage_frames(ctx, frames, idx.data() + s0, nc, 3, gbase + s0, piped ? ctx->copy_stream : ctx->cs(), &stage_off, &gp->rowcopy, yuv))) return rc;
            if (piped) {
                while (ctx->chunk_events.size() <= jobs.size()) {
                    hipEvent_t ev; NVCA_HIP_CHECK(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
                    ctx->chunk_events.push_back(ev);
                }
                NVCA_HIP_CHECK(ctx, hipEventRecord(ctx->chunk_events[jobs.size()], ctx->copy_stream));
                NVCA_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->cs(), ctx->chunk_events[jobs.size()], 0));
            }
            int hist_clean = ws.ln().hist_clean;                                // k_lut leaves the histograms it read zeroed again
            if (hist_clean < nc) {
                NVCA_HIP_CHECK(ctx, hipMemsetAsync(ws.ln().hist.p, 0, (size_t)nc * 256 * sizeof(unsigned), ctx->cs()));
                hist_clean = nc;
            }
            ws.ln().hist_clean = 0;                                             // dirty until the LUT kernel is queued
            CascadeJob job; job.r0 = gbase + s0; job.n = nc; job.total = n;
            unsigned long long *z_hits = nullptr, *z_deep = nullptr;
            if (!lbp && (rc = cascade_counters(ctx, gp->det, job, &z_hits, &z_deep))) return rc;      // (the LBP launch set resets its own counters)
            if (yuv) {
              TimedLaunch t(ctx, NVCA_K_GRAY);                             // cvtColor(YUV2BGR) + cv::resize + cvtColor :805-806 (+ histogram)
              const bool wide = launch_gray_yuv(ctx->cs(), ws.res[ws.cur_res].srcptrs.as<const uint8_t *>() + gbase + s0, gp->g, yuv_planes(yuv), gp->view(),
                              ws.ln().gray.as<uint8_t>(), ws.ln().hist.as<unsigned>(), nc, frames_yuv_aligned16(frames, idx.data() + s0, nc, *yuv));
              if (ctx->sw.plan_debug) fprintf(stderr, "[nvca plan] %s gray of %d frame(s) %d x %d -> %d x %d: %s\n", yuv_is_422(yuv->format) ? "4:2:2" : "4:2:0", nc, f0.width, f0.height, cols, rows, gray_yuv_kernel_name(yuv->format, wide));
            } else
            { TimedLaunch t(ctx, NVCA_K_GRAY);                             // cv::resize + cvtColor :805-806 (+ histogram)
              launch_gray(ctx->cs(), ws.res[ws.cur_res].srcptrs.as<const uint8_t *>() + gbase + s0, gp->g, gp->view(),
                          ws.ln().gray.as<uint8_t>(), ws.ln().hist.as<unsigned>(), nc, frames_aligned4(frames, idx.data() + s0, nc)); }
            { TimedLaunch t(ctx, NVCA_K_LUT);                              // equalizeHist :807 (applied inside the integral pass / where the pyramid reads the image)
              launch_lut(ctx->cs(), ws.ln().hist.as<unsigned>(), cols * rows, ws.ln().lut.as<uint8_t>(), nc, 1, z_hits, z_deep); }
            job.counters_zeroed = !lbp;
            ws.ln().hist_clean = hist_clean;
            if (lbp) {
                // detectMultiScale :809-811 on a new-format cascade: the pyramid of the equalised working image, read from the lane's gray
                // slots through their LUTs, the LBP evaluator, groupRectangles on the candidate keys (lbp_job.cpp)
                const PyrSource src{ws.ln().gray.as<uint8_t>(), gp->g.gpitch, gp->g.gray_slot, ws.ln().lut.as<uint8_t>()};
                if (!scan->lv.empty()) { if ((rc = lbp_launch_set(ctx, scan, src, cols, rows, nc, job, gthr.data() + s0, tk.band_done))) return rc; }
                else { if ((rc = empty_job(ctx, job))) return rc; NVCA_HIP_CHECK(ctx, hipEventRecord(tk.band_done, ctx->cs())); }
            } else {
            run_integral(ctx, gp->g, ws.ln().lut.as<uint8_t>(), nc);
            if (streams[idx[0]]->cascade->c.has_tilted && (rc = run_tilted(ctx, gp->g, ws.ln().lut.as<uint8_t>(), nc))) return rc;
            if ((rc = cascade_enqueue(ctx, gp->det, gp->g.sum_slot, gp->g.spitch, job, gthr.data() + s0, true, tk.band_done))) return rc;   // detectMultiScale :809-811
            }
            band_recorded = true;
            jobs.push_back(job);
        }
        gbase += batch;
    }
    if (!band_recorded) NVCA_HIP_CHECK(ctx, hipEventRecord(tk.band_done, ctx->cs()));       // nothing analysed: nothing to wait for
    if (!tk.done) NVCA_HIP_CHECK(ctx, hipEventCreateWithFlags(&tk.done, hipEventDisableTiming));
    NVCA_HIP_CHECK(ctx, hipEventRecord(tk.done, ctx->cs()));
    tk.pending = true;
    gates.armed = false;
    return NVCA_OK;
}

static void face_release(FaceTicket &tk)
{
    for (FaceTicket::Group &g : tk.groups) { if (g.gp) g.gp->inflight--; if (g.scan && g.scan != g.gp) g.scan->inflight--; }
    tk.groups.clear(); tk.pending = false;
}

// second half: wait for the batch, turn candidates into tracked faces and boxes (frame order)
static int face_collect(nvca_ctx *ctx, int res, FaceTicket &tk, nvca_rect *out, int *ids, int cap, int *n_out)
{
    (void)hipSetDevice(ctx->device);
    Workspace &ws = *ctx->ws;
    struct UseRes { Workspace &w; UseRes(Workspace &x, int r) : w(x) { w.cur_res = r; } ~UseRes() { w.cur_res = 0; } } use_res(ws, res);
    struct UseLane { nvca_ctx *c; int old; UseLane(nvca_ctx *x, int l) : c(x), old(x->cur_lane) { c->cur_lane = l; } ~UseLane() { c->cur_lane = old; } } use_lane(ctx, tk.lane);
    const int n = tk.n;
    hipError_t he = hipEventSynchronize(tk.done);
    if (he != hipSuccess) { ctx->set_error(std::string("hipEventSynchronize: ") + hipGetErrorString(he)); face_release(tk); return NVCA_ERR_HIP; }
    drain_timer(ctx);
    int rc = NVCA_OK;
    for (FaceTicket::Group &grp : tk.groups) {
        int gi0 = grp.jobs.empty() ? 0 : grp.jobs.front().r0;
        for (const CascadeJob &job : grp.jobs) {
            std::vector<std::vector<nvca_rect>> raw;
            std::vector<char> grouped;
            if ((rc = cascade_collect(ctx, grp.scan->det, job, raw, &grouped))) { face_release(tk); return rc; }
            for (int b = 0; b < job.n; b++) {
                const int gi = job.r0 - gi0 + b;                         // position inside the group
                if (grp.gthr[gi] != 0 && !grouped[b]) group_rectangles(raw[b], grp.gthr[gi], 0.2);
                tk.work[grp.idx[gi]].det.swap(raw[b]);
            }
        }
    }
    // ---- pass 3: temporal logic + emission, in frame order
    for (int i = 0; i < n; i++) {
        nvca_face_stream *s = tk.streams[i];
        FrameWork &w = tk.work[i];
        if (w.analysed) {
            if (!w.det.empty()) s->faces.track(w.det, s->p.track_threshold);           // :813-816
            else if (s->frames_with_no_detection < kMaxNoDetection) s->frames_with_no_detection += 1;   // :817-826
            else { s->frames_with_no_detection = 0; s->faces.clear(); }
        }
        const int nf = (int)s->faces.faces.size();
        n_out[i] = nf;
        for (int k = 0; k < std::min(nf, cap); k++) {                  // kms_face_send_event :208-211
            const nvca_rect &r = s->faces.faces[k].box;
            nvca_rect &o = out[(size_t)i * cap + k];
            o.x = (int)((unsigned)r.x * (unsigned)w.norm_scale); o.y = (int)((unsigned)r.y * (unsigned)w.norm_scale);
            o.w = (int)((unsigned)r.w * (unsigned)w.norm_scale); o.h = (int)((unsigned)r.h * (unsigned)w.norm_scale);
            if (ids) ids[(size_t)i * cap + k] = s->faces.faces[k].id;
        }
    }
    face_release(tk);
    return NVCA_OK;
}

void nvca::free_face_ticket(FaceTicket *t)
{
    if (!t) return;
    if (t->done) (void)hipEventDestroy(t->done);
    if (t->band_done) (void)hipEventDestroy(t->band_done);
    delete t;
}

static FaceTicket &ticket_slot(nvca_ctx *ctx, int k)
{
    if (!ctx->face_tickets[k]) ctx->face_tickets[k] = new FaceTicket();
    return *ctx->face_tickets[k];
}

extern "C" {

int nvca_face_batch_process(nvca_ctx *ctx, int n, nvca_face_stream *const *streams, const nvca_frame *frames,
                            nvca_rect *out, int *ids, int cap, int *n_out)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (n < 0 || (n > 0 && (!streams || !frames || !n_out)) || cap < 0 || (cap > 0 && !out)) return NVCA_ERR_ARG;
    // a stream's frames are consumed in order: the synchronous call may not overtake a submitted batch of the same stream
    for (int k = 1; k < 3; k++)
        if (ctx->face_tickets[k] && ctx->face_tickets[k]->pending)
            for (int i = 0; i < n; i++)
                for (nvca_face_stream *s : ctx->face_tickets[k]->streams)
                    if (s == streams[i]) { ctx->set_error("a stream of this batch has a submitted batch in flight: collect it first"); return NVCA_ERR_ARG; }
    FaceTicket &tk = ticket_slot(ctx, 0);
    int rc = face_submit(ctx, n, streams, frames, 0, tk);
    if (rc) { (void)hipStreamSynchronize(ctx->cs()); face_release(tk); return rc; }
    return face_collect(ctx, 0, tk, out, ids, cap, n_out);
}
NVCA_API_CATCH(ctx)

// Pipelined form of nvca_face_batch_process for a serving loop: submit() queues a batch and returns, collect() waits for
// the oldest submitted batch and delivers its boxes.  Up to two batches may be in flight, so the host-side work between
// batches (result unpacking, the caller's own bookkeeping) overlaps the GPU.  Batches are collected in submission order.
int nvca_face_batch_submit(nvca_ctx *ctx, int n, nvca_face_stream *const *streams, const nvca_frame *frames, int *ticket)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (!ticket) return NVCA_ERR_ARG;
    int k = 0;
    for (int c = 1; c < 3; c++) if (!(ctx->face_tickets[c] && ctx->face_tickets[c]->pending)) { k = c; break; }
    if (!k) { ctx->set_error("two batches are in flight: collect one first"); return NVCA_ERR_ARG; }
    FaceTicket &tk = ticket_slot(ctx, k);
    tk.serial = ++ctx->face_serial;
    int rc = face_submit(ctx, n, streams, frames, k, tk);
    if (rc) { (void)hipStreamSynchronize(ctx->lane_streams[tk.lane]); face_release(tk); return rc; }
    *ticket = k;
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)
int nvca_face_batch_collect(nvca_ctx *ctx, int ticket, nvca_rect *out, int *ids, int cap, int *n_out)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (ticket < 1 || ticket > 2 || !ctx->face_tickets[ticket] || !ctx->face_tickets[ticket]->pending) { ctx->set_error("no such batch in flight"); return NVCA_ERR_ARG; }
    FaceTicket &tk = *ctx->face_tickets[ticket];
    const int other = 3 - ticket;
    if (ctx->face_tickets[other] && ctx->face_tickets[other]->pending && ctx->face_tickets[other]->serial < tk.serial) {
        ctx->set_error("batches are collected in submission order"); return NVCA_ERR_ARG;
    }
    if (cap < 0 || (cap > 0 && !out) || (tk.n > 0 && !n_out)) return NVCA_ERR_ARG;
    return face_collect(ctx, ticket, tk, out, ids, cap, n_out);
}
NVCA_API_CATCH(ctx)

int nvca_face_stream_process(nvca_face_stream *s, const nvca_frame *frame, nvca_rect *out, int *ids, int cap, int *n_out)
try {
    if (!s || !frame) return NVCA_ERR_ARG;
    nvca_face_stream *arr[1] = {s};
    return nvca_face_batch_process(s->ctx, 1, arr, frame, out, ids, cap, n_out);
}
NVCA_API_CATCH((s ? s->ctx : nullptr))

} // extern "C"
