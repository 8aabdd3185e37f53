// detect_job.cpp -- the launch sets of one detectMultiScale job: the plain scan, CV_HAAR_SCALE_IMAGE (its pyramid: pyramid.cpp) and the
// two sets of a CV_HAAR_FIND_BIGGEST_OBJECT search (the search itself: fb_search.cpp), and what a drained set's candidates become.  A
// new-format LBP cascade's set is lbp_job.cpp's.
#include "host_state.h"
#include "host_logic.h"
#include "group_levels.h"
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <new>

using namespace nvca;

// A detectMultiScale call in halves: enqueue() queues the next launch set of the call on the context's stream and returns;
// advance(), after the stream has drained, consumes what the set produced and either finishes the call or asks for another
// set (FIND_BIGGEST narrows its scan once).  Many calls can therefore share ONE wait per round (detect_rounds.cpp).  The image
// planes are shared working memory: jobs use them one after the other in stream order; what a job leaves behind for the host
// (its candidate list) lives in its own result region (CascadeJob::r0).
namespace nvca {

// a ladder step's clipped grid as the coordinate lists of a plan scale
static ScaleSpec fb_make_spec(const DetectJob &j, int spitch, const FbStep &st, const ScanGrid &g)
{
    ScaleSpec sp;
    sp.table_factor = st.factor; sp.plane_off = 0; sp.pitch = spitch; sp.plane_rows = j.rq.rows + 1; sp.adaptive = 1;
    sp.out_factor = 0; sp.out_w = st.winw; sp.out_h = st.winh;
    for (int ix = g.startX; ix < g.endX; ix++) sp.xs.push_back(cv_round(ix * st.ystep));
    for (int iy = g.startY; iy < g.endY; iy++) sp.ys.push_back(cv_round(iy * st.ystep));
    return sp;
}

// cvHaarDetectObjectsForROC, CV_HAAR_SCALE_IMAGE branch (EYE/kmseyedetect.cpp:991-993, NOSE/kmsnosedetect.cpp:843-846,
// MOUTH/kmsmouthdetect.cpp:845-848, EAR/kmseardetect.cpp:656-659): per factor the image is resized, integrated and
// scanned with the unscaled window on a fixed grid.  All pyramid levels (of both images: the ear detector scans an image
// and its mirror, EAR/kmseardetect.cpp:796-803) are evaluated by one launch set.
static int si_plan(nvca_ctx *ctx, const DetectJob &j, GeomPlan **out)
{
    const Cascade &c = j.rq.casc->c;
    const int cols = j.rq.cols, rows = j.rq.rows;
    int rc;
    // pyramid layout, resize tables and scan tables depend only on (cascade, image size, parameters): built once
    char key[256];
    snprintf(key, sizeof(key), "SI|%llu|%d|%d|%.17g|%d|%d|%d|%d", (unsigned long long)c.uid, cols, rows, j.rq.sf, j.rq.minw, j.rq.minh, j.rq.maxw, j.rq.maxh);
    GeomPlan *pp = find_plan(ctx, key);
    if (!pp) {
        std::unique_ptr<GeomPlan> np(new GeomPlan());
        // (a plan holds every level the call has: build_custom sizes the candidate key for them and refuses, loudly, what no key holds.
        // The pyramid's two halves apart: the scan tables go to the device between them)
        if ((rc = pyr_plan_tabs(ctx, *np, cols, rows, si_levels(c.ow, c.oh, cols, rows, j.rq.sf, j.rq.minw, j.rq.minh, j.rq.maxw, j.rq.maxh, kMaxPyrLevels + 1)))) return rc;
        if (!np->lv.empty()) {
            std::vector<ScaleSpec> specs;
            for (const PyrLevel &L : np->lv) specs.push_back(level_spec(np->P, L, c.ow, c.oh, 0));
            std::string err;
            if ((rc = np->det.build_custom(ctx, c, std::move(specs), false, err))) { ctx->set_error(err); return rc; }
            if ((rc = np->det.upload(ctx))) return rc;
            if ((rc = pyr_upload_levels(ctx, *np))) return rc;
        }
        pp = store_plan(ctx, key, std::move(np));
    }
    *out = pp;
    return NVCA_OK;
}

static int si_enqueue(nvca_ctx *ctx, DetectJob &j, int r0, int total)
{
    GeomPlan *pp = nullptr;
    int rc;
    if ((rc = si_plan(ctx, j, &pp))) return rc;
    j.q.phase = kJobFirstQueued; j.q.dp = nullptr;
    if (pp->lv.empty()) return NVCA_OK;
    PyrSource src;
    if ((rc = pyr_job_source(ctx, j, src)) || (rc = pyr_build(ctx, src, j.rq.cols, j.rq.rows, j.rq.nimg, pp, j.rq.casc->c.has_tilted))) return rc;
    j.q.cj = CascadeJob(); j.q.cj.r0 = r0; j.q.cj.n = j.rq.nimg; j.q.cj.total = total;
    if ((rc = cascade_enqueue(ctx, pp->det, pp->plane_total, pp->P, j.q.cj, nullptr, false))) return rc;
    j.q.gp = pp; pp->inflight++; j.q.dp = &pp->det;
    return NVCA_OK;
}

// plain scale-cascade scan (flags without SCALE_IMAGE / FIND_BIGGEST): FACE/kmsfacedetect.cpp:809-811, EYE/kmseyedetect.cpp:958-960
static int plain_enqueue(nvca_ctx *ctx, DetectJob &j, int r0, int total)
{
    GeomPlan *gp = nullptr;
    int rc;
    if ((rc = get_face_plan(ctx, j.rq.casc, j.rq.cols, j.rq.rows, j.rq.stride, 1, j.rq.cols, j.rq.rows, j.rq.sf, j.rq.minw, j.rq.minh, j.rq.maxw, j.rq.maxh, &gp))) return rc;
    const int nimg = j.rq.nimg;
    if ((rc = ensure_ws(ctx, gp->g, nimg))) return rc;
    PreGeom g = gp->g;
    const uint8_t *src = nullptr;
    size_t in_place_slot = 0;
    if (job_images_in_place(j, &in_place_slot) && j.rq.stride % 4 == 0 && ((uintptr_t)j.rq.img[0] & 3) == 0 && in_place_slot % 4 == 0) {
        src = (const uint8_t *)j.rq.img[0]; g.gpitch = j.rq.stride; g.gray_slot = in_place_slot;      // the integral kernels read rows in 4-byte words
    } else
        for (int k = 0; k < nimg; k++)
            if ((rc = stage_2d(ctx, ctx->ws->ln().gray.as<uint8_t>() + gp->g.gray_slot * k, gp->g.gpitch, j.rq.img[k], j.rq.stride, j.rq.cols, j.rq.rows, j.rq.mem))) return rc;
    run_integral(ctx, g, nullptr, nimg, src);
    if (j.rq.casc->c.has_tilted && (rc = run_tilted(ctx, g, nullptr, nimg, src))) return rc;
    j.q.gthr = (!j.rq.raw_only && j.rq.min_neighbors != 0) ? std::max(j.rq.min_neighbors, 1) : 0;
    j.q.cj = CascadeJob(); j.q.cj.r0 = r0; j.q.cj.n = nimg; j.q.cj.total = total;
    const std::vector<int> gthrv(nimg, j.q.gthr);
    if ((rc = cascade_enqueue(ctx, gp->det, gp->g.sum_slot, gp->g.spitch, j.q.cj, j.q.gthr ? gthrv.data() : nullptr, true))) return rc;
    j.q.gp = gp; gp->inflight++; j.q.dp = &gp->det; j.q.phase = kJobFirstQueued;
    return NVCA_OK;
}

// cvHaarDetectObjectsForROC with CV_HAAR_FIND_BIGGEST_OBJECT (NOSE/kmsnosedetect.cpp:870-873, MOUTH/kmsmouthdetect.cpp:870-873,
// EAR/kmseardetect.cpp:712-715): scale-cascade scan from the largest factor down; after the first grouped detection
// the scan narrows to a region of interest and a minimum size.  The serial loop changes its scan only once, so two launch
// sets do: (1) every step on its full grid (a cached plan per geometry), (2) once the region is known, the remaining steps
// on their narrowed grids.  FbSearch::replay() replays the serial logic on those results, step by step.
static int fb_stage_image(nvca_ctx *ctx, const DetectJob &j, PreGeom &g)
{
    make_geom(g, j.rq.cols, j.rq.rows, j.rq.stride, 1, j.rq.cols, j.rq.rows);
    int rc;
    if ((rc = ensure_ws(ctx, g, 1))) return rc;
    if ((rc = stage_2d(ctx, ctx->ws->ln().gray.p, g.gpitch, j.rq.img[0], j.rq.stride, j.rq.cols, j.rq.rows, j.rq.mem))) return rc;
    run_integral(ctx, g, nullptr, 1);
    if (j.rq.casc->c.has_tilted && (rc = run_tilted(ctx, g, nullptr, 1))) return rc;
    return NVCA_OK;
}

static int fb_enqueue_first(nvca_ctx *ctx, DetectJob &j, int r0, int total)
{
    const Cascade &c = j.rq.casc->c;
    const int cols = j.rq.cols, rows = j.rq.rows;
    PreGeom g; int rc;
    if ((rc = fb_stage_image(ctx, j, g))) return rc;
    j.fb.start(c.ow, c.oh, cols, rows, j.rq.sf, j.rq.minw, j.rq.minh, j.rq.maxw, j.rq.maxh);
    char key[256];
    snprintf(key, sizeof(key), "FB|%llu|%d|%d|%.17g|%d|%d|%d|%d", (unsigned long long)c.uid, cols, rows, j.rq.sf, j.rq.minw, j.rq.minh, j.rq.maxw, j.rq.maxh);
    GeomPlan *p1 = find_plan(ctx, key);
    if (!p1) {
        std::unique_ptr<GeomPlan> np(new GeomPlan());
        std::vector<ScaleSpec> specs;
        j.fb.first_set();
        np->fb_ladder = j.fb.ladder_of;
        for (size_t k = 0; k < j.fb.ladder_of.size(); k++) specs.push_back(fb_make_spec(j, g.spitch, j.fb.ladder[j.fb.ladder_of[k]], j.fb.grids[k]));
        if (!specs.empty()) {
            std::string err;
            if ((rc = np->det.build_custom(ctx, c, std::move(specs), false, err))) { ctx->set_error(err); return rc; }
            if ((rc = np->det.upload(ctx))) return rc;
        }
        p1 = store_plan(ctx, key, std::move(np));
    }
    j.q.phase = kJobFirstQueued; j.q.dp = nullptr;
    if (!p1->fb_ladder.empty()) {            // (steps the full-grid plan does not hold have nothing to scan)
        j.fb.ladder_of = p1->fb_ladder;
        j.q.cj = CascadeJob(); j.q.cj.r0 = r0; j.q.cj.n = 1; j.q.cj.total = total;
        if ((rc = cascade_enqueue(ctx, p1->det, g.sum_slot, g.spitch, j.q.cj, nullptr, false))) return rc;
        j.q.gp = p1; p1->inflight++; j.q.dp = &p1->det;
    }
    return NVCA_OK;
}

// the narrowed launch set: this step and all later ones on their narrowed grids (nothing changes the scan any more)
static int fb_enqueue_narrowed(nvca_ctx *ctx, DetectJob &j, int r0, int total)
{
    PreGeom g; int rc;
    if ((rc = fb_stage_image(ctx, j, g))) return rc;         // the planes have served other jobs in between
    j.q.cj = CascadeJob(); j.q.cj.r0 = r0; j.q.cj.n = 1; j.q.cj.total = total;
    if ((rc = cascade_enqueue(ctx, *j.q.own, g.sum_slot, g.spitch, j.q.cj, nullptr, false))) return rc;
    j.q.dp = j.q.own.get();
    return NVCA_OK;
}

// the plan of the narrowed set the replay asked for: the steps of fb.ladder_of on their narrowed grids
static int fb_plan_narrowed(nvca_ctx *ctx, DetectJob &j)
{
    const int spitch = (int)round_up(j.rq.cols + 1, 8);
    std::vector<ScaleSpec> specs;
    for (size_t k = 0; k < j.fb.ladder_of.size(); k++) specs.push_back(fb_make_spec(j, spitch, j.fb.ladder[j.fb.ladder_of[k]], j.fb.grids[k]));
    j.q.own.reset(new DetectPlan()); std::string err;
    int rc;
    if ((rc = j.q.own->build_custom(ctx, j.rq.casc->c, std::move(specs), false, err))) { ctx->set_error(err); return rc < 0 ? rc : NVCA_ERR_ARG; }
    return j.q.own->upload(ctx);
}

// queue the job's next launch set; its candidates go to result slots [r0, r0 + slots()) of `total`
int detect_job_enqueue(nvca_ctx *ctx, DetectJob &j, int r0, int total)
{
    (void)hipSetDevice(ctx->device);
    if (j.q.phase == kJobNew) {
        for (int k = 0; k < kJobImages; k++) j.out[k].clear();
        if (j.rq.kind == kJobBiggest) return fb_enqueue_first(ctx, j, r0, total);
        if (j.rq.kind == kJobScaleImage) return si_enqueue(ctx, j, r0, total);
        if (j.rq.kind == kJobLbp) return lbp_enqueue(ctx, j, r0, total);
        return plain_enqueue(ctx, j, r0, total);
    }
    if (j.q.phase == kJobNarrowedQueued) return fb_enqueue_narrowed(ctx, j, r0, total);
    return NVCA_OK;
}

// after the stream has drained: consume the queued set's results.  kJobDone: the call is complete (out[] holds the objects);
// kJobNarrowedQueued: it needs another set (enqueue again)
int detect_job_advance(nvca_ctx *ctx, DetectJob &j)
{
    int rc = NVCA_OK;
    std::vector<std::vector<nvca_rect>> raw;
    std::vector<char> grouped;
    std::vector<std::vector<int>> sc;
    std::vector<std::vector<LevelRec>> recs;
    bool have = j.q.dp != nullptr;
    const bool was_fused = j.sm.fused;
    if (j.sm.fused) {
        if ((rc = roi_job_candidates(ctx, j, raw, grouped, sc))) return rc;
        have = true;
    } else
    if (j.q.dp) rc = cascade_collect(ctx, *j.q.dp, j.q.cj, raw, j.rq.kind == kJobPlain ? &grouped : nullptr, j.rq.kind == kJobBiggest ? &sc : nullptr, j.rq.levels ? &recs : nullptr);
    if (j.q.gp) { j.q.gp->inflight--; j.q.gp = nullptr; }
    if (rc == NVCA_ERR_OVERFLOW && j.q.regrown < 2 && ctx->hit_cap_wanted > ctx->hit_cap) {
        // More raw candidates than the lists hold.  OpenCV has no such limit (and a FIND_BIGGEST search would have stopped at
        // its first object long before: NOSE/kmsnosedetect.cpp:870-873, MOUTH/kmsmouthdetect.cpp:870-873, EAR/kmseardetect.cpp:712-715),
        // so the call must answer, not fail: the same launch set runs once more with lists of exactly the size the exact count
        // asks for (run_detect_jobs applies hit_cap_wanted before the next round), and the serial logic is replayed on the
        // complete candidate lists -- the result is what the reference returns.
        j.q.regrown++; j.q.dp = nullptr;
        if (j.q.phase == kJobFirstQueued) j.q.phase = kJobNew;              // the first (or only) set again; a narrowed FIND_BIGGEST set stays in phase 2
        return NVCA_OK;
    }
    if (rc) { j.q.phase = kJobDone; return rc; }
    if (j.rq.kind == kJobPlain) {
        if (have)
            for (int k = 0; k < j.rq.nimg; k++) {
                if (j.q.gthr && !grouped[k]) group_rectangles(raw[k], j.q.gthr, 0.2);
                j.out[k].swap(raw[k]);
            }
        j.q.phase = kJobDone;
    } else if (j.rq.kind == kJobLbp && j.rq.levels) {
        // detectMultiScale with outputRejectLevels: the triples in canonical order, grouped by the weighted form
        j.out_levels.clear(); j.out_weights.clear();
        if (have) {
            for (const LevelRec &r : recs[0]) { j.out_levels.push_back(r.level); j.out_weights.push_back(r.weight); }
            j.out[0].swap(raw[0]);
            if (!j.rq.raw_only && !group_rectangles_levels(j.out[0], j.out_levels, j.out_weights, j.rq.min_neighbors, 0.2)) {
                ctx->set_error("internal: a levels job's records do not match its candidates"); j.q.phase = kJobDone; return NVCA_ERR_INTERNAL;
            }
        }
        j.q.phase = kJobDone;
    } else if (j.rq.kind == kJobScaleImage || j.rq.kind == kJobLbp) {
        if (have) { if (!j.rq.raw_only) group_all(raw, j.rq.min_neighbors); for (int k = 0; k < j.rq.nimg; k++) j.out[k].swap(raw[k]); }
        j.q.phase = kJobDone;
    } else {
        if (have) {
            // the large-image path numbers a candidate by its scale inside the plan, the small-image path by its ladder step directly
            if (!j.fb.take(raw[0], sc[0], was_fused)) { ctx->set_error("internal: candidate of an unknown ladder step"); j.q.phase = kJobDone; return NVCA_ERR_INTERNAL; }
        }
        j.q.dp = nullptr;
        if (j.fb.replay(j.rq.min_neighbors, (j.rq.flags & NVCA_HAAR_DO_ROUGH_SEARCH) != 0, j.out[0])) j.q.phase = kJobDone;
        else {
            // the narrowed set: on the small-image path the grids go into the next round's launch as they are (roi_batch.cpp), otherwise into a plan of this call
            if (!j.sm.small && (rc = fb_plan_narrowed(ctx, j))) { j.q.phase = kJobDone; return rc; }
            j.q.phase = kJobNarrowedQueued;
        }
    }
    j.q.dp = nullptr;
    return NVCA_OK;
}

} // namespace nvca

nvca::DetectJob *nvca::detect_job_new() { return new (std::nothrow) DetectJob(); }
void nvca::detect_job_free(DetectJob *j) { delete j; }
const std::vector<nvca_rect> &nvca::detect_job_out(const DetectJob *j, int k) { return j->out[k]; }
int nvca::detect_job_add_image(DetectJob *j, const void *image)
{
    if (j->rq.kind == kJobBiggest || j->q.phase != kJobNew || j->rq.nimg >= kJobImages) return -1;
    j->rq.img[j->rq.nimg] = image;
    return j->rq.nimg++;
}

// fill in a job from detectMultiScale's arguments (flags decide the kind); NVCA_ERR_ARG for bad arguments
int nvca::make_detect_job(nvca_ctx *ctx, DetectJob &j, const nvca_cascade *casc, const void *gray, int w, int h, int stride, int mem,
                          double sf, int min_neighbors, int flags, int minw, int minh, int maxw, int maxh, bool raw_only)
{
    if (check_img(ctx, gray, w, h, stride, 1, mem) || !casc || !(sf > 1.0)) return NVCA_ERR_ARG;
    if (maxw == 0 || maxh == 0) { maxw = w; maxh = h; }
    j = DetectJob();
    j.rq.casc = casc; j.rq.img[0] = gray; j.rq.nimg = 1; j.rq.cols = w; j.rq.rows = h; j.rq.stride = stride; j.rq.mem = mem;
    j.rq.sf = sf; j.rq.min_neighbors = min_neighbors; j.rq.minw = minw; j.rq.minh = minh; j.rq.maxw = maxw; j.rq.maxh = maxh; j.rq.raw_only = raw_only;
    if (casc->new_format()) j.rq.kind = kJobLbp;           // the new-format scan ignores flags (cascadedetect.cpp)
    else if (flags & NVCA_HAAR_FIND_BIGGEST_OBJECT) {
        flags &= ~(NVCA_HAAR_SCALE_IMAGE | NVCA_HAAR_DO_CANNY_PRUNING);
        if (raw_only) return NVCA_ERR_ARG;
        j.rq.kind = kJobBiggest;
    } else if (flags & NVCA_HAAR_SCALE_IMAGE) j.rq.kind = kJobScaleImage;
    else j.rq.kind = kJobPlain;
    j.rq.flags = flags;
    j.rq.small_route = casc->format == NVCA_CASCADE_HAAR_NEW && casc->small_route.load(std::memory_order_relaxed) != 0;
    return NVCA_OK;
}
