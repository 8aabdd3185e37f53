// roi_batch.cpp -- the small-image path of detectMultiScale: every small job of a round in one k_roi launch (kernels_roi.hip) --
// the jobs on new-format LBP cascades in one k_roi_lbp launch beside it (kernels_roi_lbp.hip), the jobs on new-format HAAR cascades
// that were opted in (nvca_cascade_set_small_route) in one k_roi_hnew launch (kernels_roi_hnew.hip) --, and their candidates handed
// back to the jobs.
#include "host_state.h"
#include "hnew_roi_tables.h"
#include <cstring>
#include <algorithm>

using namespace nvca;

namespace nvca {

// ---- small images: one launch for every such job of a round (kernels_roi.hip) -----------------------------------------------
// A job qualifies when its image's integral pair fits the workgroup's LDS, the cascade is a stump cascade with upright
// features, and the ladder fits the candidate key.  No plan is built: the launch gets, per job, a handful of step records
// (the cached stump table of the step's factor, the variance rectangle, the grid limits) -- so a face region of a size never
// seen before costs no table work, and all regions of all streams of a round share ONE launch.
static constexpr int kRoiMaxWords = 14848;          // (cols + 1) * (rows + 2) words per plane: the part detectors' 160 x 90 face-pass image still fits (two planes + queues + a level image = 157 KB of the 160 KB of LDS)
bool roi_eligible(const nvca_ctx *ctx, const DetectJob &j, int njobs_in_round)
{
    if (!ctx->sw.roi || j.rq.levels) return false;          // (a levels job always takes the large-image evaluator: k_roi_lbp has no last-stages launch)
    if (j.rq.kind == kJobLbp && j.rq.casc->format != NVCA_CASCADE_LBP) {
        // a new-format HAAR cascade: neither k_roi nor k_roi_lbp evaluates it.  One that was opted in when the job was built takes
        // k_roi_hnew under the LBP branch's rules, with its own LDS bound (kRoiHnewMaxBytes, hnew_roi_tables.h)
        if (!j.rq.small_route || j.rq.nimg != 1 || j.rq.image_axis || !hnew_roi_fits_lds(j.rq.cols, j.rq.rows)) return false;
        return j.rq.mem == NVCA_MEM_DEVICE || njobs_in_round == 1;              // a host image is staged in the lane's one gray buffer
    }
    if (j.rq.kind == kJobLbp) {
        // a new-format LBP cascade (its Haar model is empty): ONE image whose working set fits k_roi_lbp's LDS (kRoiLbpMaxBytes,
        // lbp_roi_tables.h); a job of several images, and every job of the _batch entry points, keeps the image axis of the
        // large-image evaluator
        if (j.rq.nimg != 1 || j.rq.image_axis || !lbp_roi_fits_lds(j.rq.cols, j.rq.rows)) return false;
        return j.rq.mem == NVCA_MEM_DEVICE || njobs_in_round == 1;              // a host image is staged in the lane's one gray buffer
    }
    const Cascade &c = j.rq.casc->c;
    if (!c.stump_based || c.has_tilted || (j.rq.nimg != 1 && j.rq.mem != NVCA_MEM_DEVICE)) return false;
    if ((long long)(j.rq.cols + 1) * (j.rq.rows + 2) > kRoiMaxWords || j.rq.cols < 1 || j.rq.rows < 1) return false;
    if (j.rq.mem != NVCA_MEM_DEVICE && njobs_in_round != 1) return false;       // a host image is staged in the lane's one gray buffer
    return true;
}
static const StageRec *roi_stage_recs(nvca_ctx *ctx, const Cascade &c)
{
    auto it = ctx->roi_stage_recs.find(c.uid);
    if (it != ctx->roi_stage_recs.end()) return it->second->as<StageRec>();
    std::vector<StageRec> st; build_stage_recs(c, st);
    std::unique_ptr<DevBuf> d(new DevBuf());
    if (d->ensure(st.size() * sizeof(StageRec) + 8) || hipMemcpy(d->p, st.data(), st.size() * sizeof(StageRec), hipMemcpyHostToDevice) != hipSuccess) {
        d->release(); ctx->set_error("allocation failed (stage records)"); return nullptr;
    }
    const StageRec *p = d->as<StageRec>();
    ctx->roi_stage_recs[c.uid] = d.release();
    return p;
}
// the cascade's table for k_roi_lbp (lbp_roi_tables.cpp), cached per context and cascade beside the Haar cascades' stage records
static const StageRec *roi_lbp_recs(nvca_ctx *ctx, const nvca_cascade *casc)
{
    auto it = ctx->roi_stage_recs.find(casc->c.uid);
    if (it != ctx->roi_stage_recs.end()) return it->second->as<StageRec>();
    std::vector<unsigned char> blob; build_lbp_roi_table(casc->lbp, blob);
    std::unique_ptr<DevBuf> d(new DevBuf());
    if (d->ensure(blob.size()) || hipMemcpy(d->p, blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess) {
        d->release(); ctx->set_error("allocation failed (LBP cascade records)"); return nullptr;
    }
    const StageRec *p = d->as<StageRec>();
    ctx->roi_stage_recs[casc->c.uid] = d.release();
    return p;
}
// ... and for k_roi_hnew (hnew_roi_tables.cpp), in the same cache: a cascade has one format
static const StageRec *roi_hnew_recs(nvca_ctx *ctx, const nvca_cascade *casc)
{
    auto it = ctx->roi_stage_recs.find(casc->c.uid);
    if (it != ctx->roi_stage_recs.end()) return it->second->as<StageRec>();
    std::vector<unsigned char> blob; build_hnew_roi_table(casc->hnew, blob);
    std::unique_ptr<DevBuf> d(new DevBuf());
    if (d->ensure(blob.size()) || hipMemcpy(d->p, blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess) {
        d->release(); ctx->set_error("allocation failed (HAAR cascade records)"); return nullptr;
    }
    const StageRec *p = d->as<StageRec>();
    ctx->roi_stage_recs[casc->c.uid] = d.release();
    return p;
}
static ScaleTable *roi_table(nvca_ctx *ctx, RoiBatch &rb, const Cascade &c, double factor)
{
    ScaleTable *t = get_scale_table(ctx, c, factor);
    if (t) { t->refs++; rb.held.push_back(t); }
    return t;
}
static void roi_step_common(RoiStep &st, const ScaleTable &t)
{
    memset(&st, 0, sizeof(st));
    st.trecs = t.dev.as<TStumpRec>(); st.ex = t.ex; st.ey = t.ey; st.ew = t.ew; st.eh = t.eh; st.inv_area = t.inv_area; st.step = 1;
}
// returns NVCA_OK with j.sm.fused set when the job's next set went into the batch, NVCA_OK with j.sm.fused clear when it has to take
// the large-image path after all (too many steps), or an error
int roi_add_job(nvca_ctx *ctx, RoiBatch &rb, DetectJob &j)
{
    const Cascade &c = j.rq.casc->c;
    const int cols = j.rq.cols, rows = j.rq.rows;
    j.sm.fused = false;
    const bool lbp = j.rq.kind == kJobLbp, hnew = lbp && j.rq.casc->format == NVCA_CASCADE_HAAR_NEW;      // (lbp: either new-format evaluator)
    const StageRec *d_stages = hnew ? roi_hnew_recs(ctx, j.rq.casc) : lbp ? roi_lbp_recs(ctx, j.rq.casc) : roi_stage_recs(ctx, c);
    if (!d_stages) return NVCA_ERR_NOMEM;
    std::vector<RoiStep> steps; std::vector<DetectJob::RoiStepInfo> info; std::vector<unsigned char> tabs;
    const size_t tab0 = rb.tabs.size();
    int lev_bytes = 0, lbp_plane_words = 0;
    bool fits = true;
    const bool dense = j.rq.kind == kJobBiggest && j.q.phase == kJobNew && ctx->sw.fb_dense && j.rq.nimg == 1;
    std::vector<DetectJob::RejInfo> rej; size_t rej_local = 0;
    if (j.q.phase == kJobNew) for (int k = 0; k < kJobImages; k++) j.out[k].clear();
    if (lbp) {
        // the levels of detectMultiScale on a new-format cascade, each with its cv::resize tables (lbp_roi_tables.cpp); a candidate maps
        // to its rectangle as a CV_HAAR_SCALE_IMAGE level's does: (cvRound(x f), cvRound(y f), cvRound(ow f), cvRound(oh f))
        LbpRoiSteps ls;
        build_lbp_roi_steps(c.ow, c.oh, cols, rows, j.rq.sf, j.rq.minw, j.rq.minh, j.rq.maxw, j.rq.maxh, tab0, ls);      // (c holds the window of either model)
        fits = ls.fits;
        // HaarEvaluator::setImage's normrect (1, 1, ow - 2, oh - 2), in the record's variance rectangle
        if (hnew) for (RoiStep &st : ls.steps) { st.ex = 1; st.ey = 1; st.ew = c.ow - 2; st.eh = c.oh - 2; }
        steps.swap(ls.steps); tabs.swap(ls.tabs); lev_bytes = ls.lev_bytes; lbp_plane_words = ls.plane_words;
        for (const LbpRoiLevel &l : ls.info) info.push_back(DetectJob::RoiStepInfo{0., l.factor, l.winw, l.winh, -1});
        j.q.phase = kJobFirstQueued;
    } else if (j.rq.kind == kJobScaleImage) {
        // the pyramid levels of si_plan, each with its cv::resize tables.  (No cap on their number here: with more of them than the key
        // holds the job takes the large-image path, below)
        ScaleTable *t1 = nullptr;
        for (const SiLevel &sl : si_levels(c.ow, c.oh, cols, rows, j.rq.sf, j.rq.minw, j.rq.minh, j.rq.maxw, j.rq.maxh, (size_t)-1)) {
            const double factor = sl.factor;
            const int szw = sl.szw, szh = sl.szh, winw = sl.winw, winh = sl.winh;
            if (!t1 && !(t1 = roi_table(ctx, rb, c, 1.))) return NVCA_ERR_NOMEM;
            RoiStep st; roi_step_common(st, *t1);
            st.szw = szw; st.szh = szh; st.step = level_step(factor); st.startX = 0; st.endX = szw - c.ow; st.startY = 0; st.endY = szh - c.oh;
            if (st.endX <= 0 || st.endY <= 0) continue;
            ResizeTab tab; build_resize_tab(cols, rows, szw, szh, tab);
            st.mode = tab.mode; st.xmax = tab.xmax;
            auto put = [&](const void *p, size_t n) { const size_t at = (tab0 + tabs.size() + 15) & ~(size_t)15; tabs.resize(at - tab0 + n); if (n) memcpy(tabs.data() + at - tab0, p, n); return (int)at; };
            st.xofs_off = put(tab.xofs.data(), tab.xofs.size() * 4); st.yofs_off = put(tab.yofs.data(), tab.yofs.size() * 4);
            st.ialpha_off = put(tab.ialpha.data(), tab.ialpha.size() * 2); st.ibeta_off = put(tab.ibeta.data(), tab.ibeta.size() * 2);
            steps.push_back(st); info.push_back(DetectJob::RoiStepInfo{0., factor, winw, winh, -1});
            lev_bytes = std::max(lev_bytes, szw * szh);
        }
        j.q.phase = kJobFirstQueued;
    } else if (j.rq.kind == kJobPlain) {
        std::vector<double> factors;
        scale_grid(c.ow, c.oh, cols, rows, j.rq.sf, j.rq.minw, j.rq.minh, j.rq.maxw, j.rq.maxh, false, factors);
        for (double factor : factors) {
            const double ystep = std::max(2., factor);
            ScaleTable *t = roi_table(ctx, rb, c, factor);
            if (!t) return NVCA_ERR_NOMEM;
            RoiStep st; roi_step_common(st, *t);
            ScanGrid sg;
            if (!full_grid(cols, rows, ystep, t->winw, t->winh, sg) || !roi_grid(sg, ystep, st)) continue;
            steps.push_back(st); info.push_back(DetectJob::RoiStepInfo{ystep, 0., t->winw, t->winh, -1});
        }
        j.q.gthr = (!j.rq.raw_only && j.rq.min_neighbors != 0) ? std::max(j.rq.min_neighbors, 1) : 0;
        j.q.phase = kJobFirstQueued;
    } else {
        // the first set (every step of the call's sizes on its full grid) or the narrowed set the replay asked for: fb.ladder_of on fb.grids
        if (j.q.phase == kJobNew) {
            j.fb.start(c.ow, c.oh, cols, rows, j.rq.sf, j.rq.minw, j.rq.minh, j.rq.maxw, j.rq.maxh);
            j.fb.first_set();
            j.q.phase = kJobFirstQueued;
        }
        for (size_t k = 0; k < j.fb.ladder_of.size(); k++) {
            const int li = j.fb.ladder_of[k];
            const FbStep &fs = j.fb.ladder[li];
            ScaleTable *t = roi_table(ctx, rb, c, fs.factor);
            if (!t) return NVCA_ERR_NOMEM;
            RoiStep st; roi_step_common(st, *t);
            if (!roi_grid(j.fb.grids[k], fs.ystep, st)) continue;
            if (dense) {                     // every stage-0 passer of the full grid + the grid's reject bits: a narrowed re-scan is replayed on the host
                st.adaptive = 2; st.rej_wpr = (st.endX + 63) / 64; st.rej_off = (int)(rb.rej_words + rej_local);
                rej.push_back(DetectJob::RejInfo{st.rej_off, st.rej_wpr, st.endX, st.endY});
                rej_local += (size_t)st.rej_wpr * st.endY;
            }
            steps.push_back(st); info.push_back(DetectJob::RoiStepInfo{fs.ystep, 0., fs.winw, fs.winh, li});
        }
    }
    // the key holds 6 bits of step; a step with more windows than the queues hold goes out as bands of whole rows, one workgroup per
    // band instead of one per step walking its bands one after the other (the largest pyramid level of a 160 x 90 face pass is 10 k
    // windows: alone it set the length of the whole launch).  Every band builds the integral planes for itself.
    fits = fits && steps.size() <= 63;
    if (!roi_split_bands(steps)) fits = false;
    if (!fits && j.sm.roi_prev_phase == kJobNarrowedQueued) { ctx->set_error("internal: a narrowed search outgrew the small-image path"); return NVCA_ERR_INTERNAL; }   // (its full grids fitted)
    if (!fits) { j.q.phase = (JobPhase)j.sm.roi_prev_phase; return NVCA_OK; }       // this one takes the large-image path
    j.sm.fused = true; j.sm.rinfo.swap(info); j.q.dp = nullptr;
    j.sm.dense = dense && !rej.empty(); j.sm.rej_info.swap(rej);
    if (j.sm.dense) rb.rej_words += rej_local;
    for (int k = 0; k < kJobImages; k++) j.sm.rkeys[k].clear();
    if (steps.empty()) return NVCA_OK;                               // nothing to scan: the job completes with what it has
    rb.tabs.insert(rb.tabs.end(), tabs.begin(), tabs.end());
    for (int k = 0; k < j.rq.nimg; k++) {            // every image of the job: its own records (the steps name their image), the same tables
        RoiJobDev d; memset(&d, 0, sizeof(d));
        d.w = cols; d.h = rows; d.stride = j.rq.stride; d.img = (const uint8_t *)j.rq.img[k];
        if (j.rq.mem != NVCA_MEM_DEVICE) {
            PreGeom g; make_geom(g, cols, rows, j.rq.stride, 1, cols, rows);
            int rc;
            if ((rc = ensure_ws(ctx, g, 1))) return rc;
            if ((rc = stage_2d(ctx, ctx->ws->ln().gray.p, g.gpitch, j.rq.img[0], j.rq.stride, cols, rows, j.rq.mem))) return rc;
            d.img = ctx->ws->ln().gray.as<uint8_t>(); d.stride = g.gpitch;
        }
        std::vector<RoiStep> &all = hnew ? rb.hnew_steps : lbp ? rb.lbp_steps : rb.steps;        // (k_roi_lbp's and k_roi_hnew's records apart: each kernel is launched on its own)
        d.first_step = (int)all.size(); d.nsteps = (int)steps.size(); d.scale_image = hnew ? 3 : lbp ? 2 : j.rq.kind == kJobScaleImage;
        d.stages = d_stages; d.nstages = hnew ? (int)j.rq.casc->hnew.stages.size() : lbp ? (int)j.rq.casc->lbp.stages.size() : (int)c.stages.size(); d.pair_policy = ctx->policy == NVCA_SUM_F32PAIR; d.slot = (int)rb.jobs.size();
        for (RoiStep &st : steps) st.job = d.slot;
        all.insert(all.end(), steps.begin(), steps.end());
        rb.jobs.push_back(d); rb.owners.push_back(&j); rb.owner_img.push_back(k);
    }
    if (hnew) rb.hnew_plane_words = std::max(rb.hnew_plane_words, (lbp_plane_words + 3) & ~3);
    else if (lbp) { rb.lbp_plane_words = std::max(rb.lbp_plane_words, (lbp_plane_words + 3) & ~3); rb.lbp_lev_bytes = std::max(rb.lbp_lev_bytes, lev_bytes); }
    else { rb.plane_words = std::max(rb.plane_words, (cols + 1) * (rows + 2)); rb.lev_bytes = std::max(rb.lev_bytes, lev_bytes); }
    return NVCA_OK;
}
// upload the round's tables and launch k_roi (the Haar jobs' steps), k_roi_lbp (the LBP jobs') and k_roi_hnew (the opted-in new-format
// HAAR jobs') on the current lane
int roi_launch(nvca_ctx *ctx, RoiBatch &rb, bool full_cap)
{
    const int nj = (int)rb.jobs.size();
    const size_t jb = (size_t)nj * sizeof(RoiJobDev), sb = rb.steps.size() * sizeof(RoiStep), lb = rb.lbp_steps.size() * sizeof(RoiStep),
                 hb = rb.hnew_steps.size() * sizeof(RoiStep);
    const size_t o_steps = (jb + 255) & ~(size_t)255, o_lsteps = (o_steps + sb + 255) & ~(size_t)255, o_hsteps = (o_lsteps + lb + 255) & ~(size_t)255,
                 o_tabs = (o_hsteps + hb + 255) & ~(size_t)255,
                 total = o_tabs + rb.tabs.size() + 64;
    // the list starts at a quarter of a million candidates for the whole launch however many jobs share it; a launch that
    // overflows it is queued again with the exact size (run_detect_jobs raises hit_cap for the rest of the call)
    const long long want = (long long)ctx->hit_cap * nj;
    rb.cap = (unsigned)std::min<long long>(want, full_cap ? (1ll << 26) : (1ll << 18));
    const size_t first = std::min<size_t>(rb.cap, std::max<size_t>(8192, ctx->roi_first_hint));
    rb.first = first;
    if (ctx->rbuf().tables.ensure(total) || ctx->rbuf().h_tables.ensure(total) || ctx->rbuf().hits.ensure(((size_t)rb.cap + 1) * 8) || ctx->rbuf().h_hits.ensure(((size_t)rb.cap + 1) * 8) ||
        ctx->rbuf().rej.ensure((rb.rej_words + 1) * 8) || ctx->rbuf().h_rej.ensure((rb.rej_words + 1) * 8)) {
        ctx->set_error("allocation failed (small-image detector)"); return NVCA_ERR_NOMEM;
    }
    unsigned char *h = ctx->rbuf().h_tables.as<unsigned char>();
    memcpy(h, rb.jobs.data(), jb);
    if (sb) memcpy(h + o_steps, rb.steps.data(), sb);
    if (lb) memcpy(h + o_lsteps, rb.lbp_steps.data(), lb);
    if (hb) memcpy(h + o_hsteps, rb.hnew_steps.data(), hb);
    if (!rb.tabs.empty()) memcpy(h + o_tabs, rb.tabs.data(), rb.tabs.size());
    NVCA_HIP_CHECK(ctx, hipMemcpyAsync(ctx->rbuf().tables.p, h, total - 64, hipMemcpyHostToDevice, ctx->cs()));
    NVCA_HIP_CHECK(ctx, hipMemsetAsync(ctx->rbuf().hits.p, 0, sizeof(unsigned long long), ctx->cs()));
    const int lds = rb.plane_words * 8 + kRoiMaxWin * (8 + 2 + 2) + 16 + ((rb.lev_bytes + 15) & ~15) + 64;      // k_roi's carve-up
    const int lbp_lds = roi_lbp_lds_bytes(rb.lbp_plane_words, rb.lbp_lev_bytes);                                 // k_roi_lbp's
    const int hnew_lds = roi_hnew_lds_bytes(rb.hnew_plane_words);                                                // k_roi_hnew's
    if (const int e = hb ? roi_hnew_grant_lds(hnew_lds) : 0) { ctx->set_error(std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString((hipError_t)e)); return NVCA_ERR_HIP; }
    if (const int e = sb ? roi_grant_lds(lds) : 0) { ctx->set_error(std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString((hipError_t)e)); return NVCA_ERR_HIP; }
    if (const int e = lb ? roi_lbp_grant_lds(lbp_lds) : 0) { ctx->set_error(std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString((hipError_t)e)); return NVCA_ERR_HIP; }
    const unsigned char *d = ctx->rbuf().tables.as<unsigned char>();
    // the Haar jobs' steps, the LBP jobs' and the new-format HAAR jobs': three kernels on one lane, one job table, one candidate list, one wait
    { TimedLaunch t(ctx, NVCA_K_ROI);
      if (sb) launch_roi(ctx->cs(), (const RoiJobDev *)d, (int)rb.steps.size(), (const RoiStep *)(d + o_steps), d + o_tabs, ctx->rbuf().hits.as<unsigned long long>(), rb.cap, rb.plane_words, lds,
                 ctx->rbuf().rej.as<unsigned long long>());
      if (lb) launch_roi_lbp(ctx->cs(), (const RoiJobDev *)d, (int)rb.lbp_steps.size(), (const RoiStep *)(d + o_lsteps), d + o_tabs, ctx->rbuf().hits.as<unsigned long long>(), rb.cap,
                             rb.lbp_plane_words, lbp_lds);
      if (hb) launch_roi_hnew(ctx->cs(), (const RoiJobDev *)d, (int)rb.hnew_steps.size(), (const RoiStep *)(d + o_hsteps), d + o_tabs, ctx->rbuf().hits.as<unsigned long long>(), rb.cap,
                              rb.hnew_plane_words, hnew_lds); }
    if (rb.rej_words) NVCA_HIP_CHECK(ctx, hipMemcpyAsync(ctx->rbuf().h_rej.p, ctx->rbuf().rej.p, rb.rej_words * 8, hipMemcpyDeviceToHost, ctx->cs()));
    NVCA_LAUNCH_CHECK(ctx);
    NVCA_HIP_CHECK(ctx, hipMemcpyAsync(ctx->rbuf().h_hits.p, ctx->rbuf().hits.p, (first + 1) * 8, hipMemcpyDeviceToHost, ctx->cs()));
    return NVCA_OK;
}
// after the lane has drained: hand every job its candidates; NVCA_ERR_OVERFLOW (with hit_cap_wanted set) when the list was too short
int roi_collect(nvca_ctx *ctx, RoiBatch &rb)
{
    unsigned long long *hh = ctx->rbuf().h_hits.as<unsigned long long>();
    const unsigned long long total = hh[0];
    const int nj = (int)rb.jobs.size();
    if (total > rb.cap) {
        const unsigned long long per = (total + (unsigned long long)nj - 1) / (unsigned long long)nj + 64;
        if (per <= (unsigned long long)kMaxHitCap && (long long)per > ctx->hit_cap_wanted) ctx->hit_cap_wanted = (int)per;
        ctx->set_error("raw candidate capacity exceeded (nvca_ctx_set_hit_capacity)");
        return NVCA_ERR_OVERFLOW;
    }
    // the list's head came back with the launch; how much of it to fetch that way next time follows the recent rounds (a second
    // copy is a second wait)
    ctx->roi_first_hint = std::max<size_t>((size_t)(total + total / 4), ctx->roi_first_hint - ctx->roi_first_hint / 16);
    const size_t first = rb.first;
    if (total > first) {
        NVCA_HIP_CHECK(ctx, hipMemcpyAsync(hh + 1 + first, ctx->rbuf().hits.as<unsigned long long>() + 1 + first, (total - first) * 8, hipMemcpyDeviceToHost, ctx->cs()));
        NVCA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->cs()));
    }
    // the dense jobs' reject bits: per ladder step of the job (FbSearch)
    for (DetectJob *o : rb.owners) {
        if (!o->sm.dense) continue;
        const unsigned long long *hr = ctx->rbuf().h_rej.as<unsigned long long>();
        o->fb.dense_begin();
        for (size_t k = 0; k < o->sm.rej_info.size() && k < o->sm.rinfo.size(); k++) {
            const DetectJob::RejInfo &ri = o->sm.rej_info[k];
            const int li = o->sm.rinfo[k].ladder;
            if (li < 0 || (size_t)li >= o->fb.ladder.size() || (size_t)ri.off + (size_t)ri.wpr * ri.ny > rb.rej_words) { ctx->set_error("internal: reject bitmap of an unknown ladder step"); return NVCA_ERR_INTERNAL; }
            o->fb.dense_step((size_t)li, hr + ri.off, ri.wpr, ri.ny);
        }
    }
    // (the list is in the order the workgroups appended: every job sorts its own keys into the serial order when it advances)
    for (unsigned long long i = 0; i < total; i++) {
        const unsigned long long slot = hh[1 + i] >> 32;
        const unsigned key = (unsigned)hh[1 + i];
        if (slot >= (unsigned long long)nj || (key >> 26) >= rb.owners[slot]->sm.rinfo.size()) {
            ctx->set_error("internal: candidate of an unknown job / step (device result rejected)"); return NVCA_ERR_INTERNAL;
        }
        rb.owners[slot]->sm.rkeys[rb.owner_img[slot]].push_back(key);
    }
    return NVCA_OK;
}
// candidates of the round's k_roi launch, sorted into the serial order (step, row, column) -> rectangle
int roi_job_candidates(nvca_ctx *ctx, DetectJob &j, std::vector<std::vector<nvca_rect>> &raw, std::vector<char> &grouped, std::vector<std::vector<int>> &sc)
{
    raw.assign(j.rq.nimg, {}); sc.assign(j.rq.nimg, {}); grouped.assign(j.rq.nimg, 0);
    for (int k = 0; k < j.rq.nimg; k++) {
        std::sort(j.sm.rkeys[k].begin(), j.sm.rkeys[k].end());
        raw[k].reserve(j.sm.rkeys[k].size()); sc[k].reserve(j.sm.rkeys[k].size());
        for (unsigned key : j.sm.rkeys[k]) {
            const DetectJob::RoiStepInfo &ri = j.sm.rinfo[key >> 26];
            const int iy = (key >> 13) & 8191, ix = key & 8191;
            if (j.sm.dense && k == 0) {
                // a dense launch reports every window that passes the cascade; the serial walk of the FULL grid (start column 0) visits only some
                const int seen = j.fb.dense_candidate((size_t)ri.ladder, ix, iy);
                if (seen < 0) { ctx->set_error("internal: dense candidate outside its reject bitmap (device result rejected)"); j.q.phase = kJobDone; return NVCA_ERR_INTERNAL; }
                if (!seen) continue;
            }
            if (ri.out_factor != 0) raw[k].push_back(nvca_rect{cv_round(ix * ri.out_factor), cv_round(iy * ri.out_factor), ri.winw, ri.winh});
            else raw[k].push_back(nvca_rect{cv_round(ix * ri.ystep), cv_round(iy * ri.ystep), ri.winw, ri.winh});
            sc[k].push_back(ri.ladder);
        }
        j.sm.rkeys[k].clear();
    }
    j.sm.fused = false;
    return NVCA_OK;
}

} // namespace nvca
