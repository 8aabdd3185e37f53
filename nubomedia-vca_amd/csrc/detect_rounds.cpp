// detect_rounds.cpp -- rounds of detectMultiScale jobs that share one wait: every unfinished job of a set queues its next launch
// set (detect_job.cpp; the small images of a round go into one launch: roi_batch.cpp), the lanes are waited for once, every job is
// advanced.  The part detectors queue the face passes of every stream of a tick, then every ROI pass, with three synchronisations
// per tick instead of several per stream (part_call.cpp).
#include "host_state.h"
#include <cstdio>
#include <algorithm>
#include <atomic>
#include <new>

using namespace nvca;

namespace nvca {

// One round of a job set in two halves, so that a caller may leave a round queued and come back for it (part_call.cpp: a submitted part-detector
// batch keeps its face passes in flight while the batch before it is collected).  begin: every unfinished job queues its next launch
// set (small images: all in ONE k_roi launch); end: the lanes are waited for, the candidates handed out, every job advanced.
struct JobRound { RoiBatch rb; bool used[kLanes] = {false}; int rc = NVCA_OK; double t_queued = 0; int roi_regrown = 0; };
static int jobs_round_begin(nvca_ctx *ctx, DetectJob *const *jobs, int n, const int *lanes, int lane0, JobRound &R, bool *pending_out)
{
    const bool stats = ctx->sw.part_stats > 0;
    PartStats &ps = ctx->stats;
    if (ctx->hit_cap_wanted > ctx->hit_cap) ctx->hit_cap = ctx->hit_cap_wanted;      // a set overflowed in the last round: it runs again with room (this call only)
    int pending = 0;
    for (int i = 0; i < n; i++) if (jobs[i]->q.phase != kJobDone) pending++;
    if (!pending) { *pending_out = false; return NVCA_OK; }
    *pending_out = true;
    R.rc = NVCA_OK;
    for (bool &u : R.used) u = false;
    {
        PartStats::Timer t_enqueue(stats, ps.enqueue);
        // small images first: every such job of the round goes into ONE k_roi launch (no plan, no per-job launches)
        R.rb.reset();
        for (int i = 0; i < n && !R.rc; i++) {
            DetectJob &j = *jobs[i];
            if (j.q.phase == kJobDone) continue;
            if (j.q.phase == kJobNew && j.q.regrown == 0) j.sm.small = roi_eligible(ctx, j, n);
            if (!j.sm.small) continue;
            ctx->cur_lane = lanes ? lanes[i] : lane0;
            if (R.rb.jobs.empty()) R.rb.lane = ctx->cur_lane;
            j.sm.roi_prev_phase = j.q.phase;
            { PartStats::Timer t(stats, ps.add_jobs); R.rc = roi_add_job(ctx, R.rb, j); }
            if (stats) ps.small_jobs += 1;
            if (!R.rc && !j.sm.fused) j.sm.small = false;          // more ladder steps than the key holds: the large-image path takes it
            else R.used[ctx->cur_lane] = true;
        }
        int total = 0, r0 = 0;
        for (int i = 0; i < n; i++) if (jobs[i]->q.phase != kJobDone && !jobs[i]->sm.small) total += jobs[i]->slots();
        for (int i = 0; i < n && !R.rc; i++) {
            if (jobs[i]->q.phase == kJobDone || jobs[i]->sm.small) continue;
            ctx->cur_lane = lanes ? lanes[i] : lane0;
            R.used[ctx->cur_lane] = true;
            R.rc = detect_job_enqueue(ctx, *jobs[i], r0, total);
            r0 += jobs[i]->slots();
        }
        PartStats::Timer t_launch(stats, ps.launch);
        if (!R.rc && !R.rb.jobs.empty()) { ctx->cur_lane = R.rb.lane; R.used[R.rb.lane] = true; R.rc = roi_launch(ctx, R.rb, R.roi_regrown > 0); }
    }
    R.t_queued = stats ? mono_s() : 0;
    ctx->cur_lane = lane0;
    return NVCA_OK;          // (a failed enqueue is carried in R.rc: the round is still waited for and closed by jobs_round_end)
}
static int jobs_round_end(nvca_ctx *ctx, DetectJob *const *jobs, int n, const int *lanes, int lane0, JobRound &R)
{
    const bool stats = ctx->sw.part_stats > 0;
    PartStats &ps = ctx->stats;
    RoiBatch &rb = R.rb;
    int rc = R.rc;
    for (int l = 0; l < kLanes; l++) {
        if (!R.used[l]) continue;
        const hipError_t he = hipStreamSynchronize(ctx->lane_streams[l]);
        if (he != hipSuccess && !rc) { ctx->set_error(std::string("hipStreamSynchronize: ") + hipGetErrorString(he)); rc = NVCA_ERR_HIP; }
    }
    ctx->cur_lane = lane0;
    const double waited_s = stats ? mono_s() - R.t_queued : 0;
    ps.wait += waited_s;
    if (stats && !rb.jobs.empty() && n >= ctx->sw.part_stats) {
        int kinds[kJobKinds] = {0}, narrowed = 0;
        for (DetectJob *o : rb.owners) { kinds[o->rq.kind]++; if (o->sm.roi_prev_phase == kJobNarrowedQueued) narrowed++; }
        ps.report_round(rb.jobs.size(), kinds, narrowed, rb.steps.size() + rb.lbp_steps.size() + rb.hnew_steps.size(), waited_s);
    }
    PartStats::Timer t_advance(stats, ps.advance);
    PartStats::Timer t_collect(stats && !rc && !rb.jobs.empty(), ps.collect);
    drain_timer(ctx);
    bool roi_again = false;
    if (!rc && !rb.jobs.empty()) {
        ctx->cur_lane = rb.lane;
        const int r = roi_collect(ctx, rb);
        t_collect.stop();
        ctx->cur_lane = lane0;
        if (r == NVCA_ERR_OVERFLOW && R.roi_regrown < 2 && ctx->hit_cap_wanted > ctx->hit_cap) {
            // the round's candidate list was too short: its jobs are queued again, with room (see detect_job_advance)
            R.roi_regrown++; roi_again = true;
            if (stats) fprintf(stderr, "[nvca jobs] a small-image round overflowed its candidate list (cap %u for %zu jobs): queued again with %d per job\n", rb.cap, rb.jobs.size(), ctx->hit_cap_wanted);
            for (DetectJob *o : rb.owners) { o->q.phase = (JobPhase)o->sm.roi_prev_phase; o->sm.fused = false; for (int k = 0; k < kJobImages; k++) o->sm.rkeys[k].clear(); }
        } else if (r) rc = r;
    }
    // the small-path jobs' candidates are turned into rectangles, replayed (FIND_BIGGEST) and grouped job by job: independent
    // host work, shared with the context's helper threads (a job touches nothing but itself; set_error is locked)
    std::vector<DetectJob *> par;
    {
        PartStats::Timer t(stats, ps.advance_helpers);
        if (!rc && !roi_again)
            for (int i = 0; i < n; i++) if (jobs[i]->q.phase != kJobDone && jobs[i]->sm.fused) par.push_back(jobs[i]);
        if (par.size() >= 4) {
            // the jobs with the most candidates first: the helpers take indices in order, the long ones must not come last
            auto weight = [](const DetectJob *j) { size_t w = 0; for (int k = 0; k < j->rq.nimg; k++) w += j->sm.rkeys[k].size(); return w; };
            std::stable_sort(par.begin(), par.end(), [&](const DetectJob *x, const DetectJob *y) { return weight(x) > weight(y); });
            ensure_pool(ctx);
            struct Arg { nvca_ctx *ctx; DetectJob **jobs; std::atomic<int> rc; } arg{ctx, par.data(), {0}};
            work_pool_run(ctx->pool, (int)par.size(), [](void *a, int i) {
                Arg *g = (Arg *)a;
                int r;
                try { r = detect_job_advance(g->ctx, *g->jobs[i]); }
                catch (const std::bad_alloc &) { r = NVCA_ERR_NOMEM; }
                catch (...) { r = NVCA_ERR_INTERNAL; }
                if (r) { g->jobs[i]->q.phase = kJobDone; int z = 0; g->rc.compare_exchange_strong(z, r); }
            }, &arg);
            if (arg.rc.load()) rc = arg.rc.load();
            for (DetectJob *j : par) j->sm.roi_prev_phase = -1;          // handled
        }
    }
    {
        PartStats::Timer t(stats, ps.advance_serial);
        for (int i = 0; i < n; i++) {
            if (jobs[i]->q.phase == kJobDone) continue;
            if (rc) { if (jobs[i]->q.gp) { jobs[i]->q.gp->inflight--; jobs[i]->q.gp = nullptr; } jobs[i]->q.phase = kJobDone; continue; }
            if (roi_again && std::find(rb.owners.begin(), rb.owners.end(), jobs[i]) != rb.owners.end()) continue;
            if (par.size() >= 4 && jobs[i]->sm.roi_prev_phase == -1) { jobs[i]->sm.roi_prev_phase = 0; continue; }
            ctx->cur_lane = lanes ? lanes[i] : lane0;
            const int r = detect_job_advance(ctx, *jobs[i]);
            if (r) rc = r;
        }
        ctx->cur_lane = lane0;
    }
    if (rc)
        for (int i = 0; i < n; i++) { if (jobs[i]->q.gp) { jobs[i]->q.gp->inflight--; jobs[i]->q.gp = nullptr; } jobs[i]->q.phase = kJobDone; }
    return rc;
}
JobRound *job_round_new() { return new (std::nothrow) JobRound(); }
void job_round_free(JobRound *r) { delete r; }
// the first round of a job set, left queued (R from job_round_new).  Jobs that cannot take the small-image path make the caller
// wait for the round as before: *queued = false and nothing is launched.
int detect_jobs_begin(nvca_ctx *ctx, DetectJob *const *jobs, int n, const int *lanes, JobRound *R, bool *queued)
{
    *queued = false;
    for (int i = 0; i < n; i++) if (jobs[i]->q.phase != kJobNew || !roi_eligible(ctx, *jobs[i], n)) return NVCA_OK;
    const int lane0 = ctx->cur_lane;
    bool pending = false;
    const int rc = jobs_round_begin(ctx, jobs, n, lanes, lane0, *R, &pending);
    ctx->cur_lane = lane0;
    *queued = pending;
    return rc;
}
// ... and the rest of the set: the queued round is closed (queued == true), then round after round until every job is done
int detect_jobs_finish(nvca_ctx *ctx, DetectJob *const *jobs, int n, const int *lanes, JobRound *R, bool queued)
{
    const int lane0 = ctx->cur_lane;
    struct Restore { nvca_ctx *c; int l, cap, wanted; ~Restore() { c->cur_lane = l; c->hit_cap = cap; c->hit_cap_wanted = wanted; } } restore{ctx, lane0, ctx->hit_cap, ctx->hit_cap_wanted};
    ctx->hit_cap_wanted = 0;
    if (queued) { const int rc = jobs_round_end(ctx, jobs, n, lanes, lane0, *R); if (rc) return rc; }
    for (;;) {
        bool pending = false;
        int rc = jobs_round_begin(ctx, jobs, n, lanes, lane0, *R, &pending);
        if (!pending) return rc;
        if ((rc = jobs_round_end(ctx, jobs, n, lanes, lane0, *R))) return rc;
    }
}
// run a set of detectMultiScale calls to completion: one wait per round for all of them.  lanes (optional, [n]): the lane
// each job runs on -- jobs of one lane execute in order, lanes side by side
int run_detect_jobs(nvca_ctx *ctx, DetectJob *const *jobs, int n, const int *lanes)
{
    JobRound R;
    return detect_jobs_finish(ctx, jobs, n, lanes, &R, false);
}

} // namespace nvca
