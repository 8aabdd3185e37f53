// lbp_job.cpp -- the launch set of a detectMultiScale job on a new-format cascade: its cached plan (pyramid: pyramid.cpp; tables:
// lbp_tables.cpp, hnew_tables.cpp, hgen_tables.cpp) and the evaluator's launches (featureType LBP: kernels_cascade_lbp.hip; HAAR:
// kernels_cascade_hnew.hip, or kernels_cascade_hgen.hip for a general cascade, around the LBP file's walk kernel).
#include "host_state.h"
#include "hgen_tables.h"
#include <cstdio>
#include <cstring>
#include <algorithm>

using namespace nvca;

namespace nvca {

// cv::CascadeClassifier::detectMultiScale on a new-format cascade (OpenCV 2.4 cascadedetect.cpp): the pyramid of
// CV_HAAR_SCALE_IMAGE with its own level rules, scanned by the cascade's evaluator (the plan key carries the format).  The plan holds the pyramid
// (layout, resize tables), one scan grid per level, the cascade's tables at the pitch of the planes and of the stage-0 tile, and the
// levels as k_group reads them.  Cached per (cascade, image size, parameters): a detectMultiScale job and a face stream of one
// geometry share it.
int lbp_plan(nvca_ctx *ctx, const nvca_cascade *casc, int cols, int rows, double sf, int minw, int minh, int maxw, int maxh, GeomPlan **out)
{
    const bool hnew = casc->format == NVCA_CASCADE_HAAR_NEW;
    const int ow = casc->c.ow, oh = casc->c.oh;          // (the window, whichever model holds the cascade)
    int rc;
    char key[256];
    snprintf(key, sizeof(key), hnew ? "HNEW|%llu|%d|%d|%.17g|%d|%d|%d|%d" : "LBP|%llu|%d|%d|%.17g|%d|%d|%d|%d", (unsigned long long)casc->c.uid, cols, rows, sf, minw, minh, maxw, maxh);
    GeomPlan *pp = find_plan(ctx, key);
    if (!pp) {
        std::unique_ptr<GeomPlan> np(new GeomPlan());
        // every level the call has: build_scan_tables sizes the candidate key for them and refuses, loudly, what no key holds
        if ((rc = pyr_plan_init(ctx, *np, cols, rows, lbp_levels(ow, oh, cols, rows, sf, minw, minh, maxw, maxh, kMaxPyrLevels + 1)))) return rc;
        if (!np->lv.empty()) {
            // the scan grids: what hit_valid / hit_rect check and map a candidate key with
            for (const PyrLevel &L : np->lv) np->det.specs.push_back(level_spec(np->P, L, ow, oh, 1));
            const bool general = hnew && casc->hnew.general;
            HgenTables gt; std::string err;
            HnewTables &ht = gt.base;
            if ((rc = general ? build_hgen_tables(casc->hnew, np->lv, np->P, gt, err) :
                      hnew ? build_hnew_tables(casc->hnew, np->lv, np->P, ht, err) : build_lbp_tables(casc->lbp, np->lv, np->P, ht.scan, err))) { ctx->set_error(err); return rc; }
            const LbpTables &t = ht.scan;
            np->det.key_sy = t.key_sy; np->det.key_ss = t.key_ss;
            LbpPlan &lp = np->lbp;
            lp.format = casc->format;
            TableBlob blob;
            const size_t o_gn = general ? blob.add(gt.nodes.data(), gt.nodes.size() * sizeof(HgenNodeDev)) : 0, o_gw = general ? blob.add(gt.weak.data(), gt.weak.size() * sizeof(HgenWeakDev)) : 0;
            const size_t o_hg = hnew ? blob.add(ht.gweak.data(), ht.gweak.size() * sizeof(HnewWeakDev)) : 0, o_ht = hnew ? blob.add(ht.tweak.data(), ht.tweak.size() * sizeof(HnewWeakDev)) : 0;
            const size_t o_levels = blob.add(t.levels.data(), t.levels.size() * sizeof(LbpLevelDev)), o_tiles = blob.add(t.tiles.data(), t.tiles.size() * sizeof(LbpTile)),
                         o_stages = blob.add(t.stages.data(), t.stages.size() * sizeof(LbpStageDev)), o_gweak = blob.add(t.gweak.data(), t.gweak.size() * sizeof(LbpWeakDev)),
                         o_tweak = blob.add(t.tweak.data(), t.tweak.size() * sizeof(LbpWeakDev)),
                         o_gscales = blob.add(t.gscales.data(), t.gscales.size() * sizeof(ScaleRec)), o_gpos = blob.add(t.gpos.data(), t.gpos.size() * sizeof(int));
            if ((rc = blob.upload(ctx, lp.d_blob))) return rc;
            LbpArgs &a = lp.args; memset(&a, 0, sizeof(a));
            const unsigned char *base = lp.d_blob.as<unsigned char>();
            a.levels = (const LbpLevelDev *)(base + o_levels); a.nlev = (int)t.levels.size();
            a.tiles = (const LbpTile *)(base + o_tiles); a.ntiles = (int)t.tiles.size();
            a.stages = (const LbpStageDev *)(base + o_stages); a.nstages = (int)t.stages.size();
            a.gweak = (const LbpWeakDev *)(base + o_gweak); a.tweak = (const LbpWeakDev *)(base + o_tweak);
            a.P = np->P; a.TP = t.TP; a.ow = ow; a.oh = oh; a.nrows = t.nrows;
            a.key_sy = t.key_sy; a.key_ss = t.key_ss; a.tile_stages = t.tile_stages;
            lp.bit_words = t.bit_words; lp.positions = t.positions; lp.lds = t.lds;
            lp.gscales = (const ScaleRec *)(base + o_gscales); lp.gpos = (const int *)(base + o_gpos);
            if (hnew) {
                HnewArgs &h = lp.hnew; memset(&h, 0, sizeof(h));
                a.gweak = a.tweak = nullptr;
                h.gweak = (const HnewWeakDev *)(base + o_hg); h.tweak = (const HnewWeakDev *)(base + o_ht);
                memcpy(h.nr, ht.nr, sizeof(h.nr)); memcpy(h.nrt, ht.nrt, sizeof(h.nrt)); h.area = ht.area;
                if (general) {
                    h.gweak = h.tweak = nullptr;
                    lp.general = true; lp.has_tilted = casc->hnew.has_tilted;
                    lp.hg_nodes = (const HgenNodeDev *)(base + o_gn); lp.hg_weak = (const HgenWeakDev *)(base + o_gw);
                }
            }
        }
        pp = store_plan(ctx, key, std::move(np));
    }
    *out = pp;
    return NVCA_OK;
}

// The launch set of a new-format scan, stated once: the pyramid of `nimg` images of `src` (the caller's images, or a lane's gray slots read
// through their LUTs), the evaluator on all of them, and -- group_thr given -- groupRectangles on the device; results into slots
// cj.r0 .. cj.r0 + nimg of cj.total.  Work buffers are the current lane's.
// A levels job (cv::CascadeClassifier::detectMultiScale with outputRejectLevels) is this scan with three differences: the
// tile stages stop in front of the last three stages (tile_stages = min(its value, nstages - 3): an argument of the launches, the tables
// hold every stage at either pitch, so the plan is the plain scan's), the stage groups end there too, and ONE launch evaluates the last
// three stages on every window left, emitting each of them with the stage that rejected it and that stage's sum.
int lbp_launch_set(nvca_ctx *ctx, GeomPlan *pp, const PyrSource &src, int cols, int rows, int nimg, CascadeJob &cj, const int *group_thr,
                   hipEvent_t early_done, bool levels)
{
    Workspace &ws = *ctx->ws;
    ResultBufs &rb = ws.res[ws.cur_res];
    int rc;
    // (the pyramid launchers write the squared integral with the sum: the HAAR evaluator reads it, the LBP one ignores it)
    // (... and the tilted integral where a general HAAR cascade holds a tilted feature)
    if ((rc = pyr_build(ctx, src, cols, rows, nimg, pp, pp->lbp.has_tilted))) return rc;
    const LbpPlan &lp = pp->lbp;
    // The job's images share every launch.  Pass bits per image; the two survivor lists are the whole job's, and either holds every
    // grid position of every image: a list that could be too short would drop windows, so it is never sized by an estimate.
    const size_t entries = lp.positions * (size_t)nimg;
    if (entries > 0xffffffffull) { ctx->set_error("LBP scan: more grid positions in one job than its list counters count"); return NVCA_ERR_ARG; }
    const int r0 = cj.r0, tot = std::max(cj.total, r0 + nimg);
    const size_t hits_stride = (size_t)ctx->hit_cap + 1;
    constexpr size_t kCnt = 64;                       // list counters in front of the first list (kCnt u32 words: the list behind them stays 8-byte aligned)
    if (ws.ln().failbits.ensure(2 * lp.bit_words * nimg * sizeof(unsigned) + 8) || ws.ln().deep.ensure(kCnt * sizeof(unsigned) + entries * sizeof(unsigned long long)) ||
        ws.ln().vnf.ensure(entries * sizeof(unsigned long long) + 8) ||
        rb.hits.ensure(hits_stride * tot * sizeof(unsigned long long)) || rb.h_hits.ensure(hits_stride * tot * sizeof(unsigned long long))) {
        ctx->set_error("device allocation failed for the cascade workspace"); return NVCA_ERR_NOMEM;
    }
    if (levels) {
        if (lp.args.nstages < 4 || group_thr) { ctx->set_error("internal: a levels scan needs four stages and groups on the host"); return NVCA_ERR_INTERNAL; }
        // a record per candidate the list can hold: slot r's records at + hit_cap * r
        if (rb.recs.ensure((size_t)ctx->hit_cap * tot * sizeof(LevelRec)) || rb.h_recs.ensure((size_t)ctx->hit_cap * tot * sizeof(LevelRec))) {
            ctx->set_error("device allocation failed for the cascade workspace"); return NVCA_ERR_NOMEM;
        }
        cj.d_recs = rb.recs.as<LevelRec>() + (size_t)ctx->hit_cap * r0; cj.h_recs = rb.h_recs.as<LevelRec>() + (size_t)ctx->hit_cap * r0;
    }
    cj.n = nimg;
    cj.cap = (unsigned)ctx->hit_cap * (unsigned)nimg;         // one list for all the job's slots, as cascade_enqueue's
    cj.d_hits = rb.hits.as<unsigned long long>() + hits_stride * r0;
    cj.h_hits = rb.h_hits.as<unsigned long long>() + hits_stride * r0;
    cj.dev_group = group_thr && !ctx->sw.host_group;
    if (cj.dev_group && (rc = group_prepare(ctx, cj, group_thr))) return rc;
    NVCA_HIP_CHECK(ctx, hipMemsetAsync(cj.d_hits, 0, sizeof(unsigned long long), ctx->cs()));
    NVCA_HIP_CHECK(ctx, hipMemsetAsync(ws.ln().deep.p, 0, kCnt * sizeof(unsigned), ctx->cs()));
    LbpArgs a = lp.args;
    a.sum = ws.ln().sum.as<int>(); a.nimg = nimg; a.plane_total = pp->plane_total; a.bit_words = lp.bit_words;
    a.bits = ws.ln().failbits.as<unsigned>(); a.bits2 = a.bits + lp.bit_words * nimg;
    a.cnt = ws.ln().deep.as<unsigned>();
    a.list[0] = (unsigned long long *)(ws.ln().deep.as<unsigned>() + kCnt); a.list[1] = ws.ln().vnf.as<unsigned long long>(); a.list_cap = (unsigned)entries;
    a.hits = cj.d_hits; a.hit_cap = cj.cap;
    // where the tile stages and the stage groups end: at the cascade's end, or in front of the three stages a levels job's last launch takes
    const int s_end = levels ? a.nstages - 3 : a.nstages;
    if (levels) a.tile_stages = std::min(a.tile_stages, s_end);
    {   // the first stages everywhere, the serial walk's skip rule, then the later stages group by group on ever shorter survivor
        // lists (groups of 2, 3, 4 ... stages: survivors thin out by about half per stage).  All booked as "window per lane".
        TimedLaunch t(ctx, NVCA_K_STRIP);
        const bool hnew = lp.format == NVCA_CASCADE_HAAR_NEW;
        HnewArgs h = lp.hnew;
        h.l = a; h.sq = ws.ln().sqsum.as<unsigned>(); h.hi_mul = pp->pyr_ok ? 1 : 4;          // (where pyr_build left the levels' high-byte planes)
        HgenArgs hg; hg.h = h; hg.nodes = lp.hg_nodes; hg.weak = lp.hg_weak; hg.tilted = lp.has_tilted ? ws.ln().tilted.as<int>() : nullptr;
        const bool general = lp.general;
        if (general) launch_hgen_stage0(ctx->cs(), hg, lp.lds); else if (hnew) launch_hnew_stage0(ctx->cs(), h, lp.lds); else launch_lbp_stage0(ctx->cs(), a, lp.lds);
        launch_lbp_walk(ctx->cs(), a);
        int g = 0;          // groups launched: the survivors in front of stage s_end lie in list g & 1, counted by cnt[g]
        for (int s0 = a.tile_stages, len = 2; s0 < s_end && g + 1 < (int)kCnt; s0 += len, len++) {
            // (the last group takes every stage that is left: the counters bound the number of groups)
            const int s1 = g + 2 == (int)kCnt ? s_end : std::min(s_end, s0 + len);
            if (general) launch_hgen_rest(ctx->cs(), hg, s0, s1, g & 1, g, (unsigned)entries);
            else if (hnew) launch_hnew_rest(ctx->cs(), h, s0, s1, g & 1, g, (unsigned)entries); else launch_lbp_rest(ctx->cs(), a, s0, s1, g & 1, g, (unsigned)entries);
            g++;
            if (s1 >= s_end) break;
        }
        if (levels) { if (general) launch_hgen_levels(ctx->cs(), hg, cj.d_recs, g & 1, g, (unsigned)entries); else if (hnew) launch_hnew_levels(ctx->cs(), h, cj.d_recs, g & 1, g, (unsigned)entries); else launch_lbp_levels(ctx->cs(), a, cj.d_recs, g & 1, g, (unsigned)entries); }
    }
    if (early_done) NVCA_HIP_CHECK(ctx, hipEventRecord(early_done, ctx->cs()));
    if (cj.dev_group) {
        // k_group as the Haar stream path launches it, on the fields it reads: the candidate list, the key layout, a ScaleRec per level
        // and the levels' output coordinates (lbp_tables.cpp)
        CascadeArgs ga; memset(&ga, 0, sizeof(ga));
        ga.hits = cj.d_hits; ga.hit_cap = cj.cap; ga.key_sy = a.key_sy; ga.key_ss = a.key_ss; ga.scales = lp.gscales; ga.pos = lp.gpos;
        ga.nscales = a.nlev; ga.batch = nimg;
        TimedLaunch t(ctx, NVCA_K_GROUP);
        launch_group(ctx->cs(), ga, rb.gthr.as<int>() + r0, ctx->sw.group_zero_copy ? cj.h_grp : cj.d_grp, kGroupOutCap, nimg);
    }
    NVCA_LAUNCH_CHECK(ctx);
    return cascade_fetch(ctx, cj);
}

int lbp_enqueue(nvca_ctx *ctx, DetectJob &j, int r0, int total)
{
    GeomPlan *pp = nullptr;
    int rc;
    if ((rc = lbp_plan(ctx, j.rq.casc, j.rq.cols, j.rq.rows, j.rq.sf, j.rq.minw, j.rq.minh, j.rq.maxw, j.rq.maxh, &pp))) return rc;
    j.q.phase = kJobFirstQueued; j.q.dp = nullptr;
    if (pp->lv.empty()) return NVCA_OK;
    PyrSource src;
    if ((rc = pyr_job_source(ctx, j, src))) return rc;
    CascadeJob &cj = j.q.cj;
    cj = CascadeJob(); cj.r0 = r0; cj.total = total;
    if ((rc = lbp_launch_set(ctx, pp, src, j.rq.cols, j.rq.rows, j.rq.nimg, cj, nullptr, nullptr, j.rq.levels))) return rc;      // (grouped on the host: detect_job_advance)
    j.q.gp = pp; pp->inflight++; j.q.dp = &pp->det;
    return NVCA_OK;
}

} // namespace nvca
