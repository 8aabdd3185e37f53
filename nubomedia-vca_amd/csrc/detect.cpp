// detect.cpp -- detectMultiScale as jobs: the plain, CV_HAAR_SCALE_IMAGE and CV_HAAR_FIND_BIGGEST_OBJECT launch sets, the serial
// FIND_BIGGEST replay, rounds of jobs that share one wait (the small images of a round: roi_batch.cpp), and the detectMultiScale
// entry points.
#include "host_state.h"
#include "host_logic.h"
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <new>

using namespace nvca;

// =========================================================================
// detectMultiScale
// =========================================================================

// A detectMultiScale call in halves: enqueue() queues the next launch set of the call on the context's stream and returns;
// advance(), after the stream has drained, consumes what the set produced and either finishes the call or asks for another
// set (FIND_BIGGEST narrows its scan once).  Many calls can therefore share ONE wait per round: the part detectors queue the
// face passes of every stream of a tick, then every ROI pass, with three synchronisations per tick instead of several per
// stream (parts.cpp).  The image planes are shared working memory: jobs use them one after the other in stream order; what a
// job leaves behind for the host (its candidate list) lives in its own result region (CascadeJob::r0).
namespace nvca {

// was window ix of a grid row visited by the serial walk that started at column `start`?  (visited iff the run of stage-0 rejects
// immediately left of it, not reaching below `start`, has even length: the walk steps by 2 behind a stage-0 reject, by 1 otherwise)
static inline bool fb_visited(const unsigned long long *row, int start, int ix)
{
    int run = 0;
    for (int x = ix - 1; x >= start && ((row[x >> 6] >> (x & 63)) & 1ull); x--) run++;
    return !(run & 1);
}

static bool fb_make_spec(const DetectJob &j, int spitch, const FbStep &st, int startX, int endX, int startY, int endY, ScaleSpec &sp)
{   // scan grid of one ladder step; false: nothing to scan there
    if (!(endX > startX && endY > startY)) return false;
    sp = ScaleSpec();
    sp.table_factor = st.factor; sp.plane_off = 0; sp.pitch = spitch; sp.plane_rows = j.rows + 1; sp.adaptive = 1;
    sp.out_factor = 0; sp.out_w = st.winw; sp.out_h = st.winh;
    for (int ix = startX; ix < endX; ix++) sp.xs.push_back(cv_round(ix * st.ystep));
    for (int iy = startY; iy < endY; iy++) sp.ys.push_back(cv_round(iy * st.ystep));
    // cvRunHaarClassifierCascadeSum returns -1 (no hit, step 1) outside the image: drop such grid points
    while (!sp.xs.empty() && (sp.xs.back() + st.winw >= j.cols + 1)) sp.xs.pop_back();
    while (!sp.ys.empty() && (sp.ys.back() + st.winh >= j.rows + 1)) sp.ys.pop_back();
    const bool neg = (!sp.xs.empty() && sp.xs.front() < 0) || (!sp.ys.empty() && sp.ys.front() < 0);
    return !sp.xs.empty() && !sp.ys.empty() && !neg;
}

// cvHaarDetectObjectsForROC, CV_HAAR_SCALE_IMAGE branch (EYE/kmseyedetect.cpp:991-993, NOSE/kmsnosedetect.cpp:843-846,
// MOUTH/kmsmouthdetect.cpp:845-848, EAR/kmseardetect.cpp:656-659): per factor the image is resized, integrated and
// scanned with the unscaled window on a fixed grid.  All pyramid levels (of both images: the ear detector scans an image
// and its mirror, EAR/kmseardetect.cpp:796-803) are evaluated by one launch set.
static int si_plan(nvca_ctx *ctx, const DetectJob &j, GeomPlan **out)
{
    const Cascade &c = j.casc->c;
    const int cols = j.cols, rows = j.rows;
    int rc;
    // pyramid layout, resize tables and scan tables depend only on (cascade, image size, parameters): built once
    char key[256];
    snprintf(key, sizeof(key), "SI|%llu|%d|%d|%.17g|%d|%d|%d|%d", (unsigned long long)c.uid, cols, rows, j.sf, j.minw, j.minh, j.maxw, j.maxh);
    GeomPlan *pp = find_plan(ctx, key);
    if (!pp) {
        std::unique_ptr<GeomPlan> np(new GeomPlan());
        np->P = (int)round_up(cols + 1, 8);
        for (double factor = 1;; factor *= j.sf) {
            const int winw = cv_round(c.ow * factor), winh = cv_round(c.oh * factor);
            const int szw = cv_round(cols / factor), szh = cv_round(rows / factor);
            if (szw - c.ow + 1 <= 0 || szh - c.oh + 1 <= 0) break;
            if (winw > j.maxw || winh > j.maxh) break;
            if (winw < j.minw || winh < j.minh) continue;
            if (szw + 1 <= 1 + c.ow) continue;                   // HaarDetectObjects_ScaleImage_Invoker's early return
            PyrLevel L; L.f = factor; L.szw = szw; L.szh = szh; L.winw = winw; L.winh = winh;
            L.gpitch = (int)round_up(szw, 64); L.gray_off = np->gray_total; L.plane_off = (int)np->plane_total;
            np->gray_total += round_up((size_t)L.gpitch * szh, 256);
            np->plane_total += round_up((size_t)np->P * (szh + 1), 64);
            np->lv.push_back(L);
            if (np->lv.size() > 62) break;
        }
        std::vector<ScaleSpec> specs;
        for (const PyrLevel &L : np->lv) {
            std::unique_ptr<GeomPlan> gp(new GeomPlan());
            build_resize_tab(cols, rows, L.szw, L.szh, gp->tab);
            np->level_tabs.push_back(std::move(gp));
            ScaleSpec sp;
            sp.table_factor = 1.; sp.plane_off = L.plane_off; sp.pitch = np->P; sp.plane_rows = L.szh + 1; sp.adaptive = 0;
            sp.out_factor = L.f; sp.out_w = L.winw; sp.out_h = L.winh;
            const int ystep = L.f > 2 ? 1 : 2;
            for (int x = 0; x < L.szw - c.ow; x += ystep) sp.xs.push_back(x);
            for (int y = 0; y < L.szh - c.oh; y += ystep) sp.ys.push_back(y);
            specs.push_back(std::move(sp));
        }
        if ((rc = upload_tabs(ctx, np->level_tabs, np->d_level_tabs))) return rc;
        if (!np->lv.empty()) {
            std::string err;
            if ((rc = np->det.build_custom(ctx, c, std::move(specs), false, err))) { ctx->set_error(err); return rc; }
            if ((rc = np->det.upload(ctx))) return rc;
            std::vector<PyrLevelDev> dl(np->lv.size());
            np->pyr_ok = !ctx->sw.pyr_off;
            for (size_t li = 0; li < np->lv.size(); li++) {
                const PyrLevel &L = np->lv[li]; GeomPlan *t = np->level_tabs[li].get();
                PyrLevelDev &d = dl[li]; memset(&d, 0, sizeof(d));
                d.szw = L.szw; d.szh = L.szh; d.gpitch = L.gpitch; d.mode = t->tab.mode; d.xmax = t->tab.xmax; d.plane_off = L.plane_off;
                d.gray_off = (long long)L.gray_off;
                d.xofs = t->d_xofs.as<int>(); d.ialpha = t->d_ialpha.as<short>(); d.yofs = t->d_yofs.as<int>(); d.ibeta = t->d_ibeta.as<short>();
                np->pyr_maxw = std::max(np->pyr_maxw, L.szw); np->pyr_maxh = std::max(np->pyr_maxh, L.szh);
                if (L.szw > 1023) np->pyr_ok = false;            // one column per thread, plus the zero column
            }
            if (np->d_pyr.ensure(dl.size() * sizeof(PyrLevelDev))) { ctx->set_error("allocation failed (pyramid table)"); return NVCA_ERR_NOMEM; }
            NVCA_HIP_CHECK(ctx, hipMemcpy(np->d_pyr.p, dl.data(), dl.size() * sizeof(PyrLevelDev), hipMemcpyHostToDevice));
        }
        pp = store_plan(ctx, key, std::move(np));
    }
    *out = pp;
    return NVCA_OK;
}

// Device images of a job that sit at equal distances (the working images of a batched part call are carved that way) are read
// where they are; anything else is copied into the lane's gray slots first.
static bool job_images_in_place(const DetectJob &j, size_t *slot)
{
    if (j.mem != NVCA_MEM_DEVICE) return false;
    *slot = 0;
    if (j.nimg == 1) return true;
    const uint8_t *a = (const uint8_t *)j.img[0], *b = (const uint8_t *)j.img[1];
    if (b <= a) return false;
    const size_t d = (size_t)(b - a);
    if (d < (size_t)j.stride * (j.rows - 1) + j.cols) return false;
    for (int k = 2; k < j.nimg; k++) if ((const uint8_t *)j.img[k] != a + d * k) return false;
    *slot = d;
    return true;
}

static int si_enqueue(nvca_ctx *ctx, DetectJob &j, int r0, int total)
{
    Workspace &ws = *ctx->ws;
    const Cascade &c = j.casc->c;
    const int cols = j.cols, rows = j.rows, nimg = j.nimg;
    GeomPlan *pp = nullptr;
    int rc;
    if ((rc = si_plan(ctx, j, &pp))) return rc;
    j.phase = 1; j.dp = nullptr;
    if (pp->lv.empty()) return NVCA_OK;
    const int P = pp->P;
    const size_t gray_total = pp->gray_total, plane_total = pp->plane_total;
    PreGeom g0; make_geom(g0, cols, rows, j.stride, 1, cols, rows);
    if ((rc = ensure_ws(ctx, g0, nimg))) return rc;
    if (ws.ln().aux.ensure(gray_total * nimg + 64) || ws.ln().sum.ensure((plane_total * nimg + 4 * (size_t)P) * sizeof(int)) || ws.ln().sqsum.ensure(plane_total * nimg * sizeof(unsigned long long)) ||
        (c.has_tilted && ws.ln().tilted.ensure((plane_total * nimg + 4 * (size_t)P) * sizeof(int)))) {
        ctx->set_error("allocation failed (pyramid)"); return NVCA_ERR_NOMEM;
    }
    if (c.has_tilted && (size_t)2 * (pp->pyr_maxw + pp->pyr_maxh + 2) * sizeof(int) > 64 * 1024) { ctx->set_error("image too large for the tilted integral"); return NVCA_ERR_ARG; }
    const uint8_t *src0 = ws.ln().gray.as<uint8_t>(); int spitch0 = g0.gpitch; size_t sslot0 = g0.gray_slot;
    size_t in_place_slot = 0;
    if (job_images_in_place(j, &in_place_slot)) { src0 = (const uint8_t *)j.img[0]; spitch0 = j.stride; sslot0 = in_place_slot; }
    else
        for (int k = 0; k < nimg; k++)
            if ((rc = stage_2d(ctx, ws.ln().gray.as<uint8_t>() + g0.gray_slot * k, g0.gpitch, j.img[k], j.stride, cols, rows, j.mem))) return rc;
    if (pp->pyr_ok) {            // all levels of all images: one resize launch, one integral launch
        { TimedLaunch t(ctx, NVCA_K_RESIZE1);
          launch_pyr_resize(ctx->cs(), src0, cols, rows, spitch0, sslot0, pp->d_pyr.as<PyrLevelDev>(),
                            (int)pp->lv.size(), nimg, pp->pyr_maxw, pp->pyr_maxh, ws.ln().aux.as<uint8_t>(), gray_total); }
        { TimedLaunch t(ctx, NVCA_K_INTEGRAL);
          launch_pyr_integral(ctx->cs(), ws.ln().aux.as<uint8_t>(), gray_total, pp->d_pyr.as<PyrLevelDev>(), (int)pp->lv.size(), nimg,
                              ws.ln().sum.as<int>(), ws.ln().sqsum.as<unsigned>(), plane_total, P); }
        if (c.has_tilted) {          // cvIntegral(&img1, &sum1, &sqsum1, _tilted) per level
            TimedLaunch t(ctx, NVCA_K_INTEGRAL);
            launch_pyr_tilted(ctx->cs(), ws.ln().aux.as<uint8_t>(), gray_total, pp->d_pyr.as<PyrLevelDev>(), (int)pp->lv.size(), nimg,
                              ws.ln().tilted.as<int>(), plane_total, P, pp->pyr_maxw, pp->pyr_maxh);
        }
    } else
    for (size_t li = 0; li < pp->lv.size(); li++) {
        const PyrLevel &L = pp->lv[li];
        GeomPlan *gp = pp->level_tabs[li].get();
        uint8_t *lg = ws.ln().aux.as<uint8_t>() + L.gray_off;
        { TimedLaunch t(ctx, NVCA_K_RESIZE1);               // cvResize(img, &img1, CV_INTER_LINEAR)
          launch_resize1(ctx->cs(), src0, cols, rows, spitch0, gp->tab.mode, gp->d_xofs.as<int>(),
                         gp->d_ialpha.as<short>(), gp->d_yofs.as<int>(), gp->d_ibeta.as<short>(), gp->tab.xmax, lg, L.szw,
                         L.szh, L.gpitch, nullptr, nimg, sslot0, gray_total); }
        PreGeom g; make_geom(g, L.szw, L.szh, L.gpitch, 1, L.szw, L.szh);
        g.gpitch = L.gpitch; g.spitch = P; g.sum_slot = plane_total; g.gray_slot = gray_total;
        run_integral(ctx, g, nullptr, nimg, lg, ws.ln().sum.as<int>() + L.plane_off,
                     (unsigned long long *)(ws.ln().sqsum.as<unsigned>() + L.plane_off));     // lo plane of the level; hi plane at + plane_total
        if (c.has_tilted && (rc = run_tilted(ctx, g, nullptr, nimg, lg, ws.ln().tilted.as<int>() + L.plane_off))) return rc;
    }
    j.cj = CascadeJob(); j.cj.r0 = r0; j.cj.n = nimg; j.cj.total = total;
    if ((rc = cascade_enqueue(ctx, pp->det, plane_total, P, j.cj, nullptr, false))) return rc;
    j.gp = pp; pp->inflight++; j.dp = &pp->det;
    return NVCA_OK;
}

// plain scale-cascade scan (flags without SCALE_IMAGE / FIND_BIGGEST): FACE/kmsfacedetect.cpp:809-811, EYE/kmseyedetect.cpp:958-960
static int plain_enqueue(nvca_ctx *ctx, DetectJob &j, int r0, int total)
{
    GeomPlan *gp = nullptr;
    int rc;
    if ((rc = get_face_plan(ctx, j.casc, j.cols, j.rows, j.stride, 1, j.cols, j.rows, j.sf, j.minw, j.minh, j.maxw, j.maxh, &gp))) return rc;
    const int nimg = j.nimg;
    if ((rc = ensure_ws(ctx, gp->g, nimg))) return rc;
    PreGeom g = gp->g;
    const uint8_t *src = nullptr;
    size_t in_place_slot = 0;
    if (job_images_in_place(j, &in_place_slot) && j.stride % 4 == 0 && ((uintptr_t)j.img[0] & 3) == 0 && in_place_slot % 4 == 0) {
        src = (const uint8_t *)j.img[0]; g.gpitch = j.stride; g.gray_slot = in_place_slot;      // the integral kernels read rows in 4-byte words
    } else
        for (int k = 0; k < nimg; k++)
            if ((rc = stage_2d(ctx, ctx->ws->ln().gray.as<uint8_t>() + gp->g.gray_slot * k, gp->g.gpitch, j.img[k], j.stride, j.cols, j.rows, j.mem))) return rc;
    run_integral(ctx, g, nullptr, nimg, src);
    if (j.casc->c.has_tilted && (rc = run_tilted(ctx, g, nullptr, nimg, src))) return rc;
    j.gthr = (!j.raw_only && j.min_neighbors != 0) ? std::max(j.min_neighbors, 1) : 0;
    j.cj = CascadeJob(); j.cj.r0 = r0; j.cj.n = nimg; j.cj.total = total;
    const std::vector<int> gthrv(nimg, j.gthr);
    if ((rc = cascade_enqueue(ctx, gp->det, gp->g.sum_slot, gp->g.spitch, j.cj, j.gthr ? gthrv.data() : nullptr, true))) return rc;
    j.gp = gp; gp->inflight++; j.dp = &gp->det; j.phase = 1;
    return NVCA_OK;
}

// cvHaarDetectObjectsForROC with CV_HAAR_FIND_BIGGEST_OBJECT (NOSE/kmsnosedetect.cpp:870-873, MOUTH/kmsmouthdetect.cpp:870-873,
// EAR/kmseardetect.cpp:712-715): scale-cascade scan from the largest factor down; after the first grouped detection
// the scan narrows to a region of interest and a minimum size.  The serial loop changes its scan only once, so two launch
// sets do: (1) every step on its full grid (a cached plan per geometry), (2) once the region is known, the remaining steps
// on their narrowed grids.  fb_replay() replays the serial logic on those results, step by step.
static int fb_stage_image(nvca_ctx *ctx, const DetectJob &j, PreGeom &g)
{
    make_geom(g, j.cols, j.rows, j.stride, 1, j.cols, j.rows);
    int rc;
    if ((rc = ensure_ws(ctx, g, 1))) return rc;
    if ((rc = stage_2d(ctx, ctx->ws->ln().gray.p, g.gpitch, j.img[0], j.stride, j.cols, j.rows, j.mem))) return rc;
    run_integral(ctx, g, nullptr, 1);
    if (j.casc->c.has_tilted && (rc = run_tilted(ctx, g, nullptr, 1))) return rc;
    return NVCA_OK;
}

static int fb_enqueue_first(nvca_ctx *ctx, DetectJob &j, int r0, int total)
{
    const Cascade &c = j.casc->c;
    const int cols = j.cols, rows = j.rows;
    PreGeom g; int rc;
    if ((rc = fb_stage_image(ctx, j, g))) return rc;
    // the ladder of factors, largest first, exactly as the serial loop walks it
    j.ladder.clear();
    {
        int n_factors = 0; double factor;
        for (n_factors = 0, factor = 1; factor * c.ow < cols - 10 && factor * c.oh < rows - 10; n_factors++, factor *= j.sf)
            ;
        const double inv = 1. / j.sf; factor *= inv;
        for (; n_factors-- > 0; factor *= inv) j.ladder.push_back(FbStep{factor, std::max(2., factor), cv_round(c.ow * factor), cv_round(c.oh * factor)});
    }
    j.hits.assign(j.ladder.size(), {}); j.have.assign(j.ladder.size(), 0);
    j.all.clear(); j.scanROI = nvca_rect{0, 0, 0, 0}; j.narrowed_done = false; j.fb_i = 0; j.cur_minw = j.minw; j.cur_minh = j.minh;
    char key[256];
    snprintf(key, sizeof(key), "FB|%llu|%d|%d|%.17g|%d|%d|%d|%d", (unsigned long long)c.uid, cols, rows, j.sf, j.minw, j.minh, j.maxw, j.maxh);
    GeomPlan *p1 = find_plan(ctx, key);
    if (!p1) {
        std::unique_ptr<GeomPlan> np(new GeomPlan());
        std::vector<ScaleSpec> specs;
        for (size_t i = 0; i < j.ladder.size(); i++) {
            const FbStep &st = j.ladder[i];
            if (st.winw < j.minw || st.winh < j.minh) break;
            if (st.winw > j.maxw || st.winh > j.maxh) continue;
            ScaleSpec sp;
            if (fb_make_spec(j, g.spitch, st, 0, cv_round((cols - st.winw) / st.ystep), 0, cv_round((rows - st.winh) / st.ystep), sp)) {
                specs.push_back(std::move(sp)); np->fb_ladder.push_back((int)i);
            }
        }
        if (!specs.empty()) {
            std::string err;
            if ((rc = np->det.build_custom(ctx, c, std::move(specs), false, err))) { ctx->set_error(err); return rc; }
            if ((rc = np->det.upload(ctx))) return rc;
        }
        p1 = store_plan(ctx, key, std::move(np));
    }
    j.phase = 1; j.dp = nullptr;
    // steps the full-grid plan does not hold have nothing to scan
    for (size_t i = 0; i < j.ladder.size(); i++) j.have[i] = 1;
    if (!p1->fb_ladder.empty()) {
        j.ladder_of = p1->fb_ladder;
        j.cj = CascadeJob(); j.cj.r0 = r0; j.cj.n = 1; j.cj.total = total;
        if ((rc = cascade_enqueue(ctx, p1->det, g.sum_slot, g.spitch, j.cj, nullptr, false))) return rc;
        j.gp = p1; p1->inflight++; j.dp = &p1->det;
    }
    return NVCA_OK;
}

// the narrowed launch set: this step and all later ones on their narrowed grids (nothing changes the scan any more)
static int fb_enqueue_narrowed(nvca_ctx *ctx, DetectJob &j, int r0, int total)
{
    PreGeom g; int rc;
    if ((rc = fb_stage_image(ctx, j, g))) return rc;         // the planes have served other jobs in between
    j.cj = CascadeJob(); j.cj.r0 = r0; j.cj.n = 1; j.cj.total = total;
    if ((rc = cascade_enqueue(ctx, *j.own, g.sum_slot, g.spitch, j.cj, nullptr, false))) return rc;
    j.dp = j.own.get();
    return NVCA_OK;
}

// the serial loop of cvHaarDetectObjectsForROC on the scan results at hand; returns 1 when it needs the narrowed set first
static int fb_replay(nvca_ctx *ctx, DetectJob &j)
{
    const Cascade &c = j.casc->c;
    const bool rough = (j.flags & NVCA_HAAR_DO_ROUGH_SEARCH) != 0;
    const int cols = j.cols, rows = j.rows;
    const int spitch = (int)round_up(cols + 1, 8);
    for (size_t i = j.fb_i; i < j.ladder.size(); i++) {
        const FbStep &st = j.ladder[i];
        if (st.winw < j.cur_minw || st.winh < j.cur_minh) break;
        if (st.winw > j.maxw || st.winh > j.maxh) continue;
        const bool narrowed = j.scanROI.w * j.scanROI.h > 0;
        if (narrowed && !j.narrowed_done) {
            j.narrowed_done = true;
            std::vector<ScaleSpec> specs; j.ladder_of.clear();
            for (size_t k = i; k < j.ladder.size(); k++) {
                const FbStep &sk = j.ladder[k];
                j.hits[k].clear(); j.have[k] = 1;
                if (sk.winw < j.cur_minw || sk.winh < j.cur_minh) break;
                if (sk.winw > j.maxw || sk.winh > j.maxh) continue;
                ScaleSpec sp;
                const int sx0 = cv_round(j.scanROI.x / sk.ystep), sx1 = cv_round((j.scanROI.x + j.scanROI.w - sk.winw) / sk.ystep);
                const int sy0 = cv_round(j.scanROI.y / sk.ystep), sy1 = cv_round((j.scanROI.y + j.scanROI.h - sk.winh) / sk.ystep);
                if (j.small && j.dense && k < j.dense_hits.size() && j.rej_wpr[k] > 0) {
                    // dense first launch: the narrowed walk of this step is replayed here -- its windows are grid points of the full grid, the
                    // launch reported every one of them that passes the cascade, and which of them the walk from column sx0 visits follows
                    // from the stage-0 reject bits (no second launch, no second wait).  A step the first launch did not hold (below the call's
                    // minSize: the narrowed search lowers it to 0.4 / 0.6 of the object found) still takes the second launch, below.
                    RoiStep tmp;
                    if (roi_grid(cols, rows, sk.ystep, sk.winw, sk.winh, sx0, sx1, sy0, sy1, tmp)) {
                        const int wpr = j.rej_wpr[k];
                        for (unsigned key : j.dense_hits[k]) {            // ascending (iy, ix): the serial order
                            const int iy = (int)(key >> 13), ix = (int)(key & 8191);
                            if (iy < tmp.startY || iy >= tmp.endY || ix < tmp.startX || ix >= tmp.endX) continue;
                            if (iy >= j.rej_rows[k] || !fb_visited(j.rej_bits[k] + (size_t)iy * wpr, tmp.startX, ix)) continue;
                            j.hits[k].push_back(nvca_rect{cv_round(ix * sk.ystep), cv_round(iy * sk.ystep), sk.winw, sk.winh});
                        }
                    }
                } else if (j.small) {             // small-image path: no plan, the narrowed grids go into the next round's launch as they are
                    RoiStep tmp;
                    if (roi_grid(cols, rows, sk.ystep, sk.winw, sk.winh, sx0, sx1, sy0, sy1, tmp)) { j.ladder_of.push_back((int)k); j.have[k] = 0; }
                } else if (fb_make_spec(j, spitch, sk, sx0, sx1, sy0, sy1, sp)) {
                    specs.push_back(std::move(sp)); j.ladder_of.push_back((int)k); j.have[k] = 0;
                }
            }
            if (j.small && !j.ladder_of.empty()) { j.fb_i = i; return 1; }
            if (!specs.empty()) {
                j.own.reset(new DetectPlan()); std::string err;
                int rc;
                if ((rc = j.own->build_custom(ctx, c, std::move(specs), false, err))) { ctx->set_error(err); return rc < 0 ? rc : NVCA_ERR_ARG; }
                if ((rc = j.own->upload(ctx))) return rc;
                j.fb_i = i;
                return 1;                                    // come back with the narrowed scans
            }
        }
        j.all.insert(j.all.end(), j.hits[i].begin(), j.hits[i].end());
        if (!j.all.empty() && j.scanROI.w * j.scanROI.h == 0) {
            std::vector<nvca_rect> tmp(j.all);
            group_rectangles(tmp, std::max(j.min_neighbors, 1), 0.2);
            if (!tmp.empty()) {
                nvca_rect maxRect{0, 0, 0, 0};
                for (const nvca_rect &r : tmp) if (r.w * r.h > maxRect.w * maxRect.h) maxRect = r;
                j.all.push_back(maxRect);
                j.scanROI = maxRect;
                const int dx = cv_round(maxRect.w * 0.2), dy = cv_round(maxRect.h * 0.2);
                j.scanROI.x = std::max(j.scanROI.x - dx, 0); j.scanROI.y = std::max(j.scanROI.y - dy, 0);
                j.scanROI.w = std::min(j.scanROI.w + dx * 2, cols - 1 - j.scanROI.x);
                j.scanROI.h = std::min(j.scanROI.h + dy * 2, rows - 1 - j.scanROI.y);
                const double minScale = rough ? 0.6 : 0.4;
                j.cur_minw = cv_round(maxRect.w * minScale); j.cur_minh = cv_round(maxRect.h * minScale);
            }
        }
    }
    group_rectangles(j.all, std::max(j.min_neighbors, 1), 0.2);
    j.out[0].clear();
    if (!j.all.empty()) {
        nvca_rect best{0, 0, 0, 0};
        for (const nvca_rect &r : j.all) if (r.w * r.h > best.w * best.h) best = r;
        j.out[0].push_back(best);
    }
    return 0;
}

// queue the job's next launch set; its candidates go to result slots [r0, r0 + slots()) of `total`
static int detect_job_enqueue(nvca_ctx *ctx, DetectJob &j, int r0, int total)
{
    (void)hipSetDevice(ctx->device);
    if (j.phase == 0) {
        for (int k = 0; k < kJobImages; k++) j.out[k].clear();
        if (j.kind == 2) return fb_enqueue_first(ctx, j, r0, total);
        if (j.kind == 1) return si_enqueue(ctx, j, r0, total);
        return plain_enqueue(ctx, j, r0, total);
    }
    if (j.phase == 2) return fb_enqueue_narrowed(ctx, j, r0, total);
    return NVCA_OK;
}

// after the stream has drained: consume the queued set's results.  phase 3: the call is complete (out[] holds the objects);
// phase 2: it needs another set (enqueue again)
static int detect_job_advance(nvca_ctx *ctx, DetectJob &j)
{
    int rc = NVCA_OK;
    std::vector<std::vector<nvca_rect>> raw;
    std::vector<char> grouped;
    std::vector<std::vector<int>> sc;
    bool have = j.dp != nullptr;
    const bool was_fused = j.fused;
    if (j.fused) {
        // candidates of the round's k_roi launch, sorted into the serial order (step, row, column) -> rectangle
        raw.assign(j.nimg, {}); sc.assign(j.nimg, {}); grouped.assign(j.nimg, 0);
        for (int k = 0; k < j.nimg; k++) {
            std::sort(j.rkeys[k].begin(), j.rkeys[k].end());
            raw[k].reserve(j.rkeys[k].size()); sc[k].reserve(j.rkeys[k].size());
            for (unsigned key : j.rkeys[k]) {
                const DetectJob::RoiStepInfo &ri = j.rinfo[key >> 26];
                const int iy = (key >> 13) & 8191, ix = key & 8191;
                if (j.dense && k == 0) {
                    // a dense launch reports every window that passes the cascade; the serial walk of the FULL grid (start column 0) visits only some
                    const size_t li = (size_t)ri.ladder;
                    if (li >= j.rej_bits.size() || j.rej_wpr[li] <= 0 || iy >= j.rej_rows[li] || ix >= j.rej_wpr[li] * 64) {
                        ctx->set_error("internal: dense candidate outside its reject bitmap (device result rejected)"); j.phase = 3; return NVCA_ERR_INTERNAL;
                    }
                    j.dense_hits[li].push_back((unsigned)(iy << 13 | ix));
                    if (!fb_visited(j.rej_bits[li] + (size_t)iy * j.rej_wpr[li], 0, ix)) continue;
                }
                if (ri.out_factor != 0) raw[k].push_back(nvca_rect{cv_round(ix * ri.out_factor), cv_round(iy * ri.out_factor), ri.winw, ri.winh});
                else raw[k].push_back(nvca_rect{cv_round(ix * ri.ystep), cv_round(iy * ri.ystep), ri.winw, ri.winh});
                sc[k].push_back(ri.ladder);
            }
            j.rkeys[k].clear();
        }
        j.fused = false;
        have = true;
    } else
    if (j.dp) rc = cascade_collect(ctx, *j.dp, j.cj, raw, j.kind == 0 ? &grouped : nullptr, j.kind == 2 ? &sc : nullptr);
    if (j.gp) { j.gp->inflight--; j.gp = nullptr; }
    if (rc == NVCA_ERR_OVERFLOW && j.regrown < 2 && ctx->hit_cap_wanted > ctx->hit_cap) {
        // More raw candidates than the lists hold.  OpenCV has no such limit (and a FIND_BIGGEST search would have stopped at
        // its first object long before: NOSE/kmsnosedetect.cpp:870-873, MOUTH/kmsmouthdetect.cpp:870-873, EAR/kmseardetect.cpp:712-715),
        // so the call must answer, not fail: the same launch set runs once more with lists of exactly the size the exact count
        // asks for (run_detect_jobs applies hit_cap_wanted before the next round), and the serial logic is replayed on the
        // complete candidate lists -- the result is what the reference returns.
        j.regrown++; j.dp = nullptr;
        if (j.phase == 1) j.phase = 0;              // the first (or only) set again; a narrowed FIND_BIGGEST set stays in phase 2
        return NVCA_OK;
    }
    if (rc) { j.phase = 3; return rc; }
    if (j.kind == 0) {
        if (have)
            for (int k = 0; k < j.nimg; k++) {
                if (j.gthr && !grouped[k]) group_rectangles(raw[k], j.gthr, 0.2);
                j.out[k].swap(raw[k]);
            }
        j.phase = 3;
    } else if (j.kind == 1) {
        if (have) { if (!j.raw_only) group_all(raw, j.min_neighbors); for (int k = 0; k < j.nimg; k++) j.out[k].swap(raw[k]); }
        j.phase = 3;
    } else {
        if (have) {
            for (size_t k = 0; k < raw[0].size(); k++) {
                // the large-image path numbers a candidate by its scale inside the plan (ladder_of maps it back), the small-image
                // path by its ladder step directly
                size_t li = (size_t)sc[0][k];
                if (!was_fused) { if (li >= j.ladder_of.size()) li = (size_t)-1; else li = (size_t)j.ladder_of[li]; }
                if (li >= j.hits.size()) { ctx->set_error("internal: candidate of an unknown ladder step"); j.phase = 3; return NVCA_ERR_INTERNAL; }
                j.hits[li].push_back(raw[0][k]);
            }
            for (int li : j.ladder_of) j.have[li] = 1;
        }
        j.dp = nullptr;
        const int r = fb_replay(ctx, j);
        if (r < 0) { j.phase = 3; return r; }
        j.phase = r == 1 ? 2 : 3;
    }
    j.dp = nullptr;
    return NVCA_OK;
}

// run a set of detectMultiScale calls to completion: one wait per round for all of them.  lanes (optional, [n]): the lane
// each job runs on -- jobs of one lane execute in order, lanes side by side
double g_jobs_fine_s[6] = {0, 0, 0, 0, 0, 0};        // NVCA_PART_STATS: roi_add_job, roi_launch, roi_collect, helper-thread advance, serial advance, small-path jobs (count)
double g_jobs_enqueue_s = 0, g_jobs_wait_s = 0, g_jobs_advance_s = 0;      // NVCA_PART_STATS (diagnostic, one context at a time): where run_detect_jobs spends the host's time
// One round of a job set in two halves, so that a caller may leave a round queued and come back for it (parts.cpp: a submitted part-detector
// batch keeps its face passes in flight while the batch before it is collected).  begin: every unfinished job queues its next launch
// set (small images: all in ONE k_roi launch); end: the lanes are waited for, the candidates handed out, every job advanced.
struct JobRound { RoiBatch rb; bool used[kLanes] = {false}; int rc = NVCA_OK; double t1 = 0; int roi_regrown = 0; };
static int jobs_round_begin(nvca_ctx *ctx, DetectJob *const *jobs, int n, const int *lanes, int lane0, JobRound &R, bool *pending_out)
{
    const bool g_job_stats = ctx->sw.part_stats > 0;
    const int roi_regrown = R.roi_regrown;
    {
        if (ctx->hit_cap_wanted > ctx->hit_cap) ctx->hit_cap = ctx->hit_cap_wanted;      // a set overflowed in the last round: it runs again with room (this call only)
        int pending = 0;
        for (int i = 0; i < n; i++) if (jobs[i]->phase != 3) pending++;
        if (!pending) { *pending_out = false; return NVCA_OK; }
        *pending_out = true;
        int &rc = R.rc; rc = NVCA_OK;
        bool (&used)[kLanes] = R.used;
        for (bool &u : used) u = false;
        const double t0 = g_job_stats ? mono_s() : 0;
        // small images first: every such job of the round goes into ONE k_roi launch (no plan, no per-job launches)
        R.rb.reset();
        RoiBatch &rb = R.rb;
        for (int i = 0; i < n && !rc; i++) {
            DetectJob &j = *jobs[i];
            if (j.phase == 3) continue;
            if (j.phase == 0 && j.regrown == 0) j.small = roi_eligible(ctx, j, n);
            if (!j.small) continue;
            ctx->cur_lane = lanes ? lanes[i] : lane0;
            if (rb.jobs.empty()) rb.lane = ctx->cur_lane;
            j.roi_prev_phase = j.phase;
            const double ta = g_job_stats ? mono_s() : 0;
            rc = roi_add_job(ctx, rb, j);
            if (g_job_stats) { g_jobs_fine_s[0] += mono_s() - ta; g_jobs_fine_s[5] += 1; }
            if (!rc && !j.fused) j.small = false;          // more ladder steps than the key holds: the large-image path takes it
            else used[ctx->cur_lane] = true;
        }
        int total = 0, r0 = 0;
        for (int i = 0; i < n; i++) if (jobs[i]->phase != 3 && !jobs[i]->small) total += jobs[i]->slots();
        for (int i = 0; i < n && !rc; i++) {
            if (jobs[i]->phase == 3 || jobs[i]->small) continue;
            ctx->cur_lane = lanes ? lanes[i] : lane0;
            used[ctx->cur_lane] = true;
            rc = detect_job_enqueue(ctx, *jobs[i], r0, total);
            r0 += jobs[i]->slots();
        }
        const double tl = g_job_stats ? mono_s() : 0;
        if (!rc && !rb.jobs.empty()) { ctx->cur_lane = rb.lane; used[rb.lane] = true; rc = roi_launch(ctx, rb, roi_regrown > 0); }
        const double t1 = g_job_stats ? mono_s() : 0;
        R.t1 = t1;
        if (g_job_stats) g_jobs_fine_s[1] += t1 - tl;
        if (g_job_stats) g_jobs_enqueue_s += t1 - t0;
    }
    ctx->cur_lane = lane0;
    return NVCA_OK;          // (a failed enqueue is carried in R.rc: the round is still waited for and closed by jobs_round_end)
}
static int jobs_round_end(nvca_ctx *ctx, DetectJob *const *jobs, int n, const int *lanes, int lane0, JobRound &R)
{
    const bool g_job_stats = ctx->sw.part_stats > 0;
    int rc = R.rc;
    bool (&used)[kLanes] = R.used;
    RoiBatch &rb = R.rb;
    int &roi_regrown = R.roi_regrown;
    const double t1 = R.t1;
    {
        for (int l = 0; l < kLanes; l++) {
            if (!used[l]) continue;
            const hipError_t he = hipStreamSynchronize(ctx->lane_streams[l]);
            if (he != hipSuccess && !rc) { ctx->set_error(std::string("hipStreamSynchronize: ") + hipGetErrorString(he)); rc = NVCA_ERR_HIP; }
        }
        ctx->cur_lane = lane0;
        const double t2 = g_job_stats ? mono_s() : 0;
        if (g_job_stats) g_jobs_wait_s += t2 - t1;
        if (g_job_stats && !rb.jobs.empty() && n >= ctx->sw.part_stats) {
            static int lines = 0;
            if (++lines > 200 && lines <= 212) {          // (a dozen rounds of the steady state: what a round holds and how long its launch took)
                int kinds[3] = {0, 0, 0}, narrowed = 0;
                for (DetectJob *o : rb.owners) { kinds[o->kind]++; if (o->roi_prev_phase == 2) narrowed++; }
                fprintf(stderr, "[nvca jobs] small-image round: %zu images (plain %d, scale-image %d, biggest-object %d of which narrowed %d), %zu workgroups, waited %.0f us\n",
                        rb.jobs.size(), kinds[0], kinds[1], kinds[2], narrowed, rb.steps.size(), (t2 - t1) * 1e6);
            }
        }
        struct Adv { double t; bool on; ~Adv() { if (on) g_jobs_advance_s += mono_s() - t; } } adv{t2, g_job_stats};
        drain_timer(ctx);
        bool roi_again = false;
        if (!rc && !rb.jobs.empty()) {
            ctx->cur_lane = rb.lane;
            const int r = roi_collect(ctx, rb);
            if (g_job_stats) g_jobs_fine_s[2] += mono_s() - t2;
            ctx->cur_lane = lane0;
            if (r == NVCA_ERR_OVERFLOW && roi_regrown < 2 && ctx->hit_cap_wanted > ctx->hit_cap) {
                // the round's candidate list was too short: its jobs are queued again, with room (see detect_job_advance)
                roi_regrown++; roi_again = true;
                if (g_job_stats) fprintf(stderr, "[nvca jobs] a small-image round overflowed its candidate list (cap %u for %zu jobs): queued again with %d per job\n", rb.cap, rb.jobs.size(), ctx->hit_cap_wanted);
                for (DetectJob *o : rb.owners) { o->phase = o->roi_prev_phase; o->fused = false; for (int k = 0; k < kJobImages; k++) o->rkeys[k].clear(); }
            } else if (r) rc = r;
        }
        // the small-path jobs' candidates are turned into rectangles, replayed (FIND_BIGGEST) and grouped job by job: independent
        // host work, shared with the context's helper threads (a job touches nothing but itself; set_error is locked)
        std::vector<DetectJob *> par;
        const double tp0 = g_job_stats ? mono_s() : 0;
        if (!rc && !roi_again)
            for (int i = 0; i < n; i++) if (jobs[i]->phase != 3 && jobs[i]->fused) par.push_back(jobs[i]);
        if (par.size() >= 4) {
            // the jobs with the most candidates first: the helpers take indices in order, the long ones must not come last
            auto weight = [](const DetectJob *j) { size_t w = 0; for (int k = 0; k < j->nimg; k++) w += j->rkeys[k].size(); return w; };
            std::stable_sort(par.begin(), par.end(), [&](const DetectJob *x, const DetectJob *y) { return weight(x) > weight(y); });
            ensure_pool(ctx);
            struct Arg { nvca_ctx *ctx; DetectJob **jobs; std::atomic<int> rc; } arg{ctx, par.data(), {0}};
            work_pool_run(ctx->pool, (int)par.size(), [](void *a, int i) {
                Arg *g = (Arg *)a;
                int r;
                try { r = detect_job_advance(g->ctx, *g->jobs[i]); }
                catch (const std::bad_alloc &) { r = NVCA_ERR_NOMEM; }
                catch (...) { r = NVCA_ERR_INTERNAL; }
                if (r) { g->jobs[i]->phase = 3; int z = 0; g->rc.compare_exchange_strong(z, r); }
            }, &arg);
            if (arg.rc.load()) rc = arg.rc.load();
            for (DetectJob *j : par) j->roi_prev_phase = -1;          // handled
        }
        const double tp1 = g_job_stats ? mono_s() : 0;
        if (g_job_stats) g_jobs_fine_s[3] += tp1 - tp0;
        for (int i = 0; i < n; i++) {
            if (jobs[i]->phase == 3) continue;
            if (rc) { if (jobs[i]->gp) { jobs[i]->gp->inflight--; jobs[i]->gp = nullptr; } jobs[i]->phase = 3; continue; }
            if (roi_again && std::find(rb.owners.begin(), rb.owners.end(), jobs[i]) != rb.owners.end()) continue;
            if (par.size() >= 4 && jobs[i]->roi_prev_phase == -1) { jobs[i]->roi_prev_phase = 0; continue; }
            ctx->cur_lane = lanes ? lanes[i] : lane0;
            const int r = detect_job_advance(ctx, *jobs[i]);
            if (r) rc = r;
        }
        ctx->cur_lane = lane0;
        if (g_job_stats) g_jobs_fine_s[4] += mono_s() - tp1;
        if (rc) {
            for (int i = 0; i < n; i++) { if (jobs[i]->gp) { jobs[i]->gp->inflight--; jobs[i]->gp = nullptr; } jobs[i]->phase = 3; }
            return rc;
        }
        return NVCA_OK;
    }
}
JobRound *job_round_new() { return new (std::nothrow) JobRound(); }
void job_round_free(JobRound *r) { delete r; }
// the first round of a job set, left queued (R from job_round_new).  Jobs that cannot take the small-image path make the caller
// wait for the round as before: *queued = false and nothing is launched.
int detect_jobs_begin(nvca_ctx *ctx, DetectJob *const *jobs, int n, const int *lanes, JobRound *R, bool *queued)
{
    *queued = false;
    for (int i = 0; i < n; i++) if (jobs[i]->phase != 0 || !roi_eligible(ctx, *jobs[i], n)) return NVCA_OK;
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
int run_detect_jobs(nvca_ctx *ctx, DetectJob *const *jobs, int n, const int *lanes)
{
    JobRound R;
    return detect_jobs_finish(ctx, jobs, n, lanes, &R, false);
}

} // namespace nvca

nvca::DetectJob *nvca::detect_job_new() { return new (std::nothrow) DetectJob(); }
void nvca::detect_job_free(DetectJob *j) { delete j; }
const std::vector<nvca_rect> &nvca::detect_job_out(const DetectJob *j, int k) { return j->out[k]; }
int nvca::detect_job_add_image(DetectJob *j, const void *image)
{
    if (j->kind == 2 || j->phase != 0 || j->nimg >= kJobImages) return -1;
    j->img[j->nimg] = image;
    return j->nimg++;
}

// fill in a job from detectMultiScale's arguments (flags decide the kind); NVCA_ERR_ARG for bad arguments
int nvca::make_detect_job(nvca_ctx *ctx, DetectJob &j, const nvca_cascade *casc, const void *gray, int w, int h, int stride, int mem,
                          double sf, int min_neighbors, int flags, int minw, int minh, int maxw, int maxh, bool raw_only)
{
    if (check_img(ctx, gray, w, h, stride, 1, mem) || !casc || !(sf > 1.0)) return NVCA_ERR_ARG;
    if (maxw == 0 || maxh == 0) { maxw = w; maxh = h; }
    j = DetectJob();
    j.casc = casc; j.img[0] = gray; j.nimg = 1; j.cols = w; j.rows = h; j.stride = stride; j.mem = mem;
    j.sf = sf; j.min_neighbors = min_neighbors; j.minw = minw; j.minh = minh; j.maxw = maxw; j.maxh = maxh; j.raw_only = raw_only;
    if (flags & NVCA_HAAR_FIND_BIGGEST_OBJECT) {
        flags &= ~(NVCA_HAAR_SCALE_IMAGE | NVCA_HAAR_DO_CANNY_PRUNING);
        if (raw_only) return NVCA_ERR_ARG;
        j.kind = 2;
    } else if (flags & NVCA_HAAR_SCALE_IMAGE) j.kind = 1;
    else j.kind = 0;
    j.flags = flags;
    return NVCA_OK;
}

extern "C" {

static int detect_gray(nvca_ctx *ctx, const nvca_cascade *casc, const void *gray, int w, int h, int stride, int mem,
                       double sf, int min_neighbors, int flags, int minw, int minh, int maxw, int maxh, bool raw_only,
                       std::vector<nvca_rect> &out)
{
    NVCA_LOCK_OR_FAIL(ctx);
    DetectJob j;
    int rc = make_detect_job(ctx, j, casc, gray, w, h, stride, mem, sf, min_neighbors, flags, minw, minh, maxw, maxh, raw_only);
    if (rc) return rc;
    DetectJob *jp = &j;
    if ((rc = run_detect_jobs(ctx, &jp, 1, nullptr))) return rc;
    out.swap(j.out[0]);
    return NVCA_OK;
}

int nvca_detect_multiscale(nvca_ctx *ctx, const nvca_cascade *cascade, const void *gray, int w, int h, int stride,
                           int mem, double scale_factor, int min_neighbors, int flags, int min_w, int min_h,
                           int max_w, int max_h, nvca_rect *out, int cap, int *n_out)
try {
    if (!n_out || cap < 0 || (cap > 0 && !out)) return NVCA_ERR_ARG;
    std::vector<nvca_rect> r;
    int rc = detect_gray(ctx, cascade, gray, w, h, stride, mem, scale_factor, min_neighbors, flags, min_w, min_h, max_w,
                         max_h, false, r);
    if (rc) return rc;
    *n_out = (int)r.size();
    for (int i = 0; i < std::min<int>(cap, (int)r.size()); i++) out[i] = r[i];
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)

int nvca_detect_raw(nvca_ctx *ctx, const nvca_cascade *cascade, const void *gray, int w, int h, int stride, int mem,
                    double scale_factor, int flags, int min_w, int min_h, int max_w, int max_h, nvca_rect *out,
                    int cap, int *n_out)
try {
    if (!n_out || cap < 0 || (cap > 0 && !out)) return NVCA_ERR_ARG;
    if (flags & NVCA_HAAR_FIND_BIGGEST_OBJECT) return NVCA_ERR_ARG;
    std::vector<nvca_rect> r;
    int rc = detect_gray(ctx, cascade, gray, w, h, stride, mem, scale_factor, 0, flags, min_w, min_h, max_w, max_h, true, r);
    if (rc) return rc;
    *n_out = (int)r.size();
    for (int i = 0; i < std::min<int>(cap, (int)r.size()); i++) out[i] = r[i];
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)

int nvca_group_rectangles(nvca_ctx *ctx, nvca_rect *rects, int n, int group_threshold, double eps, int *n_out)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (!ctx || n < 0 || (n > 0 && !rects) || !n_out) return NVCA_ERR_ARG;
    std::vector<nvca_rect> v(rects, rects + n);
    group_rectangles(v, group_threshold, eps);
    for (size_t i = 0; i < v.size(); i++) rects[i] = v[i];
    *n_out = (int)v.size();
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)

} // extern "C"
