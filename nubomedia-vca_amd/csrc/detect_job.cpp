// detect_job.cpp -- the launch sets of one detectMultiScale job: the plain scan, CV_HAAR_SCALE_IMAGE and the two sets of a
// CV_HAAR_FIND_BIGGEST_OBJECT search (the search itself: fb_search.cpp), and what a drained set's candidates become.
#include "host_state.h"
#include "host_logic.h"
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

// The pyramid levels of cvHaarDetectObjectsForROC's CV_HAAR_SCALE_IMAGE branch with its break / continue rules
std::vector<SiLevel> si_levels(int ow, int oh, int cols, int rows, double sf, int minw, int minh, int maxw, int maxh, size_t cap)
{
    std::vector<SiLevel> lv;
    for (double factor = 1; lv.size() < cap; factor *= sf) {
        const int winw = cv_round(ow * factor), winh = cv_round(oh * factor);
        const int szw = cv_round(cols / factor), szh = cv_round(rows / factor);
        if (szw - ow + 1 <= 0 || szh - oh + 1 <= 0) break;
        if (winw > maxw || winh > maxh) break;
        if (winw < minw || winh < minh) continue;
        if (szw + 1 <= 1 + ow) continue;                   // HaarDetectObjects_ScaleImage_Invoker's early return
        lv.push_back(SiLevel{factor, szw, szh, winw, winh});
    }
    return lv;
}

// The pyramid levels of cv::CascadeClassifier::detectMultiScale on a new-format cascade (OpenCV 2.4 cascadedetect.cpp; SURVEY.md
// A.15).  si_levels' sibling; its rules differ in two places: a level needs sz - window > 0 (no + 1: the last column and row of
// window positions are never visited), and there is no scale-image invoker's early return.
std::vector<SiLevel> lbp_levels(int ow, int oh, int cols, int rows, double sf, int minw, int minh, int maxw, int maxh, size_t cap)
{
    std::vector<SiLevel> lv;
    for (double factor = 1; lv.size() < cap; factor *= sf) {
        const int winw = cv_round(ow * factor), winh = cv_round(oh * factor);
        const int szw = cv_round(cols / factor), szh = cv_round(rows / factor);
        if (szw - ow <= 0 || szh - oh <= 0) break;
        if (winw > maxw || winh > maxh) break;
        if (winw < minw || winh < minh) continue;
        lv.push_back(SiLevel{factor, szw, szh, winw, winh});
    }
    return lv;
}

// the layout of a pyramid inside the lane's gray / plane buffers: level after level
static void pyr_add_level(GeomPlan &np, const SiLevel &sl)
{
    PyrLevel L; L.f = sl.factor; L.szw = sl.szw; L.szh = sl.szh; L.winw = sl.winw; L.winh = sl.winh;
    L.gpitch = (int)round_up(L.szw, 64); L.gray_off = np.gray_total; L.plane_off = (int)np.plane_total;
    np.gray_total += round_up((size_t)L.gpitch * L.szh, 256);
    np.plane_total += round_up((size_t)np.P * (L.szh + 1), 64);
    np.lv.push_back(L);
}

// the device level table of the one-launch pyramid kernels (the levels' resize tables are on the device)
static int pyr_upload_levels(nvca_ctx *ctx, GeomPlan &np)
{
    std::vector<PyrLevelDev> dl(np.lv.size());
    np.pyr_ok = !ctx->sw.pyr_off;
    for (size_t li = 0; li < np.lv.size(); li++) {
        const PyrLevel &L = np.lv[li]; GeomPlan *t = np.level_tabs[li].get();
        PyrLevelDev &d = dl[li]; memset(&d, 0, sizeof(d));
        d.szw = L.szw; d.szh = L.szh; d.gpitch = L.gpitch; d.plane_off = L.plane_off;
        d.gray_off = (long long)L.gray_off;
        d.tab = t->view();
        np.pyr_maxw = std::max(np.pyr_maxw, L.szw); np.pyr_maxh = std::max(np.pyr_maxh, L.szh);
        if (L.szw > 1023) np.pyr_ok = false;            // one column per thread, plus the zero column
    }
    if (np.d_pyr.ensure(dl.size() * sizeof(PyrLevelDev))) { ctx->set_error("allocation failed (pyramid table)"); return NVCA_ERR_NOMEM; }
    NVCA_HIP_CHECK(ctx, hipMemcpy(np.d_pyr.p, dl.data(), dl.size() * sizeof(PyrLevelDev), hipMemcpyHostToDevice));
    return NVCA_OK;
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
        np->P = (int)round_up(cols + 1, 8);
        for (const SiLevel &sl : si_levels(c.ow, c.oh, cols, rows, j.rq.sf, j.rq.minw, j.rq.minh, j.rq.maxw, j.rq.maxh, 63)) pyr_add_level(*np, sl);          // (a plan holds at most 63 levels)
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
            if ((rc = pyr_upload_levels(ctx, *np))) return rc;
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
    if (j.rq.mem != NVCA_MEM_DEVICE) return false;
    *slot = 0;
    if (j.rq.nimg == 1) return true;
    const uint8_t *a = (const uint8_t *)j.rq.img[0], *b = (const uint8_t *)j.rq.img[1];
    if (b <= a) return false;
    const size_t d = (size_t)(b - a);
    if (d < (size_t)j.rq.stride * (j.rq.rows - 1) + j.rq.cols) return false;
    for (int k = 2; k < j.rq.nimg; k++) if ((const uint8_t *)j.rq.img[k] != a + d * k) return false;
    *slot = d;
    return true;
}

// the job's images resized to every level of the plan's pyramid and integrated (the squared integral with them; the tilted one when asked)
static int pyr_build(nvca_ctx *ctx, DetectJob &j, GeomPlan *pp, bool has_tilted)
{
    Workspace &ws = *ctx->ws;
    const int cols = j.rq.cols, rows = j.rq.rows, nimg = j.rq.nimg;
    int rc;
    const int P = pp->P;
    const size_t gray_total = pp->gray_total, plane_total = pp->plane_total;
    PreGeom g0; make_geom(g0, cols, rows, j.rq.stride, 1, cols, rows);
    if ((rc = ensure_ws(ctx, g0, nimg))) return rc;
    if (ws.ln().aux.ensure(gray_total * nimg + 64) || ws.ln().sum.ensure((plane_total * nimg + 4 * (size_t)P) * sizeof(int)) || ws.ln().sqsum.ensure(plane_total * nimg * sizeof(unsigned long long)) ||
        (has_tilted && ws.ln().tilted.ensure((plane_total * nimg + 4 * (size_t)P) * sizeof(int)))) {
        ctx->set_error("allocation failed (pyramid)"); return NVCA_ERR_NOMEM;
    }
    if (has_tilted && (size_t)2 * (pp->pyr_maxw + pp->pyr_maxh + 2) * sizeof(int) > 64 * 1024) { ctx->set_error("image too large for the tilted integral"); return NVCA_ERR_ARG; }
    const uint8_t *src0 = ws.ln().gray.as<uint8_t>(); int spitch0 = g0.gpitch; size_t sslot0 = g0.gray_slot;
    size_t in_place_slot = 0;
    if (job_images_in_place(j, &in_place_slot)) { src0 = (const uint8_t *)j.rq.img[0]; spitch0 = j.rq.stride; sslot0 = in_place_slot; }
    else
        for (int k = 0; k < nimg; k++)
            if ((rc = stage_2d(ctx, ws.ln().gray.as<uint8_t>() + g0.gray_slot * k, g0.gpitch, j.rq.img[k], j.rq.stride, cols, rows, j.rq.mem))) return rc;
    if (pp->pyr_ok) {            // all levels of all images: one resize launch, one integral launch
        { TimedLaunch t(ctx, NVCA_K_RESIZE1);
          launch_pyr_resize(ctx->cs(), src0, cols, rows, spitch0, sslot0, pp->d_pyr.as<PyrLevelDev>(),
                            (int)pp->lv.size(), nimg, pp->pyr_maxw, pp->pyr_maxh, ws.ln().aux.as<uint8_t>(), gray_total); }
        { TimedLaunch t(ctx, NVCA_K_INTEGRAL);
          launch_pyr_integral(ctx->cs(), ws.ln().aux.as<uint8_t>(), gray_total, pp->d_pyr.as<PyrLevelDev>(), (int)pp->lv.size(), nimg,
                              ws.ln().sum.as<int>(), ws.ln().sqsum.as<unsigned>(), plane_total, P); }
        if (has_tilted) {          // cvIntegral(&img1, &sum1, &sqsum1, _tilted) per level
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
          launch_resize1(ctx->cs(), src0, cols, rows, spitch0, gp->view(), lg, L.szw, L.szh, L.gpitch, nullptr, nimg, sslot0, gray_total); }
        PreGeom g; make_geom(g, L.szw, L.szh, L.gpitch, 1, L.szw, L.szh);
        g.gpitch = L.gpitch; g.spitch = P; g.sum_slot = plane_total; g.gray_slot = gray_total;
        run_integral(ctx, g, nullptr, nimg, lg, ws.ln().sum.as<int>() + L.plane_off,
                     (unsigned long long *)(ws.ln().sqsum.as<unsigned>() + L.plane_off));     // lo plane of the level; hi plane at + plane_total
        if (has_tilted && (rc = run_tilted(ctx, g, nullptr, nimg, lg, ws.ln().tilted.as<int>() + L.plane_off))) return rc;
    }
    return NVCA_OK;
}

static int si_enqueue(nvca_ctx *ctx, DetectJob &j, int r0, int total)
{
    GeomPlan *pp = nullptr;
    int rc;
    if ((rc = si_plan(ctx, j, &pp))) return rc;
    j.q.phase = kJobFirstQueued; j.q.dp = nullptr;
    if (pp->lv.empty()) return NVCA_OK;
    if ((rc = pyr_build(ctx, j, pp, j.rq.casc->c.has_tilted))) return rc;
    j.q.cj = CascadeJob(); j.q.cj.r0 = r0; j.q.cj.n = j.rq.nimg; j.q.cj.total = total;
    if ((rc = cascade_enqueue(ctx, pp->det, pp->plane_total, pp->P, j.q.cj, nullptr, false))) return rc;
    j.q.gp = pp; pp->inflight++; j.q.dp = &pp->det;
    return NVCA_OK;
}

// cv::CascadeClassifier::detectMultiScale on a new-format LBP cascade (OpenCV 2.4 cascadedetect.cpp): the pyramid of
// CV_HAAR_SCALE_IMAGE with its own level rules, scanned by the LBP evaluator (kernels_cascade_lbp.hip).  The plan holds the pyramid
// (layout, resize tables), one scan grid per level and the cascade's tables at the pitch of the planes and of the stage-0 tile.
static int lbp_plan(nvca_ctx *ctx, const DetectJob &j, GeomPlan **out)
{
    const LbpCascade &c = j.rq.casc->lbp;
    const int cols = j.rq.cols, rows = j.rq.rows;
    int rc;
    char key[256];
    snprintf(key, sizeof(key), "LBP|%llu|%d|%d|%.17g|%d|%d|%d|%d", (unsigned long long)j.rq.casc->c.uid, cols, rows, j.rq.sf, j.rq.minw, j.rq.minh, j.rq.maxw, j.rq.maxh);
    GeomPlan *pp = find_plan(ctx, key);
    if (!pp) {
        std::unique_ptr<GeomPlan> np(new GeomPlan());
        np->P = (int)round_up(cols + 1, 8);
        for (const SiLevel &sl : lbp_levels(c.ow, c.oh, cols, rows, j.rq.sf, j.rq.minw, j.rq.minh, j.rq.maxw, j.rq.maxh, 63)) pyr_add_level(*np, sl);
        if (!np->lv.empty()) {
            for (const PyrLevel &L : np->lv) {
                std::unique_ptr<GeomPlan> gp(new GeomPlan());
                build_resize_tab(cols, rows, L.szw, L.szh, gp->tab);
                np->level_tabs.push_back(std::move(gp));
            }
            if ((rc = upload_tabs(ctx, np->level_tabs, np->d_level_tabs))) return rc;
            if ((rc = pyr_upload_levels(ctx, *np))) return rc;
            // the scan grids: what hit_valid / hit_rect check and map a candidate key with, and the evaluator's level records
            LbpPlan &lp = np->lbp;
            std::vector<LbpLevelDev> levels; std::vector<LbpTile> tiles;
            size_t bit_words = 0; int nrows = 0; size_t positions = 0;
            for (size_t li = 0; li < np->lv.size(); li++) {
                const PyrLevel &L = np->lv[li];
                ScaleSpec sp;
                sp.table_factor = 1.; sp.plane_off = L.plane_off; sp.pitch = np->P; sp.plane_rows = L.szh + 1; sp.adaptive = 1;
                sp.out_factor = L.f; sp.out_w = L.winw; sp.out_h = L.winh;
                const int step = L.f > 2. ? 1 : 2;
                for (int x = 0; x < L.szw - c.ow; x += step) sp.xs.push_back(x);
                for (int y = 0; y < L.szh - c.oh; y += step) sp.ys.push_back(y);
                LbpLevelDev d; memset(&d, 0, sizeof(d));
                d.plane_off = L.plane_off; d.szw = L.szw; d.szh = L.szh; d.nx = (int)sp.xs.size(); d.ny = (int)sp.ys.size(); d.step = step;
                d.wpr = (d.nx + kLbpTileW - 1) / kLbpTileW; d.bit_off = (int)bit_words; d.row_first = nrows;
                bit_words += (size_t)d.wpr * d.ny; nrows += d.ny; positions += (size_t)d.nx * d.ny;
                for (int ty = 0; ty * kLbpTileH < d.ny; ty++)
                    for (int tx = 0; tx < d.wpr; tx++) tiles.push_back(LbpTile{(int)li, tx, ty, 0});
                levels.push_back(d);
                np->det.specs.push_back(std::move(sp));
            }
            {   // the candidate key, sized as DetectPlan::build_tables sizes it
                auto bits = [](size_t n) { int b = 1; while ((1ull << b) < n) b++; return b; };
                size_t mx = 1, my = 1;
                for (const ScaleSpec &sp : np->det.specs) { mx = std::max(mx, sp.xs.size()); my = std::max(my, sp.ys.size()); }
                const int bx = bits(mx), by = bits(my), bs = bits(np->det.specs.size());
                if (bx + by + bs > 32 || bit_words > (1u << 30) || positions > (1u << 30)) { ctx->set_error("scan too large for the candidate key (levels x rows x columns of windows beyond 2^32)"); return NVCA_ERR_ARG; }
                np->det.key_sy = bx; np->det.key_ss = bx + by;
            }
            const int TP = lbp_tile_pitch(c.ow);
            std::vector<LbpWeakDev> gweak(c.weak.size()), tweak(c.weak.size());
            for (size_t i = 0; i < c.weak.size(); i++) {
                const LbpWeak &w = c.weak[i]; const LbpFeature &f = c.features[(size_t)w.feature];
                for (std::vector<LbpWeakDev> *tab : {&gweak, &tweak}) {
                    LbpWeakDev &d = (*tab)[i]; memset(&d, 0, sizeof(d));
                    const int pitch = tab == &gweak ? np->P : TP;
                    for (int r = 0; r < 4; r++)
                        for (int q = 0; q < 4; q++) d.off[r * 4 + q] = (f.y + r * f.h) * pitch + f.x + q * f.w;
                    memcpy(d.subset, w.subset, sizeof(d.subset)); d.leaf[0] = w.leaf[0]; d.leaf[1] = w.leaf[1];
                }
            }
            std::vector<LbpStageDev> stages;
            for (const LbpStage &st : c.stages) stages.push_back(LbpStageDev{st.first, st.count, st.threshold, 0});
            // one allocation and one copy for all tables
            struct Item { const void *h; size_t n; size_t off; } items[] = {
                {levels.data(), levels.size() * sizeof(LbpLevelDev), 0}, {tiles.data(), tiles.size() * sizeof(LbpTile), 0},
                {stages.data(), stages.size() * sizeof(LbpStageDev), 0}, {gweak.data(), gweak.size() * sizeof(LbpWeakDev), 0},
                {tweak.data(), tweak.size() * sizeof(LbpWeakDev), 0}};
            size_t total = 0;
            for (Item &it : items) { it.off = total; total += (it.n + 255) & ~(size_t)255; }
            std::vector<unsigned char> blob(total);
            for (Item &it : items) memcpy(blob.data() + it.off, it.h, it.n);
            if (lp.d_blob.ensure(total)) { ctx->set_error("hipMalloc failed for plan tables"); return NVCA_ERR_NOMEM; }
            NVCA_HIP_CHECK(ctx, hipMemcpy(lp.d_blob.p, blob.data(), total, hipMemcpyHostToDevice));
            LbpArgs &a = lp.args; memset(&a, 0, sizeof(a));
            const unsigned char *base = lp.d_blob.as<unsigned char>();
            a.levels = (const LbpLevelDev *)(base + items[0].off); a.nlev = (int)levels.size();
            a.tiles = (const LbpTile *)(base + items[1].off); a.ntiles = (int)tiles.size();
            a.stages = (const LbpStageDev *)(base + items[2].off); a.nstages = (int)stages.size();
            a.gweak = (const LbpWeakDev *)(base + items[3].off); a.tweak = (const LbpWeakDev *)(base + items[4].off);
            a.P = np->P; a.TP = TP; a.ow = c.ow; a.oh = c.oh; a.nrows = nrows;
            a.key_sy = np->det.key_sy; a.key_ss = np->det.key_ss;
            a.tile_stages = std::min(a.nstages, 3);          // at LDS speed while most windows are alive; later stages see scattered survivors
            lp.bit_words = bit_words; lp.positions = positions;
            // the stage-0 tile at step 2 (the larger one); a window too large for 64 KiB of LDS gathers from the plane instead
            const size_t lds = (size_t)TP * lbp_tile_rows(c.oh, 2) * sizeof(int);
            lp.lds = lds <= 64 * 1024 ? (int)lds : 0;
        }
        pp = store_plan(ctx, key, std::move(np));
    }
    *out = pp;
    return NVCA_OK;
}

static int lbp_enqueue(nvca_ctx *ctx, DetectJob &j, int r0, int total)
{
    Workspace &ws = *ctx->ws;
    ResultBufs &rb = ws.res[ws.cur_res];
    GeomPlan *pp = nullptr;
    int rc;
    if ((rc = lbp_plan(ctx, j, &pp))) return rc;
    j.q.phase = kJobFirstQueued; j.q.dp = nullptr;
    if (pp->lv.empty()) return NVCA_OK;
    // (the pyramid launchers write the squared integral with the sum: it is computed and ignored here)
    if ((rc = pyr_build(ctx, j, pp, false))) return rc;
    const LbpPlan &lp = pp->lbp;
    const int tot = std::max(total, r0 + 1);
    const size_t hits_stride = (size_t)ctx->hit_cap + 1;
    constexpr size_t kCnt = 64;                       // list counters in front of the first list
    if (ws.ln().failbits.ensure(2 * lp.bit_words * sizeof(unsigned) + 8) || ws.ln().deep.ensure((kCnt + lp.positions) * sizeof(unsigned)) ||
        ws.ln().vnf.ensure(lp.positions * sizeof(unsigned) + 8) ||
        rb.hits.ensure(hits_stride * tot * sizeof(unsigned long long)) || rb.h_hits.ensure(hits_stride * tot * sizeof(unsigned long long))) {
        ctx->set_error("device allocation failed for the cascade workspace"); return NVCA_ERR_NOMEM;
    }
    CascadeJob &cj = j.q.cj;
    cj = CascadeJob(); cj.r0 = r0; cj.n = 1; cj.total = total;
    cj.cap = (unsigned)ctx->hit_cap;
    cj.d_hits = rb.hits.as<unsigned long long>() + hits_stride * r0;
    cj.h_hits = rb.h_hits.as<unsigned long long>() + hits_stride * r0;
    NVCA_HIP_CHECK(ctx, hipMemsetAsync(cj.d_hits, 0, sizeof(unsigned long long), ctx->cs()));
    NVCA_HIP_CHECK(ctx, hipMemsetAsync(ws.ln().deep.p, 0, kCnt * sizeof(unsigned), ctx->cs()));
    LbpArgs a = lp.args;
    a.sum = ws.ln().sum.as<int>();
    a.bits = ws.ln().failbits.as<unsigned>(); a.bits2 = a.bits + lp.bit_words;
    a.cnt = ws.ln().deep.as<unsigned>();
    a.list[0] = ws.ln().deep.as<unsigned>() + kCnt; a.list[1] = ws.ln().vnf.as<unsigned>(); a.list_cap = (unsigned)lp.positions;
    a.hits = cj.d_hits; a.hit_cap = cj.cap;
    {   // the first stages everywhere, the serial walk's skip rule, then the later stages group by group on ever shorter survivor
        // lists (groups of 2, 3, 4 ... stages: survivors thin out by about half per stage).  All booked as "window per lane".
        TimedLaunch t(ctx, NVCA_K_STRIP);
        launch_lbp_stage0(ctx->cs(), a, lp.lds);
        launch_lbp_walk(ctx->cs(), a);
        int g = 0;
        for (int s0 = a.tile_stages, len = 2; s0 < a.nstages && g + 1 < (int)kCnt; s0 += len, len++, g++) {
            // (the last group takes every stage that is left: the counters bound the number of groups)
            const int s1 = g + 2 == (int)kCnt ? a.nstages : std::min(a.nstages, s0 + len);
            launch_lbp_rest(ctx->cs(), a, s0, s1, g & 1, g, (unsigned)lp.positions);
            if (s1 >= a.nstages) break;
        }
    }
    NVCA_LAUNCH_CHECK(ctx);
    cj.first = std::min<size_t>(cj.cap, 2048);
    NVCA_HIP_CHECK(ctx, hipMemcpyAsync(cj.h_hits, cj.d_hits, (cj.first + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->cs()));
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
    bool have = j.q.dp != nullptr;
    const bool was_fused = j.sm.fused;
    if (j.sm.fused) {
        // candidates of the round's k_roi launch, sorted into the serial order (step, row, column) -> rectangle
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
        have = true;
    } else
    if (j.q.dp) rc = cascade_collect(ctx, *j.q.dp, j.q.cj, raw, j.rq.kind == kJobPlain ? &grouped : nullptr, j.rq.kind == kJobBiggest ? &sc : nullptr);
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
    if (j->rq.kind == kJobBiggest || j->rq.kind == kJobLbp || j->q.phase != kJobNew || j->rq.nimg >= kJobImages) return -1;
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
    if (casc->format == NVCA_CASCADE_LBP) j.rq.kind = kJobLbp;           // the new-format scan ignores flags (cascadedetect.cpp)
    else if (flags & NVCA_HAAR_FIND_BIGGEST_OBJECT) {
        flags &= ~(NVCA_HAAR_SCALE_IMAGE | NVCA_HAAR_DO_CANNY_PRUNING);
        if (raw_only) return NVCA_ERR_ARG;
        j.rq.kind = kJobBiggest;
    } else if (flags & NVCA_HAAR_SCALE_IMAGE) j.rq.kind = kJobScaleImage;
    else j.rq.kind = kJobPlain;
    j.rq.flags = flags;
    return NVCA_OK;
}
