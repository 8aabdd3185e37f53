// pyramid.cpp -- the image pyramid of the CV_HAAR_SCALE_IMAGE and new-format LBP scans on the device: a plan's layout (pyr_levels.h),
// resize tables and level table, a level's scan grid, and the launches that resize a job's images to every level and integrate them.
#include "host_state.h"
#include <climits>
#include <cstring>
#include <algorithm>

using namespace nvca;

namespace nvca {

// the plan's pyramid for a cols x rows image: the layout of `levels` and every level's resize table, the tables on the device
int pyr_plan_tabs(nvca_ctx *ctx, GeomPlan &np, int cols, int rows, const std::vector<SiLevel> &levels)
{
    // What a plan cannot hold is refused here, before anything is built: a call is answered from all of its levels or not at all.
    if (levels.size() > kMaxPyrLevels) { ctx->set_error("scan too large: more than 4095 pyramid levels (a scale factor this close to 1)"); return NVCA_ERR_ARG; }
    PyrLayout lay = pyr_layout(levels, cols);
    // (a level's planes lie at an int offset: PyrLevel::plane_off, LbpLevelDev, ScaleSpec)
    if (lay.plane_total > (size_t)INT_MAX) { ctx->set_error("scan too large: the pyramid's integral planes pass 2^31 elements an image"); return NVCA_ERR_ARG; }
    np.P = lay.P; np.gray_total = lay.gray_total; np.plane_total = lay.plane_total; np.lv = std::move(lay.lv);
    for (const PyrLevel &L : np.lv) {
        std::unique_ptr<GeomPlan> gp(new GeomPlan());
        build_resize_tab(cols, rows, L.szw, L.szh, gp->tab);
        np.level_tabs.push_back(std::move(gp));
    }
    return upload_tabs(ctx, np.level_tabs, np.d_level_tabs);
}

// the device level table of the one-launch pyramid kernels (the levels' resize tables are on the device)
int pyr_upload_levels(nvca_ctx *ctx, GeomPlan &np)
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

// both halves; a pyramid without levels has nothing on the device
int pyr_plan_init(nvca_ctx *ctx, GeomPlan &np, int cols, int rows, const std::vector<SiLevel> &levels)
{
    int rc;
    if ((rc = pyr_plan_tabs(ctx, np, cols, rows, levels)) || np.lv.empty()) return rc;
    return pyr_upload_levels(ctx, np);
}

// a level's scan grid as a plan scale: the unscaled ow x oh window on the level's planes (pitch P), every level_step pixels
ScaleSpec level_spec(int P, const PyrLevel &L, int ow, int oh, int adaptive)
{
    ScaleSpec sp;
    sp.table_factor = 1.; sp.plane_off = L.plane_off; sp.pitch = P; sp.plane_rows = L.szh + 1; sp.adaptive = adaptive;
    sp.out_factor = L.f; sp.out_w = L.winw; sp.out_h = L.winh;
    const int step = level_step(L.f);
    for (int i = 0, n = level_positions(L.szw, ow, step); i < n; i++) sp.xs.push_back(i * step);
    for (int i = 0, n = level_positions(L.szh, oh, step); i < n; i++) sp.ys.push_back(i * step);
    return sp;
}

// Device images of a job that sit at equal distances (the working images of a batched part call are carved that way) are read
// where they are; anything else is copied into the lane's gray slots first.
bool job_images_in_place(const DetectJob &j, size_t *slot)
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

// where a job's images are read from: in place when they allow it, otherwise copied into the lane's gray slots first
int pyr_job_source(nvca_ctx *ctx, const DetectJob &j, PyrSource &src)
{
    Workspace &ws = *ctx->ws;
    const int cols = j.rq.cols, rows = j.rq.rows, nimg = j.rq.nimg;
    int rc;
    PreGeom g0; make_geom(g0, cols, rows, j.rq.stride, 1, cols, rows);
    if ((rc = ensure_ws(ctx, g0, nimg))) return rc;
    src = PyrSource{ws.ln().gray.as<uint8_t>(), g0.gpitch, g0.gray_slot, nullptr};
    size_t in_place_slot = 0;
    if (job_images_in_place(j, &in_place_slot)) src = PyrSource{(const uint8_t *)j.rq.img[0], j.rq.stride, in_place_slot, nullptr};
    else
        for (int k = 0; k < nimg; k++)
            if ((rc = stage_2d(ctx, ws.ln().gray.as<uint8_t>() + g0.gray_slot * k, g0.gpitch, j.rq.img[k], j.rq.stride, cols, rows, j.rq.mem))) return rc;
    return NVCA_OK;
}

// `nimg` cols x rows images of `src` resized to every level of the plan's pyramid and integrated (the squared integral with them; the
// tilted one when asked).  The caller has sized the lane's pre-processing buffers for the images (ensure_ws).
int pyr_build(nvca_ctx *ctx, const PyrSource &src, int cols, int rows, int nimg, GeomPlan *pp, bool has_tilted)
{
    Workspace &ws = *ctx->ws;
    int rc;
    const int P = pp->P;
    const size_t gray_total = pp->gray_total, plane_total = pp->plane_total;
    // (the one-launch resize has a (level, image) pair in grid.z, which ends at 65535)
    if (pp->pyr_ok && pp->lv.size() * (size_t)nimg > 65535) { ctx->set_error("scan too large: pyramid levels x images of one job beyond 65535"); return NVCA_ERR_ARG; }
    if (ws.ln().aux.ensure(gray_total * nimg + 64) || ws.ln().sum.ensure((plane_total * nimg + 4 * (size_t)P) * sizeof(int)) || ws.ln().sqsum.ensure(plane_total * nimg * sizeof(unsigned long long)) ||
        (has_tilted && ws.ln().tilted.ensure((plane_total * nimg + 4 * (size_t)P) * sizeof(int)))) {
        ctx->set_error("allocation failed (pyramid)"); return NVCA_ERR_NOMEM;
    }
    if (has_tilted && (size_t)2 * (pp->pyr_maxw + pp->pyr_maxh + 2) * sizeof(int) > 64 * 1024) { ctx->set_error("image too large for the tilted integral"); return NVCA_ERR_ARG; }
    if (pp->pyr_ok) {            // all levels of all images: one resize launch, one integral launch
        { TimedLaunch t(ctx, NVCA_K_RESIZE1);
          launch_pyr_resize(ctx->cs(), src.img, cols, rows, src.pitch, src.slot, pp->d_pyr.as<PyrLevelDev>(),
                            (int)pp->lv.size(), nimg, pp->pyr_maxw, pp->pyr_maxh, ws.ln().aux.as<uint8_t>(), gray_total, src.luts); }
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
          launch_resize1(ctx->cs(), src.img, cols, rows, src.pitch, gp->view(), lg, L.szw, L.szh, L.gpitch, nullptr, nimg, src.slot, gray_total, src.luts); }
        PreGeom g; make_geom(g, L.szw, L.szh, L.gpitch, 1, L.szw, L.szh);
        g.gpitch = L.gpitch; g.spitch = P; g.sum_slot = plane_total; g.gray_slot = gray_total;
        run_integral(ctx, g, nullptr, nimg, lg, ws.ln().sum.as<int>() + L.plane_off,
                     (unsigned long long *)(ws.ln().sqsum.as<unsigned>() + L.plane_off));     // lo plane of the level; hi plane at + plane_total
        if (has_tilted && (rc = run_tilted(ctx, g, nullptr, nimg, lg, ws.ln().tilted.as<int>() + L.plane_off))) return rc;
    }
    return NVCA_OK;
}

} // namespace nvca
