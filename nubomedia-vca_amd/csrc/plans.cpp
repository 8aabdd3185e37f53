// plans.cpp -- the plan cache (per cascade and geometry: working-image geometry, resize tables, scan tables), workspace sizing,
// and the launch sequences of the integral and cascade passes (a cascade job is enqueued, then collected after its stream drains).
#include "host_state.h"
#include "host_logic.h"
#include <cstdio>
#include <cstring>
#include <algorithm>

using namespace nvca;

namespace nvca {

static RowCopy make_rowcopy(const ResizeTab &t)
{
    RowCopy rc;
    if (t.mode != 1 || t.dh <= 0) return rc;
    std::vector<int> rows;
    auto clampr = [&](int r) { return r >= 0 ? (r < t.sh ? r : t.sh - 1) : 0; };
    for (int dy = 0; dy < t.dh; dy++) { rows.push_back(clampr(t.yofs[dy])); rows.push_back(clampr(t.yofs[dy] + 1)); }
    std::sort(rows.begin(), rows.end());
    rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
    if (rows.size() * 2 > (size_t)t.sh) return rc;              // no saving worth a strided copy
    std::vector<std::pair<int, int>> runs;                          // maximal runs of consecutive rows
    for (int r : rows) { if (!runs.empty() && runs.back().first + runs.back().second == r) runs.back().second++; else runs.push_back({r, 1}); }
    const int period = runs.size() > 1 ? runs[1].first - runs[0].first : t.sh;
    for (size_t i = 0; i < runs.size(); i++)
        if (runs[i].second != runs[0].second || runs[i].first != runs[0].first + (int)i * period) return rc;
    rc.on = true; rc.first = runs[0].first; rc.period = period; rc.run = runs[0].second; rc.count = (int)runs.size();
    return rc;
}

DetectPlan::~DetectPlan()
{
    release_tables();
    d_scales.release(); d_stages.release(); d_strips.release(); d_pos.release(); d_order.release(); d_tasks.release(); d_tiles.release(); d_tile_order.release(); d_tcoords.release(); d_bands.release(); d_band_order.release(); d_deeprecs.release(); d_stage_hint.release(); d_stage_first.release(); d_stage_thr.release(); d_blob.release();
}

// one device allocation and one copy for all tables of a plan (a FIND_BIGGEST scan builds a plan per scale, per call)
size_t TableBlob::add(const void *h, size_t n)
{
    const size_t off = bytes.size();
    bytes.resize(off + ((n + 255) & ~(size_t)255));
    if (n && h) memcpy(bytes.data() + off, h, n);
    return off;
}
int TableBlob::upload(nvca_ctx *ctx, DevBuf &blob)
{
    if (blob.ensure(bytes.size())) { ctx->set_error("hipMalloc failed for plan tables"); return NVCA_ERR_NOMEM; }
    NVCA_HIP_CHECK(ctx, hipMemcpy(blob.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
    return NVCA_OK;
}

int DetectPlan::upload(nvca_ctx *ctx)
{
    struct Item { DevBuf *d; const void *h; size_t n; size_t off; } items[] = {
        {&d_scales, scales.data(), scales.size() * sizeof(ScaleRec)},
        {&d_stages, stages.data(), stages.size() * sizeof(StageRec)},
        {&d_strips, strips.data(), strips.size() * sizeof(StripRec)},
        {&d_pos, pos.data(), pos.size() * sizeof(int)},
        {&d_order, order.data(), order.size() * sizeof(int)},
        {&d_tasks, tasks.data(), tasks.size() * sizeof(unsigned)},
        {&d_tiles, tiles.data(), tiles.size() * sizeof(TileRec)},
        {&d_tile_order, tile_order.data(), tile_order.size() * sizeof(int)},
        {&d_tcoords, tcoords.data(), tcoords.size() * sizeof(unsigned short)},
        {&d_bands, bands.data(), bands.size() * sizeof(BandRec)},
        {&d_band_order, band_order.data(), band_order.size() * sizeof(int)},
        {&d_deeprecs, deeprecs.data(), deeprecs.size() * sizeof(DeepRec)},
        {&d_stage_hint, nullptr, tiles.empty() ? (size_t)0 : 8 * sizeof(int)},          // zero: nothing known yet
        {&d_stage_first, stage_first.data(), stage_first.size() * sizeof(int)},
        {&d_stage_thr, stage_thr.data(), stage_thr.size() * sizeof(float)},
    };
    TableBlob blob;
    for (auto &it : items) it.off = blob.add(it.h, it.n);
    if (blob.bytes.empty()) return NVCA_OK;
    for (auto &it : items) it.d->release();
    int rc;
    if ((rc = blob.upload(ctx, d_blob))) return rc;
    for (auto &it : items) { it.d->p = it.n ? (unsigned char *)d_blob.p + it.off : nullptr; it.d->bytes = 0; }       // views
    return NVCA_OK;
}

void make_geom(PreGeom &g, int sw, int sh, int sstride, int cn, int w, int h)
{
    memset(&g, 0, sizeof(g));
    g.sw = sw; g.sh = sh; g.sstride = sstride; g.cn = cn;
    g.w = w; g.h = h;
    g.gpitch = (int)round_up(w, 64);
    g.spitch = (int)round_up(w + 1, 8);
    g.nbands = (h + kIntegralBand - 1) / kIntegralBand;
    g.gray_slot = round_up((size_t)g.gpitch * h, 256);
    g.sum_slot = round_up((size_t)g.spitch * (h + 1), 64);
    g.band_slot = (size_t)g.nbands * round_up(w, 8);
}

int ensure_ws(nvca_ctx *ctx, const PreGeom &g, int batch)
{
    Workspace &ws = *ctx->ws;
    int e = 0;
    e |= ws.ln().gray.ensure(g.gray_slot * batch + 64);
    { void *old = ws.ln().hist.p; e |= ws.ln().hist.ensure((size_t)batch * 256 * sizeof(unsigned)); if (ws.ln().hist.p != old) ws.ln().hist_clean = 0; }
    e |= ws.ln().lut.ensure((size_t)batch * 256);
    e |= ws.ln().bandsum.ensure(g.band_slot * batch * sizeof(unsigned));
    e |= ws.ln().bandsq.ensure(g.band_slot * batch * sizeof(unsigned));
    e |= ws.ln().sum.ensure((g.sum_slot * batch + 4 * (size_t)g.spitch) * sizeof(int));      // a few spare rows: a scaled feature corner may round past the window by a pixel or two
    e |= ws.ln().sqsum.ensure(g.sum_slot * batch * sizeof(unsigned long long));
    e |= ws.res[ws.cur_res].srcptrs.ensure((size_t)batch * sizeof(void *));
    e |= ws.res[ws.cur_res].h_srcptrs.ensure((size_t)batch * sizeof(void *));
    if (e) { ctx->set_error("device/pinned allocation failed for the workspace"); return NVCA_ERR_NOMEM; }
    return NVCA_OK;
}

static int upload_tab(nvca_ctx *ctx, GeomPlan &gp)
{
    const ResizeTab &t = gp.tab;
    if (t.mode != 1) return NVCA_OK;
    if (gp.d_xofs.ensure(t.xofs.size() * 4) || gp.d_yofs.ensure(t.yofs.size() * 4) ||
        gp.d_ialpha.ensure(t.ialpha.size() * 2) || gp.d_ibeta.ensure(t.ibeta.size() * 2)) {
        ctx->set_error("hipMalloc failed for resize tables"); return NVCA_ERR_NOMEM;
    }
    NVCA_HIP_CHECK(ctx, hipMemcpy(gp.d_xofs.p, t.xofs.data(), t.xofs.size() * 4, hipMemcpyHostToDevice));
    NVCA_HIP_CHECK(ctx, hipMemcpy(gp.d_yofs.p, t.yofs.data(), t.yofs.size() * 4, hipMemcpyHostToDevice));
    NVCA_HIP_CHECK(ctx, hipMemcpy(gp.d_ialpha.p, t.ialpha.data(), t.ialpha.size() * 2, hipMemcpyHostToDevice));
    NVCA_HIP_CHECK(ctx, hipMemcpy(gp.d_ibeta.p, t.ibeta.data(), t.ibeta.size() * 2, hipMemcpyHostToDevice));
    return NVCA_OK;
}

// the resize tables of several levels in one allocation (owned by `blob`) and one copy; the levels' buffers become views
int upload_tabs(nvca_ctx *ctx, std::vector<std::unique_ptr<GeomPlan>> &levels, DevBuf &blob)
{
    auto al = [](size_t n) { return (n + 255) & ~(size_t)255; };
    size_t total = 0;
    for (auto &gp : levels) { const ResizeTab &t = gp->tab; if (t.mode != 1) continue; total += al(t.xofs.size() * 4) + al(t.yofs.size() * 4) + al(t.ialpha.size() * 2) + al(t.ibeta.size() * 2); }
    if (!total) return NVCA_OK;
    std::vector<unsigned char> h(total);
    if (blob.ensure(total)) { ctx->set_error("hipMalloc failed for resize tables"); return NVCA_ERR_NOMEM; }
    size_t off = 0;
    auto put = [&](DevBuf &d, const void *src, size_t n) { memcpy(h.data() + off, src, n); d.release(); d.p = (unsigned char *)blob.p + off; d.bytes = 0; off += al(n); };
    for (auto &gp : levels) {
        const ResizeTab &t = gp->tab;
        if (t.mode != 1) continue;
        put(gp->d_xofs, t.xofs.data(), t.xofs.size() * 4); put(gp->d_yofs, t.yofs.data(), t.yofs.size() * 4);
        put(gp->d_ialpha, t.ialpha.data(), t.ialpha.size() * 2); put(gp->d_ibeta, t.ibeta.data(), t.ibeta.size() * 2);
    }
    NVCA_HIP_CHECK(ctx, hipMemcpy(blob.p, h.data(), total, hipMemcpyHostToDevice));
    return NVCA_OK;
}

// ---- launch sequences ----------------------------------------------------

// integral planes for `batch` slots (lut == nullptr -> identity); gray / sum / sq default to the workspace planes
void run_integral(nvca_ctx *ctx, const PreGeom &g, const uint8_t *lut, int batch, const uint8_t *gray, int *sum,
                  unsigned long long *sq)
{
    Workspace &ws = *ctx->ws;
    if (!gray) gray = ws.ln().gray.as<uint8_t>();
    if (!sum) sum = ws.ln().sum.as<int>();
    if (!sq) sq = ws.ln().sqsum.as<unsigned long long>();
    if (batch <= 64 && small_integral_fits(g)) {         // small images (ROI searches and working images of the part detectors): one launch, a workgroup per image
        TimedLaunch t(ctx, NVCA_K_INTEGRAL);
        launch_small_integral(ctx->cs(), gray, lut, 256, g, sum, sq, batch);
        return;
    }
    { TimedLaunch t(ctx, NVCA_K_COLSUM);
      launch_colsum(ctx->cs(), gray, lut, 256, g, ws.ln().bandsum.as<unsigned>(), ws.ln().bandsq.as<unsigned>(), batch); }
    { TimedLaunch t(ctx, NVCA_K_BANDSCAN);
      launch_bandscan(ctx->cs(), g, ws.ln().bandsum.as<unsigned>(), ws.ln().bandsq.as<unsigned>(), batch); }
    { TimedLaunch t(ctx, NVCA_K_INTEGRAL);
      launch_integral(ctx->cs(), gray, lut, 256, g, ws.ln().bandsum.as<unsigned>(), ws.ln().bandsq.as<unsigned>(), sum, sq, batch); }
}

// tilted integral planes for `batch` slots (cascades with tilted features only); same geometry and equalisation LUT as run_integral
int run_tilted(nvca_ctx *ctx, const PreGeom &g, const uint8_t *lut, int batch, const uint8_t *gray, int *tilted)
{
    Workspace &ws = *ctx->ws;
    if (g.w + 1 > 8 * 1024 || (size_t)2 * (g.w + g.h + 2) * sizeof(int) > 64 * 1024) { ctx->set_error("image too large for the tilted integral"); return NVCA_ERR_ARG; }
    if (!tilted) {
        if (ws.ln().tilted.ensure((g.sum_slot * batch + 4 * (size_t)g.spitch) * sizeof(int))) { ctx->set_error("device allocation failed (tilted integral)"); return NVCA_ERR_NOMEM; }
        tilted = ws.ln().tilted.as<int>();
    }
    if (!gray) gray = ws.ln().gray.as<uint8_t>();
    TimedLaunch t(ctx, NVCA_K_INTEGRAL);
    launch_tilted(ctx->cs(), gray, lut, 256, g, tilted, batch);
    return NVCA_OK;
}

// the two list counters a job's kernels append to (so that the caller's k_lut launch can reset them); sizes the lists
int cascade_counters(nvca_ctx *ctx, DetectPlan &dp, const CascadeJob &job, unsigned long long **hits, unsigned long long **deep)
{
    Workspace &ws = *ctx->ws;
    ResultBufs &rb = ws.res[ws.cur_res];
    const int total = std::max(job.total, job.r0 + job.n);
    const size_t hits_stride = (size_t)ctx->hit_cap + 1;
    const unsigned deep_cap = (unsigned)std::min<size_t>((size_t)dp.tasks.size() * 64 * job.n + 64, 1u << 28);
    if (ws.ln().deep.ensure(((size_t)deep_cap + 1) * sizeof(unsigned long long)) ||
        rb.hits.ensure(hits_stride * total * sizeof(unsigned long long)) || rb.h_hits.ensure(hits_stride * total * sizeof(unsigned long long))) {
        ctx->set_error("device allocation failed for the cascade workspace"); return NVCA_ERR_NOMEM;
    }
    *hits = rb.hits.as<unsigned long long>() + hits_stride * job.r0;
    *deep = ws.ln().deep.as<unsigned long long>();
    return NVCA_OK;
}

// A job whose candidates k_group turns into boxes (job.dev_group): its box-table region -- per result slot a table, a job's tables
// followed by the 64-bit raw count -- and its slots' groupRectangles thresholds on the device
int group_prepare(nvca_ctx *ctx, CascadeJob &job, const int *group_thr)
{
    ResultBufs &rb = ctx->ws->res[ctx->ws->cur_res];
    const int batch = job.n, total = std::max(job.total, job.r0 + job.n);
    const size_t grp_stride = 2 + 4 * kGroupOutCap + 2;
    const void *old_gthr = rb.gthr.p;
    if (rb.grp.ensure((size_t)total * grp_stride * sizeof(int)) || rb.h_grp.ensure((size_t)total * grp_stride * sizeof(int)) ||
        rb.gthr.ensure((size_t)total * sizeof(int)) || rb.h_gthr.ensure((size_t)total * sizeof(int))) {
        ctx->set_error("device allocation failed for the grouping workspace"); return NVCA_ERR_NOMEM;
    }
    if (rb.gthr.p != old_gthr) rb.gthr_last.clear();          // a new buffer holds no thresholds yet
    job.d_grp = rb.grp.as<int>() + grp_stride * job.r0; job.h_grp = rb.h_grp.as<int>() + grp_stride * job.r0;
    if (rb.gthr_last.size() < (size_t)total) rb.gthr_last.resize(total, -1);
    if (memcmp(rb.gthr_last.data() + job.r0, group_thr, batch * sizeof(int)) != 0) {
        NVCA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->cs()));             // h_gthr may still feed an earlier copy
        memcpy(rb.h_gthr.as<int>() + job.r0, group_thr, batch * sizeof(int));
        NVCA_HIP_CHECK(ctx, hipMemcpyAsync(rb.gthr.as<int>() + job.r0, rb.h_gthr.as<int>() + job.r0, batch * sizeof(int), hipMemcpyHostToDevice, ctx->cs()));
        std::copy(group_thr, group_thr + batch, rb.gthr_last.begin() + job.r0);
    }
    return NVCA_OK;
}

// behind a job's last kernel: what the host reads once the stream has drained, on its way
int cascade_fetch(nvca_ctx *ctx, CascadeJob &job)
{
    const size_t rec = 2 + 4 * kGroupOutCap;
    if (job.dev_group && ctx->sw.group_zero_copy) {
        // nothing to copy: k_group wrote the host buffer
    } else if (job.dev_group) {      // the device hands back final boxes; the raw list is only fetched for frames it declined
        NVCA_HIP_CHECK(ctx, hipMemcpyAsync(job.h_grp, job.d_grp, (rec * job.n + 2) * sizeof(int), hipMemcpyDeviceToHost, ctx->cs()));
    } else {              // one D2H covers the count and (almost always) every candidate
        job.first = std::min<size_t>(job.cap, 2048);
        NVCA_HIP_CHECK(ctx, hipMemcpyAsync(job.h_hits, job.d_hits, (job.first + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->cs()));
    }
    return NVCA_OK;
}

int cascade_enqueue(nvca_ctx *ctx, DetectPlan &dp, size_t sum_slot, int spitch, CascadeJob &job, const int *group_thr, bool want_group,
                    hipEvent_t early_done)
{
    Workspace &ws = *ctx->ws;
    ResultBufs &rb = ws.res[ws.cur_res];
    const bool grp_zero_copy = ctx->sw.group_zero_copy;
    const int batch = job.n, total = std::max(job.total, job.r0 + job.n);
    int rc;
    const size_t hits_stride = (size_t)ctx->hit_cap + 1;                 // u64 words per result slot
    const unsigned cap = (unsigned)ctx->hit_cap * (unsigned)batch;
    const unsigned deep_cap = (unsigned)std::min<size_t>((size_t)dp.tasks.size() * 64 * batch + 64, 1u << 28);   // every window may survive
    if (ws.ln().failbits.ensure(dp.tasks.size() * sizeof(unsigned long long) * batch + 8) ||
        ws.ln().vnf.ensure(dp.tasks.size() * 64 * sizeof(double) * batch + 8) ||
        ws.ln().deep.ensure(((size_t)deep_cap + 1) * sizeof(unsigned long long)) ||
        rb.hits.ensure(hits_stride * total * sizeof(unsigned long long)) || rb.h_hits.ensure(hits_stride * total * sizeof(unsigned long long))) {
        ctx->set_error("device allocation failed for the cascade workspace"); return NVCA_ERR_NOMEM;
    }
    job.cap = cap;
    job.d_hits = rb.hits.as<unsigned long long>() + hits_stride * job.r0;
    job.h_hits = rb.h_hits.as<unsigned long long>() + hits_stride * job.r0;
    if (!job.counters_zeroed) {
        NVCA_HIP_CHECK(ctx, hipMemsetAsync(job.d_hits, 0, sizeof(unsigned long long), ctx->cs()));
        NVCA_HIP_CHECK(ctx, hipMemsetAsync(ws.ln().deep.p, 0, sizeof(unsigned long long), ctx->cs()));
    }
    const bool skip_cascade = ctx->sw.skip_cascade;
    const bool host_group = ctx->sw.host_group;
    const bool dev_group = group_thr && want_group && dp.device_group_ok && !host_group && !dp.tasks.empty() && !skip_cascade;
    job.dev_group = dev_group;
    if (dev_group && (rc = group_prepare(ctx, job, group_thr))) return rc;
    if (!dp.tasks.empty() && !skip_cascade) {
        CascadeArgs a;
        a.sum = ws.ln().sum.as<int>(); a.sqsum = ws.ln().sqsum.as<unsigned long long>();
        a.sum_slot = sum_slot; a.spitch = spitch;
        a.scales = dp.d_scales.as<ScaleRec>();
        a.stages = dp.d_stages.as<StageRec>(); a.strips = dp.d_strips.as<StripRec>(); a.pos = dp.d_pos.as<int>();
        a.order = dp.d_order.as<int>(); a.blocks_per_frame = dp.blocks_per_frame;
        a.tasks = dp.d_tasks.as<unsigned>(); a.ntasks = (int)dp.tasks.size();
        a.failbits = ws.ln().failbits.as<unsigned long long>(); a.vnf = ws.ln().vnf.as<double>();
        a.nstages = (int)dp.stages.size(); a.pair_policy = ctx->policy == NVCA_SUM_F32PAIR; a.stage_order = ctx->sw.stage_order ? 1 : 0; a.stage_hint = dp.d_stage_hint.as<int>(); a.stage_first = dp.d_stage_first.as<int>(); a.stage_thr = dp.d_stage_thr.as<float>(); a.spec_pairs = ctx->sw.spec_pairs; a.pair_max = std::min(32, std::max(0, ctx->sw.pair_max));
        a.deep_stage = dp.deep_stage; a.deep = ws.ln().deep.as<unsigned long long>(); a.deep_cap = deep_cap;
        a.hits = job.d_hits; a.hit_cap = cap;
        a.tiles = dp.d_tiles.as<TileRec>(); a.tile_order = dp.d_tile_order.as<int>();
        a.tile_blocks_per_frame = dp.tile_blocks_per_frame;
        a.tcoords = dp.d_tcoords.as<unsigned short>(); a.tile_lds = dp.tile_lds;
        a.nscales = (int)dp.scales.size(); a.key_sy = dp.key_sy; a.key_ss = dp.key_ss;
        a.bands = dp.d_bands.as<BandRec>(); a.band_order = dp.d_band_order.as<int>(); a.band_blocks_per_frame = dp.band_blocks_per_frame; a.batch = batch;
        { const int bm = ctx->sw.band_map; a.band_map = (bm > 0 && batch % (8 * bm) == 0) ? bm : 0; }
        a.deeprecs = dp.deeprecs.empty() ? nullptr : dp.d_deeprecs.as<DeepRec>(); a.deep_lds = dp.deep_lds;
        a.tilted = dp.needs_tilted ? ws.ln().tilted.as<int>() : nullptr;
        a.galpha = dp.tabs.empty() ? nullptr : dp.tabs[0]->d_galpha; a.gcls_first = dp.tabs.empty() ? nullptr : dp.tabs[0]->d_gcls_first;
        a.stump_based = dp.generic_stumps ? 1 : 0;
        if (dp.generic) {
            // tree weak classifiers / tilted features: stage-0 pre-pass for every window, then the remaining stages on the
            // visited survivors, window per lane (kernels_cascade_gather.hip, "general cascades")
            if (dp.needs_tilted && !a.tilted) { ctx->set_error("internal: tilted integral missing"); return NVCA_ERR_ARG; }
            { TimedLaunch t(ctx, NVCA_K_STAGE0); launch_gen_stage0(ctx->cs(), a, batch); }
            { TimedLaunch t(ctx, NVCA_K_STRIP); launch_gen_rest(ctx->cs(), a, batch); }
        } else {
#ifdef NVCA_STAMPS
        {   // diagnostic build: the stamps of the last band launch are written to $NVCA_STAMPS_OUT when the context synchronises
            static DevBuf dbgbuf;
            a.dbg = nullptr;
            if (switches().stamps_out && !dbgbuf.ensure(64 * 16 * 64 * 8)) { a.dbg = dbgbuf.as<unsigned long long>(); (void)hipMemsetAsync(a.dbg, 0, 64 * 16 * 64 * 8, ctx->cs()); ctx->stamps = a.dbg; }
        }
#endif
        // one workgroup per band of window rows (k_band) when the batch offers enough bands to fill the workgroup slots (256 CUs x
        // kTilesPerCu: >= 270 bands per slot of a CU); otherwise stage-0 pre-pass + one workgroup per tile.  NVCA_BAND=0/1 forces the choice.
        const int band_env = ctx->sw.band;
        const bool use_band = !dp.bands.empty() && (band_env >= 0 ? band_env != 0 : (long long)dp.bands.size() * batch >= 270 * kTilesPerCu);     // measured crossover at 1080p with two 24-row tiles per CU (540; 68 bands per frame): 4 frames -21 %, 8 frames +5 %, 12 frames +24 %
        auto launch = [&](int (*fn)(hipStream_t, const CascadeArgs &, int, int *)) {     // k_tile / k_band: dynamic LDS above 64 KiB has to be granted
            const int e = fn(ctx->cs(), a, batch, ctx->lds_grant);
            if (e) ctx->set_error(std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString((hipError_t)e));
            return e;
        };
        if (!use_band) { TimedLaunch t(ctx, NVCA_K_STAGE0); launch_stage0(ctx->cs(), a, batch); }
        if (use_band) {
            TimedLaunch t(ctx, NVCA_K_BAND); if (launch(launch_band)) return NVCA_ERR_HIP;
        } else {
            { TimedLaunch t(ctx, NVCA_K_TILE); if (launch(launch_tile)) return NVCA_ERR_HIP; }
            { TimedLaunch t(ctx, NVCA_K_STRIP); launch_strip(ctx->cs(), a, batch); }
        }
        if (early_done) NVCA_HIP_CHECK(ctx, hipEventRecord(early_done, ctx->cs()));
        { TimedLaunch t(ctx, NVCA_K_DEEP); launch_deep(ctx->cs(), a, batch); }
        }
        // the box tables are small (a few KB per frame): the grouping kernel stores them straight into the page-locked host
        // buffer (plain stores, visible to the host once the stream has drained) -- no copy operation behind the last kernel
        if (dev_group) { TimedLaunch t(ctx, NVCA_K_GROUP); launch_group(ctx->cs(), a, rb.gthr.as<int>() + job.r0, grp_zero_copy ? job.h_grp : job.d_grp, kGroupOutCap, batch); }
    }
    NVCA_LAUNCH_CHECK(ctx);
    return cascade_fetch(ctx, job);
}

// after the stream has been synchronised: raw[b] / grouped[b] for the job's n frames
int cascade_collect(nvca_ctx *ctx, DetectPlan &dp, const CascadeJob &job, std::vector<std::vector<nvca_rect>> &raw,
                    std::vector<char> *grouped, std::vector<std::vector<int>> *scale_of, std::vector<std::vector<LevelRec>> *recs)
{
    const bool hostprof = ctx->sw.host_profile;
    const int batch = job.n;
    raw.assign(batch, {});
    if (scale_of) scale_of->assign(batch, {});
    if (grouped) grouped->assign(batch, 0);
    unsigned long long *hh = job.h_hits;
    if (job.dev_group) {
        const int *tail = job.h_grp + (size_t)(2 + 4 * kGroupOutCap) * batch;
        hh[0] = ((unsigned long long)(unsigned)tail[1] << 32) | (unsigned)tail[0];
    }
    const unsigned long long total = hh[0];
    if (hostprof) {
        unsigned long long dc = 0;
        (void)hipMemcpy(&dc, ctx->ws->ln().deep.p, sizeof(dc), hipMemcpyDeviceToHost);
        fprintf(stderr, "[nvca host] deep windows (last job) %llu, raw candidates %llu (job of %d)\n", dc, total, batch);
    }
    if (total > job.cap) {
        // the count is exact (the kernels count every candidate, they only store the first `cap`): remember the capacity per
        // frame that would have held this launch set.  The detectMultiScale entry points re-run the set once with it
        // (detect_job_advance); the batched face path starts its next batch with it.
        const unsigned long long per = (total + (unsigned long long)batch - 1) / (unsigned long long)batch + 64;
        if (per <= (unsigned long long)kMaxHitCap && (long long)per > ctx->hit_cap_wanted) ctx->hit_cap_wanted = (int)per;
        ctx->set_error("raw candidate capacity exceeded (nvca_ctx_set_hit_capacity)");
        return NVCA_ERR_OVERFLOW;
    }
    size_t have = job.first;
    if (job.dev_group) {
        const size_t rec = 2 + 4 * kGroupOutCap;
        bool need_raw = false;
        grouped->assign(batch, 1);
        for (int b = 0; b < batch; b++) {
            const int *r = job.h_grp + rec * b;
            if (r[0] < 0 || r[0] > kGroupOutCap) { (*grouped)[b] = 0; need_raw = need_raw || r[1] > 0; continue; }
            raw[b].resize(r[0]);
            for (int k = 0; k < r[0]; k++) raw[b][k] = nvca_rect{r[2 + 4 * k], r[3 + 4 * k], r[4 + 4 * k], r[5 + 4 * k]};
        }
        if (!need_raw) return NVCA_OK;
        have = 0;
    }
    if (total > have) {
        NVCA_HIP_CHECK(ctx, hipMemcpyAsync(hh + 1 + have, job.d_hits + 1 + have, (total - have) * sizeof(unsigned long long),
                                           hipMemcpyDeviceToHost, ctx->cs()));
        NVCA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->cs()));
    }
    if (recs) {
        // a levels job: candidate i's record lies under the same index; the keys are sorted with their records attached
        recs->assign(batch, {});
        if (!job.d_recs || !job.h_recs || job.dev_group) { ctx->set_error("internal: a levels job without its record array"); return NVCA_ERR_INTERNAL; }
        if (total) {
            NVCA_HIP_CHECK(ctx, hipMemcpyAsync(job.h_recs, job.d_recs, total * sizeof(LevelRec), hipMemcpyDeviceToHost, ctx->cs()));
            NVCA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->cs()));
        }
        std::vector<std::pair<unsigned long long, LevelRec>> kv(total);
        for (unsigned long long i = 0; i < total; i++) kv[i] = {hh[1 + i], job.h_recs[i]};
        std::sort(kv.begin(), kv.end(), [](const std::pair<unsigned long long, LevelRec> &x, const std::pair<unsigned long long, LevelRec> &y) { return x.first < y.first; });
        for (unsigned long long i = 0; i < total; i++) { hh[1 + i] = kv[i].first; job.h_recs[i] = kv[i].second; }
    } else
    std::sort(hh + 1, hh + 1 + total);
    for (unsigned long long i = 0; i < total; i++) {
        // a candidate word comes from the device: it indexes host tables only after it has been checked against them (a kernel that
        // did not run, or ran on stale tables, must end as an error code, never as a wild host access)
        const unsigned long long slot_u = hh[1 + i] >> 32;
        if (slot_u >= (unsigned long long)batch || !dp.hit_valid((unsigned)hh[1 + i])) {
            ctx->set_error("internal: candidate list holds an entry outside the scan (device result rejected)");
            return NVCA_ERR_INTERNAL;
        }
        const int slot = (int)slot_u;
        if (!job.dev_group || !(*grouped)[slot]) {
            raw[slot].push_back(dp.hit_rect((unsigned)hh[1 + i]));
            if (scale_of) (*scale_of)[slot].push_back((int)((unsigned)hh[1 + i] >> dp.key_ss));
            if (recs) (*recs)[slot].push_back(job.h_recs[i]);
        }
    }
    return NVCA_OK;
}

void group_all(std::vector<std::vector<nvca_rect>> &raw, int min_neighbors)
{
    const double GROUP_EPS = 0.2;
    for (auto &r : raw)
        if (min_neighbors != 0) group_rectangles(r, std::max(min_neighbors, 1), GROUP_EPS);
}

GeomPlan *find_plan(nvca_ctx *ctx, const std::string &key)
{
    auto it = ctx->plans.find(key);
    if (it == ctx->plans.end()) return nullptr;
    it->second->last_use = ++ctx->next_uid;
    return it->second.get();
}

// Plans are cached per (cascade, geometry).  ROI-driven callers (the part detectors) ask for ever new geometries, so the
// cache is bounded: beyond kMaxPlans the least recently used plan goes (its device tables are idle: the stream is drained).
static constexpr size_t kMaxPlans = 1024;
GeomPlan *store_plan(nvca_ctx *ctx, const std::string &key, std::unique_ptr<GeomPlan> gp)
{
    if (ctx->plans.size() >= kMaxPlans) {
        // kernels that read a victim's tables may still be queued on any lane: drain the device once, then drop the least
        // recently used quarter in one go (ROI-driven callers would otherwise pay the drain for every new geometry)
        (void)hipDeviceSynchronize();
        std::vector<std::pair<uint64_t, std::string>> order;
        for (auto &kv : ctx->plans) if (kv.second->inflight == 0) order.emplace_back(kv.second->last_use, kv.first);
        std::sort(order.begin(), order.end());
        for (size_t i = 0; i < order.size() && i < kMaxPlans / 4; i++) ctx->plans.erase(order[i].second);
    }
    gp->last_use = ++ctx->next_uid;
    GeomPlan *p = gp.get();
    ctx->plans[key] = std::move(gp);
    return p;
}

// the pre-processing half of a face plan: working-image geometry, resize table, row copy of host frames
static int face_plan_pre(nvca_ctx *ctx, GeomPlan &gp, int W, int H, int stride, int cn, int cols, int rows)
{
    make_geom(gp.g, W, H, stride, cn, cols, rows);
    build_resize_tab(W, H, cols, rows, gp.tab);
    gp.rowcopy = make_rowcopy(gp.tab);
    return upload_tab(ctx, gp);
}
static void yuv_key(char *key, size_t room, const nvca_pixel_layout *yuv)
{
    if (yuv) snprintf(key, room, "|Y%d|%zu|%zu|%zu|%d|%d|%d", yuv->format, yuv->offset[0], yuv->offset[1], yuv->offset[2],
                      yuv->stride[0], yuv->stride[1], yuv->stride[2]);
}

// plan for "BGR frame -> working image -> scale-cascade scan"
// (yuv: the frames are 4:2:0 buffers of this layout; stride is their luma stride, cn 1)
int get_face_plan(nvca_ctx *ctx, const nvca_cascade *casc, int W, int H, int stride, int cn, int cols, int rows,
                  double sf, int minw, int minh, int maxw, int maxh, GeomPlan **out, const nvca_pixel_layout *yuv)
{
    // multi-scale-factor 0 (scaleFactor 1.0): OpenCV's assertion fires in detectMultiScale, the reference logs it and passes the frame on
    // untouched (FACE/kmsfacedetect.cpp:540-542 installs the property with range 0 .. 51); every other value is a ladder that ends
    if (!(sf > 1.0)) { ctx->set_error("scaleFactor must be greater than 1 (multi-scale-factor 0)"); return NVCA_ERR_ARG; }
    char key[384];
    int kl = snprintf(key, sizeof(key), "F|%llu|%d|%d|%d|%d|%d|%d|%.17g|%d|%d|%d|%d", (unsigned long long)casc->c.uid, W, H, stride,
                      cn, cols, rows, sf, minw, minh, maxw, maxh);
    yuv_key(key + kl, sizeof(key) - kl, yuv);
    if (GeomPlan *gp = find_plan(ctx, key)) { *out = gp; return NVCA_OK; }
    std::unique_ptr<GeomPlan> gp(new GeomPlan());
    int rc = face_plan_pre(ctx, *gp, W, H, stride, cn, cols, rows);
    if (rc) return rc;
    std::string err;
    rc = gp->det.build_scale_cascade(ctx, casc->c, cols, rows, gp->g.spitch, sf, minw, minh, maxw, maxh, err);
    if (rc) { ctx->set_error(err); return rc; }
    rc = gp->det.upload(ctx);
    if (rc) return rc;
    gp->has_det = true;
    *out = store_plan(ctx, key, std::move(gp));
    return NVCA_OK;
}

// that plan's pre-processing half alone, whatever scans the working image (a face stream on a new-format LBP cascade: its scan is
// the cached "LBP|" plan, lbp_job.cpp)
int get_face_pre_plan(nvca_ctx *ctx, int W, int H, int stride, int cn, int cols, int rows, GeomPlan **out, const nvca_pixel_layout *yuv)
{
    char key[256];
    int kl = snprintf(key, sizeof(key), "FP|%d|%d|%d|%d|%d|%d", W, H, stride, cn, cols, rows);
    yuv_key(key + kl, sizeof(key) - kl, yuv);
    if (GeomPlan *gp = find_plan(ctx, key)) { *out = gp; return NVCA_OK; }
    std::unique_ptr<GeomPlan> gp(new GeomPlan());
    int rc = face_plan_pre(ctx, *gp, W, H, stride, cn, cols, rows);
    if (rc) return rc;
    *out = store_plan(ctx, key, std::move(gp));
    return NVCA_OK;
}

// resize coefficient tables for (source size -> destination size), cached with the other plans
int get_resize_plan(nvca_ctx *ctx, int sw, int sh, int dw, int dh, GeomPlan **out)
{
    char key[96];
    snprintf(key, sizeof(key), "RZ|%d|%d|%d|%d", sw, sh, dw, dh);
    if (GeomPlan *gp = find_plan(ctx, key)) { *out = gp; return NVCA_OK; }
    std::unique_ptr<GeomPlan> gp(new GeomPlan());
    build_resize_tab(sw, sh, dw, dh, gp->tab);
    int rc = upload_tab(ctx, *gp);
    if (rc) return rc;
    *out = store_plan(ctx, key, std::move(gp));
    return NVCA_OK;
}

} // namespace nvca
