// lbp_roi_tables.cpp -- step records, bands and the cascade table of the small-image LBP evaluator (lbp_roi_tables.h): pure host code.
#include "lbp_roi_tables.h"
#include "pixel_rules.h"
#include "pyr_levels.h"
#include <algorithm>
#include <cstring>

namespace nvca {

void build_lbp_roi_steps(const LbpCascade &c, int cols, int rows, double sf, int minw, int minh, int maxw, int maxh, size_t tab0, LbpRoiSteps &out)
{
    build_lbp_roi_steps(c.ow, c.oh, cols, rows, sf, minw, minh, maxw, maxh, tab0, out);
}

void build_lbp_roi_steps(int ow, int oh, int cols, int rows, double sf, int minw, int minh, int maxw, int maxh, size_t tab0, LbpRoiSteps &out)
{
    out = LbpRoiSteps();
    // (one level more than the key holds is enough to know that the job does not fit)
    const std::vector<SiLevel> levels = lbp_levels(ow, oh, cols, rows, sf, minw, minh, maxw, maxh, 64);
    if (levels.size() > 63) { out.fits = false; return; }
    for (const SiLevel &sl : levels) {
        RoiStep st; memset(&st, 0, sizeof(st));
        st.szw = sl.szw; st.szh = sl.szh; st.step = level_step(sl.factor);
        st.startX = 0; st.endX = sl.szw - ow; st.startY = 0; st.endY = sl.szh - oh;       // origins below size - window (level_positions)
        if (st.endX <= 0 || st.endY <= 0) continue;
        ResizeTab tab; build_resize_tab(cols, rows, sl.szw, sl.szh, tab);
        st.mode = tab.mode; st.xmax = tab.xmax;
        auto put = [&](const void *p, size_t n) {
            const size_t at = (tab0 + out.tabs.size() + 15) & ~(size_t)15;
            out.tabs.resize(at - tab0 + n);
            if (n) memcpy(out.tabs.data() + at - tab0, p, n);
            return (int)at;
        };
        if (tab.mode == 1) {          // (the identity and the 2 x 2 area rule read no table)
            st.xofs_off = put(tab.xofs.data(), tab.xofs.size() * 4); st.yofs_off = put(tab.yofs.data(), tab.yofs.size() * 4);
            st.ialpha_off = put(tab.ialpha.data(), tab.ialpha.size() * 2); st.ibeta_off = put(tab.ibeta.data(), tab.ibeta.size() * 2);
        }
        out.steps.push_back(st); out.info.push_back(LbpRoiLevel{sl.factor, sl.winw, sl.winh});
        out.plane_words = std::max(out.plane_words, (sl.szw + 1) * (sl.szh + 1));
        if (tab.mode != 0) out.lev_bytes = std::max(out.lev_bytes, sl.szw * sl.szh);
    }
}

bool roi_split_bands(std::vector<RoiStep> &steps)
{
    bool fits = true;
    std::vector<RoiStep> bands;
    for (size_t li = 0; li < steps.size(); li++) {
        RoiStep st = steps[li];
        const int nx = (st.endX - st.startX + st.step - 1) / st.step, ny = (st.endY - st.startY + st.step - 1) / st.step;
        if (nx > kRoiMaxWin) fits = false;                       // (a grid row longer than the queues: not with images this small)
        st.key_step = (int)li;
        st.key_x0 = st.startX; st.key_dx = st.step; st.key_dy = st.step;
        const int rows_per = nx > 0 && nx < kRoiMaxWin ? kRoiMaxWin / nx : 1;
        for (int gy0 = 0; gy0 < std::max(ny, 1); gy0 += rows_per) {
            RoiStep b = st;
            b.startY = st.startY + gy0 * st.step;
            b.endY = std::min(st.endY, st.startY + (gy0 + rows_per) * st.step);
            b.key_y0 = b.startY;
            bands.push_back(b);
        }
    }
    steps.swap(bands);
    return fits;
}

void build_lbp_roi_table(const LbpCascade &c, std::vector<unsigned char> &blob)
{
    const size_t o_weak = roi_lbp_weak_off((int)c.stages.size());
    blob.assign(o_weak + c.weak.size() * sizeof(RoiLbpWeak) + 64, 0);       // (a wide scalar load behind the last record stays inside)
    LbpStageDev *st = (LbpStageDev *)blob.data();
    for (size_t i = 0; i < c.stages.size(); i++) st[i] = LbpStageDev{c.stages[i].first, c.stages[i].count, c.stages[i].threshold, 0};
    RoiLbpWeak *wk = (RoiLbpWeak *)(blob.data() + o_weak);
    for (size_t i = 0; i < c.weak.size(); i++) {
        const LbpWeak &w = c.weak[i]; const LbpFeature &f = c.features[(size_t)w.feature];
        RoiLbpWeak &d = wk[i];
        d.x = f.x; d.y = f.y; d.w = f.w; d.h = f.h;
        memcpy(d.subset, w.subset, sizeof(d.subset)); d.leaf[0] = w.leaf[0]; d.leaf[1] = w.leaf[1];
    }
}

} // namespace nvca
