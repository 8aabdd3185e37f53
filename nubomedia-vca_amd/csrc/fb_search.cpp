// fb_search.cpp -- scan grids and the CV_HAAR_FIND_BIGGEST_OBJECT search of cvHaarDetectObjectsForROC (NOSE/kmsnosedetect.cpp:870-873,
// MOUTH/kmsmouthdetect.cpp:870-873, EAR/kmseardetect.cpp:712-715) as pure host code: see fb_search.h.
#include "fb_search.h"
#include "host_logic.h"
#include "host_math.h"
#include <algorithm>

namespace nvca {

bool clip_grid(int cols, int rows, double ystep, int winw, int winh, ScanGrid &g)
{
    if (!(g.endX > g.startX && g.endY > g.startY)) return false;
    while (g.endX > g.startX && cv_round((g.endX - 1) * ystep) + winw >= cols + 1) g.endX--;
    while (g.endY > g.startY && cv_round((g.endY - 1) * ystep) + winh >= rows + 1) g.endY--;
    if (!(g.endX > g.startX && g.endY > g.startY)) return false;
    return cv_round(g.startX * ystep) >= 0 && cv_round(g.startY * ystep) >= 0;
}

bool full_grid(int cols, int rows, double ystep, int winw, int winh, ScanGrid &g)
{
    g = ScanGrid{0, cv_round((cols - winw) / ystep), 0, cv_round((rows - winh) / ystep)};
    return clip_grid(cols, rows, ystep, winw, winh, g);
}

bool roi_grid(const ScanGrid &g, double ystep, RoiStep &st)
{
    if (g.endX > 8191 || g.endY > 8191) return false;
    st.startX = g.startX; st.endX = g.endX; st.startY = g.startY; st.endY = g.endY; st.ystep = ystep; st.adaptive = 1;
    return true;
}

void FbSearch::start(int ow, int oh, int cols_, int rows_, double sf, int minw_, int minh_, int maxw_, int maxh_)
{
    cols = cols_; rows = rows_; minw = minw_; minh = minh_; maxw = maxw_; maxh = maxh_;
    ladder.clear();
    int n_factors = 0; double factor;
    for (n_factors = 0, factor = 1; factor * ow < cols - 10 && factor * oh < rows - 10; n_factors++, factor *= sf)
        ;
    const double inv = 1. / sf; factor *= inv;
    for (; n_factors-- > 0; factor *= inv) ladder.push_back(FbStep{factor, std::max(2., factor), cv_round(ow * factor), cv_round(oh * factor)});
    hits.assign(ladder.size(), {}); ladder_of.clear(); grids.clear();
    all.clear(); scanROI = nvca_rect{0, 0, 0, 0}; narrowed_done = false; fb_i = 0; cur_minw = minw; cur_minh = minh;
    dense_hits.clear(); rej_bits.clear(); rej_wpr.clear(); rej_rows.clear();
}

void FbSearch::first_set()
{
    ladder_of.clear(); grids.clear();
    for (size_t i = 0; i < ladder.size(); i++) {
        const FbStep &st = ladder[i];
        if (st.winw < minw || st.winh < minh) break;
        if (st.winw > maxw || st.winh > maxh) continue;
        ScanGrid g;
        if (full_grid(cols, rows, st.ystep, st.winw, st.winh, g)) { ladder_of.push_back((int)i); grids.push_back(g); }
    }
}

bool FbSearch::narrowed_grid(size_t step, ScanGrid &g) const
{
    const FbStep &st = ladder[step];
    g = ScanGrid{cv_round(scanROI.x / st.ystep), cv_round((scanROI.x + scanROI.w - st.winw) / st.ystep),
                 cv_round(scanROI.y / st.ystep), cv_round((scanROI.y + scanROI.h - st.winh) / st.ystep)};
    return clip_grid(cols, rows, st.ystep, st.winw, st.winh, g);
}

bool FbSearch::take(const std::vector<nvca_rect> &raw, const std::vector<int> &sc, bool by_step)
{
    for (size_t k = 0; k < raw.size(); k++) {
        size_t li = (size_t)sc[k];
        if (!by_step) li = li < ladder_of.size() ? (size_t)ladder_of[li] : (size_t)-1;
        if (li >= hits.size()) return false;
        hits[li].push_back(raw[k]);
    }
    return true;
}

void FbSearch::dense_begin()
{
    rej_bits.assign(ladder.size(), nullptr); rej_wpr.assign(ladder.size(), 0); rej_rows.assign(ladder.size(), 0); dense_hits.assign(ladder.size(), {});
}

int FbSearch::dense_candidate(size_t li, int ix, int iy)
{
    if (li >= rej_bits.size() || rej_wpr[li] <= 0 || iy >= rej_rows[li] || ix >= rej_wpr[li] * 64) return -1;
    dense_hits[li].push_back((unsigned)(iy << 13 | ix));
    return fb_visited(rej_bits[li] + (size_t)iy * rej_wpr[li], 0, ix) ? 1 : 0;
}

bool FbSearch::replay(int min_neighbors, bool rough, std::vector<nvca_rect> &out)
{
    for (size_t i = fb_i; i < ladder.size(); i++) {
        const FbStep &st = ladder[i];
        if (st.winw < cur_minw || st.winh < cur_minh) break;
        if (st.winw > maxw || st.winh > maxh) continue;
        if (scanROI.w * scanROI.h > 0 && !narrowed_done) {
            // this step and all later ones on their narrowed grids (nothing changes the scan any more)
            narrowed_done = true; ladder_of.clear(); grids.clear();
            for (size_t k = i; k < ladder.size(); k++) {
                const FbStep &sk = ladder[k];
                hits[k].clear();
                if (sk.winw < cur_minw || sk.winh < cur_minh) break;
                if (sk.winw > maxw || sk.winh > maxh) continue;
                ScanGrid g;
                if (!narrowed_grid(k, g)) continue;
                if (k >= rej_wpr.size() || rej_wpr[k] <= 0) { ladder_of.push_back((int)k); grids.push_back(g); continue; }
                // dense first set: the narrowed walk of this step is replayed here -- its windows are grid points of the full grid, the
                // set reported every one of them that passes the cascade, and which of them the walk from column startX visits follows
                // from the stage-0 reject bits (no second set).  A step the first set did not hold (below the call's minSize: the
                // narrowed search lowers it to 0.4 / 0.6 of the object found) is still asked for, above.
                const int wpr = rej_wpr[k];
                for (unsigned key : dense_hits[k]) {            // ascending (iy, ix): the serial order
                    const int iy = (int)(key >> 13), ix = (int)(key & 8191);
                    if (iy < g.startY || iy >= g.endY || ix < g.startX || ix >= g.endX) continue;
                    if (iy >= rej_rows[k] || !fb_visited(rej_bits[k] + (size_t)iy * wpr, g.startX, ix)) continue;
                    hits[k].push_back(nvca_rect{cv_round(ix * sk.ystep), cv_round(iy * sk.ystep), sk.winw, sk.winh});
                }
            }
            if (!ladder_of.empty()) { fb_i = i; return false; }          // come back with the narrowed scans
        }
        all.insert(all.end(), hits[i].begin(), hits[i].end());
        if (!all.empty() && scanROI.w * scanROI.h == 0) {
            std::vector<nvca_rect> tmp(all);
            group_rectangles(tmp, std::max(min_neighbors, 1), 0.2);
            if (!tmp.empty()) {
                nvca_rect maxRect{0, 0, 0, 0};
                for (const nvca_rect &r : tmp) if (r.w * r.h > maxRect.w * maxRect.h) maxRect = r;
                all.push_back(maxRect);
                scanROI = maxRect;
                const int dx = cv_round(maxRect.w * 0.2), dy = cv_round(maxRect.h * 0.2);
                scanROI.x = std::max(scanROI.x - dx, 0); scanROI.y = std::max(scanROI.y - dy, 0);
                scanROI.w = std::min(scanROI.w + dx * 2, cols - 1 - scanROI.x);
                scanROI.h = std::min(scanROI.h + dy * 2, rows - 1 - scanROI.y);
                const double minScale = rough ? 0.6 : 0.4;
                cur_minw = cv_round(maxRect.w * minScale); cur_minh = cv_round(maxRect.h * minScale);
            }
        }
    }
    group_rectangles(all, std::max(min_neighbors, 1), 0.2);
    out.clear();
    if (!all.empty()) {
        nvca_rect best{0, 0, 0, 0};
        for (const nvca_rect &r : all) if (r.w * r.h > best.w * best.h) best = r;
        out.push_back(best);
    }
    return true;
}

} // namespace nvca
