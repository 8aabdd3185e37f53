// hnew_tables.cpp -- the device tables of a new-format HAAR scan (hnew_tables.h): pure host code.
#include "hnew_tables.h"
#include <cstring>

namespace nvca {

// the corners of rect (x, y, w, h) in the order p0 - p1 - p2 + p3 of HaarEvaluator's CALC_SUM
static void rect_corners(int *off, int x, int y, int w, int h, int pitch)
{
    off[0] = y * pitch + x; off[1] = y * pitch + x + w; off[2] = (y + h) * pitch + x; off[3] = (y + h) * pitch + x + w;
}

int build_hnew_tables(const HnewCascade &c, const std::vector<PyrLevel> &lv, int P, HnewTables &out, std::string &err)
{
    out = HnewTables();
    if (int rc = build_scan_tables(c.ow, c.oh, c.stages, lv, P, out.scan, err)) return rc;
    out.gweak.resize(c.weak.size()); out.tweak.resize(c.weak.size());
    for (size_t i = 0; i < c.weak.size(); i++) {
        const HnewWeak &w = c.weak[i]; const HnewFeature &f = c.features[(size_t)w.feature];
        for (std::vector<HnewWeakDev> *tab : {&out.gweak, &out.tweak}) {
            HnewWeakDev &d = (*tab)[i]; memset(&d, 0, sizeof(d));
            const int pitch = tab == &out.gweak ? P : out.scan.TP;
            for (int r = 0; r < 3; r++) {
                if (r < f.nrect) rect_corners(d.off + 4 * r, f.rect[r][0], f.rect[r][1], f.rect[r][2], f.rect[r][3], pitch);
                d.w[r] = r < f.nrect ? f.weight[r] : 0.f;
            }
            d.thr = w.threshold; d.leaf[0] = w.leaf[0]; d.leaf[1] = w.leaf[1];
        }
    }
    // HaarEvaluator::setImage: normrect = Rect(1, 1, origWinSize.width - 2, origWinSize.height - 2)
    rect_corners(out.nr, 1, 1, c.ow - 2, c.oh - 2, P);
    rect_corners(out.nrt, 1, 1, c.ow - 2, c.oh - 2, out.scan.TP);
    out.area = (double)(c.ow - 2) * (double)(c.oh - 2);
    return NVCA_OK;
}

} // namespace nvca
