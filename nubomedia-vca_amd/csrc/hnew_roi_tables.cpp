// hnew_roi_tables.cpp -- the cascade table of the small-image evaluator of new-format HAAR cascades (hnew_roi_tables.h): pure host code.
#include "hnew_roi_tables.h"
#include <cstring>

namespace nvca {

void build_hnew_roi_table(const HnewCascade &c, std::vector<unsigned char> &blob)
{
    const size_t o_weak = roi_hnew_weak_off((int)c.stages.size());
    blob.assign(o_weak + c.weak.size() * sizeof(RoiHnewWeak) + 64, 0);      // (a wide scalar load behind the last record stays inside)
    LbpStageDev *st = (LbpStageDev *)blob.data();
    for (size_t i = 0; i < c.stages.size(); i++) st[i] = LbpStageDev{c.stages[i].first, c.stages[i].count, c.stages[i].threshold, 0};
    RoiHnewWeak *wk = (RoiHnewWeak *)(blob.data() + o_weak);
    for (size_t i = 0; i < c.weak.size(); i++) {
        const HnewWeak &w = c.weak[i]; const HnewFeature &f = c.features[(size_t)w.feature];
        RoiHnewWeak &d = wk[i];
        for (int r = 0; r < 3; r++) {          // a missing rect: four zeros, weight 0 (hnew_tables.cpp)
            if (r < f.nrect) memcpy(d.rect[r], f.rect[r], sizeof(d.rect[r]));
            d.w[r] = r < f.nrect ? f.weight[r] : 0.f;
        }
        d.thr = w.threshold; d.leaf[0] = w.leaf[0]; d.leaf[1] = w.leaf[1];
    }
}

} // namespace nvca
