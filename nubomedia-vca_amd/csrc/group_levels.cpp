// group_levels.cpp -- cv::groupRectangles with reject levels and level weights (OpenCV 2.4 cascadedetect.cpp, from memory; SURVEY.md
// A.17).  The partition and the averaging are group_rectangles' own (host_logic.cpp, group_classes); what is stated here is what the
// weighted form does differently.
#include "group_levels.h"
#include "host_logic.h"
#include <algorithm>
#include <cfloat>
#include <cmath>

namespace nvca {

static inline int cv_round(double v) { return (int)lrint(v); }

bool group_rectangles_levels(std::vector<nvca_rect> &rects, std::vector<int> &levels, std::vector<double> &weights, int groupThreshold, double eps)
{
    if (levels.size() != rects.size() || weights.size() != rects.size()) return false;
    if (groupThreshold <= 0 || rects.empty()) return true;
    std::vector<int> labels, rw;
    std::vector<nvca_rect> rr;
    const int nclasses = group_classes(rects, eps, labels, rr, rw);
    std::vector<int> max_level(nclasses, 0);
    std::vector<double> max_weight(nclasses, DBL_MIN);
    for (size_t i = 0; i < rects.size(); i++) {
        const int c = labels[i];
        if (levels[i] > max_level[c]) { max_level[c] = levels[i]; max_weight[c] = weights[i]; }
        else if (levels[i] == max_level[c] && weights[i] > max_weight[c]) max_weight[c] = weights[i];
    }
    rects.clear(); levels.clear(); weights.clear();
    for (int i = 0; i < nclasses; i++) {
        const nvca_rect r1 = rr[i];
        const int n1 = max_level[i];          // (the quirk: a class's own weight is its level, its partner's below the member count)
        if (n1 <= groupThreshold) continue;
        int j;
        for (j = 0; j < nclasses; j++) {
            const int n2 = rw[j];
            if (j == i || n2 <= groupThreshold) continue;
            const nvca_rect r2 = rr[j];
            const int dx = cv_round(r2.w * eps), dy = cv_round(r2.h * eps);
            if (r1.x >= r2.x - dx && r1.y >= r2.y - dy && r1.x + r1.w <= r2.x + r2.w + dx &&
                r1.y + r1.h <= r2.y + r2.h + dy && (n2 > std::max(3, n1) || n1 < 3))
                break;
        }
        if (j == nclasses) { rects.push_back(r1); levels.push_back(n1); weights.push_back(max_weight[i]); }
    }
    return true;
}

} // namespace nvca
