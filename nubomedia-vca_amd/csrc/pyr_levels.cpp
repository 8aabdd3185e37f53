// pyr_levels.cpp -- pyramid levels and their layout (pyr_levels.h): pure host code.
#include "pyr_levels.h"
#include "host_math.h"

namespace nvca {

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
PyrLayout pyr_layout(const std::vector<SiLevel> &levels, int cols)
{
    PyrLayout lay;
    lay.P = (int)round_up(cols + 1, 8);
    for (const SiLevel &sl : levels) {
        PyrLevel L; L.f = sl.factor; L.szw = sl.szw; L.szh = sl.szh; L.winw = sl.winw; L.winh = sl.winh;
        L.gpitch = (int)round_up(L.szw, 64); L.gray_off = lay.gray_total; L.plane_off = (int)lay.plane_total;
        lay.gray_total += round_up((size_t)L.gpitch * L.szh, 256);
        lay.plane_total += round_up((size_t)lay.P * (L.szh + 1), 64);
        lay.lv.push_back(L);
    }
    return lay;
}

} // namespace nvca
