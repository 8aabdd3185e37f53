// hnew_tables.h -- the device tables of a new-format HAAR scan (kernels_cascade_hnew.hip), built as pure host code beside the LBP
// scan's (lbp_tables.h): what depends on the levels alone IS the LBP scan's (build_scan_tables); this unit adds the weak records
// and the normalisation rectangle.
#pragma once
#include "lbp_tables.h"

namespace nvca {

struct HnewTables {
    LbpTables scan;                             // levels, tiles, stages, key layout, k_group's records (gweak / tweak empty)
    std::vector<HnewWeakDev> gweak, tweak;      // corner offsets at the planes' pitch P / at the stage-0 tile's pitch scan.TP
    int nr[4] = {0, 0, 0, 0}, nrt[4] = {0, 0, 0, 0};      // normrect's corners at the two pitches
    double area = 0.;
};
int build_hnew_tables(const HnewCascade &c, const std::vector<PyrLevel> &lv, int P, HnewTables &out, std::string &err);

} // namespace nvca
