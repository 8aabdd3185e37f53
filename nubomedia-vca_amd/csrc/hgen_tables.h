// hgen_tables.h -- the device tables of a general new-format HAAR scan (kernels_cascade_hgen.hip), built as pure host
// code beside hnew_tables.h's: the scan's own tables are the LBP scan's (build_scan_tables), the normalisation rectangle is the stump
// evaluator's; this unit adds the node records and the weak classifiers' places in them.
#pragma once
#include "hnew_tables.h"

namespace nvca {

struct HgenTables {
    HnewTables base;                        // scan, nr / nrt, area (gweak / tweak empty)
    std::vector<HgenNodeDev> nodes;         // every node of the cascade in file order
    std::vector<HgenWeakDev> weak;          // per weak classifier: its first node and its node count
};
int build_hgen_tables(const HnewCascade &c, const std::vector<PyrLevel> &lv, int P, HgenTables &out, std::string &err);

} // namespace nvca
