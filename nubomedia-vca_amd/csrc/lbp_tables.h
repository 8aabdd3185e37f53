// lbp_tables.h -- the device tables of a new-format LBP scan (kernels_cascade_lbp.hip), built from the cascade and the pyramid's
// levels as pure host code (no HIP, no context): lbp_job.cpp uploads them as they come out of here.
#pragma once
#include "cascade_model.h"
#include "device_records.h"
#include "pyr_levels.h"
#include <string>
#include <vector>

namespace nvca {

struct LbpTables {
    std::vector<LbpLevelDev> levels; std::vector<LbpTile> tiles; std::vector<LbpStageDev> stages;
    // device grouping (k_group, kernels_group.hip): a ScaleRec per level -- window size, grid extents, where its columns' and rows' OUTPUT
    // coordinates lie in gpos -- and those coordinates, cvRound(origin * factor), rounded here
    std::vector<ScaleRec> gscales; std::vector<int> gpos;
    std::vector<LbpWeakDev> gweak, tweak;     // corner offsets at the planes' pitch P / at the stage-0 tile's pitch TP
    int TP = 0, nrows = 0;                    // scan rows of all levels
    int key_sy = 0, key_ss = 0;               // candidate key = level << key_ss | gy << key_sy | gx
    int tile_stages = 0;                      // stages the tile kernel evaluates
    int lds = 0;                              // bytes of the stage-0 tile (0: the window is too large, stage 0 gathers from the plane)
    size_t bit_words = 0, positions = 0;      // stage-0 pass bits (u32 words) and grid positions of all levels
};
// the part every new-format scan shares, whatever its evaluator (gweak / tweak stay empty): levels, tiles, stages, key layout, k_group's
// records, the stage-0 tile's pitch and LDS bytes -- from the window, the stages' shape and the levels alone
int build_scan_tables(int ow, int oh, const std::vector<LbpStage> &stages, const std::vector<PyrLevel> &lv, int P, LbpTables &out, std::string &err);
// the tables of cascade `c` on levels `lv` whose planes have pitch P; NVCA_ERR_ARG (with err) when the scan outgrows the candidate key
int build_lbp_tables(const LbpCascade &c, const std::vector<PyrLevel> &lv, int P, LbpTables &out, std::string &err);

} // namespace nvca
