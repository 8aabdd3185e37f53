// lbp_roi_tables.h -- what the small-image LBP evaluator (kernels_roi_lbp.hip) is launched with, built as pure host code (no HIP, no
// context): whether an image fits the workgroup's LDS, a job's step records with their resize tables, the bands of whole rows a step
// goes out as, and a cascade's device table.  roi_batch.cpp uploads them as they come out of here.
#pragma once
#include "cascade_model.h"
#include "device_records.h"
#include <vector>

namespace nvca {

// The LDS bound of a small LBP job.  Its working set is the sum plane of its largest level -- the image itself: (cols + 1) x (rows + 1)
// words -- the largest RESIZED level as bytes (below cols x rows), the two queues, the counters and the short-queue votes
// (roi_lbp_lds_bytes): 4 (cols + 1)(rows + 1) + cols rows + 24 592 bytes of the CU's 160 KiB, 64 bytes kept spare.  Five bytes a pixel
// against k_roi's eight and a half (two planes of (cols + 1)(rows + 2) words and a level image): the 160 x 90 face-pass image takes
// 73 008 of these bytes (each part rounded up to 16), 160 x 120 (outside kRoiMaxWords) 97 136.
static constexpr int kRoiLbpMaxBytes = 160 * 1024 - (2 * kRoiMaxWin * 2 + 16 + kRoiLbpVoteWords * 4) - 64;      // 139 184
static_assert(kRoiLbpMaxBytes == 160 * 1024 - roi_lbp_fixed_bytes() - 64, "the bound follows the kernel's carve-up");
inline long long lbp_roi_image_bytes(int cols, int rows)
{
    return 4 * ((((long long)cols + 1) * (rows + 1) + 3) & ~3ll) + (((long long)cols * rows + 15) & ~15ll);
}
inline bool lbp_roi_fits_lds(int cols, int rows) { return cols >= 1 && rows >= 1 && lbp_roi_image_bytes(cols, rows) <= kRoiLbpMaxBytes; }

struct LbpRoiLevel { double factor; int winw, winh; };
struct LbpRoiSteps {
    std::vector<RoiStep> steps;             // one per level with a grid, in level order (before roi_split_bands)
    std::vector<LbpRoiLevel> info;          // [step]: what maps a candidate of the step to its rectangle
    std::vector<unsigned char> tabs;        // the levels' cv::resize tables; the steps' offsets count from the launch blob's base
    int plane_words = 0, lev_bytes = 0;     // the largest level's sum plane (words) and the largest resized level (bytes)
    bool fits = true;                       // false: more levels than the candidate key holds
};
// the levels of detectMultiScale(cols x rows, sf, min, max) on cascade c, each with its grid and resize tables; tab0: bytes the
// launch's table blob holds already
void build_lbp_roi_steps(const LbpCascade &c, int cols, int rows, double sf, int minw, int minh, int maxw, int maxh, size_t tab0, LbpRoiSteps &out);
// the same on the window size alone, which is all of a cascade that the levels read: what the new-format HAAR route (hnew_roi_tables.h) calls
void build_lbp_roi_steps(int ow, int oh, int cols, int rows, double sf, int minw, int minh, int maxw, int maxh, size_t tab0, LbpRoiSteps &out);
// A step's rows are independent of one another: a step with more grid positions than the queues hold goes out as several records,
// a band of whole rows each, all with the step's number in the key.  false: a single grid row is longer than the queues.
bool roi_split_bands(std::vector<RoiStep> &steps);
// the cascade as k_roi_lbp reads it: its LbpStageDev records, then (at roi_lbp_weak_off) a RoiLbpWeak per weak classifier
void build_lbp_roi_table(const LbpCascade &c, std::vector<unsigned char> &blob);

} // namespace nvca
