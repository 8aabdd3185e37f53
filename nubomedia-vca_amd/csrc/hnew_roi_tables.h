// hnew_roi_tables.h -- what the small-image evaluator of new-format HAAR cascades (kernels_roi_hnew.hip) is launched with, built as
// pure host code (no HIP, no context): whether an image fits the workgroup's LDS, and a cascade's device table.  The step records,
// their resize tables and the bands are the LBP route's (lbp_roi_tables.h: build_lbp_roi_steps on the window size, roi_split_bands).
#pragma once
#include "lbp_roi_tables.h"

namespace nvca {

// The LDS bound of a small new-format HAAR job.  Its working set is the sum plane and the squared plane of its largest level -- the
// image itself: (cols + 1) x (rows + 1) words each -- and the fixed part of roi_hnew_lds_bytes (queues, counters, votes, vnf; the
// resized level image lies over the last two): 8 align4((cols + 1)(rows + 1)) + 40 976 bytes of the CU's 160 KiB, 64 bytes kept spare.
// The part detectors' 160 x 90 face-pass image (161 x 91 = 14 651 words) is inside, 160 x 120 outside, as it is outside k_roi's bound.
static constexpr int kRoiHnewMaxBytes = 160 * 1024 - (2 * kRoiMaxWin * 2 + 16 + kRoiHnewVoteWords * 4 + kRoiMaxWin * 8) - 64;      // 122 800
static_assert(kRoiHnewMaxBytes == 160 * 1024 - roi_hnew_fixed_bytes() - 64, "the bound follows the kernel's carve-up");
static_assert(8 * ((161 * 91 + 3) & ~3) <= kRoiHnewMaxBytes, "the part detectors' 160 x 90 face-pass image stays inside the bound");
// the squared plane is u32 without a high-byte plane: an image inside the bound has at most kRoiHnewMaxBytes / 8 pixels, and their
// squares sum to less than 2^32
static_assert(65025ull * (kRoiHnewMaxBytes / 8) < (1ull << 32), "the total of squares of an image inside the bound fits 32 bits");
// ... and its resized levels, smaller than the image, fit the room over votes + vnf
static_assert(kRoiHnewMaxBytes / 8 <= kRoiHnewLevBytes, "a level image fits the room it is staged in");
inline long long hnew_roi_image_bytes(int cols, int rows) { return 8 * ((((long long)cols + 1) * (rows + 1) + 3) & ~3ll); }
inline bool hnew_roi_fits_lds(int cols, int rows) { return cols >= 1 && rows >= 1 && hnew_roi_image_bytes(cols, rows) <= kRoiHnewMaxBytes; }

// the cascade as k_roi_hnew reads it: its LbpStageDev records, then (at roi_hnew_weak_off) a RoiHnewWeak per weak classifier, and
// room for a wide scalar load behind the last record
void build_hnew_roi_table(const HnewCascade &c, std::vector<unsigned char> &blob);

} // namespace nvca
