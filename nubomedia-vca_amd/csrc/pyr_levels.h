// pyr_levels.h -- the image pyramid of a CV_HAAR_SCALE_IMAGE call and of detectMultiScale on a new-format cascade as plain host
// arithmetic (no HIP, no context): which levels a call has, the grid a level is scanned on, and where the levels lie in a lane's gray
// and plane buffers.  pyramid.cpp puts the layout on the device; lbp_tables.cpp and roi_batch.cpp read the same rules.
#pragma once
#include <cstddef>
#include <vector>

namespace nvca {

// The most levels a plan of the large-image routes holds.  OpenCV's loop has no bound (a scale factor just above 1 makes it as long as
// one likes); a call with more levels is refused with NVCA_ERR_ARG, never answered from its first levels.  The callers ask for one
// level more than this, so that "too many" shows.
constexpr size_t kMaxPyrLevels = 4095;

// the pyramid levels of a CV_HAAR_SCALE_IMAGE call, smallest factor first, at most `cap` of them
struct SiLevel { double factor; int szw, szh, winw, winh; };
std::vector<SiLevel> si_levels(int ow, int oh, int cols, int rows, double sf, int minw, int minh, int maxw, int maxh, size_t cap);
// ... of detectMultiScale on a new-format cascade
std::vector<SiLevel> lbp_levels(int ow, int oh, int cols, int rows, double sf, int minw, int minh, int maxw, int maxh, size_t cap);

// a level's grid: window origins every level_step pixels from 0 while they stay below size - window (both scans)
inline int level_step(double f) { return f > 2 ? 1 : 2; }
inline int level_positions(int sz, int win, int step) { return sz > win ? (sz - win + step - 1) / step : 0; }

// a level inside the lane's buffers: its gray image (pitch gpitch bytes) at byte gray_off, its integral planes (pitch P) at element plane_off
struct PyrLevel { double f; int szw, szh, winw, winh; size_t gray_off; int gpitch; int plane_off; };
struct PyrLayout {
    int P = 0;                                  // pitch of every level's planes: that of the full image
    std::vector<PyrLevel> lv;
    size_t gray_total = 0, plane_total = 0;     // bytes / elements of one image's levels
};
PyrLayout pyr_layout(const std::vector<SiLevel> &levels, int cols);

} // namespace nvca
