// trk_host.h -- the pure host parts of nvca_tracker_batch_process (tracker.cpp): which trackers of a call share a launch set, which
// pixel kernel a launch set takes, how many bytes a host frame needs in the staging buffer, and the per-slot component lists out of
// the words the device left.  No HIP header, no context: a plain C++ compiler takes trk_host.cpp (tests/san/trk_host_driver.cpp
// drives it under the sanitizers).
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/nubovca.h"
#include "trk_layout.h"

namespace nvca {

// ---- launch sets: one per (width, height, format) -- the pixel kernels are instances per format, the planes travel per slot.  Sets
// in the order of their first member, members ascending: set s is member[begin[s] .. begin[s + 1]).
struct TrkFrameKey { int w, h, fmt; };
struct TrkLaunchSets {
    std::vector<int> member, begin;
    int count() const { return (int)begin.size() - 1; }
};
void trk_launch_sets(const TrkFrameKey *keys, int n, TrkLaunchSets &sets);

// ---- the wide pixel kernels' loads, for ONE member of a launch set (one member that fails sends its whole set to the general kernel).
// Every format: width % 4 == 0.  BGRA (k_trk_pixel4: 16-byte loads of four pixels): `stride` and a device frame's base on 16 bytes.
// 4:2:0 (k_trk_pixel_yuv8; the strides are the layout's, `stride` is not read): luma rows and NV12 chroma rows on 8 bytes (8-byte loads),
// I420 chroma rows on 4 (4 bytes of each plane).  Packed 4:2:2 (k_trk_pixel_yuv422x4: 8-byte loads of two pixel pairs): the plane's rows
// on 8 bytes -- base + offset[0] and stride[0].  A host frame is staged and counts as base 0: the staging buffer is 256-byte aligned
// and every staged frame starts on a multiple of 256 bytes in it (trk_staged_bytes).
bool trk_wide_ok(int fmt, const nvca_pixel_layout *layout, int mem, uintptr_t base, int stride, int width);

// ---- bytes a host frame takes in the staging buffer (what is copied: a 4:2:0 / 4:2:2 frame's extent, a packed frame's rows), a multiple of 256
size_t trk_staged_bytes(const nvca_pixel_layout *yuv, int stride, int w, int h);

// ---- the component list as the device left it (trk_layout.h).  trk_component_count: the header's count against the list -- NVCA_OK, or
// the code and text of a refusal.  trk_component_lists: the `total` components behind the header as one list of boxes per slot, in
// seed order (raster order of each component's first seed pixel = cvSegmentMotion's output order); a slot outside [0, batch) refuses.
int trk_component_count(int total, std::string &err);
int trk_component_lists(const int *words, int total, int batch, std::vector<std::vector<nvca_rect>> &lists, std::string &err);

} // namespace nvca
