// host_logic.h -- sequential host-side pieces (see host_logic.cpp)
#pragma once
#include <vector>
#include "../../include/nubovca.h"
#include "pixel_rules.h"

namespace nvca {

void group_rectangles(std::vector<nvca_rect> &rects, int groupThreshold, double eps,
                      std::vector<int> *weights = nullptr);

// its first half, shared with the weighted form (group_levels.cpp): cv::partition under SimilarRects(eps) -- labels[i] is rects[i]'s
// class, classes numbered by their first member -- and per class the averaged rectangle rr[c] and the member count rw[c]; returns the
// number of classes
int group_classes(const std::vector<nvca_rect> &rects, double eps, std::vector<int> &labels, std::vector<nvca_rect> &rr, std::vector<int> &rw);

struct TrackedFace { nvca_rect box; int id; };
struct Faces {                 // FACE/Faces.hpp: the per-stream list with ids
    std::vector<TrackedFace> faces;
    int next_id = 0;
    void track(const std::vector<nvca_rect> &current, int track_threshold);
    void clear() { faces.clear(); }
};

void join_objects(std::vector<nvca_rect> &seg_bounds, int min_area, long max_area, int distance);

// argument checks the drawing entry points share (NVCA_OK / NVCA_ERR_ARG).  nvca_draw_shapes / nvca_draw_shapes_yuv420: 0 .. 1024 shapes,
// known kinds, coordinates and sizes within 2^24; nvca_overlay_blend / nvca_overlay_blend_yuv420: the image, its placement and the boxes
int check_shape_list(const nvca_shape *shapes, int n);
int check_overlay_args(const nvca_rect *boxes, int n, const nvca_overlay *ov);

// part detectors' merging heuristics (EYE/kmseyedetect.cpp:778-913, NOSE/kmsnosedetect.cpp:745-790, MOUTH/kmsmouthdetect.cpp:750-796)
void merge_consecutive_nm(std::vector<nvca_rect> &cn, const std::vector<nvca_rect> &old, const nvca_rect &face, int scale, int dis, std::vector<nvca_rect> &res);
bool contain_bb(int px, int py, const nvca_rect &r);
void merge_eyes_current(const nvca_rect &face_bb, const std::vector<nvca_rect> &eye_r, std::vector<nvca_rect> &eyes, int scale, bool eye_left);
void merge_eyes_consecutive(std::vector<nvca_rect> &ce, const std::vector<nvca_rect> &old, std::vector<nvca_rect> &res);
void to_global(std::vector<nvca_rect> &v, const nvca_rect &face, int scale);

} // namespace nvca
