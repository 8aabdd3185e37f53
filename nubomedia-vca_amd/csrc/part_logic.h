// part_logic.h -- the per-frame state machine of the eye / nose / mouth / ear elements (see part_logic.cpp): pure host code on
// box lists, no HIP, no context.  part_call.cpp drives it around the device work; the CPU driver under tests/san drives it alone.
#pragma once
#include <deque>
#include <vector>
#include "../../include/nubovca.h"
#include "host_logic.h"
#include "host_math.h"

namespace nvca {

typedef std::vector<nvca_rect> RectV;

// what a stream carries from frame to frame
struct PartState {
    RectV faces, la, lb;                     // faces; eyes_r / noses / mouths / lear; eyes_l / rear
    int num_frame = 0, num_frames_to_process = 0, no_det_a = 0, no_det_b = 0;      // (EAR: one counter for both sides, in no_det_a)
    std::deque<RectV> queue;                 // face lists pushed by an upstream face detector (detect-event), at most kQueueLimit
    static constexpr size_t kQueueLimit = 16;
    void push_faces(const nvca_rect *f, int n) { if (queue.size() < kQueueLimit) queue.emplace_back(f, f + n); }
};

// conf_images: the three scales and the two working-image sizes of a W x H frame
struct PartScales {
    double o2f = 1, x2o = 1, f2x = 1;        // original -> face-pass image, part image -> original, face-pass image -> part image
    int fw = 0, fh = 0, pw = 0, ph = 0;      // face-pass image, part image
};
bool part_scales(const nvca_part_params &p, int W, int H, PartScales &out);       // false: frame too small

// the face passes of the elements.  A stream's face pass is one of these at scaleFactor 1 + scale_factor_pct / 100.
enum PartFacePass { kPassNone = -1, kPassEye = 0, kPassNoseMouth = 1, kPassEar = 2 };
struct FacePassRule { int min_neighbors, flags, minw, minh; bool max_is_image, mirrored; };
const FacePassRule &face_pass_rule(int pass);

// what the gate decided for one frame of one stream, and what the stream wants computed for it
struct PartFrame {
    bool early_return = false, run = false, popped = false;      // popped: a queued face list was taken (it is now PartState::faces)
    // working images (all of them [equalizeHist](resize(gray)) of the frame): the part image pw x ph, always equalized after the resize
    bool eye_chain = false;                  // the resizes read the equalized full-size gray image (EYE), not the plain gray image
    bool face_image = false, face_post_eq = false, mirror = false;     // a face-pass image fw x fh; equalized after the resize; with its mirror image
    int pass = kPassNone; double pass_sf = 0;        // the face pass over the face-pass image
    RectV faces;                             // no face pass of its own (detect-event): the faces the gate took for THIS frame
};
PartFrame part_gate(PartState &st, const nvca_part_params &p);

// one detectMultiScale call on a sub-matrix of the part image
struct PartSearch {
    nvca_rect roi{0, 0, 0, 0};
    int cascade = 0, side = 0;               // cascade a (0) or b (1); side: EYE right (0) / left (1), EAR side 0 / 1
    double sf = 1.1; int min_neighbors = 0, flags = 0, minw = 0, minh = 0;
    bool valid = false;                      // false: cv::Mat's ROI constructor would have thrown (the reference never gets there with such
                                             // a rectangle: nothing is searched, nothing is detected)
};
// the searches of a frame that runs, in order (per face; EYE: right then left; EAR: every face of side 0, then of side 1).
// `faces` / `faces_mirror`: the results of the stream's face pass on the image / its mirror image (null where there is none).
void part_rois(PartState &st, const nvca_part_params &p, const PartScales &sc, const PartFrame &pf, const RectV *faces, const RectV *faces_mirror,
               std::vector<PartSearch> &out);
// the merging heuristics, the hysteresis and the per-call clearing; results[k]: what search k found (null: not searched)
void part_finish(PartState &st, const nvca_part_params &p, const PartScales &sc, const PartFrame &pf, const std::vector<PartSearch> &searches,
                 const std::vector<const RectV *> &results);

// Roll-back.  The gate and part_rois advance the state; whoever may still fail after them takes a snapshot first.
struct PartSnap {
    RectV faces, la, lb; int num_frame = 0, to_process = 0, no_a = 0, no_b = 0;
    bool popped = false; RectV front;        // the gate took a queued face list: it goes back to the head of the queue
    void note_popped(const PartState &st) { popped = true; front = st.faces; }     // right after a gate that reported `popped`
};
PartSnap part_snapshot(const PartState &st);
void part_restore(PartState &st, PartSnap &snap);

} // namespace nvca
