// part_call.h -- one batched call of the part detectors: what parts.cpp (entry points, tickets), part_call.cpp (the call's two
// halves) and part_images.cpp (its working images) hand to each other.
#pragma once
#include "host_state.h"
#include "part_logic.h"
#include <algorithm>
#include <deque>

struct nvca_part_stream {
    nvca_ctx *ctx;
    nvca_part_params p;
    const nvca_cascade *face, *a, *b;
    nvca::PartState st;
    nvca_pixel_layout input{};        // format NVCA_PIX_BGR: packed BGR frames; else the planes of its 4:2:0 frames (nvca_part_stream_set_input)
    const nvca_pixel_layout *yuv() const { return input.format != NVCA_PIX_BGR ? &input : nullptr; }
};

namespace nvca {

// Streams of one batched call that were handed the same frame (the part detectors of one video stream all see the buffer the
// face detector saw) share what they compute identically from it: the upload, the working images and the face pass.  And the
// frames of the call share launches: every working image of one (frame geometry, size, chain) is made by one launch set, every
// face pass of one kind over those images is one job.  Same arithmetic on the same bytes: the results are those of per-stream calls.
struct FrameGroup {
    const void *data = nullptr; int w = 0, h = 0, stride = 0, mem = 0;
    nvca_pixel_layout layout{};              // of the streams that were handed the frame (format NVCA_PIX_BGR: a packed frame); a call keeps the layouts it was submitted with
    const nvca_pixel_layout *yuv() const { return layout.format != NVCA_PIX_BGR ? &layout : nullptr; }
    const void *bgr = nullptr;               // the frame on the device (the caller's, or the one upload of a host frame): packed BGR, or the base of its planes
    int eye_index = -1;                      // an eye detector looks at it: index of its full-size gray image / LUT
    size_t upload_at = 0, gray_at = 0;       // arena offsets
};
struct ImageRef { int batch = -1, k = 0; };
struct ImageBatch {                          // the working images [equalizeHist](resize(gray or equalized gray)) of one size
    int W = 0, H = 0, stride = 0, dw = 0, dh = 0; bool eye = false, post_eq = true, flips = false;
    nvca_pixel_layout layout{};              // of the source frames (one launch set reads planes of one layout)
    std::vector<int> members;                // frame groups, image k belongs to members[k]
    size_t at = 0, slot = 0; uint8_t *base = nullptr;        // image k at base + k * slot (pitch dw), its mirror image at base + (count + k) * slot
    const uint8_t *image(int k, bool mirrored = false) const { return base + slot * ((mirrored ? members.size() : 0) + k); }
};
struct FacePass {                            // one face pass (part_logic.h: PartFacePass) of one cascade at one scale factor over images of one batch
    int type = 0; const nvca_cascade *c = nullptr; int batch = 0; double sf = 0;
    std::vector<int> members;                // images of the batch that some stream wants searched
    std::vector<DetectJob *> jobs;           // kJobImages images per job (image + mirror image pairs: half as many)
    int per_job() const { return face_pass_rule(type).mirrored ? kJobImages / 2 : kJobImages; }
    ~FacePass() { for (DetectJob *j : jobs) detect_job_free(j); }
};
// One frame of one part stream on its way through a batched call: what the phases hand to each other.
struct PartWork {
    nvca_part_stream *s = nullptr; const nvca_frame *f = nullptr;
    PartScales sc; PartFrame gate;
    int lane = 0, group = -1, pass = -1;
    ImageRef small, part_ref;
    std::vector<PartSearch> searches;        // (part_logic.h: part_rois) ...
    std::vector<DetectJob *> jobs;           // ... and their queued jobs; nullptr: not a valid ROI, nothing is searched
    ~PartWork() { for (DetectJob *j : jobs) detect_job_free(j); }
};
struct PartCall {
    nvca_ctx *ctx = nullptr; int n = 0, parity = 0, seq = 0;
    std::vector<nvca_part_stream *> streams; std::vector<nvca_frame> frames;
    std::vector<FrameGroup> groups;
    std::vector<ImageBatch> batches;
    std::deque<FacePass> passes;
    std::vector<PartWork> work;
    std::vector<DetectJob *> jobs;
    std::vector<int> job_lane;
    int n_eye = 0;
    JobRound *round = nullptr; bool queued = false;       // the face passes' first round, left in flight by the front half
    double t0 = 0, t1 = 0;
    // The gates of the front half (and part_rois in the back half) advance per-stream state; plans, buffers and launches come after
    // them and may still fail (too many scales, allocation, a refused launch).  Whatever the error, the call leaves every
    // stream as it found it -- the GStreamer shim re-runs the streams one by one after a refused batch, and a gate that had
    // already advanced would then advance twice and drop a queued face event.  Nothing of the call may stay in flight either:
    // the caller's frames (H2D copies) and the arena are only safe to reuse once the lanes have drained.
    std::vector<PartSnap> snaps; bool armed = true;
    bool holds(const nvca_part_stream *s) const { return std::find(streams.begin(), streams.end(), s) != streams.end(); }
    ~PartCall();
};

// ---- part_call.cpp: a batched call in two halves
int part_front(nvca_ctx *ctx, PartCall &c, int n, nvca_part_stream *const *streams, const nvca_frame *frames);
int part_back(nvca_ctx *ctx, PartCall &c, nvca_rect *out_a, int cap_a, int *n_a, nvca_rect *out_b, int cap_b, int *n_b);

// ---- part_images.cpp: every working image the call needs, in a handful of launches on the current lane
int part_images(nvca_ctx *ctx, std::vector<FrameGroup> &groups, std::vector<ImageBatch> &batches, int n_eye);
int part_images_done(nvca_ctx *ctx, const int *lanes, int n);       // the lanes that read the images wait for them

} // namespace nvca
