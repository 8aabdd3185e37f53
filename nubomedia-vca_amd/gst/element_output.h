// element_output.h -- what an element hands on for one processed frame, as pure code: from result rectangles and the parameters
// that matter to the downstream event, the signal payload and the outlines to draw.  Nothing here calls the library, touches an
// element, reads the clock or the environment, so tests/san/gst_output_driver.cpp checks it where there is no GPU.
#pragma once
#include <gst/gst.h>
#include <memory>
#include <string>
#include <vector>
#include "nubovca.h"

namespace nvca_gst {

struct StructureFree { void operator()(GstStructure *s) const { gst_structure_free(s); } };
struct ElementOutput {
    std::unique_ptr<GstStructure, StructureFree> event;    // goes downstream as a CUSTOM_DOWNSTREAM event; empty: nothing is pushed
    std::string payload;                                   // what the string signal carries when signal_due lets it out
    std::vector<nvca_shape> shapes;                        // outlines for one nvca_draw_shapes call, in drawing order
};

// boxes in frame coordinates, as the library returns them
ElementOutput face_output(const nvca_rect *boxes, int n, int frame_width, guint64 pts, int width_to_process, int view, bool overlay_set);
ElementOutput tracker_output(const nvca_rect *boxes, int n, int visual_mode);
// a / b: the library's two result lists of an NVCA_PART_* stream (eye: right / left; ear: left / right side); faces: nvca_part_stream_faces
ElementOutput part_output(int kind, const nvca_rect *a, int na, const nvca_rect *b, int nb, const nvca_rect *faces, int nfaces,
                          int frame_width, guint64 pts, int detect_event, int view, bool overlay_set);

// activate-events / events-ms: n results of this frame, the last signal at last_ms
bool signal_due(int n, int server_events, double now_ms, double last_ms, int events_ms);

// upstream events
bool message_has_motion(const GstStructure *m);
int message_faces(const GstStructure *m, nvca_rect *faces, int cap);       // returns how many were stored (at most cap)

}  // namespace nvca_gst
