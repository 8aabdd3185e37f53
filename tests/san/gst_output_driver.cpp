// gst_output_driver.cpp -- test infrastructure: the GStreamer shim's pure output code (gst/element_output.cpp) on cases read from a
// file, one per line (numbers separated by blanks; a box is "x y w h"):
//   face <frame width> <pts> <width_to_process> <view> <overlay set> <n> <boxes>
//   tracker <visual mode> <n> <boxes>
//   part <kind> <frame width> <pts> <detect_event> <view> <overlay set> <na> <boxes a> <nb> <boxes b> <nfaces> <faces>
//   due <n> <server_events> <now ms> <last ms> <events_ms>
//   motion <structure>            faces <cap> <structure>          (gst_structure_from_string)
// For an output case it prints three lines -- "event <gst_structure_to_string | none>", "payload <string>", "shapes <kind,x,y,w,h,
// b,g,r,a;...>" -- and for the others one: "due <0|1>", "motion <0|1>", "faces <n> <x,y,w,h;...>".
#include <gst/gst.h>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../nubomedia-vca_amd/gst/element_output.h"
using namespace nvca_gst;

static std::vector<nvca_rect> boxes(std::istream &in)
{
    int n = 0;
    in >> n;
    std::vector<nvca_rect> r((size_t)n);
    for (auto &b : r) in >> b.x >> b.y >> b.w >> b.h;
    return r;
}
static void print(const ElementOutput &o)
{
    gchar *ev = o.event ? gst_structure_to_string(o.event.get()) : NULL;
    printf("event %s\npayload %s\nshapes ", ev ? ev : "none", o.payload.c_str());
    g_free(ev);
    for (const nvca_shape &s : o.shapes) printf("%d,%d,%d,%d,%d,%d,%d,%d,%d;", s.kind, s.x, s.y, s.w, s.h, s.bgra[0], s.bgra[1], s.bgra[2], s.bgra[3]);
    printf("\n");
}

int main(int argc, char **argv)
{
    gst_init(&argc, &argv);
    if (argc < 2) { fprintf(stderr, "usage: %s <cases file>\n", argv[0]); return 2; }
    std::ifstream file(argv[1]);
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "face") {
            int width, w2p, view, overlay; guint64 pts;
            in >> width >> pts >> w2p >> view >> overlay;
            const std::vector<nvca_rect> b = boxes(in);
            print(face_output(b.data(), (int)b.size(), width, pts, w2p, view, overlay != 0));
        } else if (what == "tracker") {
            int visual;
            in >> visual;
            const std::vector<nvca_rect> b = boxes(in);
            print(tracker_output(b.data(), (int)b.size(), visual));
        } else if (what == "part") {
            int kind, width, detect_event, view, overlay; guint64 pts;
            in >> kind >> width >> pts >> detect_event >> view >> overlay;
            const std::vector<nvca_rect> a = boxes(in), b = boxes(in), f = boxes(in);
            print(part_output(kind, a.data(), (int)a.size(), b.data(), (int)b.size(), f.data(), (int)f.size(), width, pts, detect_event, view, overlay != 0));
        } else if (what == "due") {
            int n, server_events, events_ms; double now, last;
            in >> n >> server_events >> now >> last >> events_ms;
            printf("due %d\n", signal_due(n, server_events, now, last, events_ms) ? 1 : 0);
        } else if (what == "motion" || what == "faces") {
            int cap = 0;
            if (what == "faces") in >> cap;
            std::string text;
            std::getline(in, text);
            GstStructure *m = gst_structure_from_string(text.c_str(), NULL);
            if (!m) { fprintf(stderr, "bad structure: %s\n", text.c_str()); return 3; }
            if (what == "motion") printf("motion %d\n", message_has_motion(m) ? 1 : 0);
            else {
                std::vector<nvca_rect> f((size_t)cap + 1, nvca_rect{-1, -1, -1, -1});       // one guard entry behind the capacity
                const int n = message_faces(m, f.data(), cap);
                printf("faces %d ", n);
                for (int i = 0; i < n; i++) printf("%d,%d,%d,%d;", f[i].x, f[i].y, f[i].w, f[i].h);
                printf("\n");
                if (f[(size_t)cap].x != -1) { fprintf(stderr, "wrote behind the capacity\n"); return 4; }
            }
            gst_structure_free(m);
        } else if (!what.empty()) { fprintf(stderr, "unknown case: %s\n", line.c_str()); return 3; }
    }
    return 0;
}
