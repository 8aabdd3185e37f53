// element_output.cpp -- the reference elements' send_event / draw rules (element_output.h), one statement each.
#include "element_output.h"
#include <math.h>
#include <stdio.h>

namespace nvca_gst {

static std::string box_str(const nvca_rect &r)
{
    return "x:" + std::to_string((guint)r.x) + ",y:" + std::to_string((guint)r.y) + ",width:" + std::to_string((guint)r.w) +
           ",height:" + std::to_string((guint)r.h) + ";";
}
// field "<idx>" of the message: a structure <sname> with type / x / y / width / height (times mul)
static void add_box(GstStructure *message, const char *sname, const char *type, int idx, const nvca_rect &r, int mul)
{
    GstStructure *st = gst_structure_new(sname, "type", G_TYPE_STRING, type, "x", G_TYPE_UINT, (guint)r.x * mul, "y", G_TYPE_UINT,
                                         (guint)r.y * mul, "width", G_TYPE_UINT, (guint)r.w * mul, "height", G_TYPE_UINT, (guint)r.h * mul, NULL);
    char id[16]; snprintf(id, sizeof(id), "%d", idx);
    gst_structure_set(message, id, GST_TYPE_STRUCTURE, st, NULL);
    gst_structure_free(st);
}
static GstStructure *new_message(const char *name, bool stamped, guint64 pts)
{
    GstStructure *message = gst_structure_new_empty(name);
    if (stamped) {
        GstStructure *ts = gst_structure_new("time", "pts", G_TYPE_UINT64, pts, NULL);
        gst_structure_set(message, "timestamp", GST_TYPE_STRUCTURE, ts, NULL);
        gst_structure_free(ts);
    }
    return message;
}
// corners (x0, y0) and (x1, y1) inclusive, as cvRectangle takes them
static nvca_shape rect3(int x0, int y0, int x1, int y1, const guint8 *col)
{
    return nvca_shape{NVCA_SHAPE_RECT3, x0, y0, x1 - x0, y1 - y0, {col[0], col[1], col[2], col[3]}};
}
static nvca_shape ring4(int cx, int cy, int radius, const guint8 *col)
{
    return nvca_shape{NVCA_SHAPE_RING4, cx, cy, radius, 0, {col[0], col[1], col[2], col[3]}};
}
#define BGR_OF_RGB(r, g, b) {b, g, r, 0}

ElementOutput face_output(const nvca_rect *boxes, int n, int frame_width, guint64 pts, int width_to_process, int view, bool overlay_set)
{
    ElementOutput o;                                        // kms_face_send_event, FACE/kmsfacedetect.cpp:179-249
    o.event.reset(new_message("message", true, pts));
    for (int i = 0; i < n; i++) { add_box(o.event.get(), "face", "face", i, boxes[i], 1); o.payload += box_str(boxes[i]); }
    if (view > 0 && !overlay_set) {
        // Faces::draw: (x, y) .. (x + w - 1, y + h - 1) of the working-image box, times the integer scale, in
        // colors[1] = CV_RGB(0,128,255)  (FACE/BaseFace.cpp:70-82, FACE/kmsfacedetect.cpp:144-151,832-850)
        static const guint8 col[4] = BGR_OF_RGB(0, 128, 255);
        const int scale = frame_width / width_to_process;
        for (int i = 0; i < n; i++)
            o.shapes.push_back(rect3(boxes[i].x, boxes[i].y, boxes[i].x + boxes[i].w - scale, boxes[i].y + boxes[i].h - scale, col));
    }
    return o;
}

ElementOutput tracker_output(const nvca_rect *boxes, int n, int visual_mode)
{
    ElementOutput o;                                        // signal only, no downstream event: TRK/gstnubotracker.cpp:383-414
    static const guint8 col[4] = {0, 0, 255, 0};            /* :389: tl() .. br(), Scalar(0,0,255) */
    for (int i = 0; i < n; i++) {
        if (visual_mode > 0) o.shapes.push_back(rect3(boxes[i].x, boxes[i].y, boxes[i].x + boxes[i].w, boxes[i].y + boxes[i].h, col));
        o.payload += box_str(boxes[i]);
    }
    return o;
}

ElementOutput part_output(int kind, const nvca_rect *a, int na, const nvca_rect *b, int nb, const nvca_rect *faces, int nfaces,
                          int frame_width, guint64 pts, int detect_event, int view, bool overlay_set)
{
    ElementOutput o;
    int i = 0;
    if (kind == NVCA_PART_EYE) {                            // left eyes first, then right eyes (EYE/kmseyedetect.cpp:245-284)
        o.event.reset(new_message("message", true, pts));
        for (int k = 0; k < nb; k++, i++) { add_box(o.event.get(), "eye_left", "eye", i, b[k], 1); o.payload += box_str(b[k]); }
        for (int k = 0; k < na; k++, i++) { add_box(o.event.get(), "eye_right", "eye", i, a[k], 1); o.payload += box_str(a[k]); }
    } else if (kind == NVCA_PART_NOSE) {                    // "noses" carries no timestamp (NOSE/kmsnosedetect.cpp:226-249)
        o.event.reset(new_message("noses", false, pts));
        for (int k = 0; k < na; k++, i++) { add_box(o.event.get(), "noses", "nose", i, a[k], 1); o.payload += box_str(a[k]); }
    } else if (kind == NVCA_PART_MOUTH) {                   // faces x norm_faces (int of scale_o2f), then mouths (MOUTH/kmsmouthdetect.cpp:210-256,305-309)
        const int norm_faces = detect_event ? 1 : (int)(((float)frame_width) / ((float)160));
        o.event.reset(new_message("message", true, pts));
        for (int k = 0; k < nfaces; k++, i++) add_box(o.event.get(), "face", "face", i, faces[k], norm_faces);
        for (int k = 0; k < na; k++, i++) { add_box(o.event.get(), "mouth", "mouth", i, a[k], 1); o.payload += box_str(a[k]); }
    } else {                                                // EAR: right list then left list; the reference builds a message and
        for (int k = 0; k < nb; k++) o.payload += box_str(b[k]);   // never pushes it (EAR/kmseardetect.cpp:196-290), so there is none
        for (int k = 0; k < na; k++) o.payload += box_str(a[k]);
    }
    if (1 != view || overlay_set) return o;
    if (kind == NVCA_PART_EYE) {                            // one circle per side, first box only; the right eye's radius is
        static const guint8 col[4] = {255, 0, 0, 0};        // reused for the left eye (EYE/kmseyedetect.cpp:1071-1099), Scalar(255, 0, 0)
        int radius = -1;
        const nvca_rect *first[2] = {na > 0 ? a : NULL, nb > 0 ? b : NULL};       // right eye, then left eye
        for (const nvca_rect *e : first) {
            if (!e) continue;
            if (radius < 0) radius = (int)lrint((e->w + e->h) * 0.25);
            o.shapes.push_back(ring4(e->x + e->w / 2, e->y + e->h / 2, radius, col));
        }
        return o;
    }
    // palettes and corner arithmetic as written in NOSE :808-815,902-905 (x + w, y + h - 1),
    // MOUTH :814-821,900-903 (x + w - 1, y + h - 1), EAR :736-743,754-758 (x + w, y + h - 1)
    static const guint8 nose_col[8][4] = {BGR_OF_RGB(255, 0, 255), BGR_OF_RGB(255, 0, 0), BGR_OF_RGB(255, 255, 0), BGR_OF_RGB(255, 128, 0),
                                          BGR_OF_RGB(0, 255, 0), BGR_OF_RGB(0, 255, 255), BGR_OF_RGB(0, 128, 255), BGR_OF_RGB(0, 0, 255)};
    static const guint8 mouth_col[8][4] = {BGR_OF_RGB(255, 255, 0), BGR_OF_RGB(255, 128, 0), BGR_OF_RGB(255, 0, 0), BGR_OF_RGB(255, 0, 255),
                                           BGR_OF_RGB(0, 128, 255), BGR_OF_RGB(0, 0, 255), BGR_OF_RGB(0, 255, 255), BGR_OF_RGB(0, 255, 0)};
    static const guint8 ear_col[8][4] = {BGR_OF_RGB(0, 0, 255), BGR_OF_RGB(0, 128, 255), BGR_OF_RGB(0, 255, 255), BGR_OF_RGB(0, 255, 0),
                                         BGR_OF_RGB(255, 128, 0), BGR_OF_RGB(255, 255, 0), BGR_OF_RGB(255, 0, 0), BGR_OF_RGB(255, 0, 255)};
    const guint8 (*pal)[4] = kind == NVCA_PART_NOSE ? nose_col : kind == NVCA_PART_MOUTH ? mouth_col : ear_col;
    const int dx = kind == NVCA_PART_MOUTH ? -1 : 0;
    int j = 0;              // ear: right list first (EAR :815-816); the palette index runs on into the left list (the reference restarts it, :735)
    if (kind == NVCA_PART_EAR) for (int k = 0; k < nb; k++, j++) o.shapes.push_back(rect3(b[k].x, b[k].y, b[k].x + b[k].w + dx, b[k].y + b[k].h - 1, pal[j % 8]));
    for (int k = 0; k < na; k++, j++) o.shapes.push_back(rect3(a[k].x, a[k].y, a[k].x + a[k].w + dx, a[k].y + a[k].h - 1, pal[j % 8]));
    return o;
}

// every element's send_event: something was found, events are on, and the last signal is more than events-ms old
// (FACE/kmsfacedetect.cpp:228-241, TRK/gstnubotracker.cpp:402-413)
bool signal_due(int n, int server_events, double now_ms, double last_ms, int events_ms)
{
    return n > 0 && server_events == 1 && now_ms - last_ms > events_ms;
}

// a queued upstream "message": does it carry a "motion" structure?  (FACE/kmsfacedetect.cpp:680-712)
bool message_has_motion(const GstStructure *m)
{
    const gint len = gst_structure_n_fields(m);
    for (gint i = 0; i < len; i++) {
        const gchar *name = gst_structure_nth_field_name(m, i);
        if (g_strcmp0(name, "motion") == 0 && gst_structure_has_field_typed(m, name, GST_TYPE_STRUCTURE)) return true;
    }
    return false;
}

// faces handed over by an upstream element (EYE/kmseyedetect.cpp:680-724): sub-structures whose type == "face"
int message_faces(const GstStructure *m, nvca_rect *faces, int cap)
{
    int n = 0;
    const gint len = gst_structure_n_fields(m);
    for (gint i = 0; i < len && n < cap; i++) {
        const gchar *name = gst_structure_nth_field_name(m, i);
        if (g_strcmp0(name, "timestamp") == 0) continue;
        GstStructure *d = NULL;
        if (!gst_structure_get(m, name, GST_TYPE_STRUCTURE, &d, NULL) || !d) continue;
        if (g_strcmp0(gst_structure_get_string(d, "type"), "face") == 0) {
            guint x = 0, y = 0, w = 0, h = 0;
            gst_structure_get(d, "x", G_TYPE_UINT, &x, "y", G_TYPE_UINT, &y, "width", G_TYPE_UINT, &w, "height", G_TYPE_UINT, &h, NULL);
            faces[n++] = nvca_rect{(int)x, (int)y, (int)w, (int)h};
        }
        gst_structure_free(d);
    }
    return n;
}

}  // namespace nvca_gst
