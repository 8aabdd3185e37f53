// gstnubovca.cpp -- GStreamer shim: the reference's element surface
// on top of libnubovca_hip's C ABI.  Written from scratch; it keeps, per element,
//   factory name, GstVideoFilter base, in-place transform, caps, property names /
//   ranges / initial values, the string signal and the downstream custom event
// of the reference so that an unmodified pipeline (or Kurento's generic filter with
// "filter-factory" = element name) keeps working:
//   nubofacedetector  FACE/kmsfacedetect.cpp   (caps BGR  :129-133, props :1043-1102, signal "face-event" :1108-1113,
//                                               event "message" :196-226, motion events :680-755)
//   nubotracker       TRK/gstnubotracker.cpp   (caps BGRA :57-61,  props :504-542,  signal "tracker-event" :547-552)
//   nuboeyedetector / nubonosedetector / nubomouthdetector / nuboeardetector
//                     EYE/kmseyedetect.cpp:1274-1320 (props), :220-308 (event: eye_left*, eye_right*), :192-218,680-764 (faces in)
//                     NOSE/kmsnosedetect.cpp:1089-1135, :212-273 (event "noses")   MOUTH/kmsmouthdetect.cpp:205-282 (faces + mouths)
//                     EAR/kmseardetect.cpp:994-1038 ("meta-data"), :196-290 (signal only: the event is built but never pushed)
// All pixel work happens in the library (HIP); the shim is glue only: this file holds the per-GPU frontend, the one batching
// round and the GObject surface, combiner.h the leader election, element_output.cpp what an element emits for a frame.  One
// plugin ("nubovca") registers every factory; the reference ships one plugin per element.
#include <gst/gst.h>
#include <gst/video/video.h>
#include <gst/video/gstvideofilter.h>
#include <sys/time.h>
#include <time.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <mutex>
#include <atomic>
#include <map>
#include <memory>
#include <vector>
#include <algorithm>
#include "nubovca.h"
#include "combiner.h"
#include "element_output.h"
using namespace nvca_gst;

GST_DEBUG_CATEGORY_STATIC(nubovca_debug);
// No C++ exception crosses into GLib / GStreamer's C frames: every GObject / GstBaseTransform callback of the elements is a
// function-try-block ending in one of these.  A frame whose processing failed is passed on untouched with GST_FLOW_OK -- the
// reference never lets an error out of the element either (FACE/kmsfacedetect.cpp:897).
static void nvca_gst_caught(const char *where) noexcept
{
    try { throw; }
    catch (const std::exception &e) { g_warning("nubovca: %s: %s (frame / request dropped)", where, e.what()); }
    catch (...) { g_warning("nubovca: %s: unknown exception (frame / request dropped)", where); }
}
#define NVCA_GST_CATCH(where, ret) catch (...) { nvca_gst_caught(where); return ret; }
#define NVCA_GST_CATCH_VOID(where) catch (...) { nvca_gst_caught(where); }
// The element mutex inside a guarded callback is held through this: when an exception unwinds the try block the mutex is released
// BEFORE the handler runs -- a streaming thread that caught bad_alloc must not keep the element's GRecMutex locked for good (a
// property set from the application thread, or finalize, would block on it forever).
struct NvcaRecLock {
    GRecMutex *m;
    explicit NvcaRecLock(GRecMutex *mu) : m(mu) { g_rec_mutex_lock(m); }
    ~NvcaRecLock() { g_rec_mutex_unlock(m); }
    NvcaRecLock(const NvcaRecLock &) = delete;
    NvcaRecLock &operator=(const NvcaRecLock &) = delete;
};
#define GST_CAT_DEFAULT nubovca_debug

#define OPENCV_CASCADE_DIR "/usr/share/opencv/haarcascades"     /* FACE/kmsfacedetect.cpp:40 */

// ---------------------------------------------------------------- per-GPU frontend
// A media stream (= one element instance, one streaming thread: FACE/kmsfacedetect.cpp:857-898) is the independent unit: it
// lives on ONE GPU for its whole life, because its temporal state (Faces, the tracker's MHI and previous frame) is device
// resident.  The process holds one slot per visible GPU -- context, cascade handles, frame combiners -- created on first
// use; an element takes slot (instance counter mod slots) at its first frame and never migrates.  No data crosses GPUs.
//   NVCA_DEVICE=d        pin the whole process to GPU d (one slot)
//   NVCA_VIRTUAL_GPUS=n  n slots on one device (NVCA_DEVICE or 0): the multi-GPU code path on a one-GPU box, and a way to
//                        let several launch-bound pipelines queue their work in parallel
struct SharedCascade { nvca_cascade *h; int refs; };
struct GpuSlot;
static std::mutex g_ctx_mutex;
static std::vector<GpuSlot *> g_slots;          // filled once, entries live for the process
static bool g_slots_ready = false;
static int g_instances = 0;                     // elements that have taken a slot so far
// One frame on its way through a Combiner: the owner's handle, frame and result buffers (Lists lists of Cap rectangles) go in,
// status and counts come back.  kFaceCap, kTrkCap and kPartCap are the capacities of every buffer and call of their family.
static const int kFaceCap = 256, kTrkCap = 4096, kPartCap = 64;
template <class Handle, int Lists, int Cap> struct Req {
    static constexpr int lists = Lists, cap = Cap;
    Handle *h; nvca_frame frame; nvca_rect *out[Lists]; int n[Lists]; int rc; bool done;
};
typedef Req<nvca_face_stream, 1, kFaceCap> FaceReq;
typedef Req<nvca_part_stream, 2, kPartCap> PartReq;         // out[0] / out[1]: the library's lists a / b
struct TrkReq : Req<nvca_tracker, 1, kTrkCap> { double ts; };
struct GpuSlot {
    int index = 0, device = 0;
    nvca_ctx *ctx = nullptr;
    // Elements that name the same cascade file share one handle per GPU: their plans and scale tables are then shared in the
    // context, and their frames can ride in one batch (streams batch only when cascade, geometry and parameters agree).
    std::map<std::string, SharedCascade> cascades;
    Combiner<FaceReq> face_q;
    Combiner<TrkReq> trk_q;
    Combiner<PartReq> part_q;                   // eye / nose / mouth / ear elements of all streams of the slot
    std::atomic<int> registered{0};             // pool memories page-locked so far (NVCA_GST_STATS)
};

static void make_slots_locked()
{
    if (g_slots_ready) return;
    g_slots_ready = true;
    const char *dev = getenv("NVCA_DEVICE"), *virt = getenv("NVCA_VIRTUAL_GPUS");
    std::vector<int> devices;
    if (virt && atoi(virt) > 0) devices.assign((size_t)std::min(atoi(virt), 64), dev ? atoi(dev) : 0);
    else if (dev) devices.push_back(atoi(dev));
    else {
        int n = 0;
        if (nvca_device_count(&n) != NVCA_OK || n <= 0) n = 1;      // ctx creation reports the missing device
        for (int d = 0; d < n; d++) devices.push_back(d);
    }
    for (size_t i = 0; i < devices.size(); i++) { GpuSlot *g = new GpuSlot(); g->index = (int)i; g->device = devices[i]; g_slots.push_back(g); }
}
// NVCA_GST_REGISTER=1: pool memory that keeps coming back (decoders and converters recycle their GstBufferPool memories) is
// page-locked once with nvca_host_register, so its H2D copies are DMA from the buffer instead of going through the runtime's
// staging copy; the registration ends with the GstMemory (weak reference).  One-shot memories are left alone.  Off by
// default: measured on 16 x 1080p branches it gains 3 % when whole frames are copied and LOSES 23 % in the elements' default
// shrink-first mode, where only the rows the resize reads cross PCIe -- a strided DMA out of page-locked memory is slower
// than the runtime's packing of those rows from pageable memory.
struct RegNote { nvca_ctx *ctx; void *ptr; };
static void on_memory_gone(gpointer data, GstMiniObject *)
{
    RegNote *r = (RegNote *)data;
    nvca_host_unregister(r->ctx, r->ptr);
    delete r;
}
static void note_frame_memory(GpuSlot *g, GstVideoFrame *frame)
{
    static const bool off = !(getenv("NVCA_GST_REGISTER") && atoi(getenv("NVCA_GST_REGISTER")) != 0);
    static const GQuark seen_q = g_quark_from_static_string("nubovca-seen");
    GstMemory *mem = frame->map[0].memory;
    if (off || !g || !g->ctx || !mem || !frame->map[0].data || !frame->map[0].size) return;
    GstMiniObject *mo = GST_MINI_OBJECT_CAST(mem);
    const int seen = GPOINTER_TO_INT(gst_mini_object_get_qdata(mo, seen_q));
    if (seen < 0) return;                                   // registered, or registration refused once
    if (seen + 1 < 3) { gst_mini_object_set_qdata(mo, seen_q, GINT_TO_POINTER(seen + 1), NULL); return; }
    gst_mini_object_set_qdata(mo, seen_q, GINT_TO_POINTER(-1), NULL);
    if (nvca_host_register(g->ctx, frame->map[0].data, frame->map[0].size) != NVCA_OK) return;
    gst_mini_object_weak_ref(mo, on_memory_gone, new RegNote{g->ctx, frame->map[0].data});
    g->registered++;
}
// the slot an element lives on: assigned round-robin at its first frame, then fixed
static GpuSlot *take_slot()
{
    std::lock_guard<std::mutex> lk(g_ctx_mutex);
    make_slots_locked();
    GpuSlot *g = g_slots[(size_t)(g_instances++) % g_slots.size()];
    if (!g->ctx) {
        const int rc = nvca_ctx_create(g->device, &g->ctx);
        if (rc != NVCA_OK) { GST_ERROR("nvca_ctx_create(%d) failed (%d): no HIP device; frames pass through untouched", g->device, rc); g->ctx = nullptr; }
    }
    if (getenv("NVCA_GST_STATS")) fprintf(stderr, "nubovca: element %d -> slot %d (device %d)\n", g_instances - 1, g->index, g->device);
    return g;
}
static nvca_cascade *acquire_cascade(GpuSlot *g, const std::string &path)
{
    std::lock_guard<std::mutex> lk(g_ctx_mutex);
    auto it = g->cascades.find(path);
    if (it != g->cascades.end()) { it->second.refs++; return it->second.h; }
    nvca_cascade *h = nullptr;
    // (general: an installed new-format file with tree weak classifiers or tilted features -- haarcascade_frontalface_alt2.xml, the
    // *_2splits eye files -- loads as well; a file of stumps on upright features is the cascade the plain load makes)
    if (nvca_cascade_load_xml_ex(g->ctx, path.c_str(), NVCA_LOAD_HAAR_GENERAL, &h) != NVCA_OK) return nullptr;
    // a new-format HAAR file (OpenCV 3 / 4's haarcascade_*.xml): the part elements' face-region searches share one small-image launch
    // a round instead of a launch set each (nothing changes for the other formats; results never depend on it)
    (void)nvca_cascade_set_small_route(h, 1);
    g->cascades[path] = SharedCascade{h, 1};
    return h;
}
static void release_cascade(GpuSlot *g, nvca_cascade *h)
{
    if (!g) return;
    std::lock_guard<std::mutex> lk(g_ctx_mutex);
    for (auto it = g->cascades.begin(); it != g->cascades.end(); ++it)
        if (it->second.h == h) {
            if (--it->second.refs == 0) { nvca_cascade_free(h); g->cascades.erase(it); }
            return;
        }
}

// One round of a Combiner, for every family.  More than one request: the batched entry point is tried; when the family accepts
// its status, every owner gets that status, its counts and its rectangles.  Otherwise -- a single frame, or a batch not accepted --
// each request gets its own call and its own status, so one bad frame does not fail its neighbours.
// A family states its batched call, its single call and which batch statuses it accepts.
template <class Family, class R> static void run_round(nvca_ctx *ctx, std::vector<R *> &round)
{
    const int n = (int)round.size();
    bool batched = false;
    if (n > 1) {
        std::vector<decltype(R::h)> handles(n);
        std::vector<nvca_frame> frames(n);
        std::vector<nvca_rect> out[R::lists];
        std::vector<int> n_out[R::lists];
        for (int l = 0; l < R::lists; l++) { out[l].resize((size_t)n * R::cap); n_out[l].assign(n, 0); }
        for (int i = 0; i < n; i++) { handles[i] = round[i]->h; frames[i] = round[i]->frame; }
        const int rc = Family::batch(ctx, round, handles.data(), frames.data(), out, n_out);
        batched = Family::accepts(rc);
        for (int i = 0; batched && i < n; i++) {
            R *r = round[i];
            r->rc = rc;
            for (int l = 0; l < R::lists; l++) {
                r->n[l] = rc == NVCA_OK ? n_out[l][i] : 0;
                memcpy(r->out[l], out[l].data() + (size_t)i * R::cap, sizeof(nvca_rect) * (size_t)std::min(r->n[l], (int)R::cap));
            }
        }
    }
    if (!batched)
        for (R *r : round) r->rc = Family::single(r);
}
struct FaceCalls {
    static int batch(nvca_ctx *ctx, std::vector<FaceReq *> &round, nvca_face_stream **h, nvca_frame *f, std::vector<nvca_rect> *out, std::vector<int> *n_out)
    { return nvca_face_batch_process(ctx, (int)round.size(), h, f, out[0].data(), NULL, kFaceCap, n_out[0].data()); }
    static int single(FaceReq *r) { return nvca_face_stream_process(r->h, &r->frame, r->out[0], NULL, kFaceCap, &r->n[0]); }
    // a batch is refused with NVCA_ERR_ARG before any stream is touched (every frame is validated first): then each frame
    // runs alone.  Any other failure came after the streams' frame gates advanced and is reported to every owner as it is.
    static bool accepts(int rc) { return rc != NVCA_ERR_ARG; }
};
struct TrkCalls {
    static int batch(nvca_ctx *ctx, std::vector<TrkReq *> &round, nvca_tracker **h, nvca_frame *f, std::vector<nvca_rect> *out, std::vector<int> *n_out)
    {
        std::vector<double> ts(round.size());
        for (size_t i = 0; i < round.size(); i++) ts[i] = round[i]->ts;
        return nvca_tracker_batch_process(ctx, (int)round.size(), h, f, ts.data(), out[0].data(), kTrkCap, n_out[0].data());
    }
    static int single(TrkReq *r) { return nvca_tracker_process(r->h, &r->frame, r->ts, r->out[0], kTrkCap, &r->n[0]); }
    static bool accepts(int rc) { return FaceCalls::accepts(rc); }
};
struct PartCalls {
    static int batch(nvca_ctx *ctx, std::vector<PartReq *> &round, nvca_part_stream **h, nvca_frame *f, std::vector<nvca_rect> *out, std::vector<int> *n_out)
    { return nvca_part_batch_process(ctx, (int)round.size(), h, f, out[0].data(), kPartCap, n_out[0].data(), out[1].data(), kPartCap, n_out[1].data()); }
    static int single(PartReq *r) { return nvca_part_stream_process(r->h, &r->frame, r->out[0], kPartCap, &r->n[0], r->out[1], kPartCap, &r->n[1]); }
    // any failure leaves every stream of the call as it was (part_logic.cpp: PartSnap; part_call.h: PartCall): each frame then
    // runs on its own, so one bad frame does not fail its neighbours
    static bool accepts(int rc) { return rc == NVCA_OK; }
};

// the slot's shared handle of a file of the cascade directory; a failure is logged, not fatal (FACE/kmsfacedetect.cpp:167-176)
static bool need_cascade(GpuSlot *g, const char *file, nvca_cascade **c)
{
    if (!file || *c) return true;
    const char *dir = getenv("NVCA_CASCADE_DIR");
    const std::string path = std::string(dir ? dir : OPENCV_CASCADE_DIR) + "/" + file;
    *c = acquire_cascade(g, path);
    if (!*c) GST_ERROR("Error charging cascade %s: %s", path.c_str(), nvca_last_error(g->ctx));
    return *c != nullptr;
}
static double now_ms()
{
    struct timeval t; gettimeofday(&t, NULL);
    return t.tv_sec * 1000.0 + t.tv_usec / 1000.0;
}

// ---------------------------------------------------------------- what the three element families share
static nvca_frame frame_of(GstVideoFrame *frame)
{
    nvca_frame nf;
    nf.data = GST_VIDEO_FRAME_PLANE_DATA(frame, 0);
    nf.width = GST_VIDEO_FRAME_WIDTH(frame); nf.height = GST_VIDEO_FRAME_HEIGHT(frame);
    nf.stride = GST_VIDEO_FRAME_PLANE_STRIDE(frame, 0);
    nf.mem = NVCA_MEM_HOST; nf.pts = GST_BUFFER_PTS(frame->buffer);
    return nf;
}
// view-* outlines (element_output.cpp lists them): the library draws them on the mapped frame, in place, with the rasterisation
// rules nubovca.h states for nvca_draw_shapes (checked by tests/test_draw_cpu.py and tests/test_gpu_draw.py).  Host frames need
// no context, so outlines are drawn even where no GPU slot came up.
static void draw_outlines(GstVideoFrame *frame, const std::vector<nvca_shape> &shapes)
{
    if (shapes.empty()) return;
    const nvca_frame nf = frame_of(frame);
    nvca_draw_shapes(NULL, &nf, GST_VIDEO_FRAME_COMP_PSTRIDE(frame, 0), shapes.data(), (int)shapes.size());
}
// activate-events / events-ms: the string signal goes out at most once per events-ms (signal_due)
struct EventsThrottle { int server_events, events_ms; double last_ms; };
static void throttle_init(EventsThrottle &t) { t.server_events = 0; t.events_ms = 30001; t.last_ms = 0; }
static void emit_if_due(gpointer element, guint signal, EventsThrottle &t, int n, const std::string &payload)
{
    const double now = now_ms();
    if (!signal_due(n, t.server_events, now, t.last_ms, t.events_ms)) return;
    t.last_ms = now;
    g_signal_emit(element, signal, 0, payload.c_str());
}
static void push_event(gpointer element, ElementOutput &out)
{
    if (out.event) gst_pad_push_event(GST_BASE_TRANSFORM(element)->srcpad, gst_event_new_custom(GST_EVENT_CUSTOM_DOWNSTREAM, out.event.release()));
}
static void install_pads(gpointer klass, const char *caps_string)
{
    GstCaps *caps = gst_caps_from_string(caps_string);
    gst_element_class_add_pad_template(GST_ELEMENT_CLASS(klass), gst_pad_template_new("src", GST_PAD_SRC, GST_PAD_ALWAYS, caps));
    gst_element_class_add_pad_template(GST_ELEMENT_CLASS(klass), gst_pad_template_new("sink", GST_PAD_SINK, GST_PAD_ALWAYS, caps));
    gst_caps_unref(caps);
}
// NVCA_GST_STATS, at finalize: the largest round of the element's combiner
template <class Q> static void print_batch_stats(Q &q, const char *what, int slot)
{
    std::lock_guard<std::mutex> lk(q.m);
    fprintf(stderr, "nubovca: largest combined %s batch %d (slot %d)\n", what, q.max_batch, slot);
}
// Properties, for every family: each is an int -- prop_int(element, id, set) names the field a write or a read goes to -- but
// set_max_area (long) and image-to-overlay (boxed), which prop_other(element, id, value to set or NULL, value to fill) handles.
template <class E> static void set_property(GObject *o, guint id, const GValue *v, GParamSpec *ps)
try {
    E *e = (E *)o;
    NvcaRecLock nvca_lock_(&e->mutex);
    int *field = prop_int(e, id, true);
    if (field) *field = g_value_get_int(v);
    else if (!prop_other(e, id, v, NULL)) G_OBJECT_WARN_INVALID_PROPERTY_ID(o, id, ps);
    if (field == &e->events.server_events) e->events.last_ms = now_ms();
    sync_params(e);
}
NVCA_GST_CATCH_VOID(E::set_where)
template <class E> static void get_property(GObject *o, guint id, GValue *v, GParamSpec *ps)
try {
    E *e = (E *)o;
    NvcaRecLock nvca_lock_(&e->mutex);
    if (const int *field = prop_int(e, id, false)) g_value_set_int(v, *field);
    else if (!prop_other(e, id, NULL, v)) G_OBJECT_WARN_INVALID_PROPERTY_ID(o, id, ps);
}
NVCA_GST_CATCH_VOID(E::get_where)
// image-to-overlay: accepted and kept; overlay drawing is out of scope
static bool overlay_prop(GstStructure **held, const GValue *set, GValue *get)
{
    if (!set) { g_value_set_boxed(get, *held); return true; }
    if (*held) gst_structure_free(*held);
    *held = (GstStructure *)g_value_dup_boxed(set);
    return true;
}

// =====================================================================================
// nubofacedetector
// =====================================================================================
struct NvcaFace {
    GstVideoFilter base;
    GRecMutex mutex;
    GpuSlot *slot;                  /* the GPU this stream lives on (taken at the first frame) */
    nvca_cascade *cascade; nvca_face_stream *stream;
    nvca_face_params p;
    int view_faces, send_meta_data;
    EventsThrottle events;
    GQueue *events_queue;
    GstStructure *image_to_overlay;
    static constexpr const char *set_where = "nvca_face_set_property", *get_where = "nvca_face_get_property";
};
struct NvcaFaceClass { GstVideoFilterClass parent; };
G_DEFINE_TYPE(NvcaFace, nvca_face, GST_TYPE_VIDEO_FILTER)

enum { FP_0, FP_VIEW, FP_DETECT_EVENT, FP_META, FP_WIDTH, FP_X_EVERY_4, FP_EUCLID, FP_TRACK, FP_AREA, FP_SCALE, FP_EVENTS,
       FP_EVENTS_MS, FP_OVERLAY };
static guint face_signal = 0;

// the int behind a property, for a write (set) or a read
static int *prop_int(NvcaFace *f, guint id, bool set)
{
    switch (id) {
    case FP_VIEW: return &f->view_faces;
    case FP_DETECT_EVENT: return &f->p.detect_event;
    case FP_META: return &f->send_meta_data;
    case FP_X_EVERY_4: return &f->p.process_x_every_4;
    case FP_WIDTH: return &f->p.width_to_process;
    case FP_SCALE: return &f->p.scale_factor_pct;
    case FP_EUCLID: return &f->p.euclidean_threshold;
    case FP_TRACK: return set ? &f->p.euclidean_threshold : &f->p.track_threshold;   /* sic: FACE/kmsfacedetect.cpp:548-550 */
    case FP_AREA: return &f->p.area_threshold;
    case FP_EVENTS: return &f->events.server_events;
    case FP_EVENTS_MS: return &f->events.events_ms;
    }
    return NULL;
}
static bool prop_other(NvcaFace *f, guint id, const GValue *set, GValue *get) { return id == FP_OVERLAY && overlay_prop(&f->image_to_overlay, set, get); }
static void sync_params(NvcaFace *f) { if (f->stream) nvca_face_stream_set_params(f->stream, &f->p); }

static gboolean nvca_face_sink_event(GstBaseTransform *trans, GstEvent *event)
try {
    NvcaFace *f = (NvcaFace *)trans;
    if (GST_EVENT_TYPE(event) == GST_EVENT_CUSTOM_DOWNSTREAM) {
        const GstStructure *s = gst_event_get_structure(event);
        if (s) { GST_OBJECT_LOCK(f); g_queue_push_tail(f->events_queue, gst_structure_copy(s)); GST_OBJECT_UNLOCK(f); }
    }
    return GST_BASE_TRANSFORM_CLASS(nvca_face_parent_class)->sink_event(trans, event);
}
NVCA_GST_CATCH("nvca_face_sink_event", FALSE)

static void face_lazy_init(NvcaFace *f)
{
    if (f->stream) return;
    if (!f->slot) f->slot = take_slot();
    nvca_ctx *ctx = f->slot->ctx;
    if (!ctx) return;
    if (!need_cascade(f->slot, "haarcascade_frontalface_alt.xml", &f->cascade)) return;
    if (nvca_face_stream_create_any(ctx, f->cascade, &f->p, &f->stream) != NVCA_OK) f->stream = nullptr;
}

static GstFlowReturn nvca_face_transform_frame_ip(GstVideoFilter *filter, GstVideoFrame *frame)
try {
    NvcaFace *f = (NvcaFace *)filter;
    NvcaRecLock nvca_lock_(&f->mutex);
    face_lazy_init(f);
    if (f->stream && f->p.width_to_process > 0) {
        // upstream "motion" messages arm the detector when detect-event = 1
        GST_OBJECT_LOCK(f);
        while (GstStructure *m = (GstStructure *)g_queue_pop_head(f->events_queue)) {
            if (f->p.detect_event && message_has_motion(m)) nvca_face_stream_motion_event(f->stream);
            gst_structure_free(m);
        }
        GST_OBJECT_UNLOCK(f);
        note_frame_memory(f->slot, frame);
        nvca_rect boxes[kFaceCap];
        FaceReq req{f->stream, frame_of(frame), {boxes}, {0}, NVCA_OK, false};
        nvca_ctx *ctx = f->slot->ctx;
        const int rc = f->slot->face_q.process(&req, [ctx](std::vector<FaceReq *> &round) { run_round<FaceCalls>(ctx, round); });
        if (rc != NVCA_OK) GST_ERROR("nvca_face_stream_process: %d", rc);
        else {
            const int n = std::min(req.n[0], kFaceCap);
            ElementOutput out = face_output(boxes, n, req.frame.width, req.frame.pts, f->p.width_to_process, f->view_faces, f->image_to_overlay != NULL);
            push_event(f, out);
            draw_outlines(frame, out.shapes);
            emit_if_due(f, face_signal, f->events, n, out.payload);
        }
    }
    return GST_FLOW_OK;                                     /* always: FACE/kmsfacedetect.cpp:897 */
}
NVCA_GST_CATCH("nvca_face_transform_frame_ip", GST_FLOW_OK)

static void nvca_face_finalize(GObject *o)
try {
    NvcaFace *f = (NvcaFace *)o;
    if (getenv("NVCA_GST_STATS") && f->slot) {
        print_batch_stats(f->slot->face_q, "face", f->slot->index);
        fprintf(stderr, "nubovca: page-locked pool memories %d (slot %d)\n", f->slot->registered.load(), f->slot->index);
    }
    if (f->stream) nvca_face_stream_destroy(f->stream);
    if (f->cascade) release_cascade(f->slot, f->cascade);
    if (f->image_to_overlay) gst_structure_free(f->image_to_overlay);
    g_queue_free_full(f->events_queue, (GDestroyNotify)gst_structure_free);
    g_rec_mutex_clear(&f->mutex);
    G_OBJECT_CLASS(nvca_face_parent_class)->finalize(o);
}
NVCA_GST_CATCH_VOID("nvca_face_finalize")

static void nvca_face_init(NvcaFace *f)
try {
    nvca_face_params_default(&f->p);                        /* defaults of FACE/kmsfacedetect.cpp:979-999 */
    f->view_faces = 0; f->send_meta_data = 0;
    throttle_init(f->events);
    f->cascade = nullptr; f->stream = nullptr; f->image_to_overlay = nullptr;
    f->events_queue = g_queue_new();
    g_rec_mutex_init(&f->mutex);
}
NVCA_GST_CATCH_VOID("nvca_face_init")

#define INT_PROP(klass, id, name, nick, blurb, lo, hi) \
    g_object_class_install_property(klass, id, g_param_spec_int(name, nick, blurb, lo, hi, 0, (GParamFlags)G_PARAM_READWRITE))

static void nvca_face_class_init(NvcaFaceClass *klass)
{
    GObjectClass *go = G_OBJECT_CLASS(klass);
    GstVideoFilterClass *vf = GST_VIDEO_FILTER_CLASS(klass);
    install_pads(klass, GST_VIDEO_CAPS_MAKE("{ BGR }"));
    gst_element_class_set_static_metadata(GST_ELEMENT_CLASS(klass), "face detection filter element", "Video/Filter",
                                          "Haar face detector (MI355X / HIP implementation of NuboFaceDetector)", "nubovca-hip");
    go->set_property = set_property<NvcaFace>; go->get_property = get_property<NvcaFace>; go->finalize = nvca_face_finalize;
    INT_PROP(go, FP_VIEW, "view-faces", "view faces", "draw or hide the detected faces on the stream", 0, 1);
    INT_PROP(go, FP_DETECT_EVENT, "detect-event", "detect event", "0 => always; 1 => only after a motion event", 0, 1);
    INT_PROP(go, FP_META, "send-meta-data", "send meta data", "0 (default) => no meta data; 1 => send the face boxes as metadata", 0, 1);
    INT_PROP(go, FP_WIDTH, "width-to-process", "width to process", "width of the image the algorithm processes", 0, 640);
    INT_PROP(go, FP_X_EVERY_4, "process-x-every-4-frames", "process x every 4 frames", "1,2,3,4 (default)", 0, 4);
    INT_PROP(go, FP_EUCLID, "euclidean-distance", "euclidean distance", "0 - 20 (8 default)", 0, 20);
    INT_PROP(go, FP_TRACK, "track-threshold", "track threshold", "0 - 100 (30 default)", 0, 100);
    INT_PROP(go, FP_AREA, "area-threshold", "area threshold", "0 - 1000 (500 default)", 0, 1000);
    INT_PROP(go, FP_SCALE, "multi-scale-factor", "multi scale factor", "5-50 (25 default)", 0, 51);
    INT_PROP(go, FP_EVENTS, "activate-events", "Activate Events", "0 (default) => no events to the server; 1 => send events", 0, 1);
    INT_PROP(go, FP_EVENTS_MS, "events-ms", "Activate Events", "the time, it takes to send events to the servers", 0, 30000);
    g_object_class_install_property(go, FP_OVERLAY, g_param_spec_boxed("image-to-overlay", "image to overlay",
                                    "set the url of the image to overlay the faces", GST_TYPE_STRUCTURE,
                                    (GParamFlags)(G_PARAM_READWRITE | G_PARAM_STATIC_STRINGS)));
    vf->transform_frame_ip = GST_DEBUG_FUNCPTR(nvca_face_transform_frame_ip);
    GST_BASE_TRANSFORM_CLASS(klass)->sink_event = GST_DEBUG_FUNCPTR(nvca_face_sink_event);
    face_signal = g_signal_new("face-event", G_TYPE_FROM_CLASS(klass), G_SIGNAL_RUN_LAST, 0, NULL, NULL, NULL, G_TYPE_NONE, 1,
                               G_TYPE_STRING);
}

// =====================================================================================
// nubotracker
// =====================================================================================
struct NvcaTrk {
    GstVideoFilter base;
    GRecMutex mutex;
    GpuSlot *slot;
    nvca_tracker *trk;
    nvca_tracker_params p;
    int visual_mode;
    EventsThrottle events;
    static constexpr const char *set_where = "nvca_trk_set_property", *get_where = "nvca_trk_get_property";
};
struct NvcaTrkClass { GstVideoFilterClass parent; };
G_DEFINE_TYPE(NvcaTrk, nvca_trk, GST_TYPE_VIDEO_FILTER)
enum { TP_0, TP_THRESHOLD, TP_MIN_AREA, TP_MAX_AREA, TP_DISTANCE, TP_VISUAL, TP_EVENTS, TP_EVENTS_MS };
static guint trk_signal = 0;

static int *prop_int(NvcaTrk *t, guint id, bool)
{
    switch (id) {
    case TP_THRESHOLD: return &t->p.threshold;
    case TP_MIN_AREA: return &t->p.min_area;
    case TP_DISTANCE: return &t->p.distance;
    case TP_VISUAL: return &t->visual_mode;
    case TP_EVENTS: return &t->events.server_events;
    case TP_EVENTS_MS: return &t->events.events_ms;
    }
    return NULL;
}
static bool prop_other(NvcaTrk *t, guint id, const GValue *set, GValue *get)
{
    if (id != TP_MAX_AREA) return false;
    if (set) t->p.max_area = g_value_get_long(set); else g_value_set_long(get, t->p.max_area);
    return true;
}
static void sync_params(NvcaTrk *t) { if (t->trk) nvca_tracker_set_params(t->trk, &t->p); }

static GstFlowReturn nvca_trk_transform_frame_ip(GstVideoFilter *filter, GstVideoFrame *frame)
try {
    NvcaTrk *t = (NvcaTrk *)filter;
    NvcaRecLock nvca_lock_(&t->mutex);
    if (!t->trk) { if (!t->slot) t->slot = take_slot(); nvca_ctx *ctx = t->slot->ctx; if (ctx && nvca_tracker_create(ctx, &t->p, &t->trk) != NVCA_OK) t->trk = nullptr; }
    if (t->trk) {
        note_frame_memory(t->slot, frame);
        const double timestamp = 1000.0 * clock() / CLOCKS_PER_SEC;          /* TRK/gstnubotracker.cpp:349 */
        const std::unique_ptr<nvca_rect[]> bx(new nvca_rect[kTrkCap]);
        TrkReq req{{t->trk, frame_of(frame), {bx.get()}, {0}, NVCA_OK, false}, timestamp};
        nvca_ctx *ctx = t->slot->ctx;
        const int rc = t->slot->trk_q.process(&req, [ctx](std::vector<TrkReq *> &round) { run_round<TrkCalls>(ctx, round); });
        if (rc != NVCA_OK) GST_ERROR("nvca_tracker_process: %d", rc);
        else {
            const int n = std::min(req.n[0], kTrkCap);
            const ElementOutput out = tracker_output(bx.get(), n, t->visual_mode);
            draw_outlines(frame, out.shapes);
            emit_if_due(t, trk_signal, t->events, n, out.payload);
        }
    }
    return GST_FLOW_OK;
}
NVCA_GST_CATCH("nvca_trk_transform_frame_ip", GST_FLOW_OK)

static void nvca_trk_finalize(GObject *o)
try {
    NvcaTrk *t = (NvcaTrk *)o;
    if (getenv("NVCA_GST_STATS") && t->slot) print_batch_stats(t->slot->trk_q, "tracker", t->slot->index);
    if (t->trk) nvca_tracker_destroy(t->trk);
    g_rec_mutex_clear(&t->mutex);
    G_OBJECT_CLASS(nvca_trk_parent_class)->finalize(o);
}
NVCA_GST_CATCH_VOID("nvca_trk_finalize")
static void nvca_trk_init(NvcaTrk *t)
try {
    nvca_tracker_params_default(&t->p);                     /* TRK/gstnubotracker.cpp:457-466 */
    t->visual_mode = 0; t->trk = nullptr;
    throttle_init(t->events);
    g_rec_mutex_init(&t->mutex);
}
NVCA_GST_CATCH_VOID("nvca_trk_init")
static void nvca_trk_class_init(NvcaTrkClass *klass)
{
    GObjectClass *go = G_OBJECT_CLASS(klass);
    install_pads(klass, GST_VIDEO_CAPS_MAKE("{ BGRA }"));
    gst_element_class_set_static_metadata(GST_ELEMENT_CLASS(klass), "motion tracker filter element", "Video/Filter",
                                          "Motion-history tracker (MI355X / HIP implementation of NuboTracker)", "nubovca-hip");
    go->set_property = set_property<NvcaTrk>; go->get_property = get_property<NvcaTrk>; go->finalize = nvca_trk_finalize;
    INT_PROP(go, TP_THRESHOLD, "set_threshold", "threshold", "motion threshold (20 default)", 0, 255);
    INT_PROP(go, TP_MIN_AREA, "set_min_area", "min area", "minimum object area (50 default)", 0, 10000);
    g_object_class_install_property(go, TP_MAX_AREA, g_param_spec_long("set_max_area", "max area", "maximum object area (30000 default)",
                                                                       0, 300000, 0, (GParamFlags)G_PARAM_READWRITE));
    INT_PROP(go, TP_DISTANCE, "set_distance", "distance", "merge distance (35 default)", 0, 2000);
    INT_PROP(go, TP_VISUAL, "set_visual_mode", "visual mode", "draw the objects (0 default)", 0, 4);
    INT_PROP(go, TP_EVENTS, "activate-events", "Activate Events", "0 (default) => no events to the server", 0, 1);
    INT_PROP(go, TP_EVENTS_MS, "events-ms", "Activate Events", "the time, it takes to send events to the servers", 0, 30000);
    GST_VIDEO_FILTER_CLASS(klass)->transform_frame_ip = GST_DEBUG_FUNCPTR(nvca_trk_transform_frame_ip);
    trk_signal = g_signal_new("tracker-event", G_TYPE_FROM_CLASS(klass), G_SIGNAL_RUN_LAST, 0, NULL, NULL, NULL, G_TYPE_NONE, 1,
                              G_TYPE_STRING);
}

// =====================================================================================
// nuboeyedetector / nubonosedetector / nubomouthdetector / nuboeardetector  (one implementation, four GTypes)
// =====================================================================================
struct PartDesc {
    int kind; const char *factory, *type_name, *view_prop, *meta_prop, *signal, *face_file, *a_file, *b_file, *longname;
    guint signal_id; gpointer parent_class;
};
static PartDesc part_descs[4] = {
    {NVCA_PART_EYE, "nuboeyedetector", "NvcaEyeDetect", "view-eyes", "send-meta-data", "eye-event", "haarcascade_frontalface_alt.xml",
     "haarcascade_mcs_righteye.xml", "haarcascade_mcs_lefteye.xml", "eye detection filter element", 0, NULL},
    {NVCA_PART_NOSE, "nubonosedetector", "NvcaNoseDetect", "view-noses", "send-meta-data", "nose-event", "haarcascade_frontalface_alt.xml",
     "haarcascade_mcs_nose.xml", NULL, "nose detection filter element", 0, NULL},
    {NVCA_PART_MOUTH, "nubomouthdetector", "NvcaMouthDetect", "view-mouths", "send-meta-data", "mouth-event", "haarcascade_frontalface_alt.xml",
     "haarcascade_mcs_mouth.xml", NULL, "mouth detection filter element", 0, NULL},
    /* EAR: LEFT_SIDE uses mcs_rightear.xml, RIGHT_SIDE mcs_leftear.xml (sic, EAR/kmseardetect.cpp:29-31,796,801); property "meta-data" */
    {NVCA_PART_EAR, "nuboeardetector", "NvcaEarDetect", "view-ears", "meta-data", "ear-event", "haarcascade_profileface.xml",
     "haarcascade_mcs_rightear.xml", "haarcascade_mcs_leftear.xml", "ear detection filter element", 0, NULL},
};
struct NvcaPart {
    GstVideoFilter base;
    GRecMutex mutex;
    PartDesc *desc;
    GpuSlot *slot;
    nvca_cascade *cf, *ca, *cb; nvca_part_stream *stream;
    nvca_part_params p;
    int view, meta_data;
    EventsThrottle events;
    GstStructure *image_to_overlay;
    static constexpr const char *set_where = "nvca_part_set_property", *get_where = "nvca_part_get_property";
};
struct NvcaPartClass { GstVideoFilterClass parent; PartDesc *desc; };
enum { PP_0, PP_VIEW, PP_DETECT_EVENT, PP_META, PP_WIDTH, PP_X_EVERY_4, PP_SCALE, PP_EVENTS, PP_EVENTS_MS, PP_OVERLAY };

static int *prop_int(NvcaPart *f, guint id, bool)
{
    switch (id) {
    case PP_VIEW: return &f->view;
    case PP_DETECT_EVENT: return &f->p.detect_event;
    case PP_META: return &f->meta_data;
    case PP_WIDTH: return &f->p.width_to_process;
    case PP_X_EVERY_4: return &f->p.process_x_every_4;
    case PP_SCALE: return &f->p.scale_factor_pct;
    case PP_EVENTS: return &f->events.server_events;
    case PP_EVENTS_MS: return &f->events.events_ms;
    }
    return NULL;
}
static bool prop_other(NvcaPart *f, guint id, const GValue *set, GValue *get) { return id == PP_OVERLAY && overlay_prop(&f->image_to_overlay, set, get); }
static void sync_params(NvcaPart *f) { if (f->stream) nvca_part_stream_set_params(f->stream, &f->p); }

static void part_lazy_init(NvcaPart *f)
{
    if (f->stream) return;
    if (!f->slot) f->slot = take_slot();
    nvca_ctx *ctx = f->slot->ctx;
    if (!ctx) return;
    const PartDesc *d = f->desc;
    if (!need_cascade(f->slot, d->face_file, &f->cf) || !need_cascade(f->slot, d->a_file, &f->ca) || !need_cascade(f->slot, d->b_file, &f->cb)) return;
    if (nvca_part_stream_create_any(ctx, &f->p, f->cf, f->ca, f->cb, &f->stream) != NVCA_OK) f->stream = nullptr;
}

// faces handed over by an upstream element (message_faces)
static gboolean nvca_part_sink_event(GstBaseTransform *trans, GstEvent *event)
try {
    NvcaPart *f = (NvcaPart *)trans;
    if (GST_EVENT_TYPE(event) == GST_EVENT_CUSTOM_DOWNSTREAM && f->desc->kind != NVCA_PART_EAR) {
        const GstStructure *m = gst_event_get_structure(event);
        NvcaRecLock nvca_lock_(&f->mutex);
        if (m && f->p.detect_event) {
            part_lazy_init(f);
            nvca_rect faces[kPartCap];
            const int n = message_faces(m, faces, kPartCap);
            if (f->stream) nvca_part_stream_push_faces(f->stream, faces, n);
        }
    }
    return GST_BASE_TRANSFORM_CLASS(f->desc->parent_class)->sink_event(trans, event);
}
NVCA_GST_CATCH("nvca_part_sink_event", FALSE)

static GstFlowReturn nvca_part_transform_frame_ip(GstVideoFilter *filter, GstVideoFrame *frame)
try {
    NvcaPart *f = (NvcaPart *)filter;
    NvcaRecLock nvca_lock_(&f->mutex);
    part_lazy_init(f);
    if (f->stream && f->p.width_to_process > 0) {
        note_frame_memory(f->slot, frame);
        nvca_rect a[kPartCap], b[kPartCap], faces[kPartCap];
        // part detectors of other streams (and other kinds) that arrive meanwhile share the call: nvca_part_batch_process
        PartReq req{f->stream, frame_of(frame), {a, b}, {0, 0}, NVCA_OK, false};
        nvca_ctx *ctx = f->slot->ctx;
        const int rc = f->slot->part_q.process(&req, [ctx](std::vector<PartReq *> &round) { run_round<PartCalls>(ctx, round); });
        if (rc != NVCA_OK) GST_ERROR("nvca_part_stream_process: %d", rc);
        else {
            const int na = std::min(req.n[0], kPartCap), nb = std::min(req.n[1], kPartCap);
            int nfaces = 0;
            nvca_part_stream_faces(f->stream, faces, kPartCap, &nfaces);
            ElementOutput out = part_output(f->desc->kind, a, na, b, nb, faces, std::min(nfaces, kPartCap), req.frame.width, req.frame.pts,
                                            f->p.detect_event, f->view, f->image_to_overlay != NULL);
            draw_outlines(frame, out.shapes);
            push_event(f, out);
            emit_if_due(f, f->desc->signal_id, f->events, na + nb, out.payload);
        }
    }
    return GST_FLOW_OK;
}
NVCA_GST_CATCH("nvca_part_transform_frame_ip", GST_FLOW_OK)

static void nvca_part_finalize(GObject *o)
try {
    NvcaPart *f = (NvcaPart *)o;
    if (getenv("NVCA_GST_STATS") && f->slot) print_batch_stats(f->slot->part_q, "part-detector", f->slot->index);
    if (f->stream) nvca_part_stream_destroy(f->stream);
    if (f->cf) release_cascade(f->slot, f->cf);
    if (f->ca) release_cascade(f->slot, f->ca);
    if (f->cb) release_cascade(f->slot, f->cb);
    if (f->image_to_overlay) gst_structure_free(f->image_to_overlay);
    g_rec_mutex_clear(&f->mutex);
    G_OBJECT_CLASS(f->desc->parent_class)->finalize(o);
}
NVCA_GST_CATCH_VOID("nvca_part_finalize")
static void nvca_part_instance_init(GTypeInstance *inst, gpointer klass)
try {
    NvcaPart *f = (NvcaPart *)inst;
    f->desc = ((NvcaPartClass *)klass)->desc;
    nvca_part_params_default(&f->p, f->desc->kind);      /* width-to-process 320, process 4 of 4, scale factor 25 */
    f->view = 0; f->meta_data = 0;
    throttle_init(f->events);
    f->cf = f->ca = f->cb = nullptr; f->stream = nullptr; f->image_to_overlay = nullptr;
    g_rec_mutex_init(&f->mutex);
}
NVCA_GST_CATCH_VOID("nvca_part_instance_init")
static void nvca_part_class_init(gpointer klass, gpointer class_data)
{
    PartDesc *d = (PartDesc *)class_data;
    ((NvcaPartClass *)klass)->desc = d;
    d->parent_class = g_type_class_peek_parent(klass);
    GObjectClass *go = G_OBJECT_CLASS(klass);
    install_pads(klass, GST_VIDEO_CAPS_MAKE("{ BGR }"));
    gst_element_class_set_static_metadata(GST_ELEMENT_CLASS(klass), d->longname, "Video/Filter",
                                          "Haar part detector (MI355X / HIP implementation)", "nubovca-hip");
    go->set_property = set_property<NvcaPart>; go->get_property = get_property<NvcaPart>; go->finalize = nvca_part_finalize;
    INT_PROP(go, PP_VIEW, d->view_prop, "view", "draw or hide the detections on the stream", 0, 1);
    INT_PROP(go, PP_DETECT_EVENT, "detect-event", "detect event", "0 => own face pass; 1 => faces come from upstream events", 0, 1);
    INT_PROP(go, PP_META, d->meta_prop, "send meta data", "0 (default) => no meta data", 0, 1);
    INT_PROP(go, PP_WIDTH, "width-to-process", "width to process", "width of the image the part cascade processes (320 default)", 0, 640);
    INT_PROP(go, PP_X_EVERY_4, "process-x-every-4-frames", "process x every 4 frames", "1,2,3,4 (default)", 0, 4);
    INT_PROP(go, PP_SCALE, "multi-scale-factor", "multi scale factor", "5-50 (25 default)", 0, 51);
    INT_PROP(go, PP_EVENTS, "activate-events", "Activate Events", "0 (default) => no events to the server", 0, 1);
    INT_PROP(go, PP_EVENTS_MS, "events-ms", "Activate Events", "the time, it takes to send events to the servers", 0, 30000);
    g_object_class_install_property(go, PP_OVERLAY, g_param_spec_boxed("image-to-overlay", "image to overlay", "set the url of the image to overlay",
                                    GST_TYPE_STRUCTURE, (GParamFlags)(G_PARAM_READWRITE | G_PARAM_STATIC_STRINGS)));
    GST_VIDEO_FILTER_CLASS(klass)->transform_frame_ip = GST_DEBUG_FUNCPTR(nvca_part_transform_frame_ip);
    if (d->kind != NVCA_PART_EAR) GST_BASE_TRANSFORM_CLASS(klass)->sink_event = GST_DEBUG_FUNCPTR(nvca_part_sink_event);   /* ear: not overridden */
    d->signal_id = g_signal_new(d->signal, G_TYPE_FROM_CLASS(klass), G_SIGNAL_RUN_LAST, 0, NULL, NULL, NULL, G_TYPE_NONE, 1, G_TYPE_STRING);
}
static GType nvca_part_type(PartDesc *d)
{
    GTypeInfo info; memset(&info, 0, sizeof(info));
    info.class_size = sizeof(NvcaPartClass); info.class_init = nvca_part_class_init; info.class_data = d;
    info.instance_size = sizeof(NvcaPart); info.instance_init = nvca_part_instance_init;
    return g_type_register_static(GST_TYPE_VIDEO_FILTER, d->type_name, &info, (GTypeFlags)0);
}

// =====================================================================================
static void debug_category_once()
{
    static gsize once = 0;
    if (g_once_init_enter(&once)) {
        GST_DEBUG_CATEGORY_INIT(nubovca_debug, "nubovca", 0, "NUBOMEDIA-VCA Haar path on MI355X");
        g_once_init_leave(&once, 1);
    }
}
// One element under a plugin of its own: the reference ships six plugins (libnubofacedetector.so with plugin name
// nubofacedetector, libnuboeyedetector.so / eyefilter, libnubonosedetector.so / nubonosedetector, libnubomouthdetector.so /
// nubomouthdetector, libnuboeardetector.so / earfilter, libnubotracker.so / nubotracker -- modules/nubo_*/.../src/gst-plugins/
// nubo*.c, GST_PLUGIN_DEFINE), and deployments that name them (GST_PLUGIN_PATH entries, `gst-inspect-1.0 <plugin>`, registry
// checks) find the same six here: gst_reference_names/lib<name>.so are stubs (plugin_alias.cpp) that register their element
// through this entry point.  The element types, the batching state and the contexts live in THIS library once, whichever plugin
// registered the factory: branches of different elements are still combined into batched calls.
extern "C" __attribute__((visibility("default"))) gboolean nvca_gst_register_element(GstPlugin *plugin, const char *factory)
{
    debug_category_once();
    if (!plugin || !factory) return FALSE;
    if (!strcmp(factory, "nubofacedetector")) return gst_element_register(plugin, factory, GST_RANK_NONE, nvca_face_get_type());
    if (!strcmp(factory, "nubotracker")) return gst_element_register(plugin, factory, GST_RANK_NONE, nvca_trk_get_type());
    for (PartDesc &d : part_descs)
        if (!strcmp(factory, d.factory)) return gst_element_register(plugin, factory, GST_RANK_NONE, nvca_part_type(&d));
    return FALSE;
}

static gboolean plugin_init(GstPlugin *plugin)
{
    gboolean ok = nvca_gst_register_element(plugin, "nubofacedetector") && nvca_gst_register_element(plugin, "nubotracker");
    for (PartDesc &d : part_descs) ok = ok && nvca_gst_register_element(plugin, d.factory);
    return ok;
}

#ifndef PACKAGE
#define PACKAGE "nubovca"
#endif
GST_PLUGIN_DEFINE(GST_VERSION_MAJOR, GST_VERSION_MINOR, nubovca, "NUBOMEDIA-VCA detection filters on MI355X (HIP)", plugin_init,
                  "0.1", "LGPL", "nubovca-hip", "https://github.com/nubomedia/NUBOMEDIA-VCA")
