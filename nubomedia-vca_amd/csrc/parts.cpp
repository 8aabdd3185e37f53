// parts.cpp -- NuboEyeDetector / NuboNoseDetector / NuboMouthDetector / NuboEarDetector stream objects: the nvca_part_* entry
// points and the rules of the two tickets (slot, submit order, refusals, abandon).  The per-frame state machine of the elements is
// part_logic.cpp (pure host code), a batched call's two halves are part_call.cpp, its working images part_images.cpp.
#include "part_call.h"
#include <algorithm>

using namespace nvca;

namespace nvca {
// outstanding calls that hold stream s (nullptr: any) are given up: rolled back (newest first), drained, deleted
void part_calls_abandon(nvca_ctx *ctx, const nvca_part_stream *s)
{
    bool hit = false;
    for (const PartCall *c : ctx->part_calls)
        if (c && (!s || c->holds(s))) hit = true;
    if (!hit) return;
    // (both go: the newer call's gates were taken on top of the older one's)
    PartCall *a = ctx->part_calls[0], *b = ctx->part_calls[1];
    if (a && b && a->seq > b->seq) std::swap(a, b);          // a: older, b: newer
    ctx->part_calls[0] = ctx->part_calls[1] = nullptr;
    delete b;
    delete a;
}
} // namespace nvca

namespace {
// the slot of the next call, or -1 when two are in flight
int part_call_slot(nvca_ctx *ctx)
{
    const int parity = ctx->part_seq & 1;
    return ctx->part_calls[parity] ? -1 : parity;
}
} // namespace

namespace {
// what both create calls check and make; any_format: a role may be a new-format LBP cascade
int part_stream_make(nvca_ctx *ctx, const nvca_part_params *params, const nvca_cascade *face, const nvca_cascade *a, const nvca_cascade *b,
                     bool any_format, nvca_part_stream **out)
{
    if (!ctx || !params || !face || !a || !out || params->kind < NVCA_PART_EYE || params->kind > NVCA_PART_EAR) return NVCA_ERR_ARG;
    if ((params->kind == NVCA_PART_EYE || params->kind == NVCA_PART_EAR) && !b) return NVCA_ERR_ARG;
    if (!any_format && (face->format != NVCA_CASCADE_HAAR || a->format != NVCA_CASCADE_HAAR || (b && b->format != NVCA_CASCADE_HAAR))) {
        ctx->set_error("nvca_part_stream_create does not take an LBP cascade in any role (nvca_part_stream_create_any does)"); return NVCA_ERR_UNSUPPORTED;
    }
    nvca_part_stream *s = new (std::nothrow) nvca_part_stream();
    if (!s) return NVCA_ERR_NOMEM;
    s->ctx = ctx; s->p = *params; s->face = face; s->a = a; s->b = b;
    *out = s;
    return NVCA_OK;
}
} // namespace

extern "C" {

void nvca_part_params_default(nvca_part_params *p, int kind)
try {
    if (!p) return;
    p->kind = kind; p->width_to_process = 320; p->process_x_every_4 = 4; p->scale_factor_pct = 25; p->detect_event = 0;
}
NVCA_API_CATCH_VOID

int nvca_part_stream_create(nvca_ctx *ctx, const nvca_part_params *params, const nvca_cascade *face, const nvca_cascade *a,
                            const nvca_cascade *b, nvca_part_stream **out)
try {
    return part_stream_make(ctx, params, face, a, b, false, out);
}
NVCA_API_CATCH(ctx)
int nvca_part_stream_create_any(nvca_ctx *ctx, const nvca_part_params *params, const nvca_cascade *face, const nvca_cascade *a,
                                const nvca_cascade *b, nvca_part_stream **out)
try {
    return part_stream_make(ctx, params, face, a, b, true, out);
}
NVCA_API_CATCH(ctx)
void nvca_part_stream_destroy(nvca_part_stream *s)
try {
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    {
        // a submitted, not yet collected batch holds this stream (its gates' snapshot, its jobs): such calls are abandoned first --
        // the newer one before the older one, each rolled back and drained -- and their tickets become unknown
        std::lock_guard<std::recursive_mutex> lk(s->ctx->mu);
        part_calls_abandon(s->ctx, s);
    }
    (void)hipStreamSynchronize(s->ctx->stream);
    delete s;
}
NVCA_API_CATCH_VOID
int nvca_part_stream_set_params(nvca_part_stream *s, const nvca_part_params *params)
try {
    if (!s || !params || params->kind != s->p.kind) return NVCA_ERR_ARG;
    s->p = *params;
    return NVCA_OK;
}
NVCA_API_CATCH((s ? s->ctx : nullptr))
int nvca_part_stream_set_input(nvca_part_stream *s, const nvca_pixel_layout *layout)
try {
    if (!s) return NVCA_ERR_ARG;
    nvca_pixel_layout in{};
    if (int rc = parse_pixel_layout(s->ctx, layout, in)) return rc;
    s->input = in;                    // a submitted call keeps the layout it was submitted with (its frame groups hold it)
    return NVCA_OK;
}
NVCA_API_CATCH((s ? s->ctx : nullptr))
int nvca_part_stream_push_faces(nvca_part_stream *s, const nvca_rect *faces, int n)
try {
    if (!s || n < 0 || (n > 0 && !faces)) return NVCA_ERR_ARG;
    s->st.push_faces(faces, n);
    return NVCA_OK;
}
NVCA_API_CATCH((s ? s->ctx : nullptr))

int nvca_part_stream_faces(const nvca_part_stream *s, nvca_rect *out, int cap, int *n_out)
try {
    if (!s || !n_out || cap < 0 || (cap > 0 && !out)) return NVCA_ERR_ARG;
    *n_out = (int)s->st.faces.size();
    for (int i = 0; i < std::min(*n_out, cap); i++) out[i] = s->st.faces[i];
    return NVCA_OK;
}
NVCA_API_CATCH((s ? s->ctx : nullptr))

} // extern "C"

extern "C" {

// One transform_frame_ip of every stream of the batch.  The streams' device work is queued together and waited for three
// times per call, however many streams there are: (1) the working images of all frames (a launch set per image size) and the
// face passes (an N-image job per kind of pass), (2) every part search in every face's region (FIND_BIGGEST searches that
// narrow their scan take one more round), (3) nothing -- the merging heuristics that follow are host code on the collected boxes.
int nvca_part_batch_process(nvca_ctx *ctx, int n, nvca_part_stream *const *streams, const nvca_frame *frames, nvca_rect *out_a, int cap_a,
                            int *n_a, nvca_rect *out_b, int cap_b, int *n_b)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (n < 0 || (n > 0 && (!streams || !frames || !n_a || !n_b)) || cap_a < 0 || cap_b < 0 || (cap_a > 0 && !out_a) || (cap_b > 0 && !out_b)) return NVCA_ERR_ARG;
    const int slot = part_call_slot(ctx);
    if (slot < 0) { ctx->set_error("two part batches are in flight: collect one first"); return NVCA_ERR_ARG; }
    // a stream of an outstanding ticket would have its back halves run out of order (this call's before the ticket's): refused
    for (const PartCall *o : ctx->part_calls)
        if (o)
            for (int i = 0; i < n; i++)
                if (o->holds(streams[i])) { ctx->set_error("part stream has a submitted batch outstanding: collect it first"); return NVCA_ERR_ARG; }
    PartCall call; call.parity = slot;
    int rc = part_front(ctx, call, n, streams, frames);
    if (!rc) rc = part_back(ctx, call, out_a, cap_a, n_a, out_b, cap_b, n_b);
    return rc;
}
NVCA_API_CATCH(ctx)

// The same call in two halves (see part_front / part_back).  submit: gates, working images and face passes are queued, *ticket names
// the call; the frames must stay valid until the ticket is collected.  collect: the oldest outstanding ticket only (the streams' state
// machines advance in submit order).  At most two tickets are outstanding.  A failed collect rolls its streams back as a failed
// nvca_part_batch_process does -- and abandons a newer outstanding ticket with it (that ticket's streams are rolled back first).
int nvca_part_batch_submit(nvca_ctx *ctx, int n, nvca_part_stream *const *streams, const nvca_frame *frames, int *ticket)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (!ticket) return NVCA_ERR_ARG;
    const int slot = part_call_slot(ctx);
    if (slot < 0) { ctx->set_error("two part batches are in flight: collect one first"); return NVCA_ERR_ARG; }
    // a stream may not sit in two outstanding calls whose order the library cannot see: it may (tick k, tick k + 1), in submit order
    std::unique_ptr<PartCall> call(new PartCall());
    call->parity = slot; call->seq = ctx->part_seq;
    const int rc = part_front(ctx, *call, n, streams, frames);
    if (rc) return rc;                                   // (~PartCall rolls the gates back)
    ctx->part_calls[slot] = call.release();
    *ticket = ctx->part_seq++;
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)
int nvca_part_batch_collect(nvca_ctx *ctx, int ticket, nvca_rect *out_a, int cap_a, int *n_a, nvca_rect *out_b, int cap_b, int *n_b)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    const int slot = ticket & 1, other = slot ^ 1;
    PartCall *call = ticket >= 0 ? ctx->part_calls[slot] : nullptr;
    if (!call || call->seq != ticket) { ctx->set_error("unknown part-batch ticket"); return NVCA_ERR_ARG; }
    PartCall *newer = ctx->part_calls[other];
    if (newer && newer->seq < ticket) { ctx->set_error("part-batch tickets are collected in submit order"); return NVCA_ERR_ARG; }
    const int rc = part_back(ctx, *call, out_a, cap_a, n_a, out_b, cap_b, n_b);
    if (rc && rc != NVCA_ERR_ARG) {                      // (bad output arguments: the ticket stays collectable)
        if (newer) { ctx->part_calls[other] = nullptr; delete newer; }       // its gates were taken on top of this call's: back first
        ctx->part_calls[slot] = nullptr; delete call;
        return rc;
    }
    if (rc) return rc;
    ctx->part_calls[slot] = nullptr; delete call;
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)

int nvca_part_stream_process(nvca_part_stream *s, const nvca_frame *f, nvca_rect *out_a, int cap_a, int *n_a, nvca_rect *out_b,
                             int cap_b, int *n_b)
try {
    if (!s || !f) return NVCA_ERR_ARG;
    nvca_part_stream *arr[1] = {s};
    return nvca_part_batch_process(s->ctx, 1, arr, f, out_a, cap_a, n_a, out_b, cap_b, n_b);
}
NVCA_API_CATCH((s ? s->ctx : nullptr))

} // extern "C"
