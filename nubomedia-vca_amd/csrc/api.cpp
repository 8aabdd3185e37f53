// api.cpp -- C ABI of libnubovca_hip (include/nubovca.h): the context and its options, kernel timing, caller memory
// registration and the cascade entry points.  The other entry points: imgproc.cpp, detect.cpp, face_stream.cpp, parts.cpp,
// tracker.cpp.
#include "host_state.h"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <new>

using namespace nvca;

// =========================================================================
// context
// =========================================================================
nvca_ctx::nvca_ctx() {}
nvca_ctx::~nvca_ctx()
{
    plans.clear();
    nvca::free_scale_tables(this);
    if (ws) ws->release_all();
    trk.release_all();
    nvca::part_calls_abandon(this, nullptr);                   // submitted, never collected: rolled back (newest first), drained
    for (nvca::PartWorkspace &w : part_sets) w.release_all();
    if (identity_lut) (void)hipFree(identity_lut);
    bounce.release();
    nvca::work_pool_destroy(pool); pool = nullptr;
    overlay_img.release();
    for (auto &kv : roi_stage_recs) { kv.second->release(); delete kv.second; }
    for (RoiBuffers &b : roi_bufs) { b.tables.release(); b.hits.release(); b.h_tables.release(); b.h_hits.release(); }
    for (auto e : timer.pool) (void)hipEventDestroy(e);
    for (auto &e : timer.pending) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (nvca::FaceTicket *&t : face_tickets) { nvca::free_face_ticket(t); t = nullptr; }
    for (hipEvent_t e : chunk_events) (void)hipEventDestroy(e);
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    for (int l = 1; l < nvca::kLanes; l++) if (lane_streams[l]) (void)hipStreamDestroy(lane_streams[l]);
    if (stream) (void)hipStreamDestroy(stream);
}

extern "C" {

const char *nvca_version(void) { return "nubovca-hip 0.1 (gfx950)"; }

int nvca_device_count(int *n)
try {
    if (!n) return NVCA_ERR_ARG;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || c <= 0) { *n = 0; return NVCA_ERR_NO_DEVICE; }
    *n = c;
    return NVCA_OK;
}
NVCA_API_CATCH(nullptr)

int nvca_ctx_create(int device_id, nvca_ctx **out)
try {
    if (!out) return NVCA_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return NVCA_ERR_NO_DEVICE;   // no CPU fallback
    if (device_id < 0 || device_id >= n) return NVCA_ERR_NO_DEVICE;
    if (hipSetDevice(device_id) != hipSuccess) return NVCA_ERR_HIP;
    nvca_ctx *ctx = new (std::nothrow) nvca_ctx();
    if (!ctx) return NVCA_ERR_NOMEM;
    ctx->sw = switches();                                   // the environment is read here, once per process
    ctx->device = device_id;
    ctx->ws.reset(new Workspace());
    ctx->ws->cur_lane = &ctx->cur_lane;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return NVCA_ERR_HIP; }
    ctx->lane_streams[0] = ctx->stream;
    for (int l = 1; l < kLanes; l++)
        if (hipStreamCreateWithFlags(&ctx->lane_streams[l], hipStreamNonBlocking) != hipSuccess) { delete ctx; return NVCA_ERR_HIP; }
    *out = ctx;
    return NVCA_OK;
}
NVCA_API_CATCH(nullptr)

void nvca_ctx_destroy(nvca_ctx *ctx)
try {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    delete ctx;
}
NVCA_API_CATCH_VOID

const char *nvca_last_error(const nvca_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int nvca_ctx_set_hit_capacity(nvca_ctx *ctx, int cap)
try {
    if (!ctx || cap < 1 || cap > kMaxHitCap) return NVCA_ERR_ARG;
    ctx->hit_cap = cap;
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)
// One of the A/B switches of DESIGN.md's appendix, for this context (the environment variable of the same name, without
// the NVCA_ prefix and in lower case, sets the process default).  Switches that shape plans drop the context's cached plans.
int nvca_ctx_set_option(nvca_ctx *ctx, const char *name, int value)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (!name) return NVCA_ERR_ARG;
    bool replan = false;
    if (!option_set(ctx->sw, name, value, &replan)) { ctx->set_error(std::string("unknown option: ") + name); return NVCA_ERR_ARG; }
    if (!strcmp(name, "host_threads")) { work_pool_destroy(ctx->pool); ctx->pool = nullptr; ctx->pool_tried = false; }     // the pool is rebuilt at its next use
    if (replan) {
        for (auto &kv : ctx->plans) if (kv.second->inflight) { ctx->set_error("a batch is in flight: collect it before changing a plan option"); return NVCA_ERR_ARG; }
        (void)hipSetDevice(ctx->device);
        NVCA_HIP_CHECK(ctx, hipDeviceSynchronize());
        ctx->plans.clear();
    }
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)
// the value a switch holds for this context right now (what the environment or an earlier nvca_ctx_set_option left)
int nvca_ctx_get_option(nvca_ctx *ctx, const char *name, int *value)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (!name || !value) return NVCA_ERR_ARG;
    if (!option_get(ctx->sw, name, value)) { ctx->set_error(std::string("unknown option: ") + name); return NVCA_ERR_ARG; }
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)
int nvca_ctx_set_sum_policy(nvca_ctx *ctx, int policy)
try {
    if (!ctx || (policy != NVCA_SUM_F32PAIR && policy != NVCA_SUM_F64)) return NVCA_ERR_ARG;
    ctx->policy = policy;
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)
int nvca_ctx_synchronize(nvca_ctx *ctx)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (!ctx) return NVCA_ERR_ARG;
    NVCA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->cs()));
    NVCA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->lane_streams[kFaceLane2]));      // a submitted batch may run there
    NVCA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->lane_streams[kTrackerLane]));
#ifdef NVCA_STAMPS
    if (ctx->stamps && switches().stamps_out) {
        std::vector<unsigned long long> h(64 * 16 * 64);
        (void)hipMemcpy(h.data(), ctx->stamps, h.size() * 8, hipMemcpyDeviceToHost);
        if (FILE *f = fopen(switches().stamps_out, "wb")) { fwrite(h.data(), 8, h.size(), f); fclose(f); }
    }
    if (switches().stamps_out) roi_stamps_dump((std::string(switches().stamps_out) + ".roi.txt").c_str());
#endif
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)
void *nvca_ctx_stream(nvca_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int nvca_host_register(nvca_ctx *ctx, void *ptr, size_t bytes)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (!ptr || !bytes) return NVCA_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    if (ctx->host_ranges.covering(ptr, 1) >= 0 || !ctx->host_ranges.add(ptr, bytes)) { ctx->set_error("nvca_host_register: the range overlaps one that is registered"); return NVCA_ERR_ARG; }
    const hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterDefault);
    if (e != hipSuccess) {
        bool found; (void)ctx->host_ranges.remove(ptr, &found); ctx->host_ranges.retired.pop_back();       // never was
        ctx->set_error(std::string("hipHostRegister: ") + hipGetErrorString(e));
        return NVCA_ERR_HIP;
    }
    if (alloc_log()) fprintf(stderr, "[nvca alloc] host register   %p .. %p (%zu bytes)%s\n", ptr, (void *)((char *)ptr + bytes), bytes, ctx->host_ranges.was_registered(ptr, bytes) ? " -- overlaps a range released earlier" : "");
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)
// The pages are released only when every stream that carried a copy of the range since it was registered has drained: the
// batched face path copies host frames on the copy stream and on the lanes of the two batches in flight, not only on the
// context's own stream -- an unregister behind a failed or abandoned batch must not pull pages from under a copy.
int nvca_host_unregister(nvca_ctx *ctx, void *ptr)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (!ptr) return NVCA_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    const int i = ctx->host_ranges.find(ptr);
    if (i < 0) { ctx->set_error("nvca_host_unregister: not a pointer nvca_host_register was given"); return NVCA_ERR_ARG; }
    const uint64_t streams = ctx->host_ranges.live[(size_t)i].streams;
    for (int id = 0; id < 64; id++)
        if ((streams >> id) & 1ull) {
            hipStream_t st = stream_of_id(ctx, id);
            if (st) NVCA_HIP_CHECK(ctx, hipStreamSynchronize(st)); else NVCA_HIP_CHECK(ctx, hipDeviceSynchronize());
        }
    bool found; (void)ctx->host_ranges.remove(ptr, &found);
    if (alloc_log()) fprintf(stderr, "[nvca alloc] host unregister %p (streams drained: 0x%llx)\n", ptr, (unsigned long long)streams);
    NVCA_HIP_CHECK(ctx, hipHostUnregister(ptr));
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)

int nvca_ctx_enable_kernel_timing(nvca_ctx *ctx, int on)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (!ctx) return NVCA_ERR_ARG;
    (void)hipStreamSynchronize(ctx->cs());
    drain_timer(ctx);
    ctx->timer.on = on != 0;
    ctx->timer.stride = on > 1 ? on : 1; ctx->timer.seq[0] = ctx->timer.seq[1] = 0; ctx->timer.sample = true;
    for (int k = 0; k < NVCA_K_COUNT; k++) { ctx->timer.total_ms[k] = 0; ctx->timer.launches[k] = 0; }
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)
int nvca_ctx_kernel_timing(nvca_ctx *ctx, double *total_ms, int64_t *launches)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (!ctx) return NVCA_ERR_ARG;
    NVCA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->cs()));
    drain_timer_now(ctx);
    for (int k = 0; k < NVCA_K_COUNT; k++) {
        if (total_ms) total_ms[k] = ctx->timer.total_ms[k];
        if (launches) launches[k] = ctx->timer.launches[k];
        ctx->timer.total_ms[k] = 0; ctx->timer.launches[k] = 0;
    }
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)
const char *nvca_kernel_name(int k)
{
    static const char *names[NVCA_K_COUNT] = {"gray_resize_hist", "equalize_lut", "integral_colsum", "integral_bandscan",
                                              "integral_rows", "cascade_stage0", "cascade_strip", "cascade_deep",
                                              "group_rects", "tracker", "resize_gray", "cascade_tile", "cascade_band", "cascade_roi"};
    return (k >= 0 && k < NVCA_K_COUNT) ? names[k] : "?";
}

// =========================================================================
// cascade
// =========================================================================
int nvca_cascade_load_mem(nvca_ctx *ctx, const char *xml, int64_t len, nvca_cascade **out)
try {
    return nvca_cascade_load_mem_ex(ctx, xml, len, 0u, out);
}
NVCA_API_CATCH(ctx)

int nvca_cascade_load_mem_ex(nvca_ctx *ctx, const char *xml, int64_t len, unsigned flags, nvca_cascade **out)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (!ctx || !xml || len <= 0 || !out) return NVCA_ERR_ARG;
    *out = nullptr;
    if (flags & ~(unsigned)NVCA_LOAD_HAAR_GENERAL) { ctx->set_error("cascade load: unknown flag bits"); return NVCA_ERR_ARG; }
    std::unique_ptr<nvca_cascade> c(new nvca_cascade());
    std::string err;
    CascadeFile f;
    int rc = parse_cascade_file(xml, (size_t)len, flags, f, err);
    if (rc) { ctx->set_error("cascade XML: " + err); return rc; }
    c->c = std::move(f.haar); c->lbp = std::move(f.lbp); c->hnew = std::move(f.hnew); c->format = f.format;
    c->ctx = ctx;
    c->c.uid = ctx->next_uid++;
    *out = c.release();
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)

// the loader alone, on the host: no device, no context (a deployment can check its cascade files on a box without a GPU; the
// CPU test-suite and the sanitizer build run the parser through the ABI this way)
int nvca_cascade_validate_mem(const char *xml, int64_t len, int *win_w, int *win_h, int *n_stages, int *n_weak, char *err, int err_cap)
try {
    return nvca_cascade_validate_mem_ex(xml, len, 0u, win_w, win_h, n_stages, n_weak, err, err_cap);
}
NVCA_API_CATCH(nullptr)

int nvca_cascade_validate_mem_ex(const char *xml, int64_t len, unsigned flags, int *win_w, int *win_h, int *n_stages, int *n_weak, char *err, int err_cap)
try {
    if (err && err_cap > 0) err[0] = 0;
    if (!xml || len <= 0 || (flags & ~(unsigned)NVCA_LOAD_HAAR_GENERAL)) return NVCA_ERR_ARG;
    CascadeFile f;
    std::string msg;
    const int rc = parse_cascade_file(xml, (size_t)len, flags, f, msg);
    if (rc) { if (err && err_cap > 0) snprintf(err, (size_t)err_cap, "%s", msg.c_str()); return rc; }
    const bool lbp = f.format == NVCA_CASCADE_LBP, hnew = f.format == NVCA_CASCADE_HAAR_NEW;
    if (win_w) *win_w = f.haar.ow;
    if (win_h) *win_h = f.haar.oh;
    if (n_stages) *n_stages = lbp ? (int)f.lbp.stages.size() : hnew ? (int)f.hnew.stages.size() : (int)f.haar.stages.size();
    if (n_weak) *n_weak = lbp ? (int)f.lbp.weak.size() : hnew ? (int)f.hnew.nweak() : (int)f.haar.cls.size();
    return NVCA_OK;
}
NVCA_API_CATCH(nullptr)

// Throws on purpose, below the barrier every entry point has: what the caller gets back is the barrier's status code.
// kind 0: std::bad_alloc, 1: std::length_error out of a container, 2: std::runtime_error, 3: a non-standard exception,
// 4: std::out_of_range out of vector::at; anything else: NVCA_OK.  (tests/test_abi_cpu.py)
int nvca_abi_selftest(int kind)
try {
    std::vector<int> v;
    if (kind == 0) throw std::bad_alloc();
    if (kind == 1) v.resize(v.max_size() + 1);
    if (kind == 2) throw std::runtime_error("selftest");
    if (kind == 3) throw 42;
    if (kind == 4) return v.at(7);
    return NVCA_OK;
}
NVCA_API_CATCH(nullptr)

int nvca_cascade_load_xml(nvca_ctx *ctx, const char *path, nvca_cascade **out)
try {
    return nvca_cascade_load_xml_ex(ctx, path, 0u, out);
}
NVCA_API_CATCH(ctx)

int nvca_cascade_load_xml_ex(nvca_ctx *ctx, const char *path, unsigned flags, nvca_cascade **out)
try {
    if (!ctx || !path || !out) return NVCA_ERR_ARG;
    std::ifstream f(path, std::ios::binary);
    if (!f) { ctx->set_error(std::string("cannot open cascade file ") + path); return NVCA_ERR_IO; }
    std::stringstream ss; ss << f.rdbuf();
    const std::string s = ss.str();
    if (s.empty()) { ctx->set_error(std::string("empty cascade file ") + path); return NVCA_ERR_IO; }
    return nvca_cascade_load_mem_ex(ctx, s.data(), (int64_t)s.size(), flags, out);
}
NVCA_API_CATCH(ctx)

void nvca_cascade_free(nvca_cascade *c)
try {
    if (!c) return;
    // drop cached plans that reference this cascade
    if (c->ctx) {
        std::lock_guard<std::recursive_mutex> lk(c->ctx->mu);
        char pre[64];
        for (auto it = c->ctx->plans.begin(); it != c->ctx->plans.end();) {
            const std::string &k = it->first;
            snprintf(pre, sizeof(pre), "|%llu|", (unsigned long long)c->c.uid);
            if (k.find(pre) != std::string::npos && it->second->inflight == 0) { (void)hipDeviceSynchronize(); it = c->ctx->plans.erase(it); }
            else ++it;
        }
        { auto sr = c->ctx->roi_stage_recs.find((uint64_t)c->c.uid);
          if (sr != c->ctx->roi_stage_recs.end()) { (void)hipDeviceSynchronize(); sr->second->release(); delete sr->second; c->ctx->roi_stage_recs.erase(sr); } }
        bool drained = false;
        for (auto it = c->ctx->scale_tables.begin(); it != c->ctx->scale_tables.end();) {      // and its stump tables (one drain of the device for all of them)
            if (it->first.first == (uint64_t)c->c.uid && it->second->refs == 0) {
                if (!drained) { (void)hipDeviceSynchronize(); drained = true; }
                delete it->second; it = c->ctx->scale_tables.erase(it);
            } else ++it;
        }
    }
    delete c;
}
NVCA_API_CATCH_VOID

int nvca_cascade_info(const nvca_cascade *c, int *win_w, int *win_h, int *n_stages, int *n_weak)
try {
    if (!c) return NVCA_ERR_ARG;
    if (win_w) *win_w = c->c.ow;
    if (win_h) *win_h = c->c.oh;
    const bool lbp = c->format == NVCA_CASCADE_LBP, hnew = c->format == NVCA_CASCADE_HAAR_NEW;
    if (n_stages) *n_stages = lbp ? (int)c->lbp.stages.size() : hnew ? (int)c->hnew.stages.size() : (int)c->c.stages.size();
    if (n_weak) *n_weak = lbp ? (int)c->lbp.weak.size() : hnew ? (int)c->hnew.nweak() : (int)c->c.cls.size();
    return NVCA_OK;
}
NVCA_API_CATCH((c ? c->ctx : nullptr))

// which branch of cv::CascadeClassifier::load (cascadedetect.cpp) took the file
int nvca_cascade_format(const nvca_cascade *c, int *format, int *n_features)
try {
    if (!c) return NVCA_ERR_ARG;
    if (format) *format = c->format;
    if (n_features) *n_features = c->format == NVCA_CASCADE_LBP ? (int)c->lbp.features.size() : c->format == NVCA_CASCADE_HAAR_NEW ? (int)c->hnew.features.size() : 0;
    return NVCA_OK;
}
NVCA_API_CATCH((c ? c->ctx : nullptr))

// what cascadedetect.cpp's Data::read / LBPEvaluator::read keep of an LBP cascade, flat
int nvca_cascade_dump_lbp(const nvca_cascade *c, int *rects, int *feature_idx, int32_t *subsets, float *leaves, int *stage_sizes, float *stage_thr)
try {
    if (!c || c->format != NVCA_CASCADE_LBP) return NVCA_ERR_ARG;
    const LbpCascade &l = c->lbp;
    for (size_t i = 0; i < l.features.size() && rects; i++) { rects[i * 4] = l.features[i].x; rects[i * 4 + 1] = l.features[i].y; rects[i * 4 + 2] = l.features[i].w; rects[i * 4 + 3] = l.features[i].h; }
    for (size_t i = 0; i < l.weak.size(); i++) {
        if (feature_idx) feature_idx[i] = l.weak[i].feature;
        if (subsets) memcpy(subsets + i * 8, l.weak[i].subset, sizeof(int32_t) * 8);
        if (leaves) { leaves[i * 2] = l.weak[i].leaf[0]; leaves[i * 2 + 1] = l.weak[i].leaf[1]; }
    }
    for (size_t s = 0; s < l.stages.size(); s++) {
        if (stage_sizes) stage_sizes[s] = l.stages[s].count;
        if (stage_thr) stage_thr[s] = l.stages[s].threshold;
    }
    return NVCA_OK;
}
NVCA_API_CATCH((c ? c->ctx : nullptr))

// what Data::read / HaarEvaluator::read keep of a new-format HAAR cascade, flat
int nvca_cascade_dump_haar_new(const nvca_cascade *c, int *rects, float *weights, int *rect_counts, int *feature_idx, float *thr, float *leaves,
                               int *stage_sizes, float *stage_thr)
try {
    if (!c || c->format != NVCA_CASCADE_HAAR_NEW || c->hnew.general) return NVCA_ERR_ARG;          // (a general cascade: nvca_cascade_dump_haar_tree)
    const HnewCascade &h = c->hnew;
    for (size_t i = 0; i < h.features.size(); i++) {
        if (rects) memcpy(rects + i * 12, h.features[i].rect, sizeof(int) * 12);
        if (weights) memcpy(weights + i * 3, h.features[i].weight, sizeof(float) * 3);
        if (rect_counts) rect_counts[i] = h.features[i].nrect;
    }
    for (size_t i = 0; i < h.weak.size(); i++) {
        if (feature_idx) feature_idx[i] = h.weak[i].feature;
        if (thr) thr[i] = h.weak[i].threshold;
        if (leaves) { leaves[i * 2] = h.weak[i].leaf[0]; leaves[i * 2 + 1] = h.weak[i].leaf[1]; }
    }
    for (size_t s = 0; s < h.stages.size(); s++) {
        if (stage_sizes) stage_sizes[s] = h.stages[s].count;
        if (stage_thr) stage_thr[s] = h.stages[s].threshold;
    }
    return NVCA_OK;
}
NVCA_API_CATCH((c ? c->ctx : nullptr))

int nvca_cascade_tree_info(const nvca_cascade *c, int *n_nodes, int *n_leaves, int *general)
try {
    if (!c || c->format != NVCA_CASCADE_HAAR_NEW) return NVCA_ERR_ARG;
    const HnewCascade &h = c->hnew;
    if (n_nodes) *n_nodes = h.general ? (int)h.nodes.size() : (int)h.weak.size();
    if (n_leaves) *n_leaves = h.general ? (int)h.leaves.size() : 2 * (int)h.weak.size();
    if (general) *general = h.general ? 1 : 0;
    return NVCA_OK;
}
NVCA_API_CATCH((c ? c->ctx : nullptr))

// a new-format HAAR cascade in terms that express trees: a stump cascade's weak classifiers as the one-node trees "0 -1" they are
int nvca_cascade_dump_haar_tree(const nvca_cascade *c, int *rects, float *weights, int *rect_counts, int *tilted, int *node_counts,
                                int *nodes, float *node_thr, float *leaves, int *stage_sizes, float *stage_thr)
try {
    if (!c || c->format != NVCA_CASCADE_HAAR_NEW) return NVCA_ERR_ARG;
    const HnewCascade &h = c->hnew;
    for (size_t i = 0; i < h.features.size(); i++) {
        if (rects) memcpy(rects + i * 12, h.features[i].rect, sizeof(int) * 12);
        if (weights) memcpy(weights + i * 3, h.features[i].weight, sizeof(float) * 3);
        if (rect_counts) rect_counts[i] = h.features[i].nrect;
        if (tilted) tilted[i] = h.general ? (int)h.tilted[i] : 0;
    }
    if (h.general) {
        for (size_t i = 0; i < h.trees.size() && node_counts; i++) node_counts[i] = h.trees[i].nnodes;
        for (size_t i = 0; i < h.nodes.size(); i++) {
            if (nodes) { nodes[i * 3] = h.nodes[i].left; nodes[i * 3 + 1] = h.nodes[i].right; nodes[i * 3 + 2] = h.nodes[i].feature; }
            if (node_thr) node_thr[i] = h.nodes[i].threshold;
        }
        for (size_t i = 0; i < h.leaves.size() && leaves; i++) leaves[i] = h.leaves[i];
    } else
        for (size_t i = 0; i < h.weak.size(); i++) {
            if (node_counts) node_counts[i] = 1;
            if (nodes) { nodes[i * 3] = 0; nodes[i * 3 + 1] = -1; nodes[i * 3 + 2] = h.weak[i].feature; }
            if (node_thr) node_thr[i] = h.weak[i].threshold;
            if (leaves) { leaves[i * 2] = h.weak[i].leaf[0]; leaves[i * 2 + 1] = h.weak[i].leaf[1]; }
        }
    for (size_t s = 0; s < h.stages.size(); s++) {
        if (stage_sizes) stage_sizes[s] = h.stages[s].count;
        if (stage_thr) stage_thr[s] = h.stages[s].threshold;
    }
    return NVCA_OK;
}
NVCA_API_CATCH((c ? c->ctx : nullptr))

// the small-image route of a new-format HAAR cascade (k_roi_hnew), opt-in: the flag is read when a job is built (make_detect_job)
int nvca_cascade_set_small_route(nvca_cascade *c, int on)
try {
    if (!c) return NVCA_ERR_ARG;
    if (c->format == NVCA_CASCADE_HAAR_NEW && !c->hnew.general) c->small_route.store(on ? 1 : 0, std::memory_order_relaxed);
    return NVCA_OK;
}
NVCA_API_CATCH((c ? c->ctx : nullptr))

int nvca_cascade_get_small_route(const nvca_cascade *c, int *on)
try {
    if (!c || !on) return NVCA_ERR_ARG;
    *on = c->format == NVCA_CASCADE_HAAR_NEW ? c->small_route.load(std::memory_order_relaxed) : 1;
    return NVCA_OK;
}
NVCA_API_CATCH((c ? c->ctx : nullptr))

int nvca_cascade_kind(const nvca_cascade *c, int *has_tilted, int *has_trees)
try {
    if (!c) return NVCA_ERR_ARG;
    bool trees = !c->c.stump_based;          // (an old-format model that was never filled says stumps, upright)
    if (c->format == NVCA_CASCADE_HAAR_NEW) for (const HgenTree &t : c->hnew.trees) trees = trees || t.nnodes > 1;
    if (has_tilted) *has_tilted = c->c.has_tilted || (c->format == NVCA_CASCADE_HAAR_NEW && c->hnew.has_tilted) ? 1 : 0;
    if (has_trees) *has_trees = trees ? 1 : 0;
    return NVCA_OK;
}
NVCA_API_CATCH((c ? c->ctx : nullptr))

int nvca_cascade_dump(const nvca_cascade *c, int *rects, float *weights, float *thr, float *left_val,
                      float *right_val, int *stage_sizes, float *stage_thr)
try {
    if (!c || c->format != NVCA_CASCADE_HAAR) return NVCA_ERR_ARG;
    if (!c->c.stump_based) return NVCA_ERR_UNSUPPORTED;
    for (size_t i = 0; i < c->c.cls.size(); i++) {
        const HaarNode &n = c->c.nodes[c->c.cls[i].first_node];
        if (rects) memcpy(rects + i * 12, n.rect, sizeof(int) * 12);
        if (weights) memcpy(weights + i * 3, n.weight, sizeof(float) * 3);
        if (thr) thr[i] = n.threshold;
        if (left_val) left_val[i] = c->c.alpha[c->c.cls[i].first_alpha];
        if (right_val) right_val[i] = c->c.alpha[c->c.cls[i].first_alpha + 1];
    }
    for (size_t s = 0; s < c->c.stages.size(); s++) {
        if (stage_sizes) stage_sizes[s] = c->c.stages[s].ncls;
        if (stage_thr) stage_thr[s] = c->c.stages[s].threshold;
    }
    return NVCA_OK;
}
NVCA_API_CATCH((c ? c->ctx : nullptr))

} // extern "C"
