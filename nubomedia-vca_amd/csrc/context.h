// context.h -- the context (nvca_ctx), its buffers, work spaces and timers, the ABI's exception barrier and the detect-job API:
// what the host sources of the library share (not part of the ABI).
#pragma once
#include <atomic>
#include <string>
#include <vector>
#include <map>
#include <memory>
#include <mutex>
#include "cascade_model.h"
#include "switches.h"
#include "work_pool.h"
#include "launch.h"
#include "host_ranges.h"
#include "part_stats.h"

namespace nvca {

// --------------------------------------------------------------------------
// Context
// --------------------------------------------------------------------------
#define NVCA_HIP_CHECK(ctx, expr)                                                   \
    do {                                                                            \
        hipError_t e__ = (expr);                                                    \
        if (e__ != hipSuccess) {                                                    \
            (ctx)->set_error(std::string(#expr) + ": " + hipGetErrorString(e__));   \
            return NVCA_ERR_HIP;                                                    \
        }                                                                           \
    } while (0)

struct DevBuf {
    void *p = nullptr; size_t bytes = 0;
    int ensure(size_t n);          // grows (never shrinks); returns hipError as int
    void release();
    template <class T> T *as() const { return (T *)p; }
};
struct PinnedBuf {
    void *p = nullptr; size_t bytes = 0;
    int ensure(size_t n);
    void release();
    template <class T> T *as() const { return (T *)p; }
};

// Page-locked memory of the context's own that caller host memory crosses through when it is not page-locked by the caller
// (nvca_host_register): a ring of fixed slots, each with the event of the last copy that read or wrote it (host_copy.cpp, caller_h2d ...).
struct BounceRing {
    static constexpr size_t kSlot = 8u << 20;      // a 1080p BGR frame (6.2 MB) is one slot: one CPU copy (shared by the helper threads) + one DMA
    static constexpr int kSlots = 12;
    PinnedBuf buf; hipEvent_t ev[kSlots] = {}; bool pending[kSlots] = {}; int next = 0;
    void release() { for (hipEvent_t &e : ev) if (e) { (void)hipEventDestroy(e); e = nullptr; } buf.release(); }
};

// tracker workspace (tracker.cpp; sizes and parts: trk_layout.h): slot table, labels, per-root accumulators, component list, frame staging,
// segment flags, root list, live-tile list
struct TrkWorkspace {
    DevBuf slots, labels, acc, out, staging, flags, roots, tiles; PinnedBuf h_slots, h_out;
    // the live-tile list's marks are stamped with the launch's tick and never cleared (trk_layout.h, TileList): they are
    // zeroed when the buffer's layout changes (frame size, batch) and when the tick would come round
    int tick = 0, tiles_w = 0, tiles_h = 0, tiles_batch = 0;
    void release_all() { slots.release(); labels.release(); acc.release(); out.release(); staging.release(); flags.release(); roots.release(); tiles.release(); h_slots.release(); h_out.release(); tiles_w = tiles_h = tiles_batch = 0; }
};

// batched part detectors (part_images.cpp): working images of a call carved from one arena, the small tables its launches read
struct PartWorkspace {
    DevBuf arena, tables, hist, luts; PinnedBuf h_tables;
    size_t tab_used = 0;
    hipEvent_t images_done = nullptr;
    void release_all() { arena.release(); tables.release(); hist.release(); luts.release(); h_tables.release(); if (images_done) { (void)hipEventDestroy(images_done); images_done = nullptr; } }
};


struct DetectPlan;   // plan.cpp
struct ScaleTable;   // plan.cpp: one cascade at one scale factor (geometry-independent stump records), cached in the context
struct FaceTicket;   // face_stream.cpp
void free_face_ticket(FaceTicket *t);
struct PartCall;     // part_call.h: a submitted, not yet collected call of the batched part detectors
// (parts.cpp) the outstanding calls that hold stream s (nullptr: any) are given up: rolled back (newest first), drained, deleted
void part_calls_abandon(nvca_ctx *ctx, const nvca_part_stream *s);
struct GeomPlan;     // host_state.h
struct Workspace;    // host_state.h

struct KernelTimer {
    bool on = false;
    int stride = 1;                 // events ride on every stride-th batch of an entry point (they serialise consecutive launches)
    uint64_t seq[2] = {0, 0};       // batches seen: [0] face detector, [1] tracker
    bool sample = true;             // the batch being queued carries events
    void tick(int which) { sample = stride <= 1 || (seq[which]++ % (uint64_t)stride) == 0; }
    struct Ev { hipEvent_t a, b; int k; bool first; };
    std::vector<Ev> pending;
    std::vector<hipEvent_t> pool;
    double total_ms[NVCA_K_COUNT] = {0};
    int64_t launches[NVCA_K_COUNT] = {0};
};

} // namespace nvca

struct nvca_cascade {       // format LBP / HAAR_NEW: `lbp` / `hnew` is the model, c holds the window size and the uid
    nvca::Cascade c; nvca_ctx *ctx; nvca::LbpCascade lbp; int format = NVCA_CASCADE_HAAR; nvca::HnewCascade hnew;
    // a new-format file, whatever its features: the new-format scan (its own pyramid levels, step and skip rule; `flags` ignored)
    bool new_format() const { return format != NVCA_CASCADE_HAAR; }
    // NVCA_CASCADE_HAAR_NEW only (nvca_cascade_set_small_route): small images of this cascade may take k_roi_hnew.  Read when a job is
    // built (DetectJob::Request::small_route): a submitted ticket keeps the route it was built with
    std::atomic<int> small_route{0};
};

namespace nvca {
static constexpr int kLanes = 10;         // lane 0: the context's stream; 1 .. 7: the batched part detectors; 8: the face detector's second batch in flight; 9: the trackers
static constexpr int kPartLanes = 8;      // lanes [0, kPartLanes) are the ones the part detectors spread over
static constexpr int kFaceLane2 = 8;
static constexpr int kTrackerLane = 9;    // NuboTracker's kernels: its state and workspace are its own, so a face batch in flight (lane 0 / 8) and a tracker call overlap
}

struct nvca_ctx {
    int device = 0;
    hipStream_t stream = nullptr;             // lane 0
    hipStream_t lane_streams[nvca::kLanes] = {nullptr};   // [0] == stream; the others carry the batched part detectors' jobs (host_state.h, Lane)
    int cur_lane = 0;
    hipStream_t cs() const { return lane_streams[cur_lane]; }       // the stream of the lane that is being queued on
    nvca::HostRangeTable host_ranges;         // what the caller page-locked through nvca_host_register (host_ranges.h: the only caller memory a copy is handed as it stands)
    nvca::BounceRing bounce;                  // everything else crosses through here
    hipStream_t copy_stream = nullptr;        // H2D of the next chunk of host frames while the current one computes
    std::vector<hipEvent_t> chunk_events;
    nvca::FaceTicket *face_tickets[3] = {nullptr, nullptr, nullptr};   // [0] synchronous calls, [1] / [2] submit / collect
    uint64_t face_serial = 0;
    int ptr_ring_used = 0;                    // nvca_bgr2gray: entries of the frame-pointer ring handed out since the last drain
    int defer_device_sync = 0;                // > 0: primitives that write device memory return without draining the stream
                                              // (internal callers chaining primitives on the context's stream)
    std::string err;
    int hit_cap = 16384;
    int hit_cap_wanted = 0;                   // > hit_cap: a launch set produced more raw candidates than its lists hold; the per-frame size that holds it
    int policy = NVCA_SUM_F32PAIR;
    uint64_t next_uid = 1;
    nvca::KernelTimer timer;
    std::map<std::string, std::unique_ptr<nvca::GeomPlan>> plans;
    std::map<std::pair<uint64_t, uint64_t>, nvca::ScaleTable *> scale_tables;   // (cascade uid, factor bits)
    std::unique_ptr<nvca::Workspace> ws;
    nvca::TrkWorkspace trk;           // tracker buffers live and die with the context
    // the working images / tables of a batched part-detector call; two sets: a submitted call (nvca_part_batch_submit) may be in
    // flight while the one before it is collected -- a call uses the set of its ticket's parity (part_call.cpp sets part_set)
    nvca::PartWorkspace part_sets[2]; int part_set = 0;
    nvca::PartWorkspace &pw() { return part_sets[part_set]; }
    nvca::PartCall *part_calls[2] = {nullptr, nullptr};    // submitted, not yet collected part-detector calls, by ticket parity (parts.cpp)
    int part_seq = 0;                         // the next ticket
    nvca::Switches sw;                // this context's switches: the process defaults (environment), nvca_ctx_set_option overrides
    int lds_grant[2] = {0, 0};        // dynamic LDS already granted to k_tile / k_band through this context (hipFuncSetAttribute)
    void *identity_lut = nullptr;     // 256 B on device
    nvca::DevBuf overlay_img;         // the caller's overlay image on the device (nvca_overlay_blend on device frames)
    // small-image detector (kernels_roi.hip): per-cascade stage records on the device, the tables / candidate list of a launch
    std::map<uint64_t, nvca::DevBuf *> roi_stage_recs;
    // (three sets: [0] the synchronous callers', [1] / [2] the part-detector calls in flight by ticket parity -- a round of theirs stays
    // queued between submit and collect)
    struct RoiBuffers { nvca::DevBuf tables, hits, rej; nvca::PinnedBuf h_tables, h_hits, h_rej; } roi_bufs[3]; int roi_set = 0;
    RoiBuffers &rbuf() { return roi_bufs[roi_set]; }
    size_t roi_first_hint = 0;              // candidates of the recent small-image rounds (+ a quarter): what the launch copies back with itself
    nvca::WorkPool *pool = nullptr; bool pool_tried = false;
    nvca::PartStats stats;            // NVCA_PART_STATS: this context's phase timers
    std::mutex err_mu;                // set_error may be called from the helper threads
#ifdef NVCA_STAMPS
    unsigned long long *stamps = nullptr;
#endif
    std::recursive_mutex mu;          // serialises entry points: elements on different streaming threads share one context
    void set_error(const std::string &s) { std::lock_guard<std::mutex> lk(err_mu); err = s; }
    nvca_ctx();
    ~nvca_ctx();
};

// Exception barrier of the ABI.  Every extern "C" entry point is a function-try-block whose handler is one of these macros:
// nothing thrown below it (std::bad_alloc / std::length_error from the host-side containers, anything else) crosses into the
// caller's C frames -- the call returns a status code instead, as include/nubovca.h promises.  api_catch() rethrows inside its
// own try block to tell the cases apart (it never throws itself).
namespace nvca { int api_catch(nvca_ctx *ctx) noexcept; }
#define NVCA_API_CATCH(ctxexpr) catch (...) { return nvca::api_catch(ctxexpr); }
#define NVCA_API_CATCH_VOID catch (...) { (void)nvca::api_catch(nullptr); }

#define NVCA_LOCK_OR_FAIL(ctx) if (!(ctx)) return NVCA_ERR_ARG; std::lock_guard<std::recursive_mutex> nvca_lock__((ctx)->mu); (void)nvca::take_launch_error(nullptr)   /* a launch failure of an earlier call on this thread has been reported by that call */

namespace nvca {

// RAII bracket: while timing is enabled, every kernel launched inside the scope carries a start / stop event pair in
// its dispatch packet (hipExtLaunchKernelGGL) -- no separate event-record packets on the stream
struct TimedLaunch {
    nvca_ctx *ctx; int k; int n = 0; TimedLaunch *prev = nullptr; bool active = false;
    TimedLaunch(nvca_ctx *c, int kind);
    ~TimedLaunch();
};
#define NVCA_LAUNCH_CHECK(ctx)                                                                                    \
    do {                                                                                                          \
        const char *k__ = nullptr;                                                                                \
        const hipError_t le__ = nvca::take_launch_error(&k__);                                                    \
        if (le__ != hipSuccess) {                                                                                 \
            (ctx)->set_error(std::string("kernel launch failed (") + (k__ ? k__ : "?") + "): " + hipGetErrorString(le__)); \
            return NVCA_ERR_HIP;                                                                                  \
        }                                                                                                         \
    } while (0)

// ---- caller host memory <-> device (host_copy.cpp): direct only inside a range the caller registered, otherwise through the bounce ring
int caller_h2d(nvca_ctx *ctx, void *dst, const void *src, size_t bytes, hipStream_t st);
int caller_h2d_rows(nvca_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t rows, hipStream_t st);
int caller_d2h_rows(nvca_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t rows, hipStream_t st);   // returns with dst filled (the stream is drained)

// ---- the part detectors' upload ring for small tables (part_images.cpp); nvca_draw_shapes queues its shapes through it too
int part_table(nvca_ctx *ctx, const void *host, size_t bytes, void **dev);   // a small table for the next launch on the current lane (upload ring)
struct DetectJob;
int make_detect_job(nvca_ctx *ctx, DetectJob &j, const nvca_cascade *casc, const void *gray, int w, int h, int stride, int mem,
                    double sf, int min_neighbors, int flags, int minw, int minh, int maxw, int maxh, bool raw_only);
int run_detect_jobs(nvca_ctx *ctx, DetectJob *const *jobs, int n, const int *lanes);      // lanes: per job, or null (current lane)
// ... in two halves: the first round queued and left in flight, then the rest (detect_rounds.cpp)
struct JobRound;
JobRound *job_round_new();
void job_round_free(JobRound *r);
int detect_jobs_begin(nvca_ctx *ctx, DetectJob *const *jobs, int n, const int *lanes, JobRound *R, bool *queued);
int detect_jobs_finish(nvca_ctx *ctx, DetectJob *const *jobs, int n, const int *lanes, JobRound *R, bool queued);
DetectJob *detect_job_new();
void detect_job_free(DetectJob *j);
const std::vector<nvca_rect> &detect_job_out(const DetectJob *j, int k);
constexpr int kJobImages = 32;                                    // images of one geometry that a plain / SCALE_IMAGE / LBP job can carry
int detect_job_add_image(DetectJob *j, const void *image);       // one more image for the job's launch set; returns its index k (detect_job_out), -1: full / not possible

} // namespace nvca
