// host_state.h -- host-side state and helpers that the library's host sources share (not part of the ABI): the workspace, the
// cached plans and cascade jobs (plans.cpp), detectMultiScale jobs and small-image batches (detect_job.cpp, lbp_job.cpp, pyramid.cpp,
// detect_rounds.cpp, roi_batch.cpp), and the helpers one source calls in another.  plan.cpp, host_logic.cpp, group_levels.cpp, part_logic.cpp, fb_search.cpp,
// part_stats.cpp, options.cpp, cascade_xml.cpp, pyr_levels.cpp, lbp_tables.cpp, trk_host.cpp and work_pool.cpp do not include it: the CPU
// drivers under tests/ build those without it (part_logic.cpp, fb_search.cpp, part_stats.cpp, options.cpp, pyr_levels.cpp, lbp_tables.cpp and
// trk_host.cpp without any HIP header, the others with host doubles of their own).
#pragma once
#include "context.h"
#include "plan.h"
#include "fb_search.h"
#include "host_math.h"
#include "pyr_levels.h"
#include "yuv_layout.h"

namespace nvca {

// ---- runtime.cpp
bool alloc_log();                                            // NVCA_ALLOC_LOG=1: allocations and host registrations on stderr
void drain_timer_now(nvca_ctx *ctx);                         // kernel timing: event pairs -> times
void drain_timer(nvca_ctx *ctx);                             // ... once many have piled up

// what a cascade job leaves behind for the host: candidate list, box table, thresholds.  Three sets: [0] the synchronous
// entry points, [1] / [2] the two batches that may be in flight through nvca_face_batch_submit / _collect
struct ResultBufs {
    DevBuf hits, grp, gthr, staging, srcptrs;        // staging / srcptrs: host frames on their way in, frame pointer table
    PinnedBuf h_hits, h_grp, h_gthr, h_srcptrs;   // h_srcptrs: frame pointers on their way to the device array
    DevBuf recs; PinnedBuf h_recs;    // a levels job's LevelRec per candidate, laid out as hits without the count word (allocated by the first such job)
    std::vector<int> gthr_last;       // thresholds currently resident in gthr
    void release() { hits.release(); grp.release(); gthr.release(); staging.release(); srcptrs.release(); h_hits.release(); h_grp.release(); h_gthr.release(); h_srcptrs.release(); recs.release(); h_recs.release(); gthr_last.clear(); }
};
// Working memory of the kernels, per LANE.  A lane is a HIP stream with its own planes and cascade scratch: whatever runs on a
// lane is ordered by its stream, different lanes run side by side.  Everything uses lane 0 (the context's stream) except
// the batched part detectors, which spread their streams' small, launch-bound jobs over all lanes (part_call.cpp): the GPU then
// holds several of those tiny kernels at a time instead of one.  What a job leaves for the host lives in ResultBufs regions
// of its own, shared by all lanes.
struct Lane {
    DevBuf gray, hist, lut, bandsum, bandsq, sum, sqsum, tilted, staging, aux, failbits, vnf, deep;
    int hist_clean = 0;               // leading histogram slots known to be all zero
    void release_all()
    {
        gray.release(); hist.release(); lut.release(); bandsum.release(); bandsq.release(); sum.release();
        sqsum.release(); tilted.release(); staging.release(); aux.release();
        failbits.release(); vnf.release(); deep.release();
    }
};
struct Workspace {
    Lane lanes[kLanes];
    int *cur_lane = nullptr;          // the context's current lane index
    Lane &ln() { return lanes[*cur_lane]; }
    ResultBufs res[3];
    int cur_res = 0;
    void release_all()
    {
        for (Lane &l : lanes) l.release_all();
        for (ResultBufs &r : res) r.release();
    }
};

// one cached geometry: source frame -> working image -> scan tables
// Source rows a shrinking bilinear resize reads, when they form equal runs at a fixed period (integer ratios: a 1080p
// frame shrunk by 12 reads rows 12k + 5 and 12k + 6 only).  Host frames then cross PCIe as one strided 2-D copy of those
// rows -- into their natural places of the staged frame, so the kernels are unchanged -- instead of whole.
struct RowCopy {
    bool on = false;
    int first = 0, period = 0, run = 0, count = 0;
};

// new-format cascades (lbp_job.cpp, lbp_plan; the tables: lbp_tables.cpp, hnew_tables.cpp): the evaluator's tables on the device and its arguments
// but for the per-call buffers; the pyramid and the scan grids (hit_valid / hit_rect) are the GeomPlan's lv / det.specs.  `format` says which
// evaluator scans: NVCA_CASCADE_LBP (args alone) or NVCA_CASCADE_HAAR_NEW (hnew, whose `l` is filled from args at every launch set)
struct LbpPlan {
    DevBuf d_blob; LbpArgs args{};
    int format = NVCA_CASCADE_LBP; HnewArgs hnew{};
    bool general = false, has_tilted = false;  // a general HAAR cascade: the hgen launches on these tables; the pyramid builds tilted planes
    const HgenNodeDev *hg_nodes = nullptr; const HgenWeakDev *hg_weak = nullptr;      // (in d_blob)
    size_t bit_words = 0, positions = 0;      // stage-0 pass bits (u32 words) and grid positions of all levels
    int lds = 0;                              // bytes of the stage-0 tile (0: the window is too large, stage 0 gathers from the plane)
    const ScaleRec *gscales = nullptr; const int *gpos = nullptr;      // device grouping: a record per level, the levels' output coordinates (in d_blob)
    ~LbpPlan() { d_blob.release(); }
};

struct GeomPlan {
    LbpPlan lbp;
    ResizeTab tab;
    RowCopy rowcopy;
    DevBuf d_xofs, d_yofs, d_ialpha, d_ibeta;
    ResizeView view() const { return ResizeView{tab.mode, tab.xmax, d_xofs.as<int>(), d_ialpha.as<short>(), d_yofs.as<int>(), d_ibeta.as<short>()}; }      // the tables on the device
    DetectPlan det;
    PreGeom g;
    bool has_det = false;
    uint64_t last_use = 0;                                    // plan cache is LRU-bounded (store_plan)
    int inflight = 0;                                         // batches in flight that reference this plan: never evicted
    // CV_HAAR_SCALE_IMAGE / LBP: pyramid levels, their resize tables, plane layout (pyr_layout's result)
    std::vector<PyrLevel> lv;
    std::vector<std::unique_ptr<GeomPlan>> level_tabs;
    size_t gray_total = 0, plane_total = 0; int P = 0;
    std::vector<int> fb_ladder;                               // FIND_BIGGEST: ladder position of each scale of the full-grid plan
    DevBuf d_pyr, d_level_tabs; int pyr_maxw = 0, pyr_maxh = 0; bool pyr_ok = false;   // device level table (one-launch pyramid kernels)
    ~GeomPlan() { level_tabs.clear(); d_xofs.release(); d_yofs.release(); d_ialpha.release(); d_ibeta.release(); d_pyr.release(); d_level_tabs.release(); }
};

// cascade scan over the integral planes of slots [0, n); fills raw[b] (canonical scale,y,x order)
// group_thr (optional, [n]): cv::groupRectangles thresholds; when given and the plan allows it the grouping
// runs on the device (k_group) and raw[b] comes back already grouped -- grouped[b] says which.
// A job owns a result region (`r0` = index of its first frame in the caller's batch of `total` frames): its candidate
// list and box table stay untouched while later jobs are enqueued, so several jobs can be queued before one sync.
static constexpr int kMaxHitCap = 1 << 22;   // raw candidates per frame the lists are ever sized for (nvca_ctx_set_hit_capacity's limit)
static constexpr int kGroupOutCap = 64;      // final boxes per frame returned by k_group (more -> host grouping)
struct CascadeJob {
    int r0 = 0, n = 0, total = 0;
    bool dev_group = false;
    bool counters_zeroed = false;   // the caller's k_lut launch reset the two list counters (cascade_counters())
    unsigned cap = 0;
    size_t first = 0;         // raw candidates fetched with the count (raw mode)
    unsigned long long *d_hits = nullptr, *h_hits = nullptr;
    int *d_grp = nullptr, *h_grp = nullptr;
    LevelRec *d_recs = nullptr, *h_recs = nullptr;      // a levels job (lbp_launch_set): the record of candidate i of d_hits at [i]
};

// ---- plans.cpp
// several tables in one device allocation and one copy: add() copies an item in (h == nullptr: zeros) and returns its offset, a
// multiple of 256; after upload() the items lie at blob.p + offset
struct TableBlob {
    std::vector<unsigned char> bytes;
    size_t add(const void *h, size_t n);
    int upload(nvca_ctx *ctx, DevBuf &blob);
};
void make_geom(PreGeom &g, int sw, int sh, int sstride, int cn, int w, int h);
int ensure_ws(nvca_ctx *ctx, const PreGeom &g, int batch);
int upload_tabs(nvca_ctx *ctx, std::vector<std::unique_ptr<GeomPlan>> &levels, DevBuf &blob);
void run_integral(nvca_ctx *ctx, const PreGeom &g, const uint8_t *lut, int batch, const uint8_t *gray = nullptr, int *sum = nullptr,
                  unsigned long long *sq = nullptr);
int run_tilted(nvca_ctx *ctx, const PreGeom &g, const uint8_t *lut, int batch, const uint8_t *gray = nullptr, int *tilted = nullptr);
int cascade_counters(nvca_ctx *ctx, DetectPlan &dp, const CascadeJob &job, unsigned long long **hits, unsigned long long **deep);
int cascade_enqueue(nvca_ctx *ctx, DetectPlan &dp, size_t sum_slot, int spitch, CascadeJob &job, const int *group_thr, bool want_group,
                    hipEvent_t early_done = nullptr /* recorded behind the band / tile kernels, ahead of the late stages */);
// the two ends of a job that are no kernel's own (cascade_enqueue and the LBP launch set share them): the box-table region and the
// thresholds of a job k_group serves (job.dev_group); the copy of the job's results towards the host behind its last kernel
int group_prepare(nvca_ctx *ctx, CascadeJob &job, const int *group_thr);
int cascade_fetch(nvca_ctx *ctx, CascadeJob &job);
int cascade_collect(nvca_ctx *ctx, DetectPlan &dp, const CascadeJob &job, std::vector<std::vector<nvca_rect>> &raw,
                    std::vector<char> *grouped, std::vector<std::vector<int>> *scale_of = nullptr,
                    std::vector<std::vector<LevelRec>> *recs = nullptr /* a levels job: raw[b][k]'s record at (*recs)[b][k] */);
void group_all(std::vector<std::vector<nvca_rect>> &raw, int min_neighbors);
GeomPlan *find_plan(nvca_ctx *ctx, const std::string &key);
GeomPlan *store_plan(nvca_ctx *ctx, const std::string &key, std::unique_ptr<GeomPlan> gp);
int get_face_plan(nvca_ctx *ctx, const nvca_cascade *casc, int W, int H, int stride, int cn, int cols, int rows,
                  double sf, int minw, int minh, int maxw, int maxh, GeomPlan **out, const nvca_pixel_layout *yuv = nullptr);
int get_face_pre_plan(nvca_ctx *ctx, int W, int H, int stride, int cn, int cols, int rows, GeomPlan **out, const nvca_pixel_layout *yuv = nullptr);   // its pre-processing half alone
int get_resize_plan(nvca_ctx *ctx, int sw, int sh, int dw, int dh, GeomPlan **out);

// ---- host_copy.cpp
hipStream_t stream_of_id(const nvca_ctx *ctx, int id);       // the stream a bit of HostRangeTable's stream mask stands for
void ensure_pool(nvca_ctx *ctx);                             // the context's helper threads, created on first use
int stage_2d(nvca_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width_bytes, size_t height, int mem);
int unstage_2d(nvca_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width_bytes, size_t height, int mem);
int finish_device_op(nvca_ctx *ctx);
int check_img(nvca_ctx *ctx, const void *p, int w, int h, int stride, int bpp, int mem);
// 4:2:0 frames (nvca_pixel_layout): a w x h frame against its layout (NVCA_ERR_ARG with an error text) and the layout as the kernels
// read it (null / BGR: fmt 0); the bytes from its base to the end of its last plane: yuv_layout.h's yuv_extent
int check_yuv_layout(nvca_ctx *ctx, const nvca_pixel_layout &l, int w, int h);      // (ctx may be null: no error text then)
YuvPlanes yuv_planes(const nvca_pixel_layout *l);
// what every nvca_*_set_input and every 4:2:0 stream's frame check share: the caller's layout as a stream keeps it, layouts by value,
// a frame against its stream's layout, a host frame's planes to the device at the caller's offsets
int parse_pixel_layout(nvca_ctx *ctx, const nvca_pixel_layout *layout, nvca_pixel_layout &out);
int check_yuv_frame(nvca_ctx *ctx, const nvca_pixel_layout &l, const nvca_frame &f);     // (ctx may be null)
int caller_h2d_planes(nvca_ctx *ctx, void *dst, const void *src, const nvca_pixel_layout &l, int w, int h, hipStream_t st);
size_t staging_need(const nvca_frame *frames, const int *idx, int n, const nvca_pixel_layout *yuv = nullptr);
int stage_frames(nvca_ctx *ctx, const nvca_frame *frames, const int *idx, int n, int bpp, int r0 = 0, hipStream_t st = nullptr,
                 size_t *off_io = nullptr, const RowCopy *rows = nullptr, const nvca_pixel_layout *yuv = nullptr);
bool frames_aligned4(const nvca_frame *frames, const int *idx, int n);
bool frames_yuv_aligned16(const nvca_frame *frames, const int *idx, int n, const nvca_pixel_layout &l);

// ---- detectMultiScale jobs (detect_job.cpp, detect_rounds.cpp) and their small-image batches (roi_batch.cpp)
enum JobKind { kJobPlain = 0, kJobScaleImage = 1, kJobBiggest = 2, kJobLbp = 3, kJobKinds = 4 };       // scale-cascade scan, CV_HAAR_SCALE_IMAGE, CV_HAAR_FIND_BIGGEST_OBJECT, a new-format cascade, LBP or HAAR (whatever the flags)
enum JobPhase { kJobNew = 0, kJobFirstQueued = 1, kJobNarrowedQueued = 2, kJobDone = 3 };      // (narrowed: the second set of a FIND_BIGGEST search)

struct DetectJob {
    struct Request {
        JobKind kind = kJobPlain;
        const nvca_cascade *casc = nullptr;
        const void *img[kJobImages] = {nullptr}; int nimg = 1;       // plain scan / SCALE_IMAGE / LBP: images of one geometry share the launches
        int cols = 0, rows = 0, stride = 0, mem = 0;
        double sf = 1.1; int min_neighbors = 0, flags = 0, minw = 0, minh = 0, maxw = 0, maxh = 0;
        bool raw_only = false;
        bool small_route = false;                            // a new-format HAAR cascade: its small-route flag when the job was built (nvca_cascade_set_small_route)
        bool image_axis = false;                             // a job of the _batch entry points on an LBP cascade: its images, however many, share the large-image evaluator's launches
        bool levels = false;                                 // outputRejectLevels: one image, a new-format cascade of four stages or more, always the large-image evaluator
    } rq;
    std::vector<nvca_rect> out[kJobImages];          // the result, per image
    std::vector<int> out_levels; std::vector<double> out_weights;      // a levels job: rejectLevels / levelWeights of out[0]
    // progress of the queued launch set
    struct Queued {
        JobPhase phase = kJobNew;
        GeomPlan *gp = nullptr;                          // cached plan of the queued set (kept from eviction while queued)
        std::unique_ptr<DetectPlan> own;                 // FIND_BIGGEST: this call's narrowed plan
        DetectPlan *dp = nullptr;                        // plan of the queued set (null: nothing was queued)
        CascadeJob cj; int gthr = 0;
        int regrown = 0;                                 // launch sets re-run with a larger candidate list (at most one per set)
    } q;
    int slots() const { return rq.nimg; }
    FbSearch fb;                                     // FIND_BIGGEST: the serial loop between the two sets
    // small-image path (kernels_roi.hip): the job's steps of the queued launch and the candidates that came back
    struct RoiStepInfo { double ystep, out_factor; int winw, winh, ladder; };
    struct RejInfo { int off, wpr, nx, ny; };        // where a step's stage-0 reject bits lie in the launch's bitmap (word offset, words per grid row, grid size)
    struct SmallPath {
        bool small = false;                              // the job runs on the small-image path (decided at its first round)
        bool fused = false;                              // the queued set went into the round's k_roi launch
        int roi_prev_phase = 0;                          // its phase before the queued set (a set that overflowed the list is queued again); -1: advanced by a helper thread
        std::vector<RoiStepInfo> rinfo;                  // [step of the launch]
        std::vector<unsigned> rkeys[kJobImages];         // per image: step << 26 | iy << 13 | ix, ascending (= OpenCV's serial order)
        // FIND_BIGGEST with Switches::fb_dense: the queued launch was a dense one (FbSearch: dense first set).  The reject bits it hands to
        // the search stay in the launch's page-locked bitmap: valid until the next launch of its buffer set, and the job is advanced before
        bool dense = false;
        std::vector<RejInfo> rej_info;                   // [step of the launch]
    } sm;
};

struct RoiBatch {
    std::vector<RoiJobDev> jobs; std::vector<RoiStep> steps, lbp_steps /* k_roi_lbp's: the LBP jobs' */, hnew_steps /* k_roi_hnew's: the opted-in new-format HAAR jobs' */; std::vector<unsigned char> tabs; std::vector<DetectJob *> owners; std::vector<int> owner_img;
    std::vector<ScaleTable *> held;                 // stump tables of the launch: kept from eviction until it has been collected
    int plane_words = 0, lev_bytes = 0, lane = 0; unsigned cap = 0; size_t first = 0;
    int lbp_plane_words = 0, lbp_lev_bytes = 0;     // k_roi_lbp's LDS: the largest level's sum plane (words, a multiple of 4) and resized level (bytes)
    int hnew_plane_words = 0;                       // k_roi_hnew's: the largest level's plane (words, a multiple of 4; the sum and the squared plane have this size each)
    size_t rej_words = 0;                           // stage-0 reject bitmaps of the launch's dense steps (u64 words)
    void release() { for (ScaleTable *t : held) if (t->refs > 0) t->refs--; held.clear(); }
    ~RoiBatch() { release(); }
    RoiBatch() = default;
    RoiBatch(const RoiBatch &) = delete; RoiBatch &operator=(const RoiBatch &) = delete;
    // (a round object is reused from round to round: what the previous round held is released first)
    void reset() { release(); jobs.clear(); steps.clear(); lbp_steps.clear(); hnew_steps.clear(); tabs.clear(); owners.clear(); owner_img.clear(); plane_words = 0; lev_bytes = 0; lbp_plane_words = 0; lbp_lev_bytes = 0; hnew_plane_words = 0; lane = 0; cap = 0; first = 0; rej_words = 0; }
};

// ---- roi_batch.cpp
bool roi_eligible(const nvca_ctx *ctx, const DetectJob &j, int njobs_in_round);
int roi_add_job(nvca_ctx *ctx, RoiBatch &rb, DetectJob &j);
int roi_launch(nvca_ctx *ctx, RoiBatch &rb, bool full_cap);
int roi_collect(nvca_ctx *ctx, RoiBatch &rb);
// the candidates roi_collect handed a job, in the serial order, as rectangles (sc: their ladder steps)
int roi_job_candidates(nvca_ctx *ctx, DetectJob &j, std::vector<std::vector<nvca_rect>> &raw, std::vector<char> &grouped, std::vector<std::vector<int>> &sc);

// ---- pyramid.cpp: a plan's pyramid (layout: pyr_levels.h) on the device, and a job's images resized to its levels and integrated
int pyr_plan_tabs(nvca_ctx *ctx, GeomPlan &np, int cols, int rows, const std::vector<SiLevel> &levels);      // layout and resize tables
int pyr_upload_levels(nvca_ctx *ctx, GeomPlan &np);                                                         // the device level table
int pyr_plan_init(nvca_ctx *ctx, GeomPlan &np, int cols, int rows, const std::vector<SiLevel> &levels);      // both, one after the other
ScaleSpec level_spec(int P, const PyrLevel &L, int ow, int oh, int adaptive);                                // a level's scan grid
bool job_images_in_place(const DetectJob &j, size_t *slot);
// The images a pyramid is built from: image k at img + k * slot, rows `pitch` bytes apart.  luts: null, or a 256-byte table per image that
// every sample is read through -- the gray slots and LUTs a face stream's lane holds (the equalised working image is never written out).
struct PyrSource { const uint8_t *img; int pitch; size_t slot; const uint8_t *luts; };
int pyr_job_source(nvca_ctx *ctx, const DetectJob &j, PyrSource &src);       // a job's images: in place, or staged into the lane's gray slots
int pyr_build(nvca_ctx *ctx, const PyrSource &src, int cols, int rows, int nimg, GeomPlan *pp, bool has_tilted);

// ---- lbp_job.cpp: the cached plan and the launch set of a new-format scan (the evaluator by the cascade's format: LBP or HAAR), for a
// detectMultiScale job and for a face stream's chunk
int lbp_plan(nvca_ctx *ctx, const nvca_cascade *casc, int cols, int rows, double sf, int minw, int minh, int maxw, int maxh, GeomPlan **out);
// pyramid of `nimg` images of `src`, the evaluator, and -- group_thr given ([nimg] groupRectangles thresholds) and device grouping
// allowed -- k_group on the candidate keys; the job's result slots are cj.r0 .. cj.r0 + nimg of cj.total.  early_done: recorded behind the
// evaluator's launches.  Collected with cascade_collect(pp->det).  levels (outputRejectLevels; without group_thr): the
// stage groups end in front of the last three stages, which ONE launch evaluates on every window left, emitting each with a LevelRec
// (cj.d_recs); the plan is the plain scan's.
int lbp_launch_set(nvca_ctx *ctx, GeomPlan *pp, const PyrSource &src, int cols, int rows, int nimg, CascadeJob &cj,
                   const int *group_thr = nullptr, hipEvent_t early_done = nullptr, bool levels = false);
int lbp_enqueue(nvca_ctx *ctx, DetectJob &j, int r0, int total);              // the launch set of a job on a new-format LBP cascade

// ---- detect_job.cpp
int detect_job_enqueue(nvca_ctx *ctx, DetectJob &j, int r0, int total);       // queue the job's next launch set
int detect_job_advance(nvca_ctx *ctx, DetectJob &j);                          // after the stream has drained: consume what the set produced

} // namespace nvca
