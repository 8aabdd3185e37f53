// detect.cpp -- the detectMultiScale entry points of the ABI: one job (detect_job.cpp) run to completion (detect_rounds.cpp), or, for
// a batch of images of one geometry, as few jobs as hold them, run to completion together.
#include "host_state.h"
#include "host_logic.h"
#include <algorithm>
#include <memory>

using namespace nvca;

extern "C" {

static int detect_gray(nvca_ctx *ctx, const nvca_cascade *casc, const void *gray, int w, int h, int stride, int mem,
                       double sf, int min_neighbors, int flags, int minw, int minh, int maxw, int maxh, bool raw_only,
                       std::vector<nvca_rect> &out)
{
    NVCA_LOCK_OR_FAIL(ctx);
    DetectJob j;
    int rc = make_detect_job(ctx, j, casc, gray, w, h, stride, mem, sf, min_neighbors, flags, minw, minh, maxw, maxh, raw_only);
    if (rc) return rc;
    DetectJob *jp = &j;
    if ((rc = run_detect_jobs(ctx, &jp, 1, nullptr))) return rc;
    out.swap(j.out[0]);
    return NVCA_OK;
}

int nvca_detect_multiscale(nvca_ctx *ctx, const nvca_cascade *cascade, const void *gray, int w, int h, int stride,
                           int mem, double scale_factor, int min_neighbors, int flags, int min_w, int min_h,
                           int max_w, int max_h, nvca_rect *out, int cap, int *n_out)
try {
    if (!n_out || cap < 0 || (cap > 0 && !out)) return NVCA_ERR_ARG;
    std::vector<nvca_rect> r;
    int rc = detect_gray(ctx, cascade, gray, w, h, stride, mem, scale_factor, min_neighbors, flags, min_w, min_h, max_w,
                         max_h, false, r);
    if (rc) return rc;
    *n_out = (int)r.size();
    for (int i = 0; i < std::min<int>(cap, (int)r.size()); i++) out[i] = r[i];
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)

int nvca_detect_raw(nvca_ctx *ctx, const nvca_cascade *cascade, const void *gray, int w, int h, int stride, int mem,
                    double scale_factor, int flags, int min_w, int min_h, int max_w, int max_h, nvca_rect *out,
                    int cap, int *n_out)
try {
    if (!n_out || cap < 0 || (cap > 0 && !out)) return NVCA_ERR_ARG;
    if ((flags & NVCA_HAAR_FIND_BIGGEST_OBJECT) && !(cascade && cascade->new_format())) return NVCA_ERR_ARG;       // (a new-format cascade's scan ignores flags)
    std::vector<nvca_rect> r;
    int rc = detect_gray(ctx, cascade, gray, w, h, stride, mem, scale_factor, 0, flags, min_w, min_h, max_w, max_h, true, r);
    if (rc) return rc;
    *n_out = (int)r.size();
    for (int i = 0; i < std::min<int>(cap, (int)r.size()); i++) out[i] = r[i];
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)

// cv::CascadeClassifier::detectMultiScale(image, objects, rejectLevels, levelWeights, scaleFactor, minNeighbors, flags, minSize, maxSize,
// outputRejectLevels = true): one job with Request::levels, on a new-format cascade of four stages or more
static int detect_gray_levels(nvca_ctx *ctx, const nvca_cascade *casc, const void *gray, int w, int h, int stride, int mem, double sf,
                              int min_neighbors, int flags, int minw, int minh, int maxw, int maxh, bool raw_only,
                              nvca_rect *out, int *reject_levels, double *level_weights, int cap, int *n_out)
{
    if (!n_out || cap < 0 || (cap > 0 && (!out || !reject_levels || !level_weights))) return NVCA_ERR_ARG;
    NVCA_LOCK_OR_FAIL(ctx);
    DetectJob j;
    int rc = make_detect_job(ctx, j, casc, gray, w, h, stride, mem, sf, min_neighbors, flags, minw, minh, maxw, maxh, raw_only);
    if (rc) return rc;
    const size_t nstages = casc->format == NVCA_CASCADE_LBP ? casc->lbp.stages.size() : casc->format == NVCA_CASCADE_HAAR_NEW ? casc->hnew.stages.size() : 0;
    if (!casc->new_format() || nstages < 4) {
        ctx->set_error("reject levels: a new-format cascade of four stages or more (with fewer, stage-0 rejects would be emitted)");
        return NVCA_ERR_UNSUPPORTED;
    }
    j.rq.levels = true;
    DetectJob *jp = &j;
    if ((rc = run_detect_jobs(ctx, &jp, 1, nullptr))) return rc;
    const size_t n = j.out[0].size();
    *n_out = (int)n;
    for (size_t i = 0; i < std::min<size_t>((size_t)cap, n); i++) { out[i] = j.out[0][i]; reject_levels[i] = j.out_levels[i]; level_weights[i] = j.out_weights[i]; }
    return NVCA_OK;
}

int nvca_detect_raw_levels(nvca_ctx *ctx, const nvca_cascade *cascade, const void *gray, int w, int h, int stride, int mem,
                           double scale_factor, int flags, int min_w, int min_h, int max_w, int max_h, nvca_rect *out,
                           int *reject_levels, double *level_weights, int cap, int *n_out)
try {
    return detect_gray_levels(ctx, cascade, gray, w, h, stride, mem, scale_factor, 0, flags, min_w, min_h, max_w, max_h, true, out,
                              reject_levels, level_weights, cap, n_out);
}
NVCA_API_CATCH(ctx)

int nvca_detect_multiscale_levels(nvca_ctx *ctx, const nvca_cascade *cascade, const void *gray, int w, int h, int stride, int mem,
                                  double scale_factor, int min_neighbors, int flags, int min_w, int min_h, int max_w, int max_h,
                                  nvca_rect *out, int *reject_levels, double *level_weights, int cap, int *n_out)
try {
    return detect_gray_levels(ctx, cascade, gray, w, h, stride, mem, scale_factor, min_neighbors, flags, min_w, min_h, max_w, max_h, false,
                              out, reject_levels, level_weights, cap, n_out);
}
NVCA_API_CATCH(ctx)

// n images of one geometry: jobs of up to kJobImages images (a FIND_BIGGEST search carries one: its launch sets depend on what it
// finds), all of them handed to ONE run_detect_jobs call -- a round of the whole batch has one wait.  Image i answers into
// out[i * cap ...], n_out[i] is its full count.
static int detect_gray_batch(nvca_ctx *ctx, const nvca_cascade *casc, int n, const void *const *gray, int w, int h, int stride, int mem,
                             double sf, int min_neighbors, int flags, int minw, int minh, int maxw, int maxh, bool raw_only,
                             nvca_rect *out, int cap, int *n_out)
{
    NVCA_LOCK_OR_FAIL(ctx);
    if (n < 0 || !n_out || cap < 0 || (cap > 0 && !out) || (n > 0 && !gray) || !(sf > 1.0)) return NVCA_ERR_ARG;
    for (int i = 0; i < n; i++) if (!gray[i]) return NVCA_ERR_ARG;
    if (n == 0) return NVCA_OK;
    std::vector<std::unique_ptr<DetectJob>> jobs;
    std::vector<DetectJob *> jp;
    for (int i = 0; i < n; i++) {
        if (jobs.empty() || detect_job_add_image(jobs.back().get(), gray[i]) < 0) {          // (full, or a kind that carries one image)
            jobs.emplace_back(new DetectJob());
            const int rc = make_detect_job(ctx, *jobs.back(), casc, gray[i], w, h, stride, mem, sf, min_neighbors, flags, minw, minh, maxw, maxh, raw_only);
            if (rc) return rc;
            jobs.back()->rq.image_axis = true;             // (a batch's launch set does not depend on how many images its last job holds)
            jp.push_back(jobs.back().get());
        }
    }
    const int rc = run_detect_jobs(ctx, jp.data(), (int)jp.size(), nullptr);
    if (rc) return rc;
    int i = 0;
    for (const DetectJob *j : jp)
        for (int k = 0; k < j->rq.nimg; k++, i++) {
            const std::vector<nvca_rect> &r = j->out[k];
            n_out[i] = (int)r.size();
            std::copy(r.begin(), r.begin() + std::min<size_t>((size_t)cap, r.size()), out + (size_t)i * cap);
        }
    return NVCA_OK;
}

int nvca_detect_multiscale_batch(nvca_ctx *ctx, const nvca_cascade *cascade, int n, const void *const *gray, int w, int h, int stride,
                                 int mem, double scale_factor, int min_neighbors, int flags, int min_w, int min_h, int max_w,
                                 int max_h, nvca_rect *out, int cap, int *n_out)
try {
    return detect_gray_batch(ctx, cascade, n, gray, w, h, stride, mem, scale_factor, min_neighbors, flags, min_w, min_h, max_w, max_h,
                             false, out, cap, n_out);
}
NVCA_API_CATCH(ctx)

int nvca_detect_raw_batch(nvca_ctx *ctx, const nvca_cascade *cascade, int n, const void *const *gray, int w, int h, int stride, int mem,
                          double scale_factor, int flags, int min_w, int min_h, int max_w, int max_h, nvca_rect *out, int cap,
                          int *n_out)
try {
    if ((flags & NVCA_HAAR_FIND_BIGGEST_OBJECT) && !(cascade && cascade->new_format())) return NVCA_ERR_ARG;       // (as nvca_detect_raw)
    return detect_gray_batch(ctx, cascade, n, gray, w, h, stride, mem, scale_factor, 0, flags, min_w, min_h, max_w, max_h, true, out,
                             cap, n_out);
}
NVCA_API_CATCH(ctx)

int nvca_group_rectangles(nvca_ctx *ctx, nvca_rect *rects, int n, int group_threshold, double eps, int *n_out)
try {
    NVCA_LOCK_OR_FAIL(ctx);
    if (!ctx || n < 0 || (n > 0 && !rects) || !n_out) return NVCA_ERR_ARG;
    std::vector<nvca_rect> v(rects, rects + n);
    group_rectangles(v, group_threshold, eps);
    for (size_t i = 0; i < v.size(); i++) rects[i] = v[i];
    *n_out = (int)v.size();
    return NVCA_OK;
}
NVCA_API_CATCH(ctx)

} // extern "C"
