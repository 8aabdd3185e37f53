// launch.h -- what a kernel file sees of the library: the launch macro and the launch_* function of every kernel, over the
// device records and the pixel rules.  Nothing of the context.  A launch that resizes takes its geometry as one ResizeView
// (device_records.h; GeomPlan::view() for a cached plan, ResizeView{} for the identity) and computes every destination sample
// with pixel_rules.h's resize_sample.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "device_records.h"
#include "trk_layout.h"
#include "pixel_rules.h"

namespace nvca {

bool launch_events(hipEvent_t *a, hipEvent_t *b);      // event pair for the next launch of the current scope, if any
// A refused launch (bad configuration, LDS grant missing) is not sticky: the status is read right behind the launch and the
// FIRST failure of the calling thread is kept, with the kernel's name, until the entry point's next NVCA_LAUNCH_CHECK turns it
// into NVCA_ERR_HIP -- a kernel that did not run never hands stale buffers to the host logic as if they were results.
void note_launch(const char *kernel);                  // reads hipGetLastError()
hipError_t take_launch_error(const char **kernel);     // returns and clears the thread's first recorded failure
#define NVCA_LAUNCH(kern, grid, block, shmem, st, ...)                                                            \
    do {                                                                                                          \
        hipEvent_t ea__, eb__;                                                                                    \
        if (nvca::launch_events(&ea__, &eb__)) hipExtLaunchKernelGGL(kern, grid, block, shmem, st, ea__, eb__, 0, __VA_ARGS__); \
        else hipLaunchKernelGGL(kern, grid, block, shmem, st, __VA_ARGS__);                                       \
        nvca::note_launch(#kern);                                                                                 \
    } while (0)

// --------------------------------------------------------------------------
// Kernel launch wrappers (kernels_gray.hip / kernels_equalize.hip / kernels_integral.hip / kernels_cascade_*.hip / kernels_group.hip)
// --------------------------------------------------------------------------
// src[b] pointers are passed as a device array of pointers (frames need not be contiguous)
void launch_gray(hipStream_t st, const uint8_t *const *d_src, const PreGeom &g, const ResizeView &t,
                 uint8_t *gray, unsigned *hist, int batch, bool aligned4);
// the same for a 4:2:0 frame (planes `p`); aligned16: every plane and stride of every frame takes 16-byte (I420 chroma: 8-byte) loads.
// Returns whether k_gray_yuv16 took the launch (identity geometry and aligned16) and not k_gray_yuv_generic.  A packed 4:2:2 frame
// (p.fmt NVCA_PIX_YUY2 / _UYVY / _YVYU; aligned16: base, offset and stride take 16-byte loads): k_gray_yuv422_16 / k_gray_yuv422_generic.
bool launch_gray_yuv(hipStream_t st, const uint8_t *const *d_src, const PreGeom &g, const YuvPlanes &p, const ResizeView &t,
                     uint8_t *gray, unsigned *hist, int batch, bool aligned16);
const char *gray_yuv_kernel_name(int fmt, bool wide);       // the kernel launch_gray_yuv ran (the plan_debug lines name it)
void launch_yuv420_to_bgr(hipStream_t st, const uint8_t *src, int w, int h, int ystride, const YuvPlanes &p, uint8_t *dst, int dstride);
void launch_yuv422_to_bgr(hipStream_t st, const uint8_t *src, int w, int h, int sstride, const YuvPlanes &p, uint8_t *dst, int dstride);
void launch_pyr_resize(hipStream_t st, const uint8_t *src, int sw, int sh, int sstride, size_t src_slot, const PyrLevelDev *levels,
                       int nlev, int nimg, int maxw, int maxh, uint8_t *aux, size_t aux_slot,
                       const uint8_t *luts = nullptr /* [nimg][256]: the pyramid of lut[img][image]; null: of the image */);
void launch_pyr_integral(hipStream_t st, const uint8_t *aux, size_t aux_slot, const PyrLevelDev *levels, int nlev, int nimg,
                         int *sum, unsigned *sq32, size_t sum_slot, int P);
void launch_resize1(hipStream_t st, const uint8_t *src, int sw, int sh, int sstride, const ResizeView &t,
                    uint8_t *dst, int dw, int dh, int dstride, unsigned *hist, int batch = 1, size_t src_slot = 0, size_t dst_slot = 0,
                    const uint8_t *luts = nullptr /* [batch][256]: image z is read through its LUT */);
void launch_resize3(hipStream_t st, const uint8_t *src, int sw, int sh, int sstride, const ResizeView &t,
                    uint8_t *dst, int dw, int dh, int dstride);
void launch_flip_h(hipStream_t st, const uint8_t *src, int w, int h, int spitch, uint8_t *dst, int dpitch, int batch = 1, size_t src_slot = 0,
                   size_t dst_slot = 0);
void launch_hist(hipStream_t st, const uint8_t *gray, int w, int h, int pitch, unsigned *hist);
void launch_lut(hipStream_t st, unsigned *hist, int total, uint8_t *lut, int batch, int rezero = 0,
                unsigned long long *zero_a = nullptr, unsigned long long *zero_b = nullptr);
void launch_apply_lut(hipStream_t st, const uint8_t *src, int w, int h, int spitch, const uint8_t *lut,
                      uint8_t *dst, int dpitch, int batch = 1, size_t src_slot = 0, size_t dst_slot = 0);
void launch_work_resize(hipStream_t st, bool bgr, const uint8_t *const *d_srcs, const int *d_lut_idx, const uint8_t *d_luts, int sh, int sstride,
                        const ResizeView &t, uint8_t *dst, int dw, int dh, int dstride, size_t dst_slot, unsigned *hist, int batch, const YuvPlanes *yuv = nullptr);
void launch_colsum(hipStream_t st, const uint8_t *gray, const uint8_t *lut, int lut_stride, const PreGeom &g,
                   unsigned *bandsum, unsigned *bandsq, int batch);
void launch_bandscan(hipStream_t st, const PreGeom &g, unsigned *bandsum, unsigned *bandsq, int batch);
void launch_integral(hipStream_t st, const uint8_t *gray, const uint8_t *lut, int lut_stride, const PreGeom &g,
                     const unsigned *bandsum, const unsigned *bandsq, int *sum, unsigned long long *sqsum,
                     int batch);

// integral pair of small images (rows x cols fit 64 KiB of LDS) in one launch, one workgroup per image
bool small_integral_fits(const PreGeom &g);
void launch_small_integral(hipStream_t st, const uint8_t *gray, const uint8_t *lut, int lut_stride, const PreGeom &g, int *sum,
                           unsigned long long *sqsum, int batch);

// ---- tracker (kernels_trk_pixel.hip, kernels_trk_ccl.hip).  One launch set: `batch` slots of one size and format.  Every buffer's
// layout is trk_layout.h's: flags (a byte per 256-pixel row segment and slot, set by the pixel pass where the motion history holds
// anything -- the component kernels leave the other segments alone: a static scene with a few moving objects is mostly such segments --
// and the live-segment counts), tiles (the live-tile list), roots (the folded path's tile roots), out (the component list).
struct TrkLaunch {
    const TrkSlot *slots; int batch, w, h;
    int fmt;                      // 0 BGRA frames, 1 / 2: NV12 / I420 frames, planes per slot; 4 .. 6: packed 4:2:2 (NVCA_PIX_YUY2 / _UYVY / _YVYU)
    bool wide;                    // every slot takes the wide pixel kernel's loads (k_trk_pixel4 / k_trk_pixel_yuv8 / k_trk_pixel_yuv422x4; trk_host.h, trk_wide_ok)
    int *labels; CompAcc *acc;    // [batch][h][w] parent words / per-root records
    int *out; int cap;            // component list and the components it holds
    uint8_t *flags; int *roots; int roots_cap; int *tiles; int tick;
    int order;                    // Switches::trk_order
    int rows, rows_uf;            // rows a block of the per-pixel component kernels walks (NVCA_CCL_ROWS / NVCA_CCL_ROWS_UF; <= kCclRowsMax)
};
enum TrkRoute {
    kTrkPixelOnly,                // the pixel pass alone: no slot has a previous frame
    kTrkFolded,                   // pixel pass, then tile / border / fold / emit
    kTrkPerPixel,                 // pixel pass, then tile / border / flatten / reduce / collect (NVCA_TRK_FOLD=0)
    kTrkPerPixelAlone,            // the latter without the pixel pass, on the history an earlier launch left (kTrkFolded's root list overflowed)
};
void launch_trk_pixel(hipStream_t st, const TrkLaunch &L);
void launch_trk_components(hipStream_t st, const TrkLaunch &L, TrkRoute route);
inline void launch_tracker(hipStream_t st, const TrkLaunch &L, TrkRoute route)
{
    if (route != kTrkPerPixelAlone) launch_trk_pixel(st, L);
    if (route != kTrkPixelOnly) launch_trk_components(st, L, route);
}

// One launch per kernel; each is a no-op when the plan has no work for its kernel (no tasks, no tiles / bands / strips, no late stage).
void launch_stage0(hipStream_t st, const CascadeArgs &a, int batch);        // kernels_cascade_gather.hip
void launch_strip(hipStream_t st, const CascadeArgs &a, int batch);
// general cascades: variance + stage 0 for every window (reject bits + normaliser), then the remaining stages on the visited
// stage-0 survivors, window per lane
void launch_gen_stage0(hipStream_t st, const CascadeArgs &a, int batch);
void launch_gen_rest(hipStream_t st, const CascadeArgs &a, int batch);
// lds_grant: the calling context's record of the dynamic LDS already granted to k_tile ([0]) / k_band ([1]); returns a
// hipError_t (as int) when the grant is refused, 0 otherwise
int launch_tile(hipStream_t st, const CascadeArgs &a, int batch, int *lds_grant);      // kernels_cascade_tile.hip
int launch_band(hipStream_t st, const CascadeArgs &a, int batch, int *lds_grant);
void launch_deep(hipStream_t st, const CascadeArgs &a, int batch);          // kernels_cascade_deep.hip
// groupRectangles per frame on the device; out: [batch][2 + 4*out_cap] ints: count (-1 = host must group), raw count, boxes
void launch_group(hipStream_t st, const CascadeArgs &a, const int *group_thr, int *out, int out_cap, int batch);     // kernels_group.hip
// ---- new-format LBP cascades (kernels_cascade_lbp.hip): stage 0 of every grid position (pass bits), the serial walk's skip rule
// per row + compaction of the visited survivors, then stages [s0, s1) on the survivors of list `in` (count cnt[in_cnt]) -- into the
// other list and cnt[in_cnt + 1], or, when s1 is the last stage, into the candidate list.  lds: stage-0 tile bytes (0: gather from global)
// All three serve the a.nimg images of a job in one launch: grid.y, a lane per (image, row), one survivor list for all images.
void launch_lbp_stage0(hipStream_t st, const LbpArgs &a, int lds);
void launch_lbp_walk(hipStream_t st, const LbpArgs &a);
void launch_lbp_rest(hipStream_t st, const LbpArgs &a, int s0, int s1, int in, int in_cnt, unsigned max_items);
// ---- new-format HAAR cascades (kernels_cascade_hnew.hip): the same scan with the Haar evaluator -- its stage 0 and its stage groups
// around launch_lbp_walk(a.l), which reads the pass bits alone
void launch_hnew_stage0(hipStream_t st, const HnewArgs &a, int lds);
void launch_hnew_rest(hipStream_t st, const HnewArgs &a, int s0, int s1, int in, int in_cnt, unsigned max_items);
// ---- outputRejectLevels on either evaluator: the last three stages on the survivors of list `in` (count cnt[in_cnt]);
// every one of them goes to the candidate list, its LevelRec to recs (a.hit_cap records) under the same index
void launch_lbp_levels(hipStream_t st, const LbpArgs &a, LevelRec *recs, int in, int in_cnt, unsigned max_items);
void launch_hnew_levels(hipStream_t st, const HnewArgs &a, LevelRec *recs, int in, int in_cnt, unsigned max_items);
// ---- general new-format HAAR cascades (kernels_cascade_hgen.hip: trees, tilted features): the same three launches on HgenArgs
void launch_hgen_stage0(hipStream_t st, const HgenArgs &g, int lds);
void launch_hgen_rest(hipStream_t st, const HgenArgs &g, int s0, int s1, int in, int in_cnt, unsigned max_items);
void launch_hgen_levels(hipStream_t st, const HgenArgs &g, LevelRec *recs, int in, int in_cnt, unsigned max_items);
// ---- image-to-overlay and view-* outlines on a device frame (kernels_draw.hip)
void launch_overlay(hipStream_t st, uint8_t *frame, int W, int H, int stride, const OverlayPlace &p, const OverlayImage &o);
void launch_draw_shapes(hipStream_t st, uint8_t *data, int w, int h, int stride, int channels, const nvca_shape *d_shapes, int n,
                        int bx0, int by0, int bx1, int by1);
// ---- the way out in 4:2:0 (kernels_yuv_out.hip): cv::cvtColor(CV_BGR2YUV_I420) into the planes of a layout, and the two drawing kernels
// on a 4:2:0 device frame.  aligned16: the source, its stride and every plane and stride of the layout take the wide kernel's accesses;
// returns whether k_bgr_yuv16 took the launch (that, 3 channels and w % 16 == 0) and not k_bgr_yuv_generic.
bool launch_bgr_to_yuv420(hipStream_t st, const uint8_t *src, int w, int h, int sstride, int cn, uint8_t *base, int ystride, const YuvPlanes &p, bool aligned16);
// chroma blocks [cx0, cx1] x [cy0, cy1] of the frame; uv2: an NV12 pair may be written with one 2-byte store
void launch_draw_shapes_yuv(hipStream_t st, uint8_t *base, int ystride, const YuvPlanes &p, const nvca_shape *d_shapes, int n,
                            int cx0, int cy0, int cx1, int cy1, bool uv2);
void launch_overlay_yuv(hipStream_t st, uint8_t *base, int W, int H, int ystride, const YuvPlanes &yp, const OverlayPlace &p, const OverlayImage &o,
                        int cx0, int cy0, int cx1, int cy1);
// tilted integral (cv::integral's third plane) of `batch` images / of every pyramid level: one workgroup per image
void launch_tilted(hipStream_t st, const uint8_t *gray, const uint8_t *lut, int lut_stride, const PreGeom &g, int *tilted, int batch);
void launch_pyr_tilted(hipStream_t st, const uint8_t *aux, size_t aux_slot, const PyrLevelDev *levels, int nlev, int nimg,
                       int *tilted, size_t sum_slot, int P, int maxw, int maxh);
// ---- detectMultiScale on a small image in one workgroup (kernels_roi.hip)
void launch_roi(hipStream_t st, const RoiJobDev *jobs, int nsteps, const RoiStep *steps, const unsigned char *tabs, unsigned long long *hits,
                unsigned hit_cap, int plane_words, int lds_bytes, unsigned long long *rej);
#ifdef NVCA_STAMPS
void roi_stamps_dump(const char *path);     // diagnostic build: k_roi's phase sums as text
#endif
int roi_grant_lds(int bytes);     // dynamic LDS above 64 KiB is granted per function and device (monotonic, process-wide); returns a hipError_t as int
// ---- ... of a new-format LBP cascade (kernels_roi_lbp.hip): the same job table, candidate list and key as k_roi, its own step records
void launch_roi_lbp(hipStream_t st, const RoiJobDev *jobs, int nsteps, const RoiStep *steps, const unsigned char *tabs, unsigned long long *hits,
                    unsigned hit_cap, int plane_words, int lds_bytes);
int roi_lbp_grant_lds(int bytes);
// ---- ... of a new-format HAAR cascade that was opted in (kernels_roi_hnew.hip): likewise, its LDS sized by roi_hnew_lds_bytes
void launch_roi_hnew(hipStream_t st, const RoiJobDev *jobs, int nsteps, const RoiStep *steps, const unsigned char *tabs, unsigned long long *hits,
                     unsigned hit_cap, int plane_words, int lds_bytes);
int roi_hnew_grant_lds(int bytes);

} // namespace nvca
