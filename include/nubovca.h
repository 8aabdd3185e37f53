/*
 * nubovca.h -- C ABI of libnubovca_hip: the MI355X (gfx950) implementation of
 * NUBOMEDIA-VCA's per-frame Haar detection hot path.
 *
 * Every entry point replaces a call the reference makes into OpenCV 2.4 (or a
 * static function of the reference's GStreamer elements); the reference site
 * each one replaces is cited as file:line relative to the reference tree, with
 *   FACE/ = modules/nubo_face/nubo-face-detector/src/gst-plugins/
 *   TRK/  = modules/nubo_tracker/nubo-tracker/src/gst-plugins/
 *   EYE/ NOSE/ MOUTH/ EAR/ analogous.
 *
 * Conventions: plain C types only; opaque handles; the caller owns all frame
 * memory; the library owns device state.  Every function returns an int status
 * (NVCA_OK == 0, < 0 error) and never throws: every entry point is a function-try-block
 * (csrc/context.h, NVCA_API_CATCH) that turns std::bad_alloc / std::length_error into NVCA_ERR_NOMEM and anything
 * else into NVCA_ERR_INTERNAL -- the reference never lets a frame error out of the element either
 * (FACE/kmsfacedetect.cpp:897 always returns GST_FLOW_OK).  A handle may be used by one
 * thread at a time; distinct contexts may be used concurrently.  There is no
 * CPU fallback: without a HIP device nvca_ctx_create fails.
 */
#ifndef NUBOVCA_H
#define NUBOVCA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NVCA_OK              0
#define NVCA_ERR_ARG        -1   /* bad argument                                   */
#define NVCA_ERR_NO_DEVICE  -2   /* no HIP device / device id out of range         */
#define NVCA_ERR_HIP        -3   /* a HIP runtime call failed (see nvca_last_error)*/
#define NVCA_ERR_IO         -4   /* cascade file unreadable                        */
#define NVCA_ERR_PARSE      -5   /* cascade XML malformed                          */
#define NVCA_ERR_UNSUPPORTED -6  /* tree-structured STAGE graph (parent / next), or a
                                    feature that leaves the image at some scale; a
                                    new-format cascade that is not LBP with stumps; an
                                    LBP cascade handed to nvca_face_stream_create or
                                    nvca_part_stream_create (their _create_any forms
                                    take it)                                         */
#define NVCA_ERR_OVERFLOW   -7   /* more raw candidates than the context's cap     */
#define NVCA_ERR_NOMEM      -8
#define NVCA_ERR_INTERNAL   -9   /* an internal check failed (a device result out of range, an exception caught at the
                                    ABI boundary): the call's results are void, the context stays usable          */

/* where a buffer handed to the library lives */
#define NVCA_MEM_HOST   0
#define NVCA_MEM_DEVICE 1

/* detectMultiScale flags -- values of OpenCV's CV_HAAR_* */
#define NVCA_HAAR_DO_CANNY_PRUNING    1   /* accepted, ignored (never set by the reference) */
#define NVCA_HAAR_SCALE_IMAGE         2
#define NVCA_HAAR_FIND_BIGGEST_OBJECT 4
#define NVCA_HAAR_DO_ROUGH_SEARCH     8

/* feature-sum accumulation policy (OpenCV build variant) */
#define NVCA_SUM_F32PAIR 0   /* SSE2 build (distro default): 2-rect stages add in f32 */
#define NVCA_SUM_F64     1   /* plain C build                                          */

typedef struct nvca_ctx nvca_ctx;
typedef struct nvca_cascade nvca_cascade;
typedef struct nvca_face_stream nvca_face_stream;
typedef struct nvca_tracker nvca_tracker;

typedef struct nvca_rect { int x, y, w, h; } nvca_rect;

typedef struct nvca_frame {
    const void *data;     /* packed rows, BGR (3 B/px) or BGRA (4 B/px); frames of a
                             4:2:0 stream (nvca_face_stream_set_input, nvca_part_stream_set_input,
                             nvca_tracker_set_input): the buffer base the stream's
                             plane offsets count from                                */
    int width, height;    /* (4:2:0 streams: the luma size)                          */
    int stride;           /* bytes per row; the reference assumes align4(width*bpp),
                             FACE/kmsfacedetect.cpp:300-305 (4:2:0 streams: the
                             layout's stride[0])                                    */
    int mem;              /* NVCA_MEM_HOST or NVCA_MEM_DEVICE                        */
    uint64_t pts;
} nvca_frame;

/* Pixel format of a stream's frames (a property of the stream, as caps are in GStreamer; the plane table mirrors
 * GstVideoInfo's offset[] / stride[]).  4:2:0 frames are what decoders emit: a stream that takes them stands for the
 * videoconvert in front of the element plus the element, cv::cvtColor(CV_YUV2BGR_NV12 / CV_YUV2BGR_I420) in front of
 * FACE/kmsfacedetect.cpp:805 (SURVEY.md A.13 states the arithmetic). */
#define NVCA_PIX_BGR  0   /* packed, as nvca_frame describes it */
#define NVCA_PIX_NV12 1   /* plane 0: Y, w x h; plane 1: U,V interleaved, w bytes x h/2 rows */
#define NVCA_PIX_I420 2   /* plane 0: Y; plane 1: U, w/2 x h/2; plane 2: V, w/2 x h/2 */
/* (3 is no format: refused with NVCA_ERR_ARG)
 * Packed 4:2:2, what V4L2 cameras, capture cards and SDI / USB devices emit: ONE plane of 2 bytes a pixel, four bytes a pixel pair,
 * every row with its own chroma.  A stream that takes them stands for cv::cvtColor(CV_YUV2BGR_YUY2 / _UYVY / _YVYU) plus the element
 * (in row y, pixels 2k and 2k + 1 take U and V from the same four bytes; the arithmetic is A.13's).  Plane 0 only:
 * offset[0] and stride[0] >= 2 * width; offset[1..2] and stride[1..2] are ignored (a stream stores them as zero).  The width must be
 * even; the height is any positive number. */
#define NVCA_PIX_YUY2 4   /* bytes Y0 U Y1 V (YUYV) */
#define NVCA_PIX_UYVY 5   /* bytes U Y0 V Y1 */
#define NVCA_PIX_YVYU 6   /* bytes Y0 V Y1 U */
typedef struct nvca_pixel_layout {
    int    format;          /* NVCA_PIX_* */
    size_t offset[3];       /* byte offset of each plane from nvca_frame.data */
    int    stride[3];       /* bytes per row of each plane */
} nvca_pixel_layout;

/* ---- context ----------------------------------------------------------- */
/* HIP devices visible to the process (the GStreamer shim spreads its elements over them, one context per GPU) */
int  nvca_device_count(int *n);
int  nvca_ctx_create(int device_id, nvca_ctx **out);
void nvca_ctx_destroy(nvca_ctx *ctx);
/* text of the last error on this context (never NULL) */
const char *nvca_last_error(const nvca_ctx *ctx);
const char *nvca_version(void);
/* Raw-candidate capacity per frame the lists start with (default 16384, at most 2^22).  A detectMultiScale call
 * (nvca_detect_multiscale / _raw, the part detectors' searches) that produces more re-runs its launch set once with lists of
 * the exact size and answers as the reference does -- a CV_HAAR_FIND_BIGGEST_OBJECT search with a lenient cascade included
 * (NOSE/kmsnosedetect.cpp:870-873).  The batched face path reports NVCA_ERR_OVERFLOW for the batch that overflowed (never a
 * truncated list) and sizes the lists of the following batches for what that batch produced. */
int  nvca_ctx_set_hit_capacity(nvca_ctx *ctx, int cap);
int  nvca_ctx_set_sum_policy(nvca_ctx *ctx, int policy);
/* Measurement / bisecting switches, per context.  The process-wide defaults come from the environment
 * (NVCA_BAND, NVCA_TILES, ... read once, when the first context is created); this sets one for this context.  Names, in the
 * order of the table in csrc/options.cpp: "group_zerocopy", "skip_cascade", "host_group", "band_map", "band" (-1 / 0 / 1),
 * "host_profile", "sparse_ingest", "pyr_off", "part_stats", "ingest_chunk", "deep_stage", "tiles", "plan_debug", "deep_lds",
 * "trk_fold", "trk_order", "host_threads", "fb_dense", "roi", "stage_order", "pair_max", "spec_pairs", "quiet"; any other name is refused with NVCA_ERR_ARG.
 * None of them changes a result.  Switches that shape plans drop the context's cached plans (not while a submitted batch is
 * in flight).
 * nvca_ctx_get_option reads the value a switch holds for this context (so that a caller can put it back). */
int  nvca_ctx_set_option(nvca_ctx *ctx, const char *name, int value);
int  nvca_ctx_get_option(nvca_ctx *ctx, const char *name, int *value);
/* block until everything queued on the context's HIP stream has finished */
int  nvca_ctx_synchronize(nvca_ctx *ctx);
/* the hipStream_t the context launches on (for interop / profiling) */
void *nvca_ctx_stream(nvca_ctx *ctx);
/* Zero-copy ingest: page-lock caller-owned frame memory (e.g. the buffers of a GstBufferPool, mapped by
 * kms_face_detect_conf_images, FACE/kmsfacedetect.cpp:282-306) so that the H2D copies of NVCA_MEM_HOST frames are true
 * asynchronous DMA.  Optional: pageable frames work, they are just copied through the driver's staging buffers.
 * Unregister before the memory is freed. */
int  nvca_host_register(nvca_ctx *ctx, void *ptr, size_t bytes);
int  nvca_host_unregister(nvca_ctx *ctx, void *ptr);

/* Per-kernel timing with HIP events on the context's stream.  While enabled,
 * kernel launches are bracketed by events; nvca_ctx_kernel_timing drains them.
 * on == 0: off; on == 1: every launch; on == N > 1: the launches of every N-th
 * batch of the face-detector / tracker entry points only (the first one included) --
 * event-carrying launches do not overlap their neighbours, which costs a few
 * microseconds per launch. */
#define NVCA_K_GRAY      0  /* resize + BGR2GRAY + histogram            */
#define NVCA_K_LUT       1  /* equalizeHist LUT                         */
#define NVCA_K_COLSUM    2  /* integral: band column sums               */
#define NVCA_K_BANDSCAN  3  /* integral: scan over bands                */
#define NVCA_K_INTEGRAL  4  /* integral: row scan + write               */
#define NVCA_K_STAGE0    5  /* cascade: variance + stage 0, all windows */
#define NVCA_K_STRIP     6  /* cascade: early stages, window per lane   */
#define NVCA_K_DEEP      7  /* cascade: late stages, stump per lane     */
#define NVCA_K_GROUP     8  /* candidate sort + groupRectangles         */
#define NVCA_K_TRACKER   9  /* tracker pixel pass + labelling           */
#define NVCA_K_RESIZE1  10  /* 8UC1 resize (pyramid / parts)            */
#define NVCA_K_TILE     11  /* cascade: early stages from LDS-staged tiles */
#define NVCA_K_BAND     12  /* cascade: variance + stage 0 + early stages, one row of tiles per workgroup */
#define NVCA_K_ROI     13  /* cascade: a whole detectMultiScale on a small image (a face region) per workgroup */
#define NVCA_K_COUNT    14
int  nvca_ctx_enable_kernel_timing(nvca_ctx *ctx, int on);
/* total_ms[NVCA_K_COUNT], launches[NVCA_K_COUNT]; resets the accumulators */
int  nvca_ctx_kernel_timing(nvca_ctx *ctx, double *total_ms, int64_t *launches);
const char *nvca_kernel_name(int k);

/* ---- cascade: replaces cv::CascadeClassifier::load ---------------------
 * FACE/kmsfacedetect.cpp:162-177 (HAAR_CONF_FILE :40), EYE/kmseyedetect.cpp:27-29,
 * NOSE/kmsnosedetect.cpp:31-32, MOUTH/kmsmouthdetect.cpp:37-38, EAR/kmseardetect.cpp:29-31.
 * Both formats cv::CascadeClassifier::load reads (OpenCV 2.4 cascadedetect.cpp), told apart by the type_id of the first child
 * of <opencv_storage>:
 *  - old format ("opencv-haar-classifier"): stump or tree-structured weak classifiers, upright or tilted features (cascades
 *    with trees / tilted features run through the general evaluator);
 *  - new format ("opencv-cascade-classifier", what opencv_traincascade writes and what OpenCV 3 / 4 install as haarcascades/ and
 *    lbpcascades/): featureType LBP or HAAR (cascadedetect.cpp's HaarEvaluator, which is NOT the
 *    old format's arithmetic), stump weak classifiers.  Refused with NVCA_ERR_UNSUPPORTED: featureType HOG, stage types other than
 *    BOOST, trees (maxDepth > 1 or more than one internal node), tilted HAAR features, and a maxCatCount that does not fit the
 *    feature type (256 for LBP, 0 for HAAR).
 * A new-format cascade of either feature type goes through nvca_detect_multiscale / nvca_detect_raw on single images and through
 * their _batch forms on several, through the face streams made with nvca_face_stream_create_any and through the part streams made
 * with nvca_part_stream_create_any, in any role and any mixture; nvca_face_stream_create and nvca_part_stream_create refuse it
 * (NVCA_ERR_UNSUPPORTED).  Its scan ignores `flags`.
 * Its launches are booked under the existing timing slots.  An LBP cascade's single small image -- a part detector's face region,
 * the 160-px face-pass image: whatever fits one workgroup's LDS -- is scanned by the round's one small-image launch, under
 * NVCA_K_ROI (option "roi", as for old-format cascades); a new-format HAAR cascade has no small-image kernel and always takes the
 * large-image route.  Larger images and jobs of several images: the evaluator's kernels under NVCA_K_STRIP ("window per
 * lane"), the level resize and integral under NVCA_K_RESIZE1 / NVCA_K_INTEGRAL as CV_HAAR_SCALE_IMAGE books them, a face stream's
 * grouping under NVCA_K_GROUP. */
#define NVCA_CASCADE_HAAR 0
#define NVCA_CASCADE_LBP  1
#define NVCA_CASCADE_HAAR_NEW 2     /* new format, featureType HAAR */
int  nvca_cascade_load_xml(nvca_ctx *ctx, const char *path, nvca_cascade **out);
int  nvca_cascade_load_mem(nvca_ctx *ctx, const char *xml, int64_t len, nvca_cascade **out);
void nvca_cascade_free(nvca_cascade *c);
/* The loader alone: parses a cascade of either format on the host and reports its shape (any out pointer may be NULL) or the
 * loader's error text -- no device and no context needed, so cascade files can be checked on a box without a GPU.
 * Same status codes as nvca_cascade_load_mem. */
int  nvca_cascade_validate_mem(const char *xml, int64_t len, int *win_w, int *win_h, int *n_stages, int *n_weak,
                               char *err, int err_cap);
/* Exercises the exception barrier of the ABI (see "never throws" above): throws the exception `kind` names from inside an
 * entry point and returns what the barrier made of it -- 0: std::bad_alloc -> NVCA_ERR_NOMEM, 1: std::length_error ->
 * NVCA_ERR_NOMEM, 2: std::runtime_error, 3: a non-standard exception, 4: std::out_of_range -> NVCA_ERR_INTERNAL. */
int  nvca_abi_selftest(int kind);
/* window size, stage count, weak-classifier count (any pointer may be NULL) */
int  nvca_cascade_info(const nvca_cascade *c, int *win_w, int *win_h, int *n_stages, int *n_weak);
/* has_tilted / has_trees (either pointer may be NULL): what kind of cascade the loader found */
int  nvca_cascade_kind(const nvca_cascade *c, int *has_tilted, int *has_trees);
/* flat dump for cross-checking the loader: arrays sized by nvca_cascade_info;
 * rects[n_weak*12] (3 rects x,y,w,h), weights[n_weak*3], thr/left_val/right_val[n_weak],
 * stage_sizes/stage_thr[n_stages] (stump cascades only) */
int  nvca_cascade_dump(const nvca_cascade *c, int *rects, float *weights, float *thr,
                       float *left_val, float *right_val, int *stage_sizes, float *stage_thr);
/* which branch of cv::CascadeClassifier::load (cascadedetect.cpp) took the file: NVCA_CASCADE_HAAR / NVCA_CASCADE_LBP /
 * NVCA_CASCADE_HAAR_NEW, and the length of a new-format cascade's feature list (0 for an old-format cascade); either pointer may be NULL */
int  nvca_cascade_format(const nvca_cascade *c, int *format, int *n_features);
/* flat dump of an LBP cascade as cascadedetect.cpp's Data::read / LBPEvaluator::read keep it, for cross-checking the loader
 * (any pointer may be NULL): rects[n_features*4] (x, y, w, h of the top-left cell), feature_idx[n_weak], subsets[n_weak*8],
 * leaves[n_weak*2], stage_sizes / stage_thr[n_stages] -- thresholds as evaluated, after the 1e-5f.  NVCA_ERR_ARG for an
 * old-format cascade (as nvca_cascade_dump answers for an LBP cascade; nvca_cascade_kind reports (0, 0) for one). */
int  nvca_cascade_dump_lbp(const nvca_cascade *c, int *rects, int *feature_idx, int32_t *subsets, float *leaves,
                           int *stage_sizes, float *stage_thr);
/* flat dump of a new-format HAAR cascade as Data::read / HaarEvaluator::read keep it (any pointer may be NULL):
 * rects[n_features*12] (3 rects x, y, w, h; a missing one all zero), weights[n_features*3] (a missing rect's is 0),
 * rect_counts[n_features], feature_idx[n_weak], thr[n_weak], leaves[n_weak*2], stage_sizes / stage_thr[n_stages] -- thresholds as
 * evaluated, after the 1e-5f.  NVCA_ERR_ARG for any other cascade (as nvca_cascade_dump and nvca_cascade_dump_lbp answer for this
 * one; nvca_cascade_kind reports (0, 0)). */
int  nvca_cascade_dump_haar_new(const nvca_cascade *c, int *rects, float *weights, int *rect_counts, int *feature_idx, float *thr,
                                float *leaves, int *stage_sizes, float *stage_thr);
/* The small-image route of a new-format HAAR cascade (cv::CascadeClassifier::detectMultiScale on a file written by
 * opencv_traincascade -featureType HAAR), opt-in per cascade.  on != 0: a detectMultiScale job of ONE image on this
 * cascade whose two integral planes fit a workgroup's LDS (8 (cols + 1)(rows + 1) <= 122 800 bytes: 160 x 90 is inside) is served,
 * with every other small job of its round, by one launch and one wait instead of the large-image launch set and its cached plan per
 * image size -- what a part detector's face-region searches are.  The flag is read when a job is built: a submitted ticket keeps the
 * route it was built with.  Results never depend on it, and the "roi" option = 0 sends every job down the large-image route, flag or
 * not.  Default 0: a cascade nobody opted in is routed exactly as before.  On an old-format or an LBP cascade the setter returns
 * NVCA_OK and changes nothing -- their small routes are always available -- and the getter reports 1.  NVCA_ERR_ARG for NULL. */
int  nvca_cascade_set_small_route(nvca_cascade *c, int on);
int  nvca_cascade_get_small_route(const nvca_cascade *c, int *on);
/* Loading with flags.  flags == 0 is nvca_cascade_load_xml / _load_mem / _validate_mem itself; a bit that is not defined here is
 * NVCA_ERR_ARG.
 * NVCA_LOAD_HAAR_GENERAL: a new-format HAAR file may hold tree weak classifiers (internalNodes "left right featureIdx threshold" per
 * node, one leaf value more than nodes; at most 15 nodes a weak classifier, NVCA_ERR_UNSUPPORTED beyond) and tilted features
 * (<tilted>1</tilted>: every rect of the feature reads the tilted integral, with the file's weight).  The header's maxDepth is not
 * consulted.  NVCA_ERR_PARSE for a tree the evaluator could not walk safely: a node word count that is no multiple of 4, a leaf count
 * other than nodes + 1, a child node that does not lie behind its parent or lies outside the tree, a leaf index outside the leaf
 * values, a threshold or leaf that is not finite, a feature index outside the list, a tilted rect with x - h < 0, x + w > width or
 * y + w + h > height.  The format stays NVCA_CASCADE_HAAR_NEW and every entry point that takes such a cascade takes this one
 * (detectMultiScale, batches, levels, face and part streams made with _create_any).  A flagged file of stumps "0 -1" on upright
 * features is the cascade the plain load makes: the same kernels, eligible for the small route.  A cascade that does hold a tree or
 * a tilted feature ("general": nvca_cascade_kind reports which) is evaluated by its own kernels on the large-image route only:
 * nvca_cascade_set_small_route returns NVCA_OK and changes nothing, the getter reports 0, nvca_cascade_dump_haar_new answers
 * NVCA_ERR_ARG (nvca_cascade_dump_haar_tree expresses it).  On old-format and LBP files the flag changes nothing: LBP trees stay
 * refused. */
#define NVCA_LOAD_HAAR_GENERAL 1
int  nvca_cascade_load_xml_ex(nvca_ctx *ctx, const char *path, unsigned flags, nvca_cascade **out);
int  nvca_cascade_load_mem_ex(nvca_ctx *ctx, const char *xml, int64_t len, unsigned flags, nvca_cascade **out);
int  nvca_cascade_validate_mem_ex(const char *xml, int64_t len, unsigned flags, int *win_w, int *win_h, int *n_stages, int *n_weak,
                                  char *err, int err_cap);
/* the sizes of nvca_cascade_dump_haar_tree's arrays and whether the cascade is general (any pointer may be NULL); NVCA_ERR_ARG for a
 * cascade that is not NVCA_CASCADE_HAAR_NEW */
int  nvca_cascade_tree_info(const nvca_cascade *c, int *n_nodes, int *n_leaves, int *general);
/* flat dump of a new-format HAAR cascade, general or not, in terms that express trees (any pointer may be NULL):
 * rects[n_features*12], weights[n_features*3], rect_counts[n_features] as nvca_cascade_dump_haar_new's, tilted[n_features];
 * node_counts[n_weak]; per node, in file order, nodes[n_nodes*3] = left, right, featureIdx as the file has them (a child > 0: a node
 * of the same weak classifier, <= 0: its leaf -child) and node_thr[n_nodes]; leaves[n_leaves] (a weak classifier's node count + 1,
 * in file order); stage_sizes / stage_thr[n_stages], thresholds as evaluated. */
int  nvca_cascade_dump_haar_tree(const nvca_cascade *c, int *rects, float *weights, int *rect_counts, int *tilted, int *node_counts,
                                 int *nodes, float *node_thr, float *leaves, int *stage_sizes, float *stage_thr);

/* ---- imgproc primitives (each = one cv:: call of the reference) -------- */
/* cv::cvtColor(CV_BGR2GRAY) FACE/kmsfacedetect.cpp:806, TRK/gstnubotracker.cpp:356 (channels 4) */
int nvca_bgr2gray(nvca_ctx *ctx, const void *src, int w, int h, int stride, int channels,
                  int mem, void *dst_gray, int dst_stride);
/* cv::resize(INTER_LINEAR) FACE/kmsfacedetect.cpp:805 (3 ch), EYE/kmseyedetect.cpp:956,963 (1 ch) */
int nvca_resize_linear(nvca_ctx *ctx, const void *src, int sw, int sh, int sstride, int channels,
                       int mem, void *dst, int dw, int dh, int dstride);
/* cv::cvtColor(CV_YUV2BGR_NV12 / CV_YUV2BGR_I420) in front of FACE/kmsfacedetect.cpp:805 (the element's caps ask for BGR, :129-133;
 * the conversion is the pipeline's videoconvert): BT.601 limited range, integer, SURVEY.md A.13.  base: the buffer the
 * layout's offsets count from; w x h: the luma size, both even; src and dst are both host or both device memory (mem);
 * dst_bgr: packed BGR rows dst_stride bytes apart. */
int nvca_yuv420_to_bgr(nvca_ctx *ctx, const void *base, int w, int h, const nvca_pixel_layout *layout, int mem,
                       void *dst_bgr, int dst_stride);
/* cv::cvtColor(CV_YUV2BGR_YUY2 / CV_YUV2BGR_UYVY / CV_YUV2BGR_YVYU), the sibling of nvca_yuv420_to_bgr for packed 4:2:2 buffers
 * (layout->format NVCA_PIX_YUY2 / _UYVY / _YVYU; anything else, a null layout included, is NVCA_ERR_ARG): BT.601 limited range,
 * integer, SURVEY.md A.18.  base: the buffer offset[0] counts from; w: even; h: any positive number; stride[0] >= 2 * w; src and dst
 * are both host or both device memory (mem); dst_bgr: packed BGR rows dst_stride >= 3 * w bytes apart, only the pixels' own bytes are
 * written. */
int nvca_yuv422_to_bgr(nvca_ctx *ctx, const void *base, int w, int h, const nvca_pixel_layout *layout, int mem,
                       void *dst_bgr, int dst_stride);
/* cv::cvtColor(CV_BGR2YUV_I420), the inverse of nvca_yuv420_to_bgr: what the pipeline's videoconvert behind the element does
 * (FACE/run_plugin.sh:3) when a viewed frame goes on to an encoder.  OpenCV 2.4 color.cpp (RGB888toYUV420pInvoker), BT.601 limited
 * range, integer, SURVEY.md A.14: Y of every pixel; the chroma sample of a 2 x 2 block is (U, V) of the block's top-left pixel alone
 * (nothing is averaged).  OpenCV 2.4 writes I420 only; NVCA_PIX_NV12 holds the same samples with U and V interleaved.  src: packed
 * BGR (channels 3) or BGRA (channels 4, alpha ignored -- the tracker's frames, TRK/gstnubotracker.cpp:356) rows `stride` bytes apart;
 * w x h: both even; base: the buffer the layout's offsets count from; src and base are both host or both device memory (mem).  The
 * layout rules are those of the 4:2:0 streams (nvca_face_stream_set_input): plane strides at least a row, no overlapping planes,
 * gaps allowed.  Only the rows' own bytes are written: row padding, gaps between planes and whatever lies behind the last plane
 * keep their value.  Device buffers are converted in place in the order of the context's stream. */
int nvca_bgr_to_yuv420(nvca_ctx *ctx, const void *src_bgr, int w, int h, int stride, int channels, int mem,
                       void *base, const nvca_pixel_layout *layout);
/* cv::equalizeHist FACE/kmsfacedetect.cpp:807 */
int nvca_equalize_hist(nvca_ctx *ctx, const void *src_gray, int w, int h, int stride, int mem,
                       void *dst_gray, int dst_stride);
/* cv::flip(src, dst, 1) EAR/kmseardetect.cpp:800 */
int nvca_flip_horizontal(nvca_ctx *ctx, const void *src_gray, int w, int h, int stride, int mem,
                         void *dst_gray, int dst_stride);
/* view-faces / view-eyes / ...: the outlines the elements draw on a viewed frame, on the frame where it is --
 * host memory (the GStreamer shim's mapped buffer) or device memory (a viewed stream that stays in HBM makes no round trip).
 * NVCA_SHAPE_RECT3: cvRectangle(img, (x, y), (x + w, y + h), colour, 3, 8, 0) as FACE/kmsfacedetect.cpp:836-845,
 * TRK/gstnubotracker.cpp:388-395 and the nose / mouth / ear elements call it: the 3-pixel band around the outline, the four
 * outermost corner pixels left out (round joins of radius 1).  NVCA_SHAPE_RING4: circle(img, (x, y), w, colour, 4, 8, 0),
 * EYE/kmseyedetect.cpp:1075-1092: the pixels at distance [w - 2, w + 2] from the centre.  Shapes are drawn in order.
 * The rasterisation rules are this library's statement of OpenCV's thick-line code, not pixel-verified against it.
 * Host frames need no device: ctx may be NULL for them. */
#define NVCA_SHAPE_RECT3 0
#define NVCA_SHAPE_RING4 1
typedef struct { int kind; int x, y, w, h; uint8_t bgra[4]; } nvca_shape;
int nvca_draw_shapes(nvca_ctx *ctx, const nvca_frame *frame, int channels, const nvca_shape *shapes, int n);
/* The same outlines on a 4:2:0 frame (frame->data: the buffer base, frame->stride: the layout's stride[0]; layout rules and
 * refusals as nvca_face_stream_set_input states them), so that a viewed NV12 / I420 stream -- decoder, detector, outlines, encoder --
 * never holds a BGR frame: FACE/kmsfacedetect.cpp:832-850 with the face colour of FACE/BaseFace.cpp:76-80, TRK/gstnubotracker.cpp:388-395,
 * EYE/kmseyedetect.cpp:1075-1092, and the videoconvert behind the element (FACE/run_plugin.sh:3) in one call.  Coverage as
 * nvca_draw_shapes (shapes in order, the last one that covers a pixel colours it).  A covered pixel's Y byte becomes Y(colour); the
 * chroma sample of a 2 x 2 block becomes (U, V)(colour of the last shape covering the block's top-left pixel) if that pixel is
 * covered; every other byte keeps its value.  That is SURVEY.md A.14 applied to the drawn BGR image, restricted to the samples whose
 * defining pixel was drawn: an untouched region stays bit-identical (it is not converted there and back).  Host frames need no
 * device: ctx may be NULL for them. */
int nvca_draw_shapes_yuv420(nvca_ctx *ctx, const nvca_frame *frame, const nvca_pixel_layout *layout,
                            const nvca_shape *shapes, int n);
/* image-to-overlay: kms_face_detect_display_detections_overlay_img, FACE/kmsfacedetect.cpp:427-502 -- for every
 * box, in order, the overlay image is scaled (cvResize, CV_INTER_LINEAR) to (box.w * width_percent) x (box.h * height_percent),
 * placed at box.x + box.w * offset_x_percent, box.y + box.h * offset_y_percent (truncated as the reference's int arithmetic does)
 * and written onto the BGR frame where it lies inside it: 1 channel -> copied to B, G and R; 3 channels -> copied; 4 channels ->
 * blended per pixel with weight alpha / 255 in double arithmetic, truncated to 8 bits.  Boxes are frame pixels (the reference
 * passes box * scale, :840-844).  The image (what cvLoadImage(..., CV_LOAD_IMAGE_UNCHANGED) returned: fetching and decoding it
 * stay with the element) is host memory; the frame may be host memory (plain loops, ctx may be NULL) or device memory (one kernel
 * per box; a viewed stream that stays in HBM makes no round trip).  A box whose scaled size is not positive is skipped (the
 * reference's cvCreateImage would throw there). */
typedef struct nvca_overlay {
    const void *data; int width, height, stride, channels;       /* 8-bit, 1 / 3 / 4 interleaved channels, host memory */
    double offset_x_percent, offset_y_percent, width_percent, height_percent;   /* the image-to-overlay structure's fields, :351-367 */
} nvca_overlay;
int nvca_overlay_blend(nvca_ctx *ctx, const nvca_frame *frame_bgr, const nvca_rect *boxes, int n, const nvca_overlay *overlay);
/* image-to-overlay on a 4:2:0 frame (frame and layout as nvca_draw_shapes_yuv420): placement, scaling and the per-pixel blend are
 * nvca_overlay_blend's (FACE/kmsfacedetect.cpp:427-502), boxes in order, each on the frame the previous one left.  For one box, a pixel
 * inside the placed image and the frame is touched unless the image has 4 channels and its scaled alpha there is 0 (the reference
 * leaves such a pixel's BGR value as it is; here its bytes stay).  A touched pixel's BGR value before the box is SURVEY.md A.13 of
 * its Y and its block's chroma; the reference's write (:467-490) goes onto that value; Y becomes A.14's Y of the result, and the
 * chroma sample of a block becomes A.14's (U, V) of the blended top-left pixel of the block if that pixel is touched.  Every other
 * byte keeps its value.  Host frames: plain loops, ctx may be NULL; device frames: one kernel per box. */
int nvca_overlay_blend_yuv420(nvca_ctx *ctx, const nvca_frame *frame, const nvca_pixel_layout *layout,
                              const nvca_rect *boxes, int n, const nvca_overlay *overlay);
/* cv::integral as used inside detectMultiScale: sum int32 and sqsum float64,
 * both dense (h+1)*(w+1) */
int nvca_integral(nvca_ctx *ctx, const void *src_gray, int w, int h, int stride, int mem,
                  int32_t *sum, double *sqsum);

/* the third plane of cv::integral, which cvHaarDetectObjectsForROC asks for when the cascade holds tilted features
 * (haarcascade_profileface.xml, EAR/kmseardetect.cpp:29): tilted(X,Y) = sum of image(x,y) over y < Y,
 * abs(x - X + 1) <= Y - y - 1; int32, dense (h+1)*(w+1) */
int nvca_integral_tilted(nvca_ctx *ctx, const void *src_gray, int w, int h, int stride, int mem, int32_t *tilted);

/* ---- detectMultiScale ---------------------------------------------------
 * cv::CascadeClassifier::detectMultiScale(gray, objects, scaleFactor, minNeighbors,
 * flags, minSize, maxSize) -- FACE/kmsfacedetect.cpp:809-811 and the sibling call
 * sites listed in SURVEY.md Appendix B.  max_w/max_h == 0 -> image size.
 * Objects are written in OpenCV's serial order; *n_out may exceed cap (then only
 * cap are written). */
int nvca_detect_multiscale(nvca_ctx *ctx, const nvca_cascade *cascade, const void *gray,
                           int w, int h, int stride, int mem, double scale_factor,
                           int min_neighbors, int flags, int min_w, int min_h, int max_w,
                           int max_h, nvca_rect *out, int cap, int *n_out);
/* raw candidates before groupRectangles, canonical (scale, y, x) order; not
 * defined for FIND_BIGGEST_OBJECT -- except with an LBP cascade, whose scan (cascadedetect.cpp, detectMultiScale on a
 * new-format cascade) ignores flags altogether: every flags value gives the answer of 0 there */
int nvca_detect_raw(nvca_ctx *ctx, const nvca_cascade *cascade, const void *gray, int w, int h,
                    int stride, int mem, double scale_factor, int flags, int min_w, int min_h,
                    int max_w, int max_h, nvca_rect *out, int cap, int *n_out);
/* nvca_detect_multiscale on n images of ONE geometry (w, h, stride) and one memory kind, behind one wait per round of launch sets:
 * gray[i] is image i, its objects go to out[(size_t)i * cap + k] (the convention of nvca_face_batch_process), n_out[i] is its
 * full count and may exceed cap.  Image i's answer is exactly what nvca_detect_multiscale returns for it, for every cascade
 * format and every flags value that call accepts.  The images share their launch sets in groups of up to 32 (an LBP cascade's
 * evaluator and the pyramids carry an image axis; a FIND_BIGGEST_OBJECT search runs per image), so the number of launches, and
 * the waits, are per group and not per image.  Device images at equal distances in one allocation are read where they are,
 * others are copied first.  n == 0 is NVCA_OK.  NVCA_ERR_ARG: n < 0, gray or one of its entries NULL, cap < 0, cap > 0 without
 * out, n_out NULL, scale_factor <= 1.  Any failure fails the whole call: out and n_out are then unspecified. */
int nvca_detect_multiscale_batch(nvca_ctx *ctx, const nvca_cascade *cascade, int n, const void *const *gray,
                                 int w, int h, int stride, int mem, double scale_factor, int min_neighbors, int flags,
                                 int min_w, int min_h, int max_w, int max_h, nvca_rect *out, int cap, int *n_out);
/* nvca_detect_raw on n images, laid out and refused as above; FIND_BIGGEST_OBJECT on a Haar cascade is NVCA_ERR_ARG as for
 * the single call */
int nvca_detect_raw_batch(nvca_ctx *ctx, const nvca_cascade *cascade, int n, const void *const *gray,
                          int w, int h, int stride, int mem, double scale_factor, int flags,
                          int min_w, int min_h, int max_w, int max_h, nvca_rect *out, int cap, int *n_out);
/* cv::CascadeClassifier::detectMultiScale(image, objects, rejectLevels, levelWeights, scaleFactor, minNeighbors, flags, minSize,
 * maxSize, outputRejectLevels = true) (OpenCV 2.4 cascadedetect.cpp): the scan of nvca_detect_raw on a new-format
 * cascade of n stages, emitting every visited window that passes (reject level n) or is rejected by one of the last three stages
 * (reject level = that stage, n - 3 .. n - 1), each with the sum of the last stage evaluated on it as its level weight (an LBP
 * cascade's f32 sum widened to double, a HAAR cascade's f64 sum).  out[i], reject_levels[i] and level_weights[i] are one
 * detection, in the canonical (level, y, x) order of nvca_detect_raw; *n_out may exceed cap (then only cap are written).
 * Served: new-format LBP and HAAR cascades of four stages or more, single images in host or device memory; `flags` are accepted
 * and ignored.  NVCA_ERR_UNSUPPORTED: an old-format cascade, or one of fewer than four stages (stage-0 rejects would be
 * emitted).  NVCA_ERR_ARG: as nvca_detect_raw, and a NULL reject_levels or level_weights when cap > 0. */
int nvca_detect_raw_levels(nvca_ctx *ctx, const nvca_cascade *cascade, const void *gray, int w, int h,
                           int stride, int mem, double scale_factor, int flags, int min_w, int min_h,
                           int max_w, int max_h, nvca_rect *out, int *reject_levels, double *level_weights,
                           int cap, int *n_out);
/* the same overload with its grouping, cv::groupRectangles(rects, rejectLevels, levelWeights, minNeighbors, 0.2): the classes and
 * averaged rectangles of the plain form; a class answers with the largest reject level of its members and, among those, the
 * largest level weight.  A class is kept by that LEVEL, not by its member count (dropped when level <= min_neighbors), while the
 * contained-box filter reads the other class's member count -- OpenCV's behaviour, kept.  min_neighbors <= 0 returns the raw
 * triples of nvca_detect_raw_levels untouched: this library's choice (OpenCV 2.4's early return there is not remembered with
 * certainty).  Refusals as above. */
int nvca_detect_multiscale_levels(nvca_ctx *ctx, const nvca_cascade *cascade, const void *gray, int w, int h,
                                  int stride, int mem, double scale_factor, int min_neighbors, int flags,
                                  int min_w, int min_h, int max_w, int max_h, nvca_rect *out,
                                  int *reject_levels, double *level_weights, int cap, int *n_out);
/* cv::groupRectangles(rects, groupThreshold, eps) on the device; in place */
int nvca_group_rectangles(nvca_ctx *ctx, nvca_rect *rects, int n, int group_threshold, double eps,
                          int *n_out);

/* ---- NuboFaceDetector stream -------------------------------------------
 * One handle == one element instance == one media stream.  Replaces
 * kms_face_detect_conf_images + kms_face_detect_process_frame + the box scaling
 * of kms_face_send_event (FACE/kmsfacedetect.cpp:282-306, 757-853, 190-211),
 * with Faces::track_faces (FACE/Faces.cpp:78-153) kept on the host. */
typedef struct nvca_face_params {
    int width_to_process;      /* "width-to-process", default 160  (:26)            */
    int process_x_every_4;     /* "process-x-every-4-frames", 4    (:24)            */
    int scale_factor_pct;      /* "multi-scale-factor", 25 -> 1.25 (:25,142)        */
    int track_threshold;       /* 40 (:33)                                          */
    int euclidean_threshold;   /* "euclidean-distance" 8 (:32) (unused by track_faces)*/
    int area_threshold;        /* 500 (:34) (unused by track_faces)                 */
    int min_neighbors;         /* 3 (:810)                                          */
    int detect_event;          /* "detect-event" 0 (:722): 1 = analyse only after
                                  nvca_face_stream_motion_event()                   */
} nvca_face_params;
void nvca_face_params_default(nvca_face_params *p);
int  nvca_face_stream_create(nvca_ctx *ctx, const nvca_cascade *cascade,
                             const nvca_face_params *params, nvca_face_stream **out);
/* The same contract on every cascade format nvca_detect_multiscale takes: FACE/kmsfacedetect.cpp:162-177 loads whatever file
 * cv::CascadeClassifier::load reads, and :805-811 then runs cv::CascadeClassifier::detectMultiScale on it.  On a Haar cascade the
 * stream is nvca_face_stream_create's.  On a new-format LBP cascade an analysed frame is resize (or the 4:2:0 tap),
 * BGR2GRAY, equalizeHist, the LBP scan of the equalised working image (scale factor 1 + scale_factor_pct / 100, minSize (cols / 20,
 * rows / 20), no maximum size, flags ignored), groupRectangles(max(min_neighbors, 1), 0.2) -- the raw list in (level, y, x) order
 * when min_neighbors is 0 -- and the unchanged gate, track_faces and box scaling.  Everything downstream (process, the batch calls,
 * submit / collect, set_input, set_params, motion_event, host and device frames) serves both; LBP and Haar streams mix in one
 * call.  NVCA_ERR_ARG for a cascade of another context. */
int  nvca_face_stream_create_any(nvca_ctx *ctx, const nvca_cascade *cascade,
                                 const nvca_face_params *params, nvca_face_stream **out);
void nvca_face_stream_destroy(nvca_face_stream *s);
int  nvca_face_stream_set_params(nvca_face_stream *s, const nvca_face_params *params);
/* The pixel format of the stream's frames from the next frame on: NV12 / I420 frames as a decoder produced them, converted
 * where the first kernel reads them (cv::cvtColor(CV_YUV2BGR_NV12 / _I420) in front of FACE/kmsfacedetect.cpp:805, then the
 * reference's order: resize on BGR, BGR2GRAY, equalizeHist).  layout == NULL or format NVCA_PIX_BGR: back to packed BGR.
 * A frame of a 4:2:0 stream is refused with NVCA_ERR_ARG -- before any stream's frame gate advances -- when its width or
 * height is odd, its stride is not the layout's stride[0], a plane's stride is shorter than its row, or planes overlap;
 * planes may have gaps between them (1080 rows in a 1088-row allocation).  BGR and 4:2:0 streams mix in one batch.
 * Packed 4:2:2 frames (NVCA_PIX_YUY2 / _UYVY / _YVYU, cv::cvtColor(CV_YUV2BGR_YUY2 / _UYVY / _YVYU) in front of :805, SURVEY.md
 * A.18) are taken by the same rules: refused when the width is odd, stride[0] < 2 * width or the frame's stride is not stride[0]; any
 * height.  Packed, 4:2:0 and 4:2:2 streams of any byte order mix in one batch. */
int  nvca_face_stream_set_input(nvca_face_stream *s, const nvca_pixel_layout *layout);
/* a "motion" custom event arrived (FACE/kmsfacedetect.cpp:680-755): analyse the
 * next NUM_FRAMES_TO_PROCESS (10) frames */
int  nvca_face_stream_motion_event(nvca_face_stream *s);
/* One kms_face_detect_transform_frame_ip (FACE/kmsfacedetect.cpp:857-898): boxes
 * in original-frame pixels exactly as kms_face_send_event emits them; ids (may
 * be NULL) are the Faces ids. */
int  nvca_face_stream_process(nvca_face_stream *s, const nvca_frame *frame, nvca_rect *out,
                              int *ids, int cap, int *n_out);
/* Batched frontend: frame i belongs to streams[i]; a stream may appear several
 * times (consecutive frames, in order).  All analysed frames go through one
 * launch set per distinct geometry.  out is [n][cap], ids (may be NULL) likewise. */
int  nvca_face_batch_process(nvca_ctx *ctx, int n, nvca_face_stream *const *streams,
                             const nvca_frame *frames, nvca_rect *out, int *ids, int cap,
                             int *n_out);
/* The same in two halves, for a serving loop that keeps the GPU busy across batches: submit() gates the frames and queues
 * every launch, collect() waits for that batch and runs the temporal logic (Faces::track_faces, FACE/Faces.cpp:78-153).
 * Up to two batches may be in flight; they are collected in submission order.  Frame memory and the streams of a batch
 * must stay valid until the batch has been collected. */
int  nvca_face_batch_submit(nvca_ctx *ctx, int n, nvca_face_stream *const *streams, const nvca_frame *frames, int *ticket);
int  nvca_face_batch_collect(nvca_ctx *ctx, int ticket, nvca_rect *out, int *ids, int cap, int *n_out);

/* ---- part detectors: NuboEyeDetector / NuboNoseDetector / NuboMouthDetector / NuboEarDetector ----
 * One handle == one element instance.  Replaces kms_{eye,nose,mouth,ear}_detect_conf_images +
 * _process_frame (EYE/kmseyedetect.cpp:310-341,915-1064; NOSE/kmsnosedetect.cpp:275-308,792-868;
 * MOUTH/kmsmouthdetect.cpp:285-315,798-873; EAR/kmseardetect.cpp:292-319,644-729,767-812): gray (+equalize) at
 * full resolution, a face pass on the 160-px image (or faces handed over by an upstream element), then per face
 * the reference's ROI geometry and part cascades; the per-frame merging heuristics stay on the host. */
#define NVCA_PART_EYE   0
#define NVCA_PART_NOSE  1
#define NVCA_PART_MOUTH 2
#define NVCA_PART_EAR   3
typedef struct nvca_part_stream nvca_part_stream;
typedef struct nvca_part_params {
    int kind;                /* NVCA_PART_*                                                  */
    int width_to_process;    /* "width-to-process", 320 (EYE/kmseyedetect.cpp:25)            */
    int process_x_every_4;   /* "process-x-every-4-frames", 4                                */
    int scale_factor_pct;    /* "multi-scale-factor", 25 (face pass)                         */
    int detect_event;        /* "detect-event": 1 = faces come from nvca_part_stream_push_faces */
} nvca_part_params;
void nvca_part_params_default(nvca_part_params *p, int kind);
/* cascades: face (frontalface_alt; profileface for EAR); a and b:
 *   EYE  a = mcs_righteye, b = mcs_lefteye (EYE/kmseyedetect.cpp:28-29)
 *   EAR  a = LEFT_SIDE cascade (mcs_rightear, sic), b = RIGHT_SIDE cascade (EAR/kmseardetect.cpp:29-31,796,801)
 *   NOSE / MOUTH  a only (b may be NULL) */
int  nvca_part_stream_create(nvca_ctx *ctx, const nvca_part_params *params, const nvca_cascade *face,
                             const nvca_cascade *a, const nvca_cascade *b, nvca_part_stream **out);
/* The same stream on cascades of either format: each of face, a and b may be an old-format cascade or a new-format LBP cascade, in
 * any mixture (opencv_traincascade -featureType LBP files, OpenCV's lbpcascade_profileface.xml).  Same arguments, same refusals; on
 * three old-format cascades the stream is nvca_part_stream_create's.  A search on an LBP cascade is what
 * cv::CascadeClassifier::detectMultiScale does with a new-format file behind it: the element's flags are ignored
 * (CV_HAAR_FIND_BIGGEST_OBJECT and CV_HAAR_SCALE_IMAGE make no difference), the call's own scale factor, minNeighbors, minSize and
 * maxSize apply, and the raw list is grouped with groupRectangles(max(minNeighbors, 1), 0.2).  Everything downstream (process, the
 * batched call, submit / collect, set_input, set_params, push_faces, frames shared between streams) serves both; streams of either
 * kind mix in one call, and their small searches share one launch per round. */
int  nvca_part_stream_create_any(nvca_ctx *ctx, const nvca_part_params *params, const nvca_cascade *face,
                                 const nvca_cascade *a, const nvca_cascade *b, nvca_part_stream **out);
void nvca_part_stream_destroy(nvca_part_stream *s);
int  nvca_part_stream_set_params(nvca_part_stream *s, const nvca_part_params *params);
/* The pixel format of the stream's frames, as nvca_face_stream_set_input: NV12 / I420 frames are converted where the working-image
 * kernels read them -- cv::cvtColor(CV_YUV2BGR_NV12 / _I420) in front of the element's own order, cvtColor then resize then
 * equalizeHist (NOSE/kmsnosedetect.cpp:836-841, MOUTH/kmsmouthdetect.cpp:842-847, EAR/kmseardetect.cpp:787-792; EYE/kmseyedetect.cpp:948-956:
 * the full-size gray image is equalized first).  Results are those of the same stream fed the converted BGR frame, bit for bit;
 * boxes and pushed faces stay in original-frame pixels.  layout == NULL or format NVCA_PIX_BGR: back to packed BGR.  The layout holds
 * from the next nvca_part_stream_process / nvca_part_batch_process / _submit on; a submitted ticket keeps the layout it was submitted
 * with.  Packed, NV12 and I420 streams mix in one call; streams share a frame's upload and work only when the layout is equal too.
 * A frame of a 4:2:0 stream is refused with NVCA_ERR_ARG -- the whole call, before any stream's frame gate advances -- when its
 * width or height is odd, its stride is not the layout's stride[0], a plane's stride is shorter than its row, or planes overlap.
 * Packed 4:2:2 frames (NVCA_PIX_YUY2 / _UYVY / _YVYU: cv::cvtColor(CV_YUV2BGR_YUY2 / _UYVY / _YVYU) in front of the same order,
 * SURVEY.md A.18) by the same rules: an even width, any height, stride[0] >= 2 * width; they mix with the others in one call. */
int  nvca_part_stream_set_input(nvca_part_stream *s, const nvca_pixel_layout *layout);
/* one upstream "message" worth of faces, original-frame pixels (EYE/kmseyedetect.cpp:680-764) */
int  nvca_part_stream_push_faces(nvca_part_stream *s, const nvca_rect *faces, int n);
/* the face list the last processed frame worked with (working-image pixels of the face pass, or the pushed
 * faces): what kms_mouth_send_event / kms_ear_send_event put into their events */
int  nvca_part_stream_faces(const nvca_part_stream *s, nvca_rect *out, int cap, int *n_out);
/* One transform_frame_ip.  List A: eyes_r / noses / mouths / left ears; list B: eyes_l / right ears. */
int  nvca_part_stream_process(nvca_part_stream *s, const nvca_frame *frame_bgr, nvca_rect *out_a, int cap_a,
                              int *n_a, nvca_rect *out_b, int cap_b, int *n_b);

/* Batched frontend for the part detectors (BASELINE config 3, the ROI chain): frame i belongs to streams[i] (a stream at most
 * once per call; the streams may be of different kinds).  The device work of all streams is queued together: one wait for
 * every face pass, one for every part search, instead of several per stream.  Streams handed the same frame (same data
 * pointer and geometry: the detectors of one video stream) share its upload and whatever they compute identically from it;
 * working images of all frames come out of one launch set per size, face passes run as N-image jobs.  Every frame is
 * validated before any stream's frame gate advances, and a call that fails later (a plan that cannot be built, an allocation,
 * a refused launch) restores every stream's gates, queued face events and lists before it returns: ANY error leaves all
 * streams as they were, and nothing of the call stays in flight.  Results are those of
 * nvca_part_stream_process per stream.  out_a is [n][cap_a], out_b [n][cap_b]. */
int  nvca_part_batch_process(nvca_ctx *ctx, int n, nvca_part_stream *const *streams, const nvca_frame *frames,
                             nvca_rect *out_a, int cap_a, int *n_a, nvca_rect *out_b, int cap_b, int *n_b);

/* The same call in two halves, for a serving loop that keeps the GPU busy between the waits of a call (the counterpart of
 * nvca_face_batch_submit / _collect; the reference has no such boundary: its elements run one frame at a time on their streaming
 * threads, kms*detect.cpp transform_frame_ip).  submit: the streams' frame gates, the working images and the face passes are
 * queued -- nothing is waited for -- and *ticket names the call; the frames must stay valid until the ticket is collected.
 * collect: the face passes' results, the part searches, the merging heuristics; outputs as nvca_part_batch_process.  Tickets are
 * collected in submit order (the streams' state machines advance in that order); at most two are outstanding, so the usual loop
 * is submit(k + 1), collect(k) on ONE serving thread (a synchronous nvca_part_batch_process takes one of the two slots while it runs: it is
 * refused while two tickets are outstanding).  A stream may appear in both outstanding calls (not in a synchronous nvca_part_batch_process /
 * nvca_part_stream_process while a ticket of its is outstanding: refused).  A collect that fails rolls its streams back as a
 * failed nvca_part_batch_process does and abandons a newer outstanding ticket with it (rolled back first); a ticket that is never
 * collected is rolled back when the context is destroyed -- or when one of its streams is (nvca_part_stream_destroy gives up every
 * outstanding call of the context first: their tickets become unknown). */
int  nvca_part_batch_submit(nvca_ctx *ctx, int n, nvca_part_stream *const *streams, const nvca_frame *frames, int *ticket);
int  nvca_part_batch_collect(nvca_ctx *ctx, int ticket, nvca_rect *out_a, int cap_a, int *n_a, nvca_rect *out_b, int cap_b, int *n_b);

/* ---- NuboTracker stream -------------------------------------------------
 * Replaces gst_nubo_tracker_img_conf + gst_nubo_tracker_process
 * (TRK/gstnubotracker.cpp:202-237, 339-421): BGRA -> gray, absdiff, threshold,
 * updateMotionHistory, segmentMotion, __join_objects.  img_prev is per stream
 * (the reference's process-global Mat, :108, is a bug). */
typedef struct nvca_tracker_params {
    int    threshold;     /* "set_threshold" 20  (:23) */
    int    min_area;      /* "set_min_area"  50  (:24) */
    long   max_area;      /* "set_max_area"  30000 (:25) */
    int    distance;      /* "set_distance"  35  (:26) */
    double mhi_duration;  /* MHI_DURATION 0.2 (:28) */
    double seg_thresh;    /* SEGMENTATION 32  (:31) */
} nvca_tracker_params;
void nvca_tracker_params_default(nvca_tracker_params *p);
int  nvca_tracker_create(nvca_ctx *ctx, const nvca_tracker_params *params, nvca_tracker **out);
void nvca_tracker_destroy(nvca_tracker *t);
int  nvca_tracker_set_params(nvca_tracker *t, const nvca_tracker_params *params);
/* The pixel format of the tracker's frames, as nvca_face_stream_set_input: NV12 / I420 frames are converted inside the pixel
 * pass -- cv::cvtColor(CV_YUV2BGR_NV12 / _I420) in front of the cvtColor of TRK/gstnubotracker.cpp:356 -- and the boxes are those of
 * the same tracker fed the converted frame as BGRA, bit for bit.  layout == NULL or format NVCA_PIX_BGR: back to packed BGRA.
 * nvca_frame.stride is the luma stride (stride >= width * 4 is asked of packed trackers only).  Previous gray image and motion
 * history persist across a format change at the same size.  Packed, NV12 and I420 trackers mix in one nvca_tracker_batch_process
 * (one launch set per size and format).  A bad frame (odd width or height, a stride that is not the layout's stride[0], a plane
 * stride shorter than its row, overlapping planes) refuses the whole call with NVCA_ERR_ARG before any tracker's state advances.
 * Packed 4:2:2 frames (NVCA_PIX_YUY2 / _UYVY / _YVYU: cv::cvtColor(CV_YUV2BGR_YUY2 / _UYVY / _YVYU) in front of :356)
 * by the same rules: an even width, any height (odd ones included), stride[0] >= 2 * width; one launch set per size and byte order. */
int  nvca_tracker_set_input(nvca_tracker *t, const nvca_pixel_layout *layout);
/* timestamp_ms: the reference passes 1000*clock()/CLOCKS_PER_SEC (:349) */
int  nvca_tracker_process(nvca_tracker *t, const nvca_frame *frame_bgra, double timestamp_ms,
                          nvca_rect *out, int cap, int *n_out);
int  nvca_tracker_batch_process(nvca_ctx *ctx, int n, nvca_tracker *const *trackers,
                                const nvca_frame *frames, const double *timestamps_ms,
                                nvca_rect *out, int cap, int *n_out);

#ifdef __cplusplus
}
#endif
#endif /* NUBOVCA_H */
