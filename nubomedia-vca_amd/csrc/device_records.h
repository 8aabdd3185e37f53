// device_records.h -- the plain records and constants that the host table builders (plan.cpp, detect.cpp, tracker.cpp) fill and
// the kernels read, and the arithmetic both sides size buffers with.  No HIP header: a plain C++ compiler reads this file.
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define NVCA_HD __host__ __device__
#else
#define NVCA_HD
#endif

namespace nvca {

// --------------------------------------------------------------------------
// Device-side records (plain structs shared by host table builder and kernels)
// --------------------------------------------------------------------------
struct StageRec {
    int first, count; float thr;
    int flags;              // bit 0: two_rects (every stump has 2 rects); bit 1: votes may be summed in any order;
                            // bit 2: every vote is an integer multiple of 2^vote_exp and the stage's sums stay below 2^31 of them:
                            // the tile kernels add the integer votes (TStumpRec::a0i / a1i) and compare with thr_i -- bit for bit
                            // the f64 sum OpenCV forms, whatever the order
    int thr_i;              // pass  <=>  integer sum >= thr_i   (== !(sum * 2^vote_exp < (double)thr))
    int vote_exp;
    int spec_run;           // stages from this one on, this one included, whose votes are exact in any order (flag bit 1): how far a
                            // round of the tile kernels may look ahead (tile_stages, several stages per round)
    int pad1;
};

struct ScaleRec {           // one evaluated scale
    int    winw, winh;
    int    plane_off;       // element offset of this scale's sum/sqsum planes inside a slot (0: the full-image planes)
    int    pitch;           // row pitch of those planes (elements)
    int    endX, endY;      // scan grid: ix in [0,endX), iy in [0,endY)
    int    eq[4];           // equRect corner offsets
    int    xpos_off, ypos_off;           // into the position tables (indexed by ix / iy)
    int    sq32;            // 1: the squared-pixel sum of the variance window is below 2^32 at this scale (ew * eh * 255^2):
                            //    the low-word plane alone gives it exactly (modulo-2^32 corner arithmetic)
    int    task_off;        // first stage-0 wave task (64 windows) of this scale
    int    wpr;             // wave tasks (64-bit reject words) per scan row
    int    adaptive;        // 1: OpenCV's adaptive x step applies (scale-cascade scan); 0: every grid point is visited
    double inv_area;
    double factor;
    const struct TStumpRec *trecs;   // the cascade's stumps at this scale's factor (device; shared by every plan that uses the factor)
    const struct GNodeRec *grecs;    // general cascades (tree weak classifiers / tilted features): every node at this scale's factor
    const struct LStumpRec *lrecs;   // the same stumps as trecs in the compact per-lane form (tile kernels: a stump per lane)
};

// A node of a weak classifier in its general form: up to three rectangles, upright (corners of the integral image) or
// tilted (corners of the tilted integral), a threshold and two children.  Corner offsets are window-relative pixels in the
// order + - - + (cvSetImagesForHaarClassifierCascade: p0 - p1 - p2 + p3), per (cascade, factor) like TStumpRec.
struct GNodeRec {
    short dx[3][4], dy[3][4];
    float w[3];
    float thr;
    int left, right;        // > 0: node index inside the weak classifier; <= 0: leaf, alpha index = -value (absolute)
    int flags;              // low byte: rectangles (2 or 3); bit 8: tilted
    int pad;
};
static_assert(sizeof(GNodeRec) == 80, "GNodeRec layout");

struct StripRec { int scale, iy0, nrows, ix0, ncols, pad0, pad1, pad2; };   // a block's share of the scan: nrows x ncols windows
// A tile is a block of nx x ny windows (<= 32 x 16) of one scale.  The windows of a scale only ever touch the integral
// image on a near-lattice of positions (window origin + scaled rectangle corner), a small fraction of the pixels they
// span; the tile kernel stages exactly those sample rows x columns, compacted, in LDS and looks corners up through a
// column map and a row map.  Tile size in windows is therefore the same at every scale.
struct TileRec {
    int scale, ix0, iy0, nx, ny;
    int x0, y0;             // plane coordinates of the tile's first window: origin of the maps
    int ncol, nrow;         // distinct sample columns / rows staged
    int span_x, span_y;     // map extents: the largest column / row offset from (x0, y0) ever looked up, + 1
    int col_off, row_off;   // first entry of the column / row coordinate lists (plane coordinates, u16) in `tcoords`
    int pad_t;
    int pad0, pad1;
};
struct TStumpRec {          // a stump with separate corner columns / rows (window-relative pixels)
    int x0[3], x1[3], y0[3], y1[3];
    float w[3];
    int nrect;              // low byte: rectangles (2 or 3); bits 8..11 "share": bit 8 / 9: rectangle 1 has rectangle 0's rows /
                            // columns; bit 10 / 11: rectangle 2 likewise
    double thr, a0, a1;
    int a0i, a1i;           // the votes as integers (a / 2^vote_exp of the stump's stage) where StageRec flag bit 2 is set
                            // 96 bytes: the tile kernels fetch a record with two wide scalar loads (16 + 8 dwords)
};
static_assert(sizeof(TStumpRec) == 96, "TStumpRec layout is read dword by dword in kernels_cascade_tile.hip");
// The same stump in 48 bytes, for lanes that each evaluate a DIFFERENT stump (the tile kernels once few windows of a wave are
// left: lane = (window, stump) pair): three 16-byte vector loads per lane instead of a record held in scalar registers.
// Corner coordinates are window-relative pixels TIMES TWO (byte offsets into the tile's u16 maps), low half = first corner;
// rectangle 2 is absent iff both its words are zero.  Threshold and votes are the file's floats (the kernels widen them
// exactly); a stage's stumps are in the order of the TStumpRec table.
struct alignas(16) LStumpRec {
    unsigned xx0, yy0, xx1, yy1, xx2, yy2;      // per rectangle: xx = 2 x0 | 2 x1 << 16, yy = 2 y0 | 2 y1 << 16
    float w0, w1, w2, thr, a0, a1;
};
static_assert(sizeof(LStumpRec) == 48, "LStumpRec is read as three int4 in kernels_cascade_tile.hip");
// A band is one row of tiles (<= 16 window rows of one scale, the full scan width): k_band walks it left to right in one
// workgroup, so stage 0 and OpenCV's adaptive x step (which depends on the stage-0 results to the left) need no pre-pass.
// Per scale: the distinct corner columns / rows (window-relative pixels) of the late stages' stumps.  k_deep stages that
// ncol x nrow patch of a surviving window in LDS after the first late stage (ncol == 0: scale not eligible, global gathers).
struct DeepRec { int col_off, ncol, row_off, nrow, span_x, span_y, pad0, pad1; };
static constexpr int kDeepMaxSide = 64;            // patch side (distinct columns / rows)
static constexpr int kDeepMaxSpan = 1280;          // largest corner offset + 1 the patch maps cover
struct BandRec { int scale, iy0, ny, first_tile, ntiles, pad0, pad1, pad2; };
static constexpr int kTileWin = 32;                 // windows per tile row (window id = ry * 32 + rx)
static constexpr int kTileRows = 16;                // window rows per tile
static constexpr int kTileSlots = kTileWin * kTileRows;   // windows per tile = queue capacity = threads of the tile kernels
// 512 threads: three tile workgroups take 24 of a CU's 32 wave slots (6 waves a SIMD, 80 registers each) -- the third tile
// fills the rounds that are chains of dependent LDS / L2 round trips; the bandwidth-bound pre-processing kernels
// of the next batch fit beside them without ever keeping a tile workgroup from starting
static constexpr int kTileThreads = kTileSlots;
static constexpr int kTilesPerCu = 3;               // tile workgroups resident per CU
static constexpr int kTileWavesPerSimd = (kTilesPerCu * kTileThreads / 64 + 3) / 4;     // the tile kernels' launch bounds (6: 80 VGPRs)
// three tiles resident per CU (160 KiB LDS) and 4 KiB left for small workgroups beside them.  Not more: with a 53 KiB budget
// (largest tile 54 260 B, three of them 1 KiB short of 160 KiB) the band kernel measured as with two tiles per CU
static constexpr int kTileLdsBudget = 52 * 1024;
static_assert(kTilesPerCu * kTileLdsBudget <= 160 * 1024 && kTilesPerCu * kTileThreads <= 32 * 64, "tile residency per CU");
static constexpr int kTileMaxCols = 256;            // staged columns per tile (4 per lane)
// LDS bytes the tile kernel needs for a tile (host sizing and kernel carve-up agree through these)
NVCA_HD inline int tile_pitch(int ncol) { return ncol | 1; }
// fixed part (carve_tile in kernels_cascade_tile.hip): stage accumulators (8 B a queue slot) | two window queues | window origins |
// counters and stage statistics (32 words: qn[0 .. 3] queue counters and list base, qn[4 .. 15] two sets of stage statistics,
// qn[16 .. 20] stump counts) | per-window variance normaliser
NVCA_HD inline int tile_lds_fixed()
{
    return kTileSlots * 8 + 2 * kTileSlots * 2 + 4 * kTileWin + 128 + kTileSlots * 8;
}
NVCA_HD inline int tile_lds_bytes(int ncol, int nrow, int span_x, int span_y)
{
    return 4 * nrow * tile_pitch(ncol) + 2 * ((span_x + 3) & ~3) + 2 * ((span_y + 3) & ~3) + tile_lds_fixed();
}

static constexpr int kStripMaxWin = 512;   // windows per strip (LDS budget of the evaluator)
static constexpr int kIntegralBand = 16;   // rows per integral band

// ---- pre-processing (kernels_gray.hip / kernels_equalize.hip / kernels_integral.hip)
struct PreGeom {
    int sw, sh, sstride, cn;      // source frame
    int w, h, gpitch;             // working gray image (pitch in bytes)
    int spitch;                   // integral pitch (elements), rows = h+1
    int nbands;
    size_t src_slot, gray_slot, sum_slot, band_slot;   // strides between batch slots (elements of each plane)
};
// planes of a 4:2:0 source frame (nvca_pixel_layout as the kernels read it): fmt 0 = packed BGR (nothing else is used), 1 = NV12
// (off_u: the U,V plane; off_v unused), 2 = I420.  Offsets count from the frame's base pointer; the luma stride is PreGeom::sstride.
struct YuvPlanes {
    int fmt, cstride, vstride, pad;      // chroma stride (NV12: of the interleaved plane; I420: of U), I420's V stride
    long long off_y, off_u, off_v;
};
// the six values of one cv::resize(INTER_LINEAR) geometry on 8-bit images, wherever its tables lie (host vectors: ResizeTab::view,
// device buffers: GeomPlan::view, a launch's table blob: k_roi).  mode 0 identity (no table is read), 1 bilinear, 2 area 2x2 (no
// table is read).  What resize_sample (pixel_rules.h) and every kernel that resizes take.
struct ResizeView {
    int mode, xmax;               // xmax: first destination column whose right-hand source column does not exist
    const int *xofs; const short *ialpha; const int *yofs; const short *ibeta;      // [dw], [2 dw], [dh], [2 dh]
};
// one pyramid level of a CV_HAAR_SCALE_IMAGE scan (device copy): all levels are resized / integrated by one launch each
struct PyrLevelDev {
    int szw, szh, gpitch, plane_off;
    long long gray_off;
    ResizeView tab;
};

// ---- tracker (kernels_trk_pixel.hip, kernels_trk_ccl.hip); the layout of its work buffers: trk_layout.h ----
struct TrkSlot {                // per tracker in the batch
    const uint8_t *src;         // BGRA frame; 4:2:0 trackers (nvca_tracker_set_input): the base `yuv`'s plane offsets count from
    uint8_t *prev;              // previous gray  [h][w]
    float *mhi;                 // motion history [h][w]
    float ts, delbound;         // (float)timestamp, (float)(timestamp - duration)
    float seg;                  // (float)seg_thresh
    int threshold;
    int has_prev;               // num_frames > 0
    int sstride;
    int min_area;               // __join_objects drops boxes outside (min_area, max_area) before anything else:
    long long max_area;         // k_ccl_emit / k_ccl_collect do not even report them (report_component)
    YuvPlanes yuv;              // planes of a 4:2:0 frame (the luma stride is sstride); unused by the packed kernels
};
struct CompAcc { int minx, miny, maxx, maxy, seed, pad; };   // per root, stored at the root's pixel index

// A candidate's key is scale << key_ss | row << key_sy | column of its window, each field as wide as the plan's own grids need
// (CascadeArgs / LbpArgs: key_sy = bx, key_ss = bx + by): the widths for grids of at most max_nx x max_ny windows on nscales
// scales.  A field is at least one bit wide; whether the three fit a key is the caller's refusal.
inline int key_field_bits(size_t n) { int b = 1; while ((1ull << b) < n) b++; return b; }
inline void candidate_key_bits(size_t max_nx, size_t max_ny, size_t nscales, int *bx, int *by, int *bs)
{
    *bx = key_field_bits(max_nx); *by = key_field_bits(max_ny); *bs = key_field_bits(nscales);
}

struct CascadeArgs {
    const int *sum; const unsigned long long *sqsum;
    size_t sum_slot;               // elements between slots
    int spitch;
    const ScaleRec *scales; const StageRec *stages;
    const StripRec *strips; const int *pos;
    const int *order; int blocks_per_frame;   // k_strip dispatch slot -> strip
    const TileRec *tiles; const int *tile_order; int tile_blocks_per_frame;   // k_tile
    const unsigned short *tcoords; int tile_lds;
    const BandRec *bands; const int *band_order; int band_blocks_per_frame; int batch; int band_map;  // k_band
    const DeepRec *deeprecs;                  // [nscales] or null (k_deep: LDS patches)
    int nscales;
    const unsigned *tasks; int ntasks;        // k_stage0 wave tasks: scale << 20 | iy << 7 | word
    unsigned long long *failbits;             // [batch][ntasks] stage-0 reject bits
    double *vnf;                              // [batch][ntasks*64] variance normaliser per window
    int nstages; int pair_policy;  // 1 = F32PAIR
    int stage_order;               // Switches::stage_order
    int *stage_hint;               // [8] per plan: the stat words (order | entered << 16 | passed per stage) the last tile that finished left -- where a band's first tile and the per-tile kernel start from (an intentionally racy hint: plain stores, validated before use)
    int spec_pairs;                // Switches::spec_pairs
    int pair_max;                  // Switches::pair_max (<= kPairMax)
    const float *stage_thr;        // [nstages + 8]: StageRec::thr of every stage (tile_stages reads eight at once)
    const int *stage_first;        // [nstages + 1 + 8]: first stump of every stage, the stump count, then INT_MAX padding (tile_stages reads eight entries at once)
    int deep_stage;                // first stage evaluated by k_deep (== nstages: the tile kernels walk the whole cascade, k_deep is not launched)
    int deep_lds;                  // bytes of k_deep's largest window patch (dynamic LDS)
    unsigned long long *deep;      // deep[0] = count, then (slot << 32) | key
    unsigned deep_cap;
    int key_sy, key_ss;            // a candidate's key = scale << key_ss | iy << key_sy | ix: the plan sizes the three fields for its own grids (DetectPlan::key_sy / key_ss), so a ladder of hundreds of scales (multi-scale-factor 1 .. 4) fits next to small grids and a 4K grid next to 25 scales
    unsigned long long *hits;      // hits[0] = running count, hits[1..cap] = (slot << 32) | key
    unsigned hit_cap;
    // general cascades (k_gen_stage0 / k_gen_rest)
    const int *tilted;             // tilted integral planes, laid out like sum (null: the cascade has no tilted feature)
    const float *galpha;           // leaf values of every weak classifier, concatenated
    const int *gcls_first;         // first node of weak classifier c
    int stump_based;
#ifdef NVCA_STAMPS
    unsigned long long *dbg;       // diagnostic build only: per-phase s_memtime stamps of the first workgroups (scripts/stamps.py)
#endif
};

// ---- new-format LBP cascades (kernels_cascade_lbp.hip)
// A weak classifier as the evaluator reads it, wave-uniform (scalar loads): the 16 corners of its feature's 3 x 3 cells as element
// offsets from the window's origin at ONE pitch (corner (r, c) at off[r * 4 + c]), the subset, the two leaves.  A plan holds the table
// twice: at the pitch of the levels' sum planes and at the pitch of the stage-0 kernel's LDS tile.
struct LbpWeakDev { int off[16]; int subset[8]; float leaf[2]; int pad[6]; };
static_assert(sizeof(LbpWeakDev) == 128, "LbpWeakDev is fetched with wide scalar loads");
struct LbpStageDev { int first, count; float thr; int pad; };
// outputRejectLevels (k_lbp_levels / k_hnew_levels): what an emitted window carries beside its key, under the key's index of the
// candidate list -- the stage that rejected it (nstages: none) and that stage's sum, an LBP cascade's f32 sum widened
struct LevelRec { int level, pad; double weight; };
// one pyramid level's scan grid: window origins (gx * step, gy * step), gx < nx, gy < ny; its stage-0 pass bits lie at
// bits[bit_off + gy * wpr + (gx >> 5)], bit gx & 31; row_first: the level's first row in the walk kernel's row numbering
struct LbpLevelDev { int plane_off, szw, szh, nx, ny, step, wpr, bit_off, row_first, pad0, pad1, pad2; };
struct LbpTile { int level, tx, ty, pad; };       // 32 x 16 grid positions of a level from (tx * 32, ty * 16)
static constexpr int kLbpTileW = 32, kLbpTileH = 16;
// the stage-0 tile of the level's sum plane: every corner a 32 x 16-window tile reads at step 2 (step-1 tiles use its top-left part)
NVCA_HD inline int lbp_tile_pitch(int ow) { return (kLbpTileW - 1) * 2 + ow + 1; }
NVCA_HD inline int lbp_tile_rows(int oh, int step) { return (kLbpTileH - 1) * step + oh + 1; }
struct LbpArgs {
    const int *sum;                 // the levels' sum planes; image b's at sum + b * plane_total
    int nimg;                       // images of the job: they share every launch and every table
    size_t plane_total, bit_words;  // elements between two images' planes / u32 words between their pass bits
    int P, TP;                      // pitch of the planes / of the LDS tile (elements)
    int ow, oh;
    const LbpLevelDev *levels; int nlev;
    const LbpStageDev *stages; int nstages;
    const LbpWeakDev *gweak, *tweak;        // offsets at pitch P / at pitch TP
    const LbpTile *tiles; int ntiles;
    unsigned *bits, *bits2;         // per grid position of every level: passed stage 0 / passed the tile kernel's stages; image b's at + b * bit_words
    int tile_stages;                // stages the tile kernel evaluates (the first min(nstages, 3))
    int nrows;                      // scan rows of all levels (of one image)
    int key_sy, key_ss;             // candidate key = level << key_ss | gy << key_sy | gx
    unsigned *cnt;                  // [0]: entries of the list the walk kernel fills, [g]: of the list stage group g leaves
    unsigned long long *list[2]; unsigned list_cap;   // survivors of ALL images as img << 32 | key, ping-pong between stage groups
    unsigned long long *hits; unsigned hit_cap;       // hits[0] = exact count, hits[1 .. cap] = img << 32 | key (the job's one list)
};

// ---- new-format HAAR cascades (kernels_cascade_hnew.hip): the scan, its levels, tiles, stages, bit planes, lists and
// keys are the LBP evaluator's (LbpArgs, `l` below; k_lbp_walk runs on it as it is); the weak classifier is a stump on a Haar feature
// at window scale 1 and every window has a variance normaliser.
// A weak classifier, wave-uniform (scalar loads, five dwordx4): per rect the corners (x, y), (x + w, y), (x, y + h), (x + w, y + h) as
// element offsets from the window's origin at ONE pitch (rect r at off[4 r ..]; a missing rect: four zeros, weight 0), the weights, the
// stump's threshold and leaves.  A plan holds the table at the planes' pitch and at the stage-0 tile's.
struct alignas(16) HnewWeakDev { int off[12]; float w[3]; float thr; float leaf[2]; int pad[2]; };
static_assert(sizeof(HnewWeakDev) == 80, "HnewWeakDev is fetched with wide scalar loads");
struct HnewArgs {
    LbpArgs l;                      // (gweak / tweak unused)
    const HnewWeakDev *gweak, *tweak;       // offsets at pitch P / at pitch TP
    // the squared integral of the levels as the pyramid launchers leave it: image b's u32 low-word planes at sq + b * 2 * plane_total,
    // its u8 high-byte planes in the plane_total words behind them.  A level's low words lie at + plane_off elements; its high bytes at
    // + hi_mul * plane_off BYTES of the high-byte region: 1 where one launch integrates every level (k_pyr_integral), 4 where the levels
    // are integrated one by one (a plan with a level wider than 1023: each launch is handed the level's low-word plane and puts the
    // high bytes plane_total words behind THAT)
    const unsigned *sq;
    int hi_mul, pad;
    int nr[4], nrt[4];              // normrect (1, 1, ow - 2, oh - 2): its four corners in off[]'s order at pitch P / at pitch TP
    double area;                    // (ow - 2) * (oh - 2)
};

// ---- general new-format HAAR cascades (kernels_cascade_hgen.hip): the scan above with tree weak classifiers and
// tilted features.  A node, wave-uniform (scalar loads, nine dwordx4): its feature's corners as HnewWeakDev has them, at BOTH pitches
// (off: the planes' P, offt: the stage-0 tile's TP); a tilted feature's corners are (x, y), (x - h, y + h), (x + w, y + w),
// (x + w - h, y + w + h) -- the same p0 - p1 - p2 + p3 on the level's tilted plane, which is read at pitch P always.  left / right: where
// a window goes for value < thr / otherwise -- the child's index in the plan's node table (no tree base is added in the walk), or -1
// for a leaf, whose value is lv[0] / lv[1] then: a leaf is held by the node that ends in it, so the walk needs no leaf table.
struct alignas(16) HgenNodeDev { int off[12]; int offt[12]; float w[3]; float thr; int left, right, tilted, pad; float lv[2]; int pad2[2]; };
static_assert(sizeof(HgenNodeDev) == 144, "HgenNodeDev is fetched with wide scalar loads");
struct HgenWeakDev { int first, count; };          // a weak classifier's nodes in the node table: the root first, children behind parents
struct HgenArgs {
    HnewArgs h;                     // (h.gweak / h.tweak unused)
    const HgenNodeDev *nodes;
    const HgenWeakDev *weak;        // a stage's first / count index this table
    const int *tilted;              // the levels' tilted planes, laid out as l.sum; null when no feature is tilted (none is read then)
};

// ---- detectMultiScale on a small image in one workgroup (kernels_roi.hip)
struct RoiStep {                  // one ladder step (scale-cascade scan) or one pyramid level (CV_HAAR_SCALE_IMAGE) of a job
    const TStumpRec *trecs;       // the cascade's stumps at this step's factor (levels: factor 1)
    int ex, ey, ew, eh;           // variance rectangle (window-relative)
    int startX, endX, startY, endY;   // scale-cascade: grid indices, window origin = cvRound(i * ystep); levels: origins 0 .. end, every `step` pixels
    int step, adaptive, job, key_step;    // job: index of the step's job in the launch; key_step: the step's number inside its job (a candidate's key carries it; a step with many rows goes out as several records -- one workgroup each -- with the same number)
    int key_x0, key_dx, key_y0, key_dy;   // a candidate's key: column key_x0 + gx * key_dx, row key_y0 + gy * key_dy (grid indices, or level origins)
    int szw, szh;                 // level size
    int mode, xmax, xofs_off, yofs_off, ialpha_off, ibeta_off;      // the level's cv::resize tables (byte offsets into the launch's table blob)
    double inv_area, ystep;
    // adaptive == 2 ("dense", FIND_BIGGEST searches): every window that passes stage 0 goes on, visited by the serial walk or not, and the
    // stage-0 reject bits of the step's grid are written out -- row r's chunk c at rej[rej_off + r * rej_wpr + c] (64 windows a word) -- so
    // that the host can replay the walk from ANY start column: a narrowed re-scan needs no second launch (detect.cpp, fb_replay)
    int rej_off, rej_wpr;
};
struct RoiJobDev {
    const uint8_t *img; int w, h, stride;
    int first_step, nsteps, scale_image;
    const StageRec *stages; int nstages, pair_policy;
    int slot, pad;
};
static constexpr int kRoiMaxWin = 2048;           // windows of one ladder step / pyramid level of a small-image job

// ---- detectMultiScale of a new-format LBP cascade on a small image in one workgroup (kernels_roi_lbp.hip).  A job is a RoiJobDev
// (scale_image == 2; `stages` points at the cascade's RoiLbp table: nstages LbpStageDev, then -- at roi_lbp_weak_off(nstages) bytes --
// its weak classifiers), a level or a band of a level's rows a RoiStep as CV_HAAR_SCALE_IMAGE's (trecs, the variance rectangle and
// adaptive unused).  The level's plane lives in LDS at its own pitch, so a weak classifier keeps its feature rectangle and the kernel
// forms the sixteen corner offsets: (y + r h) * pitch + x + c w.
struct RoiLbpWeak { int x, y, w, h; int subset[8]; float leaf[2]; int pad[2]; };
static_assert(sizeof(RoiLbpWeak) == 64, "RoiLbpWeak is fetched with one wide scalar load");
NVCA_HD inline size_t roi_lbp_weak_off(int nstages) { return ((size_t)nstages * sizeof(LbpStageDev) + 63) & ~(size_t)63; }
// A stage on a short queue: at most kRoiLbpShortWin windows and at most kRoiLbpVoteWords votes (weak classifiers x windows padded to
// whole waves) run a wave per (weak classifier, 64 windows), every vote stored to LDS, and one lane per window adds the stage's votes in
// file order -- the same f32 additions as a window per lane.  0 switches the form off.
#ifndef NVCA_ROI_LBP_SHORT_WIN
#define NVCA_ROI_LBP_SHORT_WIN 256
#endif
static constexpr int kRoiLbpShortWin = NVCA_ROI_LBP_SHORT_WIN;
static constexpr int kRoiLbpVoteWords = 4096;
// k_roi_lbp's dynamic LDS (host sizing and kernel carve-up agree through this): sum plane | two queues | counters | votes | level image,
// every part a multiple of 16 bytes
NVCA_HD constexpr int roi_lbp_fixed_bytes() { return 2 * kRoiMaxWin * 2 + 16 + kRoiLbpVoteWords * 4; }
NVCA_HD constexpr int roi_lbp_lds_bytes(int plane_words, int lev_bytes) { return ((plane_words + 3) & ~3) * 4 + roi_lbp_fixed_bytes() + ((lev_bytes + 15) & ~15); }

// ---- detectMultiScale of a new-format HAAR cascade on a small image in one workgroup (kernels_roi_hnew.hip), for the
// cascades opted in through nvca_cascade_set_small_route.  A job is a RoiJobDev (scale_image == 3; `stages` points at the cascade's
// RoiHnew table: nstages LbpStageDev, then -- at roi_hnew_weak_off(nstages) bytes -- its weak classifiers), a level or a band of a
// level's rows a RoiStep as k_roi_lbp's.  The level's planes live in LDS at the level's own pitch, so a weak classifier keeps its
// RECTANGLES (x, y, w, h) and the kernel forms the twelve corner offsets in scalar registers; a missing rect is all zero with weight 0.
struct alignas(16) RoiHnewWeak { int rect[3][4]; float w[3]; float thr; float leaf[2]; int pad[2]; };
static_assert(sizeof(RoiHnewWeak) == 80, "RoiHnewWeak is fetched with wide scalar loads, as HnewWeakDev");
NVCA_HD inline size_t roi_hnew_weak_off(int nstages) { return ((size_t)nstages * sizeof(LbpStageDev) + 63) & ~(size_t)63; }
// A stage on a short queue (at most kRoiHnewShortWin windows): a wave per (stump, 64 windows), the f32 leaf each window's vote selected
// stored to LDS, one lane per window adding them in file order into its f64 sum -- the same additions as a window per lane.  A stage
// with more votes than kRoiHnewVoteWords runs in consecutive chunks of stumps, the partial sum carried in the owning lane's register.
// 0 switches the form off.
#ifndef NVCA_ROI_HNEW_SHORT_WIN
#define NVCA_ROI_HNEW_SHORT_WIN 256
#endif
static constexpr int kRoiHnewShortWin = NVCA_ROI_HNEW_SHORT_WIN;
static constexpr int kRoiHnewVoteWords = 4096;
static_assert(kRoiHnewShortWin <= kRoiHnewVoteWords, "a chunk holds one stump's votes of the longest short queue at least");
// k_roi_hnew's dynamic LDS (host sizing and kernel carve-up agree through this): sum plane | squared plane | two queues | counters |
// votes | vnf (an f64 per grid position of the band), every part a multiple of 16 bytes.  The resized level image (bytes, dead once the
// planes stand) lies OVER votes + vnf: kRoiHnewLevBytes of room.
static constexpr int kRoiHnewLevBytes = kRoiHnewVoteWords * 4 + kRoiMaxWin * 8;
NVCA_HD constexpr int roi_hnew_fixed_bytes() { return 2 * kRoiMaxWin * 2 + 16 + kRoiHnewLevBytes; }
NVCA_HD constexpr int roi_hnew_lds_bytes(int plane_words) { return 2 * ((plane_words + 3) & ~3) * 4 + roi_hnew_fixed_bytes(); }

} // namespace nvca
