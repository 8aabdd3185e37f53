// san_driver.cpp -- test infrastructure (never shipped): runs the product's pure-host sources -- cascade_xml.cpp (the loader),
// plan.cpp (table builders), host_logic.cpp (groupRectangles, track_faces, __join_objects, the part detectors' merging
// heuristics) and fb_search.cpp (the FIND_BIGGEST search) -- under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU.  tests/test_host_sanitizers.py builds it
// (clang++ -fsanitize=address,undefined, the product sources compiled as they are) and checks what it prints against the
// oracle.  The GPU pool has no sanitizer support (ASan / XNACK are refused there), so this is where memory errors of the host
// code are looked for.
//
// The three sources reach the HIP runtime through a handful of calls (table uploads); the driver links no HIP library and
// supplies host doubles for exactly those calls: a "device" buffer is a malloc'd block.  Nothing here runs a kernel.
#include "../../nubomedia-vca_amd/csrc/plan.h"
#include "../../nubomedia-vca_amd/csrc/host_logic.h"
#include "../../nubomedia-vca_amd/csrc/fb_search.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <set>
#include <algorithm>

// ---- host doubles of what runtime.cpp / plans.cpp / api.cpp / the HIP runtime provide to these sources -------------------
extern "C" hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind) { memcpy(dst, src, n); return hipSuccess; }
extern "C" hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
extern "C" hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
namespace nvca {
struct Workspace { int unused; };
struct GeomPlan { int unused; };
int DevBuf::ensure(size_t n) { if (n <= bytes) return 0; free(p); p = malloc(n); bytes = p ? n : 0; return p ? 0 : 1; }
void DevBuf::release() { if (p && bytes) free(p); p = nullptr; bytes = 0; }
DetectPlan::~DetectPlan() { release_tables(); d_blob.release(); }
}
nvca_ctx::nvca_ctx() {}
nvca_ctx::~nvca_ctx() { plans.clear(); nvca::free_scale_tables(this); }

using namespace nvca;

static unsigned long long g_rng = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(g_rng >> 33); }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (unsigned)(hi - lo + 1)); }

static std::string slurp(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    std::stringstream ss; ss << f.rdbuf();
    return ss.str();
}

static int fail(const char *what) { fprintf(stderr, "san_driver: FAILED: %s\n", what); return 1; }

// ---- loader ------------------------------------------------------------------------------------------------------------
static int run_loader(int argc, char **argv)
{
    for (int i = 0; i < argc; i++) {
        const std::string xml = slurp(argv[i]);
        Cascade c; std::string err;
        const int rc = parse_cascade_xml(xml.data(), xml.size(), c, err);
        printf("{\"loader\": \"%s\", \"rc\": %d, \"ow\": %d, \"oh\": %d, \"stages\": %zu, \"cls\": %zu, \"nodes\": %zu, \"alpha\": %zu, \"tilted\": %d, \"stumps\": %d}\n",
               argv[i], rc, c.ow, c.oh, c.stages.size(), c.cls.size(), c.nodes.size(), c.alpha.size(), c.has_tilted ? 1 : 0, c.stump_based ? 1 : 0);
        // damaged copies: any status will do, memory safety is the point.  Byte flips, truncations, digit runs blown up.
        int statuses[3] = {0, 0, 0};
        for (int t = 0; t < 160; t++) {
            std::string b = xml;
            const int kind = t % 4;
            if (kind == 0) for (int k = rnd_in(1, 10); k > 0; k--) b[rnd() % b.size()] = (char)rnd();
            else if (kind == 1) b.resize(rnd() % b.size());
            else if (kind == 2) { const size_t at = rnd() % b.size(); b.insert(at, "99999999999"); }
            else { const size_t at = rnd() % b.size(), n = rnd() % 200; b.erase(at, std::min(n, b.size() - at)); }
            Cascade d; std::string e2;
            const int r = parse_cascade_xml(b.data(), b.size(), d, e2);
            statuses[r == NVCA_OK ? 0 : (r == NVCA_ERR_PARSE ? 1 : 2)]++;
            if (r == NVCA_OK) {          // what the loader accepts must be internally consistent: the builders index it blindly
                for (const HaarClassifier &hc : d.cls) {
                    if (hc.first_node < 0 || hc.first_node + hc.nnodes > (int)d.nodes.size() || hc.first_alpha + hc.nnodes + 1 > (int)d.alpha.size()) return fail("accepted cascade with out-of-range classifier");
                    for (int l = 0; l < hc.nnodes; l++) {
                        const HaarNode &n = d.nodes[hc.first_node + l];
                        if (n.left > 0 && (n.left <= l || n.left >= hc.nnodes)) return fail("accepted tree with a backward child");
                        if (n.right > 0 && (n.right <= l || n.right >= hc.nnodes)) return fail("accepted tree with a backward child");
                        if (n.left <= 0 && -n.left > hc.nnodes) return fail("leaf index out of range");
                        if (n.right <= 0 && -n.right > hc.nnodes) return fail("leaf index out of range");
                    }
                }
                for (const HaarStage &st : d.stages) if (st.first_cls < 0 || st.first_cls + st.ncls > (int)d.cls.size()) return fail("accepted cascade with out-of-range stage");
            }
        }
        printf("{\"loader_fuzz\": \"%s\", \"ok\": %d, \"parse\": %d, \"other\": %d}\n", argv[i], statuses[0], statuses[1], statuses[2]);
    }
    return 0;
}

// ---- fbsearch ----------------------------------------------------------------------------------------------------------
// FbSearch (fb_search.cpp) fed the three ways the library feeds it, against a plain serial restatement of the FIND_BIGGEST loop of
// cvHaarDetectObjectsForROC -- over a synthetic window predicate instead of a cascade.
struct FbObj { int x, y, w, h; };
struct FbCase {
    int ow, oh, cols, rows; double sf; int minw, minh, maxw, maxh, mn; bool rough;
    unsigned seed; double p_rej0, p_noise; std::vector<FbObj> objs;
};
struct FbCounts { int narrowed = 0, narrowed_steps = 0, narrowed_hits = 0, below_min = 0; };

// the window predicate, a deterministic function of (ladder step, ix, iy): 0 = rejected by stage 0, -1 = rejected later, 1 = passes.
// Around a planted object (origin within 12 % of its size, width 0.85 .. 1.2 of its width) most windows pass and some are rejected
// by stage 0, so that groups form and a walk that starts at another column sees other windows.
static int fb_pred(const FbCase &c, int step, int ix, int iy, int x, int y, int winw)
{
    unsigned long long h = c.seed * 0x9E3779B97F4A7C15ull + (unsigned long long)step * 0xC2B2AE3D27D4EB4Full + (unsigned long long)ix * 0x165667B19E3779F9ull + (unsigned long long)iy * 0x27D4EB2F165667C5ull;
    h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32; h *= 0x94D049BB133111EBull; h ^= h >> 29;
    const double u = (double)(h >> 11) / 9007199254740992.0;
    for (const FbObj &o : c.objs)
        if (winw >= 0.85 * o.w && winw <= 1.2 * o.w && abs(x - o.x) <= 0.12 * o.w && abs(y - o.y) <= 0.12 * o.h) return u < 0.70 ? 1 : (u < 0.85 ? 0 : -1);
    return u < c.p_rej0 ? 0 : (u > 1. - c.p_noise ? 1 : -1);
}

static int fb_cvr(double v) { return (int)lrint(v); }
static std::vector<nvca_rect> fb_biggest(std::vector<nvca_rect> &all, int mn)
{
    group_rectangles(all, std::max(mn, 1), 0.2);
    std::vector<nvca_rect> out;
    if (!all.empty()) {
        nvca_rect best{0, 0, 0, 0};
        for (const nvca_rect &r : all) if (r.w * r.h > best.w * best.h) best = r;
        out.push_back(best);
    }
    return out;
}

// the loop itself, as OpenCV runs it: one step after the other, from the largest factor down
static std::vector<nvca_rect> fb_serial(const FbCase &c, FbCounts &n, std::vector<nvca_rect> &all)
{
    all.clear(); nvca_rect scanROI{0, 0, 0, 0};
    int minw = c.minw, minh = c.minh, n_factors = 0; double factor = 1;
    for (; factor * c.ow < c.cols - 10 && factor * c.oh < c.rows - 10; n_factors++, factor *= c.sf)
        ;
    const double sf = 1. / c.sf; factor *= sf;
    for (int step = 0; n_factors-- > 0; factor *= sf, step++) {
        const double ystep = std::max(2., factor);
        const int winw = fb_cvr(c.ow * factor), winh = fb_cvr(c.oh * factor);
        int startX = 0, startY = 0, endX = fb_cvr((c.cols - winw) / ystep), endY = fb_cvr((c.rows - winh) / ystep);
        if (winw < minw || winh < minh) break;
        if (winw > c.maxw || winh > c.maxh) continue;
        const bool narrowed = scanROI.w * scanROI.h > 0;
        if (narrowed) {
            startY = fb_cvr(scanROI.y / ystep); endY = fb_cvr((scanROI.y + scanROI.h - winh) / ystep);
            startX = fb_cvr(scanROI.x / ystep); endX = fb_cvr((scanROI.x + scanROI.w - winw) / ystep);
        }
        int windows = 0, found = 0;
        for (int iy = startY; iy < endY; iy++)
            for (int ix = startX; ix < endX;) {
                const int x = fb_cvr(ix * ystep), y = fb_cvr(iy * ystep);
                int result = -1;                    // cvRunHaarClassifierCascadeSum outside the image
                if (!(x < 0 || y < 0 || x + winw >= c.cols + 1 || y + winh >= c.rows + 1)) { result = fb_pred(c, step, ix, iy, x, y, winw); windows++; }
                if (result > 0) { all.push_back(nvca_rect{x, y, winw, winh}); found++; }
                ix += result != 0 ? 1 : 2;
            }
        if (narrowed && windows) { n.narrowed_steps++; n.narrowed_hits += found; if (winw < c.minw || winh < c.minh) n.below_min = 1; }
        if (!all.empty() && scanROI.w * scanROI.h == 0) {
            std::vector<nvca_rect> tmp(all);
            group_rectangles(tmp, std::max(c.mn, 1), 0.2);
            if (!tmp.empty()) {
                nvca_rect maxRect{0, 0, 0, 0};
                for (const nvca_rect &r : tmp) if (r.w * r.h > maxRect.w * maxRect.h) maxRect = r;
                all.push_back(maxRect);
                scanROI = maxRect;
                const int dx = fb_cvr(maxRect.w * 0.2), dy = fb_cvr(maxRect.h * 0.2);
                scanROI.x = std::max(scanROI.x - dx, 0); scanROI.y = std::max(scanROI.y - dy, 0);
                scanROI.w = std::min(scanROI.w + dx * 2, c.cols - 1 - scanROI.x);
                scanROI.h = std::min(scanROI.h + dy * 2, c.rows - 1 - scanROI.y);
                const double minScale = c.rough ? 0.6 : 0.4;
                minw = fb_cvr(maxRect.w * minScale); minh = fb_cvr(maxRect.h * minScale);
                n.narrowed = 1;
            }
        }
    }
    return fb_biggest(all, c.mn);
}

// what a launch of the library reports for one grid: the hits of the serial walk of every row (`tag` numbers the scale)
static void fb_walk(const FbCase &c, const FbStep &st, int li, const ScanGrid &g, int tag, std::vector<nvca_rect> &raw, std::vector<int> &sc)
{
    for (int iy = g.startY; iy < g.endY; iy++)
        for (int ix = g.startX; ix < g.endX;) {
            const int x = fb_cvr(ix * st.ystep), y = fb_cvr(iy * st.ystep);
            const int result = fb_pred(c, li, ix, iy, x, y, st.winw);
            if (result > 0) { raw.push_back(nvca_rect{x, y, st.winw, st.winh}); sc.push_back(tag); }
            ix += result != 0 ? 1 : 2;
        }
}

enum { kFeedPlan, kFeedSmall, kFeedDense };
static bool fb_fed(const FbCase &c, int feed, std::vector<nvca_rect> &out, std::vector<nvca_rect> &groups, int *second_set)
{
    FbSearch fb;
    struct Groups { FbSearch &fb; std::vector<nvca_rect> &to; ~Groups() { to = fb.all; } } keep{fb, groups};          // (after the last replay: the grouped list)
    fb.start(c.ow, c.oh, c.cols, c.rows, c.sf, c.minw, c.minh, c.maxw, c.maxh);
    fb.first_set();
    const std::vector<int> first = fb.ladder_of; const std::vector<ScanGrid> full = fb.grids;
    std::vector<std::vector<unsigned long long>> bits(fb.ladder.size());          // (live until the last replay)
    std::vector<nvca_rect> raw; std::vector<int> sc;
    if (feed == kFeedDense) {
        // every passing window of the full grids and the grids' stage-0 reject bits; the full walk's hits are picked from them
        fb.dense_begin();
        for (size_t k = 0; k < first.size(); k++) {
            const int li = first[k];
            const FbStep &st = fb.ladder[li];
            const ScanGrid g = full[k];
            if (g.startX || g.startY) return false;
            const int wpr = (g.endX + 63) / 64;
            bits[li].assign((size_t)wpr * g.endY, 0);
            fb.dense_step(li, bits[li].data(), wpr, g.endY);
            std::vector<unsigned> pass;
            for (int iy = 0; iy < g.endY; iy++)
                for (int ix = 0; ix < g.endX; ix++) {
                    const int result = fb_pred(c, li, ix, iy, fb_cvr(ix * st.ystep), fb_cvr(iy * st.ystep), st.winw);
                    if (result == 0) bits[li][(size_t)iy * wpr + (ix >> 6)] |= 1ull << (ix & 63);
                    if (result > 0) pass.push_back((unsigned)(iy << 13 | ix));
                }
            for (unsigned key : pass) {
                const int iy = (int)(key >> 13), ix = (int)(key & 8191);
                const int seen = fb.dense_candidate(li, ix, iy);
                if (seen < 0) return false;
                if (seen) { raw.push_back(nvca_rect{fb_cvr(ix * st.ystep), fb_cvr(iy * st.ystep), st.winw, st.winh}); sc.push_back(li); }
            }
        }
    } else
        for (size_t k = 0; k < first.size(); k++) {
            fb_walk(c, fb.ladder[first[k]], first[k], full[k], feed == kFeedPlan ? (int)k : first[k], raw, sc);
        }
    if (!fb.take(raw, sc, feed != kFeedPlan)) return false;
    *second_set = 0;
    if (fb.replay(c.mn, c.rough, out)) return true;
    // the narrowed set it asks for
    raw.clear(); sc.clear();
    *second_set = (int)fb.ladder_of.size();
    for (size_t k = 0; k < fb.ladder_of.size(); k++) {
        const int li = fb.ladder_of[k];
        const ScanGrid g = fb.grids[k];
        if (!(g.endX > g.startX && g.endY > g.startY)) return false;          // (an empty grid is not asked for)
        if (feed == kFeedDense && std::find(first.begin(), first.end(), li) != first.end()) return false;   // the first set held this step
        fb_walk(c, fb.ladder[li], li, g, feed == kFeedPlan ? (int)k : li, raw, sc);
    }
    if (!fb.take(raw, sc, feed != kFeedPlan)) return false;
    return fb.replay(c.mn, c.rough, out);          // (false: a third set -- the loop narrows once)
}

// The clipping rule on its own.  With ystep >= 2 neither formula of cvHaarDetectObjectsForROC puts a window outside the image
// ((endX - 1) * ystep <= cols - winw - ystep / 2), so no search case reaches it: hand-made grids do
static int check_clip_grid()
{
    ScanGrid g{0, 6, 0, 6};          // origins 0, 2 .. 10, window 10: on a 20 x 19 image x = 10 fits exactly, y = 10 is one too far
    if (!clip_grid(20, 19, 2., 10, 10, g) || g.endX != 6 || g.endY != 5) return fail("clip_grid: x + winw == cols stays, y + winh == rows + 1 goes");
    g = ScanGrid{0, 6, 0, 6};
    if (!clip_grid(19, 20, 2., 10, 10, g) || g.endX != 5 || g.endY != 6) return fail("clip_grid: x + winw == cols + 1 goes, y + winh == rows stays");
    g = ScanGrid{0, 8, 0, 3};
    if (!clip_grid(20, 19, 2., 10, 10, g) || g.endX != 6 || g.endY != 3) return fail("clip_grid: dropped from the end only while the window leaves the image");
    g = ScanGrid{6, 9, 0, 3};
    if (clip_grid(20, 19, 2., 10, 10, g)) return fail("clip_grid: a grid wholly outside the image has nothing to scan");
    g = ScanGrid{-2, 3, 0, 3};
    if (clip_grid(20, 19, 2., 10, 10, g)) return fail("clip_grid: a negative origin voids the grid");
    g = ScanGrid{3, 3, 0, 3};
    if (clip_grid(20, 19, 2., 10, 10, g)) return fail("clip_grid: an empty grid");
    if (!full_grid(20, 19, 2., 10, 10, g) || g.startX || g.startY || g.endX != 5 || g.endY != 4) return fail("full_grid: cvRound((cols - winw) / ystep)");
    return 0;
}

static int run_fbsearch()
{
    if (check_clip_grid()) return 1;
    const int kCases = 360;          // the last 120: objects that hug the right / bottom edge, with a smaller one nested in them
    static const int wins[4][2] = {{20, 20}, {18, 15}, {25, 15}, {24, 24}};
    static const double sfs[4] = {1.1, 1.2, 1.25, 1.3}, rej0[3] = {0.2, 0.5, 0.8}, noise[3] = {0., 0.001, 0.01};
    for (int id = 0; id < kCases; id++) {
        FbCase c;
        const int wi = rnd_in(0, 3);
        c.ow = wins[wi][0]; c.oh = wins[wi][1]; c.cols = rnd_in(60, 200); c.rows = rnd_in(50, 160); c.sf = sfs[rnd_in(0, 3)];
        c.mn = rnd_in(0, 3); c.rough = rnd() & 1; c.seed = rnd(); c.p_rej0 = rej0[rnd_in(0, 2)]; c.p_noise = noise[rnd_in(0, 2)];
        c.minw = c.minh = 1; c.maxw = c.cols; c.maxh = c.rows;
        if (rnd_in(0, 2) == 0) { c.minw = rnd_in(c.ow, 2 * c.ow); c.minh = rnd_in(c.oh, 2 * c.oh); }
        if (rnd_in(0, 3) == 0) { c.maxw = rnd_in(2 * c.ow, c.cols); c.maxh = rnd_in(2 * c.oh, c.rows); }
        const double fmax = std::min((c.cols - 10.) / c.ow, (c.rows - 10.) / c.oh);
        int nobj = rnd_in(0, 3);
        const bool edge = id >= 240;
        if (edge) nobj = std::max(nobj, 1);
        else if (id % 8 == 7) { nobj = 0; c.p_noise = 0; }          // nothing to find
        for (int k = 0; k < nobj && fmax > 1.2; k++) {
            const double f = 1. + (fmax - 1.) * rnd_in(10, 90) / 100.;
            FbObj o; o.w = (int)(c.ow * f); o.h = (int)(c.oh * f);
            o.x = rnd_in(0, std::max(0, c.cols - o.w - 1)); o.y = rnd_in(0, std::max(0, c.rows - o.h - 1));
            c.objs.push_back(o);
            if (id % 6 == 5 && k == 0) { c.minw = o.w * rnd_in(50, 80) / 100; c.minh = o.h * rnd_in(50, 80) / 100; c.maxw = c.cols; c.maxh = c.rows; }   // an object above minSize, a narrowed search that goes below it
        }
        if (edge && !c.objs.empty()) {
            // the found box widened by 20 % meets the clamp to cols - 1 / rows - 1; a nested object of 0.42 .. 0.58 of its size sits
            // astride the lowered minimum size (0.4 / 0.6 of the box found)
            FbObj &o = c.objs[0];
            if (id % 3 != 1) o.x = std::max(0, c.cols - o.w - rnd_in(0, 2));
            if (id % 3 != 2) o.y = std::max(0, c.rows - o.h - rnd_in(0, 2));
            const int pct = rnd_in(42, 58);
            FbObj in; in.w = o.w * pct / 100; in.h = o.h * pct / 100; in.x = o.x + rnd_in(0, std::max(0, o.w - in.w)); in.y = o.y + rnd_in(0, std::max(0, o.h - in.h));
            if (in.w >= c.ow && in.h >= c.oh) c.objs.push_back(in);
            c.minw = c.minh = 1; c.maxw = c.cols; c.maxh = c.rows;
        }
        FbCounts n;
        std::vector<nvca_rect> want_all, got_all[3];
        const std::vector<nvca_rect> want = fb_serial(c, n, want_all);
        std::vector<nvca_rect> got[3]; int second[3] = {0, 0, 0};
        for (int feed = 0; feed < 3; feed++)
            if (!fb_fed(c, feed, got[feed], got_all[feed], &second[feed])) { fprintf(stderr, "case %d, feed %d\n", id, feed); return fail("FbSearch refused its input or asked for a set it must not need"); }
        auto put = [](const char *name, const std::vector<nvca_rect> &v) {
            printf(", \"%s\": [", name);
            for (size_t i = 0; i < v.size(); i++) printf("%s[%d, %d, %d, %d]", i ? ", " : "", v[i].x, v[i].y, v[i].w, v[i].h);
            printf("]");
        };
        printf("{\"fbsearch\": %d", id);
        put("serial", want); put("plan", got[0]); put("small", got[1]); put("dense", got[2]);
        put("serial_groups", want_all); put("plan_groups", got_all[0]); put("small_groups", got_all[1]); put("dense_groups", got_all[2]);
        printf(", \"narrowed\": %d, \"narrowed_steps\": %d, \"narrowed_hits\": %d, \"below_min\": %d, \"second_set\": [%d, %d, %d]}\n",
               n.narrowed, n.narrowed_steps, n.narrowed_hits, n.below_min, second[0], second[1], second[2]);
    }
    printf("{\"fbsearch_cases\": %d}\n", kCases);
    return 0;
}

// ---- plans -------------------------------------------------------------------------------------------------------------
// every sample a window of a tile can touch (its origin + any corner offset of the early stages / the variance rectangle)
// must be one of the tile's staged columns / rows, inside the plane: the tile kernels look corners up through maps that are
// only filled for staged coordinates, and read the planes at those coordinates
static int check_plan(const Cascade &c, const DetectPlan &dp, int cols, int rows, int pitch)
{
    long long windows = 0, tiled = 0;
    for (size_t s = 0; s < dp.scales.size(); s++) windows += (long long)dp.scales[s].endX * dp.scales[s].endY;
    for (const TileRec &t : dp.tiles) {
        tiled += (long long)t.nx * t.ny;
        const ScaleRec &sc = dp.scales[t.scale];
        if (t.nx < 1 || t.ny < 1 || t.nx > kTileWin || t.ny > kTileRows || t.ix0 + t.nx > sc.endX || t.iy0 + t.ny > sc.endY) return fail("tile outside its scale's grid");
        if (t.ncol < 1 || t.ncol > kTileMaxCols || t.nrow < 1 || t.nrow > kTileThreads) return fail("tile sample counts");
        if (tile_lds_bytes(t.ncol, t.nrow, t.span_x, t.span_y) > dp.tile_lds || dp.tile_lds > kTileLdsBudget) return fail("tile LDS size");
        if ((size_t)t.col_off + t.ncol > dp.tcoords.size() || (size_t)t.row_off + t.nrow > dp.tcoords.size()) return fail("tile coordinate lists out of range");
        std::set<int> cs(dp.tcoords.begin() + t.col_off, dp.tcoords.begin() + t.col_off + t.ncol), rs(dp.tcoords.begin() + t.row_off, dp.tcoords.begin() + t.row_off + t.nrow);
        if ((int)cs.size() != t.ncol || (int)rs.size() != t.nrow) return fail("duplicate staged coordinate");
        if (*cs.begin() < t.x0 || *cs.rbegin() - t.x0 + 1 > t.span_x || *rs.begin() < t.y0 || *rs.rbegin() - t.y0 + 1 > t.span_y) return fail("map extents");
        if (*cs.rbegin() >= pitch || *rs.rbegin() >= rows + 1 + 4) return fail("staged coordinate outside the plane");
        const ScaleTable &tab = *dp.tabs[t.scale];
        const int early_last = std::min<int>(dp.deep_stage, (int)dp.stages.size());
        const int k1 = dp.stages[early_last - 1].first + dp.stages[early_last - 1].count;
        std::set<int> ox{tab.ex, tab.ex + tab.ew}, oy{tab.ey, tab.ey + tab.eh};
        for (int k = 0; k < k1; k++)
            for (int q = 0; q < (tab.host[k].nrect & 255); q++) { ox.insert(tab.host[k].x0[q]); ox.insert(tab.host[k].x1[q]); oy.insert(tab.host[k].y0[q]); oy.insert(tab.host[k].y1[q]); }
        for (int rx = 0; rx < t.nx; rx++) for (int o : ox) if (!cs.count(dp.pos[sc.xpos_off + t.ix0 + rx] + o)) return fail("a window's sample column is not staged");
        for (int ry = 0; ry < t.ny; ry++) for (int o : oy) if (!rs.count(dp.pos[sc.ypos_off + t.iy0 + ry] + o)) return fail("a window's sample row is not staged");
    }
    if (!dp.tiles.empty() && dp.strips.empty() && tiled != windows) return fail("tiles do not cover the grid exactly once");
    long long band_tiles = 0;
    for (const BandRec &b : dp.bands) {
        band_tiles += b.ntiles;
        if (b.first_tile < 0 || b.first_tile + b.ntiles > (int)dp.tiles.size()) return fail("band tile range");
        for (int k = 0; k < b.ntiles; k++) { const TileRec &t = dp.tiles[b.first_tile + k]; if (t.scale != b.scale || t.iy0 != b.iy0 || t.ny != b.ny || t.ix0 != k * dp.tiles[b.first_tile].nx) return fail("band is not a row of tiles"); }
    }
    if (!dp.bands.empty() && band_tiles != (long long)dp.tiles.size()) return fail("bands do not cover the tiles");
    for (const DeepRec &d : dp.deeprecs) if (d.ncol && ((size_t)d.col_off + d.ncol > dp.tcoords.size() || (size_t)d.row_off + d.nrow > dp.tcoords.size() || d.nrow * (d.ncol | 1) * 4 > dp.deep_lds)) return fail("deep patch");
    // candidate keys round-trip through hit_valid / hit_rect for every scale's last window, and junk keys are refused
    for (size_t s = 0; s < dp.specs.size(); s++) {
        if (dp.specs[s].xs.empty() || dp.specs[s].ys.empty()) continue;
        const unsigned key = ((unsigned)s << dp.key_ss) | ((unsigned)(dp.specs[s].ys.size() - 1) << dp.key_sy) | (unsigned)(dp.specs[s].xs.size() - 1);
        if (!dp.hit_valid(key)) return fail("hit_valid refuses a real window");
        const nvca_rect r = dp.hit_rect(key);
        if (r.x + r.w > cols || r.y + r.h > rows) return fail("window outside the image");
        // one past the grid in x / in y, where the key's field can express it (the fields are sized for the plan's largest grid: a
        // full field would carry into the next one and name another, real window)
        const size_t nx = dp.specs[s].xs.size(), ny = dp.specs[s].ys.size();
        if (nx < (1u << dp.key_sy) && dp.hit_valid(key + 1)) return fail("hit_valid accepts a window beyond the grid (x)");
        if (ny < (1u << (dp.key_ss - dp.key_sy)) && dp.hit_valid(key + (1u << dp.key_sy))) return fail("hit_valid accepts a window beyond the grid (y)");
    }
    if (dp.key_ss < 32 && dp.hit_valid((unsigned)dp.specs.size() << dp.key_ss)) return fail("hit_valid accepts an unknown scale");
    (void)c;
    return 0;
}

static int run_plans(const char *xml_path)
{
    const std::string xml = slurp(xml_path);
    nvca_ctx ctx;
    nvca_cascade casc; casc.ctx = &ctx;
    std::string err;
    if (parse_cascade_xml(xml.data(), xml.size(), casc.c, err)) return fail(err.c_str());
    casc.c.uid = ctx.next_uid++;
    struct G { int w, h; double sf; int minw, minh; } geoms[] = {
        {1920, 1080, 1.1, 96, 54}, {1280, 720, 1.1, 64, 36}, {640, 480, 1.25, 32, 24}, {160, 120, 1.25, 8, 6}, {160, 90, 1.25, 8, 4},
        {97, 83, 1.1, 3, 3}, {25, 25, 1.1, 0, 0}, {21, 400, 1.3, 0, 0}, {1400, 300, 1.2, 0, 0}, {3840, 2160, 1.2, 192, 108}, {320, 180, 1.1, 20, 20},
    };
    for (const G &g : geoms) {
        for (int variant = 0; variant < 3; variant++) {
            ctx.sw = Switches();
            if (variant == 1) ctx.sw.tiles = false;
            if (variant == 2) ctx.sw.deep_stage = 2;
            const int pitch = (g.w + 1 + 7) / 8 * 8;
            DetectPlan dp;
            const int rc = dp.build_scale_cascade(&ctx, casc.c, g.w, g.h, pitch, g.sf, g.minw, g.minh, g.w, g.h, err);
            if (rc) { printf("{\"plan\": [%d, %d, %.17g, %d, %d], \"variant\": %d, \"rc\": %d}\n", g.w, g.h, g.sf, g.minw, g.minh, variant, rc); continue; }
            if (check_plan(casc.c, dp, g.w, g.h, pitch)) return 1;
            printf("{\"plan\": [%d, %d, %.17g, %d, %d], \"variant\": %d, \"rc\": 0, \"factors\": [", g.w, g.h, g.sf, g.minw, g.minh, variant);
            for (size_t s = 0; s < dp.scales.size(); s++) printf("%s%.17g", s ? ", " : "", dp.scales[s].factor);
            printf("], \"grid\": [");
            for (size_t s = 0; s < dp.scales.size(); s++) printf("%s[%d, %d]", s ? ", " : "", dp.scales[s].endX, dp.scales[s].endY);
            printf("], \"tiles\": %zu, \"bands\": %zu, \"strips\": %zu, \"tile_lds\": %d}\n", dp.tiles.size(), dp.bands.size(), dp.strips.size(), dp.tile_lds);
        }
    }
    // resize tables over awkward ratios
    for (int t = 0; t < 200; t++) {
        ResizeTab tab;
        const int sw = rnd_in(1, 2000), sh = rnd_in(1, 1200), dw = rnd_in(1, 700), dh = rnd_in(1, 500);
        build_resize_tab(sw, sh, dw, dh, tab);
        if (tab.mode == 1)
            for (int dx = 0; dx < dw; dx++) if (tab.xofs[dx] < 0 || tab.xofs[dx] >= sw) return fail("resize column offset outside the source");
    }
    return 0;
}

// ---- glue --------------------------------------------------------------------------------------------------------------
static void print_rects(const char *tag, int id, const std::vector<nvca_rect> &v, const std::vector<int> *extra = nullptr)
{
    printf("{\"%s\": %d, \"out\": [", tag, id);
    for (size_t i = 0; i < v.size(); i++) printf("%s[%d, %d, %d, %d]", i ? ", " : "", v[i].x, v[i].y, v[i].w, v[i].h);
    printf("]");
    if (extra) { printf(", \"extra\": ["); for (size_t i = 0; i < extra->size(); i++) printf("%s%d", i ? ", " : "", (*extra)[i]); printf("]"); }
    printf("}\n");
}
static std::vector<nvca_rect> read_rects(std::istream &in)
{
    int n; in >> n;
    std::vector<nvca_rect> v(n);
    for (nvca_rect &r : v) in >> r.x >> r.y >> r.w >> r.h;
    return v;
}

// cases come from the pytest (which also hands them to the oracle): one per line,
//   G id thr eps n rects...            groupRectangles
//   J id min max dist n rects...       __join_objects
//   T id thr nframes {n rects...}      Faces::track over a sequence of detections
static int run_glue(const char *cases_path)
{
    std::ifstream in(cases_path);
    std::string kind;
    while (in >> kind) {
        int id; in >> id;
        if (kind == "G") {
            int thr; double eps; in >> thr >> eps;
            std::vector<nvca_rect> v = read_rects(in); std::vector<int> w;
            group_rectangles(v, thr, eps, &w);
            print_rects("group", id, v, &w);
        } else if (kind == "J") {
            int mn, dist; long mx; in >> mn >> mx >> dist;
            std::vector<nvca_rect> v = read_rects(in);
            join_objects(v, mn, mx, dist);
            print_rects("join", id, v);
        } else if (kind == "T") {
            int thr, nf; in >> thr >> nf;
            Faces f;
            for (int k = 0; k < nf; k++) {
                std::vector<nvca_rect> cur = read_rects(in);
                if (!cur.empty()) f.track(cur, thr); else if (k % 3 == 2) f.clear();
            }
            std::vector<nvca_rect> boxes; std::vector<int> ids;
            for (const TrackedFace &t : f.faces) { boxes.push_back(t.box); ids.push_back(t.id); }
            print_rects("track", id, boxes, &ids);
        } else return fail("unknown case kind");
    }
    // the part detectors' merging heuristics on random lists (their parity with the oracle is the GPU stream tests' business:
    // here they run under the sanitizers, with the list shapes -- 0..6 boxes, nested, coincident -- that exercise every erase)
    unsigned long long sum = 0;
    for (int t = 0; t < 20000; t++) {
        auto boxes = [&](int nmax) {
            std::vector<nvca_rect> v(rnd_in(0, nmax));
            for (nvca_rect &r : v) { r.x = rnd_in(0, 300); r.y = rnd_in(0, 200); r.w = rnd_in(1, 120); r.h = rnd_in(1, 120); }
            if (v.size() > 1 && rnd() % 3 == 0) v[1] = v[0];
            if (v.size() > 2 && rnd() % 3 == 0) { v[2].x = v[0].x + 2; v[2].y = v[0].y + 2; v[2].w = std::max(1, v[0].w - 4); v[2].h = std::max(1, v[0].h - 4); }
            return v;
        };
        const nvca_rect face{rnd_in(0, 200), rnd_in(0, 150), rnd_in(20, 200), rnd_in(20, 200)};
        const int scale = rnd_in(1, 6);
        std::vector<nvca_rect> a = boxes(6), b = boxes(6), old = boxes(4), res;
        to_global(a, face, scale);
        merge_eyes_current(face, b, a, scale, rnd() & 1);
        merge_eyes_consecutive(a, old, res);
        for (const nvca_rect &r : res) sum += (unsigned)(r.x * 3 + r.y * 5 + r.w * 7 + r.h * 11);
        std::vector<nvca_rect> cn = boxes(5);
        merge_consecutive_nm(cn, old, face, scale, rnd_in(1, 12), res);
        for (const nvca_rect &r : res) sum += (unsigned)(r.x + r.y + r.w + r.h);
    }
    // image-to-overlay on host frames: boxes that stick out of the frame on every side, every channel count, tiny and huge scales
    for (int t = 0; t < 300; t++) {
        const int W = rnd_in(1, 90), H = rnd_in(1, 70), stride = W * 3 + rnd_in(0, 5), cn = (int[]){1, 3, 4}[rnd() % 3], iw = rnd_in(1, 40), ih = rnd_in(1, 30);
        std::vector<uint8_t> frame((size_t)stride * H), img((size_t)iw * cn * ih);
        for (uint8_t &b : frame) b = (uint8_t)rnd();
        for (uint8_t &b : img) b = (uint8_t)rnd();
        nvca_overlay ov{img.data(), iw, ih, iw * cn, cn, (rnd_in(-20, 20)) / 10.0, (rnd_in(-20, 20)) / 10.0, rnd_in(0, 30) / 10.0, rnd_in(0, 30) / 10.0};
        std::vector<nvca_rect> bx(rnd_in(0, 3));
        for (nvca_rect &r : bx) { r.x = rnd_in(-60, 100); r.y = rnd_in(-60, 80); r.w = rnd_in(0, 120); r.h = rnd_in(0, 100); }
        overlay_blend_host(frame.data(), W, H, stride, bx.data(), (int)bx.size(), ov);
        for (uint8_t b : frame) sum += b;
    }
    printf("{\"merges_checksum\": %llu}\n", sum);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && std::string(argv[1]) == "fbsearch") return run_fbsearch();
    if (argc < 3) { fprintf(stderr, "usage: san_driver loader <xml>... | plans <xml> | glue <cases> | fbsearch\n"); return 2; }
    const std::string mode = argv[1];
    if (mode == "loader") return run_loader(argc - 2, argv + 2);
    if (mode == "plans") return run_plans(argv[2]);
    if (mode == "glue") return run_glue(argv[2]);
    if (mode == "stages") {            // the per-stage summation-order proof of a cascade (StageRec flags), for DESIGN / experiments
        const std::string xml = slurp(argv[2]);
        Cascade c; std::string err;
        if (parse_cascade_xml(xml.data(), xml.size(), c, err)) return fail(err.c_str());
        std::vector<StageRec> st; build_stage_recs(c, st);
        for (size_t i = 0; i < st.size(); i++) printf("{\"stage\": %zu, \"count\": %d, \"flags\": %d, \"thr_i\": %d, \"vote_exp\": %d}\n", i, st[i].count, st[i].flags, st[i].thr_i, st[i].vote_exp);
        return 0;
    }
    return 2;
}
