// fb_search.h -- scan grids of the scale-cascade branch of cvHaarDetectObjectsForROC and its CV_HAAR_FIND_BIGGEST_OBJECT search as
// pure host code (no HIP, no context): the factor ladder, the full and the narrowed grid of a ladder step, the one clipping rule of
// a grid, and the serial loop replayed on scan results that arrive in at most two sets.  detect_job.cpp feeds it from cached plans,
// roi_batch.cpp from the small-image launch; tests/san/san_driver.cpp drives it on the CPU against the loop itself.
#pragma once
#include "../../include/nubovca.h"
#include "device_records.h"
#include <cstddef>
#include <vector>

namespace nvca {

struct FbStep { double factor, ystep; int winw, winh; };
// grid of window origins cvRound(i * ystep), as index limits [startX, endX) x [startY, endY)
struct ScanGrid { int startX, endX, startY, endY; };

// The clipping rule of a scan grid: grid points whose window would leave the image (cvRunHaarClassifierCascadeSum returns -1 there:
// no hit, step 1) are dropped from the end, a negative origin voids the grid.  false: nothing to scan
bool clip_grid(int cols, int rows, double ystep, int winw, int winh, ScanGrid &g);
// the full grid of a window size, clipped
bool full_grid(int cols, int rows, double ystep, int winw, int winh, ScanGrid &g);
// a clipped grid as a step record of the small-image launch; its candidate key holds 13 bits of column and of row
bool roi_grid(const ScanGrid &g, double ystep, RoiStep &st);

// was window ix of a grid row visited by the serial walk that started at column `start`?  (visited iff the run of stage-0 rejects
// immediately left of it, not reaching below `start`, has even length: the walk steps by 2 behind a stage-0 reject, by 1 otherwise)
inline bool fb_visited(const unsigned long long *row, int start, int ix)
{
    int run = 0;
    for (int x = ix - 1; x >= start && ((row[x >> 6] >> (x & 63)) & 1ull); x--) run++;
    return !(run & 1);
}

// The serial loop changes its scan only once (after the first grouped detection it narrows to a region and a minimum size), so two
// sets of scan results serve it: every ladder step on its full grid, then the remaining steps on their narrowed grids.
struct FbSearch {
    int cols = 0, rows = 0, minw = 0, minh = 0, maxw = 0, maxh = 0;         // the call (start())
    std::vector<FbStep> ladder;                       // largest factor first, exactly as the serial loop walks it
    std::vector<std::vector<nvca_rect>> hits;         // [ladder step]: what the serial walk of the step's current grid finds
    std::vector<int> ladder_of;                       // ladder step of each scale of the set that is asked for / queued ...
    std::vector<ScanGrid> grids;                      // ... and its clipped grid (filled by first_set() and replay())
    // the serial loop's state between the two sets
    std::vector<nvca_rect> all; nvca_rect scanROI{0, 0, 0, 0}; bool narrowed_done = false; size_t fb_i = 0; int cur_minw = 0, cur_minh = 0;
    // Dense first set (optional): per ladder step every window of the full grid that passes the whole cascade, visited by the serial
    // walk or not (iy << 13 | ix, ascending), and the stage-0 reject bits of that grid (rej_wpr words per grid row, rej_rows rows;
    // the memory is the feeder's and must outlive the replay that follows).  A narrowed walk of such a step is replayed from them.
    std::vector<std::vector<unsigned>> dense_hits;
    std::vector<const unsigned long long *> rej_bits; std::vector<int> rej_wpr, rej_rows;

    // builds the ladder for an ow x oh window on a cols x rows image and resets the loop's state
    void start(int ow, int oh, int cols, int rows, double sf, int minw, int minh, int maxw, int maxh);
    // the first set into ladder_of / grids: the steps of the call's sizes whose full grid is not empty
    void first_set();
    bool narrowed_grid(size_t step, ScanGrid &g) const;          // from scanROI
    // a set's raw candidates (serial order) to their ladder steps.  sc[k] names a scale of the queued set (ladder_of maps it back) or,
    // by_step, the ladder step itself.  false: a candidate of an unknown ladder step
    bool take(const std::vector<nvca_rect> &raw, const std::vector<int> &sc, bool by_step);
    void dense_begin();                               // a dense first set came back: no step has reject bits yet
    void dense_step(size_t li, const unsigned long long *bits, int wpr, int rows) { rej_bits[li] = bits; rej_wpr[li] = wpr; rej_rows[li] = rows; }
    // one dense candidate of ladder step li: noted for a narrowed replay.  1: the full walk (start column 0) visits it, 0: it does
    // not, -1: outside the step's reject bitmap
    int dense_candidate(size_t li, int ix, int iy);
    // The loop on the results at hand.  true: done, `out` holds the biggest object (or nothing).  false: it needs the steps in
    // ladder_of on their narrowed grids (in grids) first (take() them, call again)
    bool replay(int min_neighbors, bool rough, std::vector<nvca_rect> &out);
};

} // namespace nvca
