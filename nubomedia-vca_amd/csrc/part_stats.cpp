// part_stats.cpp -- the stderr lines of NVCA_PART_STATS (part_stats.h)
#include "part_stats.h"
#include <cstdio>

namespace nvca {

void PartStats::report()
{
    if (++calls % 8 != 0) return;
    fprintf(stderr, "nubovca part batch (ms per call): image chains %.3f, face passes %.3f, roi set-up %.3f, roi searches %.3f | in the job rounds: enqueue %.3f, wait %.3f, advance %.3f | merging (previous calls) %.3f, whole call (previous 8) %.3f\n",
            chains / 8 * 1e3, face_passes / 8 * 1e3, roi_setup / 8 * 1e3, roi_searches / 8 * 1e3, enqueue / 8 * 1e3, wait / 8 * 1e3, advance / 8 * 1e3,
            merging / 8 * 1e3, whole / 8 * 1e3);
    fprintf(stderr, "nubovca part batch, job rounds in detail (ms per call): adding jobs %.3f (%.0f jobs), launch %.3f, collect %.3f, advance on the helpers %.3f, advance serial %.3f\n",
            add_jobs / 8 * 1e3, small_jobs / 8, launch / 8 * 1e3, collect / 8 * 1e3, advance_helpers / 8 * 1e3, advance_serial / 8 * 1e3);
    chains = face_passes = roi_setup = roi_searches = merging = whole = 0;
    clear_rounds();
}

void PartStats::report_round(size_t images, const int kinds[4], int narrowed, size_t workgroups, double waited_s)
{
    if (++rounds <= 200 || rounds > 212) return;
    fprintf(stderr, "[nvca jobs] small-image round: %zu images (plain %d, scale-image %d, biggest-object %d of which narrowed %d, LBP %d), %zu workgroups, waited %.0f us\n",
            images, kinds[0], kinds[1], kinds[2], narrowed, kinds[3], workgroups, waited_s * 1e6);
}

} // namespace nvca
