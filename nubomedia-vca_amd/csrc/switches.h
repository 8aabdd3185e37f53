// switches.h -- the context's switches and the functions of options.cpp.  Includes nothing.
#pragma once

namespace nvca {

// --------------------------------------------------------------------------
// Switches: A/B and diagnostic knobs, one row each in the table of options.cpp; none of them changes a
// result.  The environment is read ONCE per process -- when the first context is created (nvca_ctx_create) -- never on a hot
// entry point.  A context starts from those process defaults; nvca_ctx_set_option changes one of them for that context.
// --------------------------------------------------------------------------
struct Switches {
    bool group_zero_copy = true;     // NVCA_GROUP_ZEROCOPY=0: box tables through a copy instead of direct stores to the host buffer (default 1)
    bool skip_cascade = false;       // NVCA_SKIP_CASCADE: timing experiments on the pre-processing kernels only (default off)
    bool host_group = false;         // NVCA_HOST_GROUP: cv::groupRectangles on the host (default off)
    int  band_map = 0;               // NVCA_BAND_MAP=1/2: frame-major band walk (default 0: off)
    int  band = -1;                  // NVCA_BAND=0/1: force pre-pass + tile kernels / band kernel (default -1: by batch size)
    bool host_profile = false;       // NVCA_HOST_PROFILE: host-side timing prints (default off)
    bool sparse_ingest = true;       // NVCA_SPARSE_INGEST=0: whole host frames in shrink-first mode (default 1)
    bool pyr_off = false;            // NVCA_PYR_OFF: per-level launches for SCALE_IMAGE (default off)
    int  part_stats = 0;             // NVCA_PART_STATS[=n]: phase timers of part batches with n (8 when n is not given) or more streams (default 0: off)
    int  ingest_chunk = 8;           // NVCA_INGEST_CHUNK=n: chunk size of host-frame batches, 0 = no chunking (default 8)
    int  deep_stage = 0;             // NVCA_DEEP_STAGE=s: first stage of k_deep (default 0: the plan's own choice)
    bool tiles = true;               // NVCA_TILES=0: row-strip kernel instead of the tile kernels (default 1)
    bool plan_debug = false;         // NVCA_PLAN_DEBUG: per-scale tile sizes, and the gray kernel of each 4:2:0 launch, on stderr (default off)
    bool deep_lds = true;            // NVCA_DEEP_LDS_OFF: k_deep without LDS patches (default: with them)
    bool trk_fold = true;            // NVCA_TRK_FOLD=0: NuboTracker's components through the per-pixel kernels (k_ccl_flatten / _reduce / _collect) instead of the per-tile reduction + fold of tile roots (default 1)
    int  trk_order = -1;             // NVCA_TRK_ORDER: visiting order of k_ccl_reduce (default -1: decided per frame on the device)
    int  host_threads = -1;          // NVCA_HOST_THREADS=n: helper threads for per-job host work, 0: none (default -1: min(8, cores / 2) - 1)
    bool fb_dense = true;            // NVCA_FB_DENSE=0: a FIND_BIGGEST search on the small-image path re-scans its narrowed grids in a second launch instead of replaying them on the host from the first launch's dense candidates + stage-0 reject bits (default 1)
    bool roi = true;                 // NVCA_ROI=0: small images take the large-image path too (plan + four launches per job; on a new-format LBP cascade plan, pyramid and a dozen launches) (default 1)
    bool stage_order = false;        // NVCA_STAGE_ORDER=1: the tile kernels walk the early stages 1 .. 5 in the order the previous tile of the band found cheapest (cost per window killed) instead of the cascade's own; the set of survivors is the same (default 0)
    int  pair_max = 32;              // NVCA_PAIR_MAX=n (<= 32): windows up to which a round of the tile kernels runs lane = (window, stump) instead of a window per lane (default 32)
    int  spec_pairs = 1536;          // NVCA_SPEC_PAIRS=n: with at most 32 windows left a round takes as many stages as stay within n (window, stump) pairs, 512 being one step of the workgroup (default 1536)
    bool quiet = false;              // NVCA_QUIET: no one-time notes on stderr (a plan that falls back to the row-strip kernel) (default off)
    const char *stamps_out = nullptr;   // NVCA_STAMPS_OUT (diagnostic build only; not an option)
};
Switches read_switches();           // the process defaults from the environment (options.cpp); switches() keeps the first reading
bool option_set(Switches &w, const char *name, int value, bool *replan);      // false: unknown name; *replan: the cached plans depend on it
bool option_get(const Switches &w, const char *name, int *value);
const Switches &switches();

} // namespace nvca
