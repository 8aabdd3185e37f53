// part_stats.h -- NVCA_PART_STATS (diagnostic): where the batched part detectors and their job rounds spend the host's time.  One
// per context (nvca_ctx::stats); part_call.cpp and detect_rounds.cpp add to it through scoped timers, report() and report_round() print it.
#pragma once
#include <chrono>
#include <cstddef>

namespace nvca {

inline double mono_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct PartStats {
    // seconds since the last report.  A part batch by phase ...
    double chains = 0, face_passes = 0, roi_setup = 0, roi_searches = 0, merging = 0, whole = 0;
    // ... its job rounds ...
    double enqueue = 0, wait = 0, advance = 0;
    // ... and the rounds in detail (small_jobs: a count)
    double add_jobs = 0, small_jobs = 0, launch = 0, collect = 0, advance_helpers = 0, advance_serial = 0;
    int calls = 0, rounds = 0;                       // part batches reported on, small-image rounds seen
    // adds the time between its construction (or start) and its stop / destruction to a field -- when stats are on; nothing otherwise
    struct Timer {
        double *to = nullptr, t0 = 0;
        Timer(bool on, double &field) : to(on ? &field : nullptr), t0(on ? mono_s() : 0) {}
        Timer(const Timer &) = delete; Timer &operator=(const Timer &) = delete;
        double stop() { if (!to) return 0; const double d = mono_s() - t0; *to += d; to = nullptr; return d; }
        ~Timer() { stop(); }
    };
    void clear_rounds() { enqueue = wait = advance = add_jobs = small_jobs = launch = collect = advance_helpers = advance_serial = 0; }
    void report();                                   // a part batch was timed: every 8th prints the two report lines and starts over
    // a small-image round was waited for: rounds 201 .. 212 (a dozen of the steady state) print what the round held
    void report_round(size_t images, const int kinds[4] /* by JobKind */, int narrowed, size_t workgroups, double waited_s);
};

} // namespace nvca
