// combiner_driver.cpp -- test infrastructure: the GStreamer shim's frame combiner (gst/combiner.h) under ThreadSanitizer.  Twelve
// threads send 4000 requests each through ONE Combiner; the round callback marks every request of its round.  Every request is
// run exactly once and process returns that request's own status; the numbers the test bounds are printed:
//   combiner ok requests=<sum of round sizes> rounds=<rounds> largest=<largest round> max_batch=<Combiner::max_batch>
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>
#include "../../nubomedia-vca_amd/gst/combiner.h"

struct Req { int id, rc; bool done; };
static const int kThreads = 12, kPerThread = 4000;
static int status_of(int id) { return id * 7 + 3; }

int main()
{
    Combiner<Req> comb;
    std::vector<std::atomic<int>> runs(kThreads * kPerThread);
    for (auto &r : runs) r.store(0);
    std::atomic<long long> requests{0}, rounds{0};
    std::atomic<int> largest{0}, wrong{0};
    auto run = [&](std::vector<Req *> &round) {
        for (Req *r : round) { runs[r->id].fetch_add(1); r->rc = status_of(r->id); }
        requests.fetch_add((long long)round.size());
        rounds.fetch_add(1);
        int seen = largest.load();
        while ((int)round.size() > seen && !largest.compare_exchange_weak(seen, (int)round.size())) {}
        std::this_thread::yield();                          // the GPU call's place: the others queue up meanwhile
    };
    std::vector<std::thread> threads;
    for (int t = 0; t < kThreads; t++)
        threads.emplace_back([&, t] {
            for (int i = 0; i < kPerThread; i++) {
                Req r{t * kPerThread + i, -1, false};
                if (comb.process(&r, run) != status_of(r.id) || r.rc != status_of(r.id)) wrong.fetch_add(1);
            }
        });
    for (auto &th : threads) th.join();
    for (size_t i = 0; i < runs.size(); i++)
        if (runs[i].load() != 1) { fprintf(stderr, "request %zu was run %d times\n", i, runs[i].load()); return 1; }
    if (wrong.load()) { fprintf(stderr, "%d requests got another request's status\n", wrong.load()); return 1; }
    if (!comb.q.empty() || comb.leader) { fprintf(stderr, "combiner not idle at the end\n"); return 1; }
    printf("combiner ok requests=%lld rounds=%lld largest=%d max_batch=%d\n", requests.load(), rounds.load(), largest.load(), comb.max_batch);
    return 0;
}
