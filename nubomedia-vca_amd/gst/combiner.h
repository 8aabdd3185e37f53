// combiner.h -- the shim's frame combiner (standard library only: tests/san/combiner_driver.cpp runs it under ThreadSanitizer).
// Frames of different elements of one kind that arrive while the GPU is busy are combined into one batched call.  The
// first streaming thread to arrive leads: it takes whatever has queued up (its own frame included), runs the batched
// entry point on the lot and wakes the owners; threads that arrive meanwhile queue up for the next round, so the batch
// grows with the load and an idle pipeline still sees single-frame latency.  Results are those of per-frame calls:
// streams are independent and a batch keeps the order of each stream's frames.
// Req has `int rc` (what process returns to the owner; run sets it) and `bool done`.
#pragma once
#include <stdlib.h>
#include <condition_variable>
#include <mutex>
#include <vector>

template <class Req> struct Combiner {
    std::mutex m;
    std::condition_variable cv;
    std::vector<Req *> q;
    bool leader = false;
    int max_batch = 0;                                      /* largest batch seen (NVCA_GST_STATS) */
    template <class Run> int process(Req *req, Run run)
    {
        static const bool off = getenv("NVCA_GST_NO_COMBINE") != NULL;     /* A/B switch: every frame on its own */
        if (off) { std::vector<Req *> one(1, req); run(one); return req->rc; }
        std::unique_lock<std::mutex> lk(m);
        req->done = false;
        q.push_back(req);
        while (!req->done) {
            if (leader) { cv.wait(lk); continue; }
            leader = true;
            std::vector<Req *> round;
            round.swap(q);
            lk.unlock();
            run(round);
            lk.lock();
            if ((int)round.size() > max_batch) max_batch = (int)round.size();
            for (Req *r : round) r->done = true;
            leader = false;
            cv.notify_all();
        }
        return req->rc;
    }
};
