// work_pool.h -- the helper-thread pool of work_pool.cpp.  Includes nothing.
#pragma once

namespace nvca {

// A few helper threads for host work that is independent per job (the candidate lists of a round's face-region searches are
// converted, replayed and grouped job by job: 96 jobs of ~50 us on the calling thread were most of a loaded part batch).
// The caller takes part; run() returns when every index has been handled.  Created on first use, joined with the context.
struct WorkPool;
WorkPool *work_pool_create(int threads);
void work_pool_destroy(WorkPool *p);
void work_pool_run(WorkPool *p, int n, void (*fn)(void *arg, int i), void *arg);     // p == nullptr: serial
int work_pool_threads(const WorkPool *p);          // helper threads (0 for nullptr)

} // namespace nvca
