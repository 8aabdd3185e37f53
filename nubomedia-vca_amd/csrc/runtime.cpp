// runtime.cpp -- device and page-locked buffers (with the NVCA_ALLOC_GUARD / NVCA_ALLOC_LOG diagnostics), kernel timing,
// launch-error capture, the exception barrier's handler and the process-wide switches.
#include "host_state.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <stdexcept>
#include <new>

using namespace nvca;

// =========================================================================
// buffers, timing
// =========================================================================
namespace nvca {

// NVCA_ALLOC_LOG=1 (diagnostic): every device allocation and release on stderr -- a GPU memory fault names an address, this says whose
bool alloc_log() { static const bool on = getenv("NVCA_ALLOC_LOG") != nullptr; return on; }
// NVCA_ALLOC_GUARD=1 (diagnostic, "electric fence"): every device buffer is mapped through the virtual-memory API with an
// unmapped guard range before and behind it and ends (to 256 bytes) where its mapping ends, with no head-room: a kernel that
// reads or writes past a buffer faults at that access, every time, instead of now and then when the neighbouring pages happen
// to be unmapped.  Costs an allocation granule (2 MiB) per buffer; never on in production.
// NVCA_ALLOC_GUARD=1: released buffers stay mapped (leaked: a test run allocates a few GB in all); =2: they are unmapped and their
// address range stays reserved (a use after release faults too); =3: unmapped, released and the range freed.
static int alloc_guard_mode() { static const int m = getenv("NVCA_ALLOC_GUARD") ? std::max(1, atoi(getenv("NVCA_ALLOC_GUARD"))) : 0; return m; }
static bool alloc_guard() { return alloc_guard_mode() > 0; }
namespace {
struct GuardRec { void *va; size_t total, mapped, lead; hipMemGenericAllocationHandle_t h; };
std::map<void *, GuardRec> g_guard;
std::mutex g_guard_mu;
hipError_t guard_alloc(void **out, size_t n)
{
    int dev = 0; (void)hipGetDevice(&dev);
    hipMemAllocationProp prop; memset(&prop, 0, sizeof(prop));
    prop.type = hipMemAllocationTypePinned; prop.location.type = hipMemLocationTypeDevice; prop.location.id = dev;
    size_t gran = 0;
    hipError_t e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum);
    if (e != hipSuccess || gran == 0) return e != hipSuccess ? e : hipErrorUnknown;
    const size_t body = (n + 255) & ~(size_t)255, mapped = (body + gran - 1) / gran * gran;
    GuardRec r; r.total = mapped + 2 * gran; r.mapped = mapped; r.lead = gran; r.va = nullptr;
    if ((e = hipMemAddressReserve(&r.va, r.total, gran, nullptr, 0)) != hipSuccess) return e;
    if ((e = hipMemCreate(&r.h, mapped, &prop, 0)) != hipSuccess) { (void)hipMemAddressFree(r.va, r.total); return e; }
    char *base = (char *)r.va + gran;
    if ((e = hipMemMap(base, mapped, 0, r.h, 0)) != hipSuccess) { (void)hipMemRelease(r.h); (void)hipMemAddressFree(r.va, r.total); return e; }
    hipMemAccessDesc acc; memset(&acc, 0, sizeof(acc));
    acc.location.type = hipMemLocationTypeDevice; acc.location.id = dev; acc.flags = hipMemAccessFlagsProtReadWrite;
    if ((e = hipMemSetAccess(base, mapped, &acc, 1)) != hipSuccess) { (void)hipMemUnmap(base, mapped); (void)hipMemRelease(r.h); (void)hipMemAddressFree(r.va, r.total); return e; }
    *out = base + (mapped - body);                       // the buffer ends where the mapping ends
    std::lock_guard<std::mutex> lk(g_guard_mu);
    g_guard[*out] = r;
    return hipSuccess;
}
void guard_free(void *p)
{
    GuardRec r;
    { std::lock_guard<std::mutex> lk(g_guard_mu);
      auto it = g_guard.find(p);
      if (it == g_guard.end()) { (void)hipFree(p); return; }
      r = it->second; g_guard.erase(it); }
    (void)hipDeviceSynchronize();
    if (alloc_guard_mode() >= 2) (void)hipMemUnmap((char *)r.va + r.lead, r.mapped);
    if (alloc_guard_mode() >= 3) { (void)hipMemRelease(r.h); (void)hipMemAddressFree(r.va, r.total); }
}
}
int DevBuf::ensure(size_t n)
{
    if (n <= bytes) return 0;
    static bool guard_broken = false;          // the runtime refused the virtual-memory calls: said once, plain allocations from then on
    if (alloc_guard() && !guard_broken) {
        if (p) { (void)hipDeviceSynchronize(); if (alloc_log()) fprintf(stderr, "[nvca alloc] free  %p (%zu bytes, grows)\n", p, bytes); guard_free(p); p = nullptr; bytes = 0; }
        const hipError_t ge = guard_alloc(&p, n);
        if (ge == hipSuccess) {
            bytes = n;
            if (alloc_log()) fprintf(stderr, "[nvca alloc] alloc %p .. %p (%zu bytes, guarded)\n", p, (void *)((char *)p + n), n);
            return 0;
        }
        (void)hipGetLastError(); p = nullptr; bytes = 0; guard_broken = true;
        fprintf(stderr, "[nvca alloc] guard unavailable (%s): plain allocations\n", hipGetErrorString(ge));
    }
    if (p) { (void)hipDeviceSynchronize(); if (alloc_log()) fprintf(stderr, "[nvca alloc] free  %p (%zu bytes, grows)\n", p, bytes); (void)hipFree(p); p = nullptr; bytes = 0; }
    size_t want = n + n / 4;                                  // head-room: batches grow
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; e = hipMalloc(&p, n); want = n; }    // the refused head-room attempt must not surface later as a launch error
    if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; bytes = 0; return (int)e; }
    bytes = want;
    if (alloc_log()) fprintf(stderr, "[nvca alloc] alloc %p .. %p (%zu bytes, %zu asked)\n", p, (void *)((char *)p + want), want, n);
    return 0;
}
void DevBuf::release() { if (p && bytes) { if (alloc_log()) fprintf(stderr, "[nvca alloc] free  %p (%zu bytes)\n", p, bytes); if (alloc_guard()) guard_free(p); else (void)hipFree(p); } p = nullptr; bytes = 0; }     // bytes == 0: a view into another buffer
int PinnedBuf::ensure(size_t n)
{
    if (n <= bytes) return 0;
    if (p) { (void)hipDeviceSynchronize(); (void)hipHostFree(p); p = nullptr; bytes = 0; }
    hipError_t e = hipHostMalloc(&p, n, hipHostMallocDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; return (int)e; }
    bytes = n;
    return 0;
}
void PinnedBuf::release() { if (p) { (void)hipHostFree(p); p = nullptr; bytes = 0; } }

static thread_local TimedLaunch *g_scope = nullptr;
TimedLaunch::TimedLaunch(nvca_ctx *c, int kind) : ctx(c), k(kind)
{
    if (!ctx->timer.on || !ctx->timer.sample) return;
    active = true; prev = g_scope; g_scope = this;
}
TimedLaunch::~TimedLaunch()
{
    if (active) g_scope = prev;
}
static thread_local hipError_t g_launch_err = hipSuccess;
static thread_local const char *g_launch_kernel = nullptr;
void note_launch(const char *kernel)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess && g_launch_err == hipSuccess) { g_launch_err = e; g_launch_kernel = kernel; }
}
hipError_t take_launch_error(const char **kernel)
{
    const hipError_t e = g_launch_err;
    if (kernel) *kernel = g_launch_kernel;
    g_launch_err = hipSuccess; g_launch_kernel = nullptr;
    return e;
}
bool launch_events(hipEvent_t *a, hipEvent_t *b)
{
    TimedLaunch *sc = g_scope;
    if (!sc) return false;
    KernelTimer &t = sc->ctx->timer;
    auto get = [&]() {
        hipEvent_t e = nullptr;
        if (!t.pool.empty()) { e = t.pool.back(); t.pool.pop_back(); }
        else (void)hipEventCreate(&e);
        return e;
    };
    *a = get(); *b = get();
    if (!*a || !*b) return false;
    t.pending.push_back(KernelTimer::Ev{*a, *b, sc->k, sc->n++ == 0});
    return true;
}
void drain_timer_now(nvca_ctx *ctx)
{
    KernelTimer &t = ctx->timer;
    std::vector<KernelTimer::Ev> later;
    bool stop = false;
    for (auto &e : t.pending) {
        float ms = 0;
        // kernels finish in launch order: after the first pair that is not ready (a batch still in flight between
        // submit and collect) nothing later is either, and asking again for every one of them is not free
        if (stop || hipEventQuery(e.b) == hipErrorNotReady) { stop = true; later.push_back(e); continue; }
        const hipError_t r = hipEventElapsedTime(&ms, e.a, e.b);
        if (r == hipErrorNotReady) { stop = true; later.push_back(e); continue; }
        if (r == hipSuccess) { t.total_ms[e.k] += ms; if (e.first) t.launches[e.k]++; }
        t.pool.push_back(e.a); t.pool.push_back(e.b);
    }
    t.pending.swap(later);
}
// Event pairs are turned into times when somebody asks (nvca_ctx_kernel_timing) or when many have piled up: querying them
// after every batch costs more than it looks while another batch is executing.
void drain_timer(nvca_ctx *ctx)
{
    if (ctx->timer.pending.size() > 4096) drain_timer_now(ctx);
}

// handler of the ABI's function-try-blocks (NVCA_API_CATCH): called inside a catch (...) clause
int api_catch(nvca_ctx *ctx) noexcept
{
    int code = NVCA_ERR_INTERNAL;
    const char *what = "unknown exception";
    char buf[160];
    try { throw; }
    catch (const std::bad_alloc &) { code = NVCA_ERR_NOMEM; what = "out of host memory (std::bad_alloc)"; }
    catch (const std::length_error &e) { code = NVCA_ERR_NOMEM; snprintf(buf, sizeof(buf), "container size limit exceeded (%s)", e.what()); what = buf; }
    catch (const std::exception &e) { snprintf(buf, sizeof(buf), "internal error: %s", e.what()); what = buf; }
    catch (...) { }
    if (ctx) {
        try { std::lock_guard<std::recursive_mutex> lk(ctx->mu); ctx->err.assign(what); } catch (...) { }
    }
    return code;
}

const Switches &switches()
{
    static const Switches w = read_switches();      // first use: nvca_ctx_create
    return w;
}

} // namespace nvca
