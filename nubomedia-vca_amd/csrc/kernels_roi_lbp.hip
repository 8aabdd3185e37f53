// kernels_roi_lbp.hip -- cv::CascadeClassifier::detectMultiScale of a new-format LBP cascade on a SMALL image in one workgroup:
// kernels_roi.hip's sibling for the cascades of kernels_cascade_lbp.hip.  The part detectors search a face region of
// a few thousand pixels, many times per frame and stream, at a size that changes from frame to frame; the large-image route pays a
// cached plan per size and a dozen launches per region.  Here ONE launch serves every such job of a round, one workgroup per
// (job, pyramid level, band of whole grid rows):
//   * the level image: the job's image itself where the level has its size, otherwise cv::resize's 8-bit bilinear rule
//     (resize_sample, tables from the host) into LDS as bytes;
//   * its i32 sum plane in LDS at pitch szw + 1 (row scans inside waves, then the column pass) -- no squared plane, no normaliser;
//   * A  stage 0 at EVERY grid position of the band (origins gx * step, gy * step), a wave per grid row, 64 columns at a time; the
//        serial walk's skip rule (a stage-0 reject skips the next grid column) is resolved per row from the reject ballots: a column is
//        visited iff the run of stage-0 rejects immediately to its left has even length, the run's parity carried from chunk to chunk.
//        Only visited windows that pass stage 0 are queued: a skipped column that would have passed is never emitted;
//   * B  every further stage on the compacted queue, re-queued after every stage (two u16 queues, rotating counters);
//   * C  whoever is left goes to the launch's candidate list as slot << 32 | level << 26 | y << 13 | x (window origin in level pixels).
// Arithmetic of kernels_cascade_lbp.hip: the same cell order, >= ties and subset-word pick; a stage is the f32 sum of its votes in file
// order, one rounding per addition (contraction off), rejected on tmp < thr.  LBP leaves are arbitrary floats, so no partial sums in
// another order: on a short queue the VOTES are spread over the waves (a wave per weak classifier and 64 windows, the record
// wave-uniform), stored to LDS, and one lane per window adds them in file order -- the same additions.
#include "roi_lds_device.h"
#include <mutex>

namespace nvca {

// predictCategoricalStump's vote of weak classifier w (wave-uniform) on the window whose origin is p in the plane of pitch P:
// lbp_code's cell order and ties, lbp_vote's word pick (kernels_cascade_lbp.hip)
__device__ __forceinline__ float lroi_vote(const lroi_i32 *p, int P, const RoiLbpWeak &w)
{
    int v[16];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int ro = (w.y + r * w.h) * P + w.x;
#pragma unroll
        for (int c = 0; c < 4; c++) v[r * 4 + c] = p[ro + c * w.w];
    }
    auto cell = [&](int r, int c) { return v[r * 4 + c] - v[r * 4 + c + 1] - v[r * 4 + 4 + c] + v[r * 4 + 5 + c]; };
    const int ctr = cell(1, 1);
    const int code = (cell(0, 0) >= ctr ? 128 : 0) | (cell(0, 1) >= ctr ? 64 : 0) | (cell(0, 2) >= ctr ? 32 : 0) | (cell(1, 2) >= ctr ? 16 : 0) |
                     (cell(2, 2) >= ctr ? 8 : 0) | (cell(2, 1) >= ctr ? 4 : 0) | (cell(2, 0) >= ctr ? 2 : 0) | (cell(1, 0) >= ctr ? 1 : 0);
    const int i = code >> 5;
    int word = w.subset[0];
    word = i == 1 ? w.subset[1] : word; word = i == 2 ? w.subset[2] : word; word = i == 3 ? w.subset[3] : word;
    word = i == 4 ? w.subset[4] : word; word = i == 5 ? w.subset[5] : word; word = i == 6 ? w.subset[6] : word;
    word = i == 7 ? w.subset[7] : word;
    return ((unsigned)word >> (code & 31)) & 1u ? w.leaf[0] : w.leaf[1];
}

// a stage on one window: the f32 sum of the votes in file order, one rounding per addition; false: tmp < thr
__device__ __forceinline__ bool lroi_stage(const lroi_i32 *p, int P, const RoiLbpWeak *__restrict__ weak, const LbpStageDev st)
{
    float tmp = 0.f;
    for (int k = 0; k < st.count; k++) tmp += lroi_vote(p, P, weak[st.first + k]);
    return !(tmp < st.thr);
}

// One workgroup per step record: a pyramid level of a job, or a band of whole grid rows of it (at most kRoiMaxWin positions: the host
// splits, roi_split_bands).  Dynamic LDS, every part a multiple of 16 bytes (roi_lbp_lds_bytes): sum plane (plane_words) | two
// queues | counters | votes of a short-queue stage | the level image.
__global__ __launch_bounds__(kRoiLbpThreads) void k_roi_lbp(const RoiJobDev *__restrict__ jobs, const RoiStep *__restrict__ steps, const unsigned char *__restrict__ tabs,
                                                            unsigned long long *__restrict__ hits, unsigned hit_cap, int plane_words)
{
    extern __shared__ __align__(16) unsigned char roi_lbp_lds[];
    const RoiStep st = steps[blockIdx.x];
    const RoiJobDev job = jobs[st.job];
    lroi_i32 *const s = (lroi_i32 *)roi_lbp_lds;
    unsigned short *const qa = (unsigned short *)(roi_lbp_lds + (size_t)plane_words * 4);       // the second queue lies behind the first
    int *const cnt = (int *)(qa + 2 * kRoiMaxWin);
    float *const votes = (float *)(cnt + 4);
    lroi_u8 *const lev = (lroi_u8 *)(votes + kRoiLbpVoteWords);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const LbpStageDev *__restrict__ stages = (const LbpStageDev *)job.stages;
    const RoiLbpWeak *__restrict__ weak = (const RoiLbpWeak *)((const unsigned char *)job.stages + roi_lbp_weak_off(job.nstages));
    const int nst = job.nstages;
    const int szw = st.szw, szh = st.szh, P = szw + 1, step = st.step;
    const uint8_t *__restrict__ img = job.img;
    if (tid < 4) cnt[tid] = 0;
    // ---- the level and its sum plane
    if (st.mode == 0) {
        lroi_integral([&](int x, int y) { return img[(size_t)y * job.stride + x]; }, szw, szh, s, P);
    } else {
        const ResizeView rt{st.mode, st.xmax, (const int *)(tabs + st.xofs_off), (const short *)(tabs + st.ialpha_off),
                            (const int *)(tabs + st.yofs_off), (const short *)(tabs + st.ibeta_off)};
        for (int i = tid; i < szw * szh; i += kRoiLbpThreads) {
            const int y = i / szw, x = i - y * szw;
            int v;
            resize_sample<1>([&](int r, int c, int *p) { p[0] = img[(size_t)r * job.stride + c]; }, job.h, rt, x, y, &v);
            lev[i] = (uint8_t)v;
        }
        __syncthreads();
        lroi_integral([&](int x, int y) { return lev[y * szw + x]; }, szw, szh, s, P);
    }
    // the band's grid: origins startX + gx * step, startY + gy * step
    const int nx = (st.endX - st.startX + step - 1) / step, ny = (st.endY - st.startY + step - 1) / step;
    if (nx <= 0 || ny <= 0 || nx * ny > kRoiMaxWin || nst < 1) return;
    // ---- A: stage 0 everywhere, the skip rule per row
    const LbpStageDev s0 = stages[0];
    for (int gy = wave; gy < ny; gy += kRoiLbpWaves) {
        int carry = 0;
        for (int c0 = 0; c0 < nx; c0 += 64) {
            const int gx = c0 + lane;
            const bool in = gx < nx;
            bool pass0 = false;
            if (in) pass0 = lroi_stage(s + (st.startY + gy * step) * P + st.startX + gx * step, P, weak, s0);
            const unsigned long long rej = __ballot(in && !pass0);
            // column gx is visited iff the run of stage-0 rejects immediately to its left has even length
            const unsigned long long below = lane ? (rej << (64 - lane)) : 0ull;       // bit 63 = lane - 1
            int ones = lane ? __clzll((long long)~below) : 0;
            if (ones > lane) ones = lane;
            const bool visited = in && !(ones == lane ? ((lane + carry) & 1) : (ones & 1));
            lroi_push(visited && pass0, gy * nx + gx, qa, &cnt[0], lane);
            const int nin = nx - c0 < 64 ? nx - c0 : 64;                      // the reject run that ends at this chunk's right edge
            const unsigned long long top = nin < 64 ? (rej << (64 - nin)) : rej;
            int tail = ~top ? __clzll((long long)~top) : 64;
            if (tail > nin) tail = nin;
            carry = tail == nin ? ((nin + carry) & 1) : (tail & 1);
        }
    }
    // ---- B: stage after stage on the compacted queue; the counters rotate over three words (read cin, append to cout, clear the third)
    int cin = 0, cur = 0;
    for (int sidx = 1; sidx < nst; sidx++) {
        __syncthreads();
        const int n = cnt[cin];
        if (n == 0) break;
        const int cout = cin == 2 ? 0 : cin + 1;
        if (tid == 0) cnt[cout == 2 ? 0 : cout + 1] = 0;
        const unsigned short *qi = qa + cur * kRoiMaxWin;
        unsigned short *qo = qa + (cur ^ 1) * kRoiMaxWin;
        const LbpStageDev sr = stages[sidx];
        const int nch = (n + 63) >> 6, npad = nch * 64;
        if (n <= kRoiLbpShortWin && sr.count * npad <= kRoiLbpVoteWords) {
            // short queue: a wave per (weak classifier k, 64 windows), the record wave-uniform; votes[k][window]
            for (int t = wave; t < sr.count * nch; t += kRoiLbpWaves) {
                const int k = t / nch, i = (t - k * nch) * 64 + lane;
                if (i < n) {
                    const int wi = qi[i], gy = wi / nx, gx = wi - gy * nx;
                    votes[k * npad + i] = lroi_vote(s + (st.startY + gy * step) * P + st.startX + gx * step, P, weak[sr.first + k]);
                }
            }
            __syncthreads();
            if (tid < npad) {                          // the waves that hold a window of the queue (wave-uniform)
                bool pass = false; int wi = 0;
                if (tid < n) {
                    float tmp = 0.f;
                    for (int k = 0; k < sr.count; k++) tmp += votes[k * npad + tid];          // file order, one rounding per addition
                    pass = !(tmp < sr.thr); wi = qi[tid];
                }
                lroi_push(pass, wi, qo, &cnt[cout], lane);
            }
        } else {
            for (int base = 0; base < n; base += kRoiLbpThreads) {
                const int i = base + tid;
                bool pass = false; int wi = 0;
                if (i < n) {
                    wi = qi[i];
                    const int gy = wi / nx, gx = wi - gy * nx;
                    pass = lroi_stage(s + (st.startY + gy * step) * P + st.startX + gx * step, P, weak, sr);
                }
                lroi_push(pass, wi, qo, &cnt[cout], lane);
            }
        }
        cur ^= 1; cin = cout;
    }
    __syncthreads();
    // ---- C: whoever is left passed every stage
    const int nleft = cnt[cin];
    if (nleft > 0) {
        if (tid == 0) cnt[3] = (int)(unsigned)atomicAdd(hits, (unsigned long long)nleft);
        __syncthreads();
        const unsigned long long hb = (unsigned long long)(unsigned)cnt[3], slot = (unsigned long long)job.slot << 32;
        const unsigned short *qi = qa + cur * kRoiMaxWin;
        for (int k = tid; k < nleft; k += kRoiLbpThreads) {
            const int wi = qi[k], gy = wi / nx, gx = wi - gy * nx;
            const unsigned key = ((unsigned)st.key_step << 26) | ((unsigned)(st.key_y0 + gy * st.key_dy) << 13) | (unsigned)(st.key_x0 + gx * st.key_dx);
            if (hb + k < hit_cap) hits[1 + hb + k] = slot | key;
        }
    }
}

void launch_roi_lbp(hipStream_t st, const RoiJobDev *jobs, int nsteps, const RoiStep *steps, const unsigned char *tabs, unsigned long long *hits,
                    unsigned hit_cap, int plane_words, int lds_bytes)
{
    NVCA_LAUNCH(k_roi_lbp, dim3(nsteps), dim3(kRoiLbpThreads), (size_t)lds_bytes, st, jobs, steps, tabs, hits, hit_cap, plane_words);
}
int roi_lbp_grant_lds(int bytes)
{
    static std::mutex mu;
    static int granted[64] = {0};
    std::lock_guard<std::mutex> lk(mu);
    int dev = 0; (void)hipGetDevice(&dev); dev &= 63;
    if (bytes <= granted[dev]) return 0;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_roi_lbp), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return (int)e;
    granted[dev] = bytes;
    return 0;
}

} // namespace nvca
