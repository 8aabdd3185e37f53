// kernels_roi_hnew.hip -- cv::CascadeClassifier::detectMultiScale of a new-format HAAR cascade on a SMALL image in one workgroup:
// kernels_roi_lbp.hip's sibling for the cascades of kernels_cascade_hnew.hip, for the cascades that were opted in
// (nvca_cascade_set_small_route).  ONE launch serves every such job of a round, one workgroup per (job, pyramid level, band of whole
// grid rows):
//   * the level image: the job's image itself where the level has its size, otherwise cv::resize's 8-bit bilinear rule
//     (resize_sample, tables from the host) into LDS as bytes;
//   * its i32 sum plane and its u32 plane of squared sums in LDS at pitch szw + 1, both from one scan (rows inside waves, then the
//     column pass).  u32 is exact without a high-byte plane: an image inside the route's bound totals less than 2^32 in squares
//     (hnew_roi_tables.h);
//   * A  stage 0 at EVERY grid position of the band, a wave per grid row, 64 columns at a time, the serial walk's skip rule resolved
//        from the reject ballots with the run's parity carried from chunk to chunk (k_roi_lbp's rule).  A lane computes its window's
//        vnf once (hnew_norm, kernels_cascade_hnew.hip's arithmetic) and leaves it in LDS under the window's GRID index: the later
//        stages read it there, and nothing has to stay aligned with the compacted queues;
//   * B  every further stage on the compacted queue, re-queued after every stage (two u16 queues, rotating counters);
//   * C  whoever is left goes to the launch's candidate list as slot << 32 | level << 26 | y << 13 | x (window origin in level pixels).
// Arithmetic of kernels_cascade_hnew.hip (this file is compiled with -ffp-contract=off): rect sums int32; the feature value f32, one
// rounding per product and per addition, the third rect only when its weight is non-zero; the vote (double)ret * vnf < (double)thr;
// the stage sum f64, the leaves added one by one in file order; rejected on sum < (double)thr.  On a short queue the VOTES are
// spread over the waves (a wave per stump and 64 windows, the record wave-uniform), the f32 leaf each selected stored to LDS, and
// one lane per window adds them in file order into its f64 sum -- the same additions, so the same bits.  A stage with more votes
// than the vote area holds runs in consecutive chunks of stumps, the partial sum carried in the owning lane's register.
#include "roi_lds_device.h"
#include "hnew_device.h"
#include <mutex>

namespace nvca {

static constexpr int kRoiHnewThreads = kRoiLbpThreads, kRoiHnewWaves = kRoiLbpWaves;

// the sum plane and the squared plane of a w x h image, (w + 1) x (h + 1) words each at pitch P = w + 1, in place in LDS: lroi_integral's
// scheme with pix * pix as the second element of the same scan (u32 arithmetic, exact below 2^32)
template <class Pix>
__device__ __forceinline__ void hroi_integral2(Pix pix, int w, int h, lroi_i32 *s, lroi_i32 *q, int P)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int X = tid; X <= w; X += kRoiHnewThreads) { s[X] = 0; q[X] = 0; }
    for (int y = wave; y < h; y += kRoiHnewWaves) {
        unsigned cs = 0, cq = 0;
        for (int x0 = 0; x0 < w; x0 += 64) {
            const int x = x0 + lane;
            const unsigned v = x < w ? (unsigned)pix(x, y) : 0u;
            const unsigned is = lroi_wave_scan(v, lane) + cs, iq = lroi_wave_scan(v * v, lane) + cq;
            if (x < w) { s[(y + 1) * P + x + 1] = (int)is; q[(y + 1) * P + x + 1] = (int)iq; }
            cs = (unsigned)__builtin_amdgcn_readlane((int)is, 63); cq = (unsigned)__builtin_amdgcn_readlane((int)iq, 63);
        }
        if (lane == 0) { s[(y + 1) * P] = 0; q[(y + 1) * P] = 0; }
    }
    __syncthreads();
    for (int i = tid; i < 2 * w; i += kRoiHnewThreads) {          // a column of one of the two planes per thread
        lroi_i32 *const a = i < w ? s : q;
        const int x = i < w ? i : i - w;
        unsigned as = 0;
        for (int y = 1; y <= h; y++) { as += (unsigned)a[y * P + x + 1]; a[y * P + x + 1] = (int)as; }
    }
    __syncthreads();
}

// a rect's sum on the window whose origin is p in the plane of pitch P; the four corner offsets come from the wave-uniform record and
// the step's pitch, in scalar registers
__device__ __forceinline__ int hroi_rect(const lroi_i32 *p, int P, const int *r)
{
    const int o0 = r[1] * P + r[0], o2 = o0 + r[3] * P;
    return p[o0] - p[o0 + r[2]] - p[o2] + p[o2 + r[2]];
}
// predictOrderedStump's vote of stump w (wave-uniform) on that window: HaarEvaluator::operator() in f32, the compare in f64
__device__ __forceinline__ float hroi_vote(const lroi_i32 *p, int P, const RoiHnewWeak &w, double vnf)
{
    float ret = w.w[0] * (float)hroi_rect(p, P, w.rect[0]) + w.w[1] * (float)hroi_rect(p, P, w.rect[1]);
    if (w.w[2] != 0.f) ret += w.w[2] * (float)hroi_rect(p, P, w.rect[2]);          // (wave-uniform)
    return (double)ret * vnf < (double)w.thr ? w.leaf[0] : w.leaf[1];
}
// a stage on one window: the f64 sum of the leaves in file order; false: sum < thr
__device__ __forceinline__ bool hroi_stage(const lroi_i32 *p, int P, const RoiHnewWeak *__restrict__ weak, const LbpStageDev st, double vnf)
{
    double sum = 0.;
    for (int k = 0; k < st.count; k++) sum += (double)hroi_vote(p, P, weak[st.first + k], vnf);
    return !(sum < (double)st.thr);
}

// One workgroup per step record: a pyramid level of a job, or a band of whole grid rows of it (at most kRoiMaxWin positions: the host
// splits, roi_split_bands).  Dynamic LDS, every part a multiple of 16 bytes (roi_hnew_lds_bytes): sum plane | squared plane
// (plane_words each) | two queues | counters | votes of a short-queue stage | vnf per grid position; the level image, dead once the
// planes stand, lies over votes + vnf.
__global__ __launch_bounds__(kRoiHnewThreads) void k_roi_hnew(const RoiJobDev *__restrict__ jobs, const RoiStep *__restrict__ steps, const unsigned char *__restrict__ tabs,
                                                              unsigned long long *__restrict__ hits, unsigned hit_cap, int plane_words)
{
    extern __shared__ __align__(16) unsigned char roi_hnew_lds[];
    const RoiStep st = steps[blockIdx.x];
    const RoiJobDev job = jobs[st.job];
    lroi_i32 *const s = (lroi_i32 *)roi_hnew_lds;
    lroi_i32 *const q = s + plane_words;
    unsigned short *const qa = (unsigned short *)(roi_hnew_lds + (size_t)plane_words * 8);       // the second queue lies behind the first
    int *const cnt = (int *)(qa + 2 * kRoiMaxWin);
    float *const votes = (float *)(cnt + 4);
    double *const vnfs = (double *)(votes + kRoiHnewVoteWords);
    lroi_u8 *const lev = (lroi_u8 *)(cnt + 4);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const LbpStageDev *__restrict__ stages = (const LbpStageDev *)job.stages;
    const RoiHnewWeak *__restrict__ weak = (const RoiHnewWeak *)((const unsigned char *)job.stages + roi_hnew_weak_off(job.nstages));
    const int nst = job.nstages;
    const int szw = st.szw, szh = st.szh, P = szw + 1, step = st.step;
    const uint8_t *__restrict__ img = job.img;
    // (the host sizes the planes for the launch's largest level and admits only images whose levels fit: nothing is written otherwise)
    if (szw < 1 || szh < 1 || (szw + 1) * (szh + 1) > plane_words || szw * szh > kRoiHnewLevBytes) return;
    if (tid < 4) cnt[tid] = 0;
    // ---- the level and its two planes
    if (st.mode == 0) {
        hroi_integral2([&](int x, int y) { return img[(size_t)y * job.stride + x]; }, szw, szh, s, q, P);
    } else {
        const ResizeView rt{st.mode, st.xmax, (const int *)(tabs + st.xofs_off), (const short *)(tabs + st.ialpha_off),
                            (const int *)(tabs + st.yofs_off), (const short *)(tabs + st.ibeta_off)};
        for (int i = tid; i < szw * szh; i += kRoiHnewThreads) {
            const int y = i / szw, x = i - y * szw;
            int v;
            resize_sample<1>([&](int r, int c, int *p) { p[0] = img[(size_t)r * job.stride + c]; }, job.h, rt, x, y, &v);
            lev[i] = (uint8_t)v;
        }
        __syncthreads();
        hroi_integral2([&](int x, int y) { return lev[y * szw + x]; }, szw, szh, s, q, P);
    }
    // (hroi_integral2 ends on a barrier: the level image has been read for the last time, votes and vnf may be written over it)
    // the band's grid: origins startX + gx * step, startY + gy * step
    const int nx = (st.endX - st.startX + step - 1) / step, ny = (st.endY - st.startY + step - 1) / step;
    if (nx <= 0 || ny <= 0 || nx * ny > kRoiMaxWin || nst < 1) return;
    // normrect (ex, ey, ew, eh) = (1, 1, ow - 2, oh - 2): its four corners at this level's pitch, HnewArgs::nr's order
    const int n0 = st.ey * P + st.ex, n1 = n0 + st.ew, n2 = n0 + st.eh * P, n3 = n2 + st.ew;
    const double area = (double)st.ew * (double)st.eh;
    // ---- A: stage 0 everywhere, the skip rule per row
    const LbpStageDev s0 = stages[0];
    for (int gy = wave; gy < ny; gy += kRoiHnewWaves) {
        int carry = 0;
        for (int c0 = 0; c0 < nx; c0 += 64) {
            const int gx = c0 + lane;
            const bool in = gx < nx;
            bool pass0 = false;
            if (in) {
                const int o = (st.startY + gy * step) * P + st.startX + gx * step;
                const lroi_i32 *p = s + o, *pq = q + o;
                const int valsum = p[n0] - p[n1] - p[n2] + p[n3];
                const unsigned valsq = (unsigned)pq[n0] - (unsigned)pq[n1] - (unsigned)pq[n2] + (unsigned)pq[n3];      // exact: below 2^32
                const double vnf = hnew_norm(area, (double)valsq, valsum);
                vnfs[gy * nx + gx] = vnf;
                pass0 = hroi_stage(p, P, weak, s0, vnf);
            }
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
        if (n <= kRoiHnewShortWin) {
            // short queue: a wave per (stump k, 64 windows), the record wave-uniform; votes[k][window].  kper stumps a chunk (64 on a
            // queue of one wave, 16 on the longest), the f64 sum of the window under this thread's index carried from chunk to chunk
            const int nch = (n + 63) >> 6, npad = nch * 64, kper = kRoiHnewVoteWords / npad;
            double sum = 0.;
            for (int k0 = 0; k0 < sr.count; k0 += kper) {
                const int kc = sr.count - k0 < kper ? sr.count - k0 : kper;
                if (k0) __syncthreads();                   // the chunk before has been added up: its votes may be overwritten
                for (int t = wave; t < kc * nch; t += kRoiHnewWaves) {
                    const int k = t / nch, i = (t - k * nch) * 64 + lane;
                    if (i < n) {
                        const int wi = qi[i], gy = wi / nx, gx = wi - gy * nx;
                        votes[k * npad + i] = hroi_vote(s + (st.startY + gy * step) * P + st.startX + gx * step, P, weak[sr.first + k0 + k], vnfs[wi]);
                    }
                }
                __syncthreads();
                if (tid < n)
                    for (int k = 0; k < kc; k++) sum += (double)votes[k * npad + tid];          // file order, one rounding per addition
            }
            if (tid < npad) {                          // the waves that hold a window of the queue (wave-uniform)
                const bool pass = tid < n && !(sum < (double)sr.thr);
                lroi_push(pass, tid < n ? (int)qi[tid] : 0, qo, &cnt[cout], lane);
            }
        } else {
            for (int base = 0; base < n; base += kRoiHnewThreads) {
                const int i = base + tid;
                bool pass = false; int wi = 0;
                if (i < n) {
                    wi = qi[i];
                    const int gy = wi / nx, gx = wi - gy * nx;
                    pass = hroi_stage(s + (st.startY + gy * step) * P + st.startX + gx * step, P, weak, sr, vnfs[wi]);
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
        for (int k = tid; k < nleft; k += kRoiHnewThreads) {
            const int wi = qi[k], gy = wi / nx, gx = wi - gy * nx;
            const unsigned key = ((unsigned)st.key_step << 26) | ((unsigned)(st.key_y0 + gy * st.key_dy) << 13) | (unsigned)(st.key_x0 + gx * st.key_dx);
            if (hb + k < hit_cap) hits[1 + hb + k] = slot | key;
        }
    }
}

void launch_roi_hnew(hipStream_t st, const RoiJobDev *jobs, int nsteps, const RoiStep *steps, const unsigned char *tabs, unsigned long long *hits,
                     unsigned hit_cap, int plane_words, int lds_bytes)
{
    NVCA_LAUNCH(k_roi_hnew, dim3(nsteps), dim3(kRoiHnewThreads), (size_t)lds_bytes, st, jobs, steps, tabs, hits, hit_cap, plane_words);
}
int roi_hnew_grant_lds(int bytes)
{
    static std::mutex mu;
    static int granted[64] = {0};
    std::lock_guard<std::mutex> lk(mu);
    int dev = 0; (void)hipGetDevice(&dev); dev &= 63;
    if (bytes <= granted[dev]) return 0;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_roi_hnew), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return (int)e;
    granted[dev] = bytes;
    return 0;
}

} // namespace nvca
