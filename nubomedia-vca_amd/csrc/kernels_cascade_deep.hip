// kernels_cascade_deep.hip -- k_deep, the late-stage kernel: one workgroup per window that survived the stages before
// deep_stage, one stump per thread (the long stages have 33..213 stumps); after the first late stage the window's samples
// are staged in LDS.  Launched only for plans whose tiles cannot hold the late stages' samples (deep_stage < nstages).
#include "launch.h"
#include "cascade_device.h"

namespace nvca {

// A stump's vote on a window whose samples are staged, compacted, in LDS (the window's patch): every rectangle corner is two
// u16 map look-ups (column byte offset, row word offset) and one LDS read.  Values and arithmetic are those of stump_vote.
template <bool PAIR, bool UNI = true>
__device__ __forceinline__ double tile_vote(const int *T, const unsigned short *cmap, const unsigned short *rmap,
                                            int xw, int yw, double vnf, CTStumpRec &f)
{
    // the row map holds WORD offsets of the row starts from T, the column map BYTE offsets: a corner address is one shift-add
    auto at = [&](int rw, int cb) { return *(const int *)((const char *)T + ((rw << 2) + cb)); };
    auto rs = [&](int q) {
        const int c0 = cmap[xw + f.x0[q]], c1 = cmap[xw + f.x1[q]];
        const int r0 = rmap[yw + f.y0[q]], r1 = rmap[yw + f.y1[q]];
        return at(r0, c0) - at(r0, c1) - at(r1, c0) + at(r1, c1);
    };
    const int s0 = rs(0);
    const int s1 = rs(1);
    const double t = f.thr * vnf;
    double v;
    if (PAIR) {
        const float fs = (float)s0 * f.w[0] + (float)s1 * f.w[1];
        v = (double)fs;
    } else {
        v = (double)((float)s0 * f.w[0]);
        v += (double)((float)s1 * f.w[1]);
        if ((f.nrect & 255) == 3) {
            const int s2 = rs(2);
            v += (double)((float)s2 * f.w[2]);
        }
    }
    double a0 = f.a0, a1 = f.a1;
    if (UNI) asm("" : "+s"(a0), "+s"(a1));      // wave-uniform record: both votes stay in scalar registers (no dependent load of the selected one)
    return v >= t ? a1 : a0;
}

// ---- K5c: one wave per surviving window, one stump per lane -------------------
__device__ __forceinline__ double wave_sum_exact(double v)
{   // only used where every partial sum is exactly representable (StageRec flag bit 1)
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(256) void k_deep(CascadeArgs a)
{
    // one workgroup per surviving window: every late stage (33..213 stumps) is one step, stump per thread.  The first late
    // stage reads the sum plane directly; a window that passes it gets the ncol x nrow samples all later stumps can touch
    // staged in LDS (DeepRec), and the remaining ~1900 stumps x 8-12 corners become LDS reads.
    __shared__ double part[2][4];
    __shared__ double votes[256];
    extern __shared__ int T[];              // the patch: sized by the plan's largest (a.deep_lds) -- the kernel lives on the windows in flight per CU
    __shared__ unsigned short cmap[kDeepMaxSpan], rmap[kDeepMaxSpan];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long cnt = a.deep[0];
    if (cnt > a.deep_cap) {                              // list overflowed: poison the hit count (host reports it)
        if (blockIdx.x == 0 && tid == 0) atomicAdd(a.hits, 1ull << 40);
        cnt = a.deep_cap;
    }
    int flip = 0;                                        // partial-sum buffers alternate across stages AND windows
    for (unsigned long long i = blockIdx.x; i < cnt; i += gridDim.x) {
        const unsigned long long e = a.deep[1 + i];
        const int slot = (int)(e >> 32);
        const unsigned key = (unsigned)e;
        const int s = key >> a.key_ss, iy = (key >> a.key_sy) & ((1u << (a.key_ss - a.key_sy)) - 1u), ix = key & ((1u << a.key_sy) - 1u);
        const ScaleRec &sc = a.scales[s];
        const int *__restrict__ sum = a.sum + (size_t)slot * a.sum_slot + sc.plane_off;
        const unsigned off = (unsigned)(a.pos[sc.ypos_off + iy] * sc.pitch + a.pos[sc.xpos_off + ix]);
        const double vnf = a.vnf[((size_t)slot * a.ntasks + sc.task_off + (size_t)iy * sc.wpr + (ix >> 6)) * 64 + (ix & 63)];
        DeepRec d; d.ncol = 0;
        if (a.deeprecs) d = a.deeprecs[s];
        CTStumpRec *trecs = (CTStumpRec *)sc.trecs;
        bool alive = true, patch = false;
        for (int st_i = a.deep_stage; st_i < a.nstages; st_i++) {
            const StageRec st = a.stages[st_i];
            const bool pair = a.pair_policy && (st.flags & 1);
            double stage_sum = 0.0;
            if (st_i == a.deep_stage + 1 && d.ncol > 0) {           // passed the first late stage: stage the patch
                const unsigned short *__restrict__ cl = a.tcoords + d.col_off, *__restrict__ rl = a.tcoords + d.row_off;
                const int pitchP = d.ncol | 1;
                __syncthreads();                                  // previous window's patch reads are over
                for (int c = tid; c < d.ncol; c += 256) cmap[cl[c]] = (unsigned short)(c * 4);
                for (int r = tid; r < d.nrow; r += 256) rmap[rl[r]] = (unsigned short)(r * pitchP);
                for (int q = tid; q < d.ncol * d.nrow; q += 256) {
                    const int r = q / d.ncol, c = q - r * d.ncol;
                    T[r * pitchP + c] = sum[off + (unsigned)rl[r] * (unsigned)sc.pitch + cl[c]];
                }
                __syncthreads();
                patch = true;
            }
            auto vote = [&](int j) {
                if (patch) return pair ? tile_vote<true, false>(T, cmap, rmap, 0, 0, vnf, trecs[st.first + j])
                                       : tile_vote<false, false>(T, cmap, rmap, 0, 0, vnf, trecs[st.first + j]);
                return pair ? stump_vote<true>(sum, off, sc.pitch, vnf, trecs[st.first + j]) : stump_vote<false>(sum, off, sc.pitch, vnf, trecs[st.first + j]);
            };
            if (st.flags & 2) {                         // any summation order is exact
                double p = 0.0;
                for (int j = tid; j < st.count; j += 256) p += vote(j);
                p = wave_sum_exact(p);
                if (lane == 0) part[flip][wave] = p;
                __syncthreads();
                stage_sum = (part[flip][0] + part[flip][1]) + (part[flip][2] + part[flip][3]);
                flip ^= 1;
            } else {                                    // keep OpenCV's left-to-right order
                for (int c = 0; c < st.count; c += 256) {
                    const int j = c + tid;
                    const double v = j < st.count ? vote(j) : 0.0;
                    __syncthreads();
                    votes[tid] = v;
                    __syncthreads();
                    const int m = st.count - c < 256 ? st.count - c : 256;
                    for (int l = 0; l < m; l++) stage_sum += votes[l];      // every thread walks the same order
                }
            }
            if (stage_sum < (double)st.thr) { alive = false; break; }
        }
        if (alive && tid == 0) {
            const unsigned long long h = atomicAdd(a.hits, 1ull);
            if (h < a.hit_cap) a.hits[1 + h] = e;
        }
    }
}

void launch_deep(hipStream_t st, const CascadeArgs &a, int batch)
{
    if (batch <= 0 || a.ntasks <= 0 || !(a.deep_stage < a.nstages)) return;
    // grid-stride over the list, one window per workgroup at a time; small jobs (the part detectors' ROI searches) do not
    // need eight thousand workgroups to find a handful of windows
    long long wg = (long long)a.ntasks * batch / 2;
    if (wg < 128) wg = 128;
    if (wg > 8192) wg = 8192;
    NVCA_LAUNCH(k_deep, dim3((unsigned)wg), dim3(256), (size_t)(a.deeprecs ? a.deep_lds : 0), st, a);
}

} // namespace nvca
