// kernels_cascade_gather.hip -- the cascade kernels that read the integral planes with global gathers, a window per lane:
//  k_stage0      variance + stage 0 for every window (reject bits + variance normaliser per window): the pre-pass of
//                k_tile / k_strip for batches too small for k_band (plans.cpp)
//  k_strip       stages 1 .. deep_stage-1 on row strips: the older variant of k_tile (NVCA_TILES=0; the fallback when a
//                plan has no tiles)
//  k_gen_stage0, k_gen_rest   the same two steps for general cascades (tree-structured weak classifiers, tilted features)
// Stump records are geometry-independent tables per (cascade, factor), wave-uniform (scalar loads).  No MFMA: integer rect
// sums, f32 products, f64 stage sums -- exactly the reference's arithmetic (compiled with -ffp-contract=off).
#include "launch.h"
#include "cascade_device.h"

namespace nvca {

// Squared-pixel sum of the variance window from the squared integral, as the f64 OpenCV computes (every operand and every
// partial result is an integer below 2^53, so the f64 chain is exact and equals the integer result).  The plane pair is a
// u32 low-word plane and a u8 high-byte plane (the values stay below 2^40 whenever the i32 sum plane is valid); when the
// window's sum is known to be below 2^32 the low words alone give it, modulo 2^32.
__device__ __forceinline__ double window_sqsum(const unsigned *__restrict__ sql, const uint8_t *__restrict__ sqh, bool lo_only,
                                               unsigned e0, unsigned e1, unsigned e2, unsigned e3)
{
    if (lo_only) return (double)(unsigned)(sql[e0] - sql[e1] - sql[e2] + sql[e3]);
    const unsigned long long q0 = ((unsigned long long)sqh[e0] << 32) | sql[e0], q1 = ((unsigned long long)sqh[e1] << 32) | sql[e1];
    const unsigned long long q2 = ((unsigned long long)sqh[e2] << 32) | sql[e2], q3 = ((unsigned long long)sqh[e3] << 32) | sql[e3];
    return (double)q0 - (double)q1 - (double)q2 + (double)q3;
}

// one stage on one window per lane; recs are wave-uniform (scalar loads)
template <bool PAIR>
__device__ __forceinline__ bool eval_stage(const int *__restrict__ sum, unsigned off, int pitch, double vnf,
                                           CTStumpRec *recs, int count, float stage_thr)
{
    double stage_sum = 0.0;
    for (int j = 0; j < count; j++) stage_sum += stump_vote<PAIR, CTStumpRec, true>(sum, off, pitch, vnf, recs[j]);
    return !(stage_sum < (double)stage_thr);
}

__device__ __forceinline__ bool run_stage(const int *__restrict__ sum, unsigned off, int pitch, double vnf,
                                          CTStumpRec *recs, const StageRec &st, int pair_policy)
{
    if (pair_policy && (st.flags & 1)) return eval_stage<true>(sum, off, pitch, vnf, recs + st.first, st.count, st.thr);
    return eval_stage<false>(sum, off, pitch, vnf, recs + st.first, st.count, st.thr);
}

// block -> (slot, local index): 1-D grid, frame-major (few integral planes live at a time); within a
// frame consecutive local indices alternate over 8 contiguous chunks, i.e. blocks that share an XCD
// (b % 8) walk one contiguous part of the scan (speed only)
__device__ __forceinline__ bool xcd_chunk_index(int nlocal, int &slot, int &idx)
{
    const int per_frame = ((nlocal + 7) / 8) * 8;
    slot = blockIdx.x / per_frame;
    const int l = blockIdx.x - slot * per_frame;
    const int chunk = per_frame / 8;
    idx = (l & 7) * chunk + (l >> 3);
    return idx < nlocal;
}

// ---- K5a: variance + stage 0 for every window --------------------------------
__global__ __launch_bounds__(256) void k_stage0(CascadeArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int slot, bidx;
    if (!xcd_chunk_index((a.ntasks + 3) / 4, slot, bidx)) return;
    const int t = __builtin_amdgcn_readfirstlane(bidx * 4 + wave);
    if (t >= a.ntasks) return;
    const unsigned task = a.tasks[t];
    const int s = task >> 20, iy = (task >> 7) & 8191, k = task & 127;
    const ScaleRec &sc = a.scales[s];
    const int ix = k * 64 + lane;
    const bool active = ix < sc.endX;
    const int *__restrict__ sum = a.sum + (size_t)slot * a.sum_slot + sc.plane_off;
    // squared integral: a u32 low-word plane and a u8 high-byte plane per slot, see k_integral
    const unsigned *__restrict__ sql = (const unsigned *)a.sqsum + (size_t)slot * 2 * a.sum_slot + sc.plane_off;
    const uint8_t *__restrict__ sqh = (const uint8_t *)((const unsigned *)a.sqsum + (size_t)slot * 2 * a.sum_slot + a.sum_slot) + sc.plane_off;
    bool pass0 = false;
    double vnf = 1.;
    if (active) {
        const unsigned off = (unsigned)(a.pos[sc.ypos_off + iy] * sc.pitch + a.pos[sc.xpos_off + ix]);
        const unsigned e0 = off + sc.eq[0], e1 = off + sc.eq[1], e2 = off + sc.eq[2], e3 = off + sc.eq[3];
        const int ws = sum[e0] - sum[e1] - sum[e2] + sum[e3];
        const double mean = (double)ws * sc.inv_area;
        vnf = window_sqsum(sql, sqh, sc.sq32 != 0, e0, e1, e2, e3);
        vnf = vnf * sc.inv_area - mean * mean;
        vnf = vnf >= 0. ? sqrt(vnf) : 1.;
        pass0 = run_stage(sum, off, sc.pitch, vnf, (CTStumpRec *)sc.trecs, a.stages[0], a.pair_policy);
    }
    const unsigned long long fb = __ballot(active && !pass0);
    const size_t o = (size_t)slot * a.ntasks + t;
    if (lane == 0) a.failbits[o] = fb;
    a.vnf[o * 64 + lane] = vnf;
}

// ---- general cascades: tree-structured weak classifiers and / or tilted features ----------------------------------------
// cvRunHaarClassifierCascadeSum's general branch: per weak classifier a walk idx = sum < t ? left : right from the root to
// a leaf, whose value is the vote; a feature's rectangles read the integral image or, for a tilted feature, the tilted
// integral.  Window per lane, global reads (these cascades run on the part detectors' small working images; the LDS tile
// machinery above is built around upright stumps).  The stage loop is wave-uniform, so the root of every weak classifier is
// a scalar record; only the nodes below it are per-lane.
typedef const __attribute__((address_space(4))) GNodeRec CGNodeRec;
template <class Rec>
__device__ __forceinline__ double gen_node_sum(const int *__restrict__ pl, unsigned off, int pitch, const Rec &n, bool pair)
{
    auto rs = [&](int q) {
        return pl[off + (unsigned)(n.dy[q][0] * pitch + n.dx[q][0])] - pl[off + (unsigned)(n.dy[q][1] * pitch + n.dx[q][1])] -
               pl[off + (unsigned)(n.dy[q][2] * pitch + n.dx[q][2])] + pl[off + (unsigned)(n.dy[q][3] * pitch + n.dx[q][3])];
    };
    const int s0 = rs(0), s1 = rs(1);
    if (pair) return (double)((float)s0 * n.w[0] + (float)s1 * n.w[1]);       // SSE2 path of two-rectangle stump stages
    double v = (double)((float)s0 * n.w[0]);
    v += (double)((float)s1 * n.w[1]);
    if ((n.flags & 255) == 3) v += (double)((float)rs(2) * n.w[2]);
    return v;
}
// The weak classifiers of a stage are independent of one another up to their votes: four roots are evaluated per step -- their
// 32 to 48 gathers are in flight together instead of one classifier's at a time -- then each walk is finished and the votes are
// added in stage order (OpenCV's order: the f64 sum is the same).
__device__ __forceinline__ bool gen_stage(const CascadeArgs &a, const int *__restrict__ sum, const int *__restrict__ tilt, unsigned off, int pitch,
                                          double vnf, const GNodeRec *recs, const StageRec &st)
{
    const bool pair = a.pair_policy && a.stump_based && (st.flags & 1);
    double stage_sum = 0.0;
    auto finish = [&](int base, int idx) {                                  // below the root the lanes of a wave part ways
        while (idx > 0) {
            const GNodeRec &n = recs[base + idx];
            const double sn = gen_node_sum((n.flags & 256) ? tilt : sum, off, pitch, n, false);
            idx = sn < (double)n.thr * vnf ? n.left : n.right;
        }
        return (double)a.galpha[-idx];
    };
    int j = 0;
    for (; j + 4 <= st.count; j += 4) {
        int base[4], idx[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            base[u] = a.gcls_first[st.first + j + u];
            CGNodeRec &root = ((CGNodeRec *)recs)[base[u]];
            const double s = gen_node_sum((root.flags & 256) ? tilt : sum, off, pitch, root, pair);
            idx[u] = s < (double)root.thr * vnf ? root.left : root.right;   // node->threshold * variance_norm_factor
        }
#pragma unroll
        for (int u = 0; u < 4; u++) stage_sum += finish(base[u], idx[u]);
    }
    for (; j < st.count; j++) {
        const int base = a.gcls_first[st.first + j];
        CGNodeRec &root = ((CGNodeRec *)recs)[base];
        const double s = gen_node_sum((root.flags & 256) ? tilt : sum, off, pitch, root, pair);
        stage_sum += finish(base, s < (double)root.thr * vnf ? root.left : root.right);
    }
    return !(stage_sum < (double)st.thr);
}

__global__ __launch_bounds__(256) void k_gen_stage0(CascadeArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int slot, bidx;
    if (!xcd_chunk_index((a.ntasks + 3) / 4, slot, bidx)) return;
    const int t = __builtin_amdgcn_readfirstlane(bidx * 4 + wave);
    if (t >= a.ntasks) return;
    const unsigned task = a.tasks[t];
    const int s = task >> 20, iy = (task >> 7) & 8191, k = task & 127;
    const ScaleRec &sc = a.scales[s];
    const int ix = k * 64 + lane;
    const bool active = ix < sc.endX;
    const int *__restrict__ sum = a.sum + (size_t)slot * a.sum_slot + sc.plane_off;
    const int *__restrict__ tilt = a.tilted ? a.tilted + (size_t)slot * a.sum_slot + sc.plane_off : sum;
    const unsigned *__restrict__ sql = (const unsigned *)a.sqsum + (size_t)slot * 2 * a.sum_slot + sc.plane_off;
    const uint8_t *__restrict__ sqh = (const uint8_t *)((const unsigned *)a.sqsum + (size_t)slot * 2 * a.sum_slot + a.sum_slot) + sc.plane_off;
    bool pass0 = false;
    double vnf = 1.;
    if (active) {
        const unsigned off = (unsigned)(a.pos[sc.ypos_off + iy] * sc.pitch + a.pos[sc.xpos_off + ix]);
        const unsigned e0 = off + sc.eq[0], e1 = off + sc.eq[1], e2 = off + sc.eq[2], e3 = off + sc.eq[3];
        const int ws = sum[e0] - sum[e1] - sum[e2] + sum[e3];
        const double mean = (double)ws * sc.inv_area;
        vnf = window_sqsum(sql, sqh, sc.sq32 != 0, e0, e1, e2, e3);
        vnf = vnf * sc.inv_area - mean * mean;
        vnf = vnf >= 0. ? sqrt(vnf) : 1.;
        pass0 = gen_stage(a, sum, tilt, off, sc.pitch, vnf, sc.grecs, a.stages[0]);
    }
    const unsigned long long fb = __ballot(active && !pass0);
    const size_t o = (size_t)slot * a.ntasks + t;
    if (lane == 0) a.failbits[o] = fb;
    a.vnf[o * 64 + lane] = vnf;
}

__global__ __launch_bounds__(256) void k_gen_rest(CascadeArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int slot, bidx;
    if (!xcd_chunk_index((a.ntasks + 3) / 4, slot, bidx)) return;
    const int t = __builtin_amdgcn_readfirstlane(bidx * 4 + wave);
    if (t >= a.ntasks) return;
    const unsigned task = a.tasks[t];
    const int s = task >> 20, iy = (task >> 7) & 8191, k = task & 127;
    const ScaleRec &sc = a.scales[s];
    const int ix = k * 64 + lane;
    const unsigned long long *rb = a.failbits + (size_t)slot * a.ntasks + sc.task_off + (size_t)iy * sc.wpr;
    bool alive = false;
    if (ix < sc.endX && !((rb[k] >> lane) & 1ull)) alive = sc.adaptive ? visited(rb, ix) : true;
    if (!__any(alive)) return;
    const int *__restrict__ sum = a.sum + (size_t)slot * a.sum_slot + sc.plane_off;
    const int *__restrict__ tilt = a.tilted ? a.tilted + (size_t)slot * a.sum_slot + sc.plane_off : sum;
    unsigned off = 0; double vnf = 1.;
    if (alive) {
        off = (unsigned)(a.pos[sc.ypos_off + iy] * sc.pitch + a.pos[sc.xpos_off + ix]);
        vnf = a.vnf[((size_t)slot * a.ntasks + t) * 64 + lane];
    }
    for (int st_i = 1; st_i < a.nstages; st_i++) {           // wave-uniform stage loop: lanes that fell out idle
        if (!__any(alive)) return;
        if (alive) alive = gen_stage(a, sum, tilt, off, sc.pitch, vnf, sc.grecs, a.stages[st_i]);
    }
    const unsigned long long hm = __ballot(alive);
    if (!hm) return;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(a.hits, (unsigned long long)__popcll(hm));
    base = __shfl(base, 0);
    if (alive) {
        const unsigned long long pos = base + __popcll(hm & ((1ull << lane) - 1ull));
        const unsigned key = ((unsigned)s << a.key_ss) | ((unsigned)iy << a.key_sy) | (unsigned)ix;
        if (pos < a.hit_cap) a.hits[1 + pos] = ((unsigned long long)slot << 32) | key;
    }
}

// workgroups per frame of the window-per-lane kernels: four wave tasks each, a multiple of 8 (xcd_chunk_index)
static int task_blocks(const CascadeArgs &a) { return (((a.ntasks + 3) / 4 + 7) / 8) * 8; }

void launch_gen_stage0(hipStream_t st, const CascadeArgs &a, int batch)
{
    if (batch <= 0 || a.ntasks <= 0) return;
    NVCA_LAUNCH(k_gen_stage0, dim3((unsigned)task_blocks(a) * (unsigned)batch), dim3(256), 0, st, a);
}

void launch_gen_rest(hipStream_t st, const CascadeArgs &a, int batch)
{
    if (batch <= 0 || a.ntasks <= 0) return;
    NVCA_LAUNCH(k_gen_rest, dim3((unsigned)task_blocks(a) * (unsigned)batch), dim3(256), 0, st, a);
}

// ---- K5b: stages 1 .. deep_stage-1 on strips ---------------------------------
__global__ __launch_bounds__(256) void k_strip(CascadeArgs a)
{
    __shared__ unsigned short q[2][kStripMaxWin];
    __shared__ double psum[256];
    __shared__ int qn[2];
    __shared__ unsigned gbase_s;

    const int tid = threadIdx.x, lane = tid & 63;
    const int slot = blockIdx.x / a.blocks_per_frame;
    const int sidx = a.order[blockIdx.x - slot * a.blocks_per_frame];
    if (sidx < 0) return;
    const StripRec strip = a.strips[sidx];
    const ScaleRec &sc = a.scales[strip.scale];
    // a strip covers columns [ix0, ix0 + ncols) of nrows scan rows (rows longer than a strip are cut into segments)
    const int endX = strip.ncols, ix0 = strip.ix0, nwin = strip.nrows * endX;
    const int *__restrict__ sum = a.sum + (size_t)slot * a.sum_slot + sc.plane_off;
    CTStumpRec *recs = (CTStumpRec *)sc.trecs;
    const int *__restrict__ xpos = a.pos + sc.xpos_off;
    const int *__restrict__ ypos = a.pos + sc.ypos_off + strip.iy0;
    const unsigned long long *__restrict__ bits = a.failbits + (size_t)slot * a.ntasks + sc.task_off + (size_t)strip.iy0 * sc.wpr;
    const double *__restrict__ vnfp = a.vnf + ((size_t)slot * a.ntasks + sc.task_off + (size_t)strip.iy0 * sc.wpr) * 64;

    if (tid < 2) qn[tid] = 0;
    __syncthreads();

    // adaptive-step reachability + compaction of visited stage-0 survivors
    for (int base = 0; base < nwin; base += 256) {
        const int w = base + tid;
        bool keep = false;
        if (w < nwin) {
            const int r = w / endX, ix = ix0 + (w - r * endX);
            const unsigned long long *rb = bits + (size_t)r * sc.wpr;
            if (!((rb[ix >> 6] >> (ix & 63)) & 1ull)) keep = sc.adaptive ? visited(rb, ix) : true;
        }
        const unsigned long long km = __ballot(keep);
        if (km) {
            int wbase = 0;
            if (lane == 0) wbase = atomicAdd(&qn[0], __popcll(km));
            wbase = __shfl(wbase, 0);
            if (keep) q[0][wbase + __popcll(km & ((1ull << lane) - 1ull))] = (unsigned short)w;
        }
    }

    int cur = 0;
    int last = a.deep_stage < a.nstages ? a.deep_stage : a.nstages;
    for (int s = 1; s < last; s++) {
        __syncthreads();
        const int n = qn[cur];
        if (n == 0) break;
        if (tid == 0) qn[cur ^ 1] = 0;
        __syncthreads();
        const StageRec st = a.stages[s];
        if ((st.flags & 2) && n <= 128) {
            // Few survivors: most lanes would idle while one wave walks the whole stage.  The votes of this stage may be
            // summed in any order (flag bit 1), so spread its stumps over the idle lanes: thread = (window slot i,
            // stump partition p); partition p takes stumps p, p+P, ...; partial sums meet in LDS.
            int lg = 0;
            while ((1 << lg) < n) lg++;
            const int npad = 1 << lg;
            int P = 256 >> lg;
            if (P > st.count) P = st.count;
            const int i = tid & (npad - 1), p = tid >> lg;
            double part = 0.0;
            int w = 0;
            if (i < n && p < P) {
                w = q[cur][i];
                const int r = w / endX, ix = ix0 + (w - r * endX);
                const unsigned off = (unsigned)(ypos[r] * sc.pitch + xpos[ix]);
                const double vnf = vnfp[((size_t)r * sc.wpr + (ix >> 6)) * 64 + (ix & 63)];
                const bool pair = a.pair_policy && (st.flags & 1);
                if (lg >= 6) {               // a wave holds one partition: records stay wave-uniform (scalar loads)
                    const int pu = __builtin_amdgcn_readfirstlane(p);
                    for (int j = pu; j < st.count; j += P)
                        part += pair ? stump_vote<true>(sum, off, sc.pitch, vnf, recs[st.first + j]) : stump_vote<false>(sum, off, sc.pitch, vnf, recs[st.first + j]);
                } else {
                    for (int j = p; j < st.count; j += P)
                        part += pair ? stump_vote<true>(sum, off, sc.pitch, vnf, recs[st.first + j]) : stump_vote<false>(sum, off, sc.pitch, vnf, recs[st.first + j]);
                }
            }
            psum[tid] = part;
            __syncthreads();
            bool pass = false;
            if (tid < n) {
                double tot = 0.0;
                for (int pp = 0; pp < P; pp++) tot += psum[(pp << lg) + tid];
                pass = !(tot < (double)st.thr);
                w = q[cur][tid];
            }
            const unsigned long long pm = __ballot(pass);
            if (pm) {
                int wbase = 0;
                if (lane == 0) wbase = atomicAdd(&qn[cur ^ 1], __popcll(pm));
                wbase = __shfl(wbase, 0);
                if (pass) q[cur ^ 1][wbase + __popcll(pm & ((1ull << lane) - 1ull))] = (unsigned short)w;
            }
        } else
        for (int base = 0; base < n; base += 256) {
            const int i = base + tid;
            bool pass = false; int w = 0;
            if (i < n) {
                w = q[cur][i];
                const int r = w / endX, ix = ix0 + (w - r * endX);
                const unsigned off = (unsigned)(ypos[r] * sc.pitch + xpos[ix]);
                const double vnf = vnfp[((size_t)r * sc.wpr + (ix >> 6)) * 64 + (ix & 63)];
                pass = run_stage(sum, off, sc.pitch, vnf, recs, st, a.pair_policy);
            }
            const unsigned long long pm = __ballot(pass);
            if (pm) {
                int wbase = 0;
                if (lane == 0) wbase = atomicAdd(&qn[cur ^ 1], __popcll(pm));
                wbase = __shfl(wbase, 0);
                if (pass) q[cur ^ 1][wbase + __popcll(pm & ((1ull << lane) - 1ull))] = (unsigned short)w;
            }
        }
        cur ^= 1;
    }
    __syncthreads();
    const int nh = qn[cur];
    if (nh == 0) return;
    // survivors: final candidates if the cascade ends here, otherwise work for k_deep
    unsigned long long *list = last == a.nstages ? a.hits : a.deep;
    const unsigned cap = last == a.nstages ? a.hit_cap : a.deep_cap;
    if (tid == 0) gbase_s = (unsigned)atomicAdd(list, (unsigned long long)nh);
    __syncthreads();
    const unsigned gb = gbase_s;
    for (int i = tid; i < nh; i += 256) {
        const int w = q[cur][i];
        const int r = w / endX, ix = ix0 + (w - r * endX);
        const unsigned key = ((unsigned)strip.scale << a.key_ss) | ((unsigned)(strip.iy0 + r) << a.key_sy) | (unsigned)ix;
        if (gb + i < cap) list[1 + gb + i] = ((unsigned long long)slot << 32) | key;
    }
}

void launch_stage0(hipStream_t st, const CascadeArgs &a, int batch)
{
    if (batch <= 0 || a.ntasks <= 0) return;
    NVCA_LAUNCH(k_stage0, dim3((unsigned)task_blocks(a) * (unsigned)batch), dim3(256), 0, st, a);
}

void launch_strip(hipStream_t st, const CascadeArgs &a, int batch)
{
    if (batch <= 0 || a.ntasks <= 0 || a.blocks_per_frame <= 0) return;
    NVCA_LAUNCH(k_strip, dim3((unsigned)a.blocks_per_frame * (unsigned)batch), dim3(256), 0, st, a);
}

} // namespace nvca
