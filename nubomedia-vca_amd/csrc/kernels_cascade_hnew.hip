// kernels_cascade_hnew.hip -- the evaluator of new-format HAAR cascades: OpenCV 2.4 cascadedetect.cpp, CascadeClassifierInvoker over
// HaarEvaluator / predictOrderedStump.  The scan is the LBP evaluator's (kernels_cascade_lbp.hip: levels, tiles, the
// two pass-bit planes, k_lbp_walk on them, one merged survivor list of img << 32 | key, the candidate list); what differs is the weak
// classifier -- a stump on a Haar feature at window scale 1 -- and the window's variance normaliser.  A window per lane, wave64; the
// weak records are wave-uniform (scalar loads), the stage loop is wave-uniform.
//
//   k_hnew_stage0   the first stages (LbpArgs::tile_stages) at EVERY grid position, 32 x 16 positions per workgroup, the level's sum tile
//                   in LDS as k_lbp_stage0 stages it; a lane computes its window's vnf once -- the four corners of S from the tile, the
//                   four of Q (low-word and high-byte plane) from global memory: read once a window, they do not earn LDS
//   k_hnew_rest     stages [s0, s1) on the survivor list, compaction and final append as k_lbp_rest's; a survivor's vnf is RECOMPUTED
//                   from its eight corners by the same function, so it has the same bits by construction and no side array has to
//                   stay aligned with the compacted lists
//   k_hnew_levels   outputRejectLevels: the last three stages on the survivors in front of them; every one of those
//                   windows is appended to the candidate list with the stage that rejected it and that stage's sum
//
// Arithmetic (this file is compiled with -ffp-contract=off): rect sums int32; the feature value f32, one rounding per product and per
// addition; f64 for vnf (exact integer operands, one multiply-subtract pair, a correctly rounded sqrt and division), for the product
// value = (double)ret * vnf, its compare with the threshold, and the stage sum.
#include "hnew_device.h"

namespace nvca {

// a stage's sum on the window at p: the f64 sum of the stumps' leaves in file order
__device__ __forceinline__ double hnew_stage_sum(const int *__restrict__ p, const HnewWeakDev *__restrict__ weak, const LbpStageDev st, double vnf)
{
    double sum = 0.;
#pragma unroll 2          // the corner loads of two weak classifiers in flight at a time; the leaves are still added one by one, in file order
    for (int k = 0; k < st.count; k++) {
        const HnewWeakDev &w = weak[st.first + k];
        float ret = w.w[0] * (float)hnew_rect(p, w.off) + w.w[1] * (float)hnew_rect(p, w.off + 4);
        if (w.w[2] != 0.f) ret += w.w[2] * (float)hnew_rect(p, w.off + 8);          // (wave-uniform)
        sum += (double)((double)ret * vnf < (double)w.thr ? w.leaf[0] : w.leaf[1]);
    }
    return sum;
}
// a stage on the window at p; false: sum < thr, the window is rejected
__device__ __forceinline__ bool hnew_stage(const int *__restrict__ p, const HnewWeakDev *__restrict__ weak, const LbpStageDev st, double vnf)
{
    return !(hnew_stage_sum(p, weak, st, vnf) < (double)st.thr);
}

template <bool LDS>
__global__ __launch_bounds__(kLbpTileW * kLbpTileH) void k_hnew_stage0(HnewArgs h)
{
    extern __shared__ int hnew_tile[];
    const LbpArgs &a = h.l;
    const LbpTile t = a.tiles[blockIdx.x];
    const unsigned img = blockIdx.y;          // (the grid is ntiles x nimg)
    if ((unsigned)t.level >= (unsigned)a.nlev || img >= (unsigned)a.nimg) return;
    const LbpLevelDev L = a.levels[t.level];
    const int tid = threadIdx.x, lx = tid & (kLbpTileW - 1), ly = tid / kLbpTileW;
    const int gx = t.tx * kLbpTileW + lx, gy = t.ty * kLbpTileH + ly;
    const int X0 = t.tx * kLbpTileW * L.step, Y0 = t.ty * kLbpTileH * L.step;
    const bool active = gx < L.nx && gy < L.ny;
    const int *__restrict__ plane = a.sum + (size_t)img * a.plane_total + L.plane_off;
    const size_t origin = active ? (size_t)(gy * L.step) * a.P + gx * L.step : 0;
    const int *p;
    const HnewWeakDev *weak;
    const int *nr;
    if (LDS) {
        // the tile of k_lbp_stage0: columns X0 .. X0 + 31 step + ow, rows Y0 .. Y0 + 15 step + oh of the (szw + 1) x (szh + 1) plane, zeros outside
        const int tw = (kLbpTileW - 1) * L.step + a.ow + 1, th = lbp_tile_rows(a.oh, L.step);
        for (int i = tid; i < tw * th; i += kLbpTileW * kLbpTileH) {
            const int r = i / tw, c = i - r * tw;
            hnew_tile[r * a.TP + c] = (Y0 + r <= L.szh && X0 + c <= L.szw) ? plane[(size_t)(Y0 + r) * a.P + X0 + c] : 0;
        }
        __syncthreads();
        p = hnew_tile + ly * L.step * a.TP + lx * L.step; weak = h.tweak; nr = h.nrt;        // (an idle lane's window lies inside the tile as well)
    } else {
        p = plane + origin; weak = h.gweak; nr = h.nr;
    }
    double vnf = 1.;
    if (active) {         // Q is read at the window's own place in the plane: an idle lane has none
        const unsigned *lo = h.sq + (size_t)img * 2 * a.plane_total + L.plane_off + origin;
        const uint8_t *hi = (const uint8_t *)(h.sq + (size_t)img * 2 * a.plane_total + a.plane_total) + (size_t)h.hi_mul * L.plane_off + origin;
        vnf = hnew_vnf(hnew_rect(p, nr), lo, hi, h.nr, h.area);
    }
    const bool pass0 = hnew_stage(p, weak, a.stages[0], vnf) && active;
    bool alive = pass0;
    for (int s = 1; s < a.tile_stages; s++) {          // (wave-uniform: a wave leaves when none of its windows is left)
        if (!__ballot(alive)) break;
        if (alive) alive = hnew_stage(p, weak, a.stages[s], vnf);
    }
    // lanes 0 .. 31: row gy of the even lane rows, 32 .. 63: the row below
    const unsigned long long m0 = __ballot(pass0), m1 = __ballot(alive);
    if (lx == 0 && gy < L.ny) {
        const size_t w = (size_t)img * a.bit_words + L.bit_off + (size_t)gy * L.wpr + t.tx;
        a.bits[w] = (unsigned)(m0 >> (tid & 32));
        a.bits2[w] = (unsigned)(m1 >> (tid & 32));
    }
}

__global__ __launch_bounds__(256) void k_hnew_rest(HnewArgs h, int s0, int s1, int in, int in_cnt)
{
    const LbpArgs &a = h.l;
    unsigned n = a.cnt[in_cnt];
    if (n > a.list_cap) n = a.list_cap;
    const unsigned long long *__restrict__ src = in ? a.list[1] : a.list[0];
    unsigned long long *__restrict__ dst = in ? a.list[0] : a.list[1];
    const bool final = s1 >= a.nstages;
    const int lane = threadIdx.x & 63;
    for (unsigned i0 = blockIdx.x * 256u; i0 < n; i0 += gridDim.x * 256u) {          // (uniform per workgroup: the ballots below see whole waves)
        const unsigned i = i0 + threadIdx.x;
        bool alive = i < n;
        unsigned long long e = 0; size_t off = 0;
        double vnf = 1.;
        if (alive) {
            // an entry comes from device memory: its image and its key are checked against the job and the grids before they index the planes
            e = src[i];
            const unsigned img = (unsigned)(e >> 32), key = (unsigned)e;
            const unsigned lv = key >> a.key_ss, gy = (key >> a.key_sy) & ((1u << (a.key_ss - a.key_sy)) - 1u), gx = key & ((1u << a.key_sy) - 1u);
            alive = img < (unsigned)a.nimg && lv < (unsigned)a.nlev;
            if (alive) {
                const LbpLevelDev &L = a.levels[lv];
                alive = gx < (unsigned)L.nx && gy < (unsigned)L.ny;
                if (alive) {
                    const size_t origin = (size_t)(gy * L.step) * a.P + gx * L.step;
                    off = (size_t)img * a.plane_total + L.plane_off + origin;
                    const unsigned *lo = h.sq + (size_t)img * 2 * a.plane_total + L.plane_off + origin;
                    const uint8_t *hi = (const uint8_t *)(h.sq + (size_t)img * 2 * a.plane_total + a.plane_total) + (size_t)h.hi_mul * L.plane_off + origin;
                    vnf = hnew_vnf(hnew_rect(a.sum + off, h.nr), lo, hi, h.nr, h.area);
                }
            }
        }
        for (int s = s0; s < s1 && s < a.nstages; s++) {
            if (!__ballot(alive)) break;
            if (alive) alive = hnew_stage(a.sum + off, h.gweak, a.stages[s], vnf);
        }
        const unsigned long long m = __ballot(alive);
        if (!m) continue;
        const int cntm = __popcll(m), rank = __popcll(m & ((1ull << lane) - 1ull));
        if (final) {
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(a.hits, (unsigned long long)cntm);
            base = __shfl(base, 0);
            if (alive && base + rank < a.hit_cap) a.hits[1 + base + rank] = e;
        } else {
            unsigned base = 0;
            if (lane == 0) base = atomicAdd(a.cnt + in_cnt + 1, (unsigned)cntm);
            base = __shfl(base, 0);
            if (alive && base + rank < a.list_cap) dst[base + rank] = e;
        }
    }
}

// detectMultiScale with outputRejectLevels: k_lbp_levels with this evaluator -- the last three stages on the survivor
// list in front of stage nstages - 3, a survivor's vnf recomputed by hnew_vnf as k_hnew_rest does; every listed window is appended to the
// candidate list with the stage that rejected it (nstages: none did) and that stage's f64 sum in the LevelRec under the same index.
__global__ __launch_bounds__(256) void k_hnew_levels(HnewArgs h, LevelRec *__restrict__ recs, int in, int in_cnt)
{
    const LbpArgs &a = h.l;
    unsigned n = a.cnt[in_cnt];
    if (n > a.list_cap) n = a.list_cap;
    const unsigned long long *__restrict__ src = in ? a.list[1] : a.list[0];
    const int lane = threadIdx.x & 63;
    const int s0 = a.nstages - 3;
    if (s0 < 1) return;          // (a levels job has four stages at least)
    for (unsigned i0 = blockIdx.x * 256u; i0 < n; i0 += gridDim.x * 256u) {          // (uniform per workgroup: the ballots below see whole waves)
        const unsigned i = i0 + threadIdx.x;
        bool listed = i < n;
        unsigned long long e = 0; size_t off = 0;
        double vnf = 1.;
        if (listed) {
            // an entry comes from device memory: its image and its key are checked against the job and the grids before they index the planes
            e = src[i];
            const unsigned img = (unsigned)(e >> 32), key = (unsigned)e;
            const unsigned lv = key >> a.key_ss, gy = (key >> a.key_sy) & ((1u << (a.key_ss - a.key_sy)) - 1u), gx = key & ((1u << a.key_sy) - 1u);
            listed = img < (unsigned)a.nimg && lv < (unsigned)a.nlev;
            if (listed) {
                const LbpLevelDev &L = a.levels[lv];
                listed = gx < (unsigned)L.nx && gy < (unsigned)L.ny;
                if (listed) {
                    const size_t origin = (size_t)(gy * L.step) * a.P + gx * L.step;
                    off = (size_t)img * a.plane_total + L.plane_off + origin;
                    const unsigned *lo = h.sq + (size_t)img * 2 * a.plane_total + L.plane_off + origin;
                    const uint8_t *hi = (const uint8_t *)(h.sq + (size_t)img * 2 * a.plane_total + a.plane_total) + (size_t)h.hi_mul * L.plane_off + origin;
                    vnf = hnew_vnf(hnew_rect(a.sum + off, h.nr), lo, hi, h.nr, h.area);
                }
            }
        }
        bool alive = listed;
        int level = s0; double sum = 0.;
        for (int s = s0; s < a.nstages; s++) {
            if (!__ballot(alive)) break;
            if (alive) {
                const LbpStageDev st = a.stages[s];
                sum = hnew_stage_sum(a.sum + off, h.gweak, st, vnf);
                alive = !(sum < (double)st.thr);
                level = alive ? s + 1 : s;
            }
        }
        const unsigned long long m = __ballot(listed);
        if (!m) continue;
        const int cntm = __popcll(m), rank = __popcll(m & ((1ull << lane) - 1ull));
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(a.hits, (unsigned long long)cntm);
        base = __shfl(base, 0);
        if (listed && base + rank < a.hit_cap) {
            a.hits[1 + base + rank] = e;
            LevelRec r; r.level = level; r.pad = 0; r.weight = sum;
            recs[base + rank] = r;
        }
    }
}

void launch_hnew_levels(hipStream_t st, const HnewArgs &a, LevelRec *recs, int in, int in_cnt, unsigned max_items)
{
    if (max_items == 0 || a.l.nstages < 4 || !recs) return;
    unsigned blocks = (max_items + 255u) / 256u;
    if (blocks > 4096u) blocks = 4096u;
    NVCA_LAUNCH(k_hnew_levels, dim3(blocks), dim3(256), 0, st, a, recs, in, in_cnt);
}

void launch_hnew_stage0(hipStream_t st, const HnewArgs &a, int lds)
{
    if (a.l.ntiles <= 0 || a.l.nimg <= 0) return;
    const dim3 grid((unsigned)a.l.ntiles, (unsigned)a.l.nimg);
    if (lds > 0) NVCA_LAUNCH(k_hnew_stage0<true>, grid, dim3(kLbpTileW * kLbpTileH), (size_t)lds, st, a);
    else NVCA_LAUNCH(k_hnew_stage0<false>, grid, dim3(kLbpTileW * kLbpTileH), 0, st, a);
}

void launch_hnew_rest(hipStream_t st, const HnewArgs &a, int s0, int s1, int in, int in_cnt, unsigned max_items)
{
    if (max_items == 0 || s0 >= a.l.nstages) return;
    unsigned blocks = (max_items + 255u) / 256u;
    if (blocks > 4096u) blocks = 4096u;
    NVCA_LAUNCH(k_hnew_rest, dim3(blocks), dim3(256), 0, st, a, s0, s1, in, in_cnt);
}

} // namespace nvca
