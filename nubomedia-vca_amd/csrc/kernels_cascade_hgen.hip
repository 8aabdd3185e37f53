// kernels_cascade_hgen.hip -- the evaluator of GENERAL new-format HAAR cascades: tree weak classifiers (predictOrdered<HaarEvaluator>)
// and tilted features (CV_TILTED_PTRS); SURVEY.md A.19.  The three kernels are the general siblings of kernels_cascade_hnew.hip's:
// the same tiles, pass-bit planes (k_lbp_walk runs on them as it is), merged survivor list of img << 32 | key, final append and
// overflow re-run; the window's normaliser is hnew_vnf's, bit for bit.  A window per lane, wave64; node records are wave-uniform
// (scalar loads), the stage loop and the node loop are wave-uniform.
//
// The tree walk is a forward sweep: the loader guarantees that a child node lies behind its parent, so a lane's walk visits nodes in
// rising index order.  The root is evaluated by every live lane; node j > root only when the ballot finds a live lane standing at it
// (`cur == j`), by those lanes alone, from a scalar-loaded record.  A lane whose child is a leaf adds that leaf -- the node record
// carries it (lv[]) -- and stands at -1 for the rest of the tree: each lane adds exactly one leaf a tree, the trees in file order.  A
// stump is the root alone: what kernels_cascade_hnew.hip does a stump, with one compare on the child more.  No private array is indexed.
//
// Tilted corners are read from the level's tilted plane in global memory in every kernel, stage 0 included (the sum tile in LDS serves the
// upright features and the normaliser): a wave reads them at one plane offset a lane step apart, the L1 / L2 traffic of the gather form.
//
// Arithmetic (compiled with -ffp-contract=off): rect sums int32, upright or tilted; the feature value f32, one rounding per product and
// per addition, the file's weights as they stand (no halving of a tilted weight: that is the old format's); f64 for vnf,
// value = (double)ret * vnf, its compare with the threshold, and the stage sum.
#include "hnew_device.h"

namespace nvca {

__device__ __forceinline__ float hgen_feature(const int *__restrict__ p, const int *off, const float *w)
{
    float ret = w[0] * (float)hnew_rect(p, off) + w[1] * (float)hnew_rect(p, off + 4);
    if (w[2] != 0.f) ret += w[2] * (float)hnew_rect(p, off + 8);          // (wave-uniform)
    return ret;
}

// a stage's sum on the window whose origin p (the sum plane, or the stage-0 tile: TILE) and pt (the tilted plane) point at: the f64 sum of
// the leaves its trees end in, in file order.  Called by whole waves; a lane that is not `alive` evaluates nothing and returns 0.
template <bool TILE>
__device__ __forceinline__ double hgen_stage_sum(const int *__restrict__ p, const int *__restrict__ pt, const HgenArgs &g, const LbpStageDev st,
                                                 double vnf, bool alive)
{
    double sum = 0.;
    for (int k = 0; k < st.count; k++) {
        const HgenWeakDev W = g.weak[st.first + k];
        int cur = W.first;          // the node this lane's window stands at; -1: it has left the tree by a leaf
        for (int j = W.first; j < W.first + W.count; j++) {
            const bool here = alive && cur == j;
            if (j > W.first && !__ballot(here)) continue;          // (the root is every live lane's: no ballot a stump)
            if (here) {
                const HgenNodeDev &n = g.nodes[j];
                float ret;
                if (n.tilted) ret = hgen_feature(pt, n.off, n.w);          // (wave-uniform)
                else ret = hgen_feature(p, TILE ? n.offt : n.off, n.w);
                const bool lt = (double)ret * vnf < (double)n.thr;         // a tie goes right
                cur = lt ? n.left : n.right;
                if (cur < 0) sum += (double)(lt ? n.lv[0] : n.lv[1]);
            }
        }
    }
    return sum;
}

// what a survivor-list entry names, checked against the job and the grids before it indexes the planes; off: its window's origin in
// an image's planes, from the first image's first level
struct HgenWin { bool ok; unsigned img; int lv; size_t origin, off; };
__device__ __forceinline__ HgenWin hgen_entry(const LbpArgs &a, unsigned long long e)
{
    HgenWin w; w.ok = false; w.img = (unsigned)(e >> 32); w.lv = 0; w.origin = 0; w.off = 0;
    const unsigned key = (unsigned)e;
    const unsigned lv = key >> a.key_ss, gy = (key >> a.key_sy) & ((1u << (a.key_ss - a.key_sy)) - 1u), gx = key & ((1u << a.key_sy) - 1u);
    if (w.img < (unsigned)a.nimg && lv < (unsigned)a.nlev) {
        const LbpLevelDev &L = a.levels[lv];
        if (gx < (unsigned)L.nx && gy < (unsigned)L.ny) {
            w.ok = true; w.lv = (int)lv;
            w.origin = (size_t)(gy * L.step) * a.P + gx * L.step;
            w.off = (size_t)w.img * a.plane_total + L.plane_off + w.origin;
        }
    }
    return w;
}
__device__ __forceinline__ double hgen_entry_vnf(const HnewArgs &h, const HgenWin &w)
{
    const LbpArgs &a = h.l;
    const int plane_off = a.levels[w.lv].plane_off;
    const unsigned *lo = h.sq + (size_t)w.img * 2 * a.plane_total + plane_off + w.origin;
    const uint8_t *hi = (const uint8_t *)(h.sq + (size_t)w.img * 2 * a.plane_total + a.plane_total) + (size_t)h.hi_mul * plane_off + w.origin;
    return hnew_vnf(hnew_rect(a.sum + w.off, h.nr), lo, hi, h.nr, h.area);
}

template <bool LDS>
__global__ __launch_bounds__(kLbpTileW * kLbpTileH) void k_hgen_stage0(HgenArgs g)
{
    extern __shared__ int hgen_tile[];
    const HnewArgs &h = g.h;
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
    const size_t origin = active ? (size_t)(gy * L.step) * a.P + gx * L.step : 0;          // (an idle lane: the level's first window)
    const int *__restrict__ pt = (g.tilted ? g.tilted : a.sum) + (size_t)img * a.plane_total + L.plane_off + origin;
    const int *p;
    const int *nr;
    if (LDS) {
        // the tile of k_hnew_stage0: columns X0 .. X0 + 31 step + ow, rows Y0 .. Y0 + 15 step + oh of the (szw + 1) x (szh + 1) plane, zeros outside
        const int tw = (kLbpTileW - 1) * L.step + a.ow + 1, th = lbp_tile_rows(a.oh, L.step);
        for (int i = tid; i < tw * th; i += kLbpTileW * kLbpTileH) {
            const int r = i / tw, c = i - r * tw;
            hgen_tile[r * a.TP + c] = (Y0 + r <= L.szh && X0 + c <= L.szw) ? plane[(size_t)(Y0 + r) * a.P + X0 + c] : 0;
        }
        __syncthreads();
        p = hgen_tile + ly * L.step * a.TP + lx * L.step; nr = h.nrt;
    } else {
        p = plane + origin; nr = h.nr;
    }
    double vnf = 1.;
    if (active) {         // Q is read at the window's own place in the plane: an idle lane has none
        const unsigned *lo = h.sq + (size_t)img * 2 * a.plane_total + L.plane_off + origin;
        const uint8_t *hi = (const uint8_t *)(h.sq + (size_t)img * 2 * a.plane_total + a.plane_total) + (size_t)h.hi_mul * L.plane_off + origin;
        vnf = hnew_vnf(hnew_rect(p, nr), lo, hi, h.nr, h.area);
    }
    const LbpStageDev st0 = a.stages[0];
    const bool pass0 = active && !(hgen_stage_sum<LDS>(p, pt, g, st0, vnf, active) < (double)st0.thr);
    bool alive = pass0;
    for (int s = 1; s < a.tile_stages; s++) {          // (wave-uniform: a wave leaves when none of its windows is left)
        if (!__ballot(alive)) break;
        const LbpStageDev st = a.stages[s];
        alive = !(hgen_stage_sum<LDS>(p, pt, g, st, vnf, alive) < (double)st.thr) && alive;
    }
    // lanes 0 .. 31: row gy of the even lane rows, 32 .. 63: the row below
    const unsigned long long m0 = __ballot(pass0), m1 = __ballot(alive);
    if (lx == 0 && gy < L.ny) {
        const size_t w = (size_t)img * a.bit_words + L.bit_off + (size_t)gy * L.wpr + t.tx;
        a.bits[w] = (unsigned)(m0 >> (tid & 32));
        a.bits2[w] = (unsigned)(m1 >> (tid & 32));
    }
}

__global__ __launch_bounds__(256) void k_hgen_rest(HgenArgs g, int s0, int s1, int in, int in_cnt)
{
    const HnewArgs &h = g.h;
    const LbpArgs &a = h.l;
    unsigned n = a.cnt[in_cnt];
    if (n > a.list_cap) n = a.list_cap;
    const unsigned long long *__restrict__ src = in ? a.list[1] : a.list[0];
    unsigned long long *__restrict__ dst = in ? a.list[0] : a.list[1];
    const int *__restrict__ tbase = g.tilted ? g.tilted : a.sum;
    const bool final = s1 >= a.nstages;
    const int lane = threadIdx.x & 63;
    for (unsigned i0 = blockIdx.x * 256u; i0 < n; i0 += gridDim.x * 256u) {          // (uniform per workgroup: the ballots below see whole waves)
        const unsigned i = i0 + threadIdx.x;
        bool alive = i < n;
        unsigned long long e = 0; size_t off = 0;          // (a lane without a window points at the first image's first window: it reads nothing)
        double vnf = 1.;
        if (alive) {
            e = src[i];
            const HgenWin w = hgen_entry(a, e);
            alive = w.ok;
            if (alive) { off = w.off; vnf = hgen_entry_vnf(h, w); }
        }
        for (int s = s0; s < s1 && s < a.nstages; s++) {
            if (!__ballot(alive)) break;
            const LbpStageDev st = a.stages[s];
            alive = !(hgen_stage_sum<false>(a.sum + off, tbase + off, g, st, vnf, alive) < (double)st.thr) && alive;
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

// detectMultiScale with outputRejectLevels: k_hnew_levels with this evaluator
__global__ __launch_bounds__(256) void k_hgen_levels(HgenArgs g, LevelRec *__restrict__ recs, int in, int in_cnt)
{
    const HnewArgs &h = g.h;
    const LbpArgs &a = h.l;
    unsigned n = a.cnt[in_cnt];
    if (n > a.list_cap) n = a.list_cap;
    const unsigned long long *__restrict__ src = in ? a.list[1] : a.list[0];
    const int *__restrict__ tbase = g.tilted ? g.tilted : a.sum;
    const int lane = threadIdx.x & 63;
    const int s0 = a.nstages - 3;
    if (s0 < 1) return;          // (a levels job has four stages at least)
    for (unsigned i0 = blockIdx.x * 256u; i0 < n; i0 += gridDim.x * 256u) {          // (uniform per workgroup: the ballots below see whole waves)
        const unsigned i = i0 + threadIdx.x;
        bool listed = i < n;
        unsigned long long e = 0; size_t off = 0;
        double vnf = 1.;
        if (listed) {
            e = src[i];
            const HgenWin w = hgen_entry(a, e);
            listed = w.ok;
            if (listed) { off = w.off; vnf = hgen_entry_vnf(h, w); }
        }
        bool alive = listed;
        int level = s0; double sum = 0.;
        for (int s = s0; s < a.nstages; s++) {
            if (!__ballot(alive)) break;
            const LbpStageDev st = a.stages[s];
            const double v = hgen_stage_sum<false>(a.sum + off, tbase + off, g, st, vnf, alive);
            if (alive) {
                sum = v;
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

void launch_hgen_levels(hipStream_t st, const HgenArgs &g, LevelRec *recs, int in, int in_cnt, unsigned max_items)
{
    if (max_items == 0 || g.h.l.nstages < 4 || !recs) return;
    unsigned blocks = (max_items + 255u) / 256u;
    if (blocks > 4096u) blocks = 4096u;
    NVCA_LAUNCH(k_hgen_levels, dim3(blocks), dim3(256), 0, st, g, recs, in, in_cnt);
}

void launch_hgen_stage0(hipStream_t st, const HgenArgs &g, int lds)
{
    if (g.h.l.ntiles <= 0 || g.h.l.nimg <= 0) return;
    const dim3 grid((unsigned)g.h.l.ntiles, (unsigned)g.h.l.nimg);
    if (lds > 0) NVCA_LAUNCH(k_hgen_stage0<true>, grid, dim3(kLbpTileW * kLbpTileH), (size_t)lds, st, g);
    else NVCA_LAUNCH(k_hgen_stage0<false>, grid, dim3(kLbpTileW * kLbpTileH), 0, st, g);
}

void launch_hgen_rest(hipStream_t st, const HgenArgs &g, int s0, int s1, int in, int in_cnt, unsigned max_items)
{
    if (max_items == 0 || s0 >= g.h.l.nstages) return;
    unsigned blocks = (max_items + 255u) / 256u;
    if (blocks > 4096u) blocks = 4096u;
    NVCA_LAUNCH(k_hgen_rest, dim3(blocks), dim3(256), 0, st, g, s0, s1, in, in_cnt);
}

} // namespace nvca
