// kernels_cascade_lbp.hip -- the evaluator of new-format LBP cascades: OpenCV 2.4 cascadedetect.cpp, CascadeClassifierInvoker over
// LBPEvaluator / predictCategoricalStump.  A window per lane, wave64; the weak-classifier records are
// wave-uniform (scalar loads), the stage loop is wave-uniform.
//
//   k_lbp_stage0   the first stages (LbpArgs::tile_stages, at most 3) at EVERY grid position of every level, 32 x 16 positions per
//                  workgroup, corners read from a tile of the level's sum plane staged in LDS; leaves two bits per position: passed
//                  stage 0 (what the skip rule depends on), passed all of the tile's stages
//   k_lbp_walk     a thread per scan row (of every image) replays the serial walk's skip rule on the stage-0 bits (a stage-0 reject skips the next grid
//                  column: visited[i] = visited[i-1] & pass[i-1] | visited[i-2] & !pass[i-2]) and lists the VISITED survivors of the
//                  tile's stages -- a skipped column may have been evaluated there, it is never listed and so never emitted
//   k_lbp_rest     stages [s0, s1) on a list of survivors, corners gathered from the plane; the survivors are compacted into the next
//                  list (the host launches one per stage group), the last group appends to the candidate list
//   k_lbp_levels   outputRejectLevels: the last three stages on the survivors in front of them; every one of those windows
//                  is appended to the candidate list with the stage that rejected it and that stage's sum
//
// A job's images (LbpArgs::nimg, one geometry) share every launch: stage 0 has the image in grid.y, the walk a lane per (image, scan
// row), and from there on ONE survivor list holds every image's windows as img << 32 | key -- a stage group runs once on all of them,
// so its launch count does not depend on the number of images and its late, thin groups see nimg times the windows.  Image b's sum
// planes lie at sum + b * plane_total, its pass bits at bits + b * bit_words.
//
// The subset word of a vote is picked per lane by code >> 5 from eight words held in scalar registers: with seven compares and
// selects -- indexing scalar registers by a vector value would make the compiler wrap the read in a waterfall loop, and an LDS copy
// of the subsets would bound the cascade's length by the LDS left beside the tile.
#include "launch.h"

namespace nvca {

// the LBP code of the window at `p` (its origin in the plane or in the tile; w.off at that array's pitch)
__device__ __forceinline__ int lbp_code(const int *__restrict__ p, const LbpWeakDev &w)
{
    int v[16];
#pragma unroll
    for (int k = 0; k < 16; k++) v[k] = p[w.off[k]];
    auto cell = [&](int r, int c) { return v[r * 4 + c] - v[r * 4 + c + 1] - v[r * 4 + 4 + c] + v[r * 4 + 5 + c]; };
    const int ctr = cell(1, 1);
    return (cell(0, 0) >= ctr ? 128 : 0) | (cell(0, 1) >= ctr ? 64 : 0) | (cell(0, 2) >= ctr ? 32 : 0) | (cell(1, 2) >= ctr ? 16 : 0) |
           (cell(2, 2) >= ctr ? 8 : 0) | (cell(2, 1) >= ctr ? 4 : 0) | (cell(2, 0) >= ctr ? 2 : 0) | (cell(1, 0) >= ctr ? 1 : 0);
}

// predictCategoricalStump's vote: one of the two leaves
__device__ __forceinline__ float lbp_vote(int code, const LbpWeakDev &w)
{
    const int i = code >> 5;
    int word = w.subset[0];
    word = i == 1 ? w.subset[1] : word; word = i == 2 ? w.subset[2] : word; word = i == 3 ? w.subset[3] : word;
    word = i == 4 ? w.subset[4] : word; word = i == 5 ? w.subset[5] : word; word = i == 6 ? w.subset[6] : word;
    word = i == 7 ? w.subset[7] : word;
    return ((unsigned)word >> (code & 31)) & 1u ? w.leaf[0] : w.leaf[1];
}

// a stage's sum on the window at p: the f32 sum of the votes in file order, one rounding per addition (this file is compiled with
// -ffp-contract=off)
__device__ __forceinline__ float lbp_stage_sum(const int *__restrict__ p, const LbpWeakDev *__restrict__ weak, const LbpStageDev st)
{
    float tmp = 0.f;
#pragma unroll 2          // the corner loads of two weak classifiers in flight at a time; the votes are still added one by one, in file order
    for (int k = 0; k < st.count; k++) {
        const LbpWeakDev &w = weak[st.first + k];
        tmp += lbp_vote(lbp_code(p, w), w);
    }
    return tmp;
}
// a stage on the window at p; false: tmp < thr, the window is rejected
__device__ __forceinline__ bool lbp_stage(const int *__restrict__ p, const LbpWeakDev *__restrict__ weak, const LbpStageDev st)
{
    return !(lbp_stage_sum(p, weak, st) < st.thr);
}

template <bool LDS>
__global__ __launch_bounds__(kLbpTileW * kLbpTileH) void k_lbp_stage0(LbpArgs a)
{
    extern __shared__ int lbp_tile[];
    const LbpTile t = a.tiles[blockIdx.x];
    const unsigned img = blockIdx.y;          // (the grid is ntiles x nimg; tiles, levels and weak classifiers are every image's)
    if ((unsigned)t.level >= (unsigned)a.nlev || img >= (unsigned)a.nimg) return;
    const LbpLevelDev L = a.levels[t.level];
    const int tid = threadIdx.x, lx = tid & (kLbpTileW - 1), ly = tid / kLbpTileW;
    const int gx = t.tx * kLbpTileW + lx, gy = t.ty * kLbpTileH + ly;
    const int X0 = t.tx * kLbpTileW * L.step, Y0 = t.ty * kLbpTileH * L.step;
    const bool active = gx < L.nx && gy < L.ny;
    const int *__restrict__ plane = a.sum + (size_t)img * a.plane_total + L.plane_off;
    const int *p;
    const LbpWeakDev *weak;
    if (LDS) {
        // every corner the tile's windows read: columns X0 .. X0 + 31 step + ow, rows Y0 .. Y0 + 15 step + oh of the (szw + 1) x (szh + 1) plane
        const int tw = (kLbpTileW - 1) * L.step + a.ow + 1, th = lbp_tile_rows(a.oh, L.step);
        for (int i = tid; i < tw * th; i += kLbpTileW * kLbpTileH) {
            const int r = i / tw, c = i - r * tw;
            lbp_tile[r * a.TP + c] = (Y0 + r <= L.szh && X0 + c <= L.szw) ? plane[(size_t)(Y0 + r) * a.P + X0 + c] : 0;
        }
        __syncthreads();
        p = lbp_tile + ly * L.step * a.TP + lx * L.step; weak = a.tweak;        // (an idle lane's window lies inside the tile as well)
    } else {
        p = plane + (active ? (size_t)(gy * L.step) * a.P + gx * L.step : 0); weak = a.gweak;
    }
    const bool pass0 = lbp_stage(p, weak, a.stages[0]) && active;
    bool alive = pass0;
    for (int s = 1; s < a.tile_stages; s++) {          // (wave-uniform: a wave leaves when none of its windows is left)
        if (!__ballot(alive)) break;
        if (alive) alive = lbp_stage(p, weak, a.stages[s]);
    }
    // lanes 0 .. 31: row gy of the even lane rows, 32 .. 63: the row below
    const unsigned long long m0 = __ballot(pass0), m1 = __ballot(alive);
    if (lx == 0 && gy < L.ny) {
        const size_t w = (size_t)img * a.bit_words + L.bit_off + (size_t)gy * L.wpr + t.tx;
        a.bits[w] = (unsigned)(m0 >> (tid & 32));
        a.bits2[w] = (unsigned)(m1 >> (tid & 32));
    }
}

// The serial walk of a row (CascadeClassifierInvoker: "if result == 0, x += yStep") over the row's stage-0 bits, eight grid columns
// a step: the walk is a two-state machine (the next column is jumped over or not), so a table gives, per state and byte of pass
// bits, the columns visited and the state behind them.
__global__ __launch_bounds__(64) void k_lbp_walk(LbpArgs a)
{
    __shared__ unsigned short lut[512];           // [state << 8 | pass bits] -> visited bits | state behind << 8
    for (int e = threadIdx.x; e < 512; e += 64) {
        bool skip = e >> 8;
        unsigned vis = 0;
        for (int b = 0; b < 8; b++) {
            if (!skip) { vis |= 1u << b; skip = !((e >> b) & 1); }
            else skip = false;
        }
        lut[e] = (unsigned short)(vis | (skip ? 256u : 0u));
    }
    __syncthreads();
    // a lane per (image, row) -- image-major, so a wave may span two images; the lanes of the wave step through their rows' words
    // together, so that the wave appends what its 64 rows found in a word with ONE atomic (a lane whose row has ended, or that has
    // no row, takes part with nothing)
    const int pair = blockIdx.x * 64 + threadIdx.x, lane = threadIdx.x;
    int lv = 0, gy = -1, wpr = 0, img = 0;
    const unsigned *rb = nullptr, *rb2 = nullptr;
    if (pair < a.nrows * a.nimg) {
        img = pair / a.nrows;
        const int row = pair - img * a.nrows;
        while (lv + 1 < a.nlev && row >= a.levels[lv + 1].row_first) lv++;
        const LbpLevelDev &L = a.levels[lv];
        gy = row - L.row_first;
        if (gy >= 0 && gy < L.ny) {
            const size_t w = (size_t)img * a.bit_words + L.bit_off + (size_t)gy * L.wpr;
            wpr = L.wpr; rb = a.bits + w; rb2 = a.bits2 + w;
        }
    }
    const unsigned long long slot = (unsigned long long)(unsigned)img << 32;
    const bool final = a.nstages <= a.tile_stages;
    unsigned state = 0;                  // 256: the next column is jumped over (the one before it was visited and failed stage 0); every row of every image starts at 0
    for (int k = 0; __ballot(k < wpr); k++) {
        unsigned surv = 0;
        if (k < wpr) {
            const unsigned p = rb[k];
            unsigned vis = 0;
            for (int b = 0; b < 32; b += 8) {
                const unsigned e = lut[state | ((p >> b) & 255u)];
                vis |= (e & 255u) << b; state = e & 256u;
            }
            surv = vis & rb2[k];          // (bits behind the row's end are zero)
        }
        const int n = __popc(surv);
        int incl = n;                     // inclusive prefix sum of n over the wave's lanes
        for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(incl, d); if (lane >= d) incl += v; }
        const int total = __shfl(incl, 63);
        if (!total) continue;
        unsigned long long base = 0;
        if (lane == 0) base = final ? atomicAdd(a.hits, (unsigned long long)total) : (unsigned long long)atomicAdd(a.cnt, (unsigned)total);
        base = __shfl(base, 0) + (unsigned long long)(incl - n);
        for (int i = 0; surv; i++, surv &= surv - 1) {
            const unsigned key = ((unsigned)lv << a.key_ss) | ((unsigned)gy << a.key_sy) | (unsigned)(k * 32 + __ffs(surv) - 1);
            if (final) { if (base + i < a.hit_cap) a.hits[1 + base + i] = slot | key; }
            else if (base + i < a.list_cap) a.list[0][base + i] = slot | key;
        }
    }
}

__global__ __launch_bounds__(256) void k_lbp_rest(LbpArgs a, int s0, int s1, int in, int in_cnt)
{
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
        if (alive) {
            // an entry comes from device memory: its image and its key are checked against the job and the grids before they index the planes
            e = src[i];
            const unsigned img = (unsigned)(e >> 32), key = (unsigned)e;
            const unsigned lv = key >> a.key_ss, gy = (key >> a.key_sy) & ((1u << (a.key_ss - a.key_sy)) - 1u), gx = key & ((1u << a.key_sy) - 1u);
            alive = img < (unsigned)a.nimg && lv < (unsigned)a.nlev;
            if (alive) {
                const LbpLevelDev &L = a.levels[lv];
                alive = gx < (unsigned)L.nx && gy < (unsigned)L.ny;
                if (alive) off = (size_t)img * a.plane_total + (size_t)L.plane_off + (size_t)(gy * L.step) * a.P + gx * L.step;
            }
        }
        for (int s = s0; s < s1 && s < a.nstages; s++) {
            if (!__ballot(alive)) break;
            if (alive) alive = lbp_stage(a.sum + off, a.gweak, a.stages[s]);
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

// detectMultiScale with outputRejectLevels: the last three stages on the survivor list in front of stage nstages - 3.
// No window drops out: each ends with the stage that rejected it (nstages: none did) and that stage's sum -- the last stage's on a
// pass --, and every one is appended to the candidate list, its LevelRec under the same index of `recs` (hit_cap records).  The
// list's count stays exact past hit_cap, as k_lbp_rest's.
__global__ __launch_bounds__(256) void k_lbp_levels(LbpArgs a, LevelRec *__restrict__ recs, int in, int in_cnt)
{
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
        if (listed) {
            // an entry comes from device memory: its image and its key are checked against the job and the grids before they index the planes
            e = src[i];
            const unsigned img = (unsigned)(e >> 32), key = (unsigned)e;
            const unsigned lv = key >> a.key_ss, gy = (key >> a.key_sy) & ((1u << (a.key_ss - a.key_sy)) - 1u), gx = key & ((1u << a.key_sy) - 1u);
            listed = img < (unsigned)a.nimg && lv < (unsigned)a.nlev;
            if (listed) {
                const LbpLevelDev &L = a.levels[lv];
                listed = gx < (unsigned)L.nx && gy < (unsigned)L.ny;
                if (listed) off = (size_t)img * a.plane_total + (size_t)L.plane_off + (size_t)(gy * L.step) * a.P + gx * L.step;
            }
        }
        bool alive = listed;
        int level = s0; float sum = 0.f;
        for (int s = s0; s < a.nstages; s++) {
            if (!__ballot(alive)) break;
            if (alive) {
                const LbpStageDev st = a.stages[s];
                sum = lbp_stage_sum(a.sum + off, a.gweak, st);
                alive = !(sum < st.thr);
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
            LevelRec r; r.level = level; r.pad = 0; r.weight = (double)sum;
            recs[base + rank] = r;
        }
    }
}

void launch_lbp_levels(hipStream_t st, const LbpArgs &a, LevelRec *recs, int in, int in_cnt, unsigned max_items)
{
    if (max_items == 0 || a.nstages < 4 || !recs) return;
    unsigned blocks = (max_items + 255u) / 256u;
    if (blocks > 4096u) blocks = 4096u;
    NVCA_LAUNCH(k_lbp_levels, dim3(blocks), dim3(256), 0, st, a, recs, in, in_cnt);
}

void launch_lbp_stage0(hipStream_t st, const LbpArgs &a, int lds)
{
    if (a.ntiles <= 0 || a.nimg <= 0) return;
    const dim3 grid((unsigned)a.ntiles, (unsigned)a.nimg);
    if (lds > 0) NVCA_LAUNCH(k_lbp_stage0<true>, grid, dim3(kLbpTileW * kLbpTileH), (size_t)lds, st, a);
    else NVCA_LAUNCH(k_lbp_stage0<false>, grid, dim3(kLbpTileW * kLbpTileH), 0, st, a);
}

void launch_lbp_walk(hipStream_t st, const LbpArgs &a)
{
    if (a.nrows <= 0 || a.nimg <= 0) return;
    NVCA_LAUNCH(k_lbp_walk, dim3((unsigned)(a.nrows * a.nimg + 63) / 64), dim3(64), 0, st, a);
}

void launch_lbp_rest(hipStream_t st, const LbpArgs &a, int s0, int s1, int in, int in_cnt, unsigned max_items)
{
    if (max_items == 0 || s0 >= a.nstages) return;
    unsigned blocks = (max_items + 255u) / 256u;
    if (blocks > 4096u) blocks = 4096u;
    NVCA_LAUNCH(k_lbp_rest, dim3(blocks), dim3(256), 0, st, a, s0, s1, in, in_cnt);
}

} // namespace nvca
