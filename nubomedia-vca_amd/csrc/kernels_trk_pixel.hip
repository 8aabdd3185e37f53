// kernels_trk_pixel.hip -- NuboTracker's pixel pass on gfx950: replaces, inside gst_nubo_tracker_process
// (TRK/gstnubotracker.cpp:339-421),
//   cvtColor(BGRA->gray) :356, absdiff :361, threshold :364, updateMotionHistory :368
// (calcMotionGradient :372 has no observable effect: its outputs are never read; segmentMotion :376 is kernels_trk_ccl.hip).
// One streaming pass: gray, |gray - prev| > thr, MHI update, prev <- gray -- k_trk_pixel / k_trk_pixel4 on BGRA frames,
// k_trk_pixel_yuv / k_trk_pixel_yuv8 on NV12 / I420 frames -- which also leaves what the component kernels start from: a flag byte
// per 256-pixel row segment, the live-segment estimate, the list of live tiles and cleared list headers (trk_layout.h).
// HBM-bound streaming work; no MFMA.
#include "launch.h"
#include "yuv_device.h"

namespace nvca {

__device__ __forceinline__ int gray4(unsigned px)
{
    return (int)((px & 255) * 1868 + ((px >> 8) & 255) * 9617 + ((px >> 16) & 255) * 4899 + 8192) >> 14;
}

// what one lane does for the cell (row y, segment seg) of slot blockIdx.z once it knows whether the cell holds motion history: the
// flag byte, the live-segment estimate and, for the first live cell of a tile this tick, the tile's entry in the list
__device__ __forceinline__ void cell_flag(uint8_t *__restrict__ flags, int w, int h, int y, int seg, bool hit, int *__restrict__ tiles, int tick)
{
    flags[trk_flag_index(w, h, blockIdx.z, y, seg)] = hit ? 1 : 0;
    if (hit) {
        if (trk_counted_row(y)) atomicAdd(segment_counts(flags, w, h, gridDim.z) + blockIdx.z, 1);       // an estimate is all that is asked
        const TileList t = tile_list(tiles, w, h, gridDim.z, tick);
        const int local = tile_of(w, y, seg);
        if (atomicExch(&t.mark[(size_t)blockIdx.z * t.per_slot + local], tick) != tick)
            t.list[(size_t)blockIdx.z * t.per_slot + atomicAdd(&t.cnt_now[blockIdx.z], 1)] = local;
    }
}
// grids of one wave per cell: row blockIdx.y, segment blockIdx.x * 4 + wave
__device__ __forceinline__ void segment_flag(uint8_t *__restrict__ flags, int w, int h, bool any, int *__restrict__ tiles, int tick)
{
    const bool hit = __ballot(any) != 0ull;
    const int seg = blockIdx.x * 4 + (threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0 && seg < seg_per_row(w)) cell_flag(flags, w, h, blockIdx.y, seg, hit, tiles, tick);
}
__device__ __forceinline__ void pixel_pass_clears(int *__restrict__ out, int *__restrict__ roots, int *__restrict__ tiles, int w, int h, int tick)
{
    // the component kernels' counters start at zero: cleared here, by the kernel in front of them, instead of by memset launches of their own
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < kRootsHdr) {
        if (blockIdx.z == 0) { roots[threadIdx.x] = 0; if (threadIdx.x < kCompHdr) out[threadIdx.x] = 0; }
        if (threadIdx.x == 0) tile_list(tiles, w, h, gridDim.z, tick).cnt_next[blockIdx.z] = 0;
    }
}

// one pixel of the pass behind its gray value: absdiff + THRESH_BINARY, cvUpdateMotionHistory, prev <- gray; returns whether the
// pixel holds motion history
__device__ __forceinline__ bool trk_update1(const TrkSlot &s, size_t o, int g)
{
    bool live = false;
    if (s.has_prev) {
        const int d = g - (int)s.prev[o];
        const bool moved = (d < 0 ? -d : d) > s.threshold;           // absdiff + THRESH_BINARY
        const float m = s.mhi[o];
        const float v = moved ? s.ts : (m < s.delbound ? 0.f : m);   // cvUpdateMotionHistory
        s.mhi[o] = v;
        live = v != 0.f;
    }
    s.prev[o] = (uint8_t)g;
    return live;
}
// four pixels of a row (o: a multiple of 4), read and written as words
__device__ __forceinline__ bool trk_update4(const TrkSlot &s, size_t o, int g0, int g1, int g2, int g3)
{
    bool any = false;
    if (s.has_prev) {
        const unsigned pv = *(const unsigned *)(s.prev + o);
        const float4 m0 = *(const float4 *)(s.mhi + o);
        float4 m = m0;
        const int d0 = g0 - (int)(pv & 255), d1 = g1 - (int)((pv >> 8) & 255), d2 = g2 - (int)((pv >> 16) & 255), d3 = g3 - (int)(pv >> 24);
        m.x = (d0 < 0 ? -d0 : d0) > s.threshold ? s.ts : (m.x < s.delbound ? 0.f : m.x);
        m.y = (d1 < 0 ? -d1 : d1) > s.threshold ? s.ts : (m.y < s.delbound ? 0.f : m.y);
        m.z = (d2 < 0 ? -d2 : d2) > s.threshold ? s.ts : (m.z < s.delbound ? 0.f : m.z);
        m.w = (d3 < 0 ? -d3 : d3) > s.threshold ? s.ts : (m.w < s.delbound ? 0.f : m.w);
        // (stores only of what changed: on a mostly static scene the history stays zero and the gray values stay what they were --
        // 14 bytes a pixel become 9)
        if (__float_as_uint(m.x) != __float_as_uint(m0.x) || __float_as_uint(m.y) != __float_as_uint(m0.y) ||
            __float_as_uint(m.z) != __float_as_uint(m0.z) || __float_as_uint(m.w) != __float_as_uint(m0.w)) *(float4 *)(s.mhi + o) = m;
        any = m.x != 0.f || m.y != 0.f || m.z != 0.f || m.w != 0.f;
        const unsigned gv = (unsigned)g0 | ((unsigned)g1 << 8) | ((unsigned)g2 << 16) | ((unsigned)g3 << 24);
        if (gv != pv) *(unsigned *)(s.prev + o) = gv;
    } else
        *(unsigned *)(s.prev + o) = (unsigned)g0 | ((unsigned)g1 << 8) | ((unsigned)g2 << 16) | ((unsigned)g3 << 24);
    return any;
}

__global__ __launch_bounds__(256) void k_trk_pixel(const TrkSlot *__restrict__ slots, int w, int h, uint8_t *__restrict__ flags, int *__restrict__ out, int *__restrict__ roots, int *__restrict__ tiles, int tick)
{
    pixel_pass_clears(out, roots, tiles, w, h, tick);
    const TrkSlot s = slots[blockIdx.z];
    const int x4 = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y;
    bool any = false;
    const uint8_t *row = s.src + (size_t)y * s.sstride + (size_t)x4 * 4;
    const size_t o = (size_t)y * w + x4;
    const int n = x4 >= w ? 0 : (w - x4 < 4 ? w - x4 : 4);
    for (int k = 0; k < n; k++) {
        const unsigned px = (unsigned)row[k * 4] | ((unsigned)row[k * 4 + 1] << 8) | ((unsigned)row[k * 4 + 2] << 16);
        if (trk_update1(s, o + k, gray4(px))) any = true;
    }
    segment_flag(flags, w, h, any, tiles, tick);
}

// vectorised variant: w % 4 == 0, 16-byte aligned frame rows
__global__ __launch_bounds__(256) void k_trk_pixel4(const TrkSlot *__restrict__ slots, int w, int h, uint8_t *__restrict__ flags, int *__restrict__ out, int *__restrict__ roots, int *__restrict__ tiles, int tick)
{
    pixel_pass_clears(out, roots, tiles, w, h, tick);
    const TrkSlot s = slots[blockIdx.z];
    const int x4 = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y;
    bool any = false;
    if (x4 < w) {
        const uint4 px = *(const uint4 *)(s.src + (size_t)y * s.sstride + (size_t)x4 * 4);
        any = trk_update4(s, (size_t)y * w + x4, gray4(px.x), gray4(px.y), gray4(px.z), gray4(px.w));
    }
    segment_flag(flags, w, h, any, tiles, tick);
}

// ---- the pixel pass on 4:2:0 frames (nvca_tracker_set_input): cv::cvtColor(CV_YUV2BGR_NV12 / _I420) in front of TRK/gstnubotracker.cpp:356,
// computed where the frame is read -- gray = gray_of(yuv_bgr(Y, chroma(x >> 1, y >> 1))), the value BGRA2GRAY gives the converted pixel
// (gray_of has gray4's coefficients).  Behind the gray value the pass is the packed one.
// General path: any plane alignment, any stride, any even size.  k_trk_pixel's shape and grid: up to 4 pixels of one row per thread,
// byte reads, one chroma fetch per pixel pair (x4 is a multiple of 4 and the width is even: whole pairs).
template <int FMT>
__global__ __launch_bounds__(256) void k_trk_pixel_yuv(const TrkSlot *__restrict__ slots, int w, int h, uint8_t *__restrict__ flags, int *__restrict__ out, int *__restrict__ roots, int *__restrict__ tiles, int tick)
{
    pixel_pass_clears(out, roots, tiles, w, h, tick);
    const TrkSlot s = slots[blockIdx.z];
    const int x4 = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y;
    bool any = false;
    const uint8_t *row = s.src + s.yuv.off_y + (size_t)y * s.sstride + x4;
    const size_t o = (size_t)y * w + x4;
    const int n = x4 >= w ? 0 : (w - x4 < 4 ? w - x4 : 4);
    for (int k = 0; k + 1 < n; k += 2) {
        const ChromaTerm c = chroma_at<FMT>(s.src, s.yuv, (x4 + k) >> 1, y >> 1);
        if (trk_update1(s, o + k, yuv_gray(row[k], c))) any = true;
        if (trk_update1(s, o + k + 1, yuv_gray(row[k + 1], c))) any = true;
    }
    segment_flag(flags, w, h, any, tiles, tick);
}

// Wide path: w % 4 == 0, luma rows and NV12 chroma rows 8-byte aligned, I420 chroma rows 4-byte aligned.  A thread owns 8 pixels of
// two rows -- the block four chroma samples serve, each sample's term computed once for its 2 x 2 pixels -- and reads them with one
// 8-byte load per luma row and 8 bytes of chroma (NV12: 4 U,V pairs; I420: 4 bytes of each plane); prev and the motion history go
// through trk_update4, four pixels at a time, as in k_trk_pixel4.  32 lanes cover a 256-pixel segment of a row pair, so a wave holds
// FOUR (row, segment) cells: lanes 0 .. 31 rows 4 by and 4 by + 1, lanes 32 .. 63 rows 4 by + 2 and 4 by + 3 of segment blockIdx.x * 4 +
// wave (by = blockIdx.y).  Every cell belongs to one wave, and its flag is the ballot bits of its half of the wave for its row.  A
// 1920-wide row is 7.5 segments: 240 of 256 lanes work.  The unit at the end of a row with w % 8 == 4 holds 4 pixels: half loads.
template <int FMT>
__global__ __launch_bounds__(256) void k_trk_pixel_yuv8(const TrkSlot *__restrict__ slots, int w, int h, uint8_t *__restrict__ flags, int *__restrict__ out, int *__restrict__ roots, int *__restrict__ tiles, int tick)
{
    pixel_pass_clears(out, roots, tiles, w, h, tick);
    const TrkSlot s = slots[blockIdx.z];
    const int lane = threadIdx.x & 63, sub = lane & 31, seg = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int x = seg * 256 + sub * 8, ry = blockIdx.y * 2 + (lane >> 5), y0 = 2 * ry;
    bool any0 = false, any1 = false;
    if (x < w && y0 < h) {
        const bool full = x + 8 <= w;
        const uint8_t *l0 = s.src + s.yuv.off_y + (size_t)y0 * s.sstride + x, *l1 = l0 + s.sstride;
        uint2 a, b;                                         // luma of the two rows
        unsigned cu, cv;                                    // NV12: U,V pairs 0 .. 1 / 2 .. 3; I420: the U bytes / the V bytes
        if (full) { a = *(const uint2 *)l0; b = *(const uint2 *)l1; }
        else { a = make_uint2(*(const unsigned *)l0, 0u); b = make_uint2(*(const unsigned *)l1, 0u); }
        if (FMT == 1) {
            const uint8_t *c = s.src + s.yuv.off_u + (size_t)ry * s.yuv.cstride + x;
            if (full) { const uint2 cc = *(const uint2 *)c; cu = cc.x; cv = cc.y; }
            else { cu = *(const unsigned *)c; cv = 0u; }
        } else {
            const uint8_t *pu = s.src + s.yuv.off_u + (size_t)ry * s.yuv.cstride + (x >> 1), *pv = s.src + s.yuv.off_v + (size_t)ry * s.yuv.vstride + (x >> 1);
            if (full) { cu = *(const unsigned *)pu; cv = *(const unsigned *)pv; }
            else { cu = *(const unsigned short *)pu; cv = *(const unsigned short *)pv; }
        }
#pragma unroll
        for (int hf = 0; hf < 2; hf++) {
            if (hf == 1 && !full) break;
            const unsigned yw0 = hf ? a.y : a.x, yw1 = hf ? b.y : b.x;
            int g0[4], g1[4];
#pragma unroll
            for (int p = 0; p < 2; p++) {
                int U, V;
                if (FMT == 1) { const unsigned wd = (hf ? cv : cu) >> (p * 16); U = wd & 255; V = (wd >> 8) & 255; }
                else { U = (cu >> ((2 * hf + p) * 8)) & 255; V = (cv >> ((2 * hf + p) * 8)) & 255; }
                const ChromaTerm c = chroma_term(U, V);
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    g0[2 * p + j] = yuv_gray((yw0 >> ((2 * p + j) * 8)) & 255, c);
                    g1[2 * p + j] = yuv_gray((yw1 >> ((2 * p + j) * 8)) & 255, c);
                }
            }
            const size_t o = (size_t)y0 * w + x + 4 * hf;
            if (trk_update4(s, o, g0[0], g0[1], g0[2], g0[3])) any0 = true;
            if (trk_update4(s, o + w, g1[0], g1[1], g1[2], g1[3])) any1 = true;
        }
    }
    const unsigned long long b0 = __ballot(any0), b1 = __ballot(any1);
    if (sub < 2 && seg < seg_per_row(w) && y0 < h) {        // lanes 0, 1, 32, 33: one cell each (the height is even: both rows of a pair exist)
        const unsigned long long bits = sub ? b1 : b0;
        const unsigned mine = (lane >> 5) ? (unsigned)(bits >> 32) : (unsigned)bits;
        cell_flag(flags, w, h, y0 + sub, seg, mine != 0u, tiles, tick);
    }
}

// ---- the pixel pass on packed 4:2:2 frames (FMT: NVCA_PIX_YUY2 / _UYVY / _YVYU): cv::cvtColor(CV_YUV2BGR_YUY2 / _UYVY / _YVYU) in front
// of TRK/gstnubotracker.cpp:356 -- gray = gray_of(yuv_bgr(Y, the chroma of the pixel's pair IN ITS ROW)).  Both kernels
// have k_trk_pixel's shape and grid: up to 4 pixels (two pairs) of one row per thread, a row per blockIdx.y -- any height, odd ones too.
// General path: byte reads, any alignment, any stride, any even width.
template <int FMT>
__global__ __launch_bounds__(256) void k_trk_pixel_yuv422(const TrkSlot *__restrict__ slots, int w, int h, uint8_t *__restrict__ flags, int *__restrict__ out, int *__restrict__ roots, int *__restrict__ tiles, int tick)
{
    pixel_pass_clears(out, roots, tiles, w, h, tick);
    const TrkSlot s = slots[blockIdx.z];
    const int x4 = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y;
    bool any = false;
    const size_t o = (size_t)y * w + x4;
    const int n = x4 >= w ? 0 : (w - x4 < 4 ? w - x4 : 4);
    for (int k = 0; k < n; k++) {                          // (the width is even: whole pairs)
        ChromaTerm c;
        const int Y = yuv422_at<FMT>(s.src, s.yuv, s.sstride, y, x4 + k, c);
        if (trk_update1(s, o + k, yuv_gray(Y, c))) any = true;
    }
    segment_flag(flags, w, h, any, tiles, tick);
}
// Wide path, beside k_trk_pixel4: w % 4 == 0, rows 8-byte aligned (trk_wide_ok): one 8-byte load = two pairs = 4 pixels, prev and
// the motion history through trk_update4
template <int FMT>
__global__ __launch_bounds__(256) void k_trk_pixel_yuv422x4(const TrkSlot *__restrict__ slots, int w, int h, uint8_t *__restrict__ flags, int *__restrict__ out, int *__restrict__ roots, int *__restrict__ tiles, int tick)
{
    pixel_pass_clears(out, roots, tiles, w, h, tick);
    const TrkSlot s = slots[blockIdx.z];
    const int x4 = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y;
    bool any = false;
    if (x4 < w) {
        const uint2 px = *(const uint2 *)(s.src + s.yuv.off_y + (size_t)y * s.sstride + (size_t)x4 * 2);
        const ChromaTerm c0 = chroma_of_pair<FMT>(px.x), c1 = chroma_of_pair<FMT>(px.y);
        any = trk_update4(s, (size_t)y * w + x4, yuv_gray(luma_of_pair<FMT>(px.x, 0), c0), yuv_gray(luma_of_pair<FMT>(px.x, 1), c0),
                          yuv_gray(luma_of_pair<FMT>(px.y, 0), c1), yuv_gray(luma_of_pair<FMT>(px.y, 1), c1));
    }
    segment_flag(flags, w, h, any, tiles, tick);
}

// 4 pixels per thread in the packed, the general 4:2:0 and the 4:2:2 kernels (w4 = ceil(w / 4)); rows packed (prev / mhi pitch == w)
void launch_trk_pixel(hipStream_t st, const TrkLaunch &L)
{
    const int w = L.w, h = L.h;
    dim3 gp(((w + 3) / 4 + 255) / 256, h, L.batch);
    dim3 gw((seg_per_row(w) + 3) / 4, (h + 3) / 4, L.batch);        // k_trk_pixel_yuv8: a wave per segment and four rows
#define NVCA_TRK_422(FMT) do { if (L.wide) NVCA_LAUNCH(k_trk_pixel_yuv422x4<FMT>, gp, dim3(256), 0, st, L.slots, w, h, L.flags, L.out, L.roots, L.tiles, L.tick); \
                               else NVCA_LAUNCH(k_trk_pixel_yuv422<FMT>, gp, dim3(256), 0, st, L.slots, w, h, L.flags, L.out, L.roots, L.tiles, L.tick); } while (0)
    if (L.fmt == NVCA_PIX_YUY2) NVCA_TRK_422(NVCA_PIX_YUY2);
    else if (L.fmt == NVCA_PIX_UYVY) NVCA_TRK_422(NVCA_PIX_UYVY);
    else if (L.fmt == NVCA_PIX_YVYU) NVCA_TRK_422(NVCA_PIX_YVYU);
    else
#undef NVCA_TRK_422
    if (L.fmt == 1 && L.wide) NVCA_LAUNCH(k_trk_pixel_yuv8<1>, gw, dim3(256), 0, st, L.slots, w, h, L.flags, L.out, L.roots, L.tiles, L.tick);
    else if (L.fmt == 2 && L.wide) NVCA_LAUNCH(k_trk_pixel_yuv8<2>, gw, dim3(256), 0, st, L.slots, w, h, L.flags, L.out, L.roots, L.tiles, L.tick);
    else if (L.fmt == 1) NVCA_LAUNCH(k_trk_pixel_yuv<1>, gp, dim3(256), 0, st, L.slots, w, h, L.flags, L.out, L.roots, L.tiles, L.tick);
    else if (L.fmt == 2) NVCA_LAUNCH(k_trk_pixel_yuv<2>, gp, dim3(256), 0, st, L.slots, w, h, L.flags, L.out, L.roots, L.tiles, L.tick);
    else if (L.wide) NVCA_LAUNCH(k_trk_pixel4, gp, dim3(256), 0, st, L.slots, w, h, L.flags, L.out, L.roots, L.tiles, L.tick);
    else NVCA_LAUNCH(k_trk_pixel, gp, dim3(256), 0, st, L.slots, w, h, L.flags, L.out, L.roots, L.tiles, L.tick);
}

} // namespace nvca
