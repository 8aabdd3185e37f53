// roi_lds_device.h -- the small device helpers that the one-workgroup evaluators of new-format cascades share (kernels_roi_lbp.hip,
// kernels_roi_hnew.hip): the wave scan, the sum plane in LDS and the queue append.  Device code only; the kernels themselves and
// their tables stay apart.
#pragma once
#include "launch.h"

namespace nvca {

typedef __attribute__((address_space(3))) int lroi_i32;
typedef __attribute__((address_space(3))) uint8_t lroi_u8;

static constexpr int kRoiLbpThreads = 1024, kRoiLbpWaves = kRoiLbpThreads / 64;

__device__ __forceinline__ unsigned lroi_wave_scan(unsigned v, int lane)
{   // wave64 inclusive add-scan on the VALU (DPP row shifts, then the three row totals through readlane): kernels_roi.hip's
    unsigned x = v;
    x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);
    x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);
    x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x113, 0xf, 0xf, true);
    x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xe, true);
    x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xc, true);
    const unsigned t0 = (unsigned)__builtin_amdgcn_readlane((int)x, 15), t1 = (unsigned)__builtin_amdgcn_readlane((int)x, 31),
                   t2 = (unsigned)__builtin_amdgcn_readlane((int)x, 47);
    const int row = lane >> 4;
    return x + (row >= 1 ? t0 : 0u) + (row >= 2 ? t1 : 0u) + (row >= 3 ? t2 : 0u);
}

// the sum plane of a w x h image, (w + 1) x (h + 1) words at pitch P = w + 1, in place in LDS (roi_integral's scheme, the sum alone)
template <class Pix>
__device__ __forceinline__ void lroi_integral(Pix pix, int w, int h, lroi_i32 *s, int P)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int X = tid; X <= w; X += kRoiLbpThreads) s[X] = 0;
    for (int y = wave; y < h; y += kRoiLbpWaves) {
        unsigned cs = 0;
        for (int x0 = 0; x0 < w; x0 += 64) {
            const int x = x0 + lane;
            const unsigned v = x < w ? (unsigned)pix(x, y) : 0u;
            const unsigned is = lroi_wave_scan(v, lane) + cs;
            if (x < w) s[(y + 1) * P + x + 1] = (int)is;
            cs = (unsigned)__builtin_amdgcn_readlane((int)is, 63);
        }
        if (lane == 0) s[(y + 1) * P] = 0;
    }
    __syncthreads();
    for (int x = tid; x < w; x += kRoiLbpThreads) {
        unsigned as = 0;
        for (int y = 1; y <= h; y++) { as += (unsigned)s[y * P + x + 1]; s[y * P + x + 1] = (int)as; }
    }
    __syncthreads();
}

// append the lanes with `pass` set to the queue qo, counted in *cnt (whole waves call this)
__device__ __forceinline__ void lroi_push(bool pass, int wi, unsigned short *qo, int *cnt, int lane)
{
    const unsigned long long pm = __ballot(pass);
    if (!pm) return;
    int base = 0;
    if (lane == 0) base = atomicAdd(cnt, (int)__popcll(pm));
    base = __shfl(base, 0);
    if (pass) qo[base + __popcll(pm & ((1ull << lane) - 1ull))] = (unsigned short)wi;
}

} // namespace nvca
